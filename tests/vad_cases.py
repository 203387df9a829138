"""Adversarial captures for the VAD's per-frame decision (VAD.C:164: frm_sum > s_thl || frm_zero > z_thl), for every framing
the VAD kernels are instantiated for (TEST INFRASTRUCTURE ONLY; tests/test_vad_frames.py).

A capture is a noise head whose thresholds are known, followed by a body put together block by block (a block = hop samples,
a frame = two blocks) from families aimed at the places where the kernels' block algebra (csrc/sr_vad_dev.h) can go wrong:
isolated out-of-band spikes on the band edges with the crossing count at z_thl and z_thl + 1, first / last out-of-band samples
at the block's edges with the preceding out-of-band sample near or far, the same at the borders of the kernels' 63-frame
rounds, one-sided frames whose magnitude sum is s_thl and s_thl + 1, whole 32-sample mask words, and the ends of the 16-bit
code range.  What a capture really contains is never taken from the generator's intentions: the oracle's per-frame values
(Oracle.vad_frames) and edge_classes() below, both computed from the samples alone, say so.
"""
import functools
from collections import Counter

import numpy as np

import oracle_lib as ol

# name, Engine keywords, Oracle keywords: one configuration per framing the VAD kernels are instantiated for
FRAMINGS = [
    ("ref_160_80", {}, {}),
    ("ext_320_160", dict(fs=16000, nfft=512, n_mel=40), dict(fs=16000, nfft=512, n_mel=40)),
    ("gen_240_120", dict(frame_time_ms=30, frame_mov_ms=15, n_coef=16), dict(frame_time=30, frame_mov_t=15, n_coef=16)),
    ("gen_256_128", dict(frame_time_ms=32, frame_mov_ms=16, n_mel=20, n_coef=10, noise_len_ms=480),
     dict(frame_time=32, frame_mov_t=16, n_mel=20, n_coef=10, noise_len_t=480)),
    ("gen_400_200", dict(frame_time_ms=50, frame_mov_ms=25), dict(frame_time=50, frame_mov_t=25)),
    ("gen_512_256", dict(frame_time_ms=64, frame_mov_ms=32, n_mel=64, n_coef=16, noise_len_ms=960),
     dict(frame_time=64, frame_mov_t=32, n_mel=64, n_coef=16, noise_len_t=960)),
    # a hop above 40 ms: both duration limits of VAD.C:72-75 are one frame
    ("gen_512_256_4k", dict(fs=4000, frame_time_ms=128, frame_mov_ms=64, n_mel=12, n_coef=6, noise_len_ms=1920),
     dict(fs=4000, frame_time=128, frame_mov_t=64, n_mel=12, n_coef=6, noise_len_t=1920)),
]
FRAMING_IDS = [f[0] for f in FRAMINGS]
ROUND = 63      # frames per round of k_vad / per wave of k_vad_wide
MAX_SEG = 3     # VAD.H:4
GROUPS, PER_GROUP = 4, 8  # captures of one group share their length: the batch forms take one buf_len per call
EDGE_POS = ("0", "1", "hop-2", "hop-1")


def limits(orc):
    """(v_durmin, s_durmax) in frames, VAD.C:72-75"""
    step = orc.cfg.frame_time - orc.cfg.frame_mov_t
    return 80 // step, 110 // step


# ---- the endpoint state machine (VAD.C:164-216) over per-frame bits --------------------------------------------------------
def sm_step(state, loud, i, fl, hop, vmin, smax):
    """one frame: ((cur, front, back), event), event None, ("start", sample) or ("end", sample)"""
    cur, front, back = state
    if loud:
        if cur == 0:
            return (1, 1, back), None
        if cur == 1:
            front += 1
            if front >= vmin:
                return (2, 0, back), ("start", i - (vmin - 1) * hop)
            return (1, front, back), None
        if cur == 3:
            return (2, front, 0), None
        return state, None
    if cur == 2:
        return (3, front, 1), None
    if cur == 3:
        back += 1
        if back >= smax:
            return (0, front, 0), ("end", i - smax * hop + fl)
        return (3, front, back), None
    if cur == 1:
        return (0, 0, back), None
    return state, None


def segments_from_loud(loud, fl, hop, vmin, smax, max_seg=None):
    """(segments [[start, end]], end -1 = still open; index of the frame that closed the max_seg-th segment, or None)"""
    state, segs = (0, 0, 0), []
    for f, l in enumerate(loud):
        state, ev = sm_step(state, bool(l), f * hop, fl, hop, vmin, smax)
        if ev is None:
            continue
        if ev[0] == "start":
            segs.append([ev[1], -1])
        else:
            segs[-1][1] = ev[1]
            if max_seg is not None and len(segs) == max_seg:  # VAD.C:203-206
                return segs, f
    return segs, None


def decisive_share(loud, fl, hop, vmin, smax):
    """(frames whose flipped bit changes the segment list, frames).  A flip is followed from the state before its frame until
    the state machine is back on the unflipped run's track: the lists differ iff an event differs on the way."""
    F = len(loud)
    states, events, s = [], [], (0, 0, 0)
    for f in range(F):
        states.append(s)
        s, ev = sm_step(s, bool(loud[f]), f * hop, fl, hop, vmin, smax)
        events.append(ev)
    states.append(s)
    n = 0
    for f in range(F):
        s, g, bit = states[f], f, not loud[f]
        while True:
            s, ev = sm_step(s, bool(bit), g * hop, fl, hop, vmin, smax)
            if ev != events[g]:
                n += 1
                break
            g += 1
            if g == F or s == states[g]:
                break
            bit = loud[g]
    return n, F


# ---- what a capture contains, from its samples alone -------------------------------------------------------------------------
def classify(x, atap):
    """class of every sample as VAD.C:131-157 sees it: 2 above the band (x >= a_thl), 1 below (x < b_thl), 0 inside, in the
    reference's u32 arithmetic (VAD.C:112-113: both thresholds may wrap)"""
    mid, n_thl = int(atap[0]), int(atap[1])
    a_thl, b_thl = (mid + n_thl) & 0xFFFFFFFF, (mid - n_thl) & 0xFFFFFFFF
    x = np.asarray(x).astype(np.int64)
    return np.where(x >= a_thl, 2, np.where(x < b_thl, 1, 0)).astype(np.uint8)


def edge_classes(x, atap, hop, n_blocks):
    """Counter of the block-edge situations among blocks [0, n_blocks):
    ("first", position, class, "same" | "other", "prev" | "far"): the block's first out-of-band sample at offset 0, 1, hop-2 or
        hop-1, its class, against the class of the out-of-band sample before it, which lies in the previous block or at least
        three blocks back (only in-band samples between);
    ("last", "hop-1" | "hop-2", class): the block's last out-of-band sample;  ("absent",): a block without any;
    ("round", r) for r in 61, 62, 0, 1: such a "first" block at index r modulo 63, past the first round."""
    cls = classify(x[:n_blocks * hop], atap)
    idx = np.flatnonzero(cls)
    out = Counter()
    blk, off, c = idx // hop, idx % hop, cls[idx]
    out[("absent",)] = n_blocks - len(np.unique(blk))
    names = {0: "0", 1: "1", hop - 2: "hop-2", hop - 1: "hop-1"}
    first = np.flatnonzero(np.diff(blk, prepend=-1) > 0)
    for k in first:
        if k == 0 or int(off[k]) not in names:
            continue
        d = int(blk[k] - blk[k - 1])
        if d == 2:
            continue
        out[("first", names[int(off[k])], int(c[k]), "same" if c[k] == c[k - 1] else "other", "prev" if d == 1 else "far")] += 1
        if blk[k] >= ROUND - 2 and int(blk[k]) % ROUND in (61, 62, 0, 1):
            out[("round", int(blk[k]) % ROUND)] += 1
    last = np.flatnonzero(np.diff(blk, append=n_blocks + 1) > 0)
    for k in last:
        if int(off[k]) in (hop - 1, hop - 2):
            out[("last", names[int(off[k])], int(c[k]))] += 1
    return out


def required_edge_classes():
    keys = [("first", p, c, rel, d) for p in EDGE_POS for c in (1, 2) for rel in ("same", "other") for d in ("prev", "far")]
    keys += [("last", p, c) for p in ("hop-1", "hop-2") for c in (1, 2)]
    keys += [("absent",)] + [("round", r) for r in (61, 62, 0, 1)]
    return keys


# ---- the generator ---------------------------------------------------------------------------------------------------------------
class Ctx:
    """thresholds of one capture and the codes that sit exactly on its band edges"""

    def __init__(self, orc, atap):
        self.mid, self.n, self.z, self.s = (int(v) for v in atap)
        self.atap = (self.mid, self.n, self.z, self.s)
        self.a_thl, self.b_thl = (self.mid + self.n) & 0xFFFFFFFF, (self.mid - self.n) & 0xFFFFFFFF
        self.fl, self.hop = orc.frame_len, orc.hop
        self.vmin, self.smax = limits(orc)
        self.bg = min(self.mid, 65535)
        self.last = 0  # class of the last out-of-band sample written so far
        # a block of in-band samples on the band's edge makes both frames it belongs to loud by magnitude alone
        self.inband_loud = self.val("a") is not None and classify([self.val("a")], self.atap)[0] == 0 \
            and (self.val("a") - self.mid) * self.hop > self.s

    def val(self, kind):
        """A: the lowest code above the band, a: the highest code not above it, B: the highest code below the band, b: the lowest
        code not below it (with a wrapped b_thl every code that is not above is below).  None: no such 16-bit code."""
        a, b = self.a_thl, self.b_thl
        v = {"A": a, "a": a - 1, "B": (b - 1) if b <= 65535 else a - 1, "b": b if b <= 65535 else a - 1}[kind]
        return v if 0 <= v <= 65535 else None

    def of_class(self, c):
        return self.val("A" if c == 2 else "B")

    def note(self, x):
        c = classify(x, self.atap)
        nz = np.flatnonzero(c)
        if len(nz):
            self.last = int(c[nz[-1]])


def _offsets(c, rng, n):
    """n distinct sample offsets of a block, half of the time biased to the block's ends and the 32-sample word borders"""
    hop = c.hop
    n = min(n, hop)
    if n == 0:
        return np.zeros(0, np.int64)
    if rng.random() < 0.5:
        hot = np.unique(np.clip(np.concatenate([[0, 1, hop - 2, hop - 1], np.arange(31, hop, 32), np.arange(32, hop, 32),
                                                np.arange(33, hop, 32)]), 0, hop - 1))
        k = min(n, len(hot), int(rng.integers(1, 3)))
        o = set(rng.choice(hot, k, replace=False).tolist())
        while len(o) < n:
            o.add(int(rng.integers(0, hop)))
        return np.array(sorted(o), np.int64)
    return np.sort(rng.choice(hop, n, replace=False))


def spike_block(c, rng, n_alt, n_rep=0, n_deco=0):
    """in-band background with isolated spikes exactly on the band's edges: n_alt of the other class than the out-of-band sample
    before them (a band crossing each), n_rep of the same class (none), n_deco in-band samples on the edges"""
    x = np.full(c.hop, c.bg, np.int64)
    roles = np.array(["alt"] * n_alt + ["rep"] * n_rep + ["deco"] * n_deco)
    rng.shuffle(roles)
    last = c.last
    for o, r in zip(_offsets(c, rng, len(roles)), roles):
        if r == "deco":
            v = c.val("a" if rng.random() < 0.5 else "b")
        else:
            want = (3 - last) if (r == "alt" and last) else (last or int(rng.integers(1, 3)))
            v = c.of_class(want)
            if v is not None:
                last = want
        if v is not None:
            x[o] = v
    c.note(x)
    return x


def spike_run(c, rng, k, p_over=0.35):
    """k blocks whose crossing counts add up, frame by frame, to about z_thl or (with probability p_over) z_thl + 1"""
    out, a = [], int(rng.integers(0, c.z + 1))
    for _ in range(k):
        out.append(spike_block(c, rng, a, int(rng.integers(0, 3)) if rng.random() < 0.4 else 0,
                               int(rng.integers(0, 4)) if rng.random() < 0.3 else 0))
        a = int(np.clip(c.z + (1 if rng.random() < p_over else 0) - a, 0, c.z + 1))
    return out


def quiet_block(c):
    return np.full(c.hop, c.bg, np.int64)


def gap_block(c, loud):
    """a block of in-band samples only: the background, or (loud) the band's edge throughout, loud by magnitude alone"""
    if not loud:
        return quiet_block(c)
    return np.full(c.hop, c.val("a"), np.int64)


def loud_block(c, rng):
    """loud whatever the thresholds: the ends of the 16-bit range, random codes, or a dense full-scale alternation"""
    kind = rng.integers(0, 3)
    if kind == 0:
        x = rng.choice(np.array([0, 65535, c.bg]), c.hop).astype(np.int64)
    elif kind == 1:
        x = rng.integers(0, 65536, c.hop).astype(np.int64)
    else:
        x = np.where(np.arange(c.hop) % 2 == 0, 65535, 0).astype(np.int64)
    x[rng.integers(0, c.hop)] = 0
    x[rng.integers(0, c.hop)] = 65535
    c.note(x)
    return x


def energy_run(c, rng, k):
    """k one-sided blocks (every out-of-band sample on the same side: no crossing) whose magnitude sums add up, frame by frame,
    to exactly s_thl or s_thl + 1"""
    rooms = {True: 65535 - c.mid, False: c.mid}   # above / below mid: a side one sample of which can carry a whole threshold
    sides = [u for u in (True, False) if rooms[u] > c.s + 1] or [rooms[True] > rooms[False]]
    up = sides[int(rng.integers(0, len(sides)))]
    room = max(rooms[up], 0)
    out, A = [], c.s // 2 + int(rng.integers(-3, 4))
    for _ in range(k):
        A = int(np.clip(A, 0, c.s + 1))
        d = np.zeros(c.hop, np.int64)
        if rng.random() < 0.5:  # spread over the whole block
            d[:] = A // c.hop
            d[rng.choice(c.hop, A % c.hop, replace=False)] += 1
        else:                   # carried by a few samples
            m = int(rng.integers(1, 5))
            pos = rng.choice(c.hop, m, replace=False)
            d[pos] = A // m
            d[pos[0]] += A % m
        d = np.minimum(d, room)
        x = c.mid + d if up else c.mid - d
        c.note(x)
        out.append(x)
        A = c.s + int(rng.integers(0, 2)) - int(d.sum())
    return out


def word_block(c, rng):
    """whole 32-sample mask words (the last one partial where hop is no multiple of 32) filled with out-of-band samples on the
    band's edges: one class, the other, a split between the two, or a short alternation; the rest is background"""
    hop = c.hop
    x = np.full(hop, c.bg, np.int64)
    A, B = c.val("A"), c.val("B")
    if A is None or B is None:
        return spike_block(c, rng, 1)
    nw = (hop + 31) // 32
    cost = max(abs(A - c.mid), abs(B - c.mid), 1)
    k = int(np.clip((c.s // 2) // (32 * cost), 1, nw))  # keep the block's magnitude under half the threshold where that is possible
    words = set(rng.choice(nw, k, replace=False).tolist())
    if rng.random() < 0.5:
        words.add(nw - 1)      # the partial word
    for w in sorted(words)[:max(k, 1) + 1]:
        lo, hi = 32 * w, min(32 * w + 32, hop)
        n = hi - lo
        first, other = (A, B) if rng.random() < 0.5 else (B, A)
        pat = rng.integers(0, 4)
        seg = np.full(n, first, np.int64)
        if pat == 1:
            seg[int(rng.integers(1, n)):] = other
        elif pat == 2:
            m = int(rng.integers(2, min(n, c.z + 2) + 1))
            seg[:m][1::2] = other
        elif pat == 3:
            m = int(rng.integers(2, min(n, c.z + 2) + 1))
            seg[n - m:][0::2] = other
        x[lo:hi] = seg
    c.note(x)
    return x


def edge_item(c, rng, spec):
    """the blocks of one block-edge case: a block P whose last out-of-band sample has the class the spec asks for, `gap` blocks
    of in-band samples, and the target block T whose first out-of-band sample sits at the asked offset (None: the capture's
    thresholds leave no 16-bit code for one of the classes)"""
    rel, gap, pos, cf, lastpos, loud_gap = spec
    hop = c.hop
    p = cf if rel == "same" else 3 - cf
    if c.of_class(1) is None or c.of_class(2) is None:
        return None
    P = np.full(hop, c.bg, np.int64)
    e = int(rng.integers(0, c.z + 1))
    offs = _offsets(c, rng, e + 1)
    cl = p
    for o in offs[::-1]:       # alternating classes, the last one = p
        P[o] = c.of_class(cl)
        cl = 3 - cl
    T = np.full(hop, c.bg, np.int64)
    o0 = {"0": 0, "1": 1, "hop-2": hop - 2, "hop-1": hop - 1}[pos]
    T[o0] = c.of_class(cf)
    cl = cf
    if o0 + 2 < hop - 2:
        more = np.sort(rng.choice(np.arange(o0 + 1, hop - 2), min(int(rng.integers(0, c.z + 1)), hop - 3 - o0), replace=False))
        for o in more:
            cl = 3 - cl if rng.random() < 0.8 else cl
            T[o] = c.of_class(cl)
    if lastpos is not None and o0 < hop - 2:
        T[hop - 1 if lastpos == "hop-1" else hop - 2] = c.of_class(int(rng.integers(1, 3)))
    c.note(T)
    return [P] + [gap_block(c, loud_gap) for _ in range(gap)] + [T]


def edge_specs(rng):
    """every (relation, gap, position, class) combination, shuffled, each with a last-sample variant"""
    specs = [(rel, gap, pos, cf, lp) for rel in ("same", "other") for gap in (0, 3) for pos in EDGE_POS for cf in (1, 2)
             for lp in (None, "hop-1", "hop-2")]
    rng.shuffle(specs)
    return specs


def make_head(orc, rng, kind):
    """the noise head (noise_len samples).  Alternating mid +- d gives n_thl = d and s_thl = 11 * d * frame_len / 10 ("full");
    three samples of four at mid quarter s_thl ("sparse": a block of in-band samples on the band's edge is then loud on its
    own); "spiked" adds crossings to frames 0 and 1; "low" sits near code 0 with sparse larger samples, so that n_thl > mid and
    b_thl wraps (VAD.C:113); "high" sits near 65 535 with a_thl above every code"""
    N, hop = orc.noise_len, orc.hop
    i = np.arange(N)
    d = int(rng.integers(8, 41))
    if kind == "low":
        x = rng.integers(0, 4, N).astype(np.int64)
        x[::8] = int(rng.integers(150, 400))
        return x
    if kind == "high":  # three samples of four at H, one 4 d lower: mid = H - d, n_thl = 3 d, a_thl = H + 2 d > 65 535
        H = 65535 - int(rng.integers(0, d))
        return np.where(i % 4 == 0, H - 4 * d, H).astype(np.int64)
    mid = int(rng.choice([2048, 2048, 700, 30000, 61000]))
    if kind == "sparse":
        return mid + np.select([i % 8 == 0, i % 8 == 4], [d, -d], 0)
    x = mid + np.where(i % 2 == 0, d, -d)
    if kind == "spiked":
        # frames 0 and 1 (last_sig = 0 on entry to frame 0, VAD.C:99): far out-of-band spikes of alternating sign in blocks
        # 0 .. 2, the first of block 0 not on its first sample, about z_thl crossings per frame
        # Half of these heads give frame 0 exactly z_thl crossings with two spikes in block 0 (z_thl + 1 spikes in blocks 0 and 1:
        # the first one has nothing before it), the others about as many.
        z = orc.frame_len * 2 // 160
        sign = 1 if rng.random() < 0.5 else -1
        exact = rng.random() < 0.5
        for blk in range(3):
            k = max(1, (z + 1) // 2 + int(rng.integers(-1, 2)))
            if exact and blk < 2:
                k = (2, z - 1)[blk]
            lo = 1 if blk == 0 else 0
            for o in np.sort(rng.choice(np.arange(lo, hop - 1), min(k, hop - 2), replace=False)):
                x[blk * hop + o] = mid + sign * 3 * d
                sign = -sign
    return x


class Body:
    """the body's blocks in order, with what keeps a capture from completing segments: `open` bodies start a segment at once and
    never let a quiet run reach s_durmax (a surely loud block goes in before the free blocks could), `shut` bodies keep two
    quiet blocks between items short enough that no loud run reaches v_durmin"""

    def __init__(self, c, rng, n_head_blocks, style):
        self.c, self.rng, self.style, self.blocks, self.n0 = c, rng, style, [], n_head_blocks
        self.free = 0
        self.gmax = max(c.smax, 2)            # free blocks between two surely loud ones: quiet runs stay under max(s_durmax, 2)
        self.kmax = c.vmin - 2                # free blocks of a `shut` item: loud runs stay under v_durmin
        if style == "open":
            for _ in range(c.vmin + 1):
                self.blocks.append(loud_block(c, rng))

    def index(self):
        return self.n0 + len(self.blocks)

    def fits(self, k):
        return k <= (self.gmax if self.style == "open" else self.kmax)

    def lead(self, k):
        """blocks that go in before an item of k free blocks"""
        if self.style == "open":
            return 1 if self.free + k > self.gmax else 0
        return 2 if self.free else 0

    def add(self, blocks, loud=()):
        """blocks of one item; loud: indices of its blocks that are loud for certain"""
        k = len(blocks) - len(loud)
        if self.style == "open":
            if self.free + k > self.gmax:
                self.blocks.append(loud_block(self.c, self.rng))
                self.free = 0
            for i, b in enumerate(blocks):
                self.blocks.append(b)
                self.free = 0 if i in loud else self.free + 1
        else:
            if self.free:
                self.blocks += [quiet_block(self.c), quiet_block(self.c)]
            self.blocks += list(blocks)
            self.free = 1

    def tail(self):
        """three segments closed one after the other (open bodies close their first one here)"""
        c = self.c
        for _ in range(MAX_SEG):
            self.blocks += [loud_block(c, self.rng) for _ in range(c.vmin + 1)]
            self.blocks += [quiet_block(c) for _ in range(max(c.smax, 2) + 2)]
        self.free = 0


def _align(body, k_free, to_target, r):
    """fill, one block at a time, until the target block of the next item (k_free free blocks, its target to_target blocks after
    its first) lands on index r modulo ROUND"""
    for _ in range(2 * ROUND):
        if (body.index() + body.lead(k_free) + to_target) % ROUND == r:
            return
        if body.style == "open":
            body.blocks.append(loud_block(body.c, body.rng))
            body.free = 0
        else:
            body.blocks.append(quiet_block(body.c))


def make_capture(orc, rng, n_blocks, head_kind, style, late3, specs):
    """one capture of n_blocks blocks: (samples int64, atap tuple)"""
    hop = orc.hop
    head = make_head(orc, rng, head_kind)
    rc, a = orc.noise_atap(np.clip(head, 0, 65535).astype(np.uint16))
    assert rc == 0
    c = Ctx(orc, a.astuple())
    c.note(head)
    nh = len(head) // hop
    assert nh * hop == len(head)
    body = Body(c, rng, nh, style)
    n_tail = MAX_SEG * (c.vmin + 1 + max(c.smax, 2) + 2) if late3 else 0
    room = n_blocks - nh - n_tail
    served = -1   # the round border that has had its edge item
    while len(body.blocks) < room:
        idx = body.index()
        border = (idx + 14) // ROUND
        want_border = border >= 1 and border > served and ROUND - 14 <= idx % ROUND < ROUND - 5
        fam = rng.choice(["spikes", "edge", "energy", "words", "quiet"], p=[0.3, 0.4, 0.14, 0.1, 0.06])
        kcap = body.gmax if style == "open" else max(body.kmax, 1)
        if want_border or fam == "edge":
            if not specs:
                specs.extend(edge_specs(rng))
            rel, gap, pos, cf, lp = specs.pop()
            r = (61, 62, 0, 1)[int(rng.integers(0, 4))]
            if style == "shut" and gap == 3:      # the item falls into P and T, three quiet blocks between
                parts = edge_item(c, rng, (rel, 0, pos, cf, lp, False))
                if parts is None:
                    body.add(energy_run(c, rng, 1))
                    continue
                P, T = parts
                if want_border:
                    _align(body, 1, 4, r)
                    served = border
                body.add([P])
                body.blocks.append(quiet_block(c))  # two more come with add()
                body.add([T])
                continue
            loud_gap = style == "open" and c.inband_loud and gap > 0
            k_free = 2 if loud_gap else 2 + gap
            if not body.fits(k_free):
                continue
            if want_border:
                _align(body, k_free, 1 + gap, r)
                served = border
            item = edge_item(c, rng, (rel, gap, pos, cf, lp, loud_gap))
            if item is None:
                body.add(energy_run(c, rng, 1))
                continue
            body.add(item, loud=tuple(range(1, 1 + gap)) if loud_gap else ())
        elif fam == "spikes":
            body.add(spike_run(c, rng, int(rng.integers(1, kcap + 1)), 0.35 if style == "open" else 0.25))
        elif fam == "energy":
            body.add(energy_run(c, rng, int(rng.integers(1, kcap + 1))))
        elif fam == "words":
            body.add([word_block(c, rng)])
        else:
            body.add([quiet_block(c)])
    del body.blocks[room:]
    if late3:
        body.tail()
    x = np.concatenate([head] + body.blocks)
    x = np.concatenate([x, np.full(max(0, n_blocks * hop - len(x)), c.bg, np.int64)])[:n_blocks * hop]
    return np.clip(x, 0, 65535).astype(np.uint16), c.atap


def make_runs_capture(orc, rng, n_blocks):
    """a capture for the forms that only hand out segments: loud runs and quiet runs with lengths drawn around v_durmin and
    s_durmax, every frame decided by a hair -- cold blocks carry half of z_thl crossings or half of s_thl, hot blocks one
    crossing or one unit of magnitude more than a whole threshold"""
    hop = orc.hop
    head = make_head(orc, rng, "sparse" if rng.random() < 0.7 else "full")
    rc, a = orc.noise_atap(head.astype(np.uint16))
    assert rc == 0
    c = Ctx(orc, a.astuple())
    c.note(head)
    blocks, n = [], n_blocks - len(head) // hop

    def around(m):
        return max(1, m + int(rng.integers(-2, 3)))

    while len(blocks) < n:
        L, M = around(c.vmin), around(c.smax)
        by_energy = rng.random() < 0.4
        hot, cold = max(L - 1, 1), M + 1
        for k, is_hot in ((cold, False), (hot, True)):
            for _ in range(k):
                if by_energy:
                    A = c.s + 1 if is_hot else c.s // 2
                    d = np.zeros(hop, np.int64)
                    d[:] = A // hop
                    d[rng.choice(hop, A % hop, replace=False)] += 1
                    x = c.mid + d if c.mid + int(d.max()) <= 65535 else c.mid - d
                    c.note(x)
                    blocks.append(x)
                else:
                    blocks.append(spike_block(c, rng, c.z + 1 if is_hot else c.z // 2))
    x = np.concatenate([head] + blocks)[:n_blocks * hop]
    return np.clip(x, 0, 65535).astype(np.uint16), c.atap


class Cases:
    """the captures of one framing: groups of PER_GROUP rows, one length (buf_len) per group, and the oracle's view of each"""

    def __init__(self, name, ekw, okw, runs=False, seed=0):
        self.name, self.ekw, self.okw = name, ekw, okw
        self.orc = orc = ol.Oracle(max_seg=MAX_SEG, **okw)
        self.fl, self.hop = orc.frame_len, orc.hop
        self.vmin, self.smax = limits(orc)
        rng = np.random.default_rng([seed, FRAMING_IDS.index(name), int(runs)])
        self.groups = []   # (pcm uint16 [PER_GROUP, W], buf_len)
        self.rows = []     # dict(x, atap, fsum, fzero, loud, segs, done) per capture, x = its buf_len samples
        specs = []
        heads = ["sparse", "sparse", "spiked", "full", "sparse", "spiked", "low", "high"]
        for g in range(GROUPS if not runs else 2):
            nb = int(rng.integers(202, 703))
            extra = int(rng.choice([0, 1, 8, self.hop - 1]))
            buf_len = nb * self.hop + extra
            W = (buf_len + 7) // 8 * 8
            pcm = np.full((PER_GROUP, W), 0xFFFF, np.uint16)   # past buf_len everything is loud: a frame too many would show
            for r in range(PER_GROUP):
                if runs:
                    x, atap = make_runs_capture(orc, rng, nb)
                else:
                    style = "shut" if (r % 2 == 1 and self.vmin >= 3) else "open"
                    x, atap = make_capture(orc, rng, nb, heads[(r + g) % len(heads)], style, late3=(r >= PER_GROUP // 2 + 1), specs=specs)
                pcm[r, :len(x)] = x
                pcm[r, len(x):buf_len] = min(atap[0], 65535)
                self.rows.append(self._view(pcm[r, :buf_len].copy(), atap))
            self.groups.append((pcm, buf_len))

    def _view(self, x, atap):
        orc = self.orc
        a = ol.Atap(*atap)
        fsum, fzero, loud = orc.vad_frames(x, a)
        segs, done = segments_from_loud(loud, self.fl, self.hop, self.vmin, self.smax, MAX_SEG)
        return dict(x=x, atap=atap, fsum=fsum, fzero=fzero, loud=loud, segs=segs, done=done)

    def compared(self, row):
        """frames of a capture whose bits the batch kernels write: every round up to and including the one in which the
        max_seg-th segment closes"""
        F = len(row["loud"])
        return F if row["done"] is None else min(F, (row["done"] // ROUND + 1) * ROUND)


@functools.lru_cache(maxsize=None)
def cases(name, runs=False):
    f = FRAMINGS[FRAMING_IDS.index(name)]
    return Cases(f[0], f[1], f[2], runs=runs)


def coverage(cs):
    """what the captures of a framing contain within the compared range, from the oracle's values and the samples alone"""
    cov = Counter()
    per_round = {}
    for row in cs.rows:
        n = cs.compared(row)
        z, s = row["atap"][2], row["atap"][3]
        fz, fs, ld = row["fzero"][:n].astype(np.int64), row["fsum"][:n].astype(np.int64), row["loud"][:n]
        cov["frames"] += len(row["loud"])
        cov["compared"] += n
        cov["Z==z"] += int(np.sum(fz == z))
        cov["Z==z+1,sum<=s"] += int(np.sum((fz == z + 1) & (fs <= s)))
        cov["sum==s"] += int(np.sum(fs == s))
        cov["sum==s+1,Z<=z"] += int(np.sum((fs == s + 1) & (fz <= z)))
        cov["few"] += int(row["done"] is None)
        mid, n_thl = row["atap"][:2]
        cov["b_wraps"] += int(n_thl > mid)
        cov["a_over"] += int(mid + n_thl > 65535)
        cov["code0"] += int(np.any(row["x"] == 0))
        cov["code65535"] += int(np.any(row["x"] == 65535))
        c0 = classify(row["x"][:cs.hop - 1], row["atap"])   # block 0 without its last sample
        o0 = np.flatnonzero(c0)
        cov["frame0"] += int(fz[0] == z and fs[0] <= s and len(o0) > 0 and o0[0] > 0 and c0[o0[0]] != c0[o0[-1]])
        cov.update(edge_classes(row["x"], row["atap"], cs.hop, n + 1))
        for r in range((n + ROUND - 1) // ROUND):
            seen = per_round.setdefault(r, set())
            seen.update(np.unique(ld[r * ROUND:(r + 1) * ROUND]).tolist())
    cov["rounds_one_sided"] = sum(1 for v in per_round.values() if len(v) < 2)
    return cov
