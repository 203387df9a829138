"""Fixtures of tests/test_pcm_front_ends.py: every PCM entry point of the decoders under every front end.

One fixture per front end (FRONT_ENDS: the reference's, the 16 kHz extension, five of the generic one with frames of 240, 256,
320, 400 and 512 samples; n_coef 12 and max_frames 119 everywhere):

  case(name)       three channels of synthetic audio with different mid values, R3 = 3 * R1 samples each, R1 = 100 frames and a
                   remainder; the features of the first R1 samples from the CPU oracle, segment [1, R1]; a store of six templates
                   of 12..40 rows cut from those features (slot 3 invalid, slots 1 and 4 one word); skip and word costs as the
                   planted tests choose them; the grammars.  im / inf hold a fourth row of no frames: the record of a segment
                   that starts at sample 0.
  long_feats(name) the oracle's features of all R3 samples, piece by piece over segments [1 + p * hop, ...] of at most max_frames
                   frames (a frame's pre-emphasis predecessor is the sample before it, so the pieces are exact).
  want_*(name)     the restatements (spot_ref, spot_live_ref, chain_ref, gram_ref, wgram_ref, onepass_ref, onepass_gram_ref) on
                   the oracle's features, each computed once.
  schedules(name)  push schedules built from the front end's own framing, one chunking per channel.
Nothing here comes from the engine.  The arrays are read-only.  Plain module: no fixtures, no pytest settings.
"""
import functools

import numpy as np

import chain_ref
import gram_ref
import onepass_gram_ref
import onepass_ref
import oracle_lib as ol
import spot_live_ref
import spot_ref
import wgram_ref

MAXF, N_CH, N_FR = 119, 3, 100
WIN = 50                      # win_frames of every spotting call
MAX_WORDS, OP_WORDS = 6, 8    # max_words of the level decoders, words_cap of the one-pass decoders
WORD_COST = 100
MID = (2048, 2040, 2100)
POISON = 4095                 # what a chunk row holds past n[c]

# name: (engine keywords, oracle keywords)
FRONT_ENDS = {
    "reference": (dict(), dict()),
    "extension": (dict(fs=16000, nfft=512, n_mel=40), dict(fs=16000, nfft=512, n_mel=40)),
    "gen240": (dict(fs=12000), dict(fs=12000)),
    "gen256": (dict(frame_time_ms=32, frame_mov_ms=16, noise_len_ms=480), dict(frame_time=32, frame_mov_t=16, noise_len_t=480)),
    "gen320": (dict(fs=16000, n_mel=40), dict(fs=16000, n_mel=40)),
    "gen400": (dict(fs=20000, n_mel=30), dict(fs=20000, n_mel=30)),
    "gen512": (dict(frame_time_ms=64, frame_mov_ms=32, n_mel=64, noise_len_ms=960), dict(frame_time=64, frame_mov_t=32, n_mel=64, noise_len_t=960)),
}
NAMES = tuple(FRONT_ENDS)

# the store: (channel, first frame, rows) of each slot's piece; slot 3 is invalid; slots 1 and 4 are one word
PIECES = ((0, 5, 12), (1, 20, 25), (0, 45, 40), (1, 0, 20), (2, 10, 18), (2, 55, 30))
VALID = (1, 1, 1, 0, 1, 1)
WORD_OF_SLOT = (0, 1, 2, 2, 1, 3)
LABELS = (0, 1, 2, 3)


def framing(name):
    """(frame_len, hop) from the engine keywords: fs // 1000 * frame_time_ms samples, half of it"""
    kw = FRONT_ENDS[name][0]
    frame_len = kw.get("fs", 8000) // 1000 * kw.get("frame_time_ms", 20)
    return frame_len, frame_len // 2


def pcm_frames(samples, frame_len, hop):
    """brute force: the frames j whose last sample 1 + j * hop + frame_len - 1 has arrived"""
    j = 0
    while 1 + j * hop + frame_len <= samples:
        j += 1
    return j


def _freeze(fx):
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


def _audio(seed, hop, R):
    """two tones per channel whose frequencies wander over some tens of frames, and noise: u16 codes around the channel's mid"""
    rng = np.random.default_rng(seed)
    t = np.arange(R)
    X = np.empty((N_CH, R), np.uint16)
    for c in range(N_CH):
        w1 = 0.05 + 0.03 * c + 0.04 * np.sin(2 * np.pi * t / (hop * (23 + 5 * c)))
        w2 = 0.21 + 0.05 * c + 0.08 * np.sin(2 * np.pi * t / (hop * (37 - 4 * c)) + c)
        x = MID[c] + 600 * np.sin(np.cumsum(w1)) + 350 * np.sin(np.cumsum(w2)) + rng.integers(-250, 251, R)
        X[c] = np.clip(np.rint(x), 0, 4095)
    return X


def oracle(name):
    return ol.Oracle(MAXF, **FRONT_ENDS[name][1])


@functools.lru_cache(maxsize=None)
def case(name):
    frame_len, hop = framing(name)
    idx = NAMES.index(name)
    r = 1 + (7 + 13 * idx) % (hop - 1)  # 0 < r < hop: samples that never complete a frame
    assert 0 < r < hop
    R1 = 1 + (N_FR - 1) * hop + frame_len + r
    R3 = 3 * R1
    X = _audio(4100 + idx, hop, R3)
    orc = oracle(name)
    assert (orc.frame_len, orc.hop, orc.n_coef) == (frame_len, hop, 12)
    feat = np.zeros((N_CH, N_FR, 12), np.int16)
    for c in range(N_CH):
        n, m = orc.mfcc(X[c, :R1], 1, R1, ol.Atap(MID[c], 0, 0, 0))
        assert n == N_FR
        feat[c] = m
    im = np.zeros((N_CH + 1, MAXF, 12), np.int16)
    im[:N_CH, :N_FR] = feat
    inf = np.array([N_FR] * N_CH + [0], np.uint32)
    tf = np.array([p[2] for p in PIECES], np.uint32)
    tm = np.zeros((len(PIECES), int(tf.max()) + 1, 12), np.int16)
    for k, (c, at, rows) in enumerate(PIECES):
        tm[k, :rows] = feat[c, at:at + rows]
    skip = int(np.median(spot_ref.local_dis(feat[0], tm[1, :tf[1]])))  # a typical frame distance
    every = list(LABELS)
    grams = dict(anchor=gram_ref.grammar_any(LABELS),
                 seq=gram_ref.grammar_sequence([every, every, [1, 2, 3, 0], every], optional_tail=True))
    bigram = wgram_ref.grammar_bigram(LABELS, {a: {b: 130 * a + 70 * b + 9 for b in LABELS} for a in LABELS}, None, {0: 0, 1: 40, 2: 7, 3: 300})
    return _freeze(dict(name=name, ekw=FRONT_ENDS[name][0], okw=FRONT_ENDS[name][1], frame_len=frame_len, hop=hop, r=r, R1=R1, R3=R3, X=X,
                        mid=np.array(MID, np.uint32), feat=feat, im=im, inf=inf, tm=tm, tf=tf, valid=np.array(VALID, np.uint8),
                        wos=np.array(WORD_OF_SLOT, np.uint32), skip=skip, word_cost=WORD_COST, grams=grams, bigram=bigram,
                        repeat=onepass_gram_ref.grammar_repeat([every], every, 0), chunk_max=2 * frame_len + hop,
                        block=onepass_ref.reach(tf, VALID)))


def store(fx):
    return fx["tm"], fx["tf"], fx["valid"]


@functools.lru_cache(maxsize=None)
def long_feats(name):
    """int16 [N_CH, frames of R3 samples, 12]"""
    fx, orc = case(name), oracle(name)
    frame_len, hop = fx["frame_len"], fx["hop"]
    nf = pcm_frames(fx["R3"], frame_len, hop)
    out = np.zeros((N_CH, nf, 12), np.int16)
    for p in range(0, nf, MAXF):
        cnt = min(MAXF, nf - p)
        s = 1 + p * hop
        e = s + (cnt - 1) * hop + frame_len
        for c in range(N_CH):
            n, m = orc.mfcc(fx["X"][c], s, e, ol.Atap(MID[c], 0, 0, 0))
            assert n == cnt
            out[c, p:p + cnt] = m
    out.setflags(write=False)
    return out


def _frozen(out):
    for a in out if isinstance(out, tuple) else (out,):
        a.setflags(write=False)
    return out


# ---- the references, each computed once per front end ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_spot(name):
    fx = case(name)
    return _frozen(spot_ref.spot_hits(fx["im"], fx["inf"], *store(fx), MAXF, WIN))


@functools.lru_cache(maxsize=None)
def want_windows(name, long=False):
    """per channel SPOT_DTYPE [windows, K]: what a spotting session emits for the R1 (long: R3) samples"""
    fx = case(name)
    f = long_feats(name) if long else fx["feat"]
    return tuple(_frozen(spot_live_ref.window_records(f[c], *store(fx), WIN)) for c in range(N_CH))


@functools.lru_cache(maxsize=None)
def want_chain(name):
    fx = case(name)
    return _frozen(chain_ref.decode(fx["im"], fx["inf"], *store(fx), MAXF, MAX_WORDS, 0, fx["skip"], WORD_COST, fx["wos"]))


@functools.lru_cache(maxsize=None)
def want_gram(name, which):
    fx = case(name)
    return _frozen(gram_ref.decode(fx["grams"][which], fx["im"], fx["inf"], *store(fx), MAXF, MAX_WORDS, 0, fx["skip"], WORD_COST, fx["wos"]))


@functools.lru_cache(maxsize=None)
def want_wgram(name):
    fx = case(name)
    return _frozen(wgram_ref.decode(fx["bigram"], fx["im"], fx["inf"], *store(fx), MAXF, MAX_WORDS, 0, fx["skip"], WORD_COST, fx["wos"]))


@functools.lru_cache(maxsize=None)
def want_onepass(name, long=False):
    fx = case(name)
    if not long:
        return _frozen(onepass_ref.decode(fx["im"], fx["inf"], *store(fx), MAXF, OP_WORDS, fx["skip"], WORD_COST, fx["wos"]))
    f = long_feats(name)
    return _frozen(onepass_ref.decode(f, [f.shape[1]] * N_CH, *store(fx), f.shape[1], OP_WORDS, fx["skip"], WORD_COST, fx["wos"]))


@functools.lru_cache(maxsize=None)
def want_opgram(name, which):
    fx = case(name)
    gram = fx["bigram"] if which == "bigram" else fx[which]
    return _frozen(onepass_gram_ref.decode(gram, fx["im"], fx["inf"], *store(fx), MAXF, OP_WORDS, fx["skip"], WORD_COST, fx["wos"]))


# ---- push schedules -----------------------------------------------------------------------------------------------------------------
def random_chunking(rng, N, hi):
    """sizes 0..hi that sum to N, zeros and ones included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(0, hi + 1))])), N - sum(out)))
    return out


def cut(N, sizes):
    """the sizes in rotation until N samples are used up"""
    out, i = [], 0
    while sum(out) < N:
        out.append(min(sizes[i % len(sizes)], N - sum(out)))
        i += 1
    return out


def per_channel(lists):
    """one chunking per channel -> per push the counts (0 once a channel is done)"""
    n = max(len(x) for x in lists)
    return [[x[i] if i < len(x) else 0 for x in lists] for i in range(n)]


@functools.lru_cache(maxsize=None)
def schedules(name):
    """dev / host: two different schedules over R1 samples; long_spot / long_onepass: over R3.  Every one cuts a channel at
    hop - 1, hop, hop + 1, frame_len, frame_len + 1, chunk_max and 0 samples, dev and the long ones hold a random chunking, and
    dev pushes the first frame_len + 2 samples of channel 0 one at a time"""
    fx = case(name)
    fl, hop, cm, R1, R3 = fx["frame_len"], fx["hop"], fx["chunk_max"], fx["R1"], fx["R3"]
    rng = np.random.default_rng(700 + NAMES.index(name))
    edges = [hop - 1, hop, hop + 1, fl, fl + 1, cm, 0]
    return dict(dev=per_channel([[1] * (fl + 2) + cut(R1 - fl - 2, edges), random_chunking(rng, R1, cm), cut(R1, [cm, 0, fl + 1, hop + 1, hop - 1, fl, hop])]),
                host=per_channel([cut(R1, [cm, cm - 1, 1]), cut(R1, [fl + 1, hop]), cut(R1, edges[::-1])]),
                long_spot=per_channel([random_chunking(rng, R3, cm), cut(R3, [cm, hop + 1, 0, fl - 1]), cut(R3, edges)]),
                long_onepass=per_channel([cut(R3, [cm, cm - 1, 1, hop]), random_chunking(rng, R3, cm), cut(R3, edges[::-1])]))


def frames_per_push(sched, frame_len, hop):
    """per push and channel (frames before, new frames, samples after): the host-side count of a schedule"""
    got, out = [0] * len(sched[0]), []
    for cnt in sched:
        now = [g + n for g, n in zip(got, cnt)]
        out.append([(spot_live_ref.pcm_frames(g, frame_len, hop), spot_live_ref.pcm_frames(a, frame_len, hop) - spot_live_ref.pcm_frames(g, frame_len, hop), a)
                    for g, a in zip(got, now)])
        got = now
    return out


def schedule_facts(sched, frame_len, hop, win, block):
    """what a schedule must hold for a session run over it to mean anything: (a push of samples that completes no frame, a push
    that completes at least two frames and leaves samples behind its last frame, a window boundary strictly inside a push, a
    block boundary strictly inside a push)"""
    none = two_rest = in_win = in_block = False
    for cnt, row in zip(sched, frames_per_push(sched, frame_len, hop)):
        for n, (before, new, after) in zip(cnt, row):
            none |= n > 0 and new == 0
            two_rest |= new >= 2 and after > 1 + (before + new - 1) * hop + frame_len
            in_win |= any(m % win == 0 for m in range(before + 1, before + new))
            in_block |= any(m % block == 0 for m in range(before + 1, before + new))
    return none, two_rest, in_win, in_block
