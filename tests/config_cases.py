"""Seeded random configurations for tests/test_config_sweep_ref.py (CPU) and tests/test_config_sweep.py (GPU): a template
store, feature rows, call parameters, one grammar, a live push schedule and one draw of every testing hook, all from
np.random.default_rng(BASE + i) alone, so a failure names its seed.  Every draw comes from a short list that holds the edges
the hand-built fixtures visit one at a time (one-frame templates, sweeps of more than 64 columns, full-scale rows whose squared
distance wraps u32, ties, word groups of more than 64 items, the caps); here they meet.

  config(i)   i in range(N_CONFIGS) -> one frozen, cached dict:
    store     K, tm int16 [K, rows, 12], tf [K], valid uint8 [K], wos (word of slot) [K], labels (the distinct labels), amp, L
    rows      maxf, im int16 [n, maxf, 12], inf [n] (as given: a count may exceed maxf), n_frames [n] (clamped), frames_stride,
              row_kind [n], planted [n] (the planted slots of a row)
    calls     skip_kind, skip, word_cost, max_words, n_exact, words_cap, frames_cap, win, tail
    grammar   gram_kind, gram (n_states, arcs, final), wgram (the same with arc and final costs: its own where the kind has
              them, drawn small ones elsewhere), transcripts (one label list per row) and words_per_row for the forced aligner
    live      live = [(row, [chunk sizes])] per channel, reuse = (channel, row, [chunk sizes]): the channel that is ended and
              pushed a second recording
    hooks     {name: value}, 0 = unset
    refused   {family: error code} where a draw breaks a documented limit (the references' cost_ok decides)

The work of the references (plain Python for the one-pass forms) bounds the row count: a configuration whose store is long
keeps fewer rows than it drew.  Plain module: no fixtures, no pytest settings.
"""
import functools

import numpy as np

import gram_ref
import onepass_gram_ref
import onepass_ref
import wgram_ref

BASE = 54000
N_CONFIGS = 28
BAD_ARG = 3

K_DRAW = (1, 2, 3, 5, 8, 12)
K_BIG, BIG_IDS = 70, (9, 20)             # two stores of 70 short templates: a grammar level of more than 64 items
WIDE_ID, WIDE_WORDS = 14, 16             # the one configuration with max_words = 16
BANDS = ((1, 3), (4, 16), (17, 63), (64, 130))
AMPS = (2, 300, 3000, 32767)
MAXF_DRAW = (33, 64, 65, 130, 200)
ROWS_DRAW = (1, 3, 4, 5, 9)
SKIP_KINDS = ("off", "zero", "random", "max")
WORD_COSTS = (0, 700, 1 << 20)
WORDS_CAPS = (1, 2, 16, 64)
WINS = (0, 1, 7, 50)
GRAM_KINDS = ("anchor", "sequence", "pairs", "repeat", "bigram", "arcs")
COSTS = (0, "small", 1 << 24)
ROW_KINDS = ("planted", "noise", "count", "cut")
CELL_BUDGET = 1_000_000                  # one-pass reference: frames x template rows over the whole batch (plain Python cells)
DIAG_BUDGET = 90_000                     # level references: levels x slots x anti-diagonals over the whole batch (numpy steps)
HOOK_DRAWS = dict(onepass_block=(0, 1, 2, 1000), onepass_rows=(0, 1, 3), chain_rows=(0, 1, 3), chain_chunk_cols=(0, 1, 7, 64),
                  spot_chunk_cols=(0, 1, 7, 64), span_groups=(0, 1, 2), forced_prune_off=(0, 1), onepass_gram_prune_off=(0, 1))


def _pick(rng, choices, p=None):
    return choices[int(rng.choice(len(choices), p=p))]


def _subset(rng, items, lo=1):
    """a random subset of at least lo items, in the items' order"""
    items = list(items)
    n = int(rng.integers(min(lo, len(items)), len(items) + 1))
    keep = sorted(rng.choice(len(items), n, replace=False).tolist())
    return [items[i] for i in keep]


def _cost(rng):
    c = _pick(rng, COSTS, [0.4, 0.5, 0.1])
    return int(rng.integers(1, 2001)) if c == "small" else int(c)


# ---- the store -----------------------------------------------------------------------------------------------------------------
def _store(rng, i):
    big = i in BIG_IDS
    K = K_BIG if big else int(_pick(rng, K_DRAW))
    amp = int(_pick(rng, AMPS, [0.31, 0.23, 0.23, 0.23]))  # the tie-rich amplitude a little more often
    kind = _pick(rng, ("mixed", "long", "one band"), [0.6, 0.15, 0.25])
    one = int(rng.integers(0, 4))
    tf = np.zeros(K, np.uint32)
    for k in range(K):
        band = int(rng.choice(4, p=[0.3, 0.35, 0.2, 0.15]))  # drawn per template: stores mix bands
        band = min(band, 1) if big else 3 if kind == "long" else one if kind == "one band" else band
        tf[k] = rng.integers(BANDS[band][0], BANDS[band][1] + 1)
    tm = np.zeros((K, int(tf.max()) + 1, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-amp, amp + 1, (int(tf[k]), 12))
    valid = (rng.random(K) >= 0.2).astype(np.uint8)  # about one slot in five is erased
    if not valid.any():
        valid[int(rng.integers(0, K))] = 1
    if big:  # three erased slots only, and few words: more than 64 slots stay in a grammar's reach
        valid[:] = 1
        valid[rng.choice(K, 3, replace=False)] = 0
    W = int(rng.integers(1, min(K, 12) + 1))
    labels = sorted(int(w) for w in rng.choice(np.arange(3, 400), W, replace=False))  # not contiguous
    order = rng.permutation(K)
    wos = np.zeros(K, np.uint32)
    wos[order[:W]] = rng.permutation(labels)  # every word has a slot; the rest fall anywhere: several slots a word, not grouped
    wos[order[W:]] = rng.choice(labels, K - W)
    return dict(K=K, amp=amp, tm=tm, tf=tf, valid=valid, wos=wos, labels=labels, L=onepass_ref.reach(tf, valid))


# ---- the rows ------------------------------------------------------------------------------------------------------------------
def _plant(rng, st, slots, maxf):
    """the templates of `slots`, every template frame held for one or two input frames, noise of about amp / 50 on every
    coefficient, 0..2 filler frames between words -> (frames [n, 12] cut at maxf, the spans that fit)"""
    amp, noise = st["amp"], st["amp"] // 50
    frames, spans = [], []
    for j, k in enumerate(slots):
        if j:
            frames += [rng.integers(-amp, amp + 1, 12) for _ in range(int(rng.integers(0, 3)))]
        first = len(frames)
        for y in range(int(st["tf"][k])):
            for _ in range(1 + int(y > 0 and rng.integers(0, 3) == 0)):
                frames.append(st["tm"][k, y].astype(np.int64) + rng.integers(-noise, noise + 1, 12))
        if len(frames) <= maxf:
            spans.append((first, len(frames) - 1))
    return np.clip(np.array(frames[:maxf]).reshape(-1, 12), -32768, 32767).astype(np.int16), spans


def _rows(rng, st, maxf, n_rows):
    amp = st["amp"]
    ok = [int(k) for k in np.nonzero(st["valid"])[0]]
    im = rng.integers(-amp, amp + 1, (n_rows, maxf, 12)).astype(np.int16)  # what lies behind a row's count is as loud as the row
    inf = np.zeros(n_rows, np.uint32)
    kinds, planted = [], []
    for r in range(n_rows):
        kind = _pick(rng, ROW_KINDS, [0.55, 0.12, 0.2, 0.13])
        slots = [ok[int(j)] for j in rng.integers(0, len(ok), int(rng.integers(1, 5)))]
        if kind == "noise":
            slots, inf[r] = [], rng.integers(1, maxf + 1)
        else:
            f, spans = _plant(rng, st, slots, maxf)
            slots = slots[:len(spans)]
            im[r, :len(f)] = f
            inf[r] = spans[-1][1] + 1 if spans else len(f)
            if kind == "count":
                inf[r] = _pick(rng, (0, 1, 2, maxf, maxf + 7))  # the last is clamped
            elif kind == "cut" and spans:
                inf[r] = (spans[-1][0] + spans[-1][1] + 1) // 2 + 1  # the middle of the last word
        kinds.append(kind)
        planted.append(slots)
    return im, inf, kinds, planted


# ---- the grammar ---------------------------------------------------------------------------------------------------------------
def _arcs(rng, labels):
    """a random arc list over 2..6 states: no arc enters the start; with four states or more the last state is unreachable (arcs
    leave it, none enters) and the one before reaches no final state (arcs enter, none leaves); costs from {0, small, 2^24}"""
    S = int(rng.integers(2, 7))
    live = list(range(1, S - 2)) if S >= 4 else list(range(1, S))  # the states on paths from the start to a final state
    final = [0] * S
    for s in _subset(rng, live):
        final[s] = 1
    arcs = {(0, live[0], int(_pick(rng, labels)))}
    if final[live[0]] == 0:
        arcs.add((live[0], min(s for s in live if final[s]), int(_pick(rng, labels))))
    for _ in range(int(rng.integers(1, 9))):
        arcs.add((int(_pick(rng, [0] + live)), int(_pick(rng, live)), int(_pick(rng, labels))))
    if S >= 4:
        dead, lost = S - 2, S - 1
        arcs.add((int(_pick(rng, [0] + live)), dead, int(_pick(rng, labels))))
        arcs.add((lost, int(_pick(rng, live)), int(_pick(rng, labels))))
        final[lost] = int(rng.integers(0, 2))
    arcs = sorted(arcs)
    return S, arcs, final, [_cost(rng) for _ in arcs], [_cost(rng) if f else 0 for f in final]


def _grammar(rng, labels, kind, seed):
    """-> (gram, wgram)"""
    if kind in ("pairs", "bigram"):
        labels = labels[:12]  # a state per word: the grammar's 64 states bound the words of these two kinds
    if kind == "anchor":
        g = gram_ref.grammar_any(labels)
    elif kind == "sequence":
        g = gram_ref.grammar_sequence([_subset(rng, labels) for _ in range(int(rng.integers(1, 4)))], bool(rng.integers(0, 2)))
    elif kind == "pairs":
        pairs = [(a, b) for a in labels for b in labels if rng.integers(0, 2)]
        g = gram_ref.grammar_word_pairs(labels, pairs, None if rng.integers(0, 2) else _subset(rng, labels),
                                        None if rng.integers(0, 2) else _subset(rng, labels))
    elif kind == "repeat":
        g = onepass_gram_ref.grammar_repeat([_subset(rng, labels) for _ in range(int(rng.integers(0, 3)))], _subset(rng, labels), int(rng.integers(0, 3)))
    elif kind == "bigram":
        def c():
            return None if rng.integers(0, 5) == 0 else 0 if rng.integers(0, 3) == 0 else int(rng.integers(1, 2001))
        first = {w: c() for w in labels}
        first[labels[0]] = 0
        last = {w: c() for w in labels}
        last[labels[-1]] = 7
        w5 = wgram_ref.grammar_bigram(labels, {a: {b: c() for b in labels} for a in labels}, first, last)
        return tuple(w5[:3]), w5
    else:
        w5 = _arcs(rng, labels)
        return tuple(w5[:3]), w5
    return g, wgram_ref.drawn_costs(g, seed, 2000)


# ---- live use ------------------------------------------------------------------------------------------------------------------
def _chunks(rng, N, L):
    sizes = sorted({0, 1, 2, max(L - 1, 0), L, L + 1, 70})
    out = []
    while sum(out) < N:
        out.append(min(int(_pick(rng, sizes)), N - sum(out)))
    return out


@functools.lru_cache(maxsize=None)
def config(i):
    assert 0 <= i < N_CONFIGS
    rng = np.random.default_rng(BASE + i)
    st = _store(rng, i)
    maxf, n_rows = int(_pick(rng, MAXF_DRAW)), int(_pick(rng, ROWS_DRAW))
    max_words = WIDE_WORDS if i == WIDE_ID else int(rng.integers(1, 7))
    T = int(st["tf"][st["valid"] != 0].sum())
    n_ok = int((st["valid"] != 0).sum())
    while n_rows > 1 and (n_rows * maxf * T > CELL_BUDGET or n_rows * max_words * n_ok * (maxf + T // n_ok) > DIAG_BUDGET):
        n_rows = max(r for r in ROWS_DRAW if r < n_rows)
    im, inf, kinds, planted = _rows(rng, st, maxf, n_rows)
    n_frames = np.minimum(inf, maxf).astype(np.uint32)
    skip_kind = _pick(rng, SKIP_KINDS)
    skip = dict(off=None, zero=0, random=int(rng.integers(1, 3001)), max=65535)[skip_kind]
    word_cost = int(_pick(rng, WORD_COSTS, [0.5, 0.35, 0.15]))
    n_exact = int(rng.integers(1, max_words + 1)) if rng.integers(0, 3) == 0 else 0
    words_cap = int(_pick(rng, WORDS_CAPS))
    frames_cap = int(rng.integers(1, max(int(n_frames.max()), 2))) if rng.integers(0, 3) == 0 else 0  # inside the longest row
    gram_kind = _pick(rng, GRAM_KINDS)
    gram, wgram = _grammar(rng, st["labels"], gram_kind, BASE + i)
    gram_ref.check(gram, st["labels"])
    transcripts = []
    for r in range(n_rows):
        t = [int(st["wos"][k]) for k in planted[r]]
        if not t and rng.integers(0, 3):
            t = [int(w) for w in rng.choice(st["labels"], int(rng.integers(1, 4)))]
        transcripts.append(t[:max_words])
    n_ch = int(rng.integers(1, 6))
    live = [(int(r), _chunks(rng, int(n_frames[r]), st["L"])) for r in rng.integers(0, n_rows, n_ch)]
    again = int(rng.integers(0, n_rows))
    reuse = (int(rng.integers(0, n_ch)), again, _chunks(rng, int(n_frames[again]), st["L"]))
    hooks = {name: int(_pick(rng, draws)) for name, draws in HOOK_DRAWS.items()}
    cap = min(maxf, frames_cap) if frames_cap else maxf
    refused = {}
    if not onepass_ref.cost_ok(cap, st["L"], word_cost):
        refused["onepass"] = BAD_ARG
    if not onepass_gram_ref.cost_ok(cap, st["L"], word_cost, wgram):
        refused["onepass_grammar"] = BAD_ARG
    if not onepass_ref.cost_ok(maxf, st["L"], word_cost):
        refused["onepass_live"] = BAD_ARG
    if not onepass_gram_ref.cost_ok(maxf, st["L"], word_cost, wgram):
        refused["onepass_grammar_live"] = BAD_ARG
    cfg = dict(st, id=i, seed=BASE + i, maxf=maxf, im=im, inf=inf, n_frames=n_frames, frames_stride=int(_pick(rng, (1, 3, 12))), row_kind=tuple(kinds),
               planted=tuple(tuple(p) for p in planted), skip_kind=skip_kind, skip=skip, word_cost=word_cost, max_words=max_words, n_exact=n_exact,
               words_cap=words_cap, frames_cap=frames_cap, win=int(_pick(rng, WINS)), tail=bool(rng.integers(0, 3) == 0), gram_kind=gram_kind,
               gram=gram, wgram=wgram, transcripts=transcripts, words_per_row=max(1, max(len(t) for t in transcripts)), live=live, reuse=reuse,
               hooks=hooks, refused=refused)
    for v in cfg.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cfg


def store(cfg):
    return cfg["tm"], cfg["tf"], cfg["valid"]


def strided(cfg):
    """the frame counts as a strided record: all ones between them"""
    rec = np.full(len(cfg["inf"]) * cfg["frames_stride"], 0xFFFFFFFF, np.uint32)
    rec[::cfg["frames_stride"]] = cfg["inf"]
    return rec
