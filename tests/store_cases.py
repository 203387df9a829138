"""Stores of real size for tests/test_store_sizes.py: the longest template the LDS image takes, 65 536 slots, and a dense
store whose word groups and grammar item lists pass 64 entries.  Every decoder test before these ran on stores of at most
about ten slots of at most 65 rows.

  longest(cap)   3 slots of cap, cap - 63 and 30 rows (cap = max_tpl_rows of the geometry calls), max_frames = cap + 100
  sparse()       65 536 slots of 3..8 rows, ten of them valid: both ends, both sides of 64, 256 and 32 768, two exact twins
  dense()        300 valid slots of 3..8 rows in 40 words with groups of 1, 2, 63, 64, 65 and 3 slots
  too_many()     65 537 slots, one valid: what the header's limit of 65 536 refuses

A fixture is a dict: tm int16 [K, rows, 12], tf [K], valid [K] or None, wos (word of slot) [K] or None, im int16 [n, maxf, 12],
inf [n], maxf, max_words, skip, transcripts (one label list per row) and the grammars of its tests.  The arrays are
read-only.  Plain module: no fixtures, no pytest settings.
"""
import functools

import numpy as np

import gram_ref
import onepass_gram_ref
import wgram_ref

AMP = 3000


def _freeze(fx):
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


def _rand(rng, shape):
    return rng.integers(-AMP, AMP + 1, shape).astype(np.int16)


# ---- 1: the longest template ----------------------------------------------------------------------------------------------------
LONG_WORDS, LONG_SKIP, LONG_ROWS = 3, 8000, "abcde"


@functools.lru_cache(maxsize=None)
def longest(cap):
    """rows (a) 20 filler frames, template 0 with noise of +-3, template 2, filler; (b) template 0 played slower: every 16th
    row held for a second frame, cap + cap / 16 frames = max_frames at cap 1600 (a slower one does not fit max_frames);
    (c) cap / 2 frames, one too few for the cap-row word; (d) cap / 2 + 1 frames, every second row of template 0 and its
    last: the word is just reachable, along steps of two rows per frame only; (e) template 1, then template 2"""
    rng = np.random.default_rng(1600)
    maxf = cap + 100
    tf = np.array([cap, cap - 63, 30], np.uint32)
    tm = np.zeros((3, cap + 1, 12), np.int16)
    for k in range(3):
        tm[k, :tf[k]] = _rand(rng, (tf[k], 12))
    im = _rand(rng, (5, maxf, 12))  # what is not a word is filler as loud as the words
    inf = np.zeros(5, np.uint32)
    im[0, 20:20 + cap] = tm[0, :cap] + rng.integers(-3, 4, (cap, 12))
    im[0, 20 + cap:50 + cap] = tm[2, :30]
    inf[0] = min(maxf, cap + 70)
    held = np.sort(np.concatenate([np.arange(cap), np.arange(15, cap, 16)]))[:maxf]
    im[1, :len(held)] = tm[0, held]
    inf[1] = len(held)
    inf[2] = cap // 2
    im[2, :inf[2]] = tm[0, 0:2 * inf[2]:2]
    rows_d = np.concatenate([np.arange(0, cap - 1, 2), [cap - 1]])[:cap // 2 + 1]
    assert len(rows_d) == cap // 2 + 1 and rows_d[-1] == cap - 1
    im[3, :len(rows_d)] = tm[0, rows_d]
    inf[3] = len(rows_d)
    im[4, :cap - 63] = tm[1, :cap - 63]
    im[4, cap - 63:cap - 33] = tm[2, :30]
    inf[4] = cap - 33
    seq = gram_ref.grammar_sequence([[0, 1], [2]])  # "long word, then short word"
    drawn = wgram_ref.drawn_costs(gram_ref.grammar_word_pairs(range(3), [(a, b) for a in range(3) for b in range(3) if a != b or a == 2]))
    bigram = wgram_ref.grammar_bigram(range(3), {a: {b: 700 * a + 300 * b + 11 for b in range(3)} for a in range(3)}, None, {0: 5, 1: 0, 2: 900})
    return _freeze(dict(name="longest", tm=tm, tf=tf, valid=None, wos=None, im=im, inf=inf, maxf=maxf, max_words=LONG_WORDS, skip=LONG_SKIP,
                        transcripts=[[0, 2], [0], [2], [0], [1, 2]], labels=[0, 1, 2], grams=dict(seq=seq), wgrams=dict(drawn=drawn),
                        op_grams=dict(repeat=onepass_gram_ref.grammar_repeat([[0, 1]], [2], 0), bigram=bigram),
                        live_rows=(0, 3), live_sizes=(1, 63, 64, 700), spot_win=256))


def without_short_slot(fx):
    """the store of slots 0 and 1 alone: L = (cap - 63) / 2 + 1, one-pass sweeps of more than 64 columns"""
    out = dict(fx, name=fx["name"] + ", two slots", tm=fx["tm"][:2], tf=fx["tf"][:2], labels=[0, 1],
               op_grams=dict(repeat=onepass_gram_ref.grammar_repeat([[0, 1]], [0, 1], 0),
                             bigram=wgram_ref.grammar_bigram(range(2), {a: {b: 700 * a + 300 * b + 11 for b in range(2)} for a in range(2)}, None, {0: 5, 1: 0})))
    return out


# ---- 2: 65 536 slots, ten of them valid -----------------------------------------------------------------------------------------
SPARSE_K, SPARSE_MAXF, SPARSE_SKIP = 65536, 64, 5000
SPARSE_VALID = (0, 63, 64, 255, 256, 32767, 32768, 32769, 65534, 65535)
SPARSE_TWINS = ((32768, 32767), (65534, 64))  # (the copy, its original): the copy has the larger slot and loses every tie
SPARSE_WORDS = {0: (0, 65535), 1: (63, 32767, 32768), 2: (64, 65534), 3: (255, 256, 32769)}  # word 4: every invalid slot


def _plant(im, r, rng, tm, tf, slots, gap=1, lead=0):
    """templates back to back in row r with `gap` filler frames between them -> the frames used"""
    at = lead
    for i, k in enumerate(slots):
        n = int(tf[k])
        im[r, at:at + n] = tm[k, :n]
        at += n + (gap if i + 1 < len(slots) else 0)
    return at


@functools.lru_cache(maxsize=None)
def sparse(K=SPARSE_K):
    """rows (a) templates 65 535, 32 769, 256, 32 767 with one filler frame between them; (b) templates 65 534 and 0; (c) a
    random row; (d) one frame; (e) no frame"""
    rng = np.random.default_rng(65536)
    tf = rng.integers(3, 9, K).astype(np.uint32)
    tm = np.zeros((K, 9, 12), np.int16)
    valid = np.zeros(K, np.uint8)
    for k in SPARSE_VALID:
        valid[k] = 1
        tm[k, :tf[k]] = _rand(rng, (tf[k], 12))
    for copy, of in SPARSE_TWINS:
        tm[copy], tf[copy] = tm[of], tf[of]
    wos = np.full(K, 4, np.uint32)
    for w, slots in SPARSE_WORDS.items():
        wos[list(slots)] = w
    im = _rand(rng, (5, SPARSE_MAXF, 12))
    inf = np.zeros(5, np.uint32)
    inf[0] = _plant(im, 0, rng, tm, tf, (65535, 32769, 256, 32767))
    inf[1] = _plant(im, 1, rng, tm, tf, (65534, 0), gap=0)
    inf[2], inf[3], inf[4] = SPARSE_MAXF, 1, 0
    pairs = gram_ref.grammar_word_pairs(range(4), [(a, b) for a in range(4) for b in range(4) if a != b])
    arcs = pairs[1] + [(1, 2, 4), (0, 3, 4)]  # word 4 has no valid slot: its arcs yield no item
    with_none = (pairs[0], arcs, pairs[2])
    bigram = wgram_ref.grammar_bigram(range(4), {a: {b: (130 * a + 70 * b + 9 if a != b else None) for b in range(4)} for a in range(4)},
                                      None, {0: 0, 1: 40, 2: 7, 3: 300})
    return _freeze(dict(name="sparse", tm=tm, tf=tf, valid=valid, wos=wos, im=im, inf=inf, maxf=SPARSE_MAXF, max_words=4, skip=SPARSE_SKIP,
                        transcripts=[[0, 3, 3, 1], [2, 0], [1, 2, 3], [0], []], labels=[0, 1, 2, 3, 4],
                        grams=dict(seq=gram_ref.grammar_sequence([[0, 2], [3, 0], [3], [1]], optional_tail=True), none=with_none),
                        wgrams=dict(drawn=wgram_ref.drawn_costs(with_none)),
                        op_grams=dict(repeat=onepass_gram_ref.grammar_repeat([[0, 2]], [0, 1, 3, 4], 1), bigram=bigram),
                        live_rows=(0, 1), live_words=2, live_sizes=(1, 7, 8), spot_win=16))


# ---- 3: 300 valid slots in 40 words ---------------------------------------------------------------------------------------------
DENSE_K, DENSE_MAXF, DENSE_SKIP, DENSE_WORDS = 300, 64, 5000, 40
DENSE_GROUPS = (1, 2, 63, 64, 65) + (3,) * 35
DENSE_BIG = 4  # the word of 65 slots


@functools.lru_cache(maxsize=None)
def dense():
    """8 rows of 64 frames: three templates each, a filler frame between them, most from slots above 64, some above 256; the
    slots of a word are scattered over the store, the word ids are not their ranks"""
    rng = np.random.default_rng(300)
    K = DENSE_K
    assert sum(DENSE_GROUPS) == K and len(DENSE_GROUPS) == DENSE_WORDS
    ids = [1000 - 7 * w for w in range(DENSE_WORDS)]  # descending ids: the groups' order is not the ids' first appearance
    wos = np.repeat(np.array(ids, np.uint32), DENSE_GROUPS)[rng.permutation(K)]
    tf = rng.integers(3, 9, K).astype(np.uint32)
    tm = np.zeros((K, 9, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = _rand(rng, (tf[k], 12))
    big = [int(k) for k in np.nonzero(wos == ids[DENSE_BIG])[0]]
    plant = [(299, 65, 130), (257, big[-1], 64), (big[0], 288, 63), (70, 71, 72), (big[len(big) // 2], 1, 298), (100, 200, 270), (0, 150, 299), (90, 91, 260)]
    im = _rand(rng, (8, DENSE_MAXF, 12))
    inf = np.zeros(8, np.uint32)
    for r, slots in enumerate(plant):
        used = _plant(im, r, rng, tm, tf, slots, lead=r % 3)
        inf[r] = DENSE_MAXF if r % 2 else used
    pairs = gram_ref.grammar_word_pairs(ids, [(a, b) for i, a in enumerate(ids) for j, b in enumerate(ids) if (i + j) % 3 != 1])
    transcripts = [[int(wos[k]) for k in slots] for slots in plant]
    transcripts[5] = [ids[DENSE_BIG]] * 3  # the 65-slot word at every position, whatever was planted
    return _freeze(dict(name="dense", tm=tm, tf=tf, valid=None, wos=wos, im=im, inf=inf, maxf=DENSE_MAXF, max_words=3, skip=DENSE_SKIP,
                        transcripts=transcripts, labels=ids, plant=plant, big=big, grams=dict(pairs=pairs),
                        wgrams=dict(drawn=wgram_ref.drawn_costs(pairs)),
                        op_grams=dict(repeat=onepass_gram_ref.grammar_repeat([ids[:20]], ids, 1),
                                      bigram=wgram_ref.drawn_costs(pairs, seed=9, hi=3000)),
                        live_rows=(0, 1, 4), live_words=3, live_sizes=(1, 7, 8), spot_win=16))


# ---- one slot too many ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def too_many():
    """65 537 slots, slot 65 536 alone valid: three rows, the template inside the first"""
    rng = np.random.default_rng(65537)
    K = SPARSE_K + 1
    tf = np.full(K, 5, np.uint32)
    tm = np.zeros((K, 6, 12), np.int16)
    valid = np.zeros(K, np.uint8)
    valid[K - 1] = 1
    tm[K - 1, :5] = _rand(rng, (5, 12))
    im = _rand(rng, (3, 32, 12))
    im[0, 4:9] = tm[K - 1, :5]
    return _freeze(dict(name="too many", tm=tm, tf=tf, valid=valid, wos=None, im=im, inf=np.array([20, 32, 3], np.uint32), maxf=32, max_words=2,
                        skip=SPARSE_SKIP))
