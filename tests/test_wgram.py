"""Weighted grammars on the device: arc and final costs in grammar-constrained decoding (include/sr_engine.h, "weighted
grammars").

The definition lives in tests/wgram_ref.py (its own checks are tests/test_wgram_ref.py).  Every comparison here is byte for
byte against it -- records, every word row with the grammar state in `reserved`, level costs -- and, for all-zero costs,
against what the same grammar made by sr_grammar_create writes.  No tolerances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_ref
import gram_ref
import wgram_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine

BAD_ARG = 3
U32, P = C.c_uint32, C.c_void_p
MAXF, W, SKIP = chain_ref.PLANT_MAXF, 4, chain_ref.PLANT_SKIP  # 4 levels: the planted rows hold 1..4 words
SPW2 = np.arange(chain_ref.PLANT_K, dtype=np.uint32) // 2  # two slots per word: labels 0, 0, 1, 1, 2
PAIR_GRAM = gram_ref.grammar_word_pairs(range(5), [(a, b) for a in range(5) for b in range(5) if (a + b) % 2 == 1], first=[0, 1, 2, 4])
# two slots per word: word 2 enters state 3 from state 1 and from state 2
JOIN_GRAM = (4, [(0, 1, 0), (0, 2, 1), (1, 3, 2), (2, 3, 2), (3, 1, 0), (1, 1, 1), (3, 2, 1)], [0, 1, 0, 1])
GRAMS = dict(join=(JOIN_GRAM, SPW2), pairs=(PAIR_GRAM, None), anchor=(gram_ref.grammar_any(range(5)), None))
# the edge store of the grammar tests, restated: template and row lengths around the 64-column sweep and the chunk seams
EDGE_M = (1, 2, 3, 14, 63, 64, 65)
EDGE_N = sorted({0, 1, 63, 64, 65, 128, 129, MAXF} | {m // 2 for m in EDGE_M} | {m // 2 + 1 for m in EDGE_M})
EDGE_WORDS = 3
EDGE_SKIP = {2: 7, 3000: 8000}  # about what a frame costs inside a word: both choices occur
EDGE_GRAM = (4, [(0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 2, 3), (1, 2, 3), (1, 2, 4), (1, 2, 0), (2, 3, 5), (2, 3, 6), (2, 3, 4), (2, 2, 1)], [0, 0, 1, 1])


def skip_arg(skip):
    return DIS_ERR if skip is None else skip


def same(got, want, what):
    """(rec, words, level_cost) against the reference's, byte for byte"""
    for name, g, w, width in zip(("rec", "words", "level_cost"), got, want, (4, 8, 1)):
        if g is None:
            continue
        g, w = np.asarray(g).view(np.uint32).reshape(-1, width), np.asarray(w).view(np.uint32).reshape(-1, width)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero(np.any(g != w, 1))[0]
        if len(bad):
            raise AssertionError(f"{what}: {len(bad)} of {len(w)} {name} entries differ, first at {int(bad[0])}: "
                                 f"got {g[bad[0]].tolist()} want {w[bad[0]].tolist()}")


def as_bytes(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out if a is not None)


def dev(a):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def gram_call(eng, gram, im, frames, max_words, n_words=0, skip=None, word_cost=0, canary=0xA5, want_lc=True):
    """sr_decode_grammar_dp_dev into guarded buffers whose every byte starts as the canary"""
    n = len(im)
    d_im, d_frames = dev(im), dev(np.ascontiguousarray(frames, dtype=np.uint32))
    g_r = guarded_out((n,), ref.CHAIN_REC_DTYPE, canary, 4096, "cuda:0", "rec")
    g_w = guarded_out((n, max_words), ref.CHAIN_WORD_DTYPE, canary, 4096, "cuda:0", "words")
    g_l = guarded_out((n, max_words), np.uint32, canary, 4096, "cuda:0", "level_cost")
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_decode_grammar_dp_dev(eng.h, gram.g, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(1), U32(n), U32(max_words), U32(n_words),
                                        U32(skip_arg(skip)), U32(word_cost), P(g_r.ptr), P(g_w.ptr), P(g_l.ptr) if want_lc else None, P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_r.check()
    g_w.check()
    g_l.check() if want_lc else g_l.check_untouched()
    return g_r.interior(), g_w.interior(), g_l.interior() if want_lc else None


def create_weighted(eng, gram, arc_cost, final_cost, expect=0, reserved=0):
    """sr_grammar_create_weighted itself, NULL arrays as None -> a Grammar (expect 0), or the refusal's code with nothing created"""
    a = np.zeros(len(gram[1]), engine.GRAM_ARC_DTYPE)
    for i, arc in enumerate(gram[1]):
        a[i] = tuple(arc) + (reserved,)
    fin = np.ascontiguousarray(gram[2], np.uint8)
    ac = None if arc_cost is None else np.ascontiguousarray(arc_cost, np.uint32)
    fc = None if final_cost is None else np.ascontiguousarray(final_cost, np.uint32)
    g = P(0x5A5A5A5A)  # stays as it is when the call is refused
    rc = eng.L.sr_grammar_create_weighted(eng.h, U32(gram[0]), engine._vp(a), None if ac is None else engine._vp(ac), U32(len(a)), engine._vp(fin),
                                          None if fc is None else engine._vp(fc), C.byref(g))
    assert rc == expect, (rc, eng.L.sr_last_error())
    if rc:
        assert g.value == 0x5A5A5A5A
        return rc
    out = engine.Grammar.__new__(engine.Grammar)
    out.eng, out.L, out.g, out.n_states = eng, eng.L, g, gram[0]
    return out


class hooks:
    """the decoder's development hooks "chain_chunk_cols" / "chain_rows" (testing library only; read per call)"""

    def __init__(self, cols=0, rows=0):
        self.v = dict(chain_chunk_cols=cols, chain_rows=rows)

    def __enter__(self):
        for k, v in self.v.items():
            engine.dev_hook(k, v)

    def __exit__(self, *exc):
        for k in self.v:
            engine.dev_hook(k, 0)


@functools.lru_cache(maxsize=None)
def edge_fixture(amp):
    rng = np.random.default_rng(900 + amp)
    K = len(EDGE_M)
    tf = np.array(EDGE_M, np.uint32)
    tm = np.zeros((K, max(EDGE_M) + 1, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-amp, amp + 1, (tf[k], 12))
    inf = np.array(EDGE_N, np.uint32)
    im = rng.integers(-amp, amp + 1, (len(inf), MAXF, 12)).astype(np.int16)
    r = EDGE_N.index(129)
    im[r, 2:65], im[r, 65:129] = tm[4, :63], tm[5, :64]  # two long words back to back, across a sweep seam: a charged start on either side
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf)


@functools.lru_cache(maxsize=None)
def edge_want(amp, skip_on, hi):
    """the reference over the edge store under EDGE_GRAM with costs drawn from 0..hi"""
    fx = edge_fixture(amp)
    want = ref.decode(ref.drawn_costs(EDGE_GRAM, hi=hi), fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, EDGE_WORDS, 0, EDGE_SKIP[amp] if skip_on else None, 0)
    for a in want:
        a.setflags(write=False)
    return want


def edge_engine(fx, **kw):
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


def planted_engine(word_of_slot=None, **kw):
    fx = chain_ref.planted()
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    if word_of_slot is not None:
        eng.set_word_map(word_of_slot)
    return eng


def costs_for(which, kind):
    gram = GRAMS[which][0]
    if kind == "drawn":
        return ref.drawn_costs(gram)
    if kind == "bound":  # every arc and every final state at the limit
        return ref.with_costs(gram, [ref.MAX_COST] * len(gram[1]), [ref.MAX_COST * int(f != 0) for f in gram[2]])
    return ref.with_costs(gram)


class PlantedHistories:
    """the reference's histories of the planted rows under one weighted grammar, built once per (skip, word_cost): the count
    asked for changes the trace alone"""

    def __init__(self, g, wos):
        self.g, self.wos, self.fx, self.memo = g, wos, chain_ref.planted(), {}
        self.dis = [ref.slot_distances(self.fx["im"][r, :int(self.fx["inf"][r])], self.fx["tm"], self.fx["tf"]) for r in range(len(self.fx["inf"]))]

    def want(self, n_exact, skip, wc):
        if (skip, wc) not in self.memo:
            self.memo[(skip, wc)] = [ref.history(self.g, d, int(N), W, skip, wc, self.wos) for d, N in zip(self.dis, self.fx["inf"])]
        rows = [ref.to_records(ref.trace(A, E, int(N), self.g, W, n_exact, wc, self.wos), self.fx["tf"], W, self.wos)
                for (A, E), N in zip(self.memo[(skip, wc)], self.fx["inf"])]
        return tuple(np.stack([r[i] for r in rows]) for i in range(3))


# ---- 7: zero costs -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["anchor", "edge", "join"])
def test_zero_costs_give_the_unweighted_grammars_bytes_and_plan(which):
    if which == "edge":
        fx, gram_t, wos, mw, skips = edge_fixture(2), EDGE_GRAM, None, EDGE_WORDS, (EDGE_SKIP[2], None)
        eng = edge_engine(fx)
    else:
        fx, (gram_t, wos), mw, skips = chain_ref.planted(), GRAMS[which], W, (SKIP, None)
        eng = planted_engine(wos)
    plain = eng.grammar(*gram_t)
    forms = dict(null=create_weighted(eng, gram_t, None, None), zeros=create_weighted(eng, gram_t, [0] * len(gram_t[1]), [0] * gram_t[0]),
                 arcs_only=create_weighted(eng, gram_t, [0] * len(gram_t[1]), None), python=eng.grammar(*gram_t, arc_cost=None, final_cost=[0] * gram_t[0]))
    for skip in skips:
        want = ref.decode(ref.with_costs(gram_t), fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, mw, 0, skip, 0, wos)
        same(want, gram_ref.decode(gram_t, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, mw, 0, skip, 0, wos), "the reference without costs")
        first = gram_call(eng, plain, fx["im"], fx["inf"], mw, 0, skip)
        same(first, want, f"{which}: sr_grammar_create, skip {skip}")
        host = eng.decode_grammar(plain, fx["im"], fx["inf"], mw, 0, skip)
        for name, g in forms.items():
            assert g.plan(mw) == plain.plan(mw), (which, name)
            assert as_bytes(gram_call(eng, g, fx["im"], fx["inf"], mw, 0, skip)) == as_bytes(first), (which, name, skip, "device form")
            assert as_bytes(eng.decode_grammar(g, fx["im"], fx["inf"], mw, 0, skip)) == as_bytes(host) == as_bytes(first), (which, name, skip, "host form")
    for g in (plain, *forms.values()):
        g.close()
    eng.close()


# ---- 8: costs that bite --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["drawn", "bound"])
@pytest.mark.parametrize("which", ["join", "pairs"])
def test_costs_that_bite_on_the_planted_rows(which, kind):
    fx = chain_ref.planted()
    wos = GRAMS[which][1]
    g = costs_for(which, kind)
    hist = PlantedHistories(g, wos)
    eng = planted_engine(wos)
    gram = eng.grammar(*g)
    if kind == "drawn":  # the parse is not the unweighted one: the costs are looked at
        plain = eng.grammar(*g[:3])
        got, free = gram_call(eng, gram, fx["im"], fx["inf"], W, 0, None), gram_call(eng, plain, fx["im"], fx["inf"], W, 0, None)
        differ = sum(any(got[1][r][f].tolist() != free[1][r][f].tolist() for f in ("slot", "start", "end")) for r in range(len(fx["inf"])))
        assert differ >= (6 if which == "pairs" else 2), (which, differ)
        plain.close()
    for skip in (SKIP, None):
        for wc in (0, 5000, 1 << 24):
            for n_exact in (0, 2, 3):
                want = hist.want(n_exact, skip, wc)
                what = f"{which}, {kind} costs: skip {skip}, n_words {n_exact}, word_cost {wc}"
                same(gram_call(eng, gram, fx["im"], fx["inf"], W, n_exact, skip, wc), want, what)
                if wc == 5000:
                    same(eng.decode_grammar(gram, fx["im"], fx["inf"], W, n_exact, skip, wc), want, what + ", host form")
            if not wc:
                assert (want[0]["status"] == ref.CH_OK).sum() >= 4, (which, kind, skip)
    if kind == "bound":  # three words, each with its arc and word_cost at 2^24, and the final cost: seven times 2^24 and the paths, exact in u32
        top = hist.want(3, None, 1 << 24)
        assert 3 * (2 << 24) + (1 << 24) < int(top[0]["cost"][top[0]["status"] == ref.CH_OK].max()) < ref.cost_bound() < 1 << 32
    gram.close()
    eng.close()


# ---- 9: the edge store ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("amp", [2, 3000])
def test_edge_lengths_under_drawn_costs(amp):
    fx = edge_fixture(amp)
    eng = edge_engine(fx)
    # the draw of the CPU tests; at amplitude 2, where a frame costs a few units, also costs of that size -- or the costs alone decide
    for hi in ((20000, 40) if amp == 2 else (20000,)):
        g = ref.drawn_costs(EDGE_GRAM, hi=hi)
        gram = eng.grammar(*g)
        for skip_on in (True, False):
            skip = EDGE_SKIP[amp] if skip_on else None
            want = edge_want(amp, skip_on, hi)
            assert tuple(want[0][EDGE_N.index(0)]) == (DIS_ERR, 0, 0, ref.CH_NONE) and (want[0]["status"] == ref.CH_OK).sum() >= (8 if skip_on else 1)
            assert want[0][EDGE_N.index(1)]["status"] == ref.CH_NONE  # one frame holds a first word, which ends in no final state
            if (amp, hi) != (2, 20000):  # the two long words are found: a charged start on either side of column 64
                seam = want[1][EDGE_N.index(129)]
                assert seam["slot"].tolist() == [1, 4, 5] and seam["start"].tolist() == [0, 2, 65]
            same(gram_call(eng, gram, fx["im"], fx["inf"], EDGE_WORDS, 0, skip), want, f"amplitude {amp}, costs to {hi}, skip {skip}")
            same(eng.decode_grammar(gram, fx["im"], fx["inf"], EDGE_WORDS, 0, skip), want, f"amplitude {amp}, costs to {hi}, skip {skip}, host form")
        gram.close()
    eng.close()


# ---- 10: an unreachable source state with a cost on its arc --------------------------------------------------------------------
@pytest.mark.gpu
def test_an_unreachable_source_state_takes_no_cost():
    """word 2 enters state 3 from state 1 at cost 7 and from state 2 at cost 0.  Where one of the two is unreachable and the
    other is not, all ones + 7 would wrap to 6 and win the minimum: the reference with its guard dropped (wrap=True) parses
    differently, so these rows do look at the case, and the library gives the guarded parse."""
    fx = chain_ref.planted()
    cost = [7 if arc == (1, 3, 2) else 0 for arc in JOIN_GRAM[1]]
    g = ref.with_costs(JOIN_GRAM, cost, None)
    eng = planted_engine(SPW2)
    gram = eng.grammar(*g)
    for skip in (None, SKIP):
        want = ref.decode(g, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, skip, 0, SPW2)
        wrapped = ref.decode(g, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, skip, 0, SPW2, wrap=True)
        assert np.any(want[2] != wrapped[2]) and np.any(want[0]["cost"] != wrapped[0]["cost"]), skip  # the guard decides
        same(gram_call(eng, gram, fx["im"], fx["inf"], W, 0, skip), want, f"guarded charge, skip {skip}")
    gram.close()
    eng.close()


# ---- 11: ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_are_judged_on_the_costs_with_arc_and_final_costs():
    rng = np.random.default_rng(931)
    M = 9
    t, u = (rng.integers(-3000, 3001, (M, 12)).astype(np.int16) for _ in range(2))
    tm = np.zeros((4, 2 * M + 1, 12), np.int16)
    tm[0, :M] = tm[1, :M] = t                # slots 0 and 1: identical twins
    tm[2, :M] = u
    tm[3, :2 * M] = np.concatenate([t, t])   # the word t said twice, as one template
    tf = np.array([M, M, M, 2 * M], np.uint32)
    im = np.zeros((2, MAXF, 12), np.int16)
    im[0, :2 * M] = np.concatenate([t, u])
    im[1, :3 * M] = np.concatenate([t, t, t])
    inf = np.array([2 * M, 3 * M], np.uint32)
    # t (either twin) leads to state 1, the second twin also to state 2.  u enters the final states 3 and 4 from 1 and from 2.
    # After state 1: t again (staying), t into 3, or the double word into 3.
    arcs = [(0, 1, 0), (0, 1, 1), (0, 2, 1), (1, 3, 2), (2, 3, 2), (1, 4, 2), (2, 4, 2), (1, 1, 0), (1, 3, 0), (1, 3, 3)]
    final = [0, 0, 0, 1, 1]

    def g(arc=(), fin=()):
        ac = {(0, 1, 0): 20, (0, 1, 1): 20, (0, 2, 1): 20, (1, 3, 2): 5, (2, 3, 2): 5, (1, 4, 2): 5, (2, 4, 2): 5, (1, 1, 0): 4, (1, 3, 0): 3, (1, 3, 3): 7}
        ac.update(dict(arc))
        fc = {3: 9, 4: 9}
        fc.update(dict(fin))
        return ref.with_costs((5, arcs, final), [ac[a] for a in arcs], [fc.get(s, 0) for s in range(5)])

    def parse(want, r):
        n = int(want[0][r]["n_words"])
        return [(int(w["slot"]), int(w["start"]), int(w["reserved"])) for w in want[1][r, :n]]

    cases = {}
    for name, gr in (("equal", g()), ("source", g(arc={(1, 3, 2): 6})), ("final", g(fin={3: 10})), ("words", g(arc={(1, 3, 3): 8}))):
        cases[name] = (gr, ref.decode(gr, im, inf, tm, tf, None, MAXF, 4, 0, None, 0))  # no skipping: the rows are words from end to end
    # E_1 + c is the same from states 1 and 2: the smaller source state, behind the smaller twin; E_2 + final cost is the same in 3 and 4: state 3
    assert parse(cases["equal"][1], 0) == [(0, 0, 1), (2, M, 3)] and int(cases["equal"][1][0][0]["cost"]) == 20 + 5 + 9
    # one unit on the arc from state 1 and the source is state 2, which only the second twin enters
    assert parse(cases["source"][1], 0) == [(1, 0, 2), (2, M, 3)] and int(cases["source"][1][0][0]["cost"]) == 20 + 5 + 9
    # one unit on final state 3 and the parse ends in state 4
    assert parse(cases["final"][1], 0) == [(0, 0, 1), (2, M, 4)] and int(cases["final"][1][0][0]["cost"]) == 20 + 5 + 9
    # "t t t": [t, tt] costs 20 + 7 + 9 and [t, t, t] 20 + 4 + 3 + 9, equal: the fewest words; a unit on the double word's arc: three
    assert parse(cases["equal"][1], 1) == [(0, 0, 1), (3, M, 3)] and cases["equal"][1][2][1].tolist()[1:3] == [36, 36]
    assert parse(cases["words"][1], 1) == [(0, 0, 1), (0, M, 1), (0, 2 * M, 3)] and cases["words"][1][2][1].tolist()[1:3] == [37, 36]
    # the last word's cum leaves the final cost out, the record's cost holds it
    assert int(cases["equal"][1][1][0, 1]["cum"]) == 25 and int(cases["equal"][1][1][0, 1]["acc"]) == 0
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(tm, tf)
    for name, (gr, want) in cases.items():
        gram = eng.grammar(*gr)
        same(gram_call(eng, gram, im, inf, 4, 0, None), want, f"ties: {name}")
        same(gram_call(eng, gram, im, inf, 4, 3, None), ref.decode(gr, im, inf, tm, tf, None, MAXF, 4, 3, None, 0), f"ties: {name}, three words")
        same(gram_call(eng, gram, im, inf, 4, 0, 0), ref.decode(gr, im, inf, tm, tf, None, MAXF, 4, 0, 0, 0), f"ties: {name}, filler free: every placement ties")
        gram.close()
    eng.close()


# ---- 12: the plan, seams and launch groups -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plan_counts_charge_lists_and_seams_and_groups_give_identical_bytes():
    fx = edge_fixture(2)
    g = ref.drawn_costs(EDGE_GRAM, hi=40)
    eng = edge_engine(fx, testing=True)
    gram, plain = eng.grammar(*g), eng.grammar(*EDGE_GRAM)
    p, q = gram.plan(EDGE_WORDS), plain.plan(EDGE_WORDS)
    lists, sets = ref.distinct_lists(g), ref.distinct_lists(ref.with_costs(EDGE_GRAM))
    assert p["from_sets"] == len(lists) == 10 and q["from_sets"] == len(sets) == 4  # the costs tell apart what the from-sets share
    per_level = [len(x) for x in gram_ref.items_per_level(EDGE_GRAM, EDGE_WORDS, range(len(EDGE_M)))]
    assert p["items_per_level"] == q["items_per_level"] == per_level and p["launches"] == q["launches"] == 2 + 3 * sum(n > 0 for n in per_level)
    S = EDGE_GRAM[0]
    assert p["row_bytes"] == (MAXF + 1) * (EDGE_WORDS * S * 8 + (EDGE_WORDS + 1) * S * 4 + len(lists) * 4)
    assert q["row_bytes"] == (MAXF + 1) * (EDGE_WORDS * S * 8 + (EDGE_WORDS + 1) * S * 4 + len(sets) * 4)
    # two arcs of one pair at one cost: one list; the shared from-set {1} of (2, 3) and (2, 4) stays shared at equal costs
    shared = eng.grammar(*ref.with_costs(EDGE_GRAM, [3] * len(EDGE_GRAM[1]), [0, 0, 5, 0]))
    assert shared.plan(EDGE_WORDS)["from_sets"] == 4 and shared.plan(EDGE_WORDS)["items_per_level"] == per_level
    want = edge_want(2, True, 40)
    first = as_bytes(gram_call(eng, gram, fx["im"], fx["inf"], EDGE_WORDS, 0, EDGE_SKIP[2]))
    for cols, rows in ((1, 0), (7, 0), (64, 0), (65, 0), (0, 1), (0, 3), (7, 3)):
        with hooks(cols, rows):
            if rows:
                assert gram.plan(EDGE_WORDS)["rows"] == rows
            got = gram_call(eng, gram, fx["im"], fx["inf"], EDGE_WORDS, 0, EDGE_SKIP[2])
        same(got, want, f"chunk {cols}, rows {rows}")
        assert as_bytes(got) == first, (cols, rows)
    for x in (gram, plain, shared):
        x.close()
    eng.close()


# ---- 13: buffer contracts ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_nothing_is_read_past_frames_and_every_record_is_written_whole(canary):
    fx = chain_ref.planted()
    g = costs_for("pairs", "drawn")
    want = ref.decode(g, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0)
    eng = planted_engine()
    gram = eng.grammar(*g)
    rec = poison_feature_rows(fx["im"].copy(), fx["inf"])
    same(gram_call(eng, gram, rec, fx["inf"], W, 0, SKIP, 0, canary), want, "poisoned rows")
    got = gram_call(eng, gram, rec, fx["inf"], W, 0, SKIP, 0, canary, want_lc=False)  # the optional output NULL: untouched
    assert got[2] is None
    same(got, want, "poisoned rows, no level costs")
    big = fx["inf"].copy()
    big[3], big[5] = 5000, 0  # a count above max_frames is clamped; an empty row gives the whole SR_CH_NONE record
    want_big = ref.decode(g, fx["im"], big, fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0)
    assert tuple(want_big[0][5]) == (DIS_ERR, 0, 0, ref.CH_NONE)
    same(gram_call(eng, gram, fx["im"], big, W, 0, SKIP, 0, canary), want_big, "a count above max_frames, an empty row")
    gram.close()
    eng.close()


# ---- 15: refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_create_nothing_and_write_nothing():
    fx = chain_ref.planted()
    n = 3
    im, inf = fx["im"][:n], fx["inf"][:n]
    eng = planted_engine()
    L = eng.L
    gram_t = (2, [(0, 1, 0), (1, 1, 2), (1, 0, 4)], [0, 1])
    top = 1 << 24
    ok = create_weighted(eng, gram_t, [top, 0, top], [0, top])  # the limits themselves are accepted
    assert create_weighted(eng, gram_t, [0, top + 1, 0], None, BAD_ARG) == BAD_ARG and b"cost above 2^24" in L.sr_last_error()
    assert create_weighted(eng, gram_t, None, [0, top + 1], BAD_ARG) == BAD_ARG and b"final cost above 2^24" in L.sr_last_error()
    assert create_weighted(eng, gram_t, None, [1, 0], BAD_ARG) == BAD_ARG and b"not final" in L.sr_last_error()
    assert create_weighted(eng, gram_t, [1, 2, 3], [0, 4], BAD_ARG, reserved=1) == BAD_ARG and b"reserved" in L.sr_last_error()
    assert create_weighted(eng, (2, gram_t[1] + [(1, 1, 2)], [0, 1]), [1, 2, 3, 2], None, BAD_ARG) == BAD_ARG and b"duplicate" in L.sr_last_error()
    assert create_weighted(eng, (2, gram_t[1], [0, 0]), [1, 2, 3], None, BAD_ARG) == BAD_ARG and b"final" in L.sr_last_error()
    with pytest.raises(Exception):
        eng.grammar(*gram_t, arc_cost=[0, 0, top + 1])
    g = ref.with_costs(gram_t, [top, 0, top], [0, top])
    want = ref.decode(g, im, inf, fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0)
    same(gram_call(eng, ok, im, inf, W, 0, SKIP), want, "before the refusals")
    d_im, d_inf = dev(im), dev(inf)
    sid = torch.cuda.current_stream().cuda_stream

    def refused(gr, why):
        for where in ("cuda:0", None):
            o = dict(rec=guarded_out((n,), ref.CHAIN_REC_DTYPE, 0xA5, 4096, where, "rec"), words=guarded_out((n, W), ref.CHAIN_WORD_DTYPE, 0xA5, 4096, where, "words"),
                     lc=guarded_out((n, W), np.uint32, 0xA5, 4096, where, "level_cost"))
            tail = (U32(1), U32(n), U32(W), U32(0), U32(SKIP), U32(0), P(o["rec"].ptr), P(o["words"].ptr), P(o["lc"].ptr))
            if where:
                assert L.sr_decode_grammar_dp_dev(eng.h, gr.g, P(d_im.data_ptr()), P(d_inf.data_ptr()), *tail, P(sid)) == BAD_ARG
                torch.cuda.synchronize()
            else:
                assert L.sr_decode_grammar_dp(eng.h, gr.g, engine._vp(im), engine._vp(inf), *tail) == BAD_ARG
            assert why in L.sr_last_error()
            for x in o.values():
                x.check_untouched()

    eng.set_word_map(None, 1)  # the same map, set again: the weighted grammar is older than the map
    refused(ok, b"word map")
    fresh = eng.grammar(*g)
    same(gram_call(eng, fresh, im, inf, W, 0, SKIP), want, "compiled again after the map")
    eng.set_templates_dense(fx["tm"], fx["tf"])  # the same store, set again
    refused(fresh, b"template store")
    again = eng.grammar(*g)
    same(gram_call(eng, again, im, inf, W, 0, SKIP), want, "compiled again after the store")
    for x in (ok, fresh, again):
        x.close()
    eng.close()
