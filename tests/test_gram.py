"""Grammar-constrained decoding: level building over a word network (include/sr_engine.h, "grammar-constrained decoding").

The definition lives in tests/gram_ref.py (numpy; its own checks are tests/test_gram_ref.py).  Every comparison here is byte
for byte against it -- records, word rows with the grammar state in `reserved`, level costs -- and, for the anchor grammar,
against the unconstrained decoder's own output.  No tolerances.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import chain_ref
import gram_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import DIS_ERR, VAD_DTYPE, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
FUNCS = ("sr_grammar_create", "sr_grammar_plan", "sr_decode_grammar_dp_dev", "sr_decode_grammar_dp", "sr_decode_grammar_batch")
BAD_CONFIG, BAD_ARG, NO_TEMPLATES = 2, 3, 4
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
MAXF, W, SKIP = 160, chain_ref.PLANT_MAX_WORDS, chain_ref.PLANT_SKIP
SPW2 = np.arange(chain_ref.PLANT_K, dtype=np.uint32) // 2  # two slots per word: labels 0, 0, 1, 1, 2


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


# ---- CPU: the surface (fails without the feature) ----------------------------------------------------------------------------
def test_header_declares_the_grammar_api_and_libraries_export_it():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert re.search(r"\bvoid sr_grammar_destroy\s*\(", src)
    assert all(hasattr(engine.load_library(t), "sr_grammar_destroy") for t in (False, True))
    # its own section: after live connected-word decoding, before the alignment section
    assert text.index("live connected-word decoding:") < text.index("grammar-constrained decoding:") < text.index("full-DP alignment and word models")
    assert src.index("sr_decode_live_end") < src.index("sr_grammar_create") < src.index("sr_decode_grammar_batch") < src.index("sr_dtw_dp_align_dev")
    assert re.search(r"typedef struct sr_gram_arc \{\s*uint32_t from;\s*uint32_t to;\s*uint32_t word;\s*uint32_t reserved;\s*\} sr_gram_arc;", src)
    assert re.search(r"typedef struct sr_grammar sr_grammar;", src)
    assert engine.GRAM_ARC_DTYPE.itemsize == 16 and engine.GRAM_ARC_DTYPE.names == ("from", "to", "word", "reserved")
    assert engine.CHAIN_WORD_DTYPE == ref.CHAIN_WORD_DTYPE  # the state after a word travels in `reserved`: no new record
    for meth in ("grammar", "decode_grammar", "decode_grammar_dev", "decode_grammar_pcm"):
        assert callable(getattr(Engine, meth, None)), meth
    for meth in ("plan", "close"):
        assert callable(getattr(engine.Grammar, meth, None)), meth
    section = text[text.index("grammar-constrained decoding:"):text.index("full-DP alignment and word models")]
    for out_of_scope in ("live", "arc weights", "epsilon", "more than 64 states"):
        assert out_of_scope in section[section.index("Out of scope"):], out_of_scope


def test_python_grammar_builders_are_the_reference_ones():
    pairs = [(a, b) for a in range(5) for b in range(5) if (a + b) % 2]
    for name, args, kw in (("grammar_any", ([3, 5, 3, 9],), {}), ("grammar_sequence", ([[1, 2], [2, 3], [7]],), {}),
                           ("grammar_sequence", ([[1, 2], [2, 3], [7]],), dict(optional_tail=True)),
                           ("grammar_word_pairs", (range(5), pairs), dict(first=[0, 2], last=[1, 4])),
                           ("grammar_word_pairs", ([4, 8], [(4, 8), (8, 8), (4, 8)]), {})):
        got, want = getattr(engine, name)(*args, **kw), getattr(ref, name)(*args, **kw)
        assert got == want, name
        ref.check(got)


# ---- GPU: fixtures -------------------------------------------------------------------------------------------------------------
def dev(a):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def gram_call(eng, gram, im, frames, max_words, n_words=0, skip=None, word_cost=0, canary=0xA5, want_lc=True, chain=False):
    """sr_decode_grammar_dp_dev (chain: sr_decode_words_dp_dev) into guarded buffers whose every byte starts as the canary"""
    n = len(im)
    d_im, d_frames = dev(im), dev(np.ascontiguousarray(frames, dtype=np.uint32))
    g_r = guarded_out((n,), ref.CHAIN_REC_DTYPE, canary, 4096, "cuda:0", "rec")
    g_w = guarded_out((n, max_words), ref.CHAIN_WORD_DTYPE, canary, 4096, "cuda:0", "words")
    g_l = guarded_out((n, max_words), np.uint32, canary, 4096, "cuda:0", "level_cost")
    sid = torch.cuda.current_stream().cuda_stream
    tail = (P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(1), U32(n), U32(max_words), U32(n_words), U32(skip_arg(skip)), U32(word_cost),
            P(g_r.ptr), P(g_w.ptr), P(g_l.ptr) if want_lc else None, P(sid))
    rc = eng.L.sr_decode_words_dp_dev(eng.h, *tail) if chain else eng.L.sr_decode_grammar_dp_dev(eng.h, gram.g, *tail)
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_r.check()
    g_w.check()
    g_l.check() if want_lc else g_l.check_untouched()
    return g_r.interior(), g_w.interior(), g_l.interior() if want_lc else None


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


EDGE_M = (1, 2, 3, 14, 63, 64, 65)
EDGE_N = sorted({0, 1, 63, 64, 65, 128, 129, MAXF} | {m // 2 for m in EDGE_M} | {m // 2 + 1 for m in EDGE_M})
EDGE_WORDS = 3
EDGE_SKIP = {2: 7, 3000: 8000}  # about what a frame costs inside a word: both choices occur
# over the edge store: a short word, then any word, then optionally a long one; the word of slot 3 enters state 2 from 1 and from 0
EDGE_GRAM = (4, [(0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 2, 3), (1, 2, 3), (1, 2, 4), (1, 2, 0), (2, 3, 5), (2, 3, 6), (2, 3, 4), (2, 2, 1)], [0, 0, 1, 1])


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
    im[r, 2:65], im[r, 65:129] = tm[4, :63], tm[5, :64]  # two long words back to back, across a sweep seam
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf)


@functools.lru_cache(maxsize=None)
def edge_want(amp, skip_on, which):
    fx = edge_fixture(amp)
    gram = ref.grammar_any(range(len(EDGE_M))) if which == "anchor" else EDGE_GRAM
    want = ref.decode(gram, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, EDGE_WORDS, 0, EDGE_SKIP[amp] if skip_on else None, 0)
    for a in want:
        a.setflags(write=False)
    return want


def edge_engine(fx, **kw):
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


def planted_engine(word_of_slot=None, **kw):
    fx = chain_ref.planted()
    assert chain_ref.PLANT_MAXF == MAXF
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    if word_of_slot is not None:
        eng.set_word_map(word_of_slot)
    return eng


SEQ_GRAM = ref.grammar_sequence([[0, 1, 2], [2, 3, 4], [0, 4], [1, 3]], optional_tail=True)
PAIR_GRAM = ref.grammar_word_pairs(range(5), [(a, b) for a in range(5) for b in range(5) if (a + b) % 2 == 1], first=[0, 1, 2, 4])
# two slots per word (labels 0, 0, 1, 1, 2): word 2 enters state 3 from state 1 and from state 2
JOIN_GRAM = (4, [(0, 1, 0), (0, 2, 1), (1, 3, 2), (2, 3, 2), (3, 1, 0), (1, 1, 1), (3, 2, 1)], [0, 1, 0, 1])


@functools.lru_cache(maxsize=None)
def planted_want(which, n_exact=0, skip=SKIP, word_cost=0):
    fx = chain_ref.planted()
    gram, wos = dict(seq=(SEQ_GRAM, None), pairs=(PAIR_GRAM, None), join=(JOIN_GRAM, SPW2), anchor=(ref.grammar_any(range(5)), None))[which]
    want = ref.decode(gram, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, n_exact, skip, word_cost, wos)
    for a in want:
        a.setflags(write=False)
    return want


# ---- GPU 1: the anchor ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("amp", [2, 3000])
def test_anchor_grammar_equals_the_unconstrained_decoder(amp):
    fx = edge_fixture(amp)
    eng = edge_engine(fx)
    gram = eng.grammar(*engine.grammar_any(range(len(EDGE_M))))
    assert gram.plan(EDGE_WORDS)["items_per_level"] == [len(EDGE_M)] * EDGE_WORDS and gram.plan(EDGE_WORDS)["from_sets"] == 1
    for skip_on in (True, False):
        skip = EDGE_SKIP[amp] if skip_on else None
        want = edge_want(amp, skip_on, "anchor")
        free = chain_ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, EDGE_WORDS, 0, skip, 0)
        same(want, free, "the reference's anchor against the decoder's reference")
        assert (want[0]["status"] == ref.CH_OK).sum() >= 10 and tuple(want[0][0]) == (DIS_ERR, 0, 0, ref.CH_NONE)
        got = gram_call(eng, gram, fx["im"], fx["inf"], EDGE_WORDS, 0, skip)
        same(got, want, f"device form, skip {skip}")
        same(eng.decode_grammar(gram, fx["im"], fx["inf"], EDGE_WORDS, 0, skip), want, f"host form, skip {skip}")
        assert as_bytes(got) == as_bytes(gram_call(eng, None, fx["im"], fx["inf"], EDGE_WORDS, 0, skip, chain=True))  # sr_decode_words_dp_dev
        assert as_bytes(got) == as_bytes(eng.decode_words(fx["im"], fx["inf"], EDGE_WORDS, 0, skip))                 # sr_decode_words_dp
        # a grammar that bites, on the same length edges
        want_g = edge_want(amp, skip_on, "edge")
        g2 = eng.grammar(*EDGE_GRAM)
        same(gram_call(eng, g2, fx["im"], fx["inf"], EDGE_WORDS, 0, skip), want_g, f"edge grammar, skip {skip}")
        g2.close()
    gram.close()
    eng.close()


# ---- GPU 2: grammars that bite -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seq", "pairs", "join"])
def test_grammars_that_bite_on_the_planted_rows(which):
    fx = chain_ref.planted()
    gram_t, wos = dict(seq=(SEQ_GRAM, None), pairs=(PAIR_GRAM, None), join=(JOIN_GRAM, SPW2))[which]
    want = planted_want(which)
    free = chain_ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0, wos)
    differ = sum(any(want[1][r][f].tolist() != free[1][r][f].tolist() for f in ("slot", "start", "end")) for r in range(len(fx["inf"])))
    assert differ >= 4 and (want[0]["status"] == ref.CH_OK).sum() >= 8, (which, differ)  # the constraint changes the parse
    for r in range(len(fx["inf"])):
        n = int(want[0][r]["n_words"])
        assert n == 0 or ref.accepts(gram_t, [(int(w["word"]), int(w["reserved"])) for w in want[1][r, :n]])
    eng = planted_engine(wos)
    gram = eng.grammar(*gram_t)
    same(gram_call(eng, gram, fx["im"], fx["inf"], W, 0, SKIP), want, which)
    same(eng.decode_grammar(gram, fx["im"], fx["inf"], W, 0, SKIP), want, which + ", host form")
    for n_exact, skip, wc in ((2, SKIP, 0), (0, None, 5000), (3, SKIP, 1 << 24)):
        same(gram_call(eng, gram, fx["im"], fx["inf"], W, n_exact, skip, wc), planted_want(which, n_exact, skip, wc), f"{which}: n {n_exact}, skip {skip}, word_cost {wc}")
    gram.close()
    eng.close()


# ---- GPU 3: ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_go_to_start_slot_fewest_words_smallest_final_and_smallest_source_state():
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
    # t (either twin) leads to state 1, the second twin also to state 2: E_1 is the same in both.  u enters the final states 3
    # and 4 from 1 and from 2.  After state 1: t again (staying), t into 3, or the double word into 3.
    gram_t = (5, [(0, 1, 0), (0, 1, 1), (0, 2, 1), (1, 3, 2), (2, 3, 2), (1, 4, 2), (2, 4, 2), (1, 1, 0), (1, 3, 0), (1, 3, 3)], [0, 0, 0, 1, 1])
    want = ref.decode(gram_t, im, inf, tm, tf, None, MAXF, 4, 0, 0, 0)  # skip_cost 0: filler is free, every placement ties
    rec, words, lc = want
    INF = DIS_ERR
    # row 0, "t u": cost 0 in two words; the first word is the smaller twin (slot 0) into state 1; u ends in the smaller final
    # state 3, and of its two source states with E_1 = 0 the smaller, 1, is taken
    assert tuple(rec[0]) == (0, 2, 0, ref.CH_OK) and lc[0].tolist()[:2] == [INF, 0]
    assert [tuple(w)[1:4] + (int(w["reserved"]),) for w in words[0, :2]] == [(0, 0, M - 1, 1), (2, M, 2 * M - 1, 3)]
    # row 1, "t t t": [t, tt] and [t, t, t] both cost 0: the fewest words; the last word is the double one from frame M and not
    # the single one from 2M (the smallest start), both of cost 0 because filler is free
    assert tuple(rec[1]) == (0, 2, 0, ref.CH_OK) and lc[1].tolist()[:3] == [INF, 0, 0]
    assert [tuple(w)[1:4] + (int(w["reserved"]),) for w in words[1, :2]] == [(0, 0, M - 1, 1), (3, M, 3 * M - 1, 3)]
    want3 = ref.decode(gram_t, im, inf, tm, tf, None, MAXF, 4, 3, 0, 0)  # three words asked for: every one the smaller twin
    assert want3[1][1, :3]["slot"].tolist() == [0, 0, 0] and want3[1][1, :3]["reserved"].tolist() == [1, 1, 3] and want3[0][1]["cost"] == 0
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(tm, tf)
    gram = eng.grammar(*gram_t)
    same(gram_call(eng, gram, im, inf, 4, 0, 0), want, "ties")
    same(gram_call(eng, gram, im, inf, 4, 3, 0), want3, "ties, three words")
    gram.close()
    eng.close()


# ---- GPU 4: chunk seams and launch groups ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seams_and_groups_give_identical_bytes():
    fx, want = edge_fixture(2), edge_want(2, True, "edge")
    eng = edge_engine(fx, testing=True)
    gram = eng.grammar(*EDGE_GRAM)
    first = as_bytes(gram_call(eng, gram, fx["im"], fx["inf"], EDGE_WORDS, 0, EDGE_SKIP[2]))
    for cols, rows in ((1, 0), (7, 0), (64, 0), (65, 0), (0, 1), (0, 3), (7, 3)):
        with hooks(cols, rows):
            if rows:
                assert gram.plan(EDGE_WORDS)["rows"] == rows
            got = gram_call(eng, gram, fx["im"], fx["inf"], EDGE_WORDS, 0, EDGE_SKIP[2])
        same(got, want, f"chunk {cols}, rows {rows}")
        assert as_bytes(got) == first, (cols, rows)
    gram.close()
    eng.close()


# ---- GPU 5: the plan and the pruning -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plan_geometry_and_exact_pruning():
    fx = chain_ref.planted()
    eng = planted_engine()
    pos = [[0, 1, 2], [2, 3, 4], [0, 4]]
    seq = eng.grammar(*engine.grammar_sequence(pos))
    p = seq.plan(W)
    assert p["items_per_level"] == [3, 3, 2, 0, 0]  # position l's slots at level l, nothing beyond
    assert p["items_per_level"] == [len(x) for x in ref.items_per_level(ref.grammar_sequence(pos), W, range(5))]
    assert p["from_sets"] == 3 and p["launches"] == 2 + 3 * 3
    assert p["row_bytes"] == (MAXF + 1) * (W * 4 * 8 + (W + 1) * 4 * 4 + 3 * 4) and p["rows"] == min(65535, (256 << 20) // p["row_bytes"])
    assert seq.plan(3)["items_per_level"] == [3, 3, 2] and seq.plan(2)["items_per_level"] == [0, 0] and seq.plan(2)["launches"] == 2
    tail = eng.grammar(*engine.grammar_sequence(pos, optional_tail=True))
    assert tail.plan(2)["items_per_level"] == [3, 3]
    anchor = eng.grammar(*engine.grammar_any(range(5)))
    assert anchor.plan(W)["items_per_level"] == [5] * W and anchor.plan(W)["launches"] == 2 + 3 * W
    assert anchor.plan(W)["row_bytes"] == engine.decode_geometry(14, MAXF, W)["scratch_bytes"] + (MAXF + 1) * 4  # the decoder's, plus one charge row
    far = eng.grammar(3, [(0, 1, 0), (1, 0, 1)], [0, 0, 1])  # the final state is out of reach
    assert far.plan(W)["items_per_level"] == [0] * W and far.plan(W)["launches"] == 2
    out = (U32 * 4)()
    for g, mw, o in ((None, 4, out), (seq.g, 0, out), (seq.g, 17, out), (seq.g, 4, None)):
        assert eng.L.sr_grammar_plan(g, U32(mw), None, o) == BAD_ARG
    # a dead branch changes no byte: a state nothing leaves, and a state nothing reaches
    g_t = ref.grammar_sequence(pos, optional_tail=True)
    dead_t = (g_t[0] + 2, g_t[1] + [(1, 4, 0), (1, 4, 3), (5, 2, 1), (5, 5, 2)], g_t[2] + [0, 1])
    dead = eng.grammar(*dead_t)
    assert dead.plan(W)["items_per_level"] == tail.plan(W)["items_per_level"]
    want = ref.decode(g_t, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0)
    same(ref.decode(dead_t, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0), want, "the reference with the dead branch")
    same(gram_call(eng, tail, fx["im"], fx["inf"], W, 0, SKIP), want, "without the dead branch")
    same(gram_call(eng, dead, fx["im"], fx["inf"], W, 0, SKIP), want, "with the dead branch")
    for g in (seq, tail, anchor, far, dead):
        g.close()
    eng.close()


# ---- GPU 6: no parse -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_parse_gives_whole_none_records():
    fx = chain_ref.planted()
    im, inf = fx["im"][:6], fx["inf"][:6].copy()
    inf[1] = 0  # an empty row
    eng = planted_engine()
    none_rec, none_word = (DIS_ERR, 0, 0, ref.CH_NONE), (DIS_ERR,) * 8
    seq_t = ref.grammar_sequence([[0, 1, 2], [2, 3, 4], [0, 4]])
    far_t = (3, [(0, 1, 0), (1, 0, 1)], [0, 0, 1])
    for what, gram_t, mw, n_exact in (("finals beyond max_words", seq_t, 2, 0), ("finals out of reach", far_t, 4, 0),
                                      ("no accepted sequence of that length", seq_t, 4, 2), ("an empty row among others", seq_t, 4, 0)):
        want = ref.decode(gram_t, im, inf, fx["tm"], fx["tf"], None, MAXF, mw, n_exact, SKIP, 0)
        if what == "an empty row among others":
            assert tuple(want[0][1]) == none_rec and (want[0]["status"] == ref.CH_OK).sum() >= 3
        else:
            assert all(tuple(r) == none_rec for r in want[0]) and all(tuple(w) == none_word for w in want[1].ravel())
            # no level has a parse -- or, with the count given, that level has none although level 3 has
            assert np.all(want[2][:, n_exact - 1] == DIS_ERR) and np.any(want[2][:, 2] != DIS_ERR) if n_exact else np.all(want[2] == DIS_ERR)
        gram = eng.grammar(*gram_t)
        for canary in CANARIES:
            same(gram_call(eng, gram, im, inf, mw, n_exact, SKIP, 0, canary), want, what)
        gram.close()
    eng.close()


# ---- GPU 7: buffer contracts -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_nothing_is_read_past_frames_and_every_record_is_written_whole(canary):
    fx, want = chain_ref.planted(), planted_want("pairs")
    eng = planted_engine()
    gram = eng.grammar(*PAIR_GRAM)
    rec = poison_feature_rows(fx["im"].copy(), fx["inf"])
    same(gram_call(eng, gram, rec, fx["inf"], W, 0, SKIP, 0, canary), want, "poisoned rows")
    got = gram_call(eng, gram, rec, fx["inf"], W, 0, SKIP, 0, canary, want_lc=False)  # the optional output NULL: untouched
    assert got[2] is None
    same(got, want, "poisoned rows, no level costs")
    big = fx["inf"].copy()
    big[3] = 5000  # a count above max_frames is clamped
    want_big = ref.decode(PAIR_GRAM, fx["im"], big, fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0)
    same(gram_call(eng, gram, fx["im"], big, W, 0, SKIP, 0, canary), want_big, "a count above max_frames")
    gram.close()
    eng.close()


# ---- GPU 8: the forms agree, runs repeat, and the engine's scratch is ordered between streams ------------------------------------
@pytest.mark.gpu
def test_host_device_and_pcm_forms_agree_and_runs_repeat():
    T, B, maxf = 64, 6, 96
    bank = synth.word_bank(6)
    eng = Engine(max_frames=maxf, device=0)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(B) % 6, [T, 70, 50, T, 80, T], seed=61, bank=bank, S=(synth.buf_len_for(90) + 7) // 8 * 8))
    vd = eng.vad(pcm)
    assert np.all(vd["status"] == 0)
    start, end, mid = vd["seg"][:, 0].copy(), vd["seg"][:, 1].copy(), vd["mid_val"].copy()
    start[2] = 0  # a failed record: SR_ST_SEG_OOB
    n, mf, st = eng.mfcc_status(pcm, start, end, mid)
    assert st[2] != 0 and n[2] == 0 and np.all(n[[0, 1, 3, 4, 5]] > 40)
    tm = np.zeros((4, 31, 12), np.int16)  # templates: pieces of the rows themselves
    tf = np.array([20, 30, 12, 25], np.uint32)
    for k, (r, at) in enumerate(((0, 10), (1, 30), (3, 5), (4, 40))):
        tm[k, :tf[k]] = mf[r, at:at + tf[k]]
    eng.set_templates_dense(tm, tf)
    skip = int(np.median(ref.local_dis(mf[0, :n[0]], tm[1, :30])))  # a typical frame distance
    gram_t = ref.grammar_word_pairs(range(4), [(a, b) for a in range(4) for b in range(4) if a != b], last=[0, 1, 3])
    want = ref.decode(gram_t, mf, n, tm, tf, None, maxf, 4, 0, skip, 100)
    assert want[0][2]["status"] == ref.CH_NONE and (want[0]["status"] == ref.CH_OK).sum() == 5
    gram = eng.grammar(*gram_t)
    host = eng.decode_grammar(gram, mf, n, 4, 0, skip, 100)
    same(host, want, "host form")
    d1 = gram_call(eng, gram, mf, n, 4, 0, skip, 100)
    d2 = gram_call(eng, gram, mf, n, 4, 0, skip, 100, 0x3C)
    assert as_bytes(d1) == as_bytes(d2) == as_bytes(host)
    o = eng.decode_grammar_pcm(gram, pcm, start, end, mid, 4, 0, skip, 100)
    assert as_bytes((o["rec"], o["words"], o["level_cost"])) == as_bytes(host)
    assert o["mfcc"].tobytes() == mf.tobytes() and np.array_equal(o["frm_num"], n) and np.array_equal(o["status"], st)
    # the Python device form, counts taken from vad-shaped records
    recs = np.zeros(B, VAD_DTYPE)
    recs["frm_num"] = n
    d_vad, d_mf = torch.from_numpy(recs.view(np.int32).reshape(B, 12)).cuda(), torch.from_numpy(mf).cuda()
    d_rec = torch.empty(B, 4, dtype=torch.int32, device="cuda:0")
    d_words = torch.empty(B, 4, 8, dtype=torch.int32, device="cuda:0")
    d_lc = torch.empty(B, 4, dtype=torch.int32, device="cuda:0")
    eng.decode_grammar_dev(gram, d_mf, d_vad[:, 9], d_rec, d_words, d_lc, 4, 0, skip, 100, 12)
    torch.cuda.synchronize()
    assert as_bytes((d_rec.cpu().numpy(), d_words.cpu().numpy(), d_lc.cpu().numpy())) == as_bytes(host)
    gram.close()
    eng.close()


@pytest.mark.gpu
def test_scratch_order_with_the_spotter_on_another_stream():
    fx, want = chain_ref.planted(), planted_want("pairs")
    eng = planted_engine(testing=True)
    gram = eng.grammar(*PAIR_GRAM)
    n, K = len(fx["inf"]), len(fx["tf"])
    d_im, d_inf = dev(fx["im"]), dev(fx["inf"])
    s_spot, s_dec = torch.cuda.Stream(), torch.cuda.Stream()
    hits = torch.empty(n, 1, K, 4, dtype=torch.int32, device="cuda:0")
    outs = []
    torch.cuda.synchronize()
    engine.dev_hook("spot_chunk_cols", 64)  # the split form: the spotter's partial records live in the engine's scratch
    engine.dev_hook("chain_rows", 5)        # several launch groups reuse the decoder's scratch
    try:
        for _ in range(2):
            eng.spot_dev(d_im, d_inf, hits, None, 0, 1, s_spot.cuda_stream)
            o = (torch.empty(n, 4, dtype=torch.int32, device="cuda:0"), torch.empty(n, W, 8, dtype=torch.int32, device="cuda:0"),
                 torch.empty(n, W, dtype=torch.int32, device="cuda:0"))
            eng.decode_grammar_dev(gram, d_im, d_inf, *o, W, 0, SKIP, 0, 1, s_dec.cuda_stream)
            outs.append(o)
            eng.spot_dev(d_im, d_inf, hits, None, 0, 1, s_spot.cuda_stream)
        torch.cuda.synchronize()
        spot_alone = torch.empty_like(hits)
        eng.spot_dev(d_im, d_inf, spot_alone)
        torch.cuda.synchronize()
    finally:
        for h in ("spot_chunk_cols", "chain_rows"):
            engine.dev_hook(h, 0)
    for i, o in enumerate(outs):
        same([t.cpu().numpy() for t in o], want, f"interleaved call {i}")
    assert torch.equal(hits, spot_alone)  # and the spotter's records are what it writes on its own
    gram.close()
    eng.close()


# ---- GPU 9: refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing():
    fx = chain_ref.planted()
    n = 3
    im, inf = fx["im"][:n], fx["inf"][:n]
    eng, other = planted_engine(), planted_engine()
    L, v = eng.L, engine._vp
    ok_arcs = np.array([(0, 1, 0, 0), (1, 1, 2, 0), (1, 0, 4, 0)], engine.GRAM_ARC_DTYPE)
    fin = np.array([0, 1], np.uint8)

    def create(e, n_states, arcs, final, out=True):
        g = P(0x5A5A5A5A)  # stays as it is when the call is refused
        rc = L.sr_grammar_create(e.h, U32(n_states), v(arcs) if arcs is not None else None, U32(0 if arcs is None else len(arcs)),
                                 v(final) if final is not None else None, C.byref(g) if out else None)
        assert rc != 0 and g.value == 0x5A5A5A5A, L.sr_last_error()
        return rc

    def arcs_with(i, **kw):
        a = ok_arcs.copy()
        for k, x in kw.items():
            a[i][k] = x
        return a

    assert create(eng, 2, None, fin) == BAD_ARG and create(eng, 2, ok_arcs, None) == BAD_ARG and create(eng, 2, ok_arcs, fin, out=False) == BAD_ARG
    assert L.sr_grammar_create(None, U32(2), v(ok_arcs), U32(3), v(fin), C.byref(P())) == BAD_ARG
    assert create(eng, 0, ok_arcs, np.zeros(0, np.uint8)) == BAD_ARG and create(eng, 65, ok_arcs, np.ones(65, np.uint8)) == BAD_ARG
    assert create(eng, 2, ok_arcs[:0], fin) == BAD_ARG
    assert create(eng, 2, np.zeros(4097, engine.GRAM_ARC_DTYPE), fin) == BAD_ARG and b"n_arcs" in L.sr_last_error()
    assert create(eng, 2, arcs_with(1, to=2), fin) == BAD_ARG and create(eng, 2, arcs_with(2, **{"from": 2}), fin) == BAD_ARG
    assert create(eng, 2, np.concatenate([ok_arcs, ok_arcs[1:2]]), fin) == BAD_ARG and b"duplicate" in L.sr_last_error()
    assert create(eng, 2, arcs_with(0, reserved=1), fin) == BAD_ARG
    assert create(eng, 2, arcs_with(0, word=5), fin) == BAD_ARG and b"no label" in L.sr_last_error()
    assert create(eng, 2, ok_arcs, np.zeros(2, np.uint8)) == BAD_ARG and b"final" in L.sr_last_error()
    e2 = Engine(max_frames=MAXF, device=0)  # no templates
    assert create(e2, 2, ok_arcs, fin) == NO_TEMPLATES
    e3 = Engine(max_frames=MAXF, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    assert create(e3, 2, ok_arcs, fin) == BAD_CONFIG
    # the limits themselves are accepted: 64 states, 4096 arcs
    big = np.array([(s, t, 0, 0) for s in range(64) for t in range(64)], engine.GRAM_ARC_DTYPE)
    g_big = eng.grammar(64, [tuple(a)[:3] for a in big], [1] * 64)
    want_big = chain_ref.decode(im, inf, fx["tm"][:1], fx["tf"][:1], None, MAXF, 2, 0, SKIP, 0)  # every state alike: the decoder over slot 0
    got_big = gram_call(eng, g_big, im, inf, 2, 0, SKIP)
    same((got_big[0], None, got_big[2]), (want_big[0], None, want_big[2]), "64 states, 4096 arcs")
    g_big.close()

    gram, g_other = eng.grammar(2, [tuple(a)[:3] for a in ok_arcs], fin), other.grammar(2, [tuple(a)[:3] for a in ok_arcs], fin)
    gram_t = (2, [tuple(int(x) for x in tuple(a)[:3]) for a in ok_arcs], [0, 1])
    want = ref.decode(gram_t, im, inf, fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0)
    same(gram_call(eng, gram, im, inf, W, 0, SKIP), want, "before the refusals")
    d_im, d_inf = dev(im), dev(inf)
    bank = synth.word_bank(2)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 2, [40] * n, seed=5, bank=bank, S=synth.buf_len_for(60)))
    seg, mid = np.array([[4000, 9000]] * n, np.int32), np.full(n, 2048, np.uint32)
    sid = torch.cuda.current_stream().cuda_stream

    def refused(e, g, code, stride=1, max_words=W, n_words=0, skip=SKIP, wc=0, null=None, overlap=None, whole=True):
        for where in ("cuda:0", None):
            o = dict(rec=guarded_out((n,), ref.CHAIN_REC_DTYPE, 0xA5, 4096, where, "rec"),
                     words=guarded_out((n, 16), ref.CHAIN_WORD_DTYPE, 0xA5, 4096, where, "words"),
                     lc=guarded_out((n, 16), np.uint32, 0xA5, 4096, where, "level_cost"))
            a = dict(mfcc=P(d_im.data_ptr()) if where else v(im), frames=P(d_inf.data_ptr()) if where else v(inf),
                     rec=P(o["rec"].ptr), words=P(o["words"].ptr), lc=P(o["lc"].ptr))
            if null:
                a[null] = None
            if overlap:
                a[overlap[0]] = P(o[overlap[1]].ptr + overlap[2])
            args = (U32(max_words), U32(n_words), U32(skip), U32(wc), a["rec"], a["words"], a["lc"])
            if where:
                assert L.sr_decode_grammar_dp_dev(e.h, g, a["mfcc"], a["frames"], U32(stride), U32(n), *args, P(sid)) == code
                torch.cuda.synchronize()
            else:
                assert L.sr_decode_grammar_dp(e.h, g, a["mfcc"], a["frames"], U32(stride), U32(n), *args) == code
                if whole and null not in ("mfcc", "frames") and not overlap:
                    S = pcm.shape[1]
                    assert L.sr_decode_grammar_batch(e.h, g, v(pcm), U64(S), U32(S), U32(n), v(seg[:, 0].copy()), v(seg[:, 1].copy()), v(mid),
                                                     *args, None, None, None) == code
            for x in o.values():
                x.check_untouched()

    for null in ("mfcc", "frames", "rec", "words"):
        refused(eng, gram.g, BAD_ARG, null=null)
    refused(eng, None, BAD_ARG)  # a null grammar
    assert b"null grammar" in L.sr_last_error()
    refused(eng, g_other.g, BAD_ARG)  # a grammar of another engine
    assert b"another engine" in L.sr_last_error()
    refused(eng, gram.g, BAD_ARG, stride=0, whole=False)
    refused(eng, gram.g, BAD_ARG, max_words=0)
    refused(eng, gram.g, BAD_ARG, max_words=17)
    refused(eng, gram.g, BAD_ARG, n_words=W + 1)
    refused(eng, gram.g, BAD_ARG, skip=65536)
    refused(eng, gram.g, BAD_ARG, wc=(1 << 24) + 1)
    refused(eng, gram.g, BAD_ARG, overlap=("words", "rec", 16))
    refused(eng, gram.g, BAD_ARG, overlap=("lc", "words", 64))
    refused(e2, gram.g, NO_TEMPLATES)   # the decoder's own refusals come with their codes
    refused(e3, gram.g, BAD_CONFIG)
    same(gram_call(eng, gram, im, inf, W, 0, SKIP), want, "after the refusals")
    eng.set_word_map(None, 1)  # the same map, set again: the grammar is older than the map
    refused(eng, gram.g, BAD_ARG)
    assert b"word map" in L.sr_last_error()
    fresh = eng.grammar(*gram_t)
    same(gram_call(eng, fresh, im, inf, W, 0, SKIP), want, "compiled again after the map")
    eng.set_templates_dense(fx["tm"], fx["tf"])  # the same store, set again
    refused(eng, fresh.g, BAD_ARG)
    assert b"template store" in L.sr_last_error()
    again = eng.grammar(*gram_t)
    same(gram_call(eng, again, im, inf, W, 0, SKIP), want, "compiled again after the store")
    for g in (gram, g_other, fresh, again):
        g.close()
    for e in (eng, other, e2, e3):
        e.close()
