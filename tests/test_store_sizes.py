"""The decoders, the aligner, the spotter and the four live sessions on stores of real size (tests/store_cases.py): the longest
template the LDS image takes, 65 536 slots of which ten are valid, and 300 valid slots in word groups of up to 65.  Every other
decoder test runs on stores of at most about ten slots of at most 65 rows; only the spotter and the span scorer were ever run
at max_tpl_rows, and no test decoded a slot above about 10, so a kernel missing from its allow list for more than 64 KiB of
LDS, a 15-bit slot field or a word group past 65 535 slots would have passed the suite.

Every comparison is byte for byte against the restatements the per-feature tests use (chain_ref, gram_ref, wgram_ref,
onepass_ref, onepass_gram_ref, forced_ref, span_ref, spot_ref, spot_live_ref); a live session is compared, after its last push
and after its end call, with the batch reference of the whole recording.  No tolerances.  The stage calls write into guarded
buffers (the per-feature tests' helpers), once with each canary.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_ref
import forced_ref
import gram_ref
import onepass_gram_ref
import onepass_ref
import span_ref
import spot_live_ref
import spot_ref
import store_cases as sc
import test_chain as t_chain
import test_forced as t_forced
import test_gram as t_gram
import test_onepass as t_onepass
import test_onepass_gram as t_opgram
import test_span as t_span
import test_spot as t_spot
import test_spot_live as t_spot_live
import wgram_ref
from guarded import CANARIES, guarded_out
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine, SrError

BAD_ARG = 3
U32, P = C.c_uint32, C.c_void_p
CAP = engine.decode_geometry(30, 1000, 3)["max_tpl_rows"]  # host only: the longest template of every LDS-staged kernel
OP_WORDS = 8  # words_cap of the one-pass calls: some rows hold more (SR_CH_TRUNCATED), most fewer
FIXTURES = ("longest", "sparse", "dense")


def fixture(name):
    if name.startswith("longest"):
        fx = sc.longest(CAP)
        return sc.without_short_slot(fx) if name.endswith("two") else fx
    return dict(sparse=sc.sparse, dense=sc.dense)[name]()


def store(fx):
    return fx["tm"], fx["tf"], fx["valid"]


def frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


def slots_of(want, r):
    return [int(k) for k in want[1][r, :min(int(want[0][r]["n_words"]), want[1].shape[1])]["slot"]]


def as_bytes(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out if a is not None)


# ---- the references, each computed once ------------------------------------------------------------------------------------------
OFF_ROWS = dict(longest=(2, 3), sparse=(0, 1, 2, 3, 4), dense=(1, 4))  # the rows decoded without skipping as well: the reference is slow


def chain_want(name, skip_on=True, max_words=None):
    return _chain_want(name, skip_on, max_words)  # (one cache entry per reference, whatever the call spells out)


@functools.lru_cache(maxsize=None)
def _chain_want(name, skip_on, max_words):
    """skip_on False: skipping off, over OFF_ROWS[name] alone"""
    fx = fixture(name)
    rows = list(range(len(fx["inf"]))) if skip_on else list(OFF_ROWS[name])
    return frozen(chain_ref.decode(fx["im"][rows], fx["inf"][rows], *store(fx), fx["maxf"], max_words or fx["max_words"], 0,
                                   fx["skip"] if skip_on else None, 0, fx["wos"]))


def gram_want(name, which, max_words=None):
    return _gram_want(name, which, max_words)  # (one cache entry per reference, whatever the call spells out)


@functools.lru_cache(maxsize=None)
def _gram_want(name, which, max_words):
    fx = fixture(name)
    gram = gram_ref.grammar_any(fx["labels"]) if which == "anchor" else fx["grams"][which]
    return frozen(gram_ref.decode(gram, fx["im"], fx["inf"], *store(fx), fx["maxf"], max_words or fx["max_words"], 0, fx["skip"], 0, fx["wos"]))


def wgram_want(name, which, max_words=None):
    return _wgram_want(name, which, max_words)  # (one cache entry per reference, whatever the call spells out)


@functools.lru_cache(maxsize=None)
def _wgram_want(name, which, max_words):
    fx = fixture(name)
    return frozen(wgram_ref.decode(fx["wgrams"][which], fx["im"], fx["inf"], *store(fx), fx["maxf"], max_words or fx["max_words"], 0, fx["skip"], 0,
                                   fx["wos"]))


def op_rows(name):
    """the rows of the one-pass calls: the restatement is plain Python, a cell at a time, so the two-slot store takes rows (d)
    and (e) and the grammars on the cap-row store rows (a), (d) and (e); the templates stay as they are"""
    return dict(longest=[0, 1, 2, 3, 4], longest_gram=[0, 3, 4], longest_two=[3, 4]).get(name)


def onepass_want(name, rows=None):
    return _onepass_want(name, rows)  # (one cache entry per reference, whatever the call spells out)


@functools.lru_cache(maxsize=None)
def _onepass_want(name, rows):
    fx = fixture(name)
    rows = list(range(len(fx["inf"]))) if rows is None else list(rows)
    return frozen(onepass_ref.decode(fx["im"][rows], fx["inf"][rows], *store(fx), fx["maxf"], OP_WORDS, fx["skip"], 0, fx["wos"]))


def opgram_want(name, which, rows=None):
    return _opgram_want(name, which, rows)  # (one cache entry per reference, whatever the call spells out)


@functools.lru_cache(maxsize=None)
def _opgram_want(name, which, rows):
    fx = fixture(name)
    rows = list(range(len(fx["inf"]))) if rows is None else list(rows)
    return frozen(onepass_gram_ref.decode(fx["op_grams"][which], fx["im"][rows], fx["inf"][rows], *store(fx), fx["maxf"], OP_WORDS, fx["skip"], 0,
                                          fx["wos"]))


@functools.lru_cache(maxsize=None)
def forced_want(name):
    fx = fixture(name)
    return frozen(forced_ref.align(fx["im"], fx["inf"], *store(fx), fx["maxf"], fx["transcripts"], fx["max_words"], fx["skip"], 0, fx["wos"]))


# ---- CPU: the conditions the fixtures must meet (on the references alone) -----------------------------------------------------------
def test_longest_fixture_reaches_the_cap_row_word_where_it_should_and_nowhere_else():
    assert CAP >= 600
    fx = fixture("longest")
    assert fx["tf"].tolist() == [CAP, CAP - 63, 30] and fx["maxf"] == CAP + 100 and fx["inf"].max() <= fx["maxf"]
    assert fx["inf"][2] == CAP // 2 and fx["inf"][3] == CAP // 2 + 1 and (CAP - 1) * 80 >= 65536  # the image passes 64 KiB
    on, off = chain_want("longest"), chain_want("longest", False)
    assert np.all(on[0]["status"] == chain_ref.CH_OK)
    assert slots_of(on, 0) == [0, 2] and slots_of(on, 1) == [0] and slots_of(on, 4) == [1, 2]  # rows (a), (b), (e)
    assert OFF_ROWS["longest"] == (2, 3)  # rows (c) and (d) without skipping
    assert not {0, 1} & set(slots_of(on, 2)) and 0 not in slots_of(off, 0)  # (c): one frame too few for the cap-row word
    assert tuple(off[0][1])[1:] == (1, 0, chain_ref.CH_OK) and slots_of(off, 1) == [0]  # (d), skipping off: exactly the one word
    assert tuple(off[1][1, 0])[2:4] == (0, CAP // 2)
    assert onepass_ref.reach(fx["tf"]) == 16 and onepass_ref.reach(fixture("longest_two")["tf"]) == (CAP - 63) // 2 + 1 > 64


def test_sparse_fixture_decodes_the_high_slots_and_the_twins_lose_their_ties():
    fx = fixture("sparse")
    assert len(fx["tf"]) == 65536 and sorted(np.nonzero(fx["valid"])[0].tolist()) == sorted(sc.SPARSE_VALID)
    assert (fx["wos"] == 4).sum() == 65526 and not fx["valid"][fx["wos"] == 4].any() and 3 <= fx["tf"].min() and fx["tf"].max() <= 8
    for copy, of in sc.SPARSE_TWINS:
        assert fx["tf"][copy] == fx["tf"][of] and np.array_equal(fx["tm"][copy], fx["tm"][of]) and fx["wos"][copy] == fx["wos"][of]
    want = chain_want("sparse")
    assert slots_of(want, 0) == [65535, 32769, 256, 32767] and slots_of(want, 1) == [64, 0]
    assert want[1][0, :4]["word"].tolist() == [0, 3, 3, 1] and want[0][0]["cost"] == 3 * fx["skip"] and want[0][1]["cost"] == 0
    assert want[0][3]["status"] == chain_ref.CH_NONE and want[0][4]["status"] == chain_ref.CH_NONE  # one frame, no frame
    alts = span_want("sparse")[1]
    assert tuple(alts[0, 0, 0])[:3] == (0, 65535, 0)  # word 0 through its best slot 65 535
    none = gram_want("sparse", "none")
    assert 4 not in none[1]["word"][none[1]["word"] != 0xFFFFFFFF] and as_bytes(none) != as_bytes(gram_want("sparse", "anchor"))


def test_dense_fixture_decodes_high_slots_and_its_grammar_levels_pass_64_items():
    fx = fixture("dense")
    sizes = sorted(np.unique(fx["wos"], return_counts=True)[1].tolist())
    assert sizes == sorted(sc.DENSE_GROUPS) and len(fx["tf"]) == 300 and len(fx["big"]) == 65
    want = chain_want("dense")
    seen = {k for r in range(len(fx["inf"])) for k in slots_of(want, r)}
    assert len([k for k in seen if k >= 64]) >= 6 and len([k for k in seen if k >= 256]) >= 2, sorted(seen)
    assert [slots_of(want, r) for r in range(8)] == [list(p) for p in fx["plant"]]
    items = gram_ref.items_per_level(fx["grams"]["pairs"], fx["max_words"], fx["wos"])
    assert max(len(lv) for lv in items) > 64 and len(wgram_ref.distinct_lists(fx["wgrams"]["drawn"])) > 2  # (the plan's figures: GPU)
    forced = forced_want("dense")
    assert np.all(forced[0]["status"] == chain_ref.CH_OK) and set(forced[1][5]["slot"].tolist()) <= set(fx["big"])


# ---- GPU: helpers ------------------------------------------------------------------------------------------------------------------
def make_engine(fx, **kw):
    eng = Engine(max_frames=fx["maxf"], device=0, **kw)
    eng.set_templates_dense(*store(fx))
    if fx["wos"] is not None:
        eng.set_word_map(fx["wos"])
    return eng


class hooks(t_forced.hooks):
    pass


# ---- GPU 1: level building -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_decode_words(name):
    fx = fixture(name)
    eng = make_engine(fx, testing=True)
    W, tpl = fx["max_words"], int(fx["tf"].max())
    for skip_on in (True, False):
        want, skip = chain_want(name, skip_on), fx["skip"] if skip_on else None
        rows = list(range(len(fx["inf"]))) if skip_on else list(OFF_ROWS[name])
        im, inf = fx["im"][rows], fx["inf"][rows]
        for canary in CANARIES:
            t_chain.same(t_chain.dev_call(eng, im, inf, W, 0, skip, 0, canary), want, f"{name}: device form, skip {skip}")
        t_chain.same(eng.decode_words(im, inf, W, 0, skip), want, f"{name}: host form, skip {skip}")
    # chunk seams whose 2M - 2 lead-in is longer than the chunk, and launch groups of one row: the same bytes
    want, cols = chain_want(name), 256 if name == "longest" else 7
    assert 2 * tpl - 2 > cols
    for c, r in ((cols, 0), (0, 1), (cols, 1)):
        with hooks(chain_chunk_cols=c, chain_rows=r):
            g = engine.decode_geometry(tpl, fx["maxf"], W, testing=True)
            assert (not c or g["chunk_cols"] == c) and (not r or g["rows"] == r)
            t_chain.same(t_chain.dev_call(eng, fx["im"], fx["inf"], W, 0, fx["skip"]), want, f"{name}: chunk {c}, rows {r}")
    eng.close()


# ---- GPU 2: grammars, unweighted and weighted ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_decode_grammar(name):
    fx = fixture(name)
    eng = make_engine(fx)
    W = fx["max_words"]
    anchor = eng.grammar(*gram_ref.grammar_any(fx["labels"]))
    got = t_gram.gram_call(eng, anchor, fx["im"], fx["inf"], W, 0, fx["skip"])
    t_gram.same(got, chain_want(name), f"{name}: anchor grammar")  # (one state: `reserved` is 0 as in the decoder's rows)
    assert as_bytes(got) == as_bytes(t_gram.gram_call(eng, None, fx["im"], fx["inf"], W, 0, fx["skip"], chain=True))
    anchor.close()
    for which, gram in fx["grams"].items():
        g = eng.grammar(*gram)
        plan = g.plan(W)
        assert plan["items_per_level"] == [len(lv) for lv in gram_ref.items_per_level(gram, W, fx["labels"] if fx["wos"] is None else fx["wos"], fx["valid"])]
        if name == "dense":
            assert max(plan["items_per_level"]) > 64
        for canary in CANARIES:
            t_gram.same(t_gram.gram_call(eng, g, fx["im"], fx["inf"], W, 0, fx["skip"], 0, canary), gram_want(name, which), f"{name}: grammar {which}")
        t_gram.same(eng.decode_grammar(g, fx["im"], fx["inf"], W, 0, fx["skip"]), gram_want(name, which), f"{name}: grammar {which}, host form")
        g.close()
    for which, gram in fx["wgrams"].items():  # nonzero arc and final costs: the _w kernels
        assert any(gram[3]) and any(gram[4])
        g = eng.grammar(*gram)
        assert g.plan(W)["from_sets"] == len(wgram_ref.distinct_lists(gram)) and (name != "dense" or g.plan(W)["from_sets"] > 2)
        for canary in CANARIES:
            t_gram.same(t_gram.gram_call(eng, g, fx["im"], fx["inf"], W, 0, fx["skip"], 0, canary), wgram_want(name, which), f"{name}: weighted {which}")
        g.close()
    eng.close()


# ---- GPU 3: one pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES + ("longest_two",))
def test_decode_onepass(name):
    fx, rows = fixture(name), op_rows(name)
    want = onepass_want(name, None if rows is None else tuple(rows))
    rows = list(range(len(fx["inf"]))) if rows is None else rows
    im, inf = fx["im"][rows], fx["inf"][rows]
    L = onepass_ref.reach(fx["tf"], fx["valid"])
    shortest = int(fx["tf"].min() if fx["valid"] is None else fx["tf"][fx["valid"] != 0].min())
    g = engine.decode_onepass_geometry(int(fx["tf"].max()), len(fx["tf"]), fx["maxf"], shortest)
    assert g["block"] == L and (name != "longest" or -(-fx["maxf"] // L) >= 100) and (name != "longest_two" or 2 * L - 1 > 64)
    eng = make_engine(fx)
    for canary in CANARIES:
        t_onepass.same(t_onepass.dev_call(eng, im, inf, OP_WORDS, fx["skip"], 0, 0, canary), want, f"{name}: device form")
    t_onepass.same(eng.decode_onepass(im, inf, OP_WORDS, fx["skip"]), want, f"{name}: host form")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES + ("longest_two",))
def test_decode_onepass_grammar(name):
    fx = fixture(name)
    rows = op_rows("longest_gram" if name == "longest" else name) or list(range(len(fx["inf"])))
    im, inf = fx["im"][rows], fx["inf"][rows]
    eng = make_engine(fx)
    for which, gram in fx["op_grams"].items():
        want = opgram_want(name, which, tuple(rows))
        g = eng.grammar(*gram)
        kept = onepass_gram_ref.kept(gram, fx["labels"] if fx["wos"] is None else fx["wos"], fx["valid"])
        plan = engine.onepass_grammar_plan(g)
        assert (plan["kept_items"], plan["kept_states"]) == (len(kept[0]), len(kept[1])) and plan["rows"] >= 1
        for canary in CANARIES:
            t_opgram.same(t_opgram.dev_call(eng, g, im, inf, OP_WORDS, fx["skip"], 0, 0, canary), want, f"{name}: one-pass grammar {which}")
        t_opgram.same(eng.decode_onepass_grammar(g, im, inf, OP_WORDS, fx["skip"]), want, f"{name}: one-pass grammar {which}, host form")
        g.close()
    eng.close()


# ---- GPU 4: forced alignment and the gather -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_align_transcripts_and_gather(name):
    fx, want = fixture(name), forced_want(name)
    W, n = fx["max_words"], len(fx["inf"])
    eng = make_engine(fx)
    for canary in CANARIES:
        t_forced.same(t_forced.forced_call(eng, fx["im"], fx["inf"], fx["transcripts"], W, fx["skip"], 0, canary), want, f"{name}: forced alignment")
    longest = max(len(t) for t in fx["transcripts"])  # the host form's words_per_row
    t_forced.same(eng.align_transcripts(fx["im"], fx["inf"], fx["transcripts"], fx["skip"]), (want[0], np.ascontiguousarray(want[1][:, :longest])),
                  f"{name}: forced alignment, host form")
    # every word row an example, in row order; 1024 rows an example at most: the cap-row word's span does not fit and stays empty
    dst = np.arange(n * W, dtype=np.uint32)
    ex_rows = min(int(fx["inf"].max()), 1024)
    ex_want = forced_ref.gather(fx["im"], fx["inf"], fx["maxf"], want[1], dst, n * W, ex_rows)
    assert (ex_want[1] > 0).sum() >= 3 and (name != "longest" or ex_want[1][0] == 0)
    for canary in CANARIES:
        rc, g_ex, g_ef = t_forced.gather_call(eng, fx["im"], fx["inf"], want[1], dst, n * W, ex_rows, canary)
        assert rc == 0, eng.L.sr_last_error()
        g_ex.check_equals(ex_want[0])
        g_ef.check_equals(ex_want[1])
    eng.close()


# ---- GPU 5: the spotter, the span scorer, alternatives, N-best ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spot_want(name, win):
    fx = fixture(name)
    out = spot_ref.spot_hits(fx["im"], fx["inf"], *store(fx), fx["maxf"], win)
    out.setflags(write=False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_spot(name):
    fx = fixture(name)
    eng = make_engine(fx)
    for win in (0, fx["spot_win"]):
        want = spot_want(name, win)
        for canary in CANARIES:
            hits, scores = t_spot.dev_call(eng, fx["im"], fx["inf"], win, canary)
            t_spot.same(hits, want, f"{name}: spotter, windows of {win}")
            assert np.array_equal(scores, want["dis"])
    assert eng.spot(fx["im"], fx["inf"])[0].tobytes() == spot_want(name, 0).tobytes()
    if name == "sparse":
        found = spot_want(name, 0)[0, 0]
        assert all(found[k]["dis"] == 0 for k in (65535, 32769, 32767, 32768, 256)) and tuple(found[65533]) == spot_ref.NO_HIT
    eng.close()


N_BEST = 4


@functools.lru_cache(maxsize=None)
def span_want(name):
    """(span scores of the decoder's word rows, alternatives, candidate counts) in mode SR_SPAN_ACC"""
    fx, dec = fixture(name), chain_want(name)
    wos = np.arange(len(fx["tf"]), dtype=np.uint32) if fx["wos"] is None else fx["wos"]
    scores = span_ref.span_scores(fx["im"], fx["inf"], *store(fx), dec[1], span_ref.SPAN_ACC)
    return frozen((scores,) + span_ref.nbest(scores, wos, N_BEST))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("sparse", "dense"))
def test_score_word_spans_and_decode_words_alts(name):
    fx, dec = fixture(name), chain_want(name)
    scores, alts, n_matched = span_want(name)
    W = fx["max_words"]
    eng = make_engine(fx)
    for canary in CANARIES:
        t_span.same_u32(t_span.span_call(eng, fx["im"], fx["inf"], dec[1], span_ref.SPAN_ACC, canary), scores, f"{name}: span scores")
        got = t_span.alts_call(eng, fx["im"], fx["inf"], W, N_BEST, span_ref.SPAN_ACC, fx["skip"], 0, canary)
        assert as_bytes(got[:3]) == as_bytes(dec), f"{name}: the decoder's own bytes"
        t_span.same_u32(got[5], scores, f"{name}: span scores of the alternatives call")
        t_span.same_u32(got[3], alts, f"{name}: alternatives", 4)
        t_span.same_u32(got[4], n_matched, f"{name}: candidate counts")
    host = eng.decode_words_alts(fx["im"], fx["inf"], W, N_BEST, span_ref.SPAN_ACC, 0, fx["skip"], 0, want_scores=True)
    assert as_bytes(host) == as_bytes(dec + (alts, n_matched, scores))
    eng.close()


def nbest_scores(fx):
    """score rows [6, K]: all finite, all SR_DIS_ERR, the valid slots alone, one value everywhere (every word ties), the last slot
    alone, the ends of the u32 range at the two ends of the store"""
    K = len(fx["tf"])
    rng = np.random.default_rng(K)
    s = np.full((6, K), DIS_ERR, np.uint32)
    s[0] = rng.integers(0, 1 << 20, K)
    ok = np.ones(K, bool) if fx["valid"] is None else fx["valid"] != 0
    s[2, ok] = rng.integers(0, 50, int(ok.sum()))
    s[3] = 77
    s[4, K - 1] = 5
    s[5, 0], s[5, K - 1], s[5, K // 2] = 0xFFFFFFFE, 0, 0
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("sparse", "dense"))
def test_nbest_over_whole_score_rows_counts_every_slot_of_a_word(name):
    fx = fixture(name)
    K, s = len(fx["tf"]), nbest_scores(fixture(name))
    eng = make_engine(fx)
    maps = [fx["wos"], fx["wos"].max() - fx["wos"]]  # the second: the same groups under ids in reverse order
    for wos in maps:
        eng.set_word_map(wos)
        nb, nm = span_ref.nbest(s, wos, N_BEST)
        assert name != "sparse" or (nb[0, 0]["count"] == 65526 and nb[0, 0]["word"] == wos[1])  # a word's count is its whole group
        for canary in CANARIES:
            g_nb = guarded_out((len(s), N_BEST), span_ref.NBEST_DTYPE, canary, 4096, "cuda:0", "nbest")
            g_nm = guarded_out((len(s),), np.uint32, canary, 4096, "cuda:0", "n_matched")
            d_s = torch.from_numpy(s.view(np.int32)).cuda()
            assert eng.L.sr_nbest_batch_dev(eng.h, P(d_s.data_ptr()), U32(len(s)), U32(N_BEST), P(g_nb.ptr), P(g_nm.ptr),
                                            P(torch.cuda.current_stream().cuda_stream)) == 0, eng.L.sr_last_error()
            torch.cuda.synchronize()
            g_nb.check_equals(nb)
            g_nm.check_equals(nm)
        h_nb, h_nm = eng.nbest(s, N_BEST)
        assert h_nb.tobytes() == nb.tobytes() and np.array_equal(h_nm, nm)
    if name == "sparse":
        assert nm[0] == 5 and nm[4] == 1 and tuple(nb[4, 0]) == (4, 65535, 5, 1)
        # the decoder under the reversed ids: the same slots, the other words
        want = chain_ref.decode(fx["im"], fx["inf"], *store(fx), fx["maxf"], fx["max_words"], 0, fx["skip"], 0, maps[1])
        t_chain.same(t_chain.dev_call(eng, fx["im"], fx["inf"], fx["max_words"], 0, fx["skip"]), want, "sparse: word ids in reverse order")
        assert want[1][0, :4]["word"].tolist() == [4, 1, 1, 3] and want[1][0, :4]["slot"].tolist() == [65535, 32769, 256, 32767]
    eng.close()


# ---- GPU 6: the four live sessions --------------------------------------------------------------------------------------------------
def cuts(N, sizes):
    """the sizes in order while frames are left, then the rest in one push"""
    out = []
    for s in sizes:
        if sum(out) < N:
            out.append(min(s, N - sum(out)))
    if sum(out) < N:
        out.append(N - sum(out))
    return out


def live_case(name):
    fx = fixture(name)
    rows = list(fx["live_rows"])
    n = [int(v) for v in fx["inf"][rows]]
    sched = t_spot_live.per_channel([cuts(N, fx["live_sizes"]) for N in n])
    return fx, rows, fx["im"][rows], n, sched, max(max(c) for c in sched), fx.get("live_words", fx["max_words"])


def rows_np(out, W):
    torch.cuda.synchronize()
    n = out["n_rows"]

    def host(t, dt, shape):
        return t if isinstance(t, np.ndarray) else t.cpu().numpy().view(dt).reshape(shape)

    got = [host(out["rec"], chain_ref.CHAIN_REC_DTYPE, (n,)), host(out["words"], chain_ref.CHAIN_WORD_DTYPE, (n, W))]
    if out.get("level_cost") is not None:
        got.append(host(out["level_cost"], np.uint32, (n, W)))
    return got


def run_session(ses, f, n, sched, W, want, what):
    """pushes channel c's n[c] frames along the schedule (device form, poison behind every count); the rows of each channel's
    last push, and those of end(), are the batch reference's row of the whole recording"""
    n_ch = len(n)
    d_f = torch.from_numpy(np.array(f)).cuda()
    at, last = [0] * n_ch, [None] * n_ch
    for cnt in sched:
        chunk = torch.full((n_ch, max(max(cnt), 1), 12), 0x7FFF, dtype=torch.int16, device="cuda:0")
        for c in range(n_ch):
            chunk[c, :cnt[c]] = d_f[c, at[c]:at[c] + cnt[c]]
        out = ses.push_dev(chunk, np.array(cnt, np.uint32))
        at = [a + b for a, b in zip(at, cnt)]
        exp = [(c, at[c]) for c in range(n_ch) if cnt[c]]
        assert [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == exp, (what, out["rows"], exp)
        got = rows_np(out, W)
        for r, (c, _) in enumerate(exp):
            last[c] = as_bytes([a[r] for a in got])
    assert at == n
    end = ses.end(list(range(n_ch)))
    assert [(int(r["channel"]), int(r["frames"])) for r in end["rows"]] == [(c, n[c]) for c in range(n_ch)]
    got = rows_np(end, W)
    for c in range(n_ch):
        exp = as_bytes([a[c] for a in want])
        assert last[c] == exp, f"{what}: channel {c} after its last push"
        assert as_bytes([a[c] for a in got]) == exp, f"{what}: channel {c} at end"
    ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_decode_live_and_grammar_live(name):
    fx, rows, f, n, sched, chunk_max, W = live_case(name)
    eng = make_engine(fx)
    mw = None if W == fx["max_words"] else W
    run_session(eng.decode_live(len(n), chunk_max, fx["maxf"], W, 0, fx["skip"]), f, n, sched, W, [a[rows] for a in chain_want(name, True, mw)],
                f"{name}: decode_live")
    which = next(iter(fx["grams"]))
    g = eng.grammar(*fx["grams"][which])
    run_session(eng.decode_grammar_live(g, len(n), chunk_max, fx["maxf"], W, 0, fx["skip"]), f, n, sched, W,
                [a[rows] for a in gram_want(name, which, mw)], f"{name}: decode_grammar_live, grammar {which}")
    g.close()
    g = eng.grammar(*fx["wgrams"]["drawn"])
    run_session(eng.decode_grammar_live(g, len(n), chunk_max, fx["maxf"], W, 0, fx["skip"]), f, n, sched, W,
                [a[rows] for a in wgram_want(name, "drawn", mw)], f"{name}: decode_grammar_live, weighted")
    g.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_decode_onepass_live(name):
    fx, rows, f, n, sched, chunk_max, _ = live_case(name)
    op = op_rows(name)
    want = onepass_want(name, None if op is None else tuple(op))
    eng = make_engine(fx)
    run_session(eng.decode_onepass_live(len(n), chunk_max, fx["maxf"], OP_WORDS, False, fx["skip"]), f, n, sched, OP_WORDS, [a[rows] for a in want],
                f"{name}: decode_onepass_live")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_spot_live(name):
    fx, rows, f, n, sched, chunk_max, _ = live_case(name)
    win = fx["spot_win"]
    eng = make_engine(fx)
    ses = eng.spot_live(len(n), chunk_max, win)
    col = t_spot_live.Collector(ses, len(n), win)
    d_f = torch.from_numpy(np.array(f)).cuda()
    at = [0] * len(n)
    for cnt in sched:
        chunk = torch.full((len(n), max(max(cnt), 1), 12), 0x7FFF, dtype=torch.int16, device="cuda:0")
        for c in range(len(n)):
            chunk[c, :cnt[c]] = d_f[c, at[c]:at[c] + cnt[c]]
        col.take(ses.push_dev(chunk, np.array(cnt, np.uint32)), cnt)
        at = [a + b for a, b in zip(at, cnt)]
    col.end(list(range(len(n))))
    ses.close()
    for c in range(len(n)):  # the windows of a channel are the batch spotter's over the whole recording
        t_spot_live.same(col.channel(c), spot_live_ref.window_records(f[c, :n[c]], *store(fx), win), f"{name}: spot_live, channel {c}")
        assert col.channel(c).tobytes() == spot_want(name, win)[rows[c], :-(-n[c] // win)].tobytes()
    eng.close()


# ---- GPU 7: one slot more than the decoders take --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_store_of_65537_slots_is_refused_by_every_decoder_and_by_nothing_else():
    fx = sc.too_many()
    K, n, W = len(fx["tf"]), len(fx["inf"]), fx["max_words"]
    assert K == 65537
    eng = make_engine(fx)
    d_im, d_inf = t_chain.dev(fx["im"]), t_chain.dev(fx["inf"])
    sid = P(torch.cuda.current_stream().cuda_stream)
    im_p, inf_p, skip = P(d_im.data_ptr()), P(d_inf.data_ptr()), U32(fx["skip"])
    v = engine._vp

    def outs(where, **shapes):
        return {k: guarded_out(s, dt, 0xA5, 4096, where, k) for k, (s, dt) in shapes.items()}

    def untouched(g, rc, what):
        torch.cuda.synchronize()
        assert rc == BAD_ARG and b"65536" in eng.L.sr_last_error(), (what, rc, eng.L.sr_last_error())
        for x in g.values():
            x.check_untouched()

    REC, WORD = chain_ref.CHAIN_REC_DTYPE, chain_ref.CHAIN_WORD_DTYPE
    L, h = eng.L, eng.h
    for where in ("cuda:0", None):
        a, b = (im_p, inf_p) if where else (v(fx["im"]), v(fx["inf"]))
        tail = (sid,) if where else ()
        sfx = "_dev" if where else ""
        g = outs(where, rec=((n,), REC), words=((n, W), WORD), lc=((n, W), np.uint32))
        rc = getattr(L, "sr_decode_words_dp" + sfx)(h, a, b, U32(1), U32(n), U32(W), U32(0), skip, U32(0), P(g["rec"].ptr), P(g["words"].ptr), P(g["lc"].ptr), *tail)
        untouched(g, rc, "decode_words")
        g = outs(where, rec=((n,), REC), words=((n, OP_WORDS), WORD))
        rc = getattr(L, "sr_decode_onepass_dp" + sfx)(h, a, b, U32(1), U32(n), U32(0), U32(OP_WORDS), skip, U32(0), P(g["rec"].ptr), P(g["words"].ptr), *tail)
        untouched(g, rc, "decode_onepass")
        lab, cnt = t_forced.host_tables([[K - 1]] * n, W)
        g = outs(where, rec=((n,), REC), words=((n, W), WORD))
        rc = getattr(L, "sr_align_transcripts_dp" + sfx)(h, a, b, U32(1), U32(n), v(lab), v(cnt), U32(W), skip, U32(0), P(g["rec"].ptr), P(g["words"].ptr), *tail)
        untouched(g, rc, "align_transcripts")
        spans = span_ref.spans([[(0, 5), (6, 9)]] * n)
        d_w = t_span.dev(spans)
        g = outs(where, scores=((n, W, K), np.uint32))
        rc = getattr(L, "sr_score_word_spans" + sfx)(h, a, b, U32(1), U32(n), U32(W), P(d_w.data_ptr()) if where else v(spans), U32(0), P(g["scores"].ptr), *tail)
        untouched(g, rc, "score_word_spans")
        g = outs(where, rec=((n,), REC), words=((n, W), WORD), lc=((n, W), np.uint32), alts=((n, W, N_BEST), span_ref.NBEST_DTYPE), nm=((n, W), np.uint32))
        rc = getattr(L, "sr_decode_words_alts" + sfx)(h, a, b, U32(1), U32(n), U32(W), U32(0), skip, U32(0), P(g["rec"].ptr), P(g["words"].ptr), P(g["lc"].ptr),
                                                      U32(N_BEST), U32(0), P(g["alts"].ptr), P(g["nm"].ptr), None, *tail)
        untouched(g, rc, "decode_words_alts")
    # no grammar is compiled against such a store (so no grammar call and no grammar session exists), and no session opens
    for what, call in (("grammar", lambda: eng.grammar(*gram_ref.grammar_any([K - 1]))),
                       ("weighted grammar", lambda: eng.grammar(*wgram_ref.with_costs(gram_ref.grammar_any([K - 1]), [5], [7]))),
                       ("decode_live", lambda: eng.decode_live(2, 8, fx["maxf"], W, 0, fx["skip"])),
                       ("decode_onepass_live", lambda: eng.decode_onepass_live(2, 8, fx["maxf"], OP_WORDS, False, fx["skip"]))):
        with pytest.raises(SrError, match="error 3.*65536"):
            call()
    # what the header does not limit: the spotter, batch and live, the N-best stage and the gather give the reference's bytes
    want = spot_ref.spot_hits(fx["im"], fx["inf"], *store(fx), fx["maxf"], 8)
    hits, _ = t_spot.dev_call(eng, fx["im"], fx["inf"], 8, 0x3C)
    t_spot.same(hits, want, "65 537 slots: spotter")
    assert want[0, 1, K - 1]["dis"] == 0 and tuple(want[0, 1, K - 1])[1:3] == (4, 8)
    ses = eng.spot_live(1, 32, 8)
    out = ses.push(fx["im"][:1, :20], np.array([20], np.uint32))
    assert out["hits"].tobytes() == want[0, :2].tobytes()
    assert ses.end([0])["hits"].tobytes() == want[0, 2:3].tobytes()
    ses.close()
    s = nbest_scores(fx)
    nb, nm = span_ref.nbest(s, np.arange(K), N_BEST)
    h_nb, h_nm = eng.nbest(s, N_BEST)
    assert h_nb.tobytes() == nb.tobytes() and np.array_equal(h_nm, nm) and nb[4, 0]["slot"] == K - 1
    words = np.empty((n, W), WORD)
    words[...] = chain_ref.NO_WORD_ROW
    words[0, 0]["start"], words[0, 0]["end"] = 4, 8
    ex_want = forced_ref.gather(fx["im"], fx["inf"], fx["maxf"], words, np.arange(n * W, dtype=np.uint32), n * W, 8)
    rc, g_ex, g_ef = t_forced.gather_call(eng, fx["im"], fx["inf"], words, np.arange(n * W, dtype=np.uint32), n * W, 8, 0xA5)
    assert rc == 0 and g_ex.check_equals(ex_want[0]) and g_ef.check_equals(ex_want[1]) and ex_want[1][0] == 5
    eng.close()


# ---- CPU: the allow lists --------------------------------------------------------------------------------------------------------------
def launches(text):
    """every hipLaunchKernelGGL(...) of a source text -> [(kernel, dynamic LDS argument)]"""
    out, at = [], 0
    while (at := text.find("hipLaunchKernelGGL(", at)) >= 0:
        at += len("hipLaunchKernelGGL(")
        depth, args, cur = 1, [], ""
        for ch in text[at:]:
            opening, closing = ("(<{", ")>}") if not args else ("({", ")}")  # angle brackets: the kernel's template arguments only
            depth += (ch in opening) - (ch in closing)
            if depth == 0:
                break
            if ch == "," and depth == 1:
                args.append(cur.strip())
                cur = ""
            else:
                cur += ch
        args.append(cur.strip())
        out.append((args[0].strip("()").split("<")[0], args[3]))
    return out


def test_every_kernel_launched_with_dynamic_lds_is_in_its_files_allow_list():
    """sr_create raises hipFuncAttributeMaxDynamicSharedMemorySize for the kernels of every *_allow_lds list.  The runtime this was
    written on launches 128 000 bytes of dynamic LDS without the attribute as well (a scratch build with k_onepass_gram_words off
    its list passed every cap-row test above), so a missing entry shows on no GPU test here; another runtime may refuse the launch"""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stm32_speech_recognition_amd", "csrc")
    seen = 0
    for path in sorted(glob.glob(os.path.join(csrc, "k_*.hip"))):
        text = re.sub(r"//[^\n]*", "", open(path).read())
        allowed = set(re.findall(r"\{\s*\(const void \*\)\s*(\w+)", text))
        for kernel, lds in launches(text):
            if lds != "0" and allowed:  # (a file without a list keeps its dynamic LDS below 64 KiB: the frame kernels)
                assert kernel in allowed, (os.path.basename(path), kernel, lds)
                seen += 1
    assert seen >= 14  # the LDS-staged decoder, aligner and spotter kernels at least
