"""One-pass grammar decoding on the device: the one-pass recurrence over the states of a grammar, weighted grammars included
(include/sr_engine.h, "one-pass grammar decoding").

The definition lives in tests/onepass_gram_ref.py (plain Python; its own checks are tests/test_onepass_gram_ref.py).  Every
comparison here is byte for byte against it -- records and every word row with the grammar state in `reserved` -- and, where
the header promises it, against the engine's own one-pass decoder and its own level building.  No tolerances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_ref
import onepass_gram_ref as ref
import onepass_ref
import wgram_ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from spot_ref import local_dis
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import DIS_ERR, VAD_DTYPE, Engine

BAD_ARG = 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
MAXF, SKIP, K = chain_ref.PLANT_MAXF, chain_ref.PLANT_SKIP, chain_ref.PLANT_K
LONG_MAXF = onepass_ref.LONG_MAXF
ONES = 0xFFFFFFFF
COSTS = ((1500, 0), (None, 5000), (300, 5000))
LABELS = list(range(K))
PAIRS = wgram_ref.grammar_word_pairs(LABELS, [(a, b) for a in LABELS for b in LABELS if (a + b) % 2 == 0 or a == b])
GRAMS = dict(any=wgram_ref.grammar_any(LABELS), pairs=PAIRS,
             sequence=wgram_ref.grammar_sequence([LABELS, LABELS[:3], LABELS, LABELS], optional_tail=True),
             weighted=wgram_ref.drawn_costs(PAIRS))


def skip_arg(skip):
    return DIS_ERR if skip is None else skip


def same(got, want, what):
    """(rec, words) against the reference's, byte for byte"""
    for name, g, w, width in zip(("rec", "words"), got, want, (4, 8)):
        g, w = np.asarray(g).view(np.uint32).reshape(-1, width), np.asarray(w).view(np.uint32).reshape(-1, width)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero(np.any(g != w, 1))[0]
        if len(bad):
            raise AssertionError(f"{what}: {len(bad)} of {len(w)} {name} entries differ, first at {int(bad[0])}: "
                                 f"got {g[bad[0]].tolist()} want {w[bad[0]].tolist()}")


def as_bytes(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out)


def dev(a):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def dev_call(eng, gram, im, frames, words_cap, skip=None, word_cost=0, frames_cap=0, canary=0xA5, frames_stride=1, d_frames=None):
    """sr_decode_onepass_grammar_dp_dev into guarded buffers whose every byte starts as the canary -> (rec, words)"""
    n = len(im)
    d_im = dev(im)
    if d_frames is None:
        d_frames = dev(np.ascontiguousarray(frames, dtype=np.uint32))
    g_r = guarded_out((n,), ref.CHAIN_REC_DTYPE, canary, 4096, "cuda:0", "rec")
    g_w = guarded_out((n, words_cap), ref.CHAIN_WORD_DTYPE, canary, 4096, "cuda:0", "words")
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_decode_onepass_grammar_dp_dev(eng.h, gram.g, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(frames_stride), U32(n),
                                                U32(frames_cap), U32(words_cap), U32(skip_arg(skip)), U32(word_cost), P(g_r.ptr), P(g_w.ptr), P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_r.check()
    g_w.check()
    return g_r.interior(), g_w.interior()


class hooks:
    """development hooks "onepass_block" / "onepass_rows" / "onepass_gram_prune_off" (testing library only; read per call)"""

    def __init__(self, block=0, rows=0, prune_off=0):
        self.v = dict(onepass_block=block, onepass_rows=rows, onepass_gram_prune_off=prune_off)

    def __enter__(self):
        for k, v in self.v.items():
            engine.dev_hook(k, v)

    def __exit__(self, *exc):
        for k in self.v:
            engine.dev_hook(k, 0)


@functools.lru_cache(maxsize=None)
def planted_want(name, skip, wc, words_cap=16):
    fx = chain_ref.planted()
    want = ref.decode(GRAMS[name], fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, words_cap, skip, wc)
    for a in want:
        a.setflags(write=False)
    return want


def planted_engine(**kw):
    fx = chain_ref.planted()
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


def long_grammar(forbid=None):
    """the pairs grammar that allows exactly the planted bigrams of planted_long() (less the pair `forbid`)"""
    pl = ref.planted_long()
    pairs = {(a, b) for seq in pl["seq"] for a, b in zip(seq, seq[1:])} - {forbid}
    return wgram_ref.grammar_word_pairs(range(K), sorted(pairs), first={seq[0] for seq in pl["seq"]})


def forbidden_pair():
    seq = ref.planted_long()["seq"][0]
    return next((a, b) for a, b in zip(seq, seq[1:]) if a != b)


@functools.lru_cache(maxsize=None)
def long_want(forbid=None):
    pl = ref.planted_long()
    want = ref.decode(long_grammar(forbid), pl["im"], pl["inf"], pl["tm"], pl["tf"], None, LONG_MAXF, 64, SKIP, 0)
    for a in want:
        a.setflags(write=False)
    return want


# ---- GPU 1: the planted rows: the restatement, the one-pass decoder, level building ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAMS))
def test_planted_rows(name):
    fx = chain_ref.planted()
    eng = planted_engine()
    gram = eng.grammar(*GRAMS[name])
    pl = engine.onepass_grammar_plan(gram)
    items, states = ref.kept(GRAMS[name], LABELS)
    assert pl == dict(row_bytes=GRAMS[name][0] * (MAXF + 1) * 12 + len(items) * int(fx["tf"].max()) * 16, rows=min(65535, (256 << 20) // pl["row_bytes"]),
                      block=5, launches=2 * (MAXF // 5) + 2, kept_items=len(items), kept_states=len(states)), pl
    assert engine.onepass_grammar_plan(gram, 23)["launches"] == 2 * 5 + 2
    for skip, wc in COSTS:
        want = planted_want(name, skip, wc)
        rec, words = dev_call(eng, gram, fx["im"], fx["inf"], 16, skip, wc)
        same((rec, words), want, f"{name}, skip {skip}, word_cost {wc}")
        if name == "any":  # the anchor: the bytes of the engine's own one-pass decoder
            assert as_bytes((rec, words)) == as_bytes(eng.decode_onepass(fx["im"], fx["inf"], 16, skip, wc)), (skip, wc)
            assert not np.any(words["reserved"][words["slot"] != ONES])
            continue
        # the engine's own level building at max_words 16: the minimum over its level costs is unique on these rows
        l_rec, l_words, _ = eng.decode_grammar(gram, fx["im"], fx["inf"], 16, 0, skip, wc)
        assert np.all(l_rec["status"] == ref.CH_OK) and np.array_equal(rec["cost"], l_rec["cost"]) and np.array_equal(rec["n_words"], l_rec["n_words"])
        assert words.tobytes() == l_words.tobytes(), (name, skip, wc)
    if name == "sequence":  # one slot under several targets: the state says which position the word took
        w = planted_want(name, SKIP, 0)[1]
        assert any(len(set(w["reserved"][w["slot"] == k].tolist())) > 1 for k in LABELS)
    gram.close()
    eng.close()


# ---- GPU 2: more words than level building holds --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_planted_long_rows_under_the_planted_bigrams_and_with_one_pair_forbidden():
    fx = ref.planted_long()
    eng = Engine(max_frames=LONG_MAXF, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    gram = eng.grammar(*long_grammar())
    rec, words = dev_call(eng, gram, fx["im"], fx["inf"], 64, SKIP)
    same((rec, words), long_want(), "planted_long, the planted bigrams")
    assert np.all(rec["status"] == ref.CH_OK) and rec["n_words"].tolist() == list(onepass_ref.LONG_COUNTS) and min(rec["n_words"]) > 16
    for r, seq in enumerate(fx["seq"]):
        assert words[r, :len(seq)]["slot"].tolist() == seq and words[r, :len(seq)]["reserved"].tolist() == [1 + k for k in seq], r
        assert [(int(w["start"]), int(w["end"])) for w in words[r, :len(seq)]] == fx["spans"][r], r
    free = eng.decode_onepass(fx["im"], fx["inf"], 64, SKIP)
    assert rec.tobytes() == free[0].tobytes()
    same(eng.decode_onepass_grammar(gram, fx["im"], fx["inf"], 64, SKIP), long_want(), "planted_long, host form")
    gram.close()
    gram = eng.grammar(*long_grammar(forbidden_pair()))
    rec2, words2 = dev_call(eng, gram, fx["im"], fx["inf"], 64, SKIP)
    same((rec2, words2), long_want(forbidden_pair()), "planted_long, one pair forbidden")
    assert rec2[0]["cost"] > rec[0]["cost"] and words2[0].tobytes() != free[1][0].tobytes()
    gram.close()
    eng.close()


# ---- GPU 3: seams and pruning --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sequence", "weighted"])
def test_every_block_length_group_size_and_pruning_give_identical_bytes(name):
    fx, want = chain_ref.planted(), planted_want(name, SKIP, 0)
    L = ref.reach(fx["tf"])
    assert L == 5
    eng = planted_engine(testing=True)
    gram = eng.grammar(*GRAMS[name])
    first = as_bytes(dev_call(eng, gram, fx["im"], fx["inf"], 16, SKIP))
    full = engine.onepass_grammar_plan(gram)
    for block, rows, off in ((1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (L, 0, 0), (0, 1, 0), (0, 3, 0), (0, 12, 0), (2, 3, 1), (0, 0, 1)):
        with hooks(block, rows, off):
            pl = engine.onepass_grammar_plan(gram)
            assert pl["block"] == (block or L) and (not rows or pl["rows"] == rows)
            if off:
                assert pl["kept_states"] == GRAMS[name][0] and pl["kept_items"] >= full["kept_items"]
            got = dev_call(eng, gram, fx["im"], fx["inf"], 16, SKIP)
        same(got, want, f"block {block}, rows {rows}, prune_off {off}")
        assert as_bytes(got) == first, (block, rows, off)
    gram.close()
    eng.close()


@pytest.mark.gpu
def test_pruning_drops_what_cannot_matter_and_changes_no_byte():
    """state 3 is unreachable, state 4 reaches no final state; two slots per word under a word map, one of them invalid"""
    fx = chain_ref.planted()
    graph = (5, [(0, 1, 0), (1, 2, 1), (3, 2, 2), (1, 4, 2), (4, 4, 2), (2, 2, 1), (2, 1, 0)], [0, 0, 1, 0, 0], [0, 900, 5, 0, 0, 40, 7], [0, 0, 300, 0, 0])
    wmap = np.array([0, 0, 1, 1, 2], np.uint32)
    valid = np.array([1, 1, 0, 1, 1], np.uint8)
    items, states = ref.kept(graph, wmap.tolist(), valid)
    assert items == [(0, 1), (1, 1), (3, 2)] and states == [0, 1, 2]
    eng = Engine(max_frames=MAXF, device=0, testing=True)
    eng.set_templates_dense(fx["tm"], fx["tf"], valid)
    eng.set_word_map(wmap)
    gram = eng.grammar(*graph)
    pl = engine.onepass_grammar_plan(gram)
    assert (pl["kept_items"], pl["kept_states"]) == (3, 3)
    for skip, wc in COSTS:
        want = ref.decode(graph, fx["im"], fx["inf"], fx["tm"], fx["tf"], valid, MAXF, 8, skip, wc, word_of_slot=wmap)
        got = dev_call(eng, gram, fx["im"], fx["inf"], 8, skip, wc)
        same(got, want, f"pruned, skip {skip}, word_cost {wc}")
        with hooks(prune_off=1):
            off = engine.onepass_grammar_plan(gram)
            assert (off["kept_items"], off["kept_states"]) == (5, 5) and off["row_bytes"] > pl["row_bytes"]
            assert as_bytes(dev_call(eng, gram, fx["im"], fx["inf"], 8, skip, wc)) == as_bytes(got)
    assert not np.any(want[1]["slot"] == 2) and not np.any(want[1]["slot"] == 4) and set(want[1]["reserved"][want[1]["slot"] != ONES].tolist()) <= {1, 2}
    assert (want[0]["status"] == ref.CH_OK).sum() >= 6
    gram.close()
    eng.close()


@functools.lru_cache(maxsize=None)
def wide_fixture():
    """K = 3 templates of 128..150 frames: L = 65, one sweep spans more than 64 columns; two rows of 520 frames"""
    rng = np.random.default_rng(78)
    tf = np.array([128, 140, 150], np.uint32)
    tm = np.zeros((3, 151, 12), np.int16)
    for k in range(3):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    im = rng.integers(-3000, 3001, (2, 540, 12)).astype(np.int16)  # what is not a word is loud noise
    for r, order in enumerate(((1, 0, 2), (2, 2, 0))):
        at = 3 + r
        for k in order:
            n = int(tf[k])
            im[r, at:at + n] = tm[k, :n] + rng.integers(-60, 61, (n, 12))
            at += n + 2
        assert at <= 520
    inf = np.array([520, 520], np.uint32)
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf)


@pytest.mark.gpu
def test_sweeps_of_more_than_64_columns_hand_their_boundary_on():
    fx = wide_fixture()
    L = ref.reach(fx["tf"])
    assert L == 65 and min(fx["tf"]) >= 128  # a block alone is more than one sweep of 64 columns
    graph = wgram_ref.with_costs(ref.grammar_repeat([[1, 2]], [0, 2], 1), [3000, 0, 10, 20, 30, 40], None)
    eng = Engine(max_frames=540, device=0, testing=True)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    gram = eng.grammar(*graph)
    for skip in (4000, None):
        want = ref.decode(graph, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, 540, 8, skip, 0)
        if skip:
            assert want[0]["n_words"].tolist() == [3, 3] and want[1][:, :3]["slot"].tolist() == [[1, 0, 2], [2, 2, 0]]
            assert want[1][:, :3]["reserved"].tolist() == [[1, 2, 2], [1, 2, 2]]
        got = dev_call(eng, gram, fx["im"], fx["inf"], 8, skip)
        same(got, want, f"wide store, skip {skip}")
        with hooks(block=33):
            assert as_bytes(dev_call(eng, gram, fx["im"], fx["inf"], 8, skip)) == as_bytes(got)
    gram.close()
    eng.close()


# ---- GPU 4: what the grammar decides -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sequence_grammar_with_skipping_no_parse_and_filler_alone():
    fx = chain_ref.planted()
    eng = planted_engine()
    # a sequence with skipping on: the start state has no incoming arc, and the leading filler lives in it
    seq = wgram_ref.grammar_sequence([LABELS, LABELS], optional_tail=True)
    gram = eng.grammar(*seq)
    want = ref.decode(seq, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, 4, SKIP, 0)
    assert np.all(want[0]["status"] == ref.CH_OK) and want[0]["n_words"].max() == 2 and np.any(want[1][:, 0]["start"] > 0)
    same(dev_call(eng, gram, fx["im"], fx["inf"], 4, SKIP), want, "two-word sequence, skip on")
    gram.close()
    # no parse: four words do not fit ten frames
    four = wgram_ref.grammar_sequence([LABELS] * 4)
    gram = eng.grammar(*four)
    inf = np.full(len(fx["inf"]), 10, np.uint32)
    rec, words = dev_call(eng, gram, fx["im"], inf, 4, SKIP)
    same((rec, words), ref.decode(four, fx["im"], inf, fx["tm"], fx["tf"], None, MAXF, 4, SKIP, 0), "four words in ten frames")
    assert np.all(rec["status"] == ref.CH_NONE) and np.all(rec["cost"] == DIS_ERR) and np.all(words.view(np.uint32) == ONES)
    gram.close()
    # state 0 final and cheap filler: nothing was said; the same rows with state 0 not final must say something
    for final0 in (1, 0):
        loop = (2, [(0, 1, w) for w in LABELS] + [(1, 1, w) for w in LABELS], [final0, 1])
        gram = eng.grammar(*loop)
        want = ref.decode(loop, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, 8, 3, 0)
        got = dev_call(eng, gram, fx["im"], fx["inf"], 8, 3)
        same(got, want, f"cheap filler, state 0 final {final0}")
        if final0:
            assert np.all(got[0]["n_words"] == 0) and np.all(got[0]["status"] == ref.CH_OK)
            assert np.array_equal(got[0]["cost"], fx["inf"] * 3) and np.array_equal(got[0]["skipped"], fx["inf"])
        else:
            assert np.all(got[0]["n_words"] >= 1) and np.all(got[0]["status"] == ref.CH_OK)
        gram.close()
    eng.close()


@pytest.mark.gpu
def test_truncation_reports_the_true_count_the_first_words_and_their_states():
    fx = ref.planted_long()
    eng = Engine(max_frames=LONG_MAXF, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    gram = eng.grammar(*long_grammar())
    full = long_want()
    cut = dev_call(eng, gram, fx["im"], fx["inf"], 2, SKIP)
    assert np.all(cut[0]["status"] == ref.CH_TRUNCATED) and cut[0]["n_words"].tolist() == list(onepass_ref.LONG_COUNTS)
    assert cut[1].tobytes() == full[1][:, :2].tobytes() and np.array_equal(cut[0]["cost"], full[0]["cost"])
    assert np.array_equal(cut[0]["skipped"], full[0]["skipped"])
    assert cut[1]["reserved"].tolist() == [[1 + k for k in seq[:2]] for seq in fx["seq"]]
    gram.close()
    eng.close()


# ---- GPU 5: edges and contracts ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frame_edges_in_one_call():
    fx = chain_ref.planted()
    rng = np.random.default_rng(31)
    inf = np.array([0, 3, 4, 5, 6, int(fx["inf"][3]), int(fx["inf"][7]), 5000, 161, 97, 98, 101], np.uint32)
    im = fx["im"].copy()
    im[7] = rng.integers(-3000, 3001, (MAXF, 12))  # the clamped rows have frames up to the cap
    im[8, 60:] = im[3, :100]
    graph = GRAMS["weighted"]
    eng = planted_engine()
    gram = eng.grammar(*graph)
    wide = np.full((len(inf), 3), 0x7F7F7F7F, np.uint32)
    wide[:, 1] = inf
    d_wide = dev(wide)
    for skip in (SKIP, None):
        for cap in (0, 97, 5000):
            want = ref.decode(graph, im, inf, fx["tm"], fx["tf"], None, MAXF, 8, skip, 0, frames_cap=cap)
            assert tuple(want[0][0]) == (DIS_ERR, 0, 0, ref.CH_NONE)  # N = 0
            assert tuple(want[0][1]) == (DIS_ERR, 0, 0, ref.CH_NONE)  # shorter than any word's reach, and state 0 is not final
            same(dev_call(eng, gram, im, inf, 8, skip, 0, cap), want, f"skip {skip}, frames_cap {cap}")
            same(dev_call(eng, gram, im, None, 8, skip, 0, cap, 0x3C, 3, d_wide[:, 1]), want, f"skip {skip}, frames_cap {cap}, frames_stride 3")
    gram.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_nothing_is_read_past_frames_and_every_record_is_written_whole(canary):
    fx, want = chain_ref.planted(), planted_want("weighted", SKIP, 0)
    eng = planted_engine()
    gram = eng.grammar(*GRAMS["weighted"])
    rows = poison_feature_rows(fx["im"].copy(), fx["inf"])
    first = dev_call(eng, gram, rows, fx["inf"], 16, SKIP, 0, 0, canary)
    same(first, want, "poisoned rows")
    assert as_bytes(dev_call(eng, gram, rows, fx["inf"], 16, SKIP, 0, 0, canary)) == as_bytes(first)  # two runs, the same bytes
    n = len(fx["inf"])
    vad = np.full((n, 12), 0x7F7F7F7F, np.uint32)  # sr_vad_rec: frm_num is word 9 of 12
    col = VAD_DTYPE.fields["frm_num"][1] // 4
    vad[:, col] = fx["inf"]
    d = dev(vad)
    same(dev_call(eng, gram, rows, None, 16, SKIP, 0, 0, canary, 12, d[:, col]), want, "counts from vad records")
    out = [np.zeros(n, ref.CHAIN_REC_DTYPE), np.zeros((n, 16), ref.CHAIN_WORD_DTYPE)]
    v = engine._vp
    assert eng.L.sr_decode_onepass_grammar_dp(eng.h, gram.g, v(rows), P(vad.ctypes.data + 4 * col), U32(12), U32(n), U32(0), U32(16), U32(SKIP),
                                              U32(0), v(out[0]), v(out[1])) == 0
    same(out, want, "host, counts from vad records")
    gram.close()
    eng.close()


@pytest.mark.gpu
def test_host_device_and_pcm_forms_agree():
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
    skip = int(np.median(local_dis(mf[0, :n[0]], tm[1, :30])))  # a typical frame distance
    graph = wgram_ref.with_costs(ref.grammar_repeat([range(4)], range(4), 0), np.arange(8) * 37, [0, 11])
    gram = eng.grammar(*graph)
    want = ref.decode(graph, mf, n, tm, tf, None, maxf, 6, skip, 100)
    assert want[0][2]["status"] == ref.CH_NONE and (want[0]["status"] == ref.CH_OK).sum() == 5
    host = eng.decode_onepass_grammar(gram, mf, n, 6, skip, 100)
    same(host, want, "host form")
    d1 = dev_call(eng, gram, mf, n, 6, skip, 100)
    d2 = dev_call(eng, gram, mf, n, 6, skip, 100, 0, 0x3C)
    assert as_bytes(d1) == as_bytes(d2) == as_bytes(host)
    o = eng.decode_onepass_grammar_pcm(gram, pcm, start, end, mid, 6, skip, 100)
    assert as_bytes((o["rec"], o["words"])) == as_bytes(host)
    assert o["mfcc"].tobytes() == mf.tobytes() and np.array_equal(o["frm_num"], n) and np.array_equal(o["status"], st)
    d_rec = torch.empty(B, 4, dtype=torch.int32, device="cuda:0")
    d_words = torch.empty(B, 6, 8, dtype=torch.int32, device="cuda:0")
    eng.decode_onepass_grammar_dev(gram, dev(mf), dev(n), d_rec, d_words, 6, skip, 100)
    torch.cuda.synchronize()
    assert as_bytes((d_rec.cpu().numpy(), d_words.cpu().numpy())) == as_bytes(host)
    gram.close()
    eng.close()


@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing():
    fx = chain_ref.planted()
    n, W = len(fx["inf"]), 4
    eng, other = planted_engine(), planted_engine()
    gram = eng.grammar(*GRAMS["pairs"])
    foreign = other.grammar(*GRAMS["pairs"])
    want = planted_want("pairs", SKIP, 0, W)
    same(dev_call(eng, gram, fx["im"], fx["inf"], W, SKIP), want, "before the refusals")
    d_im, d_inf = dev(fx["im"]), dev(fx["inf"])
    bank = synth.word_bank(2)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 2, [40] * n, seed=5, bank=bank, S=synth.buf_len_for(60)))
    seg = np.array([[4000, 9000]] * n, np.int32)
    mid = np.full(n, 2048, np.uint32)
    sid = torch.cuda.current_stream().cuda_stream
    v = engine._vp

    def refused(g, words_cap=W, skip=SKIP, wc=0, null=None, overlap=None, frames_cap=0, says=None):
        L, h = eng.L, eng.h
        for where in ("cuda:0", None):
            out = dict(rec=guarded_out((n,), ref.CHAIN_REC_DTYPE, 0xA5, 4096, where, "rec"),
                       words=guarded_out((n, 16), ref.CHAIN_WORD_DTYPE, 0xA5, 4096, where, "words"))
            a = dict(mfcc=P(d_im.data_ptr()) if where else v(fx["im"]), frames=P(d_inf.data_ptr()) if where else v(fx["inf"]),
                     rec=P(out["rec"].ptr), words=P(out["words"].ptr), gram=g)
            if null:
                a[null] = None
            if overlap:
                a[overlap[0]] = P(out[overlap[1]].ptr + overlap[2])
            args = (U32(words_cap), U32(skip), U32(wc), a["rec"], a["words"])
            if where:
                assert L.sr_decode_onepass_grammar_dp_dev(h, a["gram"], a["mfcc"], a["frames"], U32(1), U32(n), U32(frames_cap), *args, P(sid)) == BAD_ARG
                torch.cuda.synchronize()
            else:
                assert L.sr_decode_onepass_grammar_dp(h, a["gram"], a["mfcc"], a["frames"], U32(1), U32(n), U32(frames_cap), *args) == BAD_ARG
                if null not in ("mfcc", "frames") and not overlap and not frames_cap:
                    S = pcm.shape[1]
                    assert L.sr_decode_onepass_grammar_batch(h, a["gram"], v(pcm), U64(S), U32(S), U32(n), v(seg[:, 0].copy()), v(seg[:, 1].copy()),
                                                             v(mid), *args, None, None, None) == BAD_ARG
            assert says is None or says in L.sr_last_error(), L.sr_last_error()
            for x in out.values():
                x.check_untouched()

    for null in ("mfcc", "frames", "rec", "words", "gram"):
        refused(gram.g, null=null)
    refused(gram.g, words_cap=0)
    refused(gram.g, overlap=("words", "rec", 16), says=b"overlap")
    refused(foreign.g, says=b"another engine")
    # the cost bound: 160 frames / L = 32 words of word cost 2^24 and arc cost 2^24 are 2^30 exactly; a final cost of 1 is
    # past it, and an arc cost smaller by one is within it again
    n_arcs, big, fin1 = len(PAIRS[1]), 1 << 24, [0, 1, 0, 0, 0, 0]
    for arc, fin, ok, cap in ((big, None, True, 0), (big, fin1, False, 0), (big - 1, fin1, True, 0), (big, fin1, True, 20)):
        graph = wgram_ref.with_costs(PAIRS, [arc] * n_arcs, fin)
        g = eng.grammar(*graph)
        if ok:
            same(dev_call(eng, g, fx["im"], fx["inf"], W, SKIP, big, cap),
                 ref.decode(graph, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, SKIP, big, frames_cap=cap), f"within the bound: {arc}, {fin}, {cap}")
        else:
            refused(g.g, wc=big, says=b"2^30")
            with pytest.raises(ValueError):
                ref.decode(graph, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, SKIP, big)
        g.close()
    same(dev_call(eng, gram, fx["im"], fx["inf"], W, SKIP), want, "after the refusals")
    # a grammar goes stale with the store and with the word map
    eng.set_word_map(None, 1)
    refused(gram.g, says=b"word map")
    gram.close()
    gram = eng.grammar(*GRAMS["pairs"])
    same(dev_call(eng, gram, fx["im"], fx["inf"], W, SKIP), want, "compiled again")
    eng.set_templates_dense(fx["tm"], fx["tf"])
    refused(gram.g, says=b"template store")
    for g in (gram, foreign):
        g.close()
    eng.close()
    other.close()


@pytest.mark.gpu
def test_a_single_row_over_the_group_budget_is_refused():
    """63 positions x 2 000 slots of up to 150 frames: 126 000 saved columns of 2 400 bytes each exceed a launch group's 256 MiB"""
    Kb, rows, maxf = 2000, 150, 64
    rng = np.random.default_rng(3)
    tm = rng.integers(-50, 51, (Kb, rows + 1, 12)).astype(np.int16)
    tf = np.full(Kb, 40, np.uint32)
    tf[0] = rows
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    eng.set_word_map(np.arange(Kb, dtype=np.uint32) % 20)
    big = eng.grammar(*wgram_ref.grammar_sequence([range(20)] * 63))
    pl = engine.onepass_grammar_plan(big)
    assert pl["kept_items"] == 63 * Kb and pl["row_bytes"] == 64 * (maxf + 1) * 12 + 63 * Kb * rows * 16 > 256 << 20 and pl["rows"] == 0
    im = np.zeros((1, maxf, 12), np.int16)
    inf = np.array([maxf], np.uint32)
    for where in ("cuda:0", None):
        g_r = guarded_out((1,), ref.CHAIN_REC_DTYPE, 0xA5, 4096, where, "rec")
        g_w = guarded_out((1, 4), ref.CHAIN_WORD_DTYPE, 0xA5, 4096, where, "words")
        if where:
            d_im, d_inf = dev(im), dev(inf)
            rc = eng.L.sr_decode_onepass_grammar_dp_dev(eng.h, big.g, P(d_im.data_ptr()), P(d_inf.data_ptr()), U32(1), U32(1), U32(0), U32(4),
                                                        U32(SKIP), U32(0), P(g_r.ptr), P(g_w.ptr), None)
            torch.cuda.synchronize()
        else:
            rc = eng.L.sr_decode_onepass_grammar_dp(eng.h, big.g, engine._vp(im), engine._vp(inf), U32(1), U32(1), U32(0), U32(4), U32(SKIP), U32(0),
                                                    P(g_r.ptr), P(g_w.ptr))
        assert rc == BAD_ARG and b"row_bytes = %d" % pl["row_bytes"] in eng.L.sr_last_error()
        g_r.check_untouched()
        g_w.check_untouched()
    big.close()
    small = eng.grammar(*wgram_ref.grammar_sequence([range(20)] * 2))  # the same store under a grammar that fits
    assert engine.onepass_grammar_plan(small)["rows"] >= 1
    rec, _ = eng.decode_onepass_grammar(small, im, inf, 4, SKIP)
    assert rec[0]["status"] in (ref.CH_OK, ref.CH_NONE)
    small.close()
    eng.close()
