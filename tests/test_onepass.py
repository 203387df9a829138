"""One-pass connected-word decoding: one prefix-cost array over all word counts, built in blocks (include/sr_engine.h,
"one-pass connected-word decoding").

The definition lives in tests/onepass_ref.py (plain Python; its own checks are tests/test_onepass_ref.py).  Every comparison
here is bit for bit against it: records and word rows, no tolerances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_ref
import onepass_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import DIS_ERR, VAD_DTYPE, Engine

BAD_CONFIG, BAD_ARG, NO_TEMPLATES = 2, 3, 4
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
MAXF = chain_ref.PLANT_MAXF
SKIP = chain_ref.PLANT_SKIP
ONES = 0xFFFFFFFF


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


def dev_call(eng, im, frames, words_cap, skip=None, word_cost=0, frames_cap=0, canary=0xA5, frames_stride=1, d_frames=None):
    """sr_decode_onepass_dp_dev into guarded buffers whose every byte starts as the canary -> (rec, words)"""
    n = len(im)
    d_im = dev(im)
    if d_frames is None:
        d_frames = dev(np.ascontiguousarray(frames, dtype=np.uint32))
    g_r = guarded_out((n,), ref.CHAIN_REC_DTYPE, canary, 4096, "cuda:0", "rec")
    g_w = guarded_out((n, words_cap), ref.CHAIN_WORD_DTYPE, canary, 4096, "cuda:0", "words")
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_decode_onepass_dp_dev(eng.h, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(frames_stride), U32(n), U32(frames_cap),
                                        U32(words_cap), U32(skip_arg(skip)), U32(word_cost), P(g_r.ptr), P(g_w.ptr), P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_r.check()
    g_w.check()
    return g_r.interior(), g_w.interior()


class hooks:
    """development hooks "onepass_block" / "onepass_rows" (testing library only; read per call)"""

    def __init__(self, block=0, rows=0):
        self.v = dict(onepass_block=block, onepass_rows=rows)

    def __enter__(self):
        for k, v in self.v.items():
            engine.dev_hook(k, v)

    def __exit__(self, *exc):
        for k in self.v:
            engine.dev_hook(k, 0)


@functools.lru_cache(maxsize=None)
def planted_want(skip, wc, words_cap=16):
    fx = chain_ref.planted()
    want = ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, words_cap, skip, wc)
    for a in want:
        a.setflags(write=False)
    return want


def planted_engine(**kw):
    fx = chain_ref.planted()
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


@functools.lru_cache(maxsize=None)
def long_want(skip):
    fx = ref.planted_long()
    want = ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, ref.LONG_MAXF, 64, skip, 0)
    for a in want:
        a.setflags(write=False)
    return want


# ---- GPU 1: the planted rows, against the restatement and against level building -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wc", [0, 5000])
@pytest.mark.parametrize("skip", [SKIP, None, 300])
def test_planted_rows(skip, wc):
    fx, want = chain_ref.planted(), planted_want(skip, wc)
    eng = planted_engine()
    rec, words = dev_call(eng, fx["im"], fx["inf"], 16, skip, wc)
    same((rec, words), want, f"skip {skip}, word_cost {wc}")
    if skip == SKIP:
        assert rec["n_words"].tolist() == [len(s) for s in fx["seq"]]
        assert [words[r, :len(s)]["slot"].tolist() for r, s in enumerate(fx["seq"])] == fx["seq"]
    # the engine's own level building at max_words 16: where a level holds the minimum, cost, count and word rows are its
    l_rec, l_words, _ = eng.decode_words(fx["im"], fx["inf"], 16, 0, skip, wc)
    compared = 0
    for r in range(len(rec)):
        if l_rec[r]["status"] != ref.CH_OK:
            assert rec[r]["status"] == ref.CH_NONE or rec[r]["n_words"] == 0, r
            continue
        assert rec[r]["status"] == ref.CH_OK and rec[r]["cost"] <= l_rec[r]["cost"], r
        if rec[r]["cost"] == l_rec[r]["cost"]:
            n = int(rec[r]["n_words"])
            assert n == l_rec[r]["n_words"] and words[r, :n].tobytes() == l_words[r, :n].tobytes(), r
            compared += 1
        else:  # cheaper than every level: filler alone
            assert rec[r]["n_words"] == 0 and rec[r]["cost"] == int(fx["inf"][r]) * skip, r
    assert compared == 12 or skip == 300, compared  # (at skip 300 filler beats most words)
    eng.close()


# ---- GPU 2: more words than level building holds ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_planted_long_rows_of_17_to_40_words():
    fx = ref.planted_long()
    eng = Engine(max_frames=ref.LONG_MAXF, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    rec, words = dev_call(eng, fx["im"], fx["inf"], 64, SKIP)
    same((rec, words), long_want(SKIP), "planted_long, skip on")
    assert np.all(rec["status"] == ref.CH_OK) and rec["n_words"].tolist() == list(ref.LONG_COUNTS) and min(ref.LONG_COUNTS) > 16
    for r, seq in enumerate(fx["seq"]):
        assert words[r, :len(seq)]["slot"].tolist() == seq, r
        assert [(int(w["start"]), int(w["end"])) for w in words[r, :len(seq)]] == fx["spans"][r], r
    same(dev_call(eng, fx["im"], fx["inf"], 64, None), long_want(None), "planted_long, skip off")  # (more words: bytes only)
    same(eng.decode_onepass(fx["im"], fx["inf"], 64, SKIP), long_want(SKIP), "planted_long, host form")
    eng.close()


# ---- GPU 3: seams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_block_length_and_group_size_gives_identical_bytes():
    fx, want = chain_ref.planted(), planted_want(SKIP, 0)
    L = ref.reach(fx["tf"])
    assert L == 5
    eng = planted_engine(testing=True)
    first = as_bytes(dev_call(eng, fx["im"], fx["inf"], 16, SKIP))
    for block, rows in ((1, 0), (2, 0), (3, 0), (L, 0), (0, 1), (0, 5), (2, 5)):
        with hooks(block, rows):
            g = engine.decode_onepass_geometry(14, 5, MAXF, int(fx["tf"].min()), testing=True)
            assert g["block"] == (block or L) and (not rows or g["rows"] == rows)
            got = dev_call(eng, fx["im"], fx["inf"], 16, SKIP)
        same(got, want, f"block {block}, rows {rows}")
        assert as_bytes(got) == first, (block, rows)
    eng.close()


@functools.lru_cache(maxsize=None)
def wide_fixture():
    """K = 3 templates of 70..90 frames: L >= 36, a block's sweep spans more than 64 columns; two rows of 300 frames"""
    rng = np.random.default_rng(77)
    tf = np.array([70, 80, 90], np.uint32)
    tm = np.zeros((3, 91, 12), np.int16)
    for k in range(3):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    im = rng.integers(-3000, 3001, (2, 320, 12)).astype(np.int16)  # what is not a word is loud noise
    for r, order in enumerate(((1, 0, 2), (2, 2, 0))):
        at = 3 + r
        for k in order:
            n = int(tf[k])
            im[r, at:at + n] = tm[k, :n] + rng.integers(-60, 61, (n, 12))
            at += n + 2
        assert at <= 300
    inf = np.array([300, 300], np.uint32)
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf)


@pytest.mark.gpu
def test_sweeps_of_more_than_64_columns_hand_their_boundary_on():
    fx = wide_fixture()
    L = ref.reach(fx["tf"])
    assert L == 36 and 2 * L - 1 > 64  # columns (c0_prev, cN) of one block
    eng = Engine(max_frames=320, device=0, testing=True)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    for skip in (4000, None):
        want = ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, 320, 8, skip, 0)
        if skip:
            assert want[0]["n_words"].tolist() == [3, 3] and want[1][:, :3]["slot"].tolist() == [[1, 0, 2], [2, 2, 0]]
        got = dev_call(eng, fx["im"], fx["inf"], 8, skip)
        same(got, want, f"wide store, skip {skip}")
        with hooks(block=33):
            assert as_bytes(dev_call(eng, fx["im"], fx["inf"], 8, skip)) == as_bytes(got)
    eng.close()


# ---- GPU 4: truncation -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_truncation_reports_the_true_count_and_writes_the_first_words():
    fx = chain_ref.planted()
    eng = planted_engine()
    full = dev_call(eng, fx["im"], fx["inf"], 64, SKIP)
    same(full, planted_want(SKIP, 0, 64), "words_cap 64")
    assert np.all(full[1][:, 4:].view(np.uint32) == ONES)  # at most four words a row: the tail is all ones
    cut = dev_call(eng, fx["im"], fx["inf"], 2, SKIP)
    same(cut, planted_want(SKIP, 0, 2), "words_cap 2")
    four = np.nonzero(full[0]["n_words"] == 4)[0]
    assert len(four) == 3 and np.all(cut[0]["status"][four] == ref.CH_TRUNCATED) and np.all(cut[0]["n_words"][four] == 4)
    assert cut[1].tobytes() == full[1][:, :2].tobytes() and np.array_equal(cut[0]["cost"], full[0]["cost"])
    assert np.array_equal(cut[0]["skipped"], full[0]["skipped"])
    one = dev_call(eng, fx["im"], fx["inf"], 1, SKIP)
    same(one, planted_want(SKIP, 0, 1), "words_cap 1")
    eng.close()


# ---- GPU 5: edges, rows of one call with different N -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_edges_in_one_call():
    fx = chain_ref.planted()
    rng = np.random.default_rng(31)
    inf = np.array([0, 3, 4, 5, 6, int(fx["inf"][3]), int(fx["inf"][7]), 5000, 161, 97, 98, 101], np.uint32)
    im = fx["im"].copy()
    im[7] = rng.integers(-3000, 3001, (MAXF, 12))  # the clamped rows have frames up to the cap
    im[8, 60:] = im[3, :100]
    valid = np.array([1, 0, 1, 1, 1], np.uint8)
    L = ref.reach(fx["tf"], valid)
    assert L == int(min(m for k, m in enumerate(fx["tf"]) if valid[k])) // 2 + 1 and inf[1] < L
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"], valid)
    wide = np.full((len(inf), 3), 0x7F7F7F7F, np.uint32)
    wide[:, 1] = inf
    d_wide = dev(wide)
    for skip in (SKIP, None):
        for cap in (0, 97, 5000):
            want = ref.decode(im, inf, fx["tm"], fx["tf"], valid, MAXF, 8, skip, 0, frames_cap=cap)
            rec = want[0]
            assert tuple(rec[0]) == (DIS_ERR, 0, 0, ref.CH_NONE)  # N = 0
            for r in (1, 2):  # shorter than any word's reach
                assert tuple(rec[r]) == ((int(inf[r]) * skip, 0, int(inf[r]), ref.CH_OK) if skip else (DIS_ERR, 0, 0, ref.CH_NONE)), r
            assert not np.any(want[1]["slot"] == 1)  # the invalid slot ends no word
            if skip:
                assert rec[7]["status"] == ref.CH_OK and rec[7]["cost"] > 0
                top = min(MAXF, cap or MAXF)
                for r in range(len(inf)):
                    n = int(rec[r]["n_words"])
                    assert rec[r]["skipped"] + sum(int(w["end"]) - int(w["start"]) + 1 for w in want[1][r, :n]) == min(int(inf[r]), top), r
            same(dev_call(eng, im, inf, 8, skip, 0, cap), want, f"skip {skip}, frames_cap {cap}")
            same(dev_call(eng, im, None, 8, skip, 0, cap, 0x3C, 3, d_wide[:, 1]), want, f"skip {skip}, frames_cap {cap}, frames_stride 3")
    assert inf[5] % L and inf[6] % L  # rows that end inside a block
    eng.close()


# ---- GPU 6: cross-check with the span scorer ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_word_costs_what_the_span_scorer_says():
    n_checked = 0
    for fx, maxf, want in ((chain_ref.planted(), MAXF, planted_want(SKIP, 0)), (ref.planted_long(), ref.LONG_MAXF, long_want(SKIP))):
        eng = Engine(max_frames=maxf, device=0)
        eng.set_templates_dense(fx["tm"], fx["tf"])
        rec, words = dev_call(eng, fx["im"], fx["inf"], want[1].shape[1], SKIP)
        same((rec, words), want, "before the cross-check")
        for w0 in range(0, int(rec["n_words"].max()), 16):  # the span scorer takes 16 spans a row at most
            part = np.ascontiguousarray(words[:, w0:w0 + 16])
            sc = eng.score_word_spans(fx["im"], fx["inf"], part, 0)
            for r in range(len(rec)):
                for i in range(max(0, min(16, int(rec[r]["n_words"]) - w0))):
                    assert sc[r, i, int(part[r, i]["slot"])] == part[r, i]["acc"], (r, w0 + i)
                    n_checked += 1
        eng.close()
    assert n_checked == 30 + sum(ref.LONG_COUNTS)


# ---- GPU 7: contracts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_nothing_is_read_past_frames_and_every_record_is_written_whole(canary):
    fx, want = chain_ref.planted(), planted_want(SKIP, 0)
    eng = planted_engine()
    rec = poison_feature_rows(fx["im"].copy(), fx["inf"])
    first = dev_call(eng, rec, fx["inf"], 16, SKIP, 0, 0, canary)
    same(first, want, "poisoned rows")
    assert as_bytes(dev_call(eng, rec, fx["inf"], 16, SKIP, 0, 0, canary)) == as_bytes(first)  # two runs, the same bytes
    n = len(fx["inf"])
    vad = np.full((n, 12), 0x7F7F7F7F, np.uint32)  # sr_vad_rec: frm_num is word 9 of 12
    col = VAD_DTYPE.fields["frm_num"][1] // 4
    vad[:, col] = fx["inf"]
    d = dev(vad)
    same(dev_call(eng, rec, None, 16, SKIP, 0, 0, canary, 12, d[:, col]), want, "counts from vad records")
    out = [np.zeros(n, ref.CHAIN_REC_DTYPE), np.zeros((n, 16), ref.CHAIN_WORD_DTYPE)]
    v = engine._vp
    assert eng.L.sr_decode_onepass_dp(eng.h, v(rec), P(vad.ctypes.data + 4 * col), U32(12), U32(n), U32(0), U32(16), U32(SKIP), U32(0),
                                      v(out[0]), v(out[1])) == 0
    same(out, want, "host, counts from vad records")
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
    skip = int(np.median(ref.local_dis(mf[0, :n[0]], tm[1, :30])))  # a typical frame distance
    want = ref.decode(mf, n, tm, tf, None, maxf, 6, skip, 100)
    assert want[0][2]["status"] == ref.CH_NONE and (want[0]["status"] == ref.CH_OK).sum() == 5
    assert 0 in want[1][0, :want[0][0]["n_words"]]["slot"]  # the piece of row 0 is found in row 0
    host = eng.decode_onepass(mf, n, 6, skip, 100)
    same(host, want, "host form")
    d1 = dev_call(eng, mf, n, 6, skip, 100)
    d2 = dev_call(eng, mf, n, 6, skip, 100, 0, 0x3C)
    assert as_bytes(d1) == as_bytes(d2) == as_bytes(host)
    o = eng.decode_onepass_pcm(pcm, start, end, mid, 6, skip, 100)
    assert as_bytes((o["rec"], o["words"])) == as_bytes(host)
    assert o["mfcc"].tobytes() == mf.tobytes() and np.array_equal(o["frm_num"], n) and np.array_equal(o["status"], st)
    r2, w2 = np.zeros_like(host[0]), np.zeros_like(host[1])  # every optional output NULL
    v, S = engine._vp, pcm.shape[1]
    assert eng.L.sr_decode_onepass_batch(eng.h, v(pcm), U64(S), U32(S), U32(B), v(start), v(end), v(mid), U32(6), U32(skip), U32(100), v(r2),
                                         v(w2), None, None, None) == 0
    assert r2.tobytes() == host[0].tobytes() and w2.tobytes() == host[1].tobytes()
    d_rec = torch.empty(B, 4, dtype=torch.int32, device="cuda:0")
    d_words = torch.empty(B, 6, 8, dtype=torch.int32, device="cuda:0")
    eng.decode_onepass_dev(dev(mf), dev(n), d_rec, d_words, 6, skip, 100)
    torch.cuda.synchronize()
    assert as_bytes((d_rec.cpu().numpy(), d_words.cpu().numpy())) == as_bytes(host)
    eng.close()


@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing():
    maxf, n, W = 1000, 2, 4
    cap = engine.decode_geometry(10, maxf, W)["max_tpl_rows"]
    rng = np.random.default_rng(980)
    tm = np.zeros((2, cap + 2, 12), np.int16)
    tm[:, :cap + 1] = rng.integers(-2, 3, (2, cap + 1, 12))
    im = rng.integers(-2, 3, (n, maxf, 12)).astype(np.int16)
    inf = np.array([300, 90], np.uint32)
    tf = np.array([28, 40], np.uint32)  # L = 15: 66 words in 1000 frames at most
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    want = ref.decode(im, inf, tm, tf, None, maxf, W, 3, 0)
    same(dev_call(eng, im, inf, W, 3), want, "before the refusals")
    d_im, d_inf = dev(im), dev(inf)
    bank = synth.word_bank(2)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(n), [40, 40], seed=5, bank=bank, S=synth.buf_len_for(60)))
    seg = np.array([[4000, 9000]] * n, np.int32)
    mid = np.full(n, 2048, np.uint32)
    sid = torch.cuda.current_stream().cuda_stream
    v = engine._vp

    def refused(e, code, stride=1, frames_cap=0, words_cap=W, skip=3, wc=0, null=None, overlap=None, whole=True):
        L, h = e.L, e.h
        for where in ("cuda:0", None):
            g = dict(rec=guarded_out((n,), ref.CHAIN_REC_DTYPE, 0xA5, 4096, where, "rec"),
                     words=guarded_out((n, 16), ref.CHAIN_WORD_DTYPE, 0xA5, 4096, where, "words"))
            a = dict(mfcc=P(d_im.data_ptr()) if where else v(im), frames=P(d_inf.data_ptr()) if where else v(inf),
                     rec=P(g["rec"].ptr), words=P(g["words"].ptr))
            if null:
                a[null] = None
            if overlap:
                a[overlap[0]] = P(g[overlap[1]].ptr + overlap[2])
            args = (U32(words_cap), U32(skip), U32(wc), a["rec"], a["words"])
            if where:
                assert L.sr_decode_onepass_dp_dev(h, a["mfcc"], a["frames"], U32(stride), U32(n), U32(frames_cap), *args, P(sid)) == code
                torch.cuda.synchronize()
            else:
                assert L.sr_decode_onepass_dp(h, a["mfcc"], a["frames"], U32(stride), U32(n), U32(frames_cap), *args) == code
                if whole and null not in ("mfcc", "frames") and not overlap:
                    S = pcm.shape[1]
                    assert L.sr_decode_onepass_batch(h, v(pcm), U64(S), U32(S), U32(n), v(seg[:, 0].copy()), v(seg[:, 1].copy()), v(mid), *args,
                                                     None, None, None) == code
            for x in g.values():
                x.check_untouched()

    for null in ("mfcc", "frames", "rec", "words"):
        refused(eng, BAD_ARG, null=null)
    refused(eng, BAD_ARG, stride=0, whole=False)  # (the whole path has no such argument)
    refused(eng, BAD_ARG, words_cap=0)
    refused(eng, BAD_ARG, skip=65536)
    refused(eng, BAD_ARG, skip=DIS_ERR - 1)
    refused(eng, BAD_ARG, wc=(1 << 24) + 1)
    refused(eng, BAD_ARG, wc=(1 << 30) // 66 + 1)  # the word-cost bound: below 2^24, but 66 words of it exceed 2^30
    assert b"2^30" in eng.L.sr_last_error()
    refused(eng, BAD_ARG, overlap=("words", "rec", 16))  # the word rows begin inside the records
    assert b"overlap" in eng.L.sr_last_error()
    eng.set_word_map(np.array([1, 2, 3], np.uint32))     # a stale map: made for another store
    refused(eng, BAD_ARG)
    eng.set_word_map(None, 1)
    eng.set_templates_dense(tm, np.array([cap + 1, 40], np.uint32))  # one row more than fits
    refused(eng, BAD_ARG)
    assert b"too long" in eng.L.sr_last_error()
    eng.set_templates_dense(tm, tf)
    same(dev_call(eng, im, inf, W, 3), want, "after the refusals")
    # the limits themselves are accepted: the bound at this store, and the whole word cost where frames_cap keeps the words few
    at = (1 << 30) // 66
    assert at < 1 << 24
    same(dev_call(eng, im[1:], inf[1:], 16, None, at), ref.decode(im[1:], inf[1:], tm, tf, None, maxf, 16, None, at), "at the bound")
    lim = ref.decode(im[1:], inf[1:], tm, tf, None, maxf, 16, 65535, 1 << 24, frames_cap=90)
    same(dev_call(eng, im[1:], inf[1:], 16, 65535, 1 << 24, 90), lim, "at the limits")
    eng.close()
    e2 = Engine(max_frames=maxf, device=0)  # no templates
    refused(e2, NO_TEMPLATES)
    e2.close()
    e3 = Engine(max_frames=maxf, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    refused(e3, BAD_CONFIG)
    e3.close()
