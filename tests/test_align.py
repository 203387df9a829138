"""Full-DP alignment and DBA training on the GPU (include/sr_engine.h, "full-DP alignment and word models from many examples").

The definition lives in tests/align_ref.py (numpy; tests/test_align_ref.py checks it against the scorer's oracle and against an
exhaustive enumeration).  Everything here is compared with it bit for bit: records, span rows, centroids, statistics.  A case
is a list of (N, R, kind) pairs, one reference per pair; kind "rand" draws both sequences, "const" makes both constant (every
cell of the pair ties), "same" makes the row a copy of its reference.  Small coefficients (amp 2) make ties common, amp 3000 is
the usual range, amp 32767 holds coefficients beyond +-16383, which the full-DP scorer sends down another kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import align_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine

BAD_CONFIG, BAD_ARG = 2, 3
U32, P = C.c_uint32, C.c_void_p


class hooks:
    """development hooks "align_pairs" / "align_marks_global" (testing library only; read per call)"""

    def __init__(self, pairs=0, marks_global=0):
        self.v = dict(align_pairs=pairs, align_marks_global=marks_global)

    def __enter__(self):
        for k, v in self.v.items():
            engine.dev_hook(k, v)

    def __exit__(self, *exc):
        for k in self.v:
            engine.dev_hook(k, 0)


def dev(a):
    """a device copy of a numpy array (fixtures are read-only: copy first)"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def same_rec(got, want, what, pairs=None):
    g, w = np.asarray(got).view(np.uint32).reshape(-1, 4), np.asarray(want).view(np.uint32).reshape(-1, 4)
    bad = np.nonzero(np.any(g != w, 1))[0]
    if len(bad):
        r = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} records differ, first at row {r}"
                             f"{' ' + str(pairs[r]) if pairs else ''}: got {g[r].tolist()} want {w[r].tolist()}")


def same_span(got, want, what, pairs=None):
    bad = np.nonzero(np.any(got != want, 1))[0]
    if len(bad):
        r = int(bad[0])
        x = int(np.nonzero(got[r] != want[r])[0][0])
        raise AssertionError(f"{what}: {len(bad)} span rows differ, first at row {r}{' ' + str(pairs[r]) if pairs else ''}, frame {x}: "
                             f"got {got[r, x]:#x} want {want[r, x]:#x}")


def build_case(pairs, amp, maxf, ref_rows, seed):
    """-> dict(mfcc [n, maxf, 12], frames [n], ref [n, ref_rows, 12], ref_frames [n], pairs) + the expected rec / span.  N and R
    are the counts handed to the library as they are: N above maxf, R = 0 and R above ref_rows are cases"""
    rng = np.random.default_rng(seed)
    n = len(pairs)
    mfcc = rng.integers(-amp, amp + 1, (n, maxf, 12)).astype(np.int16)
    rf = rng.integers(-amp, amp + 1, (n, ref_rows, 12)).astype(np.int16)
    for r, (N, R, kind) in enumerate(pairs):
        if kind == "const":
            mfcc[r], rf[r] = amp, (amp if r % 2 else -amp)
        elif kind == "same":
            mfcc[r, :min(R, maxf)] = rf[r, :min(R, maxf)]
    frames, ref_frames = np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)
    rec, span, _ = ref.align(mfcc, frames, rf, ref_frames)
    out = dict(mfcc=mfcc, frames=frames, ref=rf, ref_frames=ref_frames, rec=rec, span=span)
    for a in out.values():
        a.setflags(write=False)
    out["pairs"] = pairs
    return out


def dev_align(eng, fx, canary=0xA5, ref_of_row=None, want_span=True, frames_stride=1, d_frames=None, mfcc=None, rf=None):
    """sr_dtw_dp_align_dev into guarded buffers -> (rec ALIGN_DTYPE [n], span uint32 [n, max_frames] or None)"""
    n = len(fx["frames"])
    d_im, d_rf, d_rn = dev(fx["mfcc"] if mfcc is None else mfcc), dev(fx["ref"] if rf is None else rf), dev(fx["ref_frames"])
    if d_frames is None:
        d_frames = dev(fx["frames"])
    d_map = None if ref_of_row is None else dev(np.asarray(ref_of_row, dtype=np.uint32))
    g_rec = guarded_out((n,), ref.ALIGN_DTYPE, canary, 4096, "cuda:0", "rec")
    g_span = guarded_out((n, eng.max_frames), np.uint32, canary, 4096, "cuda:0", "span")
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_dtw_dp_align_dev(eng.h, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(frames_stride), U32(n), P(d_rf.data_ptr()),
                                   P(d_rn.data_ptr()), U32(d_rf.shape[1]), U32(d_rf.shape[0]), None if d_map is None else P(d_map.data_ptr()),
                                   P(g_rec.ptr), P(g_span.ptr) if want_span else None, P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_rec.check()
    g_span.check() if want_span else g_span.check_untouched()
    return g_rec.interior(), g_span.interior() if want_span else None


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
EDGE_MAXF, EDGE_ROWS = 130, 131
EDGE_N, EDGE_R = (1, 2, 63, 64, 65, 128, 130), (1, 2, 15, 16, 17, 33, 65)  # sweep seams and the boundary column; mark-word packing
EDGE_PAIRS = tuple(
    [(N, R, "rand") for N in EDGE_N for R in EDGE_R]
    # the gate's edges: N = 2R passes, 2R + 1 does not; 2N = R passes, 2N = R - 1 does not
    + [(66, 33, "rand"), (67, 33, "rand"), (32, 16, "rand"), (33, 16, "rand"), (8, 16, "rand"), (8, 17, "rand"), (65, 130, "rand"), (64, 129, "rand")]
    # dtw_limit's switch columns X1 = (2R - N) / 3, X2 = (4N - 2R) / 3 (1-based) on lanes 63 and 0 of a sweep
    + [(68, 130, "rand"), (65, 130, "const"), (80, 64, "rand"), (81, 64, "rand"), (128, 128, "rand"), (129, 96, "rand")]
    # every cell ties; identical sequences; empty rows; invalid references
    + [(64, 64, "const"), (65, 33, "const"), (100, 130, "const"), (130, 65, "const"), (1, 1, "const"), (2, 3, "const")]
    + [(65, 65, "same"), (130, 130, "same"), (17, 17, "same"), (1, 1, "same")]
    + [(0, 10, "rand"), (10, 0, "rand"), (0, 0, "rand"), (10, 132, "rand"), (300, 70, "rand"), (66, 131, "rand")])


@functools.lru_cache(maxsize=None)
def edge_fixture(amp):
    fx = build_case(EDGE_PAIRS, amp, EDGE_MAXF, EDGE_ROWS, 500 + amp)
    st = {p: int(fx["rec"][i]["status"]) for i, p in enumerate(EDGE_PAIRS)}
    X = lambda N, R: ((2 * R - N) // 3, (4 * N - 2 * R) // 3)  # noqa: E731
    assert X(68, 130)[0] == 64 and X(65, 130)[0] == 65 and X(80, 64)[1] == 64 and X(81, 64)[1] == 65 and X(129, 96)[1] == 108 and X(128, 128)[0] == 42
    assert st[(66, 33, "rand")] == st[(8, 16, "rand")] == st[(65, 130, "rand")] == ref.OK
    assert st[(67, 33, "rand")] == st[(8, 17, "rand")] == st[(64, 129, "rand")] == st[(33, 16, "rand")] == ref.GATED
    assert st[(0, 10, "rand")] == st[(10, 0, "rand")] == st[(10, 132, "rand")] == ref.GATED and st[(66, 131, "rand")] == ref.OK
    assert st[(300, 70, "rand")] == ref.OK  # clamped to 130 frames
    i = EDGE_PAIRS.index((130, 130, "same"))
    assert tuple(fx["rec"][i]) == (0, 0, 130, ref.OK) and np.array_equal(fx["span"][i], np.arange(130) * 0x10001)
    assert (fx["rec"]["status"] == ref.OK).sum() >= 30 and (fx["rec"]["status"] == ref.GATED).sum() >= 20
    return fx


LONG_MAXF, LONG_ROWS = 1100, 1024
LONG_PAIRS = ((0, 65, "rand"), (1050, 600, "rand"), (5000, 1024, "rand"), (1025, 1024, "rand"), (1024, 600, "rand"), (1000, 1024, "rand"),
              (130, 65, "rand"), (65, 65, "same"), (1024, 1024, "const"), (1024, 511, "rand"))


@functools.lru_cache(maxsize=None)
def long_fixture():
    fx = build_case(LONG_PAIRS, 2, LONG_MAXF, LONG_ROWS, 600)
    assert fx["rec"]["status"].tolist() == [ref.GATED, ref.TOO_LONG, ref.TOO_LONG, ref.TOO_LONG, ref.OK, ref.OK, ref.OK, ref.OK, ref.OK, ref.GATED]
    return fx


# ---- GPU 1: one case per place the kernel can go wrong ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("amp", [2, 3000, 32767])
def test_length_edges_records_and_spans(amp):
    fx = edge_fixture(amp)
    assert engine.align_geometry(EDGE_MAXF, EDGE_ROWS)["scratch_bytes"] == 0  # these shapes keep their marks in LDS ...
    eng = Engine(max_frames=EDGE_MAXF, device=0, testing=True)
    for marks_global in (0, 1):                                               # ... unless the hook sends them to global scratch
        for canary in CANARIES:
            with hooks(marks_global=marks_global):
                rec, span = dev_align(eng, fx, canary)
            same_rec(rec, fx["rec"], f"global {marks_global}", EDGE_PAIRS)
            same_span(span, fx["span"], f"global {marks_global}", EDGE_PAIRS)
    rec, none = dev_align(eng, fx, want_span=False)  # d_span NULL
    same_rec(rec, fx["rec"], "no span", EDGE_PAIRS)
    h_rec, h_span = eng.align(fx["mfcc"], fx["frames"], fx["ref"], fx["ref_frames"])
    assert h_rec.tobytes() == fx["rec"].tobytes() and h_span.tobytes() == fx["span"].tobytes()
    assert eng.align(fx["mfcc"], fx["frames"], fx["ref"], fx["ref_frames"], want_span=False)[0].tobytes() == fx["rec"].tobytes()
    eng.close()


@pytest.mark.gpu
def test_long_rows_zero_length_and_too_long():
    fx = long_fixture()
    g = engine.align_geometry(LONG_MAXF, LONG_ROWS)
    assert g["scratch_bytes"] == 1024 * 65 * 4 and g["pairs"] == (256 << 20) // g["scratch_bytes"]  # global marks at this size
    eng = Engine(max_frames=LONG_MAXF, device=0)
    rec, span = dev_align(eng, fx)
    same_rec(rec, fx["rec"], "long rows", LONG_PAIRS)
    same_span(span, fx["span"], "long rows", LONG_PAIRS)
    assert np.all(span[1:4] == 0xFFFFFFFF) and np.all(rec["path_len"][1:4] == 0) and np.all(rec["dis"][1:4] == DIS_ERR)
    same_rec(dev_align(eng, fx, 0x3C, want_span=False)[0], fx["rec"], "long rows, no span", LONG_PAIRS)
    eng.close()


# ---- GPU 2: references by index ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ref_of_row_with_repeats_and_an_entry_out_of_range():
    fx = edge_fixture(2)
    n = len(EDGE_PAIRS)
    rng = np.random.default_rng(700)
    idx = rng.integers(0, n, n).astype(np.uint32)
    idx[:4] = (7, 7, n, 0xFFFFFFFF)  # a repeat, and two entries that name no reference
    want_rec, want_span, _ = ref.align(fx["mfcc"], fx["frames"], fx["ref"], fx["ref_frames"], idx)
    assert want_rec["status"][2] == want_rec["status"][3] == ref.GATED and (want_rec["status"] == ref.OK).sum() >= 10
    eng = Engine(max_frames=EDGE_MAXF, device=0)
    rec, span = dev_align(eng, fx, ref_of_row=idx)
    same_rec(rec, want_rec, "ref_of_row")
    same_span(span, want_span, "ref_of_row")
    h_rec, h_span = eng.align(fx["mfcc"], fx["frames"], fx["ref"], fx["ref_frames"], idx)
    assert h_rec.tobytes() == want_rec.tobytes() and h_span.tobytes() == want_span.tobytes()
    eng.close()


# ---- GPU 3: the shipped scorer writes the same dis ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("amp", [3000, 32767])
def test_dis_equals_the_full_dp_scorer_for_every_pair(amp):
    fx = edge_fixture(amp)
    rows = [[p[0] for p in EDGE_PAIRS].index(N) for N in (0, 1, 2, 8, 17, 32, 63, 64, 65, 66, 80, 100, 128, 130)]
    slots = [[p[1] for p in EDGE_PAIRS].index(R) for R in (1, 2, 15, 16, 17, 33, 64, 65, 96, 128, 130)]
    B, K = len(rows), len(slots)
    im, inf = fx["mfcc"][rows], np.minimum(fx["frames"][rows], EDGE_MAXF)
    tm, tf = fx["ref"][slots], fx["ref_frames"][slots]
    eng = Engine(max_frames=EDGE_MAXF, device=0)
    eng.set_templates_dense(tm, tf)
    sc = eng.dtw_dp(im, inf)
    pair_fx = dict(mfcc=np.repeat(im, K, 0), frames=np.repeat(inf, K), ref=tm, ref_frames=tf)
    rec, _ = dev_align(eng, pair_fx, ref_of_row=np.tile(np.arange(K), B), want_span=False)
    assert np.array_equal(rec["dis"].reshape(B, K), sc)
    assert (sc == DIS_ERR).sum() >= 10 and (sc != DIS_ERR).sum() >= 30, ((sc == DIS_ERR).sum(), sc.size)
    assert np.array_equal(rec["status"] == ref.OK, rec["dis"] != DIS_ERR)
    eng.close()


# ---- GPU 4: launch seams -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_call_cut_into_launches_gives_the_single_launch_bytes():
    fx = edge_fixture(2)
    eng = Engine(max_frames=EDGE_MAXF, device=0, testing=True)
    first = None
    for marks_global in (0, 1):
        for pairs in (0, 30, 7, 1000):  # 79 rows: one launch, three, twelve, one
            with hooks(pairs, marks_global):
                assert engine.align_geometry(EDGE_MAXF, EDGE_ROWS, testing=True)["pairs"] == (pairs or ((1 << 20) if not marks_global else (256 << 20) // (130 * 9 * 4)))
                rec, span = dev_align(eng, fx)
            first = first or rec.tobytes() + span.tobytes()
            assert rec.tobytes() + span.tobytes() == first, (marks_global, pairs)
    assert len(EDGE_PAIRS) >= 3 * 30 - 29
    same_rec(rec, fx["rec"], "seams", EDGE_PAIRS)
    eng.close()


# ---- GPU 5: frame counts out of records; nothing read past frames ----------------------------------------------------------
@pytest.mark.gpu
def test_frames_stride_and_poisoned_rows():
    fx = edge_fixture(2)
    n = len(EDGE_PAIRS)
    eng = Engine(max_frames=EDGE_MAXF, device=0)
    im = poison_feature_rows(fx["mfcc"].copy(), np.minimum(fx["frames"], EDGE_MAXF))
    rf = poison_feature_rows(fx["ref"].copy(), np.where(fx["ref_frames"] <= EDGE_ROWS, fx["ref_frames"], 0))
    for stride in (1, 4, 12):
        recs = np.full((n, stride), 0x7F7F7F7F, np.uint32)
        recs[:, stride - 1] = fx["frames"]
        d = dev(recs)
        rec, span = dev_align(eng, fx, frames_stride=stride, d_frames=d[:, stride - 1], mfcc=im, rf=rf)
        same_rec(rec, fx["rec"], f"stride {stride}", EDGE_PAIRS)
        same_span(span, fx["span"], f"stride {stride}", EDGE_PAIRS)
        h_rec, h_span = np.zeros(n, ref.ALIGN_DTYPE), np.zeros((n, EDGE_MAXF), np.uint32)
        assert eng.L.sr_dtw_dp_align(eng.h, engine._vp(im), P(recs.ctypes.data + 4 * (stride - 1)), U32(stride), U32(n), engine._vp(rf),
                                     engine._vp(fx["ref_frames"]), U32(EDGE_ROWS), U32(n), None, engine._vp(h_rec), engine._vp(h_span)) == 0
        assert h_rec.tobytes() == fx["rec"].tobytes() and h_span.tobytes() == fx["span"].tobytes()
    eng.close()


# ---- GPU 6: refusals that write nothing ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_align_refusals_write_nothing():
    fx = edge_fixture(2)
    n = 8
    eng = Engine(max_frames=EDGE_MAXF, device=0)
    d_im, d_fr, d_rf, d_rn = dev(fx["mfcc"][:n]), dev(fx["frames"][:n]), dev(fx["ref"][:n]), dev(fx["ref_frames"][:n])
    sid = torch.cuda.current_stream().cuda_stream

    def refused(e, code, null=None, stride=1, ref_rows=EDGE_ROWS, n_ref=n, overlap=False):
        g_rec = guarded_out((n,), ref.ALIGN_DTYPE, 0xA5, 4096, "cuda:0", "rec")
        g_span = guarded_out((n, EDGE_MAXF), np.uint32, 0xA5, 4096, "cuda:0", "span")
        a = dict(mfcc=P(d_im.data_ptr()), frames=P(d_fr.data_ptr()), ref=P(d_rf.data_ptr()), ref_frames=P(d_rn.data_ptr()), rec=P(g_rec.ptr))
        if null:
            a[null] = None
        span = P(g_rec.ptr + 16) if overlap else P(g_span.ptr)
        assert e.L.sr_dtw_dp_align_dev(e.h, a["mfcc"], a["frames"], U32(stride), U32(n), a["ref"], a["ref_frames"], U32(ref_rows), U32(n_ref),
                                       None, a["rec"], span, P(sid)) == code, (null, stride, ref_rows, n_ref)
        torch.cuda.synchronize()
        g_rec.check_untouched()
        g_span.check_untouched()

    for null in ("mfcc", "frames", "ref", "ref_frames", "rec"):
        refused(eng, BAD_ARG, null=null)
    refused(eng, BAD_ARG, stride=0)
    refused(eng, BAD_ARG, ref_rows=0)
    refused(eng, BAD_ARG, ref_rows=1025)
    refused(eng, BAD_ARG, n_ref=n - 1)  # no d_ref_of_row: one reference per row is needed
    refused(eng, BAD_ARG, n_ref=0)
    refused(eng, BAD_ARG, overlap=True)
    eng.close()
    e3 = Engine(max_frames=EDGE_MAXF, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    refused(e3, BAD_CONFIG)
    e3.close()


# ---- GPU 7: training -------------------------------------------------------------------------------------------------------------
TRAIN_MAXF, TRAIN_ROWS = 80, 50
TRAIN_EX = (45, 20, 70, 33, 52, 41, 64, 30, 44, 25)  # model 0: seven examples (the 20-frame one fails the gate against 45), model 2: three
TRAIN_START = (0, 7, 7, 10)


@functools.lru_cache(maxsize=None)
def train_fixture(amp):
    rng = np.random.default_rng(900 + amp)
    E = len(TRAIN_EX)
    cen = rng.integers(-amp, amp + 1, (3, TRAIN_ROWS, 12)).astype(np.int16)
    cen_frames = np.array([45, 38, TRAIN_ROWS + 5], np.uint32)  # model 1 has no examples, model 2's centroid is invalid
    frames = np.array(TRAIN_EX, np.uint32)
    mfcc = rng.integers(-amp, amp + 1, (E, TRAIN_MAXF, 12)).astype(np.int16)
    for e in range(7):  # the examples of model 0 are warped, noisy copies of one underlying word: the alignment matters
        src = np.minimum(np.arange(frames[e]) * 45 // frames[e], 44)
        mfcc[e, :frames[e]] = cen[0, src] // 2 + rng.integers(-amp // 8 - 1, amp // 8 + 2, (frames[e], 12))
    ex_start = np.array(TRAIN_START, np.uint32)
    want = {n_iter: ref.train(mfcc, frames, ex_start, cen, cen_frames, n_iter) for n_iter in (1, 3)}
    for n_iter, (c, st) in want.items():
        assert st["n_ok"].tolist() == [[6, 0, 0]] * n_iter and st["n_fail"].tolist() == [[1, 0, 3]] * n_iter
        assert np.array_equal(c[1, :38], cen[1, :38]) and np.all(c[1, 38:] == 0) and np.array_equal(c[2], cen[2])
        assert not np.array_equal(c[0, :45], cen[0, :45]) and np.all(c[0, 45:] == 0)
    assert not np.array_equal(want[1][0], want[3][0]) and want[3][1]["acc"][2, 0] < want[3][1]["acc"][0, 0]  # the iterations chain
    for a in (mfcc, frames, ex_start, cen, cen_frames):
        a.setflags(write=False)
    return dict(mfcc=mfcc, frames=frames, ex_start=ex_start, cen=cen, cen_frames=cen_frames, want=want)


def dev_train(eng, fx, n_iter, canary, want_stats=True, mfcc=None, cen=None):
    d_im, d_fr = dev(fx["mfcc"] if mfcc is None else mfcc), dev(fx["frames"])
    d_cen, d_cf = dev(fx["cen"] if cen is None else cen), dev(fx["cen_frames"])
    M = len(fx["cen_frames"])
    g_out = guarded_out(fx["cen"].shape, np.int16, canary, 4096, "cuda:0", "cen_out")
    g_st = guarded_out((n_iter, M), ref.TRAIN_STAT_DTYPE, canary, 4096, "cuda:0", "stats")
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_train_models_dp_dev(eng.h, P(d_im.data_ptr()), P(d_fr.data_ptr()), U32(1), engine._vp(fx["ex_start"]), U32(M),
                                      P(d_cen.data_ptr()), P(d_cf.data_ptr()), U32(fx["cen"].shape[1]), U32(n_iter), P(g_out.ptr),
                                      P(g_st.ptr) if want_stats else None, P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_out.check()
    g_st.check() if want_stats else g_st.check_untouched()
    return g_out.interior(), g_st.interior() if want_stats else None


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [2, 3000])
def test_training_centroids_and_statistics(amp):
    fx = train_fixture(amp)
    eng = Engine(max_frames=TRAIN_MAXF, device=0, testing=True)
    for n_iter in (1, 3):
        want_cen, want_st = fx["want"][n_iter]
        cen, st = dev_train(eng, fx, n_iter, CANARIES[n_iter % 2])
        assert np.array_equal(cen, want_cen), (n_iter, np.argwhere(cen != want_cen)[:4].tolist())
        assert st.tobytes() == want_st.tobytes(), (n_iter, st.tolist(), want_st.tolist())
        again, st2 = dev_train(eng, fx, n_iter, CANARIES[(n_iter + 1) % 2])  # two runs: identical bytes
        assert again.tobytes() == cen.tobytes() and st2.tobytes() == st.tobytes()
        h_cen, h_st = eng.train_models(fx["mfcc"], fx["frames"], fx["ex_start"], fx["cen"], fx["cen_frames"], n_iter)  # the host form
        assert h_cen.tobytes() == cen.tobytes() and h_st.tobytes() == st.tobytes()
        assert dev_train(eng, fx, n_iter, 0xA5, want_stats=False)[0].tobytes() == cen.tobytes()
        with hooks(pairs=4, marks_global=1):  # three launches per iteration, marks in global scratch
            seam, st3 = dev_train(eng, fx, n_iter, 0x3C)
        assert seam.tobytes() == cen.tobytes() and st3.tobytes() == st.tobytes()
    # poison in the rows past the frames of the examples and of the valid centroids (the invalid one is copied through whole)
    im = poison_feature_rows(fx["mfcc"].copy(), fx["frames"])
    pc = fx["cen"].copy()
    poison_feature_rows(pc[:2], fx["cen_frames"][:2])
    cen, st = dev_train(eng, fx, 3, 0xA5, mfcc=im, cen=pc)
    assert np.array_equal(cen, fx["want"][3][0]) and st.tobytes() == fx["want"][3][1].tobytes()
    eng.close()


@pytest.mark.gpu
def test_training_refusals_write_nothing():
    fx = train_fixture(2)
    eng = Engine(max_frames=TRAIN_MAXF, device=0)
    d_im, d_fr, d_cen, d_cf = dev(fx["mfcc"]), dev(fx["frames"]), dev(fx["cen"]), dev(fx["cen_frames"])
    sid = torch.cuda.current_stream().cuda_stream
    M = 3

    def refused(ex_start=TRAIN_START, n_iter=2, cen_rows=TRAIN_ROWS, alias=None, null=None, stride=1, models=M):
        for dev in ("cuda:0", None):
            g_out = guarded_out(fx["cen"].shape, np.int16, 0xA5, 4096, dev, "cen_out")
            g_st = guarded_out((16, M), ref.TRAIN_STAT_DTYPE, 0xA5, 4096, dev, "stats")
            ex = np.array(ex_start, np.uint32)
            if dev:
                a = dict(mfcc=P(d_im.data_ptr()), frames=P(d_fr.data_ptr()), cen=P(d_cen.data_ptr()), cf=P(d_cf.data_ptr()))
            else:
                a = dict(mfcc=engine._vp(fx["mfcc"]), frames=engine._vp(fx["frames"]), cen=engine._vp(fx["cen"]), cf=engine._vp(fx["cen_frames"]))
            a.update(ex=engine._vp(ex), out=P(g_out.ptr), st=P(g_st.ptr))
            if null:
                a[null] = None
            if alias == "in":
                a["cen"] = P(g_out.ptr + 24)  # the input overlaps the output
            if alias == "stats":
                a["st"] = P(g_out.ptr + 8)
            args = (eng.h, a["mfcc"], a["frames"], U32(stride), a["ex"], U32(models), a["cen"], a["cf"], U32(cen_rows), U32(n_iter), a["out"], a["st"])
            rc = eng.L.sr_train_models_dp_dev(*args, P(sid)) if dev else eng.L.sr_train_models_dp(*args)
            assert rc == BAD_ARG, (ex_start, n_iter, cen_rows, alias, null, dev, rc)
            if dev:
                torch.cuda.synchronize()
            g_out.check_untouched()
            g_st.check_untouched()

    # the accumulator bound: examples x min(max_frames, SR_ALIGN_MAX_FRAMES) <= 65 535 -- 819 examples of 80 frames pass, 820 do not
    assert 819 * TRAIN_MAXF <= 65535 < 820 * TRAIN_MAXF
    refused(ex_start=(0, 820, 820, 823))
    refused(ex_start=(0, 3, 3, 823))
    assert b"exact" in eng.L.sr_last_error()
    refused(alias="in")
    refused(alias="stats")
    refused(ex_start=(1, 7, 7, 10))
    refused(ex_start=(0, 7, 6, 10))
    for n_iter in (0, 17):
        refused(n_iter=n_iter)
    for cen_rows in (0, 1025):
        refused(cen_rows=cen_rows)
    refused(stride=0)
    refused(models=0)
    for null in ("mfcc", "frames", "ex", "cen", "cf", "out"):
        refused(null=null)
    cen, st = dev_train(eng, fx, 1, 0xA5)  # and after all the refusals the engine still trains
    assert np.array_equal(cen, fx["want"][1][0])
    eng.close()


# ---- GPU 8: end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_train_words_then_recognise_every_training_take():
    n_words, takes, maxf = 3, 4, 96
    bank = synth.word_bank(n_words)
    labels = np.repeat(np.array([11, 5, 8], np.uint32), takes)  # the caller's word ids, not in ascending order
    word_of = np.repeat(np.arange(n_words), takes)
    lengths = [60, 48, 72, 55, 50, 64, 44, 70, 66, 52, 58, 46]
    pcm = synth.as_u16_numpy(synth.make_utterances(word_of, lengths, seed=77, bank=bank, S=(synth.buf_len_for(90) + 7) // 8 * 8))
    eng = Engine(max_frames=maxf, device=0)
    vd = eng.vad(pcm)
    assert np.all(vd["status"] == 0)
    n, mf, st = eng.mfcc_status(pcm, vd["seg"][:, 0].copy(), vd["seg"][:, 1].copy(), vd["mid_val"].copy())
    assert np.all(st == 0) and np.all(n >= 30)
    cen, frames, word_ids = eng.train_words(mf, n, labels, n_iter=4)
    assert word_ids.tolist() == [5, 8, 11] and frames.tolist() == [int(n[4]), int(n[8]), int(n[0])]  # each word starts from its first take
    assert cen.shape == (3, int(frames.max()) + 1, 12)
    # the same through the reference restatement
    order = np.argsort(labels, kind="stable")
    init = np.zeros_like(cen)
    for m, e in enumerate((4, 8, 0)):
        init[m, :n[e]] = mf[e, :n[e]]
    want, _ = ref.train(mf[order], n[order], np.array([0, 4, 8, 12], np.uint32), init, frames, 4)
    assert np.array_equal(cen, want)
    assert not np.array_equal(cen, init)
    eng.set_templates_dense(cen, frames)
    eng.set_word_map(word_ids)
    out = eng.recognize(pcm)
    assert np.all(out["results"]["status"] == 0)
    assert np.array_equal(word_ids[out["results"]["best_tpl"]], labels), (word_ids[out["results"]["best_tpl"]].tolist(), labels.tolist())
    eng.close()
