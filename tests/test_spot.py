"""Word spotting: subsequence DTW of the templates inside long feature rows (include/sr_engine.h, "word spotting").

The definition lives in tests/spot_ref.py (numpy).  The CPU tests check that restatement against itself: the scalar recurrence
against a brute-force enumeration of admissible paths, the scalar, two-state and vectorised forms against each other, and the
consequences the kernel relies on (span bounds, first reachable end, exact restart with a lead-in of 2M - 2 frames).  The GPU
tests compare whole records bit for bit with it.  Coefficients drawn from -2..2 make about a third of the end cells depend on
the tie rule; such inputs are used wherever the tie rule is under test.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import spot_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import DIS_ERR, NBEST_DTYPE, NO_WORD, RESULT_DTYPE, VAD_DTYPE, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
FUNCS = ("sr_spot_dp_batch_dev", "sr_spot_dp_batch", "sr_spot_batch", "sr_spot_geometry")
BAD_CONFIG, BAD_ARG, NO_TEMPLATES = 2, 3, 4
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
STAGE_CAP = 150 * 1024  # LdsBudget::stage_cap on MI355X
MAX_WINDOWS = 16_776_960


def same(got, want, what):
    got, want = np.asarray(got).reshape(want.shape), np.asarray(want)
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = np.nonzero(np.any(g != w, 1))[0]
    if len(bad):
        at = np.unravel_index(int(bad[0]), want.shape)
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} records differ, first at (row, window, slot) {at}: "
                             f"got {g[bad[0]].tolist()} want {w[bad[0]].tolist()}")


def all_no_hit(recs):
    return all(bool(np.all(recs[f] == 0xFFFFFFFF)) for f in recs.dtype.names)


# ---- CPU: the surface (fails without the feature) ----------------------------------------------------------------------------
def test_header_declares_the_spotting_api_and_libraries_export_it():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert src.index("sr_dtw_dp_batch_dev") < src.index("sr_spot_dp_batch_dev") < src.index("sr_delta_mfcc_batch")
    assert re.search(r"typedef struct sr_spot_hit \{\s*uint32_t dis;\s*uint32_t start;\s*uint32_t end;\s*uint32_t acc;\s*\} sr_spot_hit;", src)
    assert engine.SPOT_DTYPE == ref.SPOT_DTYPE and engine.SPOT_DTYPE.itemsize == 16
    for meth in ("spot", "spot_dev", "spot_pcm"):
        assert callable(getattr(Engine, meth, None)), meth
    assert callable(engine.spot_geometry)
    engine.dev_hook("spot_chunk_cols", 0)  # the testing library knows the hook ...
    assert engine.load_library().sr_dev_hook(b"spot_chunk_cols", C.c_int64(1)) == BAD_ARG  # ... the product library has none


# ---- CPU: the definition against itself --------------------------------------------------------------------------------------
def brute_force(d):
    """every admissible path, enumerated: start at (s, 0); diagonal, horizontal and vertical steps, the last two only directly
    after a diagonal one -> dict cell -> min (cost, start) over the paths that end there"""
    N, M = d.shape
    best = {}

    def walk(x, y, cost, start, after_diag):
        cost += int(d[x, y])
        if (x, y) not in best or (cost, start) < best[(x, y)]:
            best[(x, y)] = (cost, start)
        if x + 1 < N and y + 1 < M:
            walk(x + 1, y + 1, cost, start, True)
        if after_diag and x + 1 < N:
            walk(x + 1, y, cost, start, False)
        if after_diag and y + 1 < M:
            walk(x, y + 1, cost, start, False)

    for s in range(N):
        walk(s, 0, 0, s, False)
    return best


def small_dis(rng, N, M, amp=2):
    return ref.local_dis(rng.integers(-amp, amp + 1, (N, 12)), rng.integers(-amp, amp + 1, (M, 12)))


def test_scalar_recurrence_equals_brute_force_on_all_small_shapes():
    rng = np.random.default_rng(7)
    for N in range(1, 8):
        for M in range(1, 5):
            for _ in range(6):
                d = small_dis(rng, N, M)
                D, want = ref.dp_scalar(d), brute_force(d)
                for cell, v in D.items():
                    assert (v == ref.INF and cell not in want) or v == want[cell], (N, M, cell, v, want.get(cell))


@functools.lru_cache(maxsize=None)
def random_shapes():
    rng = np.random.default_rng(8)
    out = []
    for i in range(40):
        N, M = (80, 24) if i == 0 else (int(rng.integers(1, 81)), int(rng.integers(1, 25)))
        d = small_dis(rng, N, M, 2 if i % 4 else 3000)
        d.setflags(write=False)
        out.append((d, ref.dp_scalar(d)))
    return out


def test_scalar_two_state_and_vectorised_forms_agree():
    tie_cells = cells = 0
    for d, D in random_shapes():
        N, M = d.shape
        assert ref.dp_two_state(d) == D, (N, M)
        cost, start = ref.dp_end_row(d)
        for x in range(N):
            v = D[(x, M - 1)]
            assert (cost[x] == -1) if v == ref.INF else (int(cost[x]), int(start[x])) == v, (N, M, x)
        # how much of this depends on the tie rule: end cells whose start changes when ties go to the LARGEST start
        for x in range(N):
            if D[(x, M - 1)] != ref.INF and M > 1 and d.max() <= 10:
                cells += 1
                alt = _largest_start(d, x)
                tie_cells += alt != D[(x, M - 1)][1]
    assert cells > 200 and tie_cells * 10 > cells, (tie_cells, cells)  # small coefficients: ties are common


def _largest_start(d, x_end):
    """the largest start among the minimal-cost paths that end at (x_end, M-1): the recurrence with the tie rule reversed"""
    N, M = d.shape
    D = {}
    unreachable = (float("inf"), float("inf"))

    def at(x, y):
        return D[(x, y)] if x >= 0 and y >= 0 else unreachable

    def plus(c, add):
        return c if c == unreachable else (c[0] + add, c[1])

    for y in range(M):
        for x in range(x_end + 1):
            if y == 0:
                D[(x, 0)] = (int(d[x, 0]), -x)
                continue
            D[(x, y)] = plus(min(at(x - 1, y - 1), plus(at(x - 2, y - 1), int(d[x - 1, y])) if x >= 1 else unreachable,
                                 plus(at(x - 1, y - 2), int(d[x, y - 1]))), int(d[x, y]))
    return -D[(x_end, M - 1)][1]


def test_span_bounds_first_reachable_end_and_exact_restart():
    for d, D in random_shapes():
        N, M = d.shape
        cost, start = ref.dp_end_row(d)
        reach = np.nonzero(cost >= 0)[0]
        if N > M // 2:
            assert reach[0] == M // 2 and np.array_equal(reach, np.arange(M // 2, N)), (N, M)
        else:
            assert len(reach) == 0
        L = reach - start[reach] + 1
        if len(L):
            assert L.min() >= (1 if M == 1 else -(-(M - 1) // 2) + 1) and L.max() <= max(2 * M - 1, 1), (N, M, L.min(), L.max())
            assert cost.max() < 2 ** 31
        # D and S of end frame e depend on frames e - (2M - 2) .. e only: restart the DP there
        for e in reach[::3]:
            lo = max(0, int(e) - (2 * M - 2))
            c2, s2 = ref.dp_end_row(d[lo:e + 1])
            assert (int(c2[-1]), int(s2[-1]) + lo) == (int(cost[e]), int(start[e])), (N, M, e)


def test_geometry_stays_within_the_stage_cap():
    g = engine.spot_geometry(256, 16383, 100)
    cap = g["max_tpl_rows"]
    assert cap >= 256 and engine.spot_geometry(cap, 2000)["lds_bytes"] <= STAGE_CAP < engine.spot_geometry(cap + 1, 2000)["lds_bytes"]
    for tpl in (1, 2, 60, 130, 256, cap):
        for maxf in (2, 119, 256, 768, 16383):
            for win in (0, 1, 50, 64, 768, 1000, 20000):
                g = engine.spot_geometry(tpl, maxf, win)
                assert g["n_win"] == ref.n_windows(maxf, win) == (1 if win == 0 else -(-maxf // win)), (tpl, maxf, win)
                assert g["lds_bytes"] <= STAGE_CAP and g["max_tpl_rows"] == cap
                w = min(win, maxf) if win else maxf
                assert g["chunk_cols"] >= 1 and (g["chunk_cols"] % w == 0 or w > g["chunk_cols"]), (tpl, maxf, win, g)
    L = engine.load_library()
    out = (U32 * 4)()
    assert L.sr_spot_geometry(U32(0), U32(100), U32(0), out) == BAD_ARG and L.sr_spot_geometry(U32(10), U32(100), U32(0), None) == BAD_ARG
    assert L.sr_spot_geometry(U32(10), U32(1), U32(0), out) == BAD_ARG and L.sr_spot_geometry(U32(10), U32(16384), U32(0), out) == BAD_ARG


# ---- GPU: fixtures -------------------------------------------------------------------------------------------------------------
def dev_call(eng, im, frames, win=0, canary=None, frames_stride=1, d_frames=None, want_scores=True):
    """sr_spot_dp_batch_dev -> (hits SPOT_DTYPE [n, n_win, K], scores uint32 [n, n_win, K] or None); with a canary the
    outputs are guarded buffers whose every byte starts as the canary"""
    n, n_win, K = len(im), eng.spot_windows(win), eng.n_templates
    d_im = torch.from_numpy(np.ascontiguousarray(im)).cuda()
    if d_frames is None:
        d_frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint32).view(np.int32)).cuda()
    if canary is None:
        hits = torch.empty(n, n_win, K, 4, dtype=torch.int32, device="cuda:0")
        sc = torch.empty(n, n_win, K, dtype=torch.int32, device="cuda:0") if want_scores else None
        eng.spot_dev(d_im, d_frames, hits, sc, win, frames_stride)
        torch.cuda.synchronize()
        return hits.cpu().numpy().view(ref.SPOT_DTYPE).reshape(n, n_win, K), None if sc is None else sc.cpu().numpy().view(np.uint32)
    g_h = guarded_out((n, n_win, K), ref.SPOT_DTYPE, canary, 4096, "cuda:0", "hits")
    g_s = guarded_out((n, n_win, K), np.uint32, canary, 4096, "cuda:0", "scores")
    sid = torch.cuda.current_stream().cuda_stream
    assert eng.L.sr_spot_dp_batch_dev(eng.h, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(frames_stride), U32(n), U32(win), P(g_h.ptr),
                                      P(g_s.ptr) if want_scores else None, P(sid)) == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_h.check()
    g_s.check() if want_scores else g_s.check_untouched()
    return g_h.interior(), g_s.interior() if want_scores else None


EDGE_MAXF = 256
EDGE_M = (1, 2, 3, 63, 64, 65, 130, 7, 20, 40, 33, 100)  # slot 9 (40 frames) is erased
EDGE_N = sorted({0, 1, 63, 64, 65, 200, 300} | {m // 2 for m in EDGE_M[:7]} | {m // 2 + 1 for m in EDGE_M[:7]})


@functools.lru_cache(maxsize=None)
def edge_fixture(amp):
    rng = np.random.default_rng(100 + amp)
    K = len(EDGE_M)
    tf, valid = np.array(EDGE_M, np.uint32), np.ones(K, np.uint8)
    valid[9] = 0
    tm = np.zeros((K, max(EDGE_M) + 1, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-amp, amp + 1, (tf[k], 12))
    inf = np.array(EDGE_N, np.uint32)  # 300: above max_frames, clamped
    im = rng.integers(-amp, amp + 1, (len(inf), EDGE_MAXF, 12)).astype(np.int16)
    im[-2, 90:90 + 63] = tm[3, :63]  # a template inside the 200-frame row
    want = ref.spot_hits(im, inf, tm, tf, valid, EDGE_MAXF, 0)
    for a in (tm, tf, valid, im, inf, want):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, valid=valid, im=im, inf=inf, want=want)


@functools.lru_cache(maxsize=None)
def edge_want(amp, win):
    fx = edge_fixture(amp)
    want = ref.spot_hits(fx["im"], fx["inf"], fx["tm"], fx["tf"], fx["valid"], EDGE_MAXF, win)
    want.setflags(write=False)
    return want


def edge_engine(fx, **kw):
    eng = Engine(max_frames=EDGE_MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"], fx["valid"])
    return eng


SEAM_MAXF, SEAM_N = 768, 700
SEAM_M = (60, 1, 37, 59, 16, 2)
WINS = (0, 1, 50, 64, 768, 1000)


@functools.lru_cache(maxsize=None)
def seam_fixture():
    rng = np.random.default_rng(300)
    K = len(SEAM_M)
    tf = np.array(SEAM_M, np.uint32)
    tm = np.zeros((K, max(SEAM_M) + 1, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-2, 3, (tf[k], 12))
    inf = np.array([SEAM_N, 300, 0, SEAM_MAXF], np.uint32)
    im = rng.integers(-2, 3, (len(inf), SEAM_MAXF, 12)).astype(np.int16)
    im[3] = rng.integers(-3000, 3001, (SEAM_MAXF, 12))
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf)


@functools.lru_cache(maxsize=None)
def seam_want(win):
    fx = seam_fixture()
    want = ref.spot_hits(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, SEAM_MAXF, win)
    want.setflags(write=False)
    return want


def seam_engine(testing=False):
    fx = seam_fixture()
    eng = Engine(max_frames=SEAM_MAXF, device=0, testing=testing)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


class forced_chunk:
    """development hook "spot_chunk_cols" (testing library only; read per launch)"""

    def __init__(self, cols):
        self.cols = cols

    def __enter__(self):
        engine.dev_hook("spot_chunk_cols", self.cols)

    def __exit__(self, *exc):
        engine.dev_hook("spot_chunk_cols", 0)


# ---- GPU 1: length edges -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("amp", [2, 3000])
def test_length_edges(amp):
    fx = edge_fixture(amp)
    want = fx["want"]
    assert all_no_hit(want[:, 0, 9])  # the erased slot
    assert all_no_hit(want[0])        # N = 0
    for k, m in enumerate(EDGE_M[:7]):  # N = M / 2: nothing; N = M / 2 + 1: exactly one reachable end
        r0, r1 = EDGE_N.index(m // 2), EDGE_N.index(m // 2 + 1)
        assert want[r0, 0, k]["dis"] == DIS_ERR and want[r1, 0, k]["end"] == m // 2, (m, want[r0, 0, k], want[r1, 0, k])
    if amp == 3000:
        assert tuple(want[-2, 0, 3]) == (0, 90, 152, 0)  # the planted template
    eng = edge_engine(fx)
    hits, sc = dev_call(eng, fx["im"], fx["inf"])
    same(hits, want, "device form")
    assert np.array_equal(sc, want["dis"])
    h2, s2 = eng.spot(fx["im"], fx["inf"])
    same(h2, want, "host form")
    assert np.array_equal(s2, want["dis"])
    for win in (1, 100):
        same(dev_call(eng, fx["im"], fx["inf"], win)[0], edge_want(amp, win), f"win {win}")
    eng.close()


# ---- GPU 2: chunk seams ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chunk_seams_give_identical_bytes():
    fx = seam_fixture()
    assert engine.spot_geometry(max(SEAM_M), SEAM_MAXF)["chunk_cols"] < SEAM_N  # the default already has a seam here
    eng = seam_engine(testing=True)
    for win in (0, 50):
        want = seam_want(win)
        first = None
        for cols in (0, 64, 100, 1, 700):
            with forced_chunk(cols):
                hits, sc = dev_call(eng, fx["im"], fx["inf"], win)
            same(hits, want, f"win {win}, chunk {cols}")
            assert np.array_equal(sc, want["dis"]), (win, cols)
            first = first or hits.tobytes() + sc.tobytes()
            assert hits.tobytes() + sc.tobytes() == first, (win, cols)
    eng.close()


# ---- GPU 3: windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_windows_every_record_written(canary):
    fx = seam_fixture()
    eng = seam_engine(testing=True)
    for win in WINS:
        want = seam_want(win)
        assert want.shape[1] == eng.spot_windows(win) == (1 if win == 0 else -(-SEAM_MAXF // win))
        if 0 < win < SEAM_MAXF:  # windows entirely past N: no hit
            for r, n in enumerate(fx["inf"]):
                past = want[r, -(-int(n) // win):]
                assert all_no_hit(past), (win, r)
            assert len(want[1, -(-300 // win):]) >= 1
        for cols in (0, 100):
            with forced_chunk(cols):
                hits, sc = dev_call(eng, fx["im"], fx["inf"], win, canary)
                h_only, none = dev_call(eng, fx["im"], fx["inf"], win, canary, want_scores=False)
            same(hits, want, f"win {win}, chunk {cols}")
            same(h_only, want, f"win {win}, chunk {cols}, no scores")
            assert np.array_equal(sc, want["dis"]) and none is None
    eng.close()


# ---- GPU 4: planted words --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_planted_words_are_found_where_they_are():
    rng = np.random.default_rng(400)
    maxf, N, M = 256, 200, 20
    tm = np.zeros((2, M + 1, 12), np.int16)
    tm[:, :M] = rng.integers(-3000, 3001, (2, M, 12))
    im = rng.integers(-3000, 3001, (1, maxf, 12)).astype(np.int16)
    im[0, 50:70] = tm[0, :M]
    # 3:2: one diagonal step, then a diagonal and a horizontal one in turns -- 30 frames, an admissible path of cost 0
    idx = [0] + [y for o in range(1, 19, 2) for y in (o, o, o + 1)] + [19, 19]
    assert len(idx) == 30 and idx[:6] == [0, 1, 1, 2, 3, 3]
    im[0, 120:150] = tm[0, idx]
    tf, inf = np.array([M, M], np.uint32), np.array([N], np.uint32)
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    want = ref.spot_hits(im, inf, tm, tf, None, maxf, 64)
    # the verbatim copy ends at 69; the stretched one reaches the last template frame at 148 (its last input frame repeats it)
    assert tuple(want[0, 1, 0]) == (0, 50, 69, 0) and tuple(want[0, 2, 0]) == (0, 120, 148, 0)
    assert want[0, 0, 0]["dis"] > 100 and want[0, 1, 1]["dis"] > 100 and want[0, 3, 0]["dis"] > 100  # noise elsewhere
    hits, sc = eng.spot(im, inf, 64)
    same(hits, want, "win 64")
    same(dev_call(eng, im, inf, 64)[0], want, "win 64, device")
    whole = ref.spot_hits(im, inf, tm, tf, None, maxf, 0)
    assert tuple(whole[0, 0, 0]) == (0, 50, 69, 0)  # first minimum
    same(eng.spot(im, inf)[0], whole, "one window")
    eng.close()


# ---- GPU 5: nothing read past frames -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_is_read_past_frames_and_counts_come_from_records():
    fx = edge_fixture(2)
    eng = edge_engine(fx)
    inf = np.minimum(fx["inf"], EDGE_MAXF)
    rec = poison_feature_rows(fx["im"].copy(), inf)
    same(dev_call(eng, rec, fx["inf"])[0], fx["want"], "poisoned rows")
    same(eng.spot(rec, fx["inf"])[0], fx["want"], "poisoned rows, host")
    n = len(inf)
    vad = np.full((n, 12), 0x7F7F7F7F, np.uint32)  # sr_vad_rec: frm_num is word 9 of 12
    vad[:, VAD_DTYPE.fields["frm_num"][1] // 4] = fx["inf"]
    res = np.full((n, 4), 0x7F7F7F7F, np.uint32)   # sr_result: frm_num is word 2 of 4
    res[:, RESULT_DTYPE.fields["frm_num"][1] // 4] = fx["inf"]
    for recs, col, stride in ((vad, 9, 12), (res, 2, 4)):
        d = torch.from_numpy(recs.view(np.int32)).cuda()
        same(dev_call(eng, rec, None, 0, None, stride, d[:, col])[0], fx["want"], f"stride {stride}")
        hits = np.zeros(fx["want"].shape, ref.SPOT_DTYPE)
        assert eng.L.sr_spot_dp_batch(eng.h, engine._vp(rec), P(recs.ctypes.data + 4 * col), U32(stride), U32(n), U32(0), engine._vp(hits),
                                      None) == 0
        same(hits, fx["want"], f"host, stride {stride}")
    eng.close()


# ---- GPU 6: host form = device form = whole path ---------------------------------------------------------------------------
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
    for win in (0, 32):
        want = ref.spot_hits(mf, n, tm, tf, None, maxf, win)
        assert np.all(want[2]["dis"] == DIS_ERR)
        if win == 0:
            assert want[0, 0, 0]["dis"] == 0 and want[0, 0, 0]["end"] <= 29 and want[1, 0, 1]["dis"] == 0  # the pieces are found
        hits, sc = eng.spot(mf, n, win)
        same(hits, want, f"host, win {win}")
        d_hits, d_sc = dev_call(eng, mf, n, win)
        assert d_hits.tobytes() == hits.tobytes() and d_sc.tobytes() == sc.tobytes()
        o = eng.spot_pcm(pcm, start, end, mid, win)
        assert o["hits"].tobytes() == hits.tobytes() and o["scores"].tobytes() == sc.tobytes()
        assert o["mfcc"].tobytes() == mf.tobytes() and np.array_equal(o["frm_num"], n) and np.array_equal(o["status"], st)
        # every optional output NULL
        h2 = np.zeros_like(hits)
        v, S = engine._vp, pcm.shape[1]
        assert eng.L.sr_spot_batch(eng.h, v(pcm), U64(S), U32(S), U32(B), v(start), v(end), v(mid), U32(win), v(h2), None, None, None,
                                   None) == 0
        assert h2.tobytes() == hits.tobytes()
    # the device whole path: sr_mfcc_batch_dev, then the stage on the records' frame counts
    recs = np.zeros(B, VAD_DTYPE)
    recs["mid_val"], recs["frm_num"], recs["status"] = mid, n, st
    recs["seg"][:, 0], recs["seg"][:, 1] = np.where(st == 0, start, 1), np.where(st == 0, end, 1)
    d_pcm, d_vad = torch.from_numpy(pcm.view(np.int16)).cuda(), torch.from_numpy(recs.view(np.int32).reshape(B, 12)).cuda()
    d_mf = torch.zeros(B, maxf, 12, dtype=torch.int16, device="cuda:0")
    sid = torch.cuda.current_stream().cuda_stream
    assert eng.L.sr_mfcc_batch_dev(eng.h, P(d_pcm.data_ptr()), U64(pcm.shape[1]), U32(B), P(d_vad.data_ptr()), P(d_mf.data_ptr()), P(sid)) == 0
    d_h = torch.empty(B, 1, 4, 4, dtype=torch.int32, device="cuda:0")
    eng.spot_dev(d_mf, d_vad[:, 9], d_h, None, 0, 12)
    torch.cuda.synchronize()
    assert d_h.cpu().numpy().tobytes() == eng.spot(mf, n)[0].tobytes()
    eng.close()


# ---- GPU 7: composition with N-best ------------------------------------------------------------------------------------------
def nbest_rule(row, words, n_best):
    """the N-best rule (include/sr_engine.h) for one score row: per word the first minimum in slot order and the number of
    slots below dis_err, words ranked by (dis, slot), the tail empty"""
    best = {}
    for k, d in enumerate(int(v) for v in row):
        if d != DIS_ERR:
            e = best.setdefault(int(words[k]), [d, k, 0])
            e[2] += 1
            if d < e[0]:
                e[:2] = [d, k]
    ranked = sorted((d, k, w, c) for w, (d, k, c) in best.items())
    ent = [(w, k, d, c) for d, k, w, c in ranked[:n_best]]
    return ent + [(NO_WORD, 0xFFFFFFFF, DIS_ERR, 0)] * (n_best - len(ent)), len(ranked)


@pytest.mark.gpu
def test_nbest_over_the_window_scores():
    fx = seam_fixture()
    eng = seam_engine()
    words = np.array([5, 9, 5, 5, 9, 7], np.uint32)
    eng.set_word_map(words)
    win, n_best = 64, 2
    want = seam_want(win)
    hits, sc = eng.spot(fx["im"], fx["inf"], win)
    same(hits, want, "hits")
    rows = sc.reshape(-1, len(SEAM_M))
    nb, nm = eng.nbest(rows, n_best)
    exp = [nbest_rule(r, words, n_best) for r in want["dis"].reshape(-1, len(SEAM_M))]
    assert nb.tobytes() == np.array([e[0] for e in exp], NBEST_DTYPE).tobytes()
    assert np.array_equal(nm, [e[1] for e in exp]) and (nm == 0).sum() >= 12 and (nm == 3).sum() >= 20
    d_nb, d_nm = eng.nbest_dev(torch.from_numpy(rows.view(np.int32)).cuda(), n_best)
    torch.cuda.synchronize()
    assert engine.nbest_from_torch(d_nb).tobytes() == nb.tobytes()
    eng.close()


# ---- GPU 8: the longest template, refusals --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_longest_template_and_refusals_that_write_nothing():
    maxf, n = 1000, 2
    cap = engine.spot_geometry(10, maxf)["max_tpl_rows"]
    rng = np.random.default_rng(800)
    tm = np.zeros((2, cap + 2, 12), np.int16)
    tm[:, :cap + 1] = rng.integers(-2, 3, (2, cap + 1, 12))
    im = rng.integers(-2, 3, (n, maxf, 12)).astype(np.int16)
    inf = np.array([cap // 2 + 90, cap // 2], np.uint32)
    eng = Engine(max_frames=maxf, device=0)
    tf = np.array([cap, 40], np.uint32)
    eng.set_templates_dense(tm, tf)
    want = ref.spot_hits(im, inf, tm, tf, None, maxf, 0)
    assert want[0, 0, 0]["dis"] != DIS_ERR and want[1, 0, 0]["dis"] == DIS_ERR and want[1, 0, 1]["dis"] != DIS_ERR
    same(dev_call(eng, im, inf, 0, 0xA5)[0], want, "longest template")
    same(eng.spot(im, inf)[0], want, "longest template, host")

    d_im, d_inf = torch.from_numpy(im).cuda(), torch.from_numpy(inf.view(np.int32)).cuda()
    bank = synth.word_bank(2)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(n), [40, 40], seed=5, bank=bank, S=synth.buf_len_for(60)))
    seg = np.array([[4000, 9000]] * n, np.int32)
    mid = np.full(n, 2048, np.uint32)
    sid = torch.cuda.current_stream().cuda_stream
    v = engine._vp

    def refused(e, code, rows=n, win=0, stride=1, null=None, whole=True):
        L, h = e.L, e.h
        for dev in ("cuda:0", None):
            g = [guarded_out((n, 4, 2), ref.SPOT_DTYPE, 0xA5, 4096, dev, "hits"), guarded_out((n, 4, 2), np.uint32, 0xA5, 4096, dev, "scores")]
            a = dict(mfcc=P(d_im.data_ptr()) if dev else v(im), frames=P(d_inf.data_ptr()) if dev else v(inf), hits=P(g[0].ptr))
            if null:
                a[null] = None
            if dev:
                assert L.sr_spot_dp_batch_dev(h, a["mfcc"], a["frames"], U32(stride), U32(rows), U32(win), a["hits"], P(g[1].ptr), P(sid)) == code
                torch.cuda.synchronize()
            else:
                assert L.sr_spot_dp_batch(h, a["mfcc"], a["frames"], U32(stride), U32(rows), U32(win), a["hits"], P(g[1].ptr)) == code
                if whole and null != "mfcc" and null != "frames":
                    S = pcm.shape[1]
                    assert L.sr_spot_batch(h, v(pcm), U64(S), U32(S), U32(rows), v(seg[:, 0].copy()), v(seg[:, 1].copy()), v(mid), U32(win),
                                           a["hits"], P(g[1].ptr), None, None, None) == code
            for x in g:
                x.check_untouched()

    for null in ("mfcc", "frames", "hits"):
        refused(eng, BAD_ARG, null=null)
    refused(eng, BAD_ARG, stride=0, whole=False)  # (the whole path has no such argument)
    refused(eng, BAD_ARG, rows=MAX_WINDOWS + 1)
    refused(eng, BAD_ARG, rows=MAX_WINDOWS // 1000 + 1, win=1)  # n_win = 1000
    tf2 = np.array([cap + 1, 40], np.uint32)  # one row more than fits
    eng.set_templates_dense(tm, tf2)
    refused(eng, BAD_ARG)
    assert b"too long" in eng.L.sr_last_error()
    eng.set_templates_dense(tm, tf)
    same(dev_call(eng, im, inf)[0], want, "after the refusals")
    eng.close()
    e2 = Engine(max_frames=maxf, device=0)  # no templates
    refused(e2, NO_TEMPLATES)
    e2.close()
    e3 = Engine(max_frames=maxf, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    refused(e3, BAD_CONFIG)
    e3.close()


# ---- GPU 9: LDS poison -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lds_poison_between_calls_changes_nothing():
    fx = seam_fixture()
    eng = seam_engine()
    a = dev_call(eng, fx["im"], fx["inf"], 50)
    assert eng.lds_poison(0x5EED) > 0
    torch.cuda.synchronize()
    b = dev_call(eng, fx["im"], fx["inf"], 50)
    assert eng.lds_poison(0xFFFFFFFF) > 0
    c = dev_call(eng, fx["im"], fx["inf"], 50)
    same(a[0], seam_want(50), "before")
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
    eng.close()
