"""Long sequences, up to the 16 383-frame cap (-m gpu): every DTW launch form on both sides of the frame counts where the
plan switches forms, the full-DP scorer at long templates, the three front ends at long caps, the batch VAD past u16
buffer lengths, the u16 truncation of a segment's frame count (MFCC.C:102) and the delta cepstra's status filter.
Everything against the CPU oracle (tier (ii)); tests/test_oracle.py pins the oracle to the reference's own objects at
these lengths."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import oracle_lib as ol
from stm32_speech_recognition_amd import Engine
from stm32_speech_recognition_amd.engine import (FEAT_LOGMEL, FEAT_MAG, ST_MFCC_FAIL, ST_OK, ST_SEG_OOB, ST_VAD_FAIL,
                                                 SrError, dev_hook)
from test_frame_features import log100, mel_from_mag, windowed

pytestmark = pytest.mark.gpu

STAGE_CAP = 150 * 1024  # LdsBudget::stage_cap (csrc/sr_dtw_plan.h)
EXT = (dict(fs=16000, nfft=512, n_mel=40), dict(fs=16000, nfft=512, n_mel=40))
FRONT_ENDS = {"ref": (dict(), dict()), "ext": EXT, "gen": ol.GENERIC_CONFIGS[0]}


# ---- the DTW plan, read from the testing build's dtw_debug lines --------------------------------------------------------
_LDS = re.compile(r"k_dtw_lds geometry for K = (\d+), (\d+) rows: U = (\d+), Kc = (\d+), tie table (\d+), LDS (\d+) bytes")
_CQ = re.compile(r"k_dtw_cells for (\d+) template rows: (\d+) band points, LDS (\d+) bytes; k_dtw_quad: (\d+) x (\d+), LDS (\d+) bytes")
_DP = re.compile(r"full-DP scorer for (\d+) template rows: (\d+) lanes per pair")


def set_store_and_plan(eng, capfd, tm, tf, valid=None):
    """set a dense store on a testing-build engine with dtw_debug on; returns the plan it printed"""
    capfd.readouterr()
    dev_hook("dtw_debug", 1)
    try:
        eng.set_templates_dense(tm, tf, valid)
    finally:
        dev_hook("dtw_debug", 0)
    err = capfd.readouterr().err
    m1, m2 = _LDS.findall(err), _CQ.findall(err)
    assert len(m1) == 1 and len(m2) == 1, err
    K, R, U, kc, tie, lds = map(int, m1[0])
    rows, cpts, cbytes, qpu, qpk, qbytes = map(int, m2[0])
    return dict(K=K, R=R, U=U, kc=kc, rows=rows, cells_points=cpts, cells_bytes=cbytes, quad=(qpu, qpk), quad_bytes=qbytes)


def cells_room(R, rows):
    """band points k_dtw_cells' workgroup holds beside the staged rows (dtw_cells_lds, k_dtw_cells.hip: 12 words per input
    row, 9 per template row, 3 per input row + 1 for the ranges)"""
    return (STAGE_CAP - 4 * (12 * R + 9 * rows + 3 * (R + 1))) // 4


def oracle_scores(orc, im, inf, tm, tf, valid):
    nc = im.shape[2]
    pad = np.zeros((1, nc), np.int16)
    return np.array([[orc.dtw(np.concatenate([im[b, :inf[b] + 1], pad]), inf[b], tm[k], tf[k]) if valid[k] else ol.DIS_ERR
                      for k in range(len(tf))] for b in range(len(inf))], dtype=np.uint32)


def check_all_modes(eng, orc, im, inf, tm, tf, valid):
    want = oracle_scores(orc, im, inf, tm, tf, valid)
    wb = np.array([int(np.argmin(w)) if w.min() != ol.DIS_ERR else 0 for w in want])
    for mode in (0, 1, 2, 3):
        eng.set_small_launch(mode)
        sc, res = eng.dtw(im, inf)
        assert np.array_equal(sc, want), (mode, np.argwhere(sc != want)[:8])
        assert np.array_equal(res["best_tpl"], wb) and np.array_equal(res["min_dis"], want.min(1)), mode
    eng.set_small_launch(0)
    return want


def long_store(rng, R, nc, K, lens):
    """K templates of R + 1 rows: lens first, the rest random in [R/2, R]; speech-range rows, constant rows (ties) and
    rows at the edge of the staged form (+-16383)"""
    tf = rng.integers(max(1, R // 2), R + 1, K).astype(np.uint32)
    tf[:len(lens)] = lens
    tm = rng.integers(-3000, 3001, (K, R + 1, nc)).astype(np.int16)
    tm[1::4] = rng.integers(-4, 5, (len(tm[1::4]), 1, nc))              # one repeated row: ties everywhere
    tm[2::4] = rng.integers(-16383, 16385, (len(tm[2::4]), R + 1, nc))  # full scale the staged rows still hold
    return tm, tf


def long_inputs(rng, R, nc, lens):
    B = len(lens)
    im = rng.integers(-3000, 3001, (B, R, nc)).astype(np.int16)
    im[1::3] = rng.integers(-32768, 32768, (len(im[1::3]), R, nc))  # full scale: u32 wrap, roots past the tie table
    im[2::3] = rng.integers(-4, 5, (len(im[2::3]), 1, nc))
    return im, np.asarray(lens, np.uint32)


def lengths_for(R):
    """1, 2, R/2, R - 1, R and the 2:1 gate edges against templates of R and R/2 + 1 frames"""
    h = R // 2
    return sorted({1, 2, h - 1, h, h + 1, R - 1, R, max(1, (h + 1) // 2 - 1), max(1, (h + 1) // 2)})


# (R, n_coef, staged, quad fits, cells): both sides of every frame count where the plan changes form.  MI355X, R + 1 rows.
#   k_dtw_cells: stores of up to 400 frames (dtw_cells_max_points); from 301 frames on its band-point budget is capped
#   k_dtw_quad:  the 1 x 4 shape up to 1 096 rows of 12 coefficients, 852 of 13..16
#   k_dtw_lds:   U = 1 up to 5 326 frames (12 coefficients) / 4 146 (13..16); beyond, the unstaged walk
PLAN_CASES = [
    (400, 12, True, True, True), (401, 12, True, True, False),
    (1096, 12, True, True, False), (1097, 12, True, False, False),
    (852, 16, True, True, False), (853, 16, True, False, False),
    (4146, 16, True, False, False), (4147, 16, False, False, False),
    (5326, 12, True, False, False), (5327, 12, False, False, False),
    (16383, 12, False, False, False),
]


@pytest.mark.parametrize("R,nc,staged,quad,cells", PLAN_CASES, ids=[f"R{c[0]}-c{c[1]}" for c in PLAN_CASES])
def test_dtw_forms_at_plan_boundaries_match_oracle(capfd, R, nc, staged, quad, cells):
    """scores and argmin records of every small-launch mode against Oracle.dtw, with the form each mode must take asserted
    from the plan: staged (k_dtw_lds) or not (k_dtw / k_dtw_gen), k_dtw_quad fits or not, k_dtw_cells on or off"""
    rng = np.random.default_rng(R * 31 + nc)
    gen = nc != 12
    eng = Engine(max_frames=R, device=0, testing=True, **(dict(n_coef=nc) if gen else {}))
    orc = ol.Oracle(max_frames=R, **(dict(n_coef=nc) if gen else {}))
    h = R // 2
    tm, tf = long_store(rng, R, nc, 12, [R, 1, 2, h + 1, R - 1, h, 2 * (h // 2)])
    valid = np.ones(12, np.uint8)
    valid[-1] = 0
    plan = set_store_and_plan(eng, capfd, tm, tf, valid)
    assert plan["R"] == R and plan["rows"] == R + 1 and plan["K"] == 12
    assert (plan["U"] > 0) == staged, plan
    assert (plan["quad"] != (0, 0)) == quad, plan
    if quad and R > 800:
        assert plan["quad"] == (1, 4), plan  # the smallest shape at the top of its range
    assert (plan["cells_bytes"] > 0) == cells, plan
    if cells:  # the store's longest pairs outgrow the budget: their workgroups walk literally
        assert plan["cells_points"] == cells_room(R, R + 1), plan
    if staged and R > 4000:
        assert plan["U"] == 1 and plan["kc"] == 12, plan
    im, inf = long_inputs(rng, R, nc, lengths_for(R))
    want = check_all_modes(eng, orc, im, inf, tm, tf, valid)
    assert (want != ol.DIS_ERR).sum() >= 3 * len(inf) and (want == ol.DIS_ERR).any()
    eng.close()


def test_staged_store_of_more_than_1024_templates_walks_in_chunks(capfd):
    """U = 1 near the top of the staged range with K = 1 025: the store is walked in two chunks of 513 templates"""
    R, K = 5326, 1025
    rng = np.random.default_rng(99)
    eng, orc = Engine(max_frames=R, device=0, testing=True), ol.Oracle(max_frames=R)
    tf = rng.integers(1000, 2001, K).astype(np.uint32)
    tf[:4] = [2000, 1000, 1999, 1500]
    tm = rng.integers(-3000, 3001, (K, 2001, 12)).astype(np.int16)
    valid = np.ones(K, np.uint8)
    valid[[3, 700]] = 0
    plan = set_store_and_plan(eng, capfd, tm, tf, valid)
    assert plan["U"] == 1 and plan["kc"] == 513 and plan["quad"] == (0, 0) and plan["cells_bytes"] == 0, plan
    im, inf = long_inputs(rng, R, 12, [999, 1000, 2000, 4000, 4001, R])
    want = check_all_modes(eng, orc, im, inf, tm, tf, valid)
    assert (want[:, 512:] != ol.DIS_ERR).sum() > 1000 and (want == ol.DIS_ERR).any()
    eng.close()


# ---- the opt-in full-DP scorer ---------------------------------------------------------------------------------------------
def _dp_lanes_expected(rows, lanes):
    """lanes per pair launch_dtw_dp runs (k_dtw_dp.hip): a band kernel of G lanes holds up to 527 / 945 / 1 569 template
    rows for G = 4 / 8 / 16; beyond, G = 16, then the one-wave-per-pair kernel"""
    top = {4: 527, 8: 945, 16: 1569}
    if lanes == 1 or rows > 1569:
        return {1}
    if lanes == 0:
        return {8, 16}
    return {lanes} if rows <= top[lanes] else {16}


@pytest.mark.parametrize("rows", [945, 946, 1569, 1570, 3200])
def test_dtw_dp_long_templates_match_its_oracle(capfd, rows):
    rng = np.random.default_rng(rows)
    m = rows - 1
    eng, orc = Engine(max_frames=m, device=0, testing=True), ol.Oracle(max_frames=m)
    tf = np.array([m, (3 * m) // 4, m // 2 + 1], np.uint32)
    tm = rng.integers(-3000, 3001, (3, rows, 12)).astype(np.int16)
    tm[1] = rng.integers(-3, 4, (1, 12))
    eng.set_templates_dense(tm, tf)
    inf = np.array([m, m // 2, m // 2 + 1, (2 * m) // 3], np.uint32)
    im = rng.integers(-3000, 3001, (4, m, 12)).astype(np.int16)
    want = orc.dtw_dp_batch(im, inf, tm, tf, n_threads=12)
    assert (want != ol.DIS_ERR).sum() >= 8
    for lanes in (0, 1, 4, 8, 16):
        eng.set_dp_lanes(lanes)
        capfd.readouterr()
        dev_hook("dtw_debug", 1)
        try:
            got = eng.dtw_dp(im, inf)
        finally:
            dev_hook("dtw_debug", 0)
        g = [(int(r), int(G)) for r, G in _DP.findall(capfd.readouterr().err)]
        assert len(g) == 1 and g[0][0] == rows and g[0][1] in _dp_lanes_expected(rows, lanes), (lanes, g)
        assert np.array_equal(got, want), (lanes, np.argwhere(got != want)[:8])
    eng.close()


def test_dtw_dp_rejects_templates_past_3200_rows_and_writes_nothing():
    m = 3200  # 3 201 rows
    eng = Engine(max_frames=m, device=0)
    tm = np.zeros((2, m + 1, 12), np.int16)
    eng.set_templates_dense(tm, np.array([m, 100], np.uint32))
    mf = torch.zeros((2, m, 12), dtype=torch.int16, device="cuda:0")
    fr = torch.tensor([m, 1000], dtype=torch.int32, device="cuda:0")
    sc = torch.full((2, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    with pytest.raises(SrError, match="templates too long"):
        eng.dtw_dp_dev(mf, sc, in_frames=fr)
    with pytest.raises(SrError, match="templates too long"):
        eng.dtw_dp(np.zeros((2, m, 12), np.int16), np.array([m, 1000], np.uint32))
    torch.cuda.synchronize()
    assert (sc.cpu() == 0x5A5A5A5A).all()
    eng.close()


# ---- long captures -----------------------------------------------------------------------------------------------------
def capture(orc, S, start, tone_len, seed, amp=700.0, freq=440.0):
    """noise head, quiet lead, a tone of tone_len samples from `start` on, quiet tail: uint16 [S]"""
    rng = np.random.default_rng(seed)
    x = 2048 + rng.normal(0, 4, S)
    x[:orc.noise_len] = 2048 + rng.normal(0, 8, orc.noise_len)
    t = np.arange(tone_len)
    x[start:start + tone_len] += amp * np.sin(2 * np.pi * freq * t / orc.cfg.fs)
    return np.clip(np.round(x), 0, 4095).astype(np.uint16)


def seg0_frames(orc, x):
    """(start, end, raw frame count before the u16 truncation) of segment 0 in the oracle's VAD"""
    rc, a = orc.noise_atap(x)
    assert rc == 0
    seg = orc.vad(x, a)
    st, en = int(seg[0]), int(seg[1])
    assert st >= 1 and en > st, seg[:6]
    return st, en, ((en - st) - orc.frame_len) // orc.hop + 1


def capture_with_frames(orc, target, seed, S=None):
    """a capture whose segment 0 has exactly `target` frames (before the u16 truncation)"""
    start = orc.noise_len + 40 * orc.hop
    tail = 60 * orc.hop
    ln = (target - 1) * orc.hop + orc.frame_len
    need = start + ln + 4 * orc.hop + tail
    S = ((need + 7) // 8) * 8 if S is None else S
    for _ in range(4):
        x = capture(orc, S, start, ln, seed)
        _, _, n = seg0_frames(orc, x)
        if n == target:
            return x
        ln += (target - n) * orc.hop
    raise AssertionError(f"could not place a {target}-frame segment (got {n})")


def frm_status(st, en, fl, hop, R):
    if en < 0:
        return 0, ST_VAD_FAIL
    if st < 1:
        return 0, ST_SEG_OOB
    n = ((((en - st) & 0xFFFFFFFF) - fl) // hop + 1) & 0xFFFF
    return (0, ST_MFCC_FAIL) if n > R else (n, ST_OK)


@pytest.mark.parametrize("fe", ["ref", "ext", "gen"])
@pytest.mark.parametrize("R", [1000, 4096, 16383])
def test_front_end_at_long_caps_matches_oracle(fe, R):
    """segments of R - 1, R and R + 1 frames: VAD records, every MFCC row and the zero rows up to R, scores and records"""
    ekw, okw = FRONT_ENDS[fe]
    eng, orc = Engine(max_frames=R, device=0, **ekw), ol.Oracle(max_frames=R, **okw)
    xs = [capture_with_frames(orc, R + d, seed=R + d) for d in (-1, 0, 1)]
    S = max(len(x) for x in xs)
    pcm = np.full((3, S), 2048, np.uint16)
    for b, x in enumerate(xs):
        pcm[b, :len(x)] = x
    rng = np.random.default_rng(R)
    nc = orc.n_coef
    tf = np.array([R, R // 2 + 1], np.uint32)
    tm = rng.integers(-2000, 2001, (2, R + 1, nc)).astype(np.int16)
    eng.set_templates_dense(tm, tf)
    got = eng.recognize(pcm)
    ores, omf, osc = orc.recognize_batch(pcm, orc.make_templates(tm, tf), n_threads=3)
    assert list(ores["frm_num"]) == [R - 1, R, 0] and list(ores["status"]) == [ST_OK, ST_OK, ST_MFCC_FAIL]
    for f in ("best_tpl", "min_dis", "frm_num", "status"):
        assert np.array_equal(got["results"][f], ores[f]), f
    assert np.array_equal(got["mfcc"], omf)
    assert not got["mfcc"][0, R - 1:].any() and not got["mfcc"][2].any()
    assert np.array_equal(got["scores"], osc)
    for b in range(3):
        rc, a = orc.noise_atap(pcm[b])
        seg = orc.vad(pcm[b], a)
        v = got["vad"][b]
        assert (v["mid_val"], v["n_thl"], v["z_thl"], v["s_thl"]) == a.astuple() and np.array_equal(v["seg"], seg), b
        assert (v["frm_num"], v["status"]) == (ores["frm_num"][b], ores["status"][b])
    if fe == "ref" and R == 16383:
        # magnitude and log-Mel rows far past frame 4 096 of the R-frame record
        v = got["vad"][1]
        st, en, mid = v["seg"][0:1].astype(np.int32), v["seg"][1:2].astype(np.int32), v["mid_val"][None].astype(np.uint32)
        mag, n, status = eng.frame_features(pcm[1:2], st, en, mid, FEAT_MAG)
        lg, n2, _ = eng.frame_features(pcm[1:2], st, en, mid, FEAT_LOGMEL)
        assert n[0] == n2[0] == R and status[0] == 0
        rows = np.array([0, 4095, 4096, 4097, 8191, 12345, R - 2, R - 1])
        fr = windowed(pcm[1], int(st[0]), R, orc.frame_len, orc.hop, int(mid[0]), orc.tables()["hamm"])[rows]
        want = np.stack([orc.fft_mag(f) for f in fr])
        assert np.array_equal(mag[0, rows], want)
        mel, _ = mel_from_mag(want, orc.tables())
        assert np.array_equal(lg[0, rows].reshape(-1), log100(orc, mel))
    eng.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_vad_past_u16_buffer_lengths(mode):
    """buf_len 65 535, 65 536, 65 544 and ~10^6 (the firmware's buf_len is u16), words that start past 2^16 and 2^20"""
    orc = ol.Oracle(max_frames=400)
    eng = Engine(max_frames=400, device=0)
    S = 1 << 20 | 40000
    pcm = np.stack([capture(orc, S, start, 300 * 80, seed=i) for i, start in
                    enumerate([(1 << 16) + 400, (1 << 20) + 400, 65000, 3000, 65536 - 200 * 80])])
    eng.set_small_launch(mode)
    for buf_len in (65535, 65536, 65544, 1000000, S):
        vd = eng.vad(pcm, buf_len=buf_len)
        segs = []
        for b in range(len(pcm)):
            rc, a = orc.noise_atap(pcm[b, :buf_len])
            seg = orc.vad(pcm[b, :buf_len], a)
            assert np.array_equal(vd["seg"][b], seg), (buf_len, b, vd["seg"][b], seg)
            assert (vd["mid_val"][b], vd["n_thl"][b], vd["z_thl"][b], vd["s_thl"][b]) == a.astuple()
            assert (vd["frm_num"][b], vd["status"][b]) == frm_status(int(seg[0]), int(seg[1]), orc.frame_len, orc.hop, 400)
            segs.append(seg)
        assert sum(int(sg[0] >= 0) for sg in segs) >= 2, buf_len
        if buf_len >= 1000000:  # complete segments past 2^16 and past 2^20 (the latter only in the whole buffer)
            assert segs[0][0] > (1 << 16) and segs[0][1] > segs[0][0]
            assert buf_len < S or (segs[1][0] > (1 << 20) and segs[1][1] > segs[1][0])
    eng.set_small_launch(0)
    eng.close()


def test_u16_frame_count_wrap_agrees_everywhere():
    """a segment of 65 536 + n frames has frm_num = n (MFCC.C:102 truncates to u16); with n <= max_frames it is OK and its
    MFCC rows are the segment's first n frames -- in sr_vad_batch, sr_recognize_batch, sr_recognize_segments_batch and
    the stream VAD / recognition alike"""
    R, n = 600, 321
    orc = ol.Oracle(max_frames=R)
    eng = Engine(max_frames=R, device=0)
    x = capture_with_frames(orc, 65536 + n, seed=5)
    assert len(x) > 5_200_000
    st, en, raw = seg0_frames(orc, x)
    assert raw == 65536 + n
    rng = np.random.default_rng(3)
    tf = np.array([n, 2 * n, n // 2 + 1, 40], np.uint32)
    tm = rng.integers(-2000, 2001, (4, 2 * n + 1, 12)).astype(np.int16)
    eng.set_templates_dense(tm, tf)
    tpl = orc.make_templates(tm, tf)
    pcm = x[None]
    ores, omf, osc = orc.recognize_batch(pcm, tpl)
    assert ores["frm_num"][0] == n and ores["status"][0] == ST_OK  # the oracle's own record wraps
    rc, a = orc.noise_atap(x)
    n2, rows = orc.mfcc(x, st, en, a)
    assert n2 == n and np.array_equal(omf[0, :n], rows)
    # the first n frames of the segment, computed as a segment of n frames
    n3, rows3 = orc.mfcc(x, st, st + (n - 1) * orc.hop + orc.frame_len, a)
    assert n3 == n and np.array_equal(rows3, rows)
    for mode in (0, 1):  # four waves per capture (k_vad_wide) / one (k_vad)
        eng.set_small_launch(mode)
        vd = eng.vad(pcm)
        assert vd["seg"][0][0] == st and vd["seg"][0][1] == en and (vd["frm_num"][0], vd["status"][0]) == (n, ST_OK), mode
        got = eng.recognize(pcm)
        for f in ("best_tpl", "min_dis", "frm_num", "status"):
            assert np.array_equal(got["results"][f], ores[f]), (mode, f)
        assert np.array_equal(got["mfcc"], omf) and np.array_equal(got["scores"], osc), mode
    eng.set_small_launch(0)
    sres, ssc, svd = eng.recognize_segments(pcm)
    wres, wsc = orc.recognize_segments(x, tpl)
    for f in ("best_tpl", "min_dis", "frm_num", "status"):
        assert np.array_equal(sres[:, 0][f], wres[f]), f
    assert np.array_equal(ssc[:, 0], wsc) and sres[0, 0]["frm_num"] == n
    seg = orc.vad(x, a).reshape(-1, 2)
    nseg = int((seg[:, 0] >= 0).sum())
    out = eng.segment_stream(pcm)
    assert out["total"] == nseg and out["segs"][0]["start"] == st and out["segs"][0]["end"] == en
    assert out["segs"][0]["frm_num"] == n
    rs = eng.recognize_stream(pcm)
    assert rs["results"][0]["frm_num"] == n and rs["results"][0]["status"] == ST_OK
    assert np.array_equal(rs["mfcc"][0], omf[0]) and np.array_equal(rs["scores"][0], osc[0])
    assert rs["results"][0]["best_tpl"] == ores["best_tpl"][0] and rs["results"][0]["min_dis"] == ores["min_dis"][0]
    eng.close()


# ---- delta cepstra -----------------------------------------------------------------------------------------------------
def delta_definition(m, n):
    """the numpy statement of test_oracle.py::test_delta_mfcc_definition"""
    out = np.zeros_like(m)
    if n == 0:
        return out
    x = m[:n].astype(np.int64)
    idx = np.arange(n)
    c = lambda k: x[np.clip(idx + k, 0, n - 1)]
    num = (c(1) - c(-1)) + 2 * (c(2) - c(-2))
    out[:n] = (np.sign(num) * (np.abs(num) // 10)).astype(np.int16)
    return out


@pytest.mark.parametrize("R,nc", [(16383, 12), (300, 13), (1000, 1)])
def test_delta_mfcc_with_vad_records(R, nc):
    """sr_delta_mfcc_batch_dev with VAD records: records that are not OK give zero rows whatever their frm_num, frm_num
    above max_frames is clamped; the frame-count form on the same rows"""
    gen = nc != 12
    eng = Engine(max_frames=R, device=0, **(dict(n_coef=nc, n_mel=26) if gen else {}))
    rng = np.random.default_rng(R + nc)
    recs = [(R, ST_OK), (1, ST_OK), (2, ST_OK), (R + 7, ST_OK), (65535, ST_OK), (R // 2, ST_MFCC_FAIL), (R, ST_VAD_FAIL),
            (5, ST_SEG_OOB), (0, ST_OK), (R - 1, ST_OK)]
    B = len(recs)
    mf = rng.integers(-32768, 32768, (B, R, nc)).astype(np.int16)
    vd = np.zeros((B, 12), np.int32)
    vd[:, 9] = [f for f, _ in recs]
    vd[:, 10] = [s for _, s in recs]
    dev = torch.device("cuda", 0)
    d_mf, d_vd = torch.from_numpy(mf).to(dev), torch.from_numpy(vd).to(dev)
    out = torch.full((B, R, nc), 0x3333, dtype=torch.int16, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert eng.L.sr_delta_mfcc_batch_dev(eng.h, vp(d_mf), vp(d_vd), None, C.c_uint32(B), vp(out), C.c_void_p(s)) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b, (f, st) in enumerate(recs):
        n = min(f, R) if st == ST_OK else 0
        assert np.array_equal(got[b], delta_definition(mf[b], n)), (b, f, st)
    fr = np.array([min(f, R) if st == ST_OK else 0 for f, st in recs], np.uint32)
    assert np.array_equal(eng.delta_mfcc(mf, fr), got)
    eng.close()
