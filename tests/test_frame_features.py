"""Per-frame intermediate values of the front end (sr_frame_features_batch*, SR_FEAT_*): the FFT words, |X|*10, the Mel
energies and their log*100, emitted by the production frame kernels (k_mfcc, k_mfcc_ext, k_mfcc_gen) at the point where each
value exists, checked value for value against the oracles -- the hot path's FFT and magnitude tiers bin for bin instead of
through log -> DCT -> s16 only."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import oracle_lib as ol
from conftest import needs_ref_objects
from stm32_speech_recognition_amd import SrError, engine, synth
from stm32_speech_recognition_amd.engine import Engine, FEAT_FFT, FEAT_LOGMEL, FEAT_MAG, FEAT_MEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
KINDS = (FEAT_FFT, FEAT_MAG, FEAT_MEL, FEAT_LOGMEL)
EXT = dict(fs=16000, nfft=512, n_mel=40)


# ---- CPU: the header and the Python mirror -------------------------------------------------------------------------------
def test_header_declares_frame_feature_api_and_python_mirrors_it():
    src = open(HEADER).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+SR_FEAT_(\w+)\s+(\d+)", src)}
    assert consts == {"FFT": FEAT_FFT, "MAG": FEAT_MAG, "MEL": FEAT_MEL, "LOGMEL": FEAT_LOGMEL}
    assert len(set(consts.values())) == 4 and 0 not in consts.values()
    for fn in ("sr_frame_feature_width", "sr_frame_features_batch_dev", "sr_frame_features_batch"):
        assert re.search(r"\b%s\s*\(" % fn, src), fn
        assert hasattr(engine.load_library(), fn), fn
    assert hasattr(Engine, "frame_features") and hasattr(Engine, "frame_features_dev")


# ---- numpy restatements of MFCC.C ----------------------------------------------------------------------------------------
def cdiv(a, b):
    """C division of int64 arrays by a positive constant: truncation toward zero"""
    q = np.abs(a) // b
    return np.where(a < 0, -q, q)


def windowed(pcm, start, n, frame_len, hop, mid, hamm):
    """MFCC.C:115-124 for frames 0..n-1 of the segment at `start`: temp = (x - mid) - (x_prev - mid)*95/100 (integer),
    (s16)(temp*hamm/1000), C truncation -> int16 [n, frame_len]"""
    idx = start + hop * np.arange(n)[:, None] + np.arange(frame_len)[None, :]
    x = pcm[idx].astype(np.int64) - mid
    xp = pcm[idx - 1].astype(np.int64) - mid
    temp = x - cdiv(xp * 95, 100)
    return cdiv(temp * hamm.astype(np.int64)[None, :], 1000).astype(np.int16)


def fft_words(frames):
    """fft()'s input array (MFCC.C:37-44): the s16 samples as u16 real parts, imaginary 0, zero padded to 1024"""
    w = np.zeros((len(frames), 1024), np.uint32)
    w[:, :frames.shape[1]] = frames.view(np.uint16)
    return w


def mag_from_words(words):
    """MFCC.C:49-60 on packed words: (u32)(sqrtf((float)(re*re + im*im))*10)"""
    re_ = (words & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    im = (words >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    n = (re_ * re_ + im * im).astype(np.int32)
    return (np.sqrt(n.astype(np.float32)) * np.float32(10)).astype(np.uint32)


def mel_from_mag(mag, tab):
    """MFCC.C:128-162: E = mag^2, every term E*tri/100 and every sum u32-wrapping.  Returns (mel u32 [n, n_mel], whether
    any term wrapped)"""
    E = (mag.astype(np.uint64) * mag.astype(np.uint64)) & 0xFFFFFFFF
    nb, cen = mag.shape[1], tab["tri_cen"].astype(np.int64)
    nm = len(cen)
    out = np.zeros((len(mag), nm), np.uint64)
    wrapped = False
    for h in range(nm):
        lo = 0 if h == 0 else cen[h - 1]
        hi = nb if h == nm - 1 else cen[h + 1]
        tri = (tab["tri_even"] if h % 2 == 0 else tab["tri_odd"])[lo:hi].astype(np.uint64)
        prod = E[:, lo:hi] * tri[None, :]
        wrapped |= bool((prod > 0xFFFFFFFF).any())
        out[:, h] = ((prod & 0xFFFFFFFF) // 100).sum(axis=1) & 0xFFFFFFFF
    return out.astype(np.uint32), wrapped


def log100(orc, x):
    """sr_oracle_math_diag's (u32)(log((double)x)*100), 0 for x = 0 (MFCC.C:168)"""
    x = np.ascontiguousarray(x, np.uint32).reshape(-1)
    out = np.zeros(3 * len(x), np.uint32)
    orc.L.sr_oracle_math_diag(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint32(len(x)))
    return out[0::3]


def dct_rows(logmel, dct, n_coef):
    """MFCC.C:173-183: (s32)pow * dct / 100 truncated, accumulated into an s16"""
    d = dct.astype(np.int64).reshape(n_coef, -1)
    terms = cdiv(logmel.astype(np.int64)[:, None, :] * d[None, :, :], 100)
    return (terms.sum(axis=2) & 0xFFFF).astype(np.uint16).view(np.int16)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def vad_segments(orc, pcm):
    """segment 0 + mid value of every capture by the oracle's noise_atap / VAD (captures without one are dropped)"""
    rows, st, en, mid = [], [], [], []
    for i, row in enumerate(pcm):
        rc, a = orc.noise_atap(row)
        seg = orc.vad(row, a)
        if rc == 0 and seg[0] >= 1 and seg[1] > seg[0]:
            rows.append(i)
            st.append(seg[0])
            en.append(seg[1])
            mid.append(a.mid_val)
    return pcm[rows], np.array(st, np.int32), np.array(en, np.int32), np.array(mid, np.uint32)


def synth_batch(gains, n=8, T=64, rate=1):
    bank = synth.word_bank(10)
    out = [synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 10, [T] * n, seed=40 + k, bank=bank,
                                                    S=synth.buf_len_for(T + 4, rate), gain=g, rate=rate))
           for k, g in enumerate(gains)]
    return np.concatenate(out)


def extreme_batch(S=4000, fl=160):
    """explicit segments of full-swing captures (the window's s16 wraps), a full-scale sine and a flat one (every energy 0):
    returns pcm, start, end, mid"""
    t = np.arange(S)
    rows = [np.where(t % 2 == 0, 0, 4095), np.where((t // 3) % 2 == 0, 0, 4095),
            np.clip(np.round(2048 + 2047 * np.sin(2 * np.pi * 1000 * t / 8000)), 0, 4095), np.full(S, 2048),
            np.where((t // 7) % 2 == 0, 100, 4000)]
    pcm = np.stack(rows).astype(np.uint16)
    n = len(rows)
    return pcm, np.full(n, 1, np.int32), np.full(n, 1 + fl + 20 * (fl // 2), np.int32), np.full(n, 2048, np.uint32)


def features(eng, pcm, st, en, mid, kind, want_mfcc=False):
    r = eng.frame_features(pcm, st, en, mid, kind, want_mfcc=want_mfcc)
    assert r[0].shape[2] == eng.frame_feature_width(kind)
    return r


def check_rows_zero(feat, n):
    for b in range(len(n)):
        assert not feat[b, n[b]:].any(), b


def windows_of(orc, pcm, st, n, mid):
    tab = orc.tables()
    return [windowed(pcm[b], int(st[b]), int(n[b]), orc.frame_len, orc.hop, int(mid[b]), tab["hamm"]) for b in range(len(n))]


# ---- GPU: every kind against the oracles ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_setup():
    mf = 128
    eng, orc = Engine(max_frames=mf, device=0), ol.Oracle(max_frames=mf)
    pcm = synth_batch((1.0, 2.4, 4.0))
    real = np.load(os.path.join(ROOT, "tests", "golden", "real_speech.npz"))["pcm"]
    tiers = orc.frame_tiers(pcm)
    assert tiers["quiet"] > 0 and tiers["mid"] > 0 and tiers["loud"] > 0, tiers
    both = np.full((len(pcm) + len(real), max(pcm.shape[1], real.shape[1])), 2048, np.uint16)  # (trailing silence)
    both[:len(pcm), :pcm.shape[1]], both[len(pcm):, :real.shape[1]] = pcm, real
    p, st, en, mid = vad_segments(orc, both)
    assert len(p) >= 30
    return eng, orc, p, st, en, mid


@pytest.mark.gpu
def test_mag_reference_front_end_every_tier_bin_for_bin(ref_setup):
    """MAG is what the magnitude stage of k_mfcc consumed (QUIET / MID / LOUD tier alike): every bin of every frame equals
    the oracle's fft() (MFCC.C:27-62) of the windowed frame built in numpy"""
    eng, orc, pcm, st, en, mid = ref_setup
    feat, n, status = features(eng, pcm, st, en, mid, FEAT_MAG)
    assert (status == 0).all() and n.min() > 0
    check_rows_zero(feat, n)
    frames = windows_of(orc, pcm, st, n, mid)
    for b, fr in enumerate(frames):
        want = np.stack([orc.fft_mag(f) for f in fr])
        assert np.array_equal(feat[b, :n[b]], want), b


@pytest.mark.gpu
@needs_ref_objects
def test_mag_against_the_references_own_fft(ref_setup):
    """a few hundred frames against the fft symbol of the reference's own MFCC.C object"""
    eng, orc, pcm, st, en, mid = ref_setup
    feat, n, _ = features(eng, pcm, st, en, mid, FEAT_MAG)
    L = C.CDLL(ol.REF_PATH)
    L.fft.restype = C.POINTER(C.c_uint32)
    frames = windows_of(orc, pcm, st, n, mid)
    checked = 0
    for b in range(0, len(frames), 3):
        for f in range(0, int(n[b]), 2):
            x = np.ascontiguousarray(frames[b][f])
            p = L.fft(x.ctypes.data_as(C.c_void_p), C.c_uint16(len(x)))
            assert np.array_equal(feat[b, f], np.ctypeslib.as_array(p, shape=(512,))), (b, f)
            checked += 1
    assert checked >= 300


@pytest.mark.gpu
def test_fft_words_equal_the_product_fft_and_the_reference(ref_setup):
    """FFT = the pass-5 output words of k_mfcc's transform, bins 0..511, equal to cr4_fft_1024_stm32's words (the product's
    full transform, sr_fft_q15_batch, and with the reference objects the C transcription of the asm) -- also on full-swing
    frames whose windowed samples wrap in s16"""
    eng, orc, pcm, st, en, mid = ref_setup
    xp, xs, xe, xm = extreme_batch()
    for P, S_, E_, M_ in ((pcm, st, en, mid), (xp, xs, xe, xm)):
        feat, n, status = features(eng, P, S_, E_, M_, FEAT_FFT)
        assert (status == 0).all()
        check_rows_zero(feat, n)
        frames = windows_of(orc, P, S_, n, M_)
        words = fft_words(np.concatenate(frames))
        got = np.concatenate([feat[b, :n[b]] for b in range(len(n))])
        assert np.array_equal(got, eng.fft_q15(words)[:, :512])
        assert np.array_equal(mag_from_words(got), np.stack([orc.fft_mag(f) for f in np.concatenate(frames)]))
        if ol.RefLib.available():
            R = ol.RefLib()
            for i in range(0, len(words), max(1, len(words) // 200)):
                assert np.array_equal(got[i], R.fft(words[i])[:512]), i
    wide = windows_of(orc, xp, xs, np.array([20] * len(xp)), xm)
    full = np.concatenate(wide).astype(np.int64)
    assert np.abs(full).max() >= 30000  # full-scale windowed samples were part of the test


@pytest.mark.gpu
def test_mel_and_logmel_reference_front_end(ref_setup):
    """MEL = pow_spct before the log (u32-wrapping terms and sums, MFCC.C:128-162) from the oracle's magnitudes and tables;
    LOGMEL = (u32)(log(MEL)*100) with LOGMEL = 0 where MEL = 0; its DCT (MFCC.C:173-183) is the MFCC row of
    sr_mfcc_batch_status and of the feature call itself"""
    eng, orc, pcm, st, en, mid = ref_setup
    xp, xs, xe, xm = extreme_batch()
    tab = orc.tables()
    saw_wrap, saw_zero = False, False
    for P, S_, E_, M_ in ((pcm, st, en, mid), (xp, xs, xe, xm)):
        mel, n, status = features(eng, P, S_, E_, M_, FEAT_MEL)
        lg, n2, status2, mf = features(eng, P, S_, E_, M_, FEAT_LOGMEL, want_mfcc=True)
        assert np.array_equal(n, n2) and np.array_equal(status, status2) and (status == 0).all()
        check_rows_zero(mel, n)
        check_rows_zero(lg, n)
        n_ref, mf_ref, st_ref = eng.mfcc_status(P, S_, E_, M_)
        assert np.array_equal(n_ref, n) and np.array_equal(st_ref, status) and np.array_equal(mf, mf_ref)
        for b, fr in enumerate(windows_of(orc, P, S_, n, M_)):
            mag = np.stack([orc.fft_mag(f) for f in fr])
            want, wrapped = mel_from_mag(mag, tab)
            saw_wrap |= wrapped
            assert np.array_equal(mel[b, :n[b]], want), b
            assert np.array_equal(lg[b, :n[b]].reshape(-1), log100(orc, want)), b
            saw_zero |= bool((want == 0).any())
            assert (lg[b, :n[b]][want == 0] == 0).all()
            assert np.array_equal(dct_rows(lg[b, :n[b]], tab["dct"], eng.n_coef), mf_ref[b, :n[b]]), b
    assert saw_wrap and saw_zero


def _front_end_kinds(ekw, okw, rate, fl):
    """kinds 1-4 of one front end against the oracle's fft() / tables / log (no reference counterpart for its constants)"""
    mf = 80
    eng, orc = Engine(max_frames=mf, device=0, **ekw), ol.Oracle(max_frames=mf, **okw)
    assert orc.frame_len == fl
    pcm = synth_batch((1.0, 4.0), n=6, T=48, rate=rate)
    P, st, en, mid = vad_segments(orc, pcm)
    assert len(P) >= 8
    tab = orc.tables()
    got = {k: features(eng, P, st, en, mid, k, want_mfcc=True) for k in KINDS}
    n = got[FEAT_MAG][1]
    assert (got[FEAT_MAG][2] == 0).all() and n.min() > 0
    n_ref, mf_ref, _ = eng.mfcc_status(P, st, en, mid)
    assert np.array_equal(n_ref, n)
    for k in KINDS:
        check_rows_zero(got[k][0], n)
        assert np.array_equal(got[k][3], mf_ref), k
    assert got[FEAT_FFT][0].shape[2] == got[FEAT_MAG][0].shape[2] == orc.cfg.nfft // 2
    assert got[FEAT_MEL][0].shape[2] == got[FEAT_LOGMEL][0].shape[2] == orc.n_mel
    for b, fr in enumerate(windows_of(orc, P, st, n, mid)):
        mag = np.stack([orc.fft_mag(f) for f in fr])
        assert np.array_equal(got[FEAT_MAG][0][b, :n[b]], mag), b
        assert np.array_equal(mag_from_words(got[FEAT_FFT][0][b, :n[b]]), mag), b
        mel, _ = mel_from_mag(mag, tab)
        assert np.array_equal(got[FEAT_MEL][0][b, :n[b]], mel), b
        lg = got[FEAT_LOGMEL][0][b, :n[b]]
        assert np.array_equal(lg.reshape(-1), log100(orc, mel)), b
        assert np.array_equal(dct_rows(lg, tab["dct"], eng.n_coef), mf_ref[b, :n[b]]), b
    return eng, orc, P, st, en, mid, got


@pytest.mark.gpu
def test_extension_front_end_kinds():
    """EXTENSION front end (k_mfcc_ext, 16 kHz / 512 points / 40 Mel; no reference counterpart): widths 256 / 256 / 40 / 40"""
    eng = _front_end_kinds(EXT, EXT, 2, 320)[0]
    assert [eng.frame_feature_width(k) for k in KINDS] == [256, 256, 40, 40]


@pytest.mark.gpu
@pytest.mark.parametrize("ci,rate", [(0, 1), (1, 2)])
def test_generic_front_end_kinds(ci, rate):
    """GENERIC front end (k_mfcc_gen; no reference counterpart for its constants): the FFT words are the reference's
    1024-point transform, so they also equal the product's full FFT on the numpy-windowed frames"""
    ekw, okw = ol.GENERIC_CONFIGS[ci]
    probe = ol.Oracle(max_frames=8, **okw)
    eng, orc, P, st, en, mid, got = _front_end_kinds(ekw, okw, rate, probe.frame_len)
    assert [eng.frame_feature_width(k) for k in KINDS] == [512, 512, orc.n_mel, orc.n_mel]
    n = got[FEAT_FFT][1]
    fr = np.concatenate(windows_of(orc, P, st, n, mid))
    words = np.concatenate([got[FEAT_FFT][0][b, :n[b]] for b in range(len(n))])
    assert np.array_equal(words, eng.fft_q15(fft_words(fr))[:, :512])


# ---- GPU: launch forms, layout, failures, device form --------------------------------------------------------------------
def _short_captures(n, T=12):
    bank = synth.word_bank(6)
    return synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 6, [T] * n, seed=3, bank=bank, S=synth.buf_len_for(T + 2), gain=2.4))


@pytest.mark.gpu
def test_launch_forms_give_identical_rows():
    """B = 1 and 256 at a cap of 128 frames (k_mfcc's 1- and 4-frames-per-wave forms: 8 / 2 048 work items of 16 frames
    against kMfccFill = 1 024) and B = 4 096 at a cap of 16 frames (the 64-frame batch form, 4 096 items strided over a
    grid of 256 workgroups, set with the "mfcc_grid" test hook): identical feature rows and MFCC rows"""
    base = _short_captures(32)
    orc = ol.Oracle(max_frames=16)
    P, st, en, mid = vad_segments(orc, base)
    assert len(P) >= 16
    P, st, en, mid = P[:16], st[:16], en[:16], mid[:16]
    big = Engine(max_frames=128, device=0)
    engine.dev_hook("mfcc_grid", 256)
    try:
        small = Engine(max_frames=16, device=0, testing=True)
    finally:
        engine.dev_hook("mfcc_grid", 0)
    for kind in KINDS:
        f256, n256, s256, m256 = features(big, np.tile(P, (16, 1)), np.tile(st, 16), np.tile(en, 16), np.tile(mid, 16), kind, True)
        assert (s256 == 0).all() and n256.max() <= 16
        check_rows_zero(f256, n256)
        for b in range(3):
            f1, n1, _, m1 = features(big, P[b:b + 1], st[b:b + 1], en[b:b + 1], mid[b:b + 1], kind, True)
            assert np.array_equal(f1[0], f256[b]) and np.array_equal(m1[0], m256[b])
        f4k, n4k, s4k, m4k = features(small, np.tile(P, (256, 1)), np.tile(st, 256), np.tile(en, 256), np.tile(mid, 256),
                                      kind, True)
        assert np.array_equal(n4k, np.tile(n256[:16], 256)) and (s4k == 0).all()
        check_rows_zero(f4k, n4k)
        want = f256[:16, :16]
        assert np.array_equal(f4k.reshape(256, 16, 16, -1), np.broadcast_to(want, (256,) + want.shape)), kind
        assert np.array_equal(m4k[:16], m256[:16, :16])
        del f256, f4k


@pytest.mark.gpu
def test_failed_records_have_zero_rows_and_the_mfcc_status():
    eng = Engine(max_frames=40, device=0)
    pcm = _short_captures(6, T=30)
    S = pcm.shape[1]
    st = np.array([0, 3000, 3000, 3000, 2000, 3000], np.int32)          # OOB start / ok / shorter than a frame / end < start /
    en = np.array([2000, 3100, 3100, S + 5, 2000 + 80 * 60, 5000], np.int32)  # end past the buffer / > 40 frames / ok
    en[1] = 3000 + 160 + 80 * 9                                         # 10 frames
    en[2] = 3000 + 100
    st[3], en[3] = 3000, 2990
    mid = np.full(6, 2048, np.uint32)
    n_ref, mf_ref, st_ref = eng.mfcc_status(pcm, st, en, mid)
    assert set(st_ref.tolist()) >= {0, 2, 3}
    for kind in KINDS:
        feat, n, status, mf = features(eng, pcm, st, en, mid, kind, True)
        assert np.array_equal(status, st_ref) and np.array_equal(n, n_ref) and np.array_equal(mf, mf_ref)
        check_rows_zero(feat, n)
        assert not feat[status != 0].any()
        assert feat[status == 0].any()


@pytest.mark.gpu
def test_device_form_on_a_side_stream_equals_the_host_form():
    eng = Engine(max_frames=80, device=0)
    bank = synth.word_bank(6)
    pcm_t = synth.make_utterances(np.arange(12) % 6, [60] * 12, seed=21, bank=bank, device="cuda:0", gain=2.4)
    vad, mfcc = eng.features_dev(pcm_t)
    torch.cuda.synchronize()
    v = engine.vad_from_torch(vad)
    ok = v["status"] == 0
    assert ok.sum() >= 8
    pcm = synth.as_u16_numpy(pcm_t)
    side = torch.cuda.Stream()
    for kind in KINDS:
        mf_dev = torch.zeros_like(mfcc)
        with torch.cuda.stream(side):
            feat_t = eng.frame_features_dev(pcm_t, vad, kind, mfcc=mf_dev, stream=side)
        side.synchronize()
        feat = feat_t.cpu().numpy().view(np.uint32)
        assert np.array_equal(mf_dev.cpu().numpy(), mfcc.cpu().numpy())
        hf, n, status = features(eng, pcm[ok], v["seg"][ok, 0], v["seg"][ok, 1], v["mid_val"][ok], kind)
        assert np.array_equal(n, v["frm_num"][ok]) and (status == 0).all()
        assert np.array_equal(feat[ok], hf), kind
        check_rows_zero(feat, v["frm_num"])
        assert eng.frame_features_dev(pcm_t, vad, kind).shape == feat_t.shape  # d_mfcc = NULL: engine scratch


@pytest.mark.gpu
def test_bad_kind_or_null_feature_buffer():
    eng = Engine(max_frames=40, device=0)
    pcm = _short_captures(2, T=20)
    st, en, mid = np.array([3000, 3000], np.int32), np.array([4600, 4600], np.int32), np.array([2048, 2048], np.uint32)
    for kind in (0, 5, -1):
        assert eng.frame_feature_width(kind) == 0
        with pytest.raises(SrError, match="error 3.*feature kind"):
            eng.frame_features(pcm, st, en, mid, kind)
    L = eng.L
    p = pcm.ctypes.data_as(C.c_void_p)
    a = [x.ctypes.data_as(C.c_void_p) for x in (st, en, mid)]
    rc = L.sr_frame_features_batch(eng.h, C.c_int(FEAT_MEL), p, C.c_uint64(pcm.shape[1]), C.c_uint32(pcm.shape[1]),
                                   C.c_uint32(2), *a, None, None, None, None)
    assert rc == 3 and b"null" in L.sr_last_error()
    d_pcm = torch.from_numpy(pcm.view(np.int16)).to("cuda:0")
    d_vad = torch.zeros(2, 12, dtype=torch.int32, device="cuda:0")
    for kind, feat in ((FEAT_MEL, None), (7, torch.zeros(1, dtype=torch.int32, device="cuda:0"))):
        rc = L.sr_frame_features_batch_dev(eng.h, C.c_int(kind), C.c_void_p(d_pcm.data_ptr()), C.c_uint64(pcm.shape[1]),
                                           C.c_uint32(2), C.c_void_p(d_vad.data_ptr()),
                                           None if feat is None else C.c_void_p(feat.data_ptr()), None, None)
        assert rc == 3 and L.sr_last_error()
