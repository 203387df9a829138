"""The QUIET tier of the reference front end's frame kernel takes |X|*10 from a table instead of v_sqrt_f32
(csrc/sr_tables.h kMagTabEntries): t[n] = (u32)(sqrtf((float)n) * 10) << 2 for n = re^2 + im^2 <= 26 843, MFCC.C:58 evaluated
on the host.  CPU: the table itself against numpy and the oracle.  GPU: the kernel with the table against the same library
with the development hook "mag_table_off" (QUIET frames through the MID tier's independent arithmetic) and against the CPU
oracle, on batches large enough for the batch form of the kernel -- the form that reads the table."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import Engine, FEAT_MAG, FEAT_MEL
from test_frame_features import features, mel_from_mag, vad_segments, windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAG_SMALL_MAX = 26843  # csrc/sr_tables.h kMagSmallMax
N_SYNTH = 1024           # captures per gain: at or above the frame kernel's fill threshold, so the batch form runs
T_SYNTH = 32             # frames per synthetic capture


def mag_table(L=None):
    L = L or engine.load_library()
    L.sr_mag_table.restype = C.c_uint32
    n = L.sr_mag_table(None, C.c_uint32(0))
    out = np.zeros(n, np.uint16)
    assert L.sr_mag_table(out.ctypes.data_as(C.c_void_p), C.c_uint32(n)) == n
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_table_is_the_reference_expression_for_every_n():
    t = mag_table()
    assert len(t) == K_MAG_SMALL_MAX + 1
    n = np.arange(len(t), dtype=np.uint32)
    want = (np.sqrt(n.astype(np.float32)) * np.float32(10)).astype(np.uint32) << 2
    assert want.max() <= 0xFFFF                       # every value fits u16
    assert np.array_equal(t.astype(np.uint32), want)
    assert int(t[K_MAG_SMALL_MAX]) == 1638 << 2 and int(t[0]) == 0 and int(t[1]) == 10 << 2
    # the bound of the tier: the next magnitude step (1639) lies beyond the table, and the largest square is within the
    # fused filterbank term's range E <= 2^28 / 100 (sr_tables.h kMelFusedMaxE)
    assert (int(t[-1]) >> 2) ** 2 <= (1 << 28) // 100 and 100 * (K_MAG_SMALL_MAX + 1) < 1639 * 1639
    # a short read copies only what was asked for; both libraries hold the same table
    part = np.full(16, 0xFFFF, np.uint16)
    L = engine.load_library()
    assert L.sr_mag_table(part.ctypes.data_as(C.c_void_p), C.c_uint32(8)) == len(t)
    assert np.array_equal(part[:8], t[:8]) and (part[8:] == 0xFFFF).all()
    assert np.array_equal(mag_table(engine.load_library(testing=True)), t)


def test_table_equals_the_oracles_magnitude():
    """the oracle's own (u32)(sqrtf((float)n)*10) (sr_oracle_math_diag, MFCC.C:56-58) for every n of the table, and in
    particular for every n <= 26 843 that occurs in the spectra of the golden fixture"""
    t = mag_table().astype(np.uint32)
    orc = ol.Oracle()

    def oracle_mag(n):
        n = np.ascontiguousarray(n, np.uint32)
        out = np.zeros(3 * len(n), np.uint32)
        orc.L.sr_oracle_math_diag(n.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint32(len(n)))
        return out[2::3]

    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_golden.npz"))
    w = g["fft_out"][:, :512]
    re_ = (w & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
    im = (w >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    n = np.unique(re_ * re_ + im * im)
    n = n[n <= K_MAG_SMALL_MAX].astype(np.uint32)
    assert len(n) >= 100, len(n)
    assert np.array_equal(t[n] >> 2, oracle_mag(n))
    every = np.arange(len(t), dtype=np.uint32)
    assert np.array_equal(t >> 2, oracle_mag(every))


def test_hook_is_a_testing_build_hook_only():
    assert engine.load_library().sr_dev_hook(b"mag_table_off", C.c_int64(1)) == 3  # SR_ERR_BAD_ARG: not in the product library
    T = engine.load_library(testing=True)
    assert T.sr_dev_hook(b"mag_table_off", C.c_int64(0)) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def synth_captures(gain, n=N_SYNTH, T=T_SYNTH, seed=70):
    bank = synth.word_bank(10)
    return synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 10, [T] * n, seed=seed, bank=bank, S=synth.buf_len_for(T + 4), gain=gain))


def real_captures():
    """the 14 recorded captures, repeated to the batch form's fill threshold"""
    real = np.load(os.path.join(ROOT, "tests", "golden", "real_speech.npz"))["pcm"]
    return np.tile(real, ((N_SYNTH + len(real) - 1) // len(real), 1))


def every_segment(orc, pcm):
    """like vad_segments, with every segment the oracle's VAD finds in a capture as a row of its own (the recorded captures
    hold up to three words: 808 frames in all)"""
    rows, st, en, mid = [], [], [], []
    for i, row in enumerate(pcm):
        rc, a = orc.noise_atap(row)
        seg = orc.vad(row, a)
        for k in range(len(seg) // 2):
            if rc == 0 and seg[2 * k] >= 1 and seg[2 * k + 1] > seg[2 * k]:
                rows.append(i)
                st.append(seg[2 * k])
                en.append(seg[2 * k + 1])
                mid.append(a.mid_val)
    return pcm[rows], np.array(st, np.int32), np.array(en, np.int32), np.array(mid, np.uint32)


CASES = {"gain1.0": (lambda: synth_captures(1.0), 0.9, 1.01), "gain2.4": (lambda: synth_captures(2.4), 0.1, 0.6),
         "gain4.0": (lambda: synth_captures(4.0), -1.0, 1.01), "real": (real_captures, 0.9, 1.01)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_table_on_equals_table_off_and_the_oracle(case):
    """MFCC rows, SR_FEAT_MAG and SR_FEAT_MEL of every capture: the table against "mag_table_off" = 1 (the same library, QUIET
    frames through the MID tier) byte for byte, and both against the CPU oracle (get_mfcc; fft() of the windowed frame;
    MFCC.C:128-162 on the oracle's magnitudes).  The QUIET share of the frames (the oracle's frame_tiers) is what makes a case
    mean something: > 0.9 at gain 1.0 (and for the recorded speech: all of it), 0.1 .. 0.6 at gain 2.4."""
    make, q_lo, q_hi = CASES[case]
    raw = make()
    mf = 128 if case == "real" else T_SYNTH + 8
    orc = ol.Oracle(max_frames=mf)
    uniq = raw[:14] if case == "real" else raw
    tiers = orc.frame_tiers(uniq)
    print(case, "tiers", tiers)
    assert q_lo < tiers["quiet"] < q_hi and tiers["frames"] > 500, tiers
    pcm, st, en, mid = every_segment(orc, raw) if case == "real" else vad_segments(orc, raw)
    assert len(pcm) >= 1000, len(pcm)
    n_uniq = len(every_segment(orc, uniq)[0]) if case == "real" else len(pcm)
    eng = Engine(max_frames=mf, device=0, testing=True)
    on = {k: features(eng, pcm, st, en, mid, k, want_mfcc=True) for k in (FEAT_MAG, FEAT_MEL)}
    engine.dev_hook("mag_table_off", 1)
    try:
        off = {k: features(eng, pcm, st, en, mid, k, want_mfcc=True) for k in (FEAT_MAG, FEAT_MEL)}
    finally:
        engine.dev_hook("mag_table_off", 0)
    n = on[FEAT_MAG][1]
    assert (on[FEAT_MAG][2] == 0).all() and n.min() > 0
    for k in (FEAT_MAG, FEAT_MEL):
        for a, b in zip(on[k], off[k]):
            assert a.tobytes() == b.tobytes(), k
    assert on[FEAT_MAG][3].tobytes() == on[FEAT_MEL][3].tobytes()
    # the CPU oracle: every distinct capture (the recorded ones repeat)
    tab = orc.tables()
    frames = windows_of(orc, pcm[:n_uniq], st, n[:n_uniq], mid)
    if case == "real":
        assert int(n[:n_uniq].sum()) == 808
    for b in range(n_uniq):
        atap = ol.Atap(int(mid[b]), 0, 0, 0)
        n_o, mf_o = orc.mfcc(pcm[b], int(st[b]), int(en[b]), atap)
        assert n_o == n[b] and np.array_equal(on[FEAT_MAG][3][b, :n_o], mf_o), b
        mag = np.stack([orc.fft_mag(f) for f in frames[b]])
        assert np.array_equal(on[FEAT_MAG][0][b, :n[b]], mag), b
        assert np.array_equal(on[FEAT_MEL][0][b, :n[b]], mel_from_mag(mag, tab)[0]), b
    if case == "real":  # the repeats equal their originals
        for k in (FEAT_MAG, FEAT_MEL):
            f = on[k][0]
            assert len(f) % n_uniq == 0 and (f.reshape(len(f) // n_uniq, n_uniq, *f.shape[1:]) == f[:n_uniq]).all()


@pytest.mark.gpu
def test_first_call_with_a_cold_table_equals_the_tenth():
    """the first launch after sr_create finds the table in HBM only"""
    pcm = synth_captures(1.0, seed=71)
    orc = ol.Oracle(max_frames=T_SYNTH + 8)
    pcm, st, en, mid = vad_segments(orc, pcm)
    eng = Engine(max_frames=T_SYNTH + 8, device=0)
    first = eng.mfcc_status(pcm, st, en, mid)
    for _ in range(8):
        eng.mfcc_status(pcm, st, en, mid)
    tenth = eng.mfcc_status(pcm, st, en, mid)
    assert first[0].min() > 0 and first[1].any()
    for a, b in zip(first, tenth):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_small_launch_forms_equal_the_batch_form():
    """one capture alone (the one-frame-per-wave form) and 64 captures (the four-frame form) keep the root; the batch form
    reads the table: identical rows, magnitudes and Mel energies"""
    pcm = synth_captures(1.0, seed=72)
    orc = ol.Oracle(max_frames=T_SYNTH + 8)
    pcm, st, en, mid = vad_segments(orc, pcm)
    assert len(pcm) >= 1000
    eng = Engine(max_frames=T_SYNTH + 8, device=0)
    for kind in (FEAT_MAG, FEAT_MEL):
        fb, nb, sb, mb = features(eng, pcm, st, en, mid, kind, want_mfcc=True)
        for b in (0, 7, 500):
            f1, n1, s1, m1 = features(eng, pcm[b:b + 1], st[b:b + 1], en[b:b + 1], mid[b:b + 1], kind, want_mfcc=True)
            assert n1[0] == nb[b] and np.array_equal(f1[0], fb[b]) and np.array_equal(m1[0], mb[b]), (kind, b)
        f64, n64, s64, m64 = features(eng, pcm[:64], st[:64], en[:64], mid[:64], kind, want_mfcc=True)
        assert np.array_equal(f64, fb[:64]) and np.array_equal(m64, mb[:64]) and np.array_equal(n64, nb[:64])
