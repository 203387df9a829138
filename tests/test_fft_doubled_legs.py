"""k_mfcc's doubled-leg butterflies (csrc/sr_fft_dev.h: legs of passes 2-5 enter their multiply as 2 Y, so that X >> 15 is a
byte-aligned pick and X >> 16 one packed shift of it) against the oracles, bit for bit: the pass-5 words, the magnitudes of
every tier and the MFCC rows, in every launch form of the frame kernel, on frame counts that exercise the peeled first / last
frame of the two-frame loop, one-frame waves and the tile boundary, at amplitudes from the benchmark's to captures whose
windowed samples wrap in s16 -- the form rests on a bound of the transform's intermediate values (tests/test_fft_leg_bounds.py)
that has to hold for EVERY 16-bit capture."""
import numpy as np
import pytest

import oracle_lib as ol
from stm32_speech_recognition_amd import synth
from stm32_speech_recognition_amd.engine import Engine, FEAT_FFT, FEAT_MAG
from test_frame_features import fft_words, mag_from_words, windows_of

# one full 64-frame tile + a one-frame tile, a wave of 16 + a wave of 1, a full wave, the peeled pair, a single frame
FRAMES = np.array([65, 17, 64, 16, 2, 1])
MF = 128
BATCH, SMALL = 1, 2  # sr_set_small_launch: never / always the forms for underfilled launches
QUIET_MAX, CHEAP_MAX = 26843, 70171  # csrc/sr_tables.h: kMagSmallMax, kMagCheapMax on gfx950


def segments(start, n, fl=160, hop=80):
    st = np.full(len(n), start, np.int32)
    return st, (st + fl + hop * (np.asarray(n) - 1)).astype(np.int32)


def synth_case(gain, seed):
    """the benchmark's generator: six 70-frame words, frames taken from inside the word"""
    bank = synth.word_bank(10)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(6), [70] * 6, seed=seed, bank=bank, S=synth.buf_len_for(72), gain=gain))
    st, en = segments(synth.NOISE_LEN + synth.LEAD_QUIET + synth.HOP, FRAMES)
    return pcm, st, en, np.full(6, synth.MID, np.uint32)


def adversarial_case(lo, hi, order, seed, S=5600):
    """+-full-scale captures between the codes lo and hi around mid = (lo + hi + 1) / 2: constant, alternating (bin 512), full-
    scale sinusoids at the bins whose coefficient is +-1 or +-i in some pass (periods 4, 8 and 16 samples = bins 256, 128, 64) and
    seeded +-full-scale noise.  order: which pattern gets which frame count."""
    t = np.arange(S)
    mid, amp = (lo + hi + 1) // 2, (hi - lo) // 2
    rng = np.random.default_rng(seed)
    rows = [np.full(S, hi), np.where(t % 2 == 0, lo, hi)]
    rows += [np.clip(np.round(mid + amp * np.sin(2 * np.pi * t / p + 0.3)), lo, hi) for p in (4, 8, 16)]
    rows.append(np.where(rng.integers(0, 2, S) == 0, lo, hi))
    pcm = np.stack(rows).astype(np.uint16)[order]
    st, en = segments(1, FRAMES)
    return pcm, st, en, np.full(6, mid, np.uint32)


@pytest.fixture(scope="module")
def setup():
    return Engine(max_frames=MF, device=0), ol.Oracle(max_frames=MF)


def oracle_rows(orc, pcm, st, en, mid):
    """per capture: windowed frames (numpy, MFCC.C:115-124), the oracle's magnitudes (MFCC.C:27-62) and MFCC rows, frame peaks"""
    frames = windows_of(orc, pcm, st, FRAMES, mid)
    mags = [np.stack([orc.fft_mag(f) for f in fr]) for fr in frames]
    mf, peaks = [], []
    for b in range(len(pcm)):
        a = ol.Atap()
        a.mid_val = int(mid[b])
        n, m = orc.mfcc(pcm[b], int(st[b]), int(en[b]), a)
        assert n == FRAMES[b]
        mf.append(m)
        peaks.append(orc.frame_peaks(pcm[b], int(st[b]), int(en[b]), a))
    return frames, mags, mf, np.concatenate(peaks)


def check(eng, case, ref, mode):
    pcm, st, en, mid = case
    frames, mags, mf_ref, _ = ref
    eng.set_small_launch(mode)
    try:
        words, n, status, mf = eng.frame_features(pcm, st, en, mid, FEAT_FFT, want_mfcc=True)
        mag, n2, status2 = eng.frame_features(pcm, st, en, mid, FEAT_MAG)
        plain = eng.fft_q15(fft_words(np.concatenate(frames)))[:, :512]  # the product's full transform: plain butterflies
    finally:
        eng.set_small_launch(0)
    assert (status == 0).all() and (status2 == 0).all()
    assert np.array_equal(n, FRAMES) and np.array_equal(n2, FRAMES)
    got = np.concatenate([words[b, :n[b]] for b in range(len(n))])
    assert np.array_equal(got, plain)
    for b in range(len(n)):
        assert np.array_equal(mag_from_words(words[b, :n[b]]), mags[b]), b
        assert np.array_equal(mag[b, :n[b]], mags[b]), b
        assert np.array_equal(mf[b, :n[b]], mf_ref[b]), b
        assert not words[b, n[b]:].any() and not mag[b, n[b]:].any() and not mf[b, n[b]:].any(), b


CASES = {
    "gain1": lambda: synth_case(1.0, 71),
    "gain4": lambda: synth_case(4.0, 72),
    "adc12": lambda: adversarial_case(0, 4095, np.arange(6), 73),
    "full16": lambda: adversarial_case(0, 65535, np.roll(np.arange(6), 3), 74),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_batch_form_bit_for_bit(setup, name):
    """the 16-frames-per-wave form with its two-frame loop (what the benchmark runs), B = 6"""
    eng, orc = setup
    case = CASES[name]()
    ref = oracle_rows(orc, *case)
    peaks = ref[3]
    if name == "gain1":
        assert (peaks <= QUIET_MAX).mean() > 0.5  # the table tier
    if name == "gain4":
        assert (peaks > CHEAP_MAX).any()          # the exact-root tier
    if name == "full16":
        assert np.abs(np.concatenate(ref[0]).astype(np.int64)).max() >= 30000  # windowed samples at the s16 range's ends
    check(eng, case, ref, BATCH)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gain1", "full16"])
def test_one_frame_per_wave_form_bit_for_bit(setup, name):
    """the form for underfilled launches (forced; also what B = 6 gets by default)"""
    eng, orc = setup
    case = CASES[name]()
    ref = oracle_rows(orc, *case)
    check(eng, case, ref, SMALL)
    check(eng, case, ref, 0)


@pytest.mark.gpu
def test_four_frames_per_wave_form_bit_for_bit(setup):
    """B = 132 at a cap of 128 frames: 1 056 work items of 16 frames reach the fill mark, 264 of 64 do not -> the middle form"""
    eng, orc = setup
    pcm, st, en, mid = CASES["full16"]()
    frames, mags, mf_ref, _ = oracle_rows(orc, pcm, st, en, mid)
    R = 22
    words, n, status, mf = eng.frame_features(np.tile(pcm, (R, 1)), np.tile(st, R), np.tile(en, R), np.tile(mid, R), FEAT_FFT,
                                              want_mfcc=True)
    assert (status == 0).all() and np.array_equal(n, np.tile(FRAMES, R))
    for b in range(6):
        assert np.array_equal(mag_from_words(words[b, :n[b]]), mags[b]), b
        assert np.array_equal(mf[b, :n[b]], mf_ref[b]), b
    w6, m6 = words[:6], mf[:6]
    assert np.array_equal(words.reshape(R, 6, MF, -1), np.broadcast_to(w6, (R,) + w6.shape))
    assert np.array_equal(mf.reshape(R, 6, MF, -1), np.broadcast_to(m6, (R,) + m6.shape))
