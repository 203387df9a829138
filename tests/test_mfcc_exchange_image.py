"""The frame kernel of the reference front end (csrc/k_mfcc.hip) transposes a frame twice through the wave's LDS area: between
FFT passes 3 and 4 (the exchange) and between the magnitudes and the filterbank (the energies).  Both images are written by
lane-contiguous stores and read as 16-byte words (csrc/sr_fft_layout.h), so a wrong plane base, a wrong lane digit of the FFT
front, a wrong coefficient row or a misplaced 16-byte read moves whole groups of bins -- of one frame.  The layout itself is
checked on the CPU (tests/fft_layout/layout_check.cpp, a stand-alone program under the sanitizers); here the kernel is run on
inputs where every misplaced word shows:

  impulse     160 one-frame segments of a flat capture with one sample of amplitude 20 000 at position i = 0..159 of the frame:
              the windowed frame is non-zero at samples i and i + 1 only (pre-emphasis), so every one of the 160 non-padding
              inputs of the transform is exercised alone
  full scale  alternating 0 / 65 535 samples and full-scale noise, segments of 1, 2, 17 and 64 frames: LOUD frames, every plane of
              the energies image carries large values (and the window's s16 wraps)
  quiet       17 frames of a synthetic word at gain 1.0: the QUIET tier, the two-frame pipeline's peeled first and last frames
              and one steady iteration of the batch form

Every case runs in the three forms of the kernel -- batches of 1, 100 and 208 captures at max_frames 320 select them, as in
tests/test_mfcc_lds_traffic.py -- and is compared byte for byte with the CPU oracle: MFCC rows, |X|*10 (MAG), the filterbank
outputs (MEL), and the FFT words through their magnitudes and, as words, with the product's full transform (eng.fft_q15, an
independent kernel).  Rows >= frm_num are zero."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from stm32_speech_recognition_amd import synth
from stm32_speech_recognition_amd.engine import Engine, FEAT_FFT, FEAT_MAG, FEAT_MEL
from test_frame_features import features, fft_words, mag_from_words, mel_from_mag, vad_segments, windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
MAX_FRAMES = 320
FRAME, HOP = 160, 80
BATCHES = (1, 100, 208)
FILL = 1024                          # csrc/sr_launch.cpp kMfccFill
QUIET_MAX, CHEAP_MAX = 26843, 70171  # csrc/sr_tables.h kMagSmallMax, kMagCheapMax on gfx950
KINDS = (FEAT_FFT, FEAT_MAG, FEAT_MEL)
CASES = ("impulse", "full_scale", "quiet")


# ---- CPU: the layout header ----------------------------------------------------------------------------------------------
def test_layout_check_runs_clean_under_the_sanitizers(tmp_path):
    """both images simulated word by word and the bank model restated lane by lane (tests/fft_layout/layout_check.cpp), from the
    header the kernel takes its addresses from: a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "layout_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "fft_layout", "layout_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "layout_check ok" in run.stdout, (run.stdout, run.stderr)


def test_batch_sizes_select_the_three_forms():
    """CPU: the arithmetic of tests/test_mfcc_lds_traffic.py's docstring"""
    t64, t16 = -(-MAX_FRAMES // 64), -(-MAX_FRAMES // 16)
    assert BATCHES[0] * t16 < FILL and BATCHES[1] * t16 >= FILL > BATCHES[1] * t64 and BATCHES[2] * t64 >= FILL


# ---- the cases and what the oracle says about them (computed once; nobody writes to what these return) ----------------------
def _impulse():
    n, S = FRAME, 256
    pcm = np.full((n, S), 2048, np.uint16)
    pcm[np.arange(n), 1 + np.arange(n)] = 2048 + 20000
    return pcm, np.ones(n, np.int32), np.ones(n, np.int32), np.full(n, 2048, np.uint32)


def _full_scale():
    counts = np.array([1, 2, 17, 64] * 2, np.int32)
    S = 1 + FRAME + HOP * 63 + 7
    t = np.arange(S)
    rows = [np.where(t % 2 == 0, 0, 65535), np.random.default_rng(12).integers(0, 65536, S)]
    pcm = np.stack([rows[0]] * 4 + [rows[1]] * 4).astype(np.uint16)
    return pcm, np.ones(len(counts), np.int32), counts, np.full(len(counts), 32768, np.uint32)


def _quiet():
    orc = ol.Oracle(max_frames=MAX_FRAMES)
    raw = synth.as_u16_numpy(synth.make_utterances(np.arange(4), [64] * 4, seed=321, bank=synth.word_bank(10), S=synth.buf_len_for(70), gain=1.0))
    pcm, st, _, mid = vad_segments(orc, raw)
    for b in range(len(pcm)):
        pk = orc.frame_peaks(pcm[b], int(st[b]), int(st[b]) + FRAME + HOP * 16, ol.Atap(int(mid[b]), 0, 0, 0))[:17]
        if (pk <= QUIET_MAX).all():
            return pcm[b:b + 1], st[b:b + 1], np.array([17], np.int32), mid[b:b + 1]
    raise AssertionError("no synthetic capture with 17 QUIET frames")


@functools.lru_cache(maxsize=None)
def reference(case):
    pcm, st, counts, mid = {"impulse": _impulse, "full_scale": _full_scale, "quiet": _quiet}[case]()
    orc = ol.Oracle(max_frames=MAX_FRAMES)
    en = (st + FRAME + HOP * (counts - 1)).astype(np.int32)
    assert st.min() >= 1 and en.max() <= pcm.shape[1]
    tab = orc.tables()
    frames = windows_of(orc, pcm, st, counts, mid)
    rows, mag, mel, peaks = [], [], [], []
    for b in range(len(pcm)):
        atap = ol.Atap(int(mid[b]), 0, 0, 0)
        n, m = orc.mfcc(pcm[b], int(st[b]), int(en[b]), atap)
        assert n == counts[b]
        rows.append(m)
        mag.append(np.stack([orc.fft_mag(f) for f in frames[b]]))
        mel.append(mel_from_mag(mag[b], tab)[0])
        peaks.append(orc.frame_peaks(pcm[b], int(st[b]), int(en[b]), atap)[:n])
    return dict(pcm=pcm, st=st, en=en, mid=mid, counts=counts, frames=frames, rows=rows, mag=mag, mel=mel, peaks=peaks)


def test_cases_are_what_they_claim():
    """CPU: one input position per impulse frame, LOUD full-scale frames, QUIET frames of the quiet segment"""
    r = reference("impulse")
    for i, fr in enumerate(r["frames"]):
        assert fr.shape == (1, FRAME) and fr[0, i] != 0 and set(np.flatnonzero(fr[0])) <= {i, i + 1}, i
    assert len({m.tobytes() for m in r["mag"]}) == FRAME  # 160 different spectra
    r = reference("full_scale")
    assert all((pk > CHEAP_MAX).all() for pk in r["peaks"]) and sorted(set(r["counts"])) == [1, 2, 17, 64]
    assert max(np.abs(fr.astype(np.int64)).max() for fr in r["frames"]) >= 30000
    r = reference("quiet")
    assert r["counts"].tolist() == [17] and (r["peaks"][0] <= QUIET_MAX).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    return Engine(max_frames=MAX_FRAMES, device=0)


_PRODUCT_FFT = {}


def product_fft(eng, case):
    """the packed words of every frame of a case through the product's full transform, once"""
    if case not in _PRODUCT_FFT:
        _PRODUCT_FFT[case] = [eng.fft_q15(fft_words(fr))[:, :512] for fr in reference(case)["frames"]]
    return _PRODUCT_FFT[case]


def launches(n, B):
    """index sets of the launches of one case: one launch per capture, or launches of B captures that cover all n, cycling"""
    if B == 1:
        return [np.array([b]) for b in range(n)]
    return [(np.arange(B) + s) % n for s in range(0, n, B)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES)
def test_words_magnitudes_filterbank_and_rows(eng, case, B):
    r = reference(case)
    counts, want_words = r["counts"], product_fft(eng, case)
    for idx in launches(len(counts), B):
        got = {k: features(eng, r["pcm"][idx], r["st"][idx], r["en"][idx], r["mid"][idx], k, want_mfcc=True) for k in KINDS}
        for k in KINDS:
            feat, n, status, mf = got[k]
            assert (status == 0).all() and np.array_equal(n, counts[idx].astype(np.uint32)), k
            assert mf.tobytes() == got[FEAT_MAG][3].tobytes(), k  # every launch's MFCC rows alike
        mf, words = got[FEAT_MAG][3], got[FEAT_FFT][0]
        for i, b in enumerate(idx):
            c = int(counts[b])
            assert mf[i, :c].tobytes() == r["rows"][b].tobytes() and not mf[i, c:].any(), (b, c)
            for k, w in ((FEAT_MAG, r["mag"][b]), (FEAT_MEL, r["mel"][b])):
                assert np.array_equal(got[k][0][i, :c], w) and not got[k][0][i, c:].any(), (k, b, c)
            assert np.array_equal(words[i, :c], want_words[b]) and not words[i, c:].any(), (b, c)
            assert np.array_equal(mag_from_words(words[i, :c]), r["mag"][b]), (b, c)
