"""The frame kernel of the reference front end (csrc/k_mfcc.hip) passes every frame through the wave's LDS area four times:
window -> pass-1 gather, the exchange between passes 3 and 4, energies -> filterbank, prefixes + lane sums -> look-up.  Which
instruction stores a word, and where the word lies, is free as long as the reader finds it -- and a wrong base, offset or
EXEC mask of a lane-contiguous store, a stale multiplier register or an image that two stages hold at once shows up only
where a wave has one frame, a first and a last one, a full or an empty tile.  So: MFCC rows, VAD records and the FFT / MAG /
MEL / LOGMEL outputs against the CPU oracle, byte for byte, on captures of 1, 2, 3, 16, 17, 63, 64, 65 and max_frames frames,
at three loudnesses (every magnitude tier) and at three batch sizes that select the three forms of the kernel.

Which form runs follows from the work-item count (csrc/sr_launch.cpp, kMfccFill = 1 024): at max_frames = 320 a capture is 5
work items of 64 frames, 20 of 16 or 80 of 4.  One capture (80 < 1 024) runs the one-frame-per-wave form, 100 captures
(2 000 >= 1 024 > 500) the four-frame form and 208 captures (1 040 >= 1 024) the batch form."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from stm32_speech_recognition_amd import synth
from stm32_speech_recognition_amd.engine import Engine, FEAT_FFT, FEAT_LOGMEL, FEAT_MAG, FEAT_MEL, VAD_DTYPE
from test_frame_features import features, fft_words, log100, mag_from_words, mel_from_mag, vad_segments, windows_of

MAX_FRAMES = 320
FRAME, HOP = 160, 80
COUNTS = (1, 2, 3, 16, 17, 63, 64, 65, MAX_FRAMES)
GAINS = (1.0, 2.4, 4.0)
BATCHES = (1, 100, 208)
FILL = 1024                          # csrc/sr_launch.cpp kMfccFill
QUIET_MAX, CHEAP_MAX = 26843, 70171  # csrc/sr_tables.h kMagSmallMax, kMagCheapMax on gfx950
KINDS = (FEAT_FFT, FEAT_MAG, FEAT_MEL, FEAT_LOGMEL)
N = len(COUNTS)


def test_batch_sizes_select_the_three_forms():
    """CPU: the arithmetic of the docstring"""
    t64, t16, t4 = -(-MAX_FRAMES // 64), -(-MAX_FRAMES // 16), -(-MAX_FRAMES // 4)
    assert BATCHES[0] * t16 < FILL                                  # the smallest form
    assert BATCHES[1] * t16 >= FILL > BATCHES[1] * t64              # the four-frame form
    assert BATCHES[2] * t64 >= FILL                                 # the batch form
    assert t4 == 80


@functools.lru_cache(maxsize=None)
def reference(gain):
    """nine captures at one loudness, their explicit segments of COUNTS frames, and everything the oracle says about them
    (computed once per gain; nobody writes to what this returns)"""
    orc = ol.Oracle(max_frames=MAX_FRAMES)
    bank = synth.word_bank(10)
    raw = synth.as_u16_numpy(synth.make_utterances(np.arange(N) % 10, [MAX_FRAMES] * N, seed=111, bank=bank,
                                                    S=synth.buf_len_for(MAX_FRAMES + 6), gain=gain))
    pcm, st, _, mid = vad_segments(orc, raw)
    assert len(pcm) == N  # (every synthetic capture has a word)
    counts = np.array(COUNTS, np.int32)
    en = (st + FRAME + HOP * (counts - 1)).astype(np.int32)
    assert st.min() >= 1 and en.max() <= pcm.shape[1]
    tab = orc.tables()
    frames = windows_of(orc, pcm, st, counts, mid)
    rows, mag, mel, logmel, peaks = [], [], [], [], []
    for b in range(N):
        atap = ol.Atap(int(mid[b]), 0, 0, 0)
        n, m = orc.mfcc(pcm[b], int(st[b]), int(en[b]), atap)
        assert n == counts[b]
        rows.append(m)
        mag.append(np.stack([orc.fft_mag(f) for f in frames[b]]))
        mel.append(mel_from_mag(mag[b], tab)[0])
        logmel.append(log100(orc, mel[b]).reshape(mel[b].shape))
        peaks.append(orc.frame_peaks(pcm[b], int(st[b]), int(en[b]), atap)[:n])
    # the captures as the VAD itself cuts them: record and rows
    recs = []
    for b in range(N):
        rc, a = orc.noise_atap(raw[b])
        seg = orc.vad(raw[b], a)
        assert rc == 0 and seg[0] >= 1
        n, m = orc.mfcc(raw[b], int(seg[0]), int(seg[1]), a)
        recs.append((a.astuple(), seg, n, m))
    pk = np.concatenate(peaks)
    tiers = (int((pk <= QUIET_MAX).sum()), int(((pk > QUIET_MAX) & (pk <= CHEAP_MAX)).sum()), int((pk > CHEAP_MAX).sum()))
    return dict(orc=orc, raw=raw, pcm=pcm, st=st, en=en, mid=mid, counts=counts, frames=frames, rows=rows, mag=mag, mel=mel,
                logmel=logmel, recs=recs, tiers=tiers)


def test_gains_reach_every_tier():
    """CPU: the oracle's own spectrum puts frames of the quietest batch in the QUIET tier, of the middle one in the MID tier
    and of the loudest in the LOUD tier"""
    t = [reference(g)["tiers"] for g in GAINS]
    print("frames per tier (QUIET, MID, LOUD) at gains", GAINS, ":", t)
    assert t[0][0] > 0 and t[1][1] > 0 and t[2][2] > 0


@pytest.fixture(scope="module")
def eng():
    return Engine(max_frames=MAX_FRAMES, device=0)


def launches(B):
    """index sets of the launches of one case: nine launches of one capture, or one launch of B with the nine cycling"""
    return [np.array([b]) for b in range(N)] if B == 1 else [np.arange(B) % N]


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("gain", GAINS)
def test_rows_and_features_at_every_frame_count(eng, gain, B):
    r = reference(gain)
    orc, counts = r["orc"], r["counts"]
    for idx in launches(B):
        got = {k: features(eng, r["pcm"][idx], r["st"][idx], r["en"][idx], r["mid"][idx], k, want_mfcc=True) for k in KINDS}
        for k in KINDS:
            feat, n, status, mf = got[k]
            assert (status == 0).all() and np.array_equal(n, counts[idx].astype(np.uint32)), k
            assert mf.tobytes() == got[FEAT_MAG][3].tobytes(), k  # every launch's MFCC rows alike
            first = {}
            for i, b in enumerate(idx):  # repeats of a capture equal its first occurrence
                if b in first:
                    assert feat[i].tobytes() == feat[first[b]].tobytes() and mf[i].tobytes() == mf[first[b]].tobytes(), (k, i)
                else:
                    first[b] = i
        for b, i in first.items():
            c = int(counts[b])
            mf = got[FEAT_MAG][3][i]
            assert mf[:c].tobytes() == r["rows"][b].tobytes() and not mf[c:].any(), (b, c)
            want = {FEAT_MAG: r["mag"][b], FEAT_MEL: r["mel"][b], FEAT_LOGMEL: r["logmel"][b]}
            for k, w in want.items():
                assert np.array_equal(got[k][0][i][:c], w) and not got[k][0][i][c:].any(), (k, b, c)
            words = got[FEAT_FFT][0][i]
            assert np.array_equal(mag_from_words(words[:c]), r["mag"][b]) and not words[c:].any(), (b, c)
            if c <= 65:  # the packed words themselves, through the product's full transform (an independent kernel)
                assert np.array_equal(words[:c], eng.fft_q15(fft_words(r["frames"][b]))[:, :512]), (b, c)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("gain", GAINS)
def test_vad_records_and_rows_of_the_vads_own_segments(eng, gain, B):
    import torch
    r = reference(gain)
    for idx in launches(B):
        pcm = torch.from_numpy(r["raw"][idx].view(np.int16)).to("cuda:0")
        vad, mf = eng.features_dev(pcm)
        torch.cuda.synchronize()
        vd = np.frombuffer(vad.cpu().numpy().tobytes(), VAD_DTYPE)
        mf = mf.cpu().numpy()
        for i, b in enumerate(idx):
            atap, seg, n, rows = r["recs"][b]
            assert (vd["mid_val"][i], vd["n_thl"][i], vd["z_thl"][i], vd["s_thl"][i]) == atap, (i, b)
            assert np.array_equal(vd["seg"][i], seg) and vd["frm_num"][i] == n and vd["status"][i] == 0, (i, b)
            assert mf[i, :n].tobytes() == rows.tobytes() and not mf[i, n:].any(), (i, b)
