"""The batch form of the reference front end's frame kernel keeps two frames in flight per wave (csrc/k_mfcc.hip): frame fi's
magnitudes -- for a QUIET frame the eight table gathers -- are carried into the next iteration and turned into energies,
filterbank outputs and the row of log inputs only after frame fi+1's FFT front.  What can go wrong is bookkeeping: a first or
last frame that takes the wrong side of the prologue / epilogue, a carried magnitude, tier flag or row index that belongs to
the neighbouring frame, words of the wave's LDS scratch that two stages now hold at the same time.  So: every frame count at
which a wave or a tile starts, ends or stays empty; captures whose tier changes from frame to frame, checked through every
intermediate value; and the batch form against the two forms that still take one frame at a time.  All against the CPU
oracle, byte for byte."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import Engine, FEAT_FFT, FEAT_LOGMEL, FEAT_MAG, FEAT_MEL
from test_frame_features import features, fft_words, log100, mag_from_words, mel_from_mag, vad_segments, windows_of

MAX_FRAMES = 72          # two tiles of the batch form (4 waves x 16 frames), the second one 8 rows deep
N_BATCH = 1024           # captures per batch: the frame kernel's fill threshold, so the batch form runs (test_mag_table.py)
N_TIER = 256             # distinct captures of the tier-change batch; repeated to N_BATCH for the launch
FRAME, HOP = 160, 80
QUIET_MAX, CHEAP_MAX = 26843, 70171  # csrc/sr_tables.h kMagSmallMax, kMagCheapMax on gfx950
# frames per capture: a wave of the workgroup sees 0, 1, 2, 15 or 16 frames; 65 and 66 open a second tile with 1 and 2
EDGE_COUNTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66)


def speech(n, seed, frames=MAX_FRAMES):
    bank = synth.word_bank(10)
    return synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 10, [frames] * n, seed=seed, bank=bank,
                                                    S=synth.buf_len_for(frames + 6)))


def explicit_segments(orc, pcm, counts):
    """segment start and mid value from the oracle's VAD, the end chosen so that MFCC.C:102 gives counts[b] frames"""
    p, st, _, mid = vad_segments(orc, pcm)
    assert len(p) == len(pcm)  # (every synthetic capture has a word)
    counts = np.asarray(counts, np.int32)
    en = (st + FRAME + HOP * (counts - 1)).astype(np.int32)
    assert st.min() >= 1 and en.max() <= pcm.shape[1]
    return p, st, en, mid


def oracle_rows(orc, pcm, st, en, mid):
    out = []
    for b in range(len(pcm)):
        n, m = orc.mfcc(pcm[b], int(st[b]), int(en[b]), ol.Atap(int(mid[b]), 0, 0, 0))
        out.append(m)
        assert n == len(m)
    return out


# ---- inputs and references, computed once ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_setup():
    orc = ol.Oracle(max_frames=MAX_FRAMES)
    # the counts interleaved over the batch: consecutive work items of a wave differ in theirs
    counts = np.array([EDGE_COUNTS[(5 * b + b // 16) % 16] for b in range(N_BATCH)], np.int32)
    assert all((counts == c).sum() == N_BATCH // 16 for c in EDGE_COUNTS) and (counts[1:] != counts[:-1]).all()
    pcm, st, en, mid = explicit_segments(orc, speech(N_BATCH, seed=81), counts)
    want = oracle_rows(orc, pcm, st, en, mid)
    assert [len(w) for w in want] == counts.tolist()
    eng = Engine(max_frames=MAX_FRAMES, device=0)
    n, mf, status = eng.mfcc_status(pcm, st, en, mid)
    return eng, pcm, st, en, mid, counts, want, (n, mf, status)


@functools.lru_cache(maxsize=None)
def tier_batch(seed=83):
    """synthetic speech whose loudness changes hop by hop: every 80-sample block scaled about the capture's mid value by a
    gain drawn from {0.5, 2.4, 6}, clipped to the ADC range.  N_TIER distinct captures and the tier of each of their frames
    (nobody writes to what this returns)"""
    orc = ol.Oracle(max_frames=MAX_FRAMES)
    raw = speech(N_TIER, seed=seed)
    pcm, st, en, mid = explicit_segments(orc, raw, np.full(N_TIER, MAX_FRAMES, np.int32))
    rng = np.random.default_rng(seed)
    nblk = pcm.shape[1] // HOP
    g = rng.choice(np.array([0.5, 2.4, 6.0]), size=(len(pcm), nblk))
    # runs of two or three hops with one gain as well, so that whole frames sit in one loudness
    hold = rng.integers(1, 4, size=(len(pcm), nblk))
    for k in range(1, nblk):
        keep = (k % hold[:, k]) != 0
        g[keep, k] = g[keep, k - 1]
    body = pcm[:, :nblk * HOP].astype(np.float64).reshape(len(pcm), nblk, HOP) - mid[:, None, None].astype(np.float64)
    out = pcm.copy()
    out[:, :nblk * HOP] = np.clip(np.rint(body * g[:, :, None]) + mid[:, None, None], 0, 4095).reshape(len(pcm), -1).astype(np.uint16)
    return orc, out, st, en, mid, frame_tiers_of(orc, out, st, en, mid)


def frame_tiers_of(orc, pcm, st, en, mid):
    """tier of every frame from the oracle's own spectrum: 0 QUIET, 1 MID, 2 LOUD  [B, MAX_FRAMES]"""
    t = np.zeros((len(pcm), MAX_FRAMES), np.int8)
    for b in range(len(pcm)):
        pk = orc.frame_peaks(pcm[b], int(st[b]), int(en[b]), ol.Atap(int(mid[b]), 0, 0, 0))
        assert len(pk) == MAX_FRAMES
        t[b] = (pk > QUIET_MAX).astype(np.int8) + (pk > CHEAP_MAX)
    return t


def pair_counts(t):
    """occurrences of every ordered (previous tier, next tier) pair: over all consecutive frames, with the second frame first
    in a wave (frame 16 k), and with the second frame last in a tile (frame 63)"""
    def count(prev, nxt):
        return np.array([[int(((prev == i) & (nxt == j)).sum()) for j in range(3)] for i in range(3)])
    every = count(t[:, :-1], t[:, 1:])
    wave = count(t[:, 15:MAX_FRAMES - 1:16], t[:, 16:MAX_FRAMES:16])
    last = count(t[:, 62], t[:, 63])
    return every, wave, last


def test_tier_batch_has_every_transition_where_it_matters():
    """CPU: the oracle alone says the tier inputs hold each of the nine ordered pairs >= 20 times, and each at least once
    across a wave boundary and at a tile's last frame"""
    orc, pcm, st, en, mid, tiers = tier_batch()
    every, wave, last = pair_counts(tiers)
    print("pairs", every.tolist(), "wave boundary", wave.tolist(), "tile end", last.tolist())
    assert every.min() >= 20 and wave.min() >= 1 and last.min() >= 1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frame_counts_at_every_pipeline_edge(edge_setup):
    eng, pcm, st, en, mid, counts, want, (n, mf, status) = edge_setup
    assert (status == 0).all() and np.array_equal(n, counts.astype(np.uint32))
    for b in range(len(pcm)):
        assert mf[b, :counts[b]].tobytes() == want[b].tobytes(), (b, int(counts[b]))
        assert not mf[b, counts[b]:].any(), (b, int(counts[b]))


@pytest.mark.gpu
def test_tier_changes_between_consecutive_frames():
    orc, pcm, st, en, mid, tiers = tier_batch()
    every, wave, last = pair_counts(tiers)
    assert every.min() >= 20 and wave.min() >= 1 and last.min() >= 1
    rep = N_BATCH // N_TIER  # the launch: every capture rep times, so that the batch form runs
    pcm, st, en, mid = np.tile(pcm, (rep, 1)), np.tile(st, rep), np.tile(en, rep), np.tile(mid, rep)
    kinds = (FEAT_FFT, FEAT_MAG, FEAT_MEL, FEAT_LOGMEL)
    eng = Engine(max_frames=MAX_FRAMES, device=0, testing=True)
    on = {k: features(eng, pcm, st, en, mid, k, want_mfcc=True) for k in kinds}
    engine.dev_hook("mag_table_off", 1)
    try:
        off = {k: features(eng, pcm, st, en, mid, k, want_mfcc=True) for k in kinds}
    finally:
        engine.dev_hook("mag_table_off", 0)
    n = on[FEAT_MAG][1]
    assert (n == MAX_FRAMES).all() and (on[FEAT_MAG][2] == 0).all()
    for k in kinds:  # the table against the MID tier's arithmetic for the QUIET frames, and every launch's MFCC rows alike
        for x, y in zip(on[k], off[k]):
            assert x.tobytes() == y.tobytes(), k
        assert on[k][3].tobytes() == on[FEAT_MAG][3].tobytes(), k
    # the oracle: rows, magnitudes, filterbank outputs, their logs; the FFT words through the product's full transform (an
    # independent kernel) and through the oracle's magnitudes
    for k in kinds:  # the repeats equal their originals
        for x in (on[k][0], on[k][3]):
            assert (x.reshape(rep, N_TIER, *x.shape[1:]) == x[:N_TIER]).all(), k
    tab = orc.tables()
    want_rows = oracle_rows(orc, pcm[:N_TIER], st, en, mid)
    frames = windows_of(orc, pcm[:N_TIER], st, n[:N_TIER], mid)
    for b in range(N_TIER):
        assert on[FEAT_MAG][3][b].tobytes() == want_rows[b].tobytes(), b
        mag = np.stack([orc.fft_mag(f) for f in frames[b]])
        assert np.array_equal(on[FEAT_MAG][0][b], mag), b
        assert np.array_equal(mag_from_words(on[FEAT_FFT][0][b]), mag), b
        mel = mel_from_mag(mag, tab)[0]
        assert np.array_equal(on[FEAT_MEL][0][b], mel), b
        assert np.array_equal(on[FEAT_LOGMEL][0][b].reshape(-1), log100(orc, mel)), b
    some = np.arange(0, N_TIER, 8)
    words = fft_words(np.concatenate([frames[b] for b in some]))
    assert np.array_equal(np.concatenate([on[FEAT_FFT][0][b] for b in some]), eng.fft_q15(words)[:, :512])


@pytest.mark.gpu
def test_batch_form_equals_the_small_forms(edge_setup):
    """the forms for underfilled launches take one frame at a time.  Which one runs follows from the work-item count
    (csrc/sr_launch.cpp, kMfccFill = 1 024): at this frame cap a capture is 2 work items of 64 frames or 5 of 16, so one capture
    and 64 captures run the one-frame-per-wave form and 256 captures (1 280 >= 1 024 > 512) the four-frame form"""
    eng, pcm, st, en, mid, counts, want, (n, mf, status) = edge_setup
    seen = set()
    for b in range(64, 64 + 16):
        n1, m1, s1 = eng.mfcc_status(pcm[b:b + 1], st[b:b + 1], en[b:b + 1], mid[b:b + 1])
        assert s1[0] == 0 and n1[0] == n[b] and m1[0].tobytes() == mf[b].tobytes(), (b, int(counts[b]))
        seen.add(int(counts[b]))
    assert seen == set(EDGE_COUNTS)
    for nb in (64, 256):
        assert set(counts[:nb].tolist()) == set(EDGE_COUNTS)
        nn, mm, ss = eng.mfcc_status(pcm[:nb], st[:nb], en[:nb], mid[:nb])
        assert np.array_equal(nn, n[:nb]) and np.array_equal(ss, status[:nb]) and mm.tobytes() == mf[:nb].tobytes(), nb
