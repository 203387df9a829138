"""rocprofv3 --hip-trace --stats -- python profiles/experiments/host_call_trace.py: a fixed, deterministic series of calls of
every host-buffer entry point, so that two builds of the library (SR_ENGINE_LIB, profiles/experiments/ab_build.sh) can be
compared by their per-API CALL COUNTS: a build whose copies, memsets, launches, synchronisations, events or stream waits
differ in number from its parent's has changed a transport or a launch sequence (hipGetLastError / hipGetDevice /
hipSetDevice may differ).  No test can see that: both transports give the same bytes.

The six entry points with a pinned and a blocking transport (sr_host_call.h) run in small-launch mode 0 and 1 and on
either side of the staging area's capacity:
  captures  16 and 17 rows of 9 680 samples (19 360 bytes; the upload part holds 327 680): sr_vad_batch, sr_mfcc_batch_status,
            sr_recognize_batch (with every and with no optional output), and 257 rows (above the 256-capture cap)
  records   283 and 284 records of 48 x 12 coefficients (1 156 bytes with the frame count): sr_dtw_batch
  VAD() / noise_atap()  through the drop-in symbols; their u16 buf_len never exceeds the area, so the mode alone selects
plus spch_recg / get_mfcc / dtw and the other scalar symbols through `compat`, and one call or two of every blocking-only
entry point, among them sr_recognize_batch's chunked upload (B = 2 048) and the packed form.  N = 3 repeats of the lot.
Prints the number of calls made; the figures of interest are rocprofv3's."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from stm32_speech_recognition_amd import Engine, compat, synth  # noqa: E402
from stm32_speech_recognition_amd.engine import FEAT_LOGMEL, FEAT_MAG, load_library, pack12  # noqa: E402

R, K, NW, N = 48, 9, 5, 3
calls = 0


def did(*_):
    global calls
    calls += 1


def main():
    rng = np.random.default_rng(2027)
    bank = synth.word_bank(NW)
    S = synth.buf_len_for(60)
    assert S == 9680
    eng = Engine(max_frames=R, device=0)
    tf = np.array([24, 30, 36, 44, 17, 48, 20, 1, 2], np.uint32)
    tm = rng.integers(-900, 900, (K, R + 1, 12)).astype(np.int16)
    eng.set_templates_dense(tm, tf)
    eng.set_word_map(slots_per_word=2)
    pcm = synth.as_u16_numpy(synth.make_utterances(rng.integers(0, NW, 2048), rng.integers(20, 44, 2048), seed=5, bank=bank, S=S))
    long_pcm = np.ascontiguousarray(pcm[:12].reshape(3, 4 * S))  # three recordings of four words each
    start, end = np.full(2048, 2401, np.int32), np.full(2048, 2401 + 160 + 80 * 29, np.int32)
    mid = np.full(2048, 2048, np.uint32)
    frames = rng.integers(1, R + 1, 284).astype(np.uint32)
    recs = rng.integers(-900, 900, (284, R, 12)).astype(np.int16)
    scores = rng.integers(0, 5000, (300, K)).astype(np.uint32)
    words = rng.integers(0, 1 << 26, (4, 1024)).astype(np.uint32)
    # the drop-in symbols' implicit engine: the firmware's shapes
    L = load_library()
    L.sr_compat_engine.restype = C.c_void_p
    fw = synth.as_u16_numpy(synth.make_utterances(np.arange(8) % NW, [100] * 8, seed=9, bank=bank, S=16000))
    store, st = Engine(max_frames=119, device=0).train_store(fw, np.arange(8), n_slots=8)
    assert (st == 0).all()
    compat.set_templates(store)
    ce = C.c_void_p(L.sr_compat_engine())
    slots = [compat.v_ftr_tag.from_buffer_copy(bytes(store[k * 4096:k * 4096 + 2860])) for k in range(8)]
    for _ in range(N):
        for mode in (0, 1):
            eng.set_small_launch(mode)
            assert L.sr_set_small_launch(ce, C.c_int(mode)) == 0
            for B in (1, 16, 17, 257):
                did(eng.vad(pcm[:B]))
                did(eng.mfcc_status(pcm[:B], start[:B], end[:B], mid[:B]))
                did(eng.recognize(pcm[:B]))
                did(eng.recognize(pcm[:B], want_scores=False, want_mfcc=False, want_vad=False))
            for B in (1, 283, 284):
                did(eng.dtw(recs[:B], frames[:B]))
            at = compat.atap_tag()
            did(compat.noise_atap(fw[0], compat.ATAP_LEN, at))
            segs = compat.VAD(fw[0], compat.VCBUF_LEN, at)
            did(segs)
            ftr = compat.get_mfcc(fw[0], segs[0][0], segs[0][1], at)
            did(ftr)
            for k in range(8):
                did(compat.dtw(ftr, slots[k]))
            did(compat.spch_recg(fw[1]))
            did(compat.get_dis(recs[0, 0], recs[1, 0]), compat.dtw_limit(3, 4))
            did(compat.fft(recs[0, :13].reshape(-1).copy()), compat.cr4_fft_1024_stm32(words[0]))
            did(compat.get_mdl(ftr, slots[0]))
        eng.set_small_launch(0)
        L.sr_set_small_launch(ce, C.c_int(0))
        # blocking-only entry points
        did(eng.recognize(pcm))                                   # 2 048 captures: the chunked upload
        did(eng.recognize_packed12(pack12(pcm[:64]), S))
        did(eng.recognize_nbest(pcm[:16], 3), eng.recognize_nbest(pcm[:17], 3))
        did(eng.recognize_segments(pcm[:16]))
        did(eng.frame_features(pcm[:16], start[:16], end[:16], mid[:16], FEAT_MAG))
        did(eng.frame_features(pcm[:16], start[:16], end[:16], mid[:16], FEAT_LOGMEL, want_mfcc=True))
        did(eng.train_store(pcm[:9], np.arange(9), n_slots=9))
        did(eng.dtw_dp(recs[:16], frames[:16]), eng.delta_mfcc(recs[:16], frames[:16]))
        did(eng.get_mdl(recs[:8, :40], np.minimum(frames[:8], 40), recs[8:16, :40], np.minimum(frames[8:16], 40), 40))
        did(eng.fft_q15(words), eng.nbest(scores, 4))
        did(eng.segment_stream(long_pcm), eng.recognize_stream(long_pcm), eng.recognize_stream(long_pcm, n_best=2))
    eng.close()
    print("host_call_trace: %d groups of calls, library %s" % (calls, os.environ.get("SR_ENGINE_LIB", "in-tree")))


if __name__ == "__main__":
    main()
