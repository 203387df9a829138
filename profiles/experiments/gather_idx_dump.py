"""Indices for profiles/experiments/gather_rate.hip: re^2 + im^2 of every bin of a few thousand frames of the headline
workload (bench.py's captures: 25 synthetic words, 256 frames, gain 1.0 unless --gain says otherwise), taken from the frame
kernel's own SR_FEAT_FFT output and laid out in k_mfcc's lane order.

    python profiles/experiments/gather_idx_dump.py OUT.bin [--captures 32] [--gain 1.0]

OUT.bin: u32 n_frames, then n_frames x 64 lanes x 4 dwords; dword e3 of lane l = n(bin l + 64 e3) | n(bin l + 64 e3 + 256) << 16,
each n clamped to 65 535 (past the 26 844-entry table either way, like a bin of a frame that is not QUIET)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from stm32_speech_recognition_amd import Engine, synth  # noqa: E402
from stm32_speech_recognition_amd.engine import FEAT_FFT, vad_from_torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--captures", type=int, default=32)
ap.add_argument("--gain", type=float, default=1.0)
a = ap.parse_args()
T, NW, B = 256, 25, a.captures
eng = Engine(max_frames=320, device=0)
rng = np.random.default_rng(2026)
pcm = synth.make_utterances(rng.integers(0, NW, B), [T] * B, seed=1000, bank=synth.word_bank(NW), S=synth.buf_len_for(T),
                            device="cuda:0", gain=a.gain)
vad, _ = eng.features_dev(pcm)
w = eng.frame_features_dev(pcm, vad, FEAT_FFT).cpu().numpy().view(np.uint32)  # [B][max_frames][512] packed re | im << 16
torch.cuda.synchronize()
nf = vad_from_torch(vad)["frm_num"]
w = np.concatenate([w[b, :nf[b]] for b in range(B)])
re = (w & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)
im = (w >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
n = re * re + im * im
quiet = n.max(axis=1) <= 26843
print("%d frames, %.1f %% QUIET, median n %d, 99th percentile %d" % (len(n), 100 * quiet.mean(), np.median(n), np.percentile(n, 99)))
c = np.minimum(n, 65535).astype(np.uint32)
lane, e3 = np.arange(64)[:, None], np.arange(4)[None, :]
lo, hi = c[:, lane + 64 * e3], c[:, lane + 64 * e3 + 256]  # [frames][64][4]
with open(a.out, "wb") as f:
    np.array([len(n)], np.uint32).tofile(f)
    (lo | hi << 16).astype(np.uint32).tofile(f)
