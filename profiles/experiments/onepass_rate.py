"""One-pass connected-word decoding (sr_decode_onepass_dp_dev) against level building (sr_decode_words_dp_dev) in the same run.

    python profiles/experiments/onepass_rate.py [--rows R] [--frames N] [--launches L]
        R feature rows x N frames against 100 templates of 80..120 frames (random s16 features resident in HBM: the sweeps' work
        does not depend on the values), skipping on.  The one-pass call and the level decoder at max_words 8 and 16 alternate
        on the same engine, each timed with device events over L launches, three alternations.  The cell counts say 2 / 8 and
        2 / 16; what they do not say is what about a hundred dependent launches of short kernels cost.  One short row of the
        one-pass output is compared with the definition (tests/onepass_ref.py).  One line of JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/onepass_rate.py --trace
        The run to trace for the per-kernel breakdown (tracing only, the program after --): one warm-up and three launches of each.
        The time per block is k_onepass_words' and k_onepass_close's average; the launch share of the call is what is left of
        the event time after the kernels' own time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP = 6000
WORDS_CAP = 64


def setup(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine
    dev = torch.device("cuda", 0)
    K, N = 100, a.frames
    rng = np.random.default_rng(2028)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tm = np.zeros((K, 121, 12), np.int16)
    tm[:, :120] = rng.integers(-3000, 3001, (K, 120, 12))
    eng = Engine(max_frames=N, device=0)
    eng.set_templates_dense(tm, tf)
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (a.rows, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((a.rows,), N, dtype=torch.int32, device=dev)
    one = (torch.empty(a.rows, 4, dtype=torch.int32, device=dev), torch.empty(a.rows, WORDS_CAP, 8, dtype=torch.int32, device=dev))
    lev = {W: (torch.empty(a.rows, 4, dtype=torch.int32, device=dev), torch.empty(a.rows, W, 8, dtype=torch.int32, device=dev),
               torch.empty(a.rows, W, dtype=torch.int32, device=dev)) for W in (8, 16)}

    def fn_onepass():
        eng.decode_onepass_dev(rows, frames, *one, WORDS_CAP, SKIP, 0)

    def fn_levels(W):
        return lambda: eng.decode_words_dev(rows, frames, *lev[W], W, 0, SKIP, 0)

    return torch, eng, tm, tf, rows, one, fn_onepass, fn_levels(8), fn_levels(16)


def event_ms(torch, fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run(a):
    torch, eng, tm, tf, rows, one, fn_onepass, fn_l8, fn_l16 = setup(a)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import onepass_ref
    from stm32_speech_recognition_amd.engine import decode_onepass_geometry
    N = a.frames
    geo = decode_onepass_geometry(int(tf.max()), len(tf), N, int(tf.min()))
    res = {"rows": a.rows, "frames": N, "K": len(tf), "tpl_frames": [int(tf.min()), int(tf.max())], "launches": a.launches,
           "cells_onepass": 2 * a.rows * N * int(tf.sum()), "geometry": geo, "onepass_ms": [], "levels8_ms": [], "levels16_ms": []}
    for _ in range(3):
        res["levels8_ms"].append(round(event_ms(torch, fn_l8, a.launches), 3))
        res["onepass_ms"].append(round(event_ms(torch, fn_onepass, a.launches), 3))
        res["levels16_ms"].append(round(event_ms(torch, fn_l16, a.launches), 3))
    op, l8, l16 = (float(np.median(res[k])) for k in ("onepass_ms", "levels8_ms", "levels16_ms"))
    res["onepass_cells_per_s"] = round(res["cells_onepass"] / (op * 1e-3), 0)
    res["ratio_to_levels8"] = round(op / l8, 4)
    res["ratio_to_levels16"] = round(op / l16, 4)
    res["ms_per_block"] = round(op / ((geo["launches"] - 2) / 2), 4)
    rec, words = one
    res["words_per_row"] = [int(rec[:, 1].min()), int(rec[:, 1].max())]
    # one short row against the definition
    n_chk = min(N, 100)
    r1 = torch.empty(1, 4, dtype=torch.int32, device=rows.device)
    w1 = torch.empty(1, WORDS_CAP, 8, dtype=torch.int32, device=rows.device)
    eng.decode_onepass_dev(rows[:1], torch.tensor([n_chk], dtype=torch.int32, device=rows.device), r1, w1, WORDS_CAP, SKIP, 0)
    torch.cuda.synchronize()
    want = onepass_ref.decode(rows[:1].cpu().numpy(), [n_chk], tm, tf, None, N, WORDS_CAP, SKIP, 0)
    res["sample_equals_definition"] = bool(r1.cpu().numpy().tobytes() == want[0].tobytes() and w1.cpu().numpy().tobytes() == want[1].tobytes())
    print(json.dumps(res), flush=True)
    eng.close()


def run_trace(a):
    torch, eng, tm, tf, rows, one, fn_onepass, fn_l8, fn_l16 = setup(a)
    for fn in (fn_l8, fn_onepass):
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
