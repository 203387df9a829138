"""Connected-word decoding (sr_decode_words_dp_dev), with the word spotter as the yardstick of the same run.

    python profiles/experiments/chain_rate.py [--rows R] [--frames N] [--words W] [--launches L]
        R feature rows x N frames against 100 templates of 24..64 frames (random s16 features resident in HBM: the sweeps' work
        does not depend on the values), max_words W, skipping on.  One level of the decoder is one spotter-shaped pass, so the
        yardstick is W calls of the existing sr_spot_dp_batch_dev on the same rows with the same engine: what the levels should
        cost.  Each timed with device events over L launches, three alternations.  The share of k_chain_close + k_chain_trace
        (+ the init kernel) is taken by difference: the same call with a store of ONE one-frame template, whose sweeps are next
        to nothing, against the full call.  One row of the decoder's output is compared with the numpy definition
        (tests/chain_ref.py) at a reduced word count.  One line of JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/chain_rate.py --trace
        The run to trace for the per-kernel breakdown (tracing only, the program after --): one warm-up and three launches of each.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP = 6000


def setup(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine
    dev = torch.device("cuda", 0)
    K, N, W = 100, a.frames, a.words
    rng = np.random.default_rng(2027)
    tf = rng.integers(24, 65, K).astype(np.uint32)
    tm = np.zeros((K, 65, 12), np.int16)
    tm[:, :64] = rng.integers(-3000, 3001, (K, 64, 12))
    eng = Engine(max_frames=N, device=0)
    eng.set_templates_dense(tm, tf)
    tiny = Engine(max_frames=N, device=0)  # the same call with next to no sweep work: init + close + trace remain
    tiny.set_templates_dense(tm[:1, :2], np.array([1], np.uint32))
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (a.rows, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((a.rows,), N, dtype=torch.int32, device=dev)
    out = (torch.empty(a.rows, 4, dtype=torch.int32, device=dev), torch.empty(a.rows, W, 8, dtype=torch.int32, device=dev),
           torch.empty(a.rows, W, dtype=torch.int32, device=dev))
    hits = torch.empty(a.rows, 1, K, 4, dtype=torch.int32, device=dev)

    def fn_chain():
        eng.decode_words_dev(rows, frames, *out, W, 0, SKIP, 0)

    def fn_tiny():
        tiny.decode_words_dev(rows, frames, *out, W, 0, SKIP, 0)

    def fn_spot():
        for _ in range(W):
            eng.spot_dev(rows, frames, hits)

    return torch, eng, tiny, tm, tf, rows, out, fn_chain, fn_tiny, fn_spot


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
    torch, eng, tiny, tm, tf, rows, out, fn_chain, fn_tiny, fn_spot = setup(a)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import chain_ref
    from stm32_speech_recognition_amd.engine import decode_geometry
    N, W = a.frames, a.words
    cells = a.rows * N * int(tf.sum()) * W
    res = {"rows": a.rows, "frames": N, "K": len(tf), "max_words": W, "launches": a.launches, "cells": cells,
           "geometry": decode_geometry(int(tf.max()), N, W), "chain_ms": [], "spot_x_words_ms": [], "close_trace_ms": []}
    for _ in range(3):
        res["spot_x_words_ms"].append(round(event_ms(torch, fn_spot, a.launches), 3))
        res["chain_ms"].append(round(event_ms(torch, fn_chain, a.launches), 3))
        res["close_trace_ms"].append(round(event_ms(torch, fn_tiny, a.launches), 3))
    chain, spot, rest = (float(np.median(res[k])) for k in ("chain_ms", "spot_x_words_ms", "close_trace_ms"))
    res["chain_cells_per_s"] = round(cells / (chain * 1e-3), 0)
    res["ratio_to_spot_x_words"] = round(chain / spot, 4)
    res["close_trace_share"] = round(rest / chain, 4)
    # one short row against the definition, two levels
    n_chk = min(N, 300)
    fn_chain()
    torch.cuda.synchronize()
    rec = torch.empty(1, 4, dtype=torch.int32, device=rows.device)
    words = torch.empty(1, 2, 8, dtype=torch.int32, device=rows.device)
    lc = torch.empty(1, 2, dtype=torch.int32, device=rows.device)
    eng.decode_words_dev(rows[:1], torch.tensor([n_chk], dtype=torch.int32, device=rows.device), rec, words, lc, 2, 0, SKIP, 0)
    torch.cuda.synchronize()
    want = chain_ref.decode(rows[:1].cpu().numpy(), [n_chk], tm, tf, None, N, 2, 0, SKIP, 0)
    res["sample_equals_definition"] = bool(rec.cpu().numpy().tobytes() == want[0].tobytes() and words.cpu().numpy().tobytes() == want[1].tobytes()
                                           and lc.cpu().numpy().tobytes() == want[2].tobytes())
    print(json.dumps(res), flush=True)
    eng.close()
    tiny.close()


def run_trace(a):
    torch, eng, tiny, tm, tf, rows, out, fn_chain, fn_tiny, fn_spot = setup(a)
    for fn in (fn_spot, fn_chain):
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    eng.close()
    tiny.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
