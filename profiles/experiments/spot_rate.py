"""Word spotting (sr_spot_dp_batch_dev) on long rows, with the full-DP scorer as the yardstick of the same run.

    python profiles/experiments/spot_rate.py [--rows R] [--launches N] [--batch B]
        64 feature rows x 16 383 frames against 100 templates of 192..320 frames (random s16 features resident in HBM: the
        kernel's work does not depend on the values), win_frames 0 and 100, each timed with device events over N launches,
        three alternations with the yardstick: sr_dtw_dp_batch_dev at 65 536 x 100 x 256 frames (engine of 320 frames).
        DP cells: the spotter's are the N x M rectangles (the lead-in columns a chunk recomputes are NOT counted: they are
        overhead), the yardstick's own are the cells of dtw_limit's band, counted on the host.  One (row, slot) of the
        spotter's output is compared with the numpy definition (tests/spot_ref.py).  One line of JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/spot_rate.py --trace
        The run to trace for the per-kernel breakdown (tracing only, the program after --): one warm-up and three launches
        of each.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINS = (0, 100)


def band_cells(in_n, mdl_n):
    """cells of dtw_limit's relaxed parallelogram (DTW.C:76-109, 133-142) for one pair; 0 when the length gate refuses it"""
    if in_n == 0 or mdl_n == 0 or in_n > 2 * mdl_n or 2 * in_n < mdl_n:
        return 0
    x1, x2 = int((2 * mdl_n - in_n) / 3) & 0xFFFF, int((4 * in_n - 2 * mdl_n) / 3) & 0xFFFF
    x = np.arange(1, in_n + 1)[:, None]
    y = np.arange(1, mdl_n + 1)[None, :]
    o1 = np.where(x < x1, y >= 2 * x + 2, 2 * y + in_n - 2 * mdl_n >= x + 4)
    o2 = np.where(x < x2, 2 * y + 2 <= x, y + 4 <= 2 * x + mdl_n - 2 * in_n)
    return int((~(o1 | o2)).sum())


def setup(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine
    dev = torch.device("cuda", 0)
    K, N, T = 100, 16383, 256
    rng = np.random.default_rng(2026)
    tf = rng.integers(192, 321, K).astype(np.uint32)
    tm = np.zeros((K, 321, 12), np.int16)
    tm[:, :320] = rng.integers(-3000, 3001, (K, 320, 12))
    g = torch.Generator(device=dev).manual_seed(7)
    spot = Engine(max_frames=N, device=0)
    spot.set_templates_dense(tm, tf)
    rows = torch.randint(-3000, 3001, (a.rows, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((a.rows,), N, dtype=torch.int32, device=dev)
    band = Engine(max_frames=320, device=0)
    band.set_templates_dense(tm, tf)
    utt = torch.randint(-3000, 3001, (a.batch, 320, 12), generator=g, device=dev, dtype=torch.int16)
    utt_frames = torch.full((a.batch,), T, dtype=torch.int32, device=dev)
    dense = torch.empty(a.batch, K, dtype=torch.int32, device=dev)
    hits = {w: torch.empty(a.rows, spot.spot_windows(w), K, 4, dtype=torch.int32, device=dev) for w in WINS}
    scores = {w: torch.empty(a.rows, spot.spot_windows(w), K, dtype=torch.int32, device=dev) for w in WINS}
    fn_spot = {w: (lambda w=w: spot.spot_dev(rows, frames, hits[w], scores[w], w)) for w in WINS}
    fn_band = lambda: band.dtw_dp_dev(utt, dense, in_frames=utt_frames)
    return torch, spot, band, tm, tf, rows, hits, fn_spot, fn_band


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
    torch, spot, band, tm, tf, rows, hits, fn_spot, fn_band = setup(a)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spot_ref
    from stm32_speech_recognition_amd.engine import spot_geometry
    N = rows.shape[1]
    spot_cells = a.rows * N * int(tf.sum())
    own_cells = a.batch * sum(band_cells(256, int(m)) for m in tf)
    res = {"rows": a.rows, "frames": N, "K": len(tf), "launches": a.launches, "batch": a.batch, "spot_cells": spot_cells,
           "band_cells": own_cells, "chunk_cols": spot_geometry(int(tf.max()), N)["chunk_cols"], "band_ms": []}
    res.update({f"spot_win{w}_ms": [] for w in WINS})
    for _ in range(3):
        res["band_ms"].append(round(event_ms(torch, fn_band, a.launches), 3))
        for w in WINS:
            res[f"spot_win{w}_ms"].append(round(event_ms(torch, fn_spot[w], a.launches), 3))
    res["band_cells_per_s"] = round(own_cells / (float(np.median(res["band_ms"])) * 1e-3), 0)
    for w in WINS:
        res[f"spot_win{w}_cells_per_s"] = round(spot_cells / (float(np.median(res[f"spot_win{w}_ms"])) * 1e-3), 0)
        res[f"spot_win{w}_ratio_to_band"] = round(res[f"spot_win{w}_cells_per_s"] / res["band_cells_per_s"], 4)
    # one (row, slot) against the definition
    r, k = a.rows - 1, 3
    want = spot_ref.spot_hits(rows[r:r + 1].cpu().numpy(), [N], tm[k:k + 1], tf[k:k + 1], None, N, 100)[0, :, 0]
    got = hits[100][r, :, k].cpu().numpy().view(spot_ref.SPOT_DTYPE).reshape(-1)
    res["sample_equals_definition"] = bool(got.tobytes() == want.tobytes())
    print(json.dumps(res), flush=True)
    spot.close()
    band.close()


def run_trace(a):
    torch, spot, band, tm, tf, rows, hits, fn_spot, fn_band = setup(a)
    for fn in (fn_band, fn_spot[0], fn_spot[100]):
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    spot.close()
    band.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
