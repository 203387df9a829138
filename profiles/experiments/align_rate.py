"""What recording the predecessor marks and tracing the path back costs: sr_dtw_dp_align_dev against sr_dtw_dp_batch_dev.

    python profiles/experiments/align_rate.py [--pairs P] [--launches N]
        For T = 64, 128 and 256 frames: P pairs (row r against reference r, both T frames, random s16 features resident in
        HBM: the kernels' work does not depend on the values), in one process, three alternations of
          score   sr_dtw_dp_batch_dev under sr_set_dp_lanes(1) -- k_dtw_dp_wave64, the kernel the aligner's sweep is taken
                  from -- on the same P pairs: P / 64 rows against a store of 64 templates;
          align   sr_dtw_dp_align_dev with d_span, on an engine whose frame cap is T (so that the marks' place -- LDS or
                  global scratch -- is the one a caller with such words gets);
          train   one iteration of sr_train_models_dp_dev: the same rows as the examples of 64 models.
        Each timed with device events over N launches.  One pair of the aligner's output is compared with the numpy
        definition (tests/align_ref.py).  One line of JSON per T; ratio_per_pair = align / score.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/align_rate.py --trace
        The run to trace for the per-kernel breakdown (tracing only, the program after --): one warm-up and three launches
        of each at T = 128.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FRAMES = (64, 128, 256)
K = 64  # templates of the yardstick's store = models of the training run


def setup(a, T):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine
    dev = torch.device("cuda", 0)
    P = a.pairs // K * K
    g = torch.Generator(device=dev).manual_seed(7 + T)
    eng = Engine(max_frames=T, device=0)
    rows = torch.randint(-3000, 3001, (P, T, 12), generator=g, device=dev, dtype=torch.int16)
    refs = torch.randint(-3000, 3001, (P, T, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((P,), T, dtype=torch.int32, device=dev)
    rec = torch.empty(P, 4, dtype=torch.int32, device=dev)
    span = torch.empty(P, T, dtype=torch.int32, device=dev)
    tm = np.zeros((K, T + 1, 12), np.int16)
    tm[:, :T] = refs[:K].cpu().numpy()
    eng.set_templates_dense(tm, np.full(K, T, np.uint32))
    eng.set_dp_lanes(1)
    scores = torch.empty(P // K, K, dtype=torch.int32, device=dev)
    cen_in, cen_out = refs[:K].contiguous(), torch.empty(K, T, 12, dtype=torch.int16, device=dev)
    cen_frames = torch.full((K,), T, dtype=torch.int32, device=dev)
    ex_start = np.arange(K + 1, dtype=np.uint32) * (P // K)
    assert (P // K) * T <= 65535, "too many examples per model for this frame count: lower --pairs"
    fn = dict(score=lambda: eng.dtw_dp_dev(rows[:P // K], scores, in_frames=frames),
              align=lambda: eng.align_dev(rows, frames, refs, frames, rec, span),
              train=lambda: eng.train_models_dev(rows, frames, ex_start, cen_in, cen_frames, cen_out, 1))
    return torch, eng, fn, rows, refs, rec, span, P


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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import align_ref
    from stm32_speech_recognition_amd.engine import align_geometry
    for T in FRAMES:
        torch, eng, fn, rows, refs, rec, span, P = setup(a, T)
        res = {"frames": T, "pairs": P, "launches": a.launches, "marks_scratch_bytes_per_pair": align_geometry(T, T)["scratch_bytes"]}
        res.update({f"{k}_ms": [] for k in fn})
        for _ in range(3):
            for k in fn:
                res[f"{k}_ms"].append(round(event_ms(torch, fn[k], a.launches), 3))
        med = {k: float(np.median(res[f"{k}_ms"])) for k in fn}
        res["score_us_per_pair"] = round(med["score"] * 1e3 / P, 4)
        res["align_us_per_pair"] = round(med["align"] * 1e3 / P, 4)
        res["train_iteration_us_per_example"] = round(med["train"] * 1e3 / P, 4)
        res["ratio_per_pair"] = round(med["align"] / med["score"], 3)
        r = P - 1  # one pair against the definition
        (want, path) = align_ref.align_pair(rows[r].cpu().numpy(), refs[r].cpu().numpy())
        got = rec[r].cpu().numpy().view(np.uint32)
        res["sample_equals_definition"] = bool(tuple(int(v) for v in got) == want and
                                               np.array_equal(span[r].cpu().numpy().view(np.uint32), align_ref.spans(path, T)))
        print(json.dumps(res), flush=True)
        eng.close()


def run_trace(a):
    torch, eng, fn, *_ = setup(a, 128)
    for k in fn:
        for _ in range(4):
            fn[k]()
        torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16320)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
