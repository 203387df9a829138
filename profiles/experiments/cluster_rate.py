"""What clustering a corpus as ONE device operation saves: sr_cluster_models_dp_dev against the composition a caller had before.

    python profiles/experiments/cluster_rate.py [--words W] [--examples N] [--models C] [--iters I] [--launches L]
        W words x N examples x C models (default 100 x 64 x 4), examples of 80..120 frames: every word has C prototypes of
        different lengths, every example is a linear resampling of one of them plus noise, the models start from one example
        of each prototype.  Features resident in HBM.  In one process, three alternations of
          fused     sr_cluster_models_dp_dev, I iterations, one call;
          composed  per iteration: C sr_dtw_dp_align_dev calls without spans (every example against model c of its word), a
                    device argmin with the first-minimum key, the read-back of the assignment, the regrouping of the example
                    rows by model (host argsort, device gather) and a one-iteration sr_train_models_dp_dev.
        Each timed with device events around a synchronised window of L repetitions, after a warm-up.  The two must end in
        the same centroids.  One line of JSON; ratio = composed / fused.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/cluster_rate.py --trace
        The run to trace for the score pass's share (tracing only, the program after --): three fused calls.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LO, HI = 80, 120


def corpus(a):
    """-> mfcc int16 [E, HI, 12], frames uint32 [E], word_start, mdl_start, cen int16 [M, HI + 1, 12], cen_frames uint32 [M]"""
    rng = np.random.default_rng(5)
    W, N, Cn = a.words, a.examples, a.models
    E, M = W * N, W * Cn
    mfcc, frames = np.zeros((E, HI, 12), np.int16), np.zeros(E, np.uint32)
    cen, cen_frames = np.zeros((M, HI + 1, 12), np.int16), np.zeros(M, np.uint32)
    for w in range(W):
        lens = np.linspace(LO + 4, HI - 4, Cn).astype(int)
        protos = [rng.integers(-3000, 3001, (L, 12)) for L in lens]
        for i in range(N):
            c, e = i % Cn, w * N + i
            n = int(np.clip(lens[c] + rng.integers(-4, 5), LO, HI))
            src = np.minimum(np.arange(n) * lens[c] // n, lens[c] - 1)
            mfcc[e, :n] = np.clip(protos[c][src] + rng.integers(-300, 301, (n, 12)), -32768, 32767)
            frames[e] = n
            if i < Cn:  # the first take of each prototype seeds its model
                cen[w * Cn + c, :n], cen_frames[w * Cn + c] = mfcc[e, :n], n
    return mfcc, frames, np.arange(W + 1, dtype=np.uint32) * N, np.arange(W + 1, dtype=np.uint32) * Cn, cen, cen_frames


def setup(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine
    dev = torch.device("cuda", 0)
    mfcc, frames, ws, ms, cen, cf = corpus(a)
    E, M, Cn = len(frames), len(cf), a.models
    assert a.examples * HI <= 65535, "too many examples per word for exact sums: lower --examples"
    eng = Engine(max_frames=HI, device=0)
    d_im, d_fr = torch.from_numpy(mfcc).to(dev), torch.from_numpy(frames.view(np.int32)).to(dev)
    d_cen, d_cf = torch.from_numpy(cen).to(dev), torch.from_numpy(cf.view(np.int32)).to(dev)
    out_f, out_c = torch.empty_like(d_cen), torch.empty_like(d_cen)
    mdl0 = torch.from_numpy(np.repeat(ms[:-1], np.diff(ws)).astype(np.int32)).to(dev)  # first model of each example's word
    rec = torch.empty(Cn, E, 4, dtype=torch.int32, device=dev)
    col = torch.arange(Cn, device=dev, dtype=torch.int64)[:, None]

    def fused():
        eng.cluster_models_dev(d_im, d_fr, ws, ms, d_cen, d_cf, out_f, n_iter=a.iters)

    def composed():
        cur = d_cen
        for it in range(a.iters):
            for c in range(Cn):
                eng.align_dev(d_im, d_fr, cur, d_cf, rec[c], ref_of_row=mdl0 + c)
            key = ((rec[:, :, 0].to(torch.int64) & 0xFFFFFFFF) << 4) | col  # (dis, c): the first minimum in model order
            best = key.min(0).values
            assign = torch.where(best >> 4 == 0xFFFFFFFF, torch.full_like(best, -1), mdl0.to(torch.int64) + (best & 15))
            h = assign.cpu().numpy()                                         # the read-back
            keep = np.nonzero(h >= 0)[0]
            order = keep[np.argsort(h[keep], kind="stable")]                 # the regrouping
            ex_start = np.concatenate(([0], np.cumsum(np.bincount(h[keep], minlength=M)))).astype(np.uint32)
            idx = torch.from_numpy(order).to(dev)
            nxt = out_c if it == a.iters - 1 else torch.empty_like(d_cen)
            eng.train_models_dev(d_im[idx].contiguous(), d_fr[idx].contiguous(), ex_start, cur, d_cf, nxt, 1)
            cur = nxt

    return torch, eng, dict(fused=fused, composed=composed), out_f, out_c, E, M


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
    torch, eng, fn, out_f, out_c, E, M = setup(a)
    res = dict(words=a.words, examples_per_word=a.examples, models_per_word=a.models, frames=[LO, HI], n_iter=a.iters, launches=a.launches,
               examples=E, models=M, pairs_per_iteration=E * a.models)
    res.update({f"{k}_ms": [] for k in fn})
    for _ in range(3):
        for k in fn:
            res[f"{k}_ms"].append(round(event_ms(torch, fn[k], a.launches), 3))
    med = {k: float(np.median(res[f"{k}_ms"])) for k in fn}
    res["fused_ms_median"], res["composed_ms_median"] = med["fused"], med["composed"]
    res["ratio"] = round(med["composed"] / med["fused"], 3)
    res["same_centroids"] = bool(torch.equal(out_f, out_c))
    print(json.dumps(res), flush=True)
    eng.close()


def run_trace(a):
    torch, eng, fn, *_ = setup(a)
    for _ in range(3):
        fn["fused"]()
    torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=100)
    ap.add_argument("--examples", type=int, default=64)
    ap.add_argument("--models", type=int, default=4)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
