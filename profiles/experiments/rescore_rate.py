"""Two-pass recognition (sr_rescore_nbest_dp_dev) at the benchmark's shape: the sparse second pass against the dense full-DP
matrix, which is the only way to those scores without it.

    python profiles/experiments/rescore_rate.py [--batch B] [--launches N] [--steps N]
        65 536 captures x 100 templates (192..320 frames, slot k = take k % 4 of word k // 4: the firmware's enrolment, map
        slots_per_word = 4) x 256 frames, features and first-pass lists resident in HBM (one sr_recognize_nbest_batch_dev per
        n_best).  In one process, three alternations of: the dense scorer (sr_dtw_dp_batch_dev, all B x K pairs) and the second
        pass for n_best = 1, 2, 4, 8, each timed with device events over N launches.  Per entry: milliseconds, the pairs
        actually scored (every slot of every candidate word, counted from the lists) and nanoseconds per pair.  Then the whole
        path, three alternations over `--steps` steps with a host clock around a device synchronise: recognize_dev + the dense
        matrix against recognize_nbest_dev(rescore=True) at n_best = 4.  The rescored lists of every n_best are compared with
        dense matrix -> mask -> k_nbest on the device ("identical").  The shader clock is sampled through the run.  One line
        of JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/rescore_rate.py --trace
        The run to trace for the per-kernel breakdown (tracing only, the program after --): one warm-up and five launches of
        the dense scorer, then of the second pass at n_best = 4.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

N_BEST = (1, 2, 4, 8)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(B):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine, synth
    T, K, NW = 256, 100, 25
    dev = torch.device("cuda", 0)
    eng = Engine(max_frames=320, device=0)
    bank = synth.word_bank(NW)
    rng = np.random.default_rng(2026)
    tfr = rng.integers(192, 321, K)
    tp = synth.make_utterances(np.arange(K) // 4, tfr, seed=77, bank=bank, S=synth.buf_len_for(320), device=dev)
    tvad, tmf = eng.features_dev(tp)
    torch.cuda.synchronize()
    tm = np.concatenate([tmf.cpu().numpy(), np.zeros((K, 1, 12), np.int16)], 1)
    eng.set_templates_dense(tm, tfr.astype(np.uint32))
    eng.set_word_map(None, 4)
    pcm = synth.make_utterances(rng.integers(0, NW, B), [T] * B, seed=1000, bank=bank, S=synth.buf_len_for(T), device=dev)
    out = eng.alloc_outputs(B, dev)
    lists = {}
    for n in N_BEST:  # the first pass, once per n_best
        out["nbest"], out["n_matched"] = None, torch.empty(B, dtype=torch.int32, device=dev)
        eng.recognize_nbest_dev(pcm, out, n)
        lists[n] = out["nbest"]
    torch.cuda.synchronize()
    dense = torch.empty(B, K, dtype=torch.int32, device=dev)
    return torch, eng, pcm, out, lists, dense, K


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


def host_ms(torch, fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def candidate_mask(torch, lst, K):
    """[B, K] bool: the slots of the candidate words of every row's list (map: word = slot // 4)"""
    B = lst.shape[0]
    word, slot = lst[:, :, 0], lst[:, :, 1].to(torch.int64) & 0xFFFFFFFF
    ok = (word != -1) & (slot < K)
    hit = torch.zeros(B, (K + 3) // 4 + 1, dtype=torch.bool, device=lst.device)
    hit.scatter_(1, torch.where(ok, slot // 4, torch.full_like(slot, (K + 3) // 4)), True)
    return hit[:, :(K + 3) // 4].repeat_interleave(4, 1)[:, :K]


def run(a):
    torch, eng, pcm, out, lists, dense, K = setup(a.batch)
    sys.path.insert(0, ROOT)
    try:
        from bench import ClockSampler
    except Exception:  # the numbers stand without it; the clock is then reported as null
        ClockSampler = None
    B = a.batch
    frames = out["vad"][:, 9]  # sr_vad_rec::frm_num, 12 words per record
    res = {"B": B, "K": K, "launches": a.launches, "steps": a.steps, "dense_ms": [], "dense_pairs": B * K}
    res.update({f"rescore_n{n}_ms": [] for n in N_BEST})
    fn_dense = lambda: eng.dtw_dp_dev(out["mfcc"], dense, vad=out["vad"])
    clk = ClockSampler(period=0.02) if ClockSampler else None
    if clk:
        clk.__enter__()
    for _ in range(3):
        res["dense_ms"].append(round(event_ms(torch, fn_dense, a.launches), 3))
        for n in N_BEST:
            res[f"rescore_n{n}_ms"].append(round(event_ms(torch, lambda: eng.rescore_nbest_dev(out["mfcc"], frames, lists[n], 12), a.launches), 3))
    res["dense_ns_per_pair"] = round(float(np.median(res["dense_ms"])) * 1e6 / (B * K), 3)
    ident = True
    for n in N_BEST:
        m = candidate_mask(torch, lists[n], K)
        pairs = int(m.sum())
        res[f"rescore_n{n}_pairs"] = pairs
        res[f"rescore_n{n}_ns_per_pair"] = round(float(np.median(res[f"rescore_n{n}_ms"])) * 1e6 / max(pairs, 1), 3)
        got = eng.rescore_nbest_dev(out["mfcc"], frames, lists[n], 12)
        want = eng.nbest_dev(torch.where(m, dense, torch.full_like(dense, -1)).contiguous(), n)
        torch.cuda.synchronize()
        ident = ident and bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
    res["identical_to_dense_mask_nbest"] = ident
    # the whole path: what a caller pays for DP-ranked words
    o2 = eng.alloc_outputs(B, torch.device("cuda", 0))

    def two_pass():
        eng.recognize_nbest_dev(pcm, o2, 4, rescore=True)

    def plain_plus_dense():
        eng.recognize_dev(pcm, out)
        eng.dtw_dp_dev(out["mfcc"], dense, vad=out["vad"])

    res.update(plain_ms=[], nbest4_ms=[], plain_plus_dense_ms=[], two_pass_n4_ms=[])
    for _ in range(3):
        res["plain_ms"].append(round(host_ms(torch, lambda: eng.recognize_dev(pcm, out), a.steps), 3))
        res["plain_plus_dense_ms"].append(round(host_ms(torch, plain_plus_dense, a.steps), 3))
        res["two_pass_n4_ms"].append(round(host_ms(torch, two_pass, a.steps), 3))
    torch.cuda.synchronize()
    stage = eng.rescore_nbest_dev(o2["mfcc"], o2["vad"][:, 9], o2["nbest"], 12)
    torch.cuda.synchronize()
    res["whole_path_equals_stage_call"] = bool(torch.equal(stage[0], o2["rescored"]) and torch.equal(stage[1], o2["n_rescored"]))
    res["two_pass_faster_than_plain_plus_dense"] = bool(max(res["two_pass_n4_ms"]) < min(res["plain_plus_dense_ms"]))
    if clk:
        clk.__exit__()
        res["sclk"] = clk.summary()
    else:
        res["sclk"] = None
    print(json.dumps(res), flush=True)
    eng.close()


def run_trace(a):
    torch, eng, pcm, out, lists, dense, K = setup(a.batch)
    frames = out["vad"][:, 9]
    for _ in range(6):
        eng.dtw_dp_dev(out["mfcc"], dense, vad=out["vad"])
    torch.cuda.synchronize()
    for _ in range(6):
        eng.rescore_nbest_dev(out["mfcc"], frames, lists[4], 12)
    torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
