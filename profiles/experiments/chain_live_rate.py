"""Live connected-word decoding (sr_decode_live_push_dev) against the only way a caller had before it to follow an utterance
while it is spoken: sr_decode_words_dp_dev over the whole prefix so far.

    python profiles/experiments/chain_live_rate.py [--channels C] [--reps R] [--rounds N]
        64 channels x 100 templates of 80..120 rows, max_words 8, skipping on (random s16 features resident in HBM: the
        kernels' work does not depend on the values).  Per prefix length P in (500, 2000) and push size n in (10, 100):
          live     R consecutive sr_decode_live_push_dev of n frames per channel that take every channel from P to P + R*n
                   frames (the session is ended and refilled to P by untimed pushes before each timed window);
          batch    sr_decode_words_dp_dev over 64 rows of P + n frames: what re-decoding the prefix costs after the first of
                   those pushes;
          floor    R pushes of ONE frame at the same prefix: 2 * max_words + 2 launches and a plan upload with next to no
                   cells, the fixed cost of a push.
        Same process, the three alternated `rounds` times, each window timed with device events after a warm-up; the host's
        wall time per call next to it.  ratio = live / batch beside the cell-count ratio n / (P + n); launch_share = floor /
        live.  After the last window the rows of the live session are compared with the batch decoder's on the same frames,
        byte for byte.  One line of JSON.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PREFIXES = (500, 2000)
PUSHES = (10, 100)
MAX_WORDS, SKIP = 8, 1500


def run(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine
    dev = torch.device("cuda", 0)
    K, Cn, R = 100, a.channels, a.reps
    rng = np.random.default_rng(2028)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tf[0] = 120
    M = int(tf.max())
    tm = np.zeros((K, M + 1, 12), np.int16)
    tm[:, :M] = rng.integers(-3000, 3001, (K, M, 12))
    maxf = max(PREFIXES) + R * max(PUSHES)
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (Cn, maxf, 12), generator=g, device=dev, dtype=torch.int16)
    b_rec = torch.empty(Cn, 4, dtype=torch.int32, device=dev)
    b_words = torch.empty(Cn, MAX_WORDS, 8, dtype=torch.int32, device=dev)
    ses = eng.decode_live(Cn, max(PUSHES), maxf, MAX_WORDS, 0, SKIP)
    res = {"channels": Cn, "K": K, "tpl_rows_max": M, "max_words": MAX_WORDS, "reps": R, "rounds": a.rounds,
           "launches_per_push": 2 * MAX_WORDS + 2}

    def window(fn, reps):
        """reps calls of fn(i) between two device events -> (device ms per call, host ms per call)"""
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, host * 1e3 / reps

    def refill(P):
        """every channel ended, then pushed to P frames"""
        ses.end(np.arange(Cn))
        for lo in range(0, P, max(PUSHES)):
            ses.push_dev(rows[:, lo:min(lo + max(PUSHES), P)].contiguous(), level_cost=False)

    last = None
    for P in PREFIXES:
        for n in PUSHES:
            r = res[f"P{P}_n{n}"] = {"live_ms": [], "live_host_ms": [], "batch_ms": [], "batch_host_ms": [], "floor_ms": [], "floor_host_ms": [],
                                     "cell_ratio": round(n / (P + n), 4)}
            chunks = [rows[:, P + i * n:P + (i + 1) * n].contiguous() for i in range(R)]
            ones = [rows[:, P + i:P + i + 1].contiguous() for i in range(R)]
            frames = torch.full((Cn,), P + n, dtype=torch.int32, device=dev)
            out = {}

            def live(i):
                out["last"] = ses.push_dev(chunks[i], level_cost=False)

            def floor(i):
                ses.push_dev(ones[i], level_cost=False)

            def batch(i):
                eng.decode_words_dev(rows, frames, b_rec, b_words, None, MAX_WORDS, 0, SKIP, 0)

            batch(0)  # warm-up: code objects, scratch
            for _ in range(a.rounds):
                for name, fn, reps in (("floor", floor, R), ("live", live, R), ("batch", batch, max(R // 4, 1))):
                    if name != "batch":
                        refill(P)
                    ms, host = window(fn, reps)
                    r[f"{name}_ms"].append(round(ms, 4))
                    r[f"{name}_host_ms"].append(round(host, 4))
            med = {k: float(np.median(r[f"{k}_ms"])) for k in ("live", "batch", "floor")}
            r["ratio"] = round(med["live"] / med["batch"], 4)
            r["launch_share"] = round(med["floor"] / med["live"], 4)
            last = (P + R * n, out["last"])
    # the rows of the last live window against the batch decoder on the same frames
    N, o = last
    frames = torch.full((Cn,), N, dtype=torch.int32, device=dev)
    eng.decode_words_dev(rows, frames, b_rec, b_words, None, MAX_WORDS, 0, SKIP, 0)
    torch.cuda.synchronize()
    res["frames_compared"] = N
    res["rows_equal_batch"] = bool(torch.equal(o["rec"], b_rec) and torch.equal(o["words"], b_words) and o["n_rows"] == Cn)
    ses.close()
    print(json.dumps(res), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
