"""Live one-pass decoding (sr_onepass_live_push_dev) against the two ways a caller had before it to follow a feed while it is
spoken: the level session's push (sr_decode_live_push_dev, at most 16 words) and sr_decode_onepass_dp_dev over the whole
prefix so far.

    python profiles/experiments/onepass_live_rate.py [--channels C] [--reps R] [--rounds N]
        64 channels x 100 templates of 80..120 rows, skipping on (random s16 features resident in HBM: the kernels' work does
        not depend on the values).  Per prefix length P in (500, 2000) and push size n in (10, 100):
          onepass   R consecutive sr_onepass_live_push_dev of n frames per channel that take every channel from P to P + R*n
                    frames (the session is ended and refilled to P by untimed pushes before each timed window);
          level8    the same pushes into a sr_decode_live session at max_words 8;
          level16   ... and at max_words 16;
          batch     sr_decode_onepass_dp_dev over 64 rows of P + n frames (frames_cap = P + n): what re-decoding the prefix costs
                    after the first of those pushes;
          floor     R one-pass pushes of ONE frame at the same prefix: a sweep, a close, a trace and a plan upload with next to
                    no cells, the fixed cost of a push.
        Same process, the five alternated `rounds` times, each window timed with device events after a warm-up; the host's
        wall time per call next to it.  vs_level8 / vs_level16 = onepass / level; vs_batch = onepass / batch beside the cell
        ratio n / (P + n); launch_share = floor / onepass.  After the last window the rows of the one-pass session are compared
        with the batch call's on the same frames, byte for byte.  One line of JSON.
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
WORDS_CAP, SKIP = 64, 1500
NAMES = ("floor", "onepass", "level8", "level16", "batch")


def run(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine, engine
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
    b_words = torch.empty(Cn, WORDS_CAP, 8, dtype=torch.int32, device=dev)
    geo = engine.onepass_live_geometry(M, K, int(tf.min()), maxf, max(PUSHES))
    ses = {"onepass": eng.decode_onepass_live(Cn, max(PUSHES), maxf, WORDS_CAP, False, SKIP),
           "level8": eng.decode_live(Cn, max(PUSHES), maxf, 8, 0, SKIP), "level16": eng.decode_live(Cn, max(PUSHES), maxf, 16, 0, SKIP)}
    res = {"channels": Cn, "K": K, "tpl_rows_max": M, "L": geo["block"], "words_cap": WORDS_CAP, "reps": R, "rounds": a.rounds,
           "launches_per_push": {n: 2 * -(-n // geo["block"]) + 1 for n in (1,) + PUSHES}, "level_launches_per_push": {"level8": 18, "level16": 34},
           "state_bytes_per_channel": {"onepass": geo["state_bytes"], "level8": engine.decode_live_geometry(M, K, 8, maxf, 100)["state_bytes"],
                                       "level16": engine.decode_live_geometry(M, K, 16, maxf, 100)["state_bytes"]}}

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

    def refill(s, P):
        """every channel ended, then pushed to P frames"""
        s.end(np.arange(Cn))
        for lo in range(0, P, max(PUSHES)):
            s.push_dev(rows[:, lo:min(lo + max(PUSHES), P)].contiguous(), level_cost=False)

    last = None
    for P in PREFIXES:
        for n in PUSHES:
            r = res[f"P{P}_n{n}"] = {f"{k}_{w}": [] for k in NAMES for w in ("ms", "host_ms")}
            r["cell_ratio"] = round(n / (P + n), 4)
            chunks = [rows[:, P + i * n:P + (i + 1) * n].contiguous() for i in range(R)]
            ones = [rows[:, P + i:P + i + 1].contiguous() for i in range(R)]
            frames = torch.full((Cn,), P + n, dtype=torch.int32, device=dev)
            out = {}

            def push(name, data):
                def fn(i):
                    out[name] = ses[name].push_dev(data[i], level_cost=False)
                return fn

            def batch(i):
                eng.decode_onepass_dev(rows, frames, b_rec, b_words, WORDS_CAP, SKIP, 0, P + n)

            batch(0)  # warm-up: code objects, scratch
            for _ in range(a.rounds):
                for name, s, fn, reps in (("floor", "onepass", push("onepass", ones), R), ("onepass", "onepass", push("onepass", chunks), R),
                                          ("level8", "level8", push("level8", chunks), R), ("level16", "level16", push("level16", chunks), R),
                                          ("batch", None, batch, max(R // 4, 1))):
                    if s:
                        refill(ses[s], P)
                    ms, host = window(fn, reps)
                    r[f"{name}_ms"].append(round(ms, 4))
                    r[f"{name}_host_ms"].append(round(host, 4))
            med = {k: float(np.median(r[f"{k}_ms"])) for k in NAMES}
            r["median_ms"] = {k: round(v, 4) for k, v in med.items()}
            r["vs_level8"] = round(med["onepass"] / med["level8"], 4)
            r["vs_level16"] = round(med["onepass"] / med["level16"], 4)
            r["vs_batch"] = round(med["onepass"] / med["batch"], 4)
            r["launch_share"] = round(med["floor"] / med["onepass"], 4)
            last = (P + R * n, out["onepass"])
    # the rows of the last one-pass window against the batch call on the same frames
    N, o = last
    frames = torch.full((Cn,), N, dtype=torch.int32, device=dev)
    eng.decode_onepass_dev(rows, frames, b_rec, b_words, WORDS_CAP, SKIP, 0, N)
    torch.cuda.synchronize()
    res["frames_compared"] = N
    res["rows_equal_batch"] = bool(torch.equal(o["rec"], b_rec) and torch.equal(o["words"], b_words) and o["n_rows"] == Cn)
    for s in ses.values():
        s.close()
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
