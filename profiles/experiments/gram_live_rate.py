"""Live grammar-constrained decoding (sr_gram_live_push_dev) against the two routes a caller had before it: the grammar decoder
over the whole prefix so far (sr_decode_grammar_dp_dev), and the live decoder without a grammar (sr_decode_live_push_dev).

    python profiles/experiments/gram_live_rate.py [--channels C] [--reps R] [--rounds N]
        64 channels, templates of 80..120 rows, max_words 8, skipping on (random s16 features resident in HBM: the kernels' work
        does not depend on the values).  Two grammars, each on an engine with its own store:
          anchor    the anchor grammar (one state, every word) over 100 templates: 8 levels of 100 items, 18 launches a push;
          command   "one of 20 commands, then three of 10 digits" over its 30 words: levels of 20, 10, 10, 10 items, the levels
                    5..8 keep none, 10 launches a push.
        Per grammar, prefix length P in (500, 2000) and push size n in (10, 100):
          live      R consecutive sr_gram_live_push_dev of n frames per channel that take every channel from P to P + R*n
                    frames (the session is ended and refilled to P by untimed pushes before each timed window);
          batch     sr_decode_grammar_dp_dev over 64 rows of P + n frames: what decoding the prefix again costs after the
                    first of those pushes;
          free      (anchor only) the same R pushes into a sr_decode_live_push_dev session on the same store.
        Same process, the calls alternated `rounds` times, each window timed with device events after a warm-up; the host's
        wall time per call next to it.  After the last window of each grammar the rows of the live session are compared with
        the batch decoder's on the same frames, byte for byte.  One line of JSON, the device's shader clock in it.
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
N_CMD, N_DIG = 20, 10


def run(a):
    import torch
    sys.path.insert(0, ROOT)
    from bench import ClockSampler  # the shader clock of this process's GPU, sampled from sysfs while the windows run
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
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (Cn, maxf, 12), generator=g, device=dev, dtype=torch.int16)
    b_rec = torch.empty(Cn, 4, dtype=torch.int32, device=dev)
    b_words = torch.empty(Cn, MAX_WORDS, 8, dtype=torch.int32, device=dev)
    res = {"channels": Cn, "tpl_rows_max": M, "max_words": MAX_WORDS, "reps": R, "rounds": a.rounds}

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

    cmd, dig = list(range(N_CMD)), list(range(N_CMD, N_CMD + N_DIG))
    with ClockSampler(device=0) as clock:
        for name, n_tpl, gram_t in (("anchor", K, engine.grammar_any(range(K))), ("command", N_CMD + N_DIG, engine.grammar_sequence([cmd, dig, dig, dig]))):
            eng = Engine(max_frames=maxf, device=0)
            eng.set_templates_dense(tm[:n_tpl], tf[:n_tpl])
            gram = eng.grammar(*gram_t)
            sessions = {"live": eng.decode_grammar_live(gram, Cn, max(PUSHES), maxf, MAX_WORDS, 0, SKIP)}
            if name == "anchor":
                sessions["free"] = eng.decode_live(Cn, max(PUSHES), maxf, MAX_WORDS, 0, SKIP)
            geo = engine.grammar_live_geometry(gram, MAX_WORDS, maxf, max(PUSHES))
            out_g = res[name] = {"templates": n_tpl, "items_per_level": gram.plan(MAX_WORDS)["items_per_level"], "launches_per_push": geo["launches"],
                                 "columns": geo["columns"], "state_bytes_per_channel": geo["state_bytes"]}

            def refill(ses, P):
                """every channel ended, then pushed to P frames"""
                ses.end(np.arange(Cn))
                for lo in range(0, P, max(PUSHES)):
                    ses.push_dev(rows[:, lo:min(lo + max(PUSHES), P)].contiguous(), level_cost=False)

            last = None
            for P in PREFIXES:
                for n in PUSHES:
                    calls = list(sessions) + ["batch"]
                    r = out_g[f"P{P}_n{n}"] = {f"{c}_{k}": [] for c in calls for k in ("ms", "host_ms")}
                    chunks = [rows[:, P + i * n:P + (i + 1) * n].contiguous() for i in range(R)]
                    frames = torch.full((Cn,), P + n, dtype=torch.int32, device=dev)
                    out = {}

                    def push(ses_name):
                        def fn(i):
                            out[ses_name] = sessions[ses_name].push_dev(chunks[i], level_cost=False)
                        return fn

                    def batch(i):
                        eng.decode_grammar_dev(gram, rows, frames, b_rec, b_words, None, MAX_WORDS, 0, SKIP, 0)

                    batch(0)  # warm-up: code objects, scratch
                    for _ in range(a.rounds):
                        for c in calls:
                            if c != "batch":
                                refill(sessions[c], P)
                            ms, host = window(batch if c == "batch" else push(c), max(R // 4, 1) if c == "batch" else R)
                            r[f"{c}_ms"].append(round(ms, 4))
                            r[f"{c}_host_ms"].append(round(host, 4))
                    med = {c: float(np.median(r[f"{c}_ms"])) for c in calls}
                    r["live_over_batch"] = round(med["live"] / med["batch"], 4)
                    r["cell_ratio"] = round(n / (P + n), 4)
                    if "free" in med:
                        r["live_over_free"] = round(med["live"] / med["free"], 4)
                    last = (P + R * n, out["live"])
            # the rows of the last live window against the batch grammar decoder on the same frames
            N, o = last
            frames = torch.full((Cn,), N, dtype=torch.int32, device=dev)
            eng.decode_grammar_dev(gram, rows, frames, b_rec, b_words, None, MAX_WORDS, 0, SKIP, 0)
            torch.cuda.synchronize()
            out_g["frames_compared"] = N
            out_g["rows_equal_batch"] = bool(torch.equal(o["rec"], b_rec) and torch.equal(o["words"], b_words) and o["n_rows"] == Cn)
            out_g["rows_with_a_parse"] = int((b_rec[:, 3] == 0).sum())
            for ses in sessions.values():
                ses.close()
            gram.close()
            eng.close()
    res["shader_clock"] = clock.summary()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
