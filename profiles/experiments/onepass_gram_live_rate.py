"""Live one-pass grammar decoding (sr_onepass_gram_live_push_dev) against what a caller with a grammar on a feed had before it:
the level session under the grammar (sr_gram_live_push_dev, at most 16 words) and sr_decode_onepass_grammar_dp_dev over the
whole prefix so far; and, under the anchor grammar, against the session without a grammar (sr_onepass_live_push_dev).

    python profiles/experiments/onepass_gram_live_rate.py [--channels C] [--reps R] [--rounds N]
        64 channels, templates of 80..120 rows, utt_frames 4 000, skipping on (random s16 features resident in HBM: the kernels'
        work does not depend on the values).  Three grammars, each on an engine with its own store:
          anchor    the anchor grammar (one state, every word) over 100 templates;
          command   "one of 20 commands, then any number of 10 digits" (grammar_repeat) over its 30 words;
          bigram    a weighted bigram grammar over 30 words: 31 states, every pair allowed at a drawn cost.
        Per grammar, prefix length P in (500, 2000) and push size n in (10, 100):
          live      R consecutive sr_onepass_gram_live_push_dev of n frames per channel that take every channel from P to
                    P + R*n frames (the session is ended and refilled to P by untimed pushes before each timed window);
          floor     R such pushes of ONE frame at the same prefix: a sweep, a close, a trace and a plan upload with next to no
                    cells, the fixed cost of a push;
          free      (anchor only) the same R pushes into a sr_onepass_live session on the same store;
          level8    (command, bigram) the same pushes into a sr_gram_live session at max_words 8;
          level16   ... and at max_words 16;
          batch     sr_decode_onepass_grammar_dp_dev over 64 rows of P + n frames (frames_cap = P + n): what decoding the
                    prefix again costs after the first of those pushes.
        Same process, the calls alternated `rounds` times, each window timed with device events after a warm-up; the host's wall
        time per call next to it; per call the median over the rounds and the spread (max - min) / median.  State bytes per
        channel beside sr_gram_live_geometry's.  After the last window of each grammar the rows of the live session are
        compared with the batch decoder's on the same frames, byte for byte.  One line of JSON, the device's shader clock in it.
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
    b_words = torch.empty(Cn, WORDS_CAP, 8, dtype=torch.int32, device=dev)
    res = {"channels": Cn, "tpl_rows_max": M, "utt_frames": maxf, "words_cap": WORDS_CAP, "reps": R, "rounds": a.rounds}

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
    n_w = N_CMD + N_DIG
    pair_cost = {x: {y: int(c) for y, c in enumerate(rng.integers(0, 4000, n_w))} for x in range(n_w)}
    grams = (("anchor", K, engine.grammar_any(range(K))), ("command", n_w, engine.grammar_repeat([cmd], dig, 1)),
             ("bigram", n_w, engine.grammar_bigram(range(n_w), pair_cost)))
    with ClockSampler(device=0) as clock:
        for name, n_tpl, gram_t in grams:
            eng = Engine(max_frames=maxf, device=0)
            eng.set_templates_dense(tm[:n_tpl], tf[:n_tpl])
            gram = eng.grammar(*gram_t)
            sessions = {"live": eng.decode_onepass_grammar_live(gram, Cn, max(PUSHES), maxf, WORDS_CAP, False, SKIP)}
            geo = engine.onepass_grammar_live_geometry(gram, maxf, max(PUSHES))
            out_g = res[name] = {"templates": n_tpl, "states": gram_t[0], "kept_items": geo["items"], "kept_states": geo["states"], "L": geo["block"],
                                 "launches_per_push": {n: engine.onepass_grammar_live_geometry(gram, maxf, n)["launches"] for n in (1,) + PUSHES},
                                 "state_bytes_per_channel": {"live": geo["state_bytes"]}}
            if name == "anchor":
                sessions["free"] = eng.decode_onepass_live(Cn, max(PUSHES), maxf, WORDS_CAP, False, SKIP)
                out_g["state_bytes_per_channel"]["free"] = engine.onepass_live_geometry(M, n_tpl, int(tf[:n_tpl].min()), maxf, max(PUSHES))["state_bytes"]
            else:
                for mw in (8, 16):
                    sessions[f"level{mw}"] = eng.decode_grammar_live(gram, Cn, max(PUSHES), maxf, mw, 0, SKIP)
                    lg = engine.grammar_live_geometry(gram, mw, maxf, max(PUSHES))
                    out_g["state_bytes_per_channel"][f"level{mw}"] = lg["state_bytes"]
                    out_g.setdefault("level_launches_per_push", {})[f"level{mw}"] = lg["launches"]

            def refill(ses, P):
                """every channel ended, then pushed to P frames"""
                ses.end(np.arange(Cn))
                for lo in range(0, P, max(PUSHES)):
                    ses.push_dev(rows[:, lo:min(lo + max(PUSHES), P)].contiguous(), level_cost=False)

            last = None
            for P in PREFIXES:
                for n in PUSHES:
                    calls = ["floor"] + list(sessions) + ["batch"]
                    r = out_g[f"P{P}_n{n}"] = {f"{c}_{k}": [] for c in calls for k in ("ms", "host_ms")}
                    chunks = [rows[:, P + i * n:P + (i + 1) * n].contiguous() for i in range(R)]
                    ones = [rows[:, P + i:P + i + 1].contiguous() for i in range(R)]
                    frames = torch.full((Cn,), P + n, dtype=torch.int32, device=dev)
                    out = {}

                    def push(ses_name, data):
                        def fn(i):
                            out[ses_name] = sessions[ses_name].push_dev(data[i], level_cost=False)
                        return fn

                    def batch(i):
                        eng.decode_onepass_grammar_dev(gram, rows, frames, b_rec, b_words, WORDS_CAP, SKIP, 0, P + n)

                    batch(0)  # warm-up: code objects, scratch
                    for _ in range(a.rounds):
                        for c in calls:
                            if c != "batch":
                                refill(sessions["live" if c == "floor" else c], P)
                            fn = batch if c == "batch" else push("live", ones) if c == "floor" else push(c, chunks)
                            ms, host = window(fn, max(R // 4, 1) if c == "batch" else R)
                            r[f"{c}_ms"].append(round(ms, 4))
                            r[f"{c}_host_ms"].append(round(host, 4))
                    med = {c: float(np.median(r[f"{c}_ms"])) for c in calls}
                    r["median_ms"] = {c: round(v, 4) for c, v in med.items()}
                    r["spread"] = {c: round((max(r[f"{c}_ms"]) - min(r[f"{c}_ms"])) / med[c], 4) for c in calls}
                    r["cell_ratio"] = round(n / (P + n), 4)
                    r["live_over_batch"] = round(med["live"] / med["batch"], 4)
                    r["launch_share"] = round(med["floor"] / med["live"], 4)
                    for c in ("free", "level8", "level16"):
                        if c in med:
                            r[f"live_over_{c}"] = round(med["live"] / med[c], 4)
                    last = (P + R * n, out["live"])
            # the rows of the last live window against the batch one-pass grammar decoder on the same frames
            N, o = last
            frames = torch.full((Cn,), N, dtype=torch.int32, device=dev)
            eng.decode_onepass_grammar_dev(gram, rows, frames, b_rec, b_words, WORDS_CAP, SKIP, 0, N)
            torch.cuda.synchronize()
            out_g["frames_compared"] = N
            out_g["rows_equal_batch"] = bool(torch.equal(o["rec"], b_rec) and torch.equal(o["words"], b_words) and o["n_rows"] == Cn)
            out_g["rows_with_a_parse"] = int((b_rec[:, 3] != 1).sum())
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
