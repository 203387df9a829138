"""Weighted grammars (sr_grammar_create_weighted) against the same grammar without costs, which launches the kernels measured by
gram_rate.py and gram_live_rate.py: what arc and final costs cost, batch and live.

    python profiles/experiments/gram_weight_rate.py [--rows R] [--frames N] [--words W] [--launches L] [--reps P] [--rounds N]
        The word-pair (bigram) grammar over 30 words, templates of 80..120 frames, skipping on (random s16 features resident in
        HBM: the sweeps' work does not depend on the values): 31 states, every pair allowed, once with bigram costs of 0..20 000
        on every arc and final state (grammar_bigram), once with zero costs made by sr_grammar_create.  Same process, the two
        alternated `rounds` times, each window timed with device events after a warm-up:
          batch   sr_decode_grammar_dp_dev on 64 rows x 2 048 frames, max_words W, L launches per window.  The weighted call
                  launches k_gram_charge_w and k_gram_trace_w in the places of k_gram_charge and k_gram_trace: the expectation
                  from the code is a ratio near 1, (charge lists) x (N + 1) additions next to items x N x M cells;
          live    64 channels at a prefix of 500 frames, P consecutive sr_gram_live_push_dev of 10 and of 100 frames per
                  window (the session ended and refilled before each): k_gram_live_words_w and k_gram_live_trace_w in the
                  places of the sweep and the trace.
        One row of the weighted batch output is compared with the numpy definition (tests/wgram_ref.py) at a reduced size, and
        the rows of the last live window with the batch call on the same frames.  One line of JSON.
    python profiles/experiments/gram_weight_rate.py --ab ab_libs/base.so ab_libs/new.so [--rounds N]
        ab.py's method applied to gram_rate.py: every round runs `gram_rate.py` once per library in a child process of its own
        (SR_ENGINE_LIB selects the library the package loads), alternating, so that clock drift of the box hits both builds
        alike.  Shows whether the unweighted kernels moved between two builds (profiles/experiments/ab_build.sh builds them).
        One line of JSON: per library and per case of gram_rate.py the median ms of every round, and new over base.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP, N_WORDS, PREFIX, PUSHES = 6000, 30, 500, (10, 100)


def bigram(rng):
    return [[int(c) for c in row] for row in rng.integers(0, 20001, (N_WORDS, N_WORDS))], [int(c) for c in rng.integers(0, 20001, N_WORDS)]


def run(a):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wgram_ref
    from stm32_speech_recognition_amd import Engine, engine
    dev = torch.device("cuda", 0)
    N, W, Cn = a.frames, a.words, a.rows
    rng = np.random.default_rng(2028)
    tf = rng.integers(80, 121, N_WORDS).astype(np.uint32)
    tm = np.zeros((N_WORDS, 121, 12), np.int16)
    tm[:, :120] = rng.integers(-3000, 3001, (N_WORDS, 120, 12))
    eng = Engine(max_frames=N, device=0)
    eng.set_templates_dense(tm, tf)
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (Cn, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((Cn,), N, dtype=torch.int32, device=dev)
    cost, last = bigram(np.random.default_rng(5))
    weighted_t = engine.grammar_bigram(range(N_WORDS), cost, None, last)
    grams = dict(weighted=eng.grammar(*weighted_t), plain=eng.grammar(*weighted_t[:3]))
    outs = (torch.empty(Cn, 4, dtype=torch.int32, device=dev), torch.empty(Cn, W, 8, dtype=torch.int32, device=dev),
            torch.empty(Cn, W, dtype=torch.int32, device=dev))
    res = {"rows": Cn, "frames": N, "words": N_WORDS, "max_words": W, "launches": a.launches, "reps": a.reps, "rounds": a.rounds,
           "plan": {k: v.plan(W) for k, v in grams.items()}, "batch_ms": {k: [] for k in grams}}

    def window(fn, reps):
        fn(0)  # warm-up: code objects, scratch
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for _ in range(a.rounds):
        for k, gr in grams.items():
            res["batch_ms"][k].append(round(window(lambda i: eng.decode_grammar_dev(gr, rows, frames, *outs, W, 0, SKIP, 0), a.launches), 3))
    med = {k: float(np.median(v)) for k, v in res["batch_ms"].items()}
    res["batch_weighted_over_plain"] = round(med["weighted"] / med["plain"], 4)

    # live: both sessions at PREFIX frames, reps pushes of n frames per window
    sessions = {k: eng.decode_grammar_live(gr, Cn, max(PUSHES), N, W, 0, SKIP) for k, gr in grams.items()}
    res["live_geometry"] = {k: engine.grammar_live_geometry(gr, W, N, max(PUSHES)) for k, gr in grams.items()}
    live_out = {}

    def refill(ses):
        ses.end(np.arange(Cn))
        for lo in range(0, PREFIX, max(PUSHES)):
            ses.push_dev(rows[:, lo:min(lo + max(PUSHES), PREFIX)].contiguous(), level_cost=False)

    for n in PUSHES:
        r = res[f"live_n{n}_ms"] = {k: [] for k in grams}
        chunks = [rows[:, PREFIX + i * n:PREFIX + (i + 1) * n].contiguous() for i in range(a.reps)]
        for _ in range(a.rounds):
            for k, ses in sessions.items():
                refill(ses)  # (untimed pushes: they warm the code objects as well)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.reps):
                    live_out[k] = ses.push_dev(chunks[i], level_cost=False)
                e1.record()
                torch.cuda.synchronize()
                r[k].append(round(e0.elapsed_time(e1) / a.reps, 4))
        m = {k: float(np.median(v)) for k, v in r.items()}
        res[f"live_n{n}_weighted_over_plain"] = round(m["weighted"] / m["plain"], 4)
    # the last live window's rows (weighted) against the batch call on the same frames
    n_live = PREFIX + a.reps * PUSHES[-1]
    eng.decode_grammar_dev(grams["weighted"], rows, torch.full((Cn,), n_live, dtype=torch.int32, device=dev), outs[0], outs[1], None, W, 0, SKIP, 0)
    torch.cuda.synchronize()
    o = live_out["weighted"]
    res["live_rows_equal_batch"] = bool(torch.equal(o["rec"], outs[0]) and torch.equal(o["words"], outs[1]) and o["n_rows"] == Cn)
    res["rows_with_a_parse"] = int((outs[0][:, 3] == 0).sum())
    # one short row against the definition, three levels
    n_chk = min(N, 300)
    rec, words, lc = (torch.empty(1, 4, dtype=torch.int32, device=dev), torch.empty(1, 3, 8, dtype=torch.int32, device=dev),
                      torch.empty(1, 3, dtype=torch.int32, device=dev))
    eng.decode_grammar_dev(grams["weighted"], rows[:1], torch.tensor([n_chk], dtype=torch.int32, device=dev), rec, words, lc, 3, 0, SKIP, 0)
    torch.cuda.synchronize()
    want = wgram_ref.decode(weighted_t, rows[:1].cpu().numpy(), [n_chk], tm, tf, None, N, 3, 0, SKIP, 0)
    res["sample_equals_definition"] = bool(rec.cpu().numpy().tobytes() == want[0].tobytes() and words.cpu().numpy().tobytes() == want[1].tobytes()
                                           and lc.cpu().numpy().tobytes() == want[2].tobytes())
    print(json.dumps(res), flush=True)
    for ses in sessions.values():
        ses.close()
    for gr in grams.values():
        gr.close()
    eng.close()


def run_ab(a):
    libs = {"base": os.path.abspath(a.ab[0]), "new": os.path.abspath(a.ab[1])}
    res = {"rounds": a.rounds, "ms": {k: {} for k in libs}}
    for _ in range(a.rounds):
        for name, lib in libs.items():
            out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "experiments", "gram_rate.py")], env=dict(os.environ, SR_ENGINE_LIB=lib),
                                 capture_output=True, text=True, timeout=300)
            if out.returncode:
                print(json.dumps({"failed": name, "rc": out.returncode, "stderr": out.stderr[-2000:]}), flush=True)
                sys.exit(1)  # nothing more is started on the device after a child that failed
            one = json.loads(out.stdout.strip().splitlines()[-1])
            for k, v in one["median_ms"].items():
                res["ms"][name].setdefault(k, []).append(v)
    res["new_over_base"] = {k: round(float(np.median(res["ms"]["new"][k]) / np.median(res["ms"]["base"][k])), 4) for k in res["ms"]["base"]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab", nargs=2, metavar=("BASE", "NEW"), help="two builds of libsr_engine.so: gram_rate.py under each, alternating")
    a = ap.parse_args()
    run_ab(a) if a.ab else run(a)


if __name__ == "__main__":
    main()
