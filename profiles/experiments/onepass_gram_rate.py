"""One-pass grammar decoding (sr_decode_onepass_grammar_dp_dev) against the one-pass decoder and against grammar level building
(sr_decode_grammar_dp_dev) in the same run.

    python profiles/experiments/onepass_gram_rate.py [--rows R] [--frames N] [--launches L]
        R feature rows x N frames against templates of 80..120 frames (random s16 features resident in HBM: the sweeps' work
        does not depend on the values), skipping on.  Three cases, each timed with device events over L launches, three
        alternations, medians:
          anchor   the anchor grammar over 100 templates against sr_decode_onepass_dp_dev on the same engine.  The cell counts
                   say the ratio is 1; what is added is the per-column charge loop (one state), the close over S = 1 states and
                   the trace's item search;
          repeat   "one of 20 commands, then any number of 10 digits" (grammar_repeat) over 30 templates against
                   sr_decode_grammar_dp_dev at max_words 8 and 16, which truncate the row;
          bigram   a weighted bigram grammar over the same 30 words against the same decoder at 8 and 16.
        With each case the launches of a call and the scratch bytes of a row (sr_onepass_grammar_plan, sr_grammar_plan).  One
        short row of every one-pass grammar output is compared with the definition (tests/onepass_gram_ref.py).  One line of
        JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/onepass_gram_rate.py --trace
        The run to trace for the per-kernel breakdown (tracing only, the program after --): one warm-up and three launches of
        the anchor case and of the one-pass decoder.  Compare k_onepass_gram_words with k_onepass_words, k_onepass_gram_close
        with k_onepass_close, and the two init kernels.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP = 6000
WORDS_CAP = 64


def store(K, seed):
    rng = np.random.default_rng(seed)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tm = np.zeros((K, 121, 12), np.int16)
    tm[:, :120] = rng.integers(-3000, 3001, (K, 120, 12))
    return tm, tf


def setup(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine, engine
    dev = torch.device("cuda", 0)
    N = a.frames
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (a.rows, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((a.rows,), N, dtype=torch.int32, device=dev)
    one = (torch.empty(a.rows, 4, dtype=torch.int32, device=dev), torch.empty(a.rows, WORDS_CAP, 8, dtype=torch.int32, device=dev))
    lev = {W: (torch.empty(a.rows, 4, dtype=torch.int32, device=dev), torch.empty(a.rows, W, 8, dtype=torch.int32, device=dev),
               torch.empty(a.rows, W, dtype=torch.int32, device=dev)) for W in (8, 16)}
    big, small = Engine(max_frames=N, device=0), Engine(max_frames=N, device=0)
    stores = dict(big=store(100, 2028), small=store(30, 2029))
    big.set_templates_dense(*stores["big"])
    small.set_templates_dense(*stores["small"])
    rng = np.random.default_rng(11)
    cost = rng.integers(0, 4001, (30, 30)).tolist()
    graphs = dict(anchor=engine.grammar_any(range(100)), repeat=engine.grammar_repeat([range(20)], range(20, 30), 1),
                  bigram=engine.grammar_bigram(range(30), cost, rng.integers(0, 4001, 30).tolist(), rng.integers(0, 4001, 30).tolist()))
    engs = dict(anchor=big, repeat=small, bigram=small)
    grams = {k: engs[k].grammar(*graphs[k]) for k in graphs}

    def fn_gram(k):
        return lambda: engs[k].decode_onepass_grammar_dev(grams[k], rows, frames, *one, WORDS_CAP, SKIP, 0)

    def fn_levels(k, W):
        return lambda: engs[k].decode_grammar_dev(grams[k], rows, frames, *lev[W], W, 0, SKIP, 0)

    def fn_onepass():
        big.decode_onepass_dev(rows, frames, *one, WORDS_CAP, SKIP, 0)

    return dict(torch=torch, engine=engine, rows=rows, one=one, engs=engs, grams=grams, graphs=graphs, stores=stores, fn_gram=fn_gram,
                fn_levels=fn_levels, fn_onepass=fn_onepass)


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
    s = setup(a)
    torch, engine = s["torch"], s["engine"]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import onepass_gram_ref
    N = a.frames
    res = {"rows": a.rows, "frames": N, "launches": a.launches}
    for case in ("anchor", "repeat", "bigram"):
        gram, eng = s["grams"][case], s["engs"][case]
        tm, tf = s["stores"]["big" if case == "anchor" else "small"]
        against = {"onepass": s["fn_onepass"]} if case == "anchor" else {"levels8": s["fn_levels"](case, 8), "levels16": s["fn_levels"](case, 16)}
        ms = {k: [] for k in ["gram"] + list(against)}
        for _ in range(3):
            for k, fn in against.items():
                ms[k].append(round(event_ms(torch, fn, a.launches), 3))
            ms["gram"].append(round(event_ms(torch, s["fn_gram"](case), a.launches), 3))
        plan = engine.onepass_grammar_plan(gram)
        out = {"ms": ms, "plan": plan, "words_per_row": [int(s["one"][0][:, 1].min()), int(s["one"][0][:, 1].max())]}
        med = float(np.median(ms["gram"]))
        for k in against:
            out["ratio_to_" + k] = round(med / float(np.median(ms[k])), 4)
        if case != "anchor":
            out["levels_plan"] = {W: {k: v for k, v in gram.plan(W).items() if k != "items_per_level"} for W in (8, 16)}
        # one short row against the definition
        n_chk = min(N, 100)
        r1 = torch.empty(1, 4, dtype=torch.int32, device=s["rows"].device)
        w1 = torch.empty(1, WORDS_CAP, 8, dtype=torch.int32, device=s["rows"].device)
        eng.decode_onepass_grammar_dev(gram, s["rows"][:1], torch.tensor([n_chk], dtype=torch.int32, device=s["rows"].device), r1, w1, WORDS_CAP, SKIP, 0)
        torch.cuda.synchronize()
        want = onepass_gram_ref.decode(s["graphs"][case], s["rows"][:1].cpu().numpy(), [n_chk], tm, tf, None, N, WORDS_CAP, SKIP, 0)
        out["sample_equals_definition"] = bool(r1.cpu().numpy().tobytes() == want[0].tobytes() and w1.cpu().numpy().tobytes() == want[1].tobytes())
        res[case] = out
    print(json.dumps(res), flush=True)
    for g in s["grams"].values():
        g.close()
    for e in set(s["engs"].values()):
        e.close()


def run_trace(a):
    s = setup(a)
    for fn in (s["fn_onepass"], s["fn_gram"]("anchor")):
        for _ in range(4):
            fn()
        s["torch"].cuda.synchronize()
    for g in s["grams"].values():
        g.close()
    for e in set(s["engs"].values()):
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
