"""Grammar-constrained decoding (sr_decode_grammar_dp_dev), with the unconstrained decoder as the yardstick of the same run.

    python profiles/experiments/gram_rate.py [--rows R] [--frames N] [--words W] [--launches L]
        R feature rows x N frames against 100 templates of 80..120 frames (random s16 features resident in HBM: the sweeps'
        work does not depend on the values), skipping on.  Three comparisons, each timed with device events over L launches,
        three alternations, on one engine per store:
          anchor    the anchor grammar (one state, every word), max_words W, against sr_decode_words_dp_dev on the same rows:
                    identical cells; the difference is one charge pass per level and the per-state layout.
          command   "one of 20 commands, then three of 10 digits" over a store of the first 30 templates, max_words 4, against
                    the anchor grammar over the same 30 words: the expected ratio is that of the item-frame products
                    (sum over levels and items of the item's template frames).
          pairs     a word-pair grammar over the same 30 words with half the pairs forbidden, max_words W, against the anchor
                    over the 30 words: the same items per level past the first, plus 31-state close passes.
        One row of each grammar's output is compared with the numpy definition (tests/gram_ref.py) at a reduced size.  One
        line of JSON.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/gram_rate.py --trace [NAMES]
        The run to trace for a per-kernel breakdown (tracing only, the program after --): one warm-up and three launches of
        each named call (default chain,anchor; also anchor30_w4, command_w4, anchor30, pairs).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP = 6000
N_CMD, N_DIG = 20, 10


def setup(a):
    import torch
    sys.path.insert(0, ROOT)
    from stm32_speech_recognition_amd import Engine, engine
    dev = torch.device("cuda", 0)
    K, N, W = 100, a.frames, a.words
    rng = np.random.default_rng(2028)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tm = np.zeros((K, 121, 12), np.int16)
    tm[:, :120] = rng.integers(-3000, 3001, (K, 120, 12))
    eng = Engine(max_frames=N, device=0)
    eng.set_templates_dense(tm, tf)
    e30 = Engine(max_frames=N, device=0)  # the command-and-digits store: slots 0..19 commands, 20..29 digits
    e30.set_templates_dense(tm[:N_CMD + N_DIG], tf[:N_CMD + N_DIG])
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (a.rows, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((a.rows,), N, dtype=torch.int32, device=dev)

    def outs(w):
        return (torch.empty(a.rows, 4, dtype=torch.int32, device=dev), torch.empty(a.rows, w, 8, dtype=torch.int32, device=dev),
                torch.empty(a.rows, w, dtype=torch.int32, device=dev))

    out_w, out_4 = outs(W), outs(4)
    cmd, dig = list(range(N_CMD)), list(range(N_CMD, N_CMD + N_DIG))
    prng = np.random.default_rng(5)
    allowed = [(x, y) for x in range(30) for y in range(30) if prng.integers(0, 2)]
    gram_t = dict(anchor=engine.grammar_any(range(K)), anchor30=engine.grammar_any(range(30)),
                  command=engine.grammar_sequence([cmd, dig, dig, dig]), pairs=engine.grammar_word_pairs(range(30), allowed))
    grams = dict(anchor=eng.grammar(*gram_t["anchor"]), anchor30=e30.grammar(*gram_t["anchor30"]), command=e30.grammar(*gram_t["command"]),
                 pairs=e30.grammar(*gram_t["pairs"]))
    fns = dict(
        chain=lambda: eng.decode_words_dev(rows, frames, *out_w, W, 0, SKIP, 0),
        anchor=lambda: eng.decode_grammar_dev(grams["anchor"], rows, frames, *out_w, W, 0, SKIP, 0),
        anchor30_w4=lambda: e30.decode_grammar_dev(grams["anchor30"], rows, frames, *out_4, 4, 0, SKIP, 0),
        command_w4=lambda: e30.decode_grammar_dev(grams["command"], rows, frames, *out_4, 4, 0, SKIP, 0),
        anchor30=lambda: e30.decode_grammar_dev(grams["anchor30"], rows, frames, *out_w, W, 0, SKIP, 0),
        pairs=lambda: e30.decode_grammar_dev(grams["pairs"], rows, frames, *out_w, W, 0, SKIP, 0))
    return torch, (eng, e30), tm, tf, rows, gram_t, grams, fns, len(allowed)


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


def item_frames(gram_t, max_words, tf):
    """sum over the levels' items of the item's template frames: what the sweeps of one row column cost"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gram_ref
    return [int(sum(int(tf[k]) for k, _ in items)) for items in gram_ref.items_per_level(gram_t, max_words, range(len(tf)))]


def run(a):
    torch, engines, tm, tf, rows, gram_t, grams, fns, n_allowed = setup(a)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gram_ref
    N, W = a.frames, a.words
    res = {"rows": a.rows, "frames": N, "K": len(tf), "max_words": W, "launches": a.launches, "allowed_pairs_of_900": n_allowed,
           "plan": {k: grams[k].plan(4 if k == "command" else W) for k in grams}, "ms": {k: [] for k in fns}}
    res["plan"]["anchor30_w4"] = grams["anchor30"].plan(4)
    for _ in range(3):
        for k, fn in fns.items():
            res["ms"][k].append(round(event_ms(torch, fn, a.launches), 3))
    med = {k: float(np.median(v)) for k, v in res["ms"].items()}
    res["median_ms"] = med
    res["anchor_over_chain"] = round(med["anchor"] / med["chain"], 4)
    res["command_over_anchor30_w4"] = round(med["command_w4"] / med["anchor30_w4"], 4)
    f_cmd, f_any = item_frames(gram_t["command"], 4, tf[:30]), item_frames(gram_t["anchor30"], 4, tf[:30])
    res["item_frames_per_level"] = {"command": f_cmd, "anchor30_w4": f_any}
    res["command_over_anchor30_w4_expected"] = round(sum(f_cmd) / sum(f_any), 4)
    res["pairs_over_anchor30"] = round(med["pairs"] / med["anchor30"], 4)
    # one short row of each grammar against the definition, at most three levels
    n_chk, ok = min(N, 300), {}
    for name, (e, w) in dict(anchor=(engines[0], 2), command=(engines[1], 3), pairs=(engines[1], 3)).items():
        K = len(tf) if name == "anchor" else 30
        rec = torch.empty(1, 4, dtype=torch.int32, device=rows.device)
        words = torch.empty(1, w, 8, dtype=torch.int32, device=rows.device)
        lc = torch.empty(1, w, dtype=torch.int32, device=rows.device)
        e.decode_grammar_dev(grams[name], rows[:1], torch.tensor([n_chk], dtype=torch.int32, device=rows.device), rec, words, lc, w, 0, SKIP, 0)
        torch.cuda.synchronize()
        want = gram_ref.decode(gram_t[name], rows[:1].cpu().numpy(), [n_chk], tm[:K], tf[:K], None, N, w, 0, SKIP, 0)
        ok[name] = bool(rec.cpu().numpy().tobytes() == want[0].tobytes() and words.cpu().numpy().tobytes() == want[1].tobytes()
                        and lc.cpu().numpy().tobytes() == want[2].tobytes())
    res["sample_equals_definition"] = ok
    print(json.dumps(res), flush=True)
    for g in grams.values():
        g.close()
    for e in engines:
        e.close()


def run_trace(a):
    torch, engines, tm, tf, rows, gram_t, grams, fns, _ = setup(a)
    for k in a.trace.split(","):
        for _ in range(4):
            fns[k]()
        torch.cuda.synchronize()
    for g in grams.values():
        g.close()
    for e in engines:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--trace", nargs="?", const="chain,anchor", default="",
                    help="trace run: the calls to launch, of chain, anchor, anchor30_w4, command_w4, anchor30, pairs")
    a = ap.parse_args()
    run_trace(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
