"""Transcript-forced alignment (sr_align_transcripts_dp_dev) against the grammar-decoder calls it replaces, in one run.

    python profiles/experiments/forced_rate.py [--rows R] [--frames N] [--words W] [--launches L]
        R feature rows x N frames (random s16 features resident in HBM: the sweeps' work does not depend on the values)
        against a store of 100 templates of 80..120 frames, 10 slots per word, skipping on; every row has its own W-word
        transcript.  Three cases, each timed with device events over L repetitions, three alternations, on one engine of the
        testing library (the third case needs its hook; the other two run the same code with the hook at 0):
          forced      one sr_align_transcripts_dp_dev call over all rows;
          grammar     the R one-row sr_decode_grammar_dp_dev calls under grammar_sequence(transcript) with max_words =
                      n_words_exact = W that it replaces; the R grammars are created before the clock starts;
          prune_off   the forced call with the hook "forced_prune_off": every level sweeps every end frame.
        The three outputs are compared byte for byte, and one short row with the numpy definition (tests/forced_ref.py).
        One line of JSON.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP = 6000
K, SPW = 100, 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--launches", type=int, default=5)
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stm32_speech_recognition_amd import Engine, engine
    dev = torch.device("cuda", 0)
    R, N, W = a.rows, a.frames, a.words
    rng = np.random.default_rng(2031)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tm = np.zeros((K, 121, 12), np.int16)
    tm[:, :120] = rng.integers(-3000, 3001, (K, 120, 12))
    eng = Engine(max_frames=N, device=0, testing=True)
    eng.set_templates_dense(tm, tf)
    eng.set_word_map(slots_per_word=SPW)
    transcripts = []
    while len(transcripts) < R:  # a distinct transcript per row
        t = [int(w) for w in rng.integers(0, K // SPW, W)]
        if t not in transcripts:
            transcripts.append(t)
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (R, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((R,), N, dtype=torch.int32, device=dev)

    def outs():
        return torch.empty(R, 4, dtype=torch.int32, device=dev), torch.empty(R, W, 8, dtype=torch.int32, device=dev)

    out_f, out_g, out_p = outs(), outs(), outs()
    lc = torch.empty(1, W, dtype=torch.int32, device=dev)
    grams = [eng.grammar(*engine.grammar_sequence([[w] for w in t])) for t in transcripts]

    def forced():
        eng.align_transcripts_dev(rows, frames, transcripts, *out_f, SKIP, 0)

    def grammar():
        for r in range(R):
            eng.decode_grammar_dev(grams[r], rows[r:r + 1], frames[r:r + 1], out_g[0][r:r + 1], out_g[1][r:r + 1], lc, W, W, SKIP, 0)

    def prune_off():
        engine.dev_hook("forced_prune_off", 1)
        try:
            eng.align_transcripts_dev(rows, frames, transcripts, *out_p, SKIP, 0)
        finally:
            engine.dev_hook("forced_prune_off", 0)

    fns = dict(forced=forced, grammar=grammar, prune_off=prune_off)
    res = {"rows": R, "frames": N, "K": K, "slots_per_word": SPW, "words": W, "launches": a.launches, "ms": {k: [] for k in fns}}
    for _ in range(3):
        for k, fn in fns.items():
            res["ms"][k].append(round(event_ms(torch, fn, a.launches), 3))
    med = {k: float(np.median(v)) for k, v in res["ms"].items()}
    res["median_ms"] = med
    res["grammar_over_forced"] = round(med["grammar"] / med["forced"], 4)
    res["prune_off_over_forced"] = round(med["prune_off"] / med["forced"], 4)
    torch.cuda.synchronize()
    res["same_bytes"] = {k: bool(all(torch.equal(x, y) for x, y in zip(out_f, o))) for k, o in dict(grammar=out_g, prune_off=out_p).items()}
    res["ok_rows"] = int((out_f[0][:, 3] == 0).sum())
    # one short row against the definition
    import forced_ref
    n_chk = min(N, 700)
    rec, words = torch.empty(1, 4, dtype=torch.int32, device=dev), torch.empty(1, W, 8, dtype=torch.int32, device=dev)
    eng.align_transcripts_dev(rows[:1], torch.tensor([n_chk], dtype=torch.int32, device=dev), transcripts[:1], rec, words, SKIP, 0)
    torch.cuda.synchronize()
    want = forced_ref.align(rows[:1].cpu().numpy(), [n_chk], tm, tf, None, N, transcripts[:1], W, SKIP, 0, np.arange(K) // SPW)
    res["sample_equals_definition"] = bool(rec.cpu().numpy().tobytes() == want[0].tobytes() and words.cpu().numpy().tobytes() == want[1].tobytes())
    print(json.dumps(res), flush=True)
    for gm in grams:
        gm.close()
    eng.close()


if __name__ == "__main__":
    main()
