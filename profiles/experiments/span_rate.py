"""Word alternatives (sr_decode_words_alts_dev), with the decoder alone as the yardstick of the same run.

    python profiles/experiments/span_rate.py [--rows R] [--frames N] [--words W] [--nbest B] [--launches L]
        R feature rows x N frames against 100 templates of 80..120 frames (random s16 features resident in HBM), max_words W,
        skipping on, n_best B.  Three calls on the same rows with the same engine, each timed with device events over L launches,
        three alternations: sr_decode_words_alts_dev (decoder + span scores + N-best), sr_decode_words_dp_dev alone, and
        sr_score_word_spans_dev alone over the word rows the decoder left.  The span stage walks every template over each decoded
        word's frames once -- about one level of the decoder, not W -- so the expectation is an addition near 1/W of the
        decode.  One row of span scores is compared with the numpy definition (tests/span_ref.py).  One line of JSON.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SKIP = 6000


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
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import span_ref
    from stm32_speech_recognition_amd import Engine
    from stm32_speech_recognition_amd.engine import CHAIN_WORD_DTYPE, SPAN_ACC
    dev = torch.device("cuda", 0)
    K, N, W, B = 100, a.frames, a.words, a.nbest
    rng = np.random.default_rng(2031)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tm = np.zeros((K, 121, 12), np.int16)
    tm[:, :120] = rng.integers(-3000, 3001, (K, 120, 12))
    eng = Engine(max_frames=N, device=0)
    eng.set_templates_dense(tm, tf)
    eng.set_word_map(None, 4)  # four slots per word, as the firmware enrols
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (a.rows, N, 12), generator=g, device=dev, dtype=torch.int16)
    frames = torch.full((a.rows,), N, dtype=torch.int32, device=dev)
    rec = torch.empty(a.rows, 4, dtype=torch.int32, device=dev)
    words = torch.empty(a.rows, W, 8, dtype=torch.int32, device=dev)
    lc = torch.empty(a.rows, W, dtype=torch.int32, device=dev)
    alts = torch.empty(a.rows, W, B, 4, dtype=torch.int32, device=dev)
    nm = torch.empty(a.rows, W, dtype=torch.int32, device=dev)
    sc = torch.empty(a.rows, W, K, dtype=torch.int32, device=dev)

    def fn_alts():
        eng.decode_words_alts_dev(rows, frames, rec, words, alts, lc, nm, None, W, SPAN_ACC, 0, SKIP, 0)

    def fn_decode():
        eng.decode_words_dev(rows, frames, rec, words, lc, W, 0, SKIP, 0)

    def fn_span():
        eng.score_word_spans_dev(rows, frames, words, sc, SPAN_ACC)

    fn_decode()
    torch.cuda.synchronize()
    w = words.cpu().numpy().view(CHAIN_WORD_DTYPE).reshape(a.rows, W)
    n_words = rec.cpu().numpy().view(np.uint32)[:, 1]
    used = [(int(x["end"]) - int(x["start"]) + 1) for r in range(a.rows) for x in w[r, :n_words[r]]]
    res = {"rows": a.rows, "frames": N, "K": K, "max_words": W, "n_best": B, "launches": a.launches, "decoded_words": len(used),
           "span_frames_share": round(sum(used) / (a.rows * N), 4), "alts_ms": [], "decode_ms": [], "span_stage_ms": []}
    for _ in range(3):
        res["decode_ms"].append(round(event_ms(torch, fn_decode, a.launches), 3))
        res["alts_ms"].append(round(event_ms(torch, fn_alts, a.launches), 3))
        res["span_stage_ms"].append(round(event_ms(torch, fn_span, a.launches), 3))
    al, de, sp = (float(np.median(res[k])) for k in ("alts_ms", "decode_ms", "span_stage_ms"))
    res["alts_over_decode"] = round(al / de, 4)
    res["span_stage_over_decode"] = round(sp / de, 4)
    # one row of span scores against the definition
    fn_span()
    torch.cuda.synchronize()
    want = span_ref.span_scores(rows[:1].cpu().numpy(), [N], tm, tf, None, w[:1], SPAN_ACC)
    res["sample_equals_definition"] = bool(sc[:1].cpu().numpy().view(np.uint32).tobytes() == want.tobytes())
    print(json.dumps(res), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--nbest", type=int, default=4)
    ap.add_argument("--launches", type=int, default=5)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
