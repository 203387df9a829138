"""What a commit call of a live one-pass grammar session (sr_onepass_gram_live_commit_dev) costs next to the push it follows, and
whether the push itself costs what it cost before the call existed.

    python profiles/experiments/onepass_gram_commit_rate.py [--channels C] [--reps R] [--rounds N]
        onepass_gram_live_rate.py's shapes: 64 channels, templates of 80..120 rows, utt_frames 4 000, and its three grammars,
        each on an engine with its own store: anchor (one state, 100 templates, W = 239), command ("one of 20 commands, then
        any number of 10 digits", 3 states) and bigram (weighted, 31 states, every pair at a drawn cost).  The channels hear
        templates of the grammar's store in random order with noise of +-60, so that the parse holds words and the commit node
        moves.  Skipping ON (the section's setting; under command and bigram the start state then stays reachable and the
        common node is the root as soon as it is scanned) and OFF (every kept state is scanned and the walks are folded).  Per
        grammar, skip setting, prefix length P in (500, 2000) and push size n in (10, 100): R times a push of n frames per
        channel and a commit of every channel behind it, each call between two device events of its own; the session is ended
        and refilled to P by untimed pushes and one commit before each timed window.  commit_vs_push = median commit / median
        push.  After the last window the last commit's counts are held against the end call's rows (no more words than the
        parse, no frame past N).  One line of JSON.
    python profiles/experiments/onepass_gram_commit_rate.py --ab ab_libs/base.so ab_libs/new.so [--rounds N]
        the push alone under two builds of the library (profiles/experiments/ab_build.sh), each in a child process of its own,
        alternating, on one box: ms per push for the same grammars, P and n.  A line of JSON per child.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PREFIXES = (500, 2000)
PUSHES = (10, 100)
WORDS_CAP, SKIP = 64, 1500
N_CMD, N_DIG = 20, 10


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
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    maxf = max(PREFIXES) + R * max(PUSHES)
    cmd, dig = list(range(N_CMD)), list(range(N_CMD, N_CMD + N_DIG))
    n_w = N_CMD + N_DIG
    pair_cost = {x: {y: int(c) for y, c in enumerate(rng.integers(0, 4000, n_w))} for x in range(n_w)}
    grams = (("anchor", K, engine.grammar_any(range(K))), ("command", n_w, engine.grammar_repeat([cmd], dig, 1)),
             ("bigram", n_w, engine.grammar_bigram(range(n_w), pair_cost)))
    res = {"channels": Cn, "tpl_rows_max": M, "utt_frames": maxf, "words_cap": WORDS_CAP, "reps": R, "rounds": a.rounds, "commit": not a.push_only}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        return (e0, e1), out

    for name, n_tpl, gram_t in grams:
        if a.only and name not in a.only:
            continue
        host_rows = np.zeros((Cn, maxf + M, 12), np.int16)
        for c in range(Cn):
            at, first = 0, True
            while at < maxf:  # a command first, then digits, where the grammar tells them apart
                k = int(rng.integers(0, n_tpl)) if name != "command" else int(rng.integers(0, N_CMD)) if first else int(rng.integers(N_CMD, n_w))
                first = False
                host_rows[c, at:at + tf[k]] = tm[k, :tf[k]]
                at += int(tf[k])
        host_rows = (host_rows[:, :maxf] + rng.integers(-60, 61, (Cn, maxf, 12))).astype(np.int16)
        rows = torch.from_numpy(host_rows).to(dev)
        eng = Engine(max_frames=maxf, device=0)
        eng.set_templates_dense(tm[:n_tpl], tf[:n_tpl])
        gram = eng.grammar(*gram_t)
        geo = engine.onepass_grammar_live_geometry(gram, maxf, max(PUSHES))
        out_g = res[name] = {"templates": n_tpl, "states": gram_t[0], "kept_items": geo["items"], "kept_states": geo["states"],
                             "W": 2 * int(tf[:n_tpl].max()) - 1}
        for skip in (SKIP, None):
            if a.push_only and skip is None:
                continue
            ses = eng.decode_onepass_grammar_live(gram, Cn, max(PUSHES), maxf, WORDS_CAP, False, skip)

            def refill(P):
                ses.end(np.arange(Cn))
                for lo in range(0, P, max(PUSHES)):
                    ses.push_dev(rows[:, lo:min(lo + max(PUSHES), P)].contiguous())
                if not a.push_only:
                    ses.commit_dev()

            last = None
            for P in PREFIXES:
                for n in PUSHES:
                    r = out_g[f"skip_{'on' if skip else 'off'}_P{P}_n{n}"] = {"push_ms": [], "commit_ms": []}
                    chunks = [rows[:, P + i * n:P + (i + 1) * n].contiguous() for i in range(R)]
                    for _ in range(a.rounds):
                        refill(P)
                        torch.cuda.synchronize()
                        ev = {"push_ms": [], "commit_ms": []}
                        for i in range(R):
                            ev["push_ms"].append(timed(lambda: ses.push_dev(chunks[i]))[0])
                            if not a.push_only:
                                pair, last = timed(ses.commit_dev)
                                ev["commit_ms"].append(pair)
                        torch.cuda.synchronize()
                        for k, pairs in ev.items():
                            if pairs:
                                r[k].append(round(float(np.mean([e0.elapsed_time(e1) for e0, e1 in pairs])), 4))
                    r["median_ms"] = {k[:-3]: round(float(np.median(v)), 4) for k, v in r.items() if isinstance(v, list) and v}
                    r["spread"] = {k[:-3]: round((max(v) - min(v)) / float(np.median(v)), 4) for k, v in r.items() if isinstance(v, list) and v}
                    if not a.push_only:
                        r["commit_vs_push"] = round(r["median_ms"]["commit"] / r["median_ms"]["push"], 4)
                        r["n_committed_mean"] = round(float(last["crec"][:, 0].float().mean().item()), 2)
            if not a.push_only:
                crec = last["crec"].cpu().numpy()
                end = ses.end(np.arange(Cn))
                parsed = end["rec"]["status"] != 1
                out_g[f"skip_{'on' if skip else 'off'}_checks"] = {
                    "rows_with_a_parse": int(parsed.sum()), "committed_le_parsed": bool(np.all(crec[parsed, 0] <= end["rec"]["n_words"][parsed])),
                    "frames_le_N": bool(np.all(crec[:, 3] <= end["rows"]["frames"]))}
            ses.close()
        gram.close()
        eng.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", nargs="*", help="grammars to run (default: all three)")
    ap.add_argument("--push-only", action="store_true", help="time the pushes alone, skipping on (what --ab runs under each library)")
    ap.add_argument("--ab", nargs=2, metavar="LIB")
    a = ap.parse_args()
    if not a.ab:
        return run(a)
    for _ in range(a.rounds):
        for lib in a.ab:
            env = dict(os.environ, SR_ENGINE_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, __file__, "--push-only", "--rounds", "1", "--channels", str(a.channels), "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=500)
            print(os.path.basename(lib), p.stdout.strip().splitlines()[-1] if p.stdout.strip() else p.stderr[-600:], flush=True)


if __name__ == "__main__":
    main()
