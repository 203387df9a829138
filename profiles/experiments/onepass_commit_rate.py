"""What a commit call of a live one-pass session (sr_onepass_live_commit_dev) costs next to the push it follows, and whether the
push itself costs what it cost before the call existed.

    python profiles/experiments/onepass_commit_rate.py [--channels C] [--reps R] [--rounds N]
        onepass_live_rate.py's shape: 64 channels x 100 templates of 80..120 rows (W = 239), skipping on.  The channels hear
        templates in random order with noise of +-60, so that the parse holds words and the commit node moves.  Per prefix
        length P in (500, 2000) and push size n in (10, 100): R times a push of n frames per channel and a commit of every
        channel behind it, each call between two device events of its own; the session is ended and refilled to P by untimed
        pushes and one commit before each timed window.  commit_vs_push = median commit / median push.  After the last window
        the last commit's counts are held against the end call's rows (no more words than the parse, no frame past N).  One
        line of JSON.
    python profiles/experiments/onepass_commit_rate.py --ab ab_libs/base.so ab_libs/new.so [--rounds N]
        the push alone under two builds of the library (profiles/experiments/ab_build.sh), each in a child process of its own,
        alternating, on one box: ms per push for the same P and n.  A line of JSON per child.
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
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    maxf = max(PREFIXES) + R * max(PUSHES)
    host_rows = np.zeros((Cn, maxf + M, 12), np.int16)
    for c in range(Cn):
        at = 0
        while at < maxf:
            k = int(rng.integers(0, K))
            host_rows[c, at:at + tf[k]] = tm[k, :tf[k]]
            at += int(tf[k])
    host_rows = (host_rows[:, :maxf] + rng.integers(-60, 61, (Cn, maxf, 12))).astype(np.int16)
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    rows = torch.from_numpy(host_rows).to(dev)
    ses = eng.decode_onepass_live(Cn, max(PUSHES), maxf, WORDS_CAP, False, SKIP)
    res = {"channels": Cn, "K": K, "tpl_rows_max": M, "W": 2 * M - 1, "words_cap": WORDS_CAP, "reps": R, "rounds": a.rounds, "commit": not a.push_only}

    def refill(P):
        ses.end(np.arange(Cn))
        for lo in range(0, P, max(PUSHES)):
            ses.push_dev(rows[:, lo:min(lo + max(PUSHES), P)].contiguous())
        if not a.push_only:
            ses.commit_dev()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        return (e0, e1), out

    last = None
    for P in PREFIXES:
        for n in PUSHES:
            r = res[f"P{P}_n{n}"] = {"push_ms": [], "commit_ms": []}
            chunks = [rows[:, P + i * n:P + (i + 1) * n].contiguous() for i in range(R)]
            for _ in range(a.rounds):
                refill(P)
                torch.cuda.synchronize()
                ev, new = {"push_ms": [], "commit_ms": []}, 0
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
            if not a.push_only:
                r["commit_vs_push"] = round(r["median_ms"]["commit"] / r["median_ms"]["push"], 4)
                r["n_committed_mean"] = round(float(last["crec"][:, 0].float().mean().item()), 2)
    if not a.push_only:
        crec = last["crec"].cpu().numpy()
        end = ses.end(np.arange(Cn))
        res["committed_le_parsed"] = bool(np.all(crec[:, 0] <= end["rec"]["n_words"]))
        res["frames_le_N"] = bool(np.all(crec[:, 3] <= end["rows"]["frames"]))
    ses.close()
    print(json.dumps(res), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--push-only", action="store_true", help="time the pushes alone (what --ab runs under each library)")
    ap.add_argument("--ab", nargs=2, metavar="LIB")
    a = ap.parse_args()
    if not a.ab:
        return run(a)
    for _ in range(a.rounds):
        for lib in a.ab:
            env = dict(os.environ, SR_ENGINE_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, __file__, "--push-only", "--rounds", "1", "--channels", str(a.channels), "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=300)
            print(os.path.basename(lib), p.stdout.strip().splitlines()[-1] if p.stdout.strip() else p.stderr[-600:], flush=True)


if __name__ == "__main__":
    main()
