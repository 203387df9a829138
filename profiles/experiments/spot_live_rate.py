"""Live word spotting (sr_spot_live_push_dev) against the stateless alternative a caller had before it.

    python profiles/experiments/spot_live_rate.py [--channels C] [--launches N]
        64 channels x 100 templates of 80..120 rows (random s16 features resident in HBM: the kernels' work does not depend
        on the values).  Per push size n in (10, 100):
          live       one sr_spot_live_push_dev of n frames per channel, windows of 50 end frames, the state on the device;
          stateless  one sr_spot_dp_batch_dev over rows that hold the last 2M - 2 + n frames (M = the longest template): what a
                     caller without the session re-runs on every push to get the same end frames.
        Same process, alternated three times, each timed with device events over N calls after a warm-up call; the host's
        wall time per call is reported next to it (a push is a 2 KiB plan upload and one launch: where the two agree the
        figure is the host's enqueue rate, not the kernel's time).  ratio = live / stateless beside the cell-count ratio
        n / (n + 2M - 2).  One (channel, slot) of a fresh session is compared with tests/spot_live_ref.py.  One line of JSON.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PUSHES = (10, 100)
WIN = 50


def timed(torch, fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, t_enq * 1e3 / n


def run(a):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spot_live_ref
    from stm32_speech_recognition_amd import Engine
    from stm32_speech_recognition_amd.engine import SPOT_DTYPE, SPOT_WIN_DTYPE, _vp
    dev = torch.device("cuda", 0)
    K, Cn = 100, a.channels
    rng = np.random.default_rng(2027)
    tf = rng.integers(80, 121, K).astype(np.uint32)
    tf[0] = 120
    M = int(tf.max())
    tm = np.zeros((K, M + 1, 12), np.int16)
    tm[:, :M] = rng.integers(-3000, 3001, (K, M, 12))
    hist = 2 * M - 2
    maxf = hist + max(PUSHES)
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    g = torch.Generator(device=dev).manual_seed(9)
    rows = torch.randint(-3000, 3001, (Cn, maxf, 12), generator=g, device=dev, dtype=torch.int16)
    sid = torch.cuda.current_stream().cuda_stream
    res = {"channels": Cn, "K": K, "tpl_rows_max": M, "history_frames": hist, "win_frames": WIN, "launches": a.launches}
    fns = {}
    for n in PUSHES:
        ses = eng.spot_live(Cn, n, WIN)
        max_rows = Cn * (-(-n // WIN))
        chunk = rows[:, :n].contiguous()
        hits = torch.empty(max_rows, K, 4, dtype=torch.int32, device=dev)
        sc = torch.empty(max_rows, K, dtype=torch.int32, device=dev)
        wins, n_rows = np.zeros(max_rows, SPOT_WIN_DTYPE), C.c_uint32(0)

        def live(ses=ses, chunk=chunk, hits=hits, sc=sc, wins=wins, n_rows=n_rows, n=n, max_rows=max_rows):
            rc = eng.L.sr_spot_live_push_dev(ses.l, _vp(chunk), C.c_uint64(n * 12), None, C.c_uint32(n), C.c_uint32(max_rows), _vp(hits),
                                             _vp(sc), _vp(wins), C.byref(n_rows), C.c_void_p(sid))
            assert rc == 0, eng.L.sr_last_error()

        frames = torch.full((Cn,), hist + n, dtype=torch.int32, device=dev)
        s_hits = torch.empty(Cn, 1, K, 4, dtype=torch.int32, device=dev)
        s_sc = torch.empty(Cn, 1, K, dtype=torch.int32, device=dev)
        fns[n] = (live, lambda frames=frames, s_hits=s_hits, s_sc=s_sc: eng.spot_dev(rows, frames, s_hits, s_sc, 0), ses)
        res[f"n{n}"] = {"live_ms": [], "live_host_ms": [], "stateless_ms": [], "stateless_host_ms": [],
                        "cell_ratio": round(n / (n + hist), 4)}
    for _ in range(3):
        for n in PUSHES:
            live, stateless, _ = fns[n]
            for name, fn in (("live", live), ("stateless", stateless)):
                ms, host = timed(torch, fn, a.launches)
                res[f"n{n}"][f"{name}_ms"].append(round(ms, 4))
                res[f"n{n}"][f"{name}_host_ms"].append(round(host, 4))
    for n in PUSHES:
        r = res[f"n{n}"]
        r["ratio"] = round(float(np.median(r["live_ms"])) / float(np.median(r["stateless_ms"])), 4)
        fns[n][2].close()
    # one (channel, slot) of a fresh session against the definition
    ses = eng.spot_live(Cn, 100, WIN)
    h_rows = rows[:, :250].cpu().numpy()
    got = []
    for lo, hi in ((0, 100), (100, 110), (110, 210), (210, 250)):
        o = ses.push_dev(rows[:, lo:hi].contiguous())
        torch.cuda.synchronize()
        hits = o["hits"].cpu().numpy().view(SPOT_DTYPE).reshape(o["n_rows"], K)
        got += [hits[r, 3] for r in range(o["n_rows"]) if o["wins"][r]["channel"] == Cn - 1]
    want = spot_live_ref.window_records(h_rows[Cn - 1], tm[3:4], tf[3:4], None, WIN)[:5, 0]
    res["sample_equals_definition"] = bool(np.array(got, SPOT_DTYPE).tobytes() == want.tobytes())
    ses.close()
    print(json.dumps(res), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--launches", type=int, default=2000)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
