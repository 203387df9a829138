"""Live sessions (sr_live_push_dev) at 100 ms pushes: per-push time and audio seconds per wall second, against what a caller
has to do without sessions.

    python profiles/experiments/live_rate.py [--channels 1,1024,65536] [--pushes 200] [--window-calls 20]
        Per channel count C: a session of C channels, chunk_max 800; synthetic speech (one generated recording, every channel
        at its own offset into it behind a common quiet noise head), 80 templates x 119 frames.  After 40 warm-up pushes (the
        noise heads complete in push 3) `--pushes` pushes of 800 samples, each timed with a host clock around the push and a
        device synchronise; the whole timed run twice (the spread).  Then the comparison point: sr_recognize_stream_dev over a
        sliding window of one ring length per channel (sr_live_geometry), thresholds handed in, once per 100 ms, `--window-calls`
        calls timed the same way.  One line of JSON: median / min / max push time, audio seconds per wall second
        (C * 0.1 s / median push time), the same for the sliding window, and their ratio.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/experiments/live_rate.py --trace [--channels C]
        The run to trace for the kernel shares (tracing only, the program after --): warm-up, then 50 pushes.

The chunks are built on the device outside the timed interval; a push is timed from the call to the end of its last kernel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

CHUNK, FS, WARMUP = 800, 8000, 40


def setup(C):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from stm32_speech_recognition_amd import Engine, synth
    from stm32_speech_recognition_amd.engine import ATAP_DTYPE, live_geometry
    dev = torch.device("cuda", 0)
    eng = Engine(max_frames=119, device=0)
    rng = np.random.default_rng(2027)
    K, R = 80, 119
    tm = np.zeros((K, R + 1, 12), np.int16)
    tm[:, :R] = rng.integers(-900, 900, (K, R, 12))
    eng.set_templates_dense(tm, np.full(K, R, np.uint32))
    bank = synth.word_bank(12)
    nw = 200  # 60 s: words of 12..100 frames, 1 600 quiet samples between them
    base = synth.as_u16_numpy(synth.make_multiword(list(rng.integers(0, 12, nw)), list(rng.integers(12, 100, nw)), 7, bank,
                                                   S=60 * FS, gap=1600, gain=2.0))
    head = synth.NOISE_LEN
    vd = eng.vad(base[None, :16000])
    atap = np.zeros(C, ATAP_DTYPE)
    for f in ATAP_DTYPE.names:
        atap[f] = vd[0][f]
    base_d = torch.from_numpy(base.view(np.int16)).to(dev)
    off = torch.from_numpy(rng.integers(0, len(base) - head, C)).to(dev)
    ar = torch.arange(CHUNK, device=dev)

    def chunk(k):  # [C, 800]: the common head first, then every channel's own place in the recording
        p = k * CHUNK + ar
        idx = torch.where(p[None, :] < head, p[None, :].expand(C, -1), head + (off[:, None] + p[None, :]) % (len(base) - head))
        return base_d[idx].contiguous()

    ring = live_geometry(CHUNK)[0]
    return torch, eng, chunk, atap, ring, dev


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms, C):
    med = float(np.median(ms))
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "audio_s_per_wall_s": round(C * CHUNK / FS / (med / 1e3), 1)}


def run_one(C, a):
    torch, eng, chunk, atap, ring, dev = setup(C)
    res = {"C": C, "ring": ring, "live": [], "records": 0}
    for rep in range(2):
        sess = eng.live(C, CHUNK)
        k, ms, total = 0, [], 0
        for _ in range(WARMUP):
            sess.push_dev(chunk(k))
            k += 1
        for _ in range(a.pushes):
            x = chunk(k)
            out = {}
            ms.append(timed(torch, lambda: out.update(sess.push_dev(x, n_best=None))))
            total += int(out["count"][0])
            k += 1
        sess.close()
        res["live"].append(stats(ms, C))
        res["records"] = total
    # the comparison point: a sliding window of one ring length, re-scanned and re-recognised every 100 ms
    win = torch.cat([chunk(k) for k in range(WARMUP, WARMUP + (ring + CHUNK - 1) // CHUNK)], 1)[:, :ring // 8 * 8].contiguous()
    at = torch.from_numpy(atap.view(np.uint8).reshape(C, 12).view(np.int32).copy()).to(dev)
    max_segs = 3 * C  # a window of 1.45 s holds at most 8 END events, in speech about 1.5
    k0, ms, total = WARMUP + (ring + CHUNK - 1) // CHUNK, [], 0
    for i in range(a.window_calls + 2):
        win = torch.cat([win[:, CHUNK:], chunk(k0 + i)], 1).contiguous()
        out = {}
        t = timed(torch, lambda: out.update(eng.recognize_stream_dev(win, max_segs, atap=at)))
        if i >= 2:
            ms.append(t)
            total += int(out["seg_offsets"][-1])
    res["window"] = stats(ms, C)
    res["window_records_per_call"] = total // max(1, a.window_calls)
    res["ratio"] = round(res["window"]["median_ms"] / np.mean([r["median_ms"] for r in res["live"]]), 2)
    eng.close()
    return res


def run_trace(C):
    torch, eng, chunk, atap, ring, dev = setup(C)
    sess = eng.live(C, CHUNK)
    for k in range(WARMUP + 50):
        sess.push_dev(chunk(k))
    torch.cuda.synchronize()
    sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="1,1024,65536")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--window-calls", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    cs = [int(c) for c in a.channels.split(",")]
    if a.trace:
        return run_trace(cs[-1])
    print(json.dumps({"chunk": CHUNK, "pushes": a.pushes, "runs": [run_one(C, a) for C in cs]}), flush=True)


if __name__ == "__main__":
    main()
