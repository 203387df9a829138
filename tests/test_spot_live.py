"""Live word spotting: the spotter's state carried between pushes (include/sr_engine.h, "live word spotting").

The rule: whatever the chunking, a channel's window records are those of the one-shot definition (tests/spot_ref.py) for
everything pushed to it as ONE row.  tests/spot_live_ref.py restates the resumable recurrence; the CPU tests hold it to
spot_ref over random chunkings, the GPU tests compare whole records, rows, window labels and compact scores bit for bit.
Coefficients from -2..2 make a good share of the end cells depend on the tie rule, which is what absolute starts must keep.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import spot_live_ref as live
import spot_ref as ref
from guarded import guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, NBEST_DTYPE, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_spot_live_geometry", "sr_spot_live_open", "sr_spot_live_rows", "sr_spot_live_windows", "sr_spot_live_push_dev", "sr_spot_live_push",
         "sr_spot_live_push_pcm_dev", "sr_spot_live_push_pcm", "sr_spot_live_end")
BAD_ARG = 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
MAXF, FRAME_LEN, HOP = 119, 160, 80
SLOT_M = (1, 2, 7, 24, 65, 70)  # slot 3 is erased
C_N, N_FR, CHUNK_MAX = 3, 300, 100
WINS = (16, 50, 64)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = np.nonzero(np.any(g != w, 1))[0]
    if len(bad):
        at = np.unravel_index(int(bad[0]), want.shape)
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} records differ, first at (window, slot) {at}: "
                             f"got {g[bad[0]].tolist()} want {w[bad[0]].tolist()}")


# ---- CPU: the surface (fails without the feature) ----------------------------------------------------------------------------
def test_header_declares_the_live_spotting_api_and_libraries_export_it():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\b(int|uint32_t) %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert re.search(r"\bvoid sr_spot_live_close\s*\(", src) and hasattr(engine.load_library(), "sr_spot_live_close")
    assert src.index("sr_spot_geometry") < src.index("sr_spot_live_geometry") < src.index("sr_decode_words_dp_dev")  # after the spotter's section
    assert re.search(r"typedef struct sr_spot_win \{\s*uint32_t channel;\s*uint32_t window;\s*\} sr_spot_win;", src)
    assert engine.SPOT_WIN_DTYPE == live.SPOT_WIN_DTYPE and engine.SPOT_WIN_DTYPE.itemsize == 8 and engine.SPOT_DTYPE.itemsize == 16
    assert callable(getattr(Engine, "spot_live", None)) and callable(engine.spot_live_geometry)
    for meth in ("rows", "push", "push_dev", "push_pcm", "push_pcm_dev", "end", "close"):
        assert callable(getattr(engine.SpotSession, meth, None)), meth


# ---- CPU: the design -----------------------------------------------------------------------------------------------------------
def random_chunking(rng, N, hi):
    """sizes 0..hi that sum to N, zeros and ones included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(0, hi + 1))])), N - sum(out)))
    return out


def test_resumed_recurrence_equals_the_whole_row_over_random_chunkings():
    rng = np.random.default_rng(21)
    shapes = [(80, 24, 2)] + [(int(rng.integers(1, 81)), int(rng.integers(1, 25)), 2) for _ in range(39)]
    shapes += [(80, 24, 3000), (64, 7, 3000), (33, 1, 3000), (65, 23, 3000)]
    cells = tie_cells = 0
    sizes = set()
    for N, M, amp in shapes:
        d = ref.local_dis(rng.integers(-amp, amp + 1, (N, 12)), rng.integers(-amp, amp + 1, (M, 12)))
        cost, start = ref.dp_end_row(d)
        whole = np.where(cost >= 0, (cost.astype(np.uint64) << np.uint64(32)) | start.astype(np.uint64), live.INF64)
        for hi in (None, 1, 7, N):  # all at once; zeros and ones; small sizes; any size 0..N
            chunks = [N] if hi is None else random_chunking(rng, N, hi)
            assert sum(chunks) == N and (hi != 1 or set(chunks) <= {0, 1})
            state, got, at = None, [], 0
            for n in chunks:
                end, state = live.resume(d[at:at + n], state)
                got.append(end)
                at += n
            got = np.concatenate(got)
            assert np.array_equal(got, whole), (N, M, amp, hi)
            assert state[2] == N
            sizes.update(chunks)
        for win in (1, 5, 16, N, N + 3):  # the windows built from it are spot_ref's
            q = ref.end_scores(cost, start, M)
            want = np.array([ref.window_hit(cost, start, q, w * win, (w + 1) * win) for w in range(-(-N // win))], ref.SPOT_DTYPE)
            same(live.end_records(got, M, win), want, (N, M, win))
        if amp == 2 and M > 1:  # how much of this depends on the tie rule: end cells whose start differs when ties go the other way
            rev = _end_row_largest_start(d)
            ok = cost >= 0
            cells += int(ok.sum())
            tie_cells += int((rev[ok] != start[ok]).sum())
    assert cells > 200 and tie_cells * 10 > cells, (tie_cells, cells)
    assert {0, 1, 80} <= sizes and len([v for v in sizes if 8 <= v < 80]) >= 15, sorted(sizes)  # sizes 0..N reached resume()


def _end_row_largest_start(d):
    """the end row's starts with the tie rule reversed (largest start among equal costs): resume() on states whose low word
    holds ~start"""
    N, M = d.shape
    pd, pm = np.full(M, live.INF64, np.uint64), np.full(M, live.INF64, np.uint64)
    out = np.zeros(N, np.int64)
    for x in range(N):
        add = d[x].astype(np.uint64) << np.uint64(32)
        cd = np.full(M, live.INF64, np.uint64)
        cd[1:] = live._plus(pm[:-1], add[1:])
        cn = np.empty(M, np.uint64)
        cn[0] = add[0] | np.uint64(0xFFFFFFFF - x)
        cn[1:] = live._plus(np.minimum(pd[1:], cd[:-1]), add[1:])
        pd, pm = cd, np.minimum(cd, cn)
        out[x] = 0xFFFFFFFF - int(pm[M - 1] & np.uint64(0xFFFFFFFF))
    return out


def test_window_records_of_a_long_recording_are_spot_hits_of_one_row():
    rng = np.random.default_rng(22)
    tm, tf = rng.integers(-2, 3, (3, 11, 12)).astype(np.int16), np.array([10, 3, 1], np.uint32)
    valid = np.array([1, 0, 1], np.uint8)
    feat = rng.integers(-2, 3, (57, 12)).astype(np.int16)
    for win in (1, 8, 57, 100):
        want = ref.spot_hits(feat[None], [57], tm, tf, valid, 57, win)[0]
        same(live.window_records(feat, tm, tf, valid, win), want[:-(-57 // win)], win)


# ---- CPU: geometry ---------------------------------------------------------------------------------------------------------------
def test_geometry_and_row_counts_follow_their_definitions():
    cap = engine.spot_geometry(10, 119)["max_tpl_rows"]
    rng = np.random.default_rng(23)
    for W in (1, 2, 16, 50, 64, 119, 1000):
        for chunk in (1, 10, 63, 64, 65, 119, 5000):
            g = engine.spot_live_geometry(70, 6, chunk, W)
            assert g["state_bytes"] == 6 * (70 * 16 + 32) and g["max_tpl_rows"] == cap
            per_entry = [len(live.push_windows([b], [chunk], W)) for b in (0, W // 2, W - 1, W, 3 * W + 1)]
            assert g["max_windows"] == -(-chunk // W) == max(per_entry) == per_entry[2], (W, chunk)  # entering on a window's last frame
            before, new = rng.integers(0, 3 * W + 5, 9), rng.integers(0, chunk + 1, 9)
            rows = live.push_windows(before, new, W)
            assert engine.spot_live_windows(W, before, new) == len(rows), (W, chunk)  # the library's count, what sr_spot_live_rows sums
            assert len(rows) == sum((int(b) + int(n)) // W - int(b) // W for b, n in zip(before, new)) and rows == sorted(rows)
    assert engine.spot_live_geometry(16383, 65536, 1, 1)["state_bytes"] == 0xFFFFFFFF  # saturates
    L = engine.load_library()
    out = (U32 * 3)()
    for bad in ((0, 1, 1, 1), (16384, 1, 1, 1), (10, 0, 1, 1), (10, 1, 0, 1), (10, 1, 1, 0)):
        assert L.sr_spot_live_geometry(*(U32(v) for v in bad), out) == BAD_ARG, bad
    assert L.sr_spot_live_geometry(U32(10), U32(1), U32(1), U32(1), None) == BAD_ARG
    assert engine.spot_live_windows(16, [0xFFFF0000 - 5, 3], [5, 100]) == 1 + 6     # up to the frame limit ...
    assert engine.spot_live_windows(16, [0xFFFF0000 - 5, 3], [6, 100]) == 0         # ... and not past it
    L.sr_spot_live_windows.restype = U32
    assert L.sr_spot_live_windows(U32(0), engine._vp(np.zeros(1, np.uint32)), engine._vp(np.ones(1, np.uint32)), U32(1)) == 0
    assert L.sr_spot_live_windows(U32(4), None, None, U32(1)) == 0
    L.sr_spot_live_rows.restype = U32
    assert L.sr_spot_live_rows(None, None, U32(5)) == 0
    assert live.pcm_frames(160, 160, 80) == 0 and live.pcm_frames(161, 160, 80) == 1 and live.pcm_frames(241, 160, 80) == 2


def test_host_mirror_runs_clean_under_the_sanitizers(tmp_path):
    """windows and row bases of a push, PCM framing and its agreement with the decoders' plan, refusal order, the flush list of
    csrc/sr_spot_live_plan.h against values worked out by hand: a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "spot_live_plan", "plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)


# ---- GPU: fixtures -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store():
    rng = np.random.default_rng(500)
    K = len(SLOT_M)
    tf, valid = np.array(SLOT_M, np.uint32), np.ones(K, np.uint8)
    valid[3] = 0
    tm = np.zeros((K, max(SLOT_M) + 1, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-2, 3, (tf[k], 12))
    for a in (tm, tf, valid):
        a.setflags(write=False)
    return tm, tf, valid


@functools.lru_cache(maxsize=None)
def feats(amp):
    rng = np.random.default_rng(600 + amp)
    f = rng.integers(-amp, amp + 1, (C_N, N_FR, 12)).astype(np.int16)
    f[1, 100:165] = store()[0][4, :65]  # a template inside channel 1, across window edges
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want(amp, win, n_frames=N_FR):
    """per channel SPOT_DTYPE [ceil(n_frames / win), K]: the records of the channel's first n_frames frames as one row"""
    tm, tf, valid = store()
    out = [live.window_records(feats(amp)[c, :n_frames], tm, tf, valid, win) for c in range(C_N)]
    for a in out:
        a.setflags(write=False)
    return out


def make_engine(**kw):
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(*store())
    return eng


class Collector:
    """feeds a session push by push and files every emitted row under its (channel, window); every push is checked against what
    the counts alone say: n_rows, the window labels and their order, compact scores = the dis fields"""

    def __init__(self, ses, n_channels, win):
        self.ses, self.win = ses, win
        self.count = [0] * n_channels
        self.recs = [dict() for _ in range(n_channels)]

    def take(self, out, new):
        exp = live.push_windows(self.count, new, self.win)
        assert out["n_rows"] == len(exp) and [(int(w["channel"]), int(w["window"])) for w in out["wins"]] == exp, (out["wins"], exp)
        hits = out["hits"]
        if not isinstance(hits, np.ndarray):
            torch.cuda.synchronize()
            hits = hits.cpu().numpy().view(ref.SPOT_DTYPE).reshape(len(exp), hits.shape[1])
            sc = out["scores"].cpu().numpy().view(np.uint32)
        else:
            sc = out["scores"]
        assert np.array_equal(sc, hits["dis"])
        for r, (c, w) in enumerate(exp):
            assert w not in self.recs[c], "a window emitted twice"
            self.recs[c][w] = hits[r].copy()
        self.count = [a + int(b) for a, b in zip(self.count, new)]

    def end(self, channels):
        out = self.ses.end(channels)
        exp = [(c, self.count[c] // self.win) for c in channels if self.count[c] % self.win]
        assert out["n_rows"] == len(exp) and [(int(w["channel"]), int(w["window"])) for w in out["wins"]] == exp
        for r, (c, w) in enumerate(exp):
            assert w not in self.recs[c]
            self.recs[c][w] = out["hits"][r].copy()
        for c in channels:
            self.count[c] = 0

    def channel(self, c):
        n = len(self.recs[c])
        assert sorted(self.recs[c]) == list(range(n)), sorted(self.recs[c])
        return np.array([self.recs[c][w] for w in range(n)], ref.SPOT_DTYPE).reshape(n, -1)


def feed(eng, f, schedule, win, form="dev", chunk_max=CHUNK_MAX, end=True):
    """f int16 [C, N, 12]; schedule: per push the counts [C] -> the Collector after every push (and the end of every channel)"""
    n_ch = len(f)
    ses = eng.spot_live(n_ch, chunk_max, win)
    col = Collector(ses, n_ch, win)
    d_f = torch.from_numpy(np.array(f)).cuda()
    at = [0] * n_ch
    for cnt in schedule:
        F = max(max(cnt), 1)
        assert ses.rows(np.array(cnt, np.uint32)) == len(live.push_windows(col.count, cnt, win))
        if form == "dev":
            chunk = torch.full((n_ch, F, 12), 0x7FFF, dtype=torch.int16, device="cuda:0")  # poison past n[c]
            for c in range(n_ch):
                chunk[c, :cnt[c]] = d_f[c, at[c]:at[c] + cnt[c]]
            out = ses.push_dev(chunk, np.array(cnt, np.uint32))
        else:
            chunk = np.zeros((n_ch, F, 12), np.int16)
            for c in range(n_ch):
                chunk[c, :cnt[c]] = f[c, at[c]:at[c] + cnt[c]]
            out = ses.push(poison_feature_rows(chunk, cnt), np.array(cnt, np.uint32))
        col.take(out, cnt)
        at = [a + b for a, b in zip(at, cnt)]
    assert at == [f.shape[1]] * n_ch or not end
    if end:
        col.end(list(range(n_ch)))
        ses.close()
    return col if end else (col, ses)


def uniform(sizes, n_ch=C_N):
    return [[s] * n_ch for s in sizes]


def cut(N, sizes):
    """the sizes in rotation until N frames are used up"""
    out, i = [], 0
    while sum(out) < N:
        out.append(min(sizes[i % len(sizes)], N - sum(out)))
        i += 1
    return out


def per_channel(lists):
    """one chunking per channel -> per push the counts (0 once a channel is done)"""
    n = max(len(x) for x in lists)
    return [[x[i] if i < len(x) else 0 for x in lists] for i in range(n)]


def chunkings(N=N_FR):
    rng = np.random.default_rng(700)
    rand = lambda: random_chunking(rng, N, CHUNK_MAX)  # noqa: E731
    return {"at once": uniform(cut(N, [CHUNK_MAX])),
            "one frame": uniform([1] * N),
            "63/64/65": uniform(cut(N, [63, 64, 65])),
            "random": uniform(rand()),
            "per channel": per_channel([cut(N, [CHUNK_MAX]), rand(), cut(N, [65, 1, 64, 0, 63])])}


# ---- GPU 1: chunking invariance ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("win", WINS)
def test_every_chunking_gives_the_records_of_the_whole_recording(win):
    """300 frames per channel against an engine whose max_frames is 119: the one-shot spotter's cap does not apply"""
    assert N_FR > MAXF
    eng = make_engine()
    exp = want(2, win)
    assert exp[1][164 // win, 4]["dis"] == 0 and 95 <= exp[1][164 // win, 4]["start"] <= 105  # the planted template, absolute start
    assert all(np.all(e[:, 3]["dis"] == DIS_ERR) for e in exp)                           # the erased slot
    for name, sched in chunkings().items():
        col = feed(eng, feats(2), sched, win, "host" if name == "random" else "dev")
        for c in range(C_N):
            same(col.channel(c), exp[c], f"win {win}, chunking '{name}', channel {c}")
    eng.close()


# ---- GPU 2: equality with the one-shot spotter while it applies ---------------------------------------------------------------
@pytest.mark.gpu
def test_equals_the_one_shot_spotter_up_to_max_frames():
    eng = make_engine()
    f = feats(2)[:, :MAXF]
    for win in WINS:
        hits, _ = eng.spot(np.ascontiguousarray(f), np.full(C_N, MAXF, np.uint32), win)
        assert hits.shape[1] == -(-MAXF // win)
        col = feed(eng, f, uniform(cut(MAXF, [40, 1, 64])), win)
        for c in range(C_N):
            same(col.channel(c), hits[c], f"win {win}, channel {c}")
            same(col.channel(c), want(2, win, MAXF)[c], f"reference, win {win}, channel {c}")
    eng.close()


# ---- GPU 3: end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_emits_the_open_window_and_leaves_the_channel_fresh():
    eng, win, f = make_engine(), 50, feats(2)
    col, ses = feed(eng, f[:, :130], uniform(cut(130, [64])), win, end=False)
    assert ses.end([])["n_rows"] == 0
    col.end([1])  # 130 % 50 != 0: window 2 of channel 1, 30 frames of it
    same(col.channel(1), live.window_records(f[1, :130], *store(), win), "ended channel")
    # channel 1 again from frame 0 (the same frames give the same records from window 0); channels 0 and 2 go on
    first = col.channel(1)
    col.recs[1] = {}
    d_f = torch.from_numpy(np.array(f)).cuda()
    chunk = torch.stack([d_f[0, 130:200], d_f[1, 0:70], d_f[2, 130:200]])
    col.take(ses.push_dev(chunk), [70, 70, 70])
    chunk = torch.stack([d_f[0, 200:230], d_f[1, 70:100], d_f[2, 200:230]])
    col.take(ses.push_dev(chunk), [30, 30, 30])
    col.end([0, 1, 2])  # channel 1 stands at 100 = 2 * 50: nothing open; the others at 230
    same(col.channel(1), first[:2], "restarted channel")
    for c in (0, 2):
        same(col.channel(c), live.window_records(f[c, :230], *store(), win), f"channel {c}")
    assert ses.end([0, 1, 2, 1])["n_rows"] == 0  # all fresh
    ses.close()
    eng.close()


@pytest.mark.gpu
def test_a_channel_listed_twice_in_end_counts_once():
    """K = 300 slots: the flush kernel's threads of two list entries would sit in different workgroups, so a second entry for
    the same channel must never reach the device (its reset could overtake the first entry's read of the carry)"""
    rng = np.random.default_rng(950)
    K, n_ch, N, win = 300, 2, 20, 16
    tm, tf = np.zeros((K, 3, 12), np.int16), np.full(K, 2, np.uint32)
    tm[:, :2] = rng.integers(-2, 3, (K, 2, 12))
    f = rng.integers(-2, 3, (n_ch, N, 12)).astype(np.int16)
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(tm, tf)
    exp = [live.window_records(f[c], tm, tf, None, win) for c in range(n_ch)]
    assert all(np.all(e[1]["dis"] != DIS_ERR) for e in exp)  # the open window has a hit in every slot
    ses = eng.spot_live(n_ch, N, win)
    for _ in range(3):
        out = ses.push_dev(torch.from_numpy(f).cuda())
        assert out["n_rows"] == n_ch
        end = ses.end([1, 1, 0, 1, 0])
        assert end["n_rows"] == 2 and [(int(w["channel"]), int(w["window"])) for w in end["wins"]] == [(1, 1), (0, 1)]
        same(end["hits"][0], exp[1][1], "channel 1, listed three times")
        same(end["hits"][1], exp[0][1], "channel 0, listed twice")
    ses.close()
    eng.close()


@pytest.mark.gpu
def test_pushes_on_different_streams_and_host_pushes_are_ordered():
    """no synchronisation between the pushes: each runs behind the last one's event, whatever stream it is on"""
    eng, win, f = make_engine(), 16, feats(2)
    ses = eng.spot_live(C_N, CHUNK_MAX, win)
    col = Collector(ses, C_N, win)
    d_f = torch.from_numpy(np.array(f)).cuda()
    sizes = cut(N_FR, [7, 64, 1, 33, 100])
    edges = np.concatenate([[0], np.cumsum(sizes)])
    chunks = [d_f[:, a:b].contiguous() for a, b in zip(edges[:-1], edges[1:])]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    outs = []
    for i, (n, chunk) in enumerate(zip(sizes, chunks)):
        st = streams[i % 3]
        outs.append(ses.push_dev(chunk, stream=st) if st is not None else ses.push(np.array(f[:, edges[i]:edges[i + 1]])))
    torch.cuda.synchronize()
    for n, out in zip(sizes, outs):
        col.take(out, [n] * C_N)
    col.end([0, 1, 2])
    for c in range(C_N):
        same(col.channel(c), want(2, win)[c], f"channel {c}")
    ses.close()
    eng.close()


# ---- GPU 4: PCM sessions ---------------------------------------------------------------------------------------------------------
def feed_pcm(eng, X, mid, schedule, win, chunk_max, dev):
    ses = eng.spot_live(len(X), chunk_max, win, mid)
    frames = lambda r: [live.pcm_frames(v, FRAME_LEN, HOP) for v in r]  # noqa: E731
    col, got = Collector(ses, len(X), win), [0] * len(X)
    for cnt in schedule:
        S = (max(max(cnt), 1) + 7) // 8 * 8
        chunk = np.full((len(X), S), 4095, np.uint16)  # poison past n[c]
        for c in range(len(X)):
            chunk[c, :cnt[c]] = X[c, got[c]:got[c] + cnt[c]]
        new = [a - b for a, b in zip(frames([g + n for g, n in zip(got, cnt)]), frames(got))]
        assert ses.rows(np.array(cnt, np.uint32)) == len(live.push_windows(col.count, new, win))
        if dev:
            out = ses.push_pcm_dev(torch.from_numpy(chunk.view(np.int16)).cuda(), np.array(cnt, np.uint32))
        else:
            out = ses.push_pcm(chunk, np.array(cnt, np.uint32))
        col.take(out, new)
        got = [g + n for g, n in zip(got, cnt)]
    assert got == [X.shape[1]] * len(X)
    col.end(list(range(len(X))))
    ses.close()
    return col


@pytest.mark.gpu
def test_pcm_sessions_frame_the_samples_as_the_whole_path_does():
    rng = np.random.default_rng(800)
    eng = Engine(max_frames=MAXF, device=0)
    R1 = 1 + (MAXF - 1) * HOP + FRAME_LEN + 37  # 119 frames and a remainder
    X = (2048 + 600 * np.sin(np.arange(3 * R1)[None] * np.array([[0.05], [0.11]])) + rng.integers(-300, 301, (2, 3 * R1))).astype(np.uint16)
    mid = np.array([2048, 2040], np.uint32)
    n, mf = eng.mfcc(X[:, :R1], [1, 1], [R1, R1], mid)
    assert list(n) == [MAXF, MAXF]
    tm, tf, valid = np.zeros((6, 71, 12), np.int16), np.array(SLOT_M, np.uint32), np.array([1, 1, 1, 0, 1, 1], np.uint8)
    for k, (c, at) in enumerate(((0, 5), (1, 20), (0, 33), (1, 0), (1, 40), (0, 10))):
        tm[k, :tf[k]] = mf[c, at:at + tf[k]]
    eng.set_templates_dense(tm, tf, valid)
    win, chunk_max = 50, 400
    sched = uniform([1] * 400, 2) + per_channel([cut(R1 - 400, [HOP - 1, HOP, FRAME_LEN, 400, 0, 237]), random_chunking(rng, R1 - 400, chunk_max)])
    o = eng.spot_pcm(X[:, :R1], [1, 1], [R1, R1], mid, win)
    assert o["hits"][0, 0, 0]["dis"] == 0 and o["hits"][1, 2, 4]["dis"] == 0  # the pieces are found
    for dev in (True, False):
        col = feed_pcm(eng, X[:, :R1], mid, sched if dev else per_channel([cut(R1, [400, 399, 1]), cut(R1, [161, 80])]), win, chunk_max, dev)
        for c in range(2):
            same(col.channel(c), o["hits"][c], f"dev {dev}, channel {c}")
    # three times as long: past the whole path's cap; the frames piece by piece, the records from the reference
    R3 = 3 * R1
    nf = live.pcm_frames(R3, FRAME_LEN, HOP)
    assert nf > 3 * MAXF
    pieces = []
    for p in range(0, nf, MAXF):
        cnt = min(MAXF, nf - p)
        s, e = 1 + p * HOP, 1 + p * HOP + (cnt - 1) * HOP + FRAME_LEN
        n, m = eng.mfcc(X, [s, s], [e, e], mid)
        assert list(n) == [cnt, cnt]
        pieces.append(m[:, :cnt])
    allf = np.concatenate(pieces, 1)
    col = feed_pcm(eng, X, mid, per_channel([random_chunking(rng, R3, chunk_max), cut(R3, [400, 81, 0, 159])]), win, chunk_max, True)
    for c in range(2):
        same(col.channel(c), live.window_records(allf[c], tm, tf, valid, win), f"long recording, channel {c}")
    eng.close()


# ---- GPU 5: contracts ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", (0xA5, 0x3C))
def test_guards_refusals_and_twin_sessions(canary):
    eng, win, f = make_engine(), 16, feats(2)
    K = len(SLOT_M)
    exp = want(2, win)
    ses, twin = eng.spot_live(C_N, CHUNK_MAX, win), eng.spot_live(C_N, CHUNK_MAX, win)
    col = Collector(ses, C_N, win)
    sid = torch.cuda.current_stream().cuda_stream
    L = eng.L
    at = [0] * C_N
    tm, tf, valid = store()

    def push(cnt, max_rows, ok=True, to=ses):
        F = max(max(cnt), 1)
        chunk = np.zeros((C_N, F, 12), np.int16)
        for c in range(C_N):
            chunk[c, :min(cnt[c], N_FR - at[c])] = f[c, at[c]:at[c] + cnt[c]]
        d_chunk = torch.from_numpy(poison_feature_rows(chunk, np.minimum(cnt, F))).cuda()
        g_h = guarded_out((max_rows, K), ref.SPOT_DTYPE, canary, 4096, "cuda:0", "hits")
        g_s = guarded_out((max_rows, K), np.uint32, canary, 4096, "cuda:0", "scores")
        wins, n = np.full(max_rows + 1, 0x5A5A5A5A, np.uint32).repeat(2).view(live.SPOT_WIN_DTYPE), U32(0xDEAD)
        ct = np.array(cnt, np.uint32)
        rc = L.sr_spot_live_push_dev(to.l, P(d_chunk.data_ptr()), U64(F * 12), engine._vp(ct), U32(0), U32(max_rows), P(g_h.ptr), P(g_s.ptr),
                                     engine._vp(wins), C.byref(n), P(sid))
        torch.cuda.synchronize()
        if not ok:
            assert rc == BAD_ARG and n.value == 0xDEAD and np.all(wins.view(np.uint32) == 0x5A5A5A5A), (rc, cnt)
            g_h.check_untouched()
            g_s.check_untouched()
            return None
        assert rc == 0, L.sr_last_error()
        g_h.check()
        g_s.check()
        hits, sc = g_h.interior(), g_s.interior()
        raw_h, raw_s = hits.view(np.uint8).reshape(max_rows, -1), sc.view(np.uint8).reshape(max_rows, -1)
        assert np.all(raw_h[n.value:] == canary) and np.all(raw_s[n.value:] == canary)       # rows >= *n_rows stay untouched
        assert np.all(wins.view(np.uint32)[2 * n.value:] == 0x5A5A5A5A)
        return dict(hits=hits[:n.value], scores=sc[:n.value], wins=wins[:n.value], n_rows=n.value)

    def both(cnt):
        rows = ses.rows(np.array(cnt, np.uint32))
        a, b = push(cnt, rows + 3), push(cnt, rows + 3, to=twin)
        assert a["hits"].tobytes() == b["hits"].tobytes() and a["scores"].tobytes() == b["scores"].tobytes()  # two sessions, identical bytes
        col.take(a, cnt)
        for c in range(C_N):
            at[c] += cnt[c]

    both([40, 17, 0])
    rows = ses.rows(np.array([64, 64, 64], np.uint32))
    assert rows == 12 and push([64, 64, 64], rows - 1, ok=False) is None           # max_rows too small
    assert b"max_rows" in L.sr_last_error()
    assert push([CHUNK_MAX + 1, 1, 1], 64, ok=False) is None and ses.rows(np.array([CHUNK_MAX + 1, 1, 1], np.uint32)) == 0
    both([64, 64, 64])
    eng.set_templates_dense(tm, tf, valid)                                         # the same rows, but a new store
    assert push([10, 0, 0], 8, ok=False) is None and b"store changed" in L.sr_last_error()
    assert push([0, 0, 0], 8)["n_rows"] == 0                                       # nothing pushed, nothing refused
    # the refused pushes changed nothing: ended here, the records are those of the frames that were accepted
    done = list(at)
    assert done == [104, 81, 64] and ses.end([0, 1, 2])["n_rows"] == 0  # the open window of a channel whose store was replaced is dropped
    col.count = [0] * C_N
    for c in range(C_N):
        same(col.channel(c), exp[c][:done[c] // win], f"closed windows, channel {c}")
    # bound to the new store now: the whole recording again
    col.recs = [dict() for _ in range(C_N)]
    for c in range(C_N):
        at[c] = 0
    twin.end([0, 1, 2])
    for cnt in cut(N_FR, [100, 99, 1]):
        both([cnt] * C_N)
    col.end([0, 1, 2])
    for c in range(C_N):
        same(col.channel(c), exp[c], f"after the refusals, channel {c}")
    ses.close()
    twin.close()
    eng.close()


# ---- GPU 6: N-best over the compact scores ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nbest_over_the_compact_scores_of_a_push():
    eng, win, f = make_engine(), 16, feats(2)
    eng.set_word_map(np.array([5, 9, 5, 5, 9, 7], np.uint32))
    ses = eng.spot_live(C_N, CHUNK_MAX, win)  # (opened after the map: setting a map leaves the store alone)
    out = ses.push_dev(torch.from_numpy(np.array(f[:, :CHUNK_MAX])).cuda())
    assert out["n_rows"] == C_N * (CHUNK_MAX // win) and out["scores"].is_contiguous()
    d_nb, d_nm = eng.nbest_dev(out["scores"], 2)
    torch.cuda.synchronize()
    rows = np.array([want(2, win)[int(w["channel"])][int(w["window"])]["dis"] for w in out["wins"]], np.uint32)
    nb, nm = eng.nbest(rows, 2)
    assert engine.nbest_from_torch(d_nb).tobytes() == nb.tobytes() and np.array_equal(d_nm.cpu().numpy().view(np.uint32), nm)
    assert nb.dtype == NBEST_DTYPE and (nm > 0).sum() >= 10
    ses.close()
    eng.close()


# ---- GPU 7: amplitude ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_amplitude_with_wrapping_distances():
    tm, tf, valid = store()
    big = np.array(tm)
    big[5, :70] = np.random.default_rng(900).integers(-30000, 30001, (70, 12))  # squared differences that wrap u32
    f = feats(3000).copy()
    f[2, 200:270] = -big[5, :70]
    d2 = ((f[2, 200:270].astype(np.int64) - big[5, :70]) ** 2).sum(1)
    assert d2.max() >= 2 ** 32
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(big, tf, valid)
    col = feed(eng, f, chunkings()["random"], 50)
    for c in range(C_N):
        same(col.channel(c), live.window_records(f[c], big, tf, valid, 50), f"channel {c}")
    eng.close()
