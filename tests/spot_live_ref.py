"""Live word spotting (include/sr_engine.h, "live word spotting") restated in numpy: the spotter's two-state recurrence
resumed from one column, and the window records of a recording of any length.

  resume          the recurrence over a chunk of new columns given the previous column: Dd = d + min(Dd, Dn)(x-1,y-1),
                  Dn = d + min(Dd(x-1,y), Dd(x,y-1)), row 0 a start of the Dn kind, on packed u64 states (cost << 32 | start)
                  with ABSOLUTE starts.  The state is (Dd, min(Dd, Dn)) of the last column and the number of columns so far.
  end_records     window records from the packed end-row values of a whole recording.
  window_records  the same for feature frames, through spot_ref.dp_end_row over the recording as ONE row: what a session must
                  emit for a channel, whatever the chunking.
Both reductions take an `origin`: the records of the same frames when the first of them is frame `origin` of its channel and
nothing before it is reachable (the development hook "spot_live_origin"): starts, ends and window cuts move, nothing else.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import spot_ref as ref

INF64 = ref.INF64
SPOT_WIN_DTYPE = np.dtype([("channel", "<u4"), ("window", "<u4")])
MAX_FRAMES = 0xFFFF0000  # a channel's frame count: absolute starts live in the low word of a state


def _plus(c, add):
    return np.where(c == INF64, INF64, c + add)


def resume(d_chunk, state=None):
    """d_chunk int64 [n, M]: local distances of n new columns; state None (a fresh channel) or what an earlier call returned
    -> (end uint64 [n]: packed min(Dd, Dn) of the template's last row per new column, all ones = unreachable; the new state)"""
    d_chunk = np.asarray(d_chunk, np.int64)
    n, M = d_chunk.shape
    if state is None:
        state = (np.full(M, INF64, np.uint64), np.full(M, INF64, np.uint64), 0)
    pd, pm, x0 = state  # Dd and min(Dd, Dn) of column x0 - 1
    end = np.empty(n, np.uint64)
    for i in range(n):
        add = d_chunk[i].astype(np.uint64) << np.uint64(32)
        cd = np.full(M, INF64, np.uint64)
        cd[1:] = _plus(pm[:-1], add[1:])                         # (x-1, y-1)
        cn = np.empty(M, np.uint64)
        cn[0] = add[0] | np.uint64(x0 + i)                       # row 0: a start
        cn[1:] = _plus(np.minimum(pd[1:], cd[:-1]), add[1:])     # (x-1, y) and (x, y-1)
        pd, pm = cd, np.minimum(cd, cn)
        end[i] = pm[M - 1]
    return end, (pd, pm, x0 + n)


def n_window_rows(N, win, origin=0):
    """windows that hold one of the frames [origin, origin + N), or stand open at origin: origin // win .. ceil((origin + N) / win) - 1"""
    return -(-(int(origin) + int(N)) // int(win)) - int(origin) // int(win)


def _reduce(cost, start, q, win, origin):
    """per-end-frame results of the pushed frames AS THEIR OWN RECORDING (relative starts, q from relative figures: a path's
    length does not move with it) -> SPOT_DTYPE [n_window_rows]: the windows cut at ABSOLUTE multiples of win when the first
    pushed frame is frame `origin` of its channel, starts and ends absolute.  Row i is window origin // win + i; the first is
    partial when origin % win != 0.  All in Python ints: positions reach 0xFFFF0000."""
    N, win, origin = len(cost), int(win), int(origin)
    w0 = origin // win
    out = np.empty(n_window_rows(N, win, origin), ref.SPOT_DTYPE)
    for i in range(len(out)):
        lo, hi = max((w0 + i) * win - origin, 0), (w0 + i + 1) * win - origin
        hit = ref.window_hit(cost, start, q, lo, hi)
        out[i] = hit if hit == ref.NO_HIT else (hit[0], hit[1] + origin, hit[2] + origin, hit[3])
    return out


def end_records(end, M, win, origin=0):
    """packed end-row values of the pushed columns 0..N-1 (relative starts) -> SPOT_DTYPE [n_window_rows(N, win, origin)]: per
    window the first minimum of q(e) over its reachable end frames; origin: see _reduce"""
    end = np.asarray(end, np.uint64)
    ok = end != INF64
    cost = np.where(ok, (end >> np.uint64(32)).astype(np.int64), -1)
    start = np.where(ok, (end & np.uint64(0xFFFFFFFF)).astype(np.int64), 0)
    return _reduce(cost, start, ref.end_scores(cost, start, M), win, origin)


def window_records(feat, tm, tf, valid, win, origin=0):
    """feat int16 [N, 12]: everything pushed to a channel; templates as spot_ref.spot_hits -> SPOT_DTYPE [n_window_rows, K]
    (ceil(N / win) rows for origin 0); the last window is the open one when (origin + N) % win != 0.  origin: the channel's
    frame count before the first pushed frame, nothing before it reachable (see _reduce)"""
    N, K = len(feat), len(tm)
    out = np.empty((n_window_rows(N, win, origin), K), ref.SPOT_DTYPE)
    out[...] = ref.NO_HIT
    for k in range(K):
        M = int(tf[k]) if valid is None or valid[k] else 0
        if M == 0 or N == 0:
            continue
        cost, start = ref.dp_end_row(ref.local_dis(feat, tm[k, :M]))
        out[:, k] = _reduce(cost, start, ref.end_scores(cost, start, M), win, origin)
    return out


def push_windows(before, new, win):
    """frame counts per channel before a push and the new frames -> the (channel, window) rows the push emits, in order"""
    return [(c, w) for c, (b, n) in enumerate(zip(before, new)) for w in range(int(b) // win, (int(b) + int(n)) // win)]


def pcm_frames(samples, frame_len, hop):
    """frames of R samples framed as a segment with start = 1, end = R: frame j exists once R >= 1 + j * hop + frame_len"""
    return (samples - 1 - frame_len) // hop + 1 if samples >= 1 + frame_len else 0
