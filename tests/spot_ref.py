"""The word spotter's definition (include/sr_engine.h, "word spotting") restated in numpy: subsequence DTW of one template
inside one feature row, symmetric P = 1 step pattern, ties broken towards the smallest start frame.

Three forms of the same thing, compared with each other by tests/test_spot.py:
  dp_scalar     the recurrence as the header states it, on (cost, start) tuples, plain loops;
  dp_two_state  the two-state form ("arrived by a diagonal step" / "arrived by a horizontal or vertical step"), plain loops;
  dp_end_row    the two-state form vectorised by anti-diagonals on packed u64 states (cost << 32 | start): a few million
                cells a second, which is what the GPU tests use.
spot_hits() turns end rows into the window records the library writes.  Plain module: no fixtures, no pytest settings.
"""
import numpy as np

DIS_ERR = 0xFFFFFFFF
INF = (float("inf"), float("inf"))           # an unreachable cell of the tuple forms
INF64 = np.uint64(0xFFFFFFFFFFFFFFFF)        # ... of the packed form
SPOT_DTYPE = np.dtype([("dis", "<u4"), ("start", "<u4"), ("end", "<u4"), ("acc", "<u4")])
NO_HIT = (DIS_ERR, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)


def local_dis(inp, mdl):
    """get_dis (DTW.C:45-62) of every (input frame, template frame): the squared differences summed in u32 wrap, the root
    taken in float32 and truncated -> int64 [N, M]"""
    a, b = np.asarray(inp, np.int64), np.asarray(mdl, np.int64)
    d2 = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)) & 0xFFFFFFFF  # = sum (a - b)^2 mod 2^32
    return np.sqrt(d2.astype(np.float32)).astype(np.int64)


def _plus(c, d):
    return c if c == INF else (c[0] + d, c[1])


def dp_scalar(d):
    """D(x,0) = d(x,0), S(x,0) = x; D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-2,y-1) + d(x-1,y), D(x-1,y-2) + d(x,y-1)) with
    candidates compared as (cost, start) -> dict (x, y) -> (cost, start) or INF"""
    N, M = d.shape
    D = {}

    def at(x, y):
        return D[(x, y)] if x >= 0 and y >= 0 else INF

    for y in range(M):
        for x in range(N):
            if y == 0:
                D[(x, 0)] = (int(d[x, 0]), x)
                continue
            best = min(at(x - 1, y - 1),
                       _plus(at(x - 2, y - 1), int(d[x - 1, y])) if x >= 1 else INF,
                       _plus(at(x - 1, y - 2), int(d[x, y - 1])))
            D[(x, y)] = _plus(best, int(d[x, y]))
    return D


def dp_two_state(d):
    """Dd = d + min(Dd, Dn)(x-1,y-1); Dn = d + min(Dd(x-1,y), Dd(x,y-1)); row 0 is of the Dn kind -> dict of min(Dd, Dn)"""
    N, M = d.shape
    Dd, Dn = {}, {}

    def at(T, x, y):
        return T[(x, y)] if x >= 0 and y >= 0 else INF

    for y in range(M):
        for x in range(N):
            c = int(d[x, y])
            if y == 0:
                Dd[(x, 0)], Dn[(x, 0)] = INF, (c, x)
                continue
            Dd[(x, y)] = _plus(min(at(Dd, x - 1, y - 1), at(Dn, x - 1, y - 1)), c)
            Dn[(x, y)] = _plus(min(at(Dd, x - 1, y), at(Dd, x, y - 1)), c)
    return {p: min(Dd[p], Dn[p]) for p in Dd}


def dp_end_row(d):
    """the end row of the two-state form, by anti-diagonals -> (cost int64 [N], start int64 [N]); cost -1 = unreachable"""
    N, M = d.shape
    if N == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    # index + 1 in both directions: row / column 0 of the arrays are the unreachable border
    Dd = np.full((N + 1, M + 1), INF64, np.uint64)
    Dm = np.full((N + 1, M + 1), INF64, np.uint64)
    dd = d.astype(np.uint64) << np.uint64(32)

    def plus(c, add):
        return np.where(c == INF64, INF64, c + add)

    for s in range(N + M - 1):
        ys = np.arange(max(0, s - (N - 1)), min(M - 1, s) + 1)
        xs = s - ys
        add = dd[xs, ys]
        cd = plus(Dm[xs, ys], add)                                   # (x-1, y-1) in shifted indices
        cn = plus(np.minimum(Dd[xs, ys + 1], Dd[xs + 1, ys]), add)   # (x-1, y) and (x, y-1)
        first = ys == 0
        cd = np.where(first, INF64, cd)
        cn = np.where(first, add | xs.astype(np.uint64), cn)
        Dd[xs + 1, ys + 1] = cd
        Dm[xs + 1, ys + 1] = np.minimum(cd, cn)
    end = Dm[1:, M]
    ok = end != INF64
    return np.where(ok, (end >> np.uint64(32)).astype(np.int64), -1), np.where(ok, (end & np.uint64(0xFFFFFFFF)).astype(np.int64), 0)


def end_scores(cost, start, M):
    """q(e) = D / (L + M), L = e - S + 1 -> int64 [N], -1 where the end frame is unreachable"""
    e = np.arange(len(cost))
    return np.where(cost >= 0, cost // np.maximum(e - start + 1 + M, 1), -1)


def window_hit(cost, start, q, lo, hi):
    """the first minimum of q(e) over the reachable end frames of [lo, hi) -> a SPOT_DTYPE tuple"""
    best = None
    for e in range(lo, min(hi, len(cost))):
        if q[e] >= 0 and (best is None or q[e] < q[best]):
            best = e
    return NO_HIT if best is None else (int(q[best]), int(start[best]), best, int(cost[best]))


def n_windows(max_frames, win_frames):
    return 1 if win_frames == 0 else -(-max_frames // win_frames)


def spot_hits(mfcc, frames, tm, tf, valid, max_frames, win_frames=0):
    """mfcc int16 [n_rows, max_frames, 12], frames [n_rows] (clamped to max_frames), templates tm int16 [K, rows, 12] of tf
    frames, valid [K] or None -> SPOT_DTYPE [n_rows, n_win, K]"""
    n_rows, K = len(mfcc), len(tm)
    n_win = n_windows(max_frames, win_frames)
    out = np.empty((n_rows, n_win, K), SPOT_DTYPE)
    out[...] = NO_HIT
    for r in range(n_rows):
        N = min(int(frames[r]), max_frames)
        for k in range(K):
            M = int(tf[k]) if valid is None or valid[k] else 0
            if M == 0 or N == 0:
                continue
            cost, start = dp_end_row(local_dis(mfcc[r, :N], tm[k, :M]))
            q = end_scores(cost, start, M)
            for w in range(n_win):
                lo, hi = (0, N) if win_frames == 0 else (w * win_frames, (w + 1) * win_frames)
                out[r, w, k] = window_hit(cost, start, q, lo, hi)
    return out
