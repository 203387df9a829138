"""The full-DP aligner's and the DBA trainer's definitions (include/sr_engine.h, "full-DP alignment and word models from many
examples") restated in numpy.

  pair    an input row in[0..N) and a reference ref[0..R); d = get_dis; gate N >= 1, R >= 1, not (N > 2R or 2N < R); cells inside
          dtw_limit's parallelogram; D(1,1) = d(1,1), D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-1,y), D(x,y-1)); acc = D(N,R),
          dis = acc // (N + R).
  path    traced back from (N,R): at each cell the reachable predecessor of minimal D, ties (x-1,y-1), (x-1,y), (x,y-1).
  span    span[x] = y_first | y_last << 16 (0-based, inclusive), path_len = number of path points.
  train   per iteration every example is aligned against its model's centroid, the frames matched to a centroid row are
          averaged (s32 sum, division truncating toward zero), rows nobody was matched to stay.

The DP runs by anti-diagonals in int64 (a few million cells a second); the trace-back reads D itself, not recorded choices.
Indices here are 0-based: cell (x, y) is the definition's (x + 1, y + 1).  Plain module: no fixtures, no pytest settings.
"""
import numpy as np

from spot_ref import local_dis  # get_dis of every (input frame, reference frame)

DIS_ERR = 0xFFFFFFFF
NONE32 = 0xFFFFFFFF
MAX_FRAMES = 1024  # SR_ALIGN_MAX_FRAMES
OK, GATED, TOO_LONG = 0, 1, 2
ALIGN_DTYPE = np.dtype([("dis", "<u4"), ("acc", "<u4"), ("path_len", "<u4"), ("status", "<u4")])
TRAIN_STAT_DTYPE = np.dtype([("n_ok", "<u4"), ("n_fail", "<u4"), ("acc", "<u8")])
INF = np.int64(1) << 40  # an unreachable cell


def gate(N, R):
    return N >= 1 and R >= 1 and not (N > 2 * R or 2 * N < R)


def inside(N, R):
    """dtw_limit (DTW.C:76-109) for a pair that passed the gate -> bool [N, R], True = inside the parallelogram"""
    X1, X2 = ((2 * R - N) // 3) & 0xFFFF, ((4 * N - 2 * R) // 3) & 0xFFFF  # DTW.C:141-142 (both numerators are >= 0)
    x, y = np.arange(1, N + 1)[:, None], np.arange(1, R + 1)[None, :]
    o1 = np.where(x < X1, y >= 2 * x + 2, 2 * y + N - 2 * R >= x + 4)
    o2 = np.where(x < X2, 2 * y + 2 <= x, y + 4 <= 2 * x + R - 2 * N)
    return ~(o1 | o2)


def dp(d, band=None):
    """the recurrence over the cells of `band` (default: dtw_limit's) -> D int64 [N, R], INF = unreachable"""
    N, R = d.shape
    band = inside(N, R) if band is None else band
    D = np.full((N + 1, R + 1), INF, np.int64)  # index + 1 in both directions: row / column 0 are the unreachable border
    for s in range(N + R - 1):
        ys = np.arange(max(0, s - (N - 1)), min(R - 1, s) + 1)
        xs = s - ys
        best = np.minimum(np.minimum(D[xs, ys], D[xs, ys + 1]), D[xs + 1, ys])
        if s == 0:
            best[:] = 0
        D[xs + 1, ys + 1] = np.where((best < INF) & band[xs, ys], best + d[xs, ys], INF)
    return D[1:, 1:]


def trace(D):
    """the path from (N-1, R-1) back to (0, 0) along D, as a list of (x, y) from the start; None: the end cell is unreachable"""
    N, R = D.shape
    if D[N - 1, R - 1] >= INF:
        return None
    x, y = N - 1, R - 1
    path = [(x, y)]
    while (x, y) != (0, 0):
        best, step = INF, None
        for dx, dy in ((1, 1), (1, 0), (0, 1)):  # the tie order: a later candidate must be strictly better
            if x - dx >= 0 and y - dy >= 0 and D[x - dx, y - dy] < best:
                best, step = D[x - dx, y - dy], (dx, dy)
        x, y = x - step[0], y - step[1]
        path.append((x, y))
    return path[::-1]


def spans(path, N):
    """span[x] = y_first | y_last << 16 of a path that covers input frames 0..N-1 -> uint32 [N]"""
    first, last = np.full(N, 1 << 20, np.int64), np.full(N, -1, np.int64)
    for x, y in path:
        first[x], last[x] = min(first[x], y), max(last[x], y)
    return (first | (last << 16)).astype(np.uint32)


def align_pair(inp, ref):
    """inp int16 [N, 12] (N <= MAX_FRAMES), ref int16 [R, 12] -> ((dis, acc, path_len, status), path or None)"""
    N, R = len(inp), len(ref)
    if not gate(N, R):
        return (DIS_ERR, NONE32, 0, GATED), None
    D = dp(local_dis(inp, ref))
    path = trace(D)
    if path is None:
        return (DIS_ERR, NONE32, 0, GATED), None
    acc = int(D[N - 1, R - 1])
    return (acc // (N + R), acc, len(path), OK), path


def align(mfcc, frames, ref, ref_frames, ref_of_row=None):
    """mfcc int16 [n, max_frames, 12], frames [n] (clamped to max_frames); ref int16 [n_ref, ref_rows, 12], ref_frames [n_ref]
    (0 or above ref_rows: invalid); ref_of_row [n] or None -> (rec ALIGN_DTYPE [n], span uint32 [n, max_frames], paths)"""
    n, max_frames = mfcc.shape[:2]
    rec, span, paths = np.empty(n, ALIGN_DTYPE), np.full((n, max_frames), NONE32, np.uint32), []
    for r in range(n):
        N = min(int(frames[r]), max_frames)
        k = r if ref_of_row is None else int(ref_of_row[r])
        R = int(ref_frames[k]) if k < len(ref) else 0
        R = R if R <= ref.shape[1] else 0
        if N > MAX_FRAMES:
            rec[r], path = (DIS_ERR, NONE32, 0, TOO_LONG), None
        elif R == 0:
            rec[r], path = (DIS_ERR, NONE32, 0, GATED), None
        else:
            rec[r], path = align_pair(mfcc[r, :N], ref[k, :R])
        if path is not None:
            span[r, :N] = spans(path, N)
        paths.append(path)
    return rec, span, paths


def train_iteration(mfcc, frames, ex_start, cen, cen_frames):
    """one DBA iteration -> (centroids int16 like cen, stats TRAIN_STAT_DTYPE [M])"""
    M, cen_rows = cen.shape[:2]
    out, stats = np.zeros_like(cen), np.zeros(M, TRAIN_STAT_DTYPE)
    E = int(ex_start[M])
    model_of = np.repeat(np.arange(M), np.diff(np.asarray(ex_start, np.int64)))
    rec, _, paths = align(mfcc[:E], frames[:E], cen, cen_frames, model_of)
    for m in range(M):
        F = int(cen_frames[m])
        if F < 1 or F > cen_rows:  # an invalid centroid: copied through, its examples GATED
            out[m] = cen[m]
            stats[m]["n_fail"] = int(ex_start[m + 1]) - int(ex_start[m])
            continue
        total, cnt = np.zeros((F, 12), np.int64), np.zeros(F, np.int64)
        for e in range(int(ex_start[m]), int(ex_start[m + 1])):
            if rec[e]["status"] != OK:
                stats[m]["n_fail"] += 1
                continue
            stats[m]["n_ok"] += 1
            stats[m]["acc"] += int(rec[e]["acc"])
            for x, y in paths[e]:
                total[y] += mfcc[e, x]
                cnt[y] += 1
        assert np.abs(total).max(initial=0) < 2 ** 31 and cnt.max(initial=0) <= 65535
        mean = np.sign(total) * (np.abs(total) // np.maximum(cnt, 1)[:, None])  # truncation toward zero
        out[m, :F] = np.where(cnt[:, None] > 0, mean, cen[m, :F])
    return out, stats


def train(mfcc, frames, ex_start, cen, cen_frames, n_iter):
    """-> (centroids after n_iter chained iterations, stats TRAIN_STAT_DTYPE [n_iter, M])"""
    stats = []
    for _ in range(n_iter):
        cen, st = train_iteration(mfcc, frames, ex_start, cen, cen_frames)
        stats.append(st)
    return cen, np.array(stats)
