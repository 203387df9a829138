"""The span scorer's definition (include/sr_engine.h, "word alternatives") restated in numpy: the cost F of the best word path of
one template over one fixed span of frames, start AND end pinned -- the connected-word decoder's word (tests/chain_ref.py) with
the one chargeable start column S and the one end column e.

  d(x,y)    spot_ref.local_dis of the span's frames in[S..e] and the template's M frames: int64 [L, M], L = e - S + 1
  paths     from (0, 0) to (L-1, M-1), steps (+1,+1), (+1,0), (0,+1), every horizontal or vertical step directly after a
            diagonal one, the start cell of the non-diagonal kind (so the first step is diagonal)
  F         the minimum over the paths of the sum of d; None when there is no path
  q         F // (L + M)

F is stated three ways, compared with each other and with an enumeration of the paths by tests/test_span_ref.py:
  span_scalar     the header's three-term recurrence on plain costs, D(0,0) = d(0,0), the rest of row 0 unreachable;
  span_two_state  the two-state form ("arrived by a diagonal step" / "by a horizontal or vertical one"), plain loops;
  span_end        the two-state form vectorised by anti-diagonals, which the GPU tests use.
None of them knows the reach rule (M//2 + 1 <= L <= 2M - 1): the recurrences produce it.
span_scores() turns word rows into the score rows the library writes, nbest() restates sr_nbest_batch over them, planted() is
the generator of the end-to-end tests: templates long enough for a span to cross a 64-column sweep of the kernel.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

from spot_ref import DIS_ERR, local_dis  # noqa: F401  (re-exported)

SPAN_ACC, SPAN_DIS = 0, 1
ALL_ONES = 0xFFFFFFFF
NO_WORD = 0xFFFFFFFF
NBEST_DTYPE = np.dtype([("word", "<u4"), ("slot", "<u4"), ("dis", "<u4"), ("count", "<u4")])
NO_CANDIDATE = (NO_WORD, 0xFFFFFFFF, DIS_ERR, 0)
CHAIN_WORD_DTYPE = np.dtype([("word", "<u4"), ("slot", "<u4"), ("start", "<u4"), ("end", "<u4"), ("acc", "<u4"), ("dis", "<u4"),
                             ("cum", "<u4"), ("reserved", "<u4")])
_INF = float("inf")


def _out(v):
    return None if v == _INF else int(v)


def span_scalar(d):
    """D(0,0) = d(0,0), D(x>0,0) unreachable; D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-2,y-1) + d(x-1,y), D(x-1,y-2) + d(x,y-1))
    -> D(L-1, M-1) or None"""
    L, M = d.shape
    D = {}

    def at(x, y):
        return D[(x, y)] if x >= 0 and y >= 0 else _INF

    for y in range(M):
        for x in range(L):
            if y == 0:
                D[(x, 0)] = int(d[0, 0]) if x == 0 else _INF
                continue
            best = min(at(x - 1, y - 1),
                       at(x - 2, y - 1) + int(d[x - 1, y]) if x >= 1 else _INF,
                       at(x - 1, y - 2) + int(d[x, y - 1]))
            D[(x, y)] = best + int(d[x, y])
    return _out(D[(L - 1, M - 1)])


def span_two_state(d):
    """Dd = d + min(Dd, Dn)(x-1,y-1); Dn = d + min(Dd(x-1,y), Dd(x,y-1)); (0, 0) is of the Dn kind, the rest of row 0 unreachable"""
    L, M = d.shape
    Dd, Dn = {}, {}

    def at(T, x, y):
        return T[(x, y)] if x >= 0 and y >= 0 else _INF

    for y in range(M):
        for x in range(L):
            c = int(d[x, y])
            if y == 0:
                Dd[(x, 0)], Dn[(x, 0)] = _INF, (c if x == 0 else _INF)
                continue
            Dd[(x, y)] = min(at(Dd, x - 1, y - 1), at(Dn, x - 1, y - 1)) + c
            Dn[(x, y)] = min(at(Dd, x - 1, y), at(Dd, x, y - 1)) + c
    return _out(min(Dd[(L - 1, M - 1)], Dn[(L - 1, M - 1)]))


_NONE = np.int64(1) << np.int64(62)  # unreachable, in the vectorised form (a cost stays below 2^31)


def span_end(d):
    """the two-state form by anti-diagonals on int64 costs (spot_ref.dp_end_row with one start column, the end cell alone)"""
    L, M = d.shape
    Dd = np.full((L + 1, M + 1), _NONE, np.int64)  # index + 1 in both directions: row / column 0 are the unreachable border
    Dm = np.full((L + 1, M + 1), _NONE, np.int64)
    d = d.astype(np.int64)

    def plus(c, add):
        return np.where(c >= _NONE, _NONE, c + add)

    for s in range(L + M - 1):
        ys = np.arange(max(0, s - (L - 1)), min(M - 1, s) + 1)
        xs = s - ys
        add = d[xs, ys]
        cd = plus(Dm[xs, ys], add)                                   # (x-1, y-1) in shifted indices
        cn = plus(np.minimum(Dd[xs, ys + 1], Dd[xs + 1, ys]), add)   # (x-1, y) and (x, y-1)
        first = ys == 0
        cd = np.where(first, _NONE, cd)
        cn = np.where(first, np.where(xs == 0, add, _NONE), cn)
        Dd[xs + 1, ys + 1] = cd
        Dm[xs + 1, ys + 1] = np.minimum(cd, cn)
    v = Dm[L, M]
    return None if v >= _NONE else int(v)


def paths(L, M):
    """every admissible path from (0, 0) to (L-1, M-1) as a list of cells, by depth-first search: after a diagonal step any of
    the three steps, after any other step (and at the start cell) a diagonal one only"""
    out = []

    def walk(x, y, free, cells):
        if (x, y) == (L - 1, M - 1):
            out.append(list(cells))
            return
        steps = ((1, 1), (1, 0), (0, 1)) if free else ((1, 1),)
        for dx, dy in steps:
            nx, ny = x + dx, y + dy
            if nx < L and ny < M:
                cells.append((nx, ny))
                walk(nx, ny, (dx, dy) == (1, 1), cells)
                cells.pop()

    walk(0, 0, False, [(0, 0)])
    return out


def span_row(feat, N, start, end, tm, tf, valid, mode, form=span_end):
    """one span of one feature row (N = its clamped frame count) -> the score row, list [K] of ints"""
    K = len(tm)
    if start == ALL_ONES or end == ALL_ONES or start > end or end >= N:
        return [DIS_ERR] * K
    row = []
    for k in range(K):
        M = int(tf[k]) if valid is None or valid[k] else 0
        F = form(local_dis(feat[start:end + 1], tm[k, :M])) if M else None
        row.append(DIS_ERR if F is None else F if mode == SPAN_ACC else F // (end - start + 1 + M))
    return row


def span_scores(mfcc, frames, tm, tf, valid, words, mode, form=span_end):
    """mfcc int16 [n_rows, max_frames, 12], frames [n_rows] (clamped to max_frames), templates tm int16 [K, rows, 12] of tf
    frames, valid [K] or None, words CHAIN_WORD_DTYPE [n_rows, words_per_row] (start and end are read) -> uint32 [n_rows,
    words_per_row, K]"""
    n_rows, wpr = words.shape
    out = np.empty((n_rows, wpr, len(tm)), np.uint32)
    for r in range(n_rows):
        N = min(int(frames[r]), mfcc.shape[1])
        for i in range(wpr):
            out[r, i] = span_row(mfcc[r], N, int(words[r, i]["start"]), int(words[r, i]["end"]), tm, tf, valid, mode, form)
    return out


def spans(rows):
    """[[(start, end), ...] per row] -> CHAIN_WORD_DTYPE [n_rows, words_per_row], every other field a value nothing may read"""
    w = np.empty((len(rows), len(rows[0])), CHAIN_WORD_DTYPE)
    w[...] = (0xDEADBEEF,) * 8
    for r, row in enumerate(rows):
        assert len(row) == len(rows[0])
        for i, (s, e) in enumerate(row):
            w[r, i]["start"], w[r, i]["end"] = s, e
    return w


def nbest(scores, word_of_slot, n_best):
    """sr_nbest_batch restated: scores uint32 [..., K] -> (NBEST_DTYPE [..., n_best], n_matched uint32 [...]).  A word's
    distance is the first minimum of its slots in slot order, candidates rank by (dis, slot)."""
    scores = np.asarray(scores, np.uint32)
    K = scores.shape[-1]
    flat = scores.reshape(-1, K)
    nb = np.empty((len(flat), n_best), NBEST_DTYPE)
    nb[...] = NO_CANDIDATE
    nm = np.zeros(len(flat), np.uint32)
    for r, row in enumerate(flat):
        best = {}
        for k, dis in enumerate(int(v) for v in row):
            if dis == DIS_ERR:
                continue
            w = int(word_of_slot[k])
            if w not in best:
                best[w] = [dis, k, 1]
            else:
                best[w][2] += 1
                if dis < best[w][0]:
                    best[w][:2] = [dis, k]
        cands = sorted((dis, k, w, c) for w, (dis, k, c) in best.items())
        nm[r] = len(cands)
        for i, (dis, k, w, c) in enumerate(cands[:n_best]):
            nb[r, i] = (w, k, dis, c)
    return nb.reshape(scores.shape[:-1] + (n_best,)), nm.reshape(scores.shape[:-1])


# ---- planted words: the rows of the end-to-end tests ---------------------------------------------------------------------------
PLANT_SEED, PLANT_ROWS, PLANT_K, PLANT_MAXF, PLANT_MAX_WORDS, PLANT_SKIP = 4711, 6, 6, 320, 4, 1500


def planted(seed=PLANT_SEED, n_rows=PLANT_ROWS):
    """chain_ref.planted() with long templates: K = 6 random templates of 40..70 frames; rows of 1..4 planted words, each
    time-stretched (a template frame lasts one or two input frames), noise of +-60 on every coefficient and 0..5 quiet frames
    (+-40) before, between and after -> dict(tm, tf, im, inf, seq = the planted slots per row, spans = their frames).  A word
    covers up to 93 frames, so spans cross the kernel's 64-column sweeps."""
    rng = np.random.default_rng(seed)
    tf = rng.integers(40, 71, PLANT_K).astype(np.uint32)
    tm = np.zeros((PLANT_K, 71, 12), np.int16)
    for k in range(PLANT_K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    im = np.zeros((n_rows, PLANT_MAXF, 12), np.int16)
    inf = np.zeros(n_rows, np.uint32)
    seq, sps = [], []
    for r in range(n_rows):
        n_words = 1 + r % 4
        slots = [int(k) for k in rng.integers(0, PLANT_K, n_words)]
        frames, sp = [], []

        def quiet():
            for _ in range(int(rng.integers(0, 6))):
                frames.append(rng.integers(-40, 41, 12))

        quiet()
        for k in slots:
            M = int(tf[k])
            idx, y = [], 0
            while y < M:  # after a diagonal step: one time in three the frame is held for a second input frame
                idx.append(y)
                if y > 0 and int(rng.integers(0, 3)) == 0:
                    idx.append(y)
                y += 1
            sp.append((len(frames), len(frames) + len(idx) - 1))
            for y in idx:
                frames.append(tm[k, y].astype(np.int64) + rng.integers(-60, 61, 12))
            quiet()
        assert len(frames) <= PLANT_MAXF
        im[r, :len(frames)] = np.array(frames)
        inf[r] = len(frames)
        seq.append(slots)
        sps.append(sp)
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf, seq=seq, spans=sps)
