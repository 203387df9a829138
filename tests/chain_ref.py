"""The connected-word decoder's definition (include/sr_engine.h, "connected-word decoding") restated in numpy: level-building
DTW over a template store.  Level l holds the best parse of every prefix of a row into exactly l words; one level is the word
spotter's recurrence (tests/spot_ref.py) with a CHARGED start row, E_{l-1}(x) + d(x, 0), a minimum over the slots per end frame
and, when skipping is on, a prefix minimum that lets frames between words be skipped at skip_cost each.

  d(x,y)   spot_ref.local_dis.
  E_0(p)   p * skip_cost when skipping is on, else 0 for p = 0 and unreachable for p > 0            (p = 0..N, a prefix length)
  level    D(x,0) = E_{l-1}(x) + d(x,0), S(x,0) = x, unreachable where E_{l-1}(x) is; otherwise the spotter's
           D(x,y) = d(x,y) + min(D(x-1,y-1), D(x-2,y-1) + d(x-1,y), D(x-1,y-2) + d(x,y-1)), candidates compared as (cost, start)
  A_l(p)   min over the valid slots k of (D_k(p-1, M_k-1) + word_cost, S, k), compared as (cost, start, slot)          (p >= 1)
  E_l(p)   min(A_l(p).cost, E_l(p-1) + skip_cost), the second term only when skipping is on; E_l(0) unreachable
  count    n_words_exact, or the n of 1..max_words with the smallest E_n(N), the fewest words among equal costs
  trace    p = N; l = n..1: while A_l(p) is unreachable or A_l(p).cost != E_l(p): p -= 1; word l = A_l(p), end = p-1; p = S

The level is stated three ways, compared with each other by tests/test_chain_ref.py:
  level_scalar     the recurrence as the header states it, on (cost, start) tuples, plain loops;
  level_two_state  the two-state form with a charged start row, plain loops;
  level_end_row    the two-state form vectorised by anti-diagonals on packed u64 states, which the GPU tests use.
decode_row() builds levels, count and trace on any of them; decode() turns rows into the records the library writes.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

from spot_ref import DIS_ERR, INF, INF64, local_dis  # noqa: F401  (re-exported)

CH_OK, CH_NONE = 0, 1
CHAIN_REC_DTYPE = np.dtype([("cost", "<u4"), ("n_words", "<u4"), ("skipped", "<u4"), ("status", "<u4")])
CHAIN_WORD_DTYPE = np.dtype([("word", "<u4"), ("slot", "<u4"), ("start", "<u4"), ("end", "<u4"), ("acc", "<u4"), ("dis", "<u4"),
                             ("cum", "<u4"), ("reserved", "<u4")])
NO_WORD_ROW = (0xFFFFFFFF,) * 8
MAX_WORDS, MAX_SKIP, MAX_WORD_COST, MAX_FRAMES, MAX_D = 16, 65535, 1 << 24, 16383, 65536


def cost_bound():
    """what no cost of a call inside the argument limits reaches: at most 3L cells of at most MAX_D each in a word over L
    frames (a skipped frame costs less than one cell), MAX_WORDS words of at most MAX_WORD_COST"""
    return 3 * MAX_FRAMES * MAX_D + MAX_WORDS * MAX_WORD_COST


def e0(N, skip):
    """E_0: list of N + 1 costs, None = unreachable; skip None = no skipping"""
    return [0] + [None if skip is None else p * skip for p in range(1, N + 1)]


def _plus(c, d):
    return c if c == INF else (c[0] + int(d), c[1])


def level_scalar(d, e_prev):
    """d int64 [N, M], e_prev list [N + 1] -> the end row: list [N] of (cost, start) or INF"""
    N, M = d.shape
    D = {}

    def at(x, y):
        return D[(x, y)] if x >= 0 and y >= 0 else INF

    for y in range(M):
        for x in range(N):
            if y == 0:
                D[(x, 0)] = INF if e_prev[x] is None else (e_prev[x] + int(d[x, 0]), x)
                continue
            best = min(at(x - 1, y - 1),
                       _plus(at(x - 2, y - 1), d[x - 1, y]) if x >= 1 else INF,
                       _plus(at(x - 1, y - 2), d[x, y - 1]))
            D[(x, y)] = _plus(best, d[x, y])
    return [D[(x, M - 1)] for x in range(N)]


def level_two_state(d, e_prev):
    """Dd = d + min(Dd, Dn)(x-1,y-1); Dn = d + min(Dd(x-1,y), Dd(x,y-1)); row 0 is of the Dn kind and charged"""
    N, M = d.shape
    Dd, Dn = {}, {}

    def at(T, x, y):
        return T[(x, y)] if x >= 0 and y >= 0 else INF

    for y in range(M):
        for x in range(N):
            c = int(d[x, y])
            if y == 0:
                Dd[(x, 0)], Dn[(x, 0)] = INF, INF if e_prev[x] is None else (e_prev[x] + c, x)
                continue
            Dd[(x, y)] = _plus(min(at(Dd, x - 1, y - 1), at(Dn, x - 1, y - 1)), c)
            Dn[(x, y)] = _plus(min(at(Dd, x - 1, y), at(Dd, x, y - 1)), c)
    return [min(Dd[(x, M - 1)], Dn[(x, M - 1)]) for x in range(N)]


def level_end_row(d, e_prev):
    """the two-state form by anti-diagonals on packed states cost << 32 | start (spot_ref.dp_end_row with a charged row 0)"""
    N, M = d.shape
    if N == 0:
        return []
    Dd = np.full((N + 1, M + 1), INF64, np.uint64)  # index + 1 in both directions: row / column 0 are the unreachable border
    Dm = np.full((N + 1, M + 1), INF64, np.uint64)
    dd = d.astype(np.uint64) << np.uint64(32)
    ok = np.array([e is not None for e in e_prev[:N]])
    charge = np.array([0 if e is None else e for e in e_prev[:N]], np.uint64) << np.uint64(32)

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
        cn = np.where(first, np.where(ok[xs], (charge[xs] + add) | xs.astype(np.uint64), INF64), cn)
        Dd[xs + 1, ys + 1] = cd
        Dm[xs + 1, ys + 1] = np.minimum(cd, cn)
    return [INF if v == INF64 else (int(v) >> 32, int(v) & 0xFFFFFFFF) for v in Dm[1:, M]]


def decode_row(dis, N, max_words, n_exact=0, skip=None, word_cost=0, level=level_end_row):
    """dis: per slot the local distances int64 [N, M_k], or None for an invalid slot -> dict(status, cost, n_words, skipped,
    words = [(slot, start, end, acc, cum)] in spoken order, level_cost = [E_l(N) or None for l = 1..max_words])"""
    E = [e0(N, skip)] + [[None] * (N + 1) for _ in range(max_words)]
    A = [None] + [[None] * (N + 1) for _ in range(max_words)]
    for l in range(1, max_words + 1):
        for k, d in enumerate(dis):
            if d is None:
                continue
            for x, v in enumerate(level(d, E[l - 1])):
                if v != INF:
                    cand = (v[0] + word_cost, v[1], k)
                    if A[l][x + 1] is None or cand < A[l][x + 1]:
                        A[l][x + 1] = cand
        for p in range(1, N + 1):
            best = None if A[l][p] is None else A[l][p][0]
            if skip is not None and E[l][p - 1] is not None and (best is None or E[l][p - 1] + skip < best):
                best = E[l][p - 1] + skip
            E[l][p] = best
    level_cost = [E[l][N] for l in range(1, max_words + 1)]
    n = n_exact
    if not n:
        finite = [(c, l + 1) for l, c in enumerate(level_cost) if c is not None]
        n = min(finite)[1] if finite else 1
    out = dict(status=CH_NONE, cost=None, n_words=0, skipped=0, words=[], level_cost=level_cost)
    if level_cost[n - 1] is None:
        return out
    p, words = N, []
    for l in range(n, 0, -1):
        while A[l][p] is None or A[l][p][0] != E[l][p]:
            p -= 1
        cost, start, slot = A[l][p]
        words.append((slot, start, p - 1, cost - word_cost - E[l - 1][start], E[l][p]))
        p = start
    assert skip is not None or p == 0
    words.reverse()
    out.update(status=CH_OK, cost=level_cost[n - 1], n_words=n, words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def decode(mfcc, frames, tm, tf, valid, max_frames, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None, level=level_end_row):
    """mfcc int16 [n_rows, max_frames, 12], frames [n_rows] (clamped to max_frames), templates tm int16 [K, rows, 12] of tf
    frames, valid [K] or None, word_of_slot [K] or None (word = slot) -> (rec CHAIN_REC_DTYPE [n_rows], words CHAIN_WORD_DTYPE
    [n_rows, max_words], level_cost uint32 [n_rows, max_words])"""
    n_rows, K = len(mfcc), len(tm)
    rec = np.zeros(n_rows, CHAIN_REC_DTYPE)
    words = np.empty((n_rows, max_words), CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    lc = np.full((n_rows, max_words), DIS_ERR, np.uint32)
    for r in range(n_rows):
        N = min(int(frames[r]), max_frames)
        dis = [local_dis(mfcc[r, :N], tm[k, :int(tf[k])]) if (valid is None or valid[k]) and int(tf[k]) > 0 else None for k in range(K)]
        o = decode_row(dis, N, max_words, n_exact, skip, word_cost, level)
        lc[r] = [DIS_ERR if c is None else c for c in o["level_cost"]]
        if o["status"] != CH_OK:
            rec[r] = (DIS_ERR, 0, 0, CH_NONE)
            continue
        rec[r] = (o["cost"], o["n_words"], o["skipped"], CH_OK)
        for i, (slot, start, end, acc, cum) in enumerate(o["words"]):
            word = slot if word_of_slot is None else int(word_of_slot[slot])
            words[r, i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, 0)
    return rec, words, lc


# ---- planted words: the rows of the CPU and the GPU test ---------------------------------------------------------------------
PLANT_SEED, PLANT_ROWS, PLANT_K, PLANT_MAXF, PLANT_MAX_WORDS, PLANT_SKIP = 2024, 12, 5, 160, 5, 1500


def planted(seed=PLANT_SEED, n_rows=PLANT_ROWS):
    """K = 5 random templates of 8..14 frames; rows of 1..4 planted words, each time-stretched (a template frame lasts one or two input
    frames: a horizontal step directly after a diagonal one, which the step pattern admits), with noise of +-60 on every coefficient and 0..5 quiet
    frames (+-40) before, between and after -> dict(tm, tf, im, inf, seq = the planted slots per row, spans = their frames)"""
    rng = np.random.default_rng(seed)
    tf = rng.integers(8, 15, PLANT_K).astype(np.uint32)
    tm = np.zeros((PLANT_K, 15, 12), np.int16)
    for k in range(PLANT_K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    im = np.zeros((n_rows, PLANT_MAXF, 12), np.int16)
    inf = np.zeros(n_rows, np.uint32)
    seq, spans = [], []
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
        spans.append(sp)
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf, seq=seq, spans=spans)
