"""The one-pass connected-word decoder's definition (include/sr_engine.h, "one-pass connected-word decoding") restated in plain
Python: ONE prefix-cost array E(p) over all word counts instead of chain_ref's one per level.  Everything not restated is
chain_ref's: d, the word path, skip_cost, word_cost, the key (cost, start, slot), the records.

  E(0)     0
  D_k      the spotter's recurrence with a charged start: D_k(x,0) = E(x) + d(x,0), S = x, unreachable where E(x) is
  A(p)     min over the valid slots of (D_k(p-1, M_k-1) + word_cost, S, k), compared as (cost, start, slot)            (p >= 1)
  E(p)     min(A(p).cost, E(p-1) + skip_cost), the second term only when skipping is on
  result   E(N) unreachable or N = 0: CH_NONE.  Otherwise cost = E(N), n_words = the words on the trace (0 is possible)
  trace    p = N; while p > 0: A(p) unreachable or A(p).cost != E(p): p -= 1; else word = A(p), end = p-1, cum = E(p),
           acc = cost - word_cost - E(start), p = start

The arrays A and E are stated two ways, compared with each other by tests/test_onepass_ref.py:
  history_sync    time-synchronous: per frame one column of every slot (the two-state form, plain loops on tuples);
  history_blocks  what the kernels do: blocks of n <= L = min_k(M_k // 2 + 1) frames.  A block [c0, cN) sweeps, per slot, the
                  columns (c0_prev, cN) from the saved EXACT column at c0_prev, charging E(col) for col <= c0 and nothing
                  behind c0, saves column c0, sends the ends of the columns >= c0 to A(col + 1), then closes E over (c0, cN].
trace_row() walks either; decode() turns rows into the records the library writes.  Plain module: no fixtures, no pytest
settings.
"""
import numpy as np

import chain_ref
from chain_ref import CH_NONE, CH_OK, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, NO_WORD_ROW  # noqa: F401  (re-exported)
from spot_ref import DIS_ERR, INF, local_dis  # noqa: F401  (re-exported)

CH_TRUNCATED = 2
WORD_COST_SUM = 1 << 30


def reach(tf, valid=None):
    """L: min over the valid slots of M // 2 + 1; 0 = no valid slot"""
    lens = [int(m) for k, m in enumerate(tf) if int(m) > 0 and (valid is None or valid[k])]
    return min(m // 2 + 1 for m in lens) if lens else 0


def cost_ok(cap, L, word_cost):
    return not L or (cap // L) * word_cost <= WORD_COST_SUM


def _plus(c, d):
    return c if c == INF else (c[0] + int(d), c[1])


def _column(d_col, left, charge, x):
    """one column of the two-state form: d_col [M], left = the column x - 1 as (Dd [M], Dm [M]) or None, charge = E(x) or None
    -> (Dd, Dm), Dm = min(Dd, Dn)"""
    M = len(d_col)
    Dd, Dm = [INF] * M, [INF] * M
    for y in range(M):
        c = int(d_col[y])
        if y == 0:
            dn = INF if charge is None else (charge + c, x)
        else:
            Dd[y] = _plus(left[1][y - 1], c) if left else INF
            dn = _plus(min(left[0][y] if left else INF, Dd[y - 1]), c)
        Dm[y] = min(Dd[y], dn)
    return Dd, Dm


def _send(A, p, v, word_cost, k):
    if v != INF:
        cand = (v[0] + word_cost, v[1], k)
        if A[p] is None or cand < A[p]:
            A[p] = cand


def _close(A, E, lo, hi, skip):
    for p in range(lo + 1, hi + 1):
        best = None if A[p] is None else A[p][0]
        if skip is not None and E[p - 1] is not None and (best is None or E[p - 1] + skip < best):
            best = E[p - 1] + skip
        E[p] = best


def history_sync(dis, N, skip=None, word_cost=0):
    """dis: per slot the local distances int64 [N, M_k], or None for an invalid slot -> (A [N + 1] of (cost, start, slot) or
    None, E [N + 1] of cost or None)"""
    A, E = [None] * (N + 1), [0] + [None] * N
    cols = [None] * len(dis)
    for x in range(N):
        for k, d in enumerate(dis):
            if d is None:
                continue
            cols[k] = _column(d[x], cols[k], E[x], x)
            _send(A, x + 1, cols[k][1][-1], word_cost, k)
        _close(A, E, x, x + 1, skip)
    return A, E


def history_blocks(dis, N, n, skip=None, word_cost=0, cap=None):
    """the block form with blocks of n frames over cap >= N frames (the host's bound; default N)"""
    cap = N if cap is None else cap
    assert n >= 1 and cap >= N
    A, E = [None] * (N + 1), [0] + [None] * N
    saved = [None] * len(dis)  # per slot the exact column at the previous block's c0
    for c0 in range(0, cap, n):
        if N <= c0:
            break
        cN = min(c0 + n, cap, N)
        for k, d in enumerate(dis):
            if d is None:
                continue
            col = saved[k]
            for x in range(c0 - n + 1 if c0 else 0, cN):
                col = _column(d[x], col, E[x] if x <= c0 else None, x)
                if x == c0:
                    saved[k] = col
                if x >= c0:
                    _send(A, x + 1, col[1][-1], word_cost, k)
        _close(A, E, c0, cN, skip)
    return A, E


def trace_row(A, E, N, word_cost=0):
    """-> dict(status, cost, n_words, skipped, words = [(slot, start, end, acc, cum)] in spoken order)"""
    out = dict(status=CH_NONE, cost=None, n_words=0, skipped=0, words=[])
    if N == 0 or E[N] is None:
        return out
    p, words = N, []
    while p > 0:
        if A[p] is None or A[p][0] != E[p]:
            p -= 1
            continue
        cost, start, slot = A[p]
        words.append((slot, start, p - 1, cost - word_cost - E[start], E[p]))
        p = start
    words.reverse()
    out.update(status=CH_OK, cost=E[N], n_words=len(words), words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def decode_row(dis, N, skip=None, word_cost=0, block=0):
    A, E = history_blocks(dis, N, block, skip, word_cost) if block else history_sync(dis, N, skip, word_cost)
    return trace_row(A, E, N, word_cost)


def decode(mfcc, frames, tm, tf, valid, max_frames, words_cap, skip=None, word_cost=0, word_of_slot=None, frames_cap=0, block=0):
    """mfcc int16 [n_rows, max_frames, 12], frames [n_rows] (clamped to min(max_frames, frames_cap), frames_cap 0 = max_frames),
    templates tm int16 [K, rows, 12] of tf frames, valid [K] or None, word_of_slot [K] or None (word = slot) -> (rec
    CHAIN_REC_DTYPE [n_rows], words CHAIN_WORD_DTYPE [n_rows, words_cap])"""
    n_rows, K = len(mfcc), len(tm)
    cap = min(max_frames, frames_cap) if frames_cap else max_frames
    if not cost_ok(cap, reach(tf, valid), word_cost):
        raise ValueError("(frames_cap / L) * word_cost exceeds 2^30")
    rec = np.zeros(n_rows, CHAIN_REC_DTYPE)
    words = np.empty((n_rows, words_cap), CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    for r in range(n_rows):
        N = min(int(frames[r]), cap)
        dis = [local_dis(mfcc[r, :N], tm[k, :int(tf[k])]) if (valid is None or valid[k]) and int(tf[k]) > 0 else None for k in range(K)]
        o = decode_row(dis, N, skip, word_cost, block)
        if o["status"] != CH_OK:
            rec[r] = (DIS_ERR, 0, 0, CH_NONE)
            continue
        rec[r] = (o["cost"], o["n_words"], o["skipped"], CH_TRUNCATED if o["n_words"] > words_cap else CH_OK)
        for i, (slot, start, end, acc, cum) in enumerate(o["words"][:words_cap]):
            word = slot if word_of_slot is None else int(word_of_slot[slot])
            words[r, i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, 0)
    return rec, words


# ---- planted words: long rows, more words than level building holds ---------------------------------------------------------------
LONG_SEED, LONG_COUNTS, LONG_MAXF = 4242, (17, 24, 32, 40), 1024


def planted_long():
    """chain_ref.planted()'s generator with seed 4242, word counts (17, 24, 32, 40) and max_frames 1024 -> the same dict"""
    rng = np.random.default_rng(LONG_SEED)
    K = chain_ref.PLANT_K
    tf = rng.integers(8, 15, K).astype(np.uint32)
    tm = np.zeros((K, 15, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    n_rows = len(LONG_COUNTS)
    im = np.zeros((n_rows, LONG_MAXF, 12), np.int16)
    inf = np.zeros(n_rows, np.uint32)
    seq, spans = [], []
    for r in range(n_rows):
        slots = [int(k) for k in rng.integers(0, K, LONG_COUNTS[r])]
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
        assert len(frames) <= LONG_MAXF
        im[r, :len(frames)] = np.array(frames)
        inf[r] = len(frames)
        seq.append(slots)
        spans.append(sp)
    for a in (tm, tf, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im, inf=inf, seq=seq, spans=spans)
