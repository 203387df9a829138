"""Live connected-word decoding (include/sr_engine.h, "live connected-word decoding") restated in numpy: one level of the
decoder resumed from one column, and the parse of every prefix of a recording from ONE history.

  resume_level     spot_live_ref.resume with a CHARGED row 0: the recurrence over a chunk of new columns given the previous
                   column and E_{l-1} over the chunk's columns, on packed u64 states (cost << 32 | start), starts absolute.
  history          A_l(p) and E_l(p) of a whole recording, level by level (chain_ref's definitions).  They depend on frames
                   < p only, so the history of a recording is a prefix of that of any longer one ...
  trace            ... and count selection and trace at any N <= len read A, E and N alone.
  prefix_decodes   history once, trace at every requested N: what a session must emit after a push that takes a channel to
                   N frames, whatever the chunking.  tests/test_chain_live.py holds it to chain_ref.decode_row of each prefix.
  to_records       the same as the records the library writes; Recording = a channel's history built once, a row per N.
  Channel          a push as the device runs it: init of the new positions, per level the resumed columns and the keys'
                   minimum, E_l extended from the carried E_l(x0), the trace.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import chain_ref as ref
from spot_ref import DIS_ERR, INF, INF64, local_dis

CHAIN_LIVE_ROW_DTYPE = np.dtype([("channel", "<u4"), ("frames", "<u4")])
MAX_FRAMES = ref.MAX_FRAMES  # utt_frames at most: the u32 cost bound and the start field of a key end there


def _plus(c, add):
    return np.where(c == INF64, INF64, c + add)


def resume_level(d_chunk, e_prev_slice, state=None):
    """d_chunk int64 [n, M]: local distances of n new columns; e_prev_slice [n]: E_{l-1}(x) of those columns, None =
    unreachable; state None (a fresh channel) or what an earlier call returned -> (end uint64 [n]: packed min(Dd, Dn) of the
    template's last row per new column, all ones = unreachable; the new state)"""
    d_chunk = np.asarray(d_chunk, np.int64)
    n, M = d_chunk.shape
    assert len(e_prev_slice) == n
    if state is None:
        state = (np.full(M, INF64, np.uint64), np.full(M, INF64, np.uint64), 0)
    pd, pm, x0 = state  # Dd and min(Dd, Dn) of column x0 - 1
    end = np.empty(n, np.uint64)
    for i in range(n):
        add = d_chunk[i].astype(np.uint64) << np.uint64(32)
        cd = np.full(M, INF64, np.uint64)
        cd[1:] = _plus(pm[:-1], add[1:])                         # (x-1, y-1)
        cn = np.empty(M, np.uint64)
        e = e_prev_slice[i]                                      # row 0: a charged start
        cn[0] = INF64 if e is None else ((np.uint64(int(e)) << np.uint64(32)) + add[0]) | np.uint64(x0 + i)
        cn[1:] = _plus(np.minimum(pd[1:], cd[:-1]), add[1:])     # (x-1, y) and (x, y-1)
        pd, pm = cd, np.minimum(cd, cn)
        end[i] = pm[M - 1]
    return end, (pd, pm, x0 + n)


def history(dis, N, max_words, skip=None, word_cost=0):
    """dis as chain_ref.decode_row takes it (per slot int64 [N, M_k] or None) -> (A, E): A[l][p] = (cost, start, slot) or None
    for l = 1..max_words (A[0] unused), E[l][p] = cost or None for l = 0..max_words, p = 0..N"""
    E = [ref.e0(N, skip)] + [[None] * (N + 1) for _ in range(max_words)]
    A = [None] + [[None] * (N + 1) for _ in range(max_words)]
    for l in range(1, max_words + 1):
        for k, d in enumerate(dis):
            if d is None:
                continue
            for x, v in enumerate(ref.level_end_row(d, E[l - 1])):
                if v != INF:
                    cand = (v[0] + word_cost, v[1], k)
                    if A[l][x + 1] is None or cand < A[l][x + 1]:
                        A[l][x + 1] = cand
        for p in range(1, N + 1):
            best = None if A[l][p] is None else A[l][p][0]
            if skip is not None and E[l][p - 1] is not None and (best is None or E[l][p - 1] + skip < best):
                best = E[l][p - 1] + skip
            E[l][p] = best
    return A, E


def trace(A, E, N, max_words, n_exact=0, word_cost=0):
    """count selection and trace of the prefix of N frames from a history of at least N + 1 positions -> chain_ref.decode_row's
    dict"""
    level_cost = [E[l][N] if N else None for l in range(1, max_words + 1)]
    n = n_exact
    if not n:
        finite = [(c, l + 1) for l, c in enumerate(level_cost) if c is not None]
        n = min(finite)[1] if finite else 1
    out = dict(status=ref.CH_NONE, cost=None, n_words=0, skipped=0, words=[], level_cost=level_cost)
    if level_cost[n - 1] is None:
        return out
    p, words = N, []
    for l in range(n, 0, -1):
        while A[l][p] is None or A[l][p][0] != E[l][p]:
            p -= 1
        cost, start, slot = A[l][p]
        words.append((slot, start, p - 1, cost - word_cost - E[l - 1][start], E[l][p]))
        p = start
    words.reverse()
    out.update(status=ref.CH_OK, cost=level_cost[n - 1], n_words=n, words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def prefix_decodes(dis, N, prefixes, max_words, n_exact=0, skip=None, word_cost=0):
    """the history of the whole row once, then {n: the parse of its first n frames} for n in prefixes"""
    A, E = history(dis, N, max_words, skip, word_cost)
    return {int(n): trace(A, E, int(n), max_words, n_exact, word_cost) for n in prefixes}


def to_records(o, tf, max_words, word_of_slot=None):
    """chain_ref.decode_row's dict -> (rec CHAIN_REC_DTYPE [], words CHAIN_WORD_DTYPE [max_words], level_cost uint32 [max_words])"""
    rec = np.zeros((), ref.CHAIN_REC_DTYPE)
    words = np.empty(max_words, ref.CHAIN_WORD_DTYPE)
    words[...] = ref.NO_WORD_ROW
    lc = np.array([DIS_ERR if c is None else c for c in o["level_cost"]], np.uint32)
    if o["status"] != ref.CH_OK:
        rec[()] = (DIS_ERR, 0, 0, ref.CH_NONE)
        return rec, words, lc
    rec[()] = (o["cost"], o["n_words"], o["skipped"], ref.CH_OK)
    for i, (slot, start, end, acc, cum) in enumerate(o["words"]):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        words[i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, 0)
    return rec, words, lc


def slot_distances(feat, tm, tf, valid=None):
    """feat int16 [N, 12] -> per slot the local distances, None for an invalid slot (chain_ref.decode's rule)"""
    return [local_dis(feat, tm[k, :int(tf[k])]) if (valid is None or valid[k]) and int(tf[k]) > 0 else None for k in range(len(tm))]


class Recording:
    """everything pushed to a channel, its history built once; row(N) = the records a session emits when the channel stands at
    N frames"""

    def __init__(self, feat, tm, tf, valid, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None):
        self.N, self.tf, self.max_words, self.n_exact, self.word_cost, self.word_of_slot = len(feat), tf, max_words, n_exact, word_cost, word_of_slot
        self.A, self.E = history(slot_distances(feat, tm, tf, valid), self.N, max_words, skip, word_cost)
        self._rows = {}

    def row(self, N, n_exact=None):
        """n_exact None: the recording's own; the history does not depend on it"""
        n_exact = self.n_exact if n_exact is None else n_exact
        assert 0 <= N <= self.N
        if (N, n_exact) not in self._rows:
            self._rows[(N, n_exact)] = to_records(trace(self.A, self.E, N, self.max_words, n_exact, self.word_cost), self.tf,
                                                  self.max_words, self.word_of_slot)
        return self._rows[(N, n_exact)]


class Channel:
    """one channel of a session, step by step as the device runs a push: the new positions initialised, per level every
    slot's column resumed and its end frames' keys sent to A_l, E_l extended from the carried E_l(x0); then the trace.  The
    history after any pushes is history() of everything pushed."""

    def __init__(self, M_of_slot, max_words, n_exact=0, skip=None, word_cost=0):
        self.M, self.W, self.n_exact, self.skip, self.word_cost = M_of_slot, max_words, n_exact, skip, word_cost
        self.N = 0
        self.cols = [[None] * len(M_of_slot) for _ in range(max_words + 1)]  # resume_level's state per (level, slot)
        self.E = [[0]] + [[None] for _ in range(max_words)]                  # position 0 of a fresh channel
        self.A = [None] + [[None] for _ in range(max_words)]

    def push(self, dis_chunk):
        """dis_chunk: per slot the local distances int64 [n, M_k] of the n new frames, None for an invalid slot -> the parse of
        everything pushed so far (chain_ref.decode_row's dict)"""
        n = next(len(d) for d in dis_chunk if d is not None) if any(d is not None for d in dis_chunk) else 0
        x0 = self.N
        self.E[0] += [None if self.skip is None else p * self.skip for p in range(x0 + 1, x0 + n + 1)]
        for l in range(1, self.W + 1):
            self.A[l] += [None] * n
            for k, d in enumerate(dis_chunk):
                if d is None:
                    continue
                end, self.cols[l][k] = resume_level(d, self.E[l - 1][x0:x0 + n], self.cols[l][k])
                for i, v in enumerate(end):
                    if v != INF64:
                        cand = ((int(v) >> 32) + self.word_cost, int(v) & 0xFFFFFFFF, k)
                        if self.A[l][x0 + i + 1] is None or cand < self.A[l][x0 + i + 1]:
                            self.A[l][x0 + i + 1] = cand
            for p in range(x0 + 1, x0 + n + 1):  # the close: from the carried E_l(x0) on
                best = None if self.A[l][p] is None else self.A[l][p][0]
                if self.skip is not None:
                    js = [self.A[l][j][0] + (p - j) * self.skip for j in range(x0 + 1, p + 1) if self.A[l][j] is not None]
                    if self.E[l][x0] is not None:
                        js.append(self.E[l][x0] + (p - x0) * self.skip)
                    best = min(js) if js else None
                self.E[l].append(best)
        self.N += n
        return trace(self.A, self.E, self.N, self.W, self.n_exact, self.word_cost)


def pcm_frames(samples, frame_len, hop):
    """frames of R samples framed as a segment with start = 1, end = R: frame j exists once R >= 1 + j * hop + frame_len"""
    return (samples - 1 - frame_len) // hop + 1 if samples >= 1 + frame_len else 0
