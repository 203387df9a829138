"""Live grammar-constrained decoding (include/sr_engine.h, "live grammar-constrained decoding") restated in numpy and Python
ints: gram_ref's levels over a word network, kept as ONE history per recording and resumed from push to push as
chain_live_ref resumes the unconstrained decoder's.

  history    A[l][t][p] = (cost, start, slot) or None (l = 1..max_words; A[0] unused) and E[l][t][p] = cost or None (l =
             0..max_words) of a whole recording, by gram_ref's definitions.  They depend on frames < p only, so the history of
             a recording is a prefix of that of any longer one ...
  trace      ... and level costs, count, end state and the walk back through levels and states at any N <= len read A, E and
             N alone -> gram_ref.decode_row's dict.
  Recording  a channel's history built once, the records of a row per N (the state after each word in `reserved`).
  Channel    a push as the device runs it: the new positions initialised in every level and state, per level every kept
             (slot, target) item's column resumed with the charge taken as the minimum over its from-set, the keys' minimum
             into A_l(., target), E_l(., target) extended from the carried E_l(x0, target); then the trace.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import chain_live_ref as live
import gram_ref as ref
from chain_live_ref import CHAIN_LIVE_ROW_DTYPE, pcm_frames, slot_distances  # noqa: F401
from spot_ref import DIS_ERR, INF, INF64


# The four grammars of the live tests over chain_ref.planted()'s five slots, as (grammar, word_of_slot or None = word = slot):
# the anchor; a sequence whose tail is optional; word pairs with half the pairs forbidden and a restricted first word; a small
# network over two slots per word (labels 0, 0, 1, 1, 2) in which word 2 enters state 3 from state 1 AND from state 2, word 1
# enters state 2 from 0 and from 3 and word 0 enters state 1 from 0 and from 3: from-sets of more than one state.
SPW2 = np.arange(ref.chain_ref.PLANT_K, dtype=np.uint32) // 2
SPW2.setflags(write=False)
GRAMMARS = dict(
    anchor=(ref.grammar_any(range(5)), None),
    seq=(ref.grammar_sequence([[0, 1, 2], [2, 3, 4], [0, 4], [1, 3]], optional_tail=True), None),
    pairs=(ref.grammar_word_pairs(range(5), [(a, b) for a in range(5) for b in range(5) if (a + b) % 2 == 1], first=[0, 1, 2, 4]), None),
    join=((4, [(0, 1, 0), (0, 2, 1), (1, 3, 2), (2, 3, 2), (3, 1, 0), (1, 1, 1), (3, 2, 1)], [0, 1, 0, 1]), SPW2))


def labels(K, word_of_slot=None):
    return list(range(K)) if word_of_slot is None else [int(w) for w in word_of_slot]


def charge(E_prev, frm, x):
    """C_l(x; t, w): the cheapest state of the from-set at column x, None = unreachable"""
    return min((E_prev[s][x] for s in frm if E_prev[s][x] is not None), default=None)


def history(gram, dis, N, max_words, skip=None, word_cost=0, word_of_slot=None):
    """dis as gram_ref.decode_row takes it (per slot int64 [N, M_k] or None) -> (A, E): what a session keeps.  Level l holds
    the items sr_grammar_plan keeps there (gram_ref.items_per_level: the exact pruning, which depends on the grammar and
    max_words alone and changes no output of any prefix); everything else stays unreachable."""
    S = gram[0]
    lab, pairs = labels(len(dis), word_of_slot), ref.pairs_of(gram)
    items = ref.items_per_level(gram, max_words, lab, [d is not None for d in dis])
    none = [None] * (N + 1)
    E = [[ref.e0(N, skip) if s == 0 else list(none) for s in range(S)]] + [[list(none) for _ in range(S)] for _ in range(max_words)]
    A = [None] + [[list(none) for _ in range(S)] for _ in range(max_words)]
    for l in range(1, max_words + 1):
        C = {}
        for k, t in items[l - 1]:
            tw = (t, lab[k])
            if tw not in C:
                C[tw] = [charge(E[l - 1], pairs[tw], x) for x in range(N + 1)]
            for x, v in enumerate(ref.level_end_row(dis[k], C[tw])):
                if v != INF:
                    cand = (v[0] + word_cost, v[1], k)
                    if A[l][t][x + 1] is None or cand < A[l][t][x + 1]:
                        A[l][t][x + 1] = cand
        for t in range(S):
            for p in range(1, N + 1):
                best = None if A[l][t][p] is None else A[l][t][p][0]
                if skip is not None and E[l][t][p - 1] is not None and (best is None or E[l][t][p - 1] + skip < best):
                    best = E[l][t][p - 1] + skip
                E[l][t][p] = best
    return A, E


def trace(A, E, N, gram, max_words, n_exact=0, word_cost=0, word_of_slot=None):
    """level costs, count, end state and trace of the prefix of N frames from a history of at least N + 1 positions ->
    gram_ref.decode_row's dict (words = [(slot, start, end, acc, cum, state after the word)])"""
    S, _, final = gram
    pairs = ref.pairs_of(gram)
    finals = [f for f in range(S) if final[f]]
    level_cost = [min((E[l][f][N] for f in finals if E[l][f][N] is not None), default=None) if N else None for l in range(1, max_words + 1)]
    n = n_exact
    if not n:
        finite = [(c, l + 1) for l, c in enumerate(level_cost) if c is not None]
        n = min(finite)[1] if finite else 1
    out = dict(status=ref.CH_NONE, cost=None, n_words=0, skipped=0, words=[], level_cost=level_cost)
    if level_cost[n - 1] is None:
        return out
    p, t, words = N, min(f for f in finals if E[n][f][N] == level_cost[n - 1]), []
    for l in range(n, 0, -1):
        while A[l][t][p] is None or A[l][t][p][0] != E[l][t][p]:
            p -= 1
        cost, start, slot = A[l][t][p]
        w = slot if word_of_slot is None else int(word_of_slot[slot])
        frm = pairs[(t, w)]
        c = charge(E[l - 1], frm, start)
        words.append((slot, start, p - 1, cost - word_cost - c, E[l][t][p], t))
        p, t = start, min(s for s in frm if E[l - 1][s][start] == c)
    assert t == 0
    words.reverse()
    out.update(status=ref.CH_OK, cost=level_cost[n - 1], n_words=n, words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def to_records(o, tf, max_words, word_of_slot=None):
    """gram_ref.decode_row's dict -> (rec CHAIN_REC_DTYPE [], words CHAIN_WORD_DTYPE [max_words], level_cost uint32 [max_words])"""
    rec = np.zeros((), ref.CHAIN_REC_DTYPE)
    words = np.empty(max_words, ref.CHAIN_WORD_DTYPE)
    words[...] = ref.NO_WORD_ROW
    lc = np.array([DIS_ERR if c is None else c for c in o["level_cost"]], np.uint32)
    if o["status"] != ref.CH_OK:
        rec[()] = (DIS_ERR, 0, 0, ref.CH_NONE)
        return rec, words, lc
    rec[()] = (o["cost"], o["n_words"], o["skipped"], ref.CH_OK)
    for i, (slot, start, end, acc, cum, state) in enumerate(o["words"]):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        words[i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, state)
    return rec, words, lc


class Recording:
    """everything pushed to a channel under one grammar, its history built once; row(N) = the records a session emits when
    the channel stands at N frames"""

    def __init__(self, gram, feat, tm, tf, valid, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None):
        self.gram, self.N, self.tf, self.max_words, self.n_exact = gram, len(feat), tf, max_words, n_exact
        self.word_cost, self.word_of_slot = word_cost, word_of_slot
        self.A, self.E = history(gram, slot_distances(feat, tm, tf, valid), self.N, max_words, skip, word_cost, word_of_slot)
        self._rows = {}

    def row(self, N, n_exact=None):
        """n_exact None: the recording's own; the history does not depend on it"""
        n_exact = self.n_exact if n_exact is None else n_exact
        assert 0 <= N <= self.N
        if (N, n_exact) not in self._rows:
            o = trace(self.A, self.E, N, self.gram, self.max_words, n_exact, self.word_cost, self.word_of_slot)
            self._rows[(N, n_exact)] = to_records(o, self.tf, self.max_words, self.word_of_slot)
        return self._rows[(N, n_exact)]


class Channel:
    """one channel of a session, step by step as the device runs a push.  items[l - 1] = the (slot, target) items level l keeps
    (gram_ref.items_per_level): only those are swept and only their targets closed; everything else stays as init left it."""

    def __init__(self, gram, M_of_slot, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None, valid=None):
        self.gram, self.M, self.W, self.n_exact, self.skip, self.word_cost = gram, M_of_slot, max_words, n_exact, skip, word_cost
        self.word_of_slot, self.valid = word_of_slot, valid
        self.lab = labels(len(M_of_slot), word_of_slot)
        self.items = ref.items_per_level(gram, max_words, self.lab, valid)
        self.pairs = ref.pairs_of(gram)
        self.N, S = 0, gram[0]
        self.cols = [dict() for _ in range(max_words + 1)]  # per level: item -> chain_live_ref.resume_level's state
        self.E = [[[] for _ in range(S)] for _ in range(max_words + 1)]
        self.A = [None] + [[[] for _ in range(S)] for _ in range(max_words)]

    def push(self, dis_chunk):
        """dis_chunk: per slot the local distances int64 [n, M_k] of the n new frames, None for an invalid slot -> the parse of
        everything pushed so far (gram_ref.decode_row's dict)"""
        n = next(len(d) for d in dis_chunk if d is not None)
        x0, S = self.N, self.gram[0]
        if n:  # (a push of 0 frames touches nothing, as the kernels return at once for n = 0)
            # init: the new positions (x0, x0 + n], and position 0 for a fresh channel
            new = list(range(x0 + 1 if x0 else 0, x0 + n + 1))
            for l in range(self.W + 1):
                for s in range(S):
                    self.E[l][s] += [(0 if p == 0 else (None if self.skip is None else p * self.skip)) if (l == 0 and s == 0) else None for p in new]
                    if l:
                        self.A[l][s] += [None] * len(new)
            for l in range(1, self.W + 1):
                for (k, t) in self.items[l - 1]:
                    d = dis_chunk[k]
                    frm = self.pairs[(t, self.lab[k])]
                    C = [charge(self.E[l - 1], frm, x) for x in range(x0, x0 + n)]  # in the kernel: once per lane and sweep
                    end, self.cols[l][(k, t)] = live.resume_level(d, C, self.cols[l].get((k, t)))
                    for i, v in enumerate(end):
                        if v != INF64:
                            cand = ((int(v) >> 32) + self.word_cost, int(v) & 0xFFFFFFFF, k)
                            if self.A[l][t][x0 + i + 1] is None or cand < self.A[l][t][x0 + i + 1]:
                                self.A[l][t][x0 + i + 1] = cand
                for t in sorted({t for _, t in self.items[l - 1]}):  # the close: from the carried E_l(x0, t) on
                    A, E = self.A[l][t], self.E[l][t]
                    for p in range(x0 + 1, x0 + n + 1):
                        best = None if A[p] is None else A[p][0]
                        if self.skip is not None:
                            js = [A[j][0] + (p - j) * self.skip for j in range(x0 + 1, p + 1) if A[j] is not None]
                            if E[x0] is not None:
                                js.append(E[x0] + (p - x0) * self.skip)
                            best = min(js) if js else None
                        E[p] = best
            self.N += n
        if not self.N:
            return dict(status=ref.CH_NONE, cost=None, n_words=0, skipped=0, words=[], level_cost=[None] * self.W)
        return trace(self.A, self.E, self.N, self.gram, self.W, self.n_exact, self.word_cost, self.word_of_slot)

    def end(self):
        """the recording ends: the channel is as freshly opened (the columns of a fresh channel are never read)"""
        self.__init__(self.gram, self.M, self.W, self.n_exact, self.skip, self.word_cost, self.word_of_slot, self.valid)
