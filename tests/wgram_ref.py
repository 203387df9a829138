"""Weighted grammars (include/sr_engine.h, "weighted grammars") restated in numpy and Python ints: gram_ref's level building
over a word network whose arcs and final states carry costs.

  grammar  gram_ref's (n_states, arcs, final) followed by arc_cost [n_arcs] and final_cost [n_states] (each may be None or
           missing: all 0); c(s,t,w) = the cost of arc (s,t,w); the CHARGE LIST of a pair (t, w) = its (s, c(s,t,w)) by
           ascending s
  charge   C_l(x; t, w) = min over the (s, c) of the list with E_{l-1}(x, s) finite of E_{l-1}(x, s) + c; unreachable when
           there is no such s.  An unreachable E never has a cost added to it
  level, A_l, E_l   gram_ref's with that charge: the arc cost is part of a word's key cost and of cum
  L_l      min over the final f with E_l(N, f) finite of E_l(N, f) + final_cost[f]
  count    gram_ref's over these L_l
  end      the smallest final f with E_n(N, f) + final_cost[f] = L_n
  trace    gram_ref's with acc = key cost - word_cost - C_l(S; t, w(k)) (the word's own path cost), cum = E_l(p,t) (the last
           word's cum excludes the final cost, the record's cost includes it) and the source state the smallest s of the list
           with E_{l-1}(S, s) finite and E_{l-1}(S, s) + c = C_l(S; t, w(k))

history() builds A and E of a whole row once; trace() reads them at any prefix N (they depend on frames < p only), which is
what a live session emits after a push; decode_row() / decode() are the two in a row, in gram_ref's formats.
enumerate_cost() is an independent statement of L_n over every accepted STATE PATH of n arcs (two paths with one label
sequence can cost differently).  wrap=True drops the guard of the charge on purpose -- an unreachable E (all ones) plus c
wraps to c - 1, as a kernel that adds blindly would compute -- and exists only so that a test can prove it looks at a case
where the guard matters.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import chain_ref
import gram_ref
from chain_ref import CH_NONE, CH_OK, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, NO_WORD_ROW, e0, level_end_row  # noqa: F401
from gram_ref import check, grammar_any, grammar_sequence, grammar_word_pairs  # noqa: F401  (unweighted builders, re-exported)
from spot_ref import DIS_ERR, INF, local_dis

MAX_COST = 1 << 24


def cost_bound():
    """what no cost of a call inside the argument limits reaches: the decoder's bound, one arc per word, one final cost"""
    return chain_ref.cost_bound() + chain_ref.MAX_WORDS * MAX_COST + MAX_COST


def grammar_bigram(labels, cost, first_cost=None, last_cost=None):
    """one state per word (1 + its index in labels) plus the start; cost[a][b] the cost of b after a (None: forbidden),
    first_cost[w] of starting with w (None: forbidden), last_cost[w] the final cost after w (None: may not end here); the two
    vectors None: every word may start / end at cost 0 -> (n_states, arcs, final, arc_cost, final_cost)"""
    labels = list(dict.fromkeys(int(w) for w in labels))
    st = {w: 1 + i for i, w in enumerate(labels)}
    arcs = [((0, st[w], w), 0 if first_cost is None else first_cost[w]) for w in labels if first_cost is None or first_cost[w] is not None]
    arcs += [((st[a], st[b], b), cost[a][b]) for a in labels for b in labels if cost[a][b] is not None]
    ends = [(last_cost is None or last_cost[w] is not None, 0 if last_cost is None or last_cost[w] is None else last_cost[w]) for w in labels]
    return 1 + len(labels), [a for a, _ in arcs], [0] + [int(f) for f, _ in ends], [int(c) for _, c in arcs], [0] + [int(c) for _, c in ends]


def with_costs(gram, arc_cost=None, final_cost=None):
    """gram_ref's grammar with costs behind it"""
    return tuple(gram[:3]) + (None if arc_cost is None else [int(c) for c in arc_cost], None if final_cost is None else [int(c) for c in final_cost])


def drawn_costs(gram, seed=7, hi=20000):
    """the draw of the tests: arc costs first, then final costs masked to the final states"""
    rng = np.random.default_rng(seed)
    arc = rng.integers(0, hi + 1, len(gram[1]))
    fin = rng.integers(0, hi + 1, gram[0]) * (np.asarray(gram[2]) != 0)
    return with_costs(gram, arc, fin)


def costs_of(gram):
    """(arc_cost [n_arcs], final_cost [n_states]) as ints, the limits checked"""
    S, arcs, final = gram[:3]
    ac = [0] * len(arcs) if len(gram) < 4 or gram[3] is None else [int(c) for c in gram[3]]
    fc = [0] * S if len(gram) < 5 or gram[4] is None else [int(c) for c in gram[4]]
    assert len(ac) == len(arcs) and len(fc) == S and all(0 <= c <= MAX_COST for c in ac + fc)
    assert all(final[s] or not fc[s] for s in range(S))
    return ac, fc


def lists_of(gram):
    """{(t, w): [(s, c) by ascending s]}, in the order (t, w): the charge lists"""
    ac, _ = costs_of(gram)
    out = {}
    for (s, t, w), c in zip(gram[1], ac):
        out.setdefault((t, w), []).append((s, c))
    return {tw: sorted(out[tw]) for tw in sorted(out)}


def distinct_lists(gram):
    """the distinct charge lists in the order of their first pair (t, w): what sr_grammar_plan counts in out[3]"""
    return list(dict.fromkeys(tuple(v) for v in lists_of(gram).values()))


def _plus(e, c, wrap):
    if e is not None:
        return e + c
    if not wrap:
        return None
    v = (DIS_ERR + c) & 0xFFFFFFFF  # the unguarded sum, as 32-bit arithmetic gives it
    return None if v == DIS_ERR else v


def charge(E_prev, lst, x, wrap=False):
    """C_l(x; t, w) over the charge list, None = unreachable"""
    return min((v for v in (_plus(E_prev[s][x], c, wrap) for s, c in lst) if v is not None), default=None)


def history(gram, dis, N, max_words, skip=None, word_cost=0, word_of_slot=None, wrap=False):
    """dis per slot int64 [N, M_k] or None -> (A, E): A[l][t][p] = (cost, start, slot) or None, E[l][t][p] = cost or None"""
    S = gram[0]
    K = len(dis)
    lab = list(range(K)) if word_of_slot is None else [int(w) for w in word_of_slot]
    lists = lists_of(gram)
    none = [None] * (N + 1)
    E = [[e0(N, skip) if s == 0 else list(none) for s in range(S)]] + [[list(none) for _ in range(S)] for _ in range(max_words)]
    A = [None] + [[list(none) for _ in range(S)] for _ in range(max_words)]
    for l in range(1, max_words + 1):
        for (t, w), lst in lists.items():
            C = [charge(E[l - 1], lst, x, wrap) for x in range(N + 1)]
            if all(c is None for c in C[:N]):
                continue  # nothing starts: every end is unreachable
            for k in range(K):
                if lab[k] != w or dis[k] is None:
                    continue
                for x, v in enumerate(level_end_row(dis[k], C)):
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


def trace(A, E, N, gram, max_words, n_exact=0, word_cost=0, word_of_slot=None, wrap=False):
    """level costs, count, end state and the walk back at the prefix of N frames of a history of at least N + 1 positions ->
    gram_ref.decode_row's dict (words = [(slot, start, end, acc, cum, state after the word)])"""
    S, _, final = gram[:3]
    _, fc = costs_of(gram)
    lists = lists_of(gram)
    finals = [f for f in range(S) if final[f]]
    level_cost = [min((E[l][f][N] + fc[f] for f in finals if E[l][f][N] is not None), default=None) if N else None for l in range(1, max_words + 1)]
    n = n_exact
    if not n:
        finite = [(c, l + 1) for l, c in enumerate(level_cost) if c is not None]
        n = min(finite)[1] if finite else 1
    out = dict(status=CH_NONE, cost=None, n_words=0, skipped=0, words=[], level_cost=level_cost)
    if level_cost[n - 1] is None:
        return out
    p, t, words = N, min(f for f in finals if E[n][f][N] is not None and E[n][f][N] + fc[f] == level_cost[n - 1]), []
    for l in range(n, 0, -1):
        if E[l][t][p] is None:
            assert wrap  # only the unguarded sum walks into a state that was never reached
            break
        while A[l][t][p] is None or A[l][t][p][0] != E[l][t][p]:
            p -= 1
        cost, start, slot = A[l][t][p]
        w = slot if word_of_slot is None else int(word_of_slot[slot])
        lst = lists[(t, w)]
        c = charge(E[l - 1], lst, start, wrap)
        words.append((slot, start, p - 1, cost - word_cost - c, E[l][t][p], t))
        p, t = start, min(s for s, ac in lst if _plus(E[l - 1][s][start], ac, wrap) == c)
    assert wrap or (t == 0 and (E[0][0][p] is not None))
    words.reverse()
    out.update(status=CH_OK, cost=level_cost[n - 1], n_words=n, words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def decode_row(gram, dis, N, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None, wrap=False):
    """gram_ref.decode_row under costs"""
    A, E = history(gram, dis, N, max_words, skip, word_cost, word_of_slot, wrap)
    return trace(A, E, N, gram, max_words, n_exact, word_cost, word_of_slot, wrap)


def to_records(o, tf, max_words, word_of_slot=None):
    """decode_row's dict -> (rec CHAIN_REC_DTYPE [], words CHAIN_WORD_DTYPE [max_words], level_cost uint32 [max_words])"""
    rec = np.zeros((), CHAIN_REC_DTYPE)
    words = np.empty(max_words, CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    lc = np.array([DIS_ERR if c is None else c for c in o["level_cost"]], np.uint32)
    if o["status"] != CH_OK:
        rec[()] = (DIS_ERR, 0, 0, CH_NONE)
        return rec, words, lc
    rec[()] = (o["cost"], o["n_words"], o["skipped"], CH_OK)
    for i, (slot, start, end, acc, cum, state) in enumerate(o["words"]):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        words[i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, state)
    return rec, words, lc


def slot_distances(feat, tm, tf, valid=None):
    """per slot the local distances int64 [N, M_k] of a row of N frames, None for an invalid or empty slot"""
    return [local_dis(feat, tm[k, :int(tf[k])]) if (valid is None or valid[k]) and int(tf[k]) > 0 else None for k in range(len(tm))]


def decode(gram, mfcc, frames, tm, tf, valid, max_frames, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None, wrap=False):
    """gram_ref.decode under costs: the same three arrays"""
    n_rows = len(mfcc)
    rec = np.zeros(n_rows, CHAIN_REC_DTYPE)
    words = np.empty((n_rows, max_words), CHAIN_WORD_DTYPE)
    lc = np.empty((n_rows, max_words), np.uint32)
    for r in range(n_rows):
        N = min(int(frames[r]), max_frames)
        o = decode_row(gram, slot_distances(mfcc[r, :N], tm, tf, valid), N, max_words, n_exact, skip, word_cost, word_of_slot, wrap)
        rec[r], words[r], lc[r] = to_records(o, tf, max_words, word_of_slot)
    return rec, words, lc


class Recording:
    """everything pushed to a channel under one grammar, its history built once; row(N) = the records a live session emits
    when the channel stands at N frames: the prefix as one row"""

    def __init__(self, gram, feat, tm, tf, valid, max_words, skip=None, word_cost=0, word_of_slot=None):
        self.gram, self.N, self.tf, self.max_words, self.word_cost, self.word_of_slot = gram, len(feat), tf, max_words, word_cost, word_of_slot
        self.A, self.E = history(gram, slot_distances(feat, tm, tf, valid), self.N, max_words, skip, word_cost, word_of_slot)
        self._rows = {}

    def row(self, N, n_exact=0):
        assert 0 <= N <= self.N
        if (N, n_exact) not in self._rows:
            o = trace(self.A, self.E, N, self.gram, self.max_words, n_exact, self.word_cost, self.word_of_slot)
            self._rows[(N, n_exact)] = to_records(o, self.tf, self.max_words, self.word_of_slot)
        return self._rows[(N, n_exact)]


def accepted_paths(gram, n):
    """every state path of exactly n arcs from state 0 to a final state, as tuples of arc indices"""
    arcs, final = gram[1], gram[2]
    paths = [((), 0)]
    for _ in range(n):
        paths = [(p + (i,), t) for p, at in paths for i, (s, t, _) in enumerate(arcs) if s == at]
    return [p for p, at in paths if final[at]]


def enumerate_cost(gram, dis, N, n, skip=None, word_cost=0, word_of_slot=None):
    """L_n the long way: per accepted state path of n arcs the unconstrained chain with only that arc's word at each level and
    the arc's cost added to what the word builds on (prefixes shared between paths are computed once), the final cost of the
    path's last state added at N, and the minimum over the paths; None = no parse"""
    K = len(dis)
    lab = list(range(K)) if word_of_slot is None else [int(w) for w in word_of_slot]
    ac, fc = costs_of(gram)
    arcs = gram[1]
    memo = {(): e0(N, skip)}

    def prefix(path):
        if path not in memo:
            prev, A = [None if e is None else e + ac[path[-1]] for e in prefix(path[:-1])], [None] * (N + 1)
            for k in range(K):
                if lab[k] == arcs[path[-1]][2] and dis[k] is not None:
                    for x, v in enumerate(level_end_row(dis[k], prev)):
                        if v != INF and (A[x + 1] is None or v[0] + word_cost < A[x + 1]):
                            A[x + 1] = v[0] + word_cost
            E = [None] * (N + 1)
            for p in range(1, N + 1):
                E[p] = A[p]
                if skip is not None and E[p - 1] is not None and (E[p] is None or E[p - 1] + skip < E[p]):
                    E[p] = E[p - 1] + skip
            memo[path] = E
        return memo[path]

    if not N:
        return None
    return min((prefix(p)[N] + fc[arcs[p[-1]][1]] for p in accepted_paths(gram, n) if prefix(p)[N] is not None), default=None)


planted = chain_ref.planted
