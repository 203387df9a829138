"""Grammar-constrained decoding (include/sr_engine.h, "grammar-constrained decoding") restated in numpy: the connected-word
decoder's level building (tests/chain_ref.py) over a finite-state word network.

  grammar  states 0..S-1, state 0 the start, final[s] flags the final states, distinct arcs (from, to, word); word is a label
           of the word map; slots(w) = the valid slots with label w; From(t, w) = {s : (s, t, w) is an arc}
  E_0(p,s) chain_ref.e0 for s = 0, unreachable for every other state
  charge   C_l(x; t, w) = min over s in From(t, w) of E_{l-1}(x, s)
  level    per pair (t, w) with an arc and per slot k of slots(w): chain_ref's level with the charge in the place of E_{l-1}
  A_l(p,t) min over those pairs and slots of (D_k(p-1, M_k-1) + word_cost, S, k), compared as (cost, start, slot)    (p >= 1)
  E_l(p,t) min(A_l(p,t).cost, E_l(p-1,t) + skip_cost), the second term only when skipping is on; E_l(0,t) unreachable
  L_l      min over the final states f of E_l(N, f)
  count    n_words_exact, or the n of 1..max_words with the smallest L_n, the fewest words among equal costs
  end      the smallest final f with E_n(N, f) = L_n
  trace    p = N, t = f; l = n..1: while A_l(p,t) is unreachable or A_l(p,t).cost != E_l(p,t): p -= 1; word l = A_l(p,t) with
           slot k, start S, end p-1, cum E_l(p,t), state t; acc = cost - word_cost - C_l(S; t, w(k)); the source state is the
           smallest s of From(t, w(k)) with E_{l-1}(S, s) = C_l(S; t, w(k)); p = S, t = s

decode_row() and decode() are chain_ref's with the grammar in front; enumerate_cost() is an independent statement of L_n: it
lists every label sequence of length n the grammar accepts and chains chain_ref.level_end_row over that position's slots only.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import chain_ref
from chain_ref import CH_NONE, CH_OK, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, NO_WORD_ROW, e0, level_end_row  # noqa: F401
from spot_ref import DIS_ERR, INF, local_dis

MAX_STATES, MAX_ARCS = 64, 4096


# ---- the three grammar builders of the Python interface, restated --------------------------------------------------------------
def grammar_any(labels):
    """the anchor: one state, final, one loop per label: every sequence of words"""
    return 1, [(0, 0, int(w)) for w in dict.fromkeys(labels)], [1]


def grammar_sequence(positions, optional_tail=False):
    """position i takes one label of positions[i]: state i --w--> state i + 1; the last state is final, every state past the
    start as well when optional_tail is set"""
    n = len(positions)
    arcs = [(i, i + 1, int(w)) for i, ws in enumerate(positions) for w in dict.fromkeys(ws)]
    return n + 1, arcs, [int(i == n or (optional_tail and i >= 1)) for i in range(n + 1)]


def grammar_word_pairs(labels, allowed_pairs, first=None, last=None):
    """one state per word (1 + its index in labels) plus the start: a word of `first` may begin, b may follow a when (a, b) is
    allowed, a word of `last` may end (None: any)"""
    labels = list(dict.fromkeys(int(w) for w in labels))
    st = {w: 1 + i for i, w in enumerate(labels)}
    arcs = [(0, st[w], w) for w in labels if first is None or w in first]
    arcs += [(st[a], st[b], int(b)) for a, b in dict.fromkeys((int(a), int(b)) for a, b in allowed_pairs)]
    return 1 + len(labels), arcs, [0] + [int(last is None or w in last) for w in labels]


def check(gram, labels=None):
    n_states, arcs, final = gram
    assert 1 <= n_states <= MAX_STATES and 1 <= len(arcs) <= MAX_ARCS and len(final) == n_states and any(final)
    assert len(set(arcs)) == len(arcs) and all(s < n_states and t < n_states for s, t, _ in arcs)
    assert labels is None or all(w in labels for _, _, w in arcs)


def pairs_of(gram):
    """{(t, w): sorted From(t, w)}, in the order (t, w)"""
    out = {}
    for s, t, w in gram[1]:
        out.setdefault((t, w), []).append(s)
    return {tw: sorted(out[tw]) for tw in sorted(out)}


def accepts(gram, seq):
    """walks (label, state after it) pairs from state 0 along arcs to a final state"""
    arcs, at = set(gram[1]), 0
    for w, t in seq:
        if (at, t, w) not in arcs:
            return False
        at = t
    return bool(gram[2][at])


def items_per_level(gram, max_words, word_of_slot, valid=None):
    """the exact pruning: level l keeps the (slot, target) items whose from-set meets the states reachable from 0 in exactly
    l - 1 arcs and whose target reaches a final state within max_words - l further arcs -> list of sorted item lists"""
    S, arcs, final = gram
    reach = [{0}]
    for _ in range(max_words):
        reach.append({t for s, t, _ in arcs if s in reach[-1]})
    togo = [{s for s in range(S) if final[s]}]  # within j arcs
    for _ in range(max_words):
        togo.append(togo[-1] | {s for s, t, _ in arcs if t in togo[-1]})
    out = []
    for l in range(1, max_words + 1):
        out.append(sorted((k, t) for (t, w), frm in pairs_of(gram).items() if set(frm) & reach[l - 1] and t in togo[max_words - l]
                          for k, lab in enumerate(word_of_slot) if lab == w and (valid is None or valid[k])))
    return out


def decode_row(gram, dis, N, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None, level=level_end_row):
    """chain_ref.decode_row under the grammar (word_of_slot None: word = slot).  words = [(slot, start, end, acc, cum, state
    after the word)]; level_cost = [L_l or None]"""
    S, arcs, final = gram
    K = len(dis)
    lab = list(range(K)) if word_of_slot is None else [int(w) for w in word_of_slot]
    pairs = pairs_of(gram)
    none = [None] * (N + 1)
    E = [[e0(N, skip) if s == 0 else list(none) for s in range(S)]] + [[list(none) for _ in range(S)] for _ in range(max_words)]
    A = [None] + [[list(none) for _ in range(S)] for _ in range(max_words)]
    Cs = [None] + [{} for _ in range(max_words)]
    for l in range(1, max_words + 1):
        for (t, w), frm in pairs.items():
            C = [min((E[l - 1][s][x] for s in frm if E[l - 1][s][x] is not None), default=None) for x in range(N + 1)]
            Cs[l][(t, w)] = C
            if all(c is None for c in C[:N]):
                continue  # nothing starts: every end is unreachable
            for k in range(K):
                if lab[k] != w or dis[k] is None:
                    continue
                for x, v in enumerate(level(dis[k], C)):
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
    finals = [f for f in range(S) if final[f]]
    level_cost = [min((E[l][f][N] for f in finals if E[l][f][N] is not None), default=None) for l in range(1, max_words + 1)]
    n = n_exact
    if not n:
        finite = [(c, l + 1) for l, c in enumerate(level_cost) if c is not None]
        n = min(finite)[1] if finite else 1
    out = dict(status=CH_NONE, cost=None, n_words=0, skipped=0, words=[], level_cost=level_cost)
    if level_cost[n - 1] is None:
        return out
    p, t, words = N, min(f for f in finals if E[n][f][N] == level_cost[n - 1]), []
    for l in range(n, 0, -1):
        while A[l][t][p] is None or A[l][t][p][0] != E[l][t][p]:
            p -= 1
        cost, start, slot = A[l][t][p]
        C = Cs[l][(t, lab[slot])]
        words.append((slot, start, p - 1, cost - word_cost - C[start], E[l][t][p], t))
        p, t = start, min(s for s in pairs[(t, lab[slot])] if E[l - 1][s][start] == C[start])
    assert t == 0 and (skip is not None or p == 0)
    words.reverse()
    out.update(status=CH_OK, cost=level_cost[n - 1], n_words=n, words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def decode(gram, mfcc, frames, tm, tf, valid, max_frames, max_words, n_exact=0, skip=None, word_cost=0, word_of_slot=None,
           level=level_end_row):
    """chain_ref.decode under the grammar: the same three arrays, the state after each word in the word rows' `reserved`"""
    n_rows, K = len(mfcc), len(tm)
    rec = np.zeros(n_rows, CHAIN_REC_DTYPE)
    words = np.empty((n_rows, max_words), CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    lc = np.full((n_rows, max_words), DIS_ERR, np.uint32)
    for r in range(n_rows):
        N = min(int(frames[r]), max_frames)
        dis = [local_dis(mfcc[r, :N], tm[k, :int(tf[k])]) if (valid is None or valid[k]) and int(tf[k]) > 0 else None for k in range(K)]
        o = decode_row(gram, dis, N, max_words, n_exact, skip, word_cost, word_of_slot, level)
        lc[r] = [DIS_ERR if c is None else c for c in o["level_cost"]]
        if o["status"] != CH_OK:
            rec[r] = (DIS_ERR, 0, 0, CH_NONE)
            continue
        rec[r] = (o["cost"], o["n_words"], o["skipped"], CH_OK)
        for i, (slot, start, end, acc, cum, state) in enumerate(o["words"]):
            word = slot if word_of_slot is None else int(word_of_slot[slot])
            words[r, i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, state)
    return rec, words, lc


def accepted_sequences(gram, n):
    """every label sequence of exactly n words that leads from state 0 to a final state"""
    _, arcs, final = gram
    at = {(): {0}}
    for _ in range(n):
        nxt = {}
        for seq, states in at.items():
            for s, t, w in arcs:
                if s in states:
                    nxt.setdefault(seq + (w,), set()).add(t)
        at = nxt
    return sorted(seq for seq, states in at.items() if any(final[s] for s in states))


def enumerate_cost(gram, dis, N, n, skip=None, word_cost=0, word_of_slot=None):
    """L_n the long way: per accepted label sequence of length n the unconstrained chain with only that position's slots at
    each level (prefixes shared between sequences are computed once), and the minimum over the sequences; None = no parse"""
    K = len(dis)
    lab = list(range(K)) if word_of_slot is None else [int(w) for w in word_of_slot]
    memo = {(): e0(N, skip)}

    def prefix(seq):
        if seq not in memo:
            prev, A = prefix(seq[:-1]), [None] * (N + 1)
            for k in range(K):
                if lab[k] == seq[-1] and dis[k] is not None:
                    for x, v in enumerate(level_end_row(dis[k], prev)):
                        if v != INF and (A[x + 1] is None or v[0] + word_cost < A[x + 1]):
                            A[x + 1] = v[0] + word_cost
            E = [None] * (N + 1)
            for p in range(1, N + 1):
                E[p] = A[p]
                if skip is not None and E[p - 1] is not None and (E[p] is None or E[p - 1] + skip < E[p]):
                    E[p] = E[p - 1] + skip
            memo[seq] = E
        return memo[seq]

    return min((c for c in (prefix(seq)[N] for seq in accepted_sequences(gram, n)) if c is not None), default=None)


planted = chain_ref.planted
