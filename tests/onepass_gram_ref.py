"""One-pass grammar decoding (include/sr_engine.h, "one-pass grammar decoding") restated in plain Python: onepass_ref's ONE
prefix-cost array, kept per state of a weighted grammar (wgram_ref's notation: states 0..S-1, state 0 the start, the charge
list of a pair (t, w), final_cost).  Everything not restated is onepass_ref's: d, the word path, skip_cost, word_cost, the key
(cost, start, slot), the records, CH_TRUNCATED.

  E(0, 0)   0; E(0, s) unreachable for s != 0
  charge    C(x; t, w) = min over the (s, c) of the list of (t, w) with E(x, s) reachable of E(x, s) + c; else unreachable.  An
            unreachable E never has a cost added to it
  D_k,t     per item (slot k, target t), k a valid slot of a word w with a pair (t, w): the spotter's recurrence with a charged
            start, D(x, 0) = C(x; t, w) + d(x, 0), S = x
  A(p, t)   min over the items into t of (D_k,t(p-1, M_k-1) + word_cost, S, k), compared as (cost, start, slot)       (p >= 1)
  E(p, t)   min(A(p, t).cost, E(p-1, t) + skip_cost), the second term only when skipping is on
  result    over the final f with E(N, f) reachable: cost = min E(N, f) + final_cost[f], end state the smallest such f; none,
            or N = 0: CH_NONE
  trace     p = N, t = end state; while p > 0: A(p, t) unreachable or A(p, t).cost != E(p, t): p -= 1; else word = A(p, t),
            end = p-1, cum = E(p, t), acc = cost - word_cost - C(start; t, w(k)), reserved = t; the source state is the smallest
            s of the list with E(start, s) reachable and E(start, s) + c = C(start; t, w(k)); p = start, t = s

The arrays are stated two ways, compared with each other by tests/test_onepass_gram_ref.py:
  history_sync    time-synchronous: per frame one column of every item, then E of every state;
  history_blocks  what the kernels do: onepass_ref.history_blocks' blocks of n <= L frames, per item.
wrap=True drops the guard of the charge on purpose (wgram_ref's: all ones + c wraps to c - 1) and exists only so that a test
can prove it looks at a case where the guard matters.  grammar_repeat() restates the builder of the Python interface.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import onepass_ref
import wgram_ref
from chain_ref import CH_NONE, CH_OK, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, NO_WORD_ROW  # noqa: F401  (re-exported)
from onepass_ref import CH_TRUNCATED, _close, _column, _send, planted_long, reach  # noqa: F401  (re-exported)
from spot_ref import DIS_ERR
from wgram_ref import costs_of, lists_of

COST_SUM = 1 << 30


def grammar_repeat(positions, loop_labels, min_repeat=1):
    """a sequence followed by a loop: position i takes one label of positions[i] (state i -> i + 1), then at least min_repeat
    words of loop_labels; the first min_repeat of them advance a state each, the last of these states is final and loops on
    every loop label (min_repeat 0: the state after the sequence is final and loops) -> (n_states, arcs, final)"""
    n, loop = len(positions), list(dict.fromkeys(int(w) for w in loop_labels))
    arcs = [(i, i + 1, int(w)) for i, ws in enumerate(positions) for w in dict.fromkeys(ws)]
    arcs += [(n + j, n + j + 1, w) for j in range(min_repeat) for w in loop]
    last = n + min_repeat
    arcs += [(last, last, w) for w in loop]
    return last + 1, arcs, [int(s == last) for s in range(last + 1)]


def cost_ok(cap, L, word_cost, gram):
    """(cap / L) x (word_cost + the largest arc cost) + the largest final cost <= 2^30"""
    ac, fc = costs_of(gram)
    return not L or (cap // L) * (word_cost + max(ac, default=0)) + max(fc, default=0) <= COST_SUM


def items_of(gram, dis, word_of_slot=None):
    """[(slot, target, charge list)]: per pair (t, w) every usable slot of w"""
    lab = list(range(len(dis))) if word_of_slot is None else [int(w) for w in word_of_slot]
    return [(k, t, lst) for (t, w), lst in lists_of(gram).items() for k in range(len(dis)) if lab[k] == w and dis[k] is not None]


def charge(E, lst, x, wrap=False):
    """C(x; t, w) over the charge list, None = unreachable"""
    return wgram_ref.charge(E, lst, x, wrap)


def _empty(S, N):
    A = [[None] * (N + 1) for _ in range(S)]
    E = [[None] * (N + 1) for _ in range(S)]
    E[0][0] = 0
    return A, E


def history_sync(gram, dis, N, skip=None, word_cost=0, word_of_slot=None, wrap=False):
    """dis per slot int64 [N, M_k] or None -> (A, E): A[t][p] = (cost, start, slot) or None, E[t][p] = cost or None"""
    S = gram[0]
    items = items_of(gram, dis, word_of_slot)
    A, E = _empty(S, N)
    cols = [None] * len(items)
    for x in range(N):
        for i, (k, t, lst) in enumerate(items):
            cols[i] = _column(dis[k][x], cols[i], charge(E, lst, x, wrap), x)
            _send(A[t], x + 1, cols[i][1][-1], word_cost, k)
        for t in range(S):
            _close(A[t], E[t], x, x + 1, skip)
    return A, E


def history_blocks(gram, dis, N, n, skip=None, word_cost=0, word_of_slot=None, cap=None, wrap=False):
    """the block form with blocks of n frames over cap >= N frames (the host's bound; default N)"""
    cap = N if cap is None else cap
    assert n >= 1 and cap >= N
    S = gram[0]
    items = items_of(gram, dis, word_of_slot)
    A, E = _empty(S, N)
    saved = [None] * len(items)  # per item the exact column at the previous block's c0
    for c0 in range(0, cap, n):
        if N <= c0:
            break
        cN = min(c0 + n, cap, N)
        for i, (k, t, lst) in enumerate(items):
            col = saved[i]
            for x in range(c0 - n + 1 if c0 else 0, cN):
                col = _column(dis[k][x], col, charge(E, lst, x, wrap) if x <= c0 else None, x)
                if x == c0:
                    saved[i] = col
                if x >= c0:
                    _send(A[t], x + 1, col[1][-1], word_cost, k)
        for t in range(S):
            _close(A[t], E[t], c0, cN, skip)
    return A, E


def trace_row(A, E, N, gram, word_cost=0, word_of_slot=None, wrap=False):
    """-> dict(status, cost, n_words, skipped, state, words = [(slot, start, end, acc, cum, state after the word)])"""
    S, _, final = gram[:3]
    _, fc = costs_of(gram)
    lists = lists_of(gram)
    out = dict(status=CH_NONE, cost=None, n_words=0, skipped=0, state=None, words=[])
    ends = [(E[f][N] + fc[f], f) for f in range(S) if final[f] and E[f][N] is not None] if N else []
    if not ends:
        return out
    total, t = min(ends)
    p, words = N, []
    while p > 0:
        if E[t][p] is None:
            assert wrap  # only the unguarded sum walks into a state that was never reached
            break
        if A[t][p] is None or A[t][p][0] != E[t][p]:
            p -= 1
            continue
        cost, start, slot = A[t][p]
        lst = lists[(t, slot if word_of_slot is None else int(word_of_slot[slot]))]
        c = charge(E, lst, start, wrap)
        words.append((slot, start, p - 1, cost - word_cost - c, E[t][p], t))
        p, t = start, min(s for s, ac in lst if wgram_ref._plus(E[s][start], ac, wrap) == c)
    assert wrap or t == 0
    words.reverse()
    out.update(status=CH_OK, cost=total, n_words=len(words), words=words, state=min(ends)[1],
               skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def decode_row(gram, dis, N, skip=None, word_cost=0, word_of_slot=None, block=0, wrap=False):
    A, E = (history_blocks(gram, dis, N, block, skip, word_cost, word_of_slot, None, wrap) if block else
            history_sync(gram, dis, N, skip, word_cost, word_of_slot, wrap))
    return trace_row(A, E, N, gram, word_cost, word_of_slot, wrap)


def decode(gram, mfcc, frames, tm, tf, valid, max_frames, words_cap, skip=None, word_cost=0, word_of_slot=None, frames_cap=0, block=0):
    """onepass_ref.decode under the grammar: (rec CHAIN_REC_DTYPE [n_rows], words CHAIN_WORD_DTYPE [n_rows, words_cap]), the
    state after each word in the word rows' `reserved`"""
    n_rows = len(mfcc)
    cap = min(max_frames, frames_cap) if frames_cap else max_frames
    if not cost_ok(cap, reach(tf, valid), word_cost, gram):
        raise ValueError("(frames_cap / L) * (word_cost + arc cost) + final cost exceeds 2^30")
    rec = np.zeros(n_rows, CHAIN_REC_DTYPE)
    words = np.empty((n_rows, words_cap), CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    for r in range(n_rows):
        N = min(int(frames[r]), cap)
        o = decode_row(gram, wgram_ref.slot_distances(mfcc[r, :N], tm, tf, valid), N, skip, word_cost, word_of_slot, block)
        if o["status"] != CH_OK:
            rec[r] = (DIS_ERR, 0, 0, CH_NONE)
            continue
        rec[r] = (o["cost"], o["n_words"], o["skipped"], CH_TRUNCATED if o["n_words"] > words_cap else CH_OK)
        for i, (slot, start, end, acc, cum, state) in enumerate(o["words"][:words_cap]):
            word = slot if word_of_slot is None else int(word_of_slot[slot])
            words[r, i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, state)
    return rec, words


# ---- the static pruning of sr_onepass_gram_plan.h, restated ----------------------------------------------------------------------
def kept(gram, word_of_slot, valid=None):
    """(kept items [(slot, target)] ascending, kept states ascending): an item is kept when its charge list names a state
    reachable from state 0 in any number of arcs and its target reaches a final state; a state when a kept charge list names
    it or when it is final and reachable"""
    S, arcs, final = gram[:3]
    fwd = {0}
    while True:
        more = fwd | {t for s, t, _ in arcs if s in fwd}
        if more == fwd:
            break
        fwd = more
    back = {s for s in range(S) if final[s]}
    while True:
        more = back | {s for s, t, _ in arcs if t in back}
        if more == back:
            break
        back = more
    items, states = [], {s for s in fwd if final[s]}
    for (t, w), lst in lists_of(gram).items():
        if not ({s for s, _ in lst} & fwd) or t not in back:
            continue
        slots = [k for k, lab in enumerate(word_of_slot) if lab == w and (valid is None or valid[k])]
        items += [(k, t) for k in slots]
        if slots:
            states |= {s for s, _ in lst}
    return sorted(items), sorted(states)
