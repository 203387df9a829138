"""The commit rule of a live one-pass session (include/sr_engine.h, "live one-pass connected-word decoding", sr_onepass_live_commit)
restated in plain Python over (A, E, N, W), A and E as onepass_ref builds them: which words of the parse at N frames can no
longer change, whatever is heard later.

  hit(q)       q >= 1, A(q) reachable and A(q).cost == E(q): a word ends at q - 1 and closes E there
  end(p)       the largest q <= p with hit(q), or 0: where onepass_ref.trace_row, started at p, finds its first word
  walk(p)      end(p) -> end(start(A(end(p)))) -> ... -> 0: the nodes of the words trace_row would write from p.  A(p) and E(p)
               depend on frames < p only, so the walk from a position never changes
  W            2 * max_k M_k - 1 over the valid slots (0: no valid slot): a word over M template frames covers at most 2M - 1
               input frames, so every hypothesis alive in column N - 1 started at or after N - W
  entries(N)   the positions x in [max(0, N - W), N] where E(x) is reachable; if there are none, the largest reachable x <= N
  c(N)         the deepest node shared by the walks from all entries; the committed words are those on the walk from c(N)
  Cursor       what a session delivers call by call: the committed words not yet delivered, words_cap at a time
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import onepass_ref as ref
from onepass_ref import CHAIN_WORD_DTYPE, NO_WORD_ROW

COMMIT_REC_DTYPE = np.dtype([("n_committed", "<u4"), ("first", "<u4"), ("n_new", "<u4"), ("frames", "<u4")])
assert COMMIT_REC_DTYPE.itemsize == 16


def window(tf, valid=None):
    lens = [int(m) for k, m in enumerate(tf) if int(m) > 0 and (valid is None or valid[k])]
    return 2 * max(lens) - 1 if lens else 0


def hit(A, E, q):
    return q >= 1 and A[q] is not None and A[q][0] == E[q]


def end(A, E, p):
    while p > 0 and not hit(A, E, p):
        p -= 1
    return p


def walk(A, E, p):
    """the nodes from end(p) down, the final 0 included"""
    q, out = end(A, E, p), []
    while q:
        out.append(q)
        q = end(A, E, A[q][1])
    return out + [0]


def entries(A, E, N, W):
    """-> (the entry positions, whether the window held none)"""
    xs = [x for x in range(max(0, N - W), N + 1) if E[x] is not None]
    if xs:
        return xs, False
    return [max(x for x in range(N + 1) if E[x] is not None)], True  # E(0) = 0 is always reachable


def commit_node(A, E, N, W):
    shared = None
    for x in entries(A, E, N, W)[0]:
        nodes = set(walk(A, E, x))
        shared = nodes if shared is None else shared & nodes
    return max(shared)  # a node's ancestors are all below it: the deepest shared node is the largest


def committed(A, E, N, W, word_cost=0):
    """-> (c(N), the committed words [(slot, start, end, acc, cum)] in spoken order, as onepass_ref.trace_row writes them)"""
    c = commit_node(A, E, N, W)
    words = []
    for q in walk(A, E, c)[:-1]:
        cost, start, slot = A[q]
        words.append((slot, start, q - 1, cost - word_cost - E[start], E[q]))
    return c, words[::-1]


def walks_below_window(A, E, N, W):
    """the nodes q inside the window whose word starts below it, over all entry walks: where a walk leaves the window"""
    lo, out = max(0, N - W), set()
    for x in entries(A, E, N, W)[0]:
        for q in walk(A, E, x)[:-1]:
            if q >= lo and A[q][1] < lo:
                out.add(q)
    return sorted(out)


def landings(A, E, N, W):
    """per entry walk the first node below the window: where the walks land once they have left it"""
    lo = max(0, N - W)
    return {next(q for q in walk(A, E, x) if q < lo or q == 0) for x in entries(A, E, N, W)[0]}


def word_rows(words, tf, words_cap, word_of_slot=None):
    out = np.empty(words_cap, CHAIN_WORD_DTYPE)
    out[...] = NO_WORD_ROW
    for i, (slot, start, last, acc, cum) in enumerate(words):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        out[i] = (word, slot, start, last, acc, acc // (last - start + 1 + int(tf[slot])), cum, 0)
    return out


class Cursor:
    """the delivery of one channel's committed words over the commit calls of a recording"""

    def __init__(self, words_cap):
        self.words_cap, self.first = words_cap, 0

    def reset(self):
        self.first = 0

    def take(self, c, words, tf, word_of_slot=None):
        """c, words = committed(...) at the channel's N -> (rec COMMIT_REC_DTYPE [], rows CHAIN_WORD_DTYPE [words_cap], the
        delivered words)"""
        assert len(words) >= self.first
        n_new = min(len(words) - self.first, self.words_cap)
        new = words[self.first:self.first + n_new]
        rec = np.zeros((), COMMIT_REC_DTYPE)
        rec[()] = (len(words), self.first, n_new, c)
        self.first += n_new
        return rec, word_rows(new, tf, self.words_cap, word_of_slot), new


def history_with_starts(dis, N, skip=None, word_cost=0):
    """onepass_ref.history_sync with, per frame x, the starts of every hypothesis alive in the exact column x (either state, any
    row of any slot) -> (A, E, starts [N] of sets)"""
    A, E = [None] * (N + 1), [0] + [None] * N
    cols, starts = [None] * len(dis), []
    for x in range(N):
        alive = set()
        for k, d in enumerate(dis):
            if d is None:
                continue
            cols[k] = ref._column(d[x], cols[k], E[x], x)
            ref._send(A, x + 1, cols[k][1][-1], word_cost, k)
            alive |= {v[1] for state in cols[k] for v in state if v != ref.INF}
        ref._close(A, E, x, x + 1, skip)
        starts.append(alive)
    return A, E, starts
