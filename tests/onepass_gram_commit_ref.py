"""The commit rule of a live one-pass grammar session (include/sr_engine.h, "live one-pass grammar decoding", COMMITTED WORDS,
sr_onepass_gram_live_commit) restated in plain Python over (A, E, N, W, gram, kept states), A and E as onepass_gram_ref builds
them: which words every parse a recording can still get begins with, whatever is heard later.

  kept         the grammar's static lists (onepass_gram_ref.kept): the kept states the rule ranges over, the kept items W is of
  hit(q, t)    q >= 1, A(q, t) reachable and A(q, t).cost == E(q, t): a word into t ends at q - 1 and closes E there
  node         (q, t) with t kept and hit(q, t); or the root (0, 0)
  end(p, t)    the node (q, t) with the largest q <= p, the root if state t has none: where onepass_gram_ref.trace_row, at p in
               state t, finds its first word
  parent       of (q, t), whose word starts at x with source state s (the smallest state of the charge list that carries the
               charge, as the trace defines it): end(x, s)
  walk(p, t)   end(p, t), its parent, ... down to the root
  W            2 * max M_k - 1 over the slots of the kept items, 0 if none are kept
  entries(N)   the (x, s), s kept, x in [max(0, N - W), N], with E(x, s) reachable; none: every reachable (x, s) at the largest
               x <= N that has one
  c(N)         the deepest node shared by the walks from all entries -- by SET INTERSECTION here; shared nodes lie on one chain
               and a walk holds one node per position, so the deepest is the one at the largest position
  Tree         hit, end, walk, commit_node and committed of ONE history, with the word of a node worked out once
  Cursor       what a session delivers call by call: the committed words not yet delivered, words_cap at a time
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import onepass_gram_ref as gref
import onepass_ref as ref
import wgram_ref
from onepass_commit_ref import COMMIT_REC_DTYPE
from onepass_ref import CHAIN_WORD_DTYPE, NO_WORD_ROW

ROOT = (0, 0)


def window(gram, tf, word_of_slot, valid=None):
    """W from the kept items of the grammar over a store with frame counts tf"""
    items, _ = gref.kept(gram, [int(w) for w in word_of_slot], valid)
    lens = [int(tf[k]) for k, _ in items]
    return 2 * max(lens) - 1 if lens else 0


def kept_states(gram, word_of_slot, valid=None):
    return gref.kept(gram, [int(w) for w in word_of_slot], valid)[1]


def hit(A, E, q, t):
    return q >= 1 and A[t][q] is not None and A[t][q][0] == E[t][q]


def end(A, E, p, t):
    while p > 0 and not hit(A, E, p, t):
        p -= 1
    return (p, t) if p else ROOT


class Tree:
    """the nodes of one history under one grammar.  A walk never changes (A and E at p depend on frames < p only), so the
    parent of a node is worked out once, whatever N the rule is asked at"""

    def __init__(self, A, E, gram, word_cost=0, word_of_slot=None):
        self.A, self.E, self.gram, self.word_cost, self.word_of_slot = A, E, gram, word_cost, word_of_slot
        self.lists = wgram_ref.lists_of(gram)
        self._word = {}

    def word_at(self, node):
        """the word of a node other than the root -> ((slot, start, end, acc, cum, state after the word), (start, source))"""
        if node not in self._word:
            q, t = node
            cost, start, slot = self.A[t][q]
            lst = self.lists[(t, slot if self.word_of_slot is None else int(self.word_of_slot[slot]))]
            c = gref.charge(self.E, lst, start)
            src = min(s for s, ac in lst if wgram_ref._plus(self.E[s][start], ac, False) == c)
            self._word[node] = (slot, start, q - 1, cost - self.word_cost - c, self.E[t][q], t), (start, src)
        return self._word[node]

    def parent(self, node):
        return end(self.A, self.E, *self.word_at(node)[1])

    def walk(self, p, t):
        """the nodes from end(p, t) down, the root included"""
        node, out = end(self.A, self.E, p, t), []
        while node != ROOT:
            out.append(node)
            node = self.parent(node)
        return out + [ROOT]

    def commit_node(self, N, W, states):
        shared = None
        for x, s in entries(self.A, self.E, N, W, states)[0]:
            nodes = set(self.walk(x, s))
            shared = nodes if shared is None else shared & nodes
        if shared is None:
            return ROOT
        deepest = max(q for q, _ in shared)
        at = [n for n in shared if n[0] == deepest]
        assert len(at) == 1  # a walk holds one node per position
        return at[0]

    def committed(self, N, W, states):
        """-> (c(N) as (position, state), the committed words [(slot, start, end, acc, cum, state)] in spoken order, as
        onepass_gram_ref.trace_row writes them)"""
        c = self.commit_node(N, W, states)
        return c, [self.word_at(n)[0] for n in self.walk(*c)[:-1]][::-1]


def walk(A, E, gram, p, t, word_of_slot=None):
    return Tree(A, E, gram, 0, word_of_slot).walk(p, t)


def entries(A, E, N, W, states):
    """-> (the entries [(x, s)], whether the window held none)"""
    inside = [(x, s) for s in states for x in range(max(0, N - W), N + 1) if E[s][x] is not None]
    if inside:
        return inside, False
    below = [(x, s) for s in states for x in range(N + 1) if E[s][x] is not None]
    last = max((x for x, _ in below), default=None)
    return [(x, s) for x, s in below if x == last], True  # none at all: state 0 is not kept, nothing parses


def commit_node(A, E, N, W, gram, states, word_of_slot=None):
    return Tree(A, E, gram, 0, word_of_slot).commit_node(N, W, states)


def committed(A, E, N, W, gram, states, word_cost=0, word_of_slot=None):
    return Tree(A, E, gram, word_cost, word_of_slot).committed(N, W, states)


def word_rows(words, tf, words_cap, word_of_slot=None):
    out = np.empty(words_cap, CHAIN_WORD_DTYPE)
    out[...] = NO_WORD_ROW
    for i, (slot, start, last, acc, cum, state) in enumerate(words):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        out[i] = (word, slot, start, last, acc, acc // (last - start + 1 + int(tf[slot])), cum, state)
    return out


class Cursor:
    """the delivery of one channel's committed words over the commit calls of a recording; node = the last delivered word's
    node with its state"""

    def __init__(self, words_cap):
        self.words_cap, self.first, self.node = words_cap, 0, ROOT

    def reset(self):
        self.first, self.node = 0, ROOT

    def take(self, c, words, tf, word_of_slot=None):
        """c, words = committed(...) at the channel's N -> (rec COMMIT_REC_DTYPE [], rows CHAIN_WORD_DTYPE [words_cap], the
        delivered words)"""
        assert len(words) >= self.first
        if self.first:  # what was delivered stays where it was: the cursor's node is on the walk from c
            w = words[self.first - 1]
            assert (w[2] + 1, w[5]) == self.node, (w, self.node)
        n_new = min(len(words) - self.first, self.words_cap)
        new = words[self.first:self.first + n_new]
        rec = np.zeros((), COMMIT_REC_DTYPE)
        rec[()] = (len(words), self.first, n_new, c[0])
        self.first += n_new
        if new:
            self.node = (new[-1][2] + 1, new[-1][5])
        return rec, word_rows(new, tf, self.words_cap, word_of_slot), new


def history_with_starts(gram, dis, N, skip=None, word_cost=0, word_of_slot=None, keep=None):
    """onepass_gram_ref.history_sync with, per frame x, the starts of every hypothesis alive in the exact column x (either
    state, any row of any item; keep: of the items (slot, target) in it only, which are also the only ones swept then)
    -> (A, E, starts [N] of sets)"""
    S = gram[0]
    items = [it for it in gref.items_of(gram, dis, word_of_slot) if keep is None or (it[0], it[1]) in keep]
    A, E = gref._empty(S, N)
    cols, starts = [None] * len(items), []
    for x in range(N):
        alive = set()
        for i, (k, t, lst) in enumerate(items):
            cols[i] = ref._column(dis[k][x], cols[i], gref.charge(E, lst, x), x)
            ref._send(A[t], x + 1, cols[i][1][-1], word_cost, k)
            alive |= {v[1] for state in cols[i] for v in state if v != ref.INF}
        for t in range(S):
            ref._close(A[t], E[t], x, x + 1, skip)
        starts.append(alive)
    return A, E, starts
