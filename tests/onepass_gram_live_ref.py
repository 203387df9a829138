"""Live one-pass grammar decoding (include/sr_engine.h, "live one-pass grammar decoding") restated in plain Python on top of
onepass_gram_ref and onepass_live_ref: the block form over the states of a grammar with the boundaries set by the pushes, and
the parse of every prefix of a recording from ONE history.

  history_pushes   onepass_gram_ref.history_blocks with per-block c0_prev: every push cut into blocks of at most L frames
                   (onepass_live_ref.cut_blocks), the first block of a push resuming from the columns saved at the first frame
                   of the last block of the push before.  tests/test_onepass_gram_live_ref.py holds it equal to
                   onepass_gram_ref.history_sync for every chunking.
  prefix property  A(p, t) and E(p, t) depend on frames < p only, so the history of a recording is a prefix of that of any
                   longer one, and onepass_gram_ref.trace_row at N gives the row a session emits when a channel stands at N.
  to_records       that row as the library writes it: the first words_cap words, or (tail) the last; the grammar state after
                   each word in `reserved`.
  Recording        a channel's history built once (history_sync), a row per N.
  Channel          a push as the device runs it: per block every item swept from its saved column with
                   onepass_gram_ref.charge, then every state closed.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import onepass_gram_ref as gref
import onepass_ref as ref
from onepass_live_ref import CHAIN_LIVE_ROW_DTYPE, MAX_FRAMES, cut_blocks, pcm_frames, slot_distances  # noqa: F401  (re-exported)
from onepass_ref import CH_NONE, CH_OK, CH_TRUNCATED, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, DIS_ERR, NO_WORD_ROW  # noqa: F401


class Channel:
    """one channel of a session, step by step as the device runs a push: per block [c0, cN) every item's columns (c0_prev, cN)
    swept from the saved exact column at c0_prev -- the charge of the item's list for col <= c0, nothing behind c0 -- column c0
    saved, the ends of the columns >= c0 sent to A(col + 1, target); then E of every state closed over (c0, cN].  dis_chunk
    arrives push by push; the channel keeps the distances of what it has heard (the device keeps the feature row)."""

    def __init__(self, gram, n_slots, L, skip=None, word_cost=0, word_of_slot=None, wrap=False):
        self.gram, self.L, self.skip, self.word_cost, self.word_of_slot, self.wrap = gram, L, skip, word_cost, word_of_slot, wrap
        self.S = gram[0]
        self.N, self.c0_prev = 0, 0
        self.A, self.E = gref._empty(self.S, 0)
        self.dis = [None] * n_slots
        self.items = None  # fixed by the first push: the usable slots are the store's
        self.saved = None

    def push(self, dis_chunk, block=None):
        """dis_chunk: per slot the local distances int64 [n, M_k] of the n new frames, None for an invalid slot; block: frames
        per block of this push, 1..L (default L) -> the parse of everything pushed so far (onepass_gram_ref.trace_row's dict)"""
        block = self.L if block is None else block
        assert 1 <= block <= max(self.L, 1)
        n = next((len(d) for d in dis_chunk if d is not None), 0)
        for k, d in enumerate(dis_chunk):
            if d is not None:
                self.dis[k] = d if self.dis[k] is None else np.concatenate([self.dis[k], d])
        if self.items is None:
            self.items = gref.items_of(self.gram, dis_chunk, self.word_of_slot)
            self.saved = [None] * len(self.items)
        for t in range(self.S):
            self.A[t] += [None] * n
            self.E[t] += [None] * n
        for c0, cN in cut_blocks(self.N, n, block):
            for i, (k, t, lst) in enumerate(self.items):
                col = self.saved[i]
                for x in range(self.c0_prev + 1 if c0 else 0, cN):
                    col = ref._column(self.dis[k][x], col, gref.charge(self.E, lst, x, self.wrap) if x <= c0 else None, x)
                    if x == c0:
                        self.saved[i] = col
                    if x >= c0:
                        ref._send(self.A[t], x + 1, col[1][-1], self.word_cost, k)
            for t in range(self.S):
                ref._close(self.A[t], self.E[t], c0, cN, self.skip)
            self.c0_prev = c0
        self.N += n
        return gref.trace_row(self.A, self.E, self.N, self.gram, self.word_cost, self.word_of_slot, self.wrap)


def history_pushes(gram, dis, N, cuts, L, skip=None, word_cost=0, block=None, word_of_slot=None, wrap=False):
    """dis as onepass_gram_ref.history_sync takes it; cuts: the pushes' frame counts, which sum to N (zeros allowed); every push
    is cut into blocks of at most `block` <= L frames (default L) -> (A, E)"""
    assert sum(cuts) == N
    ch = Channel(gram, len(dis), L, skip, word_cost, word_of_slot, wrap)
    at = 0
    for n in cuts:
        ch.push([None if d is None else d[at:at + n] for d in dis], block)
        at += n
    return ch.A, ch.E


def to_records(o, tf, words_cap, tail=False, word_of_slot=None):
    """onepass_gram_ref.trace_row's dict -> (rec CHAIN_REC_DTYPE [], words CHAIN_WORD_DTYPE [words_cap])"""
    rec = np.zeros((), CHAIN_REC_DTYPE)
    words = np.empty(words_cap, CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    if o["status"] != CH_OK:
        rec[()] = (DIS_ERR, 0, 0, CH_NONE)
        return rec, words
    rec[()] = (o["cost"], o["n_words"], o["skipped"], CH_TRUNCATED if o["n_words"] > words_cap else CH_OK)
    shown = o["words"][-words_cap:] if tail else o["words"][:words_cap]
    for i, (slot, start, end, acc, cum, state) in enumerate(shown):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        words[i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, state)
    return rec, words


class Recording:
    """everything pushed to a channel under a grammar, its history built once (time-synchronous); row(N) = the records a
    session emits when the channel stands at N frames"""

    def __init__(self, gram, feat, tm, tf, valid, words_cap, skip=None, word_cost=0, tail=False, word_of_slot=None, wrap=False):
        self.gram, self.N, self.tf, self.words_cap, self.word_cost = gram, len(feat), tf, words_cap, word_cost
        self.tail, self.word_of_slot, self.wrap = tail, word_of_slot, wrap
        self.dis = slot_distances(feat, tm, tf, valid)
        self.A, self.E = gref.history_sync(gram, self.dis, self.N, skip, word_cost, word_of_slot, wrap)
        self._rows = {}

    def parse(self, N):
        assert 0 <= N <= self.N
        return gref.trace_row(self.A, self.E, N, self.gram, self.word_cost, self.word_of_slot, self.wrap)

    def row(self, N, words_cap=None, tail=None):
        """words_cap / tail None: the recording's own; the history depends on neither"""
        key = (N, self.words_cap if words_cap is None else words_cap, self.tail if tail is None else tail)
        if key not in self._rows:
            self._rows[key] = to_records(self.parse(N), self.tf, key[1], key[2], self.word_of_slot)
        return self._rows[key]
