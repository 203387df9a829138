"""Live one-pass connected-word decoding (include/sr_engine.h, "live one-pass connected-word decoding") restated in plain
Python on top of onepass_ref: the block form with the boundaries set by the pushes, and the parse of every prefix of a
recording from ONE history.

  cut_blocks       a push of n frames behind x0 as blocks of at most `block` frames: [(c0, cN)].
  history_pushes   onepass_ref.history_blocks with per-block c0_prev: every push cut into blocks of at most L frames, the first
                   block of a push resuming from the column saved at the first frame of the last block of the push before.
                   tests/test_onepass_live_ref.py holds it equal to onepass_ref.history_sync for every chunking.
  prefix property  A(p) and E(p) depend on frames < p only, so the history of a recording is a prefix of that of any longer
                   one, and onepass_ref.trace_row at N gives the row a session emits when a channel stands at N frames.
  to_records       that row as the library writes it: the first words_cap words, or (tail) the last -- words[-words_cap:].
  Recording        a channel's history built once (history_sync), a row per N.
  Channel          a push as the device runs it: per block the sweep of every slot from its saved column, then the close.
Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import onepass_ref as ref
from onepass_ref import CH_NONE, CH_OK, CH_TRUNCATED, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, DIS_ERR, NO_WORD_ROW, local_dis

CHAIN_LIVE_ROW_DTYPE = np.dtype([("channel", "<u4"), ("frames", "<u4")])
MAX_FRAMES = 16383  # utt_frames at most: the u32 cost bound and the start field of a key end there


def cut_blocks(x0, n, block):
    assert block >= 1
    return [(c0, min(c0 + block, x0 + n)) for c0 in range(x0, x0 + n, block)]


class Channel:
    """one channel of a session, step by step as the device runs a push: per block [c0, cN) every slot's columns (c0_prev, cN)
    swept from the saved exact column at c0_prev -- E(col) charged for col <= c0, nothing behind c0 -- column c0 saved, the ends
    of the columns >= c0 sent to A(col + 1); then E closed over (c0, cN].  dis_chunk arrives push by push; the channel keeps
    the distances of what it has heard (the device keeps the feature row)."""

    def __init__(self, n_slots, L, skip=None, word_cost=0):
        self.L, self.skip, self.word_cost = L, skip, word_cost
        self.N, self.c0_prev = 0, 0
        self.A, self.E = [None], [0]
        self.saved = [None] * n_slots
        self.dis = [None] * n_slots

    def push(self, dis_chunk, block=None):
        """dis_chunk: per slot the local distances int64 [n, M_k] of the n new frames, None for an invalid slot; block: frames
        per block of this push, 1..L (default L) -> the parse of everything pushed so far (onepass_ref.trace_row's dict)"""
        block = self.L if block is None else block
        assert 1 <= block <= max(self.L, 1)
        n = next((len(d) for d in dis_chunk if d is not None), 0)
        for k, d in enumerate(dis_chunk):
            if d is not None:
                self.dis[k] = d if self.dis[k] is None else np.concatenate([self.dis[k], d])
        self.A += [None] * n
        self.E += [None] * n
        for c0, cN in cut_blocks(self.N, n, block):
            for k, d in enumerate(self.dis):
                if d is None:
                    continue
                col = self.saved[k]
                for x in range(self.c0_prev + 1 if c0 else 0, cN):
                    col = ref._column(d[x], col, self.E[x] if x <= c0 else None, x)
                    if x == c0:
                        self.saved[k] = col
                    if x >= c0:
                        ref._send(self.A, x + 1, col[1][-1], self.word_cost, k)
            ref._close(self.A, self.E, c0, cN, self.skip)
            self.c0_prev = c0
        self.N += n
        return ref.trace_row(self.A, self.E, self.N, self.word_cost)


def history_pushes(dis, N, cuts, L, skip=None, word_cost=0, block=None):
    """dis as onepass_ref.history_sync takes it; cuts: the pushes' frame counts, which sum to N (zeros allowed); every push is cut
    into blocks of at most `block` <= L frames (default L) -> (A, E)"""
    assert sum(cuts) == N
    ch = Channel(len(dis), L, skip, word_cost)
    at = 0
    for n in cuts:
        ch.push([None if d is None else d[at:at + n] for d in dis], block)
        at += n
    return ch.A, ch.E


def to_records(o, tf, words_cap, tail=False, word_of_slot=None):
    """onepass_ref.trace_row's dict -> (rec CHAIN_REC_DTYPE [], words CHAIN_WORD_DTYPE [words_cap])"""
    rec = np.zeros((), CHAIN_REC_DTYPE)
    words = np.empty(words_cap, CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    if o["status"] != CH_OK:
        rec[()] = (DIS_ERR, 0, 0, CH_NONE)
        return rec, words
    rec[()] = (o["cost"], o["n_words"], o["skipped"], CH_TRUNCATED if o["n_words"] > words_cap else CH_OK)
    shown = o["words"][-words_cap:] if tail else o["words"][:words_cap]
    for i, (slot, start, end, acc, cum) in enumerate(shown):
        word = slot if word_of_slot is None else int(word_of_slot[slot])
        words[i] = (word, slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, 0)
    return rec, words


def slot_distances(feat, tm, tf, valid=None):
    """feat int16 [N, 12] -> per slot the local distances, None for an invalid slot (onepass_ref.decode's rule)"""
    return [local_dis(feat, tm[k, :int(tf[k])]) if (valid is None or valid[k]) and int(tf[k]) > 0 else None for k in range(len(tm))]


class Recording:
    """everything pushed to a channel, its history built once (time-synchronous); row(N) = the records a session emits when the
    channel stands at N frames"""

    def __init__(self, feat, tm, tf, valid, words_cap, skip=None, word_cost=0, tail=False, word_of_slot=None):
        self.N, self.tf, self.words_cap, self.word_cost, self.tail, self.word_of_slot = len(feat), tf, words_cap, word_cost, tail, word_of_slot
        self.A, self.E = ref.history_sync(slot_distances(feat, tm, tf, valid), self.N, skip, word_cost)
        self._rows = {}

    def parse(self, N):
        assert 0 <= N <= self.N
        return ref.trace_row(self.A, self.E, N, self.word_cost)

    def row(self, N, words_cap=None, tail=None):
        """words_cap / tail None: the recording's own; the history depends on neither"""
        key = (N, self.words_cap if words_cap is None else words_cap, self.tail if tail is None else tail)
        if key not in self._rows:
            self._rows[key] = to_records(self.parse(N), self.tf, key[1], key[2], self.word_of_slot)
        return self._rows[key]


def pcm_frames(samples, frame_len, hop):
    """frames of R samples framed as a segment with start = 1, end = R: frame j exists once R >= 1 + j * hop + frame_len"""
    return (samples - 1 - frame_len) // hop + 1 if samples >= 1 + frame_len else 0
