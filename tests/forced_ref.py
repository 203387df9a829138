"""Transcript-forced alignment (include/sr_engine.h, "forced alignment against a transcript") restated in numpy on top of
chain_ref.level_end_row, the span gather, and the train_connected composition on top of cluster_ref.  OPT-IN EXTENSION, no
reference counterpart.

  row      transcript t[0..n) of labels of the word map, n = 0..words_per_row; slots(w) = the VALID slots with label w
  levels   chain_ref's E_0, charged start, key (cost, start, slot), E_l, skip_cost, word_cost; at level l the minimum of A_l runs
           over slots(t[l-1]) only; the count is n
  status   NONE when n = 0, when some slots(t[i]) is empty, or when E_n(N) is unreachable
  trace    chain_ref's; the word's 1-based position travels in `reserved`
  prune    minlen(w) = min over slots(w) of M // 2 + 1; tail_l = the sum of minlen over the positions after l; level l is swept
           over the end frames e with e + 1 <= N - tail_l only.  align_row takes a `prune` flag: both settings give the same
           records (tests/test_forced_ref.py), which is the header's argument run.
  gather   example e = the frames start..end of the span that names it (start <= end < N, at most ex_rows frames), zero rows
           behind them; an invalid or too long span and an unnamed example give a zero row of 0 frames
  train    per iteration: align, gather every transcript word (examples grouped by word in sr_word_groups order -- words by
           their first slot -- and inside a word by (row, position)), one cluster_ref iteration with all slots of a word as its
           models (an invalid slot = a centroid of 0 frames), the new centroids become the store

Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import cluster_ref
from chain_ref import CH_NONE, CH_OK, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, NO_WORD_ROW, e0, level_end_row
from spot_ref import DIS_ERR, INF, local_dis

NONE = 0xFFFFFFFF
MAX_WORDS = 16


def labels_of(K, word_of_slot=None):
    return list(range(K)) if word_of_slot is None else [int(w) for w in word_of_slot]


def minlen_of(lab, tf, valid):
    """{label: min over its valid slots of M // 2 + 1}; a label without a valid slot is absent"""
    out = {}
    for k, w in enumerate(lab):
        if (valid is None or valid[k]) and int(tf[k]) > 0:
            out[w] = min(out.get(w, 1 << 30), int(tf[k]) // 2 + 1)
    return out


def align_row(dis, N, pos_slots, skip=None, word_cost=0, tails=None):
    """dis: per slot the local distances int64 [N, M_k] (None: an invalid slot); pos_slots[i] = the valid slots of position i;
    tails[l - 1] = tail_l, or None for no pruning -> dict(status, cost, n_words, skipped, words = [(slot, start, end, acc, cum,
    position)])"""
    n = len(pos_slots)
    out = dict(status=CH_NONE, cost=None, n_words=0, skipped=0, words=[])
    if n == 0:
        return out
    E = [e0(N, skip)] + [[None] * (N + 1) for _ in range(n)]
    A = [None] + [[None] * (N + 1) for _ in range(n)]
    for l in range(1, n + 1):
        bound = N if tails is None else max(N - tails[l - 1], 0)  # end frames e with e + 1 <= bound
        for k in pos_slots[l - 1]:
            for x, v in enumerate(level_end_row(dis[k][:bound], E[l - 1][:bound + 1])):
                if v != INF:
                    cand = (v[0] + word_cost, v[1], k)
                    if A[l][x + 1] is None or cand < A[l][x + 1]:
                        A[l][x + 1] = cand
        for p in range(1, N + 1):
            best = None if A[l][p] is None else A[l][p][0]
            if skip is not None and E[l][p - 1] is not None and (best is None or E[l][p - 1] + skip < best):
                best = E[l][p - 1] + skip
            E[l][p] = best
    if E[n][N] is None:
        return out
    p, words = N, []
    for l in range(n, 0, -1):
        while A[l][p] is None or A[l][p][0] != E[l][p]:
            p -= 1
        cost, start, slot = A[l][p]
        words.append((slot, start, p - 1, cost - word_cost - E[l - 1][start], E[l][p], l))
        p = start
    assert skip is not None or p == 0
    words.reverse()
    out.update(status=CH_OK, cost=E[n][N], n_words=n, words=words, skipped=N - sum(w[2] - w[1] + 1 for w in words))
    return out


def align(mfcc, frames, tm, tf, valid, max_frames, transcripts, words_per_row, skip=None, word_cost=0, word_of_slot=None, prune=True):
    """mfcc int16 [n_rows, max_frames, 12], frames [n_rows] (clamped), store tm / tf / valid, transcripts = a list of label lists
    -> (rec CHAIN_REC_DTYPE [n_rows], words CHAIN_WORD_DTYPE [n_rows, words_per_row]).  Raises ValueError where the library
    refuses: words_per_row outside 1..16, a transcript longer than it, a label no slot carries."""
    n_rows, K = len(mfcc), len(tm)
    lab = labels_of(K, word_of_slot)
    if not 1 <= words_per_row <= MAX_WORDS:
        raise ValueError("words_per_row")
    for r, t in enumerate(transcripts):
        if len(t) > words_per_row:
            raise ValueError(f"row {r}: {len(t)} words")
        for i, w in enumerate(t):
            if int(w) not in lab:
                raise ValueError(f"row {r}, position {i}: label {w}")
    ok = [(valid is None or valid[k]) and int(tf[k]) > 0 for k in range(K)]
    minlen = minlen_of(lab, tf, valid)
    rec = np.zeros(n_rows, CHAIN_REC_DTYPE)
    words = np.empty((n_rows, words_per_row), CHAIN_WORD_DTYPE)
    words[...] = NO_WORD_ROW
    for r in range(n_rows):
        N, t = min(int(frames[r]), max_frames), [int(w) for w in transcripts[r]]
        pos_slots = [[k for k in range(K) if lab[k] == w and ok[k]] for w in t]
        need = sorted({k for s in pos_slots for k in s})
        dis = [local_dis(mfcc[r, :N], tm[k, :int(tf[k])]) if k in need else None for k in range(K)]
        tails = [sum(minlen.get(w, 0) for w in t[l:]) for l in range(1, len(t) + 1)] if prune else None
        o = align_row(dis, N, pos_slots, skip, word_cost, tails)
        if o["status"] != CH_OK:
            rec[r] = (DIS_ERR, 0, 0, CH_NONE)
            continue
        rec[r] = (o["cost"], o["n_words"], o["skipped"], CH_OK)
        for i, (slot, start, end, acc, cum, pos) in enumerate(o["words"]):
            words[r, i] = (lab[slot], slot, start, end, acc, acc // (end - start + 1 + int(tf[slot])), cum, pos)
    return rec, words


def gather(mfcc, frames, max_frames, words, dst_of_span, n_ex, ex_rows):
    """words CHAIN_WORD_DTYPE [n_rows, words_per_row]; dst_of_span [n_rows * words_per_row]: an example index or NONE ->
    (ex int16 [n_ex, ex_rows, 12], ex_frames uint32 [n_ex]).  Raises ValueError for a destination at or above n_ex or named twice."""
    words = np.asarray(words).reshape(len(mfcc), -1)
    wpr = words.shape[1]
    dst = [int(d) for d in dst_of_span]
    assert len(dst) == len(mfcc) * wpr
    named = [d for d in dst if d != NONE]
    if any(d >= n_ex for d in named) or len(set(named)) != len(named):
        raise ValueError("dst_of_span")
    ex, ex_frames = np.zeros((n_ex, ex_rows, 12), np.int16), np.zeros(n_ex, np.uint32)
    for i, d in enumerate(dst):
        if d == NONE:
            continue
        r, w = i // wpr, words[i // wpr, i % wpr]
        N, start, end = min(int(frames[r]), max_frames), int(w["start"]), int(w["end"])
        if start <= end < N and end - start + 1 <= ex_rows:
            L = end - start + 1
            ex[d, :L], ex_frames[d] = mfcc[r, start:end + 1], L
    return ex, ex_frames


CORPUS_MAXF, CORPUS_ROWS = 64, 54
CORPUS_WORDS = np.array([5, 9, 5, 2, 7, 9, 2, 7, 5, 9, 2, 7], np.uint32)  # 4 words x 3 slots, not slot // 3


def corpus(seed=31, long_row=False):
    """The random corpus of the CPU and the GPU test: 12 slots = 4 words x 3 slots under CORPUS_WORDS; every slot of word 7 and
    slot 8 of word 5 invalid; templates of 1..12 frames; CORPUS_ROWS rows of 0..69 frames at max_frames 64 (0, 1, 64 and 69
    among them) with transcripts of 0..6 words.  long_row: one more row of 64 frames whose transcript is 16 times the word
    with the shortest valid template.  -> dict(tm, tf, valid, words, im, inf, transcripts), arrays read-only"""
    rng = np.random.default_rng(seed)
    K = len(CORPUS_WORDS)
    tf = rng.integers(1, 13, K).astype(np.uint32)
    tf[0], tf[3] = 1, 12
    tm = np.zeros((K, 13, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    valid = np.array([w != 7 for w in CORPUS_WORDS], np.uint8)
    valid[8] = 0
    n_rows = CORPUS_ROWS + int(long_row)
    inf = rng.integers(0, 70, n_rows).astype(np.uint32)
    inf[:4] = (0, 1, 64, 69)
    im = rng.integers(-3000, 3001, (n_rows, CORPUS_MAXF, 12)).astype(np.int16)
    transcripts = [[int(w) for w in rng.choice([5, 9, 2, 7], int(n), p=[0.3, 0.3, 0.3, 0.1])] for n in rng.integers(0, 7, CORPUS_ROWS)]
    transcripts[1], transcripts[2] = [5], [9, 2, 5]
    if long_row:
        inf[-1] = 64
        shortest = min((int(tf[k]), k) for k in range(K) if valid[k])[1]
        transcripts.append([int(CORPUS_WORDS[shortest])] * 16)
    for a in (tm, tf, valid, im, inf):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, valid=valid, words=CORPUS_WORDS, im=im, inf=inf, transcripts=transcripts)


def noisy_store(tm, tf, seed=5, amp=500):
    """the training tests' starting models: every frame of every template plus uniform integer noise of +-amp, template by template"""
    rng = np.random.default_rng(seed)
    out = np.array(tm, np.int64)
    for k in range(len(tm)):
        out[k, :int(tf[k])] += rng.integers(-amp, amp + 1, (int(tf[k]), 12))
    return out.astype(np.int16)


def word_groups(lab):
    """sr_word_groups: (order = the slots grouped by word, ascending inside a word, words by their first slot; group_start; word_id)"""
    ids = list(dict.fromkeys(lab))
    order = [k for w in ids for k in range(len(lab)) if lab[k] == w]
    start = np.concatenate(([0], np.cumsum([lab.count(w) for w in ids])))
    return order, start, ids


def example_layout(lab, transcripts, words_per_row):
    """-> (dst_of_span [n_rows * words_per_row], word_start [words + 1]): every transcript word is an example; the examples are
    grouped by word in word_groups order and, inside a word, in (row, position) order"""
    _, _, ids = word_groups(lab)
    dst = np.full(len(transcripts) * words_per_row, NONE, np.uint32)
    word_start, e = [0], 0
    for w in ids:
        for r, t in enumerate(transcripts):
            for i, x in enumerate(t):
                if int(x) == w:
                    dst[r * words_per_row + i] = e
                    e += 1
        word_start.append(e)
    return dst, np.array(word_start, np.uint32)


def train_connected(mfcc, frames, transcripts, tm, tf, valid, max_frames, n_iter=4, skip=None, word_cost=0, word_of_slot=None, ex_rows=None):
    """Engine.train_connected -> dict(cen int16 like tm (slot order), frames, iters = [(OK rows, the sum of their costs)], words =
    the last alignment's word rows, recs = every iteration's records)"""
    K = len(tm)
    lab = labels_of(K, word_of_slot)
    W = max(1, max(len(t) for t in transcripts))
    ex_rows = min(max_frames, 1024) if ex_rows is None else ex_rows
    order, gstart, _ = word_groups(lab)
    dst, word_start = example_layout(lab, transcripts, W)
    cen_frames = np.array([int(tf[k]) if (valid is None or valid[k]) else 0 for k in order], np.uint32)
    tm, iters, recs = np.array(tm), [], []
    for _ in range(n_iter):
        rec, words = align(mfcc, frames, tm, tf, valid, max_frames, transcripts, W, skip, word_cost, word_of_slot)
        ok = rec["status"] == CH_OK
        iters.append((int(ok.sum()), int(rec["cost"][ok].astype(np.int64).sum())))
        recs.append(rec)
        ex, ex_frames = gather(mfcc, frames, max_frames, words, dst, int(word_start[-1]), ex_rows)
        got = cluster_ref.cluster(ex, ex_frames, word_start, gstart.astype(np.uint32), np.ascontiguousarray(tm[order]), cen_frames, 1)
        tm = tm.copy()
        tm[order] = got["cen"]
    return dict(cen=tm, frames=np.array(tf, np.uint32), iters=iters, words=words, recs=recs)
