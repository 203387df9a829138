"""Word-model clustering (include/sr_engine.h, "word models: clustering a word's examples into templates") restated in numpy on
top of align_ref.align_pair.  OPT-IN EXTENSION, no reference counterpart.

  inputs     W words; word w owns the example rows [word_start[w], word_start[w+1]) of mfcc [E, max_frames, 12] and the models
             [mdl_start[w], mdl_start[w+1]) of cen [M, cen_rows, 12] with cen_frames [M]; 1..16 models per word, a word may have
             no examples.
  score      s(e, m) = the aligner's dis of (row e as input, centroid m as reference), DIS_ERR when the pair is not OK: an empty
             row, a failed gate, an unreachable end cell, an invalid centroid (0 frames or more than cen_rows), N above 1024.
  assign     the first minimum in model order over the models of the example's word -- key (dis, m); NONE when every score is
             DIS_ERR, and then best = DIS_ERR.
  iteration  assign against the set that enters, then one DBA iteration with model_of = assign: s32 sums, division truncating
             toward zero, rows nobody matched stay, F_m fixed, rows past F_m zero, an invalid centroid copied through, a model
             without examples stays, unassigned examples contribute nothing.  Iterations chain.
  records    stats[m] = (n_ok = examples assigned to m, n_fail = 0, acc = the sum of their acc against the entering centroid);
             iter = (n_assigned, n_unassigned, n_moved against the previous iteration's assignment -- everything unassigned
             before the first --, n_empty = models with n_ok 0, acc = the sum of stats.acc).

Plain module: no fixtures, no pytest settings.
"""
import numpy as np

import align_ref

DIS_ERR = 0xFFFFFFFF
NONE = 0xFFFFFFFF
CLUSTER_MAX = 16
ITER_DTYPE = np.dtype([("n_assigned", "<u4"), ("n_unassigned", "<u4"), ("n_moved", "<u4"), ("n_empty", "<u4"), ("acc", "<u8")])
TRAIN_STAT_DTYPE = align_ref.TRAIN_STAT_DTYPE


def check(word_start, mdl_start, max_frames):
    """the conditions the library checks on the host arrays -> None, or what is wrong"""
    ws, ms = np.asarray(word_start, np.int64), np.asarray(mdl_start, np.int64)
    if len(ws) < 2 or len(ws) != len(ms):
        return "no words"
    if ws[0] != 0 or ms[0] != 0 or np.any(np.diff(ws) < 0) or np.any(np.diff(ms) < 0):
        return "not ascending from 0"
    if np.any(np.diff(ms) < 1) or np.any(np.diff(ms) > CLUSTER_MAX):
        return "1..16 models per word"
    if np.any(np.diff(ws) * min(max_frames, align_ref.MAX_FRAMES) > 65535):
        return "accumulator bound"
    return None


def word_of(word_start):
    return np.repeat(np.arange(len(word_start) - 1), np.diff(np.asarray(word_start, np.int64)))


def score(mfcc, frames, word_start, mdl_start, cen, cen_frames):
    """-> (dis uint32 [E, 16], acc uint32 [E, 16], paths {(e, m): path}) over every (example, model of its word) pair; columns
    at and beyond the word's model count hold DIS_ERR / 0xFFFFFFFF"""
    E, max_frames, cen_rows = int(word_start[-1]), mfcc.shape[1], cen.shape[1]
    dis, acc, paths = np.full((E, CLUSTER_MAX), DIS_ERR, np.uint32), np.full((E, CLUSTER_MAX), NONE, np.uint32), {}
    for e, w in enumerate(word_of(word_start)):
        N = min(int(frames[e]), max_frames)
        for c, m in enumerate(range(int(mdl_start[w]), int(mdl_start[w + 1]))):
            R = int(cen_frames[m])
            if N > align_ref.MAX_FRAMES or R < 1 or R > cen_rows:
                continue
            rec, path = align_ref.align_pair(mfcc[e, :N], cen[m, :R])
            if rec[3] == align_ref.OK:
                dis[e, c], acc[e, c], paths[(e, m)] = rec[0], rec[1], path
    return dis, acc, paths


def assign_rows(dis, word_start, mdl_start):
    """-> (assign uint32 [E]: model index or NONE, best uint32 [E], column of the choice int [E] (-1: none))"""
    E = len(dis)
    assign, best, col = np.full(E, NONE, np.uint32), np.full(E, DIS_ERR, np.uint32), np.full(E, -1, np.int64)
    for e, w in enumerate(word_of(word_start)):
        for c in range(int(mdl_start[w + 1]) - int(mdl_start[w])):
            if dis[e, c] < best[e]:  # strictly: the first minimum in model order
                best[e], col[e], assign[e] = dis[e, c], c, int(mdl_start[w]) + c
    return assign, best, col


def iteration(mfcc, frames, word_start, mdl_start, cen, cen_frames, prev=None):
    """one iteration -> dict(cen, assign, best, dis, stats TRAIN_STAT_DTYPE [M], iter ITER_DTYPE scalar)"""
    E, M, cen_rows = int(word_start[-1]), int(mdl_start[-1]), cen.shape[1]
    dis, acc, paths = score(mfcc, frames, word_start, mdl_start, cen, cen_frames)
    assign, best, col = assign_rows(dis, word_start, mdl_start)
    prev = np.full(E, NONE, np.uint32) if prev is None else prev
    stats, out = np.zeros(M, TRAIN_STAT_DTYPE), np.zeros_like(cen)
    for m in range(M):
        F = int(cen_frames[m])
        if F < 1 or F > cen_rows:  # an invalid centroid: copied through (nobody can be assigned to it)
            out[m] = cen[m]
            continue
        total, cnt = np.zeros((F, 12), np.int64), np.zeros(F, np.int64)
        for e in np.nonzero(assign == m)[0]:
            stats[m]["n_ok"] += 1
            stats[m]["acc"] += int(acc[e, col[e]])
            for x, y in paths[(int(e), m)]:
                total[y] += mfcc[e, x]
                cnt[y] += 1
        assert np.abs(total).max(initial=0) < 2 ** 31 and cnt.max(initial=0) <= 65535
        mean = np.sign(total) * (np.abs(total) // np.maximum(cnt, 1)[:, None])  # truncation toward zero
        out[m, :F] = np.where(cnt[:, None] > 0, mean, cen[m, :F])
    it = np.zeros((), ITER_DTYPE)
    it["n_assigned"], it["n_unassigned"] = int((assign != NONE).sum()), int((assign == NONE).sum())
    it["n_moved"], it["n_empty"], it["acc"] = int((assign != prev).sum()), int((stats["n_ok"] == 0).sum()), int(stats["acc"].sum())
    return dict(cen=out, assign=assign, best=best, dis=dis, stats=stats, iter=it)


def cluster(mfcc, frames, word_start, mdl_start, cen, cen_frames, n_iter):
    """-> dict(cen, assign (the last iteration's), stats [n_iter, M], iter [n_iter], assigns [n_iter, E], dis [n_iter, E, 16])"""
    prev, steps = None, []
    for _ in range(n_iter):
        steps.append(iteration(mfcc, frames, word_start, mdl_start, cen, cen_frames, prev))
        cen, prev = steps[-1]["cen"], steps[-1]["assign"]
    return dict(cen=cen, assign=prev, stats=np.array([s["stats"] for s in steps]), iter=np.array([s["iter"] for s in steps], ITER_DTYPE),
                assigns=np.array([s["assign"] for s in steps]), dis=np.array([s["dis"] for s in steps]))


def default_seeds(frames, rows, n_mdl):
    """the examples cluster_words starts a word's n_mdl models from: position ((2c + 1) n) // (2C) of the word's rows in stable
    ascending order of frame count"""
    by_len = np.asarray(rows)[np.argsort(np.asarray(frames)[rows], kind="stable")]
    return [int(by_len[((2 * c + 1) * len(rows)) // (2 * n_mdl)]) for c in range(n_mdl)]


def cluster_words(mfcc, frames, labels, max_frames, n_clusters=4, n_iter=4):
    """Engine.cluster_words with the default initialisation -> (cen, cen_frames, word_ids, valid, assign in input order)"""
    frames = np.minimum(np.asarray(frames, np.uint32), max_frames)
    labels = np.asarray(labels, np.uint32)
    words, counts = np.unique(labels, return_counts=True)
    order = np.argsort(labels, kind="stable")
    word_start = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
    n_mdl = np.minimum(counts, n_clusters)
    mdl_start = np.concatenate(([0], np.cumsum(n_mdl))).astype(np.uint32)
    seeds = []
    for w in range(len(words)):
        seeds += default_seeds(frames, order[word_start[w]:word_start[w + 1]], int(n_mdl[w]))
    cen_frames = frames[seeds]
    cen = np.zeros((len(seeds), int(cen_frames.max()) + 1, 12), np.int16)
    for m, e in enumerate(seeds):
        cen[m, :cen_frames[m]] = mfcc[e, :cen_frames[m]]
    got = cluster(mfcc[order], frames[order], word_start, mdl_start, cen, cen_frames, n_iter)
    assign = np.empty_like(got["assign"])
    assign[order] = got["assign"]
    return got["cen"], cen_frames, np.repeat(words, n_mdl).astype(np.uint32), (got["stats"][-1]["n_ok"] > 0).astype(np.uint8), assign


# ---- the planted corpus of the tests ------------------------------------------------------------------------------------------
PLANT_MAXF, PLANT_ROWS = 80, 81
PLANT_LENGTHS = ((30, 70), (40, 44), (25, 50))  # the two prototypes of each word
PLANT_TAKES = 6


def planted(seed, amp=3000, noise=300, takes=PLANT_TAKES):
    """3 words x 2 random prototypes x `takes` examples: each example a random monotone resampling of its prototype to within
    +-1/8 of its length plus uniform noise -> dict(mfcc [E, 80, 12], frames [E], word_start, proto_of [E] (0 / 1), protos, lens)"""
    rng = np.random.default_rng(seed)
    rows, frames, proto_of, protos = [], [], [], []
    for lens in PLANT_LENGTHS:
        for k, L in enumerate(lens):
            proto = rng.integers(-amp, amp + 1, (L, 12))
            protos.append(proto)
            for _ in range(takes):
                n = int(rng.integers(L - L // 8, L + L // 8 + 1))
                src = np.sort(rng.integers(0, L, n))  # monotone, random
                src[0], src[-1] = 0, L - 1
                ex = np.clip(proto[src] + rng.integers(-noise, noise + 1, (n, 12)), -32768, 32767)
                row = np.zeros((PLANT_MAXF, 12), np.int16)
                row[:n] = ex
                rows.append(row)
                frames.append(n)
                proto_of.append(k)
    per = 2 * takes
    return dict(mfcc=np.array(rows), frames=np.array(frames, np.uint32), word_start=np.arange(4, dtype=np.uint32) * per,
                proto_of=np.array(proto_of), protos=protos)


def init_from(pl, seeds_per_word):
    """centroids copied from examples: seeds_per_word[w] = the rows (absolute) of word w's models -> (cen, cen_frames, mdl_start)"""
    seeds = [e for s in seeds_per_word for e in s]
    cen, cf = np.zeros((len(seeds), PLANT_ROWS, 12), np.int16), pl["frames"][seeds].copy()
    for m, e in enumerate(seeds):
        cen[m, :cf[m]] = pl["mfcc"][e, :cf[m]]
    return cen, cf, np.concatenate(([0], np.cumsum([len(s) for s in seeds_per_word]))).astype(np.uint32)
