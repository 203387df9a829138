"""The connected-word decoder's definition (tests/chain_ref.py) against itself: the three statements of a level against each
other, the scalar one against an enumeration of every segmentation and every path, planted words, exact covers, exact counts
and the u32 cost bound.  CPU only; the GPU tests (tests/test_chain.py) compare the library with the same module bit for bit.
Coefficients drawn from -2..2 make ties common, so that the tie rule (cost, start, slot, fewest words) is exercised."""
import itertools

import numpy as np

import chain_ref as ref


def small_store(rng, K, amp=2, max_m=5):
    Ms = [int(rng.integers(1, max_m + 1)) for _ in range(K)]
    return [rng.integers(-amp, amp + 1, (m, 12)) for m in Ms]


def small_dis(rng, N, tpls, amp=2):
    inp = rng.integers(-amp, amp + 1, (N, 12))
    return [ref.local_dis(inp, t) for t in tpls]


def test_three_forms_agree_on_all_small_shapes():
    rng = np.random.default_rng(11)
    cases = tie_cases = 0
    for N in range(0, 11):
        for K, max_words in itertools.product((1, 2, 3), (1, 2, 3)):
            tpls = small_store(rng, K)
            dis = small_dis(rng, N, tpls)
            if K == 3:
                dis[1] = None  # an invalid slot
            for skip in (None, 3):
                for n_exact in (0, max_words):
                    outs = [ref.decode_row(dis, N, max_words, n_exact, skip, 1, level)
                            for level in (ref.level_scalar, ref.level_two_state, ref.level_end_row)]
                    assert outs[0] == outs[1] == outs[2], (N, K, max_words, skip, n_exact)
                    cases += 1
                    tie_cases += outs[0]["status"] == ref.CH_OK and outs[0]["cost"] < 40
    assert cases == 11 * 9 * 4 and tie_cases > 50


def word_costs(d):
    """every admissible path of one slot, enumerated: (start, end) -> the cheapest path from (start, 0) to (end, M - 1)"""
    N, M = d.shape
    best = {}

    def walk(x, y, cost, start, after_diag):
        cost += int(d[x, y])
        if y == M - 1 and cost < best.get((start, x), cost + 1):
            best[(start, x)] = cost
        if x + 1 < N and y + 1 < M:
            walk(x + 1, y + 1, cost, start, True)
        if after_diag and x + 1 < N:
            walk(x + 1, y, cost, start, False)
        if after_diag and y + 1 < M:
            walk(x, y + 1, cost, start, False)

    for s in range(N):
        walk(s, 0, 0, s, False)
    return best


def brute_force(dis, N, max_words, skip, word_cost):
    """every segmentation of the row into words and skipped frames -> [min cost with exactly l words or None for l = 1..max_words]"""
    per_slot = [word_costs(d) for d in dis if d is not None and N > 0]
    best = [None] * (max_words + 1)

    def go(pos, n, cost):
        if pos == N:
            if best[n] is None or cost < best[n]:
                best[n] = cost
            return
        if skip is not None:
            go(pos + 1, n, cost + skip)
        if n < max_words:
            for wc in per_slot:
                for e in range(pos, N):
                    if (pos, e) in wc:
                        go(e + 1, n + 1, cost + wc[(pos, e)] + word_cost)

    go(0, 0, 0)
    return best[1:]


def test_scalar_form_equals_brute_force():
    rng = np.random.default_rng(12)
    finite = 0
    for N in range(0, 8):
        for K, max_words, skip in itertools.product((1, 2), (1, 2, 3), (None, 2)):
            tpls = small_store(rng, K, max_m=4)
            dis = small_dis(rng, N, tpls)
            o = ref.decode_row(dis, N, max_words, 0, skip, 1, ref.level_scalar)
            want = brute_force(dis, N, max_words, skip, 1)
            assert o["level_cost"] == want, (N, K, max_words, skip, o["level_cost"], want)
            if o["status"] == ref.CH_OK:
                finite += 1
                fin = [c for c in want if c is not None]
                assert o["cost"] == min(fin) and o["n_words"] == want.index(min(fin)) + 1  # the fewest words among equal costs
                # the traced words are a parse of that cost: in order, disjoint, their own costs among the enumerated paths
                at, total = 0, 0
                for slot, start, end, acc, cum in o["words"]:
                    assert at <= start <= end < N and (skip is not None or start == at)
                    assert acc == word_costs(dis[slot])[(start, end)]  # the cheapest path of that span
                    total += acc + 1 + (start - at) * (skip or 0)
                    assert cum == total
                    at = end + 1
                assert total + (N - at) * (skip or 0) == o["cost"] and o["skipped"] == N - sum(w[2] - w[1] + 1 for w in o["words"])
            else:
                assert all(c is None for c in want)
    assert finite > 40


def test_planted_words_are_all_recovered():
    fx = ref.planted()
    assert len(fx["seq"]) >= 12 and sorted({len(s) for s in fx["seq"]}) == [1, 2, 3, 4]
    rec, words, lc = ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, ref.PLANT_MAXF, ref.PLANT_MAX_WORDS, 0, ref.PLANT_SKIP, 0)
    for r, seq in enumerate(fx["seq"]):  # every row counts
        assert rec[r]["status"] == ref.CH_OK and rec[r]["n_words"] == len(seq), (r, rec[r])
        assert words[r, :len(seq)]["slot"].tolist() == seq, r
        for w, (s, e) in zip(words[r], fx["spans"][r]):
            assert abs(int(w["start"]) - s) <= 2 and abs(int(w["end"]) - e) <= 2, (r, w, s, e)
        assert np.all(words[r, len(seq):].view(np.uint32) == 0xFFFFFFFF)


def test_exact_cover_without_skipping():
    rng = np.random.default_rng(14)
    tf = np.array([9, 12, 7, 10], np.uint32)
    tm = np.zeros((4, 13, 12), np.int16)
    for k in range(4):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    order = [2, 0, 3]
    row = np.concatenate([tm[k, :tf[k]] for k in order])
    im = np.zeros((1, 40, 12), np.int16)
    im[0, :len(row)] = row
    rec, words, lc = ref.decode(im, [len(row)], tm, tf, None, 40, 4, 0, None, 0)
    assert tuple(rec[0]) == (0, 3, 0, ref.CH_OK)
    assert words[0, :3]["slot"].tolist() == order and words[0, :3]["start"].tolist() == [0, 7, 16] and words[0, :3]["end"].tolist() == [6, 15, 25]
    assert np.all(words[0, :3]["acc"] == 0) and np.all(words[0, :3]["cum"] == 0) and lc[0, 2] == 0 and lc[0, 0] > 0


def test_exact_count_is_honoured():
    fx = ref.planted()
    r = 2  # three planted words
    free = ref.decode(fx["im"][r:r + 1], fx["inf"][r:r + 1], fx["tm"], fx["tf"], None, ref.PLANT_MAXF, 4, 0, ref.PLANT_SKIP, 0)
    assert free[0][0]["n_words"] == 3
    for n in (1, 2, 3, 4):
        rec, words, lc = ref.decode(fx["im"][r:r + 1], fx["inf"][r:r + 1], fx["tm"], fx["tf"], None, ref.PLANT_MAXF, 4, n, ref.PLANT_SKIP, 0)
        assert rec[0]["status"] == ref.CH_OK and rec[0]["n_words"] == n and rec[0]["cost"] == lc[0, n - 1] >= free[0][0]["cost"]
        assert np.array_equal(lc, free[2]) and np.all(words[0, n:].view(np.uint32) == 0xFFFFFFFF)
    # a count without a parse: one frame cannot hold two words
    d = [np.zeros((1, 1), np.int64)]
    assert ref.decode_row(d, 1, 2, 2)["status"] == ref.CH_NONE and ref.decode_row(d, 1, 2, 1)["status"] == ref.CH_OK


def test_cost_bound_at_the_argument_limits():
    assert ref.cost_bound() == 3 * 16383 * 65536 + 16 * (1 << 24) < 2 ** 32 - 1  # all ones stays free for "unreachable"
    # get_dis never exceeds MAX_D: the squared sum is taken mod 2^32 before the root
    worst = ref.local_dis(np.full((1, 12), -32768), np.full((1, 12), 32767))
    assert 0 <= int(worst[0, 0]) <= ref.MAX_D and int(np.sqrt(np.float32(2 ** 32 - 1))) <= ref.MAX_D
    # a word over L frames has at most 3L cells (a path has L + M - 1 at most and M <= 2L), a skipped frame costs less than a cell
    for L in range(1, 40):
        for M in range(1, 2 * L + 1):
            assert L + M - 1 <= 3 * L
    assert ref.MAX_SKIP < ref.MAX_D
    # the worst row the limits admit, level by level in plain integers: the longest row, every cell at MAX_D
    N = ref.MAX_FRAMES
    assert ref.MAX_WORDS * ref.MAX_WORD_COST + 3 * N * ref.MAX_D == ref.cost_bound()
    # a small instance at the per-cell limit: costs add up exactly
    d = [np.full((6, 3), ref.MAX_D, np.int64)]
    o = ref.decode_row(d, 6, 2, 0, ref.MAX_SKIP, ref.MAX_WORD_COST)
    assert o["status"] == ref.CH_OK and o["cost"] < ref.cost_bound() and o["cost"] == min(c for c in o["level_cost"] if c is not None)
