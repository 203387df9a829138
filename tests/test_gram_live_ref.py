"""The live grammar decoder's reference (tests/gram_live_ref.py) held to the batch definition (tests/gram_ref.py), on the CPU:
ONE history of a recording gives gram_ref.decode_row of every prefix, and a channel stepped push by push as the device runs it
keeps exactly that history, whatever the chunking.  No tolerances: Python ints and tuples compared whole.
"""
import functools

import numpy as np
import pytest

import gram_live_ref as live
import gram_ref as ref

W, SKIP = ref.chain_ref.PLANT_MAX_WORDS, ref.chain_ref.PLANT_SKIP
ROWS = ref.chain_ref.PLANT_ROWS


@functools.lru_cache(maxsize=None)
def planted_dis(r):
    fx = ref.planted()
    N = int(fx["inf"][r])
    return N, live.slot_distances(fx["im"][r, :N], fx["tm"], fx["tf"])


def random_chunking(rng, N, hi):
    """sizes 0..hi that sum to N, zeros and ones included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(0, hi + 1))])), N - sum(out)))
    return out


def cut(N, sizes):
    out, i = [], 0
    while sum(out) < N:
        out.append(min(sizes[i % len(sizes)], N - sum(out)))
        i += 1
    return out


def test_the_four_grammars_are_grammars_and_two_have_joined_from_sets():
    for name, (gram, wos) in live.GRAMMARS.items():
        ref.check(gram, None if wos is None else set(wos.tolist()))
    assert max(len(f) for f in ref.pairs_of(live.GRAMMARS["join"][0]).values()) == 2
    assert max(len(f) for f in ref.pairs_of(live.GRAMMARS["pairs"][0]).values()) >= 3
    assert max(len(f) for f in ref.pairs_of(live.GRAMMARS["anchor"][0]).values()) == 1


@pytest.mark.parametrize("which", list(live.GRAMMARS))
def test_one_history_gives_the_batch_definition_of_every_prefix(which):
    """every prefix N of every planted row: trace(history of the whole row, N) is gram_ref.decode_row of the first N frames.
    The parameter variants (no skipping, a given count, a word cost) run on one row."""
    gram, wos = live.GRAMMARS[which]
    parsed = 0
    for r in range(ROWS):
        N, dis = planted_dis(r)
        for skip, n_exact, wc in ((SKIP, 0, 0), (None, 0, 0), (SKIP, 3, 1000)) if r == 1 else ((SKIP, 0, 0),):
            A, E = live.history(gram, dis, N, W, skip, wc, wos)
            for n in range(N + 1):
                got = live.trace(A, E, n, gram, W, n_exact, wc, wos)
                want = ref.decode_row(gram, [d[:n] for d in dis], n, W, n_exact, skip, wc, wos)
                assert got == want, (which, r, n, skip, n_exact, wc)
            parsed += got["status"] == ref.CH_OK
            if n_exact == 0 and got["status"] == ref.CH_OK:
                assert ref.accepts(gram, [(s if wos is None else int(wos[s]), st) for s, _, _, _, _, st in got["words"]])
    assert parsed >= 8, (which, parsed)  # the grammars accept most of the planted rows: the walk through the states is exercised


def test_a_channel_pushed_step_by_step_keeps_the_batch_history():
    """init of the new positions in every state, resumed columns of the kept items with the charge taken over the from-set,
    the keys' minimum, E_l(., t) extended from the carried E_l(x0, t): after every push the parse, and at the end the whole
    history, are those of everything pushed as one row.  Pushes of 0 frames change nothing."""
    rng = np.random.default_rng(35)
    sizes = set()
    for which, r, skip, n_exact, wc in (("anchor", 3, SKIP, 0, 0), ("seq", 7, None, 0, 0), ("pairs", 11, SKIP, 3, 1000), ("join", 2, 700, 0, 0),
                                        ("join", 10, SKIP, 0, 0), ("seq", 6, SKIP, 0, 0)):
        gram, wos = live.GRAMMARS[which]
        N, dis = planted_dis(r)
        dis = dis[:3] + [None] + dis[4:] if which == "anchor" else dis  # an invalid slot (the anchor has a loop for every other)
        valid = [d is not None for d in dis]
        A, E = live.history(gram, dis, N, W, skip, wc, wos)
        for chunks in ([N], cut(N, [1]), cut(N, [63, 64, 65]), random_chunking(rng, N, 40), [0] + random_chunking(rng, N, 9)):
            ch = live.Channel(gram, [None if d is None else d.shape[1] for d in dis], W, n_exact, skip, wc, wos, valid)
            at = 0
            for n in chunks:
                got = ch.push([None if d is None else d[at:at + n] for d in dis])
                at += n
                assert got == live.trace(A, E, at, gram, W, n_exact, wc, wos), (which, r, skip, chunks, at)
            assert at == N and ch.A[1:] == A[1:] and ch.E == E, (which, r, skip, chunks)
            sizes.update(chunks)
    assert {0, 1} <= sizes and max(sizes) >= 64


def test_pruned_levels_stay_unreachable_and_records_carry_the_state():
    """a sequence of three positions under max_words 5: levels 4 and 5 keep no item and their costs stay None; the records hold
    the state after each word in `reserved`"""
    gram = ref.grammar_sequence([[0, 1, 2], [2, 3, 4], [0, 4]])
    fx = ref.planted()
    assert [len(i) for i in ref.items_per_level(gram, W, range(5))] == [3, 3, 2, 0, 0]
    seen = 0
    for r in range(ROWS):
        N, dis = planted_dis(r)
        ch = live.Channel(gram, [d.shape[1] for d in dis], W, 0, SKIP)
        got = ch.push(dis)
        assert got == ref.decode_row(gram, dis, N, W, 0, SKIP) and got["level_cost"][3:] == [None, None]
        rec, words, lc = live.to_records(got, fx["tf"], W)
        assert lc[3:].tolist() == [live.DIS_ERR] * 2
        if got["status"] == ref.CH_OK:
            seen += 1
            assert words[:3]["reserved"].tolist() == [1, 2, 3] and int(rec["n_words"]) == 3
    assert seen >= 3
