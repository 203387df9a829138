"""The grammar-constrained decoder's definition (tests/gram_ref.py) held to an independent statement of it and to the
unconstrained decoder (tests/chain_ref.py).  CPU only, exact comparisons.

  - L_n of decode_row equals enumerate_cost -- every accepted label sequence of length n, chained level by level with only
    that position's slots -- for every n, with and without skipping;
  - the anchor grammar (one state, every word) gives chain_ref.decode byte for byte, under a 2-slots-per-word map as well;
  - every decoded sequence, walked through the states in `reserved`, is accepted by its grammar.
"""
import functools

import numpy as np
import pytest

import chain_ref
import gram_ref as ref

ROWS, MAX_WORDS = 6, 3
SPW2 = np.arange(chain_ref.PLANT_K) // 2  # word = slot / 2: labels 0, 0, 1, 1, 2


def grammars():
    """name -> (grammar, word_of_slot or None)"""
    pairs = [(a, b) for a in range(5) for b in range(5) if (a + b) % 2 == 1]  # no word after one of its own parity
    return {
        "anchor": (ref.grammar_any(range(5)), None),
        "sequence": (ref.grammar_sequence([[0, 1, 2], [2, 3, 4], [0, 4]], optional_tail=True), None),
        "pairs": (ref.grammar_word_pairs(range(5), pairs, first=[0, 1, 2, 4]), None),
        "joined, two slots per word": ((4, [(0, 1, 0), (0, 2, 1), (1, 3, 2), (2, 3, 2), (3, 1, 0), (1, 1, 1)], [0, 1, 0, 1]), SPW2),
    }


@functools.lru_cache(maxsize=None)
def row_dis(r):
    fx = chain_ref.planted()
    N = int(fx["inf"][r])
    return N, [ref.local_dis(fx["im"][r, :N], fx["tm"][k, :int(fx["tf"][k])]) for k in range(chain_ref.PLANT_K)]


def test_grammar_builders():
    assert ref.grammar_any([3, 5, 3]) == (1, [(0, 0, 3), (0, 0, 5)], [1])
    assert ref.grammar_sequence([[1], [2, 3]]) == (3, [(0, 1, 1), (1, 2, 2), (1, 2, 3)], [0, 0, 1])
    assert ref.grammar_sequence([[1], [2], [3]], optional_tail=True)[2] == [0, 1, 1, 1]
    S, arcs, final = ref.grammar_word_pairs([7, 9], [(7, 9), (9, 9)], first=[7], last=[9])
    assert (S, sorted(arcs), final) == (3, [(0, 1, 7), (1, 2, 9), (2, 2, 9)], [0, 0, 1])
    for g, wos in grammars().values():
        ref.check(g, set(range(5)) if wos is None else set(int(w) for w in wos))
    assert ref.accepted_sequences(ref.grammar_sequence([[1], [2, 3]]), 2) == [(1, 2), (1, 3)]
    assert ref.accepted_sequences(ref.grammar_sequence([[1], [2, 3]]), 1) == []


@pytest.mark.parametrize("name", list(grammars()))
def test_level_costs_equal_the_enumeration_of_accepted_sequences(name):
    gram, wos = grammars()[name]
    finite = 0
    for skip in (None, chain_ref.PLANT_SKIP):
        for r in range(ROWS):
            N, dis = row_dis(r)
            o = ref.decode_row(gram, dis, N, MAX_WORDS, 0, skip, 17, wos)
            for n in range(1, MAX_WORDS + 1):
                want = ref.enumerate_cost(gram, dis, N, n, skip, 17, wos)
                assert o["level_cost"][n - 1] == want, (name, skip, r, n)
                finite += want is not None
            exact = ref.decode_row(gram, dis, N, MAX_WORDS, 2, skip, 17, wos)  # the count given
            assert exact["cost"] == o["level_cost"][1] and exact["n_words"] == (2 if exact["status"] == ref.CH_OK else 0)
    assert finite >= 8, (name, finite)  # the comparison is of costs, not of "no parse" with "no parse"


@pytest.mark.parametrize("wos", [None, SPW2], ids=["word = slot", "two slots per word"])
def test_the_anchor_grammar_is_the_unconstrained_decoder(wos):
    fx = chain_ref.planted()
    labels = range(5) if wos is None else wos
    for skip, n_exact, wc in ((chain_ref.PLANT_SKIP, 0, 0), (None, 0, 5000), (chain_ref.PLANT_SKIP, 2, 0)):
        args = (fx["im"], fx["inf"], fx["tm"], fx["tf"], None, chain_ref.PLANT_MAXF, chain_ref.PLANT_MAX_WORDS, n_exact, skip, wc, wos)
        want, got = chain_ref.decode(*args), ref.decode(ref.grammar_any(labels), *args)
        for w, g in zip(want, got):
            assert w.dtype == g.dtype and w.tobytes() == g.tobytes(), (skip, n_exact, wc)
        assert np.all(got[1]["reserved"][got[1]["slot"] != 0xFFFFFFFF] == 0)


@pytest.mark.parametrize("name", list(grammars()))
def test_every_decoded_sequence_is_accepted_by_its_grammar(name):
    gram, wos = grammars()[name]
    fx = chain_ref.planted()
    free = chain_ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, chain_ref.PLANT_MAXF, chain_ref.PLANT_MAX_WORDS, 0,
                            chain_ref.PLANT_SKIP, 0, wos)
    rec, words, lc = ref.decode(gram, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, chain_ref.PLANT_MAXF, chain_ref.PLANT_MAX_WORDS, 0,
                                chain_ref.PLANT_SKIP, 0, wos)
    differ = 0
    for r in range(len(rec)):
        n = int(rec[r]["n_words"])
        if rec[r]["status"] == ref.CH_OK:
            assert ref.accepts(gram, [(int(w["word"]), int(w["reserved"])) for w in words[r, :n]]), (name, r)
            assert rec[r]["cost"] >= free[0][r]["cost"]  # a constraint never makes a parse cheaper
        assert np.all(words[r, n:].view(np.uint32) == 0xFFFFFFFF)
        differ += any(words[r][f].tolist() != free[1][r][f].tolist() for f in ("slot", "start", "end"))
    assert (rec["status"] == ref.CH_OK).sum() >= 8
    assert differ >= (0 if name == "anchor" else 4), (name, differ)  # the constraint bites
