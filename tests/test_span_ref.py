"""CPU checks of tests/span_ref.py, the span scorer's definition (include/sr_engine.h, "word alternatives"): its three forms
against each other, against the decoder's level with one chargeable start, and against an enumeration of every admissible path
(which also produces the reach rule); then the header's three facts on the decoders' references."""
import functools

import numpy as np
import pytest

import chain_ref
import gram_ref
import span_ref as ref
import wgram_ref
from spot_ref import DIS_ERR

SETTINGS = ((chain_ref.PLANT_SKIP, 0), (None, 0), (chain_ref.PLANT_SKIP, 700))  # (skip_cost, word_cost)
# grammars that never take word 0, which the planted rows hold most often: with every frame in a word (no skipping) the
# decoder has to put another word over those stretches
NO_ZERO_GRAM = gram_ref.grammar_any([1, 2, 3, 4])
NO_ZERO_BIGRAM = wgram_ref.grammar_bigram([1, 2, 3, 4], {a: {b: 1000 * a + 300 * b for b in range(1, 5)} for a in range(1, 5)},
                                          first_cost={1: 0, 2: 500, 3: 0, 4: 2000}, last_cost={1: 0, 2: 0, 3: 900, 4: 0})


def reach(L, M):
    return M // 2 + 1 <= L <= 2 * M - 1


def test_the_three_forms_and_the_decoders_level_agree():
    rng = np.random.default_rng(11)
    finite = 0
    for M in range(1, 10):
        for L in range(1, 21):
            d = rng.integers(0, 5000 if (L + M) % 3 else 3, (L, M)).astype(np.int64)  # small values: ties between paths
            want = ref.span_scalar(d)
            assert ref.span_two_state(d) == want and ref.span_end(d) == want, (L, M)
            lvl = chain_ref.level_end_row(d, [0] + [None] * L)[L - 1]  # the decoder's level, start column 0 alone chargeable
            assert (None if lvl == chain_ref.INF else lvl[0]) == want and (want is None or lvl[1] == 0), (L, M)
            assert (want is not None) == reach(L, M), (L, M)
            finite += want is not None
    assert finite > 50


def test_F_is_the_minimum_over_every_admissible_path_and_the_reach_rule_follows():
    rng = np.random.default_rng(12)
    for M in range(1, 6):
        for L in range(1, 10):
            ps = ref.paths(L, M)
            assert bool(ps) == reach(L, M), (L, M, len(ps))  # the rule comes out of the enumeration
            for p in ps:  # what the enumeration admits is what the header describes
                steps = [(x1 - x0, y1 - y0) for (x0, y0), (x1, y1) in zip(p, p[1:])]
                assert p[0] == (0, 0) and p[-1] == (L - 1, M - 1) and set(steps) <= {(1, 1), (1, 0), (0, 1)}
                assert all(s == (1, 1) or prev == (1, 1) for prev, s in zip([None] + steps, steps))
                assert len(p) <= 2 * M - 1
            assert len(set(map(tuple, ps))) == len(ps)
            for amp in (4, 60000):
                d = rng.integers(0, amp, (L, M)).astype(np.int64)
                want = min((sum(int(d[c]) for c in p) for p in ps), default=None)
                assert ref.span_scalar(d) == want and ref.span_two_state(d) == want and ref.span_end(d) == want, (L, M, amp)
    assert len(ref.paths(1, 1)) == 1 and not ref.paths(2, 1) and not ref.paths(1, 2) and len(ref.paths(9, 5)) == 1 and len(ref.paths(7, 5)) > 1


def test_invalid_spans_and_slots_score_dis_err_and_modes_divide():
    fx = chain_ref.planted()
    N = int(fx["inf"][0])
    valid = np.array([1, 0, 1, 1, 1], np.uint8)
    M0 = int(fx["tf"][0])
    for s, e in ((ref.ALL_ONES, 5), (3, ref.ALL_ONES), (9, 8), (N - M0, N), (0, 0)):
        assert ref.span_row(fx["im"][0], N, s, e, fx["tm"], fx["tf"], None, ref.SPAN_ACC) == [DIS_ERR] * 5, (s, e)
    acc = ref.span_row(fx["im"][0], N, N - M0, N - 1, fx["tm"], fx["tf"], valid, ref.SPAN_ACC)
    dis = ref.span_row(fx["im"][0], N, N - M0, N - 1, fx["tm"], fx["tf"], valid, ref.SPAN_DIS)
    assert acc[1] == DIS_ERR and acc[0] != DIS_ERR
    assert dis == [DIS_ERR if a == DIS_ERR else a // (M0 + int(fx["tf"][k])) for k, a in enumerate(acc)]
    w = ref.spans([[(N - M0, N - 1), (9, 8)]])
    sc = ref.span_scores(fx["im"][:1], fx["inf"][:1], fx["tm"], fx["tf"], valid, w, ref.SPAN_ACC)
    assert sc.shape == (1, 2, 5) and sc[0, 0].tolist() == acc and sc[0, 1].tolist() == [DIS_ERR] * 5
    assert sc.tolist() == ref.span_scores(fx["im"][:1], fx["inf"][:1], fx["tm"], fx["tf"], valid, w, ref.SPAN_ACC, ref.span_two_state).tolist()


def word_facts(fx, rec, words, valid=None):
    """fact 1 on every decoded word -> [(row, position, decoded slot, first minimum of F in slot order)]"""
    out = []
    for r in range(len(rec)):
        N = int(fx["inf"][r])
        for i in range(int(rec[r]["n_words"])):
            w = words[r, i]
            slot, s, e = int(w["slot"]), int(w["start"]), int(w["end"])
            F = ref.span_row(fx["im"][r], N, s, e, fx["tm"], fx["tf"], valid, ref.SPAN_ACC)
            q = ref.span_row(fx["im"][r], N, s, e, fx["tm"], fx["tf"], valid, ref.SPAN_DIS)
            assert F[slot] == int(w["acc"]) and q[slot] == int(w["dis"]), (r, i, F, tuple(w))
            out.append((r, i, slot, F.index(min(F))))
        for i in range(int(rec[r]["n_words"]), words.shape[1]):  # the unused word rows are invalid spans
            assert ref.span_row(fx["im"][r], N, int(words[r, i]["start"]), int(words[r, i]["end"]), fx["tm"], fx["tf"], valid,
                                ref.SPAN_ACC) == [DIS_ERR] * len(fx["tf"])
    return out


@functools.lru_cache(maxsize=None)
def unconstrained(skip, word_cost):
    fx = chain_ref.planted()
    return chain_ref.decode(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, chain_ref.PLANT_MAXF, chain_ref.PLANT_MAX_WORDS, 0, skip, word_cost)


@pytest.mark.parametrize("skip,word_cost", SETTINGS)
def test_facts_1_and_2_on_the_unconstrained_decoder(skip, word_cost):
    fx = chain_ref.planted()
    rec, words, _ = unconstrained(skip, word_cost)
    facts = word_facts(fx, rec, words)
    assert len(facts) >= 12
    for r, i, slot, first_min in facts:
        assert slot == first_min, (r, i)  # fact 2: the decoded slot is the first minimum of F over the span
    # ... which is entry 0 of the N-best over the span's score row, under any word map
    sc = ref.span_scores(fx["im"], fx["inf"], fx["tm"], fx["tf"], None, words, ref.SPAN_ACC)
    for wos in (np.arange(5), np.arange(5) // 2, np.array([7, 3, 7, 100, 3])):
        nb, nm = ref.nbest(sc, wos, 3)
        for r, i, slot, _ in facts:
            assert nb[r, i, 0]["slot"] == slot and nb[r, i, 0]["dis"] == words[r, i]["acc"] and nb[r, i, 0]["word"] == wos[slot]
            assert nm[r, i] >= 1 and (nb[r, i, 1]["word"] == ref.NO_WORD or nb[r, i, 1]["dis"] >= nb[r, i, 0]["dis"])
        for r in range(len(rec)):
            n = int(rec[r]["n_words"])
            assert not nm[r, n:].any() and all(tuple(x) == ref.NO_CANDIDATE for x in nb[r, n:].reshape(-1))


def test_facts_1_and_3_under_a_grammar_and_a_weighted_grammar():
    fx = chain_ref.planted()
    args = (fx["im"], fx["inf"], fx["tm"], fx["tf"], None, chain_ref.PLANT_MAXF, chain_ref.PLANT_MAX_WORDS, 0, None, 0)
    for name, (rec, words, _) in (("any but 0", gram_ref.decode(NO_ZERO_GRAM, *args)), ("bigram", wgram_ref.decode(NO_ZERO_BIGRAM, *args))):
        facts = word_facts(fx, rec, words)  # fact 1: F_slot == acc, whatever the grammar charged
        assert len(facts) >= 12, name
        other = [(r, i) for r, i, slot, first_min in facts if slot != first_min]
        assert all(slot != 0 for _, _, slot, _ in facts)
        assert other, name  # fact 3: the grammar forbade the acoustically best word somewhere; entry 0 is that word all the same
