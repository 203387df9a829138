"""One-pass grammar decoding on the CPU: the restatement (tests/onepass_gram_ref.py) stated time-synchronously and in the
kernels' block form, held equal for every block length 1..L and shown to differ beyond L; its relation to level building
under a grammar (tests/wgram_ref.py) and to the one-pass decoder (tests/onepass_ref.py); the long planted rows under a
bigram grammar; the surface of the feature; and the host-only planning (csrc/sr_onepass_gram_plan.h) under the sanitizers.
No device; tests/test_onepass_gram.py compares the kernels with this restatement byte for byte.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import pytest

import chain_ref
import onepass_gram_ref as ref
import onepass_ref
import wgram_ref
from spot_ref import local_dis
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_decode_onepass_grammar_dp_dev", "sr_decode_onepass_grammar_dp", "sr_decode_onepass_grammar_batch", "sr_onepass_grammar_plan")
HOOK = "onepass_gram_prune_off"
COSTS = ((1500, 0), (None, 5000), (300, 5000))
K = chain_ref.PLANT_K


def grammars():
    """the four grammars of the planted rows, by name"""
    labels = list(range(K))
    pairs = wgram_ref.grammar_word_pairs(labels, [(a, b) for a in labels for b in labels if (a + b) % 2 == 0 or a == b])
    return dict(any=wgram_ref.grammar_any(labels), pairs=pairs,
                sequence=wgram_ref.grammar_sequence([labels, labels[:3], labels, labels], optional_tail=True),
                weighted=wgram_ref.drawn_costs(pairs))


GRAMS = tuple(grammars())


@functools.lru_cache(maxsize=None)
def planted_dis(r):
    pl = chain_ref.planted()
    N = int(pl["inf"][r])
    return N, tuple(local_dis(pl["im"][r, :N], pl["tm"][k, :int(pl["tf"][k])]) for k in range(K))


@functools.lru_cache(maxsize=None)
def sync(name, r, skip, wc):
    N, dis = planted_dis(r)
    return ref.history_sync(grammars()[name], list(dis), N, skip, wc)


@functools.lru_cache(maxsize=None)
def levels(name, r, skip, wc):
    N, dis = planted_dis(r)
    return wgram_ref.decode_row(grammars()[name], list(dis), N, 16, 0, skip, wc)


# ---- 1: the two statements of the history -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAMS)
def test_block_form_equals_the_time_synchronous_form_up_to_L_and_not_beyond(name):
    pl, gram = chain_ref.planted(), grammars()[name]
    L = ref.reach(pl["tf"])
    assert L == 5
    for skip, wc in COSTS:
        differs = 0
        for r in range(chain_ref.PLANT_ROWS):
            N, dis = planted_dis(r)
            want = sync(name, r, skip, wc)
            for n in range(1, L + 1):
                assert ref.history_blocks(gram, list(dis), N, n, skip, wc) == want, (r, skip, wc, n)
            assert ref.history_blocks(gram, list(dis), N, L, skip, wc, cap=N + 7) == want  # the host's bound may lie above the row
            differs += ref.history_blocks(gram, list(dis), N, L + 1, skip, wc) != want
        assert differs >= 4, (skip, wc, differs)  # the bound is tight: one frame more and words that start inside a block are missed


# ---- 2: relation to level building under the grammar -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAMS)
def test_cost_is_the_minimum_over_the_levels_and_the_words_are_level_buildings(name):
    gram = grammars()[name]
    _, fc = wgram_ref.costs_of(gram)
    for skip, wc in COSTS:
        for r in range(chain_ref.PLANT_ROWS):
            N, _ = planted_dis(r)
            lv = levels(name, r, skip, wc)
            A, E = sync(name, r, skip, wc)
            got = ref.trace_row(A, E, N, gram, wc)
            costs = [c for c in lv["level_cost"] if c is not None]
            if gram[2][0] and skip is not None:  # state 0 final: filler alone is a parse
                costs.append(N * skip + fc[0])
            assert costs and got["status"] == ref.CH_OK and got["cost"] == min(costs), (r, skip, wc)
            assert costs.count(min(costs)) == 1, (r, skip, wc)  # the minimum is unique: the two decoders must agree
            if lv["cost"] == min(costs):
                assert got["words"] == lv["words"] and got["skipped"] == lv["skipped"] and got["n_words"] == lv["n_words"], (r, skip, wc)
            else:
                assert got["n_words"] == 0 and got["skipped"] == N and name == "any"


def test_anchor_grammar_is_the_one_pass_decoder():
    gram = grammars()["any"]
    for skip, wc in COSTS:
        for r in range(chain_ref.PLANT_ROWS):
            N, dis = planted_dis(r)
            want = onepass_ref.decode_row(list(dis), N, skip, wc)
            A, E = sync("any", r, skip, wc)
            got = ref.trace_row(A, E, N, gram, wc)
            assert (got["status"], got["cost"], got["n_words"], got["skipped"]) == (want["status"], want["cost"], want["n_words"], want["skipped"])
            assert [w[:5] for w in got["words"]] == want["words"] and all(w[5] == 0 for w in got["words"]) and got["state"] == 0


@pytest.mark.parametrize("name", GRAMS)
def test_cost_is_the_enumerated_minimum_on_the_three_shortest_rows(name):
    pl, gram = chain_ref.planted(), grammars()[name]
    L = ref.reach(pl["tf"])
    _, fc = wgram_ref.costs_of(gram)
    short = sorted(range(chain_ref.PLANT_ROWS), key=lambda r: int(pl["inf"][r]))[:3]
    for skip, wc in COSTS:
        for r in short:
            N, dis = planted_dis(r)
            costs = [wgram_ref.enumerate_cost(gram, list(dis), N, n, skip, wc) for n in range(1, N // L + 1)]
            costs = [c for c in costs if c is not None]
            if gram[2][0] and skip is not None:
                costs.append(N * skip + fc[0])
            A, E = sync(name, r, skip, wc)
            got = ref.trace_row(A, E, N, gram, wc)
            assert (got["cost"] if got["status"] == ref.CH_OK else None) == min(costs, default=None), (r, skip, wc)


def test_the_guard_of_the_charge_matters():
    """state 2 is never reached (its only way in needs a word no slot carries); the pair (3, word 0) lists it at a cost, and
    all ones + 7 wraps to 6: a blind sum charges the word 6 from a state nobody is in"""
    _, dis = planted_dis(3)
    N = len(dis[0])
    gram = (4, [(0, 1, 1), (1, 3, 0), (2, 3, 0), (0, 2, 9)], [0, 0, 0, 1], [0, 50000, 7, 0], None)
    d = [dis[0], dis[1]]
    good = ref.decode_row(gram, d, N, 1500, 0, word_of_slot=[0, 1])
    bad = ref.decode_row(gram, d, N, 1500, 0, word_of_slot=[0, 1], wrap=True)
    assert good["status"] == ref.CH_OK and all(w[5] in (1, 3) for w in good["words"])
    assert (bad["cost"], bad["words"]) != (good["cost"], good["words"]) and bad["cost"] < good["cost"]
    for n in (1, 3, 5):
        assert ref.decode_row(gram, d, N, 1500, 0, word_of_slot=[0, 1], block=n) == good


# ---- 3: rows that level building cannot hold ----------------------------------------------------------------------------------------
def long_grammar(forbid=None):
    """the pairs grammar that allows exactly the planted bigrams of planted_long() (less the pair `forbid`)"""
    pl = ref.planted_long()
    pairs = {(a, b) for seq in pl["seq"] for a, b in zip(seq, seq[1:])} - {forbid}
    return wgram_ref.grammar_word_pairs(range(K), sorted(pairs), first={seq[0] for seq in pl["seq"]})


@functools.lru_cache(maxsize=None)
def long_want(forbid=None):
    pl = ref.planted_long()
    out = ref.decode(long_grammar(forbid), pl["im"], pl["inf"], pl["tm"], pl["tf"], None, onepass_ref.LONG_MAXF, 64, chain_ref.PLANT_SKIP, 0)
    for a in out:
        a.setflags(write=False)
    return out


def forbidden_pair():
    """a planted pair of different words in row 0"""
    seq = ref.planted_long()["seq"][0]
    return next((a, b) for a, b in zip(seq, seq[1:]) if a != b)


def test_planted_long_rows_under_the_planted_bigrams():
    pl = ref.planted_long()
    rec, words = long_want()
    assert rec["status"].tolist() == [ref.CH_OK] * 4 and rec["n_words"].tolist() == list(onepass_ref.LONG_COUNTS) and min(rec["n_words"]) > 16
    for r, seq in enumerate(pl["seq"]):
        assert words[r, :len(seq)]["slot"].tolist() == seq, r
        assert words[r, :len(seq)]["reserved"].tolist() == [1 + k for k in seq], r
    free = onepass_ref.decode(pl["im"], pl["inf"], pl["tm"], pl["tf"], None, onepass_ref.LONG_MAXF, 64, chain_ref.PLANT_SKIP, 0)
    assert rec.tobytes() == free[0].tobytes()  # the grammar allows what was said: the unconstrained cost
    rec2, words2 = long_want(forbidden_pair())
    assert rec2[0]["status"] == ref.CH_OK and rec2[0]["cost"] > rec[0]["cost"]
    n = int(rec2[0]["n_words"])
    assert words2[0, :n]["slot"].tolist() != free[1][0, :int(free[0][0]["n_words"])]["slot"].tolist()
    said = words2[0, :n]["slot"].tolist()
    assert forbidden_pair() not in set(zip(said, said[1:]))


# ---- 4: the builder and the pruning ---------------------------------------------------------------------------------------------------
def test_grammar_repeat_and_the_kept_lists():
    assert ref.grammar_repeat([[7, 8]], [1, 2], 1) == (3, [(0, 1, 7), (0, 1, 8), (1, 2, 1), (1, 2, 2), (2, 2, 1), (2, 2, 2)], [0, 0, 1])
    assert ref.grammar_repeat([[7]], [1], 0) == (2, [(0, 1, 7), (1, 1, 1)], [0, 1])
    assert ref.grammar_repeat([], [3], 2) == (3, [(0, 1, 3), (1, 2, 3), (2, 2, 3)], [0, 0, 1])
    assert engine.grammar_repeat([[7, 8]], [1, 2], 1) == ref.grammar_repeat([[7, 8]], [1, 2], 1)
    assert engine.grammar_repeat([[7], [8]], [1, 1, 2], 0) == ref.grammar_repeat([[7], [8]], [1, 1, 2], 0)
    # state 3 is unreachable, state 4 reaches no final state: their items go, and so does the item out of state 3
    gram = (5, [(0, 1, 0), (1, 2, 1), (3, 2, 2), (1, 4, 3), (4, 4, 3), (2, 2, 4)], [0, 0, 1, 0, 0])
    items, states = ref.kept(gram, [0, 1, 2, 3, 4, 4])
    assert items == [(0, 1), (1, 2), (4, 2), (5, 2)] and states == [0, 1, 2]
    seq = wgram_ref.grammar_sequence([[0, 1], [2]])
    assert ref.kept(seq, [0, 1, 2]) == ([(0, 1), (1, 1), (2, 2)], [0, 1, 2])  # state 0 has no incoming arc and is kept
    assert ref.kept(seq, [0, 1, 2], [1, 0, 1]) == ([(0, 1), (2, 2)], [0, 1, 2])


# ---- 5: the surface (fails without the feature) -----------------------------------------------------------------------------------------
def test_header_library_and_python_surface():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    section = re.sub(r"[\s*]+", " ", text[text.index("one-pass grammar decoding: word networks without a word cap"):])
    for phrase in ("An unreachable E never has a cost added to it", "The walk always ends in state 0", "n_words 0 with SR_CH_OK",
                   "Under ties the two decoders may choose differently", "2^30", "every final state that can be reached"):
        assert phrase in section, phrase
    hooks = text[text.index("Development and test hooks"):]
    assert '"%s"' % HOOK in hooks
    engine.dev_hook(HOOK, 0)  # the testing library knows the hook, the product library has none, not even its name
    assert engine.load_library().sr_dev_hook(HOOK.encode(), C.c_int64(1)) == 3
    assert HOOK.encode() + b"\0" not in open(engine.LIB_PATH, "rb").read()
    for m in ("decode_onepass_grammar", "decode_onepass_grammar_dev", "decode_onepass_grammar_pcm"):
        assert callable(getattr(Engine, m, None)), m
    assert callable(engine.onepass_grammar_plan) and callable(engine.grammar_repeat)
    out = (C.c_uint32 * 6)()
    assert engine.load_library().sr_onepass_grammar_plan(None, C.c_uint32(0), out) == 3


# ---- 6: the planning under the sanitizers --------------------------------------------------------------------------------------------
def test_plan_runs_clean_under_the_sanitizers(tmp_path):
    """reachability, the kept items and states, the bytes of a row and the refusals (csrc/sr_onepass_gram_plan.h) over random
    grammars against a brute-force restatement: a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "onepass_gram_plan", "plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
