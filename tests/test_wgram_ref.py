"""Weighted grammars on the CPU: the reference (tests/wgram_ref.py) against gram_ref and against its own independent statement,
the condition that the drawn costs change parses, the surface of the library and the Python interface, and the host-only
compile step (csrc/sr_gram_compile.h) under the sanitizers.  No device.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import chain_ref
import gram_ref
import wgram_ref as ref
from stm32_speech_recognition_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
MAXF, W, SKIP = chain_ref.PLANT_MAXF, 4, chain_ref.PLANT_SKIP  # 4 levels: the planted rows hold 1..4 words
SPW2 = np.arange(chain_ref.PLANT_K, dtype=np.uint32) // 2  # two slots per word: labels 0, 0, 1, 1, 2
PAIR_GRAM = gram_ref.grammar_word_pairs(range(5), [(a, b) for a in range(5) for b in range(5) if (a + b) % 2 == 1], first=[0, 1, 2, 4])
JOIN_GRAM = (4, [(0, 1, 0), (0, 2, 1), (1, 3, 2), (2, 3, 2), (3, 1, 0), (1, 1, 1), (3, 2, 1)], [0, 1, 0, 1])
GRAMS = dict(join=(JOIN_GRAM, SPW2), pairs=(PAIR_GRAM, None))


@functools.lru_cache(maxsize=None)
def planted_dis():
    fx = chain_ref.planted()
    return [ref.slot_distances(fx["im"][r, :int(fx["inf"][r])], fx["tm"], fx["tf"]) for r in range(len(fx["inf"]))]


@functools.lru_cache(maxsize=None)
def rows(which, costs, skip):
    """decode_row of every planted row under grammar `which` with the drawn costs or with none"""
    fx = chain_ref.planted()
    gram, wos = GRAMS[which]
    g = ref.drawn_costs(gram) if costs else ref.with_costs(gram)
    return [ref.decode_row(g, planted_dis()[r], int(fx["inf"][r]), W, 0, skip, 0, wos) for r in range(len(fx["inf"]))]


# ---- 1: zero costs are gram_ref ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(GRAMS))
def test_zero_costs_equal_the_unweighted_reference_in_every_field(which):
    fx = chain_ref.planted()
    gram, wos = GRAMS[which]
    for skip, n_exact, wc in ((SKIP, 0, 0), (None, 0, 5000), (SKIP, 3, 0)):
        want = gram_ref.decode(gram, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, n_exact, skip, wc, wos)
        for g in (gram, ref.with_costs(gram), ref.with_costs(gram, [0] * len(gram[1]), [0] * gram[0])):
            got = ref.decode(g, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, n_exact, skip, wc, wos)
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes(), (which, skip, n_exact, wc)
        assert (want[0]["status"] == ref.CH_OK).sum() >= 6


# ---- 2: the level cost against every accepted state path -----------------------------------------------------------------------
@pytest.mark.parametrize("skip", [SKIP, None])
@pytest.mark.parametrize("which", list(GRAMS))
def test_level_costs_equal_the_enumeration_of_state_paths(which, skip):
    fx = chain_ref.planted()
    gram, wos = GRAMS[which]
    g = ref.drawn_costs(gram)
    assert max(g[3]) > 10000 and max(g[4]) > 0 and all(f or not c for f, c in zip(g[2], g[4]))
    finite = 0
    for r, o in enumerate(rows(which, True, skip)):
        for n in range(1, W + 1):
            want = ref.enumerate_cost(g, planted_dis()[r], int(fx["inf"][r]), n, skip, 0, wos)
            assert o["level_cost"][n - 1] == want, (which, skip, r, n)
            finite += want is not None
    assert finite >= 20


# ---- 3: the costs bite -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,skip,at_least", [("pairs", None, 6), ("pairs", SKIP, 2), ("join", None, 2), ("join", SKIP, 2)])
def test_the_drawn_costs_change_parses(which, skip, at_least):
    with_c, without = rows(which, True, skip), rows(which, False, skip)
    assert all(o["status"] == ref.CH_OK for o in with_c) and all(o["status"] == ref.CH_OK for o in without)
    changed = sum([w[:3] for w in a["words"]] != [w[:3] for w in b["words"]] for a, b in zip(with_c, without))
    print(f"{which}, skip {skip}: {changed} of {len(with_c)} rows parse differently under the drawn costs")  # 8, 3, 2, 3 when this was written
    assert changed >= at_least, (which, skip, changed)


# ---- 4: the surface (fails without the feature) --------------------------------------------------------------------------------
def test_header_declares_weighted_grammars_and_libraries_export_them():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.search(r"\bint sr_grammar_create_weighted\s*\(\s*sr_engine \*h,\s*uint32_t n_states,\s*const sr_gram_arc \*arcs,\s*const uint32_t \*arc_cost,"
                     r"\s*uint32_t n_arcs,\s*const uint8_t \*final_state,\s*const uint32_t \*final_cost,\s*sr_grammar \*\*out\)", src)
    for testing in (False, True):
        assert hasattr(engine.load_library(testing), "sr_grammar_create_weighted"), testing
    at = [text.index(h) for h in ("grammar-constrained decoding:", "live grammar-constrained decoding:", "full-DP alignment and word models")]
    assert at[0] < text.index("int sr_grammar_create_weighted") < at[1]
    for section in (text[at[0]:at[1]], text[at[1]:at[2]]):  # arc weights are no longer out of scope of either section
        scope = section[section.rindex("Out of scope"):]
        assert "arc weights" not in scope[:scope.index("*/")]
    assert "3 774 676 992 < 2^32" in text and 3 * 16383 * 65536 + 16 * (1 << 24) + 16 * (1 << 24) + (1 << 24) == 3774676992 == ref.cost_bound()
    import inspect
    assert list(inspect.signature(engine.Engine.grammar).parameters)[1:] == ["n_states", "arcs", "final", "arc_cost", "final_cost"]
    assert callable(engine.grammar_bigram)


def test_create_weighted_refuses_null_handles():
    L, g = engine.load_library(), C.c_void_p(0x5A5A5A5A)
    arcs, fin = np.zeros(1, engine.GRAM_ARC_DTYPE), np.ones(1, np.uint8)
    assert L.sr_grammar_create_weighted(None, C.c_uint32(1), engine._vp(arcs), None, C.c_uint32(1), engine._vp(fin), None, C.byref(g)) == 3
    assert g.value == 0x5A5A5A5A and b"null" in L.sr_last_error()


# ---- 5: the Python builder -------------------------------------------------------------------------------------------------------
def test_python_grammar_bigram_is_the_reference_one():
    rng = np.random.default_rng(3)
    labels = [4, 8, 2, 8]
    cost = {a: {b: (None if (a + b) % 3 == 0 else int(rng.integers(0, 9000))) for b in (2, 4, 8)} for a in (2, 4, 8)}
    table = [[None if (a * b) % 4 == 1 else a * 10 + b for b in range(5)] for a in range(5)]
    for args, kw in (((labels, cost), {}), ((labels, cost), dict(first_cost={4: 7, 8: None, 2: 0}, last_cost={4: None, 8: 11, 2: 5})),
                     ((range(5), table), dict(first_cost=[1, None, 3, 4, None])), ((range(5), table), dict(last_cost=[None, 0, 9, None, 1 << 24]))):
        got, want = engine.grammar_bigram(*args, **kw), ref.grammar_bigram(*args, **kw)
        assert got == want and len(got) == 5
        gram_ref.check(got[:3])
        ac, fc = ref.costs_of(got)
        assert len(ac) == len(got[1]) and got[0] == 1 + len(set(args[0]))
    n_states, arcs, final, ac, fc = ref.grammar_bigram(range(5), table, first_cost=[1, None, 3, 4, None], last_cost=[None, 0, 9, None, 2])
    assert (0, 2, 1) not in arcs and ac[arcs.index((0, 3, 2))] == 3 and ac[arcs.index((1 + 2, 1 + 4, 4))] == 24 and (1 + 1, 1 + 1, 1) not in arcs
    assert final == [0, 0, 1, 1, 0, 1] and fc == [0, 0, 0, 9, 0, 2]


# ---- 6: the compile step under the sanitizers ----------------------------------------------------------------------------------
def test_compile_step_runs_clean_under_the_sanitizers(tmp_path):
    """the checks, the charge lists, the items and the per-level lists of csrc/sr_gram_compile.h over random grammars of up to
    64 states and 4096 arcs against a brute-force restatement: a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "compile_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "gram_compile", "compile_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "compile_check ok" in run.stdout, (run.stdout, run.stderr)
