"""Live one-pass grammar decoding on the CPU: the surface of the feature, the restatement (tests/onepass_gram_live_ref.py)
held to onepass_gram_ref's time-synchronous history for every chunking and every block length, the prefix property that gives
every push's row from one history, and the host-only planning (csrc/sr_onepass_gram_live_plan.h) under the sanitizers.  No
device; tests/test_onepass_gram_live.py compares the kernels with this restatement byte for byte.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import chain_ref
import onepass_gram_live_ref as live
import onepass_gram_ref as gref
import wgram_ref
from spot_ref import local_dis
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_onepass_gram_live_geometry", "sr_onepass_gram_live_open", "sr_onepass_gram_live_set_grammar", "sr_onepass_gram_live_push_dev",
         "sr_onepass_gram_live_push", "sr_onepass_gram_live_push_pcm_dev", "sr_onepass_gram_live_push_pcm", "sr_onepass_gram_live_end")
K = chain_ref.PLANT_K
LABELS = list(range(K))
SMALL_N = 10  # frames of the recording whose every composition is pushed: two of the shortest words' reach, L = 5


def grammars():
    """the five grammars of the planted rows, by name"""
    pairs = wgram_ref.grammar_word_pairs(LABELS, [(a, b) for a in LABELS for b in LABELS if (a + b) % 2 == 0 or a == b])
    return dict(any=wgram_ref.grammar_any(LABELS), pairs=pairs,
                sequence=wgram_ref.grammar_sequence([LABELS, LABELS[:3], LABELS, LABELS], optional_tail=True),
                weighted=wgram_ref.drawn_costs(pairs), repeat=gref.grammar_repeat([LABELS[:3]], LABELS, 1))


GRAMS = tuple(grammars())


# ---- the surface (fails without the feature) -----------------------------------------------------------------------------------
def test_header_declares_the_nine_calls_and_both_libraries_export_them():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
    assert re.search(r"\bvoid sr_onepass_gram_live_close\s*\(", src)
    for fn in FUNCS + ("sr_onepass_gram_live_close",):
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert len(FUNCS) + 1 == 9
    assert src.index("sr_onepass_grammar_plan") < src.index("sr_onepass_gram_live_geometry")  # after the one-pass grammar section
    assert "live one-pass grammar decoding" in open(HEADER).read()
    assert issubclass(engine.OnePassGrammarSession, engine.OnePassSession) and engine.OnePassGrammarSession._PREFIX == "sr_onepass_gram_live_"
    assert callable(getattr(Engine, "decode_onepass_grammar_live", None)) and callable(engine.onepass_grammar_live_geometry)
    for meth in ("push", "push_dev", "push_pcm", "push_pcm_dev", "end", "close", "set_grammar"):
        assert callable(getattr(engine.OnePassGrammarSession, meth, None)), meth
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for unit in ("k_onepass_gram_live.hip", "sr_onepass_gram_live.cpp", "sr_onepass_gram_live_plan.h"):
        assert unit in mk, unit


# ---- the design ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_dis(r, N=None):
    pl = chain_ref.planted()
    N = int(pl["inf"][r]) if N is None else N
    return N, tuple(local_dis(pl["im"][r, :N], pl["tm"][k, :int(pl["tf"][k])]) for k in range(K))


def compositions(N):
    """every way to write N as an ordered sum of positive parts: 2^(N - 1) of them"""
    if N == 0:
        yield []
        return
    for first in range(1, N + 1):
        for rest in compositions(N - first):
            yield [first] + rest


def with_zeros(cuts):
    """an empty push in front of every push and behind the last"""
    out = [0]
    for n in cuts:
        out += [n, 0]
    return out


@pytest.mark.parametrize("name", GRAMS)
def test_every_composition_and_block_length_keeps_the_time_synchronous_history(name):
    """the first SMALL_N frames of a planted row x every composition of SMALL_N into pushes, each also with empty pushes around
    every push x every block length 1..L x skipping on and off: history_pushes == history_sync"""
    pl, gram = chain_ref.planted(), grammars()[name]
    L = gref.reach(pl["tf"])
    assert L == 5
    N, dis = planted_dis(0, SMALL_N)
    comps = list(compositions(N))
    assert len(comps) == 2 ** (N - 1)
    for skip, wc in ((1500, 0), (None, 0)):
        want = gref.history_sync(gram, list(dis), N, skip, wc)
        # words end behind the first block of every block length: their columns were handed from block to block
        assert any(a is not None for A in want[0] for a in A[L + 1:])
        for block in range(1, L + 1):
            for cuts in comps:
                assert live.history_pushes(gram, list(dis), N, cuts, L, skip, wc, block) == want, (skip, block, cuts)
            for cuts in comps[::7]:
                assert live.history_pushes(gram, list(dis), N, with_zeros(cuts), L, skip, wc, block) == want, (skip, block, cuts)


def random_cuts(rng, N, hi):
    """push sizes 0..hi that sum to N, zeros included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(1, hi + 1))])), N - sum(out)))
    return out


@pytest.mark.parametrize("name", GRAMS)
def test_whole_planted_rows_in_random_pushes_and_changing_blocks(name):
    """whole recordings, where words end and the states of the grammar are all in use: random pushes of 0..13 frames, one-frame
    pushes, one push, and a block length that changes from push to push"""
    pl, gram = chain_ref.planted(), grammars()[name]
    L = gref.reach(pl["tf"])
    rng = np.random.default_rng(2025)
    for r in (0, 5, 11):
        N, dis = planted_dis(r)
        for skip, wc in ((1500, 0), (None, 5000), (300, 5000)):
            want = gref.history_sync(gram, list(dis), N, skip, wc)
            for cuts in (random_cuts(rng, N, 13), [1] * N, [N]):
                assert live.history_pushes(gram, list(dis), N, cuts, L, skip, wc) == want, (r, skip, wc, cuts)
            ch = live.Channel(gram, len(dis), L, skip, wc)
            at = 0
            for n in random_cuts(rng, N, 13):
                ch.push([d[at:at + n] for d in dis], int(rng.integers(1, L + 1)))
                at += n
            assert (ch.A, ch.E) == want, (r, skip, wc)


def test_blocks_longer_than_L_are_wrong():
    pl, gram = chain_ref.planted(), grammars()["pairs"]
    L = gref.reach(pl["tf"])
    differs = 0
    for r in range(chain_ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        ch = live.Channel(gram, len(dis), L + 1, 1500, 0)
        ch.push(list(dis))
        differs += (ch.A, ch.E) != gref.history_sync(gram, list(dis), N, 1500, 0)
    assert differs >= 2


@pytest.mark.parametrize("name", GRAMS)
def test_one_history_gives_the_row_of_every_prefix(name):
    """Recording.row(N) equals decode_row of the prefix, head and tail, with the state in `reserved`"""
    pl, gram = chain_ref.planted(), grammars()[name]
    tm, tf = pl["tm"], pl["tf"]
    n_words = 0
    for r in (1, 7):
        full_N = int(pl["inf"][r])
        for skip, wc in ((1500, 0), (None, 5000)):
            rec = live.Recording(gram, pl["im"][r, :full_N], tm, tf, None, 2, skip, wc)
            for N in sorted({0, 1, 4, 5, 6, full_N} | set(range(0, full_N + 1, 7))):
                o = gref.decode_row(gram, [d[:N] for d in rec.dis], N, skip, wc)
                assert rec.parse(N) == o, (r, skip, wc, N)
                for cap, tail in ((2, False), (2, True), (16, False)):
                    got = rec.row(N, cap, tail)
                    want = live.to_records(o, tf, cap, tail)
                    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
                    if o["status"] == live.CH_OK:
                        shown = o["words"][-cap:] if tail else o["words"][:cap]
                        assert got[1]["reserved"][:len(shown)].tolist() == [w[5] for w in shown]
                        assert got[1]["slot"][:len(shown)].tolist() == [w[0] for w in shown]
                        n_words += len(shown)
            # the batch restatement's rows are the head form's
            whole = gref.decode(gram, pl["im"][r:r + 1], pl["inf"][r:r + 1], tm, tf, None, chain_ref.PLANT_MAXF, 2, skip, wc)
            assert rec.row(full_N)[0].tobytes() == whole[0][0].tobytes() and rec.row(full_N)[1].tobytes() == whole[1][0].tobytes()
    assert n_words > 0


def test_host_plan_runs_clean_under_the_sanitizers(tmp_path):
    """the state bytes, the launch counts, the block cuts, the mirror's advance and reset against a brute-force restatement
    (csrc/sr_onepass_gram_live_plan.h): a stand-alone program on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "onepass_gram_live_plan", "plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
