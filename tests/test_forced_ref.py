"""Transcript-forced alignment on the CPU: the restatement (tests/forced_ref.py) against the grammar decoder's restatement
(gram_ref.decode_row under grammar_sequence) with the column pruning on and off, the planted rows the GPU tests rely on, the
gather and the training composition, the surface of the feature, and the host-only planning (csrc/sr_forced_plan.h) under the
sanitizers.  No device; tests/test_forced.py compares the kernels with this restatement byte for byte.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import chain_ref
import forced_ref as ref
import gram_ref
from spot_ref import local_dis
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_align_transcripts_dp_dev", "sr_align_transcripts_dp", "sr_gather_word_spans_dev", "sr_gather_word_spans")
SKIPS = (None, 900, 2500)
WORD_COST = 77


@functools.lru_cache(maxsize=None)
def corpus_want(skip, prune):
    fx = ref.corpus()
    W = max(len(t) for t in fx["transcripts"])
    return ref.align(fx["im"], fx["inf"], fx["tm"], fx["tf"], fx["valid"], ref.CORPUS_MAXF, fx["transcripts"], W, skip, WORD_COST, fx["words"], prune)


# ---- 1: the definition is the grammar decoder's, one sequence per row; the pruning changes nothing ------------------------------
@pytest.mark.parametrize("skip", SKIPS)
def test_forced_equals_the_grammar_decoder_under_a_sequence_grammar(skip):
    fx = ref.corpus()
    K, n_ok, n_none = len(fx["tm"]), 0, 0
    assert fx["valid"].sum() == 8 and sorted(set(fx["words"].tolist())) == [2, 5, 7, 9] and not fx["valid"][fx["words"] == 7].any()
    assert {0, 1, 64, 69} <= set(fx["inf"].tolist()) and {len(t) for t in fx["transcripts"]} == set(range(7))
    for prune in (True, False):
        rec, words = corpus_want(skip, prune)
        for r, t in enumerate(fx["transcripts"]):
            if not t:
                assert rec[r].tolist() == (ref.DIS_ERR, 0, 0, ref.CH_NONE) and np.all(words[r].view(np.uint32) == 0xFFFFFFFF)
                continue
            N, n = min(int(fx["inf"][r]), ref.CORPUS_MAXF), len(t)
            dis = [local_dis(fx["im"][r, :N], fx["tm"][k, :int(fx["tf"][k])]) if fx["valid"][k] else None for k in range(K)]
            o = gram_ref.decode_row(gram_ref.grammar_sequence([[w] for w in t]), dis, N, n, n, skip, WORD_COST, fx["words"])
            assert np.all(words[r, n:].view(np.uint32) == 0xFFFFFFFF)
            if o["status"] != ref.CH_OK:
                assert rec[r].tolist() == (ref.DIS_ERR, 0, 0, ref.CH_NONE) and np.all(words[r].view(np.uint32) == 0xFFFFFFFF), r
                n_none += prune
                continue
            n_ok += prune
            assert rec[r].tolist() == (o["cost"], n, o["skipped"], ref.CH_OK), (r, prune)
            for i, (slot, start, end, acc, cum, state) in enumerate(o["words"]):
                want = (int(fx["words"][slot]), slot, start, end, acc, acc // (end - start + 1 + int(fx["tf"][slot])), cum, state)
                assert words[r, i].tolist() == want and state == i + 1, (r, i, prune)
    assert n_ok >= 10 and n_none >= 5, (n_ok, n_none)  # both outcomes occur among the rows with a transcript


def test_pruning_gives_the_same_records_and_really_prunes():
    fx = ref.corpus()
    for skip in SKIPS:
        a, b = corpus_want(skip, True), corpus_want(skip, False)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    minlen = ref.minlen_of(ref.labels_of(12, fx["words"]), fx["tf"], fx["valid"])
    assert 7 not in minlen and minlen[5] == 1 and all(1 <= m <= 7 for m in minlen.values())
    assert max(sum(minlen.get(w, 0) for w in t[1:]) for t in fx["transcripts"] if t) >= 5  # some level 1 loses five columns or more


def test_a_label_outside_the_word_map_is_refused():
    fx = ref.corpus()
    args = (fx["im"][:2], fx["inf"][:2], fx["tm"], fx["tf"], fx["valid"], ref.CORPUS_MAXF)
    with pytest.raises(ValueError, match="row 1, position 1"):
        ref.align(*args, [[5], [9, 4]], 2, word_of_slot=fx["words"])
    with pytest.raises(ValueError):
        ref.align(*args, [[5], [9, 2, 5]], 2, word_of_slot=fx["words"])
    with pytest.raises(ValueError):
        ref.align(*args, [[5], [9]], 17, word_of_slot=fx["words"])


# ---- 2: the planted rows ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_want(skip):
    pl = chain_ref.planted()
    return ref.align(pl["im"], pl["inf"], pl["tm"], pl["tf"], None, chain_ref.PLANT_MAXF, pl["seq"], chain_ref.PLANT_MAX_WORDS, skip, 0)


def test_planted_spans_are_recovered_with_skipping():
    pl = chain_ref.planted()
    rec, words = planted_want(chain_ref.PLANT_SKIP)
    assert np.all(rec["status"] == ref.CH_OK)
    got = [[(int(w["start"]), int(w["end"])) for w in words[r, :len(pl["seq"][r])]] for r in range(chain_ref.PLANT_ROWS)]
    assert sum(len(s) for s in pl["spans"]) == 30 and got == pl["spans"]  # 30 of 30
    assert [[int(w["slot"]) for w in words[r, :len(s)]] for r, s in enumerate(pl["seq"])] == pl["seq"]


# ---- 3: gather and the training composition ------------------------------------------------------------------------------------
def test_gather_restated():
    rng = np.random.default_rng(3)
    im, inf = rng.integers(-99, 100, (2, 10, 12)).astype(np.int16), np.array([10, 25], np.uint32)  # row 1 is clamped to 10 frames
    words = np.zeros((2, 3), ref.CHAIN_WORD_DTYPE)
    words["start"], words["end"] = [[0, 4, 8], [9, 5, 0]], [[3, 4, 10], [9, 4, 9]]  # (0, 8..10) ends past N; (1, 5..4) is inverted
    dst = [1, 0, 4, ref.NONE, 5, 2]
    ex, ef = ref.gather(im, inf, 10, words, dst, 7, 4)
    assert ef.tolist() == [1, 4, 0, 0, 0, 0, 0]  # example 2: 10 frames > ex_rows; 3 and 6: nobody names them; 4 and 5: invalid spans
    assert np.array_equal(ex[1], im[0, 0:4]) and np.array_equal(ex[0, :1], im[0, 4:5]) and not ex[0, 1:].any() and not ex[2:].any()
    ex, ef = ref.gather(im, inf, 10, words, dst, 7, 10)
    assert ef.tolist() == [1, 4, 10, 0, 0, 0, 0] and np.array_equal(ex[2], im[1])
    for bad in ([1, 0, 4, 1, 5, 2], [1, 0, 7, ref.NONE, 5, 2]):
        with pytest.raises(ValueError):
            ref.gather(im, inf, 10, words, bad, 7, 4)


@functools.lru_cache(maxsize=None)
def train_case():
    """the GPU test's case: 16 planted rows, the store = the planted templates + uniform noise of +-500, two iterations"""
    pl = chain_ref.planted(seed=7, n_rows=16)
    tm = ref.noisy_store(pl["tm"], pl["tf"])
    want = ref.train_connected(pl["im"], pl["inf"], pl["seq"], tm, pl["tf"], None, chain_ref.PLANT_MAXF, 2, chain_ref.PLANT_SKIP, 0)
    tm.setflags(write=False)
    return pl, tm, want


def test_train_connected_composition_on_the_planted_rows():
    pl, tm, want = train_case()
    assert sum(len(s) for s in pl["seq"]) == 40
    first = ref.align(pl["im"], pl["inf"], tm, pl["tf"], None, chain_ref.PLANT_MAXF, pl["seq"], 4, chain_ref.PLANT_SKIP, 0)[1]
    got = [[(int(w["start"]), int(w["end"])) for w in first[r, :len(s)]] for r, s in enumerate(pl["seq"])]
    assert got == pl["spans"]  # all 40 spans of the first alignment are the planted ones
    assert want["iters"] == [(16, 845359), (16, 277561)]  # every row parses; the re-averaged templates fit better
    assert not np.array_equal(want["cen"], tm) and want["cen"].shape == tm.shape and np.array_equal(want["frames"], pl["tf"])
    for k in range(chain_ref.PLANT_K):  # rows past a template's frames stay zero
        assert not want["cen"][k, int(pl["tf"][k]):].any()


def test_example_layout_groups_by_word_in_group_order():
    lab = [5, 9, 5, 2]
    dst, ws = ref.example_layout(lab, [[9, 5], [], [5, 5, 2]], 3)
    assert ws.tolist() == [0, 3, 4, 5]  # words in the order of their first slot: 5, 9, 2
    assert dst.tolist() == [3, 0, ref.NONE, ref.NONE, ref.NONE, ref.NONE, 1, 2, 4]
    assert ref.word_groups(lab) [0] == [0, 2, 1, 3] and ref.word_groups(lab)[2] == [5, 9, 2]
    got = Engine.word_groups(words=np.array(lab, np.uint32))
    assert got["order"].tolist() == [0, 2, 1, 3] and got["group_start"].tolist() == [0, 2, 3, 4] and got["word_id"].tolist() == [5, 9, 2]


# ---- 4: the surface (fails without the feature) ------------------------------------------------------------------------------------
def test_header_library_and_python_surface():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    # its own section: after the clustering section, before the delta-MFCC extension
    assert text.index("clustering a word's examples into templates") < text.index("forced alignment against a transcript") < text.index("delta MFCC by the standard")
    assert src.index("sr_cluster_models_dp") < src.index("sr_align_transcripts_dp_dev") < src.index("sr_gather_word_spans") < src.index("sr_delta_mfcc_batch")
    section = text[text.index("forced alignment against a transcript"):text.index("delta MFCC by the standard")]
    flat = re.sub(r"[\s*]+", " ", section[section.index("Out of scope"):])
    for word in ("alternatives per position", "optional words", "live sessions", "device-side store update", "changing template lengths"):
        assert word in flat, word
    assert '"forced_prune_off"' in text[text.index("Development and test hooks"):]
    assert engine.load_library().sr_dev_hook(b"forced_prune_off", C.c_int64(1)) == 3  # not in the product library
    assert b"not compiled into the product library" in engine.load_library().sr_last_error()
    engine.dev_hook("forced_prune_off", 1)
    engine.dev_hook("forced_prune_off", 0)
    for m in ("align_transcripts", "align_transcripts_dev", "gather_word_spans", "gather_word_spans_dev", "train_connected"):
        assert callable(getattr(Engine, m, None)), m


# ---- 5: the planning under the sanitizers ----------------------------------------------------------------------------------------
def test_plan_runs_clean_under_the_sanitizers(tmp_path):
    """the store under the word map, the checks on transcript / n_words / dst_of_span, minlen and tail, the item lists and the
    launch groups (csrc/sr_forced_plan.h) over random corpora against a brute-force restatement: a stand-alone program on the CPU
    under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "forced_plan", "plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
