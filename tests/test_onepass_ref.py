"""One-pass connected-word decoding on the CPU: the restatement (tests/onepass_ref.py) stated time-synchronously and in the
kernels' block form, held equal for every block length 1..L and shown to differ beyond L; its relation to level building
(tests/chain_ref.py); the long planted rows that level building cannot hold; the surface of the feature; and the host-only
planning (csrc/sr_onepass_plan.h) under the sanitizers.  No device; tests/test_onepass.py compares the kernels with this
restatement byte for byte.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import chain_ref
import onepass_ref as ref
from spot_ref import local_dis
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_decode_onepass_dp_dev", "sr_decode_onepass_dp", "sr_decode_onepass_batch", "sr_decode_onepass_geometry")
HOOKS = ("onepass_block", "onepass_rows")
SKIPS = (1500, None, 0, 300)
WORD_COSTS = (0, 5000)


@functools.lru_cache(maxsize=None)
def planted_dis(r):
    pl = chain_ref.planted()
    N = int(pl["inf"][r])
    return N, tuple(local_dis(pl["im"][r, :N], pl["tm"][k, :int(pl["tf"][k])]) for k in range(chain_ref.PLANT_K))


# ---- 1: the two statements of the history -----------------------------------------------------------------------------------------
def test_block_form_equals_the_time_synchronous_form_up_to_L_and_not_beyond():
    pl = chain_ref.planted()
    L = ref.reach(pl["tf"])
    assert L == 5 == min(int(m) for m in pl["tf"]) // 2 + 1
    differs = 0
    for r in range(chain_ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        for skip, wc in ((1500, 0), (None, 5000), (300, 5000)):
            want = ref.history_sync(dis, N, skip, wc)
            for n in range(1, L + 1):
                assert ref.history_blocks(dis, N, n, skip, wc) == want, (r, skip, wc, n)
            assert ref.history_blocks(dis, N, L, skip, wc, cap=N + 7) == want  # the host's bound may lie above the row
            differs += ref.history_blocks(dis, N, L + 1, skip, wc) != want
    assert differs >= 6  # the bound is tight: one frame more and words that start inside a block are missed


# ---- 2: relation to level building ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wc", WORD_COSTS)
@pytest.mark.parametrize("skip", SKIPS)
def test_cost_is_the_minimum_over_the_levels_and_the_words_are_level_buildings(skip, wc):
    pl = chain_ref.planted()
    n_words = 0
    for r in range(chain_ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        lv = chain_ref.decode_row(list(dis), N, 16, 0, skip, wc)
        got = ref.decode_row(list(dis), N, skip, wc)
        costs = [c for c in lv["level_cost"] if c is not None] + ([N * skip] if skip is not None else [])
        if not costs:
            assert got["status"] == ref.CH_NONE
            continue
        assert got["status"] == ref.CH_OK and got["cost"] == min(costs), r
        if lv["status"] == chain_ref.CH_OK and lv["cost"] == min(costs):  # (a row cheaper as filler alone has no level to compare)
            assert got["words"] == lv["words"] and got["skipped"] == lv["skipped"], r
            n_words += got["n_words"]
        else:
            assert got["n_words"] == 0 and got["skipped"] == N
    if skip in (1500, None):  # (at skip 0 and 300 filler is cheaper than most words)
        assert n_words >= 12


def test_a_row_cheaper_as_filler_is_nothing_was_said():
    rng = np.random.default_rng(5)
    d = [rng.integers(900, 1000, (30, 9))]
    got = ref.decode_row(d, 30, 10, 0)
    assert (got["status"], got["cost"], got["n_words"], got["skipped"], got["words"]) == (ref.CH_OK, 300, 0, 30, [])
    assert ref.decode_row(d, 3, None, 0)["status"] == ref.CH_NONE and ref.decode_row(d, 0, 10, 0)["status"] == ref.CH_NONE
    assert ref.decode_row(d, 3, 10, 0)["cost"] == 30  # shorter than any word's reach


# ---- 3: rows that level building cannot hold --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_want(skip):
    pl = ref.planted_long()
    want = ref.decode(pl["im"], pl["inf"], pl["tm"], pl["tf"], None, ref.LONG_MAXF, 64, skip, 0)
    for a in want:
        a.setflags(write=False)
    return want


def test_planted_long_rows_are_recovered():
    pl = ref.planted_long()
    assert pl["inf"].tolist() == [303, 384, 591, 702] and [len(s) for s in pl["seq"]] == list(ref.LONG_COUNTS)
    rec, words = long_want(chain_ref.PLANT_SKIP)
    assert np.all(rec["status"] == ref.CH_OK) and rec["n_words"].tolist() == list(ref.LONG_COUNTS)
    for r, seq in enumerate(pl["seq"]):
        assert words[r, :len(seq)]["slot"].tolist() == seq, r
        assert [(int(w["start"]), int(w["end"])) for w in words[r, :len(seq)]] == pl["spans"][r], r
        assert np.all(words[r, len(seq):].view(np.uint32) == 0xFFFFFFFF)


def test_truncation_keeps_the_first_words_and_the_true_count():
    pl = chain_ref.planted()
    full = ref.decode(pl["im"], pl["inf"], pl["tm"], pl["tf"], None, chain_ref.PLANT_MAXF, 8, chain_ref.PLANT_SKIP, 0)
    cut = ref.decode(pl["im"], pl["inf"], pl["tm"], pl["tf"], None, chain_ref.PLANT_MAXF, 2, chain_ref.PLANT_SKIP, 0)
    assert np.array_equal(cut[0]["n_words"], full[0]["n_words"]) and np.array_equal(cut[0]["cost"], full[0]["cost"])
    assert cut[0]["status"].tolist() == [ref.CH_TRUNCATED if n > 2 else ref.CH_OK for n in full[0]["n_words"]]
    assert (cut[0]["status"] == ref.CH_TRUNCATED).sum() == 6 and cut[1].tobytes() == full[1][:, :2].tobytes()
    with pytest.raises(ValueError):
        ref.decode(pl["im"], pl["inf"], pl["tm"], pl["tf"], None, 16383, 8, None, 1 << 24, frames_cap=0)  # 3276 words x 2^24


# ---- 4: the surface (fails without the feature) -------------------------------------------------------------------------------------
def test_header_library_and_python_surface():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert re.search(r"#define SR_CH_TRUNCATED 2u", src) and engine.CH_TRUNCATED == ref.CH_TRUNCATED == 2
    section = re.sub(r"[\s*]+", " ", text[text.index("one-pass connected-word decoding: no word cap"):text.index("delta MFCC by the standard")])
    for phrase in ("Byte equality with the level decoder is NOT promised", "fewest words globally", "traces locally", "M / 2 + 1",
                   "E(N) = min(N skip_cost when skipping is on, min over n >= 1 of E_n(N))"):
        assert phrase in section, phrase
    hooks = text[text.index("Development and test hooks"):]
    blob = open(engine.LIB_PATH, "rb").read()
    for hook in HOOKS:
        assert '"%s"' % hook in hooks, hook
        engine.dev_hook(hook, 0)  # the testing library knows the hook ...
        assert engine.load_library().sr_dev_hook(hook.encode(), C.c_int64(1)) == 3  # ... the product library has none,
        assert b"not compiled into the product library" in engine.load_library().sr_last_error()
        assert hook.encode() + b"\0" not in blob, hook                                 # not even its name
    for m in ("decode_onepass", "decode_onepass_dev", "decode_onepass_pcm"):
        assert callable(getattr(Engine, m, None)), m
    assert callable(engine.decode_onepass_geometry)


def test_geometry_state_rows_block_and_launches():
    g = engine.decode_onepass_geometry(120, 100, 2048, 80)
    assert g["state_bytes"] == 2049 * 12 + 100 * 120 * 16 and g["rows"] == (256 << 20) // g["state_bytes"]
    assert g["block"] == 41 and g["launches"] == 2 * -(-2048 // 41) + 2 == 102
    g = engine.decode_onepass_geometry(15, 5, 160, 8)
    assert g == dict(state_bytes=161 * 12 + 5 * 15 * 16, rows=65535, block=5, launches=66)
    L, out = engine.load_library(), (C.c_uint32 * 4)()
    for a in ((0, 5, 160, 8), (15, 0, 160, 8), (15, 65537, 160, 8), (15, 5, 1, 8), (15, 5, 16384, 8), (15, 5, 160, 0), (15, 5, 160, 16)):
        assert L.sr_decode_onepass_geometry(*(C.c_uint32(v) for v in a), out) == 3, a
    assert L.sr_decode_onepass_geometry(*(C.c_uint32(v) for v in (15, 5, 160, 8)), None) == 3
    try:  # the hooks: a block is clamped to 1..L
        for block, want in ((1, 1), (3, 3), (5, 5), (6, 5), (1000, 5)):
            engine.dev_hook("onepass_block", block)
            assert engine.decode_onepass_geometry(15, 5, 160, 8, testing=True)["block"] == want
        engine.dev_hook("onepass_block", 2)
        engine.dev_hook("onepass_rows", 3)
        g = engine.decode_onepass_geometry(15, 5, 160, 8, testing=True)
        assert g["rows"] == 3 and g["launches"] == 162
    finally:
        for h in HOOKS:
            engine.dev_hook(h, 0)


# ---- 5: the planning under the sanitizers ----------------------------------------------------------------------------------------
def test_plan_runs_clean_under_the_sanitizers(tmp_path):
    """the block length, the word-cost bound, the block list and the launch groups (csrc/sr_onepass_plan.h) over random stores
    and frame bounds against a brute-force restatement: a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "onepass_plan", "plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
