"""Live one-pass connected-word decoding on the CPU: the surface of the feature, the geometry formulas, the restatement
(tests/onepass_live_ref.py) held to onepass_ref's time-synchronous history for every chunking, the prefix property that gives
every push's row from one history, the tail form, and the host-only planning (csrc/sr_onepass_live_plan.h) under the
sanitizers.  No device; tests/test_onepass_live.py compares the kernels with this restatement byte for byte.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import chain_ref
import onepass_live_ref as live
import onepass_ref as ref
from spot_ref import local_dis
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_onepass_live_geometry", "sr_onepass_live_open", "sr_onepass_live_push_dev", "sr_onepass_live_push",
         "sr_onepass_live_push_pcm_dev", "sr_onepass_live_push_pcm", "sr_onepass_live_end")
BAD_ARG = 3
U32 = C.c_uint32
COSTS = ((1500, 0), (None, 5000), (300, 5000))


# ---- the surface (fails without the feature) -----------------------------------------------------------------------------------
def test_header_declares_the_live_one_pass_api_and_libraries_export_it():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert re.search(r"\bvoid sr_onepass_live_close\s*\(", src)
    assert hasattr(engine.load_library(), "sr_onepass_live_close") and hasattr(engine.load_library(True), "sr_onepass_live_close")
    assert src.index("sr_decode_onepass_geometry") < src.index("sr_onepass_live_geometry")  # after the one-pass section
    assert re.search(r"#define SR_OP_LIVE_TAIL 1u", src) and engine.OP_LIVE_TAIL == 1
    assert "a live (push) form" not in open(HEADER).read()  # no longer out of the one-pass section's scope
    assert callable(getattr(Engine, "decode_onepass_live", None)) and callable(engine.onepass_live_geometry)
    for meth in ("push", "push_dev", "push_pcm", "push_pcm_dev", "end", "close"):
        assert callable(getattr(engine.OnePassSession, meth, None)), meth
    assert isinstance(engine.OnePassSession.frames, property)
    assert engine.CHAIN_LIVE_ROW_DTYPE == live.CHAIN_LIVE_ROW_DTYPE
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for unit in ("k_onepass_live.hip", "sr_onepass_live.cpp", "sr_onepass_live_plan.h"):
        assert unit in mk, unit


def test_geometry_follows_its_formulas():
    cap = engine.spot_geometry(10, 119)["max_tpl_rows"]
    for tpl, K, mn, utt, chunk in ((15, 9, 8, 200, 64), (1, 1, 1, 1, 1), (120, 100, 80, 2000, 100), (90, 3, 70, 16383, 16383), (14, 5, 8, 160, 13)):
        g = engine.onepass_live_geometry(tpl, K, mn, utt, chunk)
        L = mn // 2 + 1
        assert g["state_bytes"] == (utt + 1) * 12 + K * tpl * 16 + utt * 24, (tpl, K, utt)
        assert g["max_tpl_rows"] == cap and g["block"] == L
        assert g["launches"] == 2 * -(-chunk // L) + 1 <= 2 * -(-chunk // L) + 2
        assert g["block"] == engine.decode_onepass_geometry(tpl, K, max(utt, 2), mn)["block"]  # the batch decoder's L
    # per channel: one saved column per slot and ONE history, against the level session's max_words of each
    lv = engine.decode_live_geometry(120, 100, 8, 2000, 100)
    op = engine.onepass_live_geometry(120, 100, 80, 2000, 100)
    assert op["state_bytes"] < lv["state_bytes"] / 4 and op["launches"] == 7 < lv["launches"] == 18
    assert engine.onepass_live_geometry(16383, 65536, 1, 16383, 1)["state_bytes"] == 0xFFFFFFFF  # saturates
    try:  # the testing library's hook caps the live block length too
        engine.dev_hook("onepass_block", 2)
        g = engine.onepass_live_geometry(14, 5, 8, 160, 13, testing=True)
        assert g["block"] == 5 and g["launches"] == 2 * 7 + 1
    finally:
        engine.dev_hook("onepass_block", 0)
    L, out = engine.load_library(), (U32 * 4)()
    for bad in ((0, 1, 1, 1, 1), (16384, 1, 1, 1, 1), (10, 0, 1, 1, 1), (10, 65537, 1, 1, 1), (10, 1, 0, 1, 1), (10, 1, 11, 1, 1), (10, 1, 1, 0, 1),
                (10, 1, 1, 16384, 1), (10, 1, 1, 10, 0), (10, 1, 1, 10, 11)):
        assert L.sr_onepass_live_geometry(*(U32(v) for v in bad), out) == BAD_ARG, bad
    assert L.sr_onepass_live_geometry(U32(10), U32(1), U32(1), U32(10), U32(1), None) == BAD_ARG


# ---- the design ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_dis(r):
    pl = chain_ref.planted()
    N = int(pl["inf"][r])
    return N, tuple(local_dis(pl["im"][r, :N], pl["tm"][k, :int(pl["tf"][k])]) for k in range(chain_ref.PLANT_K))


@functools.lru_cache(maxsize=None)
def planted_history(r, skip, wc):
    N, dis = planted_dis(r)
    return ref.history_sync(dis, N, skip, wc)


def random_cuts(rng, N, hi):
    """push sizes 0..hi that sum to N, zeros included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(1, hi + 1))])), N - sum(out)))
    return out


def test_pushes_cut_into_blocks_keep_the_time_synchronous_history():
    """12 planted rows x 3 cost settings x (3 random chunkings of 1..13 frames, one-frame pushes, one whole-row push): every
    history equals history_sync; so does one whose pushes are cut into shorter blocks, of a length that changes between pushes"""
    pl = chain_ref.planted()
    L = ref.reach(pl["tf"])
    assert L == 5
    rng = np.random.default_rng(2024)
    sizes, n_hist = set(), 0
    for r in range(chain_ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        for skip, wc in COSTS:
            want = planted_history(r, skip, wc)
            for cuts in [random_cuts(rng, N, 13) for _ in range(3)] + [[1] * N, [N]]:
                assert live.history_pushes(dis, N, cuts, L, skip, wc) == want, (r, skip, wc, cuts)
                sizes.update(cuts)
                n_hist += 1
            cuts = random_cuts(rng, N, 13)
            ch = live.Channel(len(dis), L, skip, wc)
            at = 0
            for n in cuts:  # the block length of a push is the caller's business as long as it is at most L
                ch.push([d[at:at + n] for d in dis], int(rng.integers(1, L + 1)))
                at += n
            assert (ch.A, ch.E) == want, (r, skip, wc, cuts)
    assert n_hist == 12 * 3 * 5 and {0, 1, 5, 6, 13} <= sizes and max(sizes) > 60


def test_blocks_longer_than_L_are_wrong():
    """the bound is tight in the live form as well: pushes cut into blocks of L + 1 frames miss words"""
    pl = chain_ref.planted()
    L = ref.reach(pl["tf"])
    differs = 0
    for r in range(chain_ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        ch = live.Channel(len(dis), L + 1, 1500, 0)
        ch.push(list(dis))
        differs += (ch.A, ch.E) != planted_history(r, 1500, 0)
    assert differs >= 2


def test_one_history_gives_every_pushs_row():
    """the prefix property: A and E of a prefix are a prefix of the history, so trace_row at N is the parse of the first N frames"""
    for r in range(chain_ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        for skip, wc in COSTS if r < 3 else COSTS[:1]:
            A, E = planted_history(r, skip, wc)
            ch = live.Channel(len(dis), 5, skip, wc)
            for n in sorted({0, 1, 4, 5, 6, N} | set(range(0, N + 1, 9))):
                a, e = ref.history_sync([d[:n] for d in dis], n, skip, wc)
                assert (a, e) == (A[:n + 1], E[:n + 1]), (r, n)
                assert ref.trace_row(A, E, n, wc) == ref.decode_row([d[:n] for d in dis], n, skip, wc), (r, n)
            at = 0
            for n in random_cuts(np.random.default_rng(r), N, 13):  # ... and a channel says the same after every push
                got = ch.push([d[at:at + n] for d in dis])
                at += n
                assert got == ref.trace_row(A, E, at, wc), (r, skip, wc, at)


def test_rows_head_and_tail():
    """to_records: the batch call's rows for the head form; the tail form is words[-words_cap:], the record the same"""
    pl = chain_ref.planted()
    tm, tf = pl["tm"], pl["tf"]
    batch = ref.decode(pl["im"], pl["inf"], tm, tf, None, chain_ref.PLANT_MAXF, 2, 1500, 0)
    full = ref.decode(pl["im"], pl["inf"], tm, tf, None, chain_ref.PLANT_MAXF, 16, 1500, 0)
    n_trunc = 0
    for r in range(chain_ref.PLANT_ROWS):
        N = int(pl["inf"][r])
        rec = live.Recording(pl["im"][r, :N], tm, tf, None, 2, 1500, 0)
        head, tail = rec.row(N), rec.row(N, tail=True)
        assert head[0].tobytes() == batch[0][r].tobytes() and head[1].tobytes() == batch[1][r].tobytes(), r
        assert tail[0].tobytes() == head[0].tobytes()
        n = int(full[0][r]["n_words"])
        want = np.empty(2, ref.CHAIN_WORD_DTYPE)
        want[...] = ref.NO_WORD_ROW
        want[:min(n, 2)] = full[1][r, max(n - 2, 0):n]
        assert tail[1].tobytes() == want.tobytes(), r
        n_trunc += n > 2
        assert rec.row(0)[0]["status"] == ref.CH_NONE and np.all(rec.row(0)[1].view(np.uint32) == 0xFFFFFFFF)
        wide = rec.row(N, 16)
        assert wide[0].tobytes() == full[0][r].tobytes() and wide[1].tobytes() == full[1][r].tobytes() == rec.row(N, 16, True)[1].tobytes()
    assert n_trunc >= 6


def test_host_mirror_runs_clean_under_the_sanitizers(tmp_path):
    """the cut of every push into blocks against a frame-by-frame model, the refusals and their order, the end list and what it
    wipes, the geometry formulas (csrc/sr_onepass_live_plan.h): a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "onepass_live_plan", "plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
