"""Word-model clustering on the CPU: the restatement (tests/cluster_ref.py) against the DBA trainer's (align_ref.train), against
the scorer's own oracle, and on a planted corpus whose properties the GPU tests rely on; the surface of the feature; the host-only
planning (csrc/sr_cluster_plan.h) under the sanitizers.  No device; tests/test_cluster.py compares the kernels with this
restatement byte for byte.

The planted corpus (cluster_ref.planted): 3 words, each with two random prototypes of lengths (30, 70), (40, 44), (25, 50), six
examples per prototype, each a random monotone resampling to within +-1/8 of the prototype's length plus noise.  Four
initialisations are fixtures, each asserted to have the property it is there for:
  quantile   two models per word seeded by length quantile: iteration 1 recovers the planted partition, iteration 2 moves nobody;
  copy       model 1 of each word a COPY of model 0 (a third model from another example): every tie goes to model 0, the copies
             stay empty in iteration 1 and take examples back in iteration 2 (n_moved > 0 after the first iteration);
  short      both models of the (30, 70) word seeded from its 30-frame prototype: its 70-frame examples can never pass the gate
             (F_m never changes) and stay unassigned in every iteration;
  small      amplitude 2 / noise 1, three models per word: examples whose two best models tie in dis, in every iteration.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import align_ref
import cluster_ref as ref
from oracle_lib import Oracle
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_cluster_assign_dev", "sr_cluster_assign", "sr_cluster_models_dp_dev", "sr_cluster_models_dp")
PLANT_SEED, N_ITER = 6, 3


def tie_count(dis, word_start, mdl_start):
    """examples whose two best models have the same (valid) dis"""
    n = 0
    for e, w in enumerate(ref.word_of(word_start)):
        row = np.sort(dis[e, :int(mdl_start[w + 1]) - int(mdl_start[w])].astype(np.int64))
        n += len(row) >= 2 and row[0] == row[1] and row[0] != ref.DIS_ERR
    return n


@functools.lru_cache(maxsize=None)
def planted_case(name):
    """-> dict(mfcc, frames, word_start, mdl_start, cen, cen_frames, proto_of, want = cluster_ref.cluster(..., N_ITER)); read-only"""
    pl = ref.planted(PLANT_SEED, amp=2, noise=1) if name == "small" else ref.planted(PLANT_SEED)
    ws, fr = pl["word_start"], pl["frames"]
    quant = [ref.default_seeds(fr, np.arange(ws[w], ws[w + 1]), 3 if name == "small" else 2) for w in range(3)]
    if name == "copy":
        seeds = [[q[0], q[0], q[1]] for q in quant]
    elif name == "short":
        seeds = [sorted(range(0, ref.PLANT_TAKES), key=lambda e: fr[e])[:2], quant[1], quant[2]]  # the two shortest takes of prototype 0
    else:
        seeds = quant
    cen, cf, ms = ref.init_from(pl, seeds)
    out = dict(mfcc=pl["mfcc"], frames=fr, word_start=ws, mdl_start=ms, cen=cen, cen_frames=cf, proto_of=pl["proto_of"])
    out["want"] = ref.cluster(pl["mfcc"], fr, ws, ms, cen, cf, N_ITER)
    for a in list(out.values()) + list(out["want"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- 1: one model per word is the DBA trainer ------------------------------------------------------------------------------------
def test_one_model_per_word_is_the_dba_trainer():
    pl = ref.planted(PLANT_SEED)
    ws = pl["word_start"]
    cen, cf, ms = ref.init_from(pl, [[int(ws[w])] for w in range(3)])  # each word starts from its first example, a short one
    got = ref.cluster(pl["mfcc"], pl["frames"], ws, ms, cen, cf, 2)
    want_cen, want_st = align_ref.train(pl["mfcc"], pl["frames"], ws, cen, cf, 2)
    assert np.array_equal(got["cen"], want_cen) and not np.array_equal(want_cen, cen)
    assert np.array_equal(got["stats"]["n_ok"], want_st["n_ok"]) and np.array_equal(got["stats"]["acc"], want_st["acc"])
    assert np.all(got["stats"]["n_fail"] == 0)
    assert got["iter"]["n_unassigned"].tolist() == want_st["n_fail"].sum(1).tolist() and want_st["n_fail"].sum() > 0
    assert np.all(got["iter"]["n_assigned"] + got["iter"]["n_unassigned"] == 36)
    assert got["iter"]["acc"].tolist() == want_st["acc"].sum(1).tolist()
    assert got["iter"]["n_moved"].tolist() == [int(got["iter"]["n_assigned"][0]), 0]  # with one model nobody can move later


# ---- 2: the scores are the scorer's ----------------------------------------------------------------------------------------------
def test_scores_equal_the_full_dp_oracle_on_a_sample_of_pairs():
    fx = planted_case("short")
    orc = Oracle()
    dis = fx["want"]["dis"][0]
    n_err = n_ok = 0
    for e in range(0, 36, 2):
        w = int(ref.word_of(fx["word_start"])[e])
        for c in range(ref.CLUSTER_MAX):
            m = int(fx["mdl_start"][w]) + c
            if m >= fx["mdl_start"][w + 1]:
                assert dis[e, c] == ref.DIS_ERR
                continue
            N, R = int(fx["frames"][e]), int(fx["cen_frames"][m])
            assert dis[e, c] == orc.dtw_dp(fx["mfcc"][e, :N], N, fx["cen"][m, :R], R), (e, m)
            n_err, n_ok = n_err + (dis[e, c] == ref.DIS_ERR), n_ok + (dis[e, c] != ref.DIS_ERR)
    assert n_err >= 4 and n_ok >= 20


# ---- 3: the planted corpus has the properties its cases are there for ----------------------------------------------------------
def test_quantile_init_recovers_the_planted_partition_then_nobody_moves():
    fx = planted_case("quantile")
    w = fx["want"]
    assert w["iter"]["n_moved"].tolist() == [36, 0, 0] and np.all(w["iter"]["n_unassigned"] == 0) and np.all(w["iter"]["n_empty"] == 0)
    for k in range(3):
        a = w["assigns"][0][12 * k:12 * k + 12] - fx["mdl_start"][k]
        p = fx["proto_of"][12 * k:12 * k + 12]
        assert np.array_equal(a, p) or np.array_equal(a, 1 - p), (k, a.tolist())  # (which model got which prototype is the seeds' order)
    assert np.all(w["stats"]["n_ok"] == 6) and not np.array_equal(w["cen"], fx["cen"])
    assert w["iter"]["acc"][1] < w["iter"]["acc"][0]  # the re-averaged centroids are closer to their examples


def test_copy_init_ties_go_to_the_first_model_and_the_copies_fill_later():
    fx = planted_case("copy")
    w, ms = fx["want"], fx["mdl_start"]
    copies = ms[:-1] + 1
    assert np.array_equal(fx["cen"][copies], fx["cen"][copies - 1])
    d0 = w["dis"][0]
    assert np.array_equal(d0[:, 0], d0[:, 1])  # a copy scores as its original ...
    assert tie_count(d0, fx["word_start"], ms) >= 10  # ... and where the pair is the best, that is a tie between different models
    assert np.all(w["stats"]["n_ok"][0][copies] == 0) and w["iter"]["n_empty"][0] == 3 and not np.any(np.isin(w["assigns"][0], copies))
    assert np.all(w["stats"]["n_ok"][1][copies] > 0) and w["iter"]["n_empty"][1] == 0  # empty in one iteration, not in the next
    assert w["iter"]["n_moved"][0] == 36 and w["iter"]["n_moved"][1] > 0               # movement after the first iteration
    assert np.array_equal(w["cen"][copies], fx["cen"][copies]) is False


def test_short_seeds_leave_the_long_examples_unassigned_for_good():
    fx = planted_case("short")
    w = fx["want"]
    long_ones = np.arange(6, 12)  # the 70-frame takes of word 0
    assert np.all(fx["frames"][long_ones] > 2 * fx["cen_frames"][:2].max())  # N > 2R against both models: the gate, whatever the rows hold
    for it in range(N_ITER):
        assert np.all(w["assigns"][it][long_ones] == ref.NONE) and w["iter"]["n_unassigned"][it] >= 6
        assert np.all(w["dis"][it][long_ones] == ref.DIS_ERR)
    assert np.all(w["iter"]["n_assigned"] + w["iter"]["n_unassigned"] == 36)
    assert w["stats"]["n_ok"][:, :2].sum(1).tolist() == [6] * N_ITER  # the short takes are shared between the two models


def test_small_amplitudes_tie_in_every_iteration():
    fx = planted_case("small")
    w = fx["want"]
    assert np.all(np.diff(fx["mdl_start"]) == 3)
    t = [tie_count(d, fx["word_start"], fx["mdl_start"]) for d in w["dis"]]
    assert min(t) >= 4, t
    assert w["iter"]["n_moved"][1] > 0


def test_the_check_restated():
    assert ref.check([0, 4, 4, 9], [0, 2, 3, 19], 80) is None
    for ws, ms in (([1, 4], [0, 1]), ([0, 4], [1, 2]), ([0, 4, 3], [0, 1, 2]), ([0, 4, 5], [0, 2, 1]), ([0, 4], [0, 0]), ([0, 4], [0, 17]),
                   ([0, 820], [0, 1]), ([0], [0])):
        assert ref.check(ws, ms, 80) is not None, (ws, ms)
    assert ref.check([0, 819], [0, 1], 80) is None and ref.check([0, 64], [0, 16], 5000) is not None and ref.check([0, 63], [0, 16], 5000) is None


# ---- 4: the surface ----------------------------------------------------------------------------------------------------------------
def test_header_library_and_python_surface():
    src = open(HEADER).read()
    assert "#define SR_CLUSTER_MAX 16u" in src and "#define SR_CLUSTER_NONE 0xFFFFFFFFu" in src
    body = re.search(r"typedef struct sr_cluster_iter \{(.*?)\} sr_cluster_iter;", src, re.S).group(1)
    assert re.findall(r"(uint\d+_t) (\w+);", body) == [("uint32_t", "n_assigned"), ("uint32_t", "n_unassigned"), ("uint32_t", "n_moved"),
                                                        ("uint32_t", "n_empty"), ("uint64_t", "acc")]
    assert engine.CLUSTER_ITER_DTYPE == ref.ITER_DTYPE and ref.ITER_DTYPE.itemsize == 24 and engine.CLUSTER_MAX == ref.CLUSTER_MAX
    for lib in (engine.load_library(), engine.load_library(testing=True)):
        for f in FUNCS:
            assert f in src and hasattr(lib, f), f
    assert engine.load_library().sr_dev_hook(b"cluster_pairs", C.c_int64(1)) == 3  # not in the product library
    engine.dev_hook("cluster_pairs", 7)
    engine.dev_hook("cluster_pairs", 0)
    for m in ("cluster_assign", "cluster_assign_dev", "cluster_models", "cluster_models_dev", "cluster_words"):
        assert callable(getattr(Engine, m)), m
    flat = re.sub(r"[\s*]+", " ", src)  # the header's out-of-scope list
    for word in ("choosing the number of clusters", "splitting or merging clusters", "changing a centroid's length", "clustering across words"):
        assert word in flat, word


# ---- 5: the planning under the sanitizers ----------------------------------------------------------------------------------------
def test_plan_runs_clean_under_the_sanitizers(tmp_path):
    """the checks on word_start / mdl_start, the per-example model ranges, the score pass's workgroups and their launches
    (csrc/sr_cluster_plan.h) over random corpora: a stand-alone program on the CPU under AddressSanitizer and
    UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cluster_plan", "plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
