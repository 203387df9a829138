"""Word-model clustering on the GPU (include/sr_engine.h, "word models: clustering a word's examples into templates").

The definition lives in tests/cluster_ref.py (numpy, on top of align_ref.align_pair; tests/test_cluster_ref.py checks it against
the DBA trainer's restatement and the scorer's oracle, and asserts the properties of the planted corpus).  Everything here is
compared with it byte for byte: score rows, assignments, centroids, statistics, iteration records.

An edge case is a list of words; a word is (examples, models): examples a list of (N, kind), models a list of frame counts R.
kind "rand" draws the rows, "const" makes the word's examples +amp and its models -amp (every cell of every pair ties),
"same" makes the example a copy of the word's LAST model.  N above max_frames, R = 0 and R above cen_rows are cases.  Small
coefficients (amp 2) make ties between models common, amp 3000 is the usual range, amp 32767 is full scale.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cluster_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from oracle_lib import Oracle
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine
from test_cluster_ref import N_ITER, planted_case

BAD_CONFIG, BAD_ARG = 2, 3
U32, P = C.c_uint32, C.c_void_p
NONE = ref.NONE


class pairs_per_launch:
    """development hook "cluster_pairs" (testing library only; read per call)"""

    def __init__(self, pairs):
        self.pairs = pairs

    def __enter__(self):
        engine.dev_hook("cluster_pairs", self.pairs)

    def __exit__(self, *exc):
        engine.dev_hook("cluster_pairs", 0)


def dev(a):
    """a device copy of a numpy array (fixtures are read-only: copy first)"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        flat_g, flat_w = got.reshape(len(got), -1), want.reshape(len(want), -1)
        bad = [i for i in range(len(got)) if flat_g[i].tobytes() != flat_w[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rows differ, first at {bad[0]}: got {flat_g[bad[0]].tolist()[:16]} "
                             f"want {flat_w[bad[0]].tolist()[:16]}")


# ---- the two calls into guarded buffers --------------------------------------------------------------------------------------
def dev_assign(eng, fx, canary=0xA5, want_best=True, want_scores=True, frames_stride=1, d_frames=None, mfcc=None, cen=None):
    """sr_cluster_assign_dev -> (assign uint32 [E], best or None, scores [E, 16] or None)"""
    E = int(fx["word_start"][-1])
    d_im, d_cen, d_cf = dev(fx["mfcc"] if mfcc is None else mfcc), dev(fx["cen"] if cen is None else cen), dev(fx["cen_frames"])
    if d_frames is None:
        d_frames = dev(fx["frames"])
    g_as = guarded_out((E,), np.uint32, canary, 4096, "cuda:0", "assign")
    g_best = guarded_out((E,), np.uint32, canary, 4096, "cuda:0", "best")
    g_sc = guarded_out((E, ref.CLUSTER_MAX), np.uint32, canary, 4096, "cuda:0", "scores")
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_cluster_assign_dev(eng.h, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(frames_stride), engine._vp(fx["word_start"]),
                                     engine._vp(fx["mdl_start"]), U32(len(fx["word_start"]) - 1), P(d_cen.data_ptr()), P(d_cf.data_ptr()),
                                     U32(d_cen.shape[1]), P(g_as.ptr), P(g_best.ptr) if want_best else None,
                                     P(g_sc.ptr) if want_scores else None, P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    g_as.check()
    g_best.check() if want_best else g_best.check_untouched()
    g_sc.check() if want_scores else g_sc.check_untouched()
    return g_as.interior(), g_best.interior() if want_best else None, g_sc.interior() if want_scores else None


def dev_models(eng, fx, n_iter, canary=0xA5, want=("assign", "stats", "iter"), frames_stride=1, d_frames=None, mfcc=None, cen=None):
    """sr_cluster_models_dp_dev -> dict(cen, assign, stats, iter); an output left out of `want` is passed as NULL (-> None)"""
    E, M = int(fx["word_start"][-1]), int(fx["mdl_start"][-1])
    d_im, d_cen, d_cf = dev(fx["mfcc"] if mfcc is None else mfcc), dev(fx["cen"] if cen is None else cen), dev(fx["cen_frames"])
    if d_frames is None:
        d_frames = dev(fx["frames"])
    g = dict(cen=guarded_out(fx["cen"].shape, np.int16, canary, 4096, "cuda:0", "cen_out"),
             assign=guarded_out((E,), np.uint32, canary, 4096, "cuda:0", "assign"),
             stats=guarded_out((n_iter, M), ref.TRAIN_STAT_DTYPE, canary, 4096, "cuda:0", "stats"),
             iter=guarded_out((n_iter,), ref.ITER_DTYPE, canary, 4096, "cuda:0", "iter"))
    opt = {k: (P(g[k].ptr) if k in want else None) for k in ("assign", "stats", "iter")}
    sid = torch.cuda.current_stream().cuda_stream
    rc = eng.L.sr_cluster_models_dp_dev(eng.h, P(d_im.data_ptr()), P(d_frames.data_ptr()), U32(frames_stride), engine._vp(fx["word_start"]),
                                        engine._vp(fx["mdl_start"]), U32(len(fx["word_start"]) - 1), P(d_cen.data_ptr()), P(d_cf.data_ptr()),
                                        U32(d_cen.shape[1]), U32(n_iter), P(g["cen"].ptr), opt["assign"], opt["stats"], opt["iter"], P(sid))
    assert rc == 0, eng.L.sr_last_error()
    torch.cuda.synchronize()
    out = {}
    for k, b in g.items():
        if k == "cen" or k in want:
            b.check()
            out[k] = b.interior()
        else:
            b.check_untouched()
            out[k] = None
    return out


def same_models(got, want, n_iter, what):
    """a dev_models result against cluster_ref.cluster's first n_iter iterations (want computed with at least n_iter)"""
    if got["assign"] is not None:
        same(got["assign"], want["assigns"][n_iter - 1], what + ": assign")
    if got["stats"] is not None:
        same(got["stats"], want["stats"][:n_iter], what + ": stats")
    if got["iter"] is not None:
        same(got["iter"], want["iter"][:n_iter], what + ": iter")


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
EDGE_MAXF, EDGE_ROWS = 130, 131
EDGE_N, EDGE_R = (1, 2, 63, 64, 65, 128, 130), (1, 2, 15, 16, 17, 33, 65)  # sweep seams, the boundary column, the wave's last lane
R = "rand"
EDGE_WORDS = tuple(
    [([(N, R)], list(EDGE_R)) for N in EDGE_N]                                       # words 0..6: one example, seven models
    # 7..11 the gate's edges: N = 2R passes, 2R + 1 does not; 2N = R passes, 2N = R - 1 does not (then the second model takes it)
    + [([(66, R)], [33]), ([(67, R)], [33]), ([(8, R)], [16]), ([(8, R)], [17]), ([(8, R)], [17, 16])]
    # 12..14 pairs that are all ties; two models that tie as wholes
    + [([(64, "const")], [64, 64]), ([(65, "const"), (100, "const")], [33, 130, 65]), ([(2, "const")], [3, 1, 3])]
    # 15..17 a copy of the last model scores 0
    + [([(65, "same")], [65, 65]), ([(130, "same")], [65, 130]), ([(1, "same")], [2, 1])]
    # 18..21 centroids with frame count 0 and above cen_rows; an empty row
    + [([(10, R)], [0]), ([(10, R)], [0, 140, 12]), ([(10, R)], [140, 132]), ([(0, R)], [10])]
    # 22 a count above max_frames is clamped to 130
    + [([(300, R)], [70, 100])]
    # 23..27 model counts 1, 2, 3, 16 and 0, 1, 4, 5 examples: not a multiple of a workgroup's four waves
    + [([(40, R)] * 5, [20 + 4 * i for i in range(16)]), ([], [30, 31]), ([(50, R), (45, R), (90, R), (30, R)], [40, 50, 60]),
       ([(33, R), (64, R), (65, R), (17, R), (70, R)], [60]), ([(20, R)], [25, 40])])


def build_edge(words, amp, maxf, rows, seed):
    rng = np.random.default_rng(seed)
    ex = [(w, N, kind) for w, (exs, _) in enumerate(words) for N, kind in exs]
    md = [(w, F) for w, (_, mdl) in enumerate(words) for F in mdl]
    mfcc = rng.integers(-amp, amp + 1, (len(ex), maxf, 12)).astype(np.int16)
    cen = rng.integers(-amp, amp + 1, (len(md), rows, 12)).astype(np.int16)
    word_start = np.concatenate(([0], np.cumsum([len(e) for e, _ in words]))).astype(np.uint32)
    mdl_start = np.concatenate(([0], np.cumsum([len(m) for _, m in words]))).astype(np.uint32)
    for m, (w, F) in enumerate(md):
        if words[w][0] and words[w][0][0][1] == "const":
            cen[m] = -amp
    for e, (w, N, kind) in enumerate(ex):
        if kind == "const":
            mfcc[e] = amp
        elif kind == "same":
            last = int(mdl_start[w + 1]) - 1
            n = min(N, maxf, rows)
            mfcc[e, :n] = cen[last, :n]
    frames = np.array([N for _, N, _ in ex], np.uint32)
    cen_frames = np.array([F for _, F in md], np.uint32)
    dis, _, _ = ref.score(mfcc, frames, word_start, mdl_start, cen, cen_frames)
    assign, best, _ = ref.assign_rows(dis, word_start, mdl_start)
    out = dict(mfcc=mfcc, frames=frames, cen=cen, cen_frames=cen_frames, word_start=word_start, mdl_start=mdl_start, dis=dis, assign=assign, best=best)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_fixture(amp):
    fx = build_edge(EDGE_WORDS, amp, EDGE_MAXF, EDGE_ROWS, 1500 + amp)
    ws, ms, a, d = fx["word_start"], fx["mdl_start"], fx["assign"], fx["dis"]
    one = lambda w: int(a[ws[w]])  # noqa: E731  (the assignment of a one-example word)
    assert len(EDGE_N) == 7 and all(ws[w + 1] - ws[w] == 1 and ms[w + 1] - ms[w] == 7 for w in range(7))
    assert one(7) == ms[7] and one(8) == NONE and one(9) == ms[9] and one(10) == NONE and one(11) == ms[11] + 1
    assert one(12) == ms[12] and d[ws[12], 0] == d[ws[12], 1] != DIS_ERR      # two models tie as wholes: the first one
    assert one(14) == ms[14] and d[ws[14], 0] == d[ws[14], 2] != DIS_ERR
    for w in (15, 16, 17):
        assert one(w) == ms[w + 1] - 1 and fx["best"][ws[w]] == 0, w            # the copy's score is 0
    assert one(18) == NONE and one(19) == ms[19] + 2 and one(20) == NONE and one(21) == NONE
    assert one(22) != NONE and np.all(d[ws[22], :2] != DIS_ERR)                 # 300 frames: clamped to 130, which both models admit
    assert ms[24] - ms[23] == 16 and ws[24] - ws[23] == 5 and ws[25] == ws[24] and ws[26] - ws[25] == 4 and ws[27] - ws[26] == 5
    assert np.all(d[ws[23]:ws[24]] != DIS_ERR) and len(set(a[ws[23]:ws[24]].tolist())) >= (2 if amp > 2 else 1)
    assert (a == NONE).sum() >= 6 and (a != NONE).sum() >= 25
    for e, w in enumerate(ref.word_of(ws)):
        assert np.all(d[e, int(ms[w + 1] - ms[w]):] == DIS_ERR)
    return fx


def all_pairs(fx):
    """every (example, model of its word) pair -> (example rows, model indices, score-row columns)"""
    pe, pm, pc = [], [], []
    for e, w in enumerate(ref.word_of(fx["word_start"])):
        for c, m in enumerate(range(int(fx["mdl_start"][w]), int(fx["mdl_start"][w + 1]))):
            pe.append(e), pm.append(m), pc.append(c)
    return np.array(pe), np.array(pm, np.uint32), np.array(pc)


# ---- GPU 1: the stage, one case per place the kernels can go wrong -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("amp", [2, 3000, 32767])
def test_score_and_assign_edges(amp):
    fx = edge_fixture(amp)
    eng = Engine(max_frames=EDGE_MAXF, device=0, testing=True)
    for i, pairs in enumerate((0, 1, 7)):  # one launch; a launch per pair; launches that split words and workgroups
        with pairs_per_launch(pairs):
            assign, best, scores = dev_assign(eng, fx, CANARIES[i % 2])
        same(scores, fx["dis"], f"scores, {pairs} pairs per launch")
        same(assign, fx["assign"], f"assign, {pairs} pairs per launch")
        same(best, fx["best"], f"best, {pairs} pairs per launch")
    assign, none, none2 = dev_assign(eng, fx, 0x3C, want_best=False, want_scores=False)  # the optional outputs left out
    same(assign, fx["assign"], "assign alone")
    h_as, h_best, h_sc = eng.cluster_assign(fx["mfcc"], fx["frames"], fx["word_start"], fx["mdl_start"], fx["cen"], fx["cen_frames"])  # host form
    assert h_as.tobytes() == fx["assign"].tobytes() and h_best.tobytes() == fx["best"].tobytes() and h_sc.tobytes() == fx["dis"].tobytes()
    h_as, h_best, h_sc = eng.cluster_assign(fx["mfcc"], fx["frames"], fx["word_start"], fx["mdl_start"], fx["cen"], fx["cen_frames"], want_scores=False)
    assert h_as.tobytes() == fx["assign"].tobytes() and h_best.tobytes() == fx["best"].tobytes() and h_sc is None
    # the aligner's dis of the same pairs, on the device
    pe, pm, pc = all_pairs(fx)
    rec, _ = eng.align(fx["mfcc"][pe], fx["frames"][pe], fx["cen"], fx["cen_frames"], ref_of_row=pm, want_span=False)
    assert np.array_equal(rec["dis"], scores[pe, pc]) and (rec["dis"] != DIS_ERR).sum() >= 100 and (rec["dis"] == DIS_ERR).sum() >= 20
    eng.close()


@pytest.mark.gpu
def test_a_row_above_the_aligner_cap_is_unassigned():
    maxf, rows = 1100, 70
    fx = build_edge((([(1050, R), (60, R), (5000, R)], [64, 70]), ([(1024, R)], [64])), 2, maxf, rows, 1600)
    assert fx["assign"].tolist()[0] == NONE and fx["assign"].tolist()[2:] == [NONE, NONE] and fx["assign"][1] in (0, 1)
    assert np.all(fx["dis"][[0, 2, 3]] == DIS_ERR)  # TOO_LONG twice (1050; 5000 clamped to 1100), and 1024 against 64 fails the gate
    eng = Engine(max_frames=maxf, device=0)
    assign, best, scores = dev_assign(eng, fx)
    same(scores, fx["dis"], "scores")
    same(assign, fx["assign"], "assign")
    same(best, fx["best"], "best")
    eng.close()


# ---- GPU 2: the full operation on the planted corpus -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quantile", "copy", "short", "small"])
def test_planted_corpus_centroids_assignments_and_records(case):
    fx = planted_case(case)
    want = fx["want"]
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0)
    got = dev_models(eng, fx, N_ITER, CANARIES[0])
    same_models(got, want, N_ITER, case)
    same(got["cen"], want["cen"], case + ": centroids")
    eng.close()


# ---- GPU 3: identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_model_per_word_reproduces_the_trainer():
    fx = dict(planted_case("quantile"))
    ws = fx["word_start"]
    firsts = [int(ws[w]) for w in range(3)]  # each word starts from its first example, a short one: the long takes fail the gate
    fx["cen"], fx["cen_frames"], fx["mdl_start"] = ref.init_from(dict(mfcc=fx["mfcc"], frames=fx["frames"]), [[e] for e in firsts])
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0)
    got = dev_models(eng, fx, 3)
    d_out = torch.zeros(fx["cen"].shape, dtype=torch.int16, device="cuda:0")
    d_st = torch.zeros((3, 3, 4), dtype=torch.int32, device="cuda:0")
    eng.train_models_dev(dev(fx["mfcc"]), dev(fx["frames"]), ws, dev(fx["cen"]), dev(fx["cen_frames"]), d_out, n_iter=3, stats=d_st)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy().view(ref.TRAIN_STAT_DTYPE).reshape(3, 3)
    assert got["cen"].tobytes() == d_out.cpu().numpy().tobytes()
    assert np.array_equal(got["stats"]["n_ok"], st["n_ok"]) and np.array_equal(got["stats"]["acc"], st["acc"]) and np.all(got["stats"]["n_fail"] == 0)
    assert got["iter"]["n_unassigned"].tolist() == st["n_fail"].sum(1).tolist() and st["n_fail"].sum() > 0
    eng.close()


@pytest.mark.gpu
def test_one_iteration_is_assign_regroup_and_one_trainer_iteration():
    fx = planted_case("short")  # some examples stay unassigned: they are left out of the regrouping
    M = int(fx["mdl_start"][-1])
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0)
    got = dev_models(eng, fx, 1)
    assign, best, _ = dev_assign(eng, fx)
    same(got["assign"], assign, "the stage's assignment")
    keep = np.nonzero(assign != NONE)[0]
    order = keep[np.argsort(assign[keep], kind="stable")]
    ex_start = np.concatenate(([0], np.cumsum(np.bincount(assign[keep], minlength=M)))).astype(np.uint32)
    assert len(order) < 36
    cen, st = eng.train_models(fx["mfcc"][order], fx["frames"][order], ex_start, fx["cen"], fx["cen_frames"], 1)
    assert cen.tobytes() == got["cen"].tobytes()
    assert np.array_equal(st[0]["n_ok"], got["stats"][0]["n_ok"]) and np.array_equal(st[0]["acc"], got["stats"][0]["acc"]) and np.all(st["n_fail"] == 0)
    eng.close()


@pytest.mark.gpu
def test_launch_groups_repeats_optional_outputs_and_the_host_form():
    fx = planted_case("copy")
    want = fx["want"]
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0, testing=True)
    first = dev_models(eng, fx, N_ITER, CANARIES[0])
    same(first["cen"], want["cen"], "centroids")
    blob = lambda r: b"".join(r[k].tobytes() for k in ("cen", "assign", "stats", "iter"))  # noqa: E731
    assert blob(dev_models(eng, fx, N_ITER, CANARIES[1])) == blob(first)  # two runs: identical bytes
    for pairs in (1, 7):  # 108 pairs: a launch per pair; launches of one workgroup of four and one of three
        with pairs_per_launch(pairs):
            assert blob(dev_models(eng, fx, N_ITER, CANARIES[pairs % 2])) == blob(first), pairs
    for want_out in ((), ("assign",), ("stats",), ("iter",), ("assign", "iter")):  # leaving outputs out changes nothing else
        got = dev_models(eng, fx, N_ITER, 0xA5, want=want_out)
        assert got["cen"].tobytes() == first["cen"].tobytes(), want_out
        for k in want_out:
            assert got[k].tobytes() == first[k].tobytes(), (want_out, k)
    h_cen, h_as, h_st, h_it = eng.cluster_models(fx["mfcc"], fx["frames"], fx["word_start"], fx["mdl_start"], fx["cen"], fx["cen_frames"], N_ITER)
    assert h_cen.tobytes() + h_as.tobytes() + h_st.tobytes() + h_it.tobytes() == blob(first)
    for n_iter in (1, 2):  # an odd and an even count: where the last set lands
        got = dev_models(eng, fx, n_iter, 0x3C)
        same_models(got, want, n_iter, f"n_iter {n_iter}")
        assert got["cen"].tobytes() == ref.cluster(fx["mfcc"], fx["frames"], fx["word_start"], fx["mdl_start"], fx["cen"], fx["cen_frames"], n_iter)["cen"].tobytes()
    eng.close()


# ---- GPU 4: contracts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frames_stride_and_poisoned_rows():
    fx = planted_case("short")
    want = fx["want"]
    E = 36
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0)
    im = poison_feature_rows(fx["mfcc"].copy(), fx["frames"])
    pc = poison_feature_rows(fx["cen"].copy(), fx["cen_frames"])
    recs = np.full((E, 2), 0x7F7F7F7F, np.uint32)
    recs[:, 1] = fx["frames"]
    d = dev(recs)
    got = dev_models(eng, fx, N_ITER, 0xA5, frames_stride=2, d_frames=d[:, 1], mfcc=im, cen=pc)
    same_models(got, want, N_ITER, "stride 2, poisoned")
    same(got["cen"], want["cen"], "stride 2, poisoned: centroids")
    assign, best, scores = dev_assign(eng, fx, 0x3C, frames_stride=2, d_frames=d[:, 1], mfcc=im, cen=pc)
    same(scores, want["dis"][0], "stage, stride 2, poisoned: scores")
    same(assign, want["assigns"][0], "stage, stride 2, poisoned: assign")
    # the host forms read their counts at the stride too
    h_as = np.zeros(E, np.uint32)
    assert eng.L.sr_cluster_assign(eng.h, engine._vp(im), P(recs.ctypes.data + 4), U32(2), engine._vp(fx["word_start"]), engine._vp(fx["mdl_start"]),
                                   U32(3), engine._vp(pc), engine._vp(fx["cen_frames"]), U32(ref.PLANT_ROWS), engine._vp(h_as), None, None) == 0
    assert h_as.tobytes() == want["assigns"][0].tobytes()
    h_cen = np.zeros_like(fx["cen"])
    assert eng.L.sr_cluster_models_dp(eng.h, engine._vp(im), P(recs.ctypes.data + 4), U32(2), engine._vp(fx["word_start"]), engine._vp(fx["mdl_start"]),
                                      U32(3), engine._vp(pc), engine._vp(fx["cen_frames"]), U32(ref.PLANT_ROWS), U32(N_ITER), engine._vp(h_cen),
                                      None, None, None) == 0
    assert h_cen.tobytes() == want["cen"].tobytes()
    eng.close()


# ---- GPU 5: refusals that write nothing ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing():
    fx = planted_case("quantile")
    E, M, W = 36, 6, 3
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0)
    d_im, d_fr, d_cen, d_cf = dev(fx["mfcc"]), dev(fx["frames"]), dev(fx["cen"]), dev(fx["cen_frames"])
    sid = torch.cuda.current_stream().cuda_stream
    WS, MS = tuple(fx["word_start"].tolist()), tuple(fx["mdl_start"].tolist())

    def refused(e=eng, code=BAD_ARG, ws=WS, ms=MS, words=W, n_iter=2, cen_rows=ref.PLANT_ROWS, stride=1, null=None, alias=None, only=None):
        for call in ("models", "assign"):
            if only and call != only:
                continue
            for where in ("cuda:0", None):
                g = dict(out=guarded_out(fx["cen"].shape, np.int16, 0xA5, 4096, where, "cen_out"),
                         assign=guarded_out((E,), np.uint32, 0xA5, 4096, where, "assign"),
                         stats=guarded_out((16, M), ref.TRAIN_STAT_DTYPE, 0xA5, 4096, where, "stats"),
                         iter=guarded_out((16,), ref.ITER_DTYPE, 0xA5, 4096, where, "iter"),
                         best=guarded_out((E,), np.uint32, 0xA5, 4096, where, "best"),
                         scores=guarded_out((E, 16), np.uint32, 0xA5, 4096, where, "scores"))
                w_s, m_s = np.array(ws, np.uint32), np.array(ms, np.uint32)
                if where:
                    a = dict(mfcc=P(d_im.data_ptr()), frames=P(d_fr.data_ptr()), cen=P(d_cen.data_ptr()), cf=P(d_cf.data_ptr()))
                else:
                    a = dict(mfcc=engine._vp(fx["mfcc"]), frames=engine._vp(fx["frames"]), cen=engine._vp(fx["cen"]), cf=engine._vp(fx["cen_frames"]))
                a.update(ws=engine._vp(w_s), ms=engine._vp(m_s), **{k: P(b.ptr) for k, b in g.items()})
                if null:
                    a[null] = None
                if alias == "in":
                    a["cen"] = P(g["out"].ptr + 24)    # the input overlaps the output
                if alias == "stats":
                    a["stats"] = P(g["out"].ptr + 8)
                if alias == "iter":
                    a["iter"] = P(g["assign"].ptr + 4)
                if alias == "best":
                    a["best"] = P(g["assign"].ptr + 4)
                if alias == "scores":
                    a["scores"] = P(g["best"].ptr + 8)
                head = (e.h, a["mfcc"], a["frames"], U32(stride), a["ws"], a["ms"], U32(words), a["cen"], a["cf"], U32(cen_rows))
                if call == "models":
                    args = head + (U32(n_iter), a["out"], a["assign"], a["stats"], a["iter"])
                    rc = e.L.sr_cluster_models_dp_dev(*args, P(sid)) if where else e.L.sr_cluster_models_dp(*args)
                else:
                    args = head + (a["assign"], a["best"], a["scores"])
                    rc = e.L.sr_cluster_assign_dev(*args, P(sid)) if where else e.L.sr_cluster_assign(*args)
                assert rc == code, (call, where, ws, ms, words, n_iter, cen_rows, stride, null, alias, rc)
                if where:
                    torch.cuda.synchronize()
                for b in g.values():
                    b.check_untouched()

    refused(words=0)
    refused(ws=(1, 12, 24, 36))                      # word_start / mdl_start must ascend from 0
    refused(ws=(0, 12, 11, 36))
    refused(ms=(1, 2, 4, 6))
    refused(ms=(0, 2, 1, 6))
    refused(ms=(0, 2, 2, 6))                         # a word without models
    refused(ms=(0, 2, 19, 21))                       # a word with 17
    assert b"SR_CLUSTER_MAX" in eng.L.sr_last_error()
    # the accumulator bound counts the examples of a WORD: 819 examples of 80 frames pass, 820 do not -- however many models share them
    assert 819 * ref.PLANT_MAXF <= 65535 < 820 * ref.PLANT_MAXF
    refused(ws=(0, 12, 832, 844))
    assert b"exact" in eng.L.sr_last_error()
    refused(alias="in", only="models")
    refused(alias="stats", only="models")
    refused(alias="iter", only="models")
    refused(alias="best", only="assign")
    refused(alias="scores", only="assign")
    for n_iter in (0, 17):
        refused(n_iter=n_iter, only="models")
    for cen_rows in (0, 1025):
        refused(cen_rows=cen_rows)
    refused(stride=0)
    for null in ("mfcc", "frames", "ws", "ms", "cen", "cf"):
        refused(null=null)
    refused(null="out", only="models")
    refused(null="assign", only="assign")
    got = dev_models(eng, fx, 1)  # and after all the refusals the engine still clusters
    same(got["assign"], fx["want"]["assigns"][0], "after the refusals")
    eng.close()
    e3 = Engine(max_frames=ref.PLANT_MAXF, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    refused(e=e3, code=BAD_CONFIG)
    e3.close()


# ---- GPU 6: end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cluster_words_then_classify_fresh_examples_of_both_variants():
    pl = ref.planted(6)
    labels = np.repeat(np.array([11, 5, 8], np.uint32), 12)  # the caller's word ids, not in ascending order
    rng = np.random.default_rng(60)
    shuffle = rng.permutation(36)                          # and the corpus in no particular order
    mfcc, frames, labels = pl["mfcc"][shuffle], pl["frames"][shuffle], labels[shuffle]
    eng = Engine(max_frames=ref.PLANT_MAXF, device=0)
    cen, cf, word_ids, valid, assign = eng.cluster_words(mfcc, frames, labels, n_clusters=2, n_iter=3)
    w_cen, w_cf, w_ids, w_valid, w_assign = ref.cluster_words(mfcc, frames, labels, ref.PLANT_MAXF, n_clusters=2, n_iter=3)
    assert np.array_equal(cf, w_cf) and word_ids.tolist() == w_ids.tolist() == [5, 5, 8, 8, 11, 11] and cen.shape == w_cen.shape
    assert np.array_equal(cen, w_cen) and np.array_equal(valid, w_valid) and np.array_equal(assign, w_assign)
    assert valid.tolist() == [1] * 6 and np.array_equal(word_ids[assign], labels)  # every example sits in a model of its own word
    for lab in (11, 8):  # the short and the long takes of a word got a model each
        a, n = assign[labels == lab], frames[labels == lab]
        by_len = a[np.argsort(n, kind="stable")]
        assert len(set(by_len[:6].tolist())) == 1 and len(set(by_len[6:].tolist())) == 1 and by_len[0] != by_len[-1], (lab, by_len.tolist())
    eng.set_templates_dense(cen, cf, valid)
    eng.set_word_map(word_ids)
    # fresh examples of both variants of each word: the same prototypes, new warps and new noise
    fresh, truth = [], []
    for k, proto in enumerate(pl["protos"]):
        L = len(proto)
        for _ in range(2):
            n = int(rng.integers(L - L // 8, L + L // 8 + 1))
            src = np.sort(rng.integers(0, L, n))
            row = np.zeros((ref.PLANT_MAXF, 12), np.int16)
            row[:n] = np.clip(proto[src] + rng.integers(-300, 301, (n, 12)), -32768, 32767)
            fresh.append((row, n)), truth.append((11, 5, 8)[k // 2])
    im, inf = np.array([f[0] for f in fresh]), np.array([f[1] for f in fresh], np.uint32)
    sc, res = eng.dtw(im, inf)
    orc = Oracle(max_frames=ref.PLANT_MAXF)
    want_sc = np.array([[orc.dtw(im[b], int(inf[b]), cen[k], int(cf[k])) for k in range(6)] for b in range(len(fresh))], np.uint32)
    assert np.array_equal(sc, want_sc)
    want_word = word_ids[want_sc.argmin(1)]  # (argmin: the first minimum, the recogniser's rule)
    assert np.array_equal(word_ids[res["best_tpl"]], want_word) and np.all(want_sc.min(1) != DIS_ERR)
    assert want_word.tolist() == truth  # the reference itself recognises every fresh take
    eng.close()
