"""Contracts of the host forms of the batch stages (include/sr_engine.h): the decoders, the spotter, alignment, training,
clustering, span scoring and rescoring as they are called with HOST buffers.

The value tests of each feature hold the host form to its device form and to the CPU restatement.  This file holds what those
leave open and what the host layer of the stages (csrc/sr_stage_host.h) carries for all of them:

  refusals        which code and which sr_last_error text a bad argument gets, and that a refused call writes nothing.  The
                  expected texts are literals here, never read from the library under test;
  a refused row   mid = 65536 in row 1 of a whole-path PCM form is found after the device has been entered: the code and the text
                  are the same, frm_num[0] and status[0] are already written, every other output byte still holds the canary;
  empty calls     n_rows = 0 / B = 0 returns 0 and writes nothing;
  strided counts  every *_dp host form reads its frame counts at frames_stride: with a stride of 3 and 0xFFFFFFFF in the gaps
                  it returns the bytes it returns for dense counts.  (The existing frames_stride tests -- test_chain, test_onepass,
                  test_onepass_gram, test_spot, test_span, test_align, test_cluster, test_rescore_dp -- all call the DEVICE
                  forms; no host form is covered by them, so none is left out here.)

Shapes: max_frames 24, a store of three templates of 5, 7 and 9 frames, two rows (two and three templates one after the other).
Everything goes through ctypes, outputs are interiors of canary-filled allocations (tests/guarded.py).

What is not a refusal: the whole-path PCM forms have no overlap rule for rec / words (they decode into device copies of their
own), and no frames_stride; those two cases exist for the *_dp forms only, buf_len > pcm_stride for the PCM forms only.
"""
import ctypes as C

import numpy as np
import pytest

from guarded import CANARIES, guarded_out
from stm32_speech_recognition_amd.engine import (ALIGN_DTYPE, CHAIN_REC_DTYPE, CHAIN_WORD_DTYPE, CLUSTER_ITER_DTYPE, CLUSTER_MAX, DIS_ERR,
                                                 FEAT_MAG, NBEST_DTYPE, SPAN_ACC, SPOT_DTYPE, TRAIN_STAT_DTYPE, Engine, grammar_any)

pytestmark = pytest.mark.gpu

R, NC, K, N = 24, 12, 3, 2           # max_frames, coefficients, templates, rows
TF = np.array([5, 7, 9], np.uint32)  # the templates' frames
BUF, PSTRIDE = 1200, 1203            # samples of a capture row, samples between rows
BAD_ARG, NO_TEMPLATES = 3, 4         # SR_ERR_BAD_ARG, SR_ERR_NO_TEMPLATES (include/sr_engine.h)
NONE = 0xFFFFFFFF
P, U32, U64, I32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
DECODERS = ("words", "grammar", "onepass", "onepass_grammar")
LEVEL = ("words", "grammar")         # the level decoders: max_words, n_words_exact and level costs
FN = {("words", "dp"): "sr_decode_words_dp", ("words", "batch"): "sr_decode_words_batch",
      ("grammar", "dp"): "sr_decode_grammar_dp", ("grammar", "batch"): "sr_decode_grammar_batch",
      ("onepass", "dp"): "sr_decode_onepass_dp", ("onepass", "batch"): "sr_decode_onepass_batch",
      ("onepass_grammar", "dp"): "sr_decode_onepass_grammar_dp", ("onepass_grammar", "batch"): "sr_decode_onepass_grammar_batch"}


class Ctx:
    def __init__(self):
        rng = np.random.default_rng(5)
        self.eng = Engine(max_frames=R, device=0)
        self.empty = Engine(max_frames=R, device=0)  # no templates set
        self.tm = np.zeros((K, R + 1, NC), np.int16)
        for k in range(K):
            self.tm[k, :TF[k]] = rng.integers(-900, 900, (TF[k], NC))
        self.eng.set_templates_dense(self.tm, TF)
        self.stale = self.eng.grammar(*grammar_any(range(K)))  # compiled before the store is set again
        self.eng.set_templates_dense(self.tm, TF)
        self.gram = self.eng.grammar(*grammar_any(range(K)))
        # feature rows: templates 0 1 and 2 0 1 one after the other, a little noise on top; rows >= frames stay zero
        self.im = np.zeros((N, R, NC), np.int16)
        self.frames = np.array([12, 21], np.uint32)
        for r, seq in enumerate(((0, 1), (2, 0, 1))):
            at = 0
            for k in seq:
                self.im[r, at:at + TF[k]] = self.tm[k, :TF[k]] + rng.integers(-20, 20, (TF[k], NC))
                at += TF[k]
            assert at == self.frames[r]
        # capture rows for the whole-path forms: 10 and 12 frames of 160 samples at a hop of 80
        self.pcm = np.clip(np.round(2048 + rng.normal(0, 300, N * PSTRIDE + 8)), 0, 4095).astype(np.uint16)
        self.start = np.array([1, 81], np.int32)
        self.end = np.array([1 + 160 + 80 * 9, 81 + 160 + 80 * 11], np.int32)
        self.mid = np.array([2048, 2048], np.uint32)
        self.pcm_frames = np.array([10, 12], np.uint32)
        assert self.end.max() <= BUF
        # inputs of the other stages
        self.ref = np.ascontiguousarray(self.tm[:, :10])  # [K][10][12]: references / centroids with ref_rows = 10
        self.nbest = self.eng.nbest(self.eng.dtw_dp(self.im, self.frames), 2)[0]
        self.dwords = self.eng.decode_words(self.im, self.frames, 3)[1]
        self.transcript = np.array([[0, 1, 0], [2, 0, 1]], np.uint32)
        self.t_words = np.array([2, 3], np.uint32)
        self.awords = self.eng.align_transcripts(self.im, self.frames, [[0, 1], [2, 0, 1]])[1]
        assert self.awords.shape == (N, 3)

    def close(self):
        for g in (self.stale, self.gram):
            g.close()
        self.eng.close()
        self.empty.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def H(name, shape, dtype, canary):
    return guarded_out(shape, dtype, canary, 64, None, name)


def ptr(a):
    return P(a.ctypes.data)


def run(eng, fn, *args):
    rc = getattr(eng.L, fn)(eng.h, *args)
    return rc, eng.L.sr_last_error().decode() if rc else ""


def strided(frames, stride):
    """the counts at `stride` words, 0xFFFFFFFF between them"""
    out = np.full(max(len(frames), 1) * stride, NONE, np.uint32)
    out[:len(frames) * stride:stride] = frames
    return out


def untouched(outs):
    for g in outs.values():
        g.check_untouched()


def image(outs):
    """guards intact; every output's interior as bytes"""
    for g in outs.values():
        g.check()
    return {k: g.interior().tobytes() for k, g in outs.items()}


# ---- the four decoders, *_dp and *_batch ---------------------------------------------------------------------------------------
def decode(c, kind, form, canary, n=N, cap=3, skip=DIS_ERR, wc=0, fstride=1, overlap=False, pstride=PSTRIDE, mid=None, empty=False,
           stale=False):
    """one call of a decoder's host form; cap = max_words (level decoders) or words_cap.  An empty call (n = 0) still gets real
    buffers of one row.  Returns (rc, message, {name: GuardedOut})"""
    eng = c.empty if empty else c.eng
    rows, level = max(n, 1), kind in LEVEL
    o = {"rec": H("rec", (rows,), CHAIN_REC_DTYPE, canary), "words": H("words", (rows, max(cap, 1)), CHAIN_WORD_DTYPE, canary)}
    if level:
        o["level_cost"] = H("level_cost", (rows, max(cap, 1)), np.uint32, canary)
    w_ptr = o["rec"].ptr + 16 if overlap else o["words"].ptr  # overlap: the word rows begin inside the records
    args = [(c.stale if stale else c.gram).g] if "grammar" in kind else []
    tail = [U32(skip), U32(wc), P(o["rec"].ptr), P(w_ptr)] + ([P(o["level_cost"].ptr)] if level else [])
    if form == "dp":
        fr = strided(c.frames[:n], max(fstride, 1))
        args += [ptr(c.im), ptr(fr), U32(fstride), U32(n)] + ([U32(cap), U32(0)] if level else [U32(0), U32(cap)]) + tail
    else:
        o["mfcc"], o["frm_num"], o["status"] = H("mfcc", (rows, R, NC), np.int16, canary), H("frm_num", (rows,), np.uint32, canary), \
            H("status", (rows,), np.uint32, canary)
        mid = c.mid if mid is None else mid
        args += [ptr(c.pcm), U64(pstride), U32(BUF), U32(n), ptr(c.start), ptr(c.end), ptr(mid)] + ([U32(cap), U32(0)] if level else [U32(cap)]) \
            + tail + [P(o["mfcc"].ptr), P(o["frm_num"].ptr), P(o["status"].ptr)]
    rc, msg = run(eng, FN[kind, form], *args)
    return rc, msg, o


def refusals():
    t = []
    for kind in DECODERS:
        for form in ("dp", "batch"):
            if kind in LEVEL:
                t += [(kind, form, dict(cap=0), BAD_ARG, "max_words must be 1..16"), (kind, form, dict(cap=17), BAD_ARG, "max_words must be 1..16")]
            else:
                t += [(kind, form, dict(cap=0), BAD_ARG, "words_cap must be at least 1")]
            t += [(kind, form, dict(skip=65536), BAD_ARG, "skip_cost must be at most 65535, or SR_DIS_ERR for no skipping"),
                  (kind, form, dict(wc=(1 << 24) + 1), BAD_ARG, "word_cost must be at most 2^24"),
                  (kind, form, dict(empty=True), NO_TEMPLATES, "no templates set")]
            if form == "dp":
                t += [(kind, form, dict(fstride=0), BAD_ARG, "frames_stride must be at least 1"),
                      (kind, form, dict(overlap=True), BAD_ARG,
                       "d_rec, d_words and d_level_cost overlap" if kind in LEVEL else "d_rec and d_words overlap")]
            else:
                t += [(kind, form, dict(pstride=BUF - 1), BAD_ARG, "buf_len exceeds pcm_stride")]
            if "grammar" in kind:
                t += [(kind, form, dict(stale=True), BAD_ARG, "the template store changed since the grammar was compiled")]
    return t


@pytest.mark.parametrize("kind,form,bad,code,text", refusals(), ids=lambda v: "_".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_decoder_refusals(ctx, kind, form, bad, code, text):
    for canary in CANARIES:
        rc, msg, outs = decode(ctx, kind, form, canary, **bad)
        assert rc == code and text in msg, (rc, msg)
        untouched(outs)


# ---- the spotter ------------------------------------------------------------------------------------------------------------------
def spot(c, form, canary, n=N, fstride=1, pstride=PSTRIDE, mid=None):
    rows = max(n, 1)
    o = {"hits": H("hits", (rows, 1, K), SPOT_DTYPE, canary), "scores": H("scores", (rows, 1, K), np.uint32, canary)}
    if form == "dp":
        fr = strided(c.frames[:n], max(fstride, 1))
        rc, msg = run(c.eng, "sr_spot_dp_batch", ptr(c.im), ptr(fr), U32(fstride), U32(n), U32(0), P(o["hits"].ptr), P(o["scores"].ptr))
    else:
        o["mfcc"], o["frm_num"], o["status"] = H("mfcc", (rows, R, NC), np.int16, canary), H("frm_num", (rows,), np.uint32, canary), \
            H("status", (rows,), np.uint32, canary)
        rc, msg = run(c.eng, "sr_spot_batch", ptr(c.pcm), U64(pstride), U32(BUF), U32(n), ptr(c.start), ptr(c.end), ptr(c.mid if mid is None else mid),
                      U32(0), P(o["hits"].ptr), P(o["scores"].ptr), P(o["mfcc"].ptr), P(o["frm_num"].ptr), P(o["status"].ptr))
    return rc, msg, o


@pytest.mark.parametrize("form,bad,text", [("dp", dict(fstride=0), "frames_stride must be at least 1"),
                                           ("batch", dict(pstride=BUF - 1), "buf_len exceeds pcm_stride")], ids=["dp", "batch"])
def test_spotter_refusals(ctx, form, bad, text):
    for canary in CANARIES:
        rc, msg, outs = spot(ctx, form, canary, **bad)
        assert rc == BAD_ARG and text in msg, (rc, msg)
        untouched(outs)


# ---- a record refused after the device has been entered ------------------------------------------------------------------------
def features(c, canary, n=N, mid=None):
    w = c.eng.frame_feature_width(FEAT_MAG)
    rows = max(n, 1)
    o = {"feat": H("feat", (rows, R, w), np.uint32, canary), "mfcc": H("mfcc", (rows, R, NC), np.int16, canary),
         "frm_num": H("frm_num", (rows,), np.uint32, canary), "status": H("status", (rows,), np.uint32, canary)}
    rc, msg = run(c.eng, "sr_frame_features_batch", I32(FEAT_MAG), ptr(c.pcm), U64(PSTRIDE), U32(BUF), U32(n), ptr(c.start), ptr(c.end),
                  ptr(c.mid if mid is None else mid), P(o["feat"].ptr), P(o["mfcc"].ptr), P(o["frm_num"].ptr), P(o["status"].ptr))
    return rc, msg, o


PCM_FORMS = [("decode", k) for k in DECODERS] + [("spot", None), ("features", None)]


def pcm_call(c, what, kind, canary, **kw):
    if what == "decode":
        return decode(c, kind, "batch", canary, **kw)
    return spot(c, "batch", canary, **kw) if what == "spot" else features(c, canary, **kw)


@pytest.mark.parametrize("what,kind", PCM_FORMS, ids=[k or w for w, k in PCM_FORMS])
def test_pcm_forms_refuse_a_mid_beyond_u16_in_row_1(ctx, what, kind):
    """the records are made row by row after the device has been entered: row 0's count and status are written, nothing else"""
    bad_mid = np.array([2048, 65536], np.uint32)
    for canary in CANARIES:
        rc, msg, outs = pcm_call(ctx, what, kind, canary, mid=bad_mid)
        assert rc == BAD_ARG and "mid exceeds the u16 sample range" in msg, (rc, msg)
        fill = np.frombuffer(bytes([canary] * 4), np.uint32)[0]
        outs.pop("frm_num").check_equals(np.array([ctx.pcm_frames[0], fill], np.uint32))
        outs.pop("status").check_equals(np.array([0, fill], np.uint32))
        untouched(outs)


# ---- the other stages' host forms: one call each, counts at a stride -------------------------------------------------------------
def rescore(c, canary, n, fr, fs):
    o = {"out": H("nbest_out", (max(n, 1), 2), NBEST_DTYPE, canary), "n_rescored": H("n_rescored", (max(n, 1),), np.uint32, canary)}
    return run(c.eng, "sr_rescore_nbest_dp", ptr(c.im), ptr(fr), U32(fs), U32(n), U32(2), ptr(c.nbest), P(o["out"].ptr), P(o["n_rescored"].ptr)), o


def align(c, canary, n, fr, fs):
    o = {"rec": H("rec", (max(n, 1),), ALIGN_DTYPE, canary), "span": H("span", (max(n, 1), R), np.uint32, canary)}
    ref_of_row = np.array([1, 2], np.uint32)
    return run(c.eng, "sr_dtw_dp_align", ptr(c.im), ptr(fr), U32(fs), U32(n), ptr(c.ref), ptr(TF), U32(10), U32(K), ptr(ref_of_row),
               P(o["rec"].ptr), P(o["span"].ptr)), o


def train(c, canary, n, fr, fs):
    """one model (template 1 as its first centroid) from the n rows, two iterations"""
    o = {"cen_out": H("cen_out", (1, 10, NC), np.int16, canary), "stats": H("stats", (2, 1), TRAIN_STAT_DTYPE, canary)}
    ex_start, cen_frames = np.array([0, n], np.uint32), TF[1:2].copy()
    return run(c.eng, "sr_train_models_dp", ptr(c.im), ptr(fr), U32(fs), ptr(ex_start), U32(1), ptr(c.ref[1:2]), ptr(cen_frames), U32(10), U32(2),
               P(o["cen_out"].ptr), P(o["stats"].ptr)), o


def spans(c, canary, n, fr, fs):
    o = {"scores": H("scores", (max(n, 1), 3, K), np.uint32, canary)}
    return run(c.eng, "sr_score_word_spans", ptr(c.im), ptr(fr), U32(fs), U32(n), U32(3), ptr(c.dwords), U32(SPAN_ACC), P(o["scores"].ptr)), o


def alts(c, canary, n, fr, fs):
    m = max(n, 1)
    o = {"rec": H("rec", (m,), CHAIN_REC_DTYPE, canary), "words": H("words", (m, 3), CHAIN_WORD_DTYPE, canary),
         "level_cost": H("level_cost", (m, 3), np.uint32, canary), "alts": H("alts", (m, 3, 2), NBEST_DTYPE, canary),
         "n_matched": H("n_matched", (m, 3), np.uint32, canary), "span_scores": H("span_scores", (m, 3, K), np.uint32, canary)}
    return run(c.eng, "sr_decode_words_alts", ptr(c.im), ptr(fr), U32(fs), U32(n), U32(3), U32(0), U32(DIS_ERR), U32(0), P(o["rec"].ptr),
               P(o["words"].ptr), P(o["level_cost"].ptr), U32(2), U32(SPAN_ACC), P(o["alts"].ptr), P(o["n_matched"].ptr),
               P(o["span_scores"].ptr)), o


def forced(c, canary, n, fr, fs):
    o = {"rec": H("rec", (max(n, 1),), CHAIN_REC_DTYPE, canary), "words": H("words", (max(n, 1), 3), CHAIN_WORD_DTYPE, canary)}
    return run(c.eng, "sr_align_transcripts_dp", ptr(c.im), ptr(fr), U32(fs), U32(n), ptr(c.transcript), ptr(c.t_words), U32(3), U32(DIS_ERR),
               U32(0), P(o["rec"].ptr), P(o["words"].ptr)), o


def gather(c, canary, n, fr, fs):
    """the five aligned words of the two rows as examples 0..4; an empty call: no example wanted"""
    n_ex = 5 if n else 0
    dst = np.array([0, 1, NONE, 2, 3, 4] if n else [NONE] * 6, np.uint32)
    o = {"ex": H("ex", (max(n_ex, 1), 10, NC), np.int16, canary), "ex_frames": H("ex_frames", (max(n_ex, 1),), np.uint32, canary)}
    return run(c.eng, "sr_gather_word_spans", ptr(c.im), ptr(fr), U32(fs), U32(N), ptr(c.awords), U32(3), ptr(dst), U32(n_ex), U32(10),
               P(o["ex"].ptr), P(o["ex_frames"].ptr)), o


def cluster_assign(c, canary, n, fr, fs):
    """one word, its n examples, two models (templates 0 and 1)"""
    o = {"assign": H("assign", (max(n, 1),), np.uint32, canary), "best": H("best", (max(n, 1),), np.uint32, canary),
         "scores": H("scores", (max(n, 1), CLUSTER_MAX), np.uint32, canary)}
    word_start, mdl_start = np.array([0, n], np.uint32), np.array([0, 2], np.uint32)
    return run(c.eng, "sr_cluster_assign", ptr(c.im), ptr(fr), U32(fs), ptr(word_start), ptr(mdl_start), U32(1), ptr(c.ref), ptr(TF), U32(10),
               P(o["assign"].ptr), P(o["best"].ptr), P(o["scores"].ptr)), o


def cluster_models(c, canary, n, fr, fs):
    o = {"cen_out": H("cen_out", (2, 10, NC), np.int16, canary), "assign": H("assign", (max(n, 1),), np.uint32, canary),
         "stats": H("stats", (2, 2), TRAIN_STAT_DTYPE, canary), "iter": H("iter", (2,), CLUSTER_ITER_DTYPE, canary)}
    word_start, mdl_start = np.array([0, n], np.uint32), np.array([0, 2], np.uint32)
    return run(c.eng, "sr_cluster_models_dp", ptr(c.im), ptr(fr), U32(fs), ptr(word_start), ptr(mdl_start), U32(1), ptr(c.ref), ptr(TF), U32(10),
               U32(2), P(o["cen_out"].ptr), P(o["assign"].ptr), P(o["stats"].ptr), P(o["iter"].ptr)), o


STAGES = {"rescore": rescore, "align": align, "train": train, "spans": spans, "alts": alts, "forced": forced, "gather": gather,
          "cluster_assign": cluster_assign, "cluster_models": cluster_models}
# no rows, but work all the same: a training over no examples still runs its iterations and writes every centroid and record
RUNS_EMPTY = ("train", "cluster_models")


def stage_call(c, name, canary, n, fstride):
    """-> (rc, message, outputs) of a decoder's *_dp form, the spotter's, or one of STAGES"""
    if name in DECODERS:
        return decode(c, name, "dp", canary, n=n, fstride=fstride)
    if name == "spot":
        return spot(c, "dp", canary, n=n, fstride=fstride)
    (rc, msg), o = STAGES[name](c, canary, n, strided(c.frames[:n], fstride), fstride)
    return rc, msg, o


@pytest.mark.parametrize("name", DECODERS + ("spot",) + tuple(STAGES))
def test_strided_frame_counts_give_the_bytes_of_dense_ones(ctx, name):
    rc, msg, dense = stage_call(ctx, name, CANARIES[0], N, 1)
    assert rc == 0, msg
    rc, msg, wide = stage_call(ctx, name, CANARIES[0], N, 3)
    assert rc == 0, msg
    a, b = image(dense), image(wide)
    for k in a:
        assert a[k] == b[k], f"{name}: output {k} differs between frames_stride 1 and 3"
        assert a[k] != bytes([CANARIES[0]]) * len(a[k]), f"{name}: output {k} was never written"
    # never vacuous: the rows decode / align / score
    first = next(iter(dense.values())).interior()
    if name in DECODERS + ("alts", "forced"):
        assert (first["status"] == 0).all() and first["n_words"].tolist() == [2, 3], first
    elif name == "align":
        assert first["status"].tolist() == [0, 1], first  # 12 frames on a reference of 7: a path; 21 on 9: gated (AL_GATED)


# ---- empty calls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECODERS + ("spot",) + tuple(STAGES))
def test_a_call_without_rows_returns_ok_and_writes_nothing(ctx, name):
    got = []
    for canary in CANARIES:
        rc, msg, outs = stage_call(ctx, name, canary, 0, 1)
        assert rc == 0, msg
        if name in RUNS_EMPTY:
            outs.pop("assign", None)  # no example, no assignment
            outs["cen_out"].check_equals(ctx.ref[1:2] if name == "train" else ctx.ref[:2])  # nobody matched: every row kept
            got.append(image(outs))
        else:
            untouched(outs)
    if got:  # fully written: no byte follows the canary
        assert got[0] == got[1], name


@pytest.mark.parametrize("what,kind", PCM_FORMS, ids=[k or w for w, k in PCM_FORMS])
def test_a_pcm_call_without_rows_returns_ok_and_writes_nothing(ctx, what, kind):
    for canary in CANARIES:
        rc, msg, outs = pcm_call(ctx, what, kind, canary, n=0)
        assert rc == 0, msg
        untouched(outs)


def test_gather_without_feature_rows_still_fills_its_examples(ctx):
    """n_rows = 0 with examples wanted by no span: the host form stages no row, every example comes back empty"""
    for canary in CANARIES:
        dst = np.full(1, NONE, np.uint32)  # no span: never read
        ex, ef = H("ex", (2, 10, NC), np.int16, canary), H("ex_frames", (2,), np.uint32, canary)
        rc, msg = run(ctx.eng, "sr_gather_word_spans", ptr(ctx.im), ptr(ctx.frames), U32(1), U32(0), ptr(ctx.awords), U32(3), ptr(dst), U32(2),
                      U32(10), P(ex.ptr), P(ef.ptr))
        assert rc == 0, msg
        ex.check_equals(np.zeros((2, 10, NC), np.int16))
        ef.check_equals(np.zeros(2, np.uint32))
