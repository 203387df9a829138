"""Two-pass recognition: the N-best words of a first pass rescored with the full-DP scorer (include/sr_engine.h, "second pass").

The definition: every slot of every candidate word of a row gets the value sr_dtw_dp_batch_dev writes for that (row, slot),
and the output is what sr_nbest_batch returns for a score row holding those values at the candidate words' slots and
SR_DIS_ERR everywhere else.  Expected values therefore come from code that exists without the feature: the CPU oracle of the
full-DP scorer (oracle_lib.Oracle.dtw_dp_batch), a restatement of the N-best rule written here, and -- as a second, on-device
cross-check and where the oracle would be slow -- eng.dtw_dp over the full matrix -> mask -> eng.nbest.  Every comparison is
bit-exact.

The sparse scorer's workgroups cover ROW RANGES of 1 024 rows (band kernels, 4 / 8 / 16 lanes per pair) or 256 rows (the
generic one-wave-per-pair kernel); the shapes below cross both.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import oracle_lib as ol
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import DIS_ERR, NBEST_DTYPE, NO_WORD, RESULT_DTYPE, VAD_DTYPE, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
FUNCS = ("sr_rescore_nbest_dp_dev", "sr_rescore_nbest_dp", "sr_recognize_rescored_batch_dev", "sr_recognize_rescored_batch")
EMPTY = (NO_WORD, 0xFFFFFFFF, DIS_ERR, 0)
BAD_CONFIG, BAD_ARG, NO_TEMPLATES = 2, 3, 4
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
BAND_ROWS, WAVE_ROWS = 1024, 256  # rows one sparse workgroup covers (k_dtw_dp_band_sparse / k_dtw_dp_wave64_sparse)
LANES = (0, 4, 8, 16, 1)


# ---- the definition, restated ---------------------------------------------------------------------------------------------
def nbest_rule(row, words, n_best):
    """the N-best rule for one score row: per word the first minimum in slot order and the number of slots below dis_err,
    words ranked by (dis, slot), the tail empty -> (entries, number of candidates)"""
    best = {}
    for k, d in enumerate(int(v) for v in row):
        if d != DIS_ERR:
            e = best.setdefault(int(words[k]), [d, k, 0])
            e[2] += 1
            if d < e[0]:
                e[:2] = [d, k]
    ranked = sorted((d, k, w, c) for w, (d, k, c) in best.items())
    ent = [(w, k, d, c) for d, k, w, c in ranked[:n_best]]
    return ent + [EMPTY] * (n_best - len(ent)), len(ranked)


def rescored(dp, words, lists):
    """dp uint32 [n, K] full-DP scores, lists NBEST_DTYPE [n, n_best] -> (entries [n, n_best], n_rescored [n])"""
    words = np.asarray(words, np.uint32)
    n, K = dp.shape
    n_best = lists.shape[1]
    out, cnt = np.zeros((n, n_best), NBEST_DTYPE), np.zeros(n, np.uint32)
    for r in range(n):
        cand = {int(words[e["slot"]]) for e in lists[r] if e["word"] != NO_WORD and e["slot"] < K}  # the slot's group, not e.word
        row = np.where(np.isin(words, list(cand)), dp[r], DIS_ERR) if cand else np.full(K, DIS_ERR, np.uint32)
        ent, cnt[r] = nbest_rule(row, words, n_best)
        out[r] = np.array(ent, NBEST_DTYPE)
    return out, cnt


def masked_matrix(dp, words, lists):
    """the score rows of the definition: dp at the candidate words' slots, dis_err elsewhere"""
    words = np.asarray(words, np.uint32)
    out = np.full_like(dp, DIS_ERR)
    for r in range(len(dp)):
        ok = (lists[r]["word"] != NO_WORD) & (lists[r]["slot"] < dp.shape[1])
        m = np.isin(words, words[lists[r]["slot"][ok]])
        out[r, m] = dp[r, m]
    return out


def check(got, want, what):
    (g_nb, g_n), (w_nb, w_n) = got, want
    g_nb = np.asarray(g_nb).reshape(w_nb.shape)
    g32, w32 = g_nb.view(np.uint32).reshape(len(w_nb), -1), w_nb.view(np.uint32).reshape(len(w_nb), -1)
    bad = np.nonzero(np.any(g32 != w32, 1))[0]
    assert not len(bad), (what, "row", int(bad[0]), g_nb[bad[0]].tolist(), w_nb[bad[0]].tolist())
    assert np.array_equal(np.asarray(g_n).view(np.uint32).reshape(-1), w_n), what


# ---- the base fixture ---------------------------------------------------------------------------------------------------------
MAXF, K0, B0 = 96, 24, 70
WORDS0 = np.array([7, 7, 7, 7, 3, 9, 3, 9] + [11] * 7 + [2, 40, 41, 40, 41, 40, 41, 3, 9], np.uint32)


def stretched(rng, base, n, noise):
    idx = (np.arange(n) * base.shape[0]) // max(n, 1)
    return np.clip(base[idx] + rng.integers(-noise, noise + 1, (n, 12)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def base_fixture():
    """K = 24 templates in 7 uneven, interleaved word groups (one of 7 slots, one of a single 1-frame slot, an erased slot),
    B = 70 inputs with 0, 1, 96 and 2 frames in front; the oracle's full-DP matrix, computed once"""
    rng = np.random.default_rng(2026)
    assert len(WORDS0) == K0
    ids = list(dict.fromkeys(WORDS0.tolist()))
    pat = rng.integers(-2500, 2501, (6, MAXF, 12))
    tf = rng.integers(20, MAXF + 1, K0).astype(np.uint32)
    tf[15], tf[5] = 1, MAXF
    valid = np.ones(K0, np.uint8)
    valid[9] = 0
    tm = np.zeros((K0, MAXF + 1, 12), np.int16)
    for k in range(K0):
        tm[k, :tf[k]] = stretched(rng, pat[ids.index(int(WORDS0[k])) % 6], int(tf[k]), 900)
    inf = rng.integers(10, MAXF + 1, B0).astype(np.uint32)
    inf[:4] = [0, 1, MAXF, 2]
    im = np.zeros((B0, MAXF, 12), np.int16)
    for b in range(B0):
        im[b, :inf[b]] = stretched(rng, pat[rng.integers(0, 6)], int(inf[b]), 1200)
    dp = ol.Oracle(max_frames=MAXF).dtw_dp_batch(im, inf, tm, np.where(valid != 0, tf, 0))
    for a in (tm, tf, valid, im, inf, dp):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, valid=valid, im=im, inf=inf, dp=dp)


def base_engine(fx=None, words=WORDS0, **kw):
    fx = fx or base_fixture()
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"], fx["valid"])
    eng.set_word_map(words)
    return eng


def as_list(rows, n_best):
    """[[(word, slot), ...], ...] -> NBEST_DTYPE [n, n_best], missing entries empty"""
    out = np.array([[EMPTY] * n_best] * len(rows), NBEST_DTYPE).reshape(len(rows), n_best)
    for r, ents in enumerate(rows):
        for i, (w, s) in enumerate(ents):
            out[r, i] = (w, s, 123, 1)
    return out


def dev_call(eng, im, inf, lists, frames_stride=1, frames=None):
    d_im = torch.from_numpy(np.array(im)).cuda()
    d_inf = torch.from_numpy(np.array(inf).view(np.int32)).cuda() if frames is None else frames
    d_in = torch.from_numpy(np.array(lists).view(np.int32).reshape(len(lists), -1, 4)).cuda()
    keep = d_in.clone()
    nb, nr = eng.rescore_nbest_dev(d_im, d_inf, d_in, frames_stride)
    torch.cuda.synchronize()
    assert torch.equal(d_in, keep), "the input list was written"
    return engine.nbest_from_torch(nb), nr.cpu().numpy().view(np.uint32)


# ---- CPU: the surface (fails without the feature) ---------------------------------------------------------------------------
def test_header_declares_the_rescoring_api_and_libraries_export_it():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert src.index("sr_nbest_batch_dev") < src.index("sr_rescore_nbest_dp_dev") < src.index("sr_live_open")
    for meth in ("rescore_nbest", "rescore_nbest_dev"):
        assert callable(getattr(Engine, meth, None)), meth
    import inspect
    for meth in ("recognize_nbest", "recognize_nbest_dev"):
        assert inspect.signature(getattr(Engine, meth)).parameters["rescore"].default is False, meth


def test_restatement_on_small_rows():
    words = [5, 5, 6, 6, 7]
    ent, n = nbest_rule([9, 9, 3, DIS_ERR, DIS_ERR], words, 3)
    assert ent == [(6, 2, 3, 1), (5, 0, 9, 2), EMPTY] and n == 2
    dp = np.array([[9, 9, 3, 1, 0]], np.uint32)
    lists = as_list([[(1234, 1), (NO_WORD, 4), (6, 5), (6, 0xFFFFFFFF)]], 4)  # word field wrong, empty entry, slot = K, slot = -1
    nb, nr = rescored(dp, words, lists)
    assert nb[0].tolist() == [(5, 0, 9, 2), EMPTY, EMPTY, EMPTY] and nr[0] == 1
    assert np.array_equal(masked_matrix(dp, words, lists), [[9, 9, DIS_ERR, DIS_ERR, DIS_ERR]])


# ---- GPU 1: stage level, both forms, every lane setting -------------------------------------------------------------------------
@pytest.mark.gpu
def test_stage_level_forms_every_lane_setting():
    fx = base_fixture()
    eng = base_engine()
    im, inf, dp = fx["im"], fx["inf"], fx["dp"]
    sc, _ = eng.dtw(im, inf)
    assert np.array_equal(eng.dtw_dp(im, inf), dp)  # the dense scorer agrees with its oracle on this fixture
    for n_best in (1, 3, 16):
        first, _ = eng.nbest(sc, n_best)
        want = rescored(dp, WORDS0, first)
        empty = want[1] == 0
        changed = np.array([first[r]["word"].tolist() != want[0][r]["word"].tolist() for r in range(B0)])
        print(f"n_best {n_best}: {int(empty.sum())} rows without candidates, order changed in {int(changed.sum())} of {B0} rows, "
              f"top word in {int((first[:, 0]['word'] != want[0][:, 0]['word']).sum())}")
        assert empty.sum() >= 1 and empty[0]  # (row 0 has no frames)
        if n_best == 3:  # a kernel that copied the input list through must not pass
            assert changed[~empty].sum() * 4 >= (~empty).sum(), (int(changed.sum()), int((~empty).sum()))
        ref_bytes = None
        for lanes in LANES:
            eng.set_dp_lanes(lanes)
            got = dev_call(eng, im, inf, first)
            check(got, want, ("dev", n_best, lanes))
            host = eng.rescore_nbest(im, inf, first)
            check(host, want, ("host", n_best, lanes))
            b = got[0].tobytes() + got[1].tobytes()
            ref_bytes = ref_bytes or b
            assert b == ref_bytes and host[0].tobytes() + host[1].tobytes() == ref_bytes, lanes
        again = dev_call(eng, im, inf, first)  # (lanes = 1 still set) twice the same bytes
        assert again[0].tobytes() + again[1].tobytes() == ref_bytes
        eng.set_dp_lanes(0)
        # second cross-check, all on the device: dense matrix -> mask -> N-best
        nb2, nm2 = eng.nbest(masked_matrix(eng.dtw_dp(im, inf), WORDS0, first), n_best)
        check((nb2, nm2), want, ("dense + mask", n_best))
    eng.close()


# ---- GPU 2: hand-built lists --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hand_built_lists():
    fx = base_fixture()
    eng = base_engine()
    im, inf, dp = fx["im"], fx["inf"], fx["dp"]
    assert inf[3] == 2 and np.all(dp[3, :4] == DIS_ERR) and dp[3, 15] != DIS_ERR
    rows = [3, 10, 11, 12, 13, 14, 15, 16]
    lists = as_list([
        [(7, 0), (2, 15)],                               # 2 input frames: every slot of word 7 fails the length gate, 7 drops out
        [(3, 4), (NO_WORD, 8), (NO_WORD, 0), (40, 16)],  # empty entries in the middle (their slot fields mean nothing)
        [(11, 8), (11, 12), (9, 5), (11, 14)],           # the same word three times
        [(7, 1), (3, K0), (9, 0xFFFFFFFF), (41, 17)],    # slot = K and slot = 0xFFFFFFFF: ignored
        [(11, 9)],                                       # erased slot 9: its word 11 has valid slots
        [(7, 16), (40, 0), (5555, 22)],                  # word fields contradict the slots: groups 40, 7 and 3 are meant
        [],                                              # nothing but empty entries
        [(2, 15), (9, 23), (3, 22), (41, 21)],
    ], 4)
    want = rescored(dp[rows], WORDS0, lists)
    assert want[1].tolist()[0] == 1 and want[0][0, 0]["word"] == 2 and want[1][6] == 0
    assert want[1][2] == 2 and want[1][3] == 2 and want[0][4, 0]["word"] == 11
    assert want[0][4, 0]["count"] == (dp[14, 8:15] != DIS_ERR).sum() >= 1 and dp[14, 9] == DIS_ERR
    assert sorted(want[0][5]["word"][:3].tolist()) == [3, 7, 40]
    for lanes in LANES:
        eng.set_dp_lanes(lanes)
        check(dev_call(eng, im[rows], inf[rows], lists), want, ("dev", lanes))
        check(eng.rescore_nbest(im[rows], inf[rows], lists), want, ("host", lanes))
    eng.close()


# ---- GPU 3: ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_go_to_the_lower_slot_and_the_first_slot_of_a_word():
    fx = base_fixture()
    tm, tf = fx["tm"].copy(), fx["tf"].copy()
    tm[16], tf[16] = tm[4], tf[4]    # word 40's slot 16 = word 3's slot 4: two words tie
    tm[10], tf[10] = tm[8], tf[8]    # inside word 11: slots 8 and 10 tie
    tm[12], tf[12] = tm[8], tf[8]
    eng = base_engine(dict(tm=tm, tf=tf, valid=fx["valid"]))
    im, inf = fx["im"], fx["inf"]
    dp = ol.Oracle(max_frames=MAXF).dtw_dp_batch(im, inf, tm, np.where(fx["valid"] != 0, tf, 0))
    assert np.array_equal(dp[:, 16], dp[:, 4]) and np.array_equal(dp[:, 10], dp[:, 8])
    lists = as_list([[(40, 16), (3, 4), (11, 12)]] * B0, 3)
    want = rescored(dp, WORDS0, lists)
    nb = want[0]
    both = (dp[:, 4] != DIS_ERR) & (dp[:, 4] == dp[:, [4, 6, 22]].min(1)) & (dp[:, 4] == dp[:, [16, 18, 20]].min(1))
    assert both.sum() >= 3  # rows where the tied pair IS the best slot of both words
    for r in np.nonzero(both)[0]:
        w = nb[r]["word"].tolist()
        assert w.index(3) < w.index(40) and nb[r][w.index(3)]["slot"] == 4 and nb[r][w.index(40)]["slot"] == 16
        assert nb[r][w.index(3)]["dis"] == nb[r][w.index(40)]["dis"]
    in11 = [r for r in range(B0) if 11 in nb[r]["word"] and dp[r, 8] == dp[r, 8:15][dp[r, 8:15] != DIS_ERR].min()]
    assert len(in11) >= 3 and all(nb[r][nb[r]["word"].tolist().index(11)]["slot"] == 8 for r in in11)
    for lanes in LANES:
        eng.set_dp_lanes(lanes)
        check(dev_call(eng, im, inf, lists), want, lanes)
    eng.close()


# ---- GPU 4: row ranges and store sizes ----------------------------------------------------------------------------------------------
def random_case(seed, maxf, K, B, amp=2500):
    rng = np.random.default_rng(seed)
    tf = rng.integers(maxf // 3, maxf + 1, K).astype(np.uint32)
    tm = np.zeros((K, maxf + 1, 12), np.int16)
    tm[:, :maxf] = rng.integers(-amp, amp + 1, (K, maxf, 12))
    inf = rng.integers(maxf // 3, maxf + 1, B).astype(np.uint32)
    im = rng.integers(-amp, amp + 1, (B, maxf, 12)).astype(np.int16)
    return tm, tf, im, inf


@pytest.mark.gpu
@pytest.mark.parametrize("K,B", [(65, 1100), (1, 300), (64, 300)])
def test_row_range_and_store_size_edges(K, B):
    """1 100 rows cross the 1 024-row range of a band workgroup and four 256-row ranges of the generic kernel's; 300 rows cross
    the latter.  Checked against the dense matrix + mask + N-best on the device, and a 64-row sample against the oracle."""
    assert B > WAVE_ROWS and (K != 65 or B > BAND_ROWS)
    maxf = 40
    tm, tf, im, inf = random_case(K, maxf, K, B)
    inf[[0, B - 1]] = [0, maxf]
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    eng.set_word_map(None, 4)
    words = np.arange(K, dtype=np.uint32) // 4
    sc, _ = eng.dtw(im, inf)
    dense = eng.dtw_dp(im, inf)
    sample = np.r_[0:16, B // 2 - 16:B // 2 + 16, B - 16:B]
    dp_s = ol.Oracle(max_frames=maxf).dtw_dp_batch(im[sample], inf[sample], tm, tf)
    assert np.array_equal(dense[sample], dp_s)
    for n_best in (2, 16):
        first, _ = eng.nbest(sc, n_best)
        first[5::7, 0] = EMPTY  # not every row names its best word
        want = eng.nbest(masked_matrix(dense, words, first), n_best)
        assert (want[1] > 0).sum() > B // 2
        for lanes in LANES:
            eng.set_dp_lanes(lanes)
            got = dev_call(eng, im, inf, first)
            check(got, want, (K, n_best, lanes))
            check((got[0][sample], got[1][sample]), rescored(dp_s, words, first[sample]), (K, n_best, lanes, "oracle"))
        eng.set_dp_lanes(0)
    eng.close()


# ---- GPU 5: a store the band kernel cannot stage -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_store_with_coefficients_beyond_16383_takes_the_generic_kernel():
    maxf, K, B = 50, 10, 300
    tm, tf, im, inf = random_case(5, maxf, K, B, amp=3000)
    tm[2, 3, 5], tm[7, 0, 0], tm[7, 9, 11] = 20000, -30000, 25000
    words = np.array([1, 1, 2, 2, 2, 3, 1, 3, 9, 9], np.uint32)
    eng = Engine(max_frames=maxf, device=0)
    eng.set_templates_dense(tm, tf)
    eng.set_word_map(words)
    dp = ol.Oracle(max_frames=maxf).dtw_dp_batch(im, inf, tm, tf)
    assert np.array_equal(eng.dtw_dp(im, inf), dp)
    first, _ = eng.nbest(eng.dtw(im, inf)[0], 2)
    want = rescored(dp, words, first)
    assert (want[1] > 0).sum() > B // 2
    for lanes in LANES:
        eng.set_dp_lanes(lanes)
        check(dev_call(eng, im, inf, first), want, lanes)
    eng.close()


# ---- GPU 6: frames_stride -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frame_counts_inside_records():
    fx = base_fixture()
    eng = base_engine()
    im, inf, dp = fx["im"], fx["inf"], fx["dp"]
    first, _ = eng.nbest(eng.dtw(im, inf)[0], 3)
    want = rescored(dp, WORDS0, first)
    plain = dev_call(eng, im, inf, first)
    check(plain, want, "stride 1")
    vad = np.full((B0, 12), 0x7F7F7F7F, np.uint32)  # sr_vad_rec: frm_num is word 9 of 12
    vad[:, VAD_DTYPE.fields["frm_num"][1] // 4] = inf
    res = np.full((B0, 4), 0x7F7F7F7F, np.uint32)   # sr_result: frm_num is word 2 of 4
    res[:, RESULT_DTYPE.fields["frm_num"][1] // 4] = inf
    assert VAD_DTYPE.itemsize == 48 and VAD_DTYPE.fields["frm_num"][1] == 36 and RESULT_DTYPE.fields["frm_num"][1] == 8
    for rec, col, stride in ((vad, 9, 12), (res, 2, 4)):
        d = torch.from_numpy(rec.view(np.int32)).cuda()
        got = dev_call(eng, im, inf, first, stride, frames=d[:, col])
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), stride
        out, nr = np.zeros_like(first), np.zeros(B0, np.uint32)
        v = engine._vp
        assert eng.L.sr_rescore_nbest_dp(eng.h, v(im), P(rec.ctypes.data + 4 * col), U32(stride), U32(B0), U32(3), v(first), v(out),
                                         v(nr)) == 0
        check((out, nr), want, ("host", stride))
    eng.close()


# ---- GPU 7: the whole path ----------------------------------------------------------------------------------------------------------
def whole_path_case(B, T=64, K=12):
    rng = np.random.default_rng(41)
    maxf = T + 30
    bank = synth.word_bank(6)
    eng = Engine(max_frames=maxf, device=0)
    tfr = [int(v) for v in rng.integers(int(0.7 * T), int(1.3 * T), K)]
    tfr[3] = T // 2 - 6  # outside the length gate
    tp = synth.make_utterances(np.arange(K) % 6, tfr, seed=51, bank=bank, S=synth.buf_len_for(max(tfr)), device="cuda:0")
    vad, mf = eng.features_dev(tp)
    torch.cuda.synchronize()
    vd = engine.vad_from_torch(vad)
    assert np.all(vd["status"] == 0)
    tm = np.zeros((K, maxf + 1, 12), np.int16)
    tm[:, :maxf] = mf.cpu().numpy()
    valid = np.ones(K, np.uint8)
    valid[5] = 0
    eng.set_templates_dense(tm, vd["frm_num"], valid)
    eng.set_word_map(None, 4)  # the firmware's map
    pcm = synth.as_u16_numpy(synth.make_utterances(rng.integers(0, 6, B), [T] * B, seed=52, bank=bank))
    pcm[2] = 2048  # no speech: VAD fail
    return eng, pcm, tm, np.where(valid != 0, vd["frm_num"], 0).astype(np.uint32)


def filled(eng, B, n_best, rescore):
    o = eng.alloc_outputs(B, "cuda:0")
    o["nbest"] = torch.empty(B, n_best, 4, dtype=torch.int32, device="cuda:0")
    o["n_matched"] = torch.empty(B, dtype=torch.int32, device="cuda:0")
    if rescore:
        o["rescored"] = torch.empty(B, n_best, 4, dtype=torch.int32, device="cuda:0")
        o["n_rescored"] = torch.empty(B, dtype=torch.int32, device="cuda:0")
    for t in o.values():
        t.view(torch.uint8).fill_(0xA5)
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [False, True])
def test_whole_path_device_and_host_forms(chunks):
    B, n_best = 53, 3
    eng, pcm, tm, tf = whole_path_case(B)
    if chunks:
        eng.set_pipeline(3, 16, 4)  # 3 chunks of 18 / 18 / 17 rows on three streams
    x = torch.from_numpy(pcm.view(np.int16)).cuda()
    plain = eng.recognize_nbest_dev(x, filled(eng, B, n_best, False), n_best)
    o = eng.recognize_nbest_dev(x, filled(eng, B, n_best, True), n_best, rescore=True)
    torch.cuda.synchronize()
    for k in plain:  # every existing output: the N-best call's bytes
        assert torch.equal(o[k], plain[k]), k
    stage = eng.rescore_nbest_dev(o["mfcc"], o["vad"][:, 9], o["nbest"], 12)
    torch.cuda.synchronize()
    assert torch.equal(o["rescored"], stage[0]) and torch.equal(o["n_rescored"], stage[1])
    # ... and the definition, from the oracle, on the frame counts of the VAD records
    vd = engine.vad_from_torch(o["vad"])
    mf = o["mfcc"].cpu().numpy()
    dp = ol.Oracle(max_frames=eng.max_frames).dtw_dp_batch(mf, vd["frm_num"], tm, tf)
    first = engine.nbest_from_torch(o["nbest"])
    want = rescored(dp, np.arange(12) // 4, first)
    check((engine.nbest_from_torch(o["rescored"]), o["n_rescored"].cpu().numpy()), want, "whole path")
    assert (want[1] > 0).sum() > B // 2 and want[1][2] == 0
    # the first-pass list not wanted back
    o2 = filled(eng, B, n_best, True)
    o2["nbest"] = False
    eng.recognize_nbest_dev(x, o2, n_best, rescore=True)
    torch.cuda.synchronize()
    for k in ("results", "scores", "mfcc", "vad", "n_matched", "rescored", "n_rescored"):
        assert torch.equal(o2[k], o[k]), k
    # a side stream
    o3 = filled(eng, B, n_best, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.recognize_nbest_dev(x, o3, n_best, rescore=True)
    torch.cuda.synchronize()
    for k in o:
        assert torch.equal(o3[k], o[k]), k
    # host form
    h, hp = eng.recognize_nbest(pcm, n_best, rescore=True), eng.recognize_nbest(pcm, n_best)
    for k in hp:
        assert h[k].tobytes() == hp[k].tobytes(), k
    check((h["rescored"], h["n_rescored"]), want, "host whole path")
    check(eng.rescore_nbest(h["mfcc"], h["vad"]["frm_num"], h["nbest"]), want, "host stage on host outputs")
    L, v, S = eng.L, engine._vp, pcm.shape[1]
    rs, nr, res = np.zeros((B, n_best), NBEST_DTYPE), np.zeros(B, np.uint32), np.zeros(B, RESULT_DTYPE)
    assert L.sr_recognize_rescored_batch(eng.h, v(pcm), U64(S), U32(S), U32(B), U32(n_best), None, None, v(rs), v(nr), v(res), None, None,
                                         None) == 0  # every optional output NULL
    check((rs, nr), want, "host whole path, NULL outputs")
    assert res.tobytes() == hp["results"].tobytes()
    eng.close()


# ---- GPU 8: buffer contracts ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_guarded_outputs_and_poisoned_feature_rows(canary):
    fx = base_fixture()
    eng = base_engine()
    inf, dp = fx["inf"], fx["dp"]
    # every row >= frames[row] of a record is poison, and so are the s16 in front of record 0 and behind the last one
    rec = poison_feature_rows(fx["im"].copy(), inf)
    lead, tail = 12 * 50, 12 * 70
    flat = np.empty(lead + rec.size + tail, np.int16)
    flat[0::2], flat[1::2] = 0x7FFF, -0x8000
    flat[lead:lead + rec.size] = rec.reshape(-1)
    d_flat = torch.from_numpy(flat).cuda()
    first, _ = eng.nbest(eng.dtw(fx["im"], inf)[0], 16)
    sid = torch.cuda.current_stream().cuda_stream
    d_inf = torch.from_numpy(np.array(inf).view(np.int32)).cuda()
    for n_best in (1, 5, 16):
        lists = np.ascontiguousarray(first[:, :n_best])
        want = rescored(dp, WORDS0, lists)
        g_in = guarded_out((B0, n_best), NBEST_DTYPE, canary, 4096, "cuda:0", "nbest_in")
        g_in.flat[g_in.lo:g_in.hi] = torch.from_numpy(lists.view(np.uint8).reshape(-1)).cuda()
        for with_n in (True, False):
            g_nb = guarded_out((B0, n_best), NBEST_DTYPE, canary, 4096, "cuda:0", "rescored")
            g_nr = guarded_out((B0,), np.uint32, canary, 4096, "cuda:0", "n_rescored")
            assert eng.L.sr_rescore_nbest_dp_dev(eng.h, P(d_flat.data_ptr() + 2 * lead), P(d_inf.data_ptr()), U32(1), U32(B0), U32(n_best),
                                                 P(g_in.ptr), P(g_nb.ptr), P(g_nr.ptr) if with_n else None, P(sid)) == 0
            torch.cuda.synchronize()
            g_nb.check_equals(want[0])
            g_nr.check_equals(want[1]) if with_n else g_nr.check_untouched()
            g_in.check_equals(lists)  # never written
        h_nb = guarded_out((B0, n_best), NBEST_DTYPE, canary, 4096, None, "rescored")
        h_nr = guarded_out((B0,), np.uint32, canary, 4096, None, "n_rescored")
        keep = lists.copy()
        assert eng.L.sr_rescore_nbest_dp(eng.h, engine._vp(rec), engine._vp(inf), U32(1), U32(B0), U32(n_best), engine._vp(lists), P(h_nb.ptr),
                                         P(h_nr.ptr)) == 0
        h_nb.check_equals(want[0])
        h_nr.check_equals(want[1])
        assert lists.tobytes() == keep.tobytes()
    eng.close()


# ---- GPU 9: bad arguments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments_write_nothing():
    fx = base_fixture()
    eng = base_engine()
    n, nb_max = 9, 17
    im, inf = np.ascontiguousarray(fx["im"][4:4 + n]), np.ascontiguousarray(fx["inf"][4:4 + n])
    lists = np.ascontiguousarray(eng.nbest(eng.dtw(im, inf)[0], 16)[0])
    lists17 = np.concatenate([lists, lists[:, :1]], 1)
    d_im, d_inf = torch.from_numpy(np.array(im)).cuda(), torch.from_numpy(np.array(inf).view(np.int32)).cuda()
    d_in = torch.from_numpy(lists17.view(np.int32).reshape(n, nb_max, 4)).cuda()
    bank = synth.word_bank(6)
    pcm = synth.as_u16_numpy(synth.make_utterances(np.arange(n) % 6, [60] * n, seed=3, bank=bank))
    d_pcm = torch.from_numpy(pcm.view(np.int16)).cuda()
    S = pcm.shape[1]
    sid = torch.cuda.current_stream().cuda_stream
    v = engine._vp

    def outs(dev):
        return [guarded_out((n, nb_max), NBEST_DTYPE, 0xA5, 4096, dev, "rescored"), guarded_out((n,), np.uint32, 0xA5, 4096, dev, "n_rescored"),
                guarded_out((n, nb_max), NBEST_DTYPE, 0xA5, 4096, dev, "nbest"), guarded_out((n,), np.uint32, 0xA5, 4096, dev, "n_matched"),
                guarded_out((n,), RESULT_DTYPE, 0xA5, 4096, dev, "results")]

    def every_form(e, want, n_best=4, stride=1, null=None, alias=False, whole=True):
        L, h = e.L, e.h
        g = outs("cuda:0")
        a = dict(mfcc=P(d_im.data_ptr()), frames=P(d_inf.data_ptr()), lists=P(d_in.data_ptr()), out=P(g[0].ptr), pcm=P(d_pcm.data_ptr()),
                 res=P(g[4].ptr))
        if null:
            a[null] = None
        if alias:
            a["out"] = a["lists"]
        if null not in ("pcm", "res"):
            assert L.sr_rescore_nbest_dp_dev(h, a["mfcc"], a["frames"], U32(stride), U32(n), U32(n_best), a["lists"], a["out"], P(g[1].ptr),
                                             P(sid)) == want, "dev"
        if whole and null not in ("mfcc", "frames", "lists"):
            first = a["out"] if alias else P(g[2].ptr)
            assert L.sr_recognize_rescored_batch_dev(h, a["pcm"], U64(S), U32(S), U32(n), U32(n_best), first, P(g[3].ptr), a["out"],
                                                     P(g[1].ptr), a["res"], None, None, None, P(sid)) == want, "whole dev"
        torch.cuda.synchronize()
        for x in g:
            x.check_untouched()
        assert torch.equal(d_in.cpu(), torch.from_numpy(lists17.view(np.int32).reshape(n, nb_max, 4)))
        g = outs(None)
        a = dict(mfcc=v(im), frames=v(inf), lists=v(lists17), out=P(g[0].ptr), pcm=v(pcm), res=P(g[4].ptr))
        if null:
            a[null] = None
        if alias:
            a["out"] = a["lists"]
        if null not in ("pcm", "res"):
            assert L.sr_rescore_nbest_dp(h, a["mfcc"], a["frames"], U32(stride), U32(n), U32(n_best), a["lists"], a["out"], P(g[1].ptr)) == want, "host"
        if whole and null not in ("mfcc", "frames", "lists"):
            first = a["out"] if alias else P(g[2].ptr)
            assert L.sr_recognize_rescored_batch(h, a["pcm"], U64(S), U32(S), U32(n), U32(n_best), first, P(g[3].ptr), a["out"], P(g[1].ptr),
                                                 a["res"], None, None, None) == want, "whole host"
        for x in g:
            x.check_untouched()

    every_form(eng, BAD_ARG, n_best=0)
    every_form(eng, BAD_ARG, n_best=17)
    for null in ("mfcc", "frames", "lists", "out", "pcm", "res"):
        every_form(eng, BAD_ARG, null=null)
    every_form(eng, BAD_ARG, alias=True)
    every_form(eng, BAD_ARG, stride=0, whole=False)  # (the whole-path forms have no such argument)
    for bad_len in (K0 - 1, K0 + 1):  # a map for another number of slots
        eng.set_word_map(np.arange(bad_len, dtype=np.uint32) // 4)
        every_form(eng, BAD_ARG)
        assert b"word map" in eng.L.sr_last_error()
    eng.set_word_map(WORDS0)
    check(dev_call(eng, im, inf, lists[:, :4]), rescored(fx["dp"][4:4 + n], WORDS0, lists[:, :4]), "after the refusals")
    eng.close()
    e2 = Engine(max_frames=MAXF, device=0)  # no templates
    every_form(e2, NO_TEMPLATES)
    e2.close()
    e3 = Engine(max_frames=MAXF, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    every_form(e3, BAD_CONFIG, whole=False)  # (without a store the whole-path forms say so first, as sr_recognize_batch does)
    tm13 = np.zeros((4, MAXF + 1, 13), np.int16)
    e3.set_templates_dense(tm13, np.full(4, 30, np.uint32))
    every_form(e3, BAD_CONFIG)
    e3.close()
