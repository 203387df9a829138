"""Live connected-word decoding: the decoder's state carried between pushes (include/sr_engine.h, "live connected-word
decoding").

The rule: whatever the chunking, the row a push emits for a channel is the batch decoder's record (tests/chain_ref.py) for
everything pushed to it as ONE row.  tests/chain_live_ref.py restates the resumable level and builds one history per recording;
the CPU tests hold it to chain_ref over random chunkings and over prefixes, the GPU tests compare records, word rows, level
costs and row labels byte for byte, after every push.  No tolerances.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chain_live_ref as live
import chain_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
FUNCS = ("sr_decode_live_geometry", "sr_decode_live_open", "sr_decode_live_push_dev", "sr_decode_live_push", "sr_decode_live_push_pcm_dev",
         "sr_decode_live_push_pcm", "sr_decode_live_end")
BAD_ARG = 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
N_CH, MAX_WORDS, UTT, MAXF = 6, ref.PLANT_MAX_WORDS, 200, 200
FRAME_LEN, HOP = 160, 80


def same_row(got, want, what):
    """(rec, words, level_cost) of one emitted row against the reference's, byte for byte"""
    for name, g, w in zip(("rec", "words", "level_cost"), got, want):
        g, w = np.ascontiguousarray(g).view(np.uint32).reshape(-1), np.ascontiguousarray(w).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{what}: {name} differs from word {at} on: got {g.tolist()} want {w.tolist()}")


# ---- CPU: the surface (fails without the feature) ----------------------------------------------------------------------------
def test_header_declares_the_live_decoding_api_and_libraries_export_it():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for fn in FUNCS:
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert re.search(r"\bvoid sr_decode_live_close\s*\(", src) and hasattr(engine.load_library(), "sr_decode_live_close")
    assert src.index("sr_decode_geometry") < src.index("sr_decode_live_geometry") < src.index("sr_dtw_dp_align_dev")  # after the decoder's section
    assert re.search(r"typedef struct sr_chain_live_row \{\s*uint32_t channel;\s*uint32_t frames;\s*\} sr_chain_live_row;", src)
    assert engine.CHAIN_LIVE_ROW_DTYPE == live.CHAIN_LIVE_ROW_DTYPE and engine.CHAIN_LIVE_ROW_DTYPE.itemsize == 8
    assert engine.CHAIN_REC_DTYPE.itemsize == 16 and engine.CHAIN_WORD_DTYPE.itemsize == 32
    assert callable(getattr(Engine, "decode_live", None)) and callable(engine.decode_live_geometry)
    for meth in ("push", "push_dev", "push_pcm", "push_pcm_dev", "end", "close"):
        assert callable(getattr(engine.DecodeSession, meth, None)), meth
    assert isinstance(engine.DecodeSession.frames, property)


def test_geometry_follows_its_formulas():
    cap = engine.spot_geometry(10, 119)["max_tpl_rows"]
    for tpl, K, W, utt in ((15, 9, 5, 200), (1, 1, 1, 1), (120, 100, 8, 2000), (70, 6, 16, 16383), (14, 5, 3, 160)):
        g = engine.decode_live_geometry(tpl, K, W, utt, min(utt, 64))
        assert g["state_bytes"] == W * K * tpl * 16 + (utt + 1) * (W * 8 + (W + 1) * 4), (tpl, K, W, utt)
        assert g["max_tpl_rows"] == cap and g["launches"] == 2 * W + 2
        assert g["state_bytes"] - W * K * tpl * 16 == engine.decode_geometry(tpl, max(utt, 2), W)["scratch_bytes"] or utt < 2  # the batch scratch's row
    assert engine.decode_live_geometry(16383, 65536, 16, 16383, 1)["state_bytes"] == 0xFFFFFFFF  # saturates
    L, out = engine.load_library(), (U32 * 3)()
    for bad in ((0, 1, 1, 1, 1), (16384, 1, 1, 1, 1), (10, 0, 1, 1, 1), (10, 65537, 1, 1, 1), (10, 1, 0, 1, 1), (10, 1, 17, 1, 1), (10, 1, 1, 0, 1),
                (10, 1, 1, 16384, 1), (10, 1, 1, 10, 0), (10, 1, 1, 10, 11)):
        assert L.sr_decode_live_geometry(*(U32(v) for v in bad), out) == BAD_ARG, bad
    assert L.sr_decode_live_geometry(U32(10), U32(1), U32(1), U32(10), U32(1), None) == BAD_ARG


# ---- CPU: the design -----------------------------------------------------------------------------------------------------------
def random_chunking(rng, N, hi):
    """sizes 0..hi that sum to N, zeros and ones included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(0, hi + 1))])), N - sum(out)))
    return out


def cut(N, sizes):
    """the sizes in rotation until N frames are used up"""
    out, i = [], 0
    while sum(out) < N:
        out.append(min(sizes[i % len(sizes)], N - sum(out)))
        i += 1
    return out


def test_resumed_level_equals_the_whole_row_over_random_chunkings():
    rng = np.random.default_rng(31)
    shapes = [(130, 9, 2), (70, 1, 2), (66, 3, 3000), (129, 14, 3000)] + [(int(rng.integers(1, 100)), int(rng.integers(1, 20)), 2) for _ in range(8)]
    sizes = set()
    for N, M, amp in shapes:
        d = ref.local_dis(rng.integers(-amp, amp + 1, (N, 12)), rng.integers(-amp, amp + 1, (M, 12)))
        for skip in (None, 7 if amp == 2 else 8000):
            # E_{l-1}: level 0 (every start reachable with skipping, only frame 0 without), and a level with holes
            holes = [None if rng.integers(0, 3) == 0 else int(rng.integers(0, 50000)) for _ in range(N + 1)]
            for e_prev in (ref.e0(N, skip), holes):
                whole = ref.level_end_row(d, e_prev)
                want = np.array([live.INF64 if v == ref.INF else (v[0] << 32) | v[1] for v in whole], np.uint64)
                for chunks in ([N], cut(N, [1]), cut(N, [63, 64, 65]), cut(N, [65, 64, 63]), random_chunking(rng, N, N), random_chunking(rng, N, 7)):
                    assert sum(chunks) == N
                    state, got, at = None, [], 0
                    for n in chunks:
                        end, state = live.resume_level(d[at:at + n], e_prev[at:at + n], state)
                        got.append(end)
                        at += n
                    assert np.array_equal(np.concatenate(got), want), (N, M, amp, skip, chunks)
                    assert state[2] == N
                    sizes.update(chunks)
    assert {0, 1, 63, 64, 65, 130} <= sizes


@functools.lru_cache(maxsize=None)
def planted_dis(r):
    fx = ref.planted()
    N = int(fx["inf"][r])
    return N, live.slot_distances(fx["im"][r, :N], fx["tm"], fx["tf"])


def test_prefix_decodes_equal_the_batch_definition_of_every_prefix():
    fx = ref.planted()
    for r in range(ref.PLANT_ROWS):
        N, dis = planted_dis(r)
        prefixes = sorted({0, 1, N} | set(range(0, N + 1, 7)))
        for skip, n_exact, wc in ((ref.PLANT_SKIP, 0, 0), (None, 0, 0), (ref.PLANT_SKIP, 3, 1000)) if r < 2 else ((ref.PLANT_SKIP, 0, 0),):
            got = live.prefix_decodes(dis, N, prefixes, ref.PLANT_MAX_WORDS, n_exact, skip, wc)
            for n in prefixes:
                want = ref.decode_row([d[:n] for d in dis], n, ref.PLANT_MAX_WORDS, n_exact, skip, wc)
                assert got[n] == want, (r, n, skip, n_exact, wc)
                if skip is not None and not n_exact and n >= 7:  # 7 frames hold a word of any of the templates (8..14 rows)
                    assert want["status"] == ref.CH_OK, (r, n)
            if skip is not None and not n_exact:  # at full length: the planted slots
                assert [w[0] for w in got[N]["words"]] == fx["seq"][r], r


def test_a_channel_pushed_step_by_step_keeps_the_batch_history():
    """init of the new positions, resumed columns, the keys' minimum, E_l extended from the carried E_l(x0): after every push
    the history and the parse are those of everything pushed as one row"""
    fx, rng = ref.planted(), np.random.default_rng(33)
    for r, skip, n_exact, wc in ((3, ref.PLANT_SKIP, 0, 0), (7, None, 0, 0), (11, ref.PLANT_SKIP, 3, 1000), (2, 700, 0, 0)):
        N, dis = planted_dis(r)
        dis = dis[:2] + [None] + dis[3:]  # an invalid slot
        A, E = live.history(dis, N, 3, skip, wc)
        for chunks in ([N], cut(N, [1]), cut(N, [63, 64, 65]), random_chunking(rng, N, 40)):
            ch = live.Channel([None if d is None else d.shape[1] for d in dis], 3, n_exact, skip, wc)
            at = 0
            for n in chunks:
                got = ch.push([None if d is None else d[at:at + n] for d in dis])
                at += n
                assert got == live.trace(A, E, at, 3, n_exact, wc), (r, skip, chunks, at)
            assert ch.A[1:] == [a for a in A[1:]] and ch.E == E, (r, skip, chunks)


def test_host_mirror_runs_clean_under_the_sanitizers(tmp_path):
    """row counting, cap and refusal order, distinct-channel lists of csrc/sr_decode_live_plan.h: a stand-alone program on the
    CPU under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "decode_live_plan", "plan_check.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)


# ---- GPU: fixtures -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store():
    """the planted store (K = 5 templates of 8..14 frames), one invalid slot and templates of 1, 2 and 3 rows"""
    fx, rng = ref.planted(), np.random.default_rng(41)
    tf = np.concatenate([fx["tf"], [9, 1, 2, 3]]).astype(np.uint32)
    valid = np.ones(len(tf), np.uint8)
    valid[5] = 0
    tm = np.zeros((len(tf), 15, 12), np.int16)
    tm[:5] = fx["tm"]
    for k in range(5, len(tf)):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    for a in (tm, tf, valid):
        a.setflags(write=False)
    return tm, tf, valid


@functools.lru_cache(maxsize=None)
def feats():
    """channel c = planted rows c and 11 - c with the short templates planted behind them -> (f int16 [N_CH, UTT, 12], frames
    [N_CH])"""
    fx, (tm, tf, _) = ref.planted(), store()
    f = np.zeros((N_CH, UTT, 12), np.int16)
    n = np.zeros(N_CH, np.int64)
    for c in range(N_CH):
        N = 0
        for r in (c, ref.PLANT_ROWS - 1 - c):
            f[c, N:N + fx["inf"][r]] = fx["im"][r, :fx["inf"][r]]
            N += int(fx["inf"][r])
        for k in (8, 7, 6):  # 3, 2 and 1 rows, back to back
            f[c, N:N + tf[k]] = tm[k, :tf[k]]
            N += int(tf[k])
        n[c] = N
    assert 65 < n.min() and n.max() <= UTT and len(set(n.tolist())) > 3
    f.setflags(write=False)
    n.setflags(write=False)
    return f, n


@functools.lru_cache(maxsize=None)
def recording(c, skip, word_cost):
    """the history of channel c's recording and the silence behind it, UTT frames in all, shared by every test that feeds it (the
    history of a recording is a prefix of that of any longer one)"""
    f, _ = feats()
    return live.Recording(f[c], *store(), MAX_WORDS, 0, skip, word_cost)


def make_engine(**kw):
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(*store())
    return eng


def rows_of(out):
    """the emitted rows of a push as numpy (rec [n], words [n, W], level_cost [n, W])"""
    rec, words, lc = out["rec"], out["words"], out["level_cost"]
    if not isinstance(rec, np.ndarray):
        torch.cuda.synchronize()
        n = out["n_rows"]
        W = words.shape[1]
        rec = rec.cpu().numpy().view(ref.CHAIN_REC_DTYPE).reshape(n)
        words = words.cpu().numpy().view(ref.CHAIN_WORD_DTYPE).reshape(n, W)
        lc = lc.cpu().numpy().view(np.uint32).reshape(n, W)
    return rec, words, lc


class Follower:
    """feeds a session push by push; every push is checked against what the counts alone say (n_rows, the row labels and their
    order) and every emitted row against the reference at that channel's N"""

    def __init__(self, ses, recs, n_exact, what):
        self.ses, self.recs, self.n_exact, self.what = ses, recs, n_exact, what
        self.count = [0] * len(recs)
        self.last = [None] * len(recs)

    def take(self, out, new, emit=None, session_is_here=True):
        emit = [n > 0 for n in new] if emit is None else emit
        self.count = [a + int(b) for a, b in zip(self.count, new)]
        exp = [(c, self.count[c]) for c in range(len(new)) if emit[c]]
        assert out["n_rows"] == len(exp) and [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == exp, (out["rows"], exp)
        assert not session_is_here or self.ses.frames.tolist() == self.count
        rec, words, lc = rows_of(out)
        for r, (c, N) in enumerate(exp):
            self.last[c] = (rec[r], words[r], lc[r])
            same_row(self.last[c], self.recs[c].row(N, self.n_exact), f"{self.what}, channel {c} at {N} frames")


def feed(eng, schedule, skip, n_exact, word_cost, form, what):
    f, n = feats()
    ses = eng.decode_live(N_CH, max(max(s) for s in schedule), UTT, MAX_WORDS, n_exact, skip, word_cost)
    fol = Follower(ses, [recording(c, skip, word_cost) for c in range(N_CH)], n_exact, what)
    d_f = torch.from_numpy(np.array(f)).cuda()
    at = [0] * N_CH
    for cnt in schedule:
        F = max(max(cnt), 1)
        if form == "dev":
            chunk = torch.full((N_CH, F, 12), 0x7FFF, dtype=torch.int16, device="cuda:0")  # poison past n[c]
            for c in range(N_CH):
                chunk[c, :cnt[c]] = d_f[c, at[c]:at[c] + cnt[c]]
            out = ses.push_dev(chunk, np.array(cnt, np.uint32))
        else:
            chunk = np.zeros((N_CH, F, 12), np.int16)
            for c in range(N_CH):
                chunk[c, :cnt[c]] = f[c, at[c]:at[c] + cnt[c]]
            out = ses.push(poison_feature_rows(chunk, cnt), np.array(cnt, np.uint32))
        fol.take(out, cnt)
        at = [a + b for a, b in zip(at, cnt)]
    assert at == n.tolist()
    ses.close()
    return fol


def per_channel(lists):
    """one chunking per channel -> per push the counts (0 once a channel is done)"""
    n = max(len(x) for x in lists)
    return [[x[i] if i < len(x) else 0 for x in lists] for i in range(n)]


@functools.lru_cache(maxsize=None)
def chunkings():
    _, n = feats()
    rng = np.random.default_rng(700)
    rand = [random_chunking(rng, int(N), 70) for N in n]
    assert any(0 in r for r in rand)
    return {"one frame": per_channel([[1] * int(N) for N in n]),
            "63/64/65/rest": per_channel([cut(int(N), [63, 64, 65]) for N in n]),
            "one push": per_channel([[int(N)] for N in n]),
            "random": per_channel(rand)}


# ---- GPU 1: chunking invariance ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("skip,word_cost", [(ref.PLANT_SKIP, 0), (None, 0), (ref.PLANT_SKIP, 1000), (None, 1000)])
def test_every_chunking_gives_the_whole_recordings_parse(skip, word_cost):
    """6 channels = two groups of kSpotWaves, the second half empty; a different planted row per channel"""
    f, n = feats()
    eng = make_engine()
    for n_exact in (0, 3):
        whole = eng.decode_words(np.array(f), n.astype(np.uint32), MAX_WORDS, n_exact, skip, word_cost)
        if skip is not None and not n_exact:
            assert np.all(whole[0]["status"] == ref.CH_OK)
        for name, sched in chunkings().items():
            what = f"skip {skip}, word_cost {word_cost}, n_words {n_exact}, chunking '{name}'"
            fol = feed(eng, sched, skip, n_exact, word_cost, "host" if name == "random" else "dev", what)
            for c in range(N_CH):
                same_row(fol.last[c], (whole[0][c], whole[1][c], whole[2][c]), what + f": final row of channel {c} against decode_words")
    eng.close()


# ---- GPU 2: ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_keep_their_rule_across_a_push_boundary():
    """the tie rows of tests/test_chain.py, cut at every position: smallest start, then slot, then fewest words"""
    rng = np.random.default_rng(930)
    M, W = 9, 6
    t = rng.integers(-3000, 3001, (M, 12)).astype(np.int16)
    tm = np.zeros((4, 2 * M + 1, 12), np.int16)
    tm[0, :M] = tm[1, :M] = t                       # two identical templates
    tm[2, :2 * M] = np.concatenate([t, t])          # the word said twice, as one template
    tm[3, :M] = rng.integers(-3000, 3001, (M, 12))  # something else
    tf = np.array([M, M, 2 * M, M], np.uint32)
    rows = [np.concatenate([t, t, t]), np.concatenate([t, t])]
    recs = [live.Recording(r, tm, tf, None, W) for r in rows]
    rec, words, _ = recs[0].row(3 * M)
    assert tuple(rec[()]) == (0, 2, 0, ref.CH_OK) and [tuple(w)[:4] for w in words[:2]] == [(0, 0, 0, M - 1), (2, 2, M, 3 * M - 1)]
    rec, words, _ = recs[1].row(2 * M)
    assert tuple(rec[()]) == (0, 1, 0, ref.CH_OK) and tuple(words[0])[:4] == (2, 2, 0, 2 * M - 1)
    assert recs[0].row(3 * M, 3)[1][:3]["slot"].tolist() == [0, 0, 0]  # the count given: the smaller of the twin slots, three times
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(tm, tf)
    for n_exact in (0, 3):
        ses = eng.decode_live(2, 3 * M, 3 * M, W, n_exact)
        fol = Follower(ses, recs, n_exact, f"ties, n_words {n_exact}")
        for s in range(1, 3 * M):
            first = [s, min(s, 2 * M - 1)]
            for cnt, at in ((first, [0, 0]), ([3 * M - first[0], 2 * M - first[1]], first)):
                chunk = np.zeros((2, max(cnt), 12), np.int16)
                for c in range(2):
                    chunk[c, :cnt[c]] = rows[c][at[c]:at[c] + cnt[c]]
                fol.take(ses.push_dev(torch.from_numpy(chunk).cuda(), np.array(cnt, np.uint32)), cnt)
            end = ses.end([0, 1])
            for c in range(2):
                same_row((end["rec"][c], end["words"][c], end["level_cost"][c]), recs[c].row(len(rows[c]), n_exact), f"cut {s}: end of channel {c}")
            fol.count = [0, 0]
        ses.close()
    eng.close()


# ---- GPU 3: amplitude ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_amplitude_rows_whose_distances_wrap():
    tm, tf, valid = store()
    big = np.array(tm)
    big[4, :tf[4]] = np.random.default_rng(900).integers(-30000, 30001, (tf[4], 12))  # squared differences that wrap u32
    f, n = feats()
    f = f.copy()
    f[2, 20:20 + tf[4]] = -big[4, :tf[4]]
    d2 = ((f[2, 20:20 + tf[4]].astype(np.int64) - big[4, :tf[4]]) ** 2).sum(1)
    assert d2.max() >= 2 ** 32
    f[3] = np.random.default_rng(901).integers(-32768, 32768, (UTT, 12))
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(big, tf, valid)
    recs = [live.Recording(f[c, :n[c]], big, tf, valid, MAX_WORDS, 0, ref.PLANT_SKIP, 0) for c in range(N_CH)]
    ses = eng.decode_live(N_CH, 70, UTT, MAX_WORDS, 0, ref.PLANT_SKIP)
    fol = Follower(ses, recs, 0, "full amplitude")
    at = [0] * N_CH
    for cnt in chunkings()["random"]:
        chunk = np.zeros((N_CH, max(max(cnt), 1), 12), np.int16)
        for c in range(N_CH):
            chunk[c, :cnt[c]] = f[c, at[c]:at[c] + cnt[c]]
        fol.take(ses.push_dev(torch.from_numpy(chunk).cuda(), np.array(cnt, np.uint32)), cnt)
        at = [a + b for a, b in zip(at, cnt)]
    whole = eng.decode_words(f, n.astype(np.uint32), MAX_WORDS, 0, ref.PLANT_SKIP, 0)
    for c in range(N_CH):
        same_row(fol.last[c], (whole[0][c], whole[1][c], whole[2][c]), f"channel {c} against decode_words")
    ses.close()
    eng.close()


# ---- GPU 4: end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_returns_the_parse_and_leaves_the_channel_fresh():
    f, n = feats()
    skip = ref.PLANT_SKIP
    recs = [recording(c, skip, 0) for c in range(N_CH)]
    eng = make_engine()
    ses = eng.decode_live(N_CH, 70, UTT, MAX_WORDS, 0, skip)
    fol = Follower(ses, recs, 0, "end")
    d_f = torch.from_numpy(np.array(f)).cuda()
    assert ses.end([])["n_rows"] == 0
    cnt = [40, 50, 0, 64, 1, 0]
    fol.take(ses.push_dev(d_f[:, :64].contiguous(), np.array(cnt, np.uint32)), cnt)
    out = ses.end([1, 5, 1, 3, 5, 1])  # channel 1 and 5 listed more than once; channel 5 is empty
    assert out["n_rows"] == 3 and [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(1, 50), (5, 0), (3, 64)]
    same_row((out["rec"][0], out["words"][0], out["level_cost"][0]), recs[1].row(50), "end of channel 1")
    same_row((out["rec"][2], out["words"][2], out["level_cost"][2]), recs[3].row(64), "end of channel 3")
    assert tuple(out["rec"][1]) == (DIS_ERR, 0, 0, ref.CH_NONE) and np.all(out["words"][1].view(np.uint32) == 0xFFFFFFFF)
    assert np.all(out["level_cost"][1] == DIS_ERR)
    assert ses.frames.tolist() == [40, 0, 0, 0, 1, 0]
    fol.count = [40, 0, 0, 0, 1, 0]
    # channels 1, 3 and 5 start again at frame 0 (the same frames give the same rows); channels 0 and 4 go on
    nxt = [30, 64, 0, 10, 63, 2]
    chunk = torch.zeros(N_CH, 64, 12, dtype=torch.int16, device="cuda:0")
    for c, a in enumerate([40, 0, 0, 0, 1, 0]):
        chunk[c, :nxt[c]] = d_f[c, a:a + nxt[c]]
    fol.take(ses.push_dev(chunk, np.array(nxt, np.uint32)), nxt)
    out = ses.end(list(range(N_CH)))
    assert [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(0, 70), (1, 64), (2, 0), (3, 10), (4, 64), (5, 2)]
    for r, (c, N) in enumerate([(0, 70), (1, 64), (3, 10), (4, 64), (5, 2)]):
        r += r >= 2
        same_row((out["rec"][r], out["words"][r], out["level_cost"][r]), recs[c].row(N), f"second end, channel {c}")
    assert out["rec"][2]["status"] == ref.CH_NONE and ses.frames.tolist() == [0] * N_CH
    assert ses.end([2, 2])["n_rows"] == 1
    ses.close()
    eng.close()


# ---- GPU 5: PCM sessions ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pcm_sessions_equal_the_whole_path_on_the_whole_recording():
    rng = np.random.default_rng(800)
    R_MAXF, W, skip = 119, 5, 3000
    eng = Engine(max_frames=R_MAXF, device=0)
    R = 1 + (R_MAXF - 1) * HOP + FRAME_LEN + 37  # 119 frames and a remainder
    X = (2048 + 600 * np.sin(np.arange(R)[None] * np.array([[0.05], [0.11]])) + rng.integers(-300, 301, (2, R))).astype(np.uint16)
    mid = np.array([2048, 2040], np.uint32)
    n, mf = eng.mfcc(X, [1, 1], [R, R], mid)
    assert list(n) == [R_MAXF, R_MAXF]
    tf = np.array([1, 2, 7, 12, 20, 16], np.uint32)
    tm, valid = np.zeros((6, 21, 12), np.int16), np.array([1, 1, 1, 0, 1, 1], np.uint8)
    for k, (c, at) in enumerate(((0, 5), (1, 20), (0, 33), (1, 0), (1, 40), (0, 60))):
        tm[k, :tf[k]] = mf[c, at:at + tf[k]]
    eng.set_templates_dense(tm, tf, valid)
    whole = eng.decode_words_pcm(X, [1, 1], [R, R], mid, W, 0, skip, 0)
    assert np.all(whole["rec"]["status"] == ref.CH_OK)
    recs = [live.Recording(mf[c, :R_MAXF], tm, tf, valid, W, 0, skip, 0) for c in range(2)]
    chunk_max = 400
    scheds = {True: [[1, 1]] * 200 + per_channel([cut(R - 200, [HOP - 1, HOP, FRAME_LEN, 400, 0, 237]), random_chunking(rng, R - 200, chunk_max)]),
              False: per_channel([cut(R, [400, 399, 1]), cut(R, [161, 80])])}
    for dev, sched in scheds.items():
        ses = eng.decode_live(2, chunk_max, R_MAXF, W, 0, skip, 0, mid)
        fol = Follower(ses, recs, 0, f"pcm, dev {dev}")
        got = [0, 0]
        for cnt in sched:
            S = (max(max(cnt), 1) + 7) // 8 * 8
            chunk = np.full((2, S), 4095, np.uint16)  # poison past n[c]
            for c in range(2):
                chunk[c, :cnt[c]] = X[c, got[c]:got[c] + cnt[c]]
            now = [g + v for g, v in zip(got, cnt)]
            new = [live.pcm_frames(a, FRAME_LEN, HOP) - live.pcm_frames(b, FRAME_LEN, HOP) for a, b in zip(now, got)]
            if dev:
                out = ses.push_pcm_dev(torch.from_numpy(chunk.view(np.int16)).cuda(), np.array(cnt, np.uint32))
            else:
                out = ses.push_pcm(chunk, np.array(cnt, np.uint32))
            fol.take(out, new, [v > 0 for v in cnt])  # a row for every channel that got samples, new frame or not
            got = now
        assert got == [R, R] and fol.count == [R_MAXF, R_MAXF]
        for c in range(2):
            same_row(fol.last[c], (whole["rec"][c], whole["words"][c], whole["level_cost"][c]), f"dev {dev}: channel {c} against decode_words_pcm")
        ses.close()
    eng.close()


# ---- GPU 6: ordering -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pushes_on_different_streams_and_host_pushes_are_ordered():
    """no synchronisation between the pushes: each runs behind the last one's event, whatever stream it is on; two runs give
    identical bytes"""
    f, n = feats()
    skip = ref.PLANT_SKIP
    eng = make_engine()
    d_f = torch.from_numpy(np.array(f)).cuda()
    N = int(n.min())
    sizes = cut(N, [7, 64, 1, 33, 70])
    edges = np.concatenate([[0], np.cumsum(sizes)])
    chunks = [d_f[:, a:b].contiguous() for a, b in zip(edges[:-1], edges[1:])]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    runs = []
    for _ in range(2):
        ses = eng.decode_live(N_CH, 70, UTT, MAX_WORDS, 0, skip)
        fol = Follower(ses, [recording(c, skip, 0) for c in range(N_CH)], 0, "streams")
        outs = []
        for i, chunk in enumerate(chunks):
            st = streams[i % 3]
            outs.append(ses.push_dev(chunk, stream=st) if st is not None else ses.push(np.array(f[:, edges[i]:edges[i + 1]])))
        torch.cuda.synchronize()
        blob = b""
        for size, out in zip(sizes, outs):
            fol.take(out, [size] * N_CH, session_is_here=False)  # (checked after the last push)
            blob += b"".join(np.ascontiguousarray(a).tobytes() for a in rows_of(out))
        runs.append(blob)
        ses.close()
    assert runs[0] == runs[1]
    eng.close()


# ---- GPU 7: contracts ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_guards_and_refusals(canary):
    f, n = feats()
    skip, CHUNK = ref.PLANT_SKIP, 70
    tm, tf, valid = store()
    eng = make_engine()
    ses = eng.decode_live(N_CH, CHUNK, UTT, MAX_WORDS, 0, skip)
    recs = [recording(c, skip, 0) for c in range(N_CH)]
    fol = Follower(ses, recs, 0, f"guards, canary {canary:#x}")
    L, sid = eng.L, torch.cuda.current_stream().cuda_stream
    at = [0] * N_CH

    def push(cnt, max_rows, ok=True, null=None, overlap=False):
        F = max(max(cnt), 1)
        chunk = np.zeros((N_CH, F, 12), np.int16)
        for c in range(N_CH):
            k = min(cnt[c], UTT - at[c])
            chunk[c, :k] = f[c, at[c]:at[c] + k]
        d_chunk = torch.from_numpy(poison_feature_rows(chunk, np.minimum(cnt, F))).cuda()  # padded rows, poison past n[c]
        g_r = guarded_out((max_rows,), ref.CHAIN_REC_DTYPE, canary, 4096, "cuda:0", "rec")
        g_w = guarded_out((max_rows, MAX_WORDS), ref.CHAIN_WORD_DTYPE, canary, 4096, "cuda:0", "words")
        g_l = guarded_out((max_rows, MAX_WORDS), np.uint32, canary, 4096, "cuda:0", "level_cost")
        rows, n_rows = np.full(max_rows + 1, 0x5A5A5A5A, np.uint32).repeat(2).view(live.CHAIN_LIVE_ROW_DTYPE), U32(0xDEAD)
        ptr = dict(mfcc=P(d_chunk.data_ptr()), rec=P(g_r.ptr), words=P(g_w.ptr), lc=P(g_l.ptr), rows=engine._vp(rows))
        if null:
            ptr[null] = None
        if overlap:
            ptr["lc"] = P(g_w.ptr + 16)
        before = ses.frames
        rc = L.sr_decode_live_push_dev(ses.l, ptr["mfcc"], U64(F * 12), engine._vp(np.array(cnt, np.uint32)), U32(0), U32(max_rows), ptr["rec"],
                                       ptr["words"], ptr["lc"], ptr["rows"], C.byref(n_rows), P(sid))
        torch.cuda.synchronize()
        if not ok:
            assert rc == BAD_ARG and n_rows.value == 0xDEAD and np.all(rows.view(np.uint32) == 0x5A5A5A5A), (rc, cnt, L.sr_last_error())
            for g in (g_r, g_w, g_l):
                g.check_untouched()
            assert ses.frames.tolist() == before.tolist()
            return None
        assert rc == 0, L.sr_last_error()
        for g in (g_r, g_w, g_l):
            g.check()
        k = n_rows.value
        for g in (g_r, g_w, g_l):  # rows at and past *n_rows stay untouched
            assert np.all(g.interior().view(np.uint8).reshape(max_rows, -1)[k:] == canary)
        assert np.all(rows.view(np.uint32)[2 * k:] == 0x5A5A5A5A)
        ses._took(rows[:k])
        out = dict(rec=g_r.interior()[:k], words=g_w.interior()[:k], level_cost=g_l.interior()[:k], rows=rows[:k], n_rows=k)
        fol.take(out, cnt)
        for c in range(N_CH):
            at[c] += cnt[c]
        return out

    push([40, 17, 0, 64, 1, 65], 5 + 3)
    assert push([64] * N_CH, N_CH - 1, ok=False) is None and b"max_rows" in L.sr_last_error()       # max_rows too small
    assert push([CHUNK + 1, 1, 1, 1, 1, 1], 8, ok=False) is None and b"chunk_max" in L.sr_last_error()  # a count above chunk_max
    assert push([1] * N_CH, 8, ok=False, null="rec") is None and push([1] * N_CH, 8, ok=False, null="words") is None  # null required pointers
    assert push([1] * N_CH, 8, ok=False, null="rows") is None and push([1] * N_CH, 8, ok=False, null="mfcc") is None
    assert push([1] * N_CH, 8, ok=False, overlap=True) is None and b"overlap" in L.sr_last_error()   # overlapping outputs
    push([64] * N_CH, N_CH)
    push([64, 64, 64, 64, 64, 64], N_CH + 1)  # channels 3 and 5 stand at 192 and 193 of 200
    assert ses.frames.tolist() == [168, 145, 128, 192, 129, 193]
    assert push([1, 1, 1, 9, 1, 1], 8, ok=False) is None and b"utt_frames" in L.sr_last_error()       # past utt_frames
    eng.set_word_map(np.array([1, 2, 3], np.uint32))                                                   # a map for another store
    assert push([1] * N_CH, 8, ok=False) is None and b"word map" in L.sr_last_error()
    eng.set_word_map(None, 1)
    push([1, 0, 3, 8, 0, 7], 4)  # exactly utt_frames on channels 3 and 5: still the reference's rows (zeros past the recording)
    eng.set_templates_dense(tm, tf, valid)                                                             # the same rows, but a new store
    assert push([1, 0, 0, 0, 0, 0], 8, ok=False) is None and b"store changed" in L.sr_last_error()
    assert push([0] * N_CH, 1)["n_rows"] == 0                                                          # nothing pushed, nothing refused
    # ended against a replaced store a recording is dropped; bound to the new store the channels start again
    # end: labels that lie inside the records are refused, nothing is written, the mirror stays
    blob = np.full(N_CH * (16 + MAX_WORDS * 36 + 8), canary, np.uint8)
    ch, n_rows = np.arange(N_CH, dtype=np.uint32), U32(0xDEAD)
    at_w, at_l = blob.ctypes.data + N_CH * 16, blob.ctypes.data + N_CH * (16 + MAX_WORDS * 32)
    for rows_at in (blob.ctypes.data + 8, at_w + 32, at_l):
        assert L.sr_decode_live_end(ses.l, engine._vp(ch), U32(N_CH), P(blob.ctypes.data), P(at_w), P(at_l), P(rows_at), C.byref(n_rows)) == BAD_ARG
        assert b"rows overlaps" in L.sr_last_error() and n_rows.value == 0xDEAD and np.all(blob == canary)
    assert ses.frames.tolist() == [169, 145, 131, 200, 129, 200]
    out = ses.end(list(range(N_CH)))
    assert out["n_rows"] == N_CH and np.all(out["rec"]["status"] == ref.CH_NONE) and np.all(out["rows"]["frames"] == 0)
    fol.count = [0] * N_CH
    for c in range(N_CH):
        at[c] = 0
    push([70, 69, 1, 0, 64, 33], 5)
    ses.close()
    eng.close()
