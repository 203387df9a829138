"""Weighted grammars in live sessions (include/sr_engine.h, "weighted grammars" and "live grammar-constrained decoding").

The rule: whatever the chunking, the row a push emits for a channel is what the weighted definitions give for everything
pushed to it as ONE row.  tests/wgram_ref.py builds one history per recording (A and E depend on frames < p only) and reads
it at every prefix; records, word rows with the state in `reserved` and level costs are compared byte for byte after every
push.  No tolerances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_ref
import gram_ref
import wgram_ref as ref
from chain_live_ref import CHAIN_LIVE_ROW_DTYPE, pcm_frames
from guarded import guarded_out
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine

BAD_ARG = 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
MAXF, W, SKIP = chain_ref.PLANT_MAXF, 4, chain_ref.PLANT_SKIP
N_CH = chain_ref.PLANT_ROWS  # one channel per planted row: three groups of four waves
FRAME_LEN, HOP = 160, 80
SPW2 = np.arange(chain_ref.PLANT_K, dtype=np.uint32) // 2
PAIR_GRAM = gram_ref.grammar_word_pairs(range(5), [(a, b) for a in range(5) for b in range(5) if (a + b) % 2 == 1], first=[0, 1, 2, 4])
JOIN_GRAM = (4, [(0, 1, 0), (0, 2, 1), (1, 3, 2), (2, 3, 2), (3, 1, 0), (1, 1, 1), (3, 2, 1)], [0, 1, 0, 1])
GRAMS = dict(join=(JOIN_GRAM, SPW2), pairs=(PAIR_GRAM, None))


def same_row(got, want, what):
    """(rec, words, level_cost) of one emitted row against the reference's, byte for byte"""
    for name, g, w in zip(("rec", "words", "level_cost"), got, want):
        g, w = np.ascontiguousarray(g).view(np.uint32).reshape(-1), np.ascontiguousarray(w).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{what}: {name} differs from word {at} on: got {g.tolist()} want {w.tolist()}")


def cut(N, sizes):
    """the sizes in order, the last one repeated, until N frames are used up"""
    out, i = [], 0
    while sum(out) < N:
        out.append(min(sizes[min(i, len(sizes) - 1)], N - sum(out)))
        i += 1
    return out


def per_channel(lists):
    """one chunking per channel -> per push the counts (0 once a channel is done)"""
    n = max(len(x) for x in lists)
    return [[x[i] if i < len(x) else 0 for x in lists] for i in range(n)]


def chunkings():
    n = [int(N) for N in chain_ref.planted()["inf"]]
    return {"one frame": per_channel([[1] * N for N in n]), "sevens": per_channel([cut(N, [7]) for N in n]),
            "64, then the rest": per_channel([cut(N, [64, MAXF]) for N in n]), "whole": per_channel([[N] for N in n])}


@functools.lru_cache(maxsize=None)
def recordings(which, kind, skip, word_cost=0):
    """one history per planted row under grammar `which` with drawn costs (kind "drawn") or none (kind "zero")"""
    fx = chain_ref.planted()
    gram, wos = GRAMS[which]
    g = ref.drawn_costs(gram) if kind == "drawn" else ref.with_costs(gram)
    return [ref.Recording(g, fx["im"][r, :int(fx["inf"][r])], fx["tm"], fx["tf"], None, W, skip, word_cost, wos) for r in range(N_CH)]


def make_engine(which, **kw):
    fx = chain_ref.planted()
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    if GRAMS[which][1] is not None:
        eng.set_word_map(np.array(GRAMS[which][1]))
    return eng


def rows_of(out):
    """the emitted rows of a push as numpy (rec [n], words [n, W], level_cost [n, W])"""
    rec, words, lc = out["rec"], out["words"], out["level_cost"]
    if not isinstance(rec, np.ndarray):
        torch.cuda.synchronize()
        n = out["n_rows"]
        nw = words.shape[1]
        rec = rec.cpu().numpy().view(ref.CHAIN_REC_DTYPE).reshape(n)
        words = words.cpu().numpy().view(ref.CHAIN_WORD_DTYPE).reshape(n, nw)
        lc = lc.cpu().numpy().view(np.uint32).reshape(n, nw)
    return rec, words, lc


class Follower:
    """every push against what the counts alone say (n_rows, the row labels and their order) and every emitted row against the
    reference at that channel's N"""

    def __init__(self, ses, recs, n_exact, what):
        self.ses, self.recs, self.n_exact, self.what = ses, recs, n_exact, what
        self.count = [0] * len(recs)
        self.last = [None] * len(recs)

    def take(self, out, new, emit=None):
        emit = [n > 0 for n in new] if emit is None else emit
        self.count = [a + int(b) for a, b in zip(self.count, new)]
        exp = [(c, self.count[c]) for c in range(len(new)) if emit[c]]
        assert out["n_rows"] == len(exp) and [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == exp, (out["rows"], exp)
        assert self.ses.frames.tolist() == self.count
        rec, words, lc = rows_of(out)
        for r, (c, N) in enumerate(exp):
            self.last[c] = (rec[r], words[r], lc[r])
            same_row(self.last[c], self.recs[c].row(N, self.n_exact), f"{self.what}, channel {c} at {N} frames")


def dev_chunk(d_f, at, cnt):
    """the counts' frames of every channel from `at` on, poison past n[c]"""
    chunk = torch.full((len(cnt), max(max(cnt), 1), 12), 0x7FFF, dtype=torch.int16, device="cuda:0")
    for c in range(len(cnt)):
        chunk[c, :cnt[c]] = d_f[c, at[c]:at[c] + cnt[c]]
    return chunk


def feed(ses, fol, schedule, form="dev"):
    fx = chain_ref.planted()
    d_f = torch.from_numpy(np.array(fx["im"])).cuda()
    at = [0] * N_CH
    for cnt in schedule:
        if form == "dev":
            out = ses.push_dev(dev_chunk(d_f, at, cnt), np.array(cnt, np.uint32))
        else:
            chunk = np.full((N_CH, max(max(cnt), 1), 12), 0x7FFF, np.int16)
            for c in range(N_CH):
                chunk[c, :cnt[c]] = fx["im"][c, at[c]:at[c] + cnt[c]]
            out = ses.push(chunk, np.array(cnt, np.uint32))
        fol.take(out, cnt)
        at = [a + b for a, b in zip(at, cnt)]
    assert at == [int(N) for N in fx["inf"]]


# ---- 14a: chunking invariance --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("skip,word_cost", [(SKIP, 0), (None, 5000)])
@pytest.mark.parametrize("which", list(GRAMS))
def test_every_chunking_gives_the_weighted_parse_of_the_prefix(which, skip, word_cost):
    fx = chain_ref.planted()
    gram_t = GRAMS[which][0]
    g = ref.drawn_costs(gram_t)
    eng = make_engine(which)
    gram, plain = eng.grammar(*g), eng.grammar(*gram_t)
    recs = recordings(which, "drawn", skip, word_cost)
    for mw, utt in ((W, MAXF), (1, 1), (16, 16383)):  # the geometry is the network's: the costs move no figure
        assert engine.grammar_live_geometry(gram, mw, utt, min(utt, 64)) == engine.grammar_live_geometry(plain, mw, utt, min(utt, 64))
    for n_exact in (0, 3):
        whole = eng.decode_grammar(gram, np.array(fx["im"]), fx["inf"], W, n_exact, skip, word_cost)
        for name, sched in chunkings().items():
            what = f"{which}, skip {skip}, word_cost {word_cost}, n_words {n_exact}, chunking '{name}'"
            ses = eng.decode_grammar_live(gram, N_CH, max(max(s) for s in sched), MAXF, W, n_exact, skip, word_cost)
            fol = Follower(ses, recs, n_exact, what)
            feed(ses, fol, sched, "host" if name == "sevens" else "dev")
            for c in range(N_CH):
                same_row(fol.last[c], (whole[0][c], whole[1][c], whole[2][c]), what + f": final row of channel {c} against decode_grammar")
            if name == "sevens":  # sr_gram_live_end: the parse once more, and the channels fresh
                out = ses.end(list(range(N_CH)))
                assert out["n_rows"] == N_CH and [int(r["frames"]) for r in out["rows"]] == [int(N) for N in fx["inf"]]
                for c in range(N_CH):
                    same_row((out["rec"][c], out["words"][c], out["level_cost"][c]), recs[c].row(int(fx["inf"][c]), n_exact), what + f": end of channel {c}")
                assert ses.frames.tolist() == [0] * N_CH
            ses.close()
    if skip is not None:  # the costs are looked at: rows differ from the unweighted session's
        zero = recordings(which, "zero", skip, word_cost)
        assert sum(recs[c].row(int(fx["inf"][c]))[1].tobytes() != zero[c].row(int(fx["inf"][c]))[1].tobytes() for c in range(N_CH)) >= 2
    gram.close()
    plain.close()
    eng.close()


# ---- 14b: the grammar switched between recordings, and the zero-cost twin ------------------------------------------------------
@pytest.mark.gpu
def test_set_grammar_switches_between_unweighted_and_weighted_and_zero_costs_are_the_unweighted_bytes():
    fx = chain_ref.planted()
    which = "join"
    gram_t = GRAMS[which][0]
    g = ref.drawn_costs(gram_t)
    eng = make_engine(which)
    plain, weighted = eng.grammar(*gram_t), eng.grammar(*g)
    zeros = eng.grammar(*gram_t, arc_cost=[0] * len(gram_t[1]), final_cost=[0] * gram_t[0])
    sched = per_channel([cut(int(N), [5, 64, 1, 9]) for N in fx["inf"]])
    ses = eng.decode_grammar_live(plain, N_CH, 64, MAXF, W, 0, SKIP)
    twin = eng.decode_grammar_live(zeros, N_CH, 64, MAXF, W, 0, SKIP)
    d_f = torch.from_numpy(np.array(fx["im"])).cuda()
    for turn, (gr, kind) in enumerate(((plain, "zero"), (weighted, "drawn"), (plain, "zero"), (weighted, "drawn"))):
        if turn:
            ses.set_grammar(gr)
        fol = Follower(ses, recordings(which, kind, SKIP), 0, f"recording {turn} under the {kind} costs")
        if kind == "zero":  # the same pushes into the session of the zero-cost weighted grammar: the same bytes
            at = [0] * N_CH
            for cnt in sched:
                chunk = dev_chunk(d_f, at, cnt)
                a, b = ses.push_dev(chunk, np.array(cnt, np.uint32)), twin.push_dev(chunk, np.array(cnt, np.uint32))
                fol.take(a, cnt)
                assert a["n_rows"] == b["n_rows"] and a["rows"].tobytes() == b["rows"].tobytes()
                for x, y in zip(rows_of(a), rows_of(b)):
                    assert x.tobytes() == y.tobytes(), (turn, cnt)
                at = [p + q for p, q in zip(at, cnt)]
            ea, eb = ses.end(list(range(N_CH))), twin.end(list(range(N_CH)))
            for key in ("rec", "words", "level_cost", "rows"):
                assert ea[key].tobytes() == eb[key].tobytes(), key
        else:
            feed(ses, fol, sched)
            out = ses.end(list(range(N_CH)))
            for c in range(N_CH):
                same_row((out["rec"][c], out["words"][c], out["level_cost"][c]), fol.recs[c].row(int(fx["inf"][c])), f"turn {turn}: end of channel {c}")
        assert ses.frames.tolist() == [0] * N_CH
    ses.close()
    twin.close()
    for x in (plain, weighted, zeros):
        x.close()
    eng.close()


# ---- 14c: a PCM session ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_pcm_session_gives_the_weighted_parse_of_the_frames_so_far():
    rng = np.random.default_rng(800)
    R_MAXF, NW, skip = 119, 4, 3000
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
    # long words lead into state 1 or 2, anything may follow into the final state 3, short words stay there
    gram_t = (4, [(0, 1, 2), (0, 1, 5), (0, 2, 4), (0, 2, 3)] + [(s, 3, w) for s in (1, 2, 3) for w in (0, 1, 2, 4, 5)], [0, 0, 0, 1])
    g = ref.drawn_costs(gram_t)
    gram = eng.grammar(*g)
    whole = eng.decode_grammar_pcm(gram, X, [1, 1], [R, R], mid, NW, 0, skip, 0)
    assert np.all(whole["rec"]["status"] == ref.CH_OK)
    recs = [ref.Recording(g, mf[c, :R_MAXF], tm, tf, valid, NW, skip, 0) for c in range(2)]
    ses = eng.decode_grammar_live(gram, 2, 400, R_MAXF, NW, 0, skip, 0, mid)
    fol = Follower(ses, recs, 0, "pcm")
    got = [0, 0]
    for cnt in per_channel([cut(R, [HOP - 1, 1, FRAME_LEN, 400, 399, 237]), cut(R, [161, 80])]):
        S = (max(max(cnt), 1) + 7) // 8 * 8
        chunk = np.full((2, S), 4095, np.uint16)  # poison past n[c]
        for c in range(2):
            chunk[c, :cnt[c]] = X[c, got[c]:got[c] + cnt[c]]
        now = [a + v for a, v in zip(got, cnt)]
        new = [pcm_frames(a, FRAME_LEN, HOP) - pcm_frames(b, FRAME_LEN, HOP) for a, b in zip(now, got)]
        out = ses.push_pcm_dev(torch.from_numpy(chunk.view(np.int16)).cuda(), np.array(cnt, np.uint32))
        fol.take(out, new, [v > 0 for v in cnt])  # a row for every channel that got samples, new frame or not
        got = now
    assert got == [R, R] and fol.count == [R_MAXF, R_MAXF]
    for c in range(2):
        same_row(fol.last[c], (whole["rec"][c], whole["words"][c], whole["level_cost"][c]), f"channel {c} against decode_grammar_pcm")
    ses.close()
    gram.close()
    eng.close()


# ---- 15: a stale weighted grammar ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_stale_weighted_grammar_refuses_pushes_writes_nothing_and_is_replaced():
    fx = chain_ref.planted()
    which = "pairs"
    g = ref.drawn_costs(GRAMS[which][0])
    eng = make_engine(which)
    gram = eng.grammar(*g)
    d_f = torch.from_numpy(np.array(fx["im"])).cuda()
    ses = eng.decode_grammar_live(gram, N_CH, 64, MAXF, W, 0, SKIP)
    fol = Follower(ses, recordings(which, "drawn", SKIP), 0, "before")
    cnt = [min(int(N), 9 + c) for c, N in enumerate(fx["inf"])]
    fol.take(ses.push_dev(dev_chunk(d_f, [0] * N_CH, cnt), np.array(cnt, np.uint32)), cnt)
    eng.set_templates_dense(fx["tm"], fx["tf"])  # the same rows, but a new store
    L, sid = eng.L, torch.cuda.current_stream().cuda_stream
    g_r = guarded_out((N_CH,), ref.CHAIN_REC_DTYPE, 0xA5, 4096, "cuda:0", "rec")
    g_w = guarded_out((N_CH, W), ref.CHAIN_WORD_DTYPE, 0xA5, 4096, "cuda:0", "words")
    g_l = guarded_out((N_CH, W), np.uint32, 0xA5, 4096, "cuda:0", "level_cost")
    rows, n_rows = np.full(N_CH, 0x5A5A5A5A, np.uint32).repeat(2).view(CHAIN_LIVE_ROW_DTYPE), U32(0xDEAD)
    chunk = dev_chunk(d_f, cnt, [1] * N_CH)
    rc = L.sr_gram_live_push_dev(ses.l, P(chunk.data_ptr()), U64(12), engine._vp(np.ones(N_CH, np.uint32)), U32(0), U32(N_CH), P(g_r.ptr), P(g_w.ptr),
                                 P(g_l.ptr), engine._vp(rows), C.byref(n_rows), P(sid))
    torch.cuda.synchronize()
    assert rc == BAD_ARG and b"template store" in L.sr_last_error()
    assert n_rows.value == 0xDEAD and np.all(rows.view(np.uint32) == 0x5A5A5A5A) and ses.frames.tolist() == cnt
    for x in (g_r, g_w, g_l):
        x.check_untouched()
    l = P(0x5A5A5A5A)  # nor does a session open on it
    assert L.sr_gram_live_open(eng.h, gram.g, U32(1), U32(8), U32(MAXF), U32(W), U32(0), U32(SKIP), U32(0), None, C.byref(l)) == BAD_ARG
    assert l.value in (0x5A5A5A5A, None)
    fresh = eng.grammar(*g)
    assert L.sr_gram_live_set_grammar(ses.l, fresh.g) == BAD_ARG and b"holds a recording" in L.sr_last_error()
    out = ses.end(list(range(N_CH)))  # dropped: whole SR_CH_NONE rows, frames 0
    assert out["n_rows"] == N_CH and np.all(out["rec"]["status"] == ref.CH_NONE) and np.all(out["rec"]["cost"] == DIS_ERR)
    assert np.all(out["words"].view(np.uint32) == 0xFFFFFFFF) and np.all(out["level_cost"] == DIS_ERR) and ses.frames.tolist() == [0] * N_CH
    assert L.sr_gram_live_set_grammar(ses.l, gram.g) == BAD_ARG  # the stale grammar itself is no replacement
    ses.set_grammar(fresh)
    fol = Follower(ses, recordings(which, "drawn", SKIP), 0, "after the replacement")
    feed(ses, fol, per_channel([cut(int(N), [64, MAXF]) for N in fx["inf"]]))
    ses.close()
    for x in (gram, fresh):
        x.close()
    eng.close()
