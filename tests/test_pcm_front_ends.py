"""Every PCM entry point of the decoders under every front end (fixtures: tests/pcm_cases.py).

The front ends themselves are covered elsewhere; what had only ever run on the reference's 160 / 80 framing is the code that
feeds SAMPLES into the decoders: the five batch PCM forms (sr_spot_batch, sr_decode_words_batch, sr_decode_grammar_batch,
sr_decode_onepass_batch, sr_decode_onepass_grammar_batch) and the PCM sessions of the four feature-taking live sessions, which
share one front end (csrc/sr_live_pcm.h, the stage and keep kernels, live_pcm_frames, LiveCore).  A PCM session stages rows whose
segment starts at sample 1, so on the extension front end its frame kernel only ever takes the plain-load branch for a segment
that starts below sample 2; and kept samples, stage strides and drop = frames * hop had met one geometry.

Seven front ends: the reference's as the control, the 16 kHz extension, the generic one at frames of 240, 256, 320, 400 and 512
samples.  Expected features come from the CPU oracle, expected records from the restatements on those features; every comparison
is byte for byte.  The CPU tests hold the fixtures to the conditions that keep the GPU tests from being vacuous.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_live_ref
import chain_ref
import onepass_live_ref
import pcm_cases as pc
import spot_live_ref
import spot_ref
import test_spot_live as t_spot_live
from guarded import CANARIES, guarded_out
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import ST_OK, ST_SEG_OOB, Engine

BAD_CONFIG, BAD_ARG = 2, 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
KINDS = ("spot", "level", "gram", "wgram", "onepass")  # the session kinds: the spotter, the level decoder under no / an unweighted / a weighted grammar, one pass
REC, WORD, ROW = chain_ref.CHAIN_REC_DTYPE, chain_ref.CHAIN_WORD_DTYPE, chain_live_ref.CHAIN_LIVE_ROW_DTYPE
OP_UTT = 3 * pc.MAXF + 10  # utt_frames of the one-pass sessions: the long recording fits


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    g, w = got.view(np.uint8).reshape(-1), want.view(np.uint8).reshape(-1)
    bad = np.nonzero(g != w)[0]
    if len(bad):
        size = want.dtype.itemsize
        at = int(bad[0]) // size
        raise AssertionError(f"{what}: {len(np.unique(bad // size))} of {want.size} elements differ, first at {np.unravel_index(at, want.shape)}: "
                             f"got {got.reshape(-1)[at]} want {want.reshape(-1)[at]}")


# ---- CPU: the fixtures meet the conditions of the GPU tests (on the references alone) -----------------------------------------------
@pytest.mark.parametrize("name", pc.NAMES)
def test_fixture_conditions(name):
    fx = pc.case(name)
    fl, hop = fx["frame_len"], fx["hop"]
    kw = fx["ekw"]
    assert (fl, hop) == (kw.get("fs", 8000) // 1000 * kw.get("frame_time_ms", 20), fl // 2) and kw.get("n_coef", 12) == 12
    assert 0 < fx["r"] < hop and fx["R1"] == 1 + 99 * hop + fl + fx["r"] and fx["R3"] == 3 * fx["R1"] and fx["X"].shape == (3, fx["R3"])
    assert len(set(fx["mid"].tolist())) == 3 and fx["chunk_max"] == 2 * fl + hop
    assert len(fx["tf"]) == 6 and 12 <= fx["tf"].min() and fx["tf"].max() <= 40 and fx["valid"].tolist().count(0) == 1
    assert sorted(np.unique(fx["wos"], return_counts=True)[1].tolist())[-1] == 2 and fx["skip"] > 0
    # the spotter finds the planted pieces at distance 0, where they were cut
    hits = pc.want_spot(name)
    found = 0
    for k, (c, at, rows) in enumerate(pc.PIECES):
        h = hits[c, (at + rows - 1) // pc.WIN, k]
        if fx["valid"][k]:
            assert (h["dis"], h["start"], h["end"]) == (0, at, at + rows - 1), (k, h)
            found += 1
        else:
            assert np.all(hits[:, :, k]["dis"] == spot_ref.DIS_ERR)
    assert found >= 2 and np.all(hits[3]["dis"] == spot_ref.DIS_ERR)
    # the decoders give a parse of at least two words on every channel, and none for the row without frames
    for what, want in (("chain", pc.want_chain(name)), ("onepass", pc.want_onepass(name))):
        assert np.all(want[0]["status"][:3] == chain_ref.CH_OK) and want[0]["n_words"][:3].min() >= 2, (what, want[0])
        assert want[0]["status"][3] == chain_ref.CH_NONE
    # every grammar accepts every channel
    grams = [pc.want_gram(name, "anchor"), pc.want_gram(name, "seq"), pc.want_wgram(name), pc.want_opgram(name, "repeat"), pc.want_opgram(name, "bigram")]
    for want in grams:
        assert np.all(want[0]["status"][:3] == chain_ref.CH_OK) and want[0]["status"][3] == chain_ref.CH_NONE, want[0]
    assert any(fx["bigram"][3]) and any(fx["bigram"][4])                                  # nonzero arc and final costs
    assert any(s == t for s, t, _ in fx["repeat"][1])                                     # a loop
    assert b"".join(a.tobytes() for a in grams[2]) != b"".join(a.tobytes() for a in grams[0])  # the costs change a parse
    # the schedules
    assert fx["block"] == int(fx["tf"][fx["valid"] != 0].min()) // 2 + 1
    for which, sched in pc.schedules(name).items():
        R = fx["R3"] if which.startswith("long") else fx["R1"]
        assert [sum(cnt[c] for cnt in sched) for c in range(3)] == [R] * 3 and max(max(cnt) for cnt in sched) == fx["chunk_max"]
        assert len({tuple(cnt[c] for cnt in sched) for c in range(3)}) == 3           # the channels differ
        sizes = {n for cnt in sched for n in cnt}
        assert {hop - 1, hop, hop + 1, fl, fl + 1, fx["chunk_max"], 0} <= sizes, (which, sorted(sizes))
        assert pc.schedule_facts(sched, fl, hop, pc.WIN, fx["block"]) == (True, True, True, True), which
    dev = pc.schedules(name)["dev"]
    assert all(cnt[0] == 1 for cnt in dev[:fl + 2])                                       # one sample at a time across the first frame
    assert pc.schedules(name)["dev"] != pc.schedules(name)["host"]
    # the long recording passes max_frames, its pieces are the short recording's features where they overlap
    long = pc.long_feats(name)
    assert long.shape[1] == pc.pcm_frames(fx["R3"], fl, hop) > 2 * pc.MAXF and long.shape[1] <= OP_UTT
    assert np.array_equal(long[:, :pc.N_FR], fx["feat"])


def test_the_frame_count_of_every_prefix_is_the_same_in_every_restatement():
    for name in pc.NAMES:
        fx = pc.case(name)
        fl, hop, R1 = fx["frame_len"], fx["hop"], fx["R1"]
        brute = np.zeros(R1 + 1, np.int64)  # brute[s]: the frames whose last sample is among the first s
        for j in range(pc.N_FR + 1):
            brute[min(1 + j * hop + fl, R1 + 1):] += 1
        assert brute[R1] == pc.N_FR and brute[fl] == 0 and brute[fl + 1] == 1
        for s in (0, 1, fl, fl + 1, fl + hop, fl + hop + 1, R1):
            assert pc.pcm_frames(s, fl, hop) == brute[s]
        for s in range(R1 + 1):
            n = spot_live_ref.pcm_frames(s, fl, hop)
            assert n == chain_live_ref.pcm_frames(s, fl, hop) == onepass_live_ref.pcm_frames(s, fl, hop) == brute[s], (name, s)


# ---- GPU: helpers ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def engine_of(name):
    """one engine per front end for the whole module, its store and word map set once (a session is bound to its store)"""
    fx = pc.case(name)
    eng = Engine(max_frames=pc.MAXF, device=0, **fx["ekw"])
    eng.set_templates_dense(*pc.store(fx))
    eng.set_word_map(fx["wos"])
    return eng


def chunk_rows(X, got, cnt):
    """uint16 [C, S]: cnt[c] samples of channel c from got[c] on, poison behind them; S a multiple of 8"""
    S = (max(max(cnt), 1) + 7) // 8 * 8
    chunk = np.full((len(X), S), pc.POISON, np.uint16)
    for c in range(len(X)):
        chunk[c, :cnt[c]] = X[c, got[c]:got[c] + cnt[c]]
    return chunk


def to_device(chunk):
    return torch.from_numpy(chunk.view(np.int16)).cuda()


def open_session(kind, eng, fx, n_ch, chunk_max, utt, mid, gram=None):
    if kind == "spot":
        return eng.spot_live(n_ch, chunk_max, pc.WIN, mid)
    if kind == "level":
        return eng.decode_live(n_ch, chunk_max, utt, pc.MAX_WORDS, 0, fx["skip"], pc.WORD_COST, mid)
    if kind in ("gram", "wgram"):
        return eng.decode_grammar_live(gram, n_ch, chunk_max, utt, pc.MAX_WORDS, 0, fx["skip"], pc.WORD_COST, mid)
    return eng.decode_onepass_live(n_ch, chunk_max, utt, pc.OP_WORDS, False, fx["skip"], pc.WORD_COST, mid)


def grammar_of(kind, eng, fx):
    return eng.grammar(*fx["grams"]["seq"]) if kind == "gram" else eng.grammar(*fx["bigram"]) if kind == "wgram" else None


def want_of(kind, name):
    return dict(level=pc.want_chain, gram=lambda n: pc.want_gram(n, "seq"), wgram=pc.want_wgram, onepass=pc.want_onepass)[kind](name)


def row_bytes(out, r, W):
    """row r of a decoder push or end call as bytes: rec | words | level costs (where the session has them)"""
    n = out["n_rows"]

    def host(t, dt, shape):
        return t if isinstance(t, np.ndarray) else t.cpu().numpy().view(dt).reshape(shape)

    got = [host(out["rec"], REC, (n,)), host(out["words"], WORD, (n, W))]
    if out.get("level_cost") is not None:
        got.append(host(out["level_cost"], np.uint32, (n, W)))
    return b"".join(np.ascontiguousarray(a[r]).tobytes() for a in got)


def run_decoder(ses, X, R, sched, fl, hop, W, want, what, dev):
    """pushes R samples per channel along the schedule; the labelled rows of every push are the host-side count's, and the row of
    each channel's last push and its row at end() are the batch reference's of the whole recording"""
    n_ch = len(X)
    got, last = [0] * n_ch, [None] * n_ch
    for cnt in sched:
        chunk = chunk_rows(X, got, cnt)
        got = [g + n for g, n in zip(got, cnt)]
        exp = [(c, spot_live_ref.pcm_frames(got[c], fl, hop)) for c in range(n_ch) if cnt[c]]  # a row for every channel that got samples
        out = ses.push_pcm_dev(to_device(chunk), np.array(cnt, np.uint32)) if dev else ses.push_pcm(chunk, np.array(cnt, np.uint32))
        assert out["n_rows"] == len(exp) and [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == exp, (what, out["rows"], exp)
        for r, (c, _) in enumerate(exp):
            last[c] = (out, r)
    assert got == [R] * n_ch
    frames = spot_live_ref.pcm_frames(R, fl, hop)
    assert ses.frames.tolist() == [frames] * n_ch
    torch.cuda.synchronize()
    end = ses.end(list(range(n_ch)))
    assert [(int(r["channel"]), int(r["frames"])) for r in end["rows"]] == [(c, frames) for c in range(n_ch)]
    for c in range(n_ch):
        exp = b"".join(np.ascontiguousarray(a[c]).tobytes() for a in want)
        assert row_bytes(*last[c], W) == exp, f"{what}: channel {c} after its last push"
        assert row_bytes(end, c, W) == exp, f"{what}: channel {c} at end"
    ses.close()


def run_spotter(ses, X, R, sched, fl, hop, want, what, dev):
    """the same for a spotting session: the rows announced before each push and the window labels of each push are the host-side
    count's, the windows of a channel those of the whole recording as one row"""
    n_ch = len(X)
    col, got = t_spot_live.Collector(ses, n_ch, pc.WIN), [0] * n_ch
    for cnt in sched:
        chunk = chunk_rows(X, got, cnt)
        now = [g + n for g, n in zip(got, cnt)]
        new = [spot_live_ref.pcm_frames(a, fl, hop) - spot_live_ref.pcm_frames(b, fl, hop) for a, b in zip(now, got)]
        assert ses.rows(np.array(cnt, np.uint32)) == len(spot_live_ref.push_windows(col.count, new, pc.WIN)), what
        out = ses.push_pcm_dev(to_device(chunk), np.array(cnt, np.uint32)) if dev else ses.push_pcm(chunk, np.array(cnt, np.uint32))
        col.take(out, new)
        got = now
    assert got == [R] * n_ch and col.count == [spot_live_ref.pcm_frames(R, fl, hop)] * n_ch
    col.end(list(range(n_ch)))
    ses.close()
    for c in range(n_ch):
        same(col.channel(c), want[c], f"{what}: channel {c}")


# ---- GPU 1: the batch PCM forms ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.NAMES)
def test_batch_pcm_forms(name):
    """segment [1, R1] of three channels and, as row 3, channel 0 from sample 0: SR_ST_SEG_OOB, no frames, a record without a
    parse or a hit and an all-zero feature row, as the reference front end's tests have it"""
    fx, eng = pc.case(name), engine_of(name)
    R1, skip, wc = fx["R1"], fx["skip"], pc.WORD_COST
    pcm = np.full((4, (R1 + 7) // 8 * 8), pc.POISON, np.uint16)
    pcm[:3, :R1], pcm[3, :R1] = fx["X"][:, :R1], fx["X"][0, :R1]
    seg = ([1, 1, 1, 0], [R1] * 4, list(fx["mid"]) + [int(fx["mid"][0])])

    def front_end(o, what):
        same(o["mfcc"], fx["im"], f"{what}: features against the oracle")
        assert o["frm_num"].tolist() == fx["inf"].tolist() and o["status"].tolist() == [ST_OK] * 3 + [ST_SEG_OOB], what
        assert not o["mfcc"][3].any()

    o = eng.spot_pcm(pcm, *seg, pc.WIN)
    front_end(o, "spot_pcm")
    assert o["hits"].shape == (4, 3, 6)
    same(o["hits"], pc.want_spot(name), "spot_pcm: hits")
    same(o["scores"], pc.want_spot(name)["dis"], "spot_pcm: scores")
    o = eng.decode_words_pcm(pcm, *seg, pc.MAX_WORDS, 0, skip, wc)
    front_end(o, "decode_words_pcm")
    for f, w in zip(("rec", "words", "level_cost"), pc.want_chain(name)):
        same(o[f], w, f"decode_words_pcm: {f}")
    for which, want in (("anchor", pc.want_gram(name, "anchor")), ("seq", pc.want_gram(name, "seq")), ("bigram", pc.want_wgram(name))):
        g = eng.grammar(*(fx["bigram"] if which == "bigram" else fx["grams"][which]))
        o = eng.decode_grammar_pcm(g, pcm, *seg, pc.MAX_WORDS, 0, skip, wc)
        front_end(o, f"decode_grammar_pcm, {which}")
        for f, w in zip(("rec", "words", "level_cost"), want):
            same(o[f], w, f"decode_grammar_pcm, {which}: {f}")
        g.close()
    o = eng.decode_onepass_pcm(pcm, *seg, pc.OP_WORDS, skip, wc)
    front_end(o, "decode_onepass_pcm")
    for f, w in zip(("rec", "words"), pc.want_onepass(name)):
        same(o[f], w, f"decode_onepass_pcm: {f}")
    for which in ("repeat", "bigram"):
        g = eng.grammar(*fx[which])
        o = eng.decode_onepass_grammar_pcm(g, pcm, *seg, pc.OP_WORDS, skip, wc)
        front_end(o, f"decode_onepass_grammar_pcm, {which}")
        for f, w in zip(("rec", "words"), pc.want_opgram(name, which)):
            same(o[f], w, f"decode_onepass_grammar_pcm, {which}: {f}")
        g.close()


# ---- GPU 2: the PCM sessions over R1 samples ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", pc.NAMES)
def test_pcm_sessions(name, kind):
    """the device form under one schedule per channel, the host form under another: the batch reference of the whole recording"""
    fx, eng = pc.case(name), engine_of(name)
    fl, hop, R1 = fx["frame_len"], fx["hop"], fx["R1"]
    X = fx["X"][:, :R1]
    gram = grammar_of(kind, eng, fx)
    for form, dev in (("dev", True), ("host", False)):
        sched, what = pc.schedules(name)[form], f"{name}, {kind} session, {form} form"
        ses = open_session(kind, eng, fx, 3, fx["chunk_max"], OP_UTT if kind == "onepass" else pc.MAXF, fx["mid"], gram)
        if kind == "spot":
            run_spotter(ses, X, R1, sched, fl, hop, pc.want_windows(name), what, dev)
        else:
            W = pc.OP_WORDS if kind == "onepass" else pc.MAX_WORDS
            run_decoder(ses, X, R1, sched, fl, hop, W, [a[:3] for a in want_of(kind, name)], what, dev)
    if kind == "spot":  # the session's windows are the batch spotter's of the whole recording
        for c in range(3):
            same(pc.want_windows(name)[c], pc.want_spot(name)[c, :-(-pc.N_FR // pc.WIN)], f"{name}: the references agree, channel {c}")
    if gram is not None:
        gram.close()


# ---- GPU 3: the PCM sessions over R3 samples, past max_frames ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("spot", "onepass"))
@pytest.mark.parametrize("name", pc.NAMES)
def test_pcm_sessions_on_the_long_recording(name, kind):
    """three times max_frames worth of samples: the keep buffer is used hundreds of times, rows start at every phase of the hop"""
    fx, eng = pc.case(name), engine_of(name)
    sched, what = pc.schedules(name)["long_" + kind], f"{name}, {kind} session, long recording"
    ses = open_session(kind, eng, fx, 3, fx["chunk_max"], OP_UTT, fx["mid"])
    if kind == "spot":
        run_spotter(ses, fx["X"], fx["R3"], sched, fx["frame_len"], fx["hop"], pc.want_windows(name, True), what, True)
    else:
        run_decoder(ses, fx["X"], fx["R3"], sched, fx["frame_len"], fx["hop"], pc.OP_WORDS, pc.want_onepass(name, True), what, True)


# ---- GPU 4: the refusals that depend on the framing -----------------------------------------------------------------------------
def raw_open(kind, eng, fx, gram, n_ch, chunk_max, utt, mid):
    """the session's open call itself -> (rc, handle)"""
    L, out, v = eng.L, C.c_void_p(0x5A5A), engine._vp
    tail = (U32(fx["skip"]), U32(pc.WORD_COST), v(mid), C.byref(out))
    if kind == "spot":
        rc = L.sr_spot_live_open(eng.h, U32(n_ch), U32(chunk_max), U32(pc.WIN), v(mid), C.byref(out))
    elif kind == "level":
        rc = L.sr_decode_live_open(eng.h, U32(n_ch), U32(chunk_max), U32(utt), U32(pc.MAX_WORDS), U32(0), *tail)
    elif kind in ("gram", "wgram"):
        rc = L.sr_gram_live_open(eng.h, gram.g, U32(n_ch), U32(chunk_max), U32(utt), U32(pc.MAX_WORDS), U32(0), *tail)
    else:
        rc = L.sr_onepass_live_open(eng.h, U32(n_ch), U32(chunk_max), U32(utt), U32(pc.OP_WORDS), U32(0), *tail)
    return rc, out.value


class RawPush:
    """a push call of any session kind with guarded outputs, on the device or on the host, and sentinels in what the host gets"""

    PREFIX = dict(spot="sr_spot_live_", level="sr_decode_live_", gram="sr_gram_live_", wgram="sr_gram_live_", onepass="sr_onepass_live_")

    def __init__(self, kind, eng, ses, canary):
        self.kind, self.eng, self.ses, self.canary = kind, eng, ses, canary

    def __call__(self, fn, data, stride, counts, max_rows=8):
        device = fn.endswith("_dev")
        where, K = "cuda:0" if device else None, self.eng.n_templates
        W = pc.OP_WORDS if self.kind == "onepass" else pc.MAX_WORDS
        if self.kind == "spot":
            outs = [guarded_out((max_rows, K), spot_ref.SPOT_DTYPE, self.canary, 4096, where, "hits"),
                    guarded_out((max_rows, K), np.uint32, self.canary, 4096, where, "scores")]
        else:
            outs = [guarded_out((max_rows,), REC, self.canary, 4096, where, "rec"), guarded_out((max_rows, W), WORD, self.canary, 4096, where, "words")]
            if self.kind != "onepass":
                outs.append(guarded_out((max_rows, W), np.uint32, self.canary, 4096, where, "level_cost"))
        labels, n_rows = np.full(2 * max_rows, 0x5A5A5A5A, np.uint32), U32(0xDEAD)
        args = [self.ses.l, P(data), U64(stride), engine._vp(np.array(counts, np.uint32)), U32(0), U32(max_rows)] + [P(g.ptr) for g in outs]
        args += [engine._vp(labels), C.byref(n_rows)] + ([P(torch.cuda.current_stream().cuda_stream)] if device else [])
        rc = getattr(self.eng.L, self.PREFIX[self.kind] + fn)(*args)
        torch.cuda.synchronize()
        assert n_rows.value == 0xDEAD and np.all(labels == 0x5A5A5A5A), (self.kind, fn, "the host outputs of a refused call")
        for g in outs:
            g.check_untouched()
        return rc, self.eng.L.sr_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
@pytest.mark.parametrize("name", pc.NAMES)
def test_refusals_that_depend_on_the_framing(name, canary):
    fx, eng = pc.case(name), engine_of(name)
    fl, hop, cm = fx["frame_len"], fx["hop"], fx["chunk_max"]
    one = fx["mid"][:1].copy()
    X = fx["X"]
    for kind in KINDS:
        gram = grammar_of(kind, eng, fx)
        # a push of chunk_max samples completes at most ceil(chunk_max / hop) frames: frame_cap = min(max_frames, utt_frames) of them at most
        utt = dict(spot=pc.MAXF, level=pc.MAXF, gram=50, wgram=pc.MAXF, onepass=OP_UTT)[kind]
        cap = min(utt, pc.MAXF)
        ses = open_session(kind, eng, fx, 1, cap * hop, utt, one, gram)
        ses.close()
        rc, handle = raw_open(kind, eng, fx, gram, 1, cap * hop + 1, utt, one)
        assert rc == BAD_ARG and not handle and b"could complete more than %d frames" % cap in eng.L.sr_last_error(), (kind, rc, eng.L.sr_last_error())
        # a valid open still works: a PCM session and a feature session of the same kind
        ses = open_session(kind, eng, fx, 3, cm, utt, fx["mid"], gram)
        feat = open_session(kind, eng, fx, 3, 5, utt, None, gram)
        push, push_f = RawPush(kind, eng, ses, canary), RawPush(kind, eng, feat, canary)
        d_chunk = to_device(np.full((3, cm + 24), pc.POISON, np.uint16))
        at, S = d_chunk.data_ptr(), cm + 24
        assert at % 16 == 0 and S % 8 == 0
        for off in (2, 8):  # a device chunk that is not 16-byte aligned
            rc, why = push("push_pcm_dev", at + off, S, [hop] * 3)
            assert rc == BAD_ARG and b"16-byte aligned" in why, (kind, off, rc, why)
        rc, why = push("push_pcm_dev", at, S - 4, [hop] * 3)            # a stride that is no multiple of 8
        assert rc == BAD_ARG and b"stride % 8" in why, (kind, rc, why)
        rc, why = push("push_pcm_dev", at, hop - 8, [hop, 1, 0])         # a count above pcm_stride
        assert rc == BAD_ARG and b"exceeds pcm_stride" in why, (kind, rc, why)
        # frames into a PCM session, samples into a feature session: both forms of both
        d_frames, h_frames, h_chunk = torch.zeros(3, 5, 12, dtype=torch.int16, device="cuda:0"), np.zeros((3, 5, 12), np.int16), np.zeros((3, S), np.uint16)
        for fn, data in (("push_dev", d_frames.data_ptr()), ("push", h_frames.ctypes.data)):
            rc, why = push(fn, data, 60, [1, 1, 1])
            assert rc == BAD_ARG and b"PCM session takes samples" in why, (kind, fn, rc, why)
        for fn, data in (("push_pcm_dev", at), ("push_pcm", h_chunk.ctypes.data)):
            rc, why = push_f(fn, data, S, [1, 1, 1])
            assert rc == BAD_ARG and b"feature session takes frames" in why, (kind, fn, rc, why)
        # nothing was taken in: the next push of chunk_max samples is the session's first, 1 + (chunk_max - 1 - frame_len) // hop frames
        out = ses.push_pcm_dev(to_device(chunk_rows(X, [0] * 3, [cm] * 3)))
        first = spot_live_ref.pcm_frames(cm, fl, hop)
        assert first == 3
        if kind == "spot":
            assert out["n_rows"] == 0
        else:
            assert [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(c, first) for c in range(3)]
        torch.cuda.synchronize()
        ses.close()
        feat.close()
        if gram is not None:
            gram.close()


# ---- GPU 5: a front end of 13 coefficients ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_13_coefficient_engine_is_refused_by_the_sessions_the_one_pass_grammar_decoder_the_aligner_and_the_gather():
    fx, eng = pc.case("reference"), engine_of("reference")
    e13 = Engine(max_frames=pc.MAXF, device=0, n_mel=26, n_coef=13)  # the generic front end: 13 coefficients
    L, v = e13.L, engine._vp
    gram = eng.grammar(*fx["grams"]["anchor"])  # no grammar compiles against e13 either; the configuration is what is refused first
    g = P(0x5A5A)
    arcs, fin = np.array([(0, 0, 0, 0)], engine.GRAM_ARC_DTYPE), np.ones(1, np.uint8)
    assert L.sr_grammar_create(e13.h, U32(1), v(arcs), U32(1), v(fin), C.byref(g)) == BAD_CONFIG and g.value == 0x5A5A
    mid = fx["mid"]
    for kind in KINDS:
        for m in (None, mid):
            rc, handle = raw_open(kind, e13, fx, gram, 3, 5 if m is None else fx["chunk_max"], pc.MAXF, m)
            assert rc == BAD_CONFIG and not handle and b"12-coefficient" in L.sr_last_error(), (kind, rc, L.sr_last_error())
    n, W, maxf = 2, 4, pc.MAXF
    im, inf = np.zeros((n, maxf, 13), np.int16), np.full(n, 40, np.uint32)
    d_im, d_inf = torch.from_numpy(im).cuda(), torch.from_numpy(inf.view(np.int32)).cuda()
    sid = P(torch.cuda.current_stream().cuda_stream)
    lab, cnt = np.zeros((n, W), np.uint32), np.ones(n, np.uint32)
    words = np.empty((n, W), WORD)
    words[...] = chain_ref.NO_WORD_ROW
    words[:, 0]["start"], words[:, 0]["end"] = 2, 9
    d_words = torch.from_numpy(words.view(np.int32).reshape(n, W, 8)).cuda()
    dst = np.arange(n * W, dtype=np.uint32)
    for canary in CANARIES:
        for where in ("cuda:0", None):
            a, b, w = (P(d_im.data_ptr()), P(d_inf.data_ptr()), P(d_words.data_ptr())) if where else (v(im), v(inf), v(words))
            sfx, tail = ("_dev", (sid,)) if where else ("", ())
            rec, wrd = guarded_out((n,), REC, canary, 4096, where, "rec"), guarded_out((n, W), WORD, canary, 4096, where, "words")
            ex = guarded_out((n * W, 8, 12), np.int16, canary, 4096, where, "ex")
            exf = guarded_out((n * W,), np.uint32, canary, 4096, where, "ex_frames")
            calls = dict(
                onepass_grammar=lambda: getattr(L, "sr_decode_onepass_grammar_dp" + sfx)(e13.h, gram.g, a, b, U32(1), U32(n), U32(0), U32(W), U32(fx["skip"]),
                                                                                         U32(0), P(rec.ptr), P(wrd.ptr), *tail),
                align=lambda: getattr(L, "sr_align_transcripts_dp" + sfx)(e13.h, a, b, U32(1), U32(n), v(lab), v(cnt), U32(W), U32(fx["skip"]), U32(0),
                                                                          P(rec.ptr), P(wrd.ptr), *tail),
                gather=lambda: getattr(L, "sr_gather_word_spans" + sfx)(e13.h, a, b, U32(1), U32(n), w, U32(W), v(dst), U32(n * W), U32(8), P(ex.ptr),
                                                                        P(exf.ptr), *tail))
            for what, call in calls.items():
                rc = call()
                torch.cuda.synchronize()
                assert rc == BAD_CONFIG and b"12-coefficient" in L.sr_last_error(), (what, where, rc, L.sr_last_error())
            for buf in (rec, wrd, ex, exf):
                buf.check_untouched()
    gram.close()
    e13.close()
