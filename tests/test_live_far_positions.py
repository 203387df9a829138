"""Live sessions far into a recording: positions past 2^31 / 2^32 samples (sr_live), columns up to the 0xFFFF0000-frame cap
(sr_spot_live), and the documented deviation of a live segment of 65 536 frames or more.

Such positions cannot be pushed (2^32 samples are 8 GB a channel).  Two development hooks of the testing library let a FRESH
channel start at an arbitrary origin instead: "live_origin" (samples) and "spot_live_origin" (frames).  Both sessions are
shift-invariant, so the expected bytes are those of the EXISTING references on the pushed data alone with positions shifted in
Python-int / int64 arithmetic:
  sr_live       Engine.recognize_stream on everything pushed (what tests/test_live_session.py compares with), start and end
                + origin, an end of -1 kept, everything else unchanged;
  sr_spot_live  tests/spot_live_ref.py's window reduction with `origin`, held to tests/spot_ref.py by the CPU tests below.
No tolerances anywhere.  What must hold of the inputs -- a recognised word straddles each boundary, the partial first window
has a hit, the 65 536 + 50-frame segment exists -- is asserted on the CPU oracle / the numpy reference before any GPU call.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import oracle_lib as ol
import spot_live_ref as live
import spot_ref as ref
from guarded import guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import (ATAP_DTYPE, DIS_ERR, LIVE_SEG_DTYPE, NBEST_DTYPE, RESULT_DTYPE, ST_MFCC_FAIL, ST_OK,
                                                 Engine, SrError)
from test_live_session import KEYS, LEAD, Feeder, check_all, one_shot, spaced_words
from test_spot_live import cut, per_channel, same
from test_stream_recognition import EXT, oracle_segments, random_templates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
HOOKS = ("live_origin", "spot_live_origin")
BAD_ARG = 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
MID = 2048
ATAP = (MID, 100, 4, 4000)  # thresholds handed in: band +-100 around 2048, z_thl 4, s_thl 4000
CAP = 0xFFFF0000


@pytest.fixture(autouse=True)
def _origins_back_to_zero():
    yield
    for h in HOOKS:
        engine.dev_hook(h, 0)


# ---- CPU: the hooks' surface -----------------------------------------------------------------------------------------------------
def test_header_lists_the_origin_hooks_and_the_product_library_has_none():
    text = open(HEADER).read()
    for hook in HOOKS:
        assert '"%s"' % hook in text[text.index("Development and test hooks"):], hook  # listed with the others
        engine.dev_hook(hook, 0)  # the testing library knows the hook ...
        for v in (0, 80, 1 << 33):  # ... the product library refuses the name, whatever the value
            assert engine.load_library().sr_dev_hook(hook.encode(), C.c_int64(v)) == BAD_ARG, (hook, v)


# ---- CPU: the spotter's reference with an origin, held to spot_ref ---------------------------------------------------------------
def _small_store(rng):
    tm, tf = rng.integers(-2, 3, (3, 11, 12)).astype(np.int16), np.array([10, 3, 1], np.uint32)
    return tm, tf, np.array([1, 0, 1], np.uint8)


def _shifted(rec, by):
    out = np.array(rec)
    hit = out["dis"] != DIS_ERR
    for f in ("start", "end"):
        out[f] = np.where(hit, out[f].astype(np.int64) + by, out[f]).astype(np.uint32)
    return out


def test_reference_origin_on_a_window_edge_is_the_one_shot_reduction_shifted():
    rng = np.random.default_rng(41)
    tm, tf, valid = _small_store(rng)
    N = 57
    feat = rng.integers(-2, 3, (N, 12)).astype(np.int16)
    for win in (1, 8, 16, 57, 100):
        old = ref.spot_hits(feat[None], [N], tm, tf, valid, N, win)[0][:-(-N // win)]  # windows 0 .. of the frames alone
        assert np.any(old["dis"] != DIS_ERR) and np.all(old[:, 1]["dis"] == DIS_ERR)
        for w0 in (0, 1, 3, (1 << 31) // win, (CAP - N) // win):
            origin = w0 * win
            got = live.window_records(feat, tm, tf, valid, win, origin)  # row i is window w0 + i
            same(got, _shifted(old, origin), (win, w0))
            assert live.n_window_rows(N, win, origin) == len(old)
            assert live.push_windows([origin], [N], win) == [(0, w0 + i) for i in range(N // win)]
            for k in (0, 2):  # the packed form likewise
                cost, start = ref.dp_end_row(ref.local_dis(feat, tm[k, :tf[k]]))
                end = np.where(cost >= 0, (cost.astype(np.uint64) << np.uint64(32)) | start.astype(np.uint64), live.INF64)
                same(live.end_records(end, int(tf[k]), win, origin), np.ascontiguousarray(got[:, k]), (win, w0, k))


def _brute_force_suffix(feat, tm, tf, valid, win, origin):
    """window records of a recording of origin + N frames whose first `origin` frames are unreachable, from spot_ref alone:
    dp_end_row on the suffix, its results placed at their absolute end frames, every window of the long recording reduced"""
    N, K = len(feat), len(tm)
    out = np.empty((-(-(origin + N) // win), K), ref.SPOT_DTYPE)
    out[...] = ref.NO_HIT
    for k in range(K):
        M = int(tf[k]) if valid[k] else 0
        if not M:
            continue
        c, s = ref.dp_end_row(ref.local_dis(feat, tm[k, :M]))
        cost = np.concatenate([np.full(origin, -1, np.int64), c])
        start = np.concatenate([np.zeros(origin, np.int64), s + origin])
        q = ref.end_scores(cost, start, M)
        for w in range(len(out)):
            out[w, k] = ref.window_hit(cost, start, q, w * win, (w + 1) * win)
    return out


def test_reference_origin_inside_a_window_is_a_longer_recording_with_an_unreachable_head():
    rng = np.random.default_rng(42)
    tm, tf, valid = _small_store(rng)
    feat = rng.integers(-2, 3, (57, 12)).astype(np.int16)
    partial_with_hit = 0
    for origin, win in ((37, 16), (5, 8), (15, 16), (49, 16), (37, 1), (37, 100), (1, 57), (64, 16)):
        whole = _brute_force_suffix(feat, tm, tf, valid, win, origin)
        w0 = origin // win
        assert np.all(whole[:w0]["dis"] == DIS_ERR)  # nothing ends before the origin
        got = live.window_records(feat, tm, tf, valid, win, origin)
        same(got, whole[w0:], (origin, win))
        if origin % win:
            partial_with_hit += int(got[0, 2]["dis"] != DIS_ERR and got[0, 2]["end"] < (w0 + 1) * win)
    assert partial_with_hit >= 5  # the partial first window is not empty
    assert len(live.window_records(feat[:0], tm, tf, valid, 16, 37)) == 1 and len(live.window_records(feat[:0], tm, tf, valid, 16, 32)) == 0


# ---- sr_live: recordings whose words straddle 2^31, 2^32 samples and frame 2^32 (CPU) ---------------------------------------------
# name -> engine keywords, oracle keywords, length scale
FRONT = {"reference": ({}, {}, 1), "extension": (EXT, dict(fs=16000, nfft=512, n_mel=40), 2)}
MAXF = 119
QUIET = 4000  # samples of silence (exactly mid: in band) at the head of every recording, x the length scale


def frames_in(s, e, fl, hop):
    return ((e - s) - fl) // hop + 1


@functools.lru_cache(maxsize=None)
def far_case(name):
    """three recordings of about 60 000 samples (x the scale), one per channel, with the origin of each: channel 0 has a
    recognisable word across sample 2^31, channel 1 across 2^32, channel 2 across frame 2^32 (sample 2^32 * hop); each ends
    inside a word.  Built and checked with the CPU oracle's VAD alone."""
    _, okw, sc = FRONT[name]
    orc = ol.Oracle(max_frames=MAXF, max_seg=1 << 16, **okw)
    hop, fl = orc.hop, orc.frame_len
    at = ol.Atap(*ATAP)
    bank = synth.word_bank(10)
    to_hop = lambda v: (v + hop // 2) // hop * hop  # noqa: E731
    bounds = (1 << 31, 1 << 32, (1 << 32) * hop)
    origins = (to_hop((1 << 31) - 20000), to_hop((1 << 32) - 20000), ((1 << 32) - 300) * hop)
    recs, straddlers = [], []
    for c, (B, S0) in enumerate(zip(bounds, origins)):
        assert S0 % hop == 0
        rel = B - S0  # the boundary, counted from the first pushed sample
        y = spaced_words(70 + c, bank, 60000 * sc, gap=2400 * sc, scale=sc, lo=50, hi=100)[2400:]
        base = np.concatenate([np.full(QUIET * sc, MID, np.uint16), y])
        segs, _ = oracle_segments(orc, base, at)
        ok = [(int(s), int(e)) for s, e in segs if e > 0 and 0 < frames_in(s, e, fl, hop) <= MAXF]
        before = [(s, e) for s, e in ok if (s + e) // 2 <= rel]
        assert before, "a recognisable word at or before the boundary"
        s, e = before[-1]
        pad = (rel - (s + e) // 2) // hop * hop  # more silence in front, whole hops: the segments move with it
        later = [(s2, e2) for s2, e2 in ok if s2 > e and e2 - s2 > 2400 * sc]
        assert later, "a later word to end the recording in"
        x = np.concatenate([np.full(pad, MID, np.uint16), base])[:pad + later[-1][0] + 1600 * sc]
        assert not np.any(x[:QUIET * sc] != MID) and 40000 * sc < len(x) < 90000 * sc
        segs, _ = oracle_segments(orc, x, at)
        assert segs[-1][1] == -1, "the recording ends inside a segment"
        segs = [(int(s), int(e)) for s, e in segs]  # Python ints: the positions below do not fit the oracle's int32
        hit = [(s, e) for s, e in segs if e > 0 and 0 < frames_in(s, e, fl, hop) <= MAXF and s + S0 - LEAD < B < e + S0]
        assert len(hit) == 1, (name, c)
        assert 5 <= len(segs) <= 9
        # no segment can start where the ring holds nothing: within the lead and v_durmin - 1 hops of the origin
        assert segs[0][0] > LEAD + 7 * hop
        recs.append(x)
        straddlers.append(hit[0])
    for x in recs:
        x.setflags(write=False)
    return dict(recs=recs, origins=origins, bounds=bounds, straddlers=straddlers, hop=hop, fl=fl)


@pytest.mark.parametrize("name", list(FRONT))
def test_a_recognisable_word_straddles_each_boundary(name):
    case = far_case(name)
    hop = case["hop"]
    assert case["origins"][0] < 1 << 31 < case["origins"][0] + len(case["recs"][0])
    assert case["origins"][1] < 1 << 32 < case["origins"][1] + len(case["recs"][1])
    assert case["origins"][2] // hop < 1 << 32 < (case["origins"][2] + len(case["recs"][2])) // hop and case["origins"][2] > 1 << 38
    for (s, e), S0, B in zip(case["straddlers"], case["origins"], case["bounds"]):
        assert S0 % hop == 0 and s + S0 - LEAD < B < e + S0 and (s + S0) // hop < (e + S0) // hop


# ---- sr_live: pushes into guarded buffers ----------------------------------------------------------------------------------------
class GuardedLive:
    """sr_live_push (form "host") or sr_live_push_dev on a side stream (form "dev") through ctypes, every output of every push a
    guarded buffer of bound + 1 rows; collect() files the rows per channel as test_live_session.Feeder does"""

    def __init__(self, eng, sess, form, n_best=2, canary=0xA5):
        self.eng, self.sess, self.form, self.n_best, self.canary = eng, sess, form, n_best, canary
        self.stream = torch.cuda.Stream() if form == "dev" else None
        self.pending = []

    def _outs(self, rows):
        K, R, nc = self.eng.n_templates, self.eng.max_frames, self.eng.n_coef
        dev = "cuda:0" if self.form == "dev" else None
        mk = lambda name, shape, dt: guarded_out(shape, dt, self.canary, 4096, dev, name)  # noqa: E731
        return dict(segs=mk("segs", (rows,), LIVE_SEG_DTYPE), results=mk("results", (rows,), RESULT_DTYPE),
                    scores=mk("scores", (rows, K), np.uint32), mfcc=mk("mfcc", (rows, R, nc), np.int16),
                    nbest=mk("nbest", (rows, self.n_best), NBEST_DTYPE), n_matched=mk("n_matched", (rows,), np.uint32))

    def push(self, chunk, cnt):
        """chunk uint16 [C, W] (W a multiple of 8; what is past cnt[c] is loud), cnt [C]"""
        sess, L = self.sess, self.sess.L
        cnt = np.ascontiguousarray(cnt, np.uint32)
        rows = sess.event_bound(cnt) + 1
        g = self._outs(rows)
        p = lambda k: P(g[k].ptr)  # noqa: E731
        if self.form == "host":
            total = U32(0xFFFFFFFF)
            rc = L.sr_live_push(sess.l, engine._vp(chunk), U64(chunk.shape[1]), engine._vp(cnt), U32(0), U32(rows), p("segs"), U32(self.n_best),
                                p("nbest"), p("n_matched"), p("results"), p("scores"), p("mfcc"), C.byref(total))
            assert rc == 0, L.sr_last_error()
            self.pending.append((g, total.value, None))
        else:
            with torch.cuda.stream(self.stream):
                d = torch.from_numpy(chunk.view(np.int16)).cuda()
                count = guarded_out((1,), np.uint32, self.canary, 4096, "cuda:0", "count")
                rc = L.sr_live_push_dev(sess.l, P(d.data_ptr()), U64(chunk.shape[1]), engine._vp(cnt), U32(0), U32(rows), p("segs"), P(count.ptr),
                                        U32(self.n_best), p("nbest"), p("n_matched"), p("results"), p("scores"), p("mfcc"),
                                        P(self.stream.cuda_stream))
            assert rc == 0, L.sr_last_error()
            self.pending.append((g, count, d))  # (the chunk stays alive until the stream has used it)

    def collect(self, n_channels):
        """-> per channel dict(segs=[...], results=[...], ...) in order of emission; every guard checked"""
        if self.stream is not None:
            self.stream.synchronize()
        out = [dict(segs=[], **{k: [] for k in KEYS}) for _ in range(n_channels)]
        for g, total, _ in self.pending:
            if self.form == "dev":
                total.check()
                total = int(total.interior()[0])
            body = {}
            for k, b in g.items():
                b.check()
                body[k] = b.interior()
                assert total < len(body[k])
                if self.form == "host":  # nothing past `total` rows (the device form pads them with failed records)
                    assert np.all(body[k][total:].view(np.uint8) == self.canary), k
            segs = body["segs"][:total]
            key = segs["channel"].astype(object) * (1 << 62) + segs["start"].astype(object)
            assert all(a < b for a, b in zip(key[:-1], key[1:])), "ascending channel, then ascending start"
            for i, s in enumerate(segs):
                o = out[int(s["channel"])]
                o["segs"].append(s.copy())
                for k in KEYS:
                    o[k].append(body[k][i].copy())
        self.pending = []
        return out


def feed_live(gl, recs, sizes):
    """recs[c] -> channel c (None: a silent channel), sizes(push index) -> requested counts, until everything is pushed"""
    n_ch = len(recs)
    pos, k = [0] * n_ch, 0
    left = lambda: [0 if x is None else len(x) - p for x, p in zip(recs, pos)]  # noqa: E731
    while any(left()):
        cnt = np.minimum(np.asarray(sizes(k), np.int64), left()).astype(np.uint32)
        W = (max(int(cnt.max()), 1) + 7) // 8 * 8
        chunk = np.full((n_ch, W), 0xFFFF, np.uint16)
        for c in range(n_ch):
            if cnt[c]:
                chunk[c, :cnt[c]] = recs[c][pos[c]:pos[c] + cnt[c]]
                pos[c] += int(cnt[c])
        gl.push(chunk, cnt)
        k += 1
    return k


def check_shifted(bucket, ended, one, b, S0, what):
    """what a channel emitted and its end record (or None) against recording b of the one-shot output, positions + S0"""
    off, segs = one["seg_offsets"], one["segs"]
    want = segs[off[b]:off[b + 1]]
    n_open = int(len(want) > 0 and want[-1]["end"] < 0)
    closed = want[:len(want) - n_open]
    assert np.all(closed["end"] >= 0)
    got = np.array(bucket["segs"], LIVE_SEG_DTYPE) if bucket["segs"] else np.zeros(0, LIVE_SEG_DTYPE)
    assert len(got) == len(closed), (what, len(got), len(closed))
    exp = np.zeros(len(closed), LIVE_SEG_DTYPE)
    exp["channel"], exp["frm_num"] = got["channel"], closed["frm_num"]
    exp["start"], exp["end"] = closed["start"].astype(np.int64) + S0, closed["end"].astype(np.int64) + S0
    assert got.tobytes() == exp.tobytes(), (what, got.tolist(), exp.tolist())
    if n_open:
        assert ended is not None, what
        assert (int(ended["start"]), int(ended["end"]), int(ended["frm_num"])) == (int(want[-1]["start"]) + S0, -1, 0), (what, ended)
    else:
        assert ended is None, (what, ended)
    lo = int(off[b])
    for k in KEYS:
        if len(got):
            assert np.stack(bucket[k]).tobytes() == np.ascontiguousarray(one[k][lo:lo + len(got)]).tobytes(), (what, k)
    return len(got)


@functools.lru_cache(maxsize=None)
def far_engine(name):
    """the engine of a front end and the one-shot records of its three recordings (computed once)"""
    ekw, _, _ = FRONT[name]
    case = far_case(name)
    eng = Engine(max_frames=MAXF, testing=True, **ekw)
    random_templates(eng, np.random.default_rng(77))
    at = np.array([ATAP] * 3, ATAP_DTYPE)
    one = one_shot(eng, case["recs"], atap=at, n_best=2)
    return eng, at, one


@pytest.mark.gpu
@pytest.mark.parametrize("chunking", ["irregular", "chunk_max"])
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name", list(FRONT))
def test_live_records_far_into_a_recording_are_the_one_shot_records_shifted(name, form, chunking):
    case = far_case(name)
    recs, O, hop = case["recs"], case["origins"], case["hop"]
    eng, at, one = far_engine(name)
    # the reference's own segments: the straddling word is recognised
    off, ok = one["seg_offsets"], one["results"]["status"] == ST_OK
    for c in range(3):
        s = one["segs"][off[c]:off[c + 1]][ok[off[c]:off[c + 1]]]
        assert np.any((s["start"].astype(np.int64) + O[c] - LEAD < case["bounds"][c]) & (s["end"].astype(np.int64) + O[c] > case["bounds"][c])), c
        assert one["segs"][off[c + 1] - 1]["end"] == -1
    cm = 800 * FRONT[name][2]
    rng = np.random.default_rng(78)
    sizes = (lambda k: rng.integers(0, cm + 1, 3) * (rng.random(3) > 0.1)) if chunking == "irregular" else (lambda k: [cm] * 3)
    sess = None
    try:
        engine.dev_hook("live_origin", O[0])
        sess = eng.live(3, cm, atap=at)  # every channel fresh at O[0] ...
        for c in (1, 2):                 # ... and an ended channel fresh at the origin the hook holds then
            engine.dev_hook("live_origin", O[c])
            assert len(sess.end([c])) == 0
        gl = GuardedLive(eng, sess, form)
        assert feed_live(gl, recs, sizes) >= len(recs[0]) // cm
        out = gl.collect(3)
        # ended inside a word: {start + origin, -1}; channel 0 restarts at 0, channel 1 at O[0], channel 2 at O[1]
        ended = []
        for c, nxt in enumerate((0, O[0], O[1])):
            engine.dev_hook("live_origin", nxt)
            e = sess.end([c])
            assert len(e) == 1 and e[0]["channel"] == c
            ended.append(e[0])
        n = sum(check_shifted(out[c], ended[c], one, c, O[c], (name, form, chunking, "channel", c)) for c in range(3))
        assert n >= 12
        # the same audio again from the new origins: recording 2 unshifted on channel 0, the words across 2^31 and 2^32 on
        # other channels than before
        again = (2, 0, 1)
        feed_live(gl, [recs[b] for b in again], sizes)
        out = gl.collect(3)
        engine.dev_hook("live_origin", 0)
        ended = {int(e["channel"]): e for e in sess.end([0, 1, 2])}
        for c, (b, S0) in enumerate(zip(again, (0, O[0], O[1]))):
            check_shifted(out[c], ended.get(c), one, b, S0, (name, form, chunking, "second round, channel", c))
        assert len(sess.end([0, 1, 2])) == 0
    finally:
        engine.dev_hook("live_origin", 0)
        if sess is not None:
            sess.close()


# ---- sr_live: a segment of 65 536 frames or more (no hook: the channel's own sequence gets there) -------------------------------
LONG_FRAMES = (65536 + 50, 65535)


@functools.lru_cache(maxsize=None)
def long_case():
    """two recordings: silence, one loud stretch that the VAD reports as ONE segment of 65 586 (65 535) frames, silence, ordinary
    words.  Sized and checked with the CPU oracle's VAD."""
    orc = ol.Oracle(max_frames=MAXF, max_seg=1 << 16)
    hop, fl, at = orc.hop, orc.frame_len, ol.Atap(*ATAP)
    tail = spaced_words(91, synth.word_bank(10), 16000, lo=30, hi=60)[2400:]
    loud = np.full(hop * 65700, MID, np.int32)
    loud[0::2] += 400
    loud[1::2] -= 400
    loud = loud.astype(np.uint16)
    build = lambda n: np.concatenate([np.full(QUIET, MID, np.uint16), loud[:hop * n], np.full(40 * hop, MID, np.uint16), tail])  # noqa: E731
    segs, _ = oracle_segments(orc, build(65600), at)
    extra = frames_in(int(segs[0][0]), int(segs[0][1]), fl, hop) - 65600  # frames of the segment beyond its loud hops
    recs = []
    for want in LONG_FRAMES:
        x = build(want - extra)
        segs, _ = oracle_segments(orc, x, at)
        n = [frames_in(int(s), int(e), fl, hop) for s, e in segs]
        assert n[0] == want and len(n) >= 2 and all(0 < v <= MAXF for v in n[1:]) and segs[-1][1] > 0, n
        x.setflags(write=False)
        recs.append(x)
    return recs


def test_the_long_segments_exist_in_the_reference():
    recs = long_case()
    assert all(5_200_000 < len(x) < 5_400_000 for x in recs)
    assert (LONG_FRAMES[0] & 0xFFFF) == 50 <= MAXF < (LONG_FRAMES[1] & 0xFFFF)  # MFCC.C:102's u16 count passes the cap for the first only


@pytest.mark.gpu
def test_a_live_segment_of_65536_frames_fails_where_the_one_shot_path_takes_the_wrapped_count():
    recs = long_case()
    eng = Engine(max_frames=MAXF, testing=True)
    random_templates(eng, np.random.default_rng(79))
    at = np.array([ATAP] * 2, ATAP_DTYPE)
    one = one_shot(eng, recs, atap=at, n_best=2)
    off = one["seg_offsets"]
    first = [one["segs"][off[b]] for b in (0, 1)]
    fl, hop = 160, 80
    assert [frames_in(int(g["start"]), int(g["end"]), fl, hop) for g in first] == list(LONG_FRAMES)
    # the one-shot path: the u16-wrapped count, 50 frames recognised; 65 535 stays above the cap
    assert first[0]["frm_num"] == 50 and one["results"][off[0]]["status"] == ST_OK and one["results"][off[0]]["frm_num"] == 50
    assert first[1]["frm_num"] == 0 and one["results"][off[1]]["status"] == ST_MFCC_FAIL
    for b, x in enumerate(recs):
        sess = eng.live(1, 1 << 20, atap=at[b:b + 1])
        try:
            gl = GuardedLive(eng, sess, "host")
            step = (-(-len(x) // 6) + 7) // 8 * 8  # six pushes
            assert step <= 1 << 20 and feed_live(gl, [x], lambda k: [step]) == 6
            out = gl.collect(1)[0]
            assert len(sess.end([0])) == 0
        finally:
            sess.close()
        n = int(off[b + 1] - off[b])
        assert len(out["segs"]) == n >= 2
        g = out["segs"][0]
        assert (int(g["start"]), int(g["end"]), int(g["frm_num"])) == (int(first[b]["start"]), int(first[b]["end"]), 0)
        assert out["results"][0]["status"] == ST_MFCC_FAIL and out["results"][0]["frm_num"] == 0 and out["results"][0]["min_dis"] == DIS_ERR
        assert not np.any(out["mfcc"][0]) and np.all(out["scores"][0] == DIS_ERR)
        for k in KEYS:  # a failed record like the one-shot path's failed record of 65 535 frames
            assert out[k][0].tobytes() == np.ascontiguousarray(one[k][off[1]]).tobytes(), (b, k)
        # every other record and result byte-identical; with 65 535 frames the long one too
        keep = dict(segs=out["segs"][1 - b:], **{k: out[k][1 - b:] for k in KEYS})
        trimmed = dict(one, seg_offsets=np.array([off[b] + 1 - b, off[b + 1]], np.uint32))
        assert check_shifted(keep, None, trimmed, 0, 0, ("long", b)) == n - 1 + b


# ---- the hooks' refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_origin_hooks_are_refused_where_they_do_not_apply_and_change_nothing():
    eng = Engine(max_frames=MAXF, testing=True)
    random_templates(eng, np.random.default_rng(80))
    x = spaced_words(92, synth.word_bank(10), 30000)
    one = one_shot(eng, [x])
    assert one["total"] >= 3
    at = np.array([ATAP], ATAP_DTYPE)
    sess = given = spot = None
    try:
        # a session that computes its own noise head: no origin at open ...
        engine.dev_hook("live_origin", 8000)
        with pytest.raises(SrError, match="error 3"):
            eng.live(1, 800)
        engine.dev_hook("live_origin", 0)
        sess = eng.live(1, 800)
        f = Feeder(sess, n_best=3)
        f.load(0, x)
        for _ in range(20):
            f.push([800])
        # ... nor at end, which changes nothing: the channel goes on and gives the one-shot records of the whole recording
        engine.dev_hook("live_origin", 8000)
        seg, n = np.zeros(1, LIVE_SEG_DTYPE), U32(77)
        ch = np.zeros(1, np.uint32)
        assert sess.L.sr_live_end(sess.l, engine._vp(ch), U32(1), engine._vp(seg), C.byref(n)) == BAD_ARG
        assert n.value == 77 and not seg.view(np.uint8).any()
        engine.dev_hook("live_origin", 0)
        f.drive(lambda k: [800])
        assert check_all(f, sess.end([0]), one, [x]) >= 3
        # an origin that is no multiple of hop, or negative, with thresholds given
        for bad in (8001, 79, -80):
            engine.dev_hook("live_origin", bad)
            with pytest.raises(SrError, match="error 3"):
                eng.live(1, 800, atap=at)
        engine.dev_hook("live_origin", 0)
        given = eng.live(1, 800, atap=at)
        engine.dev_hook("live_origin", 8001)
        assert given.L.sr_live_end(given.l, engine._vp(ch), U32(1), engine._vp(seg), C.byref(n)) == BAD_ARG and n.value == 77
        # the spotter's origin above the cap
        K = eng.n_templates
        for bad in (CAP + 1, -1, 1 << 32):
            engine.dev_hook("spot_live_origin", bad)
            with pytest.raises(SrError, match="error 3"):
                eng.spot_live(1, 50, 16)
        engine.dev_hook("spot_live_origin", CAP)  # the cap itself is a valid origin: nothing more fits
        spot = eng.spot_live(1, 50, 16)
        assert spot.rows([0]) == 0 and spot.L.sr_spot_live_rows(spot.l, None, U32(1)) == 0
        engine.dev_hook("spot_live_origin", CAP + 1)
        hits, wins = np.zeros((1, K), ref.SPOT_DTYPE), np.zeros(1, live.SPOT_WIN_DTYPE)
        assert spot.L.sr_spot_live_end(spot.l, engine._vp(ch), U32(1), engine._vp(hits), engine._vp(wins), C.byref(n)) == BAD_ARG
        assert n.value == 77
    finally:
        for h in HOOKS:
            engine.dev_hook(h, 0)
        for s in (sess, given, spot):
            if s is not None:
                s.close()
        eng.close()


# ---- sr_spot_live: columns up to the cap ------------------------------------------------------------------------------------------
S_TF, S_VALID = (1, 14, 65, 9), (1, 1, 1, 0)  # K = 4 slots, the last one erased
S_C, S_N, S_CHUNK = 3, 400, 200
SPOT_ORIGINS = {"sign_bit": (1 << 31) - 130,      # columns cross 2^31 inside a 64-lane sweep and (win 50) inside a window
                "to_the_cap": CAP - S_N,          # the last frame is frame 0xFFFF0000 - 1: exactly to the cap
                "inside_a_window": 3_000_000_037}  # % 16 = 5, % 50 = 37: a partial first window
SPOT_WINS = (1, 16, 50)
SPOT_SIZES = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def s_store(amp):
    rng = np.random.default_rng(1000 + amp)
    tf, valid = np.array(S_TF, np.uint32), np.array(S_VALID, np.uint8)
    tm = np.zeros((len(S_TF), max(S_TF) + 1, 12), np.int16)
    for k in range(len(S_TF)):
        tm[k, :tf[k]] = rng.integers(-amp, amp + 1, (tf[k], 12))
    for a in (tm, tf, valid):
        a.setflags(write=False)
    return tm, tf, valid


@functools.lru_cache(maxsize=None)
def s_feats(amp):
    rng = np.random.default_rng(1100 + amp)
    f = rng.integers(-amp, amp + 1, (S_C, S_N, 12)).astype(np.int16)
    f[1, 100:165] = s_store(amp)[0][2, :65]  # a template inside channel 1
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def s_want(amp, win, origin, n=S_N):
    out = [live.window_records(s_feats(amp)[c, :n], *s_store(amp), win, origin) for c in range(S_C)]
    for a in out:
        a.setflags(write=False)
    return out


def s_schedule(win, origin, N=S_N):
    """per push the counts [3], sizes from SPOT_SIZES (the last of a channel is what is left): channel 0 walks frame by frame
    across the first window edge after its first 63 frames, channel 1 starts with 30 single frames, channel 2 is random"""
    rng = np.random.default_rng(1200 + win % 1000)

    def fill(head):
        out = list(head)
        while sum(out) < N:
            out.append(min(int(rng.choice(SPOT_SIZES)), N - sum(out)))
        return out

    edge = -(-(origin + 63) // win) * win - origin  # frames up to the first window edge at or after frame 63
    singles = [1] * max(edge - 63 + 2, 3) if edge + 2 <= 130 else [1] * 3
    return per_channel([fill([63] + singles + [64, 200]), fill([1] * 30 + [200, 65]), fill([])])


def test_spot_inputs_cross_what_they_are_meant_to_cross():
    """on the reference and the schedules alone: the sign bit inside a sweep and inside a window, the run to the cap, the
    partial first window with a hit, single-frame pushes over a window edge"""
    A = SPOT_ORIGINS["sign_bit"]
    for win in SPOT_WINS:
        starts = np.cumsum([[0, 0, 0]] + s_schedule(win, A), 0)
        sched = np.array(s_schedule(win, A))
        assert np.all(sched.sum(0) == S_N) and sched.max() <= S_CHUNK
        inside = [(int(p), int(n)) for p, n in zip(starts[:-1].ravel(), sched.ravel()) if A + p < 1 << 31 < A + p + n and 8 <= ((1 << 31) - A - p) % 64 <= 56]
        assert inside, win  # a push whose sweep holds columns on both sides of 2^31, away from the sweep's edges
        edge = -(-(A + 63) // win) * win - A
        assert all(int(starts[i, 0]) + 1 == int(starts[i + 1, 0]) for i in range(1, 4)) and (win == 1 or edge in starts[:, 0])
    assert (1 << 31) % 50 not in (0, 49)
    assert SPOT_ORIGINS["to_the_cap"] + S_N == CAP and CAP % 50 == 10
    Cc = SPOT_ORIGINS["inside_a_window"]
    for win in (16, 50):
        assert Cc % win and all(w[0, 0]["dis"] != DIS_ERR and w[0, 0]["end"] < (Cc // win + 1) * win for w in s_want(2, win, Cc))
    for amp in (2, 3000):  # shifted, the planted template is found where it was put
        g = s_want(amp, 50, A)[1][(A + 164) // 50 - A // 50, 2]
        assert g["dis"] == 0 and A + 95 <= g["start"] <= A + 105 < 1 << 31 <= g["end"] <= A + 164
    assert np.array_equal(s_want(2, 16, 0)[0]["dis"], s_want(2, 16, 1 << 31)[0]["dis"])


class Windows:
    """files every emitted row under its (channel, absolute window); every push is checked against what the counts alone say"""

    def __init__(self, n_ch, win, origin):
        self.win, self.count, self.recs = win, [origin] * n_ch, [dict() for _ in range(n_ch)]

    def take(self, out, new):
        exp = live.push_windows(self.count, new, self.win)
        assert out["n_rows"] == len(exp) and [(int(w["channel"]), int(w["window"])) for w in out["wins"]] == exp, (out["wins"], exp)
        assert np.array_equal(out["scores"], out["hits"]["dis"])
        for r, (c, w) in enumerate(exp):
            assert w not in self.recs[c], "a window emitted twice"
            self.recs[c][w] = out["hits"][r].copy()
        self.count = [a + int(b) for a, b in zip(self.count, new)]

    def end(self, ses, channels, fresh_at):
        out = ses.end(channels)
        exp = [(c, self.count[c] // self.win) for c in channels if self.count[c] % self.win]
        assert out["n_rows"] == len(exp) and [(int(w["channel"]), int(w["window"])) for w in out["wins"]] == exp, (out["wins"], exp)
        for r, (c, w) in enumerate(exp):
            assert w not in self.recs[c]
            self.recs[c][w] = out["hits"][r].copy()
        for c in channels:
            self.count[c] = fresh_at

    def channel(self, c, origin):
        n, w0 = len(self.recs[c]), origin // self.win
        assert sorted(self.recs[c]) == list(range(w0, w0 + n)), sorted(self.recs[c])
        return np.array([self.recs[c][w] for w in range(w0, w0 + n)], ref.SPOT_DTYPE).reshape(n, -1)


def spot_push(ses, chunk, cnt, form, max_rows=None, canary=0xA5, refused=False):
    """sr_spot_live_push_dev / sr_spot_live_push through ctypes into guarded hits and scores of rows + 2 rows; chunk int16
    [C, F, 12], rows past cnt[c] poisoned.  refused: the call must return SR_ERR_BAD_ARG and write nothing"""
    L, K = ses.L, ses.eng.n_templates
    ct = np.ascontiguousarray(cnt, np.uint32)
    F = chunk.shape[1]
    rows = ses.rows(ct)
    if max_rows is None:
        max_rows = rows + 2
    chunk = poison_feature_rows(np.array(chunk), np.minimum(ct, F))
    dev = "cuda:0" if form == "dev" else None
    g_h = guarded_out((max_rows, K), ref.SPOT_DTYPE, canary, 4096, dev, "hits")
    g_s = guarded_out((max_rows, K), np.uint32, canary, 4096, dev, "scores")
    wins, n = np.full(2 * (max_rows + 1), 0x5A5A5A5A, np.uint32).view(live.SPOT_WIN_DTYPE), U32(0xDEAD)
    head = (U64(F * 12), engine._vp(ct), U32(0), U32(max_rows), P(g_h.ptr), P(g_s.ptr), engine._vp(wins), C.byref(n))
    if form == "dev":
        d = torch.from_numpy(chunk).cuda()
        rc = L.sr_spot_live_push_dev(ses.l, P(d.data_ptr()), *head, P(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    else:
        rc = L.sr_spot_live_push(ses.l, engine._vp(chunk), *head)
    if refused:
        assert rc == BAD_ARG and n.value == 0xDEAD and np.all(wins.view(np.uint32) == 0x5A5A5A5A), (rc, cnt)
        g_h.check_untouched()
        g_s.check_untouched()
        return None
    assert rc == 0, L.sr_last_error()
    g_h.check()
    g_s.check()
    assert n.value == rows  # sr_spot_live_rows said how many rows the push writes
    hits, sc = g_h.interior(), g_s.interior()
    assert np.all(hits[rows:].view(np.uint8) == canary) and np.all(sc[rows:].view(np.uint8) == canary)  # rows >= *n_rows untouched
    assert np.all(wins.view(np.uint32)[2 * rows:] == 0x5A5A5A5A)
    return dict(hits=hits[:rows], scores=sc[:rows], wins=wins[:rows], n_rows=rows)


def feed_spot(ses, col, f, at, sched, form):
    for cnt in sched:
        F = max(max(cnt), 1)
        chunk = np.zeros((len(f), F, 12), np.int16)
        for c in range(len(f)):
            chunk[c, :cnt[c]] = f[c, at[c]:at[c] + cnt[c]]
            at[c] += cnt[c]
        col.take(spot_push(ses, chunk, cnt, form), cnt)


def spot_engine(amp):
    eng = Engine(max_frames=S_CHUNK, device=0, testing=True)
    eng.set_templates_dense(*s_store(amp))
    return eng


def run_spot(eng, amp, win, origin, form):
    """400 frames per channel from `origin`, every channel ended -> the Windows"""
    engine.dev_hook("spot_live_origin", origin)
    ses = eng.spot_live(S_C, S_CHUNK, win)
    try:
        col = Windows(S_C, win, origin)
        feed_spot(ses, col, s_feats(amp), [0] * S_C, s_schedule(win, origin), form)
        col.end(ses, [0, 1, 2], origin)
        assert ses.end([0, 1, 2])["n_rows"] == (S_C if origin % win else 0)  # fresh at the origin: a partial window stands open, empty
    finally:
        ses.close()
        engine.dev_hook("spot_live_origin", 0)
    return col


@pytest.mark.gpu
@pytest.mark.parametrize("win", SPOT_WINS)
@pytest.mark.parametrize("oname", list(SPOT_ORIGINS))
def test_spot_records_far_into_a_channel_are_the_reference_with_origin(oname, win):
    origin = SPOT_ORIGINS[oname]
    for amp in (2, 3000):
        exp = s_want(amp, win, origin)
        assert all(np.all(e[:, 3]["dis"] == DIS_ERR) for e in exp) and all(np.any(e[:, :3]["dis"] != DIS_ERR) for e in exp)
        eng = spot_engine(amp)
        try:
            got = {form: run_spot(eng, amp, win, origin, form) for form in ("dev", "host")}
        finally:
            eng.close()
        for c in range(S_C):
            for form in ("dev", "host"):
                same(got[form].channel(c, origin), exp[c], f"{oname}, win {win}, amp {amp}, {form} form, channel {c}")
            assert got["dev"].channel(c, origin).tobytes() == got["host"].channel(c, origin).tobytes()


@pytest.mark.gpu
def test_spot_window_of_2_pow_31_frames_completes_at_the_sign_bit():
    win, origin = 1 << 31, (1 << 31) - 100
    exp = s_want(2, win, origin)
    assert all(len(e) == 2 and e[0, 0]["end"] < 1 << 31 <= e[1, 0]["end"] for e in exp)  # a hit on either side
    eng = spot_engine(2)
    try:
        for form in ("dev", "host"):
            col = run_spot(eng, 2, win, origin, form)  # window 0 by the push that holds column 2^31 - 1, window 1 by the end
            for c in range(S_C):
                same(col.channel(c, origin), exp[c], f"{form} form, channel {c}")
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["dev", "host"])
def test_spot_frame_cap_refuses_the_push_that_would_pass_it_and_nothing_else(form):
    win, origin, f = 50, CAP - S_N, s_feats(2)
    exp = s_want(2, win, origin)
    eng = spot_engine(2)
    engine.dev_hook("spot_live_origin", origin)
    ses = eng.spot_live(S_C, S_CHUNK, win)
    try:
        col, at = Windows(S_C, win, origin), [0] * S_C
        feed_spot(ses, col, f, at, [[200, 200, 200], [200, 190, 190]], form)
        assert col.count == [CAP, CAP - 10, CAP - 10]
        for cnt in ([1, 5, 5], [1, 0, 0], [200, 10, 10]):  # channel 0 stands at exactly 0xFFFF0000 frames: one more is refused
            assert ses.rows(np.array(cnt, np.uint32)) == 0
            assert spot_push(ses, np.zeros((S_C, max(cnt), 12), np.int16), cnt, form, max_rows=8, refused=True) is None
            assert b"0xFFFF0000" in ses.L.sr_last_error()
        # the other channels of the refused calls were not advanced: their last ten frames give the records of an unrefused history
        feed_spot(ses, col, f, at, [[0, 10, 10]], form)
        assert col.count == [CAP] * S_C
        assert spot_push(ses, np.zeros((S_C, 1, 12), np.int16), [0, 0, 1], form, max_rows=8, refused=True) is None
        # the end still emits the open window (0xFFFF0000 % 50 = 10 frames of it) ...
        engine.dev_hook("spot_live_origin", 0)
        col.end(ses, [0, 1, 2], 0)
        for c in range(S_C):
            same(col.channel(c, origin), exp[c], f"{form} form, channel {c}")
            assert (CAP // win) in col.recs[c]
        # ... and the channels are usable again, from frame 0
        col = Windows(S_C, win, 0)
        feed_spot(ses, col, f, [0] * S_C, [[64, 64, 64], [1, 65, 0]], form)
        col.end(ses, [0, 1, 2], 0)
        for c, n in enumerate((65, 129, 64)):
            same(col.channel(c, 0), s_want(2, win, 0, n)[c], f"{form} form, restarted channel {c}")
    finally:
        ses.close()
        engine.dev_hook("spot_live_origin", 0)
        eng.close()


@pytest.mark.gpu
def test_spot_pcm_session_across_the_sign_bit_equals_the_feature_session():
    FRAME_LEN, HOP, win, origin = 160, 80, 50, SPOT_ORIGINS["sign_bit"]
    rng = np.random.default_rng(1300)
    eng = Engine(max_frames=S_CHUNK, device=0, testing=True)
    nf = 300
    R = 1 + (nf - 1) * HOP + FRAME_LEN + 37  # 300 frames and a remainder
    X = (2048 + 600 * np.sin(np.arange(R)[None] * np.array([[0.05], [0.11]])) + rng.integers(-300, 301, (2, R))).astype(np.uint16)
    mid = np.array([2048, 2040], np.uint32)
    pieces = []
    for p in range(0, nf, S_CHUNK):  # the frames of the whole path, piece by piece
        cnt = min(S_CHUNK, nf - p)
        s, e = 1 + p * HOP, 1 + p * HOP + (cnt - 1) * HOP + FRAME_LEN
        n, m = eng.mfcc(X, [s, s], [e, e], mid)
        assert list(n) == [cnt, cnt]
        pieces.append(m[:, :cnt])
    allf = np.ascontiguousarray(np.concatenate(pieces, 1))
    tf, valid = np.array(S_TF, np.uint32), np.array(S_VALID, np.uint8)
    tm = np.zeros((4, 66, 12), np.int16)
    for k, (c, at) in enumerate(((0, 135), (1, 120), (1, 90), (0, 10))):  # pieces of the recordings, one across frame 130
        tm[k, :tf[k]] = allf[c, at:at + tf[k]]
    eng.set_templates_dense(tm, tf, valid)
    exp = [live.window_records(allf[c], tm, tf, valid, win, origin) for c in range(2)]
    assert exp[1][(origin + 154) // win - origin // win, 2]["dis"] == 0  # found, its start below 2^31 and its end above
    assert exp[1][(origin + 154) // win - origin // win, 2]["start"] < 1 << 31 < exp[1][(origin + 154) // win - origin // win, 2]["end"]
    engine.dev_hook("spot_live_origin", origin)
    pcm = feat = None
    try:
        pcm, feat = eng.spot_live(2, 400, win, mid), eng.spot_live(2, S_CHUNK, win)
        frames = lambda r: [live.pcm_frames(v, FRAME_LEN, HOP) for v in r]  # noqa: E731
        col_p, got = Windows(2, win, origin), [0, 0]
        for i, cnt in enumerate(per_channel([cut(R, [400, 399, 1]), cut(R, [161, 80, 237, 0, 400])])):
            S = (max(max(cnt), 1) + 7) // 8 * 8
            chunk = np.full((2, S), 4095, np.uint16)  # poison past n[c]
            for c in range(2):
                chunk[c, :cnt[c]] = X[c, got[c]:got[c] + cnt[c]]
            new = [a - b for a, b in zip(frames([g + n for g, n in zip(got, cnt)]), frames(got))]
            ct = np.array(cnt, np.uint32)
            assert pcm.rows(ct) == len(live.push_windows(col_p.count, new, win))
            if i % 2:
                out = pcm.push_pcm(chunk, ct)
            else:
                out = pcm.push_pcm_dev(torch.from_numpy(chunk.view(np.int16)).cuda(), ct)
                torch.cuda.synchronize()
                K = out["hits"].shape[1]
                out = dict(out, hits=out["hits"].cpu().numpy().view(ref.SPOT_DTYPE).reshape(out["n_rows"], K),
                           scores=out["scores"].cpu().numpy().view(np.uint32))
            col_p.take(out, new)
            got = [g + n for g, n in zip(got, cnt)]
        assert got == [R, R] and col_p.count == [origin + nf] * 2
        col_p.end(pcm, [0, 1], origin)
        col_f = Windows(2, win, origin)
        feed_spot(feat, col_f, allf, [0, 0], [[n, n] for n in cut(nf, [65, 1, 64, 63])], "dev")
        col_f.end(feat, [0, 1], origin)
        for c in range(2):
            same(col_p.channel(c, origin), exp[c], f"PCM session, channel {c}")
            assert col_p.channel(c, origin).tobytes() == col_f.channel(c, origin).tobytes()
    finally:
        for s in (pcm, feat):
            if s is not None:
                s.close()
        engine.dev_hook("spot_live_origin", 0)
        eng.close()
