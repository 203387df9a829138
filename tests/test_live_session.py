"""Live sessions (sr_live_open / sr_live_push[_dev] / sr_live_end): chunked audio, the stream VAD's state carried between
pushes.  THE RULE under test: whatever the chunking, the records a session emits for a channel equal what
Engine.recognize_stream returns for everything pushed to it as one recording -- segments, results, score rows, MFCC rows and
N-best entries byte for byte.  The segments are also held to the CPU oracle's VAD with an unbounded segment count, so the
comparison does not rest on the product alone."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import oracle_lib as ol
from guarded import guarded_out
from stm32_speech_recognition_amd import engine, synth
from stm32_speech_recognition_amd.engine import (ATAP_DTYPE, DIS_ERR, LIVE_SEG_DTYPE, NBEST_DTYPE, NO_WORD, RESULT_DTYPE,
                                                 ST_MFCC_FAIL, ST_OK, ST_SEG_OOB, ST_VAD_FAIL, Engine, LiveSession)
from test_stream_recognition import EXT, GEN, MOST, constructed_cases, make_recording, oracle_segments, random_templates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
FUNCS = ("sr_live_geometry", "sr_live_events_in_frames", "sr_live_open", "sr_live_close", "sr_live_event_bound",
         "sr_live_push_dev", "sr_live_push", "sr_live_end")
BAD_ARG, NO_TEMPLATES = 3, 4
LEAD = 8  # samples before a segment in its recognition row


class LiveSeg(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("frm_num", C.c_uint32), ("start", C.c_int64), ("end", C.c_int64)]


# ---- CPU: the header, both libraries, the Python mirror ---------------------------------------------------------------------
def test_header_declares_live_api_and_libraries_export_it():
    src = open(HEADER).read()
    m = re.search(r"typedef struct sr_live_seg \{(.*?)\} sr_live_seg;", src, re.S)
    assert m, "sr_live_seg"
    fields = re.findall(r"(u?int(?:32|64)_t)\s+(\w+);", m.group(1))
    assert fields == [("uint32_t", "channel"), ("uint32_t", "frm_num"), ("int64_t", "start"), ("int64_t", "end")]
    assert C.sizeof(LiveSeg) == 24 and LIVE_SEG_DTYPE.itemsize == 24
    assert [LIVE_SEG_DTYPE.fields[f][1] for f in ("channel", "frm_num", "start", "end")] == [0, 4, 8, 16]
    assert re.search(r"typedef struct sr_live sr_live;", src)
    for fn in FUNCS:
        assert re.search(r"\b(?:int|void|uint32_t) %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    assert callable(getattr(Engine, "live", None))
    for meth in ("push", "push_dev", "end", "event_bound", "close"):
        assert callable(getattr(LiveSession, meth, None)), meth


# configuration keywords, (frame_len, hop, v_durmin, s_durmax, noise_len)
GEOMETRY_CONFIGS = [({}, (160, 80, 8, 11, 2400)), (EXT, (320, 160, 8, 11, 4800)), (MOST[0], (160, 80, 80, 110, 24000))]


def frames_of(n, fl, hop):
    return (n - fl + hop - 1) // hop if n > fl else 0


def events_in_frames(vd, sd, f):
    L = engine.load_library()
    L.sr_live_events_in_frames.restype = C.c_uint32
    return int(L.sr_live_events_in_frames(C.c_uint32(vd), C.c_uint32(sd), C.c_uint64(f)))


@pytest.mark.parametrize("kw,fr", GEOMETRY_CONFIGS, ids=["reference", "extension", "hop_1ms"])
def test_geometry_is_the_ring_rule(kw, fr):
    fl, hop, vd, sd, noise = fr
    for R in (119, 400):
        for chunk_max in (1, 79, 80, 81, 800, 801, 4000, 40000, 1 << 20):
            ring, slots, nbytes = engine.live_geometry(chunk_max, max_frames=R, **kw)
            need = max((R + sd + 4) * hop + LEAD + chunk_max, noise + fl + chunk_max)
            assert ring == -(-need // hop) * hop, (R, chunk_max)
            # a push completes at most ceil(chunk_max / hop) frames, or every frame of a head that it completes
            f_max = max(-(-chunk_max // hop), frames_of(noise - 1 + chunk_max, fl, hop))
            assert slots == events_in_frames(vd, sd, f_max) >= 1
            assert nbytes >= 2 * ring + 48 + 16 * slots
    L = engine.load_library()
    cfg = engine.Config()
    L.sr_default_config(C.byref(cfg))
    out = (C.c_uint32 * 3)()
    assert L.sr_live_geometry(C.byref(cfg), C.c_uint32(0), out) == BAD_ARG
    assert L.sr_live_geometry(C.byref(cfg), C.c_uint32((1 << 24) + 1), out) == BAD_ARG
    assert L.sr_live_geometry(None, C.c_uint32(800), out) == BAD_ARG and L.sr_live_geometry(C.byref(cfg), C.c_uint32(800), None) == BAD_ARG


def sm_step(s, loud, vd, sd):
    """StreamSm::step (csrc/sr_stream_dev.h) restated: (next state, event); event 1 = START, 2 = END"""
    nF = max(vd, 2) - 1
    sp = nF + 1
    if s == 0:
        return (1 if loud else 0), 0
    if s <= nF:
        if not loud:
            return 0, 0
        if s + 1 >= vd:
            return sp, 1
        return s + 1, 0
    if s == sp:
        return (sp if loud else sp + 1), 0
    if loud:
        return sp, 0
    back = s - sp + 1
    if back >= sd:
        return 0, 2
    return sp + back, 0


@pytest.mark.parametrize("vd,sd", [(8, 11), (80, 110), (1, 1)])
def test_event_bound_equals_exhaustive_search_over_the_state_machine(vd, sd):
    n_states = max(vd, 2) + max(sd, 2)  # silence, onset states, speech, tail states
    trans = [[sm_step(s, loud, vd, sd) for loud in (0, 1)] for s in range(n_states)]
    assert all(0 <= t[0] < n_states for row in trans for t in row)
    best = [0] * n_states  # most END events in f frames from each entering state
    for f in range(1, 201):
        best = [max((ev == 2) + best[s2] for s2, ev in trans[s]) for s in range(n_states)]
        assert max(best) == events_in_frames(vd, sd, f), (f, max(best))
    assert events_in_frames(vd, sd, 0) == 0


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def pack_ragged(recs):
    lens = np.array([len(r) for r in recs], np.uint32)
    pcm = np.full((len(recs), int(lens.max())), 2048, np.uint16)
    for b, r in enumerate(recs):
        pcm[b, :len(r)] = r
    return pcm, lens


def one_shot(eng, recs, atap=None, n_best=3):
    """Engine.recognize_stream on whole recordings: the yardstick"""
    pcm, lens = pack_ragged(recs)
    return eng.recognize_stream(pcm, lens, atap=atap, n_best=n_best)


KEYS = ("results", "scores", "mfcc", "nbest", "n_matched")


def spaced_words(seed, bank, n, gap=1600, scale=1, lo=12, hi=100):
    """n samples: a noise head, then words of lo..hi frames (x scale) that `gap` quiet samples keep apart"""
    rng = np.random.default_rng(seed)
    nw = n // (hi * 40 * scale) + 8
    x = synth.make_multiword(list(rng.integers(0, len(bank[0]), nw)), list(rng.integers(lo, hi, nw) * scale), seed, bank, S=n,
                             gap=gap, gain=2.0)
    return synth.as_u16_numpy(x)


class Feeder:
    """pushes recordings through a session chunk by chunk and files what comes out per channel"""

    def __init__(self, sess, n_best=3, recognize=True):
        self.sess, self.C, self.n_best, self.recognize = sess, sess.n_channels, n_best, recognize
        self.cur = [np.zeros(0, np.uint16)] * self.C
        self.pos = np.zeros(self.C, np.int64)
        self.out = [self._bucket() for _ in range(self.C)]
        self.pushes = 0

    @staticmethod
    def _bucket():
        return dict(segs=[], results=[], scores=[], mfcc=[], nbest=[], n_matched=[])

    def load(self, c, x):
        self.cur[c], self.pos[c] = np.ascontiguousarray(x, np.uint16), 0

    def remaining(self):
        return np.array([len(x) for x in self.cur], np.int64) - self.pos

    def push(self, want):
        cnt = np.minimum(np.asarray(want, np.int64), self.remaining()).astype(np.uint32)
        W = (int(cnt.max()) + 7) // 8 * 8
        chunk = np.full((self.C, W), 0xFFFF, np.uint16)  # what is not input is loud: a sample read too far would show
        for c in range(self.C):
            chunk[c, :cnt[c]] = self.cur[c][self.pos[c]:self.pos[c] + cnt[c]]
        self.pos += cnt
        o = self.sess.push(chunk, cnt, n_best=self.n_best if self.recognize else None, recognize=self.recognize)
        self.pushes += 1
        segs = o["segs"]
        assert o["total"] == len(segs)
        key = segs["channel"].astype(np.int64) << 40 | segs["start"]
        assert np.all(np.diff(key) > 0), "ascending channel, then ascending start"
        for i, g in enumerate(segs):
            b = self.out[int(g["channel"])]
            b["segs"].append(g.copy())
            if self.recognize:
                for k in KEYS:
                    b[k].append(o[k][i].copy())
        return o

    def drive(self, sizes):
        """sizes(push index) -> requested counts [C]; until every loaded recording is used up"""
        while np.any(self.remaining() > 0):
            self.push(sizes(self.pushes))

    def take(self, c):
        b, self.out[c] = self.out[c], self._bucket()
        return b


def check_channel(bucket, ended, ref, b, orc=None, x=None, atap=None, recognize=True):
    """what channel emitted (bucket) and its end record (or None) against recording b of the one-shot output ref"""
    off, segs = ref["seg_offsets"], ref["segs"]
    want = segs[off[b]:off[b + 1]]
    n_open = int(len(want) > 0 and want[-1]["end"] < 0)
    closed = want[:len(want) - n_open]
    assert np.all(closed["end"] >= 0)
    got = np.array(bucket["segs"], LIVE_SEG_DTYPE) if bucket["segs"] else np.zeros(0, LIVE_SEG_DTYPE)
    assert len(got) == len(closed), (b, len(got), len(closed))
    for f in ("start", "end", "frm_num"):
        assert np.array_equal(got[f], closed[f].astype(got[f].dtype)), (b, f)
    if n_open:
        assert ended is not None and (ended["start"], ended["end"], ended["frm_num"]) == (want[-1]["start"], -1, 0), b
    else:
        assert ended is None, (b, ended)
    if orc is not None:  # the unbounded oracle VAD directly
        oseg, _ = oracle_segments(orc, x, None if atap is None else ol.Atap(*[int(v) for v in atap]))
        mine = [(int(g["start"]), int(g["end"])) for g in got] + ([(int(ended["start"]), -1)] if ended is not None else [])
        assert mine == [tuple(int(v) for v in r) for r in oseg], b
    if recognize and len(got):
        lo = int(off[b])
        for k in KEYS:
            mine = np.stack(bucket[k])
            assert mine.tobytes() == np.ascontiguousarray(ref[k][lo:lo + len(got)]).tobytes(), (b, k)
    return len(got)


def check_all(feeder, ended, ref, recs, orc=None, ataps=None, recognize=True):
    by_ch = {int(g["channel"]): g for g in ended}
    assert len(by_ch) == len(ended)
    n = 0
    for c in range(len(recs)):
        n += check_channel(feeder.take(c), by_ch.get(c), ref, c, orc, recs[c], None if ataps is None else ataps[c], recognize)
    return n


@functools.lru_cache(maxsize=None)
def ragged_case():
    """8 ragged recordings of 10-25 s, an engine with 8 random templates, the one-shot reference (computed once)"""
    rng = np.random.default_rng(31)
    bank = synth.word_bank(12)
    recs = [make_recording(rng, bank, int(n)) for n in rng.integers(10 * 8000, 25 * 8000, 8)]
    recs[3] = recs[3][:len(recs[3]) - 1 + len(recs[3]) % 2]  # an odd length
    eng = Engine(testing=True)
    random_templates(eng, np.random.default_rng(32))
    ref = one_shot(eng, recs)
    assert ref["total"] > 8 * 6 and np.count_nonzero(ref["results"]["status"] == ST_OK) > 8 * 3
    return eng, recs, ref, ol.Oracle(max_seg=1 << 16)


# ---- GPU 1: any chunking equals one shot ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fixed800", "fixed80", "fixed81", "random"])
def test_any_chunking_equals_one_shot(mode):
    eng, recs, ref, orc = ragged_case()
    rng = np.random.default_rng(33)
    sizes = {"fixed800": lambda k: np.full(8, 800), "fixed80": lambda k: np.full(8, 80), "fixed81": lambda k: np.full(8, 81),
             "random": lambda k: rng.integers(0, 801, 8) * (rng.random(8) > 0.1)}[mode]  # zeros, odd counts, non-multiples of 8
    sess = eng.live(8, 800)
    try:
        f = Feeder(sess)
        for c, x in enumerate(recs):
            f.load(c, x)
        f.drive(sizes)
        ended = sess.end(np.arange(8))
        n = check_all(f, ended, ref, recs, orc if mode == "random" else None)
        assert n > 8 * 6
    finally:
        sess.close()


# ---- GPU 2: single-sample pushes --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_sample_pushes_over_a_whole_word():
    eng, recs, _, orc = ragged_case()
    recs = [spaced_words(21, synth.word_bank(12), 30000, lo=12, hi=28), recs[1][:30000]]
    ref = one_shot(eng, recs)
    x = recs[0]
    off, segs = ref["seg_offsets"], ref["segs"]
    mine = segs[off[0]:off[1]]
    ok = [g for g in mine if g["frm_num"] and g["end"] - g["start"] < 2400 and g["start"] > 4000]
    assert ok, "a short word"
    lo = int(ok[0]["start"]) - 500  # the 4 000-sample stretch [lo, lo + 4000) holds the word, its START and END events
    assert ok[0]["end"] + 11 * 80 + 160 < lo + 4000
    sess = eng.live(2, 800)
    try:
        f = Feeder(sess)
        f.load(0, x)
        f.load(1, recs[1])  # a second channel in ordinary chunks until the stretch
        while f.pos[0] < lo:
            f.push([min(800, lo - f.pos[0]), 800])
        for _ in range(4000):
            f.push([1, 0])
        f.drive(lambda k: np.full(2, 800))
        ended = sess.end([0, 1])
        assert check_all(f, ended, ref, recs, orc) >= 4
    finally:
        sess.close()


# ---- GPU 3: chunk edges against events ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constructed():
    recs, ats = constructed_cases(64)
    eng = Engine(testing=True)
    random_templates(eng, np.random.default_rng(41))
    at = np.array(ats, ATAP_DTYPE)
    ref = one_shot(eng, recs, atap=at)
    return eng, recs, ats, at, ref, ol.Oracle(max_seg=1 << 16)


@pytest.mark.gpu
def test_chunk_edges_at_start_and_end_events():
    eng, recs, ats, at, ref, orc = constructed()
    hop, fl, vd, sd = 80, 160, 8, 11
    b = 9  # active runs of 10 frames
    off, segs = ref["seg_offsets"], ref["segs"]
    first = segs[off[b]]
    j_start = int(first["start"]) // hop + vd - 1          # VAD.C:178
    j_end = (int(first["end"]) - fl) // hop + sd           # VAD.C:201
    edges = sorted({j * hop + fl + d for j0 in (j_start, j_end) for j in (j0 - 1, j0, j0 + 1) for d in (-1, 0, 1)})
    assert len(edges) == 18 and edges[-1] < len(recs[b])
    # every edge alone, one channel each: the first push ends exactly there; and one channel with every edge in turn
    C = len(edges) + 1
    one = one_shot(eng, [recs[b]] * C, atap=np.array([ats[b]] * C, ATAP_DTYPE))
    sess = eng.live(C, 8192, atap=np.array([ats[b]] * C, ATAP_DTYPE))
    try:
        f = Feeder(sess)
        for c in range(C):
            f.load(c, recs[b])
        f.push(edges + [edges[0]])
        for e0, e1 in zip(edges[:-1], edges[1:]):
            f.push([8192] * len(edges) + [e1 - e0])
        f.drive(lambda k: np.full(C, 8192))
        ended = sess.end(np.arange(C))
        assert check_all(f, ended, one, [recs[b]] * C, orc, [ats[b]] * C) == C * (off[b + 1] - off[b])
    finally:
        sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [800, 81])
def test_constructed_recordings_in_chunks(chunk):
    """every recording of constructed_cases on a channel of its own, thresholds handed in: the in-band stretch whose
    crossing class is carried over many pushes, loud from sample 0, a 200-frame segment, the four endings"""
    eng, recs, ats, at, ref, orc = constructed()
    C = len(recs)
    sess = eng.live(C, 800, atap=at)
    try:
        f = Feeder(sess)
        for c in range(C):
            f.load(c, recs[c])
        f.drive(lambda k: np.full(C, chunk))
        assert f.pushes > 3 * 64 * 80 // chunk  # the in-band stretch alone spans that many pushes
        out = [f.out[c] for c in range(C)]
        ended = sess.end(np.arange(C))
        by_ch = {int(g["channel"]): g for g in ended}
        check_all(f, ended, ref, recs, orc, ats)
    finally:
        sess.close()
    T = 64
    assert len(out[12]["segs"]) == 1 and out[12]["segs"][0]["start"] == 2400 + 5 * 80 + 80 * (3 * T + 5) - 80  # from the carried crossing
    # the four endings: silence and onset leave nothing open, speech and tail report {start, -1}
    assert 13 not in by_ch and 14 not in by_ch and len(out[13]["segs"]) == len(out[14]["segs"]) == 1
    for c in (15, 16):
        # the first loud frame is the one whose second half is loud, frame 69; the 8th opens the segment at (76 - 7) * 80
        assert by_ch[c]["end"] == -1 and by_ch[c]["frm_num"] == 0 and by_ch[c]["start"] == 2400 + 39 * 80
    g = out[17]["segs"][0]  # loud from the first sample
    assert g["start"] == 0 and g["frm_num"] == 0 and out[17]["results"][0]["status"] == ST_SEG_OOB
    assert out[17]["results"][0]["min_dis"] == DIS_ERR and not np.any(out[17]["mfcc"][0])
    s18 = out[18]["segs"]  # 200 frames, then a good one
    assert s18[0]["frm_num"] == 0 and s18[0]["end"] - s18[0]["start"] > 119 * 80 and s18[1]["frm_num"] > 0
    assert out[18]["results"][0]["status"] == ST_MFCC_FAIL and out[18]["results"][1]["status"] == ST_OK


# ---- GPU 4: ring wrap -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ring_wrap_words_straddle_multiples_of_the_ring_length():
    ring = engine.live_geometry(800)[0]
    assert ring == 11600
    bank = synth.word_bank(12)
    x = spaced_words(52, bank, 9 * ring + 1234, gap=1200)
    eng = Engine(testing=True)
    random_templates(eng, np.random.default_rng(53))
    ref = one_shot(eng, [x])
    segs = ref["segs"]
    ok = segs[ref["results"]["status"] == ST_OK]
    straddle = [k for k in range(1, 9) if np.any((ok["start"] - LEAD < k * ring) & (ok["end"] > k * ring))]
    assert len(straddle) >= 3, straddle  # recognised words whose samples wrap in the ring
    sess = eng.live(1, 800)
    try:
        f = Feeder(sess)
        f.load(0, x)
        f.drive(lambda k: [800])
        ended = sess.end([0])
        assert check_all(f, ended, ref, [x], ol.Oracle(max_seg=1 << 16)) >= 12
    finally:
        sess.close()


# ---- GPU 5: noise head ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_noise_head_in_pieces_and_in_one_push():
    eng, recs, ref, orc = ragged_case()
    x = spaced_words(55, synth.word_bank(12), 40000)
    one = one_shot(eng, [x, x])
    n_words = int(one["seg_offsets"][1])
    assert n_words >= 3 and one["segs"][2]["end"] > 0
    at = np.array([orc.noise_atap(x)[1].astuple()] * 2, ATAP_DTYPE)
    given = one_shot(eng, [x, x], atap=at)
    assert given["segs"].tobytes() == one["segs"].tobytes() and given["mfcc"].tobytes() == one["mfcc"].tobytes()
    # channel 0: the head in pieces smaller than a frame, then more small pieces; channel 1: everything in one push
    for atap in (None, at):
        sess = eng.live(2, 40000, atap=atap)
        try:
            f = Feeder(sess)
            f.load(0, x)
            f.load(1, x)
            assert sess.event_bound([0, 40000]) >= n_words
            o = f.push([0, 40000])
            assert o["total"] >= 3 and np.all(o["segs"]["channel"] == 1)
            for _ in range(30):
                if atap is None and f.pos[0] + 97 < 2400:
                    assert sess.event_bound([97, 0]) == 0  # nothing is consumed before the head is complete
                f.push([97, 0])
            f.drive(lambda k: [131, 0])
            ended = sess.end([0, 1])
            n_closed = int(np.count_nonzero(one["segs"]["end"] >= 0))
            assert check_all(f, ended, one, [x, x], orc, None if atap is None else at.tolist()) == n_closed
        finally:
            sess.close()


# ---- GPU 6: front ends ------------------------------------------------------------------------------------------------------
# name, engine / oracle keywords, word length scale, gap between words (samples: longer than the 110 ms tail), length scale,
# frame cap
FRONT_ENDS = [("reference", {}, {}, 1, 1600, 1, 119), ("extension", EXT, dict(fs=16000, nfft=512, n_mel=40), 2, 3200, 2, 119),
              ("generic", GEN[0], GEN[1], 1, 1600, 1, 119), ("most_states", MOST[0], MOST[1], 3, 10000, 2, 400)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ekw,okw,wscale,gap,lscale,R", FRONT_ENDS, ids=[f[0] for f in FRONT_ENDS])
def test_front_ends(name, ekw, okw, wscale, gap, lscale, R):
    rng = np.random.default_rng(61)
    bank = synth.word_bank(10)
    eng = Engine(max_frames=R, testing=True, **ekw)
    orc = ol.Oracle(max_frames=R, max_seg=1 << 16, **okw)
    random_templates(eng, rng)
    recs = [spaced_words(62 + i, bank, int(n), gap, wscale, hi=70)
            for i, n in enumerate(rng.integers(6 * 8000 * lscale, 9 * 8000 * lscale, 3))]
    ref = one_shot(eng, recs)
    assert np.count_nonzero(ref["results"]["status"] == ST_OK) >= 3
    cm = 1000 * lscale
    sess = eng.live(3, cm)
    try:
        f = Feeder(sess)
        for c in range(3):
            f.load(c, recs[c])
        f.drive(lambda k: rng.integers(0, cm + 1, 3))
        ended = sess.end([0, 1, 2])
        assert check_all(f, ended, ref, recs, orc) >= 3
    finally:
        sess.close()


# ---- GPU 7: capacity and errors ----------------------------------------------------------------------------------------------
class RawPush:
    """sr_live_push through ctypes with guarded outputs of `rows` rows"""

    def __init__(self, eng, rows, canary, n_best=3):
        K, R, nc = eng.n_templates, eng.max_frames, eng.n_coef
        mk = lambda name, shape, dt: guarded_out(shape, dt, canary, 4096, name=name)
        self.g = dict(segs=mk("segs", (rows,), LIVE_SEG_DTYPE), results=mk("results", (rows,), RESULT_DTYPE),
                      scores=mk("scores", (rows, K), np.uint32), mfcc=mk("mfcc", (rows, R, nc), np.int16),
                      nbest=mk("nbest", (rows, n_best), NBEST_DTYPE), n_matched=mk("n_matched", (rows,), np.uint32))
        self.total = C.c_uint32(0xFFFFFFFF)
        self.n_best = n_best

    def call(self, sess, chunk, cnt, max_segs, pcm=True, segs=True, nbest=True, n_best=None, n_all=0):
        p = lambda k, on=True: C.c_void_p(self.g[k].ptr) if on else None
        return sess.L.sr_live_push(sess.l, engine._vp(chunk) if pcm else None, C.c_uint64(chunk.shape[1]), engine._vp(cnt),
                                   C.c_uint32(n_all), C.c_uint32(max_segs), p("segs", segs),
                                   C.c_uint32(self.n_best if n_best is None else n_best), p("nbest", nbest), p("n_matched"),
                                   p("results"), p("scores"), p("mfcc"), C.byref(self.total))

    def untouched(self):
        for g in self.g.values():
            g.check_untouched()
        assert self.total.value == 0xFFFFFFFF


@pytest.mark.gpu
def test_capacity_and_bad_arguments_change_nothing():
    eng, recs, ref, orc = ragged_case()
    xs = [recs[4][:60000], recs[5][:60000]]
    one = one_shot(eng, xs)
    sess = eng.live(2, 800)
    try:
        pos, rows = 0, []
        refused = 0
        while pos < 60000:
            chunk = np.ascontiguousarray(np.stack([x[pos:pos + 800] for x in xs]))
            cnt = np.array([800, 800], np.uint32)
            bound = sess.event_bound(cnt)
            assert bound <= 2 * 2
            for canary in (0xA5, 0x3C) if pos in (8000, 24000) else (0xA5,):
                raw = RawPush(eng, bound + 3, canary)
                if bound:  # one below the bound: refused, nothing written, no state changed
                    assert raw.call(sess, chunk, cnt, bound - 1) == BAD_ARG
                    raw.untouched()
                    refused += 1
                if pos == 8000:  # bad arguments
                    big = np.array([800, 801], np.uint32)
                    assert raw.call(sess, chunk, big, bound + 3) == BAD_ARG                      # a count above chunk_max
                    assert raw.call(sess, chunk, None, bound + 3, n_all=801) == BAD_ARG
                    assert raw.call(sess, chunk, cnt, bound + 3, pcm=False) == BAD_ARG            # null required pointers
                    assert raw.call(sess, chunk, cnt, bound + 3, segs=False) == BAD_ARG
                    assert raw.call(sess, chunk, cnt, bound + 3, nbest=False) == BAD_ARG
                    assert raw.call(sess, chunk, cnt, bound + 3, n_best=17) == BAD_ARG            # n_best out of range
                    assert sess.L.sr_live_push(None, engine._vp(chunk), C.c_uint64(800), engine._vp(cnt), C.c_uint32(0),
                                               C.c_uint32(8), C.c_void_p(raw.g["segs"].ptr), C.c_uint32(0), None, None, None,
                                               None, None, None) == BAD_ARG
                    raw.untouched()
                    seg1 = np.zeros(2, LIVE_SEG_DTYPE)
                    n = C.c_uint32(77)
                    for bad in ([0, 2], [5]):  # a channel index past the end
                        ch = np.array(bad, np.uint32)
                        assert sess.L.sr_live_end(sess.l, engine._vp(ch), C.c_uint32(len(ch)), engine._vp(seg1), C.byref(n)) == BAD_ARG
                    assert n.value == 77 and not seg1.view(np.uint8).any()
            # the same push with enough room
            assert raw.call(sess, chunk, cnt, bound + 3) == 0
            t = raw.total.value
            assert t <= bound
            for k, g in raw.g.items():  # nothing past `total` rows
                g.check()
                body = g.interior()
                assert np.all(body[t:].view(np.uint8) == g.canary), k
                if t:
                    rows.append((k, body[:t].copy()))
            pos += 800
        assert refused > 40
        ended = sess.end([0, 1])
    finally:
        sess.close()
    # what the accepted pushes wrote, per channel in order of emission, is the one-shot output
    segs = np.concatenate([r for k, r in rows if k == "segs"])
    off = one["seg_offsets"]
    by_ch = {int(g["channel"]): g for g in ended}
    for c in (0, 1):
        sel = segs["channel"] == c
        want = one["segs"][off[c]:off[c + 1]]
        n_open = int(len(want) > 0 and want[-1]["end"] < 0)
        assert (c in by_ch) == bool(n_open)
        closed = want[:len(want) - n_open]
        assert np.array_equal(segs["start"][sel], closed["start"]) and np.array_equal(segs["end"][sel], closed["end"])
        for k in KEYS:
            mine = np.concatenate([r for kk, r in rows if kk == k])[sel]
            assert mine.tobytes() == np.ascontiguousarray(one[k][off[c]:off[c] + len(closed)]).tobytes(), (c, k)


@pytest.mark.gpu
def test_recognition_without_templates_is_refused():
    eng = Engine(testing=True)
    sess = eng.live(1, 800)
    try:
        x = np.full((1, 800), 2048, np.uint16)
        with pytest.raises(engine.SrError, match="error 4"):
            sess.push(x)
        o = sess.push(x, recognize=False)  # segmentation only needs no store
        assert o["total"] == 0
    finally:
        sess.close()


# ---- GPU 8: the device form on a side stream ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_form_on_side_stream_equals_host_form():
    eng, recs, ref, orc = ragged_case()
    xs = [recs[6][:64000], recs[7][:64000], recs[0][:64000]]
    rng = np.random.default_rng(81)
    plan = []
    pos = np.zeros(3, np.int64)
    while np.any(pos < 64000):
        cnt = np.minimum(rng.integers(0, 801, 3), 64000 - pos).astype(np.uint32)
        plan.append((pos.copy(), cnt))
        pos += cnt
    # host form
    sess = eng.live(3, 800)
    host = []
    try:
        for p, cnt in plan:
            chunk = np.full((3, 800), 0xFFFF, np.uint16)
            for c in range(3):
                chunk[c, :cnt[c]] = xs[c][p[c]:p[c] + cnt[c]]
            host.append(sess.push(chunk, cnt, n_best=3))
        host_end = sess.end([0, 1, 2])
    finally:
        sess.close()
    assert sum(o["total"] for o in host) > 5
    # device form: upload, push and read-back all queued on the side stream, no host sync between pushes
    sess = eng.live(3, 800)
    side = torch.cuda.Stream()
    got = []
    try:
        with torch.cuda.stream(side):
            for p, cnt in plan:
                chunk = np.full((3, 800), 0xFFFF, np.uint16)
                for c in range(3):
                    chunk[c, :cnt[c]] = xs[c][p[c]:p[c] + cnt[c]]
                x = torch.from_numpy(chunk.view(np.int16)).cuda()
                bound = sess.event_bound(cnt)
                o = sess.push_dev(x, cnt, n_best=3, max_segs=bound + 2, stream=side)
                got.append(o)
        side.synchronize()
        got = [{k: v.cpu() for k, v in o.items()} for o in got]
        dev_end = sess.end([0, 1, 2])
    finally:
        sess.close()
    assert dev_end.tobytes() == host_end.tobytes()
    for h, d in zip(host, got):
        t = h["total"]
        assert int(d["count"][0]) == t
        assert engine.live_segs_from_torch(d["segs"][:t]).tobytes() == h["segs"].tobytes()
        r = d["results"].numpy().view(np.uint32).reshape(-1, 4).copy().view(RESULT_DTYPE).reshape(-1)
        nb = d["nbest"].numpy().view(np.uint32).reshape(-1, 4).copy().view(NBEST_DTYPE).reshape(len(r), 3)
        assert r[:t].tobytes() == h["results"].tobytes() and nb[:t].tobytes() == h["nbest"].tobytes()
        assert d["scores"][:t].numpy().tobytes() == h["scores"].tobytes() and d["mfcc"][:t].numpy().tobytes() == h["mfcc"].tobytes()
        assert np.array_equal(d["n_matched"][:t].numpy().view(np.uint32), h["n_matched"])
        # padding slots: failed records, as sr_recognize_stream_nbest_dev pads them
        assert len(r) >= t + 2
        assert np.all(r[t:]["status"] == ST_VAD_FAIL) and np.all(r[t:]["min_dis"] == DIS_ERR) and np.all(r[t:]["frm_num"] == 0)
        assert not d["mfcc"][t:].numpy().any() and np.all(d["scores"][t:].numpy().view(np.uint32) == DIS_ERR)
        assert np.all(nb[t:]["word"] == NO_WORD) and np.all(nb[t:]["dis"] == DIS_ERR) and np.all(nb[t:]["count"] == 0)
        assert not d["n_matched"][t:].numpy().any()


# ---- GPU 9: end and reuse ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_and_reuse_leave_other_channels_alone():
    eng, recs, ref, orc = ragged_case()
    a, b = recs[1][:50000], recs[2][:44444]
    long = recs[3][:100001]
    late = recs[4][:40000]
    # a ends inside a segment when cut in the middle of a word: look for such a cut in the one-shot segments of recs[1]
    off, segs = ref["seg_offsets"], ref["segs"]
    mid = [g for g in segs[off[1]:off[2]] if g["end"] - g["start"] > 2400 and 20000 < g["start"] < 50000]
    assert mid
    a = recs[1][:int(mid[0]["start"]) + 1600]
    one = one_shot(eng, [a, b, long, late])
    assert one["segs"][one["seg_offsets"][1] - 1]["end"] == -1  # recording a ends inside a segment
    sess = eng.live(3, 800)
    try:
        f = Feeder(sess)
        f.load(0, a)
        f.load(1, long)
        while f.remaining()[0] > 0:  # channel 2 silent all along
            f.push([777, 800, 0])
        e = sess.end([0])
        assert len(e) == 1 and e[0]["channel"] == 0
        check_channel(f.take(0), e[0], one, 0, orc, a)
        f.load(0, b)       # channel 0 reused: as freshly opened, thresholds from ITS head
        f.load(2, late)    # channel 2 wakes up
        f.drive(lambda k: [799 - 2 * (k % 3), 800, 640])
        e = sess.end([2, 0, 1])
        by_ch = {int(g["channel"]): g for g in e}
        check_channel(f.take(0), by_ch.get(0), one, 1, orc, b)
        check_channel(f.take(1), by_ch.get(1), one, 2, orc, long)
        check_channel(f.take(2), by_ch.get(2), one, 3, orc, late)
        assert len(sess.end([0, 1, 2])) == 0  # freshly opened channels have nothing open
    finally:
        sess.close()
