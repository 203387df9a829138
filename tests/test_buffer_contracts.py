"""Buffer contracts of the C ABI (include/sr_engine.h): strides, base offsets, padding and output extents.

The value tests hand every entry point densely packed rows (pcm_stride == buf_len) and exactly sized, zero-filled outputs.
Here the library is called through ctypes directly, so the layout is the test's to choose:

Front ends: the reference's, the 16 kHz extension, the GENERIC frame kernel at the firmware's framing (13 coefficients) and at
32 / 16 ms framing (k_vad_gen, 10 coefficients).

  inputs   capture rows at pcm_stride > buf_len and at a base offset into a larger allocation, everything that is not
           rows[b][:buf_len] POISON (alternating 0 / 4095, or 0xFFFF words); feature records whose rows >= frames[b] are
           alternating +32767 / -32768.  The CPU oracle sees only the bytes the contract calls inputs.
  outputs  every output pointer is the interior of a canary-filled allocation with a guard of at least one whole record
           (and 4 KiB) on both sides (tests/guarded.py).  After the call both guards are intact and the interior equals the
           oracle byte for byte -- rows >= frm_num, whole records of failed rows and sr_vad_rec._pad (written as 0 by every
           VAD form) included -- once with each of two canaries.

Decisions this file pins:
  * host buffers need only the natural 2-byte alignment of their u16 samples; any pcm_stride >= buf_len, odd ones included;
  * the walk of dtw() reads row frames[b] of a record only when frames[b] == 1 (the first pass of the do-while of DTW.C:150-188
    evaluates point (2, 2) before the loop condition is tested); for longer sequences x < in_frames holds wherever a row is
    fetched.  Row 1 of a one-frame record lies inside the record (max_frames >= 2), so the oracle is given the record as the
    device sees it, poison rows included, and a ZERO row after it: no score may depend on memory past a record;
  * a device d_vad record with status != 0 is a failed record whatever frm_num it carries: scores SR_DIS_ERR, and the slot
    scan passes status and frm_num through.

Special rows of every batch of seven rows or more: a segment from sample 0 (SR_ST_SEG_OOB), a silent row, a segment longer
than max_frames, three segments, an onset one frame short of a segment when the buffer ends (one frame read past buf_len
would start one: the VAD's output is otherwise blind to up to seven extra frames), and speech through the last real sample.
B = 5 holds five of them (no over-long segment), B = 1 is one ordinary word.  A VAD segment always starts on a multiple of the
hop, so "starts at sample 1" exists only for the entry points that take explicit segments (sr_mfcc_batch_status,
sr_frame_features_batch), where it is the first record of every call.

Wall time on one MI355X, measured in one session: this module 18 s (58 tests, 17 s inside pytest); the -m gpu suite without
it 170 s (220 tests), at the parent commit and with this change alike.  With the four cases at the capacity edge of the pinned
staging area (16 / 17 capture rows, 283 / 284 feature records): 62 tests, 15 to 17 s.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import oracle_lib as ol
from guarded import CANARIES, _dtw_all_modes, guarded_out, padded_rows, poison_feature_rows
from stm32_speech_recognition_amd import synth
from stm32_speech_recognition_amd.engine import (ATAP_DTYPE, DIS_ERR, FEAT_FFT, FEAT_LOGMEL, FEAT_MAG, FEAT_MEL, RESULT_DTYPE,
                                                 ST_MFCC_FAIL, ST_OK, ST_SEG_OOB, ST_VAD_FAIL, STREAM_SEG_DTYPE, VAD_DTYPE,
                                                 Engine, pack12)
from test_frame_features import log100, mag_from_words, mel_from_mag, windowed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R = 48          # max_frames of every engine here
T_BUF = 60      # the capture length holds a 60-frame word, so one row can exceed R
THREADS = 16    # host threads of the oracle
EXT = dict(fs=16000, nfft=512, n_mel=40)
# "gen": the GENERIC frame kernel at the firmware's framing, 13 coefficients; "gen32": 32 / 16 ms framing (256 / 128 samples, the
# VAD kernel of the other framings, k_vad_gen), a 480 ms noise head, 20 filters, 10 coefficients
FRONTS = {"ref": ({}, {}, 1), "ext": (EXT, EXT, 2), "gen": ol.GENERIC_CONFIGS[0] + (1,), "gen32": ol.GENERIC_CONFIGS[2] + (1,)}
KINDS = (FEAT_FFT, FEAT_MAG, FEAT_MEL, FEAT_LOGMEL)
P, U32, U64, I32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int

# (B, buf_len - base, pcm_stride - round_up(buf_len, 8), lead, small-launch mode, poison, side stream): every B, buf_len
# offset, stride, lead, mode, poison and stream at least once per front end
DEV_CASES = [(1, 0, 0, 0, 0, "adc", False), (5, -1, 8, 8, 1, "ffff", True), (63, -3, 4104, 4104, 2, "adc", True),
             (65, -7, 0, 8, 3, "ffff", False), (1023, 5, 8, 4104, 0, "adc", False), (1025, -1, 4104, 0, 1, "ffff", True)]
# host forms: (B, buf_len - base, pcm_stride - buf_len, lead, mode, poison); odd strides, 2-byte aligned bases.  B = 16 / 17 at
# buf_len = base = 9 680: rows of 19 360 bytes, the most that fit the 327 680 bytes of the pinned staging area's upload part
# (sr_mfcc_batch_status adds a 48-byte record per row: 16 x 19 408 + 128 = 310 656) and the first batch that does not
HOST_CASES = {"ref": [(5, -1, 1, 1, 0, "adc"), (65, 5, 4105, 1, 1, "ffff"), (1025, -7, 3, 0, 0, "adc"),
                      (16, 0, 1, 1, 0, "adc"), (17, 0, 1, 1, 0, "ffff")],
              "ext": [(5, -3, 9, 1, 1, "ffff"), (63, 0, 1, 3, 0, "adc")],
              "gen": [(1, -7, 0, 1, 0, "adc"), (65, -1, 7, 5, 2, "ffff")],
              "gen32": [(5, 5, 3, 1, 1, "adc"), (63, -3, 1, 0, 0, "ffff")]}


class Ctx:
    def __init__(self, front):
        ekw, okw, self.rate = FRONTS[front]
        self.front = front
        self.eng = Engine(max_frames=R, device=0, **ekw)
        self.orc = ol.Oracle(max_frames=R, **okw)
        self.orc_many = ol.Oracle(max_frames=R, max_seg=64, **okw)  # the stream VAD: no bound on the segment count
        self.nc, self.fl, self.hop = self.orc.n_coef, self.orc.frame_len, self.orc.hop
        self.orc.v_durmin = 80 // (self.orc.cfg.frame_time - self.orc.cfg.frame_mov_t)  # VAD.C:72: frames that make an onset
        rng = np.random.default_rng(17)
        self.tf = np.array([24, 30, 36, 44, 17, 48, 20, 1, 2], np.uint32)  # 1 and 2 frames: the walk reads a slack row
        self.valid = np.ones(len(self.tf), np.uint8)
        self.valid[4] = 0
        self.K = len(self.tf)
        self.tm = np.zeros((self.K, R + 1, self.nc), np.int16)
        for k in range(self.K):
            self.tm[k, :self.tf[k]] = rng.integers(-900, 900, (self.tf[k], self.nc))
        self.set_default_store()
        # captures: noise head | 880 quiet samples (x rate) | up to 60 hops of speech | 20 hops of quiet, a multiple of 8 and
        # of the hop (the generator's own length for a 60-frame word at the firmware's framing)
        self.head = self.orc.noise_len
        self.p0 = self.head + 880 * self.rate
        step = int(np.lcm(8, self.hop))
        self.base = -(-(self.p0 + (T_BUF + 20) * self.hop) // step) * step
        assert self.base % 8 == 0 and self.base % self.hop == 0
        assert front not in ("ref", "ext") or self.base == synth.buf_len_for(T_BUF, self.rate)
        # generator frame counts (its frames are 160 / 80 samples x rate) whose segments have about 21..43 frames here
        unit = 80 * self.rate
        self.t_lo = (19 * self.hop + self.fl - 2 * unit) // unit + 4
        self.t_hi = (43 * self.hop + self.fl - 2 * unit) // unit - 1

    def set_default_store(self):
        self.eng.set_templates_dense(self.tm, self.tf, self.valid)
        self.tpl = self.orc.make_templates(self.tm, self.tf, self.valid)


@pytest.fixture(scope="module")
def fronts():
    made = {}

    def get(front):
        if front not in made:
            made[front] = Ctx(front)
        return made[front]
    yield get
    for c in made.values():
        c.eng.close()


def call(eng, fn, *args):
    rc = getattr(eng.L, fn)(eng.h, *args)
    assert rc == 0, (fn, rc, eng.L.sr_last_error().decode())


def frm_status(st, en, fl, hop):
    if en < 0:
        return 0, ST_VAD_FAIL
    if st < 1:
        return 0, ST_SEG_OOB
    n = ((((en - st) & 0xFFFFFFFF) - fl) // hop + 1) & 0xFFFF
    return (0, ST_MFCC_FAIL) if n > R else (n, ST_OK)


# ---- captures ----------------------------------------------------------------------------------------------------------------
def tone(x, a, b, amp=700.0):
    t = np.arange(b - a)
    x[a:b] = np.clip(np.round(2048 + amp * np.sin(2 * np.pi * 0.11 * t)), 0, 4095).astype(np.uint16)


def make_batch(c, B, buf_len, seed):
    """uint16 [B, buf_len]: synthetic words of about 21..43 frames and the special rows (module docstring)"""
    rate, hop, fl = c.rate, c.hop, c.fl
    rng = np.random.default_rng(seed)
    bank = synth.word_bank(6)
    p0, head = c.p0, c.head
    extra = head - 2400 * rate  # a noise head longer than the generator's 300 ms: more of the same noise in front
    rows = synth.as_u16_numpy(synth.make_utterances(rng.integers(0, 6, B), rng.integers(c.t_lo, c.t_hi + 1, B), seed=seed,
                                                    bank=bank, S=buf_len - extra, rate=rate))
    front_noise = np.clip(np.round(2048 + rng.normal(0, 8, (B, extra))), 0, 4095).astype(np.uint16)
    rows = np.ascontiguousarray(np.concatenate([front_noise, rows], 1))

    def quiet():
        x = 2048 + rng.normal(0, 4, buf_len)
        x[:head] = 2048 + rng.normal(0, 8, head)
        return np.clip(np.round(x), 0, 4095).astype(np.uint16)

    if B >= 5:
        x = quiet()  # speech from sample 0 on: the segment starts at sample 0 (SR_ST_SEG_OOB); the lead poison lies before it
        tone(x, 0, fl + 12 * hop)
        rows[0] = x
        rows[1] = 2048  # silent (SR_ST_VAD_FAIL)
        x = quiet()  # 60 frames > max_frames (SR_ST_MFCC_FAIL)
        tone(x, p0, p0 + 59 * hop)
        rows[2] = x
        x = quiet()  # three segments (max_seg)
        for i in range(3):
            tone(x, p0 + i * 28 * hop, p0 + i * 28 * hop + 11 * hop)
        rows[3] = x
        x = quiet()  # speech through the last real sample: the segment is still open at buf_len
        tone(x, p0, buf_len)
        rows[B - 1] = x
        # an onset ONE frame short of a segment when the buffer ends (VAD.C:173-181 needs 8 loud frames): loud from the seventh
        # frame before the last on -- no segment, but one frame read past buf_len (the poison is loud) would start one
        x = quiet()
        last = (buf_len - fl - 1) // hop * hop  # first sample of the last frame of VAD.C:121's loop
        tone(x, last - (c.orc.v_durmin - 2) * hop + hop, buf_len)
        rows[4 if B >= 7 else 2] = x
    return rows


def expected(c, rows):
    """the oracle on rows[b][:buf_len] only: (vad records, results, mfcc, scores)"""
    orc, B = c.orc, len(rows)
    vd = np.zeros(B, VAD_DTYPE)
    for b in range(B):
        rc, a = orc.noise_atap(rows[b])
        assert rc == 0
        seg = orc.vad(rows[b], a)
        vd[b]["mid_val"], vd[b]["n_thl"], vd[b]["z_thl"], vd[b]["s_thl"] = a.astuple()
        vd[b]["seg"] = seg
        vd[b]["frm_num"], vd[b]["status"] = frm_status(int(seg[0]), int(seg[1]), c.fl, c.hop)
    res, mf, sc = orc.recognize_batch(rows, c.tpl, n_threads=THREADS)
    assert np.array_equal(res["status"], vd["status"]) and np.array_equal(res["frm_num"], vd["frm_num"])
    if B >= 5:
        assert vd["status"][[0, 1, B - 1]].tolist() == [ST_SEG_OOB, ST_VAD_FAIL, ST_VAD_FAIL]
        assert vd["seg"][0, 0] == 0 and vd["seg"][B - 1, 0] > 0 and vd["seg"][B - 1, 1] == -1 and (vd["seg"][3] >= 0).all()
        assert vd["status"][2] == ST_MFCC_FAIL or B == 5
        b = 4 if B >= 7 else 2  # the onset row: no segment, and one more (loud) frame would have started one
        assert (vd["seg"][b] == -1).all()
        more = np.concatenate([rows[b], np.resize(np.array([4095, 0], np.uint16), c.hop)])
        assert orc.vad(more, ol.Atap(*[int(vd[b][f]) for f in ("mid_val", "n_thl", "z_thl", "s_thl")]))[0] > 0
    if B >= 63:  # the MFCC / DTW comparison is never vacuous
        assert ((vd["status"] == ST_OK) & (vd["frm_num"] >= 20)).sum() >= 0.8 * B
    elif B == 1:
        assert vd["status"][0] == ST_OK and vd["frm_num"][0] >= 20
    return vd, res.view(RESULT_DTYPE), mf, sc


def expected_segments(c, rows):
    ms, B = c.orc.cfg.max_seg, len(rows)
    res, sc = np.zeros((ms, B), RESULT_DTYPE), np.zeros((ms, B, c.K), np.uint32)
    for b in range(B):
        r, s = c.orc.recognize_segments(rows[b], c.tpl)
        res[:, b], sc[:, b] = r, s
    return res, sc


def expected_features(c, rows, st, en, mid, ok):
    """{kind: u32 [B, R, width]} for explicit segments; FFT: None (held to MAG through mag_from_words)"""
    orc, B = c.orc, len(rows)
    tab = orc.tables()
    nb, nm = orc.cfg.nfft // 2, orc.n_mel
    out = {FEAT_MAG: np.zeros((B, R, nb), np.uint32), FEAT_MEL: np.zeros((B, R, nm), np.uint32),
           FEAT_LOGMEL: np.zeros((B, R, nm), np.uint32)}
    for b in range(B):
        if not ok[b]:
            continue
        n = frm_status(int(st[b]), int(en[b]), c.fl, c.hop)[0]
        fr = windowed(rows[b], int(st[b]), n, c.fl, c.hop, int(mid[b]), tab["hamm"])
        mag = np.stack([orc.fft_mag(f) for f in fr])
        mel, _ = mel_from_mag(mag, tab)
        out[FEAT_MAG][b, :n], out[FEAT_MEL][b, :n] = mag, mel
        out[FEAT_LOGMEL][b, :n] = log100(orc, mel).reshape(n, nm)
    return out


def check_fft_words(g, want_mag):
    """FFT words have no CPU oracle of their own: guards, zero rows and |X|*10 of the words (MFCC.C:49-60) against MAG"""
    g.check()
    got = g.interior()
    zero = ~want_mag.any(axis=2)
    assert not got[zero].any(), f"buffer {g.name}: rows >= frm_num / failed records not zero"
    assert np.array_equal(mag_from_words(got.reshape(-1, got.shape[2])).reshape(got.shape)[~zero], want_mag[~zero]), g.name


def to_dev(flat_u16, lead):
    t = torch.from_numpy(flat_u16.view(np.int16)).to(DEV)
    ptr = t.data_ptr() + 2 * lead
    assert ptr % 16 == 0
    return t, ptr


def stream_of(side):
    s = torch.cuda.Stream(device=DEV) if side else None
    return s, (s.cuda_stream if side else 0)


def G(name, shape, dtype, canary, rec_bytes, device=DEV):
    return guarded_out(shape, dtype, canary, rec_bytes, device, name)


# ---- device forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEV_CASES, ids=lambda v: "B%d_d%d_s%d_l%d_m%d_%s_%s" % (v[:6] + ("side" if v[6] else "null",)))
@pytest.mark.parametrize("front", list(FRONTS))
def test_device_entry_points_with_padded_rows_and_guarded_outputs(fronts, front, case):
    """sr_vad_batch_dev -> sr_mfcc_batch_dev -> sr_dtw_batch_dev on the guarded outputs of the stage before,
    sr_recognize_batch_dev with every subset of its optional outputs, sr_recognize_segments_batch_dev and (B <= 65)
    sr_frame_features_batch_dev in all four kinds"""
    c = fronts(front)
    B, d, extra, lead, mode, poison, side = case
    eng, nc, K = c.eng, c.nc, c.K
    buf_len = c.base + d
    rows = make_batch(c, B, buf_len, seed=B + 7)
    stride = (buf_len + 7) // 8 * 8 + extra
    dpcm, ptr = to_dev(padded_rows(rows, stride, lead, 264, poison), lead)
    vd, res, mf, sc = expected(c, rows)
    sres, ssc = expected_segments(c, rows)
    okrow = vd["status"] == ST_OK
    feats = expected_features(c, rows, vd["seg"][:, 0], vd["seg"][:, 1], vd["mid_val"], okrow) if B <= 65 else None
    stream, sid = stream_of(side)
    eng.set_small_launch(mode)
    rec_m, ms = R * nc * 2, eng.cfg.max_seg
    try:
        for canary in CANARIES:
            torch.cuda.synchronize()
            g_vad = G("d_vad", (B,), VAD_DTYPE, canary, 48)
            g_mf = G("d_mfcc", (B, R, nc), np.int16, canary, rec_m)
            g_sc = G("d_scores", (B, K), np.uint32, canary, K * 4)
            g_res = G("d_results", (B,), RESULT_DTYPE, canary, 16)
            torch.cuda.synchronize()
            call(eng, "sr_vad_batch_dev", P(ptr), U64(stride), U32(buf_len), U32(B), P(g_vad.ptr), P(sid))
            call(eng, "sr_mfcc_batch_dev", P(ptr), U64(stride), U32(B), P(g_vad.ptr), P(g_mf.ptr), P(sid))
            call(eng, "sr_dtw_batch_dev", P(g_mf.ptr), P(g_vad.ptr), U32(B), P(g_sc.ptr), P(g_res.ptr), P(sid))
            torch.cuda.synchronize()
            g_vad.check_equals(vd)
            g_mf.check_equals(mf)
            g_sc.check_equals(sc)
            g_res.check_equals(res)
            # the whole path, every subset of the optional outputs NULL
            for want in itertools.product((True, False), repeat=3):
                outs = [G("d_results", (B,), RESULT_DTYPE, canary, 16),
                        G("d_scores", (B, K), np.uint32, canary, K * 4) if want[0] else None,
                        G("d_mfcc", (B, R, nc), np.int16, canary, rec_m) if want[1] else None,
                        G("d_vad", (B,), VAD_DTYPE, canary, 48) if want[2] else None]
                torch.cuda.synchronize()
                call(eng, "sr_recognize_batch_dev", P(ptr), U64(stride), U32(buf_len), U32(B),
                     *[P(g.ptr if g else None) for g in outs], P(sid))
                torch.cuda.synchronize()
                for g, w in zip(outs, (res, sc, mf, vd)):
                    if g:
                        g.check_equals(w)
            g_sres = G("d_results(segments)", (ms, B), RESULT_DTYPE, canary, 16 * B)
            g_ssc = G("d_scores(segments)", (ms, B, K), np.uint32, canary, B * K * 4)
            g_svad = G("d_vad(segments)", (B,), VAD_DTYPE, canary, 48)
            torch.cuda.synchronize()
            call(eng, "sr_recognize_segments_batch_dev", P(ptr), U64(stride), U32(buf_len), U32(B), P(g_sres.ptr),
                 P(g_ssc.ptr), P(g_svad.ptr), P(sid))
            torch.cuda.synchronize()
            g_sres.check_equals(sres)
            g_ssc.check_equals(ssc)
            g_svad.check_equals(vd)
            if feats is None:
                continue
            for kind in KINDS:
                w = eng.frame_feature_width(kind)
                g_ft = G("d_feat(kind %d)" % kind, (B, R, w), np.uint32, canary, R * w * 4)
                g_fm = G("d_mfcc(features)", (B, R, nc), np.int16, canary, rec_m)
                torch.cuda.synchronize()
                call(eng, "sr_frame_features_batch_dev", I32(kind), P(ptr), U64(stride), U32(B), P(g_vad.ptr), P(g_ft.ptr),
                     P(g_fm.ptr), P(sid))
                torch.cuda.synchronize()
                g_fm.check_equals(mf)
                if kind == FEAT_FFT:
                    check_fft_words(g_ft, feats[FEAT_MAG])
                else:
                    g_ft.check_equals(feats[kind])
            g_vad.check_equals(vd)  # an input of the later calls: unchanged
    finally:
        eng.set_small_launch(0)
    del dpcm, stream


@pytest.mark.parametrize("front,B,mode,lead,side", [("ref", 65, 0, 8, False), ("ref", 5, 1, 4104, True), ("ext", 65, 1, 8, True),
                                                   ("ext", 5, 2, 8, False), ("gen", 63, 0, 4104, True), ("gen", 5, 1, 8, False),
                                                   ("gen32", 65, 1, 8, True), ("gen32", 5, 0, 4104, False)])
def test_device_frame_kernels_with_caller_made_records(fronts, front, B, mode, lead, side):
    """sr_mfcc_batch_dev and sr_frame_features_batch_dev on d_vad records the CALLER wrote: a segment that starts at sample 1
    of row 0 (the pre-emphasis predecessor x[0] is the first sample of the allocation's first row: the lead poison lies
    right before it), one whose last frame ends on the last real sample of its row, failed records (frm_num 0, as
    include/sr_engine.h requires of caller-made records) whose segment fields still point outside the row; in the 64-, 16- and
    4-frame forms of the frame kernels"""
    c = fronts(front)
    eng, nc = c.eng, c.nc
    buf_len = c.base - 3
    stride = (buf_len + 7) // 8 * 8 + 8
    rows = make_batch(c, B, buf_len, seed=B + 13)
    vd = expected(c, rows)[0]
    st, en, mid, xn, xstatus, xmf = explicit_segments(c, rows, vd)
    recs = np.zeros(B, VAD_DTYPE)
    recs["seg"] = -1
    recs["mid_val"], recs["frm_num"], recs["status"] = mid, xn, xstatus
    recs["seg"][:, 0], recs["seg"][:, 1] = st, en
    bad = xstatus != 0  # failed records keep frm_num 0, as every VAD form writes them: the frame kernels take frm_num as given
    assert bad.sum() >= 3 and not recs["frm_num"][bad].any() and (recs["seg"][bad, 0] != 1).any()
    feats = expected_features(c, rows, st, en, mid, ~bad)
    dpcm, ptr = to_dev(padded_rows(rows, stride, lead, 264, "adc"), lead)
    stream, sid = stream_of(side)
    eng.set_small_launch(mode)
    try:
        for canary in CANARIES:
            g_rec = input_in_guards("d_vad(in)", recs, canary)
            g_mf = G("d_mfcc", (B, R, nc), np.int16, canary, R * nc * 2)
            torch.cuda.synchronize()
            call(eng, "sr_mfcc_batch_dev", P(ptr), U64(stride), U32(B), P(g_rec.ptr), P(g_mf.ptr), P(sid))
            torch.cuda.synchronize()
            g_mf.check_equals(xmf)
            for kind in KINDS:
                w = eng.frame_feature_width(kind)
                g_ft = G("d_feat(kind %d)" % kind, (B, R, w), np.uint32, canary, R * w * 4)
                g_fm = G("d_mfcc(features)", (B, R, nc), np.int16, canary, R * nc * 2) if kind != FEAT_MEL else None
                torch.cuda.synchronize()
                call(eng, "sr_frame_features_batch_dev", I32(kind), P(ptr), U64(stride), U32(B), P(g_rec.ptr), P(g_ft.ptr),
                     P(g_fm.ptr if g_fm else None), P(sid))
                torch.cuda.synchronize()
                if g_fm:
                    g_fm.check_equals(xmf)
                if kind == FEAT_FFT:
                    check_fft_words(g_ft, feats[FEAT_MAG])
                else:
                    g_ft.check_equals(feats[kind])
            g_rec.check_equals(recs)
    finally:
        eng.set_small_launch(0)
    del dpcm, stream


def test_chunked_pipeline_with_a_short_last_chunk(fronts):
    """sr_set_pipeline(h, 3, 64, 12) with B = 64 * 5 + 7: every chunk on an internal stream, the last one short; rows at a padded
    stride and base offset, outputs guarded"""
    c = fronts("ref")
    eng, nc, K = c.eng, c.nc, c.K
    B, buf_len, lead = 64 * 5 + 7, c.base - 3, 4104
    stride = c.base + 8
    rows = make_batch(c, B, buf_len, seed=5)
    dpcm, ptr = to_dev(padded_rows(rows, stride, lead, 264, "adc"), lead)
    vd, res, mf, sc = expected(c, rows)
    eng.set_pipeline(3, 64, 12)
    try:
        for canary, side in zip(CANARIES, (False, True)):
            stream, sid = stream_of(side)
            outs = [G("d_results", (B,), RESULT_DTYPE, canary, 16), G("d_scores", (B, K), np.uint32, canary, K * 4),
                    G("d_mfcc", (B, R, nc), np.int16, canary, R * nc * 2), G("d_vad", (B,), VAD_DTYPE, canary, 48)]
            torch.cuda.synchronize()
            call(eng, "sr_recognize_batch_dev", P(ptr), U64(stride), U32(buf_len), U32(B), *[P(g.ptr) for g in outs], P(sid))
            torch.cuda.synchronize()
            for g, w in zip(outs, (res, sc, mf, vd)):
                g.check_equals(w)
    finally:
        eng.set_pipeline()
    del dpcm


# ---- host forms ---------------------------------------------------------------------------------------------------------------
def explicit_segments(c, rows, vd):
    """segments for sr_mfcc_batch_status / sr_frame_features_batch: record 0 starts at sample 1, then the oracle's segment 0
    of every row, with bad records among them (start 0, end past buf_len, shorter than a frame, longer than max_frames)"""
    B, buf_len = rows.shape
    st, en, mid = vd["seg"][:, 0].astype(np.int32), vd["seg"][:, 1].astype(np.int32), vd["mid_val"].astype(np.uint32)
    st[0], en[0] = 1, 1 + c.fl + 10 * c.hop + 3
    if B >= 5:
        st[1], en[1] = 0, c.fl + 30 * c.hop
        st[2], en[2] = 200, 200 + c.fl + c.hop * R          # R + 1 frames
        st[3], en[3] = 100, 100 + c.fl - 1                  # shorter than a frame
        st[B - 1], en[B - 1] = buf_len - c.fl - 5, buf_len + 1  # ends past the buffer: must not reach the tail poison
    if B >= 63:
        st[5], en[5] = buf_len - c.fl - 3 * c.hop, buf_len  # the last frame ends on the last real sample
    status, n = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    mf = np.zeros((B, R, c.nc), np.int16)
    for b in range(B):
        if st[b] < 1 or en[b] > buf_len or en[b] < st[b]:
            status[b] = ST_SEG_OOB
        elif en[b] - st[b] < c.fl or (en[b] - st[b] - c.fl) // c.hop + 1 > R:
            status[b] = ST_MFCC_FAIL
        else:
            nn, m = c.orc.mfcc(rows[b], int(st[b]), int(en[b]), ol.Atap(int(mid[b]), 0, 0, 0))
            assert nn > 0
            n[b], mf[b, :nn] = nn, m
    assert status[0] == 0 and n[0] == 11
    return st, en, mid, n, status, mf


def H(name, shape, dtype, canary, rec_bytes):
    return guarded_out(shape, dtype, canary, rec_bytes, None, name)


@pytest.mark.parametrize("front,case", [(f, cs) for f in HOST_CASES for cs in HOST_CASES[f]],
                         ids=lambda v: v if isinstance(v, str) else "B%d_d%d_s%d_l%d_m%d_%s" % v)
def test_host_entry_points_with_odd_strides_and_two_byte_aligned_bases(fronts, front, case):
    """sr_vad_batch, sr_mfcc_batch_status, sr_frame_features_batch (B <= 65), sr_recognize_batch with every subset of its
    optional outputs, sr_recognize_segments_batch"""
    c = fronts(front)
    B, d, extra, lead, mode, poison = case
    eng, nc, K = c.eng, c.nc, c.K
    buf_len = c.base + d
    stride = buf_len + extra
    rows = make_batch(c, B, buf_len, seed=B + 11)
    flat = padded_rows(rows, stride, lead, 300, poison)
    ptr = flat.ctypes.data + 2 * lead
    assert ptr % 2 == 0 and (lead % 2 == 0 or ptr % 4 == 2)
    vd, res, mf, sc = expected(c, rows)
    sres, ssc = expected_segments(c, rows)
    st, en, mid, xn, xstatus, xmf = explicit_segments(c, rows, vd)
    feats = expected_features(c, rows, st, en, mid, xstatus == 0) if B <= 65 else None
    rec_m, ms = R * nc * 2, eng.cfg.max_seg
    eng.set_small_launch(mode)
    try:
        for canary in CANARIES:
            g_vad = H("vad", (B,), VAD_DTYPE, canary, 48)
            call(eng, "sr_vad_batch", P(ptr), U64(stride), U32(buf_len), U32(B), P(g_vad.ptr))
            g_vad.check_equals(vd)
            g_mf, g_n, g_st = H("mfcc", (B, R, nc), np.int16, canary, rec_m), H("frm_num", (B,), np.uint32, canary, 4), \
                H("status", (B,), np.uint32, canary, 4)
            call(eng, "sr_mfcc_batch_status", P(ptr), U64(stride), U32(buf_len), U32(B), P(st.ctypes.data), P(en.ctypes.data),
                 P(mid.ctypes.data), P(g_mf.ptr), P(g_n.ptr), P(g_st.ptr))
            g_mf.check_equals(xmf)
            g_n.check_equals(xn)
            g_st.check_equals(xstatus)
            for want in itertools.product((True, False), repeat=3):
                outs = [H("results", (B,), RESULT_DTYPE, canary, 16),
                        H("scores", (B, K), np.uint32, canary, K * 4) if want[0] else None,
                        H("mfcc", (B, R, nc), np.int16, canary, rec_m) if want[1] else None,
                        H("vad", (B,), VAD_DTYPE, canary, 48) if want[2] else None]
                call(eng, "sr_recognize_batch", P(ptr), U64(stride), U32(buf_len), U32(B), *[P(g.ptr if g else None) for g in outs])
                for g, w in zip(outs, (res, sc, mf, vd)):
                    if g:
                        g.check_equals(w)
            g_sres = H("results(segments)", (ms, B), RESULT_DTYPE, canary, 16 * B)
            g_ssc = H("scores(segments)", (ms, B, K), np.uint32, canary, B * K * 4)
            g_svad = H("vad(segments)", (B,), VAD_DTYPE, canary, 48)
            call(eng, "sr_recognize_segments_batch", P(ptr), U64(stride), U32(buf_len), U32(B), P(g_sres.ptr), P(g_ssc.ptr),
                 P(g_svad.ptr))
            g_sres.check_equals(sres)
            g_ssc.check_equals(ssc)
            g_svad.check_equals(vd)
            if feats is None:
                continue
            for kind in KINDS:
                w = eng.frame_feature_width(kind)
                g_ft = H("feat(kind %d)" % kind, (B, R, w), np.uint32, canary, R * w * 4)
                g_fm, g_n, g_st = H("mfcc(features)", (B, R, nc), np.int16, canary, rec_m), \
                    H("frm_num", (B,), np.uint32, canary, 4), H("status", (B,), np.uint32, canary, 4)
                call(eng, "sr_frame_features_batch", I32(kind), P(ptr), U64(stride), U32(buf_len), U32(B), P(st.ctypes.data),
                     P(en.ctypes.data), P(mid.ctypes.data), P(g_ft.ptr), P(g_fm.ptr), P(g_n.ptr), P(g_st.ptr))
                g_fm.check_equals(xmf)
                g_n.check_equals(xn)
                g_st.check_equals(xstatus)
                if kind == FEAT_FFT:
                    check_fft_words(g_ft, feats[FEAT_MAG])
                else:
                    g_ft.check_equals(feats[kind])
    finally:
        eng.set_small_launch(0)


@pytest.mark.parametrize("front", list(FRONTS))
def test_train_store_writes_its_records_and_nothing_else(fronts, front):
    """sr_train_store: a named slot holds 0xFF | save_mask | frm_num | frm_num rows | 0xFF to the end of the slot; slots that
    are not named, slots of failed captures and both guards keep what they held"""
    c = fronts(front)
    eng, nc = c.eng, c.nc
    B, buf_len = 9, c.base - 1
    stride, lead = buf_len + 3, 1
    rows = make_batch(c, B, buf_len, seed=3)
    flat = padded_rows(rows, stride, lead, 100, "adc")
    vd, res, mf, sc = expected(c, rows)
    slot_bytes = 4 + 2 * nc * R + 10  # not a multiple of anything
    n_slots = 14
    slots = np.array([12, 0, 5, 7, 3, 9, 1, 13, 10], np.uint32)
    for canary in CANARIES:
        g_store = H("store", (n_slots, slot_bytes), np.uint8, canary, slot_bytes)
        g_st = H("status", (B,), np.uint32, canary, 4)
        want = g_store.interior()
        for i in range(B):
            if vd["status"][i] != ST_OK:
                continue
            n = int(vd["frm_num"][i])
            rec = want[slots[i]]
            rec[:] = 0xFF
            rec[:4].view(np.uint16)[:] = (12345, n)
            rec[4:4 + n * nc * 2] = mf[i, :n].reshape(-1).view(np.uint8)
        call(eng, "sr_train_store", P(flat.ctypes.data + 2 * lead), U64(stride), U32(buf_len), U32(B), P(slots.ctypes.data),
             P(g_store.ptr), U32(n_slots), U32(slot_bytes), P(g_st.ptr))
        g_store.check_equals(want)
        g_st.check_equals(vd["status"].astype(np.uint32))
    assert (vd["status"] == ST_OK).sum() >= 4 and (vd["status"] != ST_OK).sum() >= 4


def test_packed12_rows_with_filler_and_a_poison_nibble(fronts):
    """sr_recognize_batch_packed12: odd buf_len, row_stride_bytes larger than ceil(buf_len / 2) * 3 with 0xFF filler, and the
    unused half of the last byte triple of every row carrying 0xFFF"""
    c = fronts("ref")
    eng, nc, K = c.eng, c.nc, c.K
    B, buf_len = 9, c.base - 3
    assert buf_len % 2 == 1
    rows = make_batch(c, B, buf_len, seed=29)
    vd, res, mf, sc = expected(c, rows)
    pk = pack12(np.concatenate([rows, np.full((B, 1), 0xFFF, np.uint16)], 1))
    assert pk.shape[1] == (buf_len + 1) // 2 * 3
    for pitch, lead in ((pk.shape[1] + 5, 3), (pk.shape[1], 0), (pk.shape[1] + 4099, 1)):
        img = np.full(lead + B * pitch + 64, 0xFF, np.uint8)
        for b in range(B):
            img[lead + b * pitch:lead + b * pitch + pk.shape[1]] = pk[b]
        for canary in CANARIES:
            outs = [H("results", (B,), RESULT_DTYPE, canary, 16), H("scores", (B, K), np.uint32, canary, K * 4),
                    H("mfcc", (B, R, nc), np.int16, canary, R * nc * 2), H("vad", (B,), VAD_DTYPE, canary, 48)]
            call(eng, "sr_recognize_batch_packed12", P(img.ctypes.data + lead), U64(pitch), U32(buf_len), U32(B),
                 *[P(g.ptr) for g in outs])
            for g, w in zip(outs, (res, sc, mf, vd)):
                g.check_equals(w)


# ---- stream recognition -------------------------------------------------------------------------------------------------------
def expected_stream(c, rows, lens):
    """segments of rows[b][:lens[b]] (oracle VAD, unbounded count) and each one recognised like segment 0"""
    orc, K, nc = c.orc_many, c.K, c.nc
    segs, off, atap, rec = [], [0], np.zeros(len(rows), ATAP_DTYPE), []
    for b in range(len(rows)):
        x = rows[b][:lens[b]]
        rc, a = orc.noise_atap(x)
        assert rc == 0
        atap[b] = a.astuple()
        sg = orc.vad(x, a).reshape(-1, 2)
        sg = sg[sg[:, 0] >= 0]
        assert len(sg) < 64
        for st, en in sg:
            n, status = frm_status(int(st), int(en), c.fl, c.hop)
            segs.append((b, st, en, n))
            scores, m = np.full(K, DIS_ERR, np.uint32), np.zeros((R, nc), np.int16)
            best, mind = 0, DIS_ERR
            if status == ST_OK:
                nn, mm = orc.mfcc(x, int(st), int(en), a)
                assert nn == n
                m[:n] = mm
                mz = np.concatenate([m, np.zeros((1, nc), np.int16)])
                for k in range(K):
                    if c.valid[k]:
                        scores[k] = orc.dtw(mz, n, c.tm[k], int(c.tf[k]))
                    if scores[k] < mind:
                        best, mind = k, int(scores[k])
            rec.append(((best, mind, n, status), scores, m))
        off.append(len(segs))
    return np.array(segs, STREAM_SEG_DTYPE), np.array(off, np.uint32), atap, rec


def stream_outputs(c, rec, n_out, canary_fill):
    """results / scores / mfcc [n_out] from the per-segment records; slots past them: `canary_fill` None -> failed records
    (device form), else left as they were (host form)"""
    K, nc = c.K, c.nc
    res, sc, mf = np.zeros(n_out, RESULT_DTYPE), np.full((n_out, K), DIS_ERR, np.uint32), np.zeros((n_out, R, nc), np.int16)
    res["min_dis"], res["status"] = DIS_ERR, ST_VAD_FAIL
    for i, (r, s, m) in enumerate(rec[:n_out]):
        res[i], sc[i], mf[i] = r, s, m
    if canary_fill is not None:
        for a in (res, sc, mf):
            a[len(rec):].view(np.uint8)[...] = canary_fill
    return res, sc, mf


@pytest.mark.parametrize("front,poison,side", [("ref", "adc", False), ("ext", "ffff", True), ("gen", "adc", True),
                                               ("gen32", "ffff", False)])
def test_stream_entry_points_with_short_recordings_in_padded_rows(fronts, front, poison, side):
    """sr_stream_segments_dev, sr_recognize_stream_dev and sr_recognize_stream: d_len[b] < buf_len with poison between
    d_len[b] and buf_len as well as between the rows; two slots more than there are segments"""
    c = fronts(front)
    eng, nc, K = c.eng, c.nc, c.K
    B, buf_len, lead = 7, c.base + 5, 8
    stride = (buf_len + 7) // 8 * 8 + 4104
    rows = make_batch(c, B, buf_len, seed=41)
    lens = np.array([buf_len, buf_len - 1, buf_len - 8, buf_len - 3 * c.hop - 7, buf_len - 5, buf_len - c.fl, buf_len - 2], np.uint32)
    img = rows.copy()
    for b in range(B):  # between len[b] and buf_len: the same poison as between the rows
        img[b, lens[b]:] = padded_rows(rows[b:b + 1, :lens[b]], buf_len, 0, 0, poison)[lens[b]:]
    flat = padded_rows(img, stride, lead, 264, poison)
    segs, off, atap, rec = expected_stream(c, rows, lens)
    total = len(segs)
    assert total >= B and (segs["end"] == -1).any() and (segs["start"] == 0).any() and (segs["frm_num"] >= 10).sum() >= 3
    max_segs = total + 2
    dpcm, ptr = to_dev(flat, lead)
    dlen = torch.from_numpy(lens.view(np.int32)).to(DEV)
    stream, sid = stream_of(side)
    for canary in CANARIES:
        want_segs = np.zeros(max_segs, STREAM_SEG_DTYPE)
        want_segs.view(np.uint8)[...] = canary  # records >= the total are not written
        want_segs[:total] = segs
        g_segs, g_off = G("d_segs", (max_segs,), STREAM_SEG_DTYPE, canary, 16), G("d_seg_offsets", (B + 1,), np.uint32, canary, 4)
        g_atap = G("d_atap", (B,), ATAP_DTYPE, canary, 12)
        torch.cuda.synchronize()
        call(eng, "sr_stream_segments_dev", P(ptr), U64(stride), U32(buf_len), P(dlen.data_ptr()), U32(B), P(None), U32(max_segs),
             P(g_segs.ptr), P(g_off.ptr), P(g_atap.ptr), P(sid))
        torch.cuda.synchronize()
        g_segs.check_equals(want_segs)
        g_off.check_equals(off)
        g_atap.check_equals(atap)
        # the same with the caller's thresholds (d_atap_in, itself followed by a guard) and no d_atap output
        g_at_in = input_in_guards("d_atap_in", atap, canary)
        g_segs, g_off = G("d_segs(atap_in)", (max_segs,), STREAM_SEG_DTYPE, canary, 16), G("d_seg_offsets(atap_in)", (B + 1,), np.uint32, canary, 4)
        torch.cuda.synchronize()
        call(eng, "sr_stream_segments_dev", P(ptr), U64(stride), U32(buf_len), P(dlen.data_ptr()), U32(B), P(g_at_in.ptr), U32(max_segs),
             P(g_segs.ptr), P(g_off.ptr), P(None), P(sid))
        torch.cuda.synchronize()
        g_segs.check_equals(want_segs)
        g_off.check_equals(off)
        g_at_in.check_equals(atap)
        res, sc, mf = stream_outputs(c, rec, max_segs, None)
        g_segs, g_off = G("d_segs", (max_segs,), STREAM_SEG_DTYPE, canary, 16), G("d_seg_offsets", (B + 1,), np.uint32, canary, 4)
        outs = [G("d_results", (max_segs,), RESULT_DTYPE, canary, 16), G("d_scores", (max_segs, K), np.uint32, canary, K * 4),
                G("d_mfcc", (max_segs, R, nc), np.int16, canary, R * nc * 2)]
        torch.cuda.synchronize()
        call(eng, "sr_recognize_stream_dev", P(ptr), U64(stride), U32(buf_len), P(dlen.data_ptr()), U32(B), P(None), U32(max_segs),
             P(g_segs.ptr), P(g_off.ptr), *[P(g.ptr) for g in outs], P(sid))
        torch.cuda.synchronize()
        g_segs.check_equals(want_segs)
        g_off.check_equals(off)
        for g, w in zip(outs, (res, sc, mf)):
            g.check_equals(w)
        # the host form: odd stride, 2-byte aligned base; outputs past min(total, max_segs) are not written
        hstride = buf_len + 1
        hflat = padded_rows(img, hstride, 1, 50, poison)
        res, sc, mf = stream_outputs(c, rec, max_segs, canary)
        g_segs, g_off = H("segs", (max_segs,), STREAM_SEG_DTYPE, canary, 16), H("seg_offsets", (B + 1,), np.uint32, canary, 4)
        outs = [H("results", (max_segs,), RESULT_DTYPE, canary, 16), H("scores", (max_segs, K), np.uint32, canary, K * 4),
                H("mfcc", (max_segs, R, nc), np.int16, canary, R * nc * 2)]
        g_tot = H("n_segs", (1,), np.uint32, canary, 4)
        call(eng, "sr_recognize_stream", P(hflat.ctypes.data + 2), U64(hstride), U32(buf_len), P(lens.ctypes.data), U32(B), P(None),
             U32(max_segs), P(g_segs.ptr), P(g_off.ptr), *[P(g.ptr) for g in outs], P(g_tot.ptr))
        g_segs.check_equals(want_segs)
        g_off.check_equals(off)
        g_tot.check_equals(np.array([total], np.uint32))
        for g, w in zip(outs, (res, sc, mf)):
            g.check_equals(w)
    del dpcm, stream


# ---- feature-row inputs ---------------------------------------------------------------------------------------------------------
def feature_records(c, rng):
    """records [B, R, nc] with poison rows >= frames[b]: 1 frame, max_frames, 0 frames, a failed record that kept its
    frm_num, and max_frames again as the LAST record (the back guard follows it directly)"""
    frames = np.array([1, R, 0, 20, 33, 1, R - 1, 24, 2, R], np.uint32)
    status = np.zeros(len(frames), np.uint32)
    status[7] = ST_MFCC_FAIL
    im = rng.integers(-900, 900, (len(frames), R, c.nc)).astype(np.int16)
    poison_feature_rows(im, frames)
    vd = np.zeros(len(frames), VAD_DTYPE)
    vd["frm_num"], vd["status"], vd["seg"] = frames, status, -1
    eff = np.where(status == 0, frames, 0).astype(np.uint32)
    return im, frames, vd, eff


def dtw_expected(c, im, eff, vd):
    B, K = len(im), c.K
    sc, res = np.full((B, K), DIS_ERR, np.uint32), np.zeros(B, RESULT_DTYPE)
    for b in range(B):
        mz = np.concatenate([im[b], np.zeros((1, c.nc), np.int16)])  # the record as the device sees it + a ZERO row
        best, mind = 0, DIS_ERR
        for k in range(K):
            if eff[b] and c.valid[k]:
                sc[b, k] = c.orc.dtw(mz, int(eff[b]), c.tm[k], int(c.tf[k]))
            if sc[b, k] < mind:
                best, mind = k, int(sc[b, k])
        res[b] = (best, mind, vd["frm_num"][b], vd["status"][b])
    return sc, res


def input_in_guards(name, arr, canary, device=DEV):
    """an INPUT placed in a canary-filled allocation: what follows its last record differs between the two canaries"""
    g = guarded_out(arr.shape, arr.dtype, canary, 4096, device, name)
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if device is None:
        g.flat[g.lo:g.hi] = raw
    else:
        g.flat[g.lo:g.hi] = torch.from_numpy(raw.copy()).to(device)
    return g


@pytest.mark.parametrize("front", ["ref", "gen", "gen32"])
def test_dtw_device_forms_on_records_with_poison_rows(fronts, front):
    """sr_dtw_batch_dev in every small-launch mode (k_dtw_lds, k_dtw_cells, k_dtw_quad, automatic), sr_dtw_dp_batch_dev with
    d_in_frames and with d_vad, sr_delta_mfcc_batch_dev with both: the last record has frm_num == max_frames and is followed
    directly by the back guard, whose content changes between the two runs"""
    c = fronts(front)
    eng, nc, K = c.eng, c.nc, c.K
    im, frames, vd, eff = feature_records(c, np.random.default_rng(8))
    B = len(frames)
    sc, res = dtw_expected(c, im, eff, vd)
    assert (sc != DIS_ERR).sum() >= 12 and (sc[0] != DIS_ERR).any() and (sc[7] == DIS_ERR).all() and (sc[2] == DIS_ERR).all()
    imz = np.concatenate([im, np.zeros((B, 1, nc), np.int16)], 1)
    tf_eff = np.where(c.valid != 0, c.tf, 0).astype(np.uint32)
    dp = c.orc.dtw_dp_batch(imz, eff, c.tm, tf_eff, n_threads=THREADS) if nc == 12 else None
    delta = np.zeros_like(im)
    delta_f = np.zeros_like(im)
    for b in range(B):
        delta[b, :eff[b]] = c.orc.delta_mfcc(im[b], int(eff[b]))
        delta_f[b, :frames[b]] = c.orc.delta_mfcc(im[b], int(frames[b]))
    try:
        for canary, side in zip(CANARIES, (False, True)):
            stream, sid = stream_of(side)
            g_in = input_in_guards("d_mfcc(in)", im, canary)
            g_vd = input_in_guards("d_vad(in)", vd, canary)
            g_fr = input_in_guards("d_in_frames", frames, canary)
            for mode in (1, 2, 3, 0):
                eng.set_small_launch(mode)
                g_sc, g_res = G("d_scores", (B, K), np.uint32, canary, K * 4), G("d_results", (B,), RESULT_DTYPE, canary, 16)
                torch.cuda.synchronize()
                call(eng, "sr_dtw_batch_dev", P(g_in.ptr), P(g_vd.ptr), U32(B), P(g_sc.ptr), P(g_res.ptr), P(sid))
                torch.cuda.synchronize()
                g_sc.check_equals(sc)
                g_res.check_equals(res)
                g_sc = G("d_scores(no results)", (B, K), np.uint32, canary, K * 4)
                torch.cuda.synchronize()
                call(eng, "sr_dtw_batch_dev", P(g_in.ptr), P(g_vd.ptr), U32(B), P(g_sc.ptr), P(None), P(sid))
                torch.cuda.synchronize()
                g_sc.check_equals(sc)
            eng.set_small_launch(0)
            if dp is not None:
                # with d_in_frames the counts are taken as given (record 7 is scored), with d_vad its status fails it
                dp_f = c.orc.dtw_dp_batch(imz, frames, c.tm, tf_eff, n_threads=THREADS)
                for fr_ptr, vd_ptr, want in ((g_fr.ptr, None, dp_f), (None, g_vd.ptr, dp)):
                    g_sc = G("d_scores(dp)", (B, K), np.uint32, canary, K * 4)
                    torch.cuda.synchronize()
                    call(eng, "sr_dtw_dp_batch_dev", P(g_in.ptr), P(fr_ptr), P(vd_ptr), U32(B), P(g_sc.ptr), P(sid))
                    torch.cuda.synchronize()
                    g_sc.check_equals(want)
            for fr_ptr, vd_ptr, want in ((g_fr.ptr, None, delta_f), (None, g_vd.ptr, delta)):
                g_d = G("d_delta", (B, R, nc), np.int16, canary, R * nc * 2)
                torch.cuda.synchronize()
                call(eng, "sr_delta_mfcc_batch_dev", P(g_in.ptr), P(vd_ptr), P(fr_ptr), U32(B), P(g_d.ptr), P(sid))
                torch.cuda.synchronize()
                g_d.check_equals(want)
            for g in (g_in, g_vd, g_fr):
                g.check()
    finally:
        eng.set_small_launch(0)


@pytest.mark.parametrize("B", [283, 284])
def test_dtw_host_form_on_poisoned_records_at_the_edge_of_the_staging_area(fronts, B):
    """sr_dtw_batch in every small-launch mode on the largest batch of records that fits the upload part of the pinned
    staging area and on the first that does not: a record of R = 48 frames x 12 coefficients is 1 152 bytes + 4 of its frame
    count, + 128 for the two blocks, against 327 680 bytes -- 283 records are 327 276, 284 are 328 432.  Frame counts 1..48
    (1, 2 and R among them), poison rows at and after frames[b]; every score and every result record equals the oracle's"""
    c = fronts("ref")
    assert c.nc == 12 and 283 * (R * 12 * 2 + 4) + 128 <= 327680 < 284 * (R * 12 * 2 + 4) + 128
    rng = np.random.default_rng(B)
    frames = rng.integers(1, R + 1, B).astype(np.uint32)
    frames[:3], frames[-1] = (1, 2, R), R
    im = poison_feature_rows(rng.integers(-900, 900, (B, R, c.nc)).astype(np.int16), frames)
    vd = np.zeros(B, VAD_DTYPE)
    vd["frm_num"] = frames
    want_sc, want_res = dtw_expected(c, im, frames, vd)
    assert (want_sc[:, c.valid != 0] != DIS_ERR).sum() >= B and (want_sc[:, c.valid == 0] == DIS_ERR).all()
    sc, res = _dtw_all_modes(c.eng, im, frames)
    assert np.array_equal(sc, want_sc), np.argwhere(sc != want_sc)[:4].tolist()
    assert res.tobytes() == want_res.tobytes()


def test_get_mdl_batch_on_records_with_poison_rows(fronts):
    """sr_get_mdl_batch: in1 / in2 rows >= n are poison, records of 1 frame, of every row of their record (the last pair among
    them, followed directly by the guard) and pairs outside the 1/2..2 gate; outputs guarded"""
    c = fronts("ref")
    eng, rng = c.eng, np.random.default_rng(12)
    rows1, rows2, mdl_rows = 40, 33, 36
    n1 = np.array([1, 1, 2, 40, 30, 20, 9, 40, 40], np.uint32)
    n2 = np.array([1, 2, 1, 33, 33, 11, 33, 20, 33], np.uint32)
    Pn = len(n1)
    a = poison_feature_rows(rng.integers(-900, 900, (Pn, rows1, 12)).astype(np.int16), n1)
    b = poison_feature_rows((a[:, :rows2] // 2 + rng.integers(-200, 200, (Pn, rows2, 12))).astype(np.int16), n2)
    z = np.zeros((1, 12), np.int16)
    w_mdl, w_n, w_dis = np.zeros((Pn, mdl_rows, 12), np.int16), np.zeros(Pn, np.uint32), np.zeros(Pn, np.uint32)
    for p in range(Pn):
        d, n, out = c.orc.get_mdl(np.concatenate([a[p], z]), int(n1[p]), np.concatenate([b[p], z]), int(n2[p]), mdl_rows)
        w_dis[p], w_n[p] = d, n
        w_mdl[p, :len(out)] = out
    assert (w_dis != DIS_ERR).sum() >= 6 and w_dis[6] == DIS_ERR and w_n.max() > mdl_rows  # one merged template is clipped
    for canary in CANARIES:
        g_a, g_b = input_in_guards("in1", a, canary, None), input_in_guards("in2", b, canary, None)
        g_mdl, g_n, g_dis = H("mdl", (Pn, mdl_rows, 12), np.int16, canary, mdl_rows * 24), H("mdl_frames", (Pn,), np.uint32, canary, 4), \
            H("dis", (Pn,), np.uint32, canary, 4)
        call(eng, "sr_get_mdl_batch", P(g_a.ptr), P(n1.ctypes.data), U32(rows1), P(g_b.ptr), P(n2.ctypes.data), U32(rows2), U32(Pn),
             P(g_mdl.ptr), U32(mdl_rows), P(g_n.ptr), P(g_dis.ptr))
        g_dis.check_equals(w_dis)
        g_n.check_equals(w_n)
        g_mdl.check_equals(w_mdl)


# ---- template stores ------------------------------------------------------------------------------------------------------------
def store_inputs(c, rng):
    """utterances against which a store is scored: 1 and 2 frames (the only lengths whose walk reads a template's slack row)
    and ordinary ones"""
    inf = np.array([1, 2, 1, 20, 31, 40, 2, 26], np.uint32)
    im = np.zeros((len(inf), R, c.nc), np.int16)
    for b in range(len(inf)):
        im[b, :inf[b]] = rng.integers(-900, 900, (inf[b], c.nc))
    return im, inf


def score_store(c, im, inf, image, tf, valid):
    """oracle scores against the image [K, rows, nc] the engine keeps by its slack-row rule"""
    sc = np.full((len(inf), len(tf)), DIS_ERR, np.uint32)
    for b in range(len(inf)):
        mz = np.concatenate([im[b], np.zeros((1, c.nc), np.int16)])
        for k in range(len(tf)):
            if valid[k]:
                sc[b, k] = c.orc.dtw(mz, int(inf[b]), image[k], int(tf[k]))
    return sc


@pytest.mark.parametrize("front", ["ref", "gen"])
def test_template_stores_keep_one_slack_row_when_the_stride_has_room(fronts, front):
    """sr_set_templates_dense with tpl_stride = (maxf + j) * n_coef, j = 0, 1, 7, and sr_set_templates with slot strides
    4 + 2 * n_coef * (maxf + j), 4096 and 8192; poison in every row >= frames[k].  The rule (sr_engine.cpp): the engine keeps
    rows 0..maxf of every template; row r comes from the caller's image when the stride holds it and is zero otherwise, so row
    frames[k] -- the one row past a template the walk can read, and only of a 1-frame template -- is the caller's where there
    is room.  Invalid slots hold frm_num 0xFFFF and poison.  Scores through every DTW form."""
    c = fronts(front)
    eng, nc, rng = c.eng, c.nc, np.random.default_rng(23)
    tf = np.array([1, 40, 0, 1, 25, 2, 33, 40], np.uint32)
    valid = np.array([1, 1, 1, 1, 0, 1, 1, 1], np.uint8)
    K, maxf = len(tf), 40
    im, inf = store_inputs(c, rng)
    try:
        for j in (0, 1, 7):
            src = poison_feature_rows(rng.integers(-900, 900, (K, maxf + j, nc)).astype(np.int16), tf)
            image = np.zeros((K, maxf + 1, nc), np.int16)
            image[:, :min(maxf + j, maxf + 1)] = src[:, :maxf + 1]
            want = score_store(c, im, inf, image, tf, valid)
            call(eng, "sr_set_templates_dense", P(src.ctypes.data), P(tf.ctypes.data), P(valid.ctypes.data), U32(K), U32((maxf + j) * nc))
            eng._tpl = ("set_templates_dense", (src, tf, valid))  # what clone() replays: the same call through the wrapper
            sc, res = _dtw_all_modes(eng, im, inf)
            assert np.array_equal(sc, want), (j, np.argwhere(sc != want)[:4].tolist())
            assert (want[[0, 2], 0] != DIS_ERR).all() and (want[:, 4] == DIS_ERR).all() and (want[:, 2] == DIS_ERR).all()
        for stride in [4 + 2 * nc * (maxf + j) for j in (0, 1, 7)] + [4096, 8192]:
            slot_rows = (stride - 4) // (2 * nc)
            store = np.zeros(K * stride, np.uint8)
            image = np.zeros((K, maxf + 1, nc), np.int16)
            for k in range(K):
                rec = store[k * stride:(k + 1) * stride]
                body = poison_feature_rows(rng.integers(-900, 900, (1, slot_rows, nc)).astype(np.int16), [tf[k] if valid[k] else 0])[0]
                rec[:4].view(np.uint16)[:] = (12345, tf[k]) if valid[k] else (0xFFFF, 0xFFFF)
                rec[4:4 + body.nbytes] = body.reshape(-1).view(np.uint8)
                rec[4 + body.nbytes:] = 0x7F
                if valid[k]:
                    image[k, :min(slot_rows, maxf + 1)] = body[:maxf + 1]
            want = score_store(c, im, inf, image, tf, valid)
            eng.set_templates_store(store, stride)
            sc, res = _dtw_all_modes(eng, im, inf)
            assert np.array_equal(sc, want), (stride, np.argwhere(sc != want)[:4].tolist())
    finally:
        c.set_default_store()


def test_device_pcm_that_breaks_the_alignment_rules_is_refused_and_nothing_is_written(fronts):
    """the device forms state their rule (16-byte aligned base, pcm_stride a multiple of 8, pcm_stride >= buf_len): a call that
    breaks it returns SR_ERR_BAD_ARG and writes nothing -- guards and interior keep the canary"""
    c = fronts("ref")
    eng, B, buf_len = c.eng, 3, c.base
    dpcm, ptr = to_dev(np.full(8 + B * (buf_len + 16), 2048, np.uint16), 8)
    for canary in CANARIES:
        for p, stride, bl in ((ptr + 2, buf_len + 8, buf_len), (ptr, buf_len + 4, buf_len), (ptr, buf_len, buf_len + 8)):
            outs = [G("d_results", (B,), RESULT_DTYPE, canary, 16), G("d_scores", (B, c.K), np.uint32, canary, c.K * 4),
                    G("d_mfcc", (B, R, c.nc), np.int16, canary, R * c.nc * 2), G("d_vad", (B,), VAD_DTYPE, canary, 48)]
            torch.cuda.synchronize()
            assert eng.L.sr_recognize_batch_dev(eng.h, P(p), U64(stride), U32(bl), U32(B), *[P(g.ptr) for g in outs], P(0)) == 3
            assert eng.L.sr_vad_batch_dev(eng.h, P(p), U64(stride), U32(bl), U32(B), P(outs[3].ptr), P(0)) == 3
            torch.cuda.synchronize()
            for g in outs:
                g.check_untouched()
    del dpcm
