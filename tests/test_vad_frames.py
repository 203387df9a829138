"""The VAD's per-frame decision (VAD.C:164: frm_sum > s_thl || frm_zero > z_thl) in every kernel form and every framing.

The kernels never walk the samples as the reference does: they rebuild frm_sum and the band-crossing count from per-block
summaries and a carried class (csrc/sr_vad_dev.h), and the rule that consumes the summaries exists four times (k_vad,
k_vad_wide, k_stream_tiles, k_live_scan).  Segments hide most of what can go wrong there -- a wrong bit moves a segment only
at a transition of the endpoint state machine (test_segments_alone_would_not_have_been_enough prints how rarely) -- so

  * the two batch forms are held to the oracle's sample-by-sample loop BIT BY BIT through sr_vad_debug_masks, on captures
    built to sit on every threshold and block edge (tests/vad_cases.py), and
  * the stream and live forms, which hand out segments only, run captures whose run lengths are drawn around the two
    duration limits, so that (asserted) a flipped bit changes the segment list for at least 30 % of the frames.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import vad_cases as vc
from conftest import needs_ref_objects
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import ATAP_DTYPE, ST_MFCC_FAIL, ST_OK, ST_SEG_OOB, ST_VAD_FAIL, Engine, unpack_vad_masks

# Floors of the coverage conditions, per framing, on the oracle's values within the compared range.
MIN_COMPARED_SHARE = 0.90
MIN_THRESHOLD_FRAMES = 50    # each of Z == z_thl, Z == z_thl + 1 (sum <= s_thl), sum == s_thl, sum == s_thl + 1 (Z <= z_thl)
MIN_EDGE_CLASS = 10          # each block-edge class of vad_cases.required_edge_classes()
MIN_DECISIVE_SHARE = 0.30


def seg_array(segs, n):
    out = np.full(2 * n, -1, np.int32)
    for i, (s, e) in enumerate(segs[:n]):
        out[2 * i], out[2 * i + 1] = s, e
    return out


def frm_and_status(segs, fl, hop, max_frames):
    """MFCC.C:102-107 on segment 0, as the VAD kernels report it"""
    if not segs or segs[0][1] < 0:
        return 0, ST_VAD_FAIL
    st, en = segs[0]
    if st < 1:
        return 0, ST_SEG_OOB
    n = ((((en - st) & 0xFFFFFFFF) - fl) // hop + 1) & 0xFFFF
    return (0, ST_MFCC_FAIL) if n > max_frames else (n, ST_OK)


def all_segments(cs, row, atap=None):
    """the endpoint state machine, unbounded, over the oracle's bits of one capture (for other thresholds: atap)"""
    loud = row["loud"] if atap is None else cs.orc.vad_frames(row["x"], ol.Atap(*atap))[2]
    return [tuple(s) for s in vc.segments_from_loud(loud, cs.fl, cs.hop, cs.vmin, cs.smax)[0]]


def check_coverage(cs):
    """the conditions that keep the per-frame comparison from passing vacuously, from the oracle's values alone"""
    cov = vc.coverage(cs)
    print(f"{cs.name}: {cov['compared']} of {cov['frames']} frames compared; Z==z {cov['Z==z']}, Z==z+1 {cov['Z==z+1,sum<=s']}, "
          f"sum==s {cov['sum==s']}, sum==s+1 {cov['sum==s+1,Z<=z']}; rarest edge class "
          f"{min(cov[k] for k in vc.required_edge_classes())}; {cov['few']} of {len(cs.rows)} captures under {vc.MAX_SEG} segments; "
          f"frame 0 at z_thl {cov['frame0']}, wrapped b_thl {cov['b_wraps']}, a_thl over the range {cov['a_over']}")
    assert cov["compared"] >= MIN_COMPARED_SHARE * cov["frames"]
    for k in ("Z==z", "Z==z+1,sum<=s", "sum==s", "sum==s+1,Z<=z"):
        assert cov[k] >= MIN_THRESHOLD_FRAMES, (cs.name, k, cov[k])
    for k in vc.required_edge_classes():
        assert cov[k] >= MIN_EDGE_CLASS, (cs.name, k, cov[k])
    assert cov["rounds_one_sided"] == 0            # loud and quiet frames in every round index that is compared
    assert 2 * cov["few"] >= len(cs.rows)          # at least half of the captures have all their frames evaluated
    assert cov["few"] < len(cs.rows)               # the rest close max_seg segments
    # frame 0 (last_sig = 0 on entry) exactly at z_thl, its first block's first out-of-band sample past offset 0 and of another
    # class than its last one (one crossing too many there makes the frame loud); captures whose b_thl wraps, whose a_thl lies
    # above every code, and that hold the codes 0 and 65 535.  Of 32 captures 8 have a head built for frame 0 (half of those
    # hit z_thl exactly by construction) and 4 + 4 the two range heads: two of each is what a seed cannot miss.
    assert cov["frame0"] >= 2 and cov["b_wraps"] >= 2 and cov["a_over"] >= 2 and cov["code0"] >= 2 and cov["code65535"] >= 2
    return cov


def runs_share(cs):
    n = F = 0
    for row in cs.rows:
        a, b = vc.decisive_share(row["loud"], cs.fl, cs.hop, cs.vmin, cs.smax)
        n, F = n + a, F + b
    return n / F


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vc.FRAMING_IDS)
def test_state_machine_over_oracle_bits_reproduces_oracle_segments(name):
    """sr_oracle_vad_frames is sr_oracle_vad's loop: its bits, fed to the endpoint state machine, give sr_oracle_vad's segments
    -- with the reference's three segments and with an unbounded count -- on every generated capture"""
    f = vc.FRAMINGS[vc.FRAMING_IDS.index(name)]
    many = ol.Oracle(max_seg=1 << 12, **f[2])
    for cs in (vc.cases(name), vc.cases(name, runs=True)):
        for b, row in enumerate(cs.rows):
            rc, a = cs.orc.noise_atap(row["x"])
            assert rc == 0 and a.astuple() == row["atap"], b
            F = (len(row["x"]) - cs.fl + cs.hop - 1) // cs.hop
            assert len(row["loud"]) == len(row["fsum"]) == len(row["fzero"]) == F
            assert np.array_equal(row["loud"], (row["fsum"] > a.s_thl) | (row["fzero"] > a.z_thl))
            assert np.array_equal(seg_array(row["segs"], vc.MAX_SEG), cs.orc.vad(row["x"], a)), (name, b)
            want = many.vad(row["x"], a).reshape(-1, 2)
            want = [tuple(int(v) for v in s) for s in want[want[:, 0] >= 0]]
            assert all_segments(cs, row) == want, (name, b)


@needs_ref_objects
def test_reference_objects_agree_on_the_reference_framing():
    ref = ol.RefLib()
    for cs in (vc.cases("ref_160_80"), vc.cases("ref_160_80", runs=True)):
        for b, row in enumerate(cs.rows):
            assert len(row["x"]) <= 0xFFFF
            a, seg = ref.vad(row["x"])
            assert a.astuple() == row["atap"], b
            assert np.array_equal(seg, seg_array(row["segs"], 3)), (b, seg)


@pytest.mark.parametrize("name", vc.FRAMING_IDS)
def test_generated_captures_meet_the_coverage_conditions(name):
    check_coverage(vc.cases(name))
    share = runs_share(vc.cases(name, runs=True))
    print(f"{name}: decisive share of the run-length captures {share:.3f}")
    assert share >= MIN_DECISIVE_SHARE


def test_decisive_share_helper_equals_rerunning_the_state_machine():
    rng = np.random.default_rng(5)
    for vmin, smax in ((8, 11), (5, 7), (3, 4), (2, 3), (1, 1)):
        for p in (0.5, 0.8, 0.2):
            loud = rng.random(120) < p
            base = vc.segments_from_loud(loud, 160, 80, vmin, smax)[0]
            n = 0
            for f in range(len(loud)):
                flipped = loud.copy()
                flipped[f] = not flipped[f]
                n += vc.segments_from_loud(flipped, 160, 80, vmin, smax)[0] != base
            assert vc.decisive_share(loud, 160, 80, vmin, smax) == (n, len(loud)), (vmin, smax, p)


def test_segments_alone_would_not_have_been_enough():
    """Why the per-frame comparison exists: on the captures of test_gpu_parity.test_vad_stress_matches_oracle (regenerated with
    its seed) a flipped "loud" bit changes the segment list for only a small share of the frames, so a kernel wrong in a few
    frames would most likely have passed; the run-length captures of this module are several times as sensitive."""
    orc = ol.Oracle(max_frames=119)
    rng = np.random.default_rng(2024)
    B, S = 96, 16000
    n = F = 0
    for b in range(B):
        sig = rng.normal(0, rng.choice([2, 8, 30]), S)
        for _ in range(rng.integers(0, 12)):
            p = rng.integers(2400, S - 200)
            ln = rng.integers(40, 3000)
            amp = rng.choice([15, 40, 200, 1500])
            f = rng.uniform(50, 3900)
            seg = amp * np.sin(2 * np.pi * f * np.arange(ln) / 8000 + rng.uniform(0, 6.28))
            sig[p:p + ln] += seg[:max(0, min(ln, S - p))]
        if b % 7 == 0:
            sig[rng.integers(2400, S):] += rng.choice([-60, 60])
        x = np.clip(2048 + sig, 0, 4095).astype(np.uint16)
        rc, a = orc.noise_atap(x)
        k, m = vc.decisive_share(orc.vad_frames(x, a)[2], 160, 80, 8, 11)
        n, F = n + k, F + m
    stress = n / F
    ours = runs_share(vc.cases("ref_160_80", runs=True))
    print(f"decisive share: stress captures {stress:.3f}, run-length captures {ours:.3f}")
    assert F == B * 198 and stress < MIN_DECISIVE_SHARE <= ours


# ---- GPU: the batch forms, bit by bit ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", vc.FRAMING_IDS)
def test_per_frame_bits_match_oracle(name):
    """k_vad (set_small_launch(1)) and k_vad_wide (fewer captures than CUs) against Oracle.vad_frames, every frame of every
    round up to and including the one in which the oracle's max_seg-th segment closes"""
    cs = vc.cases(name)
    check_coverage(cs)
    eng = Engine(**cs.ekw)
    try:
        b0 = 0
        for pcm, buf_len in cs.groups:
            out = {}
            for mode in (1, 0):
                eng.set_small_launch(mode)
                out[mode] = eng.vad_debug_masks(pcm, buf_len)
            eng.set_small_launch(0)
            for mode, (vd, masks) in out.items():
                for r in range(len(pcm)):
                    row, at = cs.rows[b0 + r], (name, mode, b0 + r)
                    F, n = len(row["loud"]), cs.compared(row)
                    got = unpack_vad_masks(masks[r:r + 1], F)[0]
                    bad = np.flatnonzero(got[:n] != row["loud"][:n])
                    assert len(bad) == 0, (at, row["atap"], [(int(f), int(row["fsum"][f]), int(row["fzero"][f])) for f in bad[:8]])
                    assert not got[n:].any() and not unpack_vad_masks(masks[r:r + 1])[0, F:].any(), at
                    assert (vd["mid_val"][r], vd["n_thl"][r], vd["z_thl"][r], vd["s_thl"][r]) == row["atap"], at
                    assert np.array_equal(vd["seg"][r], seg_array(row["segs"], vc.MAX_SEG)), at
                    assert (vd["frm_num"][r], vd["status"][r]) == frm_and_status(row["segs"], cs.fl, cs.hop, eng.max_frames), at
            assert out[1][0].tobytes() == out[0][0].tobytes() and np.array_equal(out[1][1], out[0][1]), name
            vd = out[1][0]
            assert np.array_equal(eng.vad(pcm, buf_len), vd)
            b0 += len(pcm)
    finally:
        eng.close()


# ---- GPU: the stream and live forms, through their segments ------------------------------------------------------------------------
def pack(rows):
    lens = np.array([len(r["x"]) for r in rows], np.uint32)
    pcm = np.full((len(rows), (int(lens.max()) + 7) // 8 * 8), 0xFFFF, np.uint16)
    for b, r in enumerate(rows):
        pcm[b, :lens[b]] = r["x"]
    return pcm, lens


def stream_segments(out, B):
    off, segs = out["seg_offsets"], out["segs"]
    assert out["total"] == off[-1] == len(segs)
    return [[(int(g["start"]), int(g["end"])) for g in segs[off[b]:off[b + 1]]] for b in range(B)]


def live_segments(eng, rows, rng, fl, hop, chunk_max, atap=None):
    """every recording pushed through one live session, a channel each, in random chunks -- half of them ending one sample before,
    on, or one sample after the point where a further frame has all its samples"""
    C = len(rows)
    lens = np.array([len(r["x"]) for r in rows], np.int64)
    pos = np.zeros(C, np.int64)
    got = [[] for _ in range(C)]
    sess = eng.live(C, chunk_max, atap)
    try:
        while np.any(pos < lens):
            cnt = rng.integers(0, chunk_max + 1, C)
            for c in range(C):
                if rng.random() < 0.5:
                    k = (pos[c] + int(rng.integers(1, chunk_max)) - fl) // hop       # a frame that ends inside the chunk's reach
                    end = k * hop + fl + int(rng.integers(-1, 2))
                    if pos[c] < end <= pos[c] + chunk_max:
                        cnt[c] = end - pos[c]
            cnt = np.minimum(cnt, lens - pos)
            W = max(8, (int(cnt.max()) + 7) // 8 * 8)
            chunk = np.full((C, W), 0xFFFF, np.uint16)   # what is not input is loud: a sample read too far would show
            for c in range(C):
                chunk[c, :cnt[c]] = rows[c]["x"][pos[c]:pos[c] + cnt[c]]
            pos += cnt
            o = sess.push(chunk, cnt.astype(np.uint32), recognize=False)
            for g in o["segs"]:
                got[int(g["channel"])].append((int(g["start"]), int(g["end"])))
        for g in sess.end(np.arange(C)):
            got[int(g["channel"])].append((int(g["start"]), -1))
    finally:
        sess.close()
    return got


@pytest.fixture
def _tile_default():
    yield
    engine.dev_hook("stream_tile_frames", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", vc.FRAMING_IDS)
def test_stream_and_live_segments_match_oracle_bits(name, _tile_default):
    """k_stream_tiles at tile sizes 16, 64 and the default, the device form of the segmentation, and k_live_scan over random chunkings: segments
    equal the state machine run over the oracle's bits (unbounded count)"""
    import torch
    cs = vc.cases(name, runs=True)
    share = runs_share(cs)
    print(f"{name}: decisive share {share:.3f} over {sum(len(r['loud']) for r in cs.rows)} frames")
    assert share >= MIN_DECISIVE_SHARE
    want = [all_segments(cs, row) for row in cs.rows]
    assert sum(len(w) for w in want) >= 5 * len(want)
    pcm, lens = pack(cs.rows)
    B = len(cs.rows)
    eng = Engine(testing=True, **cs.ekw)
    try:
        for T in (16, 64, 0):
            engine.dev_hook("stream_tile_frames", T)
            out = eng.recognize_stream(pcm, lens, recognize=False)
            got = stream_segments(out, B)
            for b in range(B):
                assert got[b] == want[b], (name, T, b)
        x = torch.from_numpy(pcm.view(np.int16)).cuda()
        ln = torch.from_numpy(lens.view(np.int32)).cuda()
        d_off = torch.zeros(B + 1, dtype=torch.int32, device=x.device)
        d_segs = torch.zeros(out["total"] + 2, 4, dtype=torch.int32, device=x.device)
        assert eng.L.sr_stream_segments_dev(eng.h, engine._vp(x), C.c_uint64(pcm.shape[1]), C.c_uint32(pcm.shape[1]), engine._vp(ln),
                                            C.c_uint32(B), None, C.c_uint32(len(d_segs)), engine._vp(d_segs), engine._vp(d_off), None,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_off.cpu().numpy().view(np.uint32), out["seg_offsets"])
        assert np.array_equal(d_segs[:out["total"]].cpu().numpy().view(np.uint8).reshape(-1), out["segs"].view(np.uint8).reshape(-1))
        got = live_segments(eng, cs.rows, np.random.default_rng(77), cs.fl, cs.hop, 16 * cs.hop)
        for b in range(B):
            assert got[b] == want[b], (name, "live", b)
    finally:
        eng.close()


# ---- GPU: thresholds handed in by the caller (the kernels' instances without the two-samples-per-instruction magnitude sum) ----
def caller_thresholds(cs, row):
    """five sets for one capture: a mid value above every sample; an empty band (every sample above or below) with the crossing
    count at its median; z_thl = 0; s_thl = 0; s_thl out of reach; and the capture's own thresholds, handed in"""
    mid, n_thl, z_thl, s_thl = row["atap"]
    x = row["x"]
    orc = cs.orc
    fs = orc.vad_frames(x, ol.Atap(70000, 20, 0, 0))[0]
    fz = orc.vad_frames(x, ol.Atap(mid, 0, 0, 0))[1]
    return [(70000, 20, 2000, int(np.sort(fs)[len(fs) // 2])),
            (mid, 0, int(np.sort(fz)[len(fz) // 2]), 0xFFFFFFFF),
            (mid, n_thl, 0, 0xFFFFFFFF),
            (mid, n_thl, z_thl, 0),
            (mid, n_thl, z_thl, s_thl)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", vc.FRAMING_IDS)
def test_caller_thresholds_stream_live_and_compat(name):
    cs = vc.cases(name, runs=True)
    rows = cs.rows
    sets = [caller_thresholds(cs, row) for row in rows]
    pcm, lens = pack(rows)
    B = len(rows)
    eng = Engine(testing=True, **cs.ekw)
    n_segs = []
    try:
        for k in range(len(sets[0])):
            at = np.array([s[k] for s in sets], ATAP_DTYPE)
            want = [all_segments(cs, rows[b], sets[b][k]) for b in range(B)]
            n_segs.append(sum(len(w) for w in want))
            got = stream_segments(eng.recognize_stream(pcm, lens, atap=at, recognize=False), B)
            for b in range(B):
                assert got[b] == want[b], (name, "stream", k, b, sets[b][k])
            got = live_segments(eng, rows, np.random.default_rng(80 + k), cs.fl, cs.hop, 64 * cs.hop, atap=at)
            for b in range(B):
                assert got[b] == want[b], (name, "live", k, b, sets[b][k])
            if name == "ref_160_80":  # the reference's own VAD symbol takes its thresholds from the caller (VAD.C:97)
                from stm32_speech_recognition_amd import compat
                for b in range(B):
                    a = compat.atap_tag(*sets[b][k])
                    segs = compat.VAD(rows[b]["x"], len(rows[b]["x"]), a)
                    w3 = [(s, None if e < 0 else e) for s, e in want[b][:3]] + [(None, None)] * 3
                    assert segs == w3[:3], (name, "compat", k, b)
    finally:
        eng.close()
    print(f"{name}: segments per threshold set {n_segs}")
    assert min(n_segs) >= B // 2  # no set degenerates to "no segment anywhere"
