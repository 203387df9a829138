"""Live one-pass connected-word decoding: no word cap, the decoder's state carried between pushes (include/sr_engine.h, "live
one-pass connected-word decoding").

The rule: whatever the chunking, the row a push emits for a channel is the one-pass decoder's record (tests/onepass_ref.py) for
everything pushed to it as ONE row.  tests/onepass_live_ref.py builds one history per recording and gives the row of every
prefix (its own checks are tests/test_onepass_live_ref.py); the tests here compare records, word rows and row labels byte for
byte, after EVERY push, and the final rows with sr_decode_onepass_dp on the same engine.  No tolerances.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_ref
import onepass_live_ref as live
import onepass_ref as ref
from guarded import CANARIES, guarded_out, poison_feature_rows
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import DIS_ERR, Engine

BAD_ARG = 3
U32, U64, P = C.c_uint32, C.c_uint64, C.c_void_p
SKIP = chain_ref.PLANT_SKIP
N_CH, UTT, MAXF, W = chain_ref.PLANT_ROWS, 80, 80, 6  # the 12 planted recordings (<= 73 frames, <= 4 words) as 12 channels
FRAME_LEN, HOP = 160, 80
ONES = 0xFFFFFFFF


def same_row(got, want, what):
    """(rec, words) of one emitted row against the reference's, byte for byte"""
    for name, g, w in zip(("rec", "words"), got, want):
        g, w = np.ascontiguousarray(g).view(np.uint32).reshape(-1), np.ascontiguousarray(w).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{what}: {name} differs from word {at} on: got {g.tolist()} want {w.tolist()}")


def rows_of(out):
    """the emitted rows of a push as numpy (rec [n], words [n, words_cap])"""
    rec, words = out["rec"], out["words"]
    if not isinstance(rec, np.ndarray):
        torch.cuda.synchronize()
        n = out["n_rows"]
        rec = rec.cpu().numpy().view(ref.CHAIN_REC_DTYPE).reshape(n)
        words = words.cpu().numpy().view(ref.CHAIN_WORD_DTYPE).reshape(n, words.shape[1])
    return rec, words


def as_bytes(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in rows_of(out)) + out["rows"].tobytes()


class Follower:
    """feeds a session push by push; every push is checked against what the counts alone say (n_rows, the row labels and their
    order) and every emitted row against the reference at that channel's N"""

    def __init__(self, ses, recs, what, words_cap=None, tail=None):
        self.ses, self.recs, self.what, self.words_cap, self.tail = ses, recs, what, words_cap, tail
        self.count = [0] * len(recs)
        self.last = [None] * len(recs)

    def take(self, out, new, emit=None, session_is_here=True):
        emit = [n > 0 for n in new] if emit is None else emit
        self.count = [a + int(b) for a, b in zip(self.count, new)]
        exp = [(c, self.count[c]) for c in range(len(new)) if emit[c]]
        assert out["n_rows"] == len(exp) and [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == exp, (out["rows"], exp)
        assert not session_is_here or self.ses.frames.tolist() == self.count
        rec, words = rows_of(out)
        for r, (c, N) in enumerate(exp):
            self.last[c] = (rec[r], words[r])
            same_row(self.last[c], self.recs[c].row(N, self.words_cap, self.tail), f"{self.what}, channel {c} at {N} frames")


def push_counts(ses, f, at, cnt, form="dev"):
    """one push of cnt[c] frames of f[c] from at[c] on, the rows past each count poisoned"""
    F = max(max(cnt), 1)
    chunk = np.zeros((len(cnt), F, 12), np.int16)
    for c in range(len(cnt)):
        chunk[c, :cnt[c]] = f[c][at[c]:at[c] + cnt[c]]
    poison_feature_rows(chunk, cnt)
    if form == "dev":
        return ses.push_dev(torch.from_numpy(chunk).cuda(), np.array(cnt, np.uint32))
    return ses.push(chunk, np.array(cnt, np.uint32))


def feed(ses, fol, f, schedule, form="dev"):
    """the whole schedule; -> the bytes of everything emitted"""
    at, blob = [0] * len(f), b""
    for i, cnt in enumerate(schedule):
        out = push_counts(ses, f, at, cnt, form if form != "mixed" else ("dev", "host")[i % 2])
        fol.take(out, cnt)
        blob += as_bytes(out)
        at = [a + b for a, b in zip(at, cnt)]
    return blob


def per_channel(lists):
    """one chunking per channel -> per push the counts (0 once a channel is done)"""
    n = max(len(x) for x in lists)
    return [[x[i] if i < len(x) else 0 for x in lists] for i in range(n)]


def random_chunking(rng, N, hi):
    """sizes 0..hi that sum to N, zeros and ones included"""
    out = []
    while sum(out) < N:
        out.append(min(int(rng.choice([0, 1, int(rng.integers(1, hi + 1))])), N - sum(out)))
    return out


def cut(N, sizes):
    """the sizes in rotation until N frames are used up"""
    out, i = [], 0
    while sum(out) < N:
        out.append(min(sizes[i % len(sizes)], N - sum(out)))
        i += 1
    return out


# ---- fixtures: the planted store, its 12 recordings as 12 channels ---------------------------------------------------------------
def planted_feats():
    """-> (f: per channel the planted recording and the silence behind it, UTT frames in all; n: the recordings' frames)"""
    fx = chain_ref.planted()
    assert np.all(fx["im"][:, fx["inf"].max():] == 0)
    return [fx["im"][c, :UTT] for c in range(N_CH)], [int(n) for n in fx["inf"]]


@functools.lru_cache(maxsize=None)
def recording(c, skip, word_cost):
    """the history of planted recording c and the silence behind it, UTT frames in all, shared by every test that feeds it (the
    history of a recording is a prefix of that of any longer one)"""
    fx = chain_ref.planted()
    return live.Recording(fx["im"][c, :UTT], fx["tm"], fx["tf"], None, W, skip, word_cost)


def planted_engine(**kw):
    fx = chain_ref.planted()
    eng = Engine(max_frames=MAXF, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


@functools.lru_cache(maxsize=None)
def chunkings():
    _, n = planted_feats()
    rng = np.random.default_rng(700)
    rand = [random_chunking(rng, N, 13) for N in n]
    assert any(0 in r for r in rand) and max(n) <= 73 and len(set(n)) > 6
    return {"one frame": per_channel([[1] * N for N in n]), "random": per_channel(rand), "one push": per_channel([[N] for N in n])}


class block_hook:
    """development hook "onepass_block" (testing library only; read per push)"""

    def __init__(self, block):
        self.block = block

    def __enter__(self):
        engine.dev_hook("onepass_block", self.block)

    def __exit__(self, *exc):
        engine.dev_hook("onepass_block", 0)


# ---- GPU 1: chunking invariance ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("word_cost", [0, 5000])
@pytest.mark.parametrize("skip", [SKIP, None, 300])
def test_every_chunking_gives_the_whole_recordings_parse(skip, word_cost):
    """12 channels = three groups of kSpotWaves; L = 5, so the one push of a whole recording runs up to 15 blocks and the
    random pushes of 1..13 frames one to three, with channels that have fewer blocks than others or none"""
    fx = chain_ref.planted()
    f, n = planted_feats()
    assert ref.reach(fx["tf"]) == 5
    eng = planted_engine()
    whole = eng.decode_onepass(fx["im"][:, :MAXF], fx["inf"], W, skip, word_cost)
    recs = [recording(c, skip, word_cost) for c in range(N_CH)]
    if skip == SKIP and not word_cost:
        assert [[int(w["slot"]) for w in recs[c].row(n[c])[1][:len(fx["seq"][c])]] for c in range(N_CH)] == fx["seq"]
    for name, sched in chunkings().items():
        what = f"skip {skip}, word_cost {word_cost}, chunking '{name}'"
        ses = eng.decode_onepass_live(N_CH, max(max(s) for s in sched), UTT, W, False, skip, word_cost)
        fol = Follower(ses, recs, what)
        feed(ses, fol, f, sched, "mixed" if name == "random" else "dev")
        assert fol.count == n
        for c in range(N_CH):
            same_row(fol.last[c], (whole[0][c], whole[1][c]), what + f": final row of channel {c} against decode_onepass")
        ses.close()
    eng.close()


# ---- GPU 2: the block hook -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_block_length_gives_identical_bytes():
    f, n = planted_feats()
    eng = planted_engine(testing=True)
    recs = [recording(c, SKIP, 0) for c in range(N_CH)]
    sched = chunkings()["random"]
    blobs = {}
    for block in (0, 1, 2, 3, 5):
        with block_hook(block):
            g = engine.onepass_live_geometry(14, 5, 8, UTT, 13, testing=True)
            assert g["block"] == 5 and g["launches"] == 2 * -(-13 // (block or 5)) + 1
            ses = eng.decode_onepass_live(N_CH, 13, UTT, W, False, SKIP)
            blobs[block] = feed(ses, Follower(ses, recs, f"block {block}"), f, sched)
            ses.close()
    assert len(set(blobs.values())) == 1
    # the hook is read per push: a recording whose pushes were cut differently, and one push of many one-frame blocks
    ses = eng.decode_onepass_live(N_CH, 73, UTT, W, False, SKIP)
    fol, at = Follower(ses, recs, "block per push"), [0] * N_CH
    for i, cnt in enumerate(per_channel([cut(N, [11, 30, 7]) for N in n])):
        with block_hook((4, 1, 0, 2)[i % 4]):
            fol.take(push_counts(ses, f, at, cnt), cnt)
        at = [a + b for a, b in zip(at, cnt)]
    ses.close()
    eng.close()


# ---- GPU 3: more than 16 words ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_recordings_of_17_to_40_words_head_and_tail():
    fx = ref.planted_long()
    n = [int(v) for v in fx["inf"]]
    f = [fx["im"][r, :n[r]] for r in range(4)]
    eng = Engine(max_frames=ref.LONG_MAXF, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    recs = [live.Recording(f[r], fx["tm"], fx["tf"], None, 64, SKIP, 0) for r in range(4)]
    sched = per_channel([cut(N, [37]) for N in n])
    for cap, tail in ((64, False), (8, False), (8, True)):
        ses = eng.decode_onepass_live(4, 37, ref.LONG_MAXF, cap, tail, SKIP)
        fol = Follower(ses, recs, f"planted_long, words_cap {cap}, tail {tail}", cap, tail)
        feed(ses, fol, f, sched)
        whole = eng.decode_onepass(fx["im"], fx["inf"], cap, SKIP, 0)
        full = eng.decode_onepass(fx["im"], fx["inf"], 64, SKIP, 0)
        assert full[0]["n_words"].tolist() == list(ref.LONG_COUNTS) and min(ref.LONG_COUNTS) > 16
        for r in range(4):
            rec, words = fol.last[r]
            assert rec.tobytes() == whole[0][r].tobytes(), (cap, tail, r)
            assert rec["n_words"] == ref.LONG_COUNTS[r] and rec["status"] == (ref.CH_OK if cap == 64 else ref.CH_TRUNCATED)
            if tail:  # the last 8 words of the parse, in spoken order
                assert words.tobytes() == full[1][r, ref.LONG_COUNTS[r] - 8:ref.LONG_COUNTS[r]].tobytes(), r
                assert words["slot"].tolist() == fx["seq"][r][-8:]
            else:
                assert words.tobytes() == whole[1][r].tobytes(), (cap, r)
                k = min(cap, ref.LONG_COUNTS[r])
                assert words["slot"][:k].tolist() == fx["seq"][r][:k] and np.all(words[k:].view(np.uint32) == ONES)
        ses.close()
    eng.close()


# ---- GPU 4: sweeps of more than 64 columns ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_fixture():
    """tests/test_onepass.py's wide store restated: K = 3 templates of 70, 80 and 90 frames, L = 36; two recordings of 300 frames"""
    rng = np.random.default_rng(77)
    tf = np.array([70, 80, 90], np.uint32)
    tm = np.zeros((3, 91, 12), np.int16)
    for k in range(3):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    im = rng.integers(-3000, 3001, (2, 320, 12)).astype(np.int16)  # what is not a word is loud noise
    for r, order in enumerate(((1, 0, 2), (2, 2, 0))):
        at = 3 + r
        for k in order:
            m = int(tf[k])
            im[r, at:at + m] = tm[k, :m] + rng.integers(-60, 61, (m, 12))
            at += m + 2
        assert at <= 300
    for a in (tm, tf, im):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, im=im)


@pytest.mark.gpu
def test_wide_store_pushes_of_one_block_three_blocks_and_one_frame():
    fx = wide_fixture()
    assert ref.reach(fx["tf"]) == 36
    f = [fx["im"][r, :300] for r in range(2)]
    eng = Engine(max_frames=320, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    # 36 behind 36: the sweep of one block spans the 71 columns (c0_prev, cN); 100: three blocks, two of them 71 columns wide
    sched = per_channel([cut(300, [36, 36, 100, 1, 36]), cut(300, [1, 100, 36, 36])])
    for skip in (4000, None):
        recs = [live.Recording(f[r], fx["tm"], fx["tf"], None, 8, skip, 0) for r in range(2)]
        if skip:
            assert [recs[r].row(300)[1][:3]["slot"].tolist() for r in range(2)] == [[1, 0, 2], [2, 2, 0]]
        ses = eng.decode_onepass_live(2, 100, 300, 8, False, skip)
        fol = Follower(ses, recs, f"wide store, skip {skip}")
        feed(ses, fol, f, sched)
        whole = eng.decode_onepass(fx["im"], np.array([300, 300], np.uint32), 8, skip, 0)
        for r in range(2):
            same_row(fol.last[r], (whole[0][r], whole[1][r]), f"wide store, skip {skip}: channel {r} against decode_onepass")
        ses.close()
    eng.close()


# ---- GPU 5: ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_keep_their_rule_across_a_push_boundary():
    """t t t against twin templates of t and one of t t: the key of position 3M is reached at equal cost by the twins from
    start 2M and by the doubled template from start M -- the smaller start wins, then the smaller slot -- and the recording is
    cut at every position, so that the two starts lie on either side of the push boundary for every cut between them"""
    rng = np.random.default_rng(930)
    M, cap = 9, 6
    t = rng.integers(-3000, 3001, (M, 12)).astype(np.int16)
    tm = np.zeros((4, 2 * M + 1, 12), np.int16)
    tm[0, :M] = tm[1, :M] = t                       # two identical templates
    tm[2, :2 * M] = np.concatenate([t, t])          # the word said twice, as one template
    tm[3, :M] = rng.integers(-3000, 3001, (M, 12))  # something else
    tf = np.array([M, M, 2 * M, M], np.uint32)
    rows = [np.concatenate([t, t, t]), np.concatenate([t, t])]
    recs = [live.Recording(r, tm, tf, None, cap) for r in rows]
    assert recs[0].A[3 * M] == (0, M, 2) and recs[0].A[M] == (0, 0, 0) and recs[1].A[2 * M] == (0, 0, 2)
    rec, words = recs[0].row(3 * M)
    assert tuple(rec[()]) == (0, 2, 0, ref.CH_OK) and [tuple(w)[:4] for w in words[:2]] == [(0, 0, 0, M - 1), (2, 2, M, 3 * M - 1)]
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(tm, tf)
    im = np.zeros((2, MAXF, 12), np.int16)
    im[0, :3 * M], im[1, :2 * M] = rows[0], rows[1]
    whole = eng.decode_onepass(im, np.array([3 * M, 2 * M], np.uint32), cap)
    ses = eng.decode_onepass_live(2, 3 * M, 3 * M, cap)
    fol = Follower(ses, recs, "ties")
    for s in range(1, 3 * M):
        first = [s, min(s, 2 * M - 1)]
        for cnt, at in ((first, [0, 0]), ([3 * M - first[0], 2 * M - first[1]], first)):
            fol.take(push_counts(ses, rows, at, cnt), cnt)
        end = ses.end([0, 1])
        for c in range(2):
            same_row((end["rec"][c], end["words"][c]), (whole[0][c], whole[1][c]), f"cut {s}: end of channel {c} against decode_onepass")
        fol.count = [0, 0]
    ses.close()
    eng.close()


# ---- GPU 6: amplitude ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_amplitude_rows_whose_distances_wrap():
    fx = chain_ref.planted()
    tf = fx["tf"]
    big = np.array(fx["tm"])
    big[4, :tf[4]] = np.random.default_rng(900).integers(-30000, 30001, (tf[4], 12))  # squared differences that wrap u32
    f, n = planted_feats()
    f = [np.array(x) for x in f[:6]]  # UTT frames each
    assert n[2] >= 20 + tf[4]
    f[2][20:20 + tf[4]] = -big[4, :tf[4]]
    d2 = ((f[2][20:20 + tf[4]].astype(np.int64) - big[4, :tf[4]]) ** 2).sum(1)
    assert d2.max() >= 2 ** 32
    f[3] = np.random.default_rng(901).integers(-32768, 32768, (UTT, 12)).astype(np.int16)
    n = [UTT] * 6
    eng = Engine(max_frames=MAXF, device=0)
    eng.set_templates_dense(big, tf)
    recs = [live.Recording(f[c], big, tf, None, W, SKIP, 0) for c in range(6)]
    ses = eng.decode_onepass_live(6, 13, UTT, W, False, SKIP)
    fol = Follower(ses, recs, "full amplitude")
    feed(ses, fol, f, per_channel([random_chunking(np.random.default_rng(902 + c), n[c], 13) for c in range(6)]))
    im = np.zeros((6, MAXF, 12), np.int16)
    for c in range(6):
        im[c, :n[c]] = f[c]
    whole = eng.decode_onepass(im, np.array(n, np.uint32), W, SKIP, 0)
    for c in range(6):
        same_row(fol.last[c], (whole[0][c], whole[1][c]), f"channel {c} against decode_onepass")
    ses.close()
    eng.close()


# ---- GPU 7: end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_returns_the_parse_and_leaves_the_channel_fresh():
    f, n = planted_feats()
    f, recs = f[:6], [recording(c, SKIP, 0) for c in range(6)]
    eng = planted_engine()
    ses = eng.decode_onepass_live(6, 40, UTT, W, False, SKIP)
    fol = Follower(ses, recs, "end")
    assert ses.end([])["n_rows"] == 0
    cnt = [25, 30, 0, 40, 1, 0]
    fol.take(push_counts(ses, f, [0] * 6, cnt), cnt)
    out = ses.end([1, 5, 1, 3, 5, 1])  # channel 1 and 5 listed more than once; channel 5 is empty
    assert out["n_rows"] == 3 and [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(1, 30), (5, 0), (3, 40)]
    same_row((out["rec"][0], out["words"][0]), recs[1].row(30), "end of channel 1")
    same_row((out["rec"][2], out["words"][2]), recs[3].row(40), "end of channel 3")
    assert tuple(out["rec"][1]) == (DIS_ERR, 0, 0, ref.CH_NONE) and np.all(out["words"][1].view(np.uint32) == ONES)
    assert ses.frames.tolist() == [25, 0, 0, 0, 1, 0]
    fol.count = [25, 0, 0, 0, 1, 0]
    # channels 1, 3 and 5 start again at frame 0 (the same frames give the same rows: no key of the old recording is left);
    # channels 0 and 4 go on
    nxt = [15, 40, 0, 10, 39, 2]
    fol.take(push_counts(ses, f, [25, 0, 0, 0, 1, 0], nxt), nxt)
    out = ses.end(list(range(6)))
    assert [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(0, 40), (1, 40), (2, 0), (3, 10), (4, 40), (5, 2)]
    for r, (c, N) in enumerate([(0, 40), (1, 40), (3, 10), (4, 40), (5, 2)]):
        r += r >= 2
        same_row((out["rec"][r], out["words"][r]), recs[c].row(N), f"second end, channel {c}")
    assert out["rec"][2]["status"] == ref.CH_NONE and ses.frames.tolist() == [0] * 6
    assert ses.end([2, 2])["n_rows"] == 1
    ses.close()
    eng.close()


# ---- GPU 8: a replaced store -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_replaced_store_refuses_pushes_and_ends_as_none():
    fx = chain_ref.planted()
    f, n = planted_feats()
    f, recs = f[:4], [recording(c, SKIP, 0) for c in range(4)]
    eng = planted_engine()
    ses = eng.decode_onepass_live(4, 40, UTT, W, False, SKIP)
    fol = Follower(ses, recs, "replaced store")
    cnt = [40, 33, 0, 7]
    fol.take(push_counts(ses, f, [0] * 4, cnt), cnt)
    other = np.array(fx["tm"][::-1])  # another store: the slots in reverse order, one frame shorter each (L = 4)
    eng.set_templates_dense(other, np.array(fx["tf"][::-1]) - 1)
    with pytest.raises(engine.SrError, match="store changed"):
        push_counts(ses, f, cnt, [1, 0, 0, 0])
    with pytest.raises(engine.SrError, match="store changed"):
        push_counts(ses, f, cnt, [0, 0, 1, 0])  # an empty channel is bound as well
    assert ses.frames.tolist() == cnt and ses.push_dev(torch.zeros(4, 1, 12, dtype=torch.int16, device="cuda:0"), np.zeros(4, np.uint32))["n_rows"] == 0
    out = ses.end([0, 2])
    assert [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(0, 0), (2, 0)]
    assert np.all(out["rec"]["status"] == ref.CH_NONE) and np.all(out["words"].view(np.uint32) == ONES)
    with pytest.raises(engine.SrError, match="store changed"):
        push_counts(ses, f, cnt, [0, 1, 0, 0])  # channel 1 has not been ended
    # channels 0 and 2 are bound to the new store: they start again, and nothing of channel 0's old recording is left
    new = [live.Recording(f[c], other, np.array(fx["tf"][::-1]) - 1, None, W, SKIP, 0) for c in range(4)]
    fol = Follower(ses, new, "after the replacement")
    fol.count = [0, 33, 0, 7]
    for at, cnt in (([0, 33, 0, 7], [40, 0, 9, 0]), ([40, 33, 9, 7], [3, 0, 30, 0])):
        fol.take(push_counts(ses, f, at, cnt), cnt)
    out = ses.end([1, 3, 0])
    assert [(int(r["channel"]), int(r["frames"])) for r in out["rows"]] == [(1, 0), (3, 0), (0, 43)]
    same_row((out["rec"][2], out["words"][2]), new[0].row(43), "end of channel 0 under the new store")
    assert np.all(out["rec"][:2]["status"] == ref.CH_NONE)
    ses.close()
    eng.close()


# ---- GPU 9: PCM sessions ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pcm_sessions_equal_the_whole_path_on_the_whole_recording():
    rng = np.random.default_rng(800)
    R_MAXF, cap, skip = 119, 12, 3000
    eng = Engine(max_frames=R_MAXF, device=0)
    R = 1 + (R_MAXF - 1) * HOP + FRAME_LEN + 37  # 119 frames and a remainder
    X = (2048 + 600 * np.sin(np.arange(R)[None] * np.array([[0.05], [0.11]])) + rng.integers(-300, 301, (2, R))).astype(np.uint16)
    mid = np.array([2048, 2040], np.uint32)
    n, mf = eng.mfcc(X, [1, 1], [R, R], mid)
    assert list(n) == [R_MAXF, R_MAXF]
    tf = np.array([4, 5, 7, 12, 20, 16], np.uint32)  # L = 3: a push of 400 samples completes up to 5 frames, two blocks
    tm, valid = np.zeros((6, 21, 12), np.int16), np.array([1, 1, 1, 0, 1, 1], np.uint8)
    for k, (c, at) in enumerate(((0, 5), (1, 20), (0, 33), (1, 0), (1, 40), (0, 60))):
        tm[k, :tf[k]] = mf[c, at:at + tf[k]]
    eng.set_templates_dense(tm, tf, valid)
    whole = eng.decode_onepass_pcm(X, [1, 1], [R, R], mid, cap, skip, 0)
    assert np.all(whole["rec"]["status"] != ref.CH_NONE) and whole["rec"]["n_words"].min() >= 1  # (a row may hold more than cap words)
    recs = [live.Recording(mf[c, :R_MAXF], tm, tf, valid, cap, skip, 0) for c in range(2)]
    chunk_max = 400
    scheds = {True: [[1, 1]] * 200 + per_channel([cut(R - 200, [HOP - 1, HOP, FRAME_LEN, 400, 0, 237]), random_chunking(rng, R - 200, chunk_max)]),
              False: per_channel([cut(R, [400, 399, 1]), cut(R, [161, 80])])}
    for dev, sched in scheds.items():
        ses = eng.decode_onepass_live(2, chunk_max, R_MAXF, cap, False, skip, 0, mid)
        fol = Follower(ses, recs, f"pcm, dev {dev}")
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
            same_row(fol.last[c], (whole["rec"][c], whole["words"][c]), f"dev {dev}: channel {c} against decode_onepass_pcm")
        ses.close()
    eng.close()


# ---- GPU 10: ordering ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pushes_on_different_streams_and_host_pushes_are_ordered():
    """no synchronisation between the pushes: each runs behind the last one's event, whatever stream it is on; two runs give
    identical bytes"""
    fx = chain_ref.planted()
    f, n = planted_feats()
    N = UTT
    d_f = torch.from_numpy(np.array(fx["im"][:, :N])).cuda()
    sizes = cut(N, [7, 13, 1, 5, 11])
    edges = np.concatenate([[0], np.cumsum(sizes)])
    chunks = [d_f[:, a:b].contiguous() for a, b in zip(edges[:-1], edges[1:])]
    eng = planted_engine()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    runs = []
    for _ in range(2):
        ses = eng.decode_onepass_live(N_CH, 13, UTT, W, False, SKIP)
        fol = Follower(ses, [recording(c, SKIP, 0) for c in range(N_CH)], "streams")
        outs = []
        for i, chunk in enumerate(chunks):
            st = streams[i % 3]
            outs.append(ses.push_dev(chunk, stream=st) if st is not None else ses.push(np.array(fx["im"][:, edges[i]:edges[i + 1]])))
        torch.cuda.synchronize()
        blob = b""
        for size, out in zip(sizes, outs):
            fol.take(out, [size] * N_CH, session_is_here=False)  # (checked after the last push)
            blob += as_bytes(out)
        runs.append(blob)
        ses.close()
    assert runs[0] == runs[1]
    eng.close()


# ---- GPU 11: contracts -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_guards_and_refusals(canary):
    fx = chain_ref.planted()
    f, n = planted_feats()
    CH, CHUNK = 6, 30
    eng = planted_engine()
    ses = eng.decode_onepass_live(CH, CHUNK, UTT, W, False, SKIP)
    recs = [recording(c, SKIP, 0) for c in range(CH)]
    fol = Follower(ses, recs, f"guards, canary {canary:#x}")
    L, sid = eng.L, torch.cuda.current_stream().cuda_stream
    at = [0] * CH

    def push(cnt, max_rows, ok=True, null=None, overlap=False):
        F = max(max(cnt), 1)
        chunk = np.zeros((CH, F, 12), np.int16)
        for c in range(CH):
            k = min(cnt[c], UTT - at[c])
            chunk[c, :k] = f[c][at[c]:at[c] + k]
        d_chunk = torch.from_numpy(poison_feature_rows(chunk, np.minimum(cnt, F))).cuda()  # padded rows, poison past n[c]
        g_r = guarded_out((max_rows,), ref.CHAIN_REC_DTYPE, canary, 4096, "cuda:0", "rec")
        g_w = guarded_out((max_rows, W), ref.CHAIN_WORD_DTYPE, canary, 4096, "cuda:0", "words")
        rows, n_rows = np.full(max_rows + 1, 0x5A5A5A5A, np.uint32).repeat(2).view(live.CHAIN_LIVE_ROW_DTYPE), U32(0xDEAD)
        ptr = dict(mfcc=P(d_chunk.data_ptr()), rec=P(g_r.ptr), words=P(g_w.ptr), rows=engine._vp(rows))
        if null:
            ptr[null] = None
        if overlap:
            ptr["words"] = P(g_r.ptr + 16)
        before = ses.frames
        rc = L.sr_onepass_live_push_dev(ses.l, ptr["mfcc"], U64(F * 12), engine._vp(np.array(cnt, np.uint32)), U32(0), U32(max_rows), ptr["rec"],
                                        ptr["words"], ptr["rows"], C.byref(n_rows), P(sid))
        torch.cuda.synchronize()
        if not ok:
            assert rc == BAD_ARG and n_rows.value == 0xDEAD and np.all(rows.view(np.uint32) == 0x5A5A5A5A), (rc, cnt, L.sr_last_error())
            for g in (g_r, g_w):
                g.check_untouched()
            assert ses.frames.tolist() == before.tolist()
            return None
        assert rc == 0, L.sr_last_error()
        for g in (g_r, g_w):
            g.check()
        k = n_rows.value
        for g in (g_r, g_w):  # rows at and past *n_rows stay untouched
            assert np.all(g.interior().view(np.uint8).reshape(max_rows, -1)[k:] == canary)
        assert np.all(rows.view(np.uint32)[2 * k:] == 0x5A5A5A5A)
        ses._took(rows[:k])
        fol.take(dict(rec=g_r.interior()[:k], words=g_w.interior()[:k], rows=rows[:k], n_rows=k), cnt)
        for c in range(CH):
            at[c] += cnt[c]
        return k

    push([20, 17, 0, 30, 1, 6], 5 + 3)
    assert push([30] * CH, CH - 1, ok=False) is None and b"max_rows" in L.sr_last_error()             # max_rows too small
    assert push([CHUNK + 1, 1, 1, 1, 1, 1], 8, ok=False) is None and b"chunk_max" in L.sr_last_error()  # a count above chunk_max
    assert push([1] * CH, 8, ok=False, null="rec") is None and push([1] * CH, 8, ok=False, null="words") is None  # null required pointers
    assert push([1] * CH, 8, ok=False, null="rows") is None and push([1] * CH, 8, ok=False, null="mfcc") is None
    assert push([1] * CH, 8, ok=False, overlap=True) is None and b"overlap" in L.sr_last_error()        # overlapping outputs
    push([30] * CH, CH)
    push([25, 30, 30, 16, 30, 30], CH + 1)
    assert ses.frames.tolist() == [75, 77, 60, 76, 61, 66]
    assert push([1, 4, 1, 1, 1, 1], 8, ok=False) is None and b"utt_frames" in L.sr_last_error()         # past utt_frames
    eng.set_word_map(np.array([1, 2, 3], np.uint32))                                                     # a map for another store
    assert push([1] * CH, 8, ok=False) is None and b"word map" in L.sr_last_error()
    eng.set_word_map(None, 1)
    push([5, 3, 0, 4, 0, 7], 4)  # exactly utt_frames on channels 0, 1 and 3
    assert ses.frames.tolist() == [80, 80, 60, 80, 61, 73] and push([0] * CH, 1) == 0                    # nothing pushed, nothing refused
    # end: labels that lie inside the records are refused, nothing is written, the mirror stays
    blob = np.full(CH * (16 + W * 32 + 8), canary, np.uint8)
    ch, n_rows = np.arange(CH, dtype=np.uint32), U32(0xDEAD)
    at_w = blob.ctypes.data + CH * 16
    for rows_at in (blob.ctypes.data + 8, at_w + 32):
        assert L.sr_onepass_live_end(ses.l, engine._vp(ch), U32(CH), P(blob.ctypes.data), P(at_w), P(rows_at), C.byref(n_rows)) == BAD_ARG
        assert b"rows overlaps" in L.sr_last_error() and n_rows.value == 0xDEAD and np.all(blob == canary)
    assert L.sr_onepass_live_end(ses.l, engine._vp(np.array([CH], np.uint32)), U32(1), P(blob.ctypes.data), P(at_w), P(at_w + CH * W * 32),
                                 C.byref(n_rows)) == BAD_ARG and np.all(blob == canary)                 # a channel past the last
    assert ses.frames.tolist() == [80, 80, 60, 80, 61, 73]
    ses.close()
    # open: flags, words_cap, the ranges and the word-cost bound (L = 5: 3 276 words in 16 383 frames at most)
    out = C.c_void_p(0x5A5A)
    for bad in (dict(flags=2), dict(flags=3), dict(words_cap=0), dict(n_channels=0), dict(utt=0), dict(utt=16384), dict(chunk=0),
                dict(chunk=UTT + 1), dict(skip=65536), dict(wc=(1 << 24) + 1), dict(wc=(1 << 30) // (16383 // 5) + 1, utt=16383)):
        a = dict(n_channels=2, chunk=10, utt=UTT, words_cap=4, flags=0, skip=SKIP, wc=0)
        a.update(bad)
        assert L.sr_onepass_live_open(eng.h, U32(a["n_channels"]), U32(a["chunk"]), U32(a["utt"]), U32(a["words_cap"]), U32(a["flags"]),
                                      U32(a["skip"]), U32(a["wc"]), None, C.byref(out)) == BAD_ARG, bad
        assert not out.value
    assert b"2^30" in L.sr_last_error()
    eng.close()
