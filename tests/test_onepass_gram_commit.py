"""Committed words of a live one-pass grammar session: sr_onepass_gram_live_commit[_dev] (include/sr_engine.h, "live one-pass
grammar decoding", COMMITTED WORDS).

The rule: after any push, a commit call delivers the words every parse the channel's recording can still get begins with -- the
words on the walk from the commit node c(N) of tests/onepass_gram_commit_ref.py -- each exactly once over the calls, words_cap
at a time, also while the row of the push is still SR_CH_NONE.  The tests compare every sr_commit_rec and every word row byte
for byte with that reference at the channel's N, whatever the chunking, and the delivered words with the rows the library's own
end call returns.  No tolerances.  The store: K = 5 templates of 4 to 9 frames (W <= 17, L = 3); 4 channels with recordings of
120 frames, twelve planted words each without an immediate repeat; utt_frames 300.

Skipping is OFF in the grammar cases.  With skipping on, the start state of a grammar that no word leads back into is reachable
at every frame -- everything so far skipped -- and the walk from there is the root alone: a later parse may still begin that
way, so the rule, truthfully, commits nothing (test_skipping_on_keeps_the_start_state_reachable_and_commits_nothing).  The anchor
grammar, whose one state every word leads back into, commits under skipping as the session without a grammar does.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import onepass_gram_commit_ref as cref
import onepass_gram_live_ref as live
import onepass_gram_ref as gref
import onepass_ref as ref
import test_onepass_gram as t_opg
import wgram_ref
from guarded import CANARIES, guarded_out
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import COMMIT_REC_DTYPE, DIS_ERR, Engine
from test_onepass_commit import as_numpy, commit
from test_onepass_live import FRAME_LEN, HOP, cut, per_channel, push_counts, rows_of

BAD_ARG = 3
U32, P = C.c_uint32, C.c_void_p
SKIP = None  # skipping off: see the module's docstring
ANCHOR_SKIP = 1500
K, N_CH, N_REC, UTT, CAP = 5, 4, 120, 300, 16
LABELS = list(range(K))
ONES = 0xFFFFFFFF


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store():
    """-> dict(tm, tf, f = the channels' recordings [N_CH][N_REC, 12], seq = the planted slots per channel)"""
    rng = np.random.default_rng(1203)
    tf = np.array([4, 6, 7, 9, 5], np.uint32)
    tm = np.zeros((K, 10, 12), np.int16)
    for k in range(K):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    f, seq = [], []
    for c in range(N_CH):
        frames, slots = [], []
        while len(frames) < N_REC + 10:
            k = int(rng.choice([w for w in LABELS if not slots or w != slots[-1]]))
            slots.append(k)
            for _ in range(int(rng.integers(0, 3))):
                frames.append(rng.integers(-40, 41, 12))
            for y in range(int(tf[k])):
                frames.append(tm[k, y].astype(np.int64) + rng.integers(-60, 61, 12))
                if int(rng.integers(0, 6)) == 0:  # a template frame may last two input frames
                    frames.append(tm[k, y].astype(np.int64) + rng.integers(-60, 61, 12))
        f.append(np.array(frames[:N_REC], np.int16))
        seq.append(slots)
    for a in [tm, tf] + f:
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, f=f, seq=seq)


def grammars():
    """the five grammars, by name.  sequence: three positions of any word, final only behind the last.  Its states count words,
    so hypotheses of different counts never merge: nothing is shared until no state is reachable in the window any more (three
    words cover at most 51 frames), and then the fallback commits all three at once -- beside rows that say SR_CH_NONE, because
    without skipping a sequence of three words parses no longer recording.  pairs: a state per word, no immediate repeat, only words 0 and 1 may end; bigram: the same shape
    under drawn costs with some pairs forbidden"""
    rng = np.random.default_rng(88)
    cost = {a: {b: (None if a == b or (a, b) in ((0, 3), (4, 2)) else int(rng.integers(0, 4000))) for b in LABELS} for a in LABELS}
    return dict(sequence=wgram_ref.grammar_sequence([LABELS] * 3),
                repeat=gref.grammar_repeat([LABELS, LABELS], LABELS, 2),
                pairs=wgram_ref.grammar_word_pairs(LABELS, [(a, b) for a in LABELS for b in LABELS if a != b], last=[0, 1]),
                bigram=wgram_ref.grammar_bigram(LABELS, cost, [0, 500, 90, 0, 2500], [300, None, 0, 1200, None]),
                anchor=wgram_ref.grammar_any(LABELS))


GRAMS = grammars()
CAPS = dict(sequence=2)  # words_cap where it is not CAP: the three words of the sequence grammar drain over two calls


@functools.lru_cache(maxsize=None)
def recording(name, c, skip=SKIP, word_cost=0):
    fx = store()
    return live.Recording(GRAMS[name], fx["f"][c], fx["tm"], fx["tf"], None, CAP, skip, word_cost)


def store_engine(**kw):
    fx = store()
    eng = Engine(max_frames=UTT, device=0, **kw)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    return eng


class Committer:
    """the reference side of a session: per channel the history of its recording (a live.Recording under the grammar), the
    window, the kept states and a cursor; take() checks one commit call against the channels' N and keeps what was delivered"""

    def __init__(self, g_py, recs, tf, words_cap, what, valid=None, word_of_slot=None):
        wos = list(range(len(tf))) if word_of_slot is None else [int(w) for w in word_of_slot]
        self.recs, self.tf, self.what, self.word_of_slot = recs, tf, what, word_of_slot
        self.W, self.states = cref.window(g_py, tf, wos, valid), cref.kept_states(g_py, wos, valid)
        self.trees = [cref.Tree(r.A, r.E, g_py, r.word_cost, word_of_slot) for r in recs]
        self.cursors = [cref.Cursor(words_cap) for _ in recs]
        self.got = [[] for _ in recs]       # the delivered word rows, as bytes
        self.calls = [0] * len(recs)        # calls that delivered a word
        self.seen = {}                      # (channel, N) -> (n_committed, frames)

    @functools.lru_cache(maxsize=None)
    def committed(self, c, N):
        return self.trees[c].committed(N, self.W, self.states)

    def take(self, out, channels, frames):
        """channels: the distinct channels in the order the rows must have; frames: every channel's N"""
        crec, words, rows = as_numpy(out)
        assert out["n_rows"] == len(channels) and [(int(r["channel"]), int(r["frames"])) for r in rows] == [(c, frames[c]) for c in channels], \
            (self.what, rows, channels, frames)
        for r, c in enumerate(channels):
            node, all_words = self.committed(c, frames[c])
            rec, want, new = self.cursors[c].take(node, all_words, self.tf, self.word_of_slot)
            what = f"{self.what}: channel {c} at {frames[c]} frames"
            assert crec[r].tobytes() == rec.tobytes(), (what, crec[r], rec)
            assert words[r].tobytes() == want.tobytes(), (what, words[r], want)
            self.got[c] += [words[r][i].tobytes() for i in range(len(new))]
            self.calls[c] += bool(new)
            self.seen[(c, frames[c])] = (int(crec[r]["n_committed"]), int(crec[r]["frames"]))

    def ended(self, c):
        self.cursors[c].reset()
        self.got[c] = []


def chunkings():
    """one frame, 7, one block (L = 3), several blocks, everything at once"""
    return {"one frame": [1], "seven": [7], "one block": [3], "several blocks": [10, 23], "at once": [N_REC]}


# ---- GPU 1: chunkings, and the end row ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAMS))
def test_every_chunking_commits_the_same_words_at_the_same_frames(name):
    """a commit of every channel after every push, the device and the host form in turn; then the end call: its row begins with
    everything that was delivered"""
    fx = store()
    assert gref.reach(fx["tf"]) == 3
    eng = store_engine()
    g_py = GRAMS[name]
    gram = eng.grammar(*g_py)
    recs = [recording(name, c) for c in range(N_CH)]
    cap = CAPS.get(name, CAP)
    seen, none_beside_words = [], 0
    for how, sizes in chunkings().items():
        sched = per_channel([cut(N_REC, sizes)] * N_CH)
        ses = eng.decode_onepass_grammar_live(gram, N_CH, max(sizes), UTT, cap, False, SKIP)
        com = Committer(g_py, recs, fx["tf"], cap, f"{name}, chunking '{how}'")
        assert com.W == 17
        at = [0] * N_CH
        for i, cnt in enumerate(sched):
            rec, _ = rows_of(push_counts(ses, fx["f"], at, cnt))
            at = [a + b for a, b in zip(at, cnt)]
            out = commit(ses, ("dev", "host")[i % 2])
            com.take(out, list(range(N_CH)), at)
            none_beside_words += int(np.sum((rec["status"] == gref.CH_NONE) & (as_numpy(out)[0]["n_committed"] > 0)))
        assert at == [N_REC] * N_CH
        if how == "at once" and name == "sequence":
            com.take(commit(ses, "dev"), list(range(N_CH)), at)  # the backlog
        if how != "at once":  # not vacuous: every channel got at least two words over at least two calls
            assert all(len(g) >= 2 for g in com.got) and all(n >= 2 for n in com.calls), (how, [len(g) for g in com.got], com.calls)
        end = ses.end(list(range(N_CH)))
        for c in range(N_CH):
            want = recs[c].row(N_REC, cap)
            assert end["rec"][c].tobytes() == want[0].tobytes() and end["words"][c].tobytes() == want[1].tobytes()
            if end["rec"][c]["status"] != gref.CH_NONE:
                assert [end["words"][c][i].tobytes() for i in range(len(com.got[c]))] == com.got[c], (name, how, c)
            else:
                assert name == "sequence"
        seen.append(com.seen)
        ses.close()
    for other in seen[1:]:  # n_committed and frames at an N do not depend on how the channel got there
        for key in set(seen[0]) & set(other):
            assert seen[0][key] == other[key], key
    assert all((c, N_REC) in s for s in seen for c in range(N_CH))
    if name == "sequence":  # words were committed while the row of the push said SR_CH_NONE
        assert none_beside_words >= N_CH
    gram.close()
    eng.close()


# ---- GPU 2: backlog ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tail", [False, True], ids=["head", "tail"])
@pytest.mark.parametrize("cap", [1, 2])
def test_a_backlog_drains_in_order(cap, tail):
    """pushes of 40 frames commit several words at once against a words_cap of 1 or 2: the backlog drains words_cap at a time,
    and the calls go on after the last push until nothing is left.  The end row is the parse's first or (SR_OP_LIVE_TAIL) last
    words_cap words, and where it shows a delivered word it shows the delivered bytes"""
    fx = store()
    eng = store_engine()
    name = "bigram"
    g_py = GRAMS[name]
    gram = eng.grammar(*g_py)
    recs = [recording(name, c) for c in range(N_CH)]
    ses = eng.decode_onepass_grammar_live(gram, N_CH, 40, UTT, cap, tail, SKIP)
    com = Committer(g_py, recs, fx["tf"], cap, f"backlog, words_cap {cap}, tail {tail}")
    at, backlog = [0] * N_CH, 0
    for i in range(3):
        push_counts(ses, fx["f"], at, [40] * N_CH)
        at = [a + 40 for a in at]
        out = commit(ses, ("dev", "host")[i % 2])
        com.take(out, list(range(N_CH)), at)
        crec = as_numpy(out)[0]
        backlog += int(np.sum(crec["n_committed"] - crec["first"] > cap))
        assert np.all(crec["n_new"] == np.minimum(crec["n_committed"] - crec["first"], cap))
    final = [com.committed(c, N_REC)[1] for c in range(N_CH)]
    assert backlog >= N_CH and min(len(w) for w in final) >= 6
    for _ in range(max(len(w) for w in final) // cap + 2):  # until drained, and once more
        out = commit(ses, "dev")
        com.take(out, list(range(N_CH)), at)
    assert np.all(as_numpy(out)[0]["n_new"] == 0)
    for c in range(N_CH):
        assert com.got[c] == [w.tobytes() for w in cref.word_rows(final[c], fx["tf"], len(final[c]))] and len(set(com.got[c])) == len(final[c])
    end = ses.end(list(range(N_CH)))
    for c in range(N_CH):
        want = recs[c].row(N_REC, cap, tail)
        assert end["rec"][c].tobytes() == want[0].tobytes() and end["words"][c].tobytes() == want[1].tobytes()
        total = int(end["rec"][c]["n_words"])
        assert end["rec"][c]["status"] != gref.CH_NONE and len(com.got[c]) <= total
        first = total - cap if tail else 0  # the row shows the words first .. first + cap - 1 of the parse
        for i in range(cap):
            if first + i < len(com.got[c]):
                assert end["words"][c][i].tobytes() == com.got[c][first + i]
    ses.close()
    gram.close()
    eng.close()


# ---- GPU 3: a window of two rounds ---------------------------------------------------------------------------------------------------
WIDE_N = 200


@functools.lru_cache(maxsize=None)
def wide_fixture():
    """three templates of 36 to 40 frames (W = 79: two rounds of 64 positions) and one of 6; a recording of 200 frames of the
    long words with the short one between them, under a word-pair grammar: a state per word, so the walks that leave the
    window below its lower edge leave it in different states"""
    rng = np.random.default_rng(977)
    tf = np.array([40, 36, 38, 6], np.uint32)
    tm = np.zeros((4, 41, 12), np.int16)
    for k in range(4):
        tm[k, :tf[k]] = rng.integers(-3000, 3001, (tf[k], 12))
    tm[1, :20] = tm[0, :20]  # words 0 and 1 begin alike: which of them is heard is decided late
    frames, last = [], None
    for k in [0, 3, 1, 2, 3, 0, 1, 3, 2]:
        for y in range(int(tf[k])):
            frames.append(tm[k, y].astype(np.int64) + rng.integers(-60, 61, 12))
            if int(rng.integers(0, 9)) == 0:
                frames.append(tm[k, y].astype(np.int64) + rng.integers(-60, 61, 12))
    assert len(frames) >= WIDE_N
    f = np.array(frames[:WIDE_N], np.int16)
    g_py = wgram_ref.grammar_word_pairs(range(4), [(a, b) for a in range(4) for b in range(4) if a != b])
    for a in (tm, tf, f):
        a.setflags(write=False)
    return dict(tm=tm, tf=tf, f=f, gram=g_py, rec=live.Recording(g_py, f, tm, tf, None, 16, SKIP, 0))


def leaving(tree, N, W, states):
    """the nodes inside the window whose word starts below it, over all entry walks: where a walk leaves the window"""
    lo, out = max(0, N - W), set()
    for x, s in cref.entries(tree.A, tree.E, N, W, states)[0]:
        out |= {n for n in tree.walk(x, s)[:-1] if n[0] >= lo and tree.word_at(n)[1][0] < lo}
    return out


@pytest.mark.gpu
def test_a_wide_window_whose_walks_leave_it_in_different_states():
    fx = wide_fixture()
    g_py, rec = fx["gram"], fx["rec"]
    eng = Engine(max_frames=WIDE_N, device=0)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    gram = eng.grammar(*g_py)
    com = Committer(g_py, [rec], fx["tf"], 16, "wide window")
    assert com.W == 79 and gref.reach(fx["tf"]) == 4
    sizes = cut(WIDE_N, [50, 37, 64, 1, 30])
    ends = np.cumsum(sizes).tolist()
    # from the reference: at an N of this schedule past the first round the walks leave the window in more than one state
    split = [N for N in ends if N > 64 + com.W and len({t for _, t in leaving(com.trees[0], N, com.W, com.states)}) > 1]
    assert split, [len(leaving(com.trees[0], N, com.W, com.states)) for N in ends]
    ses = eng.decode_onepass_grammar_live(gram, 1, 64, WIDE_N, 16, False, SKIP)
    at = 0
    for i, size in enumerate(sizes):
        push_counts(ses, [fx["f"]], [at], [size])
        at += size
        com.take(commit(ses, ("dev", "host")[i % 2]), [0], [at])
    assert len(com.got[0]) >= 2 and com.calls[0] >= 2
    end = ses.end([0])
    assert end["rec"][0]["status"] != gref.CH_NONE and [end["words"][0][i].tobytes() for i in range(len(com.got[0]))] == com.got[0]
    ses.close()
    gram.close()
    eng.close()


# ---- GPU 4: the anchor grammar, and the pruning hook ----------------------------------------------------------------------------------
def commit_blob(ses, f, sizes, n_ch):
    """the bytes of every commit call (records, word rows, row labels) of a session fed in pushes of `sizes`"""
    at, blob = [0] * n_ch, b""
    for i, cnt in enumerate(per_channel([cut(N_REC, sizes)] * n_ch)):
        push_counts(ses, f, at, cnt)
        at = [a + b for a, b in zip(at, cnt)]
        crec, words, rows = as_numpy(commit(ses, ("dev", "host")[i % 2]))
        blob += crec.tobytes() + np.ascontiguousarray(words).tobytes() + rows.tobytes()
    return blob


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [2, CAP])
def test_the_anchor_grammar_gives_the_one_pass_sessions_commit_bytes(cap):
    fx = store()
    eng = store_engine()
    gram = eng.grammar(*GRAMS["anchor"])
    for skip, wc in ((ANCHOR_SKIP, 0), (None, 5000)):
        blobs = []
        for ses in (eng.decode_onepass_grammar_live(gram, N_CH, 23, UTT, cap, False, skip, wc), eng.decode_onepass_live(N_CH, 23, UTT, cap, False, skip, wc)):
            blobs.append(commit_blob(ses, fx["f"], [23, 5, 1], N_CH))
            ses.close()
        assert blobs[0] == blobs[1], (cap, skip, wc)
        last = np.frombuffer(blobs[0][-(N_CH * 16 + N_CH * cap * 32 + N_CH * 8):][:N_CH * 16], COMMIT_REC_DTYPE)
        assert skip is None or last["n_committed"].min() >= 4  # words were compared
    gram.close()
    eng.close()


@pytest.mark.gpu
def test_the_pruning_hook_changes_no_commit_byte():
    """state 3 is unreachable (and kept all the same: a kept charge list names it), state 4 is reachable and reaches no final
    state (so it is swept under the hook and never kept); two slots per word under a word map.  The commit rule ranges over the grammar's static lists whatever the hook says"""
    fx = store()
    graph = (5, [(0, 1, 0), (1, 2, 1), (3, 2, 2), (1, 4, 2), (4, 4, 2), (2, 2, 1), (2, 1, 0), (2, 2, 2)], [0, 0, 1, 0, 0],
             [0, 900, 5, 0, 0, 40, 7, 60], [0, 0, 300, 0, 0])
    wmap = np.array([0, 0, 1, 1, 2], np.uint32)
    items, states = gref.kept(graph, wmap.tolist())
    assert states == [0, 1, 2, 3] and len(items) < len(gref.items_of(graph, [1] * K, wmap))
    eng = store_engine(testing=True)
    eng.set_word_map(wmap)
    gram = eng.grammar(*graph)
    recs = [live.Recording(graph, fx["f"][c], fx["tm"], fx["tf"], None, CAP, SKIP, 0, word_of_slot=wmap) for c in range(N_CH)]
    blobs = []
    for off in (0, 1):
        with t_opg.hooks(prune_off=off):
            assert engine.onepass_grammar_live_geometry(gram, UTT, 13)["states"] == (5 if off else 4)
            ses = eng.decode_onepass_grammar_live(gram, N_CH, 13, UTT, CAP, False, SKIP)
        com = Committer(graph, recs, fx["tf"], CAP, f"prune_off {off}", word_of_slot=wmap)
        at, blob = [0] * N_CH, b""
        for i, cnt in enumerate(per_channel([cut(N_REC, [13, 4])] * N_CH)):
            push_counts(ses, fx["f"], at, cnt)
            at = [a + b for a, b in zip(at, cnt)]
            out = commit(ses, ("dev", "host")[i % 2])
            com.take(out, list(range(N_CH)), at)
            crec, words, rows = as_numpy(out)
            blob += crec.tobytes() + np.ascontiguousarray(words).tobytes() + rows.tobytes()
        assert sum(len(g) >= 2 for g in com.got) >= 2, [len(g) for g in com.got]
        blobs.append(blob)
        ses.close()
    assert blobs[0] == blobs[1]
    gram.close()
    eng.close()


# ---- GPU 5: lists, streams, a new recording, a new grammar -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lists_empty_channels_repeated_calls_streams_a_new_recording_and_a_new_grammar():
    fx = store()
    f = fx["f"]
    eng = store_engine()
    name = "pairs"
    gram = eng.grammar(*GRAMS[name])
    recs = [recording(name, c) for c in range(N_CH)]
    ses = eng.decode_onepass_grammar_live(gram, N_CH, N_REC, UTT, CAP, False, SKIP)
    com = Committer(GRAMS[name], recs, fx["tf"], CAP, "edges")
    assert ses.commit([])["n_rows"] == 0 and ses.commit_dev([])["n_rows"] == 0
    at = [0] * N_CH
    com.take(ses.commit_dev(), list(range(N_CH)), at)  # every channel empty
    cnt = [10, 0, 17, 0]
    push_counts(ses, f, at, cnt)
    at = list(cnt)
    out = ses.commit_dev([2, 0, 2, 1, 0])  # listed twice, an empty channel; N <= W = 17 everywhere
    com.take(out, [2, 0, 1], at)
    crec, words, _ = as_numpy(out)
    assert crec.tobytes() == bytes(48) and np.all(words.view(np.uint32) == ONES)
    # the rest on one stream, the commit on another, the next push on the first again: no synchronisation in between
    s_push, s_commit = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for step in ([40] * N_CH, [N_REC - a - 40 for a in at]):
        chunk = np.zeros((N_CH, max(step), 12), np.int16)
        for c in range(N_CH):
            chunk[c, :step[c]] = f[c][at[c]:at[c] + step[c]]
        ses.push_dev(torch.from_numpy(chunk).cuda(), np.array(step, np.uint32), stream=s_push)
        at = [a + b for a, b in zip(at, step)]
        outs.append((ses.commit_dev(stream=s_commit), list(at)))
    torch.cuda.synchronize()
    for out, frames in outs:
        com.take(out, list(range(N_CH)), frames)
    assert at == [N_REC] * N_CH and all(len(g) >= 2 for g in com.got)
    # no push in between: the same count, nothing new -- in both forms
    before = {c: len(g) for c, g in enumerate(com.got)}
    for form in ("dev", "host"):
        out = commit(ses, form, [3, 1])
        com.take(out, [3, 1], at)
        crec = as_numpy(out)[0]
        assert np.all(crec["n_new"] == 0) and np.all(crec["first"] == crec["n_committed"]) and crec["n_committed"].tolist() == [before[3], before[1]]
    # the end call returns what it always did; channels 1 and 3 start again at first = 0, channel 0 keeps its cursor
    end = ses.end([1, 3])
    for r, c in enumerate((1, 3)):
        want = recs[c].row(N_REC)
        assert end["rec"][r].tobytes() == want[0].tobytes() and end["words"][r].tobytes() == want[1].tobytes()
        com.ended(c)
    at[1] = at[3] = 0
    com.take(ses.commit([1, 0, 3]), [1, 0, 3], at)
    push_counts(ses, f, at, [0, N_REC, 0, N_REC])
    at[1] = at[3] = N_REC
    out = ses.commit_dev([3, 1, 0])
    com.take(out, [3, 1, 0], at)
    crec = as_numpy(out)[0]
    assert crec["first"].tolist() == [0, 0, before[0]] and crec["n_new"].tolist() == [before[3], before[1], 0]
    # another grammar, with other states and another window's worth of kept items: the cursors start at zero under it
    ses.end(list(range(N_CH)))
    name = "bigram"
    other = eng.grammar(*GRAMS[name])
    ses.set_grammar(other)
    recs = [recording(name, c) for c in range(N_CH)]
    com = Committer(GRAMS[name], recs, fx["tf"], CAP, "after set_grammar")
    at = [0] * N_CH
    com.take(ses.commit_dev(), list(range(N_CH)), at)
    for cnt in ([70, 33, 0, 120], [50, 0, 9, 0]):
        push_counts(ses, f, at, cnt)
        at = [a + b for a, b in zip(at, cnt)]
        com.take(ses.commit_dev(), list(range(N_CH)), at)
    assert len(com.got[0]) >= 2 and len(com.got[3]) >= 2 and not com.got[2]
    ses.close()
    for g in (gram, other):
        g.close()
    eng.close()


# ---- GPU 6: a stale grammar, and a grammar that keeps nothing ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["store", "word map"])
def test_a_stale_grammar_refuses_and_its_dropped_recordings_reset_the_cursor(how):
    fx = store()
    f = fx["f"]
    eng = store_engine()
    name = "repeat"
    gram = eng.grammar(*GRAMS[name])
    ses = eng.decode_onepass_grammar_live(gram, N_CH, N_REC, UTT, CAP, False, SKIP)
    recs = [recording(name, c) for c in range(N_CH)]
    com = Committer(GRAMS[name], recs, fx["tf"], CAP, f"stale grammar ({how})")
    at = [90, 0, 120, 60]
    push_counts(ses, f, [0] * N_CH, at)
    com.take(ses.commit_dev([0]), [0], at)  # channel 0 has delivered, channels 2 and 3 have not
    assert len(com.got[0]) >= 2
    if how == "store":
        eng.set_templates_dense(fx["tm"], fx["tf"])  # the same templates: a new store all the same
    else:
        eng.set_word_map(None, 1)
    says = "template store" if how == "store" else "word map"
    for channels in ([0], [1], [], [N_CH + 3]):  # whatever is listed, an empty channel and nothing at all included: the grammar is the session's
        for fn in (ses.commit, ses.commit_dev):
            with pytest.raises(engine.SrError, match=says):
                fn(channels)
    out = ses.end(list(range(N_CH)))  # dropped: the NONE record, frames 0
    assert [tuple(r) for r in out["rec"]] == [(DIS_ERR, 0, 0, gref.CH_NONE)] * N_CH
    fresh = eng.grammar(*GRAMS[name])
    ses.set_grammar(fresh)
    com = Committer(GRAMS[name], recs, fx["tf"], CAP, f"after the replacement ({how})")
    at = [0] * N_CH
    com.take(ses.commit_dev(), list(range(N_CH)), at)  # all zero: nothing of the dropped recordings is left in a cursor
    push_counts(ses, f, at, [120, 90, 0, 60])
    at = [120, 90, 0, 60]
    out = ses.commit()
    com.take(out, list(range(N_CH)), at)
    assert np.all(as_numpy(out)[0]["first"] == 0) and len(com.got[0]) >= 2 and len(com.got[1]) >= 2
    ses.close()
    for g in (gram, fresh):
        g.close()
    eng.close()


@pytest.mark.gpu
def test_a_grammar_that_keeps_nothing_commits_nothing():
    fx = store()
    g_py = (3, [(1, 2, 0), (0, 0, 1)], [0, 0, 1])  # the final state cannot be reached from state 0
    assert gref.kept(g_py, LABELS) == ([], [])
    eng = store_engine()
    gram = eng.grammar(*g_py)
    ses = eng.decode_onepass_grammar_live(gram, N_CH, N_REC, UTT, CAP, False, SKIP)
    recs = [live.Recording(g_py, fx["f"][c], fx["tm"], fx["tf"], None, CAP, SKIP, 0) for c in range(N_CH)]
    com = Committer(g_py, recs, fx["tf"], CAP, "nothing kept")
    assert com.W == 0 and com.states == []
    at = [0] * N_CH
    for cnt in ([50, 0, 120, 7], [70, 0, 0, 1]):
        push_counts(ses, fx["f"], at, cnt)
        at = [a + b for a, b in zip(at, cnt)]
        for form in ("dev", "host"):
            out = commit(ses, form)
            com.take(out, list(range(N_CH)), at)
            crec, words, _ = as_numpy(out)
            assert crec.tobytes() == bytes(16 * N_CH) and np.all(words.view(np.uint32) == ONES)
    ses.close()
    gram.close()
    eng.close()


@pytest.mark.gpu
def test_skipping_on_keeps_the_start_state_reachable_and_commits_nothing():
    """no word leads back into the start state of the word-pair grammar, and with skipping on it is reachable at every frame:
    the walk from there is the root, a later parse may begin with everything skipped, nothing is final.  The parse itself is
    there all the while"""
    fx = store()
    name = "pairs"
    eng = store_engine()
    gram = eng.grammar(*GRAMS[name])
    recs = [recording(name, c, ANCHOR_SKIP) for c in range(N_CH)]
    assert all(r.E[0][N] == N * ANCHOR_SKIP for r in recs for N in (1, N_REC))
    ses = eng.decode_onepass_grammar_live(gram, N_CH, 50, UTT, CAP, False, ANCHOR_SKIP)
    com = Committer(GRAMS[name], recs, fx["tf"], CAP, "skipping on")
    at = [0] * N_CH
    for i, n in enumerate((50, 50, 20)):
        rec, _ = rows_of(push_counts(ses, fx["f"], at, [n] * N_CH))
        at = [a + n for a in at]
        out = commit(ses, ("dev", "host")[i % 2])
        com.take(out, list(range(N_CH)), at)
        assert as_numpy(out)[0].tobytes() == bytes(16 * N_CH) and np.all(rec["n_words"] >= 4)
    ses.close()
    gram.close()
    eng.close()


# ---- GPU 7: a sequence grammar without skipping takes the fallback -------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_empty_window_takes_the_fallback():
    """skipping off under a sequence grammar of two words: once both have ended and the longest word's reach is over, no kept
    state is reachable in the window, and the entries are the states reachable at the last position that has one"""
    fx = store()
    g_py = wgram_ref.grammar_sequence([LABELS, LABELS])
    eng = store_engine()
    gram = eng.grammar(*g_py)
    recs = [live.Recording(g_py, fx["f"][c], fx["tm"], fx["tf"], None, CAP, None, 0) for c in range(N_CH)]
    com = Committer(g_py, recs, fx["tf"], CAP, "fallback")
    taken = [N for N in (30, 60, 61, N_REC) if cref.entries(recs[0].A, recs[0].E, N, com.W, com.states)[1]]
    assert taken and 30 not in taken
    ses = eng.decode_onepass_grammar_live(gram, N_CH, 60, UTT, CAP, False, None)
    at = [0] * N_CH
    for i, n in enumerate((30, 30, 1, 59)):
        push_counts(ses, fx["f"], at, [n] * N_CH)
        at = [a + n for a in at]
        com.take(commit(ses, ("dev", "host")[i % 2]), list(range(N_CH)), at)
    assert all(len(g) == 2 for g in com.got)  # the fallback commits both words: nothing else can be heard any more
    ses.close()
    gram.close()
    eng.close()


# ---- GPU 8: PCM ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_pcm_session_commits_what_its_frames_commit():
    rng = np.random.default_rng(800)
    R_MAXF, cap, skip = 119, 12, None
    eng = Engine(max_frames=R_MAXF, device=0)
    R = 1 + (R_MAXF - 1) * HOP + FRAME_LEN + 37
    X = (2048 + 600 * np.sin(np.arange(R)[None] * np.array([[0.05], [0.11]])) + rng.integers(-300, 301, (2, R))).astype(np.uint16)
    mid = np.array([2048, 2040], np.uint32)
    n, mf = eng.mfcc(X, [1, 1], [R, R], mid)
    assert list(n) == [R_MAXF, R_MAXF]
    tf = np.array([4, 5, 7, 12, 20, 16], np.uint32)
    tm, valid = np.zeros((6, 21, 12), np.int16), np.array([1, 1, 1, 0, 1, 1], np.uint8)
    for k, (c, at) in enumerate(((0, 5), (1, 20), (0, 33), (1, 0), (1, 40), (0, 60))):
        tm[k, :tf[k]] = mf[c, at:at + tf[k]]
    eng.set_templates_dense(tm, tf, valid)
    g_py = wgram_ref.with_costs(gref.grammar_repeat([range(6)], range(6), 0), np.arange(12) * 37, [0, 11])
    gram = eng.grammar(*g_py)
    recs = [live.Recording(g_py, mf[c, :R_MAXF], tm, tf, valid, cap, skip, 0) for c in range(2)]
    com = Committer(g_py, recs, tf, cap, "pcm", valid)
    assert com.W == 39  # the invalid slot of 12 frames does not count, the one of 20 does
    ses = eng.decode_onepass_grammar_live(gram, 2, 800, R_MAXF, cap, False, skip, 0, mid)
    got = [0, 0]
    for i, cnt in enumerate(per_channel([cut(R, [800, 399, 1]), cut(R, [161, 640])])):
        S = (max(max(cnt), 1) + 7) // 8 * 8
        chunk = np.full((2, S), 4095, np.uint16)
        for c in range(2):
            chunk[c, :cnt[c]] = X[c, got[c]:got[c] + cnt[c]]
        ses.push_pcm_dev(torch.from_numpy(chunk.view(np.int16)).cuda(), np.array(cnt, np.uint32))
        got = [g + v for g, v in zip(got, cnt)]
        com.take(commit(ses, ("dev", "host")[i % 2]), [0, 1], [live.pcm_frames(g, FRAME_LEN, HOP) for g in got])
    assert got == [R, R] and all(len(g) >= 2 for g in com.got)
    end = ses.end([0, 1])
    for c in range(2):
        assert [end["words"][c][i].tobytes() for i in range(len(com.got[c]))] == com.got[c]
    ses.close()
    gram.close()
    eng.close()


# ---- GPU 9: guards and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("canary", CANARIES)
def test_guards_and_refusals(canary):
    fx = store()
    f = fx["f"]
    eng = store_engine()
    name = "bigram"
    gram = eng.grammar(*GRAMS[name])
    ses = eng.decode_onepass_grammar_live(gram, N_CH, N_REC, UTT, CAP, False, SKIP)
    recs = [recording(name, c) for c in range(N_CH)]
    com = Committer(GRAMS[name], recs, fx["tf"], CAP, f"guards, canary {canary:#x}")
    L, sid = eng.L, torch.cuda.current_stream().cuda_stream
    at = [60, 110, 0, 120]
    push_counts(ses, f, [0] * N_CH, at)

    def call(form, channels, room, ok=True, null=None, overlap=False, want=None):
        """one raw call with guarded outputs of `room` rows; ok: checked against the reference; else refused, nothing written"""
        device = "cuda:0" if form == "dev" else None
        g_c = guarded_out((room,), COMMIT_REC_DTYPE, canary, 4096, device, "crec")
        g_w = guarded_out((room, CAP), ref.CHAIN_WORD_DTYPE, canary, 4096, device, "cwords")
        rows, n_rows = np.full(room + 1, 0x5A5A5A5A, np.uint32).repeat(2).view(live.CHAIN_LIVE_ROW_DTYPE), U32(0xDEAD)
        ch = np.array(channels, np.uint32)
        ptr = dict(channels=engine._vp(ch), crec=P(g_c.ptr), cwords=P(g_w.ptr), rows=engine._vp(rows))
        if null:
            ptr[null] = None
        if overlap == "words":
            ptr["cwords"] = P(g_c.ptr + 16)
        if overlap == "rows":
            ptr["rows"] = P(g_w.ptr + 32)
        args = [ses.l, ptr["channels"], U32(len(ch)), ptr["crec"], ptr["cwords"], ptr["rows"], C.byref(n_rows)]
        rc = L.sr_onepass_gram_live_commit_dev(*args, P(sid)) if form == "dev" else L.sr_onepass_gram_live_commit(*args)
        torch.cuda.synchronize()
        if not ok:
            assert rc == BAD_ARG and n_rows.value == 0xDEAD and np.all(rows.view(np.uint32) == 0x5A5A5A5A), (rc, channels, L.sr_last_error())
            for g in (g_c, g_w):
                g.check_untouched()
            return L.sr_last_error()
        assert rc == 0, L.sr_last_error()
        for g in (g_c, g_w):
            g.check()
        k = n_rows.value
        assert k == len(want)
        for g in (g_c, g_w):  # rows at and past *n_rows stay untouched
            assert np.all(g.interior().view(np.uint8).reshape(room, -1)[k:] == canary)
        assert np.all(rows.view(np.uint32)[2 * k:] == 0x5A5A5A5A)
        com.take(dict(crec=g_c.interior()[:k], words=g_w.interior()[:k], rows=rows[:k], n_rows=k), want, at)
        return None

    for form in ("dev", "host"):
        call(form, [3, 1, 3, 2], 3 + 3, want=[3, 1, 2])
        call(form, [], 2, null="channels", want=[])  # nothing listed: no pointer is needed
        for null in ("channels", "crec", "cwords", "rows"):
            assert b"null" in call(form, [0, 1], 4, ok=False, null=null)
        assert b"past the session's last" in call(form, [0, N_CH], 4, ok=False)
        assert b"overlap" in call(form, [0, 1, 2], 4, ok=False, overlap="words")
    assert b"rows overlaps" in call("host", [0, 1, 2], 4, ok=False, overlap="rows")
    call("dev", list(range(N_CH)), N_CH, want=list(range(N_CH)))  # the refusals changed no cursor
    assert len(com.got[1]) >= 2 and len(com.got[3]) >= 2
    # a stale grammar refuses first: before the null pointer, the stranger and the overlap are looked at
    eng.set_word_map(np.array([1, 2, 3], np.uint32))  # a map for another store: the grammar is stale, and the map does not fit
    for form in ("dev", "host"):
        assert b"word map changed" in call(form, [0], 2, ok=False)
        assert b"word map changed" in call(form, [0, N_CH], 2, ok=False, null="crec")
        assert b"word map changed" in call(form, [0, 1], 2, ok=False, overlap="words")
    ses.close()
    gram.close()
    eng.close()
