"""The commit rule of a live one-pass grammar session (tests/onepass_gram_commit_ref.py) held against what it promises, on the
CPU, over random small grammars (weighted included) and random distance tables: the committed words are a prefix of every later
parse, the commit node never moves back, the block form and the time-synchronous form of the history commit alike, the anchor
grammar commits what the session without a grammar commits, the window really bounds the starts alive in the exact column --
and the cases the rule exists for are all seen.  Also the surface of the feature, and the host-only planning of a commit call
(csrc/sr_onepass_gram_commit_plan.h) under the sanitizers.  No device; tests/test_onepass_gram_commit.py compares the kernels
with this restatement byte for byte.
"""
import functools
import os
import re
import subprocess

import numpy as np

import onepass_commit_ref as cref0
import onepass_gram_commit_ref as cref
import onepass_gram_ref as gref
import onepass_ref as ref
import wgram_ref
from stm32_speech_recognition_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sr_engine.h")
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
N_MAX = 26
SEEDS = range(48)


# ---- the surface (fails without the feature) -----------------------------------------------------------------------------------
def test_header_declares_the_two_calls_and_both_libraries_export_them():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn in ("sr_onepass_gram_live_commit_dev", "sr_onepass_gram_live_commit"):
        assert re.search(r"\bint %s\s*\(" % fn, src), fn
        for testing in (False, True):
            assert hasattr(engine.load_library(testing), fn), (fn, testing)
    gram_section = text[text.index("live one-pass grammar decoding: state carried between pushes"):]
    assert "COMMITTED WORDS" in gram_section and "WHILE THE ROW ITSELF IS STILL SR_CH_NONE" in gram_section
    assert "commits in grammar sessions" not in text and "a follow-up" not in gram_section  # the two mentions this closes
    ses = engine.OnePassGrammarSession
    assert ses.commit is engine.OnePassSession.commit and ses.commit_dev is engine.OnePassSession.commit_dev  # inherited, through _PREFIX
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "sr_onepass_gram_commit_plan.h" in mk
    kern = open(os.path.join(CSRC, "k_onepass_gram_live.hip")).read()
    for k in ("k_onepass_gram_live_commit", "k_onepass_gram_live_commit_w"):
        assert 'SR_LAUNCH_POINT(s, "%s");' % k in kern, k


# ---- random small cases --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(seed):
    """a random grammar over a random store of 2..4 templates of 2..4 frames, a random distance table of N_MAX frames"""
    rng = np.random.default_rng(9000 + seed)
    K = int(rng.integers(2, 5))
    tf = [int(m) for m in rng.integers(2, 5, K)]
    n_words = int(rng.integers(2, K + 1))
    wos = [int(w) for w in rng.permutation(K) % n_words]
    S = int(rng.integers(2, 6))
    arcs = [(s, t, w) for s in range(S) for t in range(S) for w in range(n_words) if rng.random() < 0.22]
    if not any(s == 0 for s, _, _ in arcs):
        arcs.insert(0, (0, 1, 0))
    final = [int(rng.random() < 0.4) for _ in range(S)]
    if not any(final[1:]):
        final[S - 1] = 1
    gram = (S, arcs, final)
    if seed % 3 == 0:
        gram = wgram_ref.drawn_costs(gram, seed, 60)
    skip = None if seed % 2 else int(rng.integers(5, 80))
    word_cost = (0, 9)[(seed // 2) % 2]
    dis = [rng.integers(0, 50, (N_MAX, m)).astype(np.int64) for m in tf]
    return dict(gram=gram, tf=tf, wos=wos, skip=skip, word_cost=word_cost, dis=dis)


def words_differ(tree, a, b):
    return [tree.word_at(n)[0] for n in tree.walk(*a)[:-1]] != [tree.word_at(n)[0] for n in tree.walk(*b)[:-1]]


def check_case(cs, seen, what):
    gram, tf, wos, skip, wc, dis = (cs[k] for k in ("gram", "tf", "wos", "skip", "word_cost", "dis"))
    items, states = gref.kept(gram, wos)
    W = cref.window(gram, tf, wos)
    assert W == (2 * max(tf[k] for k, _ in items) - 1 if items else 0)
    A, E = gref.history_sync(gram, dis, N_MAX, skip, wc, wos)
    # the window: only kept items are swept, and every hypothesis alive in column N - 1 started at or after N - W
    Ak, Ek, starts = cref.history_with_starts(gram, dis, N_MAX, skip, wc, wos, keep=set(items))
    assert all(Ak[t] == A[t] and Ek[t] == E[t] for t in states), what
    for N in range(1, N_MAX + 1):
        assert all(x >= N - W for x in starts[N - 1]), (what, N, W, sorted(starts[N - 1])[:3])
    # the block form of the history commits what the time-synchronous form commits
    L = gref.reach(tf)
    Ab, Eb = gref.history_blocks(gram, dis, N_MAX, max(L, 1), skip, wc, wos)
    tree, tree_b = cref.Tree(A, E, gram, wc, wos), cref.Tree(Ab, Eb, gram, wc, wos)
    parses = [gref.trace_row(A, E, N, gram, wc, wos) for N in range(N_MAX + 1)]
    reachable = [s for s in range(gram[0]) if any(e is not None for e in E[s])]
    last = cref.ROOT
    for N in range(N_MAX + 1):
        c, words = tree.committed(N, W, states)
        assert tree_b.committed(N, W, states) == (c, words), (what, N)
        assert c == cref.commit_node(A, E, N, W, gram, states, wos)  # the module-level form
        assert last[0] <= c[0] <= N and last in tree.walk(*c), (what, N, c, last)  # never back, and on the same chain
        last = c
        for later in range(N, N_MAX + 1):
            if parses[later]["status"] != gref.CH_NONE:
                assert parses[later]["words"][:len(words)] == words, (what, N, later, words, parses[later]["words"])
        ent, fallback = cref.entries(A, E, N, W, states)
        if words and parses[N]["status"] == gref.CH_NONE:
            seen.setdefault("a", what)
        if any(a[0] == b[0] and a[1] != b[1] and words_differ(tree, a, b) for a in ent for b in ent):
            seen.setdefault("b", what)
        if fallback and N:
            seen.setdefault("c", what)
            assert len({x for x, _ in ent}) <= 1 and all(x < N - W for x, _ in ent)
        if set(reachable) - set(states) and tree.commit_node(N, W, reachable) != c:
            seen.setdefault("d", what)


def test_random_grammars_commit_only_what_every_later_parse_keeps_and_every_case_is_seen():
    """(a) words are committed while the row is CH_NONE; (b) two entries at one position in different states whose walks differ
    in a word; (c) the fallback of an empty window is taken; (d) a state that is reachable but not kept would have changed c,
    had it been counted.  Conditions on the inputs, found by this search over the seeds"""
    seen = {}
    for seed in SEEDS:
        check_case(case(seed), seen, f"seed {seed}")
    assert sorted(seen) == ["a", "b", "c", "d"], seen


def test_the_anchor_grammar_commits_what_the_session_without_a_grammar_commits():
    total = 0
    for seed in SEEDS[:16]:
        cs = case(seed)
        tf, skip, wc, dis = cs["tf"], cs["skip"], cs["word_cost"], cs["dis"]
        gram = wgram_ref.grammar_any(list(range(len(tf))))
        A, E = gref.history_sync(gram, dis, N_MAX, skip, wc)
        A0, E0 = ref.history_sync(dis, N_MAX, skip, wc)
        assert A[0] == A0 and E[0] == E0
        W = cref.window(gram, tf, list(range(len(tf))))
        assert W == cref0.window(tf) and cref.kept_states(gram, list(range(len(tf)))) == [0]
        tree = cref.Tree(A, E, gram, wc)
        n_words = 0
        for N in range(N_MAX + 1):
            c, words = tree.committed(N, W, [0])
            c0, words0 = cref0.committed(A0, E0, N, W, wc)
            assert c == (c0, 0) and [w[:5] for w in words] == words0 and all(w[5] == 0 for w in words), (seed, N)
            n_words = len(words)
        total += n_words
    assert total >= 16  # words were compared


def test_cursor_delivers_every_committed_word_once_and_remembers_the_node_with_its_state():
    seen = {}
    check_case(case(0), seen, "seed 0")  # (the case is sound)
    best = max(SEEDS, key=lambda s: len(_final_words(case(s))))
    cs = case(best)
    final = _final_words(cs)
    assert len(final) >= 3
    A, E = gref.history_sync(cs["gram"], cs["dis"], N_MAX, cs["skip"], cs["word_cost"], cs["wos"])
    tree, W = cref.Tree(A, E, cs["gram"], cs["word_cost"], cs["wos"]), cref.window(cs["gram"], cs["tf"], cs["wos"])
    states = cref.kept_states(cs["gram"], cs["wos"])
    for cap in (1, 2, 64):
        cur, got = cref.Cursor(cap), []
        for N in list(range(0, N_MAX + 1, 5)) + [N_MAX] * 8:
            c, words = tree.committed(N, W, states)
            rec, rows, new = cur.take(c, words, cs["tf"], cs["wos"])
            assert rec["n_committed"] == len(words) and rec["first"] == len(got) and rec["n_new"] == len(new) <= cap and rec["frames"] == c[0]
            assert rows["reserved"][:len(new)].tolist() == [w[5] for w in new] and (rows[len(new):].view("<u4") == 0xFFFFFFFF).all()
            got += new
            assert cur.node == ((got[-1][2] + 1, got[-1][5]) if got else cref.ROOT)
        assert got == final
        cur.reset()
        assert (cur.first, cur.node) == (0, cref.ROOT)


def _final_words(cs):
    A, E = gref.history_sync(cs["gram"], cs["dis"], N_MAX, cs["skip"], cs["word_cost"], cs["wos"])
    W, states = cref.window(cs["gram"], cs["tf"], cs["wos"]), cref.kept_states(cs["gram"], cs["wos"])
    return cref.committed(A, E, N_MAX, W, cs["gram"], states, cs["word_cost"], cs["wos"])[1]


def test_a_grammar_that_keeps_nothing_commits_nothing():
    gram = (2, [(1, 1, 0)], [0, 1])  # the final state cannot be reached from state 0
    assert gref.kept(gram, [0, 1]) == ([], [])
    dis = [np.zeros((8, 2), np.int64), np.zeros((8, 3), np.int64)]
    A, E = gref.history_sync(gram, dis, 8, 5, 0)
    assert cref.window(gram, [2, 3], [0, 1]) == 0
    for N in range(9):
        assert cref.entries(A, E, N, 0, []) == ([], True) and cref.committed(A, E, N, 0, gram, []) == (cref.ROOT, [])


def test_commit_plan_runs_clean_under_the_sanitizers(tmp_path):
    """the window from the kept items, the kernel's block and ring, the rows and the refusals of a commit list under the
    grammar sessions' binding (csrc/sr_onepass_gram_commit_plan.h) against a brute-force restatement: a stand-alone program on the CPU
    under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "onepass_gram_commit_plan", "plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
