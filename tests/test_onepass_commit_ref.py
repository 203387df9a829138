"""The commit rule of a live one-pass session (tests/onepass_commit_ref.py) held against what it promises, on the CPU: the
committed words are a prefix of every later parse, the commit node never moves backwards, the window really bounds the starts
alive in the exact column, nothing commits while the window reaches frame 0 -- and the rule is not vacuous.  Also builds and
runs the host-side list of a commit call (csrc/sr_onepass_live_plan.h) under the sanitizers.
"""
import functools
import os
import subprocess

import pytest

import chain_ref
import onepass_commit_ref as cref
import onepass_live_ref as live
import onepass_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
SKIP = chain_ref.PLANT_SKIP
UTT = 80
CONFIGS = [(skip, wc) for skip in (SKIP, None, 300) for wc in (0, 5000)]


@functools.lru_cache(maxsize=None)
def planted_history(c, skip, word_cost):
    fx = chain_ref.planted()
    dis = live.slot_distances(fx["im"][c, :UTT], fx["tm"], fx["tf"])
    A, E, starts = cref.history_with_starts(dis, UTT, skip, word_cost)
    assert (A, E) == ref.history_sync(dis, UTT, skip, word_cost)
    return A, E, starts


@functools.lru_cache(maxsize=None)
def long_history(r, frames):
    fx = ref.planted_long()
    dis = live.slot_distances(fx["im"][r, :frames], fx["tm"], fx["tf"])
    return cref.history_with_starts(dis, frames, SKIP, 0)


def check_recording(A, E, starts, N_max, W, word_cost, what):
    """-> per N the committed words; soundness, monotonicity, the window bound and c(N) = 0 while N <= W on the way"""
    parses = [ref.trace_row(A, E, N, word_cost) for N in range(N_max + 1)]
    out, last_c = [], 0
    for N in range(N_max + 1):
        c, words = cref.committed(A, E, N, W, word_cost)
        assert c >= last_c and c <= N, (what, N, c, last_c)
        assert N > W or (c == 0 and not words), (what, N, c)
        if N:
            assert all(s >= N - W for s in starts[N - 1]), (what, N, sorted(starts[N - 1])[:3])
        for later in range(N, N_max + 1):
            if parses[later]["status"] == ref.CH_OK:
                assert parses[later]["words"][:len(words)] == words, (what, N, later, words, parses[later]["words"])
        last_c = c
        out.append(words)
    return out


@pytest.mark.parametrize("skip,word_cost", CONFIGS)
def test_planted_rows_commit_only_what_every_later_parse_keeps(skip, word_cost):
    fx = chain_ref.planted()
    W = cref.window(fx["tf"])
    assert W == 23
    at = []
    for c in range(chain_ref.PLANT_ROWS):
        A, E, starts = planted_history(c, skip, word_cost)
        per_n = check_recording(A, E, starts, UTT, W, word_cost, f"row {c}, skip {skip}, word_cost {word_cost}")
        at.append(len(per_n[min(int(fx["inf"][c]) + 10, UTT)]))
    if skip == SKIP and not word_cost:  # the rule is not vacuous
        assert sum(n > 0 for n in at) >= 8, at
    if skip == 300 and word_cost == 5000:  # skipping is cheaper than any word: nothing parses as words, nothing commits
        assert at == [0] * chain_ref.PLANT_ROWS


def test_long_rows_commit_most_of_their_words():
    fx = ref.planted_long()
    W = cref.window(fx["tf"])
    for r in range(len(ref.LONG_COUNTS)):
        frames = min(int(fx["inf"][r]), 260 if r == 0 else 300)
        A, E, starts = long_history(r, frames)
        per_n = check_recording(A, E, starts, frames, W, 0, f"long row {r}")
        if r == 0:
            assert ref.trace_row(A, E, 260)["n_words"] == 15 and len(per_n[260]) == 13
            assert all(N - cref.commit_node(A, E, N, W) <= 47 for N in range(261))


def test_the_fallback_is_one_entry_and_the_window_edge_cases():
    """The window holds no reachable position only when skipping is off and no word can end near N.  A template of M frames
    matches every run of M // 2 + 1 .. 2M - 1 frames, at some cost, so with a valid slot every position from the shortest word
    on is reachable and the window of an N > W never is empty: on the planted rows the fallback is never taken.  It is taken
    by a store WITHOUT a valid slot (W = 0, no word at all): position 0 is the last reachable one."""
    fx = chain_ref.planted()
    W = cref.window(fx["tf"])
    for c in range(chain_ref.PLANT_ROWS):
        A, E, _ = planted_history(c, None, 0)
        assert not any(cref.entries(A, E, N, W)[1] for N in range(UTT + 1))
    A, E = ref.history_sync([None] * 5, 30, None, 0)
    assert cref.entries(A, E, 0, 0) == ([0], False)
    for N in range(1, 31):
        assert cref.entries(A, E, N, 0) == ([0], True) and cref.committed(A, E, N, 0) == (0, [])
    A, E = ref.history_sync([None] * 5, 30, SKIP, 0)  # skipping on: every position is reachable, nothing is a word
    assert all(cref.entries(A, E, N, 0) == ([N], False) and cref.committed(A, E, N, 0) == (0, []) for N in range(31))
    assert cref.window([0, 0]) == 0 and cref.window([5, 9], [1, 0]) == 9 and cref.window([5, 9]) == 17
    assert cref.committed([None], [0], 0, 23) == (0, [])


def test_cursor_delivers_every_committed_word_once():
    fx = ref.planted_long()
    W = cref.window(fx["tf"])
    A, E, _ = long_history(0, 260)
    for cap in (1, 2, 64):
        cur, got, calls = cref.Cursor(cap), [], 0
        for N in list(range(0, 261, 37)) + [260] * 16:
            c, words = cref.committed(A, E, N, W)
            rec, rows, new = cur.take(c, words, fx["tf"])
            assert rec["n_committed"] == len(words) and rec["first"] == len(got) and rec["n_new"] == len(new) <= cap and rec["frames"] == c
            assert rows["slot"][:len(new)].tolist() == [w[0] for w in new] and (rows[len(new):].view("<u4") == 0xFFFFFFFF).all()
            got += new
            calls += 1
        assert got == cref.committed(A, E, 260, W)[1] and len(got) == 13


def test_commit_list_runs_clean_under_the_sanitizers(tmp_path):
    """the rows of a commit call -- the distinct listed channels, their N, the store binding, the refusals -- and the window
    from the store's lengths (csrc/sr_onepass_live_plan.h) against a brute-force restatement: a stand-alone program on the CPU
    under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "onepass_commit_plan", "plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "plan_check ok" in run.stdout, (run.stdout, run.stderr)
