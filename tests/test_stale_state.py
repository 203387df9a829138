"""Stale LDS and stale scratch of earlier calls (include/sr_engine.h, hook "lds_poison_launches").

A kernel that reads LDS it has not written, or global scratch its own init left behind LAST time, computes the right bytes as
long as the previous tenant was a workgroup of the same kernel, or the previous call one of the same family.  Three things
take that company away:

  * the testing library overwrites every CU's LDS in front of EVERY kernel launch (launch points, csrc/sr_device.h), between
    the launches of one call too, with a pattern that loses every minimum (HIGH) and with one that wins it (LOW);
  * every family's smallest fixture that reaches its LDS paths runs under both patterns and is compared byte for byte with the
    family's CPU reference -- never with an unpoisoned GPU run;
  * the seven callers that share the decoder scratch run in every order on one engine, after a larger call of their own, and
    after a store change, with the hook off: the left-over is the real one, of another layout.

The fixtures, call helpers and references are the families' own (tests/test_<family>.py, tests/<family>_ref.py).
"""
import ctypes as C
import functools
import glob
import itertools
import os
import re

import numpy as np
import pytest
import torch

import align_ref
import chain_ref
import cluster_ref
import forced_ref
import gram_live_ref
import gram_ref
import onepass_gram_ref
import onepass_ref
import oracle_lib as ol
import pcm_cases
import span_ref
import test_align
import test_chain
import test_chain_live
import test_cluster
import test_cluster_ref
import test_forced
import test_frame_features
import test_gram
import test_gram_live
import test_live_session
import test_onepass
import test_onepass_gram
import test_onepass_live
import test_pcm_front_ends
import test_rescore_dp
import test_span
import test_spot
import test_spot_live
import test_stream_recognition
import test_wgram
import test_wgram_live
import wgram_ref
from stm32_speech_recognition_amd import engine
from stm32_speech_recognition_amd.engine import ATAP_DTYPE, Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stm32_speech_recognition_amd", "csrc")
HOOK = "lds_poison_launches"
BAD_ARG = 3
U32, U64, I64, P = C.c_uint32, C.c_uint64, C.c_int64, C.c_void_p
HIGH, LOW = 0, 1
PATTERNS = pytest.mark.parametrize("pattern", [HIGH, LOW], ids=["high", "low"])
SEED = {HIGH: 0x5EED1234, LOW: 0x0BADC0DE}


def pattern_words(pattern, seed, n):
    """word i of a poisoned CU's LDS: the two expressions of k_lds_poison / k_lds_poison_low, restated"""
    mixed = np.uint32(seed) ^ (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    return mixed | np.uint32(0x80000000) if pattern == HIGH else mixed & np.uint32(7)


def launch_points():
    """sr_lds_launch_points -> (poison launches issued through launch points since the hook was last set, the names seen)"""
    T = engine.load_library(testing=True)
    n, names = U64(0), C.create_string_buffer(8192)
    assert T.sr_lds_launch_points(C.byref(n), names, U32(len(names))) == 0, T.sr_last_error()
    return n.value, set(filter(None, names.value.decode().split(",")))


def poisoned(pattern, call, **hooks):
    """call() with a poison launch of `pattern` in front of every kernel launch (and the family's own hooks set) ->
    (what call returned, poison launches, kernel names).  The hooks are process-global: whatever happens they go back to 0."""
    try:
        for k, v in hooks.items():
            engine.dev_hook(k, v)
        engine.dev_hook(HOOK, SEED[pattern] | pattern << 32)
        out = call()
        torch.cuda.synchronize()
        count, names = launch_points()
    finally:
        engine.dev_hook(HOOK, 0)
        for k in hooks:
            engine.dev_hook(k, 0)
    return out, count, names


def same_bytes(got, want, what):
    """tuples of arrays, byte for byte (None: an output the call was not asked for)"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.nbytes == w.nbytes, (what, i, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            a, b = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{what}: output {i} differs from the reference, first at byte {at} of {a.size}: "
                                 f"got {a[at:at + 16].tolist()} want {b[at:at + 16].tolist()}")


# ---- CPU: every launch site has its launch point ---------------------------------------------------------------------------------
POINT = re.compile(r'SR_LAUNCH_POINT\(\s*([^,()]+?)\s*,\s*"(\w+)"\s*\)\s*;\s*$')
EXEMPT = re.compile(r"k_lds_poison(_low)?$")  # the poison kernels' own launches


def _close_paren(text, at):
    depth = 0
    for i in range(at, len(text)):
        depth += (text[i] == "(") - (text[i] == ")")
        if depth == 0:
            return i
    raise AssertionError("unbalanced call")


def _split_args(body):
    out, depth, cur = [], 0, ""
    for c in body:
        depth += (c == "(") - (c == ")")
        if c == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += c
    return out + [cur.strip()]


def launch_sites(text):
    """[(line, kernel, stream, name of the launch point that is the previous statement or None, its stream)] of one source"""
    code = re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)  # comments may speak of launches
    code = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), code, flags=re.S)
    sites = []
    for m in re.finditer(r"hipLaunchKernelGGL\s*\(|(\w+)\s*(?:<[^<>;(){}]*>)?\s*<<<", code):
        if m.group(1):  # kernel<<<grid, block, lds, stream>>>(...)
            kernel = m.group(1)
            cfg = _split_args(code[m.end():code.index(">>>", m.end())])
            stream = cfg[3] if len(cfg) > 3 else "0"
        else:
            args = _split_args(code[m.end():_close_paren(code, m.end() - 1)])
            kernel, stream = re.match(r"\(?\s*(\w+)", args[0]).group(1), args[4]
        before = POINT.search(code[:m.start()].rstrip())
        sites.append((code.count("\n", 0, m.start()) + 1, kernel, stream, before and before.group(2), before and before.group(1)))
    return sites


def test_the_scanner_sees_a_launch_without_its_point():
    good = 'void f(hipStream_t s)\n{\n    SR_LAUNCH_POINT(s, "k_a");\n    hipLaunchKernelGGL((k_a<4, true>), g, b, 0, s, x);\n}\n'
    assert launch_sites(good) == [(4, "k_a", "s", "k_a", "s")]
    assert launch_sites(good.replace('    SR_LAUNCH_POINT(s, "k_a");\n', ""))[0][3] is None
    assert launch_sites(good.replace('"k_a"', '"k_b"'))[0][3] == "k_b"
    assert launch_sites('SR_LAUNCH_POINT(s, "k_a");\nint n = 0;\nhipLaunchKernelGGL(k_a, g, b, 0, s);')[0][3] is None  # not the previous statement
    assert launch_sites('if (w) hipLaunchKernelGGL(k_a, g, b, 0, s);')[0][3] is None
    assert launch_sites('SR_LAUNCH_POINT(st, "k_a");\nk_a<int><<<g, b, 0, st>>>(x);') == [(2, "k_a", "st", "k_a", "st")]
    assert launch_sites("k_a<<<g, b>>>(x);") == [(1, "k_a", "0", None, None)]
    assert launch_sites("// hipLaunchKernelGGL(k_a, g, b, 0, s);\n") == []


def test_every_kernel_launch_has_a_launch_point_in_front_of_it():
    """csrc/*.hip and csrc/*.cpp: every hipLaunchKernelGGL( and every <<< has SR_LAUNCH_POINT(stream, "kernel") as the previous
    statement, with the launch's own stream and the launched kernel's name.  A kernel added later without one fails here."""
    n_sites, n_points, bad = 0, 0, []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        text = open(path).read()
        n_points += len(re.findall(r"\bSR_LAUNCH_POINT\(", text))
        for line, kernel, stream, name, point_stream in launch_sites(text):
            n_sites += 1
            if EXEMPT.match(kernel):
                n_points += 1
                if name is not None:
                    bad.append((os.path.basename(path), line, kernel, "the poison kernel must not poison itself"))
            elif name != kernel or point_stream != stream:
                bad.append((os.path.basename(path), line, kernel, f"previous statement: launch point {name!r} on {point_stream!r}"))
    assert not bad, bad
    assert n_sites >= 116 and n_points == n_sites, (n_sites, n_points)  # no launch point without a launch behind it either
    dev_h = open(os.path.join(CSRC, "sr_device.h")).read()
    tail = dev_h[dev_h.index("void launch_point(hipStream_t s, const char *kernel);"):]
    assert re.match(r"[^#]*#define SR_LAUNCH_POINT\(stream, name\) ::sr::launch_point\(\(stream\), \(name\)\)\s*#else\s*"
                    r"#define SR_LAUNCH_POINT\(stream, name\) \(\(void\)0\)\s*#endif", tail)  # nothing without -DSR_TESTING


def test_the_product_library_has_no_launch_points():
    L, T = engine.load_library(), engine.load_library(testing=True)
    assert L.sr_dev_hook(HOOK.encode(), I64(1)) == BAD_ARG and b"not compiled into the product library" in L.sr_last_error()
    n = U64(7)
    assert L.sr_lds_launch_points(C.byref(n), None, U32(0)) == BAD_ARG and n.value == 7
    assert L.sr_lds_probe(None, U32(16), None, None) == BAD_ARG and b"product library" in L.sr_last_error()
    blob = open(engine.LIB_PATH, "rb").read()
    for name in (HOOK, "k_lds_probe", "k_lds_poison_low", "_ZN2sr12launch_point"):  # not the hook, not the two kernels, not the function
        assert name.encode() not in blob, name
    assert b"k_lds_probe" in open(engine.TESTING_LIB_PATH, "rb").read()
    header = open(os.path.join(ROOT, "include", "sr_engine.h")).read()
    assert '"%s"' % HOOK in header[header.index("Development and test hooks"):]
    engine.dev_hook(HOOK, 0)
    for bad in (-1, 2 << 32, 3 << 32 | 5, 1 << 34):  # patterns 0 and 1 exist
        assert T.sr_dev_hook(HOOK.encode(), I64(bad)) == BAD_ARG, bad
    assert launch_points() == (0, set())


# ---- GPU: the mechanism -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_probe_reads_the_pattern_on_every_cu_and_the_counter_counts():
    eng = Engine(device=0, testing=True)
    n_cu, words = torch.cuda.get_device_properties(0).multi_processor_count, 2048
    sid = torch.cuda.current_stream().cuda_stream

    def probe():
        out = torch.full((n_cu * words,), 0x11111111, dtype=torch.int32, device="cuda:0")
        assert eng.L.sr_lds_probe(eng.h, U32(words), P(out.data_ptr()), P(sid)) == 0, eng.L.sr_last_error()
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32).reshape(n_cu, words)

    try:
        for pattern in (HIGH, LOW):
            engine.dev_hook(HOOK, SEED[pattern] | pattern << 32)
            want = pattern_words(pattern, SEED[pattern], words)
            for launches in (1, 2, 3):
                got = probe()
                wrong = np.nonzero(np.any(got != want, 1))[0]
                assert not len(wrong), (pattern, launches, len(wrong), int(wrong[0]), got[wrong[0], :4].tolist(), want[:4].tolist())
                assert launch_points() == (launches, {"k_lds_probe"})
        assert np.all(pattern_words(LOW, SEED[LOW], 1 << 16) < 8) and len(set(pattern_words(LOW, SEED[LOW], 64).tolist())) == 8
        assert np.all(pattern_words(HIGH, SEED[HIGH], 1 << 16) >= 1 << 31)
        # sr_lds_poison keeps its bytes: the HIGH expression under its own seed
        engine.dev_hook(HOOK, 0)
        assert eng.lds_poison(0xC0FFEE, sid) > 0
        assert np.array_equal(probe(), np.tile(pattern_words(HIGH, 0xC0FFEE, words), (n_cu, 1)))
        assert launch_points() == (0, set())  # hook 0: no poison launch, nothing counted
        assert eng.L.sr_lds_probe(eng.h, U32(4097), P(1), P(sid)) == BAD_ARG and eng.L.sr_lds_probe(eng.h, U32(0), P(1), P(sid)) == BAD_ARG
    finally:
        engine.dev_hook(HOOK, 0)
        eng.close()


# ---- GPU: every family under both patterns ------------------------------------------------------------------------------------------
SKIP, MAXF, K = chain_ref.PLANT_SKIP, chain_ref.PLANT_MAXF, chain_ref.PLANT_K
W = chain_ref.PLANT_MAX_WORDS
LABELS = list(range(K))
# three states, any word on every arc, one arc with a cost: 0 -w-> 1 -w-> 2 -w-> 2, states 1 and 2 final
GRAM3 = (3, [(0, 1, w) for w in LABELS] + [(1, 2, w) for w in LABELS] + [(2, 2, w) for w in LABELS], [0, 1, 1])
WGRAM3 = wgram_ref.with_costs(GRAM3, [700 * int(a == (1, 2, 0)) for a in GRAM3[1]], None)
REPEAT = onepass_gram_ref.grammar_repeat([LABELS], LABELS, 1)
WREPEAT = wgram_ref.drawn_costs(REPEAT)


def frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@PATTERNS
@pytest.mark.gpu
def test_spotter(pattern):
    fx = test_spot.seam_fixture()
    eng = test_spot.seam_engine(testing=True)
    try:
        # one window per row, cut into chunks of 64 columns: boundary columns in LDS, split records in scratch, the finishing pass
        want = test_spot.seam_want(0)
        got, count, names = poisoned(pattern, lambda: test_spot.dev_call(eng, fx["im"], fx["inf"], 0, 0xA5), spot_chunk_cols=64)
        same_bytes(got, (want, want["dis"]), "spotter, one window in chunks of 64 columns")
        assert (names, count) == ({"k_spot", "k_spot_finish"}, 2), (count, names)
        # windows of 50 frames, packed whole into the chunks
        want = test_spot.seam_want(50)
        got, count, names = poisoned(pattern, lambda: test_spot.dev_call(eng, fx["im"], fx["inf"], 50, 0xA5), spot_chunk_cols=64)
        same_bytes(got, (want, want["dis"]), "spotter, windows of 50 frames")
        assert (names, count) == ({"k_spot"}, 1), (count, names)
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_level_decoder(pattern):
    fx, want = chain_ref.planted(), test_chain.planted_want()
    assert fx["inf"].max() > 64  # rows longer than one sweep: the boundary column in LDS is read
    eng = test_chain.planted_engine(testing=True)
    try:
        got, count, names = poisoned(pattern, lambda: test_chain.dev_call(eng, fx["im"], fx["inf"], W, 0, SKIP), chain_rows=5)
        same_bytes(got, want, "level decoder, groups of 5 rows")
        assert names == {"k_chain_init", "k_chain_words", "k_chain_close", "k_chain_trace"}, names
        assert count == 3 * (2 * W + 2), count  # 12 rows in groups of 5: three launch groups of 2 * max_words + 2 launches
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def gram3_want(weighted):
    fx = chain_ref.planted()
    ref, g = (wgram_ref, WGRAM3) if weighted else (gram_ref, GRAM3)
    return frozen(ref.decode(g, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, W, 0, SKIP, 0))


@PATTERNS
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.gpu
def test_grammar_decoder(weighted, pattern):
    fx, want = chain_ref.planted(), gram3_want(weighted)
    if weighted:  # the costed arc is looked at
        assert frozen(gram3_want(False))[0].tobytes() != want[0].tobytes()
    eng = test_gram.planted_engine(testing=True)
    gram = eng.grammar(*(WGRAM3 if weighted else GRAM3))
    try:
        got, count, names = poisoned(pattern, lambda: test_gram.gram_call(eng, gram, fx["im"], fx["inf"], W, 0, SKIP), chain_rows=5)
        same_bytes(got, want, "grammar decoder, groups of 5 rows")
        tail = "_w" if weighted else ""
        assert names == {"k_gram_init", "k_gram_charge" + tail, "k_gram_words", "k_gram_close", "k_gram_trace" + tail}, names
        assert count == 3 * (2 + 3 * W), count  # per group: init, per level charge + sweep + close, trace
    finally:
        gram.close()
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_forced_alignment(pattern):
    fx, want = test_forced.corpus_fixture(), test_forced.corpus_want(900)
    eng = test_forced.corpus_engine(testing=True)
    try:
        call = lambda: test_forced.forced_call(eng, fx["im"], fx["inf"], fx["transcripts"], 16, 900, test_forced.WORD_COST, stride=3)  # noqa: E731
        got, count, names = poisoned(pattern, call, chain_chunk_cols=16, chain_rows=7)  # pruning on: the default
        same_bytes(got, want, "forced alignment, chunks of 16 columns, groups of 7 rows")
        assert names == {"k_chain_init", "k_forced_words", "k_chain_close", "k_forced_trace"}, names
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_span_gather(pattern):
    pl = chain_ref.planted()
    rec, words = test_forced.planted_want(SKIP)
    dst, word_start = forced_ref.example_layout(LABELS, pl["seq"], W)
    n_ex = int(word_start[-1])
    want = forced_ref.gather(pl["im"], pl["inf"], MAXF, words, dst, n_ex, 16)
    eng = test_forced.planted_engine(testing=True)
    try:
        (rc, g_ex, g_ef), count, names = poisoned(pattern, lambda: test_forced.gather_call(eng, pl["im"], pl["inf"], words, dst, n_ex, 16, 0xA5))
        assert rc == 0, eng.L.sr_last_error()
        g_ex.check_equals(want[0])
        g_ef.check_equals(want[1])
        assert names == {"k_gather_spans"} and count == 1, (count, names)
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_onepass_decoder(pattern):
    fx, want = chain_ref.planted(), test_onepass.planted_want(SKIP, 0)
    eng = test_onepass.planted_engine(testing=True)
    try:
        got, count, names = poisoned(pattern, lambda: test_onepass.dev_call(eng, fx["im"], fx["inf"], 16, SKIP, 0), onepass_block=3, onepass_rows=5)
        same_bytes(got, want, "one-pass decoder, blocks of 3 frames, groups of 5 rows")
        assert names == {"k_onepass_init", "k_onepass_words", "k_onepass_close", "k_onepass_trace"}, names
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def repeat_want(weighted):
    fx = chain_ref.planted()
    return frozen(onepass_gram_ref.decode(WREPEAT if weighted else REPEAT, fx["im"], fx["inf"], fx["tm"], fx["tf"], None, MAXF, 16, SKIP, 0))


@PATTERNS
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.gpu
def test_onepass_grammar_decoder(weighted, pattern):
    fx, want = chain_ref.planted(), repeat_want(weighted)
    eng = test_onepass_gram.planted_engine(testing=True)
    gram = eng.grammar(*(WREPEAT if weighted else REPEAT))
    try:
        call = lambda: test_onepass_gram.dev_call(eng, gram, fx["im"], fx["inf"], 16, SKIP, 0)  # noqa: E731
        got, count, names = poisoned(pattern, call, onepass_block=3, onepass_rows=5)
        same_bytes(got, want, "one-pass grammar decoder, blocks of 3 frames, groups of 5 rows")
        tail = "_w" if weighted else ""
        assert names == {"k_onepass_gram_init", "k_onepass_gram_words" + tail, "k_onepass_gram_close", "k_onepass_gram_trace" + tail}, names
    finally:
        gram.close()
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_span_scores_and_decoder_with_alternatives(pattern):
    fx = span_ref.planted()
    rec, words, lc, sc, alts, nm = test_span.planted_want(span_ref.SPAN_ACC)
    eng = Engine(max_frames=span_ref.PLANT_MAXF, device=0, testing=True)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    eng.set_word_map(None, 2)
    try:
        call = lambda: test_span.alts_call(eng, fx["im"], fx["inf"], span_ref.PLANT_MAX_WORDS, test_span.N_BEST, span_ref.SPAN_ACC, span_ref.PLANT_SKIP)  # noqa: E731
        got, count, names = poisoned(pattern, call)
        same_bytes(got, (rec, words, lc, alts, nm, sc), "decoder with alternatives")
        assert names == {"k_chain_init", "k_chain_words", "k_chain_close", "k_chain_trace", "k_span_words", "k_nbest"}, names
        got, count, names = poisoned(pattern, lambda: test_span.span_call(eng, fx["im"], fx["inf"], words, span_ref.SPAN_ACC), span_groups=3)
        same_bytes((got,), (sc,), "span scores, three groups per launch")
        assert names == {"k_span_words"} and count >= 2, (count, names)
    finally:
        eng.close()


@PATTERNS
@pytest.mark.parametrize("marks_global", [0, 1], ids=["marks_lds", "marks_global"])
@pytest.mark.gpu
def test_aligner(marks_global, pattern):
    fx = test_align.edge_fixture(3000)
    eng = Engine(max_frames=test_align.EDGE_MAXF, device=0, testing=True)
    try:
        got, count, names = poisoned(pattern, lambda: test_align.dev_align(eng, fx), align_pairs=40, align_marks_global=marks_global)
        same_bytes(got, (fx["rec"], fx["span"]), f"aligner, marks_global {marks_global}, 40 pairs per launch")
        assert names == {"k_dp_align"} and count == -(-len(test_align.EDGE_PAIRS) // 40), (count, names)
    finally:
        eng.close()


# ---- GPU: the live sessions: three pushes of uneven size, every push against the reference of the frames so far ------------------
def three_pushes(lengths, first, second):
    """per channel `first` frames, then `second`, then the rest -> per push the counts"""
    return [[min(first, N) for N in lengths], [min(second, N - min(first, N)) for N in lengths],
            [N - min(first, N) - min(second, N - min(first, N)) for N in lengths]]


@PATTERNS
@pytest.mark.gpu
def test_spot_session(pattern):
    tsl = test_spot_live
    eng, win = tsl.make_engine(testing=True), 50
    try:
        sched = tsl.uniform([65, 119, 116])  # 300 frames: a 65-row template and window edges inside every push; 119 is the most a push takes
        col, count, names = poisoned(pattern, lambda: tsl.feed(eng, tsl.feats(2), sched, win, "dev", 119))
        for c in range(tsl.C_N):
            same_bytes((col.channel(c),), (tsl.want(2, win)[c],), f"spot session, channel {c}")
        assert names >= {"k_spot_live", "k_spot_live_flush"}, names
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_level_decoder_session(pattern):
    tcl = test_chain_live
    _, n = tcl.feats()
    sched = three_pushes([int(N) for N in n], 66, 9)  # a push longer than one sweep of 64 columns
    eng = tcl.make_engine(testing=True)
    try:
        fol, count, names = poisoned(pattern, lambda: tcl.feed(eng, sched, SKIP, 0, 0, "dev", "level decoder session"))  # (checks every push)
        assert names == {"k_chain_live_init", "k_chain_live_words", "k_chain_live_close", "k_chain_live_trace"}, names
        assert count == 3 * (2 * tcl.MAX_WORDS + 2), count
    finally:
        eng.close()


@PATTERNS
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.gpu
def test_grammar_session(weighted, pattern):
    fx = chain_ref.planted()
    n = [int(N) for N in fx["inf"]]
    sched = three_pushes(n, 9, 4)
    if weighted:
        t, g = test_wgram_live, WGRAM3
        recs = [wgram_ref.Recording(g, fx["im"][r, :n[r]], fx["tm"], fx["tf"], None, t.W, SKIP, 0, None) for r in range(t.N_CH)]
    else:
        t, g = test_gram_live, GRAM3
        n = n[:t.N_CH]
        sched = three_pushes(n, 9, 4)
        recs = [gram_live_ref.Recording(g, fx["im"][r, :n[r]], fx["tm"], fx["tf"], None, t.W, 0, SKIP, 0, None) for r in range(t.N_CH)]
    eng = Engine(max_frames=MAXF, device=0, testing=True)
    eng.set_templates_dense(fx["tm"], fx["tf"])
    gram = eng.grammar(*g)
    ses = eng.decode_grammar_live(gram, t.N_CH, max(max(s) for s in sched), MAXF, t.W, 0, SKIP, 0)
    fol = t.Follower(ses, recs, 0, "grammar session")
    d_f = torch.from_numpy(np.array(fx["im"][:t.N_CH])).cuda()

    def feed():
        at = [0] * t.N_CH
        for cnt in sched:
            fol.take(ses.push_dev(t.dev_chunk(d_f, at, cnt), np.array(cnt, np.uint32)), cnt)  # every emitted row against the reference
            at = [a + b for a, b in zip(at, cnt)]
        assert at == n

    try:
        _, count, names = poisoned(pattern, feed)
        tail = "_w" if weighted else ""
        assert names == {"k_gram_live_init", "k_gram_live_words" + tail, "k_gram_live_close", "k_gram_live_trace" + tail}, names
        assert count == 3 * (2 + 2 * t.W), count  # per push: init, a sweep and a close per level, the trace
    finally:
        ses.close()
        gram.close()
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_onepass_session(pattern):
    tol = test_onepass_live
    f, n = tol.planted_feats()
    sched = three_pushes(n, 8, 5)
    chunk_max, block = max(max(s) for s in sched), 3
    eng = tol.planted_engine(testing=True)
    ses = eng.decode_onepass_live(tol.N_CH, chunk_max, tol.UTT, tol.W, False, SKIP, 0)
    fol = tol.Follower(ses, [tol.recording(c, SKIP, 0) for c in range(tol.N_CH)], "one-pass session")
    try:
        _, count, names = poisoned(pattern, lambda: tol.feed(ses, fol, f, sched, "dev"), onepass_block=block)  # (checks every push)
        assert fol.count == n
        assert names == {"k_onepass_live_words", "k_onepass_live_close", "k_onepass_live_trace"}, names
        assert count == sum(2 * -(-max(cnt) // block) + 1 for cnt in sched), count  # a sweep and a close per block, and the trace
        engine.dev_hook("onepass_block", block)
        fx = chain_ref.planted()
        geo = engine.onepass_live_geometry(int(fx["tf"].max()), K, int(fx["tf"].min()), tol.UTT, chunk_max, testing=True)
        assert geo["launches"] == 2 * -(-chunk_max // block) + 1 == max(2 * -(-max(cnt) // block) + 1 for cnt in sched)
    finally:
        engine.dev_hook("onepass_block", 0)
        ses.close()
        eng.close()


@PATTERNS
@pytest.mark.parametrize("kind", test_pcm_front_ends.KINDS)
@pytest.mark.gpu
def test_pcm_sessions(kind, pattern):
    """the PCM form of every session on the reference front end: samples in, the live front end's kernels and the session's
    under poison; expected values from the CPU oracle's features (tests/pcm_cases.py)"""
    tpf, pc = test_pcm_front_ends, pcm_cases
    fx = pc.case("reference")
    fl, hop, R1 = fx["frame_len"], fx["hop"], fx["R1"]
    eng = Engine(max_frames=pc.MAXF, device=0, testing=True, **fx["ekw"])
    eng.set_templates_dense(*pc.store(fx))
    eng.set_word_map(fx["wos"])
    gram = tpf.grammar_of(kind, eng, fx)
    try:
        ses = tpf.open_session(kind, eng, fx, 3, fx["chunk_max"], tpf.OP_UTT if kind == "onepass" else pc.MAXF, fx["mid"], gram)
        sched, X = pc.schedules("reference")["dev"], fx["X"][:, :R1]
        if kind == "spot":
            run = lambda: tpf.run_spotter(ses, X, R1, sched, fl, hop, pc.want_windows("reference"), "spot session, PCM form", True)  # noqa: E731
        else:
            W = pc.OP_WORDS if kind == "onepass" else pc.MAX_WORDS
            want = [a[:3] for a in tpf.want_of(kind, "reference")]
            run = lambda: tpf.run_decoder(ses, X, R1, sched, fl, hop, W, want, f"{kind} session, PCM form", True)  # noqa: E731
        _, count, names = poisoned(pattern, run)
        session = dict(spot="k_spot_live", level="k_chain_live_words", gram="k_gram_live_words", wgram="k_gram_live_words_w",
                       onepass="k_onepass_live_words")[kind]
        assert session in names and any(k.startswith("k_mfcc") for k in names) and count > len(sched), (count, names)
    finally:
        if gram is not None:
            gram.close()
        eng.close()


# ---- GPU: trainers, clustering, the full-DP scorer -------------------------------------------------------------------------------------
@PATTERNS
@pytest.mark.gpu
def test_trainer_two_iterations(pattern):
    fx = test_align.train_fixture(3000)
    want_cen, want_st = align_ref.train(fx["mfcc"], fx["frames"], fx["ex_start"], fx["cen"], fx["cen_frames"], 2)
    eng = Engine(max_frames=test_align.TRAIN_MAXF, device=0, testing=True)
    try:
        (cen, st), count, names = poisoned(pattern, lambda: test_align.dev_train(eng, fx, 2, 0xA5), align_pairs=4)
        same_bytes((cen, st), (want_cen, want_st), "trainer, 2 iterations, 4 pairs per launch")
        assert names >= {"k_dp_align", "k_align_accum", "k_align_finalise"}, names
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_clustering(pattern):
    fx = test_cluster_ref.planted_case("quantile")
    n_iter = test_cluster_ref.N_ITER
    eng = Engine(max_frames=cluster_ref.PLANT_MAXF, device=0, testing=True)
    try:
        got, count, names = poisoned(pattern, lambda: test_cluster.dev_models(eng, fx, n_iter), cluster_pairs=7)
        test_cluster.same_models(got, fx["want"], n_iter, "clustering, 7 pairs per launch")
        same_bytes((got["cen"],), (fx["want"]["cen"],), "clustering: centroids")
        assert names >= {"k_cluster_score", "k_cluster_assign"}, names
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_full_dp_scorer_dense_and_sparse(pattern):
    trd = test_rescore_dp
    fx = trd.base_fixture()
    eng = trd.base_engine(testing=True)
    try:
        first, _ = eng.nbest(eng.dtw(fx["im"], fx["inf"])[0], 3)  # the lists to rescore are an input: what they hold is not checked here
        want = trd.rescored(fx["dp"], trd.WORDS0, first)           # ... what comes out of them is, against the oracle's matrix
        dense, count, names = poisoned(pattern, lambda: eng.dtw_dp(fx["im"], fx["inf"]))
        same_bytes((dense,), (fx["dp"],), "full-DP scorer, dense form")
        assert any(k.startswith("k_dtw_dp") for k in names), names
        got, count, names = poisoned(pattern, lambda: trd.dev_call(eng, fx["im"], fx["inf"], first))
        trd.check(got, want, "rescoring, sparse form")
        assert any(k.startswith("k_dtw_dp") and k.endswith("sparse") for k in names) and "k_rescore_mark" in names, names
    finally:
        eng.close()


# ---- GPU: stream recognition, sr_live, the recognition path, the transform ----------------------------------------------------------------
STREAM_CASES = (12, 16, 18)  # a crossing carried over three tiles; an ending in the tail state; a 200-frame segment, then a good one


@PATTERNS
@pytest.mark.gpu
def test_stream_segments(pattern):
    tsr = test_stream_recognition
    recs, ats = tsr.constructed_cases(16)
    recs, ats = [recs[i] for i in STREAM_CASES], [ats[i] for i in STREAM_CASES]
    pcm, lens = tsr.pack(recs)
    orc = ol.Oracle(max_seg=1 << 16)
    eng = Engine(testing=True)
    try:
        call = lambda: eng.recognize_stream(pcm, lens, atap=np.array(ats, ATAP_DTYPE), want_scores=False, want_mfcc=False, recognize=False)  # noqa: E731
        out, count, names = poisoned(pattern, call, stream_tile_frames=16)
        tsr.check_against_oracle(orc, out, pcm, lens, [ol.Atap(*a) for a in ats])
        assert out["total"] >= 4 and names >= {"k_stream_tiles", "k_stream_scan", "k_stream_emit"}, (out["total"], names)
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_live_vad_session(pattern):
    tsr, tls = test_stream_recognition, test_live_session
    recs, ats = tsr.constructed_cases(16)
    recs, ats = [recs[i] for i in STREAM_CASES], [ats[i] for i in STREAM_CASES]
    orc = ol.Oracle(max_seg=1 << 16)
    eng = Engine(testing=True)
    sess = eng.live(len(recs), 8000, atap=np.array(ats, ATAP_DTYPE))
    try:
        f = tls.Feeder(sess, recognize=False)
        for c, x in enumerate(recs):
            f.load(c, x)
        sizes = (4000, 1003, 8000)

        def run():
            f.drive(lambda k: np.full(len(recs), sizes[k % 3]))
            return {int(g["channel"]): g for g in sess.end(np.arange(len(recs)))}

        ended, count, names = poisoned(pattern, run)
        assert f.pushes >= 3
        for c, x in enumerate(recs):
            want, _ = tsr.oracle_segments(orc, x, ol.Atap(*ats[c]))
            mine = [(int(g["start"]), int(g["end"])) for g in f.out[c]["segs"]] + ([(int(ended[c]["start"]), -1)] if c in ended else [])
            assert mine == [tuple(int(v) for v in r) for r in want], (c, mine, want.tolist())
        assert names >= {"k_live_append", "k_live_scan", "k_live_compact"}, names
    finally:
        sess.close()
        eng.close()


@PATTERNS
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.gpu
def test_recognition_path_on_golden_captures(mode, pattern):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_golden.npz"))
    eng = Engine(max_frames=119, device=0, testing=True)
    try:
        eng.set_templates_store(g["store"])
        eng.set_small_launch(mode)
        out, count, names = poisoned(pattern, lambda: eng.recognize(g["pcm"][:8]))
        n = g["frm_num"][:8]
        for b in range(8):
            assert np.array_equal(out["mfcc"][b, :n[b]], g["mfcc"][b, :n[b]]), (mode, b)
        assert np.array_equal(out["vad"]["seg"], g["seg"][:8]) and np.array_equal(out["vad"]["frm_num"], n)
        assert np.array_equal(out["scores"], g["recg_scores"][:8]) and np.array_equal(out["results"]["best_tpl"], g["recg_best"][:8])
        assert np.array_equal(out["results"]["min_dis"], g["recg_dis"][:8]) and np.array_equal(out["results"]["status"], g["recg_status"][:8])
        assert count >= 3 and any(k.startswith("k_vad") for k in names) and any(k.startswith("k_mfcc") for k in names), names
        assert any(k.startswith("k_dtw") for k in names), names
    finally:
        eng.close()


@PATTERNS
@pytest.mark.parametrize("front", ["reference", "extension"])
@pytest.mark.gpu
def test_frame_features_every_kind(front, pattern):
    """two captures per kind of sr_frame_features_batch, every value from the CPU oracle's transform, tables and log"""
    tff = test_frame_features
    ekw, rate = ({}, 1) if front == "reference" else (test_stream_recognition.EXT, 2)
    eng, orc = Engine(max_frames=80, device=0, testing=True, **ekw), ol.Oracle(max_frames=80, **ekw)
    try:
        P, st, en, mid = tff.vad_segments(orc, tff.synth_batch((1.0, 4.0), n=1, T=48, rate=rate))
        assert len(P) == 2
        tab, got = orc.tables(), {}
        for kind in tff.KINDS:
            got[kind], count, names = poisoned(pattern, lambda: tff.features(eng, P, st, en, mid, kind, want_mfcc=True))
            assert count >= 1 and all(k.startswith("k_mfcc") for k in names), (kind, names)
        n = got[tff.FEAT_MAG][1]
        assert (got[tff.FEAT_MAG][2] == 0).all() and n.min() > 0
        for b, fr in enumerate(tff.windows_of(orc, P, st, n, mid)):
            mag = np.stack([orc.fft_mag(f) for f in fr])
            mel, _ = tff.mel_from_mag(mag, tab)
            assert np.array_equal(got[tff.FEAT_MAG][0][b, :n[b]], mag), b
            assert np.array_equal(tff.mag_from_words(got[tff.FEAT_FFT][0][b, :n[b]]), mag), b
            assert np.array_equal(got[tff.FEAT_MEL][0][b, :n[b]], mel), b
            lg = got[tff.FEAT_LOGMEL][0][b, :n[b]]
            assert np.array_equal(lg.reshape(-1), tff.log100(orc, mel)), b
            for kind in tff.KINDS:  # the MFCC rows that come with every kind: the DCT of the log-Mel values
                assert np.array_equal(got[kind][3][b, :n[b]], tff.dct_rows(lg, tab["dct"], eng.n_coef)), (kind, b)
                tff.check_rows_zero(got[kind][0], n)
    finally:
        eng.close()


@PATTERNS
@pytest.mark.gpu
def test_fft_q15_rows(pattern):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_golden.npz"))
    eng = Engine(max_frames=119, device=0, testing=True)
    try:
        got, count, names = poisoned(pattern, lambda: eng.fft_q15(g["fft_in"][:4]))
        same_bytes((got,), (g["fft_out"][:4],), "sr_fft_q15_batch, 4 rows")
        assert (names, count) == ({"k_fft_q15"}, 1), (count, names)
    finally:
        eng.close()


# ---- GPU: stale global scratch: the seven callers of the decoder scratch, in every order on one engine -----------------------------
N_BEST = 3


def _rows(fx, rows):
    rows = list(range(len(fx["inf"]))) if rows is None else list(rows)
    return np.ascontiguousarray(fx["im"][rows]), np.ascontiguousarray(fx["inf"][rows]), [fx["seq"][r] for r in rows]


class Family:
    """one caller of s_ch_a / s_ch_e / s_op_cols: how to call it and what the reference says, over (store, rows, max_words)"""

    def __init__(self, name, want, call, gram=None):
        self.name, self._want, self._call, self.gram_t = name, want, call, gram

    def want(self, store, rows, mw):
        return _want_cached(self.name, store, rows, mw)

    def call(self, eng, grams, rows, mw):
        im, inf, seq = _rows(chain_ref.planted(), rows)
        return self._call(eng, grams.get(self.name), im, inf, seq, mw)


def stores(which):
    """"planted": chain_ref.planted()'s store; "short": the same templates cut to half their frames (4..7)"""
    fx = chain_ref.planted()
    if which == "planted":
        return fx["tm"], fx["tf"]
    tf = (fx["tf"] // 2).astype(np.uint32)
    tm = fx["tm"][:, :8].copy()
    for k in range(K):
        tm[k, tf[k]:] = 0
    return tm, tf


def _alts_want(im, inf, tm, tf, mw):
    dec = chain_ref.decode(im, inf, tm, tf, None, MAXF, mw, 0, SKIP, 0)
    sc = span_ref.span_scores(im, inf, tm, tf, None, dec[1], span_ref.SPAN_ACC)
    alts, nm = span_ref.nbest(sc, np.arange(K), N_BEST)
    return dec + (alts, nm, sc)


FAMILIES = {f.name: f for f in (
    Family("level", lambda im, inf, seq, tm, tf, mw: chain_ref.decode(im, inf, tm, tf, None, MAXF, mw, 0, SKIP, 0),
           lambda eng, g, im, inf, seq, mw: test_chain.dev_call(eng, im, inf, mw, 0, SKIP)),
    Family("grammar", lambda im, inf, seq, tm, tf, mw: gram_ref.decode(GRAM3, im, inf, tm, tf, None, MAXF, mw, 0, SKIP, 0),
           lambda eng, g, im, inf, seq, mw: test_gram.gram_call(eng, g, im, inf, mw, 0, SKIP), GRAM3),
    Family("weighted", lambda im, inf, seq, tm, tf, mw: wgram_ref.decode(WGRAM3, im, inf, tm, tf, None, MAXF, mw, 0, SKIP, 0),
           lambda eng, g, im, inf, seq, mw: test_wgram.gram_call(eng, g, im, inf, mw, 0, SKIP), WGRAM3),
    Family("forced", lambda im, inf, seq, tm, tf, mw: forced_ref.align(im, inf, tm, tf, None, MAXF, seq, mw, SKIP, 0),
           lambda eng, g, im, inf, seq, mw: test_forced.forced_call(eng, im, inf, seq, mw, SKIP, 0)),
    Family("onepass", lambda im, inf, seq, tm, tf, mw: onepass_ref.decode(im, inf, tm, tf, None, MAXF, mw, SKIP, 0),
           lambda eng, g, im, inf, seq, mw: test_onepass.dev_call(eng, im, inf, mw, SKIP, 0)),
    Family("onepass_grammar", lambda im, inf, seq, tm, tf, mw: onepass_gram_ref.decode(REPEAT, im, inf, tm, tf, None, MAXF, mw, SKIP, 0),
           lambda eng, g, im, inf, seq, mw: test_onepass_gram.dev_call(eng, g, im, inf, mw, SKIP, 0), REPEAT),
    Family("alts", lambda im, inf, seq, tm, tf, mw: _alts_want(im, inf, tm, tf, mw),
           lambda eng, g, im, inf, seq, mw: test_span.alts_call(eng, im, inf, mw, N_BEST, span_ref.SPAN_ACC, SKIP)),
)}
SMALL_ROWS = (9, 4)  # two planted words and one: within max_words 2, and not the rows a larger call's scratch begins with


@functools.lru_cache(maxsize=None)
def _want_cached(name, store, rows, mw):
    im, inf, seq = _rows(chain_ref.planted(), rows)
    tm, tf = stores(store)
    return frozen(tuple(FAMILIES[name]._want(im, inf, seq, tm, tf, mw)))


class Shared:
    """one engine over the planted store for the whole module, with the grammars compiled against it"""

    def __init__(self):
        self.eng = test_chain.planted_engine()  # the product library: no hook is wanted here
        self.compile()

    def compile(self):
        self.grams = {f.name: self.eng.grammar(*f.gram_t) for f in FAMILIES.values() if f.gram_t is not None}

    def close(self):
        for g in self.grams.values():
            g.close()
        self.eng.close()


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", list(itertools.permutations(FAMILIES, 2)), ids=lambda n: n)
def test_a_caller_after_another_caller_of_the_same_scratch(shared, a, b):
    assert engine.load_library(testing=True).sr_dev_hook(HOOK.encode(), I64(0)) == 0  # the real left-over, not a pattern
    FAMILIES[a].call(shared.eng, shared.grams, None, W)
    got = FAMILIES[b].call(shared.eng, shared.grams, None, W)
    same_bytes(got, FAMILIES[b].want("planted", None, W), f"{b} after {a}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_smaller_call_after_a_larger_one_of_the_same_caller(shared, name):
    f = FAMILIES[name]
    f.call(shared.eng, shared.grams, None, 16)                    # all 12 rows, 16 words
    got = f.call(shared.eng, shared.grams, SMALL_ROWS, 2)         # two other rows, 2 words: the scratch holds the larger layout
    same_bytes(got, f.want("planted", SMALL_ROWS, 2), f"{name}: 2 rows of 2 words after 12 rows of 16")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_call_after_the_store_was_replaced_by_shorter_templates(name):
    f = FAMILIES[name]
    s = Shared()
    try:
        f.call(s.eng, s.grams, None, W)
        for g in s.grams.values():
            g.close()
        s.eng.set_templates_dense(*stores("short"))
        s.compile()
        got = f.call(s.eng, s.grams, None, W)
        same_bytes(got, f.want("short", None, W), f"{name} after set_templates to shorter templates")
    finally:
        s.close()
