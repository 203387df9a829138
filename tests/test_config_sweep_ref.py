"""The configuration set of tests/config_cases.py looks at what it claims: coverage counted on the references alone, the
spotter's dependence on its tie rule, and the agreements the header states between the decoder families, on every
configuration.  No GPU.  The reference outputs are computed once each (lru_cache) and shared with tests/test_config_sweep.py,
which imports them from here.

The shares asserted below are conditions on the draws of config_cases, not measurements of the library: where a count falls
short the draws are tuned, never the bound.
"""
import functools

import numpy as np

import chain_ref
import config_cases as cc
import forced_ref
import gram_ref
import onepass_gram_ref
import onepass_ref
import span_ref
import spot_ref
import test_spot as t_spot
import wgram_ref

IDS = tuple(range(cc.N_CONFIGS))
CH_OK, CH_NONE, CH_TRUNCATED = chain_ref.CH_OK, chain_ref.CH_NONE, onepass_ref.CH_TRUNCATED
N_BEST = 3


def frozen(out):
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def as_bytes(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out if a is not None)


def anchor(cfg):
    return gram_ref.grammar_any(cfg["labels"])


# ---- the references, each computed once ------------------------------------------------------------------------------------------
def chain_want(i, n_exact=None):
    """n_exact None: the configuration's own (one cache entry per reference, whatever the call spells out)"""
    return _chain(i, cc.config(i)["n_exact"] if n_exact is None else n_exact)


@functools.lru_cache(maxsize=None)
def _chain(i, n_exact):
    c = cc.config(i)
    return frozen(chain_ref.decode(c["im"], c["inf"], *cc.store(c), c["maxf"], c["max_words"], n_exact, c["skip"], c["word_cost"], c["wos"]))


@functools.lru_cache(maxsize=None)
def gram_want(i, which="own"):
    """which: "own" = the drawn grammar without its costs, "anchor" = every sequence of words"""
    c = cc.config(i)
    g = anchor(c) if which == "anchor" else c["gram"]
    return frozen(gram_ref.decode(g, c["im"], c["inf"], *cc.store(c), c["maxf"], c["max_words"], c["n_exact"], c["skip"], c["word_cost"], c["wos"]))


@functools.lru_cache(maxsize=None)
def wgram_want(i, which="own"):
    """which: "own" = the drawn grammar with its costs, "zero" = with all-zero costs"""
    c = cc.config(i)
    g = c["wgram"] if which == "own" else wgram_ref.with_costs(c["gram"], [0] * len(c["gram"][1]), [0] * c["gram"][0])
    return frozen(wgram_ref.decode(g, c["im"], c["inf"], *cc.store(c), c["maxf"], c["max_words"], c["n_exact"], c["skip"], c["word_cost"], c["wos"]))


def op_block(c):
    """the block the drawn "onepass_block" hook gives: clamped to 1..L, unset = L"""
    return min(max(c["hooks"]["onepass_block"], 1), c["L"]) if c["hooks"]["onepass_block"] else c["L"]


@functools.lru_cache(maxsize=None)
def onepass_want(i, block=0, frames_cap=None):
    """None where the call is refused; frames_cap None: the configuration's own"""
    c = cc.config(i)
    cap = c["frames_cap"] if frames_cap is None else frames_cap
    if not onepass_ref.cost_ok(min(c["maxf"], cap) if cap else c["maxf"], c["L"], c["word_cost"]):
        return None
    return frozen(onepass_ref.decode(c["im"], c["inf"], *cc.store(c), c["maxf"], c["words_cap"], c["skip"], c["word_cost"], c["wos"], cap, block))


@functools.lru_cache(maxsize=None)
def opgram_want(i, which="own", block=0, frames_cap=None):
    """which: "own" = the drawn grammar with its costs, "anchor"; None where the call is refused"""
    c = cc.config(i)
    g = anchor(c) if which == "anchor" else c["wgram"]
    cap = c["frames_cap"] if frames_cap is None else frames_cap
    if not onepass_gram_ref.cost_ok(min(c["maxf"], cap) if cap else c["maxf"], c["L"], c["word_cost"], g):
        return None
    return frozen(onepass_gram_ref.decode(g, c["im"], c["inf"], *cc.store(c), c["maxf"], c["words_cap"], c["skip"], c["word_cost"], c["wos"], cap, block))


@functools.lru_cache(maxsize=None)
def forced_want(i):
    c = cc.config(i)
    return frozen(forced_ref.align(c["im"], c["inf"], *cc.store(c), c["maxf"], c["transcripts"], c["words_per_row"], c["skip"], c["word_cost"], c["wos"]))


@functools.lru_cache(maxsize=None)
def spot_want(i, win=None):
    c = cc.config(i)
    out = spot_ref.spot_hits(c["im"], c["inf"], *cc.store(c), c["maxf"], c["win"] if win is None else win)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def span_want(i):
    """(span scores of the level decoder's word rows with the count left free, alternatives, candidate counts) in mode
    SR_SPAN_ACC"""
    c, dec = cc.config(i), chain_want(i, 0)
    scores = span_ref.span_scores(c["im"], c["inf"], *cc.store(c), dec[1], span_ref.SPAN_ACC)
    return frozen((scores,) + span_ref.nbest(scores, c["wos"], N_BEST))


def unique_minimum(i, r):
    """row r: the one-pass parse can be compared with the level decoder's word rows, i.e. exactly one word count of
    1..max_words reaches the smallest level cost, the zero-word parse (N x skip_cost) does not, and at most 16 words"""
    c = cc.config(i)
    lc = [int(v) for v in chain_want(i, 0)[2][r] if v != spot_ref.DIS_ERR]
    if not lc or lc.count(min(lc)) != 1:
        return False
    return c["skip"] is None or int(c["n_frames"][r]) * c["skip"] > min(lc)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_the_configurations_are_frozen_cached_and_named_by_their_seed():
    for i in IDS:
        c = cc.config(i)
        assert c is cc.config(i) and c["seed"] == cc.BASE + i and not c["im"].flags.writeable and not c["tm"].flags.writeable
        assert c["valid"].any() and set(c["wos"].tolist()) == set(c["labels"]) and len(c["inf"]) in cc.ROWS_DRAW
        assert 1 <= c["L"] == onepass_ref.reach(c["tf"], c["valid"]) and c["maxf"] in cc.MAXF_DRAW
        assert set(c["hooks"]) == set(cc.HOOK_DRAWS) and all(c["hooks"][k] in v for k, v in cc.HOOK_DRAWS.items())
        assert all(0 <= size <= 70 for _, sizes in c["live"] for size in sizes)
    assert 24 <= cc.N_CONFIGS <= 32 and sum(cc.config(i)["K"] == cc.K_BIG for i in IDS) == 2
    assert sum(cc.config(i)["max_words"] == 16 for i in IDS) == 1


def test_coverage_of_the_configuration_set():
    cfgs = [cc.config(i) for i in IDS]
    rows = sum(len(c["inf"]) for c in cfgs)
    rec = np.concatenate([chain_want(i)[0] for i in IDS])
    n_frames = np.concatenate([c["n_frames"] for c in cfgs])
    inf = np.concatenate([c["inf"] for c in cfgs])
    maxf = np.concatenate([np.full(len(c["inf"]), c["maxf"]) for c in cfgs])
    ok = int((rec["status"] == CH_OK).sum())
    multi = int((rec["n_words"] >= 2).sum())
    none_with_frames = int(((rec["status"] == CH_NONE) & (n_frames > 0)).sum())
    l_one = sum(c["L"] == 1 for c in cfgs)
    wide = sum(2 * c["L"] - 1 > 64 for c in cfgs)
    truncated = sum(int((onepass_want(i)[0]["status"] == CH_TRUNCATED).sum()) for i in IDS if onepass_want(i) is not None)
    pruned = 0
    for c in cfgs:
        kept = onepass_gram_ref.kept(c["wgram"], c["wos"], c["valid"])
        every = [(k, t) for (t, w) in wgram_ref.lists_of(c["wgram"]) for k in range(c["K"]) if c["wos"][k] == w and c["valid"][k]]
        levels = gram_ref.items_per_level(c["gram"], c["max_words"], c["wos"], c["valid"])
        lost_state = len(kept[1]) < c["gram"][0]
        pruned += int(len(kept[0]) < len(every) or lost_state or any(len(lv) < len(every) for lv in levels))
    gram_ids = [i for i in IDS if cc.config(i)["gram_kind"] != "anchor"]
    g_rec = np.concatenate([gram_want(i)[0] for i in gram_ids])
    g_frames = np.concatenate([cc.config(i)["n_frames"] for i in gram_ids])
    g_ok, g_rows = int(((g_rec["status"] == CH_OK) & (g_frames > 0)).sum()), int((g_frames > 0).sum())
    families = sorted({f for c in cfgs for f in c["refused"]})
    refused = {f: sum(f in c["refused"] for c in cfgs) for f in families}
    big_levels = sum(max(len(lv) for lv in gram_ref.items_per_level(c["gram"], c["max_words"], c["wos"], c["valid"])) > 64 for c in cfgs)
    print(f"\nconfig sweep coverage: {len(cfgs)} configurations, {rows} rows; level decoder CH_OK {ok}, two or more words {multi}, "
          f"CH_NONE with frames {none_with_frames}; L == 1: {l_one}, 2L - 1 > 64: {wide}; one-pass CH_TRUNCATED rows {truncated}; grammars that "
          f"lose an item or a state {pruned}; grammar levels past 64 items {big_levels}; non-anchor grammar rows CH_OK {g_ok} of {g_rows}; "
          f"refused {refused}; N = 0: {int((inf == 0).sum())}, N = 1: {int((inf == 1).sum())}, clamped {int((inf > maxf).sum())}")
    assert 2 * ok >= rows and 10 * multi >= rows and none_with_frames >= 3
    assert l_one >= 3 and wide >= 2
    assert {c["amp"] for c in cfgs} == set(cc.AMPS) and {c["skip_kind"] for c in cfgs} == set(cc.SKIP_KINDS)
    assert (inf == 0).any() and (inf == 1).any() and (inf > maxf).any()
    assert truncated >= 1 and pruned >= 2 and big_levels >= 1
    assert 4 * g_ok >= g_rows
    assert refused and all(4 * n <= len(cfgs) for n in refused.values())
    # the draws themselves: every kind of everything occurs
    assert {c["gram_kind"] for c in cfgs} == set(cc.GRAM_KINDS) and {c["word_cost"] for c in cfgs} == set(cc.WORD_COSTS)
    assert {c["win"] for c in cfgs} == set(cc.WINS) and {c["words_cap"] for c in cfgs} == set(cc.WORDS_CAPS) and {c["tail"] for c in cfgs} == {False, True}
    assert {c["frames_stride"] for c in cfgs} == {1, 3, 12} and any(c["frames_cap"] for c in cfgs) and any(c["n_exact"] for c in cfgs)
    assert {k for c in cfgs for k in c["row_kind"]} == set(cc.ROW_KINDS)
    for name, draws in cc.HOOK_DRAWS.items():
        assert {c["hooks"][name] for c in cfgs} == set(draws), name
    assert sum(len(c["inf"]) % 4 != 0 for c in cfgs) >= 8  # row counts that are no multiple of the four waves of a workgroup


def test_the_spotters_hits_depend_on_the_tie_rule():
    """the reversed rule of tests/test_spot.py (ties towards the largest start) moves the start of a hit: looked for in the
    whole-row hit and the first eight windows of the drawn width, over the templates of at most 16 frames (the restated
    recurrence is plain Python)"""
    moved = {}
    for i in IDS:
        c = cc.config(i)
        for r in range(len(c["inf"])):
            N = int(c["n_frames"][r])
            for k in range(c["K"]):
                if i in moved or not c["valid"][k] or c["tf"][k] > 16:
                    continue
                d = spot_ref.local_dis(c["im"][r, :N], c["tm"][k, :int(c["tf"][k])])
                for hit in [spot_want(i, 0)[r, 0, k]] + list(spot_want(i)[r, :8, k]):
                    if i not in moved and tuple(hit) != spot_ref.NO_HIT and t_spot._largest_start(d, int(hit["end"])) != int(hit["start"]):
                        moved[i] = (r, k)
    print(f"\nconfig sweep ties: the reversed rule moves a hit in {len(moved)} configurations: {sorted(moved)}")
    assert len(moved) >= 3


def test_the_weighted_rows_depend_on_the_guard_of_the_charge():
    """wgram_ref's wrap=True adds an arc cost to an unreachable E as 32-bit arithmetic would (all ones + c = c - 1); the
    expected rows of the weighted grammar calls must change under it, or the sweep would pass a kernel without the guard"""
    moved = []
    for i in IDS:
        c = cc.config(i)
        blind = wgram_ref.decode(c["wgram"], c["im"], c["inf"], *cc.store(c), c["maxf"], c["max_words"], c["n_exact"], c["skip"], c["word_cost"], c["wos"],
                                 wrap=True)
        if as_bytes(blind) != as_bytes(wgram_want(i)):
            moved.append(i)
    print(f"\nconfig sweep: the unguarded charge changes the weighted grammar rows of {len(moved)} configurations")
    assert len(moved) >= 3


# ---- agreements between the references ---------------------------------------------------------------------------------------------
def test_anchor_grammar_is_the_level_decoder_and_zero_costs_are_no_costs():
    for i in IDS:
        assert as_bytes(gram_want(i, "anchor")) == as_bytes(chain_want(i)), i
        assert as_bytes(wgram_want(i, "zero")) == as_bytes(gram_want(i)), i
        if cc.config(i)["gram_kind"] == "anchor":
            assert as_bytes(gram_want(i)) == as_bytes(chain_want(i)), i


def test_onepass_anchor_grammar_is_the_onepass_decoder_and_blocks_are_the_synchronous_form():
    for i in IDS:
        c = cc.config(i)
        if onepass_want(i) is not None:
            assert opgram_want(i, "anchor") is not None and as_bytes(opgram_want(i, "anchor")) == as_bytes(onepass_want(i)), i
            assert as_bytes(onepass_want(i, op_block(c))) == as_bytes(onepass_want(i)), (i, op_block(c))
        if opgram_want(i) is not None:
            assert as_bytes(opgram_want(i, "own", op_block(c))) == as_bytes(opgram_want(i)), (i, op_block(c))


def test_forced_alignment_is_the_grammar_decoder_under_the_rows_sequence_grammar():
    rows = 0
    for i in IDS:
        c = cc.config(i)
        rec, words = forced_want(i)
        for r, t in enumerate(c["transcripts"]):
            if not t:
                assert tuple(rec[r]) == (spot_ref.DIS_ERR, 0, 0, CH_NONE), (i, r)
                continue
            g = gram_ref.grammar_sequence([[w] for w in t])
            got = gram_ref.decode(g, c["im"][r:r + 1], c["inf"][r:r + 1], *cc.store(c), c["maxf"], len(t), len(t), c["skip"], c["word_cost"], c["wos"])
            assert as_bytes((got[0][0], got[1][0])) == as_bytes((rec[r], words[r, :len(t)])), (i, r)
            assert all(tuple(w) == chain_ref.NO_WORD_ROW for w in words[r, len(t):]), (i, r)
            rows += 1
    print(f"\nconfig sweep: forced alignment against the sequence grammar on {rows} rows")
    assert rows >= 40


def test_onepass_cost_is_the_smallest_level_cost_and_unique_minima_give_the_same_words():
    """over the rows the frame cap leaves whole.  A parse of more than max_words words can only be cheaper"""
    cost_rows = word_rows = skipped = 0
    for i in IDS:
        c = cc.config(i)
        if onepass_want(i) is None:
            continue
        cap = min(c["maxf"], c["frames_cap"]) if c["frames_cap"] else c["maxf"]
        (o_rec, o_words), (l_rec, l_words, lc) = onepass_want(i), chain_want(i, 0)
        for r in range(len(c["inf"])):
            N = int(c["n_frames"][r])
            if N > cap or N == 0:
                continue
            best = [int(v) for v in lc[r] if v != spot_ref.DIS_ERR] + ([N * c["skip"]] if c["skip"] is not None else [])
            if o_rec[r]["status"] == CH_NONE:
                assert not best, (i, r)
                continue
            assert not best or int(o_rec[r]["cost"]) <= min(best), (i, r)
            if int(o_rec[r]["n_words"]) > c["max_words"]:
                continue
            assert int(o_rec[r]["cost"]) == min(best), (i, r)
            cost_rows += 1
            if not int(o_rec[r]["n_words"]):
                continue
            if not unique_minimum(i, r) or int(o_rec[r]["n_words"]) > 16:
                skipped += 1
                continue
            n = min(int(o_rec[r]["n_words"]), c["words_cap"])
            assert tuple(l_rec[r])[:3] == tuple(o_rec[r])[:3] and as_bytes([l_words[r, :n]]) == as_bytes([o_words[r, :n]]), (i, r)
            word_rows += 1
    print(f"\nconfig sweep: one-pass cost = smallest level cost on {cost_rows} rows; word rows compared on {word_rows}, skipped under the tie "
          f"condition {skipped}")
    assert cost_rows >= 40 and word_rows >= 20 and 2 * skipped < word_rows + skipped


def pinned(c, r, w):
    """span_ref's score of the word's own slot over the word's own span"""
    k, s, e = int(w["slot"]), int(w["start"]), int(w["end"])
    return span_ref.span_end(spot_ref.local_dis(c["im"][r, s:e + 1], c["tm"][k, :int(c["tf"][k])]))


def test_every_reference_words_acc_is_the_span_scorers_pinned_score():
    seen = 0
    for i in IDS:
        c = cc.config(i)
        for what, out in (("level", chain_want(i)), ("grammar", gram_want(i)), ("weighted", wgram_want(i)), ("one pass", onepass_want(i)),
                          ("one-pass grammar", opgram_want(i)), ("forced", forced_want(i))):
            if out is None:
                continue
            for r in range(len(c["inf"])):
                for w in out[1][r]:
                    if tuple(w) != chain_ref.NO_WORD_ROW:
                        assert int(w["acc"]) == pinned(c, r, w) and int(w["end"]) < int(c["n_frames"][r]), (i, what, r, tuple(w))
                        assert int(w["dis"]) == int(w["acc"]) // (int(w["end"]) - int(w["start"]) + 1 + int(c["tf"][int(w["slot"])])), (i, what, r)
                        seen += 1
    print(f"\nconfig sweep: acc = pinned span score on {seen} reference words")
    assert seen >= 500
