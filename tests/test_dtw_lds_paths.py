"""Every path through a step of k_dtw_lds: each case pins one branch of the walk's control flow at the smallest shape
that reaches it, and is compared for equality against the CPU oracle's greedy DTW.

k_dtw_lds keeps one lane per (utterance, template) pair; the lanes of a wave run the walk's loop together.  What can go wrong
in it is control flow: a lane that leaves the loop while its neighbours go on, trips in which no lane of a wave advances in
the template (or in the utterance), the out-of-line fix for a root that came out one short, the literal three-root form for
roots beyond the staged tie table, and the row format of 13..16 coefficients.  (-m gpu, but for the last test, which needs
none.)  Every construction is first checked on the CPU with a restatement of the reference's walk (walk(), itself held against the oracle's score for every pair of every case), so
a case that does not reach its path fails instead of passing for nothing.

A walk with all three candidates outside dtw_limit's band (DTW.C:156-184, the kernel's `lost` lanes) has no case here: no pair
inside the length gate can reach such a point, which test_no_pair_inside_the_gate_loses_the_band shows by following every
admissible move of every length pair of up to LOST_SEARCH frames."""
import numpy as np
import pytest

import oracle_lib as ol
from stm32_speech_recognition_amd import Engine
from stm32_speech_recognition_amd.engine import dev_hook
from test_long_sequences import set_store_and_plan

gpu = pytest.mark.gpu

MAXF = 48          # frame cap of every case
ROWS = MAXF + 1    # template rows: one row of slack behind the longest template (DTW.C:150-154)
LOST_SEARCH = 48
GEN13 = next(c for c in ol.GENERIC_CONFIGS if c[0].get("n_coef") == 13)
GEN16 = next(c for c in ol.GENERIC_CONFIGS if c[0].get("n_coef") == 16)


# ---- the reference's walk, restated with its trace ---------------------------------------------------------------------------
def outside(x, y, X1, X2, in_n, mdl_n):
    """dtw_limit (DTW.C:76-109): True when (x, y) lies outside the relaxed parallelogram"""
    o1 = (y >= 2 * x + 2) if x < X1 else (2 * y + in_n - 2 * mdl_n >= x + 4)
    o2 = (2 * y + 2 <= x) if x < X2 else (y + 4 <= 2 * x + mdl_n - 2 * in_n)
    return o1 or o2


def dist2(a, b):
    return int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) & 0xFFFFFFFF  # get_dis' sum in u32 wrap (DTW.C:45-62)


def root(d):
    return int(np.sqrt(np.float32(d)))  # (u32)sqrtf((float)d)


def walk(a, na, b, nb):
    """dtw (DTW.C:120-192) of a [>= na + 1 rows] against b [>= nb + 1 rows]: (score, one record per step) -- a step's record
    holds the point it starts from, which of (up, right, diagonal) lie outside, the three squared distances, the smallest
    admissible one (m2), the step's cost (mn) and the move ('u', 'r', 'd')"""
    if na > 2 * nb or 2 * na < nb:
        return ol.DIS_ERR, []
    X1, X2 = ((2 * nb - na) // 3) & 0xFFFF, ((4 * na - 2 * nb) // 3) & 0xFFFF
    x = y = 1
    dis, step, trace = root(dist2(a[0], b[0])), 1, []
    while True:
        out = (outside(x, y + 1, X1, X2, na, nb), outside(x + 1, y, X1, X2, na, nb), outside(x + 1, y + 1, X1, X2, na, nb))
        q = (dist2(b[y], a[x - 1]), dist2(b[y - 1], a[x]), dist2(b[y], a[x]))
        up, right, diag = (ol.DIS_ERR if o else root(d) for o, d in zip(out, q))
        mn = min(diag, right, up)
        dis = (dis + mn) & 0xFFFFFFFF
        mv = "d" if mn == diag else ("u" if mn == up else "r")
        adm = [d for o, d in zip(out, q) if not o]
        trace.append(dict(x=x, y=y, out=out, q=q, m2=min(adm) if adm else ol.DIS_ERR, mn=mn, mv=mv))
        x += mv in "dr"
        y += mv in "du"
        step = (step + 1) & 0xFFFF
        if not (x < na and y < nb):
            return dis // step, trace


def longest_run(moves, m):
    best = cur = 0
    for c in moves:
        cur = cur + 1 if c == m else 0
        best = max(best, cur)
    return best


class Case:
    """utterances im [B, MAXF, nc] / inf [B], templates tm [K, ROWS, nc] / tf [K] / valid [K]; the walk of every pair"""

    def __init__(self, im, inf, tm, tf, valid=None, cfg=(dict(), dict())):
        self.im, self.inf = np.ascontiguousarray(im, np.int16), np.asarray(inf, np.uint32)
        self.tm, self.tf = np.ascontiguousarray(tm, np.int16), np.asarray(tf, np.uint32)
        self.valid = np.ones(len(tf), np.uint8) if valid is None else np.asarray(valid, np.uint8)
        self.cfg = cfg
        B, K, nc = len(self.inf), len(self.tf), self.im.shape[2]
        orc = ol.Oracle(max_frames=MAXF, **cfg[1])
        pad = np.zeros((1, nc), np.int16)
        self.want = np.full((B, K), ol.DIS_ERR, np.uint32)
        self.trace = {}
        for b in range(B):
            a = np.concatenate([self.im[b], pad])  # row inf[b] is the slack row the do-while reads
            for k in range(K):
                if not self.valid[k] or not self.inf[b]:
                    continue
                na, nb = int(self.inf[b]), int(self.tf[k])
                self.want[b, k], self.trace[b, k] = walk(a, na, self.tm[k], nb)
                assert self.want[b, k] == orc.dtw(a, na, self.tm[k], nb), (b, k)  # walk() IS the oracle's walk

    def waves(self, U, kc):
        """the pairs (b, k) of every wave of the launch: templates in stable order of their length (erased slots last), kc ranks
        per workgroup, lanes rank major / utterance minor, U utterances per workgroup"""
        K, B = len(self.tf), len(self.inf)
        order = sorted(range(K), key=lambda k: int(self.tf[k]) if self.valid[k] else 1 << 32)
        out = []
        for b0 in range(0, B, U):
            for r0 in range(0, K, kc):
                lanes = [(b0 + t % U, order[r0 + t // U]) if b0 + t % U < B and r0 + t // U < min(K, r0 + kc) else None
                         for t in range(U * kc)]
                out += [[p for p in lanes[i:i + 64] if p] for i in range(0, U * kc, 64)]
        return [w for w in out if w]

    def steps(self, pairs):
        """step records of the pairs that walk at all"""
        return [self.trace[p] for p in pairs if self.trace.get(p)]

    def run(self, capfd, **hooks):
        """scores of k_dtw_lds (small-launch mode 1: the batch kernel whatever the launch size) and the plan it ran with"""
        for h, v in hooks.items():
            dev_hook(h, v)
        try:
            eng = Engine(max_frames=MAXF, device=0, testing=True, **self.cfg[0])
            plan = set_store_and_plan(eng, capfd, self.tm, self.tf, self.valid)
        finally:
            for h in hooks:
                dev_hook(h, 0)
        assert plan["U"] >= 1 and plan["K"] == len(self.tf) and plan["R"] == MAXF, plan  # the store is staged: k_dtw_lds serves it
        eng.set_small_launch(1)
        sc, res = eng.dtw(self.im, self.inf)
        eng.close()
        assert np.array_equal(sc, self.want), (plan, np.argwhere(sc != self.want)[:8])
        best = np.array([int(np.argmin(w)) if w.min() != ol.DIS_ERR else 0 for w in self.want])
        assert np.array_equal(res["best_tpl"], best) and np.array_equal(res["min_dis"], self.want.min(1))
        return plan


def rows(rng, n, nc, amp=300):
    r = rng.integers(-amp, amp + 1, (n, nc)).astype(np.int16)
    r[n // 3] = r[n // 3 + 1] if n // 3 + 1 < n else r[n // 3]  # a repeated row: exact ties between the candidates
    return r


def mixed_case(nc=12, cfg=(dict(), dict())):
    """B = 7 utterances x K = 13 templates of 1..40 frames: lanes of one wave leave the loop in many different trips, 1-frame
    sequences on both sides (the slack-row read), pairs the length gate rejects, an erased slot, an utterance without frames"""
    rng = np.random.default_rng(1007)
    inf = [23, 1, 40, 2, 0, 31, 12]
    tf = [17, 1, 40, 26, 9, 2, 33, 21, 38, 5, 14, 29, 24]
    valid = [1] * 13
    valid[7] = 0
    im, tm = np.zeros((7, MAXF, nc), np.int16), np.zeros((13, ROWS, nc), np.int16)
    for b, n in enumerate(inf):
        im[b, :n + 1] = rows(rng, n + 1, nc)
    for k, n in enumerate(tf):
        tm[k, :n + 1] = rows(rng, n + 1, nc)
    return Case(im, inf, tm, tf, valid, cfg)


def check_mixed(case, plan):
    waves = case.waves(plan["U"], plan["kc"])
    assert len(waves) > 1 and len(waves[-1]) < 64                      # more than one wave, the last one partly empty
    leave = [sorted({len(t) for t in case.steps(w)}) for w in waves]
    assert max(len(l) for l in leave) >= 4, leave                     # lanes of one wave leave in several different trips
    inf, tf = case.inf, case.tf
    gate = lambda b, k: case.valid[k] and inf[b] and not (inf[b] > 2 * tf[k] or 2 * inf[b] < tf[k])
    pairs = [(b, k) for b in range(len(inf)) for k in range(len(tf))]
    assert any(gate(b, k) and inf[b] == 1 for b, k in pairs) and any(gate(b, k) and tf[k] == 1 for b, k in pairs)
    assert any(case.valid[k] and inf[b] and not gate(b, k) for b, k in pairs) and not case.valid.all() and not inf.all()


@pytest.fixture(scope="module")
def mixed():
    return mixed_case()


@gpu
def test_lanes_leave_in_different_trips(mixed, capfd):
    plan = mixed.run(capfd)
    assert len(mixed.inf) % plan["U"] != 0, plan  # the last workgroup's utterances run past the batch
    check_mixed(mixed, plan)


@gpu
@pytest.mark.parametrize("u", [1, 16])
def test_forced_geometries(mixed, capfd, u):
    plan = mixed.run(capfd, dtw_u=u)
    assert plan["U"] == u and plan["kc"] == 13, plan
    check_mixed(mixed, plan)


@gpu
@pytest.mark.parametrize("cfg", [GEN13, GEN16], ids=["13", "16"])
def test_wide_rows(capfd, cfg):
    """the 16-wide row format (GENERIC front end's rows of 13..16 coefficients) at the mixed shape"""
    case = mixed_case(cfg[0]["n_coef"], cfg)
    check_mixed(case, case.run(capfd))


def ramp_case():
    """Monotone one-coefficient rows: the utterance dwells on a value while the template moves on, and the other way round,
    so the walk goes right several times in a row (no lane advances y), later up several times in a row (no lane advances
    x).  Every utterance and every template is the same, so every lane of every wave makes the same move in every trip."""
    tv = [0, 10, 20, 30, 40, 50, 60, 60, 60, 60, 60, 70, 80, 90, 100, 110, 120, 120, 120, 120, 120, 130, 140, 150]
    uv = [0, 10, 20, 30, 40, 40, 40, 40, 40, 50, 60, 70, 80, 90, 100, 100, 100, 100, 100, 110, 120, 130, 140, 150]
    B, K = 3, 5
    im, tm = np.zeros((B, MAXF, 12), np.int16), np.zeros((K, ROWS, 12), np.int16)
    im[:, :len(uv), 0], tm[:, :len(tv), 0] = uv, tv
    im[:, len(uv):, 0], tm[:, len(tv):, 0] = uv[-1], tv[-1]
    return Case(im, [len(uv)] * B, tm, [len(tv)] * K)


@gpu
def test_trips_without_a_y_advance_and_without_an_x_advance(capfd):
    case = ramp_case()
    moves = ["".join(s["mv"] for s in t) for t in case.steps(case.trace)]
    assert len(set(moves)) == 1 and len(moves) == 15  # one walk, in every lane
    assert longest_run(moves[0], "r") >= 3 and longest_run(moves[0], "u") >= 3, moves[0]
    case.run(capfd)


def squares_case():
    """Squared distances that are exact squares, and their neighbours: the root taken from below comes out one short exactly
    at the squares (and where the float conversion rounds onto one).  Small rows (distances up to a few dozen), rows on a
    grid of 37 with a second coefficient of 0 / 1 (k^2 and k^2 + 1 up to a million), and both against each other."""
    rng = np.random.default_rng(404)
    B, K, n = 6, 6, 30
    im, tm = np.zeros((B, MAXF, 12), np.int16), np.zeros((K, ROWS, 12), np.int16)
    for arr in (im, tm):
        arr[:3, :n + 1] = rng.integers(0, 3, (3, n + 1, 12))
        arr[3:, :n + 1, 0] = 37 * rng.integers(0, 30, (3, n + 1))
        arr[3:, :n + 1, 1] = rng.integers(0, 2, (3, n + 1))
    return Case(im, [n] * B, tm, [n] * K)


@gpu
def test_root_one_short(capfd):
    case = squares_case()
    m2 = {s["m2"] for t in case.steps(case.trace) for s in t}
    sq = {k * k for k in range(2, 1200)}
    assert len(m2 & sq) >= 8 and 0 in m2 and 1 in m2, sorted(m2)[:40]
    assert {d for d in m2 if d + 1 in sq} and {d for d in m2 if d - 1 in sq and d > 10000}, sorted(m2)[:40]
    assert max(m2 & sq) >= 250000
    case.run(capfd)


def far_case():
    """coefficients near +-16 383 (the edge of what k_dtw_lds stages): the first five rows of every sequence are small, from
    there on three coefficients sit near -16 383 in the utterances and near +16 383 in the templates.  A walk starts with small
    roots, crosses rows of one kind against the other (roots near 28 000) and ends with roots near 56 000 -- beyond every size
    of the staged tie table -- so each kind of root occurs in every lane"""
    rng = np.random.default_rng(77)
    B, K, n = 7, 13, 20
    im, tm = np.zeros((B, MAXF, 12), np.int16), np.zeros((K, ROWS, 12), np.int16)
    for arr, cnt, sign in ((im, B, -1), (tm, K, 1)):
        v = rng.integers(-200, 201, (cnt, n + 1, 12))
        v[:, 5:, :3] = sign * (16383 - rng.integers(0, 40, (cnt, n + 1 - 5, 3)))
        arr[:, :n + 1] = v
    return Case(im, [n] * B, tm, [n] * K)


@gpu
def test_roots_beyond_the_tie_table(capfd):
    case = far_case()
    assert np.abs(case.im).max() <= 16383 and np.abs(case.tm).max() <= 16383 and np.abs(case.tm).max() > 16300
    plan = case.run(capfd)
    for w in case.waves(plan["U"], plan["kc"]):
        mn = [s["mn"] for t in case.steps(w) for s in t]
        assert max(mn) >= 32768 and any(8192 < r < 32767 for r in mn) and min(mn) < 4096, (min(mn), max(mn))
    # ... and with the smallest table the plan may stage next to the largest, so that "beyond the table" starts at 4 095 / 32 767
    for g in (4096, 32768):
        case.run(capfd, dtw_tie_g=g)


def test_no_pair_inside_the_gate_loses_the_band():
    """DTW.C:156-184 with all three candidates outside: unreachable.  From (1, 1) follow EVERY admissible move (whatever the
    features, the walk makes one of them) for every length pair inside the gate: no point the loop can stand on has all three
    neighbours outside.  (The reason: the two pieces of dtw_limit's band that could pinch it off -- the lower bound of slope 2
    and the upper bound of slope 1/2 -- meet three rows behind the end point (in, mdl), and the loop ends at x = in or y = mdl.)"""
    for na in range(1, LOST_SEARCH + 1):
        for nb in range((na + 1) // 2, min(2 * na, LOST_SEARCH) + 1):
            X1, X2 = ((2 * nb - na) // 3) & 0xFFFF, ((4 * na - 2 * nb) // 3) & 0xFFFF
            seen, todo = {(1, 1)}, [(1, 1)]
            while todo:
                x, y = todo.pop()
                if (x, y) != (1, 1) and not (x < na and y < nb):
                    continue
                nxt = [p for p in ((x, y + 1), (x + 1, y), (x + 1, y + 1)) if not outside(p[0], p[1], X1, X2, na, nb)]
                assert nxt, (na, nb, x, y)
                for p in nxt:
                    if p not in seen:
                        seen.add(p)
                        todo.append(p)
