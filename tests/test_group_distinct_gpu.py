"""Aggregates over the distinct values of a group on the MI355X (run with -m gpu): sdqh_table_group_distinct
(include/sdqh_sort_distinct.h) against numpy at every size at which the sort, the wave batches or the tile carries of either stage take
another path, on patterns that put run ends, group ends and mode ties on those edges, against its sibling sdqh_table_grouping_sets,
against exact rational sums, on every table layout, over derived and text-ranked terms, and its contract.

The expected groups are the table's own rows (sdqh_table_compact) in the order of a STABLE numpy lexsort over the documented
order-preserving map (test_window_gpu.Ranked: its partition heads are the group heads, its tie heads the run heads), the runs folded
with numpy's reduceat.  Nothing is imported from the product's fold code.  Doubles in exact comparisons are integer-valued and below
2^40, so their sums are exact in any association."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from test_grouping_sets_gpu import PACK, UF, _bits, _column, _terms
from test_window_gpu import Ranked, _probed_table, _same, _stage_rows, _table, _under, db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)
from test_window_range_gpu import _range_table

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
CD, SD, AD, MODE, MC, CNT = abi.GD_COUNT_DISTINCT, abi.GD_SUM_DISTINCT, abi.GD_AVG_DISTINCT, abi.GD_MODE, abi.GD_MODE_COUNT, abi.GD_COUNT
OPS = (CD, SD, AD, MODE, MC, CNT)
I_MIN, I_MAX = abi.INT64_MIN, abi.INT64_MAX
MEASURES = [(P, 3, False), (P, 2, True), (K, 0, False)]                    # _range_table's integers, its doubles, the key
COMBOS = [(op,) + m for op in OPS for m in MEASURES]


class Distinct:
    """The groups (equal in the first ngroup terms) and value runs (equal in all) of the rows in the order of `terms`, and the
    aggregates over them, by numpy from the definition."""

    def __init__(self, rows, terms, ngroup, rank_tables=None):
        self.rows, self.ngroup = rows, ngroup
        r = Ranked(rows, terms, ngroup, rank_tables)
        self.n, self.order = r.n, r.order
        self.rstart = np.nonzero(r.tie_head)[0]                             # the runs' first sorted positions
        self.rlen = np.diff(np.append(self.rstart, self.n)).astype(np.int64)
        self.gfirst = np.nonzero(r.part_head[self.rstart])[0]               # per group its first run
        self.g, self.nruns = len(self.gfirst), len(self.rstart)
        self.runs = np.diff(np.append(self.gfirst, self.nruns)).astype(np.int64)
        self.gstart = self.rstart[self.gfirst]                              # the groups' first sorted positions
        if self.g:
            self.longest = np.maximum.reduceat(self.rlen, self.gfirst)
            group_of = np.repeat(np.arange(self.g), self.runs)
            self.tied = self.rlen == self.longest[group_of]
            self.winner = np.minimum.reduceat(np.where(self.tied, np.arange(self.nruns), self.nruns), self.gfirst)      # the earliest of the longest

    def value(self, agg):
        op, kind, index, is_f64 = agg
        f64 = op in (SD, AD, MODE) and (kind == V or (kind == P and is_f64))
        if not self.g:
            return np.zeros(0, np.float64 if (f64 or op == AD) else np.int64)
        if op == CD:
            return self.runs
        if op == CNT:
            return np.add.reduceat(self.rlen, self.gfirst)
        if op == MC:
            return self.longest
        src = np.ascontiguousarray(_column(self.rows, kind, index))
        src = src.view(np.float64) if f64 and src.dtype != np.float64 else src
        if op == MODE:
            return src[self.order[self.rstart[self.winner]]]
        reps = src[self.order[self.rstart]]                                  # the measure at every run's representative
        s = np.add.reduceat(reps, self.gfirst) if f64 else np.add.reduceat(np.ascontiguousarray(reps).view(np.uint64), self.gfirst).view(np.int64)
        return s if op == SD else s.astype(np.float64) / self.runs.astype(np.float64)


def _expect_dtype(agg):
    op, kind, _, is_f64 = agg
    return np.float64 if op == AD or (op in (SD, MODE) and (kind == V or (kind == P and is_f64))) else np.int64


def _check(ctx, t, ref, terms, aggs, what, limit=ALL, want_hits=False, min_hits=0):
    got = ctx.table_group_distinct(t, min_hits, terms, ref.ngroup, aggs, limit, 64, want_hits=want_hits)
    _same(got, ref.rows, ref.order[ref.gstart[:limit]], what)
    assert len(got[4]) == len(aggs)
    for a, agg in enumerate(aggs):
        want = ref.value(agg)[:limit]
        assert got[4][a].dtype == _expect_dtype(agg) == want.dtype, (what, agg, got[4][a].dtype, want.dtype)
        same = _bits(got[4][a]) == _bits(want)
        assert same.all(), (what, agg, int(np.argmin(same)), got[4][a][~same][:4], want[~same][:4])
    return got


def _sizes(ctx):
    T = ctx.window_geometry()
    S = ctx.sort_geometry()[0]
    assert ctx.group_distinct_geometry() == T
    return T, S, sorted({0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, S - 1, S, S + 1, 4095, 4096, 4097, 65537})


PATTERNS = ["every row its own value", "one group with one value", "every row its own group", "a value run over three tiles", "runs across a run-tile edge",
            "edges", "edges, every run a group", "mode ties", "the longest run is the last"]


def _by_runs(lens, groups, n):
    """(b, c) by sorted position of runs of the given lengths in the given groups, cut at n or filled up with runs of 3 in groups of 67 positions"""
    run = np.repeat(np.arange(len(lens)), lens)[:n]
    grp = np.repeat(np.asarray(groups), lens)[:n]
    rest = np.arange(n - len(run), dtype=np.int64)
    return (np.concatenate([grp, grp.max(initial=-1) + 1 + rest // 67]).astype(np.int64),
            np.concatenate([run, run.max(initial=-1) + 1 + rest // 3]).astype(np.int64))


def _pattern(name, n, T):
    """(a, b, c) by sorted position, each non-decreasing: (a, b) is the group, c the value"""
    pos = np.arange(n, dtype=np.int64)
    a, b, c = pos // (T + 37), pos // 67, pos // 3
    if name == "every row its own value":                                   # as many runs as rows: the upper stage crosses its own tile edges at T and 2T runs
        a, b, c = pos * 0, pos // (T + 188), pos
    elif name == "one group with one value":
        a, b, c = pos * 0, pos * 0, pos * 0
    elif name == "every row its own group":
        a, b, c = pos * 0, pos, pos * 0
    elif name == "a value run over three tiles":
        a = pos * 0
        lo, hi = T - 10, min(n, 3 * T + 6)
        if lo < n:
            b[lo:hi], c[lo:hi] = b[lo], c[lo]
    elif name == "runs across a run-tile edge":                             # runs of 3 rows, groups of 200 runs: run T lies inside a group
        a, b = pos * 0, pos // 600
    elif name in ("edges", "edges, every run a group"):
        starts = np.array([63, 64, 65, T - 1, T, T + 1])
        c = np.searchsorted(starts, pos, side="right").astype(np.int64)
        a, b = c // 4, (c // 2 if name == "edges" else c)
    elif name == "mode ties":
        a = pos * 0
        lens = [3, 3, 1, 1]                                                 # group 0: two longest runs in one wave batch
        groups = [0] * 4
        one = [1] * (T - 13) + [3] + [1] * 4 + [3] + [1]                    # group 1: two longest runs [T - 5, T - 2) and [T + 2, T + 5), on either side of the row-tile edge
        lens, groups = lens + one, groups + [1] * len(one)
        assert sum(lens[:4 + T - 13]) == T - 5 and len(lens) == T - 2
        lens, groups = lens + [2, 1, 1, 2, 1], groups + [2] * 5             # group 2: runs T - 2 .. T + 2, the longest are runs T - 2 and T + 1, on either side of the run-tile edge
        b, c = _by_runs(lens, groups, n)
    elif name == "the longest run is the last":
        a, b, c = pos * 0, pos // 10, (pos // 10) * 4 + np.array([0, 1, 1, 2, 2, 2, 3, 3, 3, 3])[pos % 10]
    return a, b, c


def _pattern_table(ctx, name, n, T, desc, rng):
    a, b, c = _pattern(name, n, T)
    if desc and n:
        a, b, c = a.max() - a, b.max() - b, c.max() - c                     # (descending terms over mirrored values: the same sorted order)
    ints = rng.integers(-1000, 1000, n).astype(np.int64)
    if n > 2:
        ints[rng.integers(0, n, 2)] = [I_MIN, I_MAX]
    if n > 70:
        ints[[61, 62, 63, 64]] = [I_MAX, I_MAX, I_MIN, I_MIN]
    dbls = rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64)
    mix = rng.permutation(n)                                                # rows in random build order
    return _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], ints[mix])


# 1. patterns x sizes, exact by bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    placements, last_wins, straddles = set(), False, False
    for i, n in enumerate(sizes):
        desc = bool(i & 1)
        terms = _terms(desc)
        t = _pattern_table(ctx, pattern, n, T, desc, rng)
        try:
            rows = _stage_rows(ctx, t, 0)
            for k, ngroup in enumerate((2, 1, 0)):                          # the value: c; the pair (b, c); all three, one group
                ref = Distinct(rows, terms, ngroup)
                assert ref.n == n
                at = (i * 3 + k) * 4
                aggs = [COMBOS[(at + j) % len(COMBOS)] for j in range(4)]
                what = (pattern, n, ngroup)
                got = _check(ctx, t, ref, terms, aggs, what)
                assert ctx.table_group_distinct_count(t, 0, terms, ngroup, aggs) == ref.g == len(got[0]), what
                again = ctx.table_group_distinct(t, 0, terms, ngroup, aggs, ALL, max(1, ref.g))
                assert all((_bits(x) == _bits(y)).all() for x, y in zip(got[4], again[4])), what
                if ref.g > 1:                                               # limit cuts the output, not the groups
                    _check(ctx, t, ref, terms, [COMBOS[3], COMBOS[10], COMBOS[13]], what + ("limit",), limit=ref.g // 2)
                if ngroup == 2 and ref.g:
                    straddles |= bool(((ref.gfirst < T) & (ref.gfirst + ref.runs > T)).any())
                    last_wins |= bool(((ref.winner == ref.gfirst + ref.runs - 1) & (ref.runs > 1)).any())
                    for j in np.nonzero(np.add.reduceat(ref.tied.astype(np.int64), ref.gfirst) > 1)[0]:
                        r1, r2 = (ref.gfirst[j] + np.nonzero(ref.tied[ref.gfirst[j]:ref.gfirst[j] + ref.runs[j]])[0])[:2]
                        p1, p2 = ref.rstart[r1], ref.rstart[r2]
                        if p1 // 64 == p2 // 64:
                            placements.add("one wave batch")
                        if p1 // T != p2 // T:
                            placements.add("row-tile edge")
                        if r1 // T != r2 // T:
                            placements.add("run-tile edge")
        finally:
            t.free()
    full = Distinct(rows, terms, 2)                                          # the largest size
    if pattern == "every row its own value":
        assert full.nruns == full.n > 2 * T and straddles
    if pattern == "runs across a run-tile edge":
        assert full.nruns > 2 * T and straddles
    if pattern == "a value run over three tiles":
        assert (full.rlen > 2 * T).any()
    if pattern in ("edges", "edges, every run a group"):
        assert set(full.rstart) == {0, 63, 64, 65, T - 1, T, T + 1}
        assert set(full.gstart) == ({0, 64, T - 1, T + 1} if pattern == "edges" else set(full.rstart))
    if pattern == "mode ties":
        assert placements == {"one wave batch", "row-tile edge", "run-tile edge"}
    if pattern == "the longest run is the last":
        assert last_wins


# 2. consistency, and agreement with the sibling ---------------------------------------------------------------------------------------------
def test_consistency_and_agreement_with_grouping_sets(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 2 * T + 77
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 4, n).astype(np.int64), rng.integers(0, 9, n).astype(np.int64)
    c = rng.integers(0, 12, n).astype(np.int64) // np.where(b == 3, 100, 1)   # the groups with b == 3 hold one value
    t = _range_table(ctx, a * PACK + b, c, rng.integers(-99, 99, n).astype(np.float64), rng.integers(-99, 99, n))
    terms = _terms(True)
    try:
        for ngroup in (0, 1, 2):
            got = ctx.table_group_distinct(t, 0, terms, ngroup, [(CNT, K, 0, False), (CD, K, 0, False), (MC, K, 0, False)], ALL, 64, want_hits=False)
            count, distinct, most = got[4]
            gs = ctx.table_grouping_sets(t, 0, terms, (1 << 3) | (1 << ngroup), [(abi.WAGG_COUNT, K, 0, False)], ALL, 64, want_hits=False)
            nruns, ngroups = int(gs[5][3]), int(gs[5][ngroup])
            run_rows, group_rows = gs[4][0][:nruns], gs[4][0][nruns:]
            assert ngroups == len(count) and (_bits(count) == _bits(group_rows)).all(), ngroup      # COUNT is grouping sets' COUNT at level ngroup
            last_run = np.searchsorted(np.cumsum(run_rows), np.cumsum(group_rows))                  # the run that ends where the group ends
            runs_in = np.diff(np.concatenate([[-1], last_run]))
            assert (distinct == runs_in).all() and int(distinct.sum()) == nruns, ngroup             # COUNT_DISTINCT is the level-nterms count inside each group
            first_run = last_run - runs_in + 1
            assert (count == np.add.reduceat(run_rows, first_run)).all() and (most <= count).all() and (most == np.maximum.reduceat(run_rows, first_run)).all()
            assert ((most == count) == (distinct == 1)).all(), ngroup
            assert ngroup != 2 or ((distinct == 1).any() and (distinct > 1).any())
    finally:
        t.free()


# 3. doubles ----------------------------------------------------------------------------------------------------------------------------------
def test_nothing_leaks_between_neighbouring_groups(hip_engine):
    ctx = hip_engine.ctx
    T, _, _ = _sizes(ctx)
    n = 2 * T + 50
    rng = np.random.default_rng(3)
    pos = np.arange(n, dtype=np.int64)
    a, b, c = pos // (T + 37), pos // 5, pos                                # every row its own value: run index = sorted position, one tile edge for both stages
    assert (T - 1) // 5 == T // 5                                           # the group of position T - 1 crosses the tile edge
    dbls = rng.integers(-9, 10, n).astype(np.float64)
    dbls[T - 1], dbls[(T // 5 + 1) * 5 + 1] = 1e300, -1e300                 # ... next to a group with the opposite giant
    mix = rng.permutation(n)
    t = _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], pos[mix])
    terms = _terms(False)
    try:
        seen = {0: 0, 1: 0, 2: 0}
        for ngroup in (2, 1, 0):
            ref = Distinct(_stage_rows(ctx, t, 0), terms, ngroup)
            got = ctx.table_group_distinct(t, 0, terms, ngroup, [(SD, P, 2, True), (AD, P, 2, True), (CD, K, 0, False), (CNT, K, 0, False)], ALL, 64)
            assert len(got[0]) == ref.g and (got[4][2] == ref.runs).all() and (got[4][3] == ref.runs).all()
            for j in range(ref.g):
                v = dbls[ref.gstart[j]:ref.gstart[j] + ref.runs[j]]         # (sorted position = pos)
                huge = int((np.abs(v) > 1e200).sum())
                if huge == 0:
                    assert got[4][0][j] == v.sum() and got[4][1][j] == v.sum() / len(v), (ngroup, j)
                elif huge == 1:                                             # the small ones vanish beside it, in any order
                    assert abs(got[4][0][j]) == 1e300, (ngroup, j)
                seen[huge] += 1
        assert seen[0] > 100 and seen[1] == 2 and seen[2] >= 2
    finally:
        t.free()


def test_general_doubles_within_the_bound(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    for n in (S + 1, 4097):
        rng = np.random.default_rng(n)
        pos = np.arange(n, dtype=np.int64)
        a, b, c = pos // (T + 37), pos // 7, pos // 2                      # groups of three or four runs, of some hundred, and one of all
        dbls = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)
        mix = rng.permutation(n)
        t = _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], pos[mix])
        terms = _terms(False)
        try:
            rows = _stage_rows(ctx, t, 0)
            checked = 0
            for ngroup in (2, 1, 0):
                ref = Distinct(rows, terms, ngroup)
                aggs = [(SD, P, 2, True), (CD, K, 0, False), (AD, P, 2, True)]
                got = ctx.table_group_distinct(t, 0, terms, ngroup, aggs, ALL, 64)
                again = ctx.table_group_distinct(t, 0, terms, ngroup, aggs, ALL, 64)
                assert all((_bits(x) == _bits(y)).all() for x, y in zip(got[4], again[4]))
                assert (_bits(got[4][2]) == _bits(got[4][0] / got[4][1].astype(np.float64))).all()      # AVG_DISTINCT = SUM_DISTINCT / COUNT_DISTINCT, one division
                assert (got[4][1] == ref.runs).all()
                reps = np.ascontiguousarray(rows[1][2]).view(np.float64)[ref.order[ref.rstart]]
                for j in range(0, ref.g, 37):
                    v = reps[ref.gfirst[j]:ref.gfirst[j] + ref.runs[j]]
                    m = int(ref.runs[j])
                    exact = sum((Fraction(float(x)) for x in v), Fraction(0))
                    gamma = Fraction((m - 1) * UF) / (1 - Fraction((m - 1) * UF))
                    assert abs(Fraction(float(got[4][0][j])) - exact) <= gamma * sum(Fraction(abs(float(x))) for x in v), (n, ngroup, j)
                    checked += 1
            assert checked >= 5
        finally:
            t.free()


def test_zeros_and_nan_payloads_are_values_of_their_own(hip_engine):
    ctx = hip_engine.ctx
    nan_a, nan_b = np.array([0x7FF8000000000001, 0xFFF8000000000002], np.uint64).view(np.float64)
    group = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2], np.int64)
    vals = np.array([0.0, -0.0, nan_a, nan_b, nan_a, -0.0, 0.0, nan_a, 5.0, nan_b, nan_b, -0.0, 1.0, nan_b])
    n = len(vals)
    t = _range_table(ctx, group, vals, vals, np.arange(n))                  # payload 1 and payload 2: the bits of the doubles
    terms = [(P, 0, False, False), (P, 1, False, True)]
    try:
        ref = Distinct(_stage_rows(ctx, t, 0), terms, 1)
        aggs = [(CD, K, 0, False), (MODE, P, 2, True), (MC, K, 0, False), (CNT, K, 0, False)]      # (no sum: which NaN's payload a sum of two carries is the adder's business)
        got = _check(ctx, t, ref, terms, aggs, "zeros and nans")
        assert got[4][0].tolist() == [5, 3] and got[4][2].tolist() == [3, 3]           # -0.0, +0.0, two NaN payloads (and 5.0): values of their own
        assert _bits(got[4][1]).tolist() == [_bits(np.array([nan_a]))[0], _bits(np.array([nan_b]))[0]]      # MODE copies the payload
        one = Distinct(_stage_rows(ctx, t, 0), terms, 0)
        got = _check(ctx, t, one, terms, [(CD, K, 0, False), (MODE, P, 2, True), (MC, K, 0, False)], "zeros and nans, one group")
        assert got[4][0].tolist() == [8] and got[4][2].tolist() == [3] and _bits(got[4][1])[0] == _bits(np.array([nan_a]))[0]      # the pairs (group, value); of two runs of three the first
        zeros = _range_table(ctx, np.zeros(6, np.int64), np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0]), np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0]), np.arange(6))
        try:
            zref = Distinct(_stage_rows(ctx, zeros, 0), terms, 1)
            got = _check(ctx, zeros, zref, terms, [(CD, K, 0, False), (MODE, P, 2, True), (SD, P, 2, True), (AD, P, 2, True)], "signed zeros")
            assert got[4][0].tolist() == [2] and _bits(got[4][1])[0] == I_MIN       # a tie of three and three: -0.0 sorts first
        finally:
            zeros.free()
    finally:
        t.free()


# 4. layouts ----------------------------------------------------------------------------------------------------------------------------------
def test_layouts(hip_engine):
    """The direct layout, a table with duplicate build keys (owner rows only), the open-addressing layout, the probed table of the
    ordering tests, each with min_hits 0 and 2; VALUE and HITS as value terms and as measures; a two-term value; no grouping term."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(n)
    part = rng.integers(0, 9, n).astype(np.int64)
    value = rng.integers(-5, 5, n).astype(np.float64)
    hits = rng.integers(0, 4, n)                                           # some entries never probed: min_hits selects
    term_lists = [([(P, 0, True, False), (H, 0, False, False)], 1), ([(P, 0, False, False), (V, 0, True, True)], 1), ([(H, 0, True, False), (P, 0, False, False), (V, 0, False, True)], 1),
                  ([(V, 0, False, True), (H, 0, False, False)], 0)]
    agg_lists = [[(SD, V, 0, True), (MODE, H, 0, False), (AD, H, 0, False), (CD, K, 0, False)],
                 [(SD, H, 0, False), (MODE, V, 0, True), (CNT, K, 0, False), (MC, K, 0, False)]]

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        done = 0
        try:
            for mh in (0, 2):
                rows = _stage_rows(ctx, t, mh)
                for terms, ngroup in term_lists:
                    ref = Distinct(rows, terms, ngroup)
                    assert 0 < ref.n < n + 1 and (mh == 0 or ref.n < n) and ref.g < ref.nruns
                    for aggs in agg_lists:
                        _check(ctx, t, ref, terms, aggs, ("layout", dups, mh, ngroup), want_hits=True, min_hits=mh)
                        done += 1
        finally:
            t.free()
        return done
    assert run(0) == 16
    assert run(200) == 16
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) == 16
    t = _probed_table(ctx, S + 1)
    try:
        pt = [(P, 0, False, False), (H, 0, False, False)]
        pa = [(AD, P, 1, True), (MODE, P, 1, True), (CD, K, 0, False), (SD, H, 0, False)]      # (the double payload counts in quarters: its sums are exact)
        for mh in (0, 2):
            rows = _stage_rows(ctx, t, mh)
            _check(ctx, t, Distinct(rows, pt, 1), pt, pa, ("probed", mh), want_hits=True, min_hits=mh)
            _check(ctx, t, Distinct(rows, pt, 0), pt, pa[::-1], ("probed", mh, "one group"), want_hits=True, min_hits=mh)
    finally:
        t.free()


def test_eight_terms_seven_of_them_grouping(hip_engine):
    ctx = hip_engine.ctx
    T, _, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(8)
    pos = np.arange(n, dtype=np.int64)
    divs = [T + 37, 300, 130, 67, 31, 9, 4, 2]                              # term i = position // divs[i]: nested divisions
    assert abi.SORT_MAX_KEYS == len(divs) and n // 2 < 1024
    mix = rng.permutation(n)
    hi, lo = np.zeros(n, np.int64), np.zeros(n, np.int64)                   # payload 0 .. 1 carry the eight digits (10 bits each: five in one word, three in the other)
    for d in divs[:5]:
        hi = hi * 1024 + (pos // d) % 1024
    for d in divs[5:]:
        lo = lo * 1024 + (pos // d) % 1024
    t = _range_table(ctx, hi[mix], lo[mix], rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64)[mix], rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)[mix])
    terms = [(P, 0, False, False, 1024 ** (4 - i), 1024, 0, None) for i in range(5)] + [(P, 1, bool(i & 1), False, 1024 ** (2 - i), 1024, 0, None) for i in range(3)]
    try:
        rows = _stage_rows(ctx, t, 0)
        aggs = [(SD, P, 3, False), (MODE, P, 3, False), (AD, P, 2, True), (CD, K, 0, False)]
        for ngroup in (7, 4, 0):
            ref = Distinct(rows, terms, ngroup)
            got = _check(ctx, t, ref, terms, aggs, ("eight terms", ngroup))
            assert ngroup != 7 or set(got[4][3].tolist()) == {1, 2}
    finally:
        t.free()


# 5. text -------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, t, terms, ngroup, aggs, limit, capacity, keys=None, out=None, nterms=None, naggs=None, no_aggs=False):
    arr = (abi.GroupAgg * max(1, len(aggs)))()
    for i, (op, kind, index, is_f64) in enumerate(aggs):
        arr[i].op, arr[i].kind, arr[i].index, arr[i].is_f64 = op, kind, index, int(is_f64)
    got = C.c_int64(-7)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = ctx.lib.sdqh_table_group_distinct(ctx.handle, t.handle, C.c_int64(0), C.c_int(len(terms) if nterms is None else nterms), abi._marshal_sort_terms(terms),
                                           C.c_int(ngroup), C.c_int(len(aggs) if naggs is None else naggs), None if no_aggs else arr, C.c_int64(limit), C.c_int64(capacity),
                                           ptr(keys), None, None, None, ptr(out), C.byref(got))
    return rc, got.value


def test_a_text_value_behind_its_ranks(hip_engine):
    """COUNT(DISTINCT text) and the MODE of a text per high half of a packed key: the text lies behind a payload of row references
    (its ranks column) — two references to the same text are one value, and MODE returns the reference of the run's first row; a
    ranks column too short for the references is the error of sdqh_table_window."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    short = ctx.upload(want[:20])
    try:
        for n in (T + 1, S + 1):
            a = rng.integers(0, n // 90 + 2, n).astype(np.int64)
            b = rng.integers(0, 40, n).astype(np.int64)
            keys = np.unique((a << 32) | b)
            keys = keys[rng.permutation(len(keys))]
            ref_col = rng.integers(0, len(text), len(keys)).astype(np.int64)
            t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ref_col), ctx.upload(ref_col * 3)], accumulate=False)
            try:
                terms = [(K, 0, False, False, 1 << 32, 0, 0, None), (P, 0, True, False, 0, 0, 0, ct)]
                ref = Distinct(_stage_rows(ctx, t, 0), terms, 1, {id(ct): want})
                assert ref.n == len(keys) and ref.g < ref.nruns < ref.n and ref.nruns <= ref.g * len(words)
                aggs = [(CD, K, 0, False), (MODE, P, 0, False), (MC, K, 0, False), (SD, P, 1, False)]
                got = _check(ctx, t, ref, terms, aggs, ("text", n))
                assert (text[got[4][1]] == text[ref.value(aggs[1])]).all() and got[4][0].max() <= len(words)
                bad = [terms[0], (P, 0, True, False, 0, 0, 0, short)]
                keys_out, out = np.full(len(keys), -7, np.int64), np.full(4 * len(keys), -7, np.int64)
                assert _raw(ctx, t, bad, 1, aggs, ALL, len(keys), keys_out, out) == (abi.ERR_INVALID, -7)
                assert (keys_out == -7).all() and (out == -7).all()
                assert b"term 1" in ctx.lib.sdqh_last_error(ctx.handle)
                _check(ctx, t, ref, terms, aggs, ("text", n, "usable after the error"))
            finally:
                t.free()
    finally:
        ct.free(); short.free()


# 6. the contract -----------------------------------------------------------------------------------------------------------------------------
def test_sizes_errors_and_empties(hip_engine):
    ctx = hip_engine.ctx
    T, _, _ = _sizes(ctx)
    n = T + 9
    pos = np.arange(n, dtype=np.int64)
    t = _range_table(ctx, (pos // 100) * PACK + pos // 10, pos // 2, pos.astype(np.float64), pos)
    empty = _range_table(ctx, pos[:0], pos[:0], pos[:0].astype(np.float64), pos[:0])
    terms = _terms(False)
    try:
        ref = Distinct(_stage_rows(ctx, t, 0), terms, 2)
        g = ref.g
        aggs = [(SD, P, 3, False)]
        keys, out = np.full(g, -7, np.int64), np.full(g, -7, np.int64)
        assert _raw(ctx, t, terms, 2, aggs, ALL, g - 1, keys, out) == (abi.ERR_OVERFLOW, g)
        assert (keys == -7).all() and (out == -7).all()
        assert _raw(ctx, t, terms, 2, aggs, 5, g, keys, out) == (abi.OK, 5) and (keys[5:] == -7).all() and (out[5:] == -7).all()      # the tail is untouched
        assert (out[:5] == ref.value(aggs[0])[:5]).all() and (keys[:5] == ref.rows[0][ref.order[ref.gstart[:5]]]).all()
        assert _raw(ctx, t, terms, 2, aggs, ALL, 0) == (abi.OK, g)                                    # count only
        assert _raw(ctx, t, terms, 1, aggs, ALL, 0) == (abi.OK, Distinct(ref.rows, terms, 1).g)
        keys[:] = -7
        assert _raw(ctx, t, terms, 2, aggs, ALL, g, keys, None) == (abi.OK, g) and (keys == ref.rows[0][ref.order[ref.gstart]]).all()      # rows only
        keys[:], out[:] = -7, -7
        assert _raw(ctx, t, terms, 2, aggs, ALL, g, None, out) == (abi.OK, g) and (out == ref.value(aggs[0])).all()      # aggregates only
        assert _raw(ctx, empty, terms, 2, aggs, ALL, 4, keys, out) == (abi.OK, 0)
        assert _raw(ctx, empty, terms, 0, aggs, ALL, 0) == (abi.OK, 0)                                # no group of nothing
        for bad in (dict(aggs=[(6, P, 3, False)]), dict(aggs=[(-1, P, 3, False)]), dict(aggs=[(SD, P, 9, False)]), dict(aggs=[(MODE, V, 0, True)]), dict(aggs=[(SD, K, 0, True)]),
                    dict(aggs=[(AD, H, 0, True)]), dict(aggs=[(SD, H, 0, False)]), dict(naggs=-1), dict(naggs=0), dict(naggs=5), dict(no_aggs=True), dict(ngroup=-1), dict(ngroup=3),
                    dict(ngroup=4), dict(nterms=0), dict(nterms=9), dict(limit=0), dict(capacity=-1)):
            args = dict(ngroup=2, aggs=aggs, limit=ALL, capacity=g, nterms=None, naggs=None, no_aggs=False)
            args.update(bad)
            keys[:], out[:] = -7, -7
            rc = _raw(ctx, t, terms, args["ngroup"], args["aggs"], args["limit"], args["capacity"], keys, out, nterms=args["nterms"], naggs=args["naggs"], no_aggs=args["no_aggs"])
            assert rc == (abi.ERR_INVALID, -7), (bad, rc)
            assert (keys == -7).all() and (out == -7).all(), bad
        _check(ctx, t, ref, terms, aggs, "usable after the errors")
    finally:
        t.free()
        empty.free()


# 7. through the engine and the decorator ---------------------------------------------------------------------------------------------------
def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator

    def both(run, calls):
        dev = run()
        note = eng.stats()["order_routes"][-1]
        assert note["route"] == "group_distinct" and note["calls"] == calls, note
        monkeypatch.setattr(eng, "device_group_distinct", False)
        host = run()
        assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["calls"] == 0
        monkeypatch.setattr(eng, "device_group_distinct", True)
        assert dev.columns == host.columns and len(dev) == len(host) > 0
        for c in dev.columns:                                               # column by column: integers and text as they are, doubles by bits
            a, b = np.asarray(dev.column(c)), np.asarray(host.column(c))
            assert a.dtype == b.dtype, c
            assert (_bits(a) == _bits(b)).all() if a.dtype.kind == "f" else (a == b).all(), c
        return dev, host, note
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by = ["o_shippriority"]
    aggs = {"days": ("count_distinct", "o_orderdate"), "busiest": ("mode", "o_orderdate"), "that_day": ("mode_count", "o_orderdate"), "orders": ("count", None)}
    dev, host, note = both(lambda: Q.q3.distincts(by, aggs)(*args), 1)
    assert note["per"] == by and note["order"] == ["o_orderdate"] and note["aggs"] == [[k] + list(v) for k, v in aggs.items()]
    assert dev.columns == by + list(aggs)
    everything = Q.q3.order_by([("o_orderdate", "asc")])(*args)
    dates = np.asarray(everything.column("o_orderdate"))
    assert int(np.asarray(dev.column("orders")).sum()) == len(dates) and int(np.asarray(dev.column("days")).sum()) >= len(np.unique(dates))
    assert (np.asarray(dev.column("that_day")) <= np.asarray(dev.column("orders"))).all() and np.isin(np.asarray(dev.column("busiest")), dates).all()
    # a text value column is counted through its ranks; an integer-valued sum comes back as the integers it is: three value columns, three calls
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    aggs16 = {"types": ("count_distinct", "p_type"), "usual_size": ("mode", "p_size"), "suppliers": ("sum_distinct", "supplier_cnt")}
    dev, host, note = both(lambda: Q.q16.distincts(["p_brand"], aggs16)(*args16), 3)
    assert note["per"] == ["p_brand"] and note["order"] == ["p_type", "p_size", "supplier_cnt"] and dev.columns == ["p_brand"] + list(aggs16)
    assert np.asarray(dev.column("p_brand")).dtype.kind == "U" and len(np.unique(np.asarray(dev.column("p_brand")))) == len(dev) > 3
    # more than four aggregates over one value column: on the host
    five = {"a": ("count_distinct", "o_orderdate"), "b": ("mode", "o_orderdate"), "c": ("mode_count", "o_orderdate"), "d": ("sum_distinct", "o_orderdate"),
            "e": ("avg_distinct", "o_orderdate")}
    wide = Q.q3.distincts(by, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == by + list(five)
    Q.q3.top(10, [("revenue", "desc")])(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]
