"""The test's own half of the tests past 256 tiles (test_group_large_gpu, test_window_large_gpu's exclusions), without a GPU.  There is
no CPU implementation of sdqh_table_grouping_sets, _group_distinct, _group_moments and _window_exclude, so what can be checked here is
that the patterns are what the GPU tests say they are: each one is built as the (keys, payload, values, hits) tuple that _stage_rows
returns, the sibling files' reference classes run on it at 2 W T + T + 1 = 262 657 rows with T = 512, and every structural claim is
asserted — the seam rule per fold array, the level counts of "halving", per >= 2 for every fold array, the 2^53 cap of the moments'
data, the mode ties either side of a seam, the pieces an exclusion leaves.  The GPU tests assert the same claims, through the same
checkers (large_patterns), on the device's rows.

Each test prints the CPU time of its reference (pytest -s); the figures stand in the docstrings of the GPU files."""
import time

import numpy as np
import pytest

import large_patterns as LP
from sdqlpy_amd import abi
from test_group_distinct_gpu import COMBOS as GD_COMBOS, Distinct
from test_group_moments_gpu import MX, MY, _exact_columns, _sorted_measure, _terms as _mo_terms
from test_grouping_sets_gpu import COMBOS, I_MAX, I_MIN, PACK, Grouped, _terms
from test_window_exclude_gpu import Excluded, _col_lists, _frames
from test_window_large_gpu import FULL, PATTERNS, SWALLOW, W, _exclude_reach, _geometry, _large_pattern, _ranged_columns, _rows_of, _structure
from test_window_gpu import Ranked

T = 512
N = 2 * W * T + T + 1
KX, KY = 123456789, -(1 << 29) + 12345


def test_sizes():
    assert W * T == 131072 and [_rows_of(s, T) for s in FULL] == [131073, N] and N == 262657
    assert [_geometry(_rows_of(s, T), T)[:2] for s in FULL] == [(257, 2), (514, 3)] and all(LP.ragged(_rows_of(s, T), T) for s in FULL)


def test_the_seam_rule_notices():
    """the checker fails on head flags that miss one part of the rule"""
    good = LP.seam_heads(N, T, [3, 1, 5, 2])
    assert LP.seam_rule(good, T, "good") == LP.seam_counts(good, T)
    L = _geometry(N, T)[1] * T
    at = 17 * L + 3
    spoils = [(True, lambda f: (f.__setitem__(slice(14 * L, at, 7), True), f.__setitem__(slice(6 * L, 8 * L, 7), True))),      # no two whole thread runs without a head
              (False, lambda f: f.__setitem__([L, 2 * L, 3 * L], False)),                       # no head on a seam
              (False, lambda f: f.__setitem__([8 * L + 1, 9 * L + 1], False)),                  # none one after
              (False, lambda f: f.__setitem__([5 * L - 1, 6 * L - 1], False)),                  # none one before
              (False, lambda f: f.__setitem__([12 * L - 5, 13 * L - 5, 14 * L - 5, 4 * L + 7, 5 * L + 7], [False] * 3 + [True] * 2))]
    for dense_tail, spoil in spoils:                                        # (the last: no thread run whose only head lies in its last tile)
        bad = good.copy()
        if not dense_tail:
            bad[at + 1:] = False                                            # one group to the end: no head meets a seam by chance
        LP.seam_rule(bad, T, "still good")
        spoil(bad)
        with pytest.raises(AssertionError):
            LP.seam_rule(bad, T, "bad")
    short = LP.cyc_heads(W * T, [3])
    with pytest.raises(AssertionError):
        LP.seam_rule(short, T, "per = 1")


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", LP.GROUPING)
def test_grouping_patterns(pattern, size):
    n = _rows_of(size, T)
    rng = np.random.default_rng(LP.GROUPING.index(pattern) * 1000003 + n)
    cols, ends = LP.grouping_columns(pattern, n, T, size == FULL[1], rng, I_MIN, I_MAX, PACK)
    t0 = time.perf_counter()
    ref = Grouped(LP.synthetic_rows(cols), _terms(size == FULL[1]))
    t1 = time.perf_counter()
    ruled = LP.grouping_claims(pattern, ref, T)
    if n == N:
        assert ruled == {LP.ROW_SEAMS: [("rows", 2, N)], LP.GROUP_SEAMS: [(3, 2, N), (2, 1, len(ref.starts[2]))]}.get(pattern, [])
    for mask in (0b1111, 0b1011, 0b0101, 0b1000, 0b0001):
        for agg in COMBOS[:4]:
            assert len(ref.column(mask, agg)) == ref.level_rows(mask).sum()
    print("PRINTED grouping sets %r n=%d: Grouped %.2f s, 20 columns %.2f s" % (pattern, n, t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", LP.DISTINCT)
def test_distinct_patterns(pattern, size):
    n = _rows_of(size, T)
    rng = np.random.default_rng(LP.DISTINCT.index(pattern) * 1000003 + n)
    cols = LP.distinct_columns(pattern, n, T, size == FULL[0], rng, I_MIN, I_MAX, PACK)
    t0 = time.perf_counter()
    ref = Distinct(LP.synthetic_rows(cols), _terms(size == FULL[0]), 2)
    t1 = time.perf_counter()
    LP.distinct_claims(pattern, ref, T)
    for agg in GD_COMBOS:
        assert len(ref.value(agg)) == ref.g
    print("PRINTED group distinct %r n=%d: Distinct %.2f s, 18 columns %.2f s" % (pattern, n, t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", LP.MOMENTS)
def test_moments_patterns(pattern, size):
    n = _rows_of(size, T)
    rng = np.random.default_rng(LP.MOMENTS.index(pattern) * 1000003 + n)
    assert LP.moments_cap(n) < 1 << 53
    cols = LP.moments_columns(pattern, n, T, size == FULL[1], rng, PACK, KX, KY)
    t0 = time.perf_counter()
    g = Grouped(LP.synthetic_rows(cols), _mo_terms(size == FULL[1]))
    LP.moments_claims(pattern, g, T)
    xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
    assert np.abs(xs - KX).max() < LP.DEV and np.abs(ys - KY).max() < LP.DEV
    for L in (2, 1, 0):                                                     # (_exact_columns asserts the centre to be every group's mean and Q, |C| < 2^53)
        _, (qx, qy, c, m) = _exact_columns(g, L, xs, ys, KX, KY)
        assert max(qx.max(), qy.max(), np.abs(c).max()) <= LP.moments_cap(n)
    print("PRINTED group moments %r n=%d: Grouped and three levels of exact columns %.2f s" % (pattern, n, time.perf_counter() - t0))


def test_every_fold_array_is_reached_with_per_2():
    """over the patterns at 262 657 rows: the rows, the group arrays of the levels 3 and 2, and the value runs obey the whole seam rule
    somewhere, with per >= 2; a ragged last thread at one of the two sizes each"""
    ref = Grouped(LP.synthetic_rows(LP.grouping_columns(LP.GROUP_SEAMS, N, T, False, np.random.default_rng(1), I_MIN, I_MAX, PACK)[0]), _terms(False))
    ruled = LP.grouping_claims(LP.GROUP_SEAMS, ref, T)
    assert [(f, to, _geometry(m, T)[1]) for f, to, m in ruled] == [(3, 2, 3), (2, 1, 2)] and all(LP.ragged(m, T) for _, _, m in ruled)
    rows = Grouped(LP.synthetic_rows(LP.grouping_columns(LP.ROW_SEAMS, N, T, False, np.random.default_rng(1), I_MIN, I_MAX, PACK)[0]), _terms(False))
    assert LP.grouping_claims(LP.ROW_SEAMS, rows, T) == [("rows", 2, N)] and LP.ragged(N, T)
    runs = Distinct(LP.synthetic_rows(LP.distinct_columns(LP.RUN_SEAMS, N, T, False, np.random.default_rng(1), I_MIN, I_MAX, PACK)), _terms(False), 2)
    LP.distinct_claims(LP.RUN_SEAMS, runs, T)
    assert W * T < runs.nruns < N and LP.ragged(runs.nruns, T)


# ---- the exclusions of test_window_large_gpu ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_exclude_patterns(pattern, size):
    n = _rows_of(size, T)
    rng = np.random.default_rng(PATTERNS.index(pattern) * 1000003 + n)
    part, value, hits = _large_pattern(pattern, n, T, rng)
    order, desc, dbls, ints = _ranged_columns(pattern, part, value, rng)
    rows = LP.synthetic_rows([part, order, dbls, ints])
    terms = [(abi.SORT_PAYLOAD, 0, False, False), (abi.SORT_PAYLOAD, 1, desc, False)]
    _structure(pattern, Ranked(rows, terms, 1), T)
    t0 = time.perf_counter()
    ref = Excluded(rows, terms, 1)
    lists = _col_lists(_frames(n, T), PATTERNS.index(pattern))
    for cols in lists:
        for col in cols:
            assert len(ref.want_col(col)) == n
    took = time.perf_counter() - t0
    if pattern == SWALLOW:
        _exclude_reach(ref, T)
    print("PRINTED exclusions %r n=%d: Excluded and its 24 columns %.2f s" % (pattern, n, took))
