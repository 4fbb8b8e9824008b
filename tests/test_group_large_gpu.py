"""The grouping extensions past 256 tiles on the MI355X (run with -m gpu): sdqh_table_grouping_sets, sdqh_table_group_distinct and
sdqh_table_group_moments against numpy at the sizes at which a thread of the one-workgroup scans (k_wagg_scan over the tile carries,
k_sort_bins over the heads per tile) folds MORE THAN ONE tile.  Their own files stop at 65 537 rows (4 098 for the moments), where
per = ceil(tiles / W) = 1, every thread's loop runs at most once and its carry-in is the identity; test_window_large_gpu covers the
window entry points there, and this file what those do not reach by reuse:

    the folds over GROUP arrays: a lower level of the grouping sets is folded over the groups of the level above it, with a tile count
        of its own, and the distinct aggregates' upper stage over the value runs — per >= 2 there only when that array is itself longer
        than W T = 131 072;
    the per-level tile offsets (k_sort_bins over tcount[L * ntiles + tile]) from which k_gs_run, k_gd_heads, k_mo_stage and k_mo_center
        derive a group's slot: a wrong offset behind one seam moves every later group;
    the moments' two rounds over the rows per level, between which every row reads its group's representative and mean.

    rows          tiles  per  runs at
    W T + 1       257    2    everything (a ragged last thread: thread 128 holds one tile)
    2 W T + T + 1 514    3    everything (per does not divide the tiles)
    W T - 1, W T, 2 W T, 2 W T + 1   one call of four columns per entry point, on one pattern

The patterns and the checkers of their structural claims live in large_patterns (test_large_patterns_cpu asserts the same claims on
synthetic rows, without a GPU); every claim is asserted here on the reference built from the DEVICE's staged rows.  The references are the
sibling files' whole-array numpy classes (Grouped, Distinct, _exact_columns, moments_reference); nothing loops over rows or groups in
Python but explicit samples of at most some forty groups.  Integer-valued doubles below 2^30 make every sum exact: bit for bit.

CPU time of the references at 262 657 rows on one core without a GPU (test_large_patterns_cpu prints them): Grouped 0.06 s and the 20
columns of five masks 0.08 s ("every row alone", the slowest); Distinct 0.05 s and its 18 columns 0.01 s; the moments' Grouped and the
_exact_columns of three levels 0.08 s ("groups of 2", the slowest); the general doubles' exact rationals 0.15 s for the nine ops of the
group of 4 685 rows — once per call and level, 12 times in all — and 0.01 s for a group of 300 rows."""
import numpy as np
import pytest

import large_patterns as LP
import moments_reference as mref
from sdqlpy_amd import abi
from sdqlpy_amd.result import MOMENT_OPS
from test_group_distinct_gpu import COMBOS as GD_COMBOS, Distinct, _check as _check_distinct
from test_group_moments_gpu import BI, MX, MY, UNI, _agg, _check_exact_levels, _level_slices, _mo_table, _sorted_measure, _terms as _mo_terms
from test_grouping_sets_gpu import COMBOS, COUNT, I_MAX, I_MIN, PACK, Grouped, _bits, _check, _terms
from test_window_gpu import _same, _stage_rows, hip_engine      # noqa: F401 (fixture)
from test_window_large_gpu import FULL, LIGHT, SWALLOW, W, _geometry, _rows_of
from test_window_range_gpu import _range_table

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P = abi.SORT_KEY, abi.SORT_PAYLOAD
MASKS = (0b1111, 0b1011, 0b0101, 0b1000, 0b0001)                           # in 0b1011 level 1 is folded straight from level 3's groups
MO_MASKS = (0b111, 0b100, 0b001, 0b101)
KX, KY = 123456789, -(1 << 29) + 12345


def _T(ctx):
    T = ctx.window_geometry()
    assert T == ctx.grouping_sets_geometry() == ctx.group_distinct_geometry() == ctx.group_moments_geometry() == ctx.window_exclude_geometry()[0]
    return T


def test_geometry(hip_engine):
    T = _T(hip_engine.ctx)
    assert T == 512 and [_geometry(_rows_of(s, T), T)[:2] for s in FULL] == [(257, 2), (514, 3)] and all(LP.ragged(_rows_of(s, T), T) for s in FULL)
    assert [_geometry(_rows_of(s, T), T)[1] for s in LIGHT] == [1, 1, 2, 3]


def _first_bad(got, want, T, what):
    """bit for bit; the message names the first differing slot, its tile, its thread run (seam) of the array it lies in"""
    same = _bits(got) == _bits(want)
    if not same.all():
        j = int(np.argmin(same))
        per = _geometry(len(want), T)[1]
        raise AssertionError((what, "slot", j, "tile", j // T, "thread run", j // (per * T), "at", j % (per * T), got[j:j + 3], want[j:j + 3]))


# 1. grouping sets -------------------------------------------------------------------------------------------------------------------------
def _grouping_calls(ctx, t, ref, terms, n, T, what, masks, shift):
    for k, mask in enumerate(masks):
        at = (shift * 5 + k) * 4
        aggs = [COMBOS[(at + j) % len(COMBOS)] for j in range(4)] if k else [(COUNT, K, 0, False)] + [COMBOS[(at + j) % len(COMBOS)] for j in range(3)]
        levels = ref.levels(mask)
        got = ctx.table_grouping_sets(t, 0, terms, mask, aggs, ALL, 64, want_hits=False)
        off = 0
        for L in levels:                                                    # level by level first: the message names the level and the slot in its group array
            m = len(ref.starts[L])
            for a, agg in enumerate(aggs):
                _first_bad(got[4][a][off:off + m], ref.value(L, agg), T, (what, bin(mask), "level", L, agg))
            off += m
        _check(ctx, t, ref, terms, mask, aggs, (what, bin(mask)))           # the sibling's: rows, level_rows, dtypes, every column
        g = int(ref.level_rows(mask).sum())
        count = ctx.table_grouping_sets_count(t, 0, terms, mask)
        assert count[0] == g == len(got[0]) and (count[1] == ref.level_rows(mask)).all(), (what, bin(mask))
        if not k:                                                           # the COUNTs of every level add up to n
            off = 0
            for L in levels:
                m = len(ref.starts[L])
                assert int(got[4][0][off:off + m].sum()) == n, (what, L)
                off += m


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", LP.GROUPING)
def test_grouping_sets(hip_engine, pattern, size):
    """Five masks of four aggregates each, rotating SUM / COUNT / MIN / MAX / AVG over the integer, the double and the key; int64's ends
    on seam positions; rows, level_rows, dtypes, the count-only call, a limit, the COUNTs of every level adding up to n."""
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(size, T)
    desc = size == FULL[1]
    rng = np.random.default_rng(LP.GROUPING.index(pattern) * 1000003 + n)
    cols, ends = LP.grouping_columns(pattern, n, T, desc, rng, I_MIN, I_MAX, PACK)
    t = _range_table(ctx, *cols)
    try:
        terms = _terms(desc)
        ref = Grouped(_stage_rows(ctx, t, 0), terms)
        assert ref.n == n
        LP.grouping_claims(pattern, ref, T)
        if pattern in ("every row alone", "halving", LP.GROUP_SEAMS):       # c = pos: the ends of int64 lie on the seams
            ints = ref.rows[1][3][ref.order]
            assert set(ints[ends].tolist()) == {I_MIN, I_MAX}
        _grouping_calls(ctx, t, ref, terms, n, T, (pattern, n), MASKS, LP.GROUPING.index(pattern) + 5 * FULL.index(size))
        _check(ctx, t, ref, terms, 0b1111, [COMBOS[0], COMBOS[13]], (pattern, n, "limit"), limit=max(1, len(ref.positions(0b1111)) // 2))
    finally:
        t.free()


@pytest.mark.parametrize("size", LIGHT)
def test_grouping_sets_one_call(hip_engine, size):
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(size, T)
    pattern = LP.GROUP_SEAMS if n > W * T else "halving"
    cols, _ = LP.grouping_columns(pattern, n, T, False, np.random.default_rng(n), I_MIN, I_MAX, PACK)
    t = _range_table(ctx, *cols)
    try:
        ref = Grouped(_stage_rows(ctx, t, 0), _terms(False))
        _grouping_calls(ctx, t, ref, _terms(False), n, T, (pattern, n), MASKS[:1], 0)
    finally:
        t.free()


# 2. group distinct ------------------------------------------------------------------------------------------------------------------------
def _distinct_calls(ctx, t, ref, terms, T, what, ncalls):
    seen = set()
    for k in range(ncalls):
        aggs = [GD_COMBOS[(k * 4 + j) % len(GD_COMBOS)] for j in range(4)]
        seen |= set(aggs)
        got = ctx.table_group_distinct(t, 0, terms, ref.ngroup, aggs, ALL, 64, want_hits=False)
        for a, agg in enumerate(aggs):
            _first_bad(got[4][a], ref.value(agg), T, (what, agg))
        _check_distinct(ctx, t, ref, terms, aggs, what)                     # the sibling's: rows, dtypes, every column
        assert ctx.table_group_distinct_count(t, 0, terms, ref.ngroup, aggs) == ref.g == len(got[0]), what
    return seen


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", LP.DISTINCT)
def test_group_distinct(hip_engine, pattern, size):
    """ngroup = 2 of three terms; all six ops over the three measures in five calls of four; a limit."""
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(size, T)
    desc = size == FULL[0]
    rng = np.random.default_rng(LP.DISTINCT.index(pattern) * 1000003 + n)
    t = _range_table(ctx, *LP.distinct_columns(pattern, n, T, desc, rng, I_MIN, I_MAX, PACK))
    try:
        terms = _terms(desc)
        ref = Distinct(_stage_rows(ctx, t, 0), terms, 2)
        assert ref.n == n
        LP.distinct_claims(pattern, ref, T)
        assert _distinct_calls(ctx, t, ref, terms, T, (pattern, n), 5) == set(GD_COMBOS)
        if ref.g > 1:
            _check_distinct(ctx, t, ref, terms, [GD_COMBOS[3], GD_COMBOS[10], GD_COMBOS[13]], (pattern, n, "limit"), limit=ref.g // 2)
    finally:
        t.free()


@pytest.mark.parametrize("size", LIGHT)
def test_group_distinct_one_call(hip_engine, size):
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(size, T)
    t = _range_table(ctx, *LP.distinct_columns(LP.MODE_TIES, n, T, False, np.random.default_rng(n), I_MIN, I_MAX, PACK))
    try:
        ref = Distinct(_stage_rows(ctx, t, 0), _terms(False), 2)
        _check_distinct(ctx, t, ref, _terms(False), [GD_COMBOS[9], GD_COMBOS[4], GD_COMBOS[12], GD_COMBOS[15]], (LP.MODE_TIES, n))      # MODE, SUM_DISTINCT, MODE_COUNT, COUNT
    finally:
        t.free()


def test_distinct_count_is_grouping_sets_count(hip_engine):
    """test_group_distinct_gpu's consistency at 262 657 rows, group seams in run space: for ngroup = 2 COUNT is grouping sets' COUNT at
    level 2, COUNT_DISTINCT the number of level-3 groups inside each, MODE_COUNT the largest of their COUNTs."""
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(FULL[1], T)
    t = _range_table(ctx, *LP.distinct_columns(LP.RUN_SEAMS, n, T, False, np.random.default_rng(n), I_MIN, I_MAX, PACK))
    try:
        terms = _terms(False)
        CD, MC, CNT = abi.GD_COUNT_DISTINCT, abi.GD_MODE_COUNT, abi.GD_COUNT
        count, distinct, most = ctx.table_group_distinct(t, 0, terms, 2, [(CNT, K, 0, False), (CD, K, 0, False), (MC, K, 0, False)], ALL, 64, want_hits=False)[4]
        gs = ctx.table_grouping_sets(t, 0, terms, 0b1100, [(COUNT, K, 0, False)], ALL, 64, want_hits=False)
        nruns, ngroups = int(gs[5][3]), int(gs[5][2])
        run_rows, group_rows = gs[4][0][:nruns], gs[4][0][nruns:]
        assert nruns > W * T and ngroups == len(count) and (_bits(count) == _bits(group_rows)).all()
        last_run = np.searchsorted(np.cumsum(run_rows), np.cumsum(group_rows))
        runs_in = np.diff(np.concatenate([[-1], last_run]))
        first_run = last_run - runs_in + 1
        assert (distinct == runs_in).all() and int(distinct.sum()) == nruns and int(count.sum()) == n
        assert (count == np.add.reduceat(run_rows, first_run)).all() and (most == np.maximum.reduceat(run_rows, first_run)).all()
    finally:
        t.free()


# 3. group moments -------------------------------------------------------------------------------------------------------------------------
AGGS_A = [_agg("var_pop", MY), _agg("var_samp", MY), _agg("stddev_pop", MY), _agg("stddev_samp", MY)]
AGGS_B = [_agg("covar_pop", MY, MX), _agg("covar_samp", MY, MX), _agg("regr_slope", MY, MX), _agg("corr", MY, MX)]
AGGS_C = [_agg("regr_intercept", MY, MX), _agg("var_pop", MX), _agg("covar_pop", MX, MX), _agg("corr", MX, MY)]


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", LP.MOMENTS)
def test_group_moments_exact_by_bits(hip_engine, pattern, size):
    """x = KX + d, y = KY + d' with integers |d|, |d'| < 2^16 whose sum over every finest group is 0: every group's mean is the centre,
    and every Q and C is an integer below 262 657 * 2^32 < 2^51 (_exact_columns asserts < 2^53), so pass 2 is exact in any association.
    Pass 1 is exact too: the rows are summed as x - x_r with x_r the group's representative, |x - x_r| < 2^17, so the partial sums are
    integers below 262 657 * 2^17 < 2^35, and S / m — S the group's sum of x - x_r, an integer multiple of m because the mean is the
    centre — is an integer: the mean comes out as the centre, bit for bit.  The sibling's assertions (_check_exact_levels)."""
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(size, T)
    desc = size == FULL[1]
    rng = np.random.default_rng(LP.MOMENTS.index(pattern) * 1000003 + n)
    LP.moments_cap(n)
    t = _mo_table(ctx, *LP.moments_columns(pattern, n, T, desc, rng, PACK, KX, KY))
    try:
        terms = _mo_terms(desc)
        g = Grouped(_stage_rows(ctx, t, 0), terms)
        assert g.n == n
        LP.moments_claims(pattern, g, T)
        xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
        assert np.abs(xs - KX).max() < LP.DEV and np.abs(ys - KY).max() < LP.DEV
        for mask in MO_MASKS:
            what = (pattern, n, bin(mask))
            got = {}
            for aggs in (AGGS_A, AGGS_B, AGGS_C):
                r = ctx.table_group_moments(t, 0, terms, mask, aggs, ALL, 64, want_hits=False)
                _same(r, g.rows, g.order[g.positions(mask)], what)
                assert (r[5] == g.level_rows(mask)).all() and all(c.dtype == np.float64 for c in r[4]), what
                got.update({(MOMENT_OPS[ag[0]], ag[1:]): c for ag, c in zip(aggs, r[4])})
            assert ctx.table_group_moments_count(t, 0, terms, mask, AGGS_A)[0] == len(r[0]), what
            for L, sl in _level_slices(g, mask):                            # first the variance alone: the message names the slot
                st = g.starts[L]
                q = np.add.reduceat(((ys - KY).astype(np.int64)) ** 2, st).astype(np.float64)
                _first_bad(got[("var_pop", MY)][sl], q / g.sizes(L).astype(np.float64), T, (what, "level", L, "var_pop"))
            _check_exact_levels(g, mask, got, xs, ys, KX, KY, what)
    finally:
        t.free()


@pytest.mark.parametrize("size", LIGHT)
def test_group_moments_one_call(hip_engine, size):
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(size, T)
    rng = np.random.default_rng(n)
    t = _mo_table(ctx, *LP.moments_columns(SWALLOW, n, T, False, rng, PACK, KX, KY))
    try:
        g = Grouped(_stage_rows(ctx, t, 0), _mo_terms(False))
        xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
        aggs = [_agg("var_pop", MY), _agg("covar_samp", MY, MX), _agg("regr_slope", MY, MX), _agg("var_samp", MX)]
        r = ctx.table_group_moments(t, 0, _mo_terms(False), 0b111, aggs, ALL, 64, want_hits=False)
        _same(r, g.rows, g.order[g.positions(0b111)], (SWALLOW, n))
        for L, sl in _level_slices(g, 0b111):
            st, m = g.starts[L], g.sizes(L).astype(np.float64)
            dx, dy = (xs - KX).astype(np.int64), (ys - KY).astype(np.int64)
            qx, qy, c = (np.add.reduceat(u, st).astype(np.float64) for u in (dx * dx, dy * dy, dx * dy))
            nan = np.array([mref.NULL_BITS], np.uint64).view(np.float64)[0]
            with np.errstate(all="ignore"):
                want = [qy / m, np.where(m > 1, c / (m - 1.0), nan), np.where(qx != 0, c / qx, nan), np.where(m > 1, qx / (m - 1.0), nan)]
            for col, w, ag in zip(r[4], want, aggs):
                _first_bad(col[sl], w, T, (SWALLOW, n, "level", L, ag))
    finally:
        t.free()


def _general_groups(n, T):
    """(a, b) by sorted position: one group of three thread runs and 77 rows, off every seam, beside groups of 300 rows (a) cut into
    fifty threes and one of 150 (b), as test_group_moments_gpu's"""
    L = _geometry(n, T)[1] * T
    pos = np.arange(n, dtype=np.int64)
    lead, big = 300 * 2 + 7 * 3, 3 * L + 77                                 # (621: off every tile edge)
    rest = np.maximum(pos - lead - big, 0)
    small_a, small_b = rest // 300, rest // 300 * 100 + np.minimum((rest % 300) // 3, 50)
    front = pos < lead
    a = np.where(front, pos // 300, np.where(pos < lead + big, 3, 4 + small_a))
    b = np.where(front, pos // 3, np.where(pos < lead + big, 300, 400 + small_b))
    return a, a * 0 + b, (lead, big)


def test_group_moments_general_doubles(hip_engine):
    """262 657 rows: one group of 4 685 rows — it swallows two whole thread runs, its sums reach it only through the carries — beside
    groups of 3, 150 and 300 rows, on the sibling's "offset" data (x = 1e6 + N(0, 1), y linear in x plus noise) and on its "wide" data
    (+-10^U(-30, 30)) in the small groups only.  Every op of the big group, and of a stride through the small ones with the last,
    against exact rationals within the header's bound (moments_reference.check); two calls, the same bits.
    PRINTED group moments, large: the worst error / bound — measured on the MI355X: 0.0961."""
    ctx = hip_engine.ctx
    T = _T(ctx)
    n = _rows_of(FULL[1], T)
    rng = np.random.default_rng(n)
    a, b, (lead, big) = _general_groups(n, T)
    in_big = (np.arange(n) >= lead) & (np.arange(n) < lead + big)
    terms = _mo_terms(False)
    worst = 0.0
    x_off = 1e6 + rng.standard_normal(n)
    y_off = -3e6 + 2.0 * (x_off - 1e6) + 0.01 * rng.standard_normal(n)
    wide = lambda: rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)      # noqa: E731
    for kind, x, y in (("offset", x_off, y_off), ("wide", np.where(in_big, x_off, wide()), np.where(in_big, y_off, wide()))):
        mix = rng.permutation(n)
        t = _mo_table(ctx, (a * PACK + b)[mix], x[mix], y[mix], mix)
        try:
            g = Grouped(_stage_rows(ctx, t, 0), terms)
            xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
            sizes = g.sizes(2)
            j_big = int(np.argmax(sizes))
            assert sizes[j_big] == big >= 3 * _geometry(n, T)[1] * T and g.starts[2][j_big] == lead and lead % T != 0 and g.sizes(1).max() == big
            assert LP.seam_counts(g.heads[2], T)[3] >= 2 and LP.seam_counts(g.heads[1], T)[3] >= 2      # two whole thread runs inside it
            assert np.sort(sizes)[-2] == 150 and (sizes == 3).sum() > 40000 and np.sort(g.sizes(1))[-2] == 300
            for aggs in ([_agg(op, MY) for op in UNI], [_agg(op, MY, MX) for op in BI[:4]], [_agg("regr_intercept", MY, MX), _agg("var_pop", MX)]):
                got = ctx.table_group_moments(t, 0, terms, 0b110, aggs, ALL, 64, want_hits=False)
                again = ctx.table_group_moments(t, 0, terms, 0b110, aggs, ALL, 64, want_hits=False)
                assert all((mref.bits(p) == mref.bits(q)).all() for p, q in zip(got[4], again[4])), kind
                checked = 0
                for L, sl in _level_slices(g, 0b110):
                    st, size = g.starts[L], g.sizes(L)
                    big_j = int(np.argmax(size))
                    for j in sorted(set(range(0, len(st), len(st) // 4 + 1)) | {len(st) - 1, big_j}):
                        rows = slice(st[j], st[j] + size[j])
                        assert size[j] <= 300 or j == big_j
                        of_y, of_x = None, None                             # one Exact per group and measure: the ops of a call share it
                        for ag, col in zip(aggs, got[4]):
                            op = MOMENT_OPS[ag[0]]
                            if ag[1:] == MX:
                                of_x = of_x or mref.Exact(xs[rows])
                                worst = max(worst, mref.check(op, col[sl][j], xs[rows], None, (kind, L, j), exact=of_x))
                            else:
                                of_y = of_y or mref.Exact(ys[rows], xs[rows])
                                worst = max(worst, mref.check(op, col[sl][j], ys[rows], xs[rows] if op in BI else None, (kind, L, j), exact=of_y))
                        checked += 1
                assert checked >= 10
        finally:
            t.free()
    print("PRINTED group moments, large: worst error / bound over the general doubles = %.4f" % worst)
    assert worst < 1.0
