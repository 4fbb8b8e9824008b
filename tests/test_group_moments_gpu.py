"""VAR / STDDEV / COVAR / CORR / REGR per group on the MI355X (run with -m gpu): sdqh_table_group_moments
(include/sdqh_sort_moments.h) by bits on data whose every intermediate is exact, on the header's exact cases, within the header's bounds
against exact rationals (moments_reference) on general doubles, beside a group that overflows, on every table layout and measure
kind, its contract, and through the decorator against the host route.

The expected groups are the table's own rows (sdqh_table_compact) in the order of a stable numpy lexsort (test_grouping_sets_gpu.Grouped),
the expected values numpy over exactly representable integers or fractions.Fraction.  Nothing is imported from the product's fold
code.  PRINTED: every general-doubles test prints its worst error / bound ratio."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import moments_reference as ref
from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import MOMENT_OPS
from test_grouping_sets_gpu import Grouped
from test_window_gpu import _probed_table, _same, _stage_rows, _table, _under, db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
PACK = 1 << 20                                                              # payload 0 of the pattern tables = a * PACK + b
MX, MY, MI = (P, 1, True), (P, 2, True), (P, 3, False)                     # the tables' two double payloads and their integer one
NULL = ref.NULL_BITS
UNI, BI = MOMENT_OPS[:4], MOMENT_OPS[4:]
OP = {name: i for i, name in enumerate(MOMENT_OPS)}


def _terms(desc):
    """(a, b): the two halves of payload 0, derived terms"""
    return [(P, 0, desc, False, PACK, 0, 0, None), (P, 0, desc, False, 1, PACK, 0, None)]


def _mo_table(ctx, ab, x, y, ints, seed=5):
    """entries with payload 0 = ab, payloads 1 / 2 = the bits of the doubles x / y, payload 3 = ints, in the build order given"""
    n = len(ab)
    keys = np.random.default_rng(seed + n).permutation(n).astype(np.int64) * 3 - n
    cols = [np.asarray(ab, np.int64), np.ascontiguousarray(x, np.float64).view(np.int64), np.ascontiguousarray(y, np.float64).view(np.int64), np.asarray(ints, np.int64)]
    return ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(c) for c in cols], accumulate=False)


def _agg(op, y, x=None):
    return (OP[op],) + y + (x if x is not None else ())


def _sizes(ctx):
    T, S = ctx.window_geometry(), ctx.sort_geometry()[0]
    assert ctx.group_moments_geometry() == ctx.grouping_sets_geometry() == T
    return T, S


def _sorted_measure(g, kind, index, is_f64):
    keys, payload, values, hits = g.rows
    src = keys if kind == K else payload[index] if kind == P else values[index] if kind == V else hits
    src = np.ascontiguousarray(src)[g.order]
    return src.view(np.float64) if (is_f64 and src.dtype != np.float64) else src.astype(np.float64)


def _level_slices(g, mask):
    """[(level, the slice of its rows in the output)] from the highest level down"""
    out, at = [], 0
    for L in g.levels(mask):
        out.append((L, slice(at, at + len(g.starts[L]))))
        at += len(g.starts[L])
    return out


# 1. exact by bits -------------------------------------------------------------------------------------------------------------------------
PATTERNS = ["one group", "groups of 2", "a group across the tile edge", "a group over three tiles", "edges"]


def _pattern(name, n, T):
    """(a, b) by sorted position, each non-decreasing: b the finest groups, a groups of those"""
    pos = np.arange(n, dtype=np.int64)
    if name == "one group":
        return pos * 0, pos * 0
    if name == "groups of 2":
        return pos // (T + 38), pos // 2
    if name == "a group across the tile edge":
        b = np.searchsorted(np.array([T - 6, T + 10]), pos, side="right").astype(np.int64) + (pos >= T + 10) * ((pos - T - 10) // 6)
        return (pos >= T + 10).astype(np.int64), b
    if name == "a group over three tiles":
        b = pos // 4
        lo, hi = T - 10, min(n, 3 * T + 6)
        if lo < n:
            b[lo:hi] = b[lo]
        return pos * 0, b
    starts = np.array([63, 64, 65, T - 1, T, T + 1])                       # "edges"
    b = np.searchsorted(starts, pos, side="right").astype(np.int64)
    return b // 3, b


def _symmetric(b, rng, centre, amp=1 << 20):
    """per position centre + d, |d| < amp, with the d of every run of b symmetric about 0: pairs +d, -d (and one 0 in a run of odd length)"""
    n = len(b)
    pos = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = b[1:] != b[:-1]
    start = np.maximum.accumulate(np.where(head, pos, 0))
    size = np.diff(np.append(np.nonzero(head)[0], n))[np.cumsum(head) - 1]
    i = pos - start
    d = rng.integers(-amp + 1, amp, n)
    d = np.where(i & 1, -d[np.maximum(pos - 1, 0)], d)
    d = np.where((size & 1) & (i == size - 1), 0, d)
    return (centre + d).astype(np.float64)


def _exact_columns(g, L, xs, ys, kx, ky):
    """every op's expected column at level L, from integers that doubles hold exactly: {op: float64 array}, and (Qx, Qy, C, m)"""
    st = g.starts[L]
    m = g.sizes(L).astype(np.float64)
    dx, dy = (xs - kx).astype(np.int64), (ys - ky).astype(np.int64)
    assert (np.add.reduceat(dx, st) == 0).all() and (np.add.reduceat(dy, st) == 0).all()      # the centre is every group's mean
    qx, qy, c = (np.add.reduceat(u, st).astype(np.float64) for u in (dx * dx, dy * dy, dx * dy))
    assert max(qx.max(), qy.max(), np.abs(c).max()) < 2.0 ** 53
    nan = np.array([NULL], np.uint64).view(np.float64)[0]
    with np.errstate(all="ignore"):
        samp = lambda q: np.where(m > 1, q / (m - 1.0), nan)              # noqa: E731
        out = {"var_pop": qy / m, "var_samp": samp(qy), "covar_pop": c / m, "covar_samp": samp(c), "regr_slope": np.where(qx != 0, c / qx, nan)}
    return out, (qx, qy, c, m)


def _check_exact_levels(g, mask, got, xs, ys, kx, ky, what):
    """the assertions of test_exact_by_bits on one mask's columns `got` = {(op, measures): column}: bits for VAR_* / COVAR_* / REGR_SLOPE,
    STDDEV within 1 ulp of the square root of the same call's variance, CORR symmetric by bits and |corr| <= 1, NULL where the header
    says so, and CORR / REGR_INTERCEPT of at most 40 groups per level against exact rationals"""
    for L, sl in _level_slices(g, mask):
        want, (qx, qy, c, m) = _exact_columns(g, L, xs, ys, kx, ky)
        for op in ("var_pop", "var_samp"):
            assert (ref.bits(got[(op, MY)][sl]) == ref.bits(want[op])).all(), (what, L, op)
        for op in ("covar_pop", "covar_samp", "regr_slope"):
            assert (ref.bits(got[(op, MY + MX)][sl]) == ref.bits(want[op])).all(), (what, L, op)
        assert (ref.bits(got[("var_pop", MX)][sl]) == ref.bits(qx / m)).all() and (ref.bits(got[("covar_pop", MX + MX)][sl]) == ref.bits(qx / m)).all(), (what, L)
        with np.errstate(all="ignore"):
            for op, var in (("stddev_pop", "var_pop"), ("stddev_samp", "var_samp")):      # within 1 ulp of the square root of the same call's variance
                s, v = got[(op, MY)][sl], got[(var, MY)][sl]
                dead = ref.bits(v) == NULL
                assert (ref.bits(s)[dead] == NULL).all() and (np.abs(ref.bits(s)[~dead].astype(np.int64) - ref.bits(np.sqrt(v[~dead])).astype(np.int64)) <= 1).all(), (what, L, op)
            corr, back = got[("corr", MY + MX)][sl], got[("corr", MX + MY)][sl]
            assert (ref.bits(corr) == ref.bits(back)).all(), (what, L, "corr swapped")
            flat = (qx == 0) | (qy == 0)
            assert (ref.bits(corr)[flat] == NULL).all() and (np.abs(corr[~flat]) <= 1.0).all(), (what, L)
            icpt = got[("regr_intercept", MY + MX)][sl]
            assert (ref.bits(icpt)[qx == 0] == NULL).all(), (what, L)
        live = np.nonzero(~flat)[0]
        for j in live[::max(1, len(live) // 40)]:                # a sample against exact rationals: 4 ulp each
            C_, QX, QY = Fraction(int(c[j])), Fraction(int(qx[j])), Fraction(int(qy[j]))
            exact_corr = float(C_) / (np.sqrt(np.float64(qx[j])) * np.sqrt(np.float64(qy[j])))
            assert abs(corr[j] - exact_corr) <= 4 * np.spacing(abs(exact_corr)), (what, L, j, corr[j], exact_corr)
            exact_icpt = Fraction(ky) - C_ / QX * kx
            scale = abs(float(ky)) + abs(float(C_ / QX * kx))
            assert abs(Fraction(float(icpt[j])) - exact_icpt) <= 4 * np.spacing(scale), (what, L, j, icpt[j], float(exact_icpt))
            assert float(Fraction(int(qy[j])) / int(m[j])) == got[("var_pop", MY)][sl][j] and float(C_ / QX) == got[("regr_slope", MY + MX)][sl][j]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_exact_by_bits(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    kx, ky = 123456789, -(1 << 29) + 12345
    aggs_a = [_agg("var_pop", MY), _agg("var_samp", MY), _agg("stddev_pop", MY), _agg("stddev_samp", MY)]
    aggs_b = [_agg("covar_pop", MY, MX), _agg("covar_samp", MY, MX), _agg("regr_slope", MY, MX), _agg("corr", MY, MX)]
    aggs_c = [_agg("regr_intercept", MY, MX), _agg("var_pop", MX), _agg("covar_pop", MX, MX), _agg("corr", MX, MY)]
    for i, n in enumerate((2, 64, 66, T, T + 2, 2 * T + 2, S + 2, 4098)):
        desc = bool(i & 1)
        terms = _terms(desc)
        a, b = _pattern(pattern, n, T)
        x, y = _symmetric(b, rng, kx), _symmetric(b, rng, ky)
        if desc:
            a, b = a.max() - a, b.max() - b
        mix = rng.permutation(n)
        t = _mo_table(ctx, (a * PACK + b)[mix], x[mix], y[mix], mix)
        try:
            g = Grouped(_stage_rows(ctx, t, 0), terms)
            xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
            for mask in (0b100, 0b111, 0b001):
                what = (pattern, n, bin(mask))
                got = {}
                for aggs in (aggs_a, aggs_b, aggs_c):
                    r = ctx.table_group_moments(t, 0, terms, mask, aggs, ALL, 64, want_hits=False)
                    _same(r, g.rows, g.order[g.positions(mask)], what)
                    assert (r[5] == g.level_rows(mask)).all() and all(c.dtype == np.float64 for c in r[4]), what
                    got.update({(MOMENT_OPS[ag[0]], ag[1:]): c for ag, c in zip(aggs, r[4])})
                sib = ctx.table_grouping_sets_count(t, 0, terms, mask)
                mine = ctx.table_group_moments_count(t, 0, terms, mask, aggs_a)
                assert mine[0] == sib[0] == len(r[0]) and (mine[1] == sib[1]).all() and (sib[1] == r[5]).all(), what
                _check_exact_levels(g, mask, got, xs, ys, kx, ky, what)
        finally:
            t.free()
    if pattern == "a group over three tiles":
        assert (g.sizes(2) > 2 * T).any()
    if pattern == "edges":
        assert set(g.starts[2]) == {0, 63, 64, 65, T - 1, T, T + 1}
    if pattern == "a group across the tile edge":
        assert {T - 6, T + 10} <= set(g.starts[2])


# 2. the exact cases -----------------------------------------------------------------------------------------------------------------------
def test_exact_cases(hip_engine):
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    every_y = [[_agg(op, MY) for op in UNI], [_agg(op, MY, MX) for op in BI[:4]], [_agg("regr_intercept", MY, MX), _agg("corr", MX, MY), _agg("regr_slope", MX, MY), _agg("covar_pop", MX, MY)]]

    def run(t, terms, mask):
        out = {}
        for aggs in every_y:
            r = ctx.table_group_moments(t, 0, terms, mask, aggs, ALL, 64, want_hits=False)
            out.update({(MOMENT_OPS[ag[0]], ag[1:]): ref.bits(c) for ag, c in zip(aggs, r[4])})
        return out
    # every row its own group
    n = T + 3
    rng = np.random.default_rng(1)
    pos = np.arange(n, dtype=np.int64)
    t = _mo_table(ctx, pos, rng.standard_normal(n) * 1e5, rng.standard_normal(n), pos)
    try:
        got = run(t, _terms(False), 0b100)
        for (op, _), b in got.items():
            assert (b == (0 if op in ("var_pop", "stddev_pop", "covar_pop") else NULL)).all() and len(b) == n, op
    finally:
        t.free()
    # constant groups of 1, 2, 65 and T + 1 rows of 0.1, of 1e300 and of -0.0: Q = +0.0 by bits, CORR / REGR_* over it NaN
    sizes = [1, 2, 65, T + 1]
    b = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    n = len(b)
    for v in (0.1, 1e300, -0.0):
        mix = rng.permutation(n)
        t = _mo_table(ctx, b[mix], np.arange(n, dtype=np.float64)[mix], np.full(n, v), mix)
        try:
            got = run(t, _terms(False), 0b100)
            one = np.array(sizes) == 1
            for op in ("var_pop", "stddev_pop"):
                assert (got[(op, MY)] == 0).all(), (v, op)
            for op in ("var_samp", "stddev_samp"):
                assert (got[(op, MY)] == np.where(one, NULL, 0)).all(), (v, op)
            assert (got[("covar_pop", MY + MX)] == 0).all() and (got[("covar_pop", MX + MY)] == 0).all() and (got[("covar_samp", MY + MX)] == np.where(one, NULL, 0)).all(), v
            assert (got[("corr", MY + MX)] == NULL).all() and (got[("corr", MX + MY)] == NULL).all() and (got[("regr_slope", MX + MY)] == NULL).all(), v      # Qy = 0
            assert (got[("regr_slope", MY + MX)] == np.where(one, NULL, 0)).all(), v                                                                      # C = 0 over Qx > 0
            icpt = got[("regr_intercept", MY + MX)]
            assert icpt[0] == NULL and (icpt[1:].view(np.float64) == v).all(), v
        finally:
            t.free()
    # symmetry by bits on general doubles, and COVAR_POP(x, x) = VAR_POP(x)
    n = 2 * T + 9
    pos = np.arange(n, dtype=np.int64)
    mix = rng.permutation(n)
    t = _mo_table(ctx, ((pos // 700) * PACK + pos // 11)[mix], 1e6 + rng.standard_normal(n), rng.standard_normal(n) * 1e-3, mix)
    try:
        pairs = [[_agg("covar_pop", MY, MX), _agg("covar_pop", MX, MY), _agg("corr", MY, MX), _agg("corr", MX, MY)],
                 [_agg("covar_samp", MY, MX), _agg("covar_samp", MX, MY), _agg("covar_pop", MX, MX), _agg("var_pop", MX)]]
        for aggs in pairs:
            r = ctx.table_group_moments(t, 0, _terms(True), 0b111, aggs, ALL, 64, want_hits=False)
            assert (ref.bits(r[4][0]) == ref.bits(r[4][1])).all() and (ref.bits(r[4][2]) == ref.bits(r[4][3])).all() and np.isfinite(r[4][2][-1])
    finally:
        t.free()


# 3. general doubles within the bound --------------------------------------------------------------------------------------------------------
def test_general_doubles_within_the_bound(hip_engine):
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    worst = 0.0
    for n in (S + 1, 4097):
        rng = np.random.default_rng(n)
        pos = np.arange(n, dtype=np.int64)
        a, b = pos // 300, pos // 300 * 100 + np.minimum((pos % 300) // 3, 50)     # a: groups of 300; b: fifty threes, then one of 150
        wide = lambda: rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)                               # noqa: E731
        x_off = 1e6 + rng.standard_normal(n)
        for kind, x, y in (("wide", wide(), wide()), ("offset", x_off, -3e6 + 2.0 * (x_off - 1e6) + 0.01 * rng.standard_normal(n))):
            mix = rng.permutation(n)
            t = _mo_table(ctx, (a * PACK + b)[mix], x[mix], y[mix], mix)
            terms = _terms(False)
            try:
                g = Grouped(_stage_rows(ctx, t, 0), terms)
                xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
                assert (g.sizes(2) <= 4).any() and (g.sizes(2) >= 100).any() and len(g.starts[0]) == 1
                for aggs in ([_agg(op, MY) for op in UNI], [_agg(op, MY, MX) for op in BI[:4]], [_agg("regr_intercept", MY, MX), _agg("var_pop", MX)]):
                    got = ctx.table_group_moments(t, 0, terms, 0b111, aggs, ALL, 64, want_hits=False)
                    again = ctx.table_group_moments(t, 0, terms, 0b111, aggs, ALL, 64, want_hits=False)
                    assert all((ref.bits(p) == ref.bits(q)).all() for p, q in zip(got[4], again[4])), (n, kind)      # no atomics: the same bits
                    checked = 0
                    for L, sl in _level_slices(g, 0b111):
                        st, size = g.starts[L], g.sizes(L)
                        for j in sorted(set(range(0, len(st), 89)) | {len(st) - 1}):
                            rows = slice(st[j], st[j] + size[j])
                            for ag, col in zip(aggs, got[4]):
                                op = MOMENT_OPS[ag[0]]
                                yy, xx = (xs[rows], None) if ag[1:] == MX else (ys[rows], xs[rows] if op in BI else None)
                                worst = max(worst, ref.check(op, col[sl][j], yy, xx, (n, kind, L, j)))
                            checked += 1
                    assert checked >= 6
            finally:
                t.free()
    print("PRINTED group moments: worst error / bound over the general doubles = %.4f" % worst)
    assert worst < 1.0


# 4. nothing leaks ---------------------------------------------------------------------------------------------------------------------------
def test_nothing_leaks_from_a_group_that_overflows(hip_engine):
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    n = 2 * T + 40
    rng = np.random.default_rng(4)
    pos = np.arange(n, dtype=np.int64)
    b = (pos + 1) // 2                                                       # groups of two: [T - 1, T] is one, across the tile edge
    kx, ky = 1000, -77
    x, y = _symmetric(b, rng, kx), _symmetric(b, rng, ky)
    x[T - 1], x[T] = 1e200, -1e200                                          # its own variance overflows
    mix = rng.permutation(n)
    t = _mo_table(ctx, (b // 300 * PACK + b)[mix], x[mix], y[mix], mix)
    terms = _terms(False)
    try:
        g = Grouped(_stage_rows(ctx, t, 0), terms)
        aggs = [_agg("var_pop", MX), _agg("stddev_samp", MX), _agg("covar_pop", MY, MX), _agg("regr_slope", MY, MX)]
        got = ctx.table_group_moments(t, 0, terms, 0b100, aggs, ALL, 64, want_hits=False)
        big = int(np.nonzero(g.starts[2] == T - 1)[0][0])
        assert g.sizes(2)[big] == 2 and not np.isfinite(got[4][0][big]) and not np.isfinite(got[4][1][big])
        xs, ys = _sorted_measure(g, *MX), _sorted_measure(g, *MY)
        keep = np.ones(len(g.starts[2]), bool)
        keep[big] = False
        xs[[T - 1, T]] = kx                                                  # (the expected columns of the others, over integers)
        want, (qx, qy, c, m) = _exact_columns(g, 2, xs, ys, kx, ky)
        assert (ref.bits(got[4][0])[keep] == ref.bits(qx / m)[keep]).all() and (ref.bits(got[4][2])[keep] == ref.bits(want["covar_pop"])[keep]).all()
        assert (ref.bits(got[4][3])[keep] == ref.bits(want["regr_slope"])[keep]).all()
        for col in got[4]:                                                   # nothing but that group is non-finite, beyond the NULLs of the two groups of one row
            assert (np.isfinite(col[keep]) | (ref.bits(col[keep]) == NULL)).all() and int((~np.isfinite(col[keep])).sum()) <= 2
    finally:
        t.free()


# 5. layouts and measures ------------------------------------------------------------------------------------------------------------------
def _check_measures(ctx, t, terms, mask, measures, min_hits, what):
    """VAR_POP / COVAR_SAMP / CORR / REGR_INTERCEPT over pairs of `measures` against the definition over the converted doubles"""
    g = Grouped(_stage_rows(ctx, t, min_hits), terms)
    assert g.n > 0
    done = 0
    for i, my in enumerate(measures):
        mx = measures[(i + 1) % len(measures)]
        aggs = [_agg("var_pop", my), _agg("covar_samp", my, mx), _agg("corr", my, mx), _agg("regr_intercept", my, mx)]
        got = ctx.table_group_moments(t, min_hits, terms, mask, aggs, ALL, 64, want_hits=True)
        _same(got, g.rows, g.order[g.positions(mask)], what)
        assert (got[5] == g.level_rows(mask)).all(), what
        ys, xs = _sorted_measure(g, *my), _sorted_measure(g, *mx)
        for L, sl in _level_slices(g, mask):
            st, size = g.starts[L], g.sizes(L)
            for j in range(0, len(st), max(1, len(st) // 6)):
                rows = slice(st[j], st[j] + size[j])
                for ag, col in zip(aggs, got[4]):
                    op = MOMENT_OPS[ag[0]]
                    ref.check(op, col[sl][j], ys[rows], xs[rows] if op in BI else None, (what, my, mx, L, j))
                done += 1
    return done


def test_layouts_and_measures(hip_engine):
    """The direct layout, a table with duplicate build keys (owner rows only), the open-addressing layout and the probed table, each
    with min_hits 0 and 2; the measures VALUE, HITS, an integer payload, a double payload and KEY, integers as their converted doubles."""
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(n)
    part = rng.integers(0, 9, n).astype(np.int64)
    value = rng.integers(-50, 50, n).astype(np.float64)
    hits = rng.integers(0, 4, n)
    terms = [(P, 0, True, False)]

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        try:
            return sum(_check_measures(ctx, t, terms, 0b11, [(V, 0, True), (H, 0, False), (K, 0, False)], mh, ("layout", dups, mh)) for mh in (0, 2))
        finally:
            t.free()
    assert run(0) > 10 and run(200) > 10
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) > 10
    t = _probed_table(ctx, S + 1)
    try:
        for mh in (0, 2):
            assert _check_measures(ctx, t, [(P, 0, False, False)], 0b11, [(P, 1, True), (V, 0, True), (H, 0, False), (P, 0, False), (K, 0, False)], mh, ("probed", mh)) > 10
    finally:
        t.free()
    pos = np.arange(200, dtype=np.int64)
    ends = rng.integers(-(1 << 62), 1 << 62, 200)
    ends[[3, 4, 150]] = [abi.INT64_MIN, abi.INT64_MAX, abi.INT64_MAX]
    t = _mo_table(ctx, pos // 7, rng.standard_normal(200), rng.standard_normal(200), ends)
    try:
        assert _check_measures(ctx, t, _terms(False), 0b101, [MI, MX, (K, 0, False)], 0, "int64 ends") > 10
    finally:
        t.free()


# 6. the contract ----------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, t, terms, levels, aggs, limit, capacity, keys=None, out=None, level_rows=None, nterms=None, naggs=None, null_aggs=False):
    got = C.c_int64(-7)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = ctx.lib.sdqh_table_group_moments(ctx.handle, t.handle, C.c_int64(0), C.c_int(len(terms) if nterms is None else nterms), abi._marshal_sort_terms(terms),
                                          C.c_uint32(levels), C.c_int(len(aggs) if naggs is None else naggs), None if null_aggs else abi._marshal_moment_aggs(aggs),
                                          C.c_int64(limit), C.c_int64(capacity), ptr(keys), None, None, None, ptr(out), ptr(level_rows), C.byref(got))
    return rc, got.value


def test_sizes_errors_and_empties(hip_engine):
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    n = T + 9
    pos = np.arange(n, dtype=np.int64)
    t = _mo_table(ctx, (pos // 100) * PACK + pos // 10, pos.astype(np.float64), (pos * pos % 17).astype(np.float64), pos)
    empty = _mo_table(ctx, pos[:0], pos[:0].astype(np.float64), pos[:0].astype(np.float64), pos[:0])
    terms = _terms(False)
    try:
        g = Grouped(_stage_rows(ctx, t, 0), terms)
        total = int(g.level_rows(0b111).sum())
        aggs = [_agg("var_pop", MX), _agg("corr", MY, MX)]
        keys, out, lr = np.full(total, -7, np.int64), np.full((2, total), -7, np.int64), np.full(9, -7, np.int64)
        assert _raw(ctx, t, terms, 0b111, aggs, ALL, total - 1, keys, out, lr) == (abi.ERR_OVERFLOW, total)
        assert (keys == -7).all() and (out == -7).all()
        assert _raw(ctx, t, terms, 0b111, aggs, 5, total, keys, out, lr) == (abi.OK, 5) and (keys[5:] == -7).all() and (out[:, 5:] == -7).all() and (out[:, :5] != -7).all()
        assert (lr == g.level_rows(0b111)).all()
        assert _raw(ctx, t, terms, 0b111, aggs, ALL, 0, None, None, lr) == (abi.OK, total)                                  # count only
        keys[:], out[:] = -7, -7
        assert _raw(ctx, t, terms, 0b110, aggs, ALL, total, keys, None, lr) == (abi.OK, int(g.level_rows(0b110).sum()))      # rows only
        assert (lr == g.level_rows(0b110)).all() and (keys[:int(lr.sum())] == g.rows[0][g.order[g.positions(0b110)]]).all()
        keys[:] = -7
        assert _raw(ctx, t, terms, 0b111, aggs, ALL, total, None, out, lr) == (abi.OK, total) and (out != -7).all()          # aggregates only
        full = ctx.table_group_moments(t, 0, terms, 0b111, aggs, ALL, 64, want_hits=False)
        assert (out[0] == ref.bits(full[4][0]).view(np.int64)).all() and (out[1] == ref.bits(full[4][1]).view(np.int64)).all()
        lr[:] = -7
        assert _raw(ctx, empty, terms, 0b111, aggs, ALL, 4, keys, out, lr) == (abi.OK, 0) and (lr == 0).all()
        x9, k_f, h_f = (P, 9, True), (K, 0, True), (H, 0, True)
        bads = [dict(aggs=[(-1,) + MX]), dict(aggs=[(9,) + MX]), dict(aggs=[_agg("var_pop", x9)]), dict(aggs=[_agg("corr", x9, MX)]), dict(aggs=[_agg("corr", MX, x9)]),
                dict(aggs=[_agg("var_pop", k_f)]), dict(aggs=[_agg("stddev_pop", h_f)]), dict(aggs=[_agg("covar_pop", MX, k_f)]), dict(aggs=[_agg("regr_slope", MX, h_f)]),
                dict(aggs=[_agg("var_pop", (H, 0, False))]),                 # a table without hits has no such field
                dict(naggs=0), dict(naggs=5), dict(null_aggs=True), dict(levels=0), dict(levels=0b1000), dict(nterms=0), dict(nterms=9), dict(limit=0), dict(capacity=-1)]
        for bad in bads:
            args = dict(levels=0b111, aggs=aggs, limit=ALL, capacity=total, nterms=None, naggs=None, null_aggs=False)
            args.update(bad)
            keys[:], out[:], lr[:] = -7, -7, -7
            rc = _raw(ctx, t, terms, args["levels"], args["aggs"], args["limit"], args["capacity"], keys, out, lr, nterms=args["nterms"], naggs=args["naggs"], null_aggs=args["null_aggs"])
            assert rc == (abi.ERR_INVALID, -7), (bad, rc)
            assert (keys == -7).all() and (out == -7).all() and (lr == -7).all(), bad
        again = ctx.table_group_moments(t, 0, terms, 0b111, aggs, ALL, 64, want_hits=False)                                  # usable after the errors
        assert all((ref.bits(p) == ref.bits(q)).all() for p, q in zip(full[4], again[4]))
    finally:
        t.free()
        empty.free()


# 7. through the engine and the decorator --------------------------------------------------------------------------------------------------
def _agree(dev, host, rows, by, aggs, sample=25):
    """the device's and the host's aggregates within the SUM of both sides' bounds, over a sample of groups of the order_by rows"""
    assert dev.columns == host.columns and len(dev) == len(host) > 3
    assert [np.asarray(a).dtype for a in dev.arrays] == [np.asarray(a).dtype for a in host.arrays]
    for c in by + (["grouping"] if "grouping" in dev.columns else []):
        p, q = np.asarray(dev.column(c)), np.asarray(host.column(c))
        assert (p.astype(str) == q.astype(str)).all(), c
    plain = len(dev) if "grouping" not in dev.columns else int((np.asarray(dev.column("grouping")) == 0).sum())
    keys = [np.asarray(rows.column(c)) for c in by]
    out = [np.asarray(dev.column(c)) for c in by]
    picks = sorted(set(range(0, plain, max(1, plain // sample))))
    for j in picks + ([len(dev) - 1] if plain < len(dev) else []):
        member = np.ones(len(rows), bool)
        if j < plain:
            for kcol, ocol in zip(keys, out):
                member &= kcol == ocol[j]
        idx = np.nonzero(member)[0]                                         # (the last row of a rollup is the grand total: every row)
        for name, spec in aggs.items():
            ys = np.asarray(rows.column(spec[1]), np.float64)[idx]
            xs = np.asarray(rows.column(spec[2]), np.float64)[idx] if len(spec) == 3 else None
            want, bound = ref.Exact(ys, xs).value(spec[0])
            d, h = np.float64(dev.column(name)[j]), np.float64(host.column(name)[j])
            if want is None:
                assert int(d.view(np.uint64)) == NULL and int(h.view(np.uint64)) == NULL, (name, j)
            else:
                assert abs(float(d) - float(h)) <= 2 * bound, (name, j, float(d), float(h), want, bound)
                assert abs(float(d) - want) <= bound, (name, j, float(d), want, bound)


def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]

    def both(run, rollup):
        dev = run()
        note = eng.stats()["order_routes"][-1]
        assert note["route"] == "group_moments" and note["calls"] == 1 and note["rollup"] is rollup, note
        monkeypatch.setattr(eng, "device_group_moments", False)
        host = run()
        assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["calls"] == 0
        monkeypatch.setattr(eng, "device_group_moments", True)
        return dev, host
    aggs = {"spread": ("stddev_samp", "revenue"), "var": ("var_pop", "revenue"), "trend": ("regr_slope", "revenue", "l_orderkey"), "flat": ("corr", "revenue", "o_shippriority")}
    rows = Q.q3.order_by([("o_orderdate", "asc")])(*args)
    dev, host = both(lambda: Q.q3.moments(["o_orderdate"], aggs)(*args), False)
    assert dev.columns == ["o_orderdate"] + list(aggs) and all(dev.column(c).dtype == np.float64 for c in aggs)
    _agree(dev, host, rows, ["o_orderdate"], aggs)
    by = ["o_orderdate", "o_shippriority"]
    aggs2 = {"spread": ("stddev_pop", "revenue"), "cov": ("covar_samp", "revenue", "l_orderkey")}
    dev, host = both(lambda: Q.q3.moments(by, aggs2, rollup=True)(*args), True)
    assert dev.columns == by + list(aggs2) + ["grouping"]
    grouping = np.asarray(dev.column("grouping"))
    assert (grouping[:-1] <= grouping[1:]).all() and grouping[-1] == 3 and (grouping == 3).sum() == 1
    _agree(dev, host, rows, by, aggs2)
    # text grouping columns go through their ranks; an integer-valued measure is the doubles the table keeps
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    rows16 = Q.q16.order_by([("p_brand", "asc")])(*args16)
    aggs16 = {"spread": ("stddev_samp", "supplier_cnt"), "var": ("var_pop", "supplier_cnt"), "self": ("covar_pop", "supplier_cnt", "supplier_cnt")}
    dev, host = both(lambda: Q.q16.moments(["p_brand"], aggs16)(*args16), False)
    _agree(dev, host, rows16, ["p_brand"], aggs16)
    # more than four aggregates: on the host
    five = dict(aggs, lo=("var_samp", "revenue"))
    wide = Q.q3.moments(["o_orderdate"], five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == ["o_orderdate"] + list(five)
