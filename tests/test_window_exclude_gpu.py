"""Window frames with rows taken out on the MI355X (run with -m gpu): sdqh_table_window_exclude (include/sdqh_sort_exclude.h) against
numpy at every size at which the sort, the tile passes or the fold tree take another path, in all three units and under all four
exclusions, at offsets around the wave, the tile and the table, on frames that do not hold their own row, on partition patterns that
exercise the carries between tiles — a tie run that spans three tiles, tie runs at a partition's first and last rows —, on values that
would betray a sum-and-subtract, on general doubles against the header's error bound, against sdqh_table_window_range /
sdqh_table_window_slide where they overlap, on every table layout, over derived terms, its limits, empties and argument errors, and
through the engine and the decorator.

The expected rows are the table's own K-F rows reordered by a stable numpy lexsort (test_window_gpu's Ranked, whose tie heads give the
tie runs).  The base frame's ends come from the independent restatements of the sibling tests (test_window_slide_gpu's Slid for ROWS,
test_window_range_gpu's Ranged for VALUE / GROUPS); the pieces are cut here, and their values are computed from prefix sums of
integers (exact mod 2^64) and sparse tables of images.  Nothing is imported from the product's fold code."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from test_window_gpu import PATTERNS, Ranked, _pattern, _probed_table, _same, _sort_bits, _stage_rows, _table, _under, db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)
from test_window_range_gpu import Ranged, _range_table
from test_window_slide_gpu import EMPTIES, QNAN, RUN_TO_RUN, TOP, Slid, _bits, _last_of, _partitions

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
SUM, COUNT, MIN, MAX, FIRST, LAST, AVG = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WSLIDE_FIRST, abi.WSLIDE_LAST, abi.WEX_AVG
OPS = (SUM, COUNT, MIN, MAX, FIRST, LAST, AVG)
VAL, GRP, ROWS = abi.WRANGE_VALUE, abi.WRANGE_GROUPS, abi.WEX_ROWS
UNITS = (VAL, GRP, ROWS)
NO, CUR, GROUP, TIES = abi.WEX_NO_OTHERS, abi.WEX_CURRENT_ROW, abi.WEX_GROUP, abi.WEX_TIES
EXCLUSIONS = (NO, CUR, GROUP, TIES)
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
RM = [(P, 2, True), (P, 3, False), (P, 0, False)]                          # _range_table's measures: a double, an integer, the partition id
EX_PATTERNS = list(PATTERNS) + ["a tie run over three tiles", "ties at the ends"]
UF = 2.0 ** -53


def _sizes(ctx):
    T = ctx.window_geometry()
    S, tile, _ = ctx.sort_geometry()
    ex_tile, narrow = ctx.window_exclude_geometry()
    assert ex_tile == T == tile and narrow == 0                            # one tile for every window pass; no kernel walks a frame
    return T, S, sorted({0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, S - 1, S, S + 1, 4095, 4096, 4097, 65537})


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _f64_measure(col):
    op, kind, _, is_f64 = col[:4]
    return kind == V or (kind == P and bool(is_f64))


def _is_f64(col):
    return col[0] == AVG or (col[0] != COUNT and _f64_measure(col))


class Excluded(Ranged):
    """Ranged with the tie run of every position and the pieces a column's exclusion leaves of its base frame.  A column is (op, kind,
    index, is_f64, unit, lo, hi, empty, exclude)."""

    def __init__(self, rows, terms, npart, rank_tables=None):
        Ranged.__init__(self, rows, terms, npart, rank_tables)
        head = self.ref.tie_head
        self.tie_a = np.maximum.accumulate(np.where(head, self.pos, 0)) if self.n else self.pos
        self.tie_b = _last_of(head)

    def base(self, unit, lo, hi):
        if unit == ROWS:
            far = self.n + 1
            return Slid.frame(self, -far if lo is None else lo, far if hi is None else hi)
        return self.ends(unit, lo, hi)

    def pieces(self, col):
        """[(holds rows?, first, last)] x 3 in position order — the part in front of what is taken out, the row itself (TIES), the part
        behind — and the number of remaining rows"""
        unit, lo, hi, _, exclude = col[4:]
        left, right, emp = self.base(unit, lo, hi)
        if exclude == NO:
            x0, x1 = right + 1, right
        elif exclude == CUR:
            x0, x1 = self.pos, self.pos
        else:
            x0, x1 = self.tie_a, self.tie_b
        a1, b1, a3, b3 = left, np.minimum(right, x0 - 1), np.maximum(left, x1 + 1), right
        p1, p3 = ~emp & (a1 <= b1), ~emp & (a3 <= b3)
        mid = (~emp & (left <= self.pos) & (self.pos <= right)) if exclude == TIES else np.zeros(self.n, bool)
        count = (np.where(p1, b1 - a1 + 1, 0) + mid + np.where(p3, b3 - a3 + 1, 0)).astype(np.int64)
        return [(p1, a1, b1), (mid, self.pos, self.pos), (p3, a3, b3)], count

    def int_sum(self, kind, index, is_f64, parts):
        """the exact sum over the pieces as int64 (wrapping); a double measure is integer-valued below 2^40 here"""
        x = self.raw(kind, index)
        if is_f64:
            xf = x.view(np.float64)
            x = xf.astype(np.int64)
            assert (x == xf).all() and (np.abs(x) < 1 << 40).all()
        c = np.concatenate((np.zeros(1, np.uint64), np.cumsum(x.view(np.uint64), dtype=np.uint64)))
        total = np.zeros(self.n, np.uint64)
        for has, a, b in parts:
            a, b = np.where(has, a, self.pos), np.where(has, b, self.pos)
            total = total + np.where(has, c[b + 1] - c[a], np.uint64(0))
        return total.view(np.int64)

    def want_col(self, col):
        op, kind, index, is_f64, unit, lo, hi, empty, exclude = col
        parts, count = self.pieces(col)
        if op == COUNT:
            return count
        none = count == 0
        is_f64 = _f64_measure(col)
        (p1, a1, b1), (mid, _, _), (p3, a3, b3) = parts
        if op in (FIRST, LAST):
            at = np.where(p1, a1, np.where(mid, self.pos, a3)) if op == FIRST else np.where(p3, b3, np.where(mid, self.pos, b1))
            v = self.raw(kind, index)[np.where(none, self.pos, at)]
        elif op in (SUM, AVG):
            v = self.int_sum(kind, index, is_f64, parts)
            if op == AVG:
                v = (v.astype(np.float64) / np.where(none, 1, count).astype(np.float64)).view(np.int64)      # (below 2^53: the conversion is exact either way)
            elif is_f64:
                v = v.astype(np.float64).view(np.int64)
        else:
            levels = self._levels(op, kind, index, is_f64)
            e = np.zeros(self.n, np.uint64)
            for has, a, b in parts:
                a, b = np.where(has, a, self.pos), np.where(has, b, self.pos)
                k = np.frexp((b - a + 1).astype(np.float64))[1] - 1
                q = np.maximum(levels[k, a], levels[k, b - (np.int64(1) << k) + 1]) if self.n else e
                e = np.where(has, np.maximum(e, q), e)
            u = ~e if op == MIN else e
            v = np.where(e == 0, QNAN, np.where(u >> np.uint64(63) != 0, u ^ TOP, ~u)).view(np.int64) if is_f64 else (u ^ TOP).view(np.int64)
        return np.where(none, np.int64(empty), v)


def _marshal(cols):
    arr = (abi.WindowExclude * max(1, len(cols)))()
    for a, (op, kind, index, is_f64, unit, lo, hi, empty, exclude) in zip(arr, cols):
        a.op, a.kind, a.index, a.is_f64, a.unit, a.empty, a.exclude = op, kind, index, int(bool(is_f64)), unit, empty, exclude
        a.flags = (abi.WRANGE_LO_UNBOUNDED if lo is None else 0) | (abi.WRANGE_HI_UNBOUNDED if hi is None else 0)
        a.lo, a.hi = abi._range_offset(lo), abi._range_offset(hi)
    return arr


def _raw(ctx, t, min_hits, npart, terms, cols, limit, capacity, keys=None, out=None, nterms=None, ncols=None, patch=None):
    got = C.c_int64(-7)
    arr = _marshal(cols)
    if patch is not None:
        patch(arr[0])
    rc = ctx.lib.sdqh_table_window_exclude(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms),
                                           abi._marshal_sort_terms(terms), C.c_int(len(cols) if ncols is None else ncols), arr,
                                           C.c_int64(limit), C.c_int64(capacity), None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                           None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value


def _limits(n):
    return sorted({1, max(1, n // 2), ALL})


def _check(ctx, t, terms, npart, what, col_lists, min_hits=1, rank_tables=None, limits=None, ref=None):
    """Every list of columns in one call each: rows and values against numpy, exact by bits; dtypes; the count-only call.  A limit cuts
    the rows returned, never the frames: the expected values are the first m of the whole table's."""
    rows = _stage_rows(ctx, t, min_hits)
    ref = ref or Excluded(rows, terms, npart, rank_tables)
    done = 0
    for i, cols in enumerate(col_lists):
        for limit in (limits(ref.n) if limits and i == 0 else (ALL,)):
            got = ctx.table_window_exclude(t, min_hits, npart, terms, cols, limit, 64, want_hits=t.accumulate)
            m = min(limit, ref.n)
            _same(got, rows, ref.order[:m], (what, cols, limit))
            assert len(got[4]) == len(cols)
            for a, col in zip(got[4], cols):
                assert a.dtype == (np.float64 if _is_f64(col) else np.int64) and len(a) == m, (what, col)
                want = ref.want_col(col)[:m]
                bad = np.nonzero(_bits(a) != want)[0]
                assert len(bad) == 0, (what, col, limit, bad[:5], _bits(a)[bad[:5]], want[bad[:5]])
                done += 1
    assert _raw(ctx, t, min_hits, npart, terms, col_lists[0], ALL, 0) == (abi.OK, ref.n), (what, "count")
    return done, ref


def _frames(n, T):
    """offsets 0, +-1, around the wave, the tile and the table, unbounded sides, and frames that do not hold their row"""
    N = max(n, 1)
    return [(0, 0), (-1, 0), (0, 1), (-1, 1), (-63, 0), (0, 64), (-65, 65), (-64, 63), (-T, 0), (0, T), (-T, T), (-N, N), (None, 0), (0, None), (None, None),
            (None, -1), (1, None), (1, 3), (-3, -1), (2, 65), (-T - 2, -2), (3, T + 3), (-N, -1), (64, None)]


def _col_lists(frames, shift):
    """Every frame once, four to a call; the unit turns with the frame and the exclusion with every third, so the 24 frames meet all 12
    pairs of them twice at every size; ops, measures and empties rotate, moved by `shift` from size to size."""
    cols = []
    for i, (lo, hi) in enumerate(frames):
        cols.append((OPS[(i + shift) % len(OPS)],) + RM[(i + shift) % len(RM)] + (UNITS[i % 3], lo, hi, EMPTIES[(i + shift) % len(EMPTIES)], EXCLUSIONS[(i // 3 + shift) % 4]))
    return [cols[i:i + 4] for i in range(0, len(cols), 4)]


def _ex_pattern(name, n, T, rng):
    """-> (partition ids, int64 order values) per row, rows in random build order.  The order values tie often; the two patterns of this
    file place their tie runs by position."""
    if name in PATTERNS:
        part = _pattern(name, n, T, rng)[0]
        return part, rng.integers(0, max(2, n // 4), n).astype(np.int64)
    pos = np.arange(n, dtype=np.int64)
    if name == "a tie run over three tiles":                               # one partition; a run from the end of the first tile into the fourth
        part, order = np.zeros(n, np.int64), pos.copy()
        order[(pos >= T - 10) & (pos <= 3 * T + 5)] = T - 10
    else:                                                                  # partitions of 150 rows whose first 3 and last 70 rows tie; every other row alone
        part, at = pos // 150, pos % 150
        order = np.where(at < 3, 0, np.where(at >= 80, 80, at))
    mix = rng.permutation(n)
    return part[mix], order[mix]


# 1. the definition: sizes x patterns x units x exclusions -------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", EX_PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes = _sizes(ctx)
    case = EX_PATTERNS.index(pattern)
    rng = np.random.default_rng(100 + case)
    met = set()
    for at, n in enumerate(sizes):
        part, order = _ex_pattern(pattern, n, T, rng)
        desc = (at + case) % 2 == 1                                        # ascending and descending alternate over the sizes
        frames = _frames(n, T)
        lists = _col_lists(frames, at)
        here = [c for cols in lists for c in cols]                         # every size, the largest included, runs every frame in all 12 pairs of unit and exclusion
        assert [(c[5], c[6]) for c in here] == frames and {(c[4], c[8]) for c in here} == {(u, x) for u in UNITS for x in EXCLUSIONS}, n
        met |= {(c[0], c[4], c[8]) for c in here}
        terms = [(P, 0, False, False), (P, 1, desc, False)]
        ints = rng.integers(-1000, 1000, n)
        if n > 2:
            ints[rng.integers(0, n, 2)] = (I_MIN, I_MAX)                   # MIN / MAX of the others when the row holds an extreme
        t = _range_table(ctx, part, order, rng.integers(-50, 50, n).astype(np.float64), ints)
        try:
            done, ref = _check(ctx, t, terms, 1, (pattern, n, desc), lists, min_hits=0, limits=_limits)
            assert done >= len(frames) == 24 and ref.n == n
            if pattern == "a tie run over three tiles" and n > 3 * T + 6:
                assert (ref.tie_b - ref.tie_a).max() == 2 * T + 15
            if n > 3:                                                      # frames look past the limit: row 0 of m = 1 counts rows that are not returned
                got = ctx.table_window_exclude(t, 0, 0, terms, [(COUNT, P, 0, False, ROWS, 0, None, 0, CUR)], 1, 64, want_hits=False)
                assert len(got[0]) == 1 and got[4][0][0] == n - 1
        finally:
            t.free()
    assert {op for op, _, _ in met} == set(OPS) and len(met) >= 60         # over the sizes every op meets most pairs (7 x 12 = 84)


# 2. nothing is added and later subtracted ---------------------------------------------------------------------------------------------------
def test_nothing_is_subtracted(hip_engine):
    """One 1e300 and one -1e300 among small integers, each inside a tie run of three.  A sum that folded the whole frame and subtracted
    what is excluded loses the small values (1e300 + 3 - 1e300 = 0): wherever what remains holds no huge value the sum is exact — on
    the huge rows themselves under CURRENT ROW, on their whole tie runs under GROUP — and the average is that sum over the count."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(n)
    pos = np.arange(n, dtype=np.int64)
    order = pos // 3                                                       # tie runs of three
    dbls = rng.integers(-9, 10, n).astype(np.float64)
    dbls[T - 2], dbls[T + 200] = 1e300, -1e300                             # (in the runs [T - 2, T] — across the tile's edge — and [T + 199, T + 201])
    mix = rng.permutation(n)
    t = _range_table(ctx, np.zeros(n, np.int64), order[mix], dbls[mix], pos[mix])
    try:
        terms = [(P, 0, False, False), (P, 1, False, False)]
        rows = _stage_rows(ctx, t, 0)
        ref = Excluded(rows, terms, 1)
        x = np.ascontiguousarray(ref.raw(P, 2)).view(np.float64)
        huge = np.abs(x) > 1e200
        small = np.where(huge, 0.0, x)
        c = np.concatenate(([0.0], np.cumsum(small)))                     # (small integers: exact)
        ch = np.concatenate(([0], np.cumsum(huge)))
        seen = 0
        for unit, lo, hi in ((ROWS, -5, 5), (ROWS, None, 2), (GRP, -2, 2), (VAL, -1, 1), (ROWS, -150, 150)):
            for exclude in (CUR, GROUP, TIES):
                cols = [(SUM, P, 2, True, unit, lo, hi, 0, exclude), (AVG, P, 2, True, unit, lo, hi, 0, exclude), (COUNT, P, 0, False, unit, lo, hi, 0, exclude)]
                got = ctx.table_window_exclude(t, 0, 1, terms, cols, ALL, 64, want_hits=False)[4]
                parts, count = ref.pieces(cols[0])
                assert (got[2] == count).all()
                total, inside = np.zeros(n), np.zeros(n, np.int64)
                for has, a, b in parts:
                    a, b = np.where(has, a, ref.pos), np.where(has, b, ref.pos)
                    total += np.where(has, c[b + 1] - c[a], 0.0)
                    inside += np.where(has, ch[b + 1] - ch[a], 0)
                clean = (inside == 0) & (count > 0)
                assert (got[0][clean] == total[clean]).all(), (unit, lo, hi, exclude)
                assert (_bits(got[1][clean]) == _bits(total[clean] / count[clean].astype(np.float64))).all(), (unit, lo, hi, exclude)
                on_huge = clean & huge if exclude == CUR else clean & (ch[ref.tie_b + 1] - ch[ref.tie_a] > 0)
                seen += int(on_huge.sum()) if exclude != TIES else 0
        assert seen >= 2 * 4 + 6 * 4                                       # the two huge rows, and the six rows of their runs, in four of the frames at least
    finally:
        t.free()


# 3. general doubles: the header's bound, m = the remaining rows ---------------------------------------------------------------------------------
def test_general_doubles_within_the_bound(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    for n in (S + 1, 4097):
        rng = np.random.default_rng(n)
        part, order = _ex_pattern("runs" if n == S + 1 else "a tie run over three tiles", n, T, rng)
        dbls = rng.normal(0.0, 1e3, n) * 10.0 ** rng.integers(-3, 6, n)
        t = _range_table(ctx, part, order, dbls, np.arange(n))
        try:
            terms = [(P, 0, False, False), (P, 1, False, False)]
            ref = Excluded(_stage_rows(ctx, t, 0), terms, 1)
            x = np.ascontiguousarray(ref.raw(P, 2)).view(np.float64)
            for unit, lo, hi, exclude in ((ROWS, -70, 70, CUR), (GRP, -3, 3, TIES), (VAL, -40, 40, GROUP), (ROWS, None, None, GROUP), (GRP, None, 1, CUR)):
                cols = [(SUM, P, 2, True, unit, lo, hi, 0, exclude), (AVG, P, 2, True, unit, lo, hi, 0, exclude)]
                got = ctx.table_window_exclude(t, 0, 1, terms, cols, ALL, 64, want_hits=False)[4]
                again = ctx.table_window_exclude(t, 0, 1, terms, cols, ALL, 64, want_hits=False)[4]
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(got, again))      # two calls, the same bits
                parts, count = ref.pieces(cols[0])
                for j in range(0, n, 37):                                  # exact arithmetic on a sample of the rows
                    vals = [Fraction(float(v)) for has, a, b in parts if has[j] for v in x[a[j]:b[j] + 1]]
                    m = len(vals)
                    assert m == count[j]
                    if m:
                        assert abs(Fraction(float(got[0][j])) - sum(vals)) <= Fraction(m - 1) * Fraction(UF) / (1 - Fraction(m - 1) * Fraction(UF)) * sum(abs(v) for v in vals), (n, unit, j)
                        assert _bits(got[1][j:j + 1])[0] == _bits(np.array([got[0][j] / np.float64(m)]))[0], (n, unit, j)
        finally:
            t.free()


# 4. where the siblings overlap -------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_siblings(hip_engine):
    """Nothing excluded: a VALUE / GROUPS column is sdqh_table_window_range's bit for bit, a double SUM of general doubles included (the
    same tree, the same query); a ROWS column is sdqh_table_window_slide's for every op but a double SUM, which is exact on
    integer-valued doubles and within the bound otherwise.  Where every row is its own tie run GROUP is CURRENT ROW and TIES takes
    nothing out (a double SUM aside: the same rows in three pieces).  An AVG has the bits of its own call's SUM over its COUNT."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    for n in (T + 1, 4097):
        rng = np.random.default_rng(n + 7)
        part = _pattern("runs", n, T, rng)[0]
        order = rng.integers(0, max(2, n // 4), n).astype(np.int64)
        wild = rng.normal(0.0, 1e3, n) * 10.0 ** rng.integers(-3, 6, n)
        t = _range_table(ctx, part, order, wild, rng.integers(-1000, 1000, n))
        try:
            terms = [(P, 0, False, False), (P, 1, True, False)]
            for lo, hi in ((-2, 0), (0, T + 1), (-65, 64), (-T - 2, -2), (3, 5), (None, 1), (None, None)):
                for ms in ([(SUM, P, 2, True), (COUNT, P, 0, False), (MIN, P, 2, True), (MAX, P, 3, False)], [(FIRST, P, 2, True), (LAST, P, 3, False), (SUM, P, 3, False)]):
                    for unit in (VAL, GRP):
                        want = ctx.table_window_range(t, 0, 1, terms, [m + (unit, lo, hi, -1) for m in ms], ALL, 64, want_hits=False)[4]
                        got = ctx.table_window_exclude(t, 0, 1, terms, [m + (unit, lo, hi, -1, NO) for m in ms], ALL, 64, want_hits=False)[4]
                        assert all((_bits(a) == _bits(b)).all() for a, b in zip(got, want)), (n, lo, hi, unit)
                    slide = ctx.table_window_slide(t, 0, 1, terms, [m + (abi.SLIDE_UNBOUNDED_PRECEDING if lo is None else lo, abi.SLIDE_UNBOUNDED_FOLLOWING if hi is None else hi, -1) for m in ms],
                                                   ALL, 64, want_hits=False)[4]
                    got = ctx.table_window_exclude(t, 0, 1, terms, [m + (ROWS, lo, hi, -1, NO) for m in ms], ALL, 64, want_hits=False)[4]
                    for m, a, b in zip(ms, got, slide):
                        if m[0] == SUM and m[3]:                           # two associations of the same rows: each within gamma(m) of exact
                            w = float(min(n, (hi if hi is not None else n) - (lo if lo is not None else -n) + 1))
                            mag = np.abs(wild).sum()
                            assert ((_bits(a) == _bits(b)) | (np.abs(a - b) <= 2 * (w * UF / (1 - w * UF)) * mag)).all(), (n, lo, hi)      # (an empty frame: `empty`'s bits, a NaN)
                        else:
                            assert (_bits(a) == _bits(b)).all(), (n, lo, hi, m)
            # every row its own tie run: order by (value, key) — the key is unique
            own = terms + [(K, 0, False, False)]
            for unit, lo, hi in ((ROWS, -3, 3), (GRP, -2, 65), (ROWS, 1, 4), (GRP, None, 0)):
                ms = [(SUM, P, 2, True), (AVG, P, 3, False), (MIN, P, 3, False), (LAST, P, 2, True)]
                cur, group, ties, none = (ctx.table_window_exclude(t, 0, 1, own, [m + (unit, lo, hi, -1, x) for m in ms], ALL, 64, want_hits=False)[4] for x in (CUR, GROUP, TIES, NO))
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(cur, group)), (n, unit, lo, hi)
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(ties[1:], none[1:])), (n, unit, lo, hi)      # (the double SUM joins three pieces there, one here: other bits)
            # AVG = the same call's SUM / COUNT, a double and an integer measure, every exclusion
            for x in EXCLUSIONS:
                for kind in ((P, 2, True), (P, 3, False)):
                    cols = [(AVG,) + kind + (GRP, -1, 2, -1, x), (SUM,) + kind + (GRP, -1, 2, -1, x), (COUNT,) + kind + (GRP, -1, 2, -1, x)]
                    avg, total, cnt = ctx.table_window_exclude(t, 0, 1, terms, cols, ALL, 64, want_hits=False)[4]
                    some = cnt > 0
                    assert avg.dtype == np.float64 and (_bits(avg[some]) == _bits(total[some].astype(np.float64) / cnt[some].astype(np.float64))).all(), (n, x, kind)
                    assert (_bits(avg[~some]) == -1).all()
        finally:
            t.free()


# 5. one call, three units, three exclusions; determinism ---------------------------------------------------------------------------------
def test_a_mixed_call_is_its_single_calls_behind_one_sort(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    for n in (S - 1, 4 * T + 3):
        rng = np.random.default_rng(n + 1)
        part, order = _ex_pattern("heavy ties", n, T, rng)
        wild = rng.normal(0.0, 1e3, n) * 10.0 ** rng.integers(-3, 6, n)
        t = _range_table(ctx, part, order, wild, rng.integers(-1000, 1000, n))
        try:
            terms = [(P, 0, False, False), (P, 1, False, False)]
            cols = [(AVG, P, 2, True, ROWS, -103, 103, 0, CUR), (SUM, P, 2, True, VAL, -20, 20, 0, GROUP), (COUNT, P, 0, False, GRP, -3, 3, 0, TIES), (MAX, P, 3, False, ROWS, None, 0, 0, NO)]
            ctx.set_profiling(1)
            try:
                mixed = ctx.table_window_exclude(t, 0, 1, terms, cols, ALL, n, want_hits=False)[4]
                k_mixed = [nm for nm, _ in ctx.profile()]
                singles, k_single = [], []
                for col in cols:
                    singles.append(ctx.table_window_exclude(t, 0, 1, terms, [col], ALL, n, want_hits=False)[4][0])
                    k_single.append([nm for nm, _ in ctx.profile()])
            finally:
                ctx.set_profiling(0)
            assert all((_bits(a) == _bits(b)).all() for a, b in zip(mixed, singles)), n
            sorts = lambda names: sorted(nm for nm in names if nm.startswith("k_sort_"))      # noqa: E731
            assert sorts(k_mixed) and all(sorts(k) == sorts(k_mixed) for k in k_single)          # one sort, whatever the columns
            assert "k_wsl_blocks" not in k_mixed and "k_wex_fold" in k_mixed and "k_wex_ties" in k_mixed and "k_wrg_stage" in k_mixed
            assert "k_wex_ties" not in k_single[0] and "k_wq_ties" not in k_single[3] and k_single[3].count("k_win_rank") == 0      # nothing built that no column reads
            assert k_mixed.count("k_win_rank") == 2 and k_single[2].count("k_win_rank") == 2 and k_single[1].count("k_win_rank") == 1
            # the same call again: the same bits; under NO_OTHERS and GROUP all rows of a tie run share a VALUE / GROUPS column's value
            again = ctx.table_window_exclude(t, 0, 1, terms, cols, ALL, n, want_hits=False)[4]
            assert all((_bits(a) == _bits(b)).all() for a, b in zip(mixed, again))
            ref = Excluded(_stage_rows(ctx, t, 0), terms, 1)
            for x in (NO, GROUP):
                shared = [(SUM, P, 2, True, VAL, -20, 20, 0, x), (AVG, P, 2, True, GRP, -1, 1, 0, x), (MIN, P, 3, False, GRP, None, 0, 0, x), (LAST, P, 3, False, VAL, -5, 30, 0, x)]
                for a in ctx.table_window_exclude(t, 0, 1, terms, shared, ALL, n, want_hits=False)[4]:
                    assert (_bits(a) == _bits(a)[ref.tie_a]).all(), (n, x)
        finally:
            t.free()


# 6. layouts and terms ---------------------------------------------------------------------------------------------------------------------
def test_layouts(hip_engine):
    """The direct layout, the open-addressing layout, a table with duplicate build keys (owner rows only), the probed table of the
    ordering tests, each with min_hits 0 and 2.  The order term is a double column of integer values: VALUE offsets are doubles."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(n)
    part, value, _ = _pattern("runs", n, T, rng)
    hits = rng.integers(0, 4, n)                                           # some entries never probed: min_hits selects
    terms = [(P, 0, False, False), (V, 0, True, True)]
    lists = [[(SUM, V, 0, True, VAL, -2.0, 64.0, 0, CUR), (MAX, H, 0, False, GRP, -T, 0, -1, GROUP), (AVG, P, 0, False, ROWS, -1, 70, I_MIN, TIES), (MIN, P, 0, False, GRP, 1, T + 1, 5, NO)],
             [(AVG, H, 0, False, VAL, -3.0, 0.0, 0, TIES), (FIRST, V, 0, True, ROWS, -2, 2, -1, GROUP), (LAST, K, 0, False, VAL, None, 1.0, 0, CUR), (COUNT, K, 0, False, ROWS, None, None, 0, TIES)]]

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        try:
            return sum(_check(ctx, t, terms, 1, ("layout", dups, mh), lists, min_hits=mh, limits=_limits)[0] for mh in (0, 2))
        finally:
            t.free()
    assert run(0) >= 2 * 8
    assert run(200) >= 2 * 8
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) >= 2 * 8
    t = _probed_table(ctx, S + 1)
    try:
        pt = [(P, 0, False, False), (V, 0, False, True)]
        pl = [[(AVG, P, 1, True, ROWS, -3, 3, 0, CUR), (MAX, P, 1, True, GRP, -1, 1, 0, GROUP), (COUNT, K, 0, False, VAL, -500.0, 500.0, 0, TIES), (FIRST, H, 0, False, ROWS, 1, 2, -1, NO)]]
        for mh in (0, 2):
            rows = _stage_rows(ctx, t, mh)
            ref = Excluded(rows, pt, 1)
            got = ctx.table_window_exclude(t, mh, 1, pt, pl[0], ALL, 64)
            _same(got, rows, ref.order, ("probed", mh))
            for a, col in zip(got[4], pl[0]):
                if col[0] == AVG:                                          # the measure counts in quarters: summed as integers (exact in doubles too), scaled back
                    parts, count = ref.pieces(col)
                    c = np.concatenate(([0.0], np.cumsum(np.ascontiguousarray(ref.raw(P, 1)).view(np.float64) * 4.0)))
                    total = sum(np.where(has, c[np.where(has, b, ref.pos) + 1] - c[np.where(has, a0, ref.pos)], 0.0) for has, a0, b in parts) / 4.0
                    some = count > 0
                    assert (_bits(a[some]) == _bits(total[some] / count[some].astype(np.float64))).all() and (_bits(a[~some]) == 0).all(), mh
                else:
                    assert (_bits(a) == ref.want_col(col)).all(), (mh, col)
    finally:
        t.free()


def test_derived_terms(hip_engine):
    """PARTITION BY the high half of a packed key — and by a text-ranked payload behind it; ROWS, GROUPS and VALUE (over the low half,
    descending) in one call."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    m = (P, 0, False)
    try:
        n = S + 1
        a = rng.integers(0, n // 90 + 2, n).astype(np.int64)
        b = rng.integers(0, 300, n).astype(np.int64)
        keys = np.unique((a << 32) | b)
        keys = keys[rng.permutation(len(keys))]
        ref_col = rng.integers(0, len(text), len(keys)).astype(np.int64)
        t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ref_col)], accumulate=False)
        try:
            hi_half, lo_half = (K, 0, False, False, 1 << 32, 0, 0, None), (K, 0, True, False, 0, 1 << 32, 0, None)
            lists = [[(AVG,) + m + (VAL, -30, 30, 0, CUR), (MIN,) + m + (ROWS, -64, 0, 0, GROUP), (LAST,) + m + (GRP, 1, 100, -1, TIES), (COUNT,) + m + (VAL, -T, T, 0, GROUP)]]
            assert _check(ctx, t, [hi_half, lo_half], 1, "derived value", lists, min_hits=0, limits=_limits)[0] >= 4
            by_text = [(P, 0, False, False, 0, 0, 0, ct), hi_half, lo_half]      # the text's rank and the key's high half partition; ties on the low half
            glists = [[(SUM,) + m + (GRP, -3, 3, 0, TIES), (MAX, K, 0, False, ROWS, -2, 2, 0, CUR), (FIRST,) + m + (ROWS, 1, 1, -1, GROUP), (AVG, K, 0, False, GRP, None, None, 0, CUR)]]
            assert _check(ctx, t, by_text, 2, "text partition", glists, min_hits=0, rank_tables={id(ct): want})[0] >= 4
        finally:
            t.free()
    finally:
        ct.free()


# 7. limits, empties, errors -----------------------------------------------------------------------------------------------------------------
def test_limits_and_empties(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = T + 1
    rng = np.random.default_rng(n)
    part, order = _ex_pattern("ties at the ends", n, T, rng)
    t = _range_table(ctx, part, order, rng.integers(-50, 50, n).astype(np.float64), rng.integers(-1000, 1000, n))
    try:
        terms = [(P, 0, False, False), (P, 1, False, False)]
        cols = [(SUM, P, 3, False, ROWS, -2, 2, 0, CUR), (AVG, P, 2, True, GRP, 0, 0, 0, GROUP), (FIRST, P, 3, False, VAL, -1, 1, -1, TIES), (COUNT, P, 0, False, ROWS, None, None, 0, GROUP)]
        ref = Excluded(_stage_rows(ctx, t, 0), terms, 1)
        for limit in (1, 7, n - 1, n, ALL):                                # a limit below n cuts the rows, never the frames
            got = ctx.table_window_exclude(t, 0, 1, terms, cols, limit, 64, want_hits=False)
            m = min(limit, n)
            assert len(got[0]) == m and all((_bits(a) == ref.want_col(c)[:m]).all() for a, c in zip(got[4], cols)), limit
        assert _raw(ctx, t, 0, 1, terms, cols, ALL, 0) == (abi.OK, n) and _raw(ctx, t, 0, 1, terms, cols, 5, 0) == (abi.OK, 5)      # the count-only call
        keys, out = np.full(n, -7, np.int64), np.full((4, n), -7, np.int64)
        assert _raw(ctx, t, 0, 1, terms, cols, ALL, n - 1, keys, out) == (abi.ERR_OVERFLOW, n)      # a capacity one too small: the needed count, nothing written
        assert (keys == -7).all() and (out == -7).all()
        assert _raw(ctx, t, 0, 1, terms, cols, ALL, n, keys, None) == (abi.OK, n)                  # out_cols = NULL: rows only
        assert (keys == rows_keys(ctx, t)[ref.order]).all()
        assert _raw(ctx, t, 0, 1, terms, cols, ALL, n, keys, out) == (abi.OK, n) and all((out[i] == ref.want_col(c)).all() for i, c in enumerate(cols))
        # what remains nothing of takes `empty` by its bits, whatever the op but COUNT: GROUPS 0..0 excluding the group is empty on every row
        for empty in EMPTIES:
            nothing = [(op, P, 2, True, GRP, 0, 0, empty, GROUP) for op in (SUM, MIN, FIRST, AVG)]
            got = ctx.table_window_exclude(t, 0, 1, terms, nothing, ALL, 64, want_hits=False)[4]
            assert all((_bits(a) == empty).all() for a in got), empty
            some = [(op, P, 3, False, ROWS, 0, 1, empty, CUR) for op in (MAX, LAST, AVG)] + [(COUNT, P, 0, False, GRP, 0, 0, empty, GROUP)]
            got = ctx.table_window_exclude(t, 0, 1, terms, some, ALL, 64, want_hits=False)[4]
            last = ref.pos == ref.end                                      # the last row of a partition has no next row
            assert last.any() and all((_bits(a)[last] == empty).all() and (_bits(a) == ref.want_col(c)).all() for a, c in zip(got[:3], some)) and (got[3] == 0).all(), empty
    finally:
        t.free()


def rows_keys(ctx, t):
    return _stage_rows(ctx, t, 0)[0]


def test_argument_errors_leave_the_context_usable(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    rng = np.random.default_rng(3)
    part, order = _ex_pattern("runs", 700, T, rng)
    t = _range_table(ctx, part, order, rng.integers(-50, 50, 700).astype(np.float64), rng.integers(-1000, 1000, 700))
    try:
        terms = [(P, 0, False, False), (P, 1, False, False)]
        fterms = [(P, 0, False, False), (P, 2, False, True)]
        m = (P, 3, False)
        ok = [(SUM,) + m + (ROWS, -1, 1, 0, CUR)]
        keys, out = np.full(700, -7, np.int64), np.full((4, 700), -7, np.int64)

        def flag(bits):
            return lambda a: setattr(a, "flags", bits)
        for npart, tm, cols, limit, nterms, ncols, patch in (
                (1, terms, [(7,) + m + (ROWS, -1, 1, 0, CUR)], ALL, None, None, None), (1, terms, [(-1,) + m + (ROWS, -1, 1, 0, CUR)], ALL, None, None, None),      # op
                (1, terms, [(SUM,) + m + (3, -1, 1, 0, CUR)], ALL, None, None, None), (1, terms, [(SUM,) + m + (-1, -1, 1, 0, CUR)], ALL, None, None, None),       # unit
                (1, terms, [(SUM,) + m + (ROWS, -1, 1, 0, 4)], ALL, None, None, None), (1, terms, [(SUM,) + m + (ROWS, -1, 1, 0, -1)], ALL, None, None, None),     # exclude
                (1, terms, ok, ALL, None, None, flag(4)), (1, terms, ok, ALL, None, None, lambda a: setattr(a, "_pad", 1)),                                        # flag bits, the pad
                (1, terms, [(SUM,) + m + (ROWS, 1, 0, 0, CUR)], ALL, None, None, None), (1, terms, [(AVG,) + m + (GRP, 1, 0, 0, TIES)], ALL, None, None, None),    # lo > hi
                (1, terms, [(SUM,) + m + (VAL, 1, 0, 0, CUR)], ALL, None, None, None), (1, fterms, [(SUM,) + m + (VAL, 0.5, 0.25, 0, CUR)], ALL, None, None, None),
                (1, fterms, [(SUM,) + m + (VAL, -math.inf, 0.0, 0, CUR)], ALL, None, None, None),                                                                  # a non-finite offset
                (1, terms + [(K, 0, False, False)], [(SUM,) + m + (VAL, -1, 1, 0, CUR)], ALL, None, None, None), (2, terms, [(SUM,) + m + (VAL, -1, 1, 0, CUR)], ALL, None, None, None),      # VALUE: two order terms, none
                (1, terms, ok, ALL, None, 0, None), (1, terms, ok * 4, ALL, None, 5, None), (1, terms, ok, 0, None, None, None), (3, terms, ok, ALL, None, None, None),
                (1, terms, ok, ALL, 0, None, None), (1, terms, [(SUM, P, 4, False, ROWS, -1, 1, 0, CUR)], ALL, None, None, None), (1, terms, [(AVG, K, 0, True, ROWS, -1, 1, 0, CUR)], ALL, None, None, None)):
            assert _raw(ctx, t, 0, npart, tm, cols, limit, 700, keys, out, nterms=nterms, ncols=ncols, patch=patch) == (abi.ERR_INVALID, -7), (npart, tm, cols, limit, nterms, ncols)
            assert (keys == -7).all() and (out == -7).all()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_exclude(t, 0, 1, terms, [(7,) + m + (ROWS, 0, 0, 0, CUR)], ALL, 64)
        assert e.value.code == abi.ERR_INVALID
        # an unbounded side ignores its offset, whatever it holds; COUNT ignores its measure, whatever it names
        assert _raw(ctx, t, 0, 1, terms, [(COUNT,) + m + (ROWS, 5, -5, 0, CUR)], ALL, 0, patch=flag(3)) == (abi.OK, 700)
        got = ctx.table_window_exclude(t, 0, 1, terms, [(COUNT, P, 9, True, ROWS, 0, 0, 7, NO)], ALL, 64, want_hits=False)
        assert got[4][0].dtype == np.int64 and (got[4][0] == 1).all()
        assert _check(ctx, t, terms, 1, "after the errors", _col_lists(_frames(700, T), 0), min_hits=0)[0] >= 24      # the context still works
    finally:
        t.free()


# 8. through the engine and the decorator -------------------------------------------------------------------------------------------------
Q3_MIXED = {"others": ("avg", "revenue", -103, 103), "near": ("sum", "revenue", -20000.0, 20000.0, None, "value"), "peers": ("count", None, -3, 3, None, "groups"),
            "best": ("max", "revenue", None, 0)}


def _q3_remaining(res, by, exclude):
    """{column: (rows, sum of |revenue|) of what remains of every row's frame} for Q3_MIXED's two summed columns, by numpy on the
    returned rows (in order already, revenue descending inside every order date)."""
    rev = np.asarray(res.column("revenue"))
    n = len(rev)
    pos = np.arange(n)
    start, end = _partitions(res, by)
    head = np.ones(n, bool)
    head[1:] = (rev[1:] != rev[:-1]) | (start[1:] != start[:-1])
    tie_a, tie_b = np.maximum.accumulate(np.where(head, pos, 0)), _last_of(head)
    mag = np.concatenate(([0.0], np.cumsum(np.abs(rev))))
    vl, vr = np.empty(n, np.int64), np.empty(n, np.int64)
    for s in np.nonzero(start == pos)[0]:                                  # value +-20000: the rows of the date whose revenue lies within 20000 of the row's
        e = end[s]
        key = -rev[s:e + 1]                                                # (ascending)
        vl[s:e + 1] = s + np.searchsorted(key, key - 20000.0, "left")
        vr[s:e + 1] = s + np.searchsorted(key, key + 20000.0, "right") - 1
    out = {}
    for c, (left, right) in (("others", (np.maximum(pos - 103, start), np.minimum(pos + 103, end))), ("near", (vl, vr))):
        rows, total = right - left + 1, mag[right + 1] - mag[left]
        if exclude != "no others":                                         # what is taken out, cut to the frame: the row, or its tie run (with the row put back)
            x0, x1 = (pos, pos) if exclude == "current row" else (np.maximum(left, tie_a), np.minimum(right, tie_b))
            rows, total = rows - (x1 - x0 + 1), total - (mag[x1 + 1] - mag[x0])
            if exclude == "ties":
                rows, total = rows + 1, total + np.abs(rev)
        out[c] = (rows, np.maximum(total, 0.0))
    return out


def test_q3_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]

    def close(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return bool(np.allclose(a, b, rtol=RUN_TO_RUN, atol=0.0, equal_nan=True)) if a.dtype.kind == "f" else bool((a == b).all())
    for exclude in EXCLUSION_NAMES:
        note = {"k": ALL, "order": ["revenue"], "ranked": [], "per": by, "exclude": exclude,
                "frames": [["others", "avg", "revenue", "rows", -103, 103, None], ["near", "sum", "revenue", "value", -20000.0, 20000.0, None], ["peers", "count", None, "groups", -3, 3, None],
                           ["best", "max", "revenue", "rows", None, 0, None]]}
        dev = Q.q3.excluding(by, order, Q3_MIXED, exclude=exclude)(*args)
        assert eng.stats()["order_routes"][-1] == dict(note, route="window_exclude")
        monkeypatch.setattr(eng, "device_window_exclude", False)
        host = Q.q3.excluding(by, order, Q3_MIXED, exclude=exclude)(*args)
        assert eng.stats()["order_routes"][-1] == dict(note, route="host")
        monkeypatch.setattr(eng, "device_window_exclude", True)
        assert dev.columns == host.columns and dev.columns[-4:] == list(Q3_MIXED) and len(dev) == len(host) > 100
        assert [dev.column(c).dtype for c in Q3_MIXED] == [host.column(c).dtype for c in Q3_MIXED] == [np.float64, np.float64, np.int64, np.float64]
        remaining = _q3_remaining(dev, by, exclude)
        for c in dev.columns:
            if c in ("others", "near"):                                    # double sums: two associations of the frame's remaining rows, each within gamma(m) of
                m, fmag = remaining[c]                                     # exact, and two runs of the query under them — the bound of the frame's own rows
                a, b = np.asarray(dev.column(c)), np.asarray(host.column(c))
                some = m > 0
                assert (np.isnan(a) == ~some).all() and (np.isnan(b) == ~some).all(), (exclude, c)
                mf = m.astype(np.float64)
                bound = (2 * mf * UF / (1 - mf * UF) + RUN_TO_RUN) * fmag
                if c == "others":                                          # the average: that sum over its count, and one more rounding on either side
                    bound = bound / np.maximum(mf, 1.0) + 2 * UF * fmag / np.maximum(mf, 1.0)
                assert (np.abs(a - b) <= bound)[some].all(), (exclude, c)
            else:
                assert close(dev.column(c), host.column(c)), (exclude, c)
    # an average is a double whatever it measures: a float default over an integer measure (q16's count of suppliers, an int64 column
    # on the host), on the device as on the host
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    half = {"a": ("avg", "supplier_cnt", 1, 2, 0.5), "n": ("count", None, 1, 2), "low": ("min", "supplier_cnt", 1, 2, -1)}      # the two rows behind: none behind a brand's last
    dev16 = Q.q16.excluding(["p_brand"], [("supplier_cnt", "desc")], half)(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "window_exclude"
    monkeypatch.setattr(eng, "device_window_exclude", False)
    host16 = Q.q16.excluding(["p_brand"], [("supplier_cnt", "desc")], half)(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    monkeypatch.setattr(eng, "device_window_exclude", True)
    assert [dev16.column(c).dtype for c in half] == [host16.column(c).dtype for c in half] == [np.float64, np.int64, np.int64] and len(dev16) == len(host16) > 100
    assert all((_bits(dev16.column(c)) == _bits(host16.column(c))).all() for c in half)          # (sums of small integers: exact on either route)
    alone = np.asarray(dev16.column("n")) == 0
    assert alone.any() and ((np.asarray(dev16.column("a")) == 0.5) == alone).all() and ((np.asarray(dev16.column("low")) == -1) == alone).all()      # (a count is at least 1: no average of others is 0.5)
    # more than four columns: on the host
    five = dict(Q3_MIXED, n=("count", None, 0, 0))
    wide = Q.q3.excluding(by, order, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns[-5:] == list(five) and (wide.column("n") == 0).all()
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


EXCLUSION_NAMES = ("current row", "group", "ties", "no others")
