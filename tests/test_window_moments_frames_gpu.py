"""sdqh_table_window_moments (include/sdqh_sort_wmoments.h) on the MI355X (run with -m gpu) where a frame is not a ROWS frame and a call
is not three payload measures: tied, descending, double and derived ORDER BY terms, VALUE and GROUPS frames whose ends differ from the
ROWS frame's with the same offsets (test_window_moments_numpy_cpu asserts that they do), npartition 0 and 2, float offsets, calls of 8
distinct measures and 4 pairs over KEY / VALUE / HITS / payloads read both ways, min_hits that drops rows, and q3 through the
decorator over an order with ties.

The header promises bits that depend on l and r alone.  So: the frame's ends from the siblings' numpy references
(test_window_exclude_gpu.Excluded.base), the leaves in the reference's row order — the device's row order is asserted equal to it, which
pins the leaf order inside ties —, the fold from the whole-array numpy restatement (window_moments_numpy_reference), and the device's
columns compared with that BY BITS ON EVERY ROW; no row and no column is skipped anywhere in this file.  Nothing is imported from the
product's fold code.  PRINTED: the accuracy test and q3 print their worst error / bound.

What these tests cannot tell, because the results do not depend on it: the direction flag of the VALUE term (the complement of a
descending sort key is the ascending key of -v - 1, of -v for a double, so the frame search finds the same ends with the flag cleared —
the descending cases here pass either way), and whether a pair is stored as (i, j) or (j, i) (dx * dy commutes).  A library that reads
every unit as ROWS fails every tied case; one that dedups measures without is_f64, or folds only the first pair's tiles, fails
test_wide_calls."""
import numpy as np
import pytest

import moments_reference as mref
import window_moments_numpy_reference as npref
import window_moments_reference as ref
from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import MOMENT_OPS
from test_window_exclude_gpu import GRP, ROWS, VAL, Excluded, _ex_pattern
from test_window_gpu import _pattern, _same, _stage_rows, _table, db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)
from test_window_moments_cpu import COLUMNS, check_bound, data
from test_window_moments_gpu import _raw
from test_window_moments_numpy_cpu import (FAR, FRAME_CASES, I_MAX, I_MIN, MD, MI, NOPS, UNITS, Expected, case_frames, case_terms, differs_from_rows, frame_case, frame_sizes,
                                           moment_columns, tied)
from test_window_range_gpu import NAN_A, NAN_B, _order_values, _range_table

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
OP = {name: i for i, name in enumerate(MOMENT_OPS)}
assert MOMENT_OPS == npref.OPS


def _geometry(ctx):
    T = ctx.window_moments_geometry()
    assert T == ctx.window_exclude_geometry()[0] == ctx.window_geometry()
    return T


def _check(ctx, t, terms, npart, what, lists, min_hits=0, rank_tables=None):
    """Every list of columns in one call each: the rows in the reference's order, every column float64 and equal by bits to the numpy
    restatement over the reference's frame ends on every row.  -> (columns compared, the Excluded, {column: the device's values})"""
    rows = _stage_rows(ctx, t, min_hits)
    exc = Excluded(rows, terms, npart, rank_tables)
    want = Expected(exc)
    done, seen = 0, {}
    for cols in lists:
        got = ctx.table_window_moments(t, min_hits, npart, terms, cols, ALL, max(exc.n, 1), want_hits=t.accumulate)
        _same(got, rows, exc.order, (what, cols))                          # the device's row order is the reference's: the leaf order among ties is pinned
        assert len(got[4]) == len(cols)
        for a, col in zip(got[4], cols):
            assert a.dtype == np.float64 and len(a) == exc.n, (what, col)
            w = want.column(col)
            bad = np.nonzero(npref.bits(a) != npref.bits(w))[0]
            assert len(bad) == 0, (what, col, len(bad), bad[:5], a[bad[:5]], w[bad[:5]], [x[bad[:5]] for x in want.ends(*col[7:])])
            seen[col] = a
            done += 1
    return done, exc, seen


# 1. partition patterns x order patterns x sizes, three units, nine ops ---------------------------------------------------------------------
@pytest.mark.parametrize("pattern,order", FRAME_CASES)
def test_patterns_against_numpy(hip_engine, pattern, order):
    """test_window_exclude_gpu's partition patterns — a tie run over three tiles and ties at the ends among them — under
    test_window_range_gpu's order patterns with gaps, heavy ties, one value and values wide apart, ascending and descending in turn,
    over test_window_exclude_gpu's 24 frames: the unit turns with the frame, four columns to a call."""
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    met = set()
    for at, n in enumerate(frame_sizes(T)):
        part, values, desc, dbls, ints = frame_case(pattern, order, at, n, T)
        fl = case_frames(order, n, T)
        lists = moment_columns(fl, at)
        here = [c for cols in lists for c in cols]
        assert [(c[8], c[9]) for c in here] == fl
        met |= {(c[0], c[7]) for c in here}
        t = _range_table(ctx, part, values, dbls, ints)
        try:
            done, exc, _ = _check(ctx, t, case_terms(desc), 1, (pattern, order, n, desc), lists)
            assert done == len(fl) >= 24 and exc.n == n
            if tied(pattern, order) and n >= T:                            # on the device's own rows: no unit could be read as ROWS
                assert differs_from_rows(exc, fl, here) == {VAL: [True] * 3, GRP: [True] * 3}, (pattern, order, n)
            if pattern == "a tie run over three tiles" and n > 3 * T + 6:
                assert (exc.tie_b - exc.tie_a).max() == 2 * T + 15
            if order == "wide" and n > 2:                                  # nothing wraps, as Python integers say
                assert not exc.base(VAL, -FAR, FAR)[2].any() and exc.base(VAL, FAR, FAR)[2].all()
                left, right, emp = exc.base(VAL, I_MIN + 1, I_MAX - 1)
                assert ((left == exc.start) & (right == exc.end) & ~emp).all() and exc.base(VAL, I_MAX - 1, I_MAX - 1)[2].sum() >= n - 2
        finally:
            t.free()
    assert met == {(op, u) for op in range(NOPS) for u in UNITS}           # over the sizes every op met every unit


# 2. a double ORDER BY term --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 2600])
def test_double_order_values(hip_engine, n):
    """test_window_range_gpu.test_double_order_values' inputs: +-0.0, +-inf, two NaN bit patterns, DBL_MAX, denormals and ordinary
    values as order values, ascending and descending, VALUE frames with float offsets.  The reference defines the frame of a NaN row
    (its own tie run) and of a row beside one, so no row is left out of the bit comparison: the share left out, 0, is below 1 %."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(n)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, NAN_A, NAN_B, np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324, -5e-324, 2.5e-310, 1.0, 1.5, 2.0, -1.0, 1e308, 3.0, 1e-5])
    order = np.resize(edge, n)[rng.permutation(n)]
    part = rng.integers(0, 3, n)
    t = _range_table(ctx, part, order, 1e6 + rng.standard_normal(n), rng.integers(-1000, 1000, n))
    frames = [(0.0, 0.0), (-0.5, 0.5), (-1e308, 1e308), (-1e-300, 1e-300), (0.5, 1.0), (-1.0, -0.5), (None, 0.0), (0.0, None), (None, -0.5), (0.5, None), (None, None), (0.0, 1e308)]
    try:
        compared = skipped = 0
        for desc in (False, True):
            terms = [(P, 0, False, False), (P, 1, desc, True)]
            cols = []
            for i, (lo, hi) in enumerate(frames):
                y, x = [(MD, MI), (MI, MD), (MD, MD), (MI, MI)][i % 4]
                cols.append(((i + 5 * int(desc)) % NOPS,) + y + x + (VAL, lo, hi))
            done, exc, _ = _check(ctx, t, terms, 1, ("doubles", n, desc), [cols[i:i + 4] for i in range(0, len(cols), 4)])
            compared += done * exc.n
            v = exc.value()[0]
            assert np.isnan(v).any() and (v == 0.0).any() and np.isinf(v).any() and exc.value()[1:] == (True, desc)
            widths = {tuple(np.unique((r - l + 1)[~e]).tolist()[:3]) for l, r, e in (exc.base(VAL, lo, hi) for lo, hi in frames)}
            assert len(widths) > 3                                         # frames of data-dependent width
            # the float lo > hi check: -0.5 > -1.0 as doubles, below it as the int64 their bits are; (-1.0, -0.5) the other way round
            out = np.full((1, n), -7, np.int64)
            assert _raw(ctx, t, [(OP["var_pop"],) + MD + MD + (VAL, abi._range_offset(-0.5), abi._range_offset(-1.0))], ALL, n, None, out, terms=terms) == (abi.ERR_INVALID, -7)
            assert _raw(ctx, t, [(OP["var_pop"],) + MD + MD + (VAL, abi._range_offset(0.5), abi._range_offset(0.25))], ALL, n, None, out, terms=terms) == (abi.ERR_INVALID, -7)
            assert (out == -7).all()
            assert _raw(ctx, t, [(OP["var_pop"],) + MD + MD + (VAL, abi._range_offset(-1.0), abi._range_offset(-0.5))], ALL, n, None, out, terms=terms) == (abi.OK, n)
        assert compared == 2 * len(frames) * n and skipped / compared < 0.01
    finally:
        t.free()


# 3. partition and term shapes ---------------------------------------------------------------------------------------------------------------
_P0, _P3, _O = (P, 0, False, False), (P, 3, False, False), (P, 1, True, False)
_DERIVED = (P, 1, True, False, 7, 40, -20, None)                           # ((order / 7) mod 40) - 20, descending
SHAPES = [("npartition 0", 0, [_O], True), ("npartition 2", 2, [_P0, _P3, _O], True), ("derived", 1, [_P0, _DERIVED], True), ("two order terms", 1, [_P0, _O, _P3], False)]


def shape_columns(n):
    """(first partition column: four values, second: three — the integer measure too —, order values: 84 of them, 12 after the division)"""
    rng = np.random.default_rng(n + 3)
    return rng.integers(0, 4, n), rng.integers(0, 3, n), rng.integers(0, 84, n)


def shape_cols(value):
    return [(OP["regr_intercept"],) + MD + MI + (GRP, -2, 1), (OP["stddev_samp"],) + MI + MI + (VAL if value else ROWS, -3, 2),
            (OP["corr"],) + MI + MD + (GRP, None, -1), (OP["covar_samp"],) + MD + MI + (VAL if value else ROWS, 1, None)]


def test_partition_and_term_shapes(hip_engine):
    """npartition 0 and 2, a derived ORDER BY term (div / mod / add), two ORDER BY terms: each under a GROUPS frame, all but the last
    also under a VALUE frame (VALUE over two ORDER BY terms is SDQH_ERR_INVALID: test_window_moments_gpu)."""
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    for n in (T + 9, 3 * T + 5):
        rng = np.random.default_rng(n + 3)
        part, third, order = shape_columns(n)
        t = _range_table(ctx, part, order, 1e6 + rng.standard_normal(n), third)
        try:
            for what, npart, terms, value in SHAPES:
                cols = shape_cols(value)
                done, exc, _ = _check(ctx, t, terms, npart, (what, n), [cols])
                assert done == 4 and (~exc.ref.tie_head).any()
                heads = int(exc.ref.part_head.sum())
                assert heads == (1 if npart == 0 else 12 if npart == 2 else 4), (what, heads)
                got = differs_from_rows(exc, None, cols)
                assert got[GRP] == [True] * 3 and (not value or got[VAL] == [True] * 3), (what, n, got)
        finally:
            t.free()


# 4. the header's bound on wide tie runs ----------------------------------------------------------------------------------------------------
def test_tie_runs_within_the_bound(hip_engine):
    """test_window_moments_cpu.data's values — quarters beside 2^30 — under heavy ties and under a tie run over three tiles at 3 T + 5
    rows: every finite result of all nine ops within the header's bound against exact rationals (ratio below 1), NULLs by bits.  A
    bound that only held for narrow frames would show on the GROUPS frame over the tie run of 2 T + 15 rows."""
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = 3 * T + 5
    y, x = data(n, 21)
    for name in ("heavy ties", "a tie run over three tiles"):
        rng = np.random.default_rng(len(name))
        if name == "heavy ties":                                           # test_window_range_gpu's order pattern: five order values, in two partitions
            part = rng.integers(0, 2, n)
            order = _order_values(name, part, rng)
        else:
            part, order = _ex_pattern(name, n, T, rng)
        t = _range_table(ctx, part, order, y, x.astype(np.int64))
        try:
            terms = case_terms(name == "heavy ties")
            fl = [(GRP, 0, 0), (GRP, -1, 1), (VAL, -3, 3), (GRP, None, 0), (VAL, 1, 40), (GRP, -2, -1)]
            m = {"y": (MD, MD), "x": (MI, MI), "yx": (MD, MI)}
            lists = [[(OP[op],) + m[which][0] + m[which][1] + f for op, which in COLUMNS[i:i + 4]] for f in fl for i in range(0, len(COLUMNS), 4)]
            done, exc, seen = _check(ctx, t, terms, 1, name, lists)
            assert done == len(fl) * len(COLUMNS)
            ys, xs = npref.leaf(exc.raw(*MD[:2]), True), npref.leaf(exc.raw(*MI[:2]), False)
            ex = ref.Exact(ys, xs)
            rows = np.arange(n)
            worst, widest = 0.0, 0
            for f in fl:
                left, right, emp = exc.base(*f)
                l, r = np.where(emp, 1, left), np.where(emp, 0, right)
                widest = max(widest, int((r - l + 1).max()))
                cols = {(op, which): seen[(OP[op],) + m[which][0] + m[which][1] + f] for op, which in COLUMNS}
                worst = max(worst, check_bound(ex, cols, rows, l, r, (name, f)))
            assert widest >= (2 * T + 15 if name != "heavy ties" else n // 8)
            print("PRINTED window moments on tie runs: worst error / bound at n = %d, %s = %.4f (widest frame %d rows)" % (n, name, worst, widest))
            assert worst < 1.0
        finally:
            t.free()


# 5. wide calls and the measure bookkeeping --------------------------------------------------------------------------------------------------
def _distinct(cols):
    """(distinct measures, distinct unordered pairs of different measures) a call's bookkeeping holds: VAR_* / STDDEV_* read Y alone"""
    meas, pairs = [], set()
    for c in cols:
        y, x = tuple(c[1:4]), tuple(c[4:7])
        two = c[0] >= OP["covar_pop"]
        for m in (y, x) if two else (y,):
            if m not in meas:
                meas.append(m)
        if two and x != y:
            pairs.add(frozenset((y, x)))
    return len(meas), len(pairs)


def _alone(ctx, t, terms, npart, cols, seen, min_hits=0):
    """each column alone in a call: the same bits — the trees are shared, the values are not touched"""
    for col in cols:
        a = ctx.table_window_moments(t, min_hits, npart, terms, [col], ALL, len(seen[col]), want_hits=False)[4][0]
        assert (npref.bits(a) == npref.bits(seen[col])).all(), col


def _near(k):
    """the bits of the doubles 2^30 + k / 4, as int64: finite and ordinary read either way"""
    return (float(1 << 30) + np.asarray(k) / 4.0).view(np.int64)


@pytest.mark.parametrize("size", ["T+9", "3T+5"])
def test_wide_calls(hip_engine, size):
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = T + 9 if size == "T+9" else 3 * T + 5
    rng = np.random.default_rng(n + 11)
    # every payload holds the bits of doubles beside 2^30: each is a measure as the integer and as the double; one partition (npartition 0)
    q = 1 << 20                                                            # a quarter, in ulps of those doubles: the VALUE offsets over the integer order term
    t = _range_table(ctx, _near(rng.integers(0, 3, n)), _near(rng.integers(0, max(2, n // 6), n)), (float(1 << 30) + rng.integers(0, 64, n) / 4.0), _near(rng.integers(-8, 8, n) * 4))
    try:
        terms = [(P, 1, True, False)]
        eight = [(OP["covar_pop"], K, 0, False, P, 0, False, ROWS, -19, 0), (OP["corr"], P, 0, True, P, 1, True, GRP, -1, 1),
                 (OP["regr_slope"], P, 2, True, P, 2, False, VAL, -3 * q, q), (OP["regr_intercept"], P, 3, False, P, 3, True, GRP, None, 0)]
        assert _distinct(eight) == (8, 4) == (2 * abi.WM_MAX_COLS, abi.WM_MAX_COLS)
        done, exc, seen = _check(ctx, t, terms, 0, ("eight measures", n), [eight])
        assert done == 4 and all(np.isfinite(a).sum() > n // 2 for a in seen.values())
        assert all(ends[:2] == [True, True] for ends in differs_from_rows(exc, None, eight).values())      # both ends of a VALUE and a GROUPS frame are not the ROWS frame's
        _alone(ctx, t, terms, 0, eight, seen)
        # four columns, two measures: one C tree asked for in both orders, C = Q where Y is X
        y, x = (P, 2, True), (P, 3, True)
        shared = [(OP["covar_pop"],) + y + x + (GRP, -1, 1), (OP["corr"],) + x + y + (GRP, -1, 1), (OP["regr_slope"],) + x + x + (ROWS, -1, 0), (OP["var_pop"],) + y + y + (VAL, -2 * q, 0)]
        assert _distinct(shared) == (2, 1)
        done, exc, seen = _check(ctx, t, terms, 0, ("two measures", n), [shared])
        slope = seen[shared[2]]
        null = npref.bits(slope) == npref.NULL_BITS
        assert (slope[~null] == 1.0).all() and 0 < null.sum() < n // 4     # REGR_SLOPE(x, x) = C / Q = Q / Q: 1.0 exactly wherever Q != 0
        _alone(ctx, t, terms, 0, shared, seen)
        # pairs (0, 1), (1, 2) and (0, 2): the last asked for as (2, 0)
        m0, m1, m2 = (K, 0, False), (P, 2, True), (P, 3, True)
        mixed = [(OP["covar_samp"],) + m0 + m1 + (ROWS, -19, 0), (OP["corr"],) + m1 + m2 + (GRP, -2, 0), (OP["regr_intercept"],) + m2 + m0 + (VAL, -q, q), (OP["stddev_pop"],) + m2 + m2 + (ROWS, None, None)]
        assert _distinct(mixed) == (3, 3)
        done, exc, seen = _check(ctx, t, terms, 0, ("three pairs", n), [mixed])
        _alone(ctx, t, terms, 0, mixed, seen)
    finally:
        t.free()
    # an accumulating table: KEY, VALUE and HITS as measures, (KEY, HITS) asked for in both orders; min_hits 2 drops the rows hit once
    part, value, hits = _pattern("runs", n, T, rng)
    value = value + rng.integers(0, 4, n) / 4.0
    t = _table(ctx, part, value, hits)
    try:
        terms = [(P, 0, False, False), (V, 0, True, True)]
        k, v, h = (K, 0, False), (V, 0, True), (H, 0, False)
        cols = [(OP["covar_samp"],) + k + v + (ROWS, -5, 3), (OP["corr"],) + h + k + (GRP, -2, 2), (OP["regr_slope"],) + v + h + (VAL, -3.0, 3.5), (OP["regr_intercept"],) + k + h + (GRP, None, 0)]
        assert _distinct(cols) == (3, 3)
        kept = []
        for min_hits in (0, 2):
            done, exc, seen = _check(ctx, t, terms, 1, ("key, value, hits", n, min_hits), [cols], min_hits=min_hits)
            assert done == 4 and all(np.isfinite(a).sum() > exc.n // 2 for a in seen.values())
            _alone(ctx, t, terms, 1, cols, seen, min_hits=min_hits)
            kept.append(exc.n)
        assert kept[0] == n and n // 2 < kept[1] < n - n // 8
    finally:
        t.free()


# 6. through the decorator, over an order with ties ------------------------------------------------------------------------------------------
def test_q3_on_the_decorator_with_a_tied_order(on_the_decorator, db, monkeypatch):
    """rolling over (PARTITION BY o_shippriority ORDER BY o_orderdate): many orders share a date, and every column is a GROUPS or a
    VALUE frame, bounded or unbounded on one side — a frame is then a SET of rows, whatever the order inside a tie run.  The device
    route and the host route are each checked against exact rationals of that set within their own bound (the header's for the
    device, the two-pass one for the host).  The two routes are NOT compared by bits: their row orders inside a tie run, and so
    their leaf orders, may differ."""
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_shippriority"], [("o_orderdate", "asc")]
    aggs = {"vol": ("stddev_samp", "revenue", -6, 0, "groups"), "beta": ("regr_slope", "revenue", "l_orderkey", -100, 100, "value"),
            "run": ("var_pop", "revenue", None, 0, "groups"), "ahead": ("corr", "revenue", "l_orderkey", 1, None, "value")}
    dev = Q.q3.rolling(by, order, aggs)(*args)
    note = eng.stats()["order_routes"][-1]
    assert note["route"] == "window_moments" and note["calls"] == 1 and note["per"] == by and [a[0] for a in note["aggs"]] == list(aggs), note
    assert {a[4] for a in note["aggs"]} == {"groups", "value"}
    monkeypatch.setattr(eng, "device_window_moments", False)
    host = Q.q3.rolling(by, order, aggs)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["calls"] == 0
    monkeypatch.setattr(eng, "device_window_moments", True)
    n = len(dev)
    assert n > 100 and len(host) == n and dev.columns == host.columns and dev.columns[-4:] == list(aggs)
    worst = {}
    for route, res, two_pass in (("device", dev, False), ("host", host, True)):
        prio, date = np.asarray(res.column("o_shippriority")), np.asarray(res.column("o_orderdate"))
        assert ((prio[1:] > prio[:-1]) | ((prio[1:] == prio[:-1]) & (date[1:] >= date[:-1]))).all() and (date[1:] == date[:-1]).sum() > n // 10      # ordered, with ties
        ys, xs = np.asarray(res.column("revenue"), np.float64), np.asarray(res.column("l_orderkey"), np.float64)
        worst[route], nulls = 0.0, 0
        for j in sorted(set(range(0, n, max(1, n // 40))) | {0, 1, n - 2, n - 1}):
            same = prio == prio[j]
            rank = np.searchsorted(np.unique(date[same]), date)
            for name, (op, *_, lo, hi, unit) in aggs.items():
                at = rank if unit == "groups" else date
                inside = same & (at >= (at[j] + lo if lo is not None else at.min())) & (at <= (at[j] + hi if hi is not None else at.max()))
                got = np.float64(res.column(name)[j])
                if not inside.any():
                    nulls += 1
                    assert int(got.view(np.uint64)) == npref.NULL_BITS, (route, name, j)
                    continue
                e = mref.Exact(ys[inside], xs[inside] if op in npref.BI else None)
                want, theirs = e.value(op)
                if want is None:
                    nulls += 1
                    assert int(got.view(np.uint64)) == npref.NULL_BITS, (route, name, j)
                    continue
                bound = theirs if two_pass else ref.FrameExact(e.m, e.muy, e.qy, e.ay, *((e.mux, e.qx, e.c, e.ax, e.abs_c) if op in npref.BI else ())).value(op)[1]
                assert abs(float(got) - want) <= bound, (route, name, j, float(got), want, bound)
                worst[route] = max(worst[route], abs(float(got) - want) / bound if bound else 0.0)
        assert nulls > 0                                                   # (nothing follows the last date of a priority)
    print("PRINTED window moments on q3 over a tied order: worst error / bound, device = %.4f, host = %.4f" % (worst["device"], worst["host"]))
