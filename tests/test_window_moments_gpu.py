"""VAR / STDDEV / COVAR / CORR / REGR over window frames on the MI355X (run with -m gpu): sdqh_table_window_moments
(include/sdqh_sort_wmoments.h) through the C ABI — by bits against the pinned fold restated in Python, within the header's bound
against exact rationals (window_moments_reference), the same frame spelled in three units, two calls, swapped measures, the NULLs,
whole partitions against sdqh_table_group_moments, a NaN row, the call's contract — and through the engine and the decorator against
the host route.  The cases are test_window_moments_cpu's.  Nothing is imported from the product's fold code.
PRINTED: every case prints its worst error / bound ratio."""
import ctypes as C

import numpy as np
import pytest

import moments_reference as mref
import window_moments_reference as ref
from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import MOMENT_OPS
from test_group_moments_gpu import PACK, _mo_table, _terms
from test_window_gpu import db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)
from test_window_moments_cpu import CASES, COLUMNS, TILE, check_bound, data, frame_ends, frames, partition_column, restated, sample_rows

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
P = abi.SORT_PAYLOAD
MYD, MXD, MXI = (P, 1, True), (P, 2, True), (P, 3, False)                 # the double measure y; x as doubles and as the integers it holds
NULL = ref.NULL_BITS
OP = {name: i for i, name in enumerate(MOMENT_OPS)}
UNIT = {"value": abi.WRANGE_VALUE, "groups": abi.WRANGE_GROUPS, "rows": abi.WEX_ROWS}
MEASURES = {"y": (MYD, MYD), "x": (MXI, MXI), "yx": (MYD, MXI)}


def _col(op, which, unit, lo, hi):
    y, x = MEASURES[which] if isinstance(which, str) else which
    return (OP[op],) + y + x + (UNIT[unit], lo, hi)


def _build(ctx, part, y, x, seed=0):
    """the table of a case in a shuffled build order: payload 0 = partition * PACK + sorted position (the two terms), 1 = y, 2 = x as
    doubles, 3 = x as integers"""
    n = len(part)
    assert n < PACK
    mix = np.random.default_rng(seed + n).permutation(n)
    ab = part * PACK + np.arange(n, dtype=np.int64)
    return _mo_table(ctx, ab[mix], y[mix], x[mix], x[mix].astype(np.int64))


def _device(ctx, t, cols, n):
    """the columns `cols`, four a call, every call's rows in sorted order"""
    out = []
    for i in range(0, len(cols), abi.WM_MAX_COLS):
        r = ctx.table_window_moments(t, 0, 1, _terms(False), cols[i:i + abi.WM_MAX_COLS], ALL, n + 1, want_hits=False)
        assert len(r[0]) == n and (np.diff(r[1][0]) > 0).all() and all(c.dtype == np.float64 and len(c) == n for c in r[4])
        out += r[4]
    return out


def _geometry(ctx):
    T = ctx.window_moments_geometry()
    assert T == ctx.window_exclude_geometry()[0] == ctx.group_moments_geometry() == TILE
    return T


# 1. bits equal the restatement, values within the bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", CASES)
def test_bits_and_bound(hip_engine, n, kind):
    """Every op over the double and the integer measure, every frame of the list: VAR_* / COVAR_* / REGR_* and the sqrt ops (STDDEV_*,
    CORR: the device's double sqrt is correctly rounded) bit for bit the pinned fold — every row up to 3 tiles + 5, sample_rows past 256
    tiles —, NULL bits on empty frames and single rows, and every finite result within the header's bound against exact."""
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    part = partition_column(kind, n, T)
    y, x = data(n)
    rows = np.arange(n) if n <= 3 * T + 5 else sample_rows(n, part, T)
    t = _build(ctx, part, y, x)
    try:
        fl = frames(T)
        got = _device(ctx, t, [_col(op, which, unit, lo, hi) for unit, lo, hi in fl for op, which in COLUMNS], n)
        if n == 0:
            return
        ex, tree = ref.Exact(y, x), ref.Tree(y, x)
        worst, empties = 0.0, 0
        for k, (unit, lo, hi) in enumerate(fl):
            l, r = frame_ends(part, lo, hi)
            empties += int((l > r).sum())
            cols = {col: got[k * len(COLUMNS) + i][rows] for i, col in enumerate(COLUMNS)}
            want = restated(tree, rows, l, r)
            for col in COLUMNS:
                same = mref.bits(cols[col]) == mref.bits(want[col])
                assert same.all(), (n, kind, unit, lo, hi, col, rows[~same][:5], cols[col][~same][:5], want[col][~same][:5])
            worst = max(worst, check_bound(ex, cols, rows, l, r, (n, kind, unit, lo, hi)))
        assert empties > 0                                                   # ([2, 5] at every partition's end)
        print("PRINTED window moments on the device: worst error / bound at n = %d, %s = %.4f" % (n, kind, worst))
        assert worst < 1.0
    finally:
        t.free()


# 2. one frame, three units; two calls; swapped measures -------------------------------------------------------------------------------------
def test_units_determinism_and_symmetry(hip_engine):
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = 3 * T + 5
    rng = np.random.default_rng(11)
    part = partition_column("tile end", n, T)
    y, x = 1e6 + rng.standard_normal(n), rng.standard_normal(n) * 1e-3 + 0.1          # general doubles: nothing is exact
    t = _build(ctx, part, y, x)
    try:
        for lo, hi in ((-5, 3), (None, 0), (-(T + 7), 3), (None, None)):
            for op in ("var_samp", "stddev_pop", "corr", "regr_intercept"):
                a, b, c = _device(ctx, t, [_col(op, (MYD, MXD), unit, lo, hi) for unit in ("rows", "value", "groups")], n)
                assert (mref.bits(a) == mref.bits(b)).all() and (mref.bits(a) == mref.bits(c)).all(), (op, lo, hi)      # the association is l's and r's alone
        cols = [_col("covar_pop", (MYD, MXD), "rows", -19, 0), _col("covar_pop", (MXD, MYD), "rows", -19, 0), _col("corr", (MYD, MXD), "rows", -19, 0), _col("corr", (MXD, MYD), "rows", -19, 0),
                _col("covar_samp", (MYD, MXD), "rows", None, 0), _col("covar_samp", (MXD, MYD), "rows", None, 0), _col("covar_pop", (MXD, MXD), "rows", -2, 2), _col("var_pop", (MXD, MXD), "rows", -2, 2)]
        got, again = _device(ctx, t, cols, n), _device(ctx, t, cols, n)
        assert all((mref.bits(p) == mref.bits(q)).all() for p, q in zip(got, again))                                    # two calls: no atomics
        for i in range(0, len(cols), 2):
            assert (mref.bits(got[i]) == mref.bits(got[i + 1])).all(), i
        assert np.isfinite(got[2]).sum() >= n - 8 and np.nanmax(np.abs(got[2])) <= 1.0                                  # (a partition's first row is NULL)
        # a column alone and the same column beside three others: the trees are shared, the bits are not touched
        alone = _device(ctx, t, cols[2:3], n)[0]
        assert (mref.bits(alone) == mref.bits(got[2])).all()
    finally:
        t.free()


# 3. the NULLs -------------------------------------------------------------------------------------------------------------------------------
def test_nulls(hip_engine):
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = T + 9
    y, x = data(n, 5)
    t = _build(ctx, partition_column("ones", n, T), y, x)                   # every row its own partition: m = 1 wherever a frame holds a row
    try:
        for lo, hi in ((-19, 0), (None, None), (0, 0)):
            got = _device(ctx, t, [_col(op, which, "rows", lo, hi) for op, which in COLUMNS], n)
            for (op, which), col in zip(COLUMNS, got):
                assert (mref.bits(col) == (0 if op in ("var_pop", "stddev_pop", "covar_pop") else NULL)).all(), (op, which, lo, hi)
        got = _device(ctx, t, [_col(op, which, "rows", 1, 3) for op, which in COLUMNS[:4] + COLUMNS[8:12]], n)      # nothing behind a single row: empty
        assert all((mref.bits(col) == NULL).all() for col in got)
    finally:
        t.free()
    # a constant column of integers: Q = +0.0 exactly, CORR / REGR over it NULL; a constant 0.1 may leave a tiny Q (the header says so)
    t = _build(ctx, partition_column("one", n, T), np.full(n, 7.0), x)
    try:
        var, corr, slope, back = _device(ctx, t, [_col("var_pop", "y", "rows", -19, 0), _col("corr", "yx", "rows", -19, 0), _col("regr_slope", "yx", "rows", -19, 0),
                                                  _col("regr_slope", (MXI, MYD), "rows", -19, 0)], n)
        assert (mref.bits(var) == 0).all() and (mref.bits(corr) == NULL).all() and (mref.bits(back) == NULL).all()
        assert mref.bits(slope)[0] == NULL and (slope[20:] == 0.0).all()
    finally:
        t.free()


# 4. a whole partition: sdqh_table_group_moments' group ---------------------------------------------------------------------------------------
def test_both_sides_unbounded_agrees_with_group_moments(hip_engine):
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = 3 * T + 5
    part = partition_column("tile end", n, T)
    y, x = data(n, 9)
    t = _build(ctx, part, y, x)
    try:
        starts, ends = ref.partition_ends(part)
        heads = np.unique(starts)
        groups = ref.Exact(y, x).frames(heads, ends[heads], abs_c=True)
        slot = np.searchsorted(heads, starts)
        ops = [("var_samp", "y"), ("stddev_pop", "y"), ("covar_pop", "yx"), ("corr", "yx"), ("regr_slope", "yx"), ("regr_intercept", "yx"), ("var_pop", "x"), ("stddev_samp", "x")]
        win = _device(ctx, t, [_col(op, which, "rows", None, None) for op, which in ops], n)
        for i in range(0, len(ops), 4):
            aggs = [(OP[op],) + MEASURES[which][0] + MEASURES[which][1] for op, which in ops[i:i + 4]]
            grp = ctx.table_group_moments(t, 0, _terms(False), 0b010, aggs, ALL, 64, want_hits=False)
            assert len(grp[0]) == len(heads)
            for (op, which), w, g in zip(ops[i:i + 4], win[i:i + 4], grp[4]):
                f = groups.swapped() if which == "x" else groups
                _, mine, null = ref.values(op, f)
                for j in range(len(heads)):
                    theirs = mref.Exact(y[heads[j]:ends[heads[j]] + 1] if which != "x" else x[heads[j]:ends[heads[j]] + 1], x[heads[j]:ends[heads[j]] + 1]).value(op)[1]
                    rows = slot == j
                    assert not null[j] and (mref.bits(w[rows]) == mref.bits(w[rows][:1])).all()                # one frame: one value
                    assert abs(w[rows][0] - g[j]) <= mine[j] + theirs, (op, which, j, w[rows][0], g[j], mine[j], theirs)
    finally:
        t.free()


# 5. a NaN row ---------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_poisons_exactly_the_frames_that_hold_it(hip_engine):
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = 2 * T + 40
    part = partition_column("tile end", n, T)
    y, x = data(n, 13)
    for at, bad in ((T - 6, np.nan), (T + 300, np.inf)):                  # (inside the partition that ends on tile 0's last position, and mid-tile)
        yy = y.copy()
        yy[at] = bad
        t = _build(ctx, part, yy, x)
        try:
            tree = ref.Tree(yy, x)
            rows = np.arange(n)
            for lo, hi in ((-19, 0), (-2, 2), (None, 0)):
                l, r = frame_ends(part, lo, hi)
                holds = (l <= at) & (at <= r)
                cols = [("var_pop", "y"), ("stddev_samp", "y"), ("covar_pop", "yx"), ("regr_slope", "yx"), ("var_pop", "x")]
                got = _device(ctx, t, [_col(op, which, "rows", lo, hi) for op, which in cols], n)
                want = restated(tree, rows, l, r)
                for (op, which), col in zip(cols, got):
                    if which == "x":                                                                # (x is clean)
                        assert np.isfinite(col).all()
                    if which != "x":
                        assert (~np.isfinite(col[holds])).all() and holds.sum() >= 3, (op, at, lo, hi)
                    clean = ~holds if which != "x" else np.ones(n, bool)
                    assert (mref.bits(col[clean]) == mref.bits(want[(op, which)][clean])).all(), (op, which, at, lo, hi)
        finally:
            t.free()


# 6. the call's contract -----------------------------------------------------------------------------------------------------------------------
def _raw(ctx, t, cols, limit, capacity, keys=None, out=None, npart=1, ncols=None, null_cols=False, terms=None):
    got = C.c_int64(-7)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    terms = _terms(False) if terms is None else terms
    arr = (abi.WindowMoment * max(1, len(cols)))()
    for i, (op, kind, index, is_f64, kind2, index2, is_f64_2, unit, lo, hi) in enumerate(cols):
        arr[i].op, arr[i].kind, arr[i].index, arr[i].is_f64, arr[i].kind2, arr[i].index2, arr[i].is_f64_2, arr[i].unit = op, kind, index, int(is_f64), kind2, index2, int(is_f64_2), unit
        arr[i].flags = (abi.WRANGE_LO_UNBOUNDED if lo is None else 0) | (abi.WRANGE_HI_UNBOUNDED if hi is None else 0)
        arr[i].lo, arr[i].hi = lo or 0, hi or 0
    rc = ctx.lib.sdqh_table_window_moments(ctx.handle, t.handle, C.c_int64(0), C.c_int(npart), C.c_int(len(terms)), abi._marshal_sort_terms(terms),
                                           C.c_int(len(cols) if ncols is None else ncols), None if null_cols else arr, C.c_int64(limit), C.c_int64(capacity),
                                           ptr(keys), None, None, None, ptr(out), C.byref(got))
    return rc, got.value


def test_sizes_errors_and_empties(hip_engine):
    ctx = hip_engine.ctx
    T = _geometry(ctx)
    n = T + 9
    part = partition_column("tile end", n, T)
    y, x = data(n, 17)
    t = _build(ctx, part, y, x)
    empty = _build(ctx, part[:0], y[:0], x[:0])
    try:
        cols = [_col("var_pop", "y", "rows", -19, 0), _col("corr", "yx", "groups", None, 2)]
        full = _device(ctx, t, cols, n)
        keys, out = np.full(n, -7, np.int64), np.full((2, n), -7, np.int64)
        assert _raw(ctx, t, cols, ALL, n - 1, keys, out) == (abi.ERR_OVERFLOW, n) and (keys == -7).all() and (out == -7).all()
        assert _raw(ctx, t, cols, 5, n, keys, out) == (abi.OK, 5) and (keys[5:] == -7).all() and (out[:, 5:] == -7).all()
        assert (out[0, :5] == mref.bits(full[0][:5]).view(np.int64)).all() and (out[1, :5] == mref.bits(full[1][:5]).view(np.int64)).all()      # frames look past `limit`
        assert _raw(ctx, t, cols, ALL, 0) == (abi.OK, n) and _raw(ctx, t, cols, 7, 0) == (abi.OK, 7)            # count only
        keys[:] = -7
        assert _raw(ctx, t, cols, ALL, n, keys, None) == (abi.OK, n) and (keys != -7).all()                         # rows only
        out[:] = -7
        assert _raw(ctx, t, cols, ALL, n, None, out) == (abi.OK, n)                                                 # columns only
        assert (out[0] == mref.bits(full[0]).view(np.int64)).all() and (out[1] == mref.bits(full[1]).view(np.int64)).all()
        assert _raw(ctx, empty, cols, ALL, 4, keys, out) == (abi.OK, 0)
        good = cols[0]
        bads = [dict(cols=[(-1,) + good[1:]]), dict(cols=[(9,) + good[1:]]), dict(cols=[good[:7] + (3, -1, 0)]), dict(cols=[good[:7] + (abi.WEX_ROWS, 1, 0)]),
                dict(cols=[_col("var_pop", ((P, 9, True),) * 2, "rows", -1, 0)]), dict(cols=[_col("corr", (MYD, (P, 9, True)), "rows", -1, 0)]),      # a measure the table lacks
                dict(cols=[_col("var_pop", ((abi.SORT_KEY, 0, True),) * 2, "rows", -1, 0)]), dict(cols=[_col("covar_pop", (MYD, (abi.SORT_HITS, 0, False)), "rows", -1, 0)]),
                dict(cols=[good[:7] + (abi.WRANGE_VALUE, -1, 1)], terms=_terms(False) + [(P, 3, False, False)]),      # a VALUE frame over two ORDER BY terms
                dict(ncols=0), dict(ncols=5), dict(null_cols=True), dict(npart=3), dict(limit=0), dict(capacity=-1)]
        for bad in bads:
            args = dict(cols=cols, limit=ALL, capacity=n, npart=1, ncols=None, null_cols=False, terms=None)
            args.update(bad)
            keys[:], out[:] = -7, -7
            rc = _raw(ctx, t, args["cols"], args["limit"], args["capacity"], keys, out, npart=args["npart"], ncols=args["ncols"], null_cols=args["null_cols"], terms=args["terms"])
            assert rc == (abi.ERR_INVALID, -7) and (keys == -7).all() and (out == -7).all(), (bad, rc)
        again = _device(ctx, t, cols, n)                                                                                # usable after the errors
        assert all((mref.bits(p) == mref.bits(q)).all() for p, q in zip(full, again))
        # VAR_* / STDDEV_* ignore X, unchecked: a second measure the table lacks changes nothing
        odd = _device(ctx, t, [_col("var_pop", (MYD, (P, 9, True)), "rows", -19, 0)], n)[0]
        assert (mref.bits(odd) == mref.bits(full[0])).all()
    finally:
        t.free()
        empty.free()


# 7. through the engine and the decorator ------------------------------------------------------------------------------------------------------
def test_q3_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_shippriority"], [("o_orderdate", "asc"), ("l_orderkey", "asc")]      # a unique order: the frames are the same rows on either route
    aggs = {"vol": ("stddev_samp", "revenue", -19, 0), "beta": ("regr_slope", "revenue", "l_orderkey", -19, 0), "all": ("var_pop", "revenue", None, None),
            "ahead": ("corr", "revenue", "l_orderkey", 1, 40, "groups")}
    rows = Q.q3.order_by([("o_shippriority", "asc")] + order)(*args)
    dev = Q.q3.rolling(by, order, aggs)(*args)
    note = eng.stats()["order_routes"][-1]
    assert note["route"] == "window_moments" and note["calls"] == 1 and note["per"] == by and [a[0] for a in note["aggs"]] == list(aggs), note
    monkeypatch.setattr(eng, "device_window_moments", False)                 # what SDQLPY_AMD_DEVICE_WINDOW_MOMENTS=0 sets
    host = Q.q3.rolling(by, order, aggs)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["calls"] == 0
    monkeypatch.setattr(eng, "device_window_moments", True)
    mine = rows.rolling(by, order, aggs)
    n = len(rows)
    assert n > 100 and dev.columns == host.columns == mine.columns == rows.columns + list(aggs) and len(dev) == len(host) == n
    assert [np.asarray(a).dtype for a in dev.arrays] == [np.asarray(a).dtype for a in host.arrays] and all(dev.column(c).dtype == np.float64 for c in aggs)
    for c in rows.columns:
        assert (np.asarray(dev.column(c)).astype(str) == np.asarray(rows.column(c)).astype(str)).all() and (np.asarray(host.column(c)).astype(str) == np.asarray(rows.column(c)).astype(str)).all(), c
    for c in aggs:
        assert (mref.bits(host.column(c)) == mref.bits(mine.column(c))).all(), c
    prio = np.asarray(rows.column("o_shippriority"))
    starts, ends = ref.partition_ends(prio)
    worst = 0.0
    for name, spec in aggs.items():
        op, ycol, xcol = spec[0], spec[1], spec[2] if op_two(spec[0]) else None
        lo, hi = spec[-3:-1] if isinstance(spec[-1], str) else spec[-2:]
        l, r = ref.rows_frames(n, starts, ends, lo, hi)                       # (unique order keys: a GROUPS frame is the ROWS frame)
        ys = np.asarray(rows.column(ycol), np.float64)
        xs = np.asarray(rows.column(xcol), np.float64) if xcol else None
        for j in sorted(set(range(0, n, max(1, n // 40))) | {0, n - 1, n - 2}):
            d, h = np.float64(dev.column(name)[j]), np.float64(host.column(name)[j])
            if l[j] > r[j]:
                assert int(d.view(np.uint64)) == NULL and int(h.view(np.uint64)) == NULL, (name, j)
                continue
            e = mref.Exact(ys[l[j]:r[j] + 1], None if xs is None else xs[l[j]:r[j] + 1])
            fe = ref.FrameExact(e.m, e.muy, e.qy, e.ay, *((e.mux, e.qx, e.c, e.ax, e.abs_c) if xs is not None else ()))
            want, theirs = e.value(op)
            _, bound = fe.value(op)
            if want is None:
                assert int(d.view(np.uint64)) == NULL and int(h.view(np.uint64)) == NULL, (name, j)
                continue
            assert abs(float(h) - want) <= theirs and abs(float(d) - want) <= bound, (name, j, float(d), float(h), want, bound, theirs)
            worst = max(worst, abs(float(d) - want) / bound if bound else 0.0)
    print("PRINTED window moments on q3: worst device error / bound = %.4f" % worst)
    five = dict(aggs, lo=("var_samp", "revenue", -3, 0))                      # more than four columns: on the host
    wide = Q.q3.rolling(by, order, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == rows.columns + list(five)


def op_two(op):
    return op in ref.BI
