"""Aggregates over window frames (over), the part that needs no GPU: the window aggregate extension's symbols
(include/sdqh_sort_frames.h, abi.WINDOW_AGG_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without
them, a compile-only context, ResultSet.over against a pure-Python reference (sort a list of tuples, walk it, running values in
Python integers / math.fsum), and the decorator surface on the CPU implementation's engine — the host route."""
import math
import os
import re
import struct

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import FRAMES, WAGG_OPS, FrameRequest, ResultSet, WindowRequest, frame_request
from test_window_cpu import NAN_A, NAN_B, SHAPES, _cases, _declared, _image, db, on_the_decorator      # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.WINDOW_AGG_EXPORTS) == _declared("sdqh_sort_frames.h") == ["sdqh_table_window_agg", "sdqh_window_agg_geometry"]
    for s in abi.WINDOW_AGG_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.EXTREMA_EXPORTS):
            assert s not in other
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_sort_window.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
    assert hip_lib.has_window_agg and hip_lib.has_window and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort_frames.h")).read()
    assert '#include "sdqh_sort_window.h"' in text
    for name, value in (("WAGG_SUM", abi.WAGG_SUM), ("WAGG_COUNT", abi.WAGG_COUNT), ("WAGG_MIN", abi.WAGG_MIN), ("WAGG_MAX", abi.WAGG_MAX),
                        ("FRAME_ROWS", abi.FRAME_ROWS), ("FRAME_RANGE", abi.FRAME_RANGE), ("FRAME_PARTITION", abi.FRAME_PARTITION), ("WAGG_MAX_AGGS", abi.WAGG_MAX_AGGS)):
        assert re.search(r"#define\s+SDQH_%s\s+%d\b" % (name, value), text), name
    assert (abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.FRAME_ROWS, abi.FRAME_RANGE, abi.FRAME_PARTITION, abi.WAGG_MAX_AGGS) == (0, 1, 2, 3, 0, 1, 2, 4)
    assert WAGG_OPS == ("sum", "count", "min", "max") and FRAMES == ("rows", "range", "partition")      # positions = the constants
    import ctypes as C
    assert C.sizeof(abi.WindowAgg) == 24 and [f for f, _ in abi.WindowAgg._fields_] == ["op", "frame", "kind", "index", "is_f64", "_pad"]
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sdqh.h")).read())


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_window_agg is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        call = lambda: ctx.table_window_agg(t, 0, 0, [(abi.SORT_KEY, 0, False, False)], [(abi.WAGG_COUNT, abi.FRAME_ROWS, abi.SORT_KEY, 0, False)], ALL, 16)
        for f in (call, ctx.window_agg_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no window aggregate extension" in str(e.value) and "libsdqloracle" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.window_agg_geometry() == ctx.window_geometry() >= 64    # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context
        terms = [(abi.SORT_KEY, 0, False, False)]
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_agg(table, 0, 0, terms, [(abi.WAGG_SUM, abi.FRAME_RANGE, abi.SORT_KEY, 0, False)], ALL, 16)
        assert e.value.code == abi.ERR_UNSUPPORTED
        for bad in ([(7, abi.FRAME_RANGE, abi.SORT_KEY, 0, False)], [(abi.WAGG_SUM, 3, abi.SORT_KEY, 0, False)], [], [(abi.WAGG_COUNT, 0, abi.SORT_KEY, 0, False)] * 5):
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_agg(table, 0, 0, terms, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, bad                    # the argument checks come first
    finally:
        ctx.close()


# ---- ResultSet.over against a walk over sorted tuples ----------------------------------------------------------------------------------
def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _wrap(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def _fold(op, vals):
    """The aggregate of a frame's values (in row order), by the header's rules, on Python values."""
    if op == "count":
        return len(vals)
    if isinstance(vals[0], int):
        return _wrap(sum(vals)) if op == "sum" else (min(vals) if op == "min" else max(vals))
    if op == "sum":
        if any(math.isnan(v) for v in vals) or (math.inf in vals and -math.inf in vals):
            return math.nan
        return math.fsum(vals)
    real = [v for v in vals if not math.isnan(v)]
    if not real:
        return NAN_A                                                       # the quiet NaN
    return (min if op == "min" else max)(real, key=lambda v: _image(v, False))     # the total order: -0.0 below +0.0


def _reference(columns, rows, by, order, aggs, k):
    """rows: list of tuples.  -> (row indices in order, {name: values}): sort (term images..., row index) tuples, walk them."""
    terms = [(b, "asc") if isinstance(b, str) else b for b in by] + list(order)
    text_rank = {}
    for name, _ in terms:
        j = columns.index(name)
        if rows and isinstance(rows[0][j], str):
            text_rank[name] = {s: i for i, s in enumerate(sorted({r[j] for r in rows}))}
    keyed = sorted((tuple(_image(text_rank[nm][r[columns.index(nm)]] if nm in text_rank else r[columns.index(nm)], d == "desc") for nm, d in terms), i)
                   for i, r in enumerate(rows))
    n = len(keyed)
    out = {name: [None] * n for name in aggs}
    a = 0
    while a < n:                                                           # a partition [a, b)
        b = a + 1
        while b < n and keyed[b][0][:len(by)] == keyed[a][0][:len(by)]:
            b += 1
        for name, (op, col, frame) in aggs.items():
            vals = [1 if col is None else rows[i][columns.index(col)] for _, i in keyed[a:b]]
            for p in range(a, b):
                if frame == "rows":
                    end = p
                elif frame == "partition":
                    end = b - 1
                else:                                                      # the last row tied with p
                    end = p
                    while end + 1 < b and keyed[end + 1][0] == keyed[p][0]:
                        end += 1
                out[name][p] = _fold(op, vals[:end - a + 1])
        a = b
    return [i for _, i in keyed][:k], {name: v[:k] for name, v in out.items()}


def _agg_cases():
    cases = dict(_cases())
    columns, arrays = cases["plain"]
    rng = np.random.default_rng(5)
    big = np.resize(np.array([0, I_MAX, -1, I_MIN, 1, I_MIN, I_MAX, 0, I_MIN + 1, I_MAX - 1, 1 << 32], np.int64), len(arrays[0]))[rng.permutation(len(arrays[0]))]
    cases["plain"] = (columns + ["big"], arrays + [big])
    cases["empty"] = (columns + ["big"], [a[:0] for a in cases["plain"][1]])
    cases["one row"] = (columns + ["big"], [a[:1] for a in cases["plain"][1]])
    return cases


def _same_value(op, got, want):
    if isinstance(want, float) and op == "sum":                            # (a sum's zero has either sign in math.fsum; a NaN any payload)
        return (math.isnan(got) and math.isnan(want)) or got == want
    return _bits(got) == _bits(want) if isinstance(want, float) else got == want


@pytest.mark.parametrize("case", ["plain", "empty", "one row"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_over_against_a_walk(case, shape):
    """Integers (with INT64_MIN / MAX: SUM wraps), integer-valued doubles (sums exact: np.cumsum = math.fsum), +-0.0 / NaN / inf, text
    partition and order columns, every op x frame, by = []; the first k rows."""
    columns, arrays = _agg_cases()[case]
    rs = ResultSet(columns, arrays)
    rows = list(zip(*[a.tolist() for a in arrays]))
    by, order = SHAPES[shape]
    if not by and not order:
        return
    done = 0
    for measure in ("g", "v", "h", "e", "big"):
        aggs = {"%s_%s" % (op, fr): (op, None if op == "count" else measure, fr) for op in WAGG_OPS for fr in FRAMES}
        assert len(aggs) == 12 > abi.WAGG_MAX_AGGS                         # the host takes any number
        for k in sorted({1, max(1, len(rows) // 2), ALL}):
            with np.errstate(invalid="ignore", over="ignore"):
                res = rs.framed(frame_request(columns, by, order, aggs, k=k))
            idx, want = _reference(columns, rows, by, order, aggs, k)
            assert res.columns == columns + list(aggs) and len(res) == len(idx)
            for c, a in zip(columns, arrays):
                got = res.column(c)
                assert got.dtype == a.dtype and all(_same_value("", x, rows[i][columns.index(c)]) for x, i in zip(got.tolist(), idx)), c
            for nm, (op, col, fr) in aggs.items():
                got = res.column(nm)
                is_f = col is not None and arrays[columns.index(col)].dtype.kind == "f"
                assert got.dtype == (np.float64 if is_f else np.int64), nm
                bad = [(j, x, w) for j, (x, w) in enumerate(zip(got.tolist(), want[nm])) if not _same_value(op, x, w)]
                assert not bad, (by, order, measure, nm, k, bad[:3])
                done += 1
    assert done >= 5 * 12 * (1 if case != "plain" else 3)


def test_over_on_a_result_set_and_its_argument_errors():
    columns, arrays = _agg_cases()["plain"]
    rs = ResultSet(columns, arrays)
    res = rs.over(["g"], [("v", "desc")], {"running": ("sum", "v"), "total": ("sum", "v", "partition"), "n": ("count", None, "partition"), "best": ("max", "h", "rows")})
    assert res.columns == columns + ["running", "total", "n", "best"] and len(res) == len(rs)
    assert [res.column(c).dtype for c in ("running", "total", "n", "best")] == [np.float64, np.float64, np.int64, np.int64]
    g, v = res.column("g"), res.column("v")
    for grp in np.unique(g):                                               # the default frame is RANGE: peers share the run's last value
        sel = g == grp
        assert (res.column("n")[sel] == sel.sum()).all() and (res.column("total")[sel] == v[sel].sum()).all()
        run = res.column("running")[sel]
        assert run[-1] == v[sel].sum() and all(run[i] == run[i + 1] for i in range(sel.sum() - 1) if v[sel][i] == v[sel][i + 1])
    rows_frame = rs.over(["g"], [("v", "desc")], {"running": ("sum", "v")}, frame="rows")
    assert (rows_frame.column("running") != res.column("running")).any()
    ok = {"x": ("sum", "v")}
    for call, exc in ((lambda: rs.over(["g"], [("v", "desc")], {"x": ("avg", "v")}), ValueError), (lambda: rs.over(["g"], [("v", "desc")], {"x": ("sum", "v", "groups")}), ValueError),
                      (lambda: rs.over(["g"], [("v", "desc")], ok, frame="groups"), ValueError), (lambda: rs.over(["g"], [("v", "desc")], {"x": ("sum", None)}), ValueError),
                      (lambda: rs.over(["g"], [("v", "desc")], {}), ValueError), (lambda: rs.over(["g"], [("v", "desc")], {"x": ("sum",)}), ValueError),
                      (lambda: rs.over(["g"], [("v", "desc")], {"x": ("sum", "s")}), ValueError), (lambda: rs.over(["g"], [("v", "down")], ok), ValueError),
                      (lambda: rs.over([], [], ok), ValueError), (lambda: rs.over(["g"], [("v", "desc")], {"h": ("sum", "v")}), KeyError),
                      (lambda: rs.over(["g"], [("v", "desc")], {"x": ("sum", "nope")}), KeyError), (lambda: rs.over(["nope"], [("v", "desc")], ok), KeyError)):
        with pytest.raises(exc):
            call()


def test_the_request_reads_as_a_top_and_travels_as_a_window():
    req = frame_request(None, ["a"], [("b", "desc")], {"t": ("sum", "b"), "n": ("count", None, "partition")})
    assert isinstance(req, FrameRequest) and isinstance(req, WindowRequest) and isinstance(req, tuple) and len(req) == 2
    assert (req[0], req[1]) == (ALL, [("a", "asc"), ("b", "desc")]) and req.by == [("a", "asc")] and req.order == [("b", "desc")] and req.npartition == 1
    assert req.aggs == [("t", "sum", "b", "range"), ("n", "count", None, "partition")] and req.name is None
    again = req.renamed([("x", "asc"), ("y", "desc")], {"b": "y"})
    assert isinstance(again, FrameRequest) and again[1] == [("x", "asc"), ("y", "desc")] and again.aggs == [("t", "sum", "y", "range"), ("n", "count", None, "partition")]
    assert req.renamed(req[1]).aggs == req.aggs
    from sdqlpy_amd import dist as sdist
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(req)
    assert "over" in str(e.value)


# ---- through the decorator on the CPU implementation's engine: the host route -------------------------------------------------------
Q3_AGGS = {"running": ("sum", "revenue"), "day_total": ("sum", "revenue", "partition"), "n": ("count", None, "partition"), "best": ("max", "revenue", "rows")}


def test_q3_on_the_host_route(on_the_decorator, db):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    res = Q.q3.over(by, order, Q3_AGGS)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by,
                                               "aggs": [["running", "sum", "revenue", "range"], ["day_total", "sum", "revenue", "partition"],
                                                        ["n", "count", None, "partition"], ["best", "max", "revenue", "rows"]]}
    assert res.columns == plain.columns + list(Q3_AGGS) and len(res) == len(plain) > 300
    assert [res.column(c).dtype for c in Q3_AGGS] == [np.float64, np.float64, np.int64, np.float64]
    dates, rev = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
    assert (dates[1:] >= dates[:-1]).all()
    for d in np.unique(dates):
        sel = np.nonzero(dates == d)[0]
        x = rev[sel]
        assert (x[1:] <= x[:-1]).all() and (res.column("n")[sel] == len(sel)).all()
        run = np.cumsum(x)
        last = np.array([np.nonzero(x == v)[0][-1] for v in x])            # the last row tied with each
        assert (res.column("running")[sel] == run[last]).all() and (res.column("day_total")[sel] == run[-1]).all()
        assert (res.column("best")[sel] == x[0]).all()
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_argument_errors_come_before_anything_is_launched(on_the_decorator, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("launched")
    monkeypatch.setattr(engine, "execute_plan", never)
    by, order, ok = ["o_orderdate"], [("revenue", "desc")], {"x": ("sum", "revenue")}
    for call, exc in ((lambda: Q.q3.over(by, order, {"x": ("avg", "revenue")}), ValueError), (lambda: Q.q3.over(by, order, {"x": ("sum", "revenue", "groups")}), ValueError),
                      (lambda: Q.q3.over(by, order, ok, frame="groups"), ValueError), (lambda: Q.q3.over(by, order, {"x": ("min", None)}), ValueError),
                      (lambda: Q.q3.over(by, order, {}), ValueError), (lambda: Q.q3.over(by, [("revenue", "down")], ok), ValueError),
                      (lambda: Q.q3.over(by, order, {"revenue": ("sum", "revenue")}), KeyError), (lambda: Q.q3.over(by, order, {"x": ("sum", "revenu")}), KeyError),
                      (lambda: Q.q3.over(["o_orderdat"], order, ok), KeyError), (lambda: Q.q3.over(by, [("revenu", "desc")], ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert callable(Q.q3.over(by, order, ok)) and callable(Q.q3.over([], order, dict(ok, n=("count", None))))      # nothing runs until it is called
