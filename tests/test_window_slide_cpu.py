"""Sliding window frames (sliding), the part that needs no GPU: the window slide extension's symbols (include/sdqh_sort_slide.h,
abi.WINDOW_SLIDE_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without them, a compile-only
context, ResultSet.sliding against a pure-Python reference (sort a list of tuples, walk it, fold every frame's slice in Python
integers / math.fsum), and the decorator surface on the CPU implementation's engine — the host route."""
import math
import os
import re
import struct

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import SLIDE_OPS, FrameRequest, ResultSet, SlideRequest, WindowRequest, slide_request
from test_window_cpu import NAN_A, NAN_B, SHAPES, _cases, _declared, _image, db, on_the_decorator      # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
FRAMES = [(-1, -1), (1, 1), (0, 0), (-2, 0), (0, 2), (-3, 4), (-5, -3), (2, 6), (None, 0), (0, None), (None, None), (-10 ** 18, 10 ** 18)]
U = 2.0 ** -53


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.WINDOW_SLIDE_EXPORTS) == _declared("sdqh_sort_slide.h") == ["sdqh_table_window_slide", "sdqh_window_slide_geometry"]
    for s in abi.WINDOW_SLIDE_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.WINDOW_AGG_EXPORTS, abi.EXTREMA_EXPORTS):
            assert s not in other
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_sort_window.h", "sdqh_sort_frames.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
    assert hip_lib.has_window_slide and hip_lib.has_window_agg and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort_slide.h")).read()
    assert '#include "sdqh_sort_frames.h"' in text
    for name, value in (("WSLIDE_FIRST", abi.WSLIDE_FIRST), ("WSLIDE_LAST", abi.WSLIDE_LAST), ("WSLIDE_MAX_AGGS", abi.WSLIDE_MAX_AGGS)):
        assert re.search(r"#define\s+SDQH_%s\s+%d\b" % (name, value), text), name
    assert re.search(r"#define\s+SDQH_SLIDE_UNBOUNDED_PRECEDING\s+INT64_MIN\b", text) and re.search(r"#define\s+SDQH_SLIDE_UNBOUNDED_FOLLOWING\s+INT64_MAX\b", text)
    assert (abi.WSLIDE_FIRST, abi.WSLIDE_LAST, abi.WSLIDE_MAX_AGGS, abi.SLIDE_UNBOUNDED_PRECEDING, abi.SLIDE_UNBOUNDED_FOLLOWING) == (4, 5, 4, I_MIN, I_MAX)
    assert SLIDE_OPS == ("sum", "count", "min", "max", "first", "last")                   # positions = the constants
    assert SLIDE_OPS[:4] == ("sum", "count", "min", "max") and (abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX) == (0, 1, 2, 3)
    import ctypes as C
    assert C.sizeof(abi.WindowSlide) == 40 and [f for f, _ in abi.WindowSlide._fields_] == ["op", "kind", "index", "is_f64", "lo", "hi", "empty"]
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sdqh.h")).read())


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_window_slide is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        call = lambda: ctx.table_window_slide(t, 0, 0, [(abi.SORT_KEY, 0, False, False)], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, -1, 0, 0)], ALL, 16)
        for f in (call, ctx.window_slide_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no window slide extension (include/sdqh_sort_slide.h)" in str(e.value) and "libsdqloracle" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        tile, narrow = ctx.window_slide_geometry()                         # (asks nothing of a device)
        assert tile == ctx.window_geometry() == ctx.window_agg_geometry() >= 64 and narrow >= 0
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context
        terms = [(abi.SORT_KEY, 0, False, False)]
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_slide(table, 0, 0, terms, [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, -2, 0, 0)], ALL, 16)
        assert e.value.code == abi.ERR_UNSUPPORTED
        one = (abi.WAGG_COUNT, abi.SORT_KEY, 0, False, -1, 1, 0)
        for bad in ([(6, abi.SORT_KEY, 0, False, -1, 1, 0)], [(-1, abi.SORT_KEY, 0, False, -1, 1, 0)], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, 1, 0, 0)], [], [one] * 5):
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_slide(table, 0, 0, terms, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, bad                    # the argument checks come first
    finally:
        ctx.close()


# ---- ResultSet.sliding against a walk over sorted tuples --------------------------------------------------------------------------------
def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _wrap(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def _fold(op, vals):
    """The value of a non-empty frame's values (in row order), by the header's rules, on Python values."""
    if op == "count":
        return len(vals)
    if op in ("first", "last"):
        return vals[0 if op == "first" else -1]
    if isinstance(vals[0], int):
        return _wrap(sum(vals)) if op == "sum" else (min(vals) if op == "min" else max(vals))
    real = [v for v in vals if v == v]
    if op == "sum":
        if len(real) < len(vals) or (math.inf in vals and -math.inf in vals):
            return math.nan
        return math.fsum(vals)
    if not real:
        return NAN_A                                                       # the quiet NaN
    return (min if op == "min" else max)(real, key=lambda v: _image(v, False))     # the total order: -0.0 below +0.0


def _normal(spec):
    """(op, col, lo, hi, default or None) of an aggregate as `sliding` takes it: lag / lead are `first` over one row."""
    if spec[0] in ("lag", "lead"):
        k = -spec[2] if spec[0] == "lag" else spec[2]
        return ("first", spec[1], k, k, spec[3] if len(spec) == 4 else None)
    return tuple(spec) + ((None,) if len(spec) == 4 else ())


def _reference(columns, rows, by, order, aggs):
    """rows: list of tuples.  -> (row indices in order, {name: values}): sort (term images..., row index) tuples, walk them; the
    frame of position p in the partition [a, b) is [max(p + lo, a), min(p + hi, b - 1)]."""
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
        for name, spec in aggs.items():
            op, col, lo, hi, default = _normal(spec)
            vals = [1 if col is None else rows[i][columns.index(col)] for _, i in keyed[a:b]]
            if default is None:
                default = NAN_A if isinstance(vals[0], float) else 0
            elif isinstance(vals[0], float):
                default = float(default)
            for p in range(a, b):
                left = a if lo is None else max(p + lo, a)
                right = b - 1 if hi is None else min(p + hi, b - 1)
                if left > right:
                    out[name][p] = 0 if op == "count" else default
                else:
                    out[name][p] = _fold(op, vals[left - a:right - a + 1])
        a = b
    return [i for _, i in keyed], out


def _slide_cases():
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


def _aggs_of(measure, is_f):
    """Every op over every frame of FRAMES, lag / lead, defaults given and implied — about eighty columns: the host takes any number."""
    given = 2.5 if is_f else -7
    aggs = {}
    for i, (lo, hi) in enumerate(FRAMES):
        for op in SLIDE_OPS:
            col = None if op == "count" else measure
            aggs["%s_%d" % (op, i)] = (op, col, lo, hi) if (i + len(op)) % 2 else (op, col, lo, hi, given)
    aggs.update(lag1=("lag", measure, 1), lag0=("lag", measure, 0), lag3=("lag", measure, 3, given), lead1=("lead", measure, 1), lead5=("lead", measure, 5, given),
                lead_far=("lead", measure, 10 ** 18), wide_count=("count", None, -40, 40), wide_sum=("sum", measure, -40, 40), wide_min=("min", measure, -33, 0))
    return aggs


@pytest.mark.parametrize("case", ["plain", "empty", "one row"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_sliding_against_a_walk(case, shape):
    """Integers (with INT64_MIN / MAX: SUM wraps), integer-valued doubles (sums exact: any association = math.fsum), +-0.0 / NaN /
    inf, text partition and order columns, every op x frame, lag / lead, by = []; the first k rows of frames that look past k."""
    columns, arrays = _slide_cases()[case]
    rs = ResultSet(columns, arrays)
    rows = list(zip(*[a.tolist() for a in arrays]))
    by, order = SHAPES[shape]
    if not by and not order:
        return
    done = 0
    for measure in ("v", "h", "e", "big"):
        is_f = arrays[columns.index(measure)].dtype.kind == "f"
        aggs = _aggs_of(measure, is_f)
        assert len(aggs) > 70 > abi.WSLIDE_MAX_AGGS
        idx_all, want_all = _reference(columns, rows, by, order, aggs)
        for k in sorted({1, max(1, len(rows) // 2), ALL}):
            with np.errstate(invalid="ignore", over="ignore"):
                res = rs.slid(slide_request(columns, by, order, aggs, k=k))
            idx = idx_all[:k]
            assert res.columns == columns + list(aggs) and len(res) == len(idx)
            for c, a in zip(columns, arrays):
                got = res.column(c)
                assert got.dtype == a.dtype and all(_same_value("", x, rows[i][columns.index(c)]) for x, i in zip(got.tolist(), idx)), c
            for nm, spec in aggs.items():
                op, col = _normal(spec)[:2]
                got = res.column(nm)
                assert got.dtype == (np.float64 if is_f and op != "count" else np.int64), nm
                bad = [(j, x, w) for j, (x, w) in enumerate(zip(got.tolist(), want_all[nm][:k])) if not _same_value(op, x, w)]
                assert not bad, (by, order, measure, nm, spec, k, bad[:3])
                done += 1
    assert done >= 4 * 70 * (1 if case != "plain" else 3)


def test_sliding_on_a_result_set_and_its_argument_errors():
    columns, arrays = _slide_cases()["plain"]
    rs = ResultSet(columns, arrays)
    by, order = ["g"], [("v", "desc")]
    res = rs.sliding(by, order, {"prev": ("lag", "v", 1), "nxt": ("lead", "h", 1, -1), "ma3": ("sum", "v", -2, 0), "n3": ("count", None, -2, 0), "lo3": ("min", "h", 0, 2)})
    assert res.columns == columns + ["prev", "nxt", "ma3", "n3", "lo3"] and len(res) == len(rs)
    assert [res.column(c).dtype for c in ("prev", "nxt", "ma3", "n3", "lo3")] == [np.float64, np.int64, np.float64, np.int64, np.int64]
    g, v, h = res.column("g"), res.column("v"), res.column("h")
    for grp in np.unique(g):
        sel = np.nonzero(g == grp)[0]
        x, y, m = v[sel], h[sel], len(sel)
        assert math.isnan(res.column("prev")[sel][0]) and (res.column("prev")[sel][1:] == x[:-1]).all()
        assert res.column("nxt")[sel][-1] == -1 and (res.column("nxt")[sel][:-1] == y[1:]).all()
        assert (res.column("n3")[sel] == np.minimum(np.arange(m) + 1, 3)).all()
        assert all(res.column("ma3")[sel][i] == x[max(0, i - 2):i + 1].sum() for i in range(m))       # (integer-valued: exact)
        assert all(res.column("lo3")[sel][i] == y[i:i + 3].min() for i in range(m))
    ok = {"x": ("sum", "v", -1, 1)}
    for call, exc in ((lambda: rs.sliding(by, order, {"x": ("avg", "v", -1, 1)}), ValueError), (lambda: rs.sliding(by, order, {"x": ("sum", "v", 1, 0)}), ValueError),
                      (lambda: rs.sliding(by, order, {"x": ("sum", "v", -1.0, 1)}), ValueError), (lambda: rs.sliding(by, order, {"x": ("sum", "v", "1", 2)}), ValueError),
                      (lambda: rs.sliding(by, order, {"x": ("lag", "v", -1)}), ValueError), (lambda: rs.sliding(by, order, {"x": ("lead", "v", 1.5)}), ValueError),
                      (lambda: rs.sliding(by, order, {"x": ("sum", None, -1, 1)}), ValueError), (lambda: rs.sliding(by, order, {"x": ("first", None, 0, 0)}), ValueError),
                      (lambda: rs.sliding(by, order, {"x": ("sum", "s", -1, 1)}), ValueError), (lambda: rs.sliding(by, order, {"x": ("first", "s", 0, 0)}), ValueError),
                      (lambda: rs.sliding(by, order, {"x": ("lag", "h", 1, 0.5)}), ValueError), (lambda: rs.sliding(by, order, {"x": ("lag", "h", 1, 1 << 63)}), ValueError),
                      (lambda: rs.sliding(by, order, {"x": ("lag", "v", 1, "zero")}), ValueError), (lambda: rs.sliding(by, order, {"x": ("sum", "v")}), ValueError),
                      (lambda: rs.sliding(by, order, {}), ValueError), (lambda: rs.sliding(by, [("v", "down")], ok), ValueError), (lambda: rs.sliding([], [], ok), ValueError),
                      (lambda: rs.sliding(by, order, {"h": ("sum", "v", -1, 1)}), KeyError), (lambda: rs.sliding(by, order, {"x": ("sum", "nope", -1, 1)}), KeyError),
                      (lambda: rs.sliding(["nope"], order, ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert rs.sliding(by, order, {"x": ("lag", "v", 1, 3)}).column("x").dtype == np.float64      # (an int default fits a float64 column)


def test_the_request_reads_as_a_top_and_travels_as_a_window():
    req = slide_request(None, ["a"], [("b", "desc")], {"p": ("lag", "b", 2, 1.5), "q": ("lead", "b", 1), "t": ("sum", "b", None, 0), "n": ("count", None, -1, None)})
    assert isinstance(req, SlideRequest) and isinstance(req, WindowRequest) and not isinstance(req, FrameRequest) and isinstance(req, tuple) and len(req) == 2
    assert (req[0], req[1]) == (ALL, [("a", "asc"), ("b", "desc")]) and req.by == [("a", "asc")] and req.order == [("b", "desc")] and req.npartition == 1
    assert req.slides == [("p", "first", "b", -2, -2, 1.5), ("q", "first", "b", 1, 1, None), ("t", "sum", "b", None, 0, None), ("n", "count", None, -1, None, None)]
    assert req.name is None and not hasattr(req, "aggs")
    again = req.renamed([("x", "asc"), ("y", "desc")], {"b": "y"})
    assert isinstance(again, SlideRequest) and again[1] == [("x", "asc"), ("y", "desc")] and again.slides[0] == ("p", "first", "y", -2, -2, 1.5) and again.slides[3] == req.slides[3]
    assert req.renamed(req[1]).slides == req.slides
    from sdqlpy_amd import dist as sdist
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(req)
    assert "sliding" in str(e.value)


# ---- through the decorator on the CPU implementation's engine: the host route -------------------------------------------------------
Q3_SLIDES = {"prev": ("lag", "revenue", 1), "ma3": ("sum", "revenue", -2, 0), "n3": ("count", None, -2, 0), "best3": ("max", "revenue", -1, 1)}
Q3_NOTE = [["prev", "first", "revenue", -1, -1, None], ["ma3", "sum", "revenue", -2, 0, None], ["n3", "count", None, -2, 0, None], ["best3", "max", "revenue", -1, 1, None]]


def test_q3_on_the_host_route(on_the_decorator, db):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    res = Q.q3.sliding(by, order, Q3_SLIDES)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "slides": Q3_NOTE}
    assert res.columns == plain.columns + list(Q3_SLIDES) and len(res) == len(plain) > 300
    assert [res.column(c).dtype for c in Q3_SLIDES] == [np.float64, np.float64, np.int64, np.float64]
    dates, rev = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
    assert (dates[1:] >= dates[:-1]).all() and (rev == np.asarray(plain.column("revenue"))).all()
    for d in np.unique(dates):
        sel = np.nonzero(dates == d)[0]
        x, m = rev[sel], len(sel)
        assert (x[1:] <= x[:-1]).all()
        prev = res.column("prev")[sel]
        assert math.isnan(prev[0]) and (prev[1:] == x[:-1]).all()
        assert (res.column("n3")[sel] == np.minimum(np.arange(m) + 1, 3)).all()
        for i in range(m):
            part = x[max(0, i - 2):i + 1]
            assert abs(res.column("ma3")[sel][i] - math.fsum(part)) <= 2 * U / (1 - 2 * U) * math.fsum(abs(p) for p in part)      # the header's bound, m = 3
            assert res.column("best3")[sel][i] == x[max(0, i - 1):i + 2].max()
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_argument_errors_come_before_anything_is_launched(on_the_decorator, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("launched")
    monkeypatch.setattr(engine, "execute_plan", never)
    by, order, ok = ["o_orderdate"], [("revenue", "desc")], {"x": ("sum", "revenue", -2, 0)}
    for call, exc in ((lambda: Q.q3.sliding(by, order, {"x": ("avg", "revenue", -2, 0)}), ValueError), (lambda: Q.q3.sliding(by, order, {"x": ("sum", "revenue", 1, 0)}), ValueError),
                      (lambda: Q.q3.sliding(by, order, {"x": ("sum", "revenue", -2.0, 0)}), ValueError), (lambda: Q.q3.sliding(by, order, {"x": ("lag", "revenue", -1)}), ValueError),
                      (lambda: Q.q3.sliding(by, order, {"x": ("min", None, 0, 1)}), ValueError), (lambda: Q.q3.sliding(by, order, {"x": ("lag", "revenue", 1, "none")}), ValueError),
                      (lambda: Q.q3.sliding(by, order, {}), ValueError), (lambda: Q.q3.sliding(by, [("revenue", "down")], ok), ValueError),
                      (lambda: Q.q3.sliding(by, order, {"revenue": ("sum", "revenue", -2, 0)}), KeyError), (lambda: Q.q3.sliding(by, order, {"x": ("sum", "revenu", -2, 0)}), KeyError),
                      (lambda: Q.q3.sliding(["o_orderdat"], order, ok), KeyError), (lambda: Q.q3.sliding(by, [("revenu", "desc")], ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert callable(Q.q3.sliding(by, order, ok)) and callable(Q.q3.sliding([], order, dict(ok, n=("count", None, None, None))))      # nothing runs until it is called
