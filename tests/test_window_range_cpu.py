"""Value and group window frames (ranged), the part that needs no GPU: the window range extension's symbols (include/sdqh_sort_range.h,
abi.WINDOW_RANGE_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without them, a compile-only
context and its argument checks, ResultSet.ranged against a pure-Python reference (sort a list of tuples, test the membership of
every row of the partition in every row's frame with Python integers / Fractions, fold the members in Python integers / math.fsum),
and the decorator surface on the CPU implementation's engine — the host route."""
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import RANGE_UNITS, SLIDE_OPS, FrameRequest, RangeRequest, ResultSet, SlideRequest, WindowRequest, range_request
from test_window_cpu import NAN_A, NAN_B, SHAPES, _cases, _declared, _image, db, on_the_decorator      # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
U = 2.0 ** -53
INT_FRAMES = [(0, 0), (-1, 0), (0, 1), (-2, 3), (1, 2), (-3, -1), (None, 0), (0, None), (None, None), (None, -2), (1, None), (-10 ** 18, 10 ** 18), (10 ** 18, None), (None, -10 ** 18)]
F64_FRAMES = [(0.0, 0.0), (-1.0, 0.0), (0.0, 1.5), (-2.5, 3.0), (0.5, 2.0), (-3.0, -1.0), (None, 0.0), (0.0, None), (None, None), (None, -2.0), (1.0, None), (-1e308, 1e308), (1e-320, 1.0),
              (-1, 2)]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.WINDOW_RANGE_EXPORTS) == _declared("sdqh_sort_range.h") == ["sdqh_table_window_range", "sdqh_window_range_geometry"]
    for s in abi.WINDOW_RANGE_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.WINDOW_AGG_EXPORTS, abi.WINDOW_SLIDE_EXPORTS, abi.EXTREMA_EXPORTS):
            assert s not in other
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_sort_window.h", "sdqh_sort_frames.h", "sdqh_sort_slide.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
    assert hip_lib.has_window_range and hip_lib.has_window_slide and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort_range.h")).read()
    assert '#include "sdqh_sort_slide.h"' in text
    for name, value in (("WRANGE_VALUE", abi.WRANGE_VALUE), ("WRANGE_GROUPS", abi.WRANGE_GROUPS), ("WRANGE_LO_UNBOUNDED", abi.WRANGE_LO_UNBOUNDED),
                        ("WRANGE_HI_UNBOUNDED", abi.WRANGE_HI_UNBOUNDED), ("WRANGE_MAX_AGGS", abi.WRANGE_MAX_AGGS)):
        assert re.search(r"#define\s+SDQH_%s\s+%d\b" % (name, value), text), name
    assert (abi.WRANGE_VALUE, abi.WRANGE_GROUPS, abi.WRANGE_LO_UNBOUNDED, abi.WRANGE_HI_UNBOUNDED, abi.WRANGE_MAX_AGGS) == (0, 1, 1, 2, 4)
    assert RANGE_UNITS == ("value", "groups") and SLIDE_OPS == ("sum", "count", "min", "max", "first", "last")      # positions = the constants
    import ctypes as C
    assert C.sizeof(abi.WindowRange) == 48
    assert [f for f, _ in abi.WindowRange._fields_] == ["op", "kind", "index", "is_f64", "unit", "flags", "lo", "hi", "empty"]
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sdqh.h")).read())
    slide = open(os.path.join(ROOT, "include", "sdqh_sort_slide.h")).read()
    assert "sdqh_table_window_range" not in slide and "sdqh_window_range_geometry" not in slide


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_window_range is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        call = lambda: ctx.table_window_range(t, 0, 0, [(abi.SORT_KEY, 0, False, False)], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, abi.WRANGE_VALUE, -1, 0, 0)], ALL, 16)
        for f in (call, ctx.window_range_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no window range extension (include/sdqh_sort_range.h)" in str(e.value) and "libsdqloracle" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        tile, narrow = ctx.window_range_geometry()                         # (asks nothing of a device)
        assert tile == ctx.window_geometry() == ctx.window_agg_geometry() == ctx.window_slide_geometry()[0] >= 64 and narrow >= 0
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context
        V, G = abi.WRANGE_VALUE, abi.WRANGE_GROUPS
        key, val = (abi.SORT_KEY, 0, False, False), (abi.SORT_VALUE, 0, True, True)
        ranks = ctx.wrap(0x20000, 64, abi.I64)
        one = (abi.WAGG_COUNT, abi.SORT_KEY, 0, False, V, -1, 1, 0)
        for npart, terms, good in ((0, [key], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, -2, 0, 0)]), (0, [key], [one] * 4), (1, [key], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, G, -2, 0, 0)]),
                                   (0, [val], [(abi.WSLIDE_FIRST, abi.SORT_KEY, 0, False, V, -0.5, 1e308, 0)]), (0, [key], [(abi.WAGG_MAX, abi.SORT_KEY, 0, False, V, None, None, 0)]),
                                   (0, [key, val], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, G, I_MIN, I_MAX, 0)]),
                                   (0, [key], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, V, 5, None, 0)]), (0, [val], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, V, -2.0, -1.0, 0)])):
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_range(table, 0, npart, terms, good, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED, good
        bad_calls = [
            (0, [key], [(6, abi.SORT_KEY, 0, False, V, -1, 1, 0)]), (0, [key], [(-1, abi.SORT_KEY, 0, False, V, -1, 1, 0)]),                   # unknown op
            (0, [key], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, 2, -1, 1, 0)]), (0, [key], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, -1, -1, 1, 0)]),      # unknown unit
            (0, [key], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, 1, 0, 0)]), (0, [key], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, G, 1, 0, 0)]),             # lo > hi, integers
            (0, [val], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, 0.5, 0.25, 0)]), (0, [val], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, -1.0, -2.0, 0)]),  # ... doubles (the bits of -1.0 are below those of -2.0)
            (0, [val], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, -math.inf, 0.0, 0)]), (0, [val], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, 0.0, math.nan, 0)]),      # a non-finite offset
            (0, [val], [(abi.WAGG_SUM, abi.SORT_KEY, 0, False, V, None, math.inf, 0)]),
            (0, [key, val], [one]), (1, [key], [one]), (0, [key[:4] + (0, 0, 0, ranks)], [one]),                                               # VALUE: two order terms, none, a ranks term
            (0, [key], []), (0, [key], [one] * 5),                                                                                             # 0 or 5 ranges
        ]
        for npart, terms, bad in bad_calls:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_range(table, 0, npart, terms, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, (npart, terms, bad)    # the argument checks come first
        # unknown flag bits: the binding only ever sets the two it knows, so the struct is filled by hand
        import ctypes as C
        arr = (abi.WindowRange * 1)()
        arr[0].op, arr[0].unit, arr[0].flags, arr[0].lo, arr[0].hi = abi.WAGG_COUNT, V, 4, -1, 1
        n = C.c_int64(-5)
        rc = ctx.lib.sdqh_table_window_range(ctx.handle, table.handle, C.c_int64(0), C.c_int(0), C.c_int(1), abi._marshal_sort_terms([key]), C.c_int(1), arr, C.c_int64(ALL), C.c_int64(16),
                                             None, None, None, None, None, C.byref(n))
        assert rc == abi.ERR_INVALID and n.value == -5
        arr[0].flags = 3
        arr[0].lo, arr[0].hi = 7, -7                                       # (both sides unbounded: the offsets are ignored)
        rc = ctx.lib.sdqh_table_window_range(ctx.handle, table.handle, C.c_int64(0), C.c_int(0), C.c_int(1), abi._marshal_sort_terms([key]), C.c_int(1), arr, C.c_int64(ALL), C.c_int64(16),
                                             None, None, None, None, None, C.byref(n))
        assert rc == abi.ERR_UNSUPPORTED and n.value == -5
    finally:
        ctx.close()


# ---- ResultSet.ranged against a walk over sorted tuples ---------------------------------------------------------------------------------
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


def _members(unit, vals, groups, runs, p, lo, hi, desc):
    """The positions (relative to the partition's start) of the frame of row p: every row of the partition tested by the header's
    definition.  vals: the order values by position (unit "value"); groups: g(i); runs: (first, last) position of i's tie run."""
    m = len(groups)
    d = -1 if desc else 1
    if unit == "groups":
        return [i for i in range(m) if (lo is None or groups[p] + lo <= groups[i]) and (hi is None or groups[i] <= groups[p] + hi)]
    vj = vals[p]
    if isinstance(vj, int):
        lo, hi = (None if x is None else Fraction(x) for x in (lo, hi))
        return [i for i in range(m) if (lo is None or lo <= d * (vals[i] - vj)) and (hi is None or d * (vals[i] - vj) <= hi)]
    if vj != vj:                                                           # a NaN row: each bounded side ends with its own tie run
        return [i for i in range(m) if (lo is None or i >= runs[p][0]) and (hi is None or i <= runs[p][1])]
    a = None if lo is None else vj + d * float(lo)                        # one IEEE addition each (d * lo is exact)
    b = None if hi is None else vj + d * float(hi)
    out = []
    for i in range(m):
        x = vals[i]
        if x != x:                                                         # never through a bounded side; an unbounded one reaches them
            at_tail = (_bits(x) < 0) == desc                               # (negative NaNs sort before every number ascending, behind them descending)
            if (hi is None) if at_tail else (lo is None):
                out.append(i)
            continue
        if a is not None and b is not None:
            ok = min(a, b) <= x <= max(a, b)
        elif a is not None:                                                # only the side towards the start is bounded
            ok = x >= a if not desc else x <= a
        elif b is not None:
            ok = x <= b if not desc else x >= b
        else:
            ok = True
        if ok:
            out.append(i)
    return out


def _reference(columns, rows, by, order, unit, frames):
    """rows: list of tuples.  -> (row indices in order, per frame the list of member row lists by sorted position)."""
    terms = [(b, "asc") if isinstance(b, str) else b for b in by] + list(order)
    text_rank = {}
    for name, _ in terms:
        j = columns.index(name)
        if rows and isinstance(rows[0][j], str):
            text_rank[name] = {s: i for i, s in enumerate(sorted({r[j] for r in rows}))}
    keyed = sorted((tuple(_image(text_rank[nm][r[columns.index(nm)]] if nm in text_rank else r[columns.index(nm)], d == "desc") for nm, d in terms), i)
                   for i, r in enumerate(rows))
    n = len(keyed)
    out = [[None] * n for _ in frames]
    a = 0
    while a < n:                                                           # a partition [a, b)
        b = a + 1
        while b < n and keyed[b][0][:len(by)] == keyed[a][0][:len(by)]:
            b += 1
        groups, runs, g, first = [], [], 0, a
        for p in range(a, b):
            if p == a or keyed[p][0] != keyed[p - 1][0]:
                g, first = g + 1, p
            groups.append(g)
            runs.append([first - a, None])
        for p in range(b - 1, a - 1, -1):
            runs[p - a][1] = p - a if p == b - 1 or groups[p - a] != groups[p - a + 1] else runs[p - a + 1][1]
        vals, desc = None, False
        if unit == "value":
            (name, direction), = order
            vals, desc = [rows[i][columns.index(name)] for _, i in keyed[a:b]], direction == "desc"
        for f, (lo, hi) in enumerate(frames):
            for p in range(a, b):
                got = _members(unit, vals, groups, runs, p - a, lo, hi, desc)
                assert got == list(range(got[0], got[-1] + 1)) if got else True        # an interval of the order
                out[f][p] = [keyed[a + i][1] for i in got]
        a = b
    return [i for _, i in keyed], out


def _range_cases():
    cases = dict(_cases())
    columns, arrays = cases["plain"]
    n = 160                                                                # (the walk tests every row of a partition against every other)
    arrays = [a[:n] for a in arrays]
    rng = np.random.default_rng(5)
    big = np.resize(np.array([0, I_MAX, -1, I_MIN, 1, I_MIN, I_MAX, 0, I_MIN + 1, I_MAX - 1, 1 << 32], np.int64), n)[rng.permutation(n)]
    wild = rng.normal(0.0, 1e3, n) * 10.0 ** rng.integers(-3, 6, n)        # general doubles: sums are checked against the bound
    tiny = np.resize(np.array([0.0, -0.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, 1.5, 2.0, np.inf, -np.inf, NAN_A, NAN_B, 2.5]), n)[rng.permutation(n)]
    cases["plain"] = (columns + ["big", "wild", "tiny"], arrays + [big, wild, tiny])
    cases["empty"] = (columns + ["big", "wild", "tiny"], [a[:0] for a in cases["plain"][1]])
    cases["one row"] = (columns + ["big", "wild", "tiny"], [a[:1] for a in cases["plain"][1]])
    return cases


RANGE_SHAPES = list(SHAPES) + [(["h"], [("big", "asc")]), (["h"], [("big", "desc")]), ([], [("tiny", "asc")]), (["g"], [("tiny", "desc")]), (["g"], [("h", "asc")])]


def _check_value(op, got, want_vals, is_f):
    """got against the fold of want_vals (the frame's measure values in row order)."""
    want = _fold(op, want_vals)
    if is_f and op == "sum":
        if math.isnan(want) or math.isinf(want):
            return (math.isnan(got) and math.isnan(want)) or got == want
        if math.isnan(got) or math.isinf(got):
            return False
        if got == want:                                                    # (math.fsum: the exact sum, rounded once)
            return True
        m, exact = len(want_vals), sum(Fraction(v) for v in want_vals)
        return abs(Fraction(got) - exact) <= Fraction(m * U) / (1 - Fraction(m * U)) * sum(abs(Fraction(v)) for v in want_vals)      # gamma(m) * sum |v|
    return _bits(got) == _bits(want) if isinstance(want, float) else got == want


@pytest.mark.parametrize("case", ["plain", "empty", "one row"])
@pytest.mark.parametrize("shape", range(len(RANGE_SHAPES)))
def test_ranged_against_a_walk(case, shape):
    """Both units, every op, integer order columns (with INT64_MIN / MAX and offsets of +-10^18: nothing wraps) and double ones (NaNs,
    +-inf, +-0.0, DBL_MAX, denormals), ascending and descending, text partition columns, by = []; the first k rows of frames that
    look past k.  A value frame over anything but one numeric order column is a ValueError."""
    columns, arrays = _range_cases()[case]
    rs = ResultSet(columns, arrays)
    rows = list(zip(*[a.tolist() for a in arrays]))
    by, order = RANGE_SHAPES[shape]
    assert by or order
    done = 0
    for unit in RANGE_UNITS:
        numeric = len(order) == 1 and arrays[columns.index(order[0][0])].dtype.kind in "if"
        if unit == "value" and not numeric:
            with pytest.raises(ValueError):
                rs.ranged(by, order, {"x": ("count", None, -1, 1)}, unit="value")
            continue
        is_fv = unit == "value" and arrays[columns.index(order[0][0])].dtype.kind == "f"
        frames = F64_FRAMES if is_fv else INT_FRAMES
        idx_all, members = _reference(columns, rows, by, order, unit, frames)
        for measure in ("v", "big", "wild", "e")[:4 if case == "plain" and shape % 2 else 3]:
            is_f = arrays[columns.index(measure)].dtype.kind == "f"
            given = 2.5 if is_f else -7
            aggs = {}
            for i, (lo, hi) in enumerate(frames):
                for op in SLIDE_OPS:
                    col = None if op == "count" else measure
                    aggs["%s_%d" % (op, i)] = (op, col, lo, hi) if (i + len(op)) % 2 else (op, col, lo, hi, given)
            assert len(aggs) > 70 > abi.WRANGE_MAX_AGGS
            for k in sorted({1, max(1, len(rows) // 2), ALL}):
                with np.errstate(invalid="ignore", over="ignore"):
                    res = rs.ranged_by(range_request(columns, by, order, aggs, unit, k=k))
                idx = idx_all[:k]
                assert res.columns == columns + list(aggs) and len(res) == len(idx)
                for c, a in zip(columns, arrays):
                    got = res.column(c)
                    assert got.dtype == a.dtype and all((_bits(x) == _bits(rows[i][columns.index(c)])) if isinstance(x, float) else x == rows[i][columns.index(c)]
                                                        for x, i in zip(got.tolist(), idx)), c
                for nm, spec in aggs.items():
                    op, f = spec[0], int(nm.split("_")[1])
                    default = (spec[4] if len(spec) == 5 else None)
                    default = (NAN_A if default is None else float(default)) if is_f else (0 if default is None else default)
                    got = res.column(nm)
                    assert got.dtype == (np.float64 if is_f and op != "count" else np.int64), nm
                    for j, x in enumerate(got.tolist()[:len(idx)]):
                        inside = members[f][j]
                        if not inside:
                            want = 0 if op == "count" else default
                            assert (_bits(x) == _bits(want)) if isinstance(want, float) else x == want, (unit, by, order, measure, nm, spec, k, j, x, want)
                        else:
                            vals = [1 if op == "count" else rows[i][columns.index(measure)] for i in inside]
                            assert _check_value(op, x, vals, is_f), (unit, by, order, measure, nm, spec, k, j, x, _fold(op, vals))
                    done += 1
    assert done >= 3 * 70 * (1 if case != "plain" else 3)


def test_ranged_on_a_result_set_and_its_argument_errors():
    columns, arrays = _range_cases()["plain"]
    rs = ResultSet(columns, arrays)
    by, order = ["g"], [("v", "desc")]
    res = rs.ranged(by, order, {"near": ("count", None, -1, 1), "top": ("max", "h", None, 0), "sv": ("sum", "v", -0.5, 0.5), "f": ("first", "h", 1, 2, -9)})
    assert res.columns == columns + ["near", "top", "sv", "f"] and len(res) == len(rs)
    assert [res.column(c).dtype for c in ("near", "top", "sv", "f")] == [np.int64, np.int64, np.float64, np.int64]
    g, v, h = res.column("g"), res.column("v"), res.column("h")
    for grp in np.unique(g):
        sel = np.nonzero(g == grp)[0]
        x, y = v[sel], h[sel]
        for i in range(len(sel)):
            assert res.column("near")[sel][i] == np.count_nonzero(np.abs(x - x[i]) <= 1)
            assert res.column("top")[sel][i] == y[x >= x[i]].max()
            assert res.column("sv")[sel][i] == x[x == x[i]].sum()                                 # (integer-valued: exact)
            later = y[(x <= x[i] - 1) & (x >= x[i] - 2)]
            assert res.column("f")[sel][i] == (later[0] if len(later) else -9)
    grp = rs.ranged(by, [("v", "desc"), ("h", "asc")], {"n": ("count", None, -1, 0)}, unit="groups")
    assert grp.column("n").min() >= 1 and grp.column("n").dtype == np.int64
    ok = {"x": ("sum", "v", -1, 1)}
    for call, exc in ((lambda: rs.ranged(by, order, {"x": ("avg", "v", -1, 1)}), ValueError), (lambda: rs.ranged(by, order, {"x": ("sum", "v", 1, 0)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("sum", "v", 0.5, 0.25)}), ValueError), (lambda: rs.ranged(by, order, {"x": ("sum", "v", "1", 2)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("sum", "v", -1.0, 1)}, unit="groups"), ValueError), (lambda: rs.ranged(by, order, {"x": ("sum", "v", -math.inf, 1)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("sum", "v", math.nan, 1.0)}), ValueError), (lambda: rs.ranged(by, order, {"x": ("sum", "v", True, 1)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("sum", None, -1, 1)}), ValueError), (lambda: rs.ranged(by, order, {"x": ("first", None, 0, 0)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("sum", "s", -1, 1)}), ValueError), (lambda: rs.ranged(by, order, {"x": ("first", "s", 0, 0)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("first", "h", 1, 1, 0.5)}), ValueError), (lambda: rs.ranged(by, order, {"x": ("first", "h", 1, 1, 1 << 63)}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("first", "v", 1, 1, "zero")}), ValueError), (lambda: rs.ranged(by, order, {"x": ("sum", "v")}), ValueError),
                      (lambda: rs.ranged(by, order, {"x": ("lag", "v", 1)}), ValueError), (lambda: rs.ranged(by, order, ok, unit="rows"), ValueError),
                      (lambda: rs.ranged(by, order, {}), ValueError), (lambda: rs.ranged(by, [("v", "down")], ok), ValueError), (lambda: rs.ranged([], [], ok), ValueError),
                      (lambda: rs.ranged(by, [("s", "asc")], ok), ValueError), (lambda: rs.ranged(by, [("v", "asc"), ("h", "asc")], ok), ValueError), (lambda: rs.ranged(by, [], ok), ValueError),
                      (lambda: rs.ranged(by, [("h", "asc")], {"x": ("sum", "v", -0.5, 1)}), ValueError),
                      (lambda: rs.ranged(by, order, {"h": ("sum", "v", -1, 1)}), KeyError), (lambda: rs.ranged(by, order, {"x": ("sum", "nope", -1, 1)}), KeyError),
                      (lambda: rs.ranged(["nope"], order, ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert rs.ranged(by, order, {"x": ("first", "v", 1, 1, 3)}).column("x").dtype == np.float64      # (an int default fits a float64 column)
    assert len(rs.ranged(by, [], {"n": ("count", None, 0, 0)}, unit="groups")) == len(rs)                # groups takes any order, none included
    assert len(rs.ranged(by, [("s", "asc"), ("v", "desc")], ok, unit="groups")) == len(rs)
    assert (rs.ranged(by, [("h", "asc")], {"x": ("count", None, -1.0, 1)}).column("x") == rs.ranged(by, [("h", "asc")], {"x": ("count", None, -1, 1)}).column("x")).all()


def test_the_request_reads_as_a_top_and_travels_as_a_window():
    req = range_request(None, ["a"], [("b", "desc")], {"p": ("first", "b", -2, -2, 1.5), "t": ("sum", "b", None, 0.5), "n": ("count", None, -1, None)})
    assert isinstance(req, RangeRequest) and isinstance(req, WindowRequest) and not isinstance(req, (FrameRequest, SlideRequest)) and isinstance(req, tuple) and len(req) == 2
    assert (req[0], req[1]) == (ALL, [("a", "asc"), ("b", "desc")]) and req.by == [("a", "asc")] and req.order == [("b", "desc")] and req.npartition == 1
    assert req.unit == "value" and req.ranges == [("p", "first", "b", -2, -2, 1.5), ("t", "sum", "b", None, 0.5, None), ("n", "count", None, -1, None, None)]
    assert req.name is None and not hasattr(req, "aggs") and not hasattr(req, "slides")
    again = req.renamed([("x", "asc"), ("y", "desc")], {"b": "y"})
    assert isinstance(again, RangeRequest) and again[1] == [("x", "asc"), ("y", "desc")] and again.ranges[0] == ("p", "first", "y", -2, -2, 1.5) and again.ranges[2] == req.ranges[2]
    assert again.unit == "value" and req.renamed(req[1]).ranges == req.ranges
    grp = range_request(None, ["a"], [], {"n": ("count", None, -1, 0)}, unit="groups")
    assert grp.unit == "groups" and grp.order == [] and grp.renamed(grp[1]).unit == "groups"
    from sdqlpy_amd import dist as sdist
    for r in (req, grp):
        with pytest.raises(frontend.UnsupportedQuery) as e:
            sdist.refuse_window(r)
        assert "ranged" in str(e.value)


# ---- through the decorator on the CPU implementation's engine: the host route -------------------------------------------------------
Q3_GROUPS = {"week": ("sum", "revenue", -6, 0), "n": ("count", None, -6, 0)}
Q3_VALUE = {"near": ("count", None, -1000.0, 1000.0), "best": ("max", "revenue", -1000.0, 1000.0)}


def test_q3_on_the_host_route(on_the_decorator, db):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    plain = Q.q3.order_by([("o_shippriority", "asc"), ("o_orderdate", "asc")])(*args)
    res = Q.q3.ranged(["o_shippriority"], [("o_orderdate", "asc")], Q3_GROUPS, unit="groups")(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["o_orderdate"], "ranked": [], "per": ["o_shippriority"], "unit": "groups",
                                               "ranges": [["week", "sum", "revenue", -6, 0, None], ["n", "count", None, -6, 0, None]]}
    assert res.columns == plain.columns + list(Q3_GROUPS) and len(res) == len(plain) > 300
    assert [res.column(c).dtype for c in Q3_GROUPS] == [np.float64, np.int64]
    dates, rev = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
    assert (dates[1:] >= dates[:-1]).all() and len(np.unique(res.column("o_shippriority"))) == 1
    days = np.unique(dates)
    for j in range(0, len(dates), 7):                                      # this order date and the six distinct dates before it
        at = np.searchsorted(days, dates[j])
        inside = (dates >= days[max(0, at - 6)]) & (dates <= dates[j])
        m = int(inside.sum())
        assert res.column("n")[j] == m
        assert abs(res.column("week")[j] - math.fsum(rev[inside])) <= m * U / (1 - m * U) * math.fsum(np.abs(rev[inside]))
    by, order = ["o_orderdate"], [("revenue", "desc")]
    res = Q.q3.ranged(by, order, Q3_VALUE)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "unit": "value",
                                               "ranges": [["near", "count", None, -1000.0, 1000.0, None], ["best", "max", "revenue", -1000.0, 1000.0, None]]}
    dates, rev = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
    for d in np.unique(dates)[::5]:
        sel = np.nonzero(dates == d)[0]
        x = rev[sel]
        assert (x[1:] <= x[:-1]).all()
        for i in range(len(sel)):
            inside = (x >= x[i] - 1000.0) & (x <= x[i] + 1000.0)
            assert res.column("near")[sel][i] == inside.sum() and res.column("best")[sel][i] == x[inside].max()
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_argument_errors_come_before_anything_is_launched(on_the_decorator, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("launched")
    monkeypatch.setattr(engine, "execute_plan", never)
    by, order, ok = ["o_orderdate"], [("revenue", "desc")], {"x": ("sum", "revenue", -2, 0)}
    for call, exc in ((lambda: Q.q3.ranged(by, order, {"x": ("avg", "revenue", -2, 0)}), ValueError), (lambda: Q.q3.ranged(by, order, {"x": ("sum", "revenue", 1, 0)}), ValueError),
                      (lambda: Q.q3.ranged(by, order, {"x": ("sum", "revenue", -2.0, 0)}, unit="groups"), ValueError), (lambda: Q.q3.ranged(by, order, ok, unit="rows"), ValueError),
                      (lambda: Q.q3.ranged(by, order, {"x": ("min", None, 0, 1)}), ValueError), (lambda: Q.q3.ranged(by, order, {"x": ("first", "revenue", 1, 1, "none")}), ValueError),
                      (lambda: Q.q3.ranged(by, order, {}), ValueError), (lambda: Q.q3.ranged(by, [("revenue", "down")], ok), ValueError),
                      (lambda: Q.q3.ranged(by, [], ok), ValueError), (lambda: Q.q3.ranged(by, order + [("o_shippriority", "asc")], ok), ValueError),
                      (lambda: Q.q3.ranged(by, order, {"revenue": ("sum", "revenue", -2, 0)}), KeyError), (lambda: Q.q3.ranged(by, order, {"x": ("sum", "revenu", -2, 0)}), KeyError),
                      (lambda: Q.q3.ranged(["o_orderdat"], order, ok), KeyError), (lambda: Q.q3.ranged(by, [("revenu", "desc")], ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert callable(Q.q3.ranged(by, order, ok)) and callable(Q.q3.ranged(by, [], dict(ok, n=("count", None, None, None)), unit="groups"))      # nothing runs until it is called


def test_a_value_frame_over_a_text_or_decoded_order_column_stays_on_the_host():
    """The device may order a text column by plain arithmetic — a sorted dictionary's code is its rank, a substr part of a mixed-radix
    key is a number of several digits — and the term then carries no ranks.  The column has no arithmetic all the same: the routing
    decision must keep a value frame over it on the host (which raises), and let a group frame through.  Offsets no int64 holds stay on
    the host too, in either unit."""
    from types import SimpleNamespace
    K, P = abi.SORT_KEY, abi.SORT_PAYLOAD
    words = np.array(["a", "b", "c"])
    radix = SimpleNamespace(key_radix=([("code", [0, 1], ("chars", 2)), ("size", [0], ("int", None)), ("brand", [0], ("int", words))], [(0, 128), (0, 128), (1, 50), (0, 3)]),
                            key_parts=None, key_decoder=None, decoder_of=lambda f, s: None)
    kf = [("k", "key")]
    assert engine._order_column_decoded(radix, kf, "code") and engine._order_column_decoded(radix, kf, "brand") and not engine._order_column_decoded(radix, kf, "size")
    packed = SimpleNamespace(key_radix=None, key_parts=("name", "nation"), key_part_decoders=[words, None], key_decoder=None, decoder_of=lambda f, s: None)
    assert engine._order_column_decoded(packed, kf, "name") and not engine._order_column_decoded(packed, kf, "nation")
    plain = SimpleNamespace(key_radix=None, key_parts=None, key_decoder=words, decoder_of=lambda f, s: words if s == 1 else None)
    fields = [("k", "key"), ("t", 1), ("i", 0)]
    assert engine._order_column_decoded(plain, fields, "k") and engine._order_column_decoded(plain, fields, "t") and not engine._order_column_decoded(plain, fields, "i")
    assert not engine._order_column_decoded(plain, fields, "a value column")

    def spec_of(decoded):
        spec = engine._FrameSpec([(K, 0, False, False, 150, 0, 0, None), (K, 0, False, False, 0, 128 * 128, 0, None)])      # a substr part as the device orders it: no ranks
        spec.decoded_order, spec.measures = decoded, [None]
        return spec
    value = range_request(None, ["size"], [("code", "asc")], {"x": ("count", None, -1, 1)}, "value")
    groups = range_request(None, ["size"], [("code", "asc")], {"x": ("count", None, -1, 1)}, "groups")
    assert engine._range_offsets(value, spec_of(())) == [(-1, 1)] and engine._range_offsets(value, spec_of(("code",))) is None
    assert engine._range_offsets(groups, spec_of(("code",))) == [(-1, 1)]
    for unit in RANGE_UNITS:
        for lo, hi in ((-10 ** 30, 0), (0, 1 << 63), (None, 10 ** 19)):
            assert engine._range_offsets(range_request(None, ["size"], [("code", "asc")], {"x": ("count", None, lo, hi)}, unit), spec_of(())) is None
        assert engine._range_offsets(range_request(None, ["size"], [("code", "asc")], {"x": ("count", None, I_MIN, I_MAX)}, unit), spec_of(())) == [(I_MIN, I_MAX)]
    # the spec itself says which order columns are decoded, whichever way the result is materialised (an aggregated table, a built one)
    made = engine._order_spec(value, lambda order, derive: [(K, 0, False, False)] * len(order), lambda nm: nm == "code")
    assert isinstance(made, engine._FrameSpec) and made.decoded_order == ("code",) and engine._range_offsets(value, made) is None
    assert engine._order_spec(value, lambda order, derive: [(K, 0, False, False)] * len(order), lambda nm: False).decoded_order == ()
    built = SimpleNamespace(key_radix=None, key_parts=None, key_decoder=None, key_name="s_suppkey", field_decoders={}, decoders={0: words},
                            decoder_of=lambda f, s: {0: words}.get(s))
    assert engine._order_column_decoded(built, [("s_suppkey", "key"), ("s_name", 0), ("s_nationkey", 1)], "s_name")
    assert not engine._order_column_decoded(built, [("s_suppkey", "key"), ("s_name", 0), ("s_nationkey", 1)], "s_nationkey")
    eng = SimpleNamespace(device_window_range=True, ctx=SimpleNamespace(library=SimpleNamespace(has_window_range=True, has_sort_terms=True)), device_sort=True)
    assert engine._order_route(eng, value, spec_of(())) == "window_range" and engine._order_route(eng, value, spec_of(("code",))) == "host"
    assert engine._order_route(eng, groups, spec_of(("code",))) == "window_range"
    with pytest.raises(abi.SdqhError) as e:                                # the binding never cuts an offset to 64 bits
        abi._range_offset(1 << 63)
    assert e.value.code == abi.ERR_INVALID and abi._range_offset(I_MIN) == I_MIN and abi._range_offset(None) == 0
