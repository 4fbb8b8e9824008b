"""Window frames with rows taken out (excluding), the part that needs no GPU: the window exclude extension's symbols
(include/sdqh_sort_exclude.h, abi.WINDOW_EXCLUDE_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without
them, a compile-only context and its argument checks, the request, ResultSet.excluding against a pure-Python restatement of the
header's definition (sort a list of tuples; for every row test every row of its partition for membership in the base frame, take rows
out by key equality, fold what remains in Python integers / math.fsum), the routing decision on a stub engine, and the decorator
surface on the CPU implementation's engine — the host route."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import (EXCLUDE_OPS, EXCLUDE_UNITS, EXCLUDES, RANGE_UNITS, SLIDE_OPS, ExcludeRequest, FrameRequest, RangeRequest, ResultSet, SlideRequest, WindowRequest,
                               exclude_request)
from test_window_cpu import NAN_A, NAN_B, _declared, _image, db, on_the_decorator      # noqa: F401 (fixtures)
from test_window_range_cpu import _bits, _check_value, _members, _range_cases, _wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
V, G, R = abi.WRANGE_VALUE, abi.WRANGE_GROUPS, abi.WEX_ROWS
NO, CUR, GROUP, TIES = abi.WEX_NO_OTHERS, abi.WEX_CURRENT_ROW, abi.WEX_GROUP, abi.WEX_TIES


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.WINDOW_EXCLUDE_EXPORTS) == _declared("sdqh_sort_exclude.h") == ["sdqh_table_window_exclude", "sdqh_window_exclude_geometry"]
    for s in abi.WINDOW_EXCLUDE_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.WINDOW_AGG_EXPORTS, abi.WINDOW_SLIDE_EXPORTS, abi.WINDOW_RANGE_EXPORTS,
                      abi.WINDOW_QUANTILE_EXPORTS, abi.EXTREMA_EXPORTS):
            assert s not in other
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_sort_window.h", "sdqh_sort_frames.h", "sdqh_sort_slide.h", "sdqh_sort_range.h", "sdqh_sort_quantile.h",
                       "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
    assert hip_lib.has_window_exclude and hip_lib.has_window_range and abi.ABI_VERSION == 7
    assert abi.WINDOW_EXTENSIONS["has_window_exclude"] == (abi.WINDOW_EXCLUDE_EXPORTS, "sdqh_sort_exclude.h", "window exclude", "has_window_range")
    text = open(os.path.join(ROOT, "include", "sdqh_sort_exclude.h")).read()
    assert '#include "sdqh_sort_range.h"' in text
    for name, value in (("WEX_ROWS", abi.WEX_ROWS), ("WEX_AVG", abi.WEX_AVG), ("WEX_NO_OTHERS", abi.WEX_NO_OTHERS), ("WEX_CURRENT_ROW", abi.WEX_CURRENT_ROW),
                        ("WEX_GROUP", abi.WEX_GROUP), ("WEX_TIES", abi.WEX_TIES), ("WEX_MAX_COLS", abi.WEX_MAX_COLS)):
        assert re.search(r"#define\s+SDQH_%s\s+%d\b" % (name, value), text), name
    assert (abi.WEX_ROWS, abi.WEX_AVG, abi.WEX_NO_OTHERS, abi.WEX_CURRENT_ROW, abi.WEX_GROUP, abi.WEX_TIES, abi.WEX_MAX_COLS) == (2, 6, 0, 1, 2, 3, 4)
    # the names' positions are the constants; the siblings' lists stay what they were
    assert EXCLUDES == ("no others", "current row", "group", "ties") and EXCLUDE_UNITS == ("value", "groups", "rows") and EXCLUDE_OPS == SLIDE_OPS + ("avg",)
    assert EXCLUDE_UNITS[:2] == RANGE_UNITS and EXCLUDE_UNITS.index("rows") == abi.WEX_ROWS and EXCLUDE_OPS.index("avg") == abi.WEX_AVG
    assert C.sizeof(abi.WindowExclude) == 56
    assert [f for f, _ in abi.WindowExclude._fields_] == ["op", "kind", "index", "is_f64", "unit", "flags", "exclude", "_pad", "lo", "hi", "empty"]
    main = open(os.path.join(ROOT, "include", "sdqh.h")).read()
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", main) and "sdqh_sort_exclude.h" not in main
    for sibling in ("sdqh_sort_range.h", "sdqh_sort_slide.h"):              # they point here, and declare nothing of it
        other = open(os.path.join(ROOT, "include", sibling)).read()
        assert "sdqh_sort_exclude.h" in other and "sdqh_table_window_exclude" not in other and '#include "sdqh_sort_exclude.h"' not in other


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_window_exclude is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        call = lambda: ctx.table_window_exclude(t, 0, 0, [(abi.SORT_KEY, 0, False, False)], [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False, R, -1, 0, 0, CUR)], ALL, 16)
        for f in (call, ctx.window_exclude_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no window exclude extension (include/sdqh_sort_exclude.h)" in str(e.value) and "libsdqloracle" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        tile, narrow = ctx.window_exclude_geometry()                       # (asks nothing of a device)
        assert tile == ctx.window_geometry() == ctx.window_range_geometry()[0] >= 64 and narrow == 0
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context
        key, val = (abi.SORT_KEY, 0, False, False), (abi.SORT_VALUE, 0, True, True)
        ranks = ctx.wrap(0x20000, 64, abi.I64)
        m = (abi.SORT_KEY, 0, False)
        one = (abi.WAGG_COUNT,) + m + (R, -1, 1, 0, CUR)
        good_calls = [
            (0, [key], [(abi.WEX_AVG,) + m + (R, -2, 0, 0, CUR)]), (0, [key], [one] * 4), (1, [key], [(abi.WAGG_COUNT,) + m + (G, -2, 0, 0, TIES)]),
            (0, [val], [(abi.WSLIDE_FIRST,) + m + (V, -0.5, 1e308, 0, GROUP)]), (0, [key], [(abi.WAGG_MAX,) + m + (V, None, None, 0, NO)]),
            (0, [key, val], [(abi.WAGG_COUNT,) + m + (G, I_MIN, I_MAX, 0, CUR), (abi.WAGG_SUM,) + m + (R, I_MIN, I_MAX, 0, CUR)]),      # two order terms: no VALUE column, so fine
            (1, [key], [(abi.WEX_AVG,) + m + (R, None, 5, 0, GROUP)]),     # no ORDER BY term: ROWS and GROUPS still stand
            (0, [key], [(abi.WAGG_SUM,) + m + (V, -1, 1, 0, CUR), (abi.WAGG_MIN,) + m + (G, 0, 0, 0, TIES), (abi.WSLIDE_LAST,) + m + (R, 1, 2, -1, NO)]),      # three units in one call
        ]
        for npart, terms, good in good_calls:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_exclude(table, 0, npart, terms, good, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED, good
        bad_calls = [
            (0, [key], [(7,) + m + (R, -1, 1, 0, CUR)]), (0, [key], [(-1,) + m + (R, -1, 1, 0, CUR)]),                                         # unknown op
            (0, [key], [(abi.WAGG_COUNT,) + m + (3, -1, 1, 0, CUR)]), (0, [key], [(abi.WAGG_COUNT,) + m + (-1, -1, 1, 0, CUR)]),               # unknown unit
            (0, [key], [(abi.WAGG_COUNT,) + m + (R, -1, 1, 0, 4)]), (0, [key], [(abi.WAGG_COUNT,) + m + (R, -1, 1, 0, -1)]),                   # unknown exclude
            (0, [key], [(abi.WAGG_SUM,) + m + (V, 1, 0, 0, CUR)]), (0, [key], [(abi.WAGG_SUM,) + m + (G, 1, 0, 0, CUR)]),                      # lo > hi, each unit
            (0, [key], [(abi.WEX_AVG,) + m + (R, 1, 0, 0, CUR)]), (0, [key], [one, (abi.WAGG_SUM,) + m + (R, 3, 2, 0, CUR)]),
            (0, [val], [(abi.WAGG_SUM,) + m + (V, 0.5, 0.25, 0, CUR)]), (0, [val], [(abi.WAGG_SUM,) + m + (V, -1.0, -2.0, 0, CUR)]),           # ... doubles
            (0, [val], [(abi.WAGG_SUM,) + m + (V, -math.inf, 0.0, 0, CUR)]), (0, [val], [(abi.WAGG_SUM,) + m + (V, 0.0, math.nan, 0, CUR)]),   # a non-finite offset
            (0, [key, val], [(abi.WAGG_COUNT,) + m + (V, -1, 1, 0, CUR)]), (1, [key], [(abi.WAGG_COUNT,) + m + (V, -1, 1, 0, CUR)]),           # VALUE: two order terms, none,
            (0, [key[:4] + (0, 0, 0, ranks)], [(abi.WAGG_COUNT,) + m + (V, -1, 1, 0, CUR)]),                                                   # a ranks term
            (0, [key, val], [one, (abi.WAGG_COUNT,) + m + (V, -1, 1, 0, NO)]),                                                                 # ... in any column of the call
            (0, [key], []), (0, [key], [one] * 5),                                                                                             # 0 or 5 columns
        ]
        for npart, terms, bad in bad_calls:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_exclude(table, 0, npart, terms, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, (npart, terms, bad)    # the argument checks come first
        # what the binding never sets: unknown flag bits, a pad that is not zero — the struct filled by hand; *out_n stays
        arr = (abi.WindowExclude * 1)()
        n = C.c_int64(-5)

        def raw():
            return ctx.lib.sdqh_table_window_exclude(ctx.handle, table.handle, C.c_int64(0), C.c_int(0), C.c_int(1), abi._marshal_sort_terms([key]), C.c_int(1), arr, C.c_int64(ALL),
                                                     C.c_int64(16), None, None, None, None, None, C.byref(n))
        arr[0].op, arr[0].unit, arr[0].exclude, arr[0].lo, arr[0].hi = abi.WAGG_COUNT, R, CUR, -1, 1
        assert raw() == abi.ERR_UNSUPPORTED and n.value == -5
        arr[0].flags = 4
        assert raw() == abi.ERR_INVALID and n.value == -5
        arr[0].flags, arr[0]._pad = 0, 1
        assert raw() == abi.ERR_INVALID and n.value == -5
        arr[0]._pad, arr[0].flags = 0, 3
        arr[0].lo, arr[0].hi = 7, -7                                       # (both sides unbounded: the offsets are ignored)
        assert raw() == abi.ERR_UNSUPPORTED and n.value == -5
        with pytest.raises(abi.SdqhError) as e:                            # the binding never cuts an argument to 64 bits
            ctx.table_window_exclude(table, 0, 0, [key], [(abi.WAGG_COUNT,) + m + (R, -(1 << 64), 1, 0, CUR)], ALL, 16)
        assert e.value.code == abi.ERR_INVALID and "does not fit int64" in str(e.value)
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_exclude(table, 0, 0, [key], [(abi.WSLIDE_FIRST,) + m + (R, -1, 1, 1 << 63, CUR)], ALL, 16)
        assert e.value.code == abi.ERR_INVALID and "does not fit int64" in str(e.value)
    finally:
        ctx.close()


# ---- the request ---------------------------------------------------------------------------------------------------------------------
def test_the_request_reads_as_a_top_and_travels_as_a_window():
    req = exclude_request(None, ["a"], [("b", "desc")], {"p": ("avg", "b", -2, 2), "t": ("sum", "b", None, 0.5, 1.5, "value"), "n": ("count", None, -1, None, None, "groups")})
    assert isinstance(req, ExcludeRequest) and isinstance(req, WindowRequest) and not isinstance(req, (FrameRequest, SlideRequest, RangeRequest)) and isinstance(req, tuple) and len(req) == 2
    assert (req[0], req[1]) == (ALL, [("a", "asc"), ("b", "desc")]) and req.by == [("a", "asc")] and req.order == [("b", "desc")] and req.npartition == 1
    assert req.exclude == "current row"
    assert req.frames == [("p", "avg", "b", "rows", -2, 2, None), ("t", "sum", "b", "value", None, 0.5, 1.5), ("n", "count", None, "groups", -1, None, None)]
    assert req.name is None and not hasattr(req, "aggs") and not hasattr(req, "slides") and not hasattr(req, "ranges")
    again = req.renamed([("x", "asc"), ("y", "desc")], {"b": "y"})
    assert isinstance(again, ExcludeRequest) and again[1] == [("x", "asc"), ("y", "desc")] and again.frames[0] == ("p", "avg", "y", "rows", -2, 2, None) and again.frames[2] == req.frames[2]
    assert again.exclude == "current row" and req.renamed(req[1]).frames == req.frames
    ties = exclude_request(None, ["a"], [], {"n": ("count", None, -1, 0)}, exclude="ties", unit="groups")
    assert ties.exclude == "ties" and ties.order == [] and ties.frames[0][3] == "groups" and ties.renamed(ties[1]).exclude == "ties"
    from sdqlpy_amd import dist as sdist
    for r in (req, ties):
        with pytest.raises(frontend.UnsupportedQuery) as e:
            sdist.refuse_window(r)
        assert "excluding" in str(e.value)


def test_excluding_argument_errors():
    columns, arrays = _range_cases()["plain"]
    rs = ResultSet(columns, arrays)
    by, order = ["g"], [("v", "desc")]
    ok = {"x": ("sum", "v", -1, 1)}
    for call, exc in ((lambda: rs.excluding(by, order, {"x": ("median", "v", -1, 1)}), ValueError), (lambda: rs.excluding(by, order, {"x": ("sum", "v", 1, 0)}), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("sum", "v", 0.5, 0.25)}, unit="value"), ValueError), (lambda: rs.excluding(by, order, {"x": ("sum", "v", "1", 2)}), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("sum", "v", -1.0, 1)}), ValueError), (lambda: rs.excluding(by, order, {"x": ("sum", "v", -1.0, 1)}, unit="groups"), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("sum", "v", -1.0, 1, None, "rows")}, unit="value"), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("sum", "v", -math.inf, 1)}, unit="value"), ValueError), (lambda: rs.excluding(by, order, {"x": ("sum", "v", True, 1)}), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("avg", None, -1, 1)}), ValueError), (lambda: rs.excluding(by, order, {"x": ("first", None, 0, 0)}), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("avg", "s", -1, 1)}), ValueError), (lambda: rs.excluding(by, order, {"x": ("first", "h", 1, 1, 0.5)}), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("first", "h", 1, 1, 1 << 63)}), ValueError), (lambda: rs.excluding(by, order, {"x": ("first", "v", 1, 1, "zero")}), ValueError),
                      (lambda: rs.excluding(by, order, {"x": ("sum", "v")}), ValueError), (lambda: rs.excluding(by, order, {"x": ("sum", "v", 0, 1, None, "rows", 7)}), ValueError),
                      (lambda: rs.excluding(by, order, ok, unit="range"), ValueError), (lambda: rs.excluding(by, order, {"x": ("sum", "v", 0, 1, None, "range")}), ValueError),
                      (lambda: rs.excluding(by, order, ok, exclude="peers"), ValueError), (lambda: rs.excluding(by, order, ok, exclude=None), ValueError),
                      (lambda: rs.excluding(by, order, {}), ValueError), (lambda: rs.excluding(by, [("v", "down")], ok), ValueError), (lambda: rs.excluding([], [], ok), ValueError),
                      (lambda: rs.excluding(by, [("s", "asc")], ok, unit="value"), ValueError), (lambda: rs.excluding(by, [("v", "asc"), ("h", "asc")], ok, unit="value"), ValueError),
                      (lambda: rs.excluding(by, [], {"x": ("sum", "v", 0, 1, None, "value")}), ValueError), (lambda: rs.excluding(by, [("h", "asc")], {"x": ("sum", "v", -0.5, 1)}, unit="value"), ValueError),
                      (lambda: rs.excluding(by, order, {"h": ("sum", "v", -1, 1)}), KeyError), (lambda: rs.excluding(by, order, {"x": ("sum", "nope", -1, 1)}), KeyError),
                      (lambda: rs.excluding(["nope"], order, ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert rs.excluding(by, order, {"x": ("first", "v", 1, 1, 3)}).column("x").dtype == np.float64          # (an int default fits a float64 column)
    assert rs.excluding(by, order, {"x": ("avg", "h", 1, 1, 3)}).column("x").dtype == np.float64            # ... and an average is one whatever it measures
    assert len(rs.excluding(by, [], {"n": ("count", None, 0, 0)}, unit="groups")) == len(rs)                    # groups and rows take any order, none included
    assert len(rs.excluding(by, [("s", "asc"), ("v", "desc")], ok)) == len(rs)


# ---- ResultSet.excluding against the definition, row by row -------------------------------------------------------------------------------
def _sorted_partitions(columns, rows, by, order):
    """-> (sorted list of (term images, row index), [(a, b)] the partitions).  Text is ranked first, as the device orders it."""
    terms = [(b, "asc") if isinstance(b, str) else b for b in by] + list(order)
    text_rank = {}
    for name, _ in terms:
        j = columns.index(name)
        if rows and isinstance(rows[0][j], str):
            text_rank[name] = {s: i for i, s in enumerate(sorted({r[j] for r in rows}))}
    keyed = sorted((tuple(_image(text_rank[nm][r[columns.index(nm)]] if nm in text_rank else r[columns.index(nm)], d == "desc") for nm, d in terms), i)
                   for i, r in enumerate(rows))
    parts, a = [], 0
    while a < len(keyed):
        b = a + 1
        while b < len(keyed) and keyed[b][0][:len(by)] == keyed[a][0][:len(by)]:
            b += 1
        parts.append((a, b))
        a = b
    return keyed, parts


def _remaining(columns, rows, keyed, parts, order, unit, lo, hi, exclude):
    """Per sorted position the row indices that remain of its frame, in position order: every row of the partition is tested for
    membership in the base frame (rows: by its distance; value / groups: test_window_range_cpu's membership walk), then the rows
    whose keys all equal the row's are taken out as `exclude` says."""
    out = [None] * len(keyed)
    for a, b in parts:
        m = b - a
        groups, g = [], 0
        for p in range(a, b):
            g += 1 if p == a or keyed[p][0] != keyed[p - 1][0] else 0
            groups.append(g)
        runs = [(min(i for i in range(m) if groups[i] == groups[p]), max(i for i in range(m) if groups[i] == groups[p])) for p in range(m)]
        vals, desc = None, False
        if unit == "value":
            (name, direction), = order
            vals, desc = [rows[i][columns.index(name)] for _, i in keyed[a:b]], direction == "desc"
        for p in range(m):
            if unit == "rows":
                base = [i for i in range(m) if (lo is None or i - p >= lo) and (hi is None or i - p <= hi)]
            else:
                base = _members(unit, vals, groups, runs, p, lo, hi, desc)
            tied = lambda i: keyed[a + i][0] == keyed[a + p][0]           # noqa: E731 (all keys equal)
            if exclude == "current row":
                base = [i for i in base if i != p]
            elif exclude == "group":
                base = [i for i in base if not tied(i)]
            elif exclude == "ties":
                base = [i for i in base if i == p or not tied(i)]
            out[a + p] = [keyed[a + i][1] for i in base]
    return out


INT_FRAMES = [(0, 0), (-1, 1), (-2, 3), (1, 2), (-3, -1), (None, 0), (0, None), (None, None), (-10 ** 18, 10 ** 18)]
F64_FRAMES = [(0.0, 0.0), (-1.0, 1.5), (0.5, 2.0), (-3.0, -1.0), (None, 0.0), (0.0, None), (None, None), (-1, 2)]
# (partition by, order by, the measures folded): integer and double order values, descending, text, +-0.0 and NaNs, INT64_MIN / MAX,
# no ORDER BY term at all (one tie run per partition), partitions of one row (by every column)
EXCLUDE_SHAPES = [
    (["g"], [("v", "desc"), ("h", "asc")], ("big", "wild")),
    ([("g", "desc")], [("v", "asc")], ("big", "e")),
    ([], [("h", "desc")], ("wild", "h")),
    (["g", "h"], [], ("big", "wild")),
    (["g", "v", "h", "s", "e"], [], ("big", "wild")),
    (["g"], [("s", "desc"), ("v", "asc")], ("h", "wild")),
    (["g"], [("tiny", "desc")], ("big", "wild")),
    (["g"], [("tiny", "asc")], ("h", "e")),
    (["h"], [("big", "asc")], ("big", "v")),
]


@pytest.mark.parametrize("exclude", EXCLUDES)
@pytest.mark.parametrize("shape", range(len(EXCLUDE_SHAPES)))
def test_excluding_against_the_definition(shape, exclude):
    """All three units x this exclusion x all seven ops, int64 and float64 measures, the first k rows of frames that look past k; what
    remains nothing of takes the default by its bits; an average is its own call's sum over its count, one division."""
    columns, arrays = _range_cases()["plain"]
    n = 120                                                                # (every row of a partition is tested against every other)
    arrays = [a[:n] for a in arrays]
    rs = ResultSet(columns, arrays)
    rows = list(zip(*[a.tolist() for a in arrays]))
    by, order, measures = EXCLUDE_SHAPES[shape]
    keyed, parts = _sorted_partitions(columns, rows, by, order)
    idx_all = [i for _, i in keyed]
    done = empties = 0
    for unit in EXCLUDE_UNITS:
        numeric = len(order) == 1 and arrays[columns.index(order[0][0])].dtype.kind in "if"
        if unit == "value" and not numeric:
            with pytest.raises(ValueError):
                rs.excluding(by, order, {"x": ("count", None, -1, 1)}, exclude=exclude, unit="value")
            continue
        is_fv = unit == "value" and arrays[columns.index(order[0][0])].dtype.kind == "f"
        frames = F64_FRAMES if is_fv else INT_FRAMES
        members = [_remaining(columns, rows, keyed, parts, order, unit, lo, hi, exclude) for lo, hi in frames]
        for measure in measures:
            is_f = arrays[columns.index(measure)].dtype.kind == "f"
            aggs = {}
            for i, (lo, hi) in enumerate(frames):
                for op in EXCLUDE_OPS:
                    given = (NAN_B if i % 2 else 2.5) if is_f or op == "avg" else -7
                    col = None if op == "count" else measure
                    aggs["%s_%d" % (op, i)] = (op, col, lo, hi) if (i + len(op)) % 2 else (op, col, lo, hi, given)
            assert len(aggs) > 50 > abi.WEX_MAX_COLS
            for k in sorted({max(1, n // 2), ALL}):
                with np.errstate(invalid="ignore", over="ignore"):
                    res = rs.excluded(exclude_request(columns, by, order, aggs, exclude, unit, k=k))
                idx = idx_all[:k]
                assert res.columns == columns + list(aggs) and len(res) == len(idx)
                for c, a in zip(columns, arrays):
                    got = res.column(c)
                    assert got.dtype == a.dtype and all((_bits(x) == _bits(rows[i][columns.index(c)])) if isinstance(x, float) else x == rows[i][columns.index(c)]
                                                        for x, i in zip(got.tolist(), idx)), c
                for nm, spec in aggs.items():
                    op, f = spec[0], int(nm.split("_")[1])
                    out_f = is_f or op == "avg"
                    default = spec[4] if len(spec) == 5 else None
                    default = (NAN_A if default is None else float(default)) if out_f else (0 if default is None else default)
                    got = res.column(nm)
                    assert got.dtype == (np.float64 if out_f and op != "count" else np.int64), nm
                    sums, counts = res.column("sum_%d" % f), res.column("count_%d" % f)
                    for j, x in enumerate(got.tolist()[:len(idx)]):
                        inside = members[f][j]
                        what = (unit, exclude, by, order, measure, nm, spec, k, j, x)
                        if not inside:
                            want = 0 if op == "count" else default
                            assert (_bits(x) == _bits(want)) if isinstance(want, float) else x == want, what
                            empties += 1
                        elif op == "avg":
                            vals = [rows[i][columns.index(measure)] for i in inside]
                            assert counts[j] == len(vals)
                            with np.errstate(invalid="ignore", over="ignore"):
                                want = float(np.float64(sums[j]) / np.float64(counts[j]))          # its own call's SUM, one conversion, one division
                                if not is_f:
                                    assert want == float(np.float64(_wrap(sum(vals))) / np.float64(len(vals)))
                            assert _bits(x) == _bits(want) or (math.isnan(x) and math.isnan(want)), what + (want,)
                        else:
                            vals = [1 if op == "count" else rows[i][columns.index(measure)] for i in inside]
                            assert _check_value(op, x, vals, is_f), what
                    done += 1
    assert done >= 2 * 2 * 2 * 50 and empties > 0
    if not order:                                                          # no ORDER BY term: the partition is one tie run, GROUP empties every frame
        with np.errstate(invalid="ignore", over="ignore"):
            res = rs.excluding(by, order, {"n": ("count", None, None, None), "m": ("max", "h", None, None, -9)}, exclude="group")
        assert (res.column("n") == 0).all() and (res.column("m") == -9).all()


def test_frames_that_do_not_hold_their_row_and_units_side_by_side():
    """A frame wholly behind or wholly in front of the row loses nothing under CURRENT ROW, and TIES never adds the row to it; four
    columns of three units in one request are the four single requests."""
    columns, arrays = _range_cases()["plain"]
    rs = ResultSet(columns, arrays)
    by, order = ["g"], [("h", "asc")]                                      # h has three values: long tie runs
    for lo, hi in ((1, 3), (-3, -1), (2, None), (None, -2)):
        aggs = {"n": ("count", None, lo, hi), "sb": ("sum", "big", lo, hi), "f": ("first", "v", lo, hi), "a": ("avg", "wild", lo, hi)}
        plain = rs.excluding(by, order, aggs, exclude="no others")
        cur = rs.excluding(by, order, aggs, exclude="current row")
        for c in aggs:
            assert (_bits_of(plain.column(c)) == _bits_of(cur.column(c))).all(), (lo, hi, c)
        ties, group = rs.excluding(by, order, aggs, exclude="ties"), rs.excluding(by, order, aggs, exclude="group")
        for c in aggs:                                                     # the row is outside its base frame: TIES is GROUP there
            assert (_bits_of(ties.column(c)) == _bits_of(group.column(c))).all(), (lo, hi, c)
        assert (ties.column("n") <= plain.column("n")).all() and (ties.column("n") < plain.column("n")).any()
    mixed = {"a": ("avg", "wild", -3, 3), "sb": ("sum", "big", -1, 1, None, "value"), "c": ("count", None, -1, 0, None, "groups"), "m": ("max", "v", None, 2, -1.0, "rows")}
    res = rs.excluding(by, order, mixed, exclude="ties")
    for c, spec in mixed.items():
        alone = rs.excluding(by, order, {c: spec[:5] if len(spec) > 4 else spec}, exclude="ties", unit=spec[5] if len(spec) == 6 else "rows")
        assert (_bits_of(res.column(c)) == _bits_of(alone.column(c))).all(), c
    # with nothing taken out a column is its sibling's: ranged for value / groups, sliding for rows (integer sums and everything not summed)
    no = rs.excluding(by, order, {"sb": ("sum", "big", -1, 1, None, "value"), "m": ("min", "wild", -2, 2, None, "groups"), "r": ("sum", "big", -2, 5), "l": ("last", "wild", 1, 4)}, exclude="no others")
    assert (_bits_of(no.column("sb")) == _bits_of(rs.ranged(by, order, {"sb": ("sum", "big", -1, 1)}).column("sb"))).all()
    assert (_bits_of(no.column("m")) == _bits_of(rs.ranged(by, order, {"m": ("min", "wild", -2, 2)}, unit="groups").column("m"))).all()
    slid = rs.sliding(by, order, {"r": ("sum", "big", -2, 5), "l": ("last", "wild", 1, 4)})
    assert (_bits_of(no.column("r")) == _bits_of(slid.column("r"))).all() and (_bits_of(no.column("l")) == _bits_of(slid.column("l"))).all()


def _bits_of(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- routing, on a stub engine ---------------------------------------------------------------------------------------------------------
def _stub(**kw):
    lib = SimpleNamespace(has_window_exclude=kw.pop("has", True), has_window_range=True, has_sort_terms=True)
    return SimpleNamespace(device_window_exclude=kw.pop("on", True), ctx=SimpleNamespace(library=lib), device_sort=True, order_routes=[])


def _spec(terms, measures, decoded=(), int_values=()):
    spec = engine._FrameSpec(terms)
    spec.measures, spec.decoded_order, spec.int_values = measures, decoded, int_values
    return spec


def test_routing():
    K, P = abi.SORT_KEY, abi.SORT_PAYLOAD
    terms = [(P, 0, False, False), (K, 0, True, False)]                    # PARTITION BY a payload column ORDER BY the integer key, descending
    m = (P, 1, False, True)
    aggs = {"a": ("avg", "x", -3, 3), "s": ("sum", "x", -5, 5, None, "value"), "c": ("count", None, -1, 1, None, "groups"), "m": ("max", "x", None, 0)}
    req = exclude_request(None, ["p"], [("k", "desc")], aggs, exclude="ties")
    fits = _spec(terms, [m, m, None, m])
    assert engine._order_route(_stub(), req, fits) == "window_exclude"
    assert engine._exclude_offsets(req, fits) == [(-3, 3), (-5, 5), (-1, 1), (None, 0)]
    assert engine._order_route(_stub(on=False), req, fits) == "host"       # the switch
    assert engine._order_route(_stub(has=False), req, fits) == "host"      # a library without the extension
    five = exclude_request(None, ["p"], [("k", "desc")], dict(aggs, e=("count", None, 0, 0)))
    assert engine._order_route(_stub(), five, _spec(terms, [m, m, None, m, None])) == "host"      # more than WEX_MAX_COLS columns
    assert engine._order_route(_stub(), req, _spec(terms, [m, m, None, m], decoded=("k",))) == "host"      # a value frame over a decoded order column
    rows_only = exclude_request(None, ["p"], [("k", "desc")], {"a": ("avg", "x", -3, 3), "c": ("count", None, -1, 1, None, "groups")})
    assert engine._order_route(_stub(), rows_only, _spec(terms, [m, None], decoded=("k",))) == "window_exclude"      # ... rows and groups need no arithmetic
    half = exclude_request(None, ["p"], [("k", "desc")], {"s": ("sum", "x", -0.5, 5, None, "value")})
    assert engine._order_route(_stub(), half, _spec(terms, [m])) == "host" and engine._exclude_offsets(half, _spec(terms, [m])) is None      # a float offset on an integer term
    wide = exclude_request(None, ["p"], [("k", "desc")], {"s": ("count", None, -(1 << 70), 5)})
    assert engine._order_route(_stub(), wide, _spec(terms, [None])) == "host"                      # an offset no int64 holds
    assert engine._order_route(_stub(), req, _spec(terms, None)) == "host"                         # a measure that is no plain column
    text = [(P, 0, False, False), (K, 0, True, False, 0, 0, 0, "ranks of some text")]
    assert engine._order_route(_stub(), req, _spec(text, [m, m, None, m])) == "host"              # a value frame over a text-ranked term
    assert engine._order_route(_stub(), rows_only, _spec(text, [m, None])) == "window_exclude"
    eng = _stub()
    engine._note_order_route(eng, req, fits, "window_exclude")
    assert eng.order_routes[-1] == {"route": "window_exclude", "k": ALL, "order": ["k"], "ranked": [], "per": ["p"], "exclude": "ties", "frames": [list(f) for f in req.frames]}
    made = engine._order_spec(req, lambda order, derive: [(K, 0, False, False)] * len(order), lambda nm: nm == "k")
    assert isinstance(made, engine._FrameSpec) and made.decoded_order == ("k",) and len(made.measures) == 4 and made.measures[2] is None
    rank = SimpleNamespace(rank=[np.zeros(2)] * 4)
    done = engine._finish_top(ResultSet(["p", "k"], [np.arange(2), np.arange(2)]), rank, req)
    assert done.columns == ["p", "k", "a", "s", "c", "m"]
    with pytest.raises(KeyError):
        engine._finish_top(ResultSet(["p", "a"], [np.arange(2), np.arange(2)]), rank, req)


def test_an_average_takes_a_double_default_whatever_it_measures():
    """On the device route too: an average over an int64 measure with a float default is marshalled as the double it is (the host
    route returns it as given), where a sum over the same measure refuses it; and an average's default never sends a column the
    table keeps as integer-valued doubles to the host."""
    import struct
    K, P = abi.SORT_KEY, abi.SORT_PAYLOAD
    terms = [(P, 0, False, False), (K, 0, True, False)]
    ints = (P, 1, False, False)                                            # an int64 payload column
    req = exclude_request(None, ["p"], [("k", "desc")], {"a": ("avg", "x", -1, 1, 0.5), "b": ("avg", "x", -1, 1), "c": ("avg", "x", -1, 1, 3), "s": ("sum", "x", -1, 1, 3)})
    spec = _spec(terms, [ints] * 4)
    assert engine._order_route(_stub(), req, spec) == "window_exclude"
    bits = lambda x: struct.unpack("<q", struct.pack("<d", x))[0]        # noqa: E731
    cols = engine._exclude_columns(req, spec)
    assert [c[0] for c in cols] == [abi.WEX_AVG] * 3 + [abi.WAGG_SUM] and all(c[1:4] == (P, 1, False) and c[4] == abi.WEX_ROWS and c[8] == abi.WEX_CURRENT_ROW for c in cols)
    assert cols[0][7] == bits(0.5) and cols[1][7] == int(np.array(np.nan).view(np.int64)) and cols[2][7] == bits(3.0) and cols[3][7] == 3
    refused = exclude_request(None, ["p"], [("k", "desc")], {"s": ("sum", "x", -1, 1, 0.5)})
    with pytest.raises(ValueError):                                        # (the host route refuses it as well: a float for an int64 column)
        engine._exclude_columns(refused, _spec(terms, [ints]))
    rs = ResultSet(["p", "k", "x"], [np.zeros(3, np.int64), np.arange(3), np.array([4, 5, 6])])
    got = rs.excluding(["p"], [("k", "desc")], {"a": ("avg", "x", 5, 6, 0.5), "m": ("avg", "x", -1, 1)})
    assert got.column("a").tolist() == [0.5] * 3 and got.column("m").tolist() == [5.0, 5.0, 5.0]
    with pytest.raises(ValueError):
        rs.excluding(["p"], [("k", "desc")], {"s": ("sum", "x", -1, 1, 0.5)})
    # a column kept as integer-valued doubles: a sum's default beyond 2^53 stays on the host, an average's is a double anyway
    dbl = (abi.SORT_VALUE, 0, False, True)
    big = exclude_request(None, ["p"], [("k", "desc")], {"a": ("avg", "x", -1, 1, (1 << 53) + 1)})
    assert engine._order_route(_stub(), big, _spec(terms, [dbl], int_values=("x",))) == "window_exclude"
    assert engine._exclude_columns(big, _spec(terms, [dbl], int_values=("x",)))[0][7] == bits(float((1 << 53) + 1))
    big_sum = exclude_request(None, ["p"], [("k", "desc")], {"s": ("sum", "x", -1, 1, (1 << 53) + 1)})
    assert engine._order_route(_stub(), big_sum, _spec(terms, [dbl], int_values=("x",))) == "host"


def test_the_switch_is_read_from_the_environment(oracle_lib, monkeypatch):
    monkeypatch.setenv("SDQLPY_AMD_DEVICE_WINDOW_EXCLUDE", "0")
    off = engine.Engine(oracle_lib.context(threads=1))
    monkeypatch.delenv("SDQLPY_AMD_DEVICE_WINDOW_EXCLUDE")
    on = engine.Engine(oracle_lib.context(threads=1))
    try:
        assert off.device_window_exclude is False and on.device_window_exclude is True
    finally:
        off.close(); on.close()


# ---- through the decorator on the CPU implementation's engine: the host route -------------------------------------------------------
Q3_MIXED = {"others": ("avg", "revenue", -103, 103), "near": ("sum", "revenue", -20000.0, 20000.0, None, "value"), "peers": ("count", None, -3, 3, None, "groups"),
            "best": ("max", "revenue", None, 0)}


def test_q3_on_the_host_route(on_the_decorator, db):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    res = Q.q3.excluding(by, order, Q3_MIXED)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "exclude": "current row",
                                               "frames": [["others", "avg", "revenue", "rows", -103, 103, None], ["near", "sum", "revenue", "value", -20000.0, 20000.0, None],
                                                          ["peers", "count", None, "groups", -3, 3, None], ["best", "max", "revenue", "rows", None, 0, None]]}
    assert res.columns == plain.columns + list(Q3_MIXED) and len(res) == len(plain) > 300
    assert [res.column(c).dtype for c in Q3_MIXED] == [np.float64, np.float64, np.int64, np.float64]
    want = plain.excluding(by, order, Q3_MIXED)
    for c in res.columns:
        a, b = np.asarray(res.column(c)), np.asarray(want.column(c))
        assert (a == b).all() or (a.dtype.kind == "f" and np.allclose(a, b, rtol=1e-10, atol=0.0, equal_nan=True)), c
    dates, rev = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
    for d in np.unique(dates)[::7]:                                        # the average of the day's other orders, by numpy
        sel = np.nonzero(dates == d)[0]
        x = rev[sel]
        for i in range(len(sel)):
            others = np.delete(x, i)
            got = res.column("others")[sel][i]
            assert (math.isnan(got) and len(others) == 0) or abs(got - others.mean()) <= 1e-9 * abs(others).max()
            assert res.column("best")[sel][i] == (x[:i].max() if i else np.float64("nan")) or (i == 0 and math.isnan(res.column("best")[sel][i]))
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_argument_errors_come_before_anything_is_launched(on_the_decorator, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("launched")
    monkeypatch.setattr(engine, "execute_plan", never)
    by, order, ok = ["o_orderdate"], [("revenue", "desc")], {"x": ("avg", "revenue", -2, 0)}
    for call, exc in ((lambda: Q.q3.excluding(by, order, {"x": ("mean", "revenue", -2, 0)}), ValueError), (lambda: Q.q3.excluding(by, order, {"x": ("sum", "revenue", 1, 0)}), ValueError),
                      (lambda: Q.q3.excluding(by, order, {"x": ("sum", "revenue", -2.0, 0)}), ValueError), (lambda: Q.q3.excluding(by, order, ok, unit="range"), ValueError),
                      (lambda: Q.q3.excluding(by, order, ok, exclude="others"), ValueError), (lambda: Q.q3.excluding(by, order, {"x": ("avg", None, 0, 1)}), ValueError),
                      (lambda: Q.q3.excluding(by, order, {}), ValueError), (lambda: Q.q3.excluding(by, [("revenue", "down")], ok), ValueError),
                      (lambda: Q.q3.excluding(by, [], ok, unit="value"), ValueError), (lambda: Q.q3.excluding(by, order + [("o_shippriority", "asc")], {"x": ("sum", "revenue", 0, 1, None, "value")}), ValueError),
                      (lambda: Q.q3.excluding(by, order, {"revenue": ("sum", "revenue", -2, 0)}), KeyError), (lambda: Q.q3.excluding(by, order, {"x": ("sum", "revenu", -2, 0)}), KeyError),
                      (lambda: Q.q3.excluding(["o_orderdat"], order, ok), KeyError), (lambda: Q.q3.excluding(by, [("revenu", "desc")], ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert callable(Q.q3.excluding(by, order, ok)) and callable(Q.q3.excluding(by, [], dict(ok, n=("count", None, None, None)), exclude="group", unit="groups"))      # nothing runs until it is called
