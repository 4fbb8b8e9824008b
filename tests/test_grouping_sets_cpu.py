"""GROUP BY ROLLUP / CUBE / GROUPING SETS over a result, the part that needs no GPU: the grouping sets extension's symbols
(include/sdqh_sort_groups.h, abi.GROUPING_SETS_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without
them, the request and its chains, ResultSet.grouped against a pure-Python restatement of the definition (a dict of lists per set,
folded in Python integers / by walking the order images), the routing decision on a stub engine and the runner's refusal."""
import ctypes as C
import math
import os
import re
import struct
from types import SimpleNamespace

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import dist as sdist
from sdqlpy_amd.result import GROUP_OPS, GroupingRequest, ResultSet, WindowRequest, cube_sets, grouping_request, rollup_sets
from test_window_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib, oracle_lib):
    assert sorted(abi.GROUPING_SETS_EXPORTS) == _declared("sdqh_sort_groups.h") == ["sdqh_grouping_sets_geometry", "sdqh_table_grouping_sets"]
    for s in abi.GROUPING_SETS_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert not hasattr(oracle_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.WINDOW_AGG_EXPORTS, abi.WINDOW_SLIDE_EXPORTS, abi.WINDOW_RANGE_EXPORTS,
                      abi.WINDOW_QUANTILE_EXPORTS, abi.WINDOW_EXCLUDE_EXPORTS, abi.EXTREMA_EXPORTS):
            assert s not in other
    assert hip_lib.has_grouping_sets and hip_lib.has_window_agg and oracle_lib.has_grouping_sets is False and abi.ABI_VERSION == 7
    assert abi.WINDOW_EXTENSIONS["has_grouping_sets"] == (abi.GROUPING_SETS_EXPORTS, "sdqh_sort_groups.h", "grouping sets", "has_window_agg")
    text = open(os.path.join(ROOT, "include", "sdqh_sort_groups.h")).read()
    assert re.search(r"#define\s+SDQH_GS_MAX_AGGS\s+%d\b" % abi.GS_MAX_AGGS, text) and abi.GS_MAX_AGGS == 4
    assert C.sizeof(abi.GroupAgg) == 16 and [f for f, _ in abi.GroupAgg._fields_] == ["op", "kind", "index", "is_f64"]
    assert GROUP_OPS[:4] == ("sum", "count", "min", "max") and [GROUP_OPS.index(o) for o in GROUP_OPS[:4]] == [abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX]
    main = open(os.path.join(ROOT, "include", "sdqh.h")).read()
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", main) and "sdqh_sort_groups.h" not in main


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        call = lambda: ctx.table_grouping_sets(t, 0, [(abi.SORT_KEY, 0, False, False)], 0b11, [(abi.WAGG_COUNT, abi.SORT_KEY, 0, False)], ALL, 16)      # noqa: E731
        for f in (call, ctx.grouping_sets_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no grouping sets extension (include/sdqh_sort_groups.h)" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses_after_the_argument_checks(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.grouping_sets_geometry() == ctx.window_geometry() >= 64   # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context: a key, hits, no payload
        key, hits = (abi.SORT_KEY, 0, False, False), (abi.SORT_HITS, 0, True, False)
        count, total = (abi.WAGG_COUNT, abi.SORT_KEY, 0, False), (abi.WAGG_SUM, abi.SORT_HITS, 0, False)
        for terms, levels, aggs in (([key], 0b11, [count]), ([key, hits], 0b101, [total, (abi.WEX_AVG, abi.SORT_KEY, 0, False)]), ([key], 0b10, []), ([key], 0b01, [count] * 4)):
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_grouping_sets(table, 0, terms, levels, aggs, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED and "compile-only" in str(e.value), (terms, levels, aggs)
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_grouping_sets_count(table, 0, terms, levels)
            assert e.value.code == abi.ERR_UNSUPPORTED
        bad_calls = [
            ([key], 0, [count]), ([key], 0b100, [count]), ([key, hits], 0b1000, []),                                    # no level, a level above nterms
            ([key], 0b11, [(7, abi.SORT_KEY, 0, False)]), ([key], 0b11, [(-1, abi.SORT_KEY, 0, False)]), ([key], 0b11, [(abi.WSLIDE_FIRST, abi.SORT_KEY, 0, False)]),      # unknown op
            ([key], 0b11, [(abi.WAGG_SUM, abi.SORT_PAYLOAD, 0, False)]), ([key], 0b11, [count, (abi.WAGG_MAX, abi.SORT_VALUE, 9, True)]),      # a measure the table lacks
            ([key], 0b11, [(abi.WAGG_MIN, abi.SORT_KEY, 0, True)]), ([key], 0b11, [(abi.WEX_AVG, abi.SORT_HITS, 0, True)]),                    # is_f64 on KEY / HITS
            ([key], 0b11, [count] * 5), ([], 0b1, [count]), ([key] * 9, 0b11, [count]),                                  # five aggregates, no term, nine terms
        ]
        for terms, levels, bad in bad_calls:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_grouping_sets(table, 0, terms, levels, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, (terms, levels, bad)   # the argument checks — the measures' too — come first
        n = C.c_int64(-5)
        lr = np.full(abi.SORT_MAX_KEYS + 1, -7, np.int64)
        arr = (abi.GroupAgg * 1)()
        arr[0].op, arr[0].kind = abi.WAGG_SUM, abi.SORT_PAYLOAD             # nothing is written on either way out, *out_n and the level counts included
        for naggs, code in ((1, abi.ERR_INVALID), (0, abi.ERR_UNSUPPORTED), (-1, abi.ERR_INVALID)):
            rc = ctx.lib.sdqh_table_grouping_sets(ctx.handle, table.handle, C.c_int64(0), C.c_int(1), abi._marshal_sort_terms([key]), C.c_uint32(3), C.c_int(naggs), arr,
                                                  C.c_int64(ALL), C.c_int64(16), None, None, None, None, None, lr.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == code and n.value == -5 and (lr == -7).all(), naggs
    finally:
        ctx.close()


# ---- the request -------------------------------------------------------------------------------------------------------------------
def test_request_errors_come_before_anything_is_launched():
    cols = ["a", "b", "c", "x"]
    ok = grouping_request(cols, [("a", ("b", "desc")), ("a",), ()], {"s": ("sum", "x"), "n": ("count", None)})
    assert isinstance(ok, GroupingRequest) and isinstance(ok, WindowRequest) and ok[0] == ALL
    assert ok[1] == [("a", "asc"), ("b", "desc")] and ok.sets == [("a", "b"), ("a",), ()] and ok.aggs == [("s", "sum", "x"), ("n", "count", None)]
    assert ok.masks() == [0, 1, 3]
    assert grouping_request(cols, [("a",)], {}).aggs == []
    for sets, aggs, err in (([("a", "a")], {}, ValueError), ([("a",), ("a",)], {}, ValueError), ([("zz",)], {}, KeyError), ([("a",)], {"b": ("count", None)}, KeyError),
                            ([("a",)], {"grouping": ("count", None)}, KeyError), ([("a",)], {"s": ("sum", "zz")}, KeyError), ([("a",)], {"s": ("median", "x")}, ValueError),
                            ([("a",)], {"s": ("sum", None)}, ValueError), ([("a",)], {"s": ("sum",)}, ValueError), ([], {}, ValueError), ("a", {}, ValueError),
                            (["a"], {}, ValueError), ([(("a", "up"),)], {}, ValueError), ([(("a", "asc"),), (("a", "desc"), "b")], {}, ValueError), ([("a",)], [], ValueError)):
        with pytest.raises(err):
            grouping_request(cols, sets, aggs)
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(ok)
    assert "grouping_sets runs on one GPU" in str(e.value)


def test_chains():
    for d in range(1, 9):
        by = list("abcdefgh")[:d]
        req = grouping_request(None, rollup_sets(by), {})
        chains = req.chains()
        assert len(chains) == 1 and chains[0][0] == tuple(by) and chains[0][1] == {d - i: i for i in range(d + 1)}
    assert rollup_sets(["a", "b"]) == [("a", "b"), ("a",), ()]
    assert cube_sets(["a", "b"]) == [("a", "b"), ("a",), ("b",), ()] and grouping_request(None, cube_sets(["a", "b"]), {}).masks() == [0, 1, 2, 3]
    assert len(grouping_request(None, cube_sets(["a", "b"]), {}).chains()) == 2
    cube3 = grouping_request(None, cube_sets(["a", "b", "c"]), {})
    assert cube3.masks() == list(range(8)) and len(cube3.chains()) == 4
    mixed = grouping_request(None, [("b",), ("a", "b", "c"), ("c", "a"), ("a",), ("c",), ("b", "a"), ()], {})
    served = {}
    for head, members in mixed.chains():
        for level, s in members.items():
            assert s not in served and mixed.sets[s] == head[:level]       # the right level of the right chain
            served[s] = head
    assert sorted(served) == list(range(7))                                 # every set exactly once
    assert len(mixed.chains()) == 3 and served[3] == ("a", "b", "c") and served[4] == ("c", "a") and served[0] == ("b", "a")


# ---- ResultSet.grouped against a dict of lists -------------------------------------------------------------------------------------------
def _key(v, desc):
    """a Python sort key with the device's total order, restated: integers as they are; doubles by sign, then magnitude, through their
    bits (-0.0 before +0.0, a NaN where its bits put it, equal only to the same bits); descending: mirrored"""
    if isinstance(v, (float, np.floating)):
        bits = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
        u = (1 << 63) + bits if bits < (1 << 63) else (1 << 64) - 1 - bits
    else:
        u = int(v) + (1 << 63)
    return (1 << 64) - 1 - u if desc else u


def _brute(columns, arrays, req):
    col = dict(zip(columns, [a.tolist() for a in arrays]))
    dt = dict(zip(columns, [np.asarray(a).dtype for a in arrays]))
    ranks = {c: {t: i for i, t in enumerate(sorted(set(col[c])))} for c in columns if dt[c].kind == "U"}
    n = len(arrays[0]) if arrays else 0
    direction = dict(req[1])
    names = [nm for nm, _ in req[1]]
    rows = []
    for s, mask in zip(req.sets, req.masks()):
        groups = {}
        for r in range(n):
            k = tuple(_key(ranks[c][col[c][r]] if c in ranks else np.asarray(arrays[columns.index(c)])[r], direction[c] == "desc") for c in s)
            groups.setdefault(k, []).append(r)
        for k in sorted(groups):
            members = groups[k]
            out = []
            for nm in names:
                out.append(col[nm][members[0]] if nm in s else ("" if dt[nm].kind == "U" else math.nan if dt[nm].kind == "f" else 0))
            for _, op, c in req.aggs:
                vals = [col[c][r] for r in members] if c is not None else None
                is_f = c is not None and dt[c].kind == "f"
                if op == "count":
                    out.append(len(members))
                elif op in ("sum", "avg"):
                    if is_f:
                        t = float(np.add.reduce(np.array(vals, np.float64)))  # (integer-valued or specials: any association agrees)
                    else:
                        t = (sum(vals) + (1 << 63)) % (1 << 64) - (1 << 63)
                    out.append(t if op == "sum" else float(np.float64(t) / np.float64(len(members))))
                else:
                    live = [v for v in vals if not (is_f and v != v)]
                    if not live:
                        out.append(math.nan)
                    else:
                        pick = min if op == "min" else max
                        out.append(pick(live, key=lambda v: _key(np.float64(v) if is_f else np.int64(v), False)))
            out.append(mask)
            rows.append(tuple(out))
    return rows


def _same_rows(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for x, y in zip(g, w):
            if isinstance(y, float):
                assert isinstance(x, float) and np.float64(x).view(np.int64) == np.float64(y).view(np.int64) or (x != x and y != y), (g, w)
            else:
                assert x == y and type(x) is type(y), (g, w)


CASES = {
    "ints at the ends": (["a", "b", "x"], [np.array([1, 1, 1, 2, 2, 3]), np.array([I_MIN, I_MAX, I_MAX, 0, 0, -1]), np.array([I_MAX, I_MAX, I_MIN, I_MIN, I_MIN, 7])]),
    "doubles": (["a", "b", "x"], [np.array([0.0, -0.0, -0.0, np.inf, -np.inf, np.nan, np.nan, 2.0]), np.array([1, 1, 1, 2, 2, 2, 3, 3]),
                                  np.array([np.nan, -0.0, 0.0, np.inf, 4.0, np.nan, -np.inf, 3.0])]),
    "text": (["a", "b", "x"], [np.array(["pear", "apple", "pear", "", "fig", "apple"]), np.array([2, 1, 2, 2, 1, 1]), np.array([1.5, 2.0, 4.0, 8.0, 16.0, 32.0])]),
    "empty": (["a", "b", "x"], [np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64)]),
    "one row": (["a", "b", "x"], [np.array([5]), np.array(["t"]), np.array([2.5])]),
    "all rows equal": (["a", "b", "x"], [np.full(9, 3), np.full(9, -0.0), np.full(9, I_MAX)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_grouped_against_a_dict_of_lists(case):
    columns, arrays = CASES[case]
    rs = ResultSet(columns, arrays)
    aggs = {"s": ("sum", "x"), "n": ("count", None), "lo": ("min", "x"), "hi": ("max", "x"), "m": ("avg", "x")}
    for sets in (rollup_sets(["a", "b"]), cube_sets([("a", "desc"), "b"]), [(("b", "desc"), "a"), ("b",)], [()]):
        req = grouping_request(columns, sets, aggs)
        got = rs.grouped(req)
        assert got.columns == [nm for nm, _ in req[1]] + list(aggs) + ["grouping"]
        _same_rows(got.ordered_rows(), _brute(columns, arrays, req))
        is_f = np.asarray(arrays[2]).dtype.kind == "f"
        want = [np.asarray(arrays[columns.index(nm)]).dtype.kind for nm, _ in req[1]] + ["f" if is_f else "i", "i", "f" if is_f else "i", "f" if is_f else "i", "f", "i"]
        assert [a.dtype.kind for a in got.arrays] == want
        assert got.arrays[-1].dtype == np.int64 and got.column("n").dtype == np.int64 and got.column("m").dtype == np.float64
    by_method = rs.rollup(["a", "b"], aggs)
    _same_rows(by_method.ordered_rows(), rs.grouped(grouping_request(columns, rollup_sets(["a", "b"]), aggs)).ordered_rows())
    _same_rows(rs.cube(["a"], {}).ordered_rows(), rs.grouping_sets([("a",), ()], {}).ordered_rows())
    if not len(arrays[0]):
        assert len(by_method) == 0                                          # no grand total of nothing


# ---- routing, on a stub engine ---------------------------------------------------------------------------------------------------------
def _stub(**kw):
    lib = SimpleNamespace(has_grouping_sets=kw.pop("has", True), has_window_agg=True, has_sort_terms=True)
    return SimpleNamespace(device_grouping_sets=kw.pop("on", True), ctx=SimpleNamespace(library=lib), device_sort=True, order_routes=[])


def _spec(terms, measures, int_values=()):
    spec = engine._FrameSpec(terms)
    spec.measures, spec.int_values = measures, int_values
    return spec


def test_routing():
    K, P = abi.SORT_KEY, abi.SORT_PAYLOAD
    terms = [(P, 0, False, False), (K, 0, True, False)]
    m = (P, 1, False, True)
    aggs = {"s": ("sum", "x"), "n": ("count", None), "a": ("avg", "x"), "h": ("max", "x")}
    req = grouping_request(None, cube_sets(["p", ("k", "desc")]), aggs)
    fits = _spec(terms, [m, None, m, m])
    assert engine._order_route(_stub(), req, fits) == "grouping_sets"
    assert engine._order_route(_stub(on=False), req, fits) == "host"       # the switch
    assert engine._order_route(_stub(has=False), req, fits) == "host"      # a library without the extension
    five = grouping_request(None, cube_sets(["p", "k"]), dict(aggs, e=("min", "x")))
    assert engine._order_route(_stub(), five, _spec(terms, [m, None, m, m, m])) == "host"      # more than GS_MAX_AGGS aggregates
    assert engine._order_route(_stub(), req, _spec(terms, None)) == "host"                     # a text measure: no plain column
    nine = grouping_request(None, rollup_sets(list("abcdefghi")), {})
    assert engine._order_route(_stub(), nine, _spec([(K, 0, False, False)] * 9, [])) == "host"  # more than SORT_MAX_KEYS grouping columns
    assert engine._order_route(_stub(), grouping_request(None, [("p",)], {}), _spec(terms[:1], [])) == "grouping_sets"
    text = [(P, 0, False, False), (K, 0, True, False, 0, 0, 0, "ranks of some text")]
    assert engine._order_route(_stub(), req, _spec(text, [m, None, m, m])) == "grouping_sets"  # a text column groups through its ranks
    assert (engine.GroupingRequest, "grouping_sets", "device_grouping_sets", "has_grouping_sets", "aggs", abi.GS_MAX_AGGS) in engine._WINDOW_ROUTES
    eng = _stub()
    engine._note_order_route(eng, req, _spec(text, [m, None, m, m]), "grouping_sets")
    assert eng.order_routes[-1] == {"route": "grouping_sets", "k": ALL, "order": [], "ranked": ["k"], "per": ["p", "k"], "sets": [list(s) for s in req.sets],
                                    "aggs": [list(a) for a in req.aggs], "calls": 2}
    engine._note_order_route(eng, req, None, "host")
    assert eng.order_routes[-1]["route"] == "host" and eng.order_routes[-1]["calls"] == 0 and eng.order_routes[-1]["sets"] == [list(s) for s in req.sets]
    made = engine._order_spec(req, lambda order, derive: [(K, 0, False, False)] * len(order), lambda nm: False)
    assert isinstance(made, engine._FrameSpec) and len(made) == 2 and len(made.measures) == 4 and made.measures[1] is None
    # the last mile: the chains' rows behind one another, the sets back in listed order
    cols = engine._GroupColumns([np.array([10, 20, 30, 30, 5, 25])])
    cols.set_of = np.array([0, 0, 1, 3, 2, 2])                              # chain (p, k): sets 0, 1, 3; chain (k): set 2
    one = grouping_request(None, cube_sets(["p", "k"]), {"s": ("sum", "x")})
    rows = ResultSet(["p", "k", "x"], [np.array([1, 1, 1, 1, 9, 9]), np.array([7, 8, 7, 7, 7, 8]), np.zeros(6)])
    done = engine._finish_top(rows, SimpleNamespace(rank=cols), one)
    assert done.columns == ["p", "k", "s", "grouping"]
    assert done.ordered_rows() == [(1, 7, 10, 0), (1, 8, 20, 0), (1, 0, 30, 1), (0, 7, 5, 2), (0, 8, 25, 2), (0, 0, 30, 3)]
    assert engine._finish_top(rows, False, one).columns == ["p", "k", "s", "grouping"]          # not ordered: the host route


def test_the_switch_is_read_from_the_environment(oracle_lib, monkeypatch):
    for value, on in (("0", False), ("1", True)):
        monkeypatch.setenv("SDQLPY_AMD_DEVICE_GROUPING_SETS", value)
        eng = engine.Engine(oracle_lib.context(threads=1))
        try:
            assert eng.device_grouping_sets is on
        finally:
            eng.close()
