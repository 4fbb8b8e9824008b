"""Aggregates over the distinct values of a group, the part that needs no GPU: the group distinct extension's symbols
(include/sdqh_sort_distinct.h, abi.GROUP_DISTINCT_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation
without them, the argument checks of a compile-only context, the request, ResultSet.distincted against a pure-Python restatement of
the definition (a dict of lists per group, collections.Counter, Python integers), the routing decision on a stub engine and the
runner's refusal."""
import collections
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import dist as sdist
from sdqlpy_amd.result import DISTINCT_OPS, DistinctRequest, ResultSet, WindowRequest, distinct_request
from test_grouping_sets_cpu import _key, _same_rows
from test_window_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib, oracle_lib):
    assert sorted(abi.GROUP_DISTINCT_EXPORTS) == _declared("sdqh_sort_distinct.h") == ["sdqh_group_distinct_geometry", "sdqh_table_group_distinct"]
    for s in abi.GROUP_DISTINCT_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert not hasattr(oracle_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.WINDOW_AGG_EXPORTS, abi.WINDOW_SLIDE_EXPORTS, abi.WINDOW_RANGE_EXPORTS,
                      abi.WINDOW_QUANTILE_EXPORTS, abi.WINDOW_EXCLUDE_EXPORTS, abi.GROUPING_SETS_EXPORTS, abi.EXTREMA_EXPORTS):
            assert s not in other
    assert hip_lib.has_group_distinct and hip_lib.has_grouping_sets and oracle_lib.has_group_distinct is False and abi.ABI_VERSION == 7
    assert abi.WINDOW_EXTENSIONS["has_group_distinct"] == (abi.GROUP_DISTINCT_EXPORTS, "sdqh_sort_distinct.h", "group distinct", "has_grouping_sets")
    text = open(os.path.join(ROOT, "include", "sdqh_sort_distinct.h")).read()
    assert re.search(r"#define\s+SDQH_GD_MAX_AGGS\s+%d\b" % abi.GD_MAX_AGGS, text) and abi.GD_MAX_AGGS == 4
    for name, value in (("COUNT_DISTINCT", abi.GD_COUNT_DISTINCT), ("SUM_DISTINCT", abi.GD_SUM_DISTINCT), ("AVG_DISTINCT", abi.GD_AVG_DISTINCT), ("MODE", abi.GD_MODE),
                        ("MODE_COUNT", abi.GD_MODE_COUNT), ("COUNT", abi.GD_COUNT)):
        assert re.search(r"#define\s+SDQH_GD_%s\s+%d\b" % (name, value), text), name
        assert DISTINCT_OPS.index(name.lower()) == value                    # the request's names are the header's numbers
    main = open(os.path.join(ROOT, "include", "sdqh.h")).read()
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", main) and "sdqh_sort_distinct.h" not in main


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        key, hits = (abi.SORT_KEY, 0, False, False), (abi.SORT_HITS, 0, False, False)
        call = lambda: ctx.table_group_distinct(t, 0, [key, hits], 1, [(abi.GD_COUNT_DISTINCT, abi.SORT_KEY, 0, False)], ALL, 16)      # noqa: E731
        count = lambda: ctx.table_group_distinct_count(t, 0, [key, hits], 1, [(abi.GD_COUNT, abi.SORT_KEY, 0, False)])                 # noqa: E731
        for f in (call, count, ctx.group_distinct_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no group distinct extension (include/sdqh_sort_distinct.h)" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses_after_the_argument_checks(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.group_distinct_geometry() == ctx.window_geometry() >= 64  # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context: a key, hits, no payload
        key, hits = (abi.SORT_KEY, 0, False, False), (abi.SORT_HITS, 0, True, False)
        cd, total = (abi.GD_COUNT_DISTINCT, abi.SORT_KEY, 0, False), (abi.GD_SUM_DISTINCT, abi.SORT_HITS, 0, False)
        every = [(op, abi.SORT_KEY, 0, False) for op in range(6)]
        for terms, ngroup, aggs in (([key], 0, [cd]), ([key, hits], 1, [total, (abi.GD_AVG_DISTINCT, abi.SORT_KEY, 0, False)]), ([key, hits], 0, every[:4]), ([key, hits], 1, every[2:]),
                                    ([key] * 8, 7, [(abi.GD_MODE, abi.SORT_HITS, 0, False)]), ([key, hits], 1, [(abi.GD_COUNT, abi.SORT_PAYLOAD, 5, True)])):      # (COUNT ignores its measure)
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_group_distinct(table, 0, terms, ngroup, aggs, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED and "compile-only" in str(e.value), (terms, ngroup, aggs)
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_group_distinct_count(table, 0, terms, ngroup, aggs)
            assert e.value.code == abi.ERR_UNSUPPORTED
        bad_calls = [
            ([key, hits], 1, [(6, abi.SORT_KEY, 0, False)]), ([key, hits], 1, [(-1, abi.SORT_KEY, 0, False)]), ([key, hits], 1, [cd, (99, abi.SORT_KEY, 0, False)]),      # unknown op
            ([key, hits], 1, [(abi.GD_SUM_DISTINCT, abi.SORT_PAYLOAD, 0, False)]), ([key, hits], 1, [cd, (abi.GD_MODE, abi.SORT_VALUE, 9, True)]),      # a measure the table lacks
            ([key, hits], 1, [(abi.GD_AVG_DISTINCT, abi.SORT_VALUE, -1, True)]),
            ([key, hits], 1, [(abi.GD_MODE, abi.SORT_KEY, 0, True)]), ([key, hits], 1, [(abi.GD_AVG_DISTINCT, abi.SORT_HITS, 0, True)]),                # is_f64 on KEY / HITS
            ([key, hits], 1, [cd] * 5), ([key, hits], 1, []),                                                                # five aggregates, none
            ([key, hits], -1, [cd]), ([key, hits], 2, [cd]), ([key], 1, [cd]), ([key, hits], 3, [cd]),                       # ngroup < 0, ngroup >= nterms
            ([], 0, [cd]), ([key] * 9, 1, [cd]),                                                                             # no term, nine terms
        ]
        for terms, ngroup, bad in bad_calls:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_group_distinct(table, 0, terms, ngroup, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, (terms, ngroup, bad)   # the argument checks — the measures' too — come first
        n = C.c_int64(-5)
        out = np.full((4, 16), -7, np.int64)
        arr = (abi.GroupAgg * 1)()
        arr[0].op, arr[0].kind = abi.GD_SUM_DISTINCT, abi.SORT_PAYLOAD     # nothing is written on either way out, *out_n included
        two = abi._marshal_sort_terms([key, hits])
        calls = ((1, arr, 1, ALL, 16, abi.ERR_INVALID), (0, arr, 1, ALL, 16, abi.ERR_INVALID), (-1, arr, 1, ALL, 16, abi.ERR_INVALID), (1, None, 1, ALL, 16, abi.ERR_INVALID),
                 (1, arr, 1, 0, 16, abi.ERR_INVALID), (1, arr, 1, ALL, -1, abi.ERR_INVALID))                                # limit < 1, capacity < 0: sdqh_table_window's
        for naggs, aggs, ngroup, limit, cap, code in calls:
            rc = ctx.lib.sdqh_table_group_distinct(ctx.handle, table.handle, C.c_int64(0), C.c_int(2), two, C.c_int(ngroup), C.c_int(naggs), aggs,
                                                   C.c_int64(limit), C.c_int64(cap), out[0].ctypes.data_as(C.c_void_p), None, None, out[1].ctypes.data_as(C.c_void_p),
                                                   out[2:].ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == code and n.value == -5 and (out == -7).all(), (naggs, ngroup, limit, cap)
        arr[0].op, arr[0].kind = abi.GD_COUNT_DISTINCT, abi.SORT_KEY
        for terms, out_n, code in ((two, C.byref(n), abi.ERR_UNSUPPORTED), (None, C.byref(n), abi.ERR_INVALID), (two, None, abi.ERR_INVALID)):
            rc = ctx.lib.sdqh_table_group_distinct(ctx.handle, table.handle, C.c_int64(0), C.c_int(2), terms, C.c_int(1), C.c_int(1), arr,
                                                   C.c_int64(ALL), C.c_int64(16), out[0].ctypes.data_as(C.c_void_p), None, None, out[1].ctypes.data_as(C.c_void_p),
                                                   out[2:].ctypes.data_as(C.c_void_p), out_n)
            assert rc == code and n.value == -5 and (out == -7).all()
        for a, b in ((None, table.handle), (ctx.handle, None)):            # no context, no table
            rc = ctx.lib.sdqh_table_group_distinct(a, b, C.c_int64(0), C.c_int(2), two, C.c_int(1), C.c_int(1), arr, C.c_int64(ALL), C.c_int64(16),
                                                   None, None, None, None, None, C.byref(n))
            assert rc == abi.ERR_INVALID and n.value == -5
    finally:
        ctx.close()


# ---- the request -------------------------------------------------------------------------------------------------------------------
def test_request_errors_come_before_anything_is_launched():
    cols = ["a", "b", "c", "x", "y"]
    ok = distinct_request(cols, ["a", ("b", "desc")], {"d": ("count_distinct", "x"), "n": ("count", None), "m": ("mode", "y"), "s": ("sum_distinct", "x")})
    assert isinstance(ok, DistinctRequest) and isinstance(ok, WindowRequest) and ok[0] == ALL
    assert ok[1] == [("a", "asc"), ("b", "desc"), ("x", "asc"), ("y", "asc")] and ok.npartition == 2 and ok.by == [("a", "asc"), ("b", "desc")] and ok.values == ["x", "y"]
    assert ok.aggs == [("d", "count_distinct", "x"), ("n", "count", None), ("m", "mode", "y"), ("s", "sum_distinct", "x")]
    assert ok.calls() == [("x", [0, 3, 1]), ("y", [2])]                     # one call per value column; the count rides in the first with room
    assert distinct_request(None, [], {"d": ("count_distinct", "zz")}).by == []      # no grouping column: one group; names checked when the result is known
    for by, aggs, err in ((["a", "a"], {"d": ("count_distinct", "x")}, ValueError), (["zz"], {"d": ("count_distinct", "x")}, KeyError),
                          (["a"], {"d": ("count_distinct", "zz")}, KeyError), (["a"], {"b": ("count", None)}, KeyError), (["a"], {"a": ("count", None)}, ValueError),
                          (["a"], {"d": ("median", "x")}, ValueError), (["a"], {"d": ("count_distinct", None)}, ValueError), (["a"], {"d": ("count", "x")}, ValueError),
                          (["a"], {"d": ("mode",)}, ValueError), (["a"], {}, ValueError), (["a"], [], ValueError), ("a", {"d": ("count_distinct", "x")}, ValueError),
                          ([("a", "up")], {"d": ("count_distinct", "x")}, ValueError), (["a"], {"d": ("count_distinct", "a")}, ValueError),
                          (["a"], {"d": ("sum_distinct", 3)}, ValueError), ([3], {"d": ("count_distinct", "x")}, ValueError)):
        with pytest.raises(err):
            distinct_request(cols, by, aggs)
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(ok)
    assert "distincts runs on one GPU" in str(e.value)
    five = distinct_request(None, ["a"], {n: (op, "x") for n, op in zip("pqrst", DISTINCT_OPS[:5])})
    assert five.calls() is None                                             # more than DISTINCT_MAX_AGGS over one value column
    assert distinct_request(None, ["a"], {"n": ("count", None)}).calls() is None      # no value column to sort by
    full = distinct_request(None, ["a"], dict({n: (op, "x") for n, op in zip("pqrs", DISTINCT_OPS[:4])}, n=("count", None), d=("count_distinct", "y")))
    assert full.calls() == [("x", [0, 1, 2, 3]), ("y", [5, 4])]             # the first call is full: the count rides in the second
    again = ok.renamed([("A", "asc"), ("B", "desc"), ("X", "asc"), ("Y", "asc")])
    assert again[1] == [("A", "asc"), ("B", "desc"), ("X", "asc"), ("Y", "asc")] and again.aggs[2] == ("m", "mode", "Y") and again.aggs[1] == ("n", "count", None)


# ---- ResultSet.distincted against a dict of lists -----------------------------------------------------------------------------------
def _brute(columns, arrays, req):
    col = dict(zip(columns, [a.tolist() for a in arrays]))
    dt = dict(zip(columns, [np.asarray(a).dtype for a in arrays]))
    ranks = {c: {t: i for i, t in enumerate(sorted(set(col[c])))} for c in columns if dt[c].kind == "U"}
    n = len(arrays[0]) if arrays else 0

    def image(c, r, desc):
        return _key(ranks[c][col[c][r]] if c in ranks else np.asarray(arrays[columns.index(c)])[r], desc)
    groups = {}
    for r in range(n):
        groups.setdefault(tuple(image(c, r, d == "desc") for c, d in req.by), []).append(r)
    rows = []
    for k in sorted(groups):
        members = groups[k]
        out = [col[nm][members[0]] for nm, _ in req.by]
        for _, op, c in req.aggs:
            if op == "count":
                out.append(len(members))
                continue
            runs = collections.Counter(image(c, r, False) for r in members)      # a value is its image: -0.0 and +0.0 are two, NaNs equal only bit for bit
            first = {}
            for r in members:
                first.setdefault(image(c, r, False), col[c][r])
            is_f = dt[c].kind == "f"
            if op == "count_distinct":
                out.append(len(runs))
            elif op in ("mode", "mode_count"):
                best = max(runs.values())
                winner = min(v for v, cnt in runs.items() if cnt == best)       # ties: the first in ascending order
                out.append(best if op == "mode_count" else first[winner])
            else:
                vals = [first[v] for v in sorted(runs)]
                if is_f:
                    t = float(np.add.reduce(np.array(vals, np.float64)))      # (integer-valued or specials: any association agrees)
                else:
                    t = (sum(vals) + (1 << 63)) % (1 << 64) - (1 << 63)
                out.append(t if op == "sum_distinct" else float(np.float64(t) / np.float64(len(runs))))
        rows.append(tuple(out))
    return rows


NAN_A, NAN_B = np.array([0x7FF8000000000001, 0xFFF8000000000002], np.uint64).view(np.float64)
CASES = {
    "ints at the ends": (["a", "b", "x"], [np.array([1, 1, 1, 2, 2, 3, 1]), np.array([I_MIN, I_MAX, I_MAX, 0, 0, -1, 5]), np.array([I_MAX, I_MAX, I_MIN, I_MIN, I_MIN, 7, 2])]),
    "wrap-around": (["a", "b", "x"], [np.array([1, 1, 1, 1, 2]), np.array([0, 0, 0, 0, 0]), np.array([I_MAX, I_MAX - 1, I_MAX, 5, I_MIN])]),
    "doubles": (["a", "b", "x"], [np.array([0.0, -0.0, -0.0, np.inf, -np.inf, np.nan, np.nan, 2.0]), np.array([1, 1, 1, 2, 2, 2, 3, 3]),
                                  np.array([np.nan, -0.0, 0.0, np.inf, 4.0, np.nan, -np.inf, 3.0])]),
    "zeros and nans": (["a", "b", "x"], [np.array([1, 1, 1, 1, 1, 1, 1, 1]), np.array([2, 2, 2, 2, 2, 2, 2, 2]), np.array([0.0, -0.0, NAN_A, NAN_B, NAN_A, -0.0, 0.0, NAN_B])]),
    "mode ties": (["a", "b", "x"], [np.array([1, 1, 1, 1, 1, 1, 2, 2, 2]), np.array([9, 9, 9, 9, 9, 9, 9, 9, 9]), np.array([7, 3, 7, 3, 5, 5, 4, 4, 4])]),
    "text": (["a", "b", "x"], [np.array(["pear", "apple", "pear", "", "fig", "apple"]), np.array([2, 1, 2, 2, 1, 1]), np.array([1.5, 2.0, 4.0, 8.0, 16.0, 32.0])]),
    "empty": (["a", "b", "x"], [np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64)]),
    "one row": (["a", "b", "x"], [np.array([5]), np.array(["t"]), np.array([2.5])]),
    "all rows equal": (["a", "b", "x"], [np.full(9, 3), np.full(9, -0.0), np.full(9, I_MAX)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_distincted_against_a_dict_of_lists(case):
    columns, arrays = CASES[case]
    rs = ResultSet(columns, arrays)
    numeric = {"d": ("count_distinct", "x"), "s": ("sum_distinct", "x"), "v": ("avg_distinct", "x"), "m": ("mode", "x"), "c": ("mode_count", "x"), "n": ("count", None)}
    other = {"d": ("count_distinct", "b"), "m": ("mode", "b"), "c": ("mode_count", "b"), "n": ("count", None), "e": ("count_distinct", "x")}     # b may be text: no sums
    for by, aggs in ((["a"], numeric), ([("a", "desc")], numeric), ([], numeric), (["a", ("b", "desc")], numeric), (["a"], other), ([("a", "desc")], other), ([], other)):
        req = distinct_request(columns, by, aggs)
        got = rs.distincted(req)
        assert got.columns == [nm for nm, _ in req.by] + list(aggs)
        _same_rows(got.ordered_rows(), _brute(columns, arrays, req))
        kind = {nm: np.asarray(a).dtype.kind for nm, a in zip(columns, arrays)}
        want = [kind[nm] for nm, _ in req.by] + [{"count_distinct": "i", "mode_count": "i", "count": "i", "avg_distinct": "f"}.get(op, kind.get(c)) for _, op, c in req.aggs]
        assert [a.dtype.kind for a in got.arrays] == want
    _same_rows(rs.distincts(["a"], numeric).ordered_rows(), rs.distincted(distinct_request(columns, ["a"], numeric)).ordered_rows())
    _same_rows(rs.windowed(distinct_request(columns, ["a"], numeric)).ordered_rows(), rs.distincts(["a"], numeric).ordered_rows())
    if not len(arrays[0]):
        assert len(rs.distincts([], numeric)) == 0                          # no group of nothing
    if case == "zeros and nans":
        assert rs.distincts(["a"], numeric).column("d").tolist() == [4]     # -0.0, +0.0 and two NaN payloads: four values
    if case == "wrap-around":
        assert rs.distincts(["a"], numeric).column("s").tolist() == [(2 * I_MAX - 1 + 5 + (1 << 63)) % (1 << 64) - (1 << 63), I_MIN]
    if case == "mode ties":
        assert rs.distincts(["a"], numeric).column("m").tolist() == [3, 4] and rs.distincts(["a"], numeric).column("c").tolist() == [2, 3]
    if case == "text":
        with pytest.raises(ValueError):
            rs.distincts(["b"], {"s": ("sum_distinct", "a")})


# ---- routing, on a stub engine ---------------------------------------------------------------------------------------------------------
def _stub(**kw):
    lib = SimpleNamespace(has_group_distinct=kw.pop("has", True), has_grouping_sets=True, has_window_agg=True, has_sort_terms=True)
    return SimpleNamespace(device_group_distinct=kw.pop("on", True), ctx=SimpleNamespace(library=lib), device_sort=True, order_routes=[])


def _spec(terms, measures, int_values=()):
    spec = engine._FrameSpec(terms)
    spec.measures, spec.int_values = measures, int_values
    return spec


def test_routing():
    K, P, V = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE
    terms = [(P, 0, False, False), (K, 0, False, False), (V, 0, False, True)]      # by p; the value columns k and x
    mk, mx = (K, 0, False, False), (V, 0, False, True)
    aggs = {"d": ("count_distinct", "k"), "m": ("mode", "k"), "s": ("sum_distinct", "x"), "n": ("count", None)}
    req = distinct_request(None, ["p"], aggs)
    fits = _spec(terms, [None, mk, mx, None])
    assert engine._order_route(_stub(), req, fits) == "group_distinct"
    assert engine._order_route(_stub(on=False), req, fits) == "host"       # the switch
    assert engine._order_route(_stub(has=False), req, fits) == "host"      # a library without the extension
    assert engine._order_route(_stub(), req, None) == "host"               # a column the device cannot order by
    five = distinct_request(None, ["p"], {n: (op, "k") for n, op in zip("abcde", DISTINCT_OPS[:5])})
    assert engine._order_route(_stub(), five, _spec(terms[:2], [None, mk, mk, mk, None])) == "host"      # more than GD_MAX_AGGS over one value column
    four = distinct_request(None, ["p"], {n: (op, "k") for n, op in zip("abcd", DISTINCT_OPS[:4])})
    assert engine._order_route(_stub(), four, _spec(terms[:2], [None, mk, mk, mk])) == "group_distinct"
    eight = distinct_request(None, ["p"], dict({n: (op, "k") for n, op in zip("abcd", DISTINCT_OPS[:4])}, **{n: (op, "x") for n, op in zip("efgh", DISTINCT_OPS[:4])}))
    assert engine._order_route(_stub(), eight, _spec(terms, [None, mk, mk, mk, None, mx, mx, mx])) == "group_distinct"      # four per value column, two calls
    assert engine._order_route(_stub(), req, _spec(terms, None)) == "host"                     # a text mode / sum: no plain column to read
    assert engine._order_route(_stub(), distinct_request(None, ["p"], {"n": ("count", None)}), _spec(terms[:1], [None])) == "host"      # no value column
    nine = distinct_request(None, list("abcdefgh"), {"z": ("count_distinct", "x")})
    assert engine._order_route(_stub(), nine, _spec([(K, 0, False, False)] * 9, [None])) == "host"       # more than SORT_MAX_KEYS terms
    text = [(P, 0, False, False), (K, 0, False, False, 0, 0, 0, "ranks of some text"), (V, 0, False, True)]
    assert engine._order_route(_stub(), req, _spec(text, [None, mk, mx, None])) == "group_distinct"      # a text value column is counted through its ranks
    assert engine._WINDOW_ROUTES[0] == (DistinctRequest, "group_distinct", "device_group_distinct", "has_group_distinct", "aggs", abi.GD_MAX_AGGS)
    eng = _stub()
    engine._note_order_route(eng, req, _spec(text, [None, mk, mx, None]), "group_distinct")
    assert eng.order_routes[-1] == {"route": "group_distinct", "k": ALL, "order": ["k", "x"], "ranked": ["k"], "per": ["p"], "aggs": [list(a) for a in req.aggs], "calls": 2,
                                    "host_measures": False}
    engine._note_order_route(eng, req, _spec(text, None), "host")
    assert eng.order_routes[-1]["route"] == "host" and eng.order_routes[-1]["calls"] == 0 and eng.order_routes[-1]["host_measures"] is True
    made = engine._order_spec(req, lambda order, derive: [(K, 0, False, False)] * len(order), lambda nm: False)
    assert isinstance(made, engine._FrameSpec) and len(made) == 3 and made.measures == [None, (K, 0, False, False), (K, 0, False, False), None]      # count_distinct reads no measure
    asked = []
    engine._order_spec(distinct_request(None, ["p"], {"d": ("count_distinct", "t"), "c": ("mode_count", "t")}), lambda order, derive: asked.append((list(order), derive)) or [mk] * len(order),
                       lambda nm: False)
    assert asked == [([("p", "asc"), ("t", "asc")], True)]                  # counting a text column's values asks for no plain column of it

    # one call per value column, the aggregates back in the request's order
    class Ctx:
        calls = []

        def table_group_distinct(self, table, min_hits, call_terms, ngroup, call_aggs, limit, cap, want_hits=True):
            self.calls.append((call_terms, ngroup, call_aggs))
            g = np.arange(3, dtype=np.int64)
            return g, None, None, None, [np.full(3, 100 * len(self.calls) + i, np.int64) for i in range(len(call_aggs))]
    eng = SimpleNamespace(ctx=Ctx())
    got = engine._distinct_calls(eng, "table", 1, req, terms, fits, 4096, False)
    assert [c[:2] for c in Ctx.calls] == [([terms[0], terms[1]], 1), ([terms[0], terms[2]], 1)]
    assert Ctx.calls[0][2] == [(abi.GD_COUNT_DISTINCT, K, 0, False), (abi.GD_MODE, K, 0, False), (abi.GD_COUNT, K, 0, False)] and Ctx.calls[1][2] == [(abi.GD_SUM_DISTINCT, V, 0, True)]
    assert [int(a[0]) for a in got[4]] == [100, 101, 200, 102] and got[0].tolist() == [0, 1, 2]
    # the last mile: `by` of the groups' rows and a column per aggregate
    rows = ResultSet(["p", "k", "x"], [np.array([1, 2, 3]), np.array([7, 8, 7]), np.zeros(3)])
    done = engine._finish_top(rows, SimpleNamespace(rank=got[4]), req)
    assert done.columns == ["p", "d", "m", "s", "n"] and done.ordered_rows() == [(1, 100, 101, 200, 102), (2, 100, 101, 200, 102), (3, 100, 101, 200, 102)]
    assert engine._finish_top(rows, False, req).columns == ["p", "d", "m", "s", "n"]           # not ordered: the host route


def test_the_switch_is_read_from_the_environment(oracle_lib, monkeypatch):
    for value, on in (("0", False), ("1", True)):
        monkeypatch.setenv("SDQLPY_AMD_DEVICE_GROUP_DISTINCT", value)
        eng = engine.Engine(oracle_lib.context(threads=1))
        try:
            assert eng.device_group_distinct is on
        finally:
            eng.close()
