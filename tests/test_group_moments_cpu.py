"""The second moments per group, the part that needs no GPU: the group moments extension's symbols (include/sdqh_sort_moments.h,
abi.GROUP_MOMENTS_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without them, the argument checks of a
compile-only context, the request, ResultSet.moments against exact rationals within the header's bounds (moments_reference), the
rollup form against ResultSet.rollup, and the routing decision, the device call and the last mile on a stub engine."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import moments_reference as ref
from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import dist as sdist
from sdqlpy_amd.result import MOMENT_OPS, MomentsRequest, ResultSet, WindowRequest, moments_request
from test_request_routes_cpu import _Recorder
from test_window_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
UNI, BI = MOMENT_OPS[:4], MOMENT_OPS[4:]


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib, oracle_lib):
    assert sorted(abi.GROUP_MOMENTS_EXPORTS) == _declared("sdqh_sort_moments.h") == ["sdqh_group_moments_geometry", "sdqh_table_group_moments"]
    for s in abi.GROUP_MOMENTS_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert not hasattr(oracle_lib.cdll, s), s
        for flag, (exports, header, _, _) in abi.WINDOW_EXTENSIONS.items():
            if flag != "has_group_moments":
                assert s not in exports and s not in _declared(header), (s, header)
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
        assert s not in abi.EXPORTS and s not in abi.SORT_EXPORTS and s not in abi.SORT_TERMS_EXPORTS and s not in abi.EXTREMA_EXPORTS
    assert hip_lib.has_group_moments and hip_lib.has_grouping_sets and oracle_lib.has_group_moments is False and abi.ABI_VERSION == 7
    assert abi.WINDOW_EXTENSIONS["has_group_moments"] == (abi.GROUP_MOMENTS_EXPORTS, "sdqh_sort_moments.h", "group moments", "has_grouping_sets")
    assert C.sizeof(abi.MomentAgg) == 32
    text = open(os.path.join(ROOT, "include", "sdqh_sort_moments.h")).read()
    assert re.search(r"#define\s+SDQH_GM_MAX_AGGS\s+%d\b" % abi.GM_MAX_AGGS, text) and abi.GM_MAX_AGGS == 4
    for value, name in enumerate(MOMENT_OPS):                              # the request's names are the header's numbers and the binding's
        assert re.search(r"#define\s+SDQH_GM_%s\s+%d\b" % (name.upper(), value), text), name
        assert getattr(abi, "GM_" + name.upper()) == value
    assert len(MOMENT_OPS) == 9 and MOMENT_OPS == ref.OPS
    main = open(os.path.join(ROOT, "include", "sdqh.h")).read()
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", main) and "sdqh_sort_moments.h" not in main


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        key = (abi.SORT_KEY, 0, False, False)
        agg = [(abi.GM_VAR_POP, abi.SORT_HITS, 0, False)]
        for f in (lambda: ctx.table_group_moments(t, 0, [key], 2, agg, ALL, 16), lambda: ctx.table_group_moments_count(t, 0, [key], 2, agg), ctx.group_moments_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no group moments extension (include/sdqh_sort_moments.h)" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses_after_the_argument_checks(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.group_moments_geometry() == ctx.grouping_sets_geometry() >= 64      # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context: a key, hits, no payload
        key, hits = (abi.SORT_KEY, 0, False, False), (abi.SORT_HITS, 0, True, False)
        K, H, P, V = abi.SORT_KEY, abi.SORT_HITS, abi.SORT_PAYLOAD, abi.SORT_VALUE
        good = [([key], 2, [(abi.GM_VAR_POP, K, 0, False)]), ([key, hits], 7, [(op, H, 0, False, K, 0, False) for op in range(4, 8)]),
                ([key], 1, [(abi.GM_STDDEV_SAMP, H, 0, False, P, 9, True)]),      # a univariate op ignores its second measure
                ([key] * 8, 1 << 8, [(abi.GM_REGR_INTERCEPT, K, 0, False, H, 0, False)])]
        for terms, levels, aggs in good:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_group_moments(table, 0, terms, levels, aggs, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED and "compile-only" in str(e.value), (terms, levels, aggs)
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_group_moments_count(table, 0, terms, levels, aggs)
            assert e.value.code == abi.ERR_UNSUPPORTED
        var = (abi.GM_VAR_POP, K, 0, False)
        bad_calls = [
            ([key], 2, [(-1, K, 0, False)]), ([key], 2, [(9, K, 0, False)]), ([key], 2, [var, (99, K, 0, False)]),                      # unknown op
            ([key], 2, [(abi.GM_VAR_SAMP, P, 0, False)]), ([key], 2, [(abi.GM_CORR, K, 0, False, V, 9, True)]), ([key], 2, [(abi.GM_CORR, V, -1, True, K, 0, False)]),      # a measure the table lacks
            ([key], 2, [(abi.GM_VAR_POP, K, 0, True)]), ([key], 2, [(abi.GM_STDDEV_POP, H, 0, True)]),                                  # is_f64 on KEY / HITS, either measure
            ([key], 2, [(abi.GM_COVAR_POP, K, 0, False, K, 0, True)]), ([key], 2, [(abi.GM_REGR_SLOPE, H, 0, False, H, 0, True)]),
            ([key], 2, [var] * 5), ([key], 2, []),                                                                                       # five aggregates, none
            ([key], 0, [var]), ([key], 4, [var]), ([key, hits], 8, [var]),                                                              # levels 0, a bit above nterms
            ([], 1, [var]), ([key] * 9, 1, [var]),                                                                                      # no term, nine terms
        ]
        for terms, levels, bad in bad_calls:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_group_moments(table, 0, terms, levels, bad, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, (terms, levels, bad)   # the argument checks — the measures' too — come first
        n = C.c_int64(-5)
        out = np.full((4, 16), -7, np.int64)
        lr = np.full(abi.SORT_MAX_KEYS + 1, -7, np.int64)
        arr = abi._marshal_moment_aggs([(abi.GM_VAR_POP, P, 0, False)])     # nothing is written on either way out, *out_n included
        two = abi._marshal_sort_terms([key, hits])
        for naggs, aggs, limit, cap in ((1, arr, ALL, 16), (0, arr, ALL, 16), (5, arr, ALL, 16), (1, None, ALL, 16), (1, arr, 0, 16), (1, arr, ALL, -1)):
            rc = ctx.lib.sdqh_table_group_moments(ctx.handle, table.handle, C.c_int64(0), C.c_int(2), two, C.c_uint32(4), C.c_int(naggs), aggs, C.c_int64(limit), C.c_int64(cap),
                                                  out[0].ctypes.data_as(C.c_void_p), None, None, out[1].ctypes.data_as(C.c_void_p), out[2:].ctypes.data_as(C.c_void_p),
                                                  lr.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == abi.ERR_INVALID and n.value == -5 and (out == -7).all() and (lr == -7).all(), (naggs, limit, cap)
    finally:
        ctx.close()


# ---- the request -------------------------------------------------------------------------------------------------------------------
def test_request_errors_come_before_anything_is_launched():
    cols = ["a", "b", "c", "x", "y"]
    ok = moments_request(cols, ["a", ("b", "desc")], {"s": ("stddev_samp", "x"), "t": ("regr_slope", "y", "x"), "r": ("corr", "x", "y")})
    assert isinstance(ok, MomentsRequest) and isinstance(ok, WindowRequest) and ok[0] == ALL
    assert ok[1] == [("a", "asc"), ("b", "desc")] and ok.npartition == 2 and ok.order == [] and ok.rollup is False and ok.sets == [("a", "b")]
    assert ok.aggs == [("s", "stddev_samp", "x", None), ("t", "regr_slope", "y", "x"), ("r", "corr", "x", "y")]
    rolled = moments_request(cols, ["a", "b"], {"s": ("var_pop", "x")}, rollup=True)
    assert rolled.rollup and rolled.sets == [("a", "b"), ("a",), ()] and rolled.masks() == [0, 1, 3]
    assert moments_request(None, ["zz"], {"d": ("var_pop", "qq")})[1] == [("zz", "asc")]      # names checked when the result is known
    for op in UNI:
        with pytest.raises(ValueError):
            moments_request(cols, ["a"], {"d": (op, "x", "y")})               # a univariate op given two columns
        assert moments_request(cols, ["a"], {"d": (op, "x")}).aggs == [("d", op, "x", None)]
    for op in BI:
        with pytest.raises(ValueError):
            moments_request(cols, ["a"], {"d": (op, "x")})                    # a bivariate op given one
        assert moments_request(cols, ["a"], {"d": (op, "y", "x")}).aggs == [("d", op, "y", "x")]
    for by, aggs, err in ((["a", "a"], {"d": ("var_pop", "x")}, ValueError), (["zz"], {"d": ("var_pop", "x")}, KeyError), (["a"], {"d": ("var_pop", "zz")}, KeyError),
                          (["a"], {"d": ("corr", "x", "zz")}, KeyError), (["a"], {"b": ("var_pop", "x")}, KeyError), (["a"], {"a": ("var_pop", "x")}, ValueError),
                          (["a"], {"d": ("variance", "x")}, ValueError), (["a"], {"d": ("var_pop", None)}, ValueError), (["a"], {"d": ("var_pop",)}, ValueError),
                          (["a"], {}, ValueError), (["a"], [], ValueError), ("a", {"d": ("var_pop", "x")}, ValueError), ([], {"d": ("var_pop", "x")}, ValueError),
                          ([("a", "up")], {"d": ("var_pop", "x")}, ValueError), (["a"], {"d": ("var_pop", "a")}, ValueError), (["a"], {"d": ("corr", "x", "a")}, ValueError),
                          (["a"], {"d": ("covar_pop", "x", 3)}, ValueError), ([3], {"d": ("var_pop", "x")}, ValueError)):
        with pytest.raises(err):
            moments_request(cols, by, aggs)
    with pytest.raises(ValueError):
        moments_request(cols, ["a"], {"grouping": ("var_pop", "x")}, rollup=True)
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(ok)
    assert "moments runs on one GPU" in str(e.value)
    again = ok.renamed([("A", "asc"), ("B", "desc")], {"x": "X", "y": "Y"})
    assert again[1] == [("A", "asc"), ("B", "desc")] and again.aggs == [("s", "stddev_samp", "X", None), ("t", "regr_slope", "Y", "X"), ("r", "corr", "X", "Y")]


# ---- ResultSet.moments against exact rationals --------------------------------------------------------------------------------------
EVERY = dict({op: (op, "y") for op in UNI}, **{op: (op, "y", "x") for op in BI})


def _groups(rs, by):
    """{the by-values of a group: its row indices}, the groups in the result's order (integer grouping columns, ascending)"""
    cols = [np.asarray(rs.column(c)) for c in by]
    out = {}
    for r in range(len(rs)):
        out.setdefault(tuple(int(c[r]) for c in cols), []).append(r)
    return dict(sorted(out.items()))


def _check_all(rs, by, what):
    got = rs.moments(by, EVERY)
    assert got.columns == by + list(EVERY) and all(a.dtype == np.float64 for a in got.arrays[len(by):])
    groups = _groups(rs, by)
    assert [tuple(int(v) for v in row[:len(by)]) for row in got.ordered_rows()] == list(groups)
    x, y = np.asarray(rs.column("x"), np.float64), np.asarray(rs.column("y"), np.float64)
    worst = 0.0
    for j, rows in enumerate(groups.values()):
        for op in MOMENT_OPS:
            worst = max(worst, ref.check(op, got.column(op)[j], y[rows], x[rows] if op in BI else None, (what, j)))
    return worst


def _offset_data(rng, n):
    x = 1e6 + rng.standard_normal(n)
    return x, -3e6 + 2.0 * (x - 1e6) + 0.01 * rng.standard_normal(n)


def test_moments_within_the_bounds_on_wide_magnitudes_and_on_offset_data():
    rng = np.random.default_rng(20261020)
    n = 1500
    g = np.concatenate([np.repeat(np.arange(100), 3), np.repeat(np.arange(100, 103), 65), np.full(n - 300 - 195, 200)])      # groups of 3, of 65, one of 1005
    wide = lambda: rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)                                              # noqa: E731
    order = rng.permutation(n)
    a = ResultSet(["g", "x", "y"], [g[order], wide()[order], wide()[order]])
    assert _check_all(a, ["g"], "wide") < 1.0
    x, y = _offset_data(rng, n)
    b = ResultSet(["g", "x", "y"], [g[order], x[order], y[order]])
    assert _check_all(b, ["g"], "offset") < 1.0
    slopes = b.moments(["g"], {"t": ("regr_slope", "y", "x")}).column("t")
    assert abs(slopes[-1] - 2.0) < 1e-2                                      # (the data's own slope, for orientation)


def test_the_naive_formula_misses_the_bound_on_offset_data():
    rng = np.random.default_rng(7)
    x, _ = _offset_data(rng, 1025)
    e = ref.Exact(x)
    want, bound = e.value("var_pop")
    two_pass = ResultSet(["g", "y"], [np.zeros(1025, np.int64), x]).moments(["g"], {"v": ("var_pop", "y")}).column("v")[0]
    assert abs(two_pass - want) <= bound
    assert abs(ref.naive_variance(x) - want) > 1000 * bound                  # the bound bites: sum x^2 - (sum x)^2 / m is nowhere near it


def test_exact_cases_constant_groups_ones_twos_and_int64_ends():
    null = ref.NULL_BITS
    # (c) constant groups of 1, 2, 65 rows of 0.1, 1e300, -0.0: every Q is +0.0 by bits
    for v in (0.1, 1e300, -0.0):
        g = np.concatenate([np.full(1, 0), np.full(2, 1), np.full(65, 2)])
        rs = ResultSet(["g", "x", "y"], [g, np.arange(68, dtype=np.float64), np.full(68, v)])
        got = rs.moments(["g"], dict(EVERY, swapped=("corr", "x", "y"), slope_on_const=("regr_slope", "x", "y")))
        for op in ("var_pop", "stddev_pop", "covar_pop"):
            assert ref.bits(got.column(op)).tolist() == [0, 0, 0], (v, op)
        for op in ("var_samp", "stddev_samp", "covar_samp"):
            assert ref.bits(got.column(op)).tolist() == [null, 0, 0], (v, op)
        assert ref.bits(got.column("corr")).tolist() == [null] * 3 and ref.bits(got.column("swapped")).tolist() == [null] * 3      # Qy = 0
        assert ref.bits(got.column("slope_on_const")).tolist() == [null] * 3                                                     # its x is the constant column
        assert ref.bits(got.column("regr_slope")).tolist() == [null, 0, 0] and ref.bits(got.column("regr_intercept"))[0] == null    # C = 0 over Qx > 0; one row: Qx = 0
        assert got.column("regr_intercept")[1:].tolist() == [v, v]
    # (d) groups of one and of two, every op against the definition
    g = np.array([0, 1, 1, 2, 3, 3])
    rs = ResultSet(["g", "x", "y"], [g, np.array([5.0, 1.0, 3.0, -2.0, 1e10, 1e10 + 2]), np.array([7.0, 10.0, 20.0, 0.5, -1.0, 3.0])])
    assert _check_all(rs, ["g"], "ones and twos") < 1.0
    got = rs.moments(["g"], EVERY)
    assert got.column("var_pop").tolist() == [0.0, 25.0, 0.0, 4.0] and got.column("var_samp")[[1, 3]].tolist() == [50.0, 8.0]
    assert got.column("regr_slope")[[1, 3]].tolist() == [5.0, 2.0] and all(ref.ulps(c, 1.0) <= 4 for c in got.column("corr")[[1, 3]])
    # (e) int64 measures, the ends included: converted to double once, doubles from then on
    ints = np.array([I_MIN, I_MAX, 0, 1, -1, I_MAX, I_MAX - 1, I_MIN], np.int64)
    other = np.array([3, -4, I_MAX, 7, 7, 8, I_MIN, 0], np.int64)
    rs = ResultSet(["g", "x", "y"], [np.array([0, 0, 0, 1, 1, 2, 2, 2]), ints, other])
    got = rs.moments(["g"], EVERY)
    xs, ys = ints.astype(np.float64), other.astype(np.float64)
    for j, rows in enumerate(([0, 1, 2], [3, 4], [5, 6, 7])):
        for op in MOMENT_OPS:
            ref.check(op, got.column(op)[j], ys[rows], xs[rows] if op in BI else None, ("int64", j))
    # (f) an empty result: no group, not even with rollup
    empty = ResultSet(["g", "x", "y"], [np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64)])
    assert len(empty.moments(["g"], EVERY)) == 0 and empty.moments(["g"], EVERY).columns == ["g"] + list(EVERY)
    assert len(empty.moments(["g"], EVERY, rollup=True)) == 0
    with pytest.raises(ValueError):
        ResultSet(["g", "t"], [np.array([1, 2]), np.array(["a", "b"])]).moments(["g"], {"v": ("var_pop", "t")})      # a text measure


def test_symmetry_by_bits_on_the_host():
    rng = np.random.default_rng(3)
    n = 400
    rs = ResultSet(["g", "x", "y"], [rng.integers(0, 9, n), rng.standard_normal(n) * 1e3 + 5e5, rng.standard_normal(n)])
    got = rs.moments(["g"], {"a": ("covar_pop", "x", "y"), "b": ("covar_pop", "y", "x"), "c": ("corr", "x", "y"), "d": ("corr", "y", "x"), "e": ("covar_pop", "x", "x"),
                             "f": ("var_pop", "x"), "p": ("covar_samp", "x", "y"), "q": ("covar_samp", "y", "x")})
    for a, b in ("ab", "cd", "ef", "pq"):
        assert (ref.bits(got.column(a)) == ref.bits(got.column(b))).all(), (a, b)


def test_rollup_has_the_sets_order_masks_and_fill_of_resultset_rollup():
    rng = np.random.default_rng(11)
    n = 300
    rs = ResultSet(["a", "b", "t", "x"], [rng.integers(0, 5, n), rng.integers(-2, 2, n).astype(np.float64), rng.choice(["p", "q", ""], n), rng.standard_normal(n)])
    for by in (["a", "b"], [("b", "desc"), "a"], ["t", "a"], ["a"]):
        names = [c if isinstance(c, str) else c[0] for c in by]
        got = rs.moments(by, {"v": ("var_pop", "x"), "s": ("stddev_samp", "x")}, rollup=True)
        want = rs.rollup(by, {"n": ("count", None), "m": ("avg", "x")})
        assert got.columns == names + ["v", "s", "grouping"] and len(got) == len(want)
        for c in names + ["grouping"]:
            g, w = np.asarray(got.column(c)), np.asarray(want.column(c))
            assert g.dtype == w.dtype and (g.astype(str) == w.astype(str)).all(), (by, c)      # NaN fills compare as text
        counts = want.column("n")
        assert (ref.bits(got.column("s"))[counts == 1] == ref.NULL_BITS).all() and np.isfinite(got.column("s")[counts > 1]).all()
        assert abs(got.column("v")[-1] - np.var(rs.column("x"))) < 1e-12        # the grand total, last
        plain = rs.moments(by, {"v": ("var_pop", "x")})
        assert plain.columns == names + ["v"] and (ref.bits(plain.column("v")) == ref.bits(got.column("v")[:len(plain)])).all()
    assert rs.windowed(moments_request(rs.columns, ["a"], {"v": ("var_pop", "x")})).ordered_rows() == rs.moments(["a"], {"v": ("var_pop", "x")}).ordered_rows()


# ---- routing, on a stub engine ---------------------------------------------------------------------------------------------------------
def _stub(**kw):
    lib = SimpleNamespace(has_group_moments=kw.pop("has", True), has_grouping_sets=True, has_window_agg=True, has_sort_terms=True)
    return SimpleNamespace(device_group_moments=kw.pop("on", True), ctx=SimpleNamespace(library=lib), device_sort=True, order_routes=[])


def _spec(terms, measures, int_values=()):
    spec = engine._FrameSpec(terms)
    spec.measures, spec.int_values = measures, int_values
    return spec


def test_routing():
    K, P, V = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE
    terms = [(P, 0, False, False), (K, 0, True, False)]
    mx, my = (V, 0, False, True), (V, 1, False, True)
    req = moments_request(None, ["p", ("k", "desc")], {"s": ("stddev_samp", "y"), "t": ("regr_slope", "y", "x")}, rollup=True)
    fits = _spec(terms, [[my], [my, mx]])
    assert engine._order_route(_stub(), req, fits) == "group_moments"
    assert engine._order_route(_stub(on=False), req, fits) == "host"       # the switch
    assert engine._order_route(_stub(has=False), req, fits) == "host"      # a library without the extension
    assert engine._order_route(_stub(), req, None) == "host"               # a column the device cannot order by
    assert engine._order_route(_stub(), req, _spec(terms, None)) == "host"      # a text measure: no plain column to read
    five = moments_request(None, ["p"], {n: ("var_pop", "y") for n in "abcde"})
    assert engine._order_route(_stub(), five, _spec(terms[:1], [[my]] * 5)) == "host"      # more than GM_MAX_AGGS
    four = moments_request(None, ["p"], {n: ("corr", "y", "x") for n in "abcd"})
    assert engine._order_route(_stub(), four, _spec(terms[:1], [[my, mx]] * 4)) == "group_moments"
    nine = moments_request(None, list("abcdefghi"), {"z": ("var_pop", "y")})
    assert engine._order_route(_stub(), nine, _spec([(K, 0, False, False)] * 9, [[my]])) == "host"      # more than SORT_MAX_KEYS terms
    rec = engine._route_of(req)
    assert rec == (MomentsRequest, "group_moments", "device_group_moments", "has_group_moments", "aggs", abi.GM_MAX_AGGS) and rec.env == "SDQLPY_AMD_DEVICE_GROUP_MOMENTS"
    assert rec in engine._WINDOW_ROUTES and engine._WINDOW_ROUTES[0].route == "group_distinct" and not any(rec.integral(item) for item in req.items)
    eng = _stub()
    engine._note_order_route(eng, req, fits, "group_moments")
    assert eng.order_routes[-1] == {"route": "group_moments", "k": ALL, "order": [], "ranked": [], "per": ["p", "k"], "aggs": [list(a) for a in req.aggs], "rollup": True, "calls": 1}
    engine._note_order_route(eng, req, None, "host")
    assert eng.order_routes[-1]["route"] == "host" and eng.order_routes[-1]["calls"] == 0
    # a column may name a pair of measures; what existing requests receive is what it was
    asked = []
    made = engine._order_spec(req, lambda order, derive: asked.append((list(order), derive)) or [(V, i, False, True) for i in range(len(order))], lambda nm: False)
    assert isinstance(made, engine._FrameSpec) and made.measures == [[(V, 0, False, True)], [(V, 0, False, True), (V, 1, False, True)]]
    assert asked == [([("p", "asc"), ("k", "desc")], True), ([("y", "asc"), ("x", "asc")], False)]
    assert engine._order_spec(req, lambda order, derive: None if not derive else [mx] * len(order), lambda nm: False).measures is None


class _MomentsRecorder(_Recorder):
    def table_compact_into_block(self, table, *args, **kwargs):           # the host route's rows: all three
        self.calls.append(("table_compact_into_block", args, kwargs))
        return self._rows(3) + (3,)

    def table_group_moments(self, table, *args, **kwargs):
        self.calls.append(("table_group_moments", args, kwargs))
        levels = [length for length in range(abi.SORT_MAX_KEYS, -1, -1) if args[2] >> length & 1]
        level_rows = np.zeros(abi.SORT_MAX_KEYS + 1, np.int64)
        level_rows[levels] = 1
        return self._rows(len(levels)) + ([np.array([2.0, 4.0, 6.0][:len(levels)]) + i for i, _ in enumerate(args[3])], level_rows)


def _run(req_of, **eng_kw):
    ctx = _MomentsRecorder()
    eng = SimpleNamespace(ctx=ctx, device_sort=True, order_routes=[], compact_hints={}, lazy_results=False, **eng_kw)
    bt = SimpleNamespace(agg=([("p", "key")], ["x", "k"], None, True, True, 2), shared_groups=False, agg_fields={}, int_values=("x",), table=object(), key_radix=None,
                         key_parts=None, key_decoder=None, decoder_of=lambda field, src: None, payload_dtypes={})
    op = SimpleNamespace(source="groups", out="result", lineno=1, fields=[("grp", 0, "p"), ("ord", 1, "k"), ("val", 1, "x")])
    rs = engine._finalize(eng, op, {"groups": ("aggregated", "bt"), "bt": bt}, req_of(["grp", "ord", "val"]))
    return eng.order_routes[-1], ctx.calls, rs


def test_through_finalize_on_a_recording_context():
    K, V = abi.SORT_KEY, abi.SORT_VALUE
    aggs = {"s": ("stddev_samp", "val"), "t": ("regr_slope", "val", "ord")}
    note, calls, rs = _run(lambda cols: moments_request(cols, ["grp"], aggs))
    assert note == {"route": "group_moments", "k": ALL, "order": [], "ranked": [], "per": ["grp"], "aggs": [["s", "stddev_samp", "val", None], ["t", "regr_slope", "val", "ord"]],
                    "rollup": False, "calls": 1}
    assert calls == [("table_group_moments", (1, [(K, 0, False, False)], 2, [(abi.GM_STDDEV_SAMP, V, 0, True), (abi.GM_REGR_SLOPE, V, 0, True, V, 1, True)], ALL, 4096), {"want_hits": False})]
    assert [(n, a.dtype.str) for n, a in zip(rs.columns, rs.arrays)] == [("grp", "<i8"), ("s", "<f8"), ("t", "<f8")] and rs.ordered_rows() == [(1, 2.0, 3.0)]
    note, calls, rs = _run(lambda cols: moments_request(cols, ["grp"], aggs, rollup=True))
    assert note["rollup"] is True and note["calls"] == 1 and calls[0][1][2] == 3
    assert rs.columns == ["grp", "s", "t", "grouping"] and rs.ordered_rows() == [(1, 2.0, 3.0, 0), (0, 4.0, 5.0, 1)]
    # five aggregates, and the switch off: the host route, no device call
    note, calls, rs = _run(lambda cols: moments_request(cols, ["grp"], {n: ("var_pop", "val") for n in "abcde"}))
    assert note["route"] == "host" and note["calls"] == 0 and not [c for c in calls if c[0] == "table_group_moments"] and rs.columns == ["grp"] + list("abcde")
    note, calls, rs = _run(lambda cols: moments_request(cols, ["grp"], aggs), device_group_moments=False)
    assert note["route"] == "host" and not [c for c in calls if c[0] == "table_group_moments"] and rs.columns == ["grp", "s", "t"]


def test_the_switch_is_read_from_the_environment(oracle_lib, monkeypatch):
    for value, on in (("0", False), ("1", True)):
        monkeypatch.setenv("SDQLPY_AMD_DEVICE_GROUP_MOMENTS", value)
        eng = engine.Engine(oracle_lib.context(threads=1))
        try:
            assert eng.device_group_moments is on
        finally:
            eng.close()
