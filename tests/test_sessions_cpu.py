"""Sessions (gaps and islands), the part that needs no GPU: the sessions extension's symbols (include/sdqh_sort_sessions.h,
abi.SESSIONS_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without them, the argument checks of a
compile-only context in their order, the request, ResultSet.sessions against a brute-force reference (sessions_reference), and the
routing decision, the device call and the last mile on the stub engine of test_request_routes_cpu."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sessions_reference as ref
from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import dist as sdist
from sdqlpy_amd.result import SESSION_HOST_MAX_COLS, SESSION_OPS, ResultSet, SessionRequest, WindowRequest, sessions_request
from test_request_routes_cpu import _Recorder
from test_window_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1


def _bits(a):
    return [int(x) for x in np.ascontiguousarray(a).view(np.uint64)]


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib, oracle_lib):
    assert sorted(abi.SESSIONS_EXPORTS) == _declared("sdqh_sort_sessions.h") == ["sdqh_sessions_geometry", "sdqh_table_sessions"]
    for s in abi.SESSIONS_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert not hasattr(oracle_lib.cdll, s), s
        for flag, (exports, header, _, _) in abi.WINDOW_EXTENSIONS.items():
            if flag != "has_sessions":
                assert s not in exports and s not in _declared(header), (s, header)
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
        assert s not in abi.EXPORTS and s not in abi.SORT_EXPORTS and s not in abi.SORT_TERMS_EXPORTS and s not in abi.EXTREMA_EXPORTS
    assert hip_lib.has_sessions and hip_lib.has_grouping_sets and oracle_lib.has_sessions is False and abi.ABI_VERSION == 7
    assert abi.WINDOW_EXTENSIONS["has_sessions"] == (abi.SESSIONS_EXPORTS, "sdqh_sort_sessions.h", "sessions", "has_grouping_sets")
    assert C.sizeof(abi.SessionRule) == 24 and C.sizeof(abi.SessionCol) == 16
    text = open(os.path.join(ROOT, "include", "sdqh_sort_sessions.h")).read()
    assert re.search(r"#define\s+SDQH_SS_MAX_COLS\s+%d\b" % abi.SS_MAX_COLS, text) and abi.SS_MAX_COLS == 4
    for name, value in (("GAP", abi.SS_GAP), ("CHANGE", abi.SS_CHANGE), ("NUMBER", abi.SS_NUMBER), ("ROW", abi.SS_ROW)):
        assert re.search(r"#define\s+SDQH_SS_%s\s+%d\b" % (name, value), text), name
    for value, name in enumerate(SESSION_OPS):                             # the request's names are the binding's numbers
        assert getattr(abi, "SS_" + name.upper()) == value
    assert (abi.SS_SUM, abi.SS_COUNT, abi.SS_MIN, abi.SS_MAX, abi.SS_FIRST, abi.SS_LAST, abi.SS_AVG) == \
        (abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WSLIDE_FIRST, abi.WSLIDE_LAST, abi.WEX_AVG)
    assert SESSION_OPS == ref.OPS and (abi.SS_NUMBER, abi.SS_ROW) == (7, 8)
    main = open(os.path.join(ROOT, "include", "sdqh.h")).read()
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", main) and "sdqh_sort_sessions.h" not in main


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        key = (abi.SORT_KEY, 0, False, False)
        for f in (lambda: ctx.table_sessions(t, 0, 0, [key], (abi.SS_GAP, 1), [], ALL, 16), lambda: ctx.table_sessions_count(t, 0, 0, [key], (abi.SS_GAP, 1)), ctx.sessions_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no sessions extension (include/sdqh_sort_sessions.h)" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses_after_the_struct_checks_and_before_the_table_checks(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.sessions_geometry() == ctx.window_geometry() >= 64          # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context: a key, hits, no payload
        K, H, P, V = abi.SORT_KEY, abi.SORT_HITS, abi.SORT_PAYLOAD, abi.SORT_VALUE
        key, hits = (K, 0, False, False), (H, 0, True, False)
        gap1, change = (abi.SS_GAP, 1), (abi.SS_CHANGE, H, 0, False)
        # what reads the caller's structs alone passes them, and what needs the table is never looked at: SDQH_ERR_UNSUPPORTED
        unsupported = [
            (1, [key, hits], gap1, [(abi.SS_SUM, K, 0, False), (abi.SS_NUMBER, K, 0, False), (abi.SS_ROW, K, 0, False)], False),
            (0, [key], (abi.SS_GAP, 0), [], True), (1, [key], change, [(abi.SS_AVG, H, 0, False)], True), (0, [key], (abi.SS_GAP, I_MAX), [(abi.SS_COUNT, P, 9, True)], False),
            (0, [(V, 0, False, True)], (abi.SS_GAP, 0.5), [], False),
            (0, [key], gap1, [(abi.SS_SUM, P, 3, False)], False),                # a measure the table lacks
            (0, [key], gap1, [(abi.SS_MIN, K, 0, True)], False), (0, [key], gap1, [(abi.SS_LAST, H, 0, True)], True),      # is_f64 on KEY / HITS
            (0, [key], (abi.SS_CHANGE, P, 7, False), [], False), (0, [key], (abi.SS_CHANGE, K, 0, True), [], False),      # ... the marker's
            (0, [(P, 5, False, False)], gap1, [], False),                        # a term the table lacks
        ]
        for npart, terms, rule, cols, per in unsupported:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_sessions(table, 0, npart, terms, rule, cols, ALL, 16, per_session=per)
            assert e.value.code == abi.ERR_UNSUPPORTED and "compile-only" in str(e.value), (npart, terms, rule, cols, per)
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_sessions_count(table, 0, 0, [key], gap1, per_session=True)
        assert e.value.code == abi.ERR_UNSUPPORTED
        s = (abi.SS_SUM, K, 0, False)
        invalid = [
            (0, [key], (2, 0), [s], False), (0, [key], (-1, 0), [s], False),                         # an unknown rule
            (0, [key], gap1, [(-1, K, 0, False)], False), (0, [key], gap1, [(9, K, 0, False)], False), (0, [key], gap1, [s, (99, K, 0, False)], False),      # an unknown op
            (0, [key], gap1, [s] * 5, False),                                                        # five columns
            (0, [key], gap1, [(abi.SS_ROW, K, 0, False)], True),                                     # ROW per session
            (0, [key], (abi.SS_GAP, -1), [s], False), (0, [key], (abi.SS_GAP, I_MIN), [s], False),   # a negative gap
            (0, [(V, 0, False, True)], (abi.SS_GAP, -0.5), [s], False), (0, [(V, 0, False, True)], (abi.SS_GAP, float("inf")), [s], False),
            (0, [(V, 0, False, True)], (abi.SS_GAP, float("nan")), [s], False), (0, [(P, 0, False, True)], (abi.SS_GAP, float("-inf")), [s], False),
            (1, [key], gap1, [s], False), (2, [key, hits], gap1, [s], False),                        # no gap term behind the partition terms
            (0, [], gap1, [s], False), (0, [key] * 9, gap1, [s], False),                             # no term, nine terms
            (2, [key], change, [s], False), (-1, [key], change, [s], False),                         # npartition outside [0, nterms]
        ]
        for npart, terms, rule, cols, per in invalid:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_sessions(table, 0, npart, terms, rule, cols, ALL, 16, per_session=per)
            assert e.value.code == abi.ERR_INVALID, (npart, terms, rule, cols, per)
        n = C.c_int64(-5)                                                  # nothing is written on either way out, *out_n included
        out = np.full((6, 16), -7, np.int64)
        one = abi._marshal_sort_terms([key])
        rule, cols = abi._marshal_session_rule(gap1), abi._marshal_session_cols([s])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        for rule_p, per, ncols, cols_p, limit, cap, want in (
                (None, 0, 1, cols, ALL, 16, abi.ERR_INVALID), (C.byref(rule), 2, 1, cols, ALL, 16, abi.ERR_INVALID), (C.byref(rule), -1, 1, cols, ALL, 16, abi.ERR_INVALID),
                (C.byref(rule), 0, -1, cols, ALL, 16, abi.ERR_INVALID), (C.byref(rule), 0, 5, cols, ALL, 16, abi.ERR_INVALID), (C.byref(rule), 0, 1, None, ALL, 16, abi.ERR_INVALID),
                (C.byref(rule), 0, 1, cols, 0, 16, abi.ERR_INVALID), (C.byref(rule), 0, 1, cols, ALL, -1, abi.ERR_INVALID),
                (C.byref(rule), 0, 1, cols, ALL, 16, abi.ERR_UNSUPPORTED), (C.byref(rule), 1, 0, None, ALL, 16, abi.ERR_UNSUPPORTED)):
            rc = ctx.lib.sdqh_table_sessions(ctx.handle, table.handle, C.c_int64(0), C.c_int(0), C.c_int(1), one, rule_p, C.c_int(per), C.c_int(ncols), cols_p,
                                             C.c_int64(limit), C.c_int64(cap), ptr(out[0]), None, None, ptr(out[1]), ptr(out[2:]), C.byref(n))
            assert rc == want and n.value == -5 and (out == -7).all(), (per, ncols, limit, cap)
        rc = ctx.lib.sdqh_table_sessions(ctx.handle, table.handle, C.c_int64(0), C.c_int(0), C.c_int(1), one, C.byref(rule), C.c_int(0), C.c_int(1), cols,
                                         C.c_int64(ALL), C.c_int64(16), ptr(out[0]), None, None, ptr(out[1]), ptr(out[2:]), None)
        assert rc == abi.ERR_INVALID and (out == -7).all()                 # no out_n
    finally:
        ctx.close()


# ---- the request -------------------------------------------------------------------------------------------------------------------
def test_request_errors_come_before_anything_is_launched():
    cols = ["p", "t", "u", "x", "m"]
    ok = sessions_request(cols, ["p"], [("t", "desc"), "u"], gap=30, cols={"s": ("sum", "x"), "n": ("count",), "k": ("number",), "r": ("row",), "a": ("first", "t")})
    assert isinstance(ok, SessionRequest) and isinstance(ok, WindowRequest) and ok[0] == ALL
    assert ok[1] == [("p", "asc"), ("t", "desc"), ("u", "asc")] and ok.npartition == 1 and ok.order == [("t", "desc"), ("u", "asc")]
    assert (ok.rule, ok.gap, ok.marker, ok.per) == ("gap", 30, None, None)
    assert ok.cols == [("s", "sum", "x"), ("n", "count", None), ("k", "number", None), ("r", "row", None), ("a", "first", "t")] and ok.items == ok.cols
    ch = sessions_request(cols, ["p"], [], change="m", cols={"s": ("avg", "x")}, per="session")
    assert (ch.rule, ch.gap, ch.marker, ch.per) == ("change", None, "m", "session") and ch.order == []
    assert sessions_request(cols, [], ["t"], gap=0.25).gap == 0.25 and sessions_request(cols, [], ["t"], gap=0).cols == []
    assert sessions_request(None, ["zz"], ["yy"], gap=1, cols={"d": ("sum", "qq")})[1] == [("zz", "asc"), ("yy", "asc")]      # names checked when the result is known
    renamed = ch.renamed([("q", "asc")], {"m": "mm", "x": "xx"})
    assert isinstance(renamed, SessionRequest) and (renamed.marker, renamed.cols, renamed.per, renamed[1]) == ("mm", [("s", "avg", "xx")], "session", [("q", "asc")])
    bad = [
        (dict(gap=1, change="m"), ValueError), (dict(), ValueError),                                  # both, neither
        (dict(gap=-1), ValueError), (dict(gap=-0.5), ValueError), (dict(gap=float("inf")), ValueError), (dict(gap=float("nan")), ValueError),
        (dict(gap=True), ValueError), (dict(gap="1"), ValueError), (dict(change=3), ValueError),
        (dict(gap=1, cols={"d": ("median", "x")}), ValueError), (dict(gap=1, cols={"d": ("sum",)}), ValueError), (dict(gap=1, cols={"d": ("sum", None)}), ValueError),
        (dict(gap=1, cols={"d": ("number", "x")}), ValueError), (dict(gap=1, cols={"d": ()}), ValueError), (dict(gap=1, cols=[("d", "sum", "x")]), ValueError),
        (dict(gap=1, cols={"r": ("row",)}, per="session"), ValueError), (dict(gap=1, per="row"), ValueError), (dict(gap=1, per=1), ValueError),
        (dict(gap=1, cols={"c%d" % i: ("count",) for i in range(SESSION_HOST_MAX_COLS + 1)}), ValueError),      # more columns than the host takes
        (dict(gap=1, cols={"d": ("sum", "zz")}), KeyError), (dict(change="zz"), KeyError), (dict(gap=1, cols={"x": ("count",)}), KeyError),
    ]
    for how, err in bad:
        with pytest.raises(err):
            sessions_request(cols, ["p"], ["t"], **how)
    assert len(sessions_request(cols, ["p"], ["t"], gap=1, cols={"c%d" % i: ("count",) for i in range(SESSION_HOST_MAX_COLS)}).cols) == SESSION_HOST_MAX_COLS
    with pytest.raises(ValueError):
        sessions_request(cols, ["p"], [], gap=1)                           # a gap with nothing to take differences of
    with pytest.raises(ValueError):
        sessions_request(cols, [], [], change="m")                         # nothing to partition or order by
    with pytest.raises(ValueError):
        sessions_request(cols, ["p"], [("t", "up")], gap=1)
    with pytest.raises(KeyError):
        sessions_request(cols, ["zz"], ["t"], gap=1)
    with pytest.raises(ValueError):
        SessionRequest(ALL, [("p", "asc")], 1, "gap", 1, None, [])         # the class checks what it is given, too
    with pytest.raises(ValueError):
        SessionRequest(ALL, [("p", "asc"), ("t", "asc")], 1, "gap", 1, None, [("r", "row", None)], "session")


# ---- the host route against the brute-force reference ------------------------------------------------------------------------------
def _check(rs, partition, order, rule, cols):
    """rs.sessions(...) per row and per session against sessions_reference over the same rows, by bits."""
    terms = [(c, "asc") if isinstance(c, str) else c for c in list(partition) + list(order)]
    arrays = {c: rs.column(c) for c in rs.columns}
    is_f = {c: arrays[c].dtype.kind == "f" for c in arrays}
    idx = ref.sort_index([arrays[c].tolist() for c, _ in terms], [d for _, d in terms], [is_f[c] for c, _ in terms])
    part_keys = [tuple(ref.total_key(arrays[c][i], is_f[c]) for c, _ in terms[:len(partition)]) for i in idx]
    part_heads = [j == 0 or part_keys[j] != part_keys[j - 1] for j in range(len(idx))]
    if "gap" in rule:
        oc, od = terms[len(partition)]
        heads = ref.session_heads(part_keys, [arrays[oc][i].item() for i in idx], od == "desc", rule["gap"], is_f[oc])
    else:
        m = arrays[rule["change"]]
        heads = ref.session_heads(part_keys, None, False, None, False, marker_bits=[ref.f_bits(m[i]) if is_f[rule["change"]] else ref.i_bits(m[i]) for i in idx])
    for per in (None, "session"):
        asked = {n: spec for n, spec in cols.items() if not (per == "session" and spec[0] == "row")}
        got = rs.sessions(partition, order, cols=asked, per=per, **rule)
        spec = [(s[0], None if len(s) == 1 or s[1] is None else [arrays[s[1]][i].item() for i in idx], len(s) > 1 and s[1] is not None and is_f[s[1]]) for s in asked.values()]
        want, starts = ref.columns(heads, part_heads, spec, per == "session")
        rows = [idx[s] for s in starts] if per == "session" else idx
        assert got.columns == rs.columns + list(asked) and len(got) == len(rows)
        for c in rs.columns:
            if arrays[c].dtype.kind not in "iubf":
                assert got.column(c).tolist() == arrays[c][rows].tolist(), (per, c)
                continue
            assert _bits(got.column(c).astype(np.float64 if is_f[c] else np.int64)) == _bits(arrays[c][rows].astype(np.float64 if is_f[c] else np.int64)), (per, c)
        for (name, s), w in zip(asked.items(), want):
            a = got.column(name)
            assert a.dtype == (np.float64 if s[0] == "avg" or (s[0] in ("sum", "min", "max", "first", "last") and is_f[s[1]]) else np.int64), (name, a.dtype)
            assert _bits(a) == w, (per, name, rule)
    return heads


ALL_COLS = {"s": ("sum", "x"), "n": ("count",), "lo": ("min", "x"), "hi": ("max", "x"), "f": ("first", "t"), "l": ("last", "t"), "a": ("avg", "x"), "k": ("number",), "r": ("row",),
            "sq": ("sum", "q"), "aq": ("avg", "q"), "mq": ("min", "q"), "xq": ("max", "q")}


def test_host_route_integers_against_the_reference():
    rng = np.random.default_rng(5)
    n = 400
    p = rng.integers(0, 4, n)
    t = rng.integers(0, 300, n)
    x = rng.integers(-50, 50, n)
    q = rng.integers(-40, 40, n) * 0.25                                   # multiples of 0.25: every partial sum is exact
    rs = ResultSet(["p", "t", "u", "x", "q"], [p, t, rng.integers(0, 3, n), x, q])
    for order in ([("t", "asc")], [("t", "desc")], [("t", "asc"), ("u", "desc")]):
        for gap in (0, 1, 2, 7, 1000):
            heads = _check(rs, ["p"], order, {"gap": gap}, ALL_COLS)
        assert sum(heads) == 4                                             # (gap 1000: the partitions alone)
    _check(rs, [], [("t", "asc")], {"gap": 3}, ALL_COLS)
    _check(rs, ["p", ("u", "desc")], ["t"], {"gap": 3.0}, {"s": ("sum", "x")})      # an integral float over an integer column is that integer
    with pytest.raises(ValueError):
        rs.sessions(["p"], ["t"], gap=0.5)                                 # ... and any other float is refused
    with pytest.raises(ValueError):
        ResultSet(["t", "w"], [t, np.array(["a"] * n)]).sessions([], ["t"], gap=1, cols={"s": ("sum", "w")})      # a text measure
    with pytest.raises(ValueError):
        ResultSet(["w"], [np.array(["a", "b"])]).sessions([], ["w"], gap=1)      # text has no arithmetic


def test_host_route_int64_extremes_and_the_exact_gap():
    # sorted: MIN MIN -1 0 MAX MAX — the differences 0, 2^63 - 1, 1, 2^63 - 1, 0
    t = np.array([I_MAX, -1, I_MIN, 0, I_MAX, I_MIN], np.int64)
    x = np.array([I_MAX, I_MAX, 1, I_MIN, -1, 7], np.int64)                # sums that wrap
    rs = ResultSet(["t", "x", "q"], [t, x, np.arange(6) * 0.5])
    for d in ("asc", "desc"):
        for gap, sessions in ((0, 4), (1, 3), (I_MAX - 1, 3), (I_MAX, 1), (1 << 63, 1)):
            assert sum(_check(rs, [], [("t", d)], {"gap": gap}, ALL_COLS)) == sessions, (d, gap)
    # INT64_MIN next to INT64_MAX is a difference of 2^64 - 1: a new session for every gap an int64 holds
    ends = ResultSet(["t", "x", "q"], [np.array([I_MAX, I_MIN], np.int64), np.array([1, 2]), np.array([0.5, 0.25])])
    for d in ("asc", "desc"):
        for gap, sessions in ((0, 2), (I_MAX, 2), ((1 << 64) - 2, 2), ((1 << 64) - 1, 1)):
            assert sum(_check(ends, [], [("t", d)], {"gap": gap}, ALL_COLS)) == sessions, (d, gap)
    # the difference exactly `gap` continues, one below cuts: 5, 9, 10, 14 by gaps 4 and 3
    small = ResultSet(["t", "x", "q"], [np.array([5, 9, 10, 14]), np.arange(4), np.arange(4) * 0.25])
    assert sum(_check(small, [], ["t"], {"gap": 4}, ALL_COLS)) == 1
    assert sum(_check(small, [], ["t"], {"gap": 3}, ALL_COLS)) == 3
    assert sum(_check(small, [], [("t", "desc")], {"gap": 3}, ALL_COLS)) == 3


def test_host_route_doubles_nan_zeros_and_the_one_addition():
    nan1, nan2 = np.array([0x7FF8000000000001, 0x7FF8000000000002], np.uint64).view(np.float64)
    t = np.array([0.1 * i for i in range(12)] + [-0.0, 0.0, nan1, nan1, nan2, -np.inf, np.inf, 1e308, -1e308])
    n = len(t)
    rs = ResultSet(["t", "x", "q"], [t, np.arange(n) - 7, np.where(np.arange(n) % 5 == 0, np.nan, np.arange(n) * 0.25 - 2.0)])
    for d in ("asc", "desc"):
        for gap in (0.0, 0.1, 0.09999999999999999, 0.10000000000000002, 0.5, 1e308, 1.7976931348623157e308):
            _check(rs, [], [("t", d)], {"gap": gap}, ALL_COLS)
    # -0.0 and +0.0 are one value under gap 0; the two NaN payloads are two sessions, equal payloads one
    z = ResultSet(["t", "x", "q"], [np.array([0.0, -0.0, nan2, nan1, nan1]), np.arange(5), np.arange(5) * 0.5])
    heads = _check(z, [], ["t"], {"gap": 0.0}, ALL_COLS)
    assert heads == [True, False, True, False, True]                       # (-0.0, +0.0) | (nan1, nan1) | nan2
    # multiples of 0.1 a rounding apart: v - gap is ONE addition, whatever the exact difference would say
    v = np.array([0.1 * i for i in range(40)])
    w = ResultSet(["t", "x", "q"], [v, np.arange(40), np.arange(40) * 0.25])
    heads = _check(w, [], ["t"], {"gap": 0.1}, ALL_COLS)
    want = [True] + [not (min(v[j] + -0.1, v[j]) <= v[j - 1]) for j in range(1, 40)]
    assert heads == want and 1 < sum(heads) < 40                           # some neighbours continue and some do not


def test_host_route_the_change_rule_and_limits():
    rng = np.random.default_rng(9)
    n = 300
    m_i = rng.integers(0, 3, n)
    m_f = np.where(rng.integers(0, 4, n) == 0, -0.0, rng.integers(0, 2, n) * 1.0)      # -0.0 and +0.0 differ as stored bits
    rs = ResultSet(["p", "t", "x", "q", "mi", "mf", "w"], [rng.integers(0, 3, n), np.arange(n)[::-1].copy(), rng.integers(-9, 9, n), rng.integers(-9, 9, n) * 0.25, m_i, m_f,
                                                           rng.choice(["a", "b"], n)])
    cols = {k: v for k, v in ALL_COLS.items()}
    for change in ("mi", "mf"):
        _check(rs, ["p"], ["t"], {"change": change}, cols)
        _check(rs, ["p"], [], {"change": change}, {"n": ("count",), "k": ("number",)})      # no order term: stored order inside a partition
    text = rs.sessions(["p"], ["t"], change="w", cols={"n": ("count",)}, per="session")             # the host takes a text marker
    assert int(text.column("n").sum()) == n
    req = sessions_request(rs.columns, ["p"], ["t"], gap=1, cols={"n": ("count",)}, k=7)
    assert len(rs.sessioned(req)) == 7 and rs.windowed(req).ordered_rows() == rs.sessioned(req).ordered_rows()
    empty = ResultSet(["t", "x"], [np.zeros(0, np.int64), np.zeros(0)])
    for per in (None, "session"):
        got = empty.sessions([], ["t"], gap=1, cols={"s": ("sum", "x"), "n": ("count",), "a": ("avg", "t")}, per=per)
        assert len(got) == 0 and [a.dtype.str for a in got.arrays] == ["<i8", "<f8", "<f8", "<i8", "<f8"]


# ---- routing, on a stub engine -----------------------------------------------------------------------------------------------------
def _stub(**kw):
    lib = SimpleNamespace(has_sessions=kw.pop("has", True), has_grouping_sets=True, has_window_agg=True, has_sort_terms=True)
    return SimpleNamespace(device_sessions=kw.pop("on", True), ctx=SimpleNamespace(library=lib), device_sort=True, order_routes=[])


def _spec(terms, measures, int_values=(), decoded_order=()):
    spec = engine._FrameSpec(terms)
    spec.measures, spec.int_values, spec.decoded_order = measures, int_values, decoded_order
    return spec


def test_routing():
    K, P, V = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE
    terms = [(P, 0, False, False), (K, 0, True, False)]
    mx = (V, 0, False, True)
    req = sessions_request(None, ["p"], [("k", "desc")], gap=30, cols={"s": ("sum", "x"), "k2": ("number",)})
    fits = _spec(terms, [mx, None])
    assert engine._order_route(_stub(), req, fits) == "sessions"
    assert engine._order_route(_stub(on=False), req, fits) == "host"       # the switch
    assert engine._order_route(_stub(has=False), req, fits) == "host"      # a library without the extension
    assert engine._order_route(_stub(), req, None) == "host"               # a column the device cannot order by
    assert engine._order_route(_stub(), req, _spec(terms, None)) == "host"      # a text measure: no plain column to read
    five = sessions_request(None, ["p"], ["k"], gap=1, cols={n: ("count",) for n in "abcde"})
    assert engine._order_route(_stub(), five, _spec(terms, [None] * 5)) == "host"      # more than SS_MAX_COLS
    four = sessions_request(None, ["p"], ["k"], gap=1, cols={n: ("avg", "x") for n in "abcd"})
    assert engine._order_route(_stub(), four, _spec(terms, [mx] * 4)) == "sessions"
    none = sessions_request(None, ["p"], ["k"], gap=1, per="session")
    assert engine._order_route(_stub(), none, _spec(terms, [])) == "sessions"           # no column at all: the representatives
    # the gap the device's term can take: a text or decoded order column, a fractional gap over integers and 2^53 over integer-valued doubles stay on the host
    text = [(P, 0, False, False), (P, 1, False, False, 1, 0, 0, object())]
    assert engine._order_route(_stub(), req, _spec(text, [mx, None])) == "host"
    assert engine._order_route(_stub(), req, _spec(terms, [mx, None], decoded_order=("k",))) == "host"
    half = sessions_request(None, ["p"], ["k"], gap=0.5)
    assert engine._order_route(_stub(), half, _spec(terms, [])) == "host"
    vterms = [(P, 0, False, False), (V, 1, False, True)]
    assert engine._order_route(_stub(), half, _spec(vterms, [])) == "sessions" and engine._session_gap(half, _spec(vterms, [])) == 0.5
    assert engine._order_route(_stub(), half, _spec(vterms, [], int_values=("k",))) == "host"
    wide = sessions_request(None, ["p"], ["k"], gap=(1 << 53) + 1)
    assert engine._order_route(_stub(), wide, _spec(vterms, [], int_values=("k",))) == "host"
    assert engine._order_route(_stub(), wide, _spec(terms, [])) == "sessions" and engine._session_gap(wide, _spec(terms, [])) == (1 << 53) + 1
    assert engine._session_gap(sessions_request(None, ["p"], ["k"], gap=3), _spec(vterms, [], int_values=("k",))) == 3.0
    assert engine._order_route(_stub(), sessions_request(None, ["p"], ["k"], gap=1 << 63), _spec(terms, [])) == "host"
    # the change rule: the marker travels behind the measures
    ch = sessions_request(None, ["p"], [], change="m", cols={"s": ("sum", "x")})
    assert engine._order_route(_stub(), ch, _spec(terms[:1], [mx, (P, 1, False, False)])) == "sessions"
    assert engine._order_route(_stub(), ch, _spec(terms[:1], None)) == "host"
    asked = []
    made = engine._order_spec(ch, lambda order, derive: asked.append((list(order), derive)) or [(V, i, False, True) for i in range(len(order))], lambda nm: False)
    assert isinstance(made, engine._FrameSpec) and made.measures == [(V, 0, False, True), (V, 1, False, True)]
    assert asked == [([("p", "asc")], True), ([("x", "asc"), ("m", "asc")], False)]
    rec = engine._route_of(req)
    assert rec == (SessionRequest, "sessions", "device_sessions", "has_sessions", "cols", abi.SS_MAX_COLS) and rec.env == "SDQLPY_AMD_DEVICE_SESSIONS"
    assert rec in engine._WINDOW_ROUTES and engine._WINDOW_ROUTES[0].route == "group_distinct" and rec.value_frames
    assert [engine._route_of(r).route for r in (req, ch)] == ["sessions"] * 2
    assert not any(isinstance(req, r.request) for r in engine._WINDOW_ROUTES[:engine._WINDOW_ROUTES.index(rec)])      # no earlier record takes it
    assert [rec.integral((n, op, "x")) for n, op in zip("abcdefghi", SESSION_OPS)] == [True, False, True, True, True, True, False, False, False]
    eng = _stub()
    engine._note_order_route(eng, req, fits, "sessions")
    assert eng.order_routes[-1] == {"route": "sessions", "k": ALL, "order": ["k"], "ranked": [], "per": ["p"], "rule": "gap", "gap": 30, "change": None,
                                    "cols": [["s", "sum", "x"], ["k2", "number", None]], "per_session": False, "calls": 1}
    engine._note_order_route(eng, ch, None, "host")
    assert eng.order_routes[-1]["route"] == "host" and eng.order_routes[-1]["calls"] == 0 and eng.order_routes[-1]["change"] == "m"


class _SessionsRecorder(_Recorder):
    def table_compact_into_block(self, table, *args, **kwargs):           # the host route's rows: all three
        self.calls.append(("table_compact_into_block", args, kwargs))
        return self._rows(3) + (3,)

    def table_sessions(self, table, *args, **kwargs):
        self.calls.append(("table_sessions", args, kwargs))
        rows = 2 if kwargs.get("per_session") else 3
        return self._rows(rows) + ([np.array([2.0, 4.0, 6.0][:rows]) + i for i, _ in enumerate(args[4])],)


def _run(req_of, **eng_kw):
    ctx = _SessionsRecorder()
    eng = SimpleNamespace(ctx=ctx, device_sort=True, order_routes=[], compact_hints={}, lazy_results=False, **eng_kw)
    bt = SimpleNamespace(agg=([("p", "key")], ["x", "k"], None, True, True, 2), shared_groups=False, agg_fields={}, int_values=("x",), table=object(), key_radix=None,
                         key_parts=None, key_decoder=None, decoder_of=lambda field, src: None, payload_dtypes={})
    op = SimpleNamespace(source="groups", out="result", lineno=1, fields=[("grp", 0, "p"), ("ord", 1, "k"), ("val", 1, "x")])
    rs = engine._finalize(eng, op, {"groups": ("aggregated", "bt"), "bt": bt}, req_of(["grp", "ord", "val"]))
    return eng.order_routes[-1], ctx.calls, rs


def test_through_finalize_on_a_recording_context():
    K, V = abi.SORT_KEY, abi.SORT_VALUE
    cols = {"s": ("sum", "val"), "a": ("avg", "val"), "k": ("number",)}
    note, calls, rs = _run(lambda c: sessions_request(c, ["grp"], [("ord", "desc")], gap=1.5, cols=cols))
    assert note == {"route": "sessions", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"], "rule": "gap", "gap": 1.5, "change": None,
                    "cols": [["s", "sum", "val"], ["a", "avg", "val"], ["k", "number", None]], "per_session": False, "calls": 1}
    assert calls == [("table_sessions", (1, 1, [(K, 0, False, False), (V, 1, True, True)], (abi.SS_GAP, 1.5),
                                         [(abi.SS_SUM, V, 0, True), (abi.SS_AVG, V, 0, True), (abi.SS_NUMBER, K, 0, False)], ALL, 4096), {"per_session": False, "want_hits": False})]
    # the sum of a column kept as integer-valued doubles is rounded back; the average and the number stay what they are
    assert [(n, a.dtype.str) for n, a in zip(rs.columns, rs.arrays)] == [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("s", "<i8"), ("a", "<f8"), ("k", "<f8")]
    assert len(rs) == 3
    note, calls, rs = _run(lambda c: sessions_request(c, ["grp"], [], change="ord", cols={"s": ("sum", "val")}, per="session"))
    assert note["per_session"] is True and note["calls"] == 1 and note["rule"] == "change" and note["change"] == "ord" and note["order"] == []
    assert calls[0][1][3] == (abi.SS_CHANGE, V, 1, True) and calls[0][2]["per_session"] is True and len(rs) == 2
    # five columns, and the switch off: the host route, no device call
    note, calls, rs = _run(lambda c: sessions_request(c, ["grp"], ["ord"], gap=1, cols={n: ("count",) for n in "abcde"}))
    assert note["route"] == "host" and note["calls"] == 0 and not [c for c in calls if c[0] == "table_sessions"] and rs.columns == ["grp", "ord", "val"] + list("abcde")
    note, calls, rs = _run(lambda c: sessions_request(c, ["grp"], ["ord"], gap=1, cols=cols), device_sessions=False)
    assert note["route"] == "host" and not [c for c in calls if c[0] == "table_sessions"] and rs.columns == ["grp", "ord", "val", "s", "a", "k"]


def test_the_switch_is_read_from_the_environment(oracle_lib, monkeypatch):
    for value, on in (("0", False), ("1", True)):
        monkeypatch.setenv("SDQLPY_AMD_DEVICE_SESSIONS", value)
        eng = engine.Engine(oracle_lib.context(threads=1))
        try:
            assert eng.device_sessions is on
        finally:
            eng.close()


def test_the_multi_gpu_runner_refuses_sessions():
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(sessions_request(None, ["p"], ["t"], gap=1))
    assert "sessions" in str(e.value)
