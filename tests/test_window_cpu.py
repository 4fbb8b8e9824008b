"""ORDER BY ... LIMIT per group (top_per / numbered), the part that needs no GPU: the window extension's symbols
(include/sdqh_sort_window.h, abi.WINDOW_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without them,
ResultSet.window_index against a pure-Python reference (sort a list of tuples, walk it), and the decorator surface on the CPU
implementation's engine — the host route."""
import os
import re
import struct

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import ResultSet, WindowRequest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
KINDS = ("row_number", "rank", "dense_rank")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(sdqh_[a-z_0-9]+)\s*\(", text)))


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.WINDOW_EXPORTS) == _declared("sdqh_sort_window.h") == ["sdqh_table_window", "sdqh_window_geometry"]
    for s in abi.WINDOW_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert s not in abi.EXPORTS and s not in abi.SORT_EXPORTS and s not in abi.SORT_TERMS_EXPORTS and s not in abi.EXTREMA_EXPORTS
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
    assert hip_lib.has_window and hip_lib.has_sort_terms and hip_lib.has_sort
    assert (abi.WIN_ROW_NUMBER, abi.WIN_RANK, abi.WIN_DENSE_RANK) == (0, 1, 2) and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort_window.h")).read()
    for name, value in (("ROW_NUMBER", 0), ("RANK", 1), ("DENSE_RANK", 2)):
        assert re.search(r"#define\s+SDQH_WIN_%s\s+%d\b" % (name, value), text)
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sdqh.h")).read())


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_window is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        for call in (lambda: ctx.table_window(t, 0, 0, [(abi.SORT_KEY, 0, False, False)], abi.WIN_RANK, 1, ALL, 16), ctx.window_geometry):
            with pytest.raises(abi.SdqhError) as e:
                call()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no window extension" in str(e.value) and "libsdqloracle" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.window_geometry() >= 64                                 # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window(table, 0, 0, [(abi.SORT_KEY, 0, False, False)], abi.WIN_RANK, 1, ALL, 16)
        assert e.value.code == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window(table, 0, 0, [(abi.SORT_KEY, 0, False, False)], 5, 1, ALL, 16)
        assert e.value.code == abi.ERR_INVALID                             # the argument checks come first
    finally:
        ctx.close()


# ---- window_index against a walk over sorted tuples -----------------------------------------------------------------------------------
def _image(x, desc):
    """A Python value as an integer that orders like the device's 64-bit key: ints as signed values, floats by sign and magnitude of
    their bits, text by itself (handled by the caller: ranked first)."""
    if isinstance(x, float):
        u = struct.unpack("<Q", struct.pack("<d", x))[0]
        u = (~u & 0xFFFFFFFFFFFFFFFF) if u >> 63 else u | (1 << 63)
    else:
        u = int(x) + (1 << 63)
    return (0xFFFFFFFFFFFFFFFF - u) if desc else u


def _reference(columns, rows, by, order, kind, per_limit, k):
    """rows: list of tuples.  -> (row indices, ranks): sort (term images..., row index) tuples, walk them."""
    terms = [(b, "asc") if isinstance(b, str) else b for b in by] + list(order)
    text_rank = {}
    for name, _ in terms:
        j = columns.index(name)
        if rows and isinstance(rows[0][j], str):
            text_rank[name] = {s: i for i, s in enumerate(sorted({r[j] for r in rows}))}
    keyed = []
    for i, r in enumerate(rows):
        imgs = tuple(_image(text_rank[nm][r[columns.index(nm)]] if nm in text_rank else r[columns.index(nm)], d == "desc") for nm, d in terms)
        keyed.append((imgs, i))
    keyed.sort()
    out, ranks, prev = [], [], None
    rn = rk = dr = 0
    for imgs, i in keyed:
        if prev is None or imgs[:len(by)] != prev[:len(by)]:
            rn = rk = dr = 1
        else:
            rn += 1
            if imgs != prev:
                rk, dr = rn, dr + 1
        prev = imgs
        rank = (rn, rk, dr)[KINDS.index(kind)]
        if rank <= per_limit:
            out.append(i); ranks.append(rank)
    return out[:k], ranks[:k]


NAN_A = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]


def _cases():
    rng = np.random.default_rng(11)
    n = 400
    g = rng.integers(0, 9, n).astype(np.int64)
    v = rng.integers(-4, 4, n).astype(np.float64)
    h = rng.integers(0, 3, n).astype(np.int64)
    s = np.array(["pear", "apple", "fig", "apple ", "Fig", "", "zz"])[rng.integers(0, 7, n)]
    edge = np.resize(np.array([0.0, -0.0, NAN_A, NAN_B, np.inf, -np.inf, 1.0, -0.0, NAN_B, 0.0, NAN_A]), n)[rng.permutation(n)]
    plain = (["g", "v", "h", "s", "e"], [g, v, h, s, edge])
    empty = (["g", "v", "h", "s", "e"], [g[:0], v[:0], h[:0], s[:0], edge[:0]])
    return {"plain": plain, "empty": empty}


SHAPES = [
    (["g"], [("v", "desc"), ("h", "asc")]),
    ([("g", "desc")], [("v", "asc")]),
    ([], [("v", "desc")]),                                                 # one partition
    (["g", "v", "h", "s", "e"], []),                                       # by = all columns
    (["s"], [("h", "desc")]),                                              # a text partition
    (["g"], [("s", "desc"), ("v", "asc")]),                                # a text order column
    (["e"], [("h", "asc")]),                                               # +-0.0 and two NaNs as partition values
    (["g"], [("e", "desc")]),                                              # ... and as order values
    (["g"], [("e", "asc")]),
]


@pytest.mark.parametrize("case", ["plain", "empty"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_window_index_against_a_walk(case, shape):
    columns, arrays = _cases()[case]
    rs = ResultSet(columns, arrays)
    rows = list(zip(*[a.tolist() for a in arrays]))
    by, order = SHAPES[shape]
    done = 0
    for kind in KINDS:
        for per_limit in (1, 2, ALL):
            want_all = _reference(columns, rows, by, order, kind, per_limit, ALL)
            for k in sorted({1, max(1, len(want_all[0]) // 2), ALL}):
                idx, rank = rs.window_index(by, order, kind, per_limit, k)
                want = _reference(columns, rows, by, order, kind, per_limit, k)
                assert idx.tolist() == want[0] and rank.tolist() == want[1] and rank.dtype == np.int64, (by, order, kind, per_limit, k)
                done += 1
    assert done >= 3 * 3 * 2
    if case == "plain" and by == ["e"]:                                    # -0.0 / +0.0 are two partitions, the NaN patterns two more
        idx, rank = rs.window_index(by, order, "row_number", 1)
        assert len(idx) == 7
    if case == "plain" and len(by) == 5:                                   # every row ties only with its copies: rank and dense_rank are 1 everywhere
        assert (rs.window_index(by, order, "rank", ALL)[1] == 1).all() and (rs.window_index(by, order, "dense_rank", ALL)[1] == 1).all()
        assert rs.window_index(by, order, "row_number", ALL)[1].max() > 1


def test_top_per_and_numbered_on_a_result_set():
    columns, arrays = _cases()["plain"]
    rs = ResultSet(columns, arrays)
    top = rs.top_per(2, ["g"], [("v", "desc")])
    idx, _ = rs.window_index(["g"], [("v", "desc")], "row_number", 2)
    assert top.columns == columns and top.ordered_rows()[:5] == [tuple(a[i].item() for a in arrays) for i in idx[:5]] and len(top) == 18
    assert len(rs.top_per(2, ["g"], [("v", "desc")], ties=True)) > 18
    num = rs.numbered(["g"], [("v", "desc")], kind="dense_rank", name="nth")
    assert num.columns == columns + ["nth"] and len(num) == len(rs) and num.column("nth").dtype == np.int64 and num.column("nth").max() <= 8
    assert rs.top_index(3, [("v", "desc")]).tolist() == np.lexsort([-arrays[1]])[:3].tolist()       # top_index is what it was
    for call, exc in ((lambda: rs.top_per(0, ["g"], [("v", "desc")]), ValueError), (lambda: rs.numbered(["g"], [("v", "desc")], kind="ntile"), ValueError),
                      (lambda: rs.numbered(["g"], [("v", "desc")], name="h"), KeyError), (lambda: rs.top_per(1, ["nope"], [("v", "desc")]), KeyError),
                      (lambda: rs.top_per(1, ["g"], [("nope", "desc")]), KeyError), (lambda: rs.top_per(1, ["g"], [("v", "down")]), ValueError)):
        with pytest.raises(exc):
            call()


def test_the_request_reads_as_a_top():
    req = WindowRequest(ALL, [("a", "asc"), ("b", "desc")], 1, abi.WIN_RANK, 3, "r")
    k, order = req[0], req[1]
    assert (k, order) == (ALL, [("a", "asc"), ("b", "desc")]) and isinstance(req, tuple) and len(req) == 2
    assert req.by == [("a", "asc")] and req.order == [("b", "desc")] and (req.kind, req.per_limit, req.name) == (1, 3, "r")
    again = req.renamed([("x", "asc"), ("y", "desc")])
    assert again[1] == [("x", "asc"), ("y", "desc")] and (again.npartition, again.kind, again.per_limit, again.name) == (1, 1, 3, "r")


# ---- through the decorator on the CPU implementation's engine: the host route -------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    qs = ["q3", "q15"]
    return tpch.generate(0.05, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))


@pytest.fixture()
def on_the_decorator(oracle_lib):
    from sdqlpy_amd import sdql_lib
    eng = engine.use_engine(engine.Engine(oracle_lib.context(threads=min(16, os.cpu_count() or 1))))
    sdql_lib._state.update(runner=None)
    yield eng
    engine.reset_default_engine()
    sdql_lib._state.update(mode=None)


def _close(a, b):
    return a == b if not isinstance(a, float) else abs(a - b) <= 1e-10 * max(abs(a), abs(b))


def _same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and all(_close(p, q) for p, q in zip(x, y)), (x, y)


def _numpy_ranks(dates, revenue):
    """Rows ordered by (date asc, revenue desc) already: (row_number, dense_rank) inside each date, by numpy."""
    n = len(dates)
    pos = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = dates[1:] != dates[:-1]
    start = np.maximum.accumulate(np.where(head, pos, 0))
    tie = head.copy()
    tie[1:] |= revenue[1:] != revenue[:-1]
    seen = np.cumsum(tie)
    return pos - start + 1, seen - seen[start] + 1


def test_q3_and_q15_on_the_host_route(on_the_decorator, db):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    everything = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    rows = everything.ordered_rows()
    assert len(rows) > 300
    for run in range(3):
        rn, dense = _numpy_ranks(everything.column("o_orderdate"), everything.column("revenue"))
        top = Q.q3.top_per(3, by, order)(*args)
        assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "kind": "row_number", "per_limit": 3}
        assert top.columns == everything.columns and 0 < len(top) < len(rows)
        _same_rows(top.ordered_rows(), [r for r, k in zip(rows, rn <= 3) if k])
        num = Q.q3.numbered(by, order, kind="dense_rank", name="nth")(*args)
        route = eng.stats()["order_routes"][-1]
        assert (route["route"], route["kind"], route["per_limit"], route["per"]) == ("host", "dense_rank", ALL, by)
        assert num.columns == everything.columns + ["nth"] and num.column("nth").dtype == np.int64
        _same_rows([r[:-1] for r in num.ordered_rows()], rows)
        assert (num.column("nth") == dense).all()
    # q15: the suppliers whose revenue is the maximum (what q15_max selects), ties kept
    args = [db[t] for t in Q.QUERY_TABLES["q15"]]
    full = Q.q15(*args)
    best = Q.q15.top_per(1, [], [("total_revenue", "desc")], ties=True)(*args)
    route = eng.stats()["order_routes"][-1]
    assert (route["route"], route["kind"], route["per"], route["per_limit"]) == ("host", "rank", [], 1)
    revenue = full.column("total_revenue")
    assert len(best) >= 1 and sorted(best.column("s_suppkey").tolist()) == sorted(full.column("s_suppkey")[revenue == revenue.max()].tolist())
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*[db[t] for t in Q.QUERY_TABLES["q3"]])
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_argument_errors_come_before_anything_is_launched(on_the_decorator, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("launched")
    monkeypatch.setattr(engine, "execute_plan", never)
    monkeypatch.setattr(frontend, "lower_function", frontend.lower_function)
    order = [("revenue", "desc")]
    for call, exc in ((lambda: Q.q3.top_per(0, ["o_orderdate"], order), ValueError), (lambda: Q.q3.top_per(-1, [], order), ValueError),
                      (lambda: Q.q3.numbered(["o_orderdate"], order, kind="ntile"), ValueError), (lambda: Q.q3.numbered(["o_orderdate"], order, name="revenue"), KeyError),
                      (lambda: Q.q3.top_per(1, ["o_orderdat"], order), KeyError), (lambda: Q.q3.top_per(1, ["o_orderdate"], [("revenu", "desc")]), KeyError),
                      (lambda: Q.q3.top_per(1, ["o_orderdate"], [("revenue", "down")]), ValueError), (lambda: Q.q15.numbered([], [("total_revenue", "desc")], name="s_name"), KeyError)):
        with pytest.raises(exc):
            call()
    assert callable(Q.q3.top_per(1, ["o_orderdate"], order)) and callable(Q.q3.numbered([("o_orderdate", "desc")], order))      # nothing runs until it is called


def test_result_columns_of_the_shipped_plans():
    want = {"q3": ["l_orderkey", "o_orderdate", "o_shippriority", "revenue"], "q15": ["s_suppkey", "s_name", "s_address", "s_phone", "total_revenue"],
            "q16": ["p_brand", "p_type", "p_size", "supplier_cnt"], "q6": None}
    for name, columns in want.items():
        assert engine.result_columns(frontend.lower_function(Q.QUERIES[name])) == columns, name


def test_the_multi_gpu_runner_refuses():
    from sdqlpy_amd import dist as sdist
    req = WindowRequest(ALL, [("o_orderdate", "asc"), ("revenue", "desc")], 1, abi.WIN_ROW_NUMBER, 3)
    with pytest.raises(frontend.UnsupportedQuery):
        sdist.refuse_window(req)
    sdist.refuse_window((10, [("revenue", "desc")]))                       # a plain top passes
    sdist.refuse_window(None)

    class Stub:                                                            # the runner's own entry makes the refusal before it looks at the query
        _inflight = {}
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.DistributedRunner._run(Stub(), "q3", {}, None, req)
    assert "top_per" in str(e.value)
