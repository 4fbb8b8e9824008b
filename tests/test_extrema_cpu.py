"""MIN / MAX aggregation (smin / smax), the part that needs no GPU: the extrema extension's symbols (include/sdqh_extrema.h,
abi.EXTREMA_EXPORTS) in the cross-compiled library and nowhere in the common boundary, the CPU implementation without them, the front
end's lowering — every accepted position, every refused one with its source line — the engine refusing such a plan up front on a
library without the extension, and the numpy restatement of the slot encoding that tests/test_extrema_gpu.py takes its expected
values from."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.frontend import Cmp, Col, ExtremaOp, HostDictOp, RecordCons, ScanOp, UnsupportedQuery, WholeKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(sdqh_[a-z_0-9]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_stay_out_of_the_common_boundary(hip_lib):
    assert sorted(abi.EXTREMA_EXPORTS) == _declared("sdqh_extrema.h")
    for s in abi.EXTREMA_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert s not in abi.EXPORTS and s not in abi.SORT_EXPORTS and s not in _declared("sdqh.h")
    assert hip_lib.has_extrema and hip_lib.has_sort
    assert (abi.EXT_MIN, abi.EXT_MAX) == (0, 1) and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_extrema.h")).read()
    assert re.search(r"#define\s+SDQH_EXT_MIN\s+0\b", text) and re.search(r"#define\s+SDQH_EXT_MAX\s+1\b", text)


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_extrema is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        v = ctx.upload(np.arange(10, dtype=np.float64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        for call in (lambda: ctx.table_extrema(t, k, 10, [(0, abi.EXT_MIN, v, True)]), lambda: ctx.table_extrema_begin(t, [0], [abi.EXT_MAX]),
                     lambda: ctx.table_extrema_fold(t, k, 10, [(0, v, True)]), lambda: ctx.table_extrema_end(t),
                     lambda: ctx.column_extrema(v, 10), ctx.extrema_geometry):
            with pytest.raises(abi.SdqhError) as e:
                call()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no extrema extension" in str(e.value)
        t.free()
    finally:
        ctx.close()


# ---- lowering ----------------------------------------------------------------------------------------------------------------------
HEAD = "def f(T, U):\n"


def _lower(*lines):
    return frontend.lower_source(HEAD + "".join("    %s\n" % ln for ln in lines) + "    return out\n", first_line=100)


def _only(plan):
    ops = [op for op in plan.ops if isinstance(op, ExtremaOp)]
    assert len(ops) == 1
    return ops[0]


def test_accepted_positions_over_a_table():
    op = _only(_lower("out = T.sum(lambda p: {p[0].k: smin(p[0].v)})"))
    assert (op.source, op.source_is_table, op.val_is_record, op.conds, op.lineno) == ("T", True, False, [], 2)
    assert isinstance(op.key, Col) and op.key.name == "k"
    assert [(nm, how, repr(e)) for nm, how, e in op.fields] == [(None, "min", "Col(v)")]
    assert repr(op) == "ExtremaOp(out <- T: if []: {Col(k): smin(Col(v))})"

    op = _only(_lower("out = T.sum(lambda p: {p[0].k: smax(p[0].v * 2.0)} if p[0].d < 5 and p[0].k != 3 else None)"))
    assert [(nm, how) for nm, how, _ in op.fields] == [(None, "max")] and len(op.conds) == 2 and all(isinstance(c, Cmp) for c in op.conds)
    assert repr(op.fields[0][2]) == "(Col(v) * Const(2.0))"

    op = _only(_lower('out = T.sum(lambda p: {record({"a": p[0].k, "b": p[0].j}): record({"lo": smin(p[0].v), "hi": smax(p[0].w), "total": p[0].v, "n": 1})}',
                      '               if p[0].d >= 7 else None)'))
    assert op.val_is_record and isinstance(op.key, RecordCons) and [n for n, _ in op.key.fields] == ["a", "b"]
    assert [(nm, how) for nm, how, _ in op.fields] == [("lo", "min"), ("hi", "max"), ("total", None), ("n", None)]
    assert len(op.conds) == 1 and op.lineno == 2

    plan = _lower("best = T.sum(lambda p: smax(p[0].v) if p[0].d == 1 else None)",
                  "out = U.sum(lambda q: {q[0].k: q[0].w} if q[0].w >= best else None)")
    op = _only(plan)
    assert op.key is None and not op.val_is_record and [(nm, how) for nm, how, _ in op.fields] == [(None, "max")] and len(op.conds) == 1
    assert repr(op) == "ExtremaOp(best <- T: if [(Col(d) == Const(1))]: smax(Col(v)))"
    later = plan.ops[1]
    assert isinstance(later, ScanOp) and repr(later.conds[0]) == "(Col(w) >= ScalarField(best.None))"      # read as any scalar sum

    op = _only(_lower("out = T.sum(lambda p: {dense(100, p[0].k): smin(p[0].v)})"))
    assert isinstance(op.key, Col)


def test_accepted_positions_over_a_result_dictionary():
    first = "d = T.sum(lambda p: {p[0].k: p[0].v})"
    op = _only(_lower(first, "out = d.sum(lambda g: smax(g[1]))"))
    assert (op.source, op.source_is_table, op.key) == ("d", False, None) and isinstance(op.fields[0][2], WholeKey) and op.fields[0][1] == "max"
    op = _only(_lower(first, "out = d.sum(lambda g: smin(g[1]) if g[1] > 0.0 else None)"))
    assert op.key is None and op.fields[0][1] == "min" and len(op.conds) == 1
    first = 'd = T.sum(lambda p: {record({"a": p[0].k, "b": p[0].j}): p[0].v})'
    op = _only(_lower(first, "out = d.sum(lambda g: {g[0].a: smax(g[1])})"))
    assert not op.source_is_table and isinstance(op.key, WholeKey) and (op.key.which, op.key.field) == (0, "a")
    op = _only(_lower(first, 'out = d.sum(lambda g: {g[0].a: record({"lo": smin(g[1]), "hi": smax(g[1]), "n": 1})} if g[0].b != 4 else None)'))
    assert op.val_is_record and [(nm, how) for nm, how, _ in op.fields] == [("lo", "min"), ("hi", "max"), ("n", None)] and len(op.conds) == 1
    # ... and such a result is read back like any aggregated dictionary
    plan = _lower("lo = T.sum(lambda p: {p[0].k: record({\"first\": smin(p[0].d)})})",
                  "out = U.sum(lambda q: {q[0].k: q[0].w} if lo[q[0].k] != None and lo[q[0].k].first == q[0].d else None)")
    assert isinstance(plan.ops[0], ExtremaOp) and isinstance(plan.ops[1], ScanOp) and "Payload(lo[Col(k)].first)" in repr(plan.ops[1])


REFUSED = [
    ("a condition", ["out = T.sum(lambda p: {p[0].k: p[0].v} if smin(p[0].v) > 1.0 else None)"], 2),
    ("a key", ["out = T.sum(lambda p: {smax(p[0].k): p[0].v})"], 2),
    ("arithmetic", ["out = T.sum(lambda p: {p[0].k: smin(p[0].v) + 1})"], 2),
    ("arithmetic inside a record", ['out = T.sum(lambda p: {p[0].k: record({"a": 2.0 * smax(p[0].v)})})'], 2),
    ("nested", ["out = T.sum(lambda p: {p[0].k: smin(smax(p[0].v))})"], 2),
    ("scalar arithmetic", ["out = T.sum(lambda p: smax(p[0].v) - 1.0)"], 2),
    ("a joinProbe's output", ['idx = T.joinBuild("k", lambda p: True, ["v"])', 'out = U.joinProbe(idx, "k", lambda q: True, lambda e, q: {q.k: smin(e.v)})'], 3),
    ("a joinBuild's filter", ['out = T.joinBuild("k", lambda p: smin(p[0].v) > 0, ["v"])'], 2),
    ("a unique key", ["out = T.sum(lambda p: {unique(p[0].k): smin(p[0].v)})"], 2),
    ("an assignment sum", ["out = T.sum(lambda p: {p[0].k: smin(p[0].v)}, False)"], 2),
    ("a later line", ["d = T.sum(lambda p: {p[0].k: p[0].v})", "e = T.sum(lambda p: {p[0].k: smin(p[0].v)})", "out = d.sum(lambda g: {g[0]: g[1] * smax(g[1])})"], 4),
    ("too many values", ['out = T.sum(lambda p: {p[0].k: record({"a": smin(p[0].v), "b": smax(p[0].v), "c": p[0].v, "d": p[0].w, "e": smin(p[0].w)})})'], 2),
]


@pytest.mark.parametrize("what,lines,line", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_positions_carry_their_line(what, lines, line):
    with pytest.raises(UnsupportedQuery) as e:
        _lower(*lines)
    msg = str(e.value)
    assert "f, line %d:" % (100 + line - 1) in msg, msg
    assert "smin" in msg and "smax" in msg or "4 values" in msg, msg
    assert lines[line - 2].strip() in msg                                          # the source line itself


def test_the_refusal_says_where_it_is_allowed():
    with pytest.raises(UnsupportedQuery) as e:
        _lower("out = T.sum(lambda p: {p[0].k: smin(p[0].v) + 1})")
    msg = str(e.value)
    assert "{key: smin(v)}" in msg and "record" in msg and "scalar sum" in msg and "never in a condition" in msg


def test_shipped_queries_lower():
    q2m = frontend.lower_function(Q.q2_min)
    kinds = [type(op).__name__ for op in q2m.ops]
    assert kinds == ["ScanOp"] * 4 + ["ExtremaOp", "ScanOp", "HostDictOp"]
    cost = q2m.ops[4]
    assert cost.out == "european_cost" and cost.source == "partsupp" and repr(cost.key) == "Col(ps_partkey)" and len(cost.conds) == 2
    assert [(nm, how, repr(e)) for nm, how, e in cost.fields] == [(None, "min", "Col(ps_supplycost)")]
    q15m = frontend.lower_function(Q.q15_max)
    assert [type(op).__name__ for op in q15m.ops] == ["ScanOp", "ExtremaOp", "ScanOp", "HostDictOp"]
    best = q15m.ops[1]
    assert (best.out, best.source, best.source_is_table, best.key) == ("best", "revenue", False, None) and best.fields[0][1] == "max"
    assert repr(q15m.ops[3].conds) == "[(kv[1] == ScalarField(best.None))]"
    assert Q.EXTREMA_QUERIES == {"q2_min": Q.q2_min, "q15_max": Q.q15_max} and not set(Q.EXTREMA_QUERIES) & set(Q.QUERIES)
    assert Q.QUERY_TABLES["q2_min"] == Q.QUERY_TABLES["q2"] and Q.QUERY_TABLES["q15_max"] == Q.QUERY_TABLES["q15"]
    assert tpch.columns_for(["q2_min"]) == tpch.columns_for(["q2"]) and tpch.columns_for(["q15_max"]) == tpch.columns_for(["q15"])
    # the two differ from their sum-only originals in exactly the loops that carry an extremum
    q2, q15 = frontend.lower_function(Q.q2), frontend.lower_function(Q.q15)
    assert [repr(a) == repr(b) for a, b in zip(q2.ops, q2m.ops)] == [True] * 4 + [False] + [True] * 2
    assert repr(q15.ops[0]) == repr(q15m.ops[0]) and repr(q15.ops[1]) == repr(q15m.ops[2])


def test_sum_only_queries_lower_to_what_they_did():
    """q2 and q15 (and every other shipped query) against the plan digests recorded before smin / smax existed."""
    with open(os.path.join(ROOT, "tests", "golden", "reference_lowering.json")) as fh:
        rec = json.load(fh)["shipped_plan_digests"]
    assert "q2" in rec and "q15" in rec
    for name in sorted(rec):
        if name in Q.QUERIES:
            fp = hashlib.sha1(frontend.lower_function(Q.QUERIES[name]).fingerprint().encode()).hexdigest()[:16]
            assert fp == rec[name], name
    assert not any(isinstance(op, ExtremaOp) for name in Q.QUERIES for op in frontend.lower_function(Q.QUERIES[name]).ops)


def test_plans_with_extrema_are_not_deferred_or_recorded():
    """sdqh_table_extrema_end waits for the device: the engine knows from the plan that nothing of it is launched unwaited."""
    tail = ['d = T.sum(lambda p: {record({"k": p[0].k}): record({"s": p[0].v})} if p[0].v < 9.0 else None)', "out = d.sum(lambda g: {unique(g[0].concat(g[1])): True})"]
    assert engine.PreparedPlan._defer_names(_lower(*tail)) == frozenset(["d", "out"])
    assert engine.PreparedPlan._defer_names(_lower("top = U.sum(lambda q: smax(q[0].w))", *tail)) == frozenset()
    assert engine.PreparedPlan._defer_names(frontend.lower_function(Q.q3)) != frozenset()
    assert engine.PreparedPlan._defer_names(frontend.lower_function(Q.q15_max)) == frozenset()
    assert engine.PreparedPlan._defer_names(frontend.lower_function(Q.q2_min)) == frozenset()


@pytest.mark.parametrize("name", ["q15_max", "q2_min", "scalar", "per key"])
def test_a_library_without_the_extension_refuses_the_plan(oracle_lib, name):
    eng = engine.Engine(oracle_lib.context(threads=2))
    try:
        if name in Q.EXTREMA_QUERIES:
            db = tpch.generate(0.002, tables=sorted(tpch.columns_for([name])), columns=tpch.columns_for([name]))
            plan, args = frontend.lower_function(Q.EXTREMA_QUERIES[name]), [db[t] for t in Q.QUERY_TABLES[name]]
        else:
            from sdqlpy_amd.sdql_lib import table_from_columns
            t = table_from_columns(["k", "v"], [np.arange(8, dtype=np.int64) % 3, np.arange(8, dtype=np.float64)])
            body = "smax(p[0].v)" if name == "scalar" else "{p[0].k: smin(p[0].v)}"
            plan, args = frontend.lower_source("def f(T):\n    out = T.sum(lambda p: %s)\n    return out\n" % body), [t]
        for _ in range(2):
            with pytest.raises(UnsupportedQuery) as e:
                engine.execute_plan(eng, plan, args)
            assert "extrema extension" in str(e.value) and "sdqh_extrema.h" in str(e.value) and "libsdqloracle" in str(e.value)
    finally:
        eng.close()


# ---- the encoding, restated (tests/test_extrema_gpu.py carries the same few lines) -------------------------------------------------
TOP = np.uint64(1) << np.uint64(63)
QNAN = np.uint64(0x7FF8000000000000)


def encode(v, is_min):
    """float64 array -> uint64: 0 for a NaN, else bits u -> ~u if the sign bit is set else u | 2^63; for MIN the complement."""
    v = np.ascontiguousarray(v, np.float64)
    u = v.view(np.uint64)
    e = np.where(u >> np.uint64(63) != 0, ~u, u | TOP)
    if is_min:
        e = ~e
    return np.where(np.isnan(v), np.uint64(0), e)


def decode(e, is_min):
    e = np.ascontiguousarray(e, np.uint64)
    u = ~e if is_min else e
    bits = np.where(u >> np.uint64(63) != 0, u ^ TOP, ~u)
    return np.where(e == 0, QNAN, bits).view(np.float64)


DBL_MAX = np.finfo(np.float64).max
EDGE = np.array([-np.inf, -DBL_MAX, -1.5, -1.0, -2.2250738585072014e-308, -2.2250738585072009e-308, -5e-324, -0.0,
                 0.0, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.0, 1.5, DBL_MAX, np.inf], np.float64)      # ascending in the total order


def test_encoding_restated_in_numpy():
    assert np.signbit(EDGE[7]) and not np.signbit(EDGE[8])
    up, down = encode(EDGE, False), encode(EDGE, True)
    assert (np.diff(up.astype(object)) > 0).all()                    # order-preserving (strictly: -0.0 below +0.0), MAX
    assert (np.diff(down.astype(object)) < 0).all()                  # reversed for MIN: the unsigned maximum is the smallest value
    for is_min, e in ((False, up), (True, down)):
        assert (e != 0).all()                                        # never the identity for a value
        assert (decode(e, is_min).view(np.int64) == EDGE.view(np.int64)).all()      # its own inverse through decode, bit for bit
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 63, 20000, dtype=np.uint64) | (rng.integers(0, 2, 20000, dtype=np.uint64) << np.uint64(63))
    vals = bits.view(np.float64)
    num = ~np.isnan(vals)
    for is_min in (False, True):
        e = encode(vals, is_min)
        assert (e[num] != 0).all() and (e[~num] == 0).all()
        assert (decode(e, is_min)[num].view(np.uint64) == bits[num]).all()
        assert np.isnan(decode(e, is_min)[~num]).all()
        order = np.argsort(e[num], kind="stable")
        v = vals[num][order]
        assert (np.diff(v) <= 0).all() if is_min else (np.diff(v) >= 0).all()
    nan = np.array([np.nan, -np.nan, np.float64(np.nan)], np.float64)
    assert (encode(nan, True) == 0).all() and (encode(nan, False) == 0).all() and np.isnan(decode(np.zeros(2, np.uint64), True)).all()
    assert decode(np.zeros(1, np.uint64), False).view(np.uint64)[0] == QNAN
    # what a fold computes: the unsigned maximum of the encodings, whatever the order of the rows
    v = np.array([0.0, -0.0, 3.0, np.nan, -7.0, -0.0, 0.0], np.float64)
    for perm in (np.arange(7), np.arange(7)[::-1], rng.permutation(7)):
        assert decode(np.array([encode(v[perm], True).max()]), True)[0] == -7.0
        assert decode(np.array([encode(v[perm], False).max()]), False)[0] == 3.0
    z = np.array([0.0, -0.0])
    for perm in ([0, 1], [1, 0]):
        assert np.signbit(decode(np.array([encode(z[perm], True).max()]), True)[0])           # min{+0.0, -0.0} = -0.0
        assert not np.signbit(decode(np.array([encode(z[perm], False).max()]), False)[0])     # max = +0.0


# ---- the engine's routing: numpy stand-ins for the two device calls ------------------------------------------------------------------
def _stand_ins(calls):
    """What the engine hands to the extension, recorded (the columns read back); the scalar call answers like the device would.  The
    table call cannot write a CPU table's slots: the rows it is given are what is checked."""
    def table_extrema(self, table, key, nrows, slot_ops, count_hits=False):
        calls.append(("table", int(nrows), key.download(0, nrows), [(int(s), int(o), c.download(0, nrows), bool(f), c.dtype) for s, o, c, f in slot_ops], bool(count_hits)))

    def column_extrema(self, col, nrows, is_f64=None):
        v = col.download(0, nrows) if nrows else np.zeros(0)
        if (is_f64 or (is_f64 is None and col.dtype == abi.F64)) and v.dtype != np.float64:
            v = v.view(np.float64)
        calls.append(("column", int(nrows), v))
        v = v.astype(np.float64)
        v = v[~np.isnan(v)]
        return (float(v.min()), float(v.max()), len(v)) if len(v) else (float("nan"), float("nan"), 0)
    return table_extrema, column_extrema


def test_engine_routes_and_what_it_folds(oracle_lib, monkeypatch):
    from sdqlpy_amd.sdql_lib import table_from_columns
    calls = []
    te, ce = _stand_ins(calls)
    monkeypatch.setattr(abi.Context, "table_extrema", te)
    monkeypatch.setattr(abi.Context, "column_extrema", ce)
    monkeypatch.setattr(oracle_lib, "has_extrema", True)
    rng = np.random.default_rng(8)
    n = 5003
    k, j, d = np.sort(rng.integers(0, 700, n)).astype(np.int64), rng.integers(0, 5, n).astype(np.int64), rng.integers(0, 10, n).astype(np.int64)
    v, w = rng.integers(-999, 999, n) / 8.0, rng.integers(-50, 50, n).astype(np.int64)
    T = table_from_columns(["k", "j", "d", "v", "w"], [k, j, d, v, w])
    eng = engine.Engine(oracle_lib.context(threads=2))

    def run(*lines):
        del calls[:]
        plan = frontend.lower_source("def f(T):\n" + "".join("    %s\n" % ln for ln in lines) + "    return out\n")
        return engine.execute_plan(eng, plan, [T])

    def routes():
        return {(r["result"], r["route"]) for r in eng.stats()["extrema_loops"]}

    def same_rows(got, want):
        """the rows of a compaction come in segments of the scan: compared as multisets"""
        a = np.lexsort([np.ascontiguousarray(c).view(np.int64) for c in reversed(got)])
        b = np.lexsort([np.ascontiguousarray(c).view(np.int64) for c in reversed(want)])
        return all(len(x) == len(y) and (np.ascontiguousarray(x).view(np.int64)[a] == np.ascontiguousarray(y).view(np.int64)[b]).all() for x, y in zip(got, want))
    try:
        # no condition, plain columns: the table's own columns, no extra pass; the loop itself ran with constants in the extremum slots
        res = run('out = T.sum(lambda p: {p[0].k: record({"lo": smin(p[0].w), "n": 1, "hi": smax(p[0].v), "total": p[0].v})})')
        (kind, rows, key, slots, count_hits), = calls
        assert (kind, rows, count_hits) == ("table", n, False) and (key == k).all() and routes() == {("out", "columns")}
        assert [(s, o, f, dt) for s, o, _, f, dt in slots] == [(0, abi.EXT_MIN, False, abi.I64), (1, abi.EXT_MAX, True, abi.F64)]      # "n" is the hit count: no slot
        assert (slots[0][2] == w).all() and (slots[1][2] == v).all()
        vals = dict(res.val_fields)
        groups, entry = np.unique(k, return_inverse=True)
        assert (np.sort(dict(res.key_fields)["k"]) == groups).all() and vals["lo"].dtype == np.int64 and vals["hi"].dtype == np.float64
        assert sorted(vals["n"].tolist()) == sorted(np.bincount(entry).tolist()) and abs(vals["total"].sum() - v.sum()) < 1e-6
        # a condition, an expression, a composite key: the rows compacted by the loop's own gates, keyed as the aggregation keys its table
        run('out = T.sum(lambda p: {record({"a": p[0].k, "b": p[0].j}): smax(p[0].v * 2.0)} if p[0].d < 4 and p[0].w != 3 else None)')
        (kind, rows, key, slots, _), = calls
        m = (d < 4) & (w != 3)
        assert routes() == {("out", "compacted")} and rows == m.sum() and [(s, o, f) for s, o, _, f, _ in slots] == [(0, abi.EXT_MAX, True)]
        assert same_rows([key, slots[0][2]], [(k[m] << 32) | j[m], (v[m] * 2.0).view(np.int64)])
        # scalars: the column itself, or the compacted values; an integer extremum is an int
        assert run("out = T.sum(lambda p: smin(p[0].w))") == int(w.min()) and calls[0][:2] == ("column", n) and routes() == {("out", "columns")}
        got = run("out = T.sum(lambda p: smax(p[0].v) if p[0].d == 7 else None)")
        assert got == v[d == 7].max() and isinstance(got, float) and calls[0][1] == (d == 7).sum() and routes() == {("out", "compacted")}
        assert np.isnan(run("out = T.sum(lambda p: smax(p[0].v) if p[0].d > 77 else None)")) and calls[0][1] == 0
        # over a result dictionary: its entries as columns (sdqh_table_columns), always compacted
        sums = np.bincount(entry, weights=v)
        got = run("g = T.sum(lambda p: {p[0].k: p[0].v})", "out = g.sum(lambda e: smax(e[1]))")
        assert abs(got - sums.max()) < 1e-9 and calls[0][1] == len(groups) and ("out", "compacted") in routes()
        got = run("g = T.sum(lambda p: {p[0].k: p[0].v})", "best = g.sum(lambda e: smax(e[1]))",
                  'out = g.sum(lambda e: {unique(record({"k": e[0], "s": e[1]})): True} if e[1] == best else None)')
        assert got.rows() == [(int(groups[np.argmax(sums)]), got.rows()[0][1])] and abs(got.rows()[0][1] - sums.max()) < 1e-9
        run('g = T.sum(lambda p: {record({"a": p[0].k, "b": p[0].j}): p[0].v})',
            'out = g.sum(lambda e: {e[0].b: record({"least": smin(e[1]), "most": smax(e[1])})} if e[1] != 0.125 else None)')
        (kind, rows, key, slots, _), = calls
        pair, e2 = np.unique((k << 32) | j, return_inverse=True)
        psum = np.bincount(e2, weights=v)
        keep = psum != 0.125
        assert rows == keep.sum() and [(s, o, f) for s, o, _, f, _ in slots] == [(0, abi.EXT_MIN, True), (1, abi.EXT_MAX, True)]
        assert sorted(key.tolist()) == sorted((pair[keep] & 0xFFFFFFFF).tolist())
        assert np.allclose(np.sort(slots[0][2].view(np.float64)), np.sort(psum[keep]), rtol=0, atol=1e-9)
    finally:
        eng.close()
