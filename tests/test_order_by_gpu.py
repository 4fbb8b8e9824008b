"""ORDER BY on the MI355X (run with -m gpu): sdqh_table_sorted (include/sdqh_sort.h) against numpy at every size at which it takes
another path, against sdqh_table_topk where both apply, on edge values, on every table layout, its overflow contract, and through the
engine and the decorator.  Comparisons are exact: the tables aggregate integer-valued doubles, so sums are the same in any order.

The expected rows are always the table's own K-F rows (sdqh_table_compact: stage order = build-row order) reordered by a STABLE
numpy lexsort over the documented order-preserving map, restated here in numpy — not imported from the code under test."""
import os

import numpy as np
import pytest

import edge_cases as E
from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q

pytestmark = pytest.mark.gpu

SPECS = [
    [(abi.SORT_VALUE, 0, True, True), (abi.SORT_PAYLOAD, 0, False, False)],                                          # value desc, payload asc
    [(abi.SORT_PAYLOAD, 0, True, False)],                                                                           # heavy ties: stage order decides almost everything
    [(abi.SORT_PAYLOAD, 1, False, True), (abi.SORT_HITS, 0, True, False), (abi.SORT_KEY, 0, True, False)],          # double payload asc, hits desc, key desc
    [(abi.SORT_KEY, 0, False, False)],
    [(abi.SORT_PAYLOAD, 0, False, False), (abi.SORT_HITS, 0, True, False), (abi.SORT_PAYLOAD, 1, True, True), (abi.SORT_VALUE, 0, False, True), (abi.SORT_KEY, 0, True, False)],
]
MIN_HITS = (0, 1, 2, 5)


@pytest.fixture(scope="module")
def hip_engine(hip_lib):
    eng = engine.Engine(hip_lib.context(device=0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oracle_engine(oracle_lib):
    eng = engine.Engine(oracle_lib.context(threads=min(16, os.cpu_count() or 1)))
    yield eng
    eng.close()


def _under(eng, options, run):
    for k, v in options.items():
        eng.ctx.set_option(k, v)
    eng.clear()
    try:
        return run()
    finally:
        for k in options:
            eng.ctx.set_option(k, 1)
        for k, v in E.DEFAULT_OPTIONS.items():
            eng.ctx.set_option(k, v)
        eng.clear()


def _sort_bits(a, is_f64, desc):
    """int64 x -> x ^ 2^63; float64 bits u -> ~u if the sign bit is set else u | 2^63; descending: the complement."""
    u = np.ascontiguousarray(a).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    u = np.where(u >> np.uint64(63) != 0, ~u, u | top) if is_f64 else u ^ top
    return ~u if desc else u


def _stage_rows(ctx, t, min_hits):
    cnt = ctx.table_compact_count(t, min_hits)
    return ctx.table_compact(t, min_hits, cnt, want_values=t.accumulate, want_hits=t.accumulate)


def _expected_order(rows, spec):
    keys, payload, values, hits = rows
    col = {abi.SORT_KEY: lambda i: keys, abi.SORT_PAYLOAD: lambda i: payload[i], abi.SORT_VALUE: lambda i: values[i], abi.SORT_HITS: lambda i: hits}
    lex = [_sort_bits(col[kind](index), kind == abi.SORT_VALUE or (kind == abi.SORT_PAYLOAD and is_f64), desc) for kind, index, desc, is_f64 in reversed(spec)]
    return np.lexsort(lex)                                               # stable; the last array is the primary column


def _same(got, rows, idx, what):
    gk, gp, gv, gh = got
    keys, payload, values, hits = rows
    assert len(gk) == len(idx), (what, len(gk), len(idx))
    assert (gk == keys[idx]).all(), what
    if payload is not None:
        for p in range(len(payload)):
            assert (gp[p] == payload[p][idx]).all(), (what, "payload", p)
    if values is not None:
        assert (gv[0].view(np.int64) == values[0][idx].view(np.int64)).all(), (what, "value")
    if hits is not None:
        assert (gh == hits[idx]).all(), (what, "hits")


def _check(ctx, t, specs, min_hits_set, what, limits=None):
    """Every spec x min_hits x limit in {1, n // 2, n, SORT_ALL} (n = the entries that min_hits selects) against numpy."""
    done = 0
    for min_hits in min_hits_set:
        rows = _stage_rows(ctx, t, min_hits)
        n = len(rows[0])
        for spec in specs:
            order = _expected_order(rows, spec)
            for limit in (limits or sorted({1, max(1, n // 2), max(1, n), abi.SORT_ALL})):
                got = ctx.table_sorted(t, min_hits, limit, spec, 64, want_hits=t.accumulate)
                _same(got, rows, order[:min(limit, n)], (what, min_hits, limit, spec))
                done += 1
    return done


def _probed_table(ctx, n, seed=9):
    """As helpers.topk_case: n entries (n distinct keys; up to 200 of them come twice in the build — the first row owns the entry),
    an integer payload of 50 values (heavy ties), a double payload, probed by three rows per build row with integer-valued doubles."""
    rng = np.random.default_rng(seed + n)
    distinct = rng.permutation(max(n, 1))[:n].astype(np.int64) * 5 + 3
    d = min(200, n // 2)
    keys = np.concatenate([distinct[:n // 2], distinct[:d], distinct[n // 2:]])
    rows = len(keys)
    pay_i = rng.integers(0, 50, rows).astype(np.int64)
    pay_f = (rng.integers(-500, 500, rows) / 4.0 + 0.0).astype(np.float64)
    pay_f[pay_f == 0.0] = 0.0                                              # no -0.0 here: the edge-value test has the pair
    pk = keys[rng.integers(0, rows, 3 * rows)] if rows else np.zeros(0, np.int64)
    pv = rng.integers(1, 1000, 3 * rows).astype(np.float64)
    ck, ci, cf, cpk, cpv = ctx.upload(keys), ctx.upload(pay_i), ctx.upload(pay_f.view(np.int64)), ctx.upload(pk), ctx.upload(pv)
    t = ctx.hash_build_unique(rows, abi.make_filter(), [], ck, [ci, cf], accumulate=True)
    if rows:
        ctx.hash_probe_aggregate(3 * rows, abi.make_filter(), t, cpk, abi.make_tuple(abi.TUPLE_A, [cpv]))
    assert ctx.table_compact_count(t, 0) == n
    return t


def _sizes(ctx):
    S, T, L = ctx.sort_geometry()
    return S, T, L, sorted({0, 1, 2, 63, 64, 65, S - 1, S, S + 1, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1, 5 * T + 17})


def test_geometry(hip_engine):
    S, T, L = hip_engine.ctx.sort_geometry()
    assert S >= 64 and T >= 64 and L >= 0 and 5 * T + 17 < 100000


# 1. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(15))
def test_sorted_against_numpy(hip_engine, which):
    """The which-th size of {0, 1, 2, 63, 64, 65, S-1, S, S+1, T-1, T, T+1, 2T+1, 3T-1, 5T+17} (fewer when some coincide)."""
    ctx = hip_engine.ctx
    sizes = _sizes(ctx)[3]
    if which >= len(sizes):
        return                                                           # (sizes of the set that coincide in this geometry)
    n = sizes[which]
    t = _probed_table(ctx, n)
    try:
        assert _check(ctx, t, SPECS, MIN_HITS, "n=%d" % n) >= 20
    finally:
        t.free()


@pytest.fixture(scope="module")
def large_table(hip_engine):
    """Where a second scan level would begin (L - 1, L, L + 1 when the library has one at a testable size), else one table of
    2 000 003 entries: tens of thousands of tiles, so a second level cannot hide."""
    ctx = hip_engine.ctx
    S, T, L, _ = _sizes(ctx)
    tables = {n: _probed_table(ctx, n) for n in ((L - 1, L, L + 1) if 0 < L <= 4_000_000 else (2_000_003,))}
    yield tables
    for t in tables.values():
        t.free()


@pytest.mark.parametrize("spec", range(len(SPECS)))
@pytest.mark.parametrize("min_hits", MIN_HITS)
def test_sorted_against_numpy_large(hip_engine, large_table, spec, min_hits):
    for n, t in large_table.items():
        assert _check(hip_engine.ctx, t, [SPECS[spec]], (min_hits,), "n=%d" % n) == 4


# 2. ------------------------------------------------------------------------------------------------------------------------------
def test_agrees_with_topk(hip_engine):
    ctx = hip_engine.ctx
    S, T, L, _ = _sizes(ctx)
    checked = 0
    for n in (S - 1, 5 * T + 17):
        t = _probed_table(ctx, n)
        try:
            for spec in SPECS:
                if len(spec) > abi.MAX_SORT_KEYS:
                    continue
                for min_hits in (0, 2):
                    for k in (1, 16, 17, 128):
                        a = ctx.table_sorted(t, min_hits, k, spec, k)
                        b = ctx.table_topk(t, min_hits, k, spec)
                        assert len(a[0]) == len(b[0]) == k
                        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2][0] == b[2][0]).all() and (a[3] == b[3]).all(), (n, spec, min_hits, k)
                        checked += 1
        finally:
            t.free()
    assert checked == 2 * 4 * 2 * 4


# 3. ------------------------------------------------------------------------------------------------------------------------------
I_MIN, I_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
EDGE_INTS = {
    "extremes": np.array([0, I_MAX, -1, I_MIN, 1, I_MIN + 1, I_MAX - 1, 255, 256, -256, 1 << 32, -(1 << 32)], np.int64),
    "top byte only": (np.arange(-128, 128, dtype=np.int64)[::-1] << 56) + 0x1234,
    "low byte only": np.arange(256, dtype=np.int64)[::-1] * 1 + (0x55 << 40),
    "all equal": np.full(7, -42, np.int64),
}
EDGE_DOUBLES = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072009e-308, 1.0, -1.0, 1.5, -1.5,
                         np.finfo(np.float64).max, np.finfo(np.float64).min, 0.0, -0.0], np.float64)


@pytest.mark.parametrize("n", [300, 1500, 2600])
@pytest.mark.parametrize("accumulate", [True, False])
def test_edge_values_in_sort_columns(hip_engine, n, accumulate):
    """INT64_MIN / INT64_MAX, keys that differ only in their top or only in their lowest byte (digit skipping both ways), all rows
    equal (the output is the stage order), +-inf, subnormals and the -0.0 / +0.0 pair — against the documented bit order: -0.0 sorts
    before +0.0.  n below and above the single-workgroup limit; every pattern repeats, so ties are everywhere."""
    ctx = hip_engine.ctx
    S, T, L, _ = _sizes(ctx)
    assert 300 < S < 1500 and 2600 > 5 * T
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) * 3 - n
    cf = ctx.upload(np.resize(EDGE_DOUBLES, n).view(np.int64))
    ck = ctx.upload(keys)
    done = 0
    for name, pattern in EDGE_INTS.items():
        ci = ctx.upload(np.resize(pattern, n))
        t = ctx.hash_build_unique(n, abi.make_filter(), [], ck, [ci, cf], accumulate=accumulate)
        try:
            rows = _stage_rows(ctx, t, 0)
            assert len(rows[0]) == n and (rows[0] == keys).all()                       # stage order = build-row order
            for spec in ([(abi.SORT_PAYLOAD, 0, False, False)], [(abi.SORT_PAYLOAD, 0, True, False)],
                         [(abi.SORT_PAYLOAD, 1, False, True)], [(abi.SORT_PAYLOAD, 1, True, True), (abi.SORT_PAYLOAD, 0, False, False)]):
                order = _expected_order(rows, spec)
                got = ctx.table_sorted(t, 0, abi.SORT_ALL, spec, n, want_hits=accumulate)
                _same(got, rows, order, (name, spec))
                done += 1
            if name == "all equal":
                got = ctx.table_sorted(t, 0, abi.SORT_ALL, [(abi.SORT_PAYLOAD, 0, True, False)], n, want_hits=accumulate)
                assert (got[0] == keys).all()
            if name == "extremes":
                asc = ctx.table_sorted(t, 0, abi.SORT_ALL, [(abi.SORT_PAYLOAD, 0, False, False)], n, want_hits=accumulate)[1][0]
                assert asc[0] == I_MIN and asc[-1] == I_MAX and (np.diff(asc.astype(object)) >= 0).all()
                f = ctx.table_sorted(t, 0, abi.SORT_ALL, [(abi.SORT_PAYLOAD, 1, False, True)], n, want_hits=accumulate)[1][1].view(np.float64)
                assert f[0] == -np.inf and f[-1] == np.inf and (np.diff(f[np.isfinite(f)]) >= 0).all()
                zeros = np.nonzero(f == 0.0)[0]
                sign = np.signbit(f[zeros])
                assert sign.any() and not sign.all() and (np.diff(sign.astype(np.int8)) <= 0).all()     # every -0.0 before every +0.0
        finally:
            t.free()
    assert done == 16


# 4. ------------------------------------------------------------------------------------------------------------------------------
def test_groupby_key_table(hip_engine):
    ctx = hip_engine.ctx
    S, T, L, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(4)
    groups = rng.permutation(n).astype(np.int64) * 7 - 1000
    keys = np.concatenate([groups, groups[rng.integers(0, n, 4 * n)]])
    keys = keys[rng.permutation(len(keys))]
    v = rng.integers(1, 60, len(keys)).astype(np.float64)
    t = ctx.groupby_key(len(keys), abi.make_filter(), ctx.upload(keys), abi.make_tuple(abi.TUPLE_A, [ctx.upload(v)]))
    try:
        assert ctx.table_compact_count(t, 1) == n
        specs = [[(abi.SORT_VALUE, 0, True, True), (abi.SORT_KEY, 0, False, False)], [(abi.SORT_HITS, 0, True, False), (abi.SORT_VALUE, 0, False, True), (abi.SORT_KEY, 0, True, False)],
                 [(abi.SORT_HITS, 0, False, False)], [(abi.SORT_KEY, 0, False, False)]]
        assert _check(ctx, t, specs, (1, 2, 5), "groupby_key") >= 36
    finally:
        t.free()


def test_open_addressing_table(hip_engine):
    ctx = hip_engine.ctx
    n = 2 * _sizes(ctx)[1] + 1

    def run():
        t = _probed_table(ctx, n)
        try:
            return _check(ctx, t, SPECS, MIN_HITS, "hash layout")
        finally:
            t.free()
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, run) >= 60


def test_shared_groups(hip_engine):
    """After sdqh_table_share_groups, with min_hits = 1: one row per group."""
    ctx = hip_engine.ctx
    n = 2 * _sizes(ctx)[1] + 1
    rng = np.random.default_rng(21)
    rows = 4 * n
    keys = rng.permutation(rows).astype(np.int64) + 100
    pa = np.concatenate([np.arange(n), rng.integers(0, n, rows - n)]).astype(np.int64)[rng.permutation(rows)]      # n groups
    pb = (pa % 5).astype(np.int64)
    t = ctx.hash_build_unique(rows, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(pa), ctx.upload(pb)], accumulate=True)
    try:
        ctx.table_share_groups(t, [0], [0], [n])
        pk = np.concatenate([keys, keys[rng.integers(0, rows, 2 * rows)]])
        ctx.hash_probe_aggregate(len(pk), abi.make_filter(), t, ctx.upload(pk), abi.make_tuple(abi.TUPLE_A, [ctx.upload(rng.integers(1, 50, len(pk)).astype(np.float64))]))
        assert ctx.table_compact_count(t, 1) == n
        specs = [[(abi.SORT_VALUE, 0, True, True), (abi.SORT_PAYLOAD, 1, False, False)], [(abi.SORT_PAYLOAD, 1, True, False)],
                 [(abi.SORT_HITS, 0, True, False), (abi.SORT_PAYLOAD, 0, True, False)], [(abi.SORT_KEY, 0, False, False)]]
        assert _check(ctx, t, specs, (1,), "shared groups") >= 12
    finally:
        t.free()


# 5. ------------------------------------------------------------------------------------------------------------------------------
def test_overflow_contract(hip_engine):
    import ctypes as C
    ctx = hip_engine.ctx
    n = 3 * _sizes(ctx)[1] - 1
    t = _probed_table(ctx, n)
    try:
        spec = SPECS[0]
        arr = (abi.SortKey * len(spec))()
        for i, (kind, index, desc, is_f64) in enumerate(spec):
            arr[i].kind, arr[i].index, arr[i].descending, arr[i].is_f64 = kind, index, int(desc), int(is_f64)
        cap = 100
        keys = np.full(cap, -7, np.int64)
        got = C.c_int64()

        def call(limit, capacity, out):
            return ctx.lib.sdqh_table_sorted(ctx.handle, t.handle, C.c_int64(0), C.c_int64(limit), C.c_int(len(spec)), arr, C.c_int64(capacity),
                                             out, None, None, None, C.byref(got))
        assert call(abi.SORT_ALL, cap, keys.ctypes.data_as(C.c_void_p)) == abi.ERR_OVERFLOW and got.value == n and (keys == -7).all()
        assert call(cap + 1, cap, keys.ctypes.data_as(C.c_void_p)) == abi.ERR_OVERFLOW and got.value == cap + 1 and (keys == -7).all()
        assert call(abi.SORT_ALL, 0, None) == abi.OK and got.value == n                        # count only
        assert call(50, 0, None) == abi.OK and got.value == 50
        assert call(cap, cap, keys.ctypes.data_as(C.c_void_p)) == abi.OK and got.value == cap and (keys != -7).all()
        assert call(0, cap, keys.ctypes.data_as(C.c_void_p)) == abi.ERR_INVALID
        rows = _stage_rows(ctx, t, 0)
        order = _expected_order(rows, spec)
        assert (keys == rows[0][order[:cap]]).all()
        _same(ctx.table_sorted(t, 0, abi.SORT_ALL, spec, 10), rows, order, "retry with the exact capacity")
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_sorted(t, 0, 10, [(abi.SORT_PAYLOAD, 2, False, False)], 10)              # a field the table lacks
        assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_sorted(t, 0, 10, [(abi.SORT_KEY, 0, False, False)] * (abi.SORT_MAX_KEYS + 1), 10)
        assert e.value.code == abi.ERR_INVALID
    finally:
        t.free()


# 6. / 7. -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    qs = ["q3", "q18"]
    return tpch.generate(0.2, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))


def _run(eng, name, db, top=None):
    query = Q.large_orders(200) if name == "q18 from 200" else Q.QUERIES[name]          # (q18 keeps a dozen rows at this size: also with its HAVING threshold lowered)
    return engine.execute_plan(eng, frontend.lower_function(query), [db[t] for t in Q.QUERY_TABLES[name.split()[0]]], top=top)


def _close(a, b):
    return a == b if not isinstance(a, float) else abs(a - b) <= 1e-10 * max(abs(a), abs(b))


def _order_key(res, order):
    """Per row, the order's columns as a tuple that sorts ascending (numeric columns only)."""
    cols = [res.column(name).tolist() for name, _ in order]
    sign = [-1 if d == "desc" else 1 for _, d in order]
    return [tuple(s * x for s, x in zip(sign, row)) for row in zip(*cols)]


def _before(a, b):
    """Does order tuple a sort strictly before b by more than the tolerance?"""
    for x, y in zip(a, b):
        if _close(x, y):
            continue
        return x < y
    return False


@pytest.mark.parametrize("name", ["q3", "q18", "q18 from 200"])
def test_through_the_engine(hip_engine, db, name, monkeypatch):
    """order_by, top(129) and top(1000) through the device call, then (7.) with Engine.device_sort off through the host route.  Sums
    may differ in their last bits between runs, so every result is checked by properties against the engine's unordered result:
    (a) its rows are rows of that result, matched by key, numbers within 1e-10 relative; (b) they are non-decreasing under the order
    by their own column values; (c) for k < n no excluded row sorts strictly before the last included one by more than that."""
    order = Q.TPCH_ORDER[name.split()[0]][1]
    everything = _run(hip_engine, name, db)
    ident = "l_orderkey" if name == "q3" else "o_orderkey"
    at = everything.columns.index(ident)
    full = {r[at]: r for r in everything.ordered_rows()}
    full_keys = dict(zip(everything.column(ident).tolist(), _order_key(everything, order)))
    n = len(full)
    assert n == len(everything.ordered_rows()) and (n > 0 if name == "q18" else n > 1000)

    def check(res, k):
        rows = res.ordered_rows()
        assert res.columns == everything.columns and len(rows) == min(k, n)
        ids = [r[at] for r in rows]
        assert len(set(ids)) == len(ids)
        for r in rows:
            assert all(_close(x, y) for x, y in zip(r, full[r[at]])), r
        keys = _order_key(res, order)
        assert not any(_before(b, a) for a, b in zip(keys, keys[1:]))
        if k < n:
            taken = set(ids)
            assert not any(_before(full_keys[i], keys[-1]) for i in full if i not in taken)

    calls = []
    real = abi.Context.table_sorted

    def spy(self, *a, **kw):
        calls.append(a[2])
        return real(self, *a, **kw)
    monkeypatch.setattr(abi.Context, "table_sorted", spy)
    for k in (abi.SORT_ALL, 129, 1000):
        res = _run(hip_engine, name, db, top=(k, order))
        assert calls and calls[-1] == k
        check(res, k)
    ncalls = len(calls)
    assert ncalls == 3
    hip_engine.device_sort = False
    try:
        for k in (abi.SORT_ALL, 129, 1000):
            check(_run(hip_engine, name, db, top=(k, order)), k)
        assert len(calls) == ncalls
    finally:
        hip_engine.device_sort = True


def test_order_by_on_the_decorator(hip_lib, db, monkeypatch):
    from sdqlpy_amd import sdql_lib
    calls = []
    real = abi.Context.table_sorted
    monkeypatch.setattr(abi.Context, "table_sorted", lambda self, *a, **kw: (calls.append(a[2]), real(self, *a, **kw))[1])
    engine.use_engine(engine.Engine(hip_lib.context(device=0)))
    try:
        order = Q.TPCH_ORDER["q3"][1]
        args = [db[t] for t in Q.QUERY_TABLES["q3"]]
        res = Q.q3.order_by(order)(*args)
        assert calls == [abi.SORT_ALL] and len(res.ordered_rows()) == len(Q.q3(*args).rows())
        keys = _order_key(res, order)
        assert not any(_before(b, a) for a, b in zip(keys, keys[1:]))
    finally:
        engine.reset_default_engine()
        sdql_lib._state.update(mode=None)
