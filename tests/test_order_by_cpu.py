"""ORDER BY beyond sdqh_table_topk, the part that needs no GPU: the ordering extension's symbols (include/sdqh_sort.h, abi.SORT_EXPORTS)
in the cross-compiled library and nowhere in the common boundary, the CPU implementation without them, `order_by` on the decorator, and
the engine's routing — checked with a numpy stand-in for abi.Context.table_sorted.  The GPU half is tests/test_order_by_gpu.py."""
import os
import re

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = [("revenue", "desc"), ("o_orderdate", "asc"), ("o_shippriority", "asc"), ("l_orderkey", "desc")]


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(sdqh_[a-z_0-9]+)\s*\(", text)))


def test_extension_symbols_are_exported_and_stay_out_of_the_common_boundary(hip_lib):
    assert sorted(abi.SORT_EXPORTS) == _declared("sdqh_sort.h")
    for s in abi.SORT_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert s not in abi.EXPORTS and s not in _declared("sdqh.h")
    assert hip_lib.has_sort
    assert abi.SORT_MAX_KEYS == 8 and abi.SORT_ALL == 1 << 62 and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort.h")).read()
    assert re.search(r"#define\s+SDQH_SORT_MAX_KEYS\s+8\b", text) and "<< 62" in text


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_sort is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        for call in (lambda: ctx.table_sorted(t, 0, abi.SORT_ALL, [(abi.SORT_KEY, 0, False, False)], 16), ctx.sort_geometry):
            with pytest.raises(abi.SdqhError) as e:
                call()
            assert e.value.code == abi.ERR_UNSUPPORTED
        t.free()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def db():
    qs = ["q3", "q18"]
    return tpch.generate(0.05, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))


@pytest.fixture()
def oracle_engine(oracle_lib):
    eng = engine.Engine(oracle_lib.context(threads=min(8, os.cpu_count() or 1)))
    yield eng
    eng.close()


def _run(eng, name, db, top=None):
    return engine.execute_plan(eng, frontend.lower_function(Q.QUERIES[name]), [db[t] for t in Q.QUERY_TABLES[name]], top=top)


@pytest.mark.parametrize("name,least", [("q3", 100), ("q18", 1), ("q18 from 200", 100)])
def test_order_by_is_top_without_a_limit(oracle_lib, db, name, least):
    """Through the decorator on the CPU implementation (the host route): every row, in the order top(10**9, order) gives.  (q18 keeps
    a row or two at this size: also with its HAVING threshold lowered to 200.)"""
    from sdqlpy_amd import sdql_lib
    query = Q.large_orders(200) if name == "q18 from 200" else Q.QUERIES[name]
    name = name.split()[0]
    order = Q.TPCH_ORDER[name][1]
    args = [db[t] for t in Q.QUERY_TABLES[name]]
    engine.use_engine(engine.Engine(oracle_lib.context(threads=min(8, os.cpu_count() or 1))))
    try:
        got = query.order_by(order)(*args)
        want = query.top(10 ** 9, order)(*args)
        everything = query(*args)
        assert got.columns == want.columns and got.ordered_rows() == want.ordered_rows()
        assert len(got.ordered_rows()) == len(everything.rows()) >= least and sorted(got.ordered_rows()) == everything.rows()
    finally:
        engine.reset_default_engine()
        sdql_lib._state.update(mode=None)


# ---- routing: a numpy stand-in for the device call ---------------------------------------------------------------------------------
def _sort_bits(a, is_f64, desc):
    """The order-preserving map onto uint64, restated: int64 x -> x ^ 2^63; float64 bits u -> ~u if the sign bit is set else u | 2^63;
    descending: the complement."""
    u = np.ascontiguousarray(a).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    u = np.where(u >> np.uint64(63) != 0, ~u, u | top) if is_f64 else u ^ top
    return ~u if desc else u


def _stand_in(calls):
    def table_sorted(self, table, min_hits, limit, sort, capacity_hint, want_hits=True):
        calls.append((int(limit), list(sort)))
        cnt = self.table_compact_count(table, min_hits)
        keys, payload, values, hits = self.table_compact(table, min_hits, cnt)
        col = {abi.SORT_KEY: lambda i: keys, abi.SORT_PAYLOAD: lambda i: payload[i], abi.SORT_VALUE: lambda i: values[i], abi.SORT_HITS: lambda i: hits}
        lex = [_sort_bits(col[kind](index), kind == abi.SORT_VALUE or (kind == abi.SORT_PAYLOAD and is_f64), desc) for kind, index, desc, is_f64 in reversed(sort)]
        idx = np.lexsort(lex)[:min(int(limit), cnt)]                      # stable: ties keep stage order
        return (keys[idx], None if payload is None else payload[:, idx], None if values is None else values[:, idx], hits[idx] if want_hits else None)
    return table_sorted


def test_engine_routes_large_orders_to_the_device_call(oracle_engine, db, monkeypatch):
    order = Q.TPCH_ORDER["q3"][1]
    host = {k: _run(oracle_engine, "q3", db, top=(k, o)).ordered_rows() for k, o in ((129, order), (abi.SORT_ALL, order), (10, order), (7, FOUR))}
    assert len(host[abi.SORT_ALL]) > 129 == len(host[129])
    calls = []
    monkeypatch.setattr(abi.Context, "table_sorted", _stand_in(calls))
    monkeypatch.setattr(oracle_engine.ctx.library, "has_sort", True)
    assert _run(oracle_engine, "q3", db, top=(129, order)).ordered_rows() == host[129]
    assert len(calls) == 1 and calls[0][0] == 129 and len(calls[0][1]) == 2 and calls[0][1][0][0] == abi.SORT_VALUE and calls[0][1][0][2]
    assert _run(oracle_engine, "q3", db, top=(abi.SORT_ALL, order)).ordered_rows() == host[abi.SORT_ALL]
    assert len(calls) == 2 and calls[1][0] == abi.SORT_ALL
    assert _run(oracle_engine, "q3", db, top=(7, FOUR)).ordered_rows() == host[7]           # four columns: beyond MAX_SORT_KEYS whatever k
    assert len(calls) == 3 and calls[2][0] == 7 and len(calls[2][1]) == 4
    assert _run(oracle_engine, "q3", db, top=(10, order)).ordered_rows() == host[10]        # what sdqh_table_topk serves stays with it
    assert len(calls) == 3
    oracle_engine.device_sort = False
    assert _run(oracle_engine, "q3", db, top=(129, order)).ordered_rows() == host[129]
    assert _run(oracle_engine, "q3", db, top=(abi.SORT_ALL, order)).ordered_rows() == host[abi.SORT_ALL]
    assert len(calls) == 3
