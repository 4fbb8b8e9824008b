"""ORDER BY over text, packed keys and mixed-radix keys, the part that needs no GPU: the sort-terms extension's symbols
(include/sdqh_sort_terms.h, abi.SORT_TERMS_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation without them,
and the engine's routing — checked with numpy stand-ins for abi.Context.table_sorted_by and abi.Context.text_ranks on the CPU
implementation.  The GPU half is tests/test_order_terms_gpu.py."""
import os
import re

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q
from order_terms_queries import (BY_NAME_ORDER, BY_PAIR_ORDER, BY_PAIR_ORDER_2, BY_TEXT_KEY_ORDERS, BY_TEXT_PART_ORDERS, SUPPLIER_COLUMNS, balance_by_name,
                                 balance_by_name_and_nation, permuted_suppliers, shuffled_suppliers, suppliers_by_name, suppliers_by_pair)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(sdqh_[a-z_0-9]+)\s*\(", text)))


# 1. ---------------------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.SORT_TERMS_EXPORTS) == _declared("sdqh_sort_terms.h")
    for s in abi.SORT_TERMS_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        assert s not in abi.EXPORTS and s not in abi.SORT_EXPORTS and s not in _declared("sdqh.h") and s not in _declared("sdqh_sort.h")
    assert hip_lib.has_sort_terms and hip_lib.has_sort
    assert abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort_terms.h")).read()
    assert re.search(r"#define\s+SDQH_TEXT_RANK_MAX_WIDTH\s+%d\b" % abi.TEXT_RANK_MAX_WIDTH, text)


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_sort_terms is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        s = ctx.upload(np.array(["b", "a"], "<U1"))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        for call in (lambda: ctx.table_sorted_by(t, 0, abi.SORT_ALL, [(abi.SORT_KEY, 0, False, False, 0, 2, 0, None)], 16), lambda: ctx.text_ranks(s, 2)):
            with pytest.raises(abi.SdqhError) as e:
                call()
            assert e.value.code == abi.ERR_UNSUPPORTED
        t.free()
    finally:
        ctx.close()


# 2. routing: numpy stand-ins for the two device calls -----------------------------------------------------------------------------------
def _sort_bits(a, is_f64, desc):
    """int64 x -> x ^ 2^63; float64 bits u -> ~u if the sign bit is set else u | 2^63; descending: the complement."""
    u = np.ascontiguousarray(a).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    u = np.where(u >> np.uint64(63) != 0, ~u, u | top) if is_f64 else u ^ top
    return ~u if desc else u


def _ranks_stand_in(calls):
    def text_ranks(self, column, nrows):
        text = column.download(0, nrows)
        calls.append((nrows, text.dtype.str))
        uniq, inv = np.unique(text, return_inverse=True)
        return self.upload(np.ascontiguousarray(inv, np.int64).reshape(nrows)), len(uniq)
    return text_ranks


def _sorted_by_stand_in(calls):
    """A stable lexsort over the derived columns of the compacted rows: field = (uint64(source) / div) % mod + add, then ranks[field]."""
    def table_sorted_by(self, table, min_hits, limit, terms, capacity_hint, want_hits=True):
        calls.append((int(limit), [tuple(t[:7]) + (t[7] is not None,) if len(t) > 4 else tuple(t) for t in terms]))
        cnt = self.table_compact_count(table, min_hits)
        keys, payload, values, hits = self.table_compact(table, min_hits, cnt, want_values=table.accumulate, want_hits=table.accumulate)
        col = {abi.SORT_KEY: lambda i: keys, abi.SORT_PAYLOAD: lambda i: payload[i], abi.SORT_VALUE: lambda i: values[i], abi.SORT_HITS: lambda i: hits}
        lex = []
        for t in reversed(terms):
            kind, index, desc, is_f64 = t[:4]
            src = col[kind](index)
            if len(t) > 4:
                div, mod, add, ranks = t[4:]
                f = np.ascontiguousarray(src).view(np.uint64)
                if div > 1:
                    f = f // np.uint64(div)
                if mod:
                    f = f % np.uint64(mod)
                v = f.astype(np.int64) + np.int64(add)
                if ranks is not None:
                    table_of_ranks = ranks.download()
                    assert ((v >= 0) & (v < len(table_of_ranks))).all()
                    v = table_of_ranks[v]
                lex.append(_sort_bits(v, False, desc))
            else:
                lex.append(_sort_bits(src, kind == abi.SORT_VALUE or (kind == abi.SORT_PAYLOAD and is_f64), desc))
        idx = np.lexsort(lex)[:min(int(limit), cnt)]                      # stable: ties keep stage order
        return (keys[idx], None if payload is None else payload[:, idx], None if values is None else values[:, idx],
                hits[idx] if want_hits and hits is not None else None)
    return table_sorted_by


Q2_SCALE = 0.8      # the smallest tenth at which q2's last loop runs on the device (its `offers` reach 256 rows); asserted below


@pytest.fixture(scope="module")
def db():
    qs = ["q16", "q3", "q18"]
    return tpch.generate(0.05, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))


@pytest.fixture(scope="module")
def db_q2():
    return tpch.generate(Q2_SCALE, tables=sorted(tpch.columns_for(["q2"])), columns=tpch.columns_for(["q2"]))


@pytest.fixture(scope="module")
def suppliers():
    return tpch.generate(0.05, tables=["supplier"], columns={"supplier": SUPPLIER_COLUMNS})["supplier"]


@pytest.fixture(scope="module")
def shuffled(suppliers):
    return shuffled_suppliers(suppliers)


@pytest.fixture()
def oracle_engine(oracle_lib):
    eng = engine.Engine(oracle_lib.context(threads=min(8, os.cpu_count() or 1)))
    yield eng
    eng.close()


@pytest.fixture()
def stand_ins(oracle_engine, monkeypatch):
    sorted_by, ranks, plain = [], [], []
    monkeypatch.setattr(abi.Context, "table_sorted_by", _sorted_by_stand_in(sorted_by))
    monkeypatch.setattr(abi.Context, "text_ranks", _ranks_stand_in(ranks))
    monkeypatch.setattr(abi.Context, "table_sorted", _sorted_by_stand_in(plain))        # (the same lexsort serves the plain call: 4-tuples)
    monkeypatch.setattr(oracle_engine.ctx.library, "has_sort", True)
    monkeypatch.setattr(oracle_engine.ctx.library, "has_sort_terms", True)
    return sorted_by, ranks, plain


def _run(eng, query, tables, top=None):
    query = Q.QUERIES[query] if isinstance(query, str) else query
    return engine.execute_plan(eng, frontend.lower_function(query), tables, top=top)


def _both_ways(eng, query, tables, order, calls):
    """order_by(order) and top(7, order): row for row what the same engine gives with device_sort off, one stand-in call each.
    Returns the terms of the two calls."""
    eng.device_sort = False
    try:
        host = {k: _run(eng, query, tables, top=(k, order)).ordered_rows() for k in (abi.SORT_ALL, 7)}
    finally:
        eng.device_sort = True
    assert len(host[abi.SORT_ALL]) > 7 == len(host[7]) and not calls
    terms = []
    for k in (abi.SORT_ALL, 7):
        before = len(calls)
        got = _run(eng, query, tables, top=(k, order))
        assert got.ordered_rows() == host[k], k
        assert len(calls) == before + 1 and calls[-1][0] == k
        route = eng.stats()["order_routes"][-1]
        assert route["route"] == "sorted_by" and route["order"] == [nm for nm, _ in order]
        terms.append(calls[-1][1])
    assert terms[0] == terms[1]
    assert len(host[abi.SORT_ALL]) == len(_run(eng, query, tables).rows())
    return terms[0], len(host[abi.SORT_ALL])


def test_q16_orders_by_the_digits_of_its_mixed_radix_key(oracle_engine, db, stand_ins):
    sorted_by, ranks, plain = stand_ins
    order = Q.TPCH_ORDER["q16"][1]
    terms, n = _both_ways(oracle_engine, "q16", [db[t] for t in Q.QUERY_TABLES["q16"]], order, sorted_by)
    assert n > 1000 and not oracle_engine.stats()["host_loops"]
    assert len(terms) == 4 and len(terms[0]) == 4                                                   # supplier_cnt desc: a plain column
    assert terms[0][0] in (abi.SORT_HITS, abi.SORT_VALUE) and terms[0][2]
    brand, kind, size = terms[1:]
    for t in (brand, kind, size):
        assert len(t) == 8 and t[0] == abi.SORT_KEY and not t[2] and not t[3]
        assert t[7] is False                                     # p_brand / p_type are sorted dictionaries, p_size a number: no rank table
    # p_size: the lowest digit, the column's own range 1 .. 50; p_type above it, p_brand the open top digit
    assert size[4] <= 1 and size[5] == 50 and size[6] == 1
    assert kind[4] == 50 and kind[5] >= 2 and kind[6] == 0
    assert brand[4] == 50 * kind[5] and brand[5] == 0 and brand[6] == 0
    assert not ranks and not plain
    assert oracle_engine.stats()["order_routes"][-1]["ranked"] == []


def test_q2_orders_by_text_behind_row_references_and_a_packed_key(oracle_engine, db_q2, stand_ins):
    sorted_by, ranks, plain = stand_ins
    order = Q.TPCH_ORDER["q2"][1]
    tables = [db_q2[t] for t in Q.QUERY_TABLES["q2"]]
    terms, n = _both_ways(oracle_engine, "q2", tables, order, sorted_by)
    assert not oracle_engine.stats()["host_loops"], oracle_engine.stats()["host_loops"]        # the precondition of Q2_SCALE
    acctbal, n_name, s_name, partkey = terms
    assert acctbal[0] == abi.SORT_PAYLOAD and acctbal[2] and acctbal[3] and len(acctbal) == 4       # a copied double, descending
    assert n_name[0] == abi.SORT_PAYLOAD and n_name[4:] == (0, 0, 0, True)                          # row references into nation's 25 names: ranked
    # the generator's supplier names increase with the row: the reference IS the rank — a plain column, no rank table
    names = db_q2["supplier"].getContainer()["data"][db_q2["supplier"].getContainer()["headers"].index("s_name")]
    assert (names[1:] > names[:-1]).all()
    assert s_name[0] == abi.SORT_PAYLOAD and len(s_name) == 4 and not s_name[2] and not s_name[3]
    assert partkey[0] == abi.SORT_KEY and partkey[4:] == (1 << 32, 0, 0, False)                      # the first half of (p_partkey, s_suppkey)
    assert ranks == [(25, "<U25")]                                                                   # once, for both runs
    assert oracle_engine.stats()["order_routes"][-1]["ranked"] == ["n_name"]
    # another run ranks nothing again; after invalidate(table) it does
    assert _run(oracle_engine, "q2", tables, top=(7, order)).size() == 7 and len(ranks) == 1
    oracle_engine.invalidate(db_q2["nation"])
    assert _run(oracle_engine, "q2", tables, top=(7, order)).size() == 7 and len(ranks) == 2
    assert not plain


def test_text_payload_descending(oracle_engine, shuffled, stand_ins):
    sorted_by, ranks, plain = stand_ins
    (term,), n = _both_ways(oracle_engine, suppliers_by_name, [shuffled], BY_NAME_ORDER, sorted_by)
    assert n == len(shuffled.getContainer()["data"][0])
    assert term[0] == abi.SORT_PAYLOAD and term[2] and term[4:] == (0, 0, 0, True)
    assert len(ranks) == 1 and ranks[0][0] == n and not plain                      # ranked once for both runs
    assert oracle_engine.stats()["order_routes"][-1]["ranked"] == ["s_name"]
    oracle_engine.invalidate(shuffled)
    assert _run(oracle_engine, suppliers_by_name, [shuffled], top=(7, BY_NAME_ORDER)).size() == 7 and len(ranks) == 2


@pytest.mark.parametrize("order", [BY_PAIR_ORDER, BY_PAIR_ORDER_2])
def test_both_halves_of_a_packed_key(oracle_engine, suppliers, stand_ins, order):
    sorted_by, ranks, plain = stand_ins
    terms, n = _both_ways(oracle_engine, suppliers_by_pair, [suppliers], order, sorted_by)
    assert n == len(suppliers.getContainer()["data"][0])
    by_name = dict(zip([nm for nm, _ in order], terms))
    assert by_name["s_nationkey"][0] == abi.SORT_KEY and by_name["s_nationkey"][4:] == (1 << 32, 0, 0, False)
    assert by_name["s_suppkey"][0] == abi.SORT_KEY and by_name["s_suppkey"][4:] == (0, 1 << 32, 0, False)
    assert [t[2] for t in terms] == [d == "desc" for _, d in order]
    assert not ranks and not plain


@pytest.fixture(scope="module")
def many_suppliers():
    """15 000 suppliers: more names than a dictionary of codes takes (4096), so a text group key travels as a row reference."""
    return tpch.generate(1.5, tables=["supplier"], columns={"supplier": SUPPLIER_COLUMNS})["supplier"]


@pytest.mark.parametrize("order", BY_TEXT_KEY_ORDERS)
def test_text_group_key_with_repeated_values_is_merged_before_it_is_ordered(oracle_engine, many_suppliers, stand_ins, order):
    """Every name three times, 5 000 distinct: the entries (one per row) that hold equal names are merged on the host, so neither ORDER
    BY nor LIMIT may run on the device ahead of that — the rows are those of device_sort = False, one per name, and no device call is made."""
    sorted_by, ranks, plain = stand_ins
    table = shuffled_suppliers(many_suppliers)
    names = table.getContainer()["data"][table.getContainer()["headers"].index("s_name")]
    assert len(names) == 15000 and len(np.unique(names)) == 5000 > 4096
    oracle_engine.device_sort = False
    host = {k: _run(oracle_engine, balance_by_name, [table], top=(k, order)).ordered_rows() for k in (abi.SORT_ALL, 7)}
    oracle_engine.device_sort = True
    assert len(host[abi.SORT_ALL]) == 5000 and len({r[0] for r in host[abi.SORT_ALL]}) == 5000
    for k in (abi.SORT_ALL, 7):
        assert _run(oracle_engine, balance_by_name, [table], top=(k, order)).ordered_rows() == host[k]
        assert oracle_engine.stats()["order_routes"][-1]["route"] == "host"
    assert not sorted_by and not ranks and not plain and not oracle_engine.stats()["host_loops"]


@pytest.mark.parametrize("order", BY_TEXT_KEY_ORDERS)
def test_text_group_key_without_repeats_is_ranked(oracle_engine, many_suppliers, stand_ins, order):
    """The same query over names that come once each, in no order: the key's row reference is ordered through the ranks of s_name."""
    sorted_by, ranks, plain = stand_ins
    terms, n = _both_ways(oracle_engine, balance_by_name, [permuted_suppliers(many_suppliers)], order, sorted_by)
    assert n == 15000 and not oracle_engine.stats()["host_loops"]
    by_name = dict(zip([nm for nm, _ in order], terms))
    assert by_name["s_name"][0] == abi.SORT_KEY and by_name["s_name"][4:] == (0, 0, 0, True)
    assert ranks == [(15000, "<U25")] and not plain
    assert oracle_engine.stats()["order_routes"][-1]["ranked"] == ["s_name"]


@pytest.mark.parametrize("order", BY_TEXT_PART_ORDERS)
def test_packed_half_behind_a_part_decoder(oracle_engine, many_suppliers, stand_ins, order):
    """(s_name, s_nationkey) packed: the first half is ranked through its part decoder where names come once, needs no rank table where
    they increase with the row, and stays on the host where a name may come twice."""
    sorted_by, ranks, plain = stand_ins
    terms, n = _both_ways(oracle_engine, balance_by_name_and_nation, [permuted_suppliers(many_suppliers)], order, sorted_by)
    by_name = dict(zip([nm for nm, _ in order], terms))
    assert n == 15000 and by_name["s_name"][4:] == (1 << 32, 0, 0, True) and by_name["s_nationkey"][4:] == (0, 1 << 32, 0, False)
    assert ranks == [(15000, "<U25")]
    del sorted_by[:]
    terms, n = _both_ways(oracle_engine, balance_by_name_and_nation, [many_suppliers], order, sorted_by)
    by_name = dict(zip([nm for nm, _ in order], terms))
    assert n == 15000 and by_name["s_name"][4:] == (1 << 32, 0, 0, False) and len(ranks) == 1
    del sorted_by[:]
    table = shuffled_suppliers(many_suppliers)
    oracle_engine.device_sort = False
    host = _run(oracle_engine, balance_by_name_and_nation, [table], top=(7, order)).ordered_rows()
    oracle_engine.device_sort = True
    assert _run(oracle_engine, balance_by_name_and_nation, [table], top=(7, order)).ordered_rows() == host
    assert oracle_engine.stats()["order_routes"][-1]["route"] == "host" and not sorted_by and len(ranks) == 1 and not plain


def test_numeric_orders_stay_where_they_were(oracle_engine, db, stand_ins):
    """q3 / q18: no derived term — abi.Context.table_sorted as before, never table_sorted_by; device_sort off: neither."""
    sorted_by, ranks, plain = stand_ins
    for name in ("q3", "q18"):
        tables = [db[t] for t in Q.QUERY_TABLES[name]]
        order = Q.TPCH_ORDER[name][1]
        before = len(plain)
        _run(oracle_engine, name, tables, top=(abi.SORT_ALL, order))
        assert len(plain) == before + 1 and plain[-1][0] == abi.SORT_ALL and all(len(t) == 4 for t in plain[-1][1])
        assert oracle_engine.stats()["order_routes"][-1]["route"] == "sorted"
        _run(oracle_engine, name, tables, top=(10, order))
        assert len(plain) == before + 1 and oracle_engine.stats()["order_routes"][-1]["route"] == "topk"
    assert not sorted_by and not ranks
    oracle_engine.device_sort = False
    nplain = len(plain)
    _run(oracle_engine, "q16", [db[t] for t in Q.QUERY_TABLES["q16"]], top=(abi.SORT_ALL, Q.TPCH_ORDER["q16"][1]))
    _run(oracle_engine, "q3", [db[t] for t in Q.QUERY_TABLES["q3"]], top=(abi.SORT_ALL, Q.TPCH_ORDER["q3"][1]))
    assert not sorted_by and not ranks and len(plain) == nplain
    assert [r["route"] for r in oracle_engine.stats()["order_routes"]][-2:] == ["host", "host"]
