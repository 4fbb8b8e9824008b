"""ORDER BY over derived columns on the MI355X (run with -m gpu): sdqh_text_ranks against numpy.unique and sdqh_table_sorted_by
(include/sdqh_sort_terms.h) against a stable numpy lexsort of the derived columns, at every size at which the sort takes another path,
on every table layout; the contract of both calls; and q16 / q2 / q2_min and two purpose-made queries through the engine.  Every
comparison is exact: order columns are integers, text and copied doubles, sums are of integer-valued doubles.

The expected rows are the table's own K-F rows (stage order = build-row order) reordered by numpy; the order-preserving map and the
derivation field = (uint64(source) / div) % mod + add are restated here, not imported from the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import edge_cases as E
from order_terms_queries import (BY_NAME_ORDER, BY_PAIR_ORDER, BY_PAIR_ORDER_2, BY_TEXT_KEY_ORDERS, BY_TEXT_PART_ORDERS, SUPPLIER_COLUMNS, balance_by_name,
                                 balance_by_name_and_nation, permuted_suppliers, shuffled_suppliers, suppliers_by_name, suppliers_by_pair)
from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q

pytestmark = pytest.mark.gpu

Q2_SCALE = 0.8      # the smallest tenth at which q2's last loop runs on the device (tests/test_order_terms_cpu.py asserts it)


@pytest.fixture(scope="module")
def hip_engine(hip_lib):
    eng = engine.Engine(hip_lib.context(device=0))
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


def _sizes(ctx):
    S, T, L = ctx.sort_geometry()
    return sorted({0, 1, 2, 63, 64, 65, T - 1, T, T + 1, S - 1, S, S + 1, 4 * T - 1, 4 * T, 4 * T + 1, 8 * T + 1, 20011})


# 3. text_ranks ----------------------------------------------------------------------------------------------------------------------------
def _text(units, width):
    """n x width code units -> '<U width' array (built from the units themselves: no Python str in between)."""
    units = np.ascontiguousarray(units, np.uint32).reshape(-1, width)
    return units.view("<U%d" % width).reshape(len(units))


def _digits(values, width, ndigits):
    """Decimal digits of `values` in the last min(width, ndigits) units behind a constant prefix ("Supplier#000012345")."""
    n = len(values)
    units = np.zeros((n, width), np.uint32)
    prefix = np.frombuffer("Supplier#".encode("utf-32-le"), np.uint32)
    nd = min(width, ndigits)
    head = min(len(prefix), width - nd)
    units[:, :head] = prefix[:head]
    rest = np.asarray(values, np.int64).copy()
    for p in range(head + nd - 1, head - 1, -1):
        units[:, p] = ord("0") + rest % 10
        rest //= 10
    return units


def _contents(n, width, rng):
    """name -> '<U width' array of n rows, for every kind of content the ranking has to get right."""
    out = {}
    base = rng.integers(ord("a"), ord("z") + 1, width).astype(np.uint32)
    out["all equal"] = _text(np.tile(base, (n, 1)), width)
    ident = np.arange(n, dtype=np.int64)
    if width == 1:
        distinct = (1 + ident + (ident >= 0xD7FF) * 0x800).astype(np.uint32).reshape(n, 1)      # n distinct code points, no surrogates
    else:
        distinct = _digits(rng.permutation(n), width, 9)
    out["all distinct"] = _text(distinct, width)
    few = rng.integers(ord("A"), ord("Z") + 1, (10, width)).astype(np.uint32)
    out["ten values"] = _text(few[rng.integers(0, 10, n)], width)
    last = np.tile(base, (n, 1)); last[:, width - 1] = rng.integers(1, 200, n)
    out["last unit only"] = _text(last, width)
    first = np.tile(base, (n, 1)); first[:, 0] = rng.integers(1, 200, n)
    out["first unit only"] = _text(first, width)
    prefixes = np.tile(base, (n, 1))
    prefixes[np.arange(width)[None, :] >= rng.integers(0, width + 1, n)[:, None]] = 0              # "", "a", "ab", ... of one text
    out["prefixes and the empty text"] = _text(prefixes, width)
    out["Supplier#%09d"] = _text(_digits(rng.integers(0, max(2, 3 * n), n), width, 9), width)
    high = np.where(rng.integers(0, 2, (n, width)) == 1, rng.integers(0x100, 0x300, (n, width)), rng.integers(0x10000, 0x110000, (n, width)))
    out["above 255 and above 0xFFFF"] = _text(high, width)
    out["sorted"] = np.sort(out["Supplier#%09d"])
    out["reverse sorted"] = np.ascontiguousarray(np.sort(out["above 255 and above 0xFFFF"])[::-1])
    return out


@pytest.mark.parametrize("width", [1, 10, 25])
def test_text_ranks_against_numpy_unique(hip_engine, width):
    """Every size x every kind of content: the ranks are np.unique's inverse, the distinct count its length, and a second call gives
    the same bits."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(100 + width)
    done = 0
    for n in _sizes(ctx):
        for what, col in _contents(n, width, rng).items():
            assert col.dtype == np.dtype("<U%d" % width) and len(col) == n
            uniq, want = np.unique(col, return_inverse=True)
            dev = ctx.upload(col)
            ranks, distinct = ctx.text_ranks(dev, n)
            got = ranks.download()
            assert got.dtype == np.int64 and len(got) == n, (what, n)
            assert distinct == len(uniq), (what, n, distinct, len(uniq))
            assert (got == want.reshape(n)).all(), (what, n)
            if n in (65, 20011):
                again, d2 = ctx.text_ranks(dev, n)
                assert d2 == distinct and (again.download() == got).all(), (what, n)
                again.free()
            ranks.free(); dev.free()
            done += 1
    assert done == 17 * 10


# 4. table_sorted_by -----------------------------------------------------------------------------------------------------------------------
def _sort_bits(a, is_f64, desc):
    """int64 x -> x ^ 2^63; float64 bits u -> ~u if the sign bit is set else u | 2^63; descending: the complement."""
    u = np.ascontiguousarray(a).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    u = np.where(u >> np.uint64(63) != 0, ~u, u | top) if is_f64 else u ^ top
    return ~u if desc else u


def _stage_rows(ctx, t, min_hits):
    cnt = ctx.table_compact_count(t, min_hits)
    return ctx.table_compact(t, min_hits, cnt, want_values=t.accumulate, want_hits=t.accumulate)


def _expected_order(rows, terms, rank_tables):
    """Stable lexsort over the derived columns.  rank_tables: id(ranks Column) -> its host array."""
    keys, payload, values, hits = rows
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
                v = rank_tables[id(ranks)][v]
            lex.append(_sort_bits(v, False, desc))
        else:
            lex.append(_sort_bits(src, kind == abi.SORT_VALUE or (kind == abi.SORT_PAYLOAD and is_f64), desc))
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


RADIX = (5, 7)              # payload 0 = (d2 * 7 + d1) * 5 + d0 with d0 < 5, d1 < 7 and an open top digit d2
MAP_ROWS = 37               # payload 1 = a reference into a table of 37 rows


def _derived_table(ctx, n, seed=3, accumulate=True):
    """n entries keyed by the packed pair (a << 32) | b — a of 40 values (heavy ties), no pair twice; up to 100 keys come twice in the
    build (the first row owns the entry) — with a mixed-radix integer and a reference into a MAP_ROWS-row table as payload, probed by
    three rows per build row with integer-valued doubles."""
    rng = np.random.default_rng(seed + n)
    a = rng.integers(0, 40, n).astype(np.int64)
    b = rng.permutation(max(n, 1))[:n].astype(np.int64) * 3 + 1
    distinct = (a << 32) | b
    d = min(100, n // 2)
    keys = np.concatenate([distinct[:n // 2], distinct[:d], distinct[n // 2:]])
    rows = len(keys)
    radix = ((rng.integers(0, 30, rows) * RADIX[1] + rng.integers(0, RADIX[1], rows)) * RADIX[0] + rng.integers(0, RADIX[0], rows)).astype(np.int64)
    ref = rng.integers(0, MAP_ROWS, rows).astype(np.int64)
    t = ctx.hash_build_unique(rows, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(radix), ctx.upload(ref)], accumulate=accumulate)
    if rows and accumulate:
        pk = keys[rng.integers(0, rows, 3 * rows)]
        ctx.hash_probe_aggregate(3 * rows, abi.make_filter(), t, ctx.upload(pk), abi.make_tuple(abi.TUPLE_A, [ctx.upload(rng.integers(1, 1000, 3 * rows).astype(np.float64))]))
    assert ctx.table_compact_count(t, 0) == n
    return t


@pytest.fixture(scope="module")
def rank_columns(hip_engine):
    """Two rank tables of MAP_ROWS rows: a non-injective map (10 values: ties fall through) and text_ranks' own output over a text
    column of few values.  -> (map Column, text ranks Column, {id(Column): host array})"""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(77)
    m = rng.integers(-5, 5, MAP_ROWS).astype(np.int64)
    cm = ctx.upload(m)
    text = _text(rng.integers(ord("a"), ord("e"), (MAP_ROWS, 3)), 3)
    ct, distinct = ctx.text_ranks(ctx.upload(text), MAP_ROWS)
    want = np.unique(text, return_inverse=True)[1].reshape(MAP_ROWS).astype(np.int64)
    assert 1 < distinct < MAP_ROWS and (ct.download() == want).all()
    yield cm, ct, {id(cm): m, id(ct): want}
    cm.free(); ct.free()


def _term_lists(cm, ct, accumulate=True):
    K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
    r0, r1 = RADIX
    lists = [
        [(K, 0, True, False, 1 << 32, 0, 0, None), (K, 0, False, False, 0, 1 << 32, 0, None)],                      # both halves of the packed key
        [(K, 0, False, False, 0, 1 << 32, 0, None), (K, 0, True, False, 1 << 32, 0, 0, None)],
        [(P, 0, False, False, r0, r1, 100, None), (P, 0, True, False, r0 * r1, 0, -3, None), (P, 0, True, False, 1, r0, 0, None)],   # digits, add != 0, open top digit
        [(P, 1, False, False, 0, 0, 0, cm), (P, 0, True, False, r0, r1, 0, None)],                                  # a non-injective rank table: ties -> next term -> stage order
        [(P, 1, True, False, 0, 0, 0, cm)],
        [(P, 1, True, False, 0, 0, 0, ct), (K, 0, False, False, 1 << 32, 0, 0, None)],                              # text_ranks' own output
        [(K, 0, False, False, 1 << 32, 0, 0, None), (P, 1, False, False, 0, 0, 0, ct), (P, 0, True, False, 0, r0, 0, None), (K, 0, True, False, 0, 1 << 32, 0, None),
         (P, 0, False, False), (K, 0, False, False), (P, 1, True, False, 0, 0, 5, None), (P, 1, False, False, 0, 0, 0, cm)],      # derived and plain mixed, 8 terms
    ]
    if accumulate:
        lists.append([(V, 0, True, True), (H, 0, True, False, 0, 3, 0, None), (P, 1, False, False, 0, 0, 0, cm), (H, 0, False, False), (K, 0, True, False, 1 << 32, 0, 0, None)])
    return lists


def _check(ctx, t, lists, tables, what, min_hits_set=(0, 2)):
    done = 0
    for min_hits in (min_hits_set if t.accumulate else (0,)):
        rows = _stage_rows(ctx, t, min_hits)
        n = len(rows[0])
        for terms in lists:
            order = _expected_order(rows, terms, tables)
            for limit in sorted({1, 129, abi.SORT_ALL}):
                got = ctx.table_sorted_by(t, min_hits, limit, terms, 64, want_hits=t.accumulate)
                _same(got, rows, order[:min(limit, n)], (what, min_hits, limit, [tm[:7] for tm in terms]))
                done += 1
    return done


@pytest.mark.parametrize("which", range(15))
def test_sorted_by_against_numpy(hip_engine, rank_columns, which):
    """The which-th size of test 3's set from 2 up."""
    ctx = hip_engine.ctx
    cm, ct, tables = rank_columns
    sizes = [n for n in _sizes(ctx) if n >= 2]
    assert len(sizes) == 15                                              # (a geometry in which sizes of the set coincide needs this list looked at again)
    n = sizes[which]
    t = _derived_table(ctx, n)
    try:
        assert _check(ctx, t, _term_lists(cm, ct), tables, "n=%d" % n) == 8 * 2 * 3
    finally:
        t.free()


LAYOUT_SIZES = {"below a tile": lambda S, T: 65, "a tile": lambda S, T: T, "the single-workgroup limit": lambda S, T: S,
                "the first radix size": lambda S, T: S + 1, "several tiles": lambda S, T: 2 * T + 1, "a tile boundary": lambda S, T: 4 * T}


@pytest.mark.parametrize("size", sorted(LAYOUT_SIZES))
def test_sorted_by_on_the_other_layouts(hip_engine, rank_columns, size):
    """A build without accumulators, the open-addressing layout, a groupby-key table and shared groups: on the single-workgroup path,
    at its limit, just beyond it, at tile boundaries and over several tiles."""
    ctx = hip_engine.ctx
    cm, ct, tables = rank_columns
    S, T, L = ctx.sort_geometry()
    n = LAYOUT_SIZES[size](S, T)
    t = _derived_table(ctx, n, accumulate=False)
    try:
        assert _check(ctx, t, _term_lists(cm, ct, False), tables, "no accumulators") == 7 * 3
    finally:
        t.free()

    def hashed():
        t = _derived_table(ctx, n)
        try:
            return _check(ctx, t, _term_lists(cm, ct), tables, "hash layout")
        finally:
            t.free()
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, hashed) == 8 * 2 * 3
    # groupby-key: the key is the only integer column — its digits and a gather through a table as wide as its range
    rng = np.random.default_rng(4)
    groups = rng.permutation(n).astype(np.int64)
    keys = np.concatenate([groups, groups[rng.integers(0, n, 4 * n)]])[rng.permutation(5 * n)]
    t = ctx.groupby_key(len(keys), abi.make_filter(), ctx.upload(keys), abi.make_tuple(abi.TUPLE_A, [ctx.upload(rng.integers(1, 60, len(keys)).astype(np.float64))]))
    wide = rng.integers(0, 12, n).astype(np.int64)
    cw = ctx.upload(wide)
    try:
        assert ctx.table_compact_count(t, 1) == n
        K, V, H = abi.SORT_KEY, abi.SORT_VALUE, abi.SORT_HITS
        lists = [[(K, 0, False, False, 0, 0, 0, cw), (V, 0, True, True)], [(K, 0, True, False, 0, 16, 0, None), (H, 0, False, False, 0, 2, 0, None), (K, 0, False, False, 16, 0, 0, None)]]
        for min_hits in (1, 2, 5):
            assert _check(ctx, t, lists, {id(cw): wide}, "groupby_key", (min_hits,)) == 6
    finally:
        t.free(); cw.free()
    # shared groups, min_hits = 1: one row per group
    rows = 4 * n
    keys = rng.permutation(rows).astype(np.int64) + 100
    pa = np.concatenate([np.arange(n), rng.integers(0, n, rows - n)]).astype(np.int64)[rng.permutation(rows)]
    pb = (pa % MAP_ROWS).astype(np.int64)
    t = ctx.hash_build_unique(rows, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(pa), ctx.upload(pb)], accumulate=True)
    try:
        ctx.table_share_groups(t, [0], [0], [n])
        pk = np.concatenate([keys, keys[rng.integers(0, rows, 2 * rows)]])
        ctx.hash_probe_aggregate(len(pk), abi.make_filter(), t, ctx.upload(pk), abi.make_tuple(abi.TUPLE_A, [ctx.upload(rng.integers(1, 50, len(pk)).astype(np.float64))]))
        assert ctx.table_compact_count(t, 1) == n
        P = abi.SORT_PAYLOAD
        lists = [[(P, 1, False, False, 0, 0, 0, cm), (P, 0, True, False, 0, 11, 0, None)], [(P, 1, True, False, 0, 0, 0, ct), (abi.SORT_VALUE, 0, True, True)]]
        assert _check(ctx, t, lists, tables, "shared groups", (1,)) == 6
    finally:
        t.free()


PLAIN_SPECS = [
    [(abi.SORT_VALUE, 0, True, True), (abi.SORT_PAYLOAD, 0, False, False)],
    [(abi.SORT_PAYLOAD, 1, True, False)],
    [(abi.SORT_HITS, 0, True, False), (abi.SORT_KEY, 0, True, False)],
    [(abi.SORT_KEY, 0, False, False)],
]


def test_underived_terms_give_what_table_sorted_gives(hip_engine):
    ctx = hip_engine.ctx
    S, T, L = ctx.sort_geometry()
    for n in (S - 1, 5 * T + 17):
        t = _derived_table(ctx, n)
        try:
            for spec in PLAIN_SPECS:
                for min_hits in (0, 2):
                    for limit in (1, 129, abi.SORT_ALL):
                        a = ctx.table_sorted(t, min_hits, limit, spec, 64)
                        for terms in (spec, [s + (0, 0, 0, None) for s in spec], [s + (1, 0, 0, None) for s in spec]):
                            b = ctx.table_sorted_by(t, min_hits, limit, terms, 64)
                            assert len(a[0]) == len(b[0]) and (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[3] == b[3]).all(), (n, spec, min_hits, limit)
                            assert (a[2].view(np.int64) == b[2].view(np.int64)).all(), (n, spec, min_hits, limit)
        finally:
            t.free()


# 5. the contract --------------------------------------------------------------------------------------------------------------------------
_raw_terms = abi._marshal_sort_terms


def test_contract_of_sorted_by(hip_engine, rank_columns):
    ctx = hip_engine.ctx
    cm, ct, tables = rank_columns
    n = 3 * ctx.sort_geometry()[1] - 1
    t = _derived_table(ctx, n)
    short = ctx.upload(np.arange(MAP_ROWS - 1, dtype=np.int64))          # one row too few for payload 1's references
    try:
        cap = 100
        keys = np.full(cap, -7, np.int64)
        pay = np.full((2, cap), -7, np.int64)
        got = C.c_int64(-7)

        def call(terms, limit, capacity, out, out_pay=None):
            arr = _raw_terms(terms)
            return ctx.lib.sdqh_table_sorted_by(ctx.handle, t.handle, C.c_int64(0), C.c_int64(limit), C.c_int(len(terms)), arr, C.c_int64(capacity),
                                                out, out_pay, None, None, C.byref(got))
        kp = keys.ctypes.data_as(C.c_void_p)
        # a field beyond the ranks column: refused, naming the term, before anything is written
        bad = [(abi.SORT_KEY, 0, False, False, 1 << 32, 0, 0, None), (abi.SORT_PAYLOAD, 1, False, False, 0, 0, 0, short)]
        assert call(bad, cap, cap, kp, pay.ctypes.data_as(C.c_void_p)) == abi.ERR_INVALID
        assert got.value == -7 and (keys == -7).all() and (pay == -7).all()
        assert "term 1" in ctx.lib.sdqh_last_error(ctx.handle).decode()
        for shifted in ([(abi.SORT_PAYLOAD, 1, False, False, 0, 0, 1, cm)], [(abi.SORT_PAYLOAD, 1, False, False, 0, 0, -1, cm)]):     # one past the end / one before the start
            assert call(shifted, cap, cap, kp) == abi.ERR_INVALID and got.value == -7 and (keys == -7).all()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_sorted_by(t, 0, 10, bad, 10)
        assert e.value.code == abi.ERR_INVALID
        # a derivation on a double
        for terms in ([(abi.SORT_VALUE, 0, False, True, 0, 5, 0, None)], [(abi.SORT_PAYLOAD, 1, False, True, 2, 0, 0, None)], [(abi.SORT_VALUE, 0, False, False, 0, 0, 0, cm)]):
            assert call(terms, cap, cap, kp) == abi.ERR_INVALID and (keys == -7).all()
        assert call([(abi.SORT_KEY, 0, False, False, -2, 0, 0, None)], cap, cap, kp) == abi.ERR_INVALID
        assert call([(abi.SORT_PAYLOAD, 2, False, False, 0, 2, 0, None)], cap, cap, kp) == abi.ERR_INVALID       # a field the table lacks
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_sorted_by(t, 0, 10, [(abi.SORT_KEY, 0, False, False, 0, 2, 0, None)] * (abi.SORT_MAX_KEYS + 1), 10)
        assert e.value.code == abi.ERR_INVALID
        # overflow and the count-only call, as sdqh_table_sorted
        terms = [(abi.SORT_PAYLOAD, 1, True, False, 0, 0, 0, cm), (abi.SORT_KEY, 0, False, False, 0, 1 << 32, 0, None)]
        assert call(terms, abi.SORT_ALL, cap, kp) == abi.ERR_OVERFLOW and got.value == n and (keys == -7).all()
        assert call(terms, cap + 1, cap, kp) == abi.ERR_OVERFLOW and got.value == cap + 1 and (keys == -7).all()
        assert call(terms, abi.SORT_ALL, 0, None) == abi.OK and got.value == n
        assert call(terms, 50, 0, None) == abi.OK and got.value == 50
        assert call(terms, 0, cap, kp) == abi.ERR_INVALID
        assert call(terms, cap, cap, kp) == abi.OK and got.value == cap and (keys != -7).all()
        rows = _stage_rows(ctx, t, 0)
        order = _expected_order(rows, terms, tables)
        assert (keys == rows[0][order[:cap]]).all()
        _same(ctx.table_sorted_by(t, 0, abi.SORT_ALL, terms, 10), rows, order, "retry with the exact capacity")
    finally:
        t.free(); short.free()


def test_contract_of_text_ranks(hip_engine):
    ctx = hip_engine.ctx
    wide = ctx.upload(np.array(["x" * (abi.TEXT_RANK_MAX_WIDTH + 1), "y"], "<U%d" % (abi.TEXT_RANK_MAX_WIDTH + 1)))
    widest = ctx.upload(np.array(["x" * abi.TEXT_RANK_MAX_WIDTH, "x" * (abi.TEXT_RANK_MAX_WIDTH - 1) + "w", "x"], "<U%d" % abi.TEXT_RANK_MAX_WIDTH))
    ints = ctx.upload(np.arange(4, dtype=np.int64))
    try:
        with pytest.raises(abi.SdqhError) as e:
            ctx.text_ranks(wide, 2)
        assert e.value.code == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.SdqhError) as e:
            ctx.text_ranks(ints, 4)
        assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.SdqhError) as e:
            ctx.text_ranks(widest, 4)                                      # more rows than the column has
        assert e.value.code == abi.ERR_INVALID
        ranks, distinct = ctx.text_ranks(widest, 3)                        # the widest column taken: the last unit decides
        assert distinct == 3 and ranks.download().tolist() == [2, 1, 0]
        ranks.free()
        empty, distinct = ctx.text_ranks(widest, 0)
        assert distinct == 0 and empty.nrows == 0
        empty.free()
    finally:
        wide.free(); widest.free(); ints.free()


# 6. through the engine --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dbs():
    q2 = tpch.columns_for(["q2"])
    q16 = tpch.columns_for(["q16", "q3"])
    suppliers = tpch.generate(0.05, tables=["supplier"], columns={"supplier": SUPPLIER_COLUMNS})["supplier"]
    many = tpch.generate(1.5, tables=["supplier"], columns={"supplier": SUPPLIER_COLUMNS})["supplier"]       # 15 000 names: beyond a dictionary of codes
    return {"q2": tpch.generate(Q2_SCALE, tables=sorted(q2), columns=q2), "q16": tpch.generate(0.2, tables=sorted(q16), columns=q16),
            "suppliers": suppliers, "shuffled": shuffled_suppliers(suppliers), "permuted": permuted_suppliers(many), "repeated": shuffled_suppliers(many)}


def _run(eng, query, tables, top=None):
    return engine.execute_plan(eng, frontend.lower_function(query), tables, top=top)


CASES = {
    "q16": (lambda: Q.q16, lambda d: [d["q16"][t] for t in Q.QUERY_TABLES["q16"]], Q.TPCH_ORDER["q16"][1], []),
    "q2": (lambda: Q.q2, lambda d: [d["q2"][t] for t in Q.QUERY_TABLES["q2"]], Q.TPCH_ORDER["q2"][1], ["n_name"]),
    "q2_min": (lambda: Q.q2_min, lambda d: [d["q2"][t] for t in Q.QUERY_TABLES["q2_min"]], Q.TPCH_ORDER["q2_min"][1], ["n_name"]),
    "by name": (lambda: suppliers_by_name, lambda d: [d["shuffled"]], BY_NAME_ORDER, ["s_name"]),
    "by pair": (lambda: suppliers_by_pair, lambda d: [d["suppliers"]], BY_PAIR_ORDER, []),
    "by pair, the other way": (lambda: suppliers_by_pair, lambda d: [d["suppliers"]], BY_PAIR_ORDER_2, []),
    "text key": (lambda: balance_by_name, lambda d: [d["permuted"]], BY_TEXT_KEY_ORDERS[0], ["s_name"]),
    "text key behind a value": (lambda: balance_by_name, lambda d: [d["permuted"]], BY_TEXT_KEY_ORDERS[1], ["s_name"]),
    "text half of a packed key": (lambda: balance_by_name_and_nation, lambda d: [d["permuted"]], BY_TEXT_PART_ORDERS[0], ["s_name"]),
    "text half of a packed key, second": (lambda: balance_by_name_and_nation, lambda d: [d["permuted"]], BY_TEXT_PART_ORDERS[1], ["s_name"]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_through_the_engine(hip_engine, dbs, name):
    """order_by, top(100) and top(5): row for row what the same engine gives with device_sort off, and ordered by sorted_by."""
    query, tables, order, ranked = CASES[name]
    query, tables = query(), tables(dbs)
    hip_engine.device_sort = False
    try:
        host = {k: _run(hip_engine, query, tables, top=(k, order)).ordered_rows() for k in (abi.SORT_ALL, 100, 5)}
        assert hip_engine.stats()["order_routes"][-1]["route"] == "host"
    finally:
        hip_engine.device_sort = True
    n = len(host[abi.SORT_ALL])
    assert n > 100 and not hip_engine.stats()["host_loops"]
    if name == "q16":
        assert n > hip_engine.ctx.sort_geometry()[0]                     # beyond the single-workgroup path
    for k in (abi.SORT_ALL, 100, 5):
        got = _run(hip_engine, query, tables, top=(k, order)).ordered_rows()
        route = hip_engine.stats()["order_routes"][-1]
        assert route["route"] == "sorted_by" and route["ranked"] == ranked, route
        assert got == host[k], (name, k)


@pytest.mark.parametrize("query,orders", [(balance_by_name, BY_TEXT_KEY_ORDERS), (balance_by_name_and_nation, BY_TEXT_PART_ORDERS)])
def test_text_keys_that_may_repeat_stay_on_the_host(hip_engine, dbs, query, orders):
    """Row references into a column in which a name comes three times: entries that hold equal text are merged on the host when the
    result is read, so ORDER BY / LIMIT is not applied ahead of that on the device — the rows are those of device_sort = False."""
    tables = [dbs["repeated"]]
    for order in orders:
        for k in (abi.SORT_ALL, 100, 5):
            hip_engine.device_sort = False
            try:
                host = _run(hip_engine, query, tables, top=(k, order)).ordered_rows()
            finally:
                hip_engine.device_sort = True
            got = _run(hip_engine, query, tables, top=(k, order)).ordered_rows()
            assert hip_engine.stats()["order_routes"][-1]["route"] == "host"
            assert got == host and len(got) == min(k, 5000 if query is balance_by_name else 15000), (order, k)


def test_numeric_order_still_reports_sorted(hip_engine, dbs):
    order = Q.TPCH_ORDER["q3"][1]
    tables = [dbs["q16"][t] for t in Q.QUERY_TABLES["q3"]]
    assert _run(hip_engine, Q.q3, tables, top=(abi.SORT_ALL, order)).size() > 129
    assert hip_engine.stats()["order_routes"][-1]["route"] == "sorted"
    _run(hip_engine, Q.q3, tables, top=(10, order))
    assert hip_engine.stats()["order_routes"][-1]["route"] == "topk"
