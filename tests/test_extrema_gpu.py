"""MIN / MAX aggregation on the MI355X (run with -m gpu): the extrema extension (include/sdqh_extrema.h) against numpy on every table
layout, key pattern, size at which the fold takes another path, and edge value; sdqh_column_extrema; and smin / smax through the
decorator, q2_min and q15_max included.

Expected values always come from numpy on the host: np.maximum.at over the slot encoding restated below (not imported from the
product), then decoded.  Extrema are compared bit for bit (view(np.int64)): min / max do not round, so there is no tolerance."""
import numpy as np
import pytest

import edge_cases as E
from sdqlpy_amd import abi, engine, sdql_lib, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import *      # noqa: F401,F403  (record, smin, smax, sdql_compile: the test's own queries)
from sdqlpy_amd.tpch import lineitem_type, supplier_type

pytestmark = pytest.mark.gpu

TOP = np.uint64(1) << np.uint64(63)
QNAN = np.uint64(0x7FF8000000000000)
DBL_MAX = np.finfo(np.float64).max
MIN, MAX = abi.EXT_MIN, abi.EXT_MAX


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


def expected(nentries, entry, values, op):
    """Per entry the extremum (float64, NaN where nothing was folded) of values[r] over the rows with entry[r] >= 0."""
    acc = np.zeros(nentries, np.uint64)
    hit = entry >= 0
    np.maximum.at(acc, entry[hit], encode(np.asarray(values, np.float64)[hit], op == MIN))
    return decode(acc, op == MIN)


def same_bits(a, b):
    return (np.ascontiguousarray(a, np.float64).view(np.int64) == np.ascontiguousarray(b, np.float64).view(np.int64)).all()


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
    S = ctx.extrema_geometry()
    return S, sorted({0, 1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, 70001})


NKEYS = 1000


def key_of(i):
    return np.asarray(i, np.int64) * 3 + 7


def _dense_table(ctx, nkeys=NKEYS):
    """nkeys entries keyed 7, 10, 13, ...: stage order = build-row order = entry number."""
    return ctx.hash_build_unique(nkeys, abi.make_filter(), [], ctx.upload(key_of(np.arange(nkeys))), [], accumulate=True)


def _read(ctx, t, min_hits=0):
    """(keys, values[4], hits) of the entries, sorted by key."""
    n = ctx.table_compact_count(t, min_hits)
    keys, _, values, hits = ctx.table_compact(t, min_hits, n + 8)
    order = np.argsort(keys, kind="stable")
    return keys[order], values[:, order], hits[order]


def _pattern(name, n, rng, nkeys=NKEYS, S=512):
    """Entry number per row (>= nkeys: a key the table does not hold)."""
    if name == "one key":
        return np.full(n, 17, np.int64)
    if name == "runs":
        # sorted runs of lengths 60, then 1, 63, 64, 65, 200 in turn: the runs start and end at every lane sooner or later, cross from
        # lane 63 of one wave to lane 0 of the next (a wave holds 128 rows: the run over rows 124 .. 187) and straddle the S seam (for
        # S = 512 the run over rows 454 .. 516)
        lens = [60]
        while sum(lens) < n:
            lens += [1, 63, 64, 65, 200]
        ent = np.repeat(np.arange(len(lens)) % nkeys, lens)[:n]
        if n > S:
            assert ent[S - 1] == ent[S] or S != 512
        return ent.astype(np.int64)
    if name == "permutation":
        return rng.permutation(np.arange(n) % nkeys).astype(np.int64)
    if name == "a third absent":
        return rng.integers(0, nkeys + nkeys // 2, n).astype(np.int64)
    raise KeyError(name)


def _values(n, rng, nan_share=0.05):
    v = (rng.integers(-10 ** 6, 10 ** 6, n) / 64.0).astype(np.float64)
    if n:
        v[rng.random(n) < nan_share] = np.nan
    return v


def test_geometry(hip_engine):
    S, sizes = _sizes(hip_engine.ctx)
    assert S >= 128 and S % 128 == 0 and 2 * S + 1 < 70001 and len(sizes) == 10


# 1. key patterns x sizes, min and max in two slots of one call, hits counted ------------------------------------------------------
@pytest.mark.parametrize("pattern", ["one key", "runs", "permutation", "a third absent"])
def test_fold_patterns_at_every_size(hip_engine, pattern):
    ctx = hip_engine.ctx
    S, sizes = _sizes(ctx)
    rng = np.random.default_rng(len(pattern))
    t = _dense_table(ctx)
    hits = np.zeros(NKEYS, np.int64)
    try:
        for n in sizes:
            ent = _pattern(pattern, n, rng, S=S)
            entry = np.where(ent < NKEYS, ent, -1)
            a, b = _values(n, rng), _values(n, rng, 0.0)
            kc, ac, bc = ctx.upload(key_of(ent)), ctx.upload(a), ctx.upload(b)
            ctx.table_extrema(t, kc, n, [(1, MIN, ac, True), (3, MAX, bc, True)], count_hits=True)
            keys, values, got_hits = _read(ctx, t)
            hits += np.bincount(entry[entry >= 0], minlength=NKEYS)
            assert (keys == key_of(np.arange(NKEYS))).all()
            assert same_bits(values[1], expected(NKEYS, entry, a, MIN)), (pattern, n, "min")
            assert same_bits(values[3], expected(NKEYS, entry, b, MAX)), (pattern, n, "max")
            assert (values[0] == 0.0).all() and (values[2] == 0.0).all(), (pattern, n, "slots not named")
            assert (got_hits == hits).all(), (pattern, n, "hits: matched rows only, NaN rows included")
        if pattern == "a third absent":
            assert hits.sum() < sum(sizes) * 0.75                               # (the absent keys were ignored, not counted)
    finally:
        t.free()


# 2. layouts -------------------------------------------------------------------------------------------------------------------------
def _mixed(n, rng, S):
    ent = np.concatenate([_pattern("runs", n // 2, rng, S=S), _pattern("a third absent", n - n // 2, rng)])
    return ent, np.where(ent < NKEYS, ent, -1)


def _layout_case(ctx, make_table, S, check_slot0=None):
    rng = np.random.default_rng(7)
    done = 0
    for n in (S + 1, 70001):
        t = make_table()
        try:
            before = _read(ctx, t)
            ent, entry = _mixed(n, rng, S)
            a, b = _values(n, rng), rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
            ctx.table_extrema(t, ctx.upload(key_of(ent)), n, [(2, MAX, ctx.upload(a), True), (1, MIN, ctx.upload(b), False)], count_hits=False)
            keys, values, hits = _read(ctx, t)
            assert (keys == before[0]).all() and (hits == before[2]).all(), "count_hits = 0 leaves hits alone"
            idx = (keys - 7) // 3
            assert same_bits(values[2], expected(NKEYS, entry, a, MAX)[idx]) and same_bits(values[1], expected(NKEYS, entry, b.astype(np.float64), MIN)[idx])
            assert same_bits(values[0], before[1][0]), "slot 0 was not named"
            done += 1
        finally:
            t.free()
    return done


def test_direct_layout(hip_engine):
    ctx = hip_engine.ctx
    assert _layout_case(ctx, lambda: _dense_table(ctx), _sizes(ctx)[0]) == 2


def test_open_addressing_layout(hip_engine):
    ctx = hip_engine.ctx
    S = _sizes(ctx)[0]
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: _layout_case(ctx, lambda: _dense_table(ctx), S)) == 2


def _summed_table(ctx, nsums, rng):
    """Entries with room for nsums doubles (sdqh_xbuild, 16 + n), slot 0 holding a real sum over three rows per key."""
    build = abi.Program()
    build.key = build.op(abi.X_COL, abi.T_I64, col=ctx.upload(key_of(rng.permutation(NKEYS))))
    t = ctx.xbuild(NKEYS, build, 7, int(key_of(NKEYS - 1)), accumulate=True, nsums=nsums)
    pk = key_of(rng.integers(0, NKEYS, 3 * NKEYS))
    add = abi.Program()
    look = add.op(abi.X_LOOKUP, abi.T_BOOL, a=add.op(abi.X_COL, abi.T_I64, col=ctx.upload(pk)), table=t)
    add.gates = [look]
    add.vals = [add.op(abi.X_COL, abi.T_F64, col=ctx.upload(rng.random(len(pk)) * 1000.0))]
    ctx.xprobe_aggregate(len(pk), add, look, t)
    return t


def test_entries_with_room_for_fewer_than_four_values(hip_engine):
    """acc_stride 3 (slot 0 a real sum that comes back bit-identical, extrema in slots 1 and 2, slot 3 does not exist) and the
    sdqh_groupby_key table, whose entries hold exactly their tuple's one value: slot 0 is the only slot there is."""
    ctx = hip_engine.ctx
    S = _sizes(ctx)[0]
    rng = np.random.default_rng(3)
    assert _layout_case(ctx, lambda: _summed_table(ctx, 3, rng), S) == 2
    t = _summed_table(ctx, 3, rng)
    try:
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_extrema_begin(t, [3], [MAX])
        assert e.value.code == abi.ERR_INVALID
    finally:
        t.free()
    n = 2 * S + 1
    ent = rng.permutation(np.arange(n) % NKEYS)
    v = rng.integers(1, 60, n).astype(np.float64)
    kc = ctx.upload(key_of(ent))
    t = ctx.groupby_key(n, abi.make_filter(), kc, abi.make_tuple(abi.TUPLE_A, [ctx.upload(v)]))
    try:
        keys, values, hits = _read(ctx, t)
        assert (keys == key_of(np.arange(NKEYS))).all() and (values[0] == np.bincount(ent, weights=v, minlength=NKEYS)).all()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_extrema_begin(t, [1], [MIN])
        assert e.value.code == abi.ERR_INVALID
        w = _values(n, rng)
        ctx.table_extrema(t, kc, n, [(0, MIN, ctx.upload(w), True)], count_hits=False)
        k2, v2, h2 = _read(ctx, t)
        assert (k2 == keys).all() and (h2 == hits).all() and same_bits(v2[0], expected(NKEYS, ent, w, MIN))
    finally:
        t.free()


def test_shared_groups(hip_engine):
    """After sdqh_table_share_groups the entries of a group fold into the first one's slots, exactly as sums do."""
    ctx = hip_engine.ctx
    S = _sizes(ctx)[0]
    rng = np.random.default_rng(21)
    groups, rows = 300, 1200
    keys = rng.permutation(rows).astype(np.int64) + 100
    group = np.concatenate([np.arange(groups), rng.integers(0, groups, rows - groups)]).astype(np.int64)[rng.permutation(rows)]
    t = ctx.hash_build_unique(rows, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(group)], accumulate=True)
    try:
        ctx.table_share_groups(t, [0], [0], [groups])
        n = 2 * S + 1
        at = np.sort(rng.integers(0, rows, n))                              # rows of one entry stand together; neighbours of one group do too, sometimes
        absent = rng.random(n) < 0.2
        pk = np.where(absent, np.int64(5), keys[at])
        entry = np.where(absent, -1, group[at])
        a, b = _values(n, rng), _values(n, rng)
        ctx.table_extrema(t, ctx.upload(pk), n, [(0, MIN, ctx.upload(a), True), (1, MAX, ctx.upload(b), True)], count_hits=True)
        cnt = ctx.table_compact_count(t, 1)
        _, payload, values, hits = ctx.table_compact(t, 1, cnt + 8)
        live = np.bincount(entry[entry >= 0], minlength=groups)
        assert cnt == (live > 0).sum() and sorted(payload[0].tolist()) == np.nonzero(live)[0].tolist()      # one row per group that received a row
        g = payload[0]
        assert same_bits(values[0], expected(groups, entry, a, MIN)[g]) and same_bits(values[1], expected(groups, entry, b, MAX)[g])
        assert (hits == live[g]).all()
    finally:
        t.free()


# 3. edge values -----------------------------------------------------------------------------------------------------------------------
def test_edge_values(hip_engine):
    ctx = hip_engine.ctx
    nan = np.nan
    cases = {                                                        # entry -> its rows' values, in row order
        0: [np.inf, -np.inf, 1.0], 1: [DBL_MAX, -DBL_MAX], 2: [5e-324, -5e-324, 2.2250738585072009e-308], 3: [0.0, -0.0], 4: [-0.0, 0.0],
        5: [nan, 3.5, nan, -2.25, nan], 6: [nan, nan], 7: [], 8: [-0.0], 9: [np.inf], 10: [-np.inf, nan], 11: [0.0, 0.0], 12: [-5e-324, -0.0],
    }
    ent = np.array([k for k, vs in cases.items() for _ in vs], np.int64)
    v = np.array([x for vs in cases.values() for x in vs], np.float64)
    t = _dense_table(ctx, 16)
    try:
        kc, vc = ctx.upload(key_of(ent)), ctx.upload(v)
        ctx.table_extrema(t, kc, len(ent), [(0, MIN, vc, True), (1, MAX, vc, True)], count_hits=True)
        keys, values, hits = _read(ctx, t)
        assert same_bits(values[0], expected(16, ent, v, MIN)) and same_bits(values[1], expected(16, ent, v, MAX))
        lo, hi = values[0], values[1]
        assert lo[0] == -np.inf and hi[0] == np.inf and lo[1] == -DBL_MAX and hi[1] == DBL_MAX and lo[2] == -5e-324 and hi[2] == 2.2250738585072009e-308
        for k in (3, 4):                                             # +-0.0 on one key, both row orders
            assert lo[k] == 0.0 and np.signbit(lo[k]) and hi[k] == 0.0 and not np.signbit(hi[k])
        assert lo[5] == -2.25 and hi[5] == 3.5 and hits[5] == 5     # NaN among numbers: skipped, but the rows count
        assert np.isnan(lo[6]) and np.isnan(hi[6]) and hits[6] == 2 and np.isnan(lo[7]) and np.isnan(hi[7]) and hits[7] == 0
        assert values[0].view(np.uint64)[6] == QNAN and values[1].view(np.uint64)[7] == QNAN
        assert np.signbit(lo[8]) and np.signbit(hi[8]) and lo[10] == -np.inf == hi[10] and np.signbit(lo[12]) and lo[12] == -5e-324 and np.signbit(hi[12]) and hi[12] == 0.0
        # the same values as raw bits in an I64-typed column (what sdqh_xcompact returns)
        ctx.table_extrema(t, kc, len(ent), [(2, MIN, ctx.upload(v.view(np.int64)), True), (3, MAX, ctx.upload(v.view(np.int64)), True)])
        again = _read(ctx, t)[1]
        assert same_bits(again[2], values[0]) and same_bits(again[3], values[1]) and same_bits(again[0], values[0])
    finally:
        t.free()


def test_integer_values(hip_engine):
    ctx = hip_engine.ctx
    big = 1 << 53
    ent = np.array([0, 0, 0, 1, 1, 2, 3, 3], np.int64)
    v = np.array([-5, 0, 7, big, -big, 0, big - 1, -(big - 1)], np.int64)
    t = _dense_table(ctx, 8)
    try:
        kc = ctx.upload(key_of(ent))
        ctx.table_extrema(t, kc, len(ent), [(0, MIN, ctx.upload(v), False), (1, MAX, ctx.upload(v), False)])
        _, values, _ = _read(ctx, t)
        assert values[0][:4].tolist() == [-5.0, -float(big), 0.0, -float(big - 1)] and values[1][:4].tolist() == [7.0, float(big), 0.0, float(big - 1)]
        assert not np.signbit(values[0][2]) and np.isnan(values[0][4:]).all()
        # beyond 2^53 an integer is not a double exactly: refused when the slots are read, never rounded silently
        for bad in (big + 1, -(big + 1)):
            ctx.table_extrema_begin(t, [0], [MAX])
            ctx.table_extrema_fold(t, kc, len(ent), [(0, ctx.upload(np.where(ent == 1, bad, v)), False)])
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_extrema_end(t)
            assert e.value.code == abi.ERR_UNSUPPORTED
        # a value beyond 2^53 on a key the table does not hold is no value of the fold
        ctx.table_extrema_begin(t, [0], [MAX])
        ctx.table_extrema_fold(t, ctx.upload(np.where(ent == 1, 5, key_of(ent))), len(ent), [(0, ctx.upload(np.where(ent == 1, big + 1, v)), False)])
        ctx.table_extrema_end(t)
        assert _read(ctx, t)[1][0][:4].tolist()[0] == 7.0 and np.isnan(_read(ctx, t)[1][0][1])
    finally:
        t.free()


# 4. several folds ---------------------------------------------------------------------------------------------------------------------
def test_several_folds_equal_one(hip_engine):
    ctx = hip_engine.ctx
    S = _sizes(ctx)[0]
    rng = np.random.default_rng(11)
    n = 3 * S + 77
    ent, entry = _mixed(n, rng, S)
    a, b = _values(n, rng), _values(n, rng)
    cut = S + 13
    results = []
    for parts in ([slice(0, n)], [slice(0, cut), slice(cut, n)], [slice(cut, n), slice(0, 0), slice(0, cut)], "shuffled"):
        t = _dense_table(ctx)
        try:
            ctx.table_extrema_begin(t, [0, 2], [MIN, MAX])
            if parts == "shuffled":
                p = rng.permutation(n)
                ctx.table_extrema_fold(t, ctx.upload(key_of(ent[p])), n, [(2, ctx.upload(b[p]), True), (0, ctx.upload(a[p]), True)], count_hits=True)
            else:
                for s in parts:
                    m = len(ent[s])
                    ctx.table_extrema_fold(t, ctx.upload(key_of(ent[s])), m, [(0, ctx.upload(a[s]), True), (2, ctx.upload(b[s]), True)], count_hits=True)
            ctx.table_extrema_end(t)
            results.append(_read(ctx, t))
        finally:
            t.free()
    want = (expected(NKEYS, entry, a, MIN), expected(NKEYS, entry, b, MAX), np.bincount(entry[entry >= 0], minlength=NKEYS))
    for keys, values, hits in results:
        assert same_bits(values[0], want[0]) and same_bits(values[2], want[1]) and (hits == want[2]).all()


# 5. argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(hip_engine):
    ctx = hip_engine.ctx
    k = ctx.upload(key_of(np.arange(50)))
    v = ctx.upload(np.arange(50, dtype=np.float64))
    text = ctx.upload(np.array(["ab"] * 50))
    plain = ctx.hash_build_unique(50, abi.make_filter(), [], k, [], accumulate=False)
    member = ctx.build_key_set(50, abi.make_filter(), [], k)
    t = _dense_table(ctx, 50)

    def ok():
        ctx.table_extrema(t, k, 50, [(0, MAX, v, True)])
        assert _read(ctx, t)[1][0].tolist() == list(range(50))

    def refused(code, call):
        with pytest.raises(abi.SdqhError) as e:
            call()
        assert e.value.code == code, str(e.value)
        ok()                                                          # the next valid call passes
    try:
        ok()
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_begin(plain, [0], [MIN]))                 # no accumulators
        refused(abi.ERR_UNSUPPORTED, lambda: ctx.table_extrema_begin(member, [0], [MIN]))            # membership only
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_begin(t, [4], [MIN]))                     # slot >= acc_stride
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_begin(t, [-1], [MIN]))
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_begin(t, [1, 1], [MIN, MAX]))             # a slot named twice
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_begin(t, [1], [2]))                       # no such operation
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_begin(t, [], []))
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_fold(t, k, 50, [(0, v, True)]))           # fold without begin (the last one has ended)
        refused(abi.ERR_INVALID, lambda: ctx.table_extrema_end(t))                                   # end without begin
        ctx.table_extrema_begin(t, [1], [MIN])
        for bad in (lambda: ctx.table_extrema_fold(t, k, 50, [(2, v, True)]),                        # a slot begin did not name
                    lambda: ctx.table_extrema_fold(t, k, 50, [(1, v, True), (1, v, True)]),
                    lambda: ctx.table_extrema_fold(t, k, 51, [(1, v, True)]),                        # columns shorter than nrows
                    lambda: ctx.table_extrema_fold(t, v, 50, [(1, v, True)]),                        # the key is not an I64 column
                    lambda: ctx.table_extrema_fold(t, k, 50, [(1, text, True)]),
                    lambda: ctx.table_extrema_fold(t, k, -1, [(1, v, True)])):
            with pytest.raises(abi.SdqhError) as e:
                bad()
            assert e.value.code == abi.ERR_INVALID, str(e.value)
        ctx.table_extrema_fold(t, k, 50, [(1, v, True)])                                             # ... and the open fold goes on
        ctx.table_extrema_fold(t, k, 0, [(1, v, True)])                                              # no rows: nothing launched
        ctx.table_extrema_end(t)
        assert _read(ctx, t)[1][1].tolist() == list(range(50))
        refused(abi.ERR_INVALID, lambda: ctx.column_extrema(text, 50))
        refused(abi.ERR_INVALID, lambda: ctx.column_extrema(v, 51))
    finally:
        for x in (plain, member, t):
            x.free()


# 6. sdqh_column_extrema ---------------------------------------------------------------------------------------------------------------
def _column_expect(v):
    num = v[~np.isnan(v)]
    if not len(num):
        return QNAN, QNAN, 0
    return decode(np.array([encode(num, True).max()]), True).view(np.uint64)[0], decode(np.array([encode(num, False).max()]), False).view(np.uint64)[0], len(num)


def _column_got(ctx, col, n, **kw):
    lo, hi, cnt = ctx.column_extrema(col, n, **kw)
    return np.array([lo]).view(np.uint64)[0], np.array([hi]).view(np.uint64)[0], cnt


def test_column_extrema(hip_engine):
    ctx = hip_engine.ctx
    S, sizes = _sizes(ctx)
    rng = np.random.default_rng(2)
    for n in sizes:
        v = _values(n, rng)
        assert _column_got(ctx, ctx.upload(v) if n else ctx.upload(np.zeros(1)), n) == _column_expect(v), n
        i = rng.integers(-(1 << 53), (1 << 53) + 1, n).astype(np.int64)
        assert _column_got(ctx, ctx.upload(i) if n else ctx.upload(np.zeros(1, np.int64)), n) == _column_expect(i.astype(np.float64)), n
        if n:
            assert _column_got(ctx, ctx.upload(v.view(np.int64)), n, is_f64=True) == _column_expect(v), n      # raw bits in an I64-typed column
    edge = np.array([np.inf, -np.inf, DBL_MAX, -DBL_MAX, 5e-324, -5e-324, 0.0, -0.0, np.nan, 1.0], np.float64)
    for pick in ([0, 1, 8], [2, 3], [4, 5, 6], [6, 7], [7, 6], [7], [8, 9, 8], [5, 7], [2, 0]):
        v = edge[pick]
        assert _column_got(ctx, ctx.upload(v), len(v)) == _column_expect(v), pick
    lo, hi, cnt = ctx.column_extrema(ctx.upload(edge[[6, 7]]), 2)
    assert np.signbit(lo) and not np.signbit(hi) and cnt == 2
    for v in (np.full(S + 3, np.nan), np.zeros(0)):
        lo, hi, cnt = ctx.column_extrema(ctx.upload(v if len(v) else np.zeros(1)), len(v))
        assert np.isnan(lo) and np.isnan(hi) and cnt == 0
    assert ctx.column_extrema(ctx.upload(np.array([1 << 53, -(1 << 53), 0], np.int64)), 3) == (-float(1 << 53), float(1 << 53), 3)
    with pytest.raises(abi.SdqhError) as e:
        ctx.column_extrema(ctx.upload(np.array([0, (1 << 53) + 1], np.int64)), 2)
    assert e.value.code == abi.ERR_UNSUPPORTED
    assert ctx.column_extrema(ctx.upload(np.array([3, -4], np.int64)), 2) == (-4.0, 3.0, 2)          # ... and the context goes on


# 7. through the decorator -------------------------------------------------------------------------------------------------------------
@sdql_compile({"lineitem": lineitem_type})
def per_order(lineitem):
    out = lineitem.sum(lambda l: {l[0].l_orderkey: record({"first": smin(l[0].l_shipdate), "dearest": smax(l[0].l_extendedprice), "qty": l[0].l_quantity})})
    return out


@sdql_compile({"lineitem": lineitem_type})
def per_order_late(lineitem):
    out = lineitem.sum(lambda l: {l[0].l_orderkey: record({"first": smin(l[0].l_shipdate), "dearest": smax(l[0].l_extendedprice), "qty": l[0].l_quantity})}
                       if l[0].l_shipdate >= 19950617 else None)
    return out


@sdql_compile({"lineitem": lineitem_type})
def dearest_early(lineitem):
    out = lineitem.sum(lambda l: smax(l[0].l_extendedprice) if l[0].l_shipdate < 19930101 else None)
    return out


@sdql_compile({"lineitem": lineitem_type})
def latest_of_none(lineitem):
    out = lineitem.sum(lambda l: smax(l[0].l_shipdate) if l[0].l_shipdate < 19000101 else None)
    return out


@pytest.fixture(scope="module", params=[0.01, 0.05])
def db(request):
    qs = ["q2_min", "q15_max", "q1", "q3"]
    return tpch.generate(request.param, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))


@pytest.fixture()
def decorated(hip_engine):
    engine.use_engine(hip_engine)
    hip_engine.extrema_loops.clear()
    yield hip_engine
    engine._engine = None
    sdql_lib._state.update(mode=None)


def _routes(eng):
    return {(r["result"], r["route"], r["runs"]) for r in eng.stats()["extrema_loops"]}


def _per_order_expect(li, mask):
    ok = li["l_orderkey"][mask]
    keys, entry = np.unique(ok, return_inverse=True)
    first = expected(len(keys), entry, li["l_shipdate"][mask].astype(np.float64), MIN)
    dearest = expected(len(keys), entry, li["l_extendedprice"][mask], MAX)
    qty = np.bincount(entry, weights=li["l_quantity"][mask], minlength=len(keys))
    return keys, first.astype(np.int64), dearest, qty


def _columns(table, names):
    return {n: tpch.column(table, n) for n in names}


@pytest.mark.parametrize("query,route", [(per_order, "columns"), (per_order_late, "compacted")])
def test_per_key_through_the_decorator(decorated, db, query, route):
    li = _columns(db["lineitem"], ["l_orderkey", "l_shipdate", "l_extendedprice", "l_quantity"])
    mask = np.ones(len(li["l_orderkey"]), bool) if route == "columns" else li["l_shipdate"] >= 19950617
    keys, first, dearest, qty = _per_order_expect(li, mask)
    for run in (1, 2, 3):                                            # the prepared plan again: settled plans take other host paths
        res = query(db["lineitem"])
        got = dict(res.key_fields)["l_orderkey"]
        vals = dict(res.val_fields)
        order = np.argsort(got, kind="stable")
        assert (got[order] == keys).all() and len(got) == len(keys)
        assert vals["first"].dtype == np.int64 and (vals["first"][order] == first).all()
        assert vals["dearest"].dtype == np.float64 and same_bits(vals["dearest"][order], dearest)
        assert (vals["qty"][order] == qty).all()                    # (quantities are whole numbers: their sums are exact in any order)
        assert _routes(decorated) == {("out", route, run)}


def test_scalar_through_the_decorator(decorated, db):
    li = _columns(db["lineitem"], ["l_shipdate", "l_extendedprice"])
    want = li["l_extendedprice"][li["l_shipdate"] < 19930101].max()
    for run in (1, 2, 3):
        got = dearest_early(db["lineitem"])
        assert isinstance(got, float) and got == want
        assert _routes(decorated) == {("out", "compacted", run)}
    assert np.isnan(latest_of_none(db["lineitem"]))                 # no row passes: nothing to fold


def test_q2_min(decorated, db):
    """Against TPC-H Q2's minimum restated in numpy: per size-15 brass part the cheapest European offer, every supplier that makes it."""
    t = {n: db[n] for n in ("region", "nation", "supplier", "part", "partsupp")}
    c = lambda tab, name: tpch.column(t[tab], name)      # noqa: E731
    europe = c("region", "r_regionkey")[c("region", "r_name") == "EUROPE"]
    nat = np.isin(c("nation", "n_regionkey"), europe)
    nation_name = dict(zip(c("nation", "n_nationkey")[nat].tolist(), c("nation", "n_name")[nat].tolist()))
    sup = np.isin(c("supplier", "s_nationkey"), list(nation_name))
    sup_row = {k: i for i, k in zip(np.nonzero(sup)[0].tolist(), c("supplier", "s_suppkey")[sup].tolist())}
    brass = (c("part", "p_size") == 15) & np.char.endswith(c("part", "p_type"), "BRASS")
    mfgr = dict(zip(c("part", "p_partkey")[brass].tolist(), c("part", "p_mfgr")[brass].tolist()))
    pk, sk, cost = c("partsupp", "ps_partkey"), c("partsupp", "ps_suppkey"), c("partsupp", "ps_supplycost")
    m = np.isin(pk, list(mfgr)) & np.isin(sk, list(sup_row))
    parts, entry = np.unique(pk[m], return_inverse=True)
    cheapest = expected(len(parts), entry, cost[m], MIN)
    best = m.copy()
    best[m] = cost[m] == cheapest[entry]
    want = []
    for p, s in zip(pk[best].tolist(), sk[best].tolist()):
        i = sup_row[s]
        want.append((float(c("supplier", "s_acctbal")[i]), str(c("supplier", "s_name")[i]), nation_name[int(c("supplier", "s_nationkey")[i])], p, mfgr[p],
                     str(c("supplier", "s_address")[i]), str(c("supplier", "s_phone")[i]), str(c("supplier", "s_comment")[i])))
    assert len(want) >= 1
    for run in (1, 2, 3):
        res = Q.run("q2_min", db)
        assert res.columns == ["s_acctbal", "s_name", "n_name", "p_partkey", "p_mfgr", "s_address", "s_phone", "s_comment"]
        assert sorted(tuple(r) for r in res.rows()) == sorted(want)
        assert _routes(decorated) == {("european_cost", "compacted", run)}
    # where a part has several European offers the minimum differs from q2's total: q2_min keeps rows q2 cannot
    assert len(want) >= len(Q.run("q2", db).rows())


def test_q15_max(decorated, db):
    top = Q.run("q15", db, (1, [("total_revenue", "desc")])).ordered_rows()[0]
    li = _columns(db["lineitem"], ["l_suppkey", "l_shipdate", "l_extendedprice", "l_discount"])
    m = (li["l_shipdate"] >= 19960101) & (li["l_shipdate"] < 19960401)
    sup, entry = np.unique(li["l_suppkey"][m], return_inverse=True)
    rev = np.bincount(entry, weights=li["l_extendedprice"][m] * (1.0 - li["l_discount"][m]), minlength=len(sup))
    ties = sup[rev == rev.max()].tolist()
    for run in (1, 2, 3):
        res = Q.run("q15_max", db)
        rows = res.rows()
        assert res.columns == ["s_suppkey", "s_name", "s_address", "s_phone", "total_revenue"]
        assert sorted(r[0] for r in rows) == ties and top[0] in ties
        for r in rows:                                               # (a sum: equal to q15's within the rounding of another order of addition)
            assert abs(r[4] - top[4]) <= 1e-10 * top[4] and r[1:4] == top[1:4]
        assert _routes(decorated) == {("best", "compacted", run)}


def test_q15_max_keeps_every_tied_supplier(decorated):
    """Two suppliers with the same two rows (a + b is b + a bit for bit) and one behind them: top(1) would keep one, q15_max keeps both."""
    from sdqlpy_amd.sdql_lib import table_from_columns
    lineitem = table_from_columns(["l_suppkey", "l_shipdate", "l_extendedprice", "l_discount"],
                                  [np.array([3, 1, 2, 1, 3, 2, 2], np.int64), np.full(7, 19960215, np.int64),
                                   np.array([100.5, 100.5, 7.0, 50.25, 50.25, 8.0, 9.0]), np.array([0.1, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0])])
    supplier = table_from_columns(["s_suppkey", "s_name", "s_address", "s_phone"],
                                  [np.array([1, 2, 3], np.int64), np.array(["one", "two", "three"]), np.array(["a", "b", "c"]), np.array(["11", "22", "33"])])
    rows = Q.q15_max(lineitem, supplier).rows()
    assert sorted(r[0] for r in rows) == [1, 3] and rows[0][4] == rows[1][4] and abs(rows[0][4] - (100.5 * 0.9 + 50.25)) < 1e-9
    assert len(Q.q15.top(1, [("total_revenue", "desc")])(lineitem, supplier).ordered_rows()) == 1


def test_per_key_over_a_result_dictionary(decorated, db):
    """{K: record(smin, smax, count)} over the entries of an aggregated dictionary: per supplier the smallest and largest order total."""
    @sdql_compile({"lineitem": lineitem_type})
    def spread(lineitem):
        per_pair = lineitem.sum(lambda l: {record({"o": l[0].l_orderkey, "s": l[0].l_suppkey}): l[0].l_quantity})
        out = per_pair.sum(lambda g: {g[0].s: record({"least": smin(g[1]), "most": smax(g[1]), "orders": 1})} if g[1] > 2.0 else None)
        return out
    li = _columns(db["lineitem"], ["l_orderkey", "l_suppkey", "l_quantity"])
    pair, entry = np.unique(li["l_orderkey"] * (1 << 32) + li["l_suppkey"], return_inverse=True)
    total = np.bincount(entry, weights=li["l_quantity"], minlength=len(pair))
    keep = total > 2.0
    sup, e2 = np.unique(pair[keep] & 0xFFFFFFFF, return_inverse=True)
    res = spread(db["lineitem"])
    assert len(res.key_fields) == 1
    got = res.key_fields[0][1]
    order = np.argsort(got, kind="stable")
    vals = dict(res.val_fields)
    assert (got[order] == sup).all()
    assert same_bits(vals["least"][order], expected(len(sup), e2, total[keep], MIN)) and same_bits(vals["most"][order], expected(len(sup), e2, total[keep], MAX))
    assert (vals["orders"][order] == np.bincount(e2, minlength=len(sup))).all()
    assert _routes(decorated) == {("out", "compacted", 1)}
