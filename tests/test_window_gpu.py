"""Ranks inside partitions on the MI355X (run with -m gpu): sdqh_table_window (include/sdqh_sort_window.h) against numpy at every size
at which the sort or the tile scan takes another path, on partition patterns that exercise the carry between tiles, on every table
layout, over derived terms, on edge values, against sdqh_table_sorted_by where both apply, its contract, and through the engine and
the decorator.  Comparisons are exact: the tables aggregate integer-valued doubles, and ranks are integers.

The expected rows are always the table's own K-F rows (sdqh_table_compact: stage order = build-row order) reordered by a STABLE numpy
lexsort over the documented order-preserving map, restated here; the ranks are computed with plain numpy on the sorted images (and,
for small n, once more by walking the sorted rows in Python).  Nothing is imported from the product's ranking code."""
import ctypes as C
import os

import numpy as np
import pytest

import edge_cases as E
from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
KINDS = (abi.WIN_ROW_NUMBER, abi.WIN_RANK, abi.WIN_DENSE_RANK)
TERMS = [(P, 0, False, False), (V, 0, True, True), (H, 0, False, False)]          # PARTITION BY payload 0 ORDER BY value desc, hits asc


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


def _sort_bits(a, is_f64, desc):
    """int64 x -> x ^ 2^63; float64 bits u -> ~u if the sign bit is set else u | 2^63; descending: the complement."""
    u = np.ascontiguousarray(a).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    u = np.where(u >> np.uint64(63) != 0, ~u, u | top) if is_f64 else u ^ top
    return ~u if desc else u


def _stage_rows(ctx, t, min_hits):
    cnt = ctx.table_compact_count(t, min_hits)
    return ctx.table_compact(t, min_hits, cnt, want_values=t.accumulate, want_hits=t.accumulate)


def _images(rows, terms, rank_tables=None):
    """The ordered 64-bit image of every term, in term order.  rank_tables: id(ranks Column) -> its host array."""
    keys, payload, values, hits = rows
    col = {K: lambda i: keys, P: lambda i: payload[i], V: lambda i: values[i], H: lambda i: hits}
    out = []
    for t in terms:
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
            out.append(_sort_bits(v, False, desc))
        else:
            out.append(_sort_bits(src, kind == V or (kind == P and is_f64), desc))
    return out


class Ranked:
    """The rows of a table in the order of `terms` and all three ranks of every sorted position, by numpy."""

    def __init__(self, rows, terms, npart, rank_tables=None):
        imgs = _images(rows, terms, rank_tables)
        n = len(rows[0])
        self.n, self.order = n, (np.lexsort(imgs[::-1]) if n else np.zeros(0, np.int64))      # stable; the last array is the primary column
        self.part_head, self.tie_head = np.zeros(n, bool), np.zeros(n, bool)
        if n:
            self.part_head[0] = self.tie_head[0] = True
        for i, u in enumerate(imgs):
            s = u[self.order]
            self.tie_head[1:] |= s[1:] != s[:-1]
            if i < npart:
                self.part_head[1:] |= s[1:] != s[:-1]
        pos = np.arange(n, dtype=np.int64)
        start = np.maximum.accumulate(np.where(self.part_head, pos, 0)) if n else pos
        tie = np.maximum.accumulate(np.where(self.tie_head, pos, 0)) if n else pos
        seen = np.cumsum(self.tie_head)
        self.ranks = {abi.WIN_ROW_NUMBER: pos - start + 1, abi.WIN_RANK: tie - start + 1, abi.WIN_DENSE_RANK: (seen - seen[start] + 1) if n else pos}
        if 0 < n <= 300:                                                   # the same once more, walking the sorted rows
            rn = rk = dr = 0
            for i in range(n):
                if self.part_head[i]:
                    rn, rk, dr = 1, 1, 1
                else:
                    rn += 1
                    if self.tie_head[i]:
                        rk, dr = rn, dr + 1
                assert (self.ranks[0][i], self.ranks[1][i], self.ranks[2][i]) == (rn, rk, dr)

    def kept(self, kind, per_limit):
        return np.nonzero(self.ranks[kind] <= per_limit)[0]


def _same(got, rows, idx, what):
    gk, gp, gv, gh = got[:4]
    keys, payload, values, hits = rows
    assert len(gk) == len(idx), (what, len(gk), len(idx))
    assert (gk == keys[idx]).all(), what
    if payload is not None:
        for p in range(len(payload)):
            assert (gp[p] == payload[p][idx]).all(), (what, "payload", p)
    if values is not None:
        assert (gv[0].view(np.int64) == values[0][idx].view(np.int64)).all(), (what, "value")
    if hits is not None and gh is not None:
        assert (gh == hits[idx]).all(), (what, "hits")


def _check(ctx, t, terms, npart, what, min_hits=1, rank_tables=None, per_limits=(1, 2, 7, ALL), kinds=KINDS):
    """kinds x per_limit x limit in {1, kept // 2, ALL}: rows and ranks against numpy; the count-only call."""
    rows = _stage_rows(ctx, t, min_hits)
    ref = Ranked(rows, terms, npart, rank_tables)
    done = 0
    for kind in kinds:
        for per_limit in per_limits:
            sel = ref.kept(kind, per_limit)
            for limit in sorted({1, max(1, len(sel) // 2), ALL}):
                got = ctx.table_window(t, min_hits, npart, terms, kind, per_limit, limit, 64, want_hits=t.accumulate)
                want = sel[:limit]
                _same(got, rows, ref.order[want], (what, kind, per_limit, limit))
                assert got[4].dtype == np.int64 and (got[4] == ref.ranks[kind][want]).all(), (what, kind, per_limit, limit, "ranks")
                done += 1
            assert _count_only(ctx, t, min_hits, npart, terms, kind, per_limit, ALL) == (abi.OK, len(sel)), (what, kind, per_limit, "count")
    return done, ref


_raw_terms = abi._marshal_sort_terms


def _raw(ctx, t, min_hits, npart, terms, kind, per_limit, limit, capacity, keys=None, rank=None, got=None, nterms=None):
    got = got if got is not None else C.c_int64(-7)
    rc = ctx.lib.sdqh_table_window(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms), _raw_terms(terms),
                                   C.c_int(kind), C.c_int64(per_limit), C.c_int64(limit), C.c_int64(capacity),
                                   None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                   None if rank is None else rank.ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value


def _count_only(ctx, t, min_hits, npart, terms, kind, per_limit, limit):
    return _raw(ctx, t, min_hits, npart, terms, kind, per_limit, limit, 0)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def _table(ctx, part, value, hits, dups=0, seed=1):
    """n = len(part) entries with payload 0 = part, value 0 = value (integer-valued) and hits as given (0: never probed); `dups` of the
    keys come a second time in the middle of the build, with another payload — the first row owns the entry."""
    n = len(part)
    rng = np.random.default_rng(seed + n)
    distinct = rng.permutation(max(n, 1))[:n].astype(np.int64) * 5 + 3
    d = min(dups, n // 2)
    keys = np.concatenate([distinct[:n // 2], distinct[:d], distinct[n // 2:]])
    pay = np.concatenate([part[:n // 2], np.full(d, -99, np.int64), part[n // 2:]]).astype(np.int64)
    t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(pay)], accumulate=True)
    if n:
        hits = np.asarray(hits, np.int64)
        pk = np.repeat(distinct, hits)
        first = np.concatenate([[0], np.cumsum(hits)[:-1]])[hits > 0]
        pv = np.ones(len(pk), np.float64)
        pv[first] = (np.asarray(value, np.float64) - (hits - 1))[hits > 0]
        if len(pk):
            ctx.hash_probe_aggregate(len(pk), abi.make_filter(), t, ctx.upload(pk), abi.make_tuple(abi.TUPLE_A, [ctx.upload(pv)]))
    assert ctx.table_compact_count(t, 0) == n
    return t


def _runs(n, lengths):
    part = np.zeros(n, np.int64)
    at = g = 0
    while at < n:
        part[at:at + lengths[g % len(lengths)]] = g
        at += lengths[g % len(lengths)]
        g += 1
    return part


def _pattern(name, n, T, rng):
    """-> (partition ids, values, hits), rows in random build order."""
    value = rng.integers(-50, 50, n).astype(np.float64)
    hits = rng.integers(1, 4, n)
    if name == "one partition":
        part = np.zeros(n, np.int64)
    elif name == "every row its own":
        part = rng.permutation(n).astype(np.int64)
    elif name == "runs":
        part = _runs(n, [60, 1, 63, 64, 65, 200])
    elif name == "a long partition":                                       # 3T + 5 rows that all tie — no head of either kind for whole tiles — then short ones
        part = np.concatenate([np.zeros(min(n, 3 * T + 5), np.int64), 1 + _runs(max(0, n - 3 * T - 5), [3, 1, 5, 2])])
        value[part == 0], hits[part == 0] = 7.0, 2
    else:                                                                  # heavy ties: five order values
        part = rng.integers(0, n // 300 + 2, n).astype(np.int64)
        value, hits = rng.choice(np.array([-3.0, 0.0, 1.0, 2.0, 1e6]), n), np.ones(n, np.int64)
    mix = rng.permutation(n)
    return part[mix], value[mix], hits[mix]


PATTERNS = ["one partition", "every row its own", "runs", "a long partition", "heavy ties"]


def _sizes(ctx):
    T = ctx.window_geometry()
    S, tile, _ = ctx.sort_geometry()
    return T, S, sorted({0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, S - 1, S, S + 1, tile - 1, tile, tile + 1, 70001})


def test_geometry(hip_engine):
    T, S, sizes = _sizes(hip_engine.ctx)
    assert T >= 64 and 3 * T + 5 + T < 70001 and len(sizes) >= 12


# 1. partition patterns x sizes x kinds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    for n in sizes:
        t = _table(ctx, *_pattern(pattern, n, T, rng))
        try:
            done, ref = _check(ctx, t, TERMS, 1, (pattern, n))
            assert done >= 3 * 4 * 1 and ref.n == n
            if pattern == "a long partition" and n == 70001:              # the carry path: a tile wholly inside a partition, with no head in it
                tiles = ref.tie_head[:(n // T) * T].reshape(-1, T)
                assert (~tiles.any(axis=1)).any()
            if pattern == "one partition" and n == 70001:                 # ... and tiles with tie heads but no partition head
                assert ref.part_head.sum() == 1 and ref.tie_head[T:2 * T].any()
            if n:                                                          # a capacity one too small: the needed count, nothing written
                kept = len(ref.kept(abi.WIN_RANK, 2))
                keys, rank = np.full(n, -7, np.int64), np.full(n, -7, np.int64)
                assert _raw(ctx, t, 1, 1, TERMS, abi.WIN_RANK, 2, ALL, kept - 1, keys, rank) == (abi.ERR_OVERFLOW, kept)
                assert (keys == -7).all() and (rank == -7).all()
                assert _raw(ctx, t, 1, 1, TERMS, abi.WIN_ROW_NUMBER, ALL, ALL, n - 1, keys, rank) == (abi.ERR_OVERFLOW, n) and (keys == -7).all()
        finally:
            t.free()


# 2. layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True])
def test_layouts(hip_engine, big):
    """The direct layout, the open-addressing layout, a table with duplicate build keys (owner rows only), a row-program build, each
    with min_hits in {0, 1, 2}."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 70001 if big else T + 1
    rng = np.random.default_rng(n)
    part, value, _ = _pattern("runs", n, T, rng)
    hits = rng.integers(0, 4, n)                                           # some entries never probed: min_hits selects

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        try:
            return sum(_check(ctx, t, TERMS, 1, ("layout", dups, mh), min_hits=mh, per_limits=(1, 7, ALL))[0] for mh in (0, 1, 2))
        finally:
            t.free()
    assert run(0) >= 3 * 3 * 3 * 2
    assert run(200) >= 3 * 3 * 3 * 2
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) >= 3 * 3 * 3 * 2
    # a row-program build (sdqh_xbuild): the key is its only integer column — partition by key % 7, order by the sum and the hits
    keys = rng.permutation(n).astype(np.int64) * 3 + 7
    build = abi.Program()
    build.key = build.op(abi.X_COL, abi.T_I64, col=ctx.upload(keys))
    t = ctx.xbuild(n, build, 7, int(keys.max()), accumulate=True, nsums=1)
    try:
        pk = keys[rng.integers(0, n, 2 * n)]
        add = abi.Program()
        look = add.op(abi.X_LOOKUP, abi.T_BOOL, a=add.op(abi.X_COL, abi.T_I64, col=ctx.upload(pk)), table=t)
        add.gates = [look]
        add.vals = [add.op(abi.X_COL, abi.T_F64, col=ctx.upload(rng.integers(0, 3, len(pk)).astype(np.float64)))]
        ctx.xprobe_aggregate(len(pk), add, look, t)
        terms = [(K, 0, True, False, 0, 7, 0, None), (V, 0, False, True), (H, 0, True, False)]
        for mh in (0, 1, 2):
            assert _check(ctx, t, terms, 1, ("xbuild", mh), min_hits=mh, per_limits=(2, ALL))[0] >= 3 * 2 * 2
    finally:
        t.free()


# 3. derived terms -----------------------------------------------------------------------------------------------------------------------
def test_derived_terms(hip_engine):
    """PARTITION BY the high half of a packed key ORDER BY its low half descending, then a text-ranked payload; a ranks column too short
    is SDQH_ERR_INVALID with nothing written, *out_n included."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    assert (ct.download() == want).all()
    short = ctx.upload(want[:20])
    try:
        for n in (T + 1, S + 1, 5 * T + 17):
            a = rng.integers(0, n // 90 + 2, n).astype(np.int64)
            b = rng.integers(0, 3000, n).astype(np.int64)                  # ordered in steps of 16: the text decides inside a step, then stage order
            keys = np.unique((a << 32) | b)
            keys = keys[rng.permutation(len(keys))]
            ref_col = rng.integers(0, len(text), len(keys)).astype(np.int64)
            t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ref_col)], accumulate=False)
            try:
                terms = [(K, 0, False, False, 1 << 32, 0, 0, None), (K, 0, True, False, 16, 1 << 28, 0, None), (P, 0, False, False, 0, 0, 0, ct)]
                assert _check(ctx, t, terms, 1, ("derived", n), min_hits=0, rank_tables={id(ct): want})[0] >= 3 * 4 * 2
                bad = terms[:2] + [(P, 0, False, False, 0, 0, 0, short)]
                out = np.full(len(keys), -7, np.int64)
                assert _raw(ctx, t, 0, 1, bad, abi.WIN_RANK, 2, ALL, len(keys), out, out.copy()) == (abi.ERR_INVALID, -7) and (out == -7).all()
                assert b"term 2" in ctx.lib.sdqh_last_error(ctx.handle)
            finally:
                t.free()
    finally:
        ct.free(); short.free()


# 4. edge values -------------------------------------------------------------------------------------------------------------------------
I_MIN, I_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NAN_A = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]
NAN_B = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
EDGE_DOUBLES = np.array([0.0, -0.0, np.inf, -np.inf, NAN_A, NAN_B, np.finfo(np.float64).max, 1.0, -0.0, NAN_B, 0.0, NAN_A, np.inf], np.float64)
EDGE_INTS = np.array([0, I_MAX, -1, I_MIN, 1, I_MIN, I_MAX, 0, I_MIN + 1, I_MAX - 1, 1 << 32], np.int64)


@pytest.mark.parametrize("n", [300, 2600])
def test_edge_values(hip_engine, n):
    """+-0.0 (two values), +-inf, two NaN bit patterns (equal only bit for bit), DBL_MAX, INT64_MIN / MAX: each as a partition term
    and as an order term, every kind."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) * 3 - n
    ints = np.resize(EDGE_INTS, n)[rng.permutation(n)]
    dbls = np.resize(EDGE_DOUBLES, n)[rng.permutation(n)]
    t = ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ints), ctx.upload(dbls.view(np.int64))], accumulate=False)
    try:
        done = 0
        for terms, npart in (([(P, 1, False, True), (P, 0, True, False)], 1), ([(P, 0, False, False), (P, 1, True, True)], 1),
                             ([(P, 1, True, True), (P, 0, False, False)], 2), ([(P, 1, False, True)], 0), ([(P, 0, True, False)], 0)):
            d, ref = _check(ctx, t, terms, npart, ("edge", terms, npart), min_hits=0, per_limits=(1, 2, ALL))
            done += d
            if terms[0][1] == 1 and npart >= 1:                            # eight different doubles under the total order: -0.0 != +0.0, two NaNs
                assert ref.part_head.sum() == 8 if npart == 1 else ref.part_head.sum() > 8
        assert done >= 5 * 3 * 3 * 2
    finally:
        t.free()


# 5. agreement -----------------------------------------------------------------------------------------------------------------------------
def _probed_table(ctx, n, seed=9):
    """The table of test_order_by_gpu: duplicates in the build, an integer payload of 50 values, a double payload, three probes per row."""
    rng = np.random.default_rng(seed + n)
    distinct = rng.permutation(max(n, 1))[:n].astype(np.int64) * 5 + 3
    d = min(200, n // 2)
    keys = np.concatenate([distinct[:n // 2], distinct[:d], distinct[n // 2:]])
    rows = len(keys)
    pay_i = rng.integers(0, 50, rows).astype(np.int64)
    pay_f = (rng.integers(-500, 500, rows) / 4.0 + 0.0).astype(np.float64)
    pk = keys[rng.integers(0, rows, 3 * rows)]
    pv = rng.integers(1, 1000, 3 * rows).astype(np.float64)
    t = ctx.hash_build_unique(rows, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(pay_i), ctx.upload(pay_f.view(np.int64))], accumulate=True)
    if rows:
        ctx.hash_probe_aggregate(3 * rows, abi.make_filter(), t, ctx.upload(pk), abi.make_tuple(abi.TUPLE_A, [ctx.upload(pv)]))
    return t


def test_agreement_with_sorted_by(hip_engine):
    """per_limit = ALL, ROW_NUMBER: exactly sdqh_table_sorted_by's rows, whatever partitions; no partition, RANK, per_limit = 1: the
    rows equal to the first in all terms."""
    from test_order_by_gpu import SPECS
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    done = 0
    for n in (S - 1, 5 * T + 17):
        t = _probed_table(ctx, n)
        try:
            for spec in SPECS:
                assert len(spec) <= abi.SORT_MAX_KEYS
                for min_hits in (0, 2):
                    want = ctx.table_sorted_by(t, min_hits, ALL, spec, n)
                    for npart in sorted({0, 1, len(spec)}):
                        got = ctx.table_window(t, min_hits, npart, spec, abi.WIN_ROW_NUMBER, ALL, ALL, n)
                        assert all((np.asarray(g).view(np.int64) == np.asarray(w).view(np.int64)).all() for g, w in zip(got[:4], want))
                        if npart == len(spec):                             # every tie its own partition: the other kinds give 1 everywhere
                            assert (ctx.table_window(t, min_hits, npart, spec, abi.WIN_DENSE_RANK, ALL, ALL, n)[4] == 1).all()
                        done += 1
                    first = ctx.table_window(t, min_hits, 0, spec, abi.WIN_RANK, 1, ALL, 64)
                    imgs = np.array([u for u in _images(tuple(None if a is None else np.asarray(a) for a in want), spec)])
                    tied = (imgs == imgs[:, :1]).all(axis=0)
                    assert tied[:tied.sum()].all() and len(first[0]) == tied.sum() and (first[0] == want[0][:tied.sum()]).all() and (first[4] == 1).all()
        finally:
            t.free()
    assert done >= 2 * 5 * 2 * 2


ENTRY_POINTS = ("table_sorted", "table_sorted_by", "table_window")
OUTPUTS = ("keys", "payload", "values", "hits")


def _entry_point_calls(ctx, t, min_hits, spec, limit, cap, want):
    """sdqh_table_sorted(spec), sdqh_table_sorted_by(spec as underived terms) and sdqh_table_window(no partition, ROW_NUMBER, every row
    kept, no rank column) through the raw C calls, each over its own arrays of `cap` rows filled with -7, of which those named in `want`
    are passed: [(return code, *out_n, {name: array}, kernel names of the call's profile)].  Doubles are held as their int64 bits."""
    lead = {"table_sorted": (C.c_int64(limit), C.c_int(len(spec)), abi._marshal_sort_keys(spec)),
            "table_sorted_by": (C.c_int64(limit), C.c_int(len(spec)), abi._marshal_sort_terms(spec)),
            "table_window": (C.c_int(0), C.c_int(len(spec)), abi._marshal_sort_terms(spec), C.c_int(abi.WIN_ROW_NUMBER), C.c_int64(ALL), C.c_int64(limit))}
    calls = []
    for name in ENTRY_POINTS:
        arrs = {"keys": np.full(cap, -7, np.int64), "payload": np.full((2, cap), -7, np.int64),
                "values": np.full((abi.TUPLE_MAX_VALUES, cap), -7, np.int64), "hits": np.full(cap, -7, np.int64)}
        outs = [arrs[o].ctypes.data_as(C.c_void_p) if o in want else None for o in OUTPUTS] + ([None] if name == "table_window" else [])
        got = C.c_int64(-7)
        rc = getattr(ctx.lib, "sdqh_" + name)(ctx.handle, t.handle, C.c_int64(min_hits), *lead[name], C.c_int64(cap), *outs, C.byref(got))
        calls.append((rc, got.value, arrs, [nm for nm, _ in ctx.profile()]))
    return calls


def test_the_three_entry_points_agree(hip_engine):
    """One path behind three entry points: for the same underived columns sdqh_table_sorted, sdqh_table_sorted_by and the window call
    that keeps every row and wants no rank return the same *out_n and bit-identical arrays — the rows numpy's stable lexsort gives —
    whichever of the output arrays are passed (the emit kernel's null pointers); arrays not passed and rows beyond *out_n keep their
    fill; a capacity below the count is SDQH_ERR_OVERFLOW with the needed count and nothing written.  The two plain calls launch no
    window kernel and exactly the kernels recorded from the commit before the paths were merged (tests/golden/order_path_kernels.json:
    the launches of a call depend on which digits of its keys vary, so they are listed per case)."""
    import json
    from test_order_by_gpu import SPECS
    ctx = hip_engine.ctx
    S, tile, _ = ctx.sort_geometry()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "order_path_kernels.json")) as fh:
        golden = json.load(fh)
    assert golden["geometry"] == [S, tile]
    wants = (OUTPUTS, ("keys",), ("values", "hits"))
    done = 0
    ctx.set_profiling(1)
    try:
        for n in (0, 1, S, S + 1, tile + 1, 3 * tile + 5):
            t = _probed_table(ctx, n)
            try:
                for min_hits in (0, 2):
                    rows = _stage_rows(ctx, t, min_hits)
                    m = len(rows[0])
                    assert m <= n and (n < S or m >= 7), (n, min_hits, m)
                    tied = False
                    for si, spec in enumerate(SPECS):
                        imgs = _images(rows, spec)
                        order = np.lexsort(imgs[::-1]) if m else np.zeros(0, np.int64)
                        tied |= m > 1 and bool(np.all([u[order][1:] == u[order][:-1] for u in imgs], axis=0).any())
                        for want in wants:
                            cap = m + 3
                            exp = {"keys": np.full(cap, -7, np.int64), "payload": np.full((2, cap), -7, np.int64),
                                   "values": np.full((abi.TUPLE_MAX_VALUES, cap), -7, np.int64), "hits": np.full(cap, -7, np.int64)}
                            if "keys" in want:
                                exp["keys"][:m] = rows[0][order]
                            if "payload" in want:
                                exp["payload"][:, :m] = np.asarray(rows[1])[:2, order]
                            if "values" in want:                               # (the value rows the table does not have are zeroed)
                                exp["values"][:, :m] = 0
                                exp["values"][0, :m] = np.ascontiguousarray(rows[2][0][order]).view(np.int64)
                            if "hits" in want:
                                exp["hits"][:m] = rows[3][order]
                            calls = _entry_point_calls(ctx, t, min_hits, spec, ALL, cap, want)
                            for name, (rc, got, arrs, kernels) in zip(ENTRY_POINTS, calls):
                                what = (n, min_hits, si, want, name)
                                assert (rc, got) == (abi.OK, m), what
                                for o in OUTPUTS:
                                    assert (arrs[o] == exp[o]).all(), what + (o,)
                                if name != "table_window" and want is OUTPUTS:
                                    assert not [k for k in kernels if k.startswith("k_win")], what
                                    assert kernels == golden["calls"]["n=%d min_hits=%d spec=%d" % (n, min_hits, si)].split(), what
                            done += 1
                        for name, (rc, got, arrs, _) in zip(ENTRY_POINTS, _entry_point_calls(ctx, t, min_hits, spec, 7, 6, OUTPUTS)):
                            assert (rc, got) == ((abi.ERR_OVERFLOW if m >= 7 else abi.OK), min(7, m)), (n, min_hits, si, name, "limit 7, capacity 6")
                            assert m < 7 or all((arrs[o] == -7).all() for o in OUTPUTS), (n, min_hits, si, name, "written on overflow")
                    assert tied or n < S, (n, min_hits, "no tie in any spec: stability is not exercised")
            finally:
                t.free()
    finally:
        ctx.set_profiling(0)
    assert done == 6 * 2 * len(SPECS) * 3


def test_window_paths_launch_what_they_launched(hip_engine):
    """One step type and one partition pass behind the five window entry points: every call of tests/golden/make_window_path_golden.py
    (ranks, frames, slides, value / group frames, quantiles; with and without a filter, a rank column, fold kernels; count-only and a
    capacity below the count; at the sizes where the sort and the tile scans change path) returns the code, the *out_n and bit for bit
    the arrays it returned at the commit before the host paths were merged, and launches exactly the kernels it launched there, in
    that order (tests/golden/window_path_kernels.json)."""
    import importlib.util
    import json
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    mod = importlib.util.spec_from_file_location("make_window_path_golden", os.path.join(golden_dir, "make_window_path_golden.py"))
    recorder = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(recorder)
    with open(os.path.join(golden_dir, "window_path_kernels.json")) as fh:
        golden = json.load(fh)
    ctx = hip_engine.ctx
    S, tile, _ = ctx.sort_geometry()
    assert golden["geometry"] == [S, tile] == [1024, 512]
    ctx.set_profiling(1)
    try:
        got = recorder.run_cases(ctx, abi, _probed_table)
    finally:
        ctx.set_profiling(0)
    assert sorted(got["calls"]) == sorted(golden["calls"]) and len(golden["calls"]) == 6 * 2 * 31
    for case, want in golden["calls"].items():
        assert got["calls"][case] == want, case
    assert any("k_wrg_upper" in c["kernels"] for c in golden["calls"].values()) and any("k_win_place" in c["kernels"] for c in golden["calls"].values())


# 6. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(hip_engine):
    ctx = hip_engine.ctx
    t = _table(ctx, *_pattern("runs", 700, 512, np.random.default_rng(3)))
    try:
        keys = np.full(700, -7, np.int64)
        for npart, terms, kind, per_limit, limit, nterms in ((1, TERMS, abi.WIN_RANK, 0, ALL, None), (1, TERMS, abi.WIN_RANK, 2, 0, None), (1, TERMS, 3, 2, ALL, None),
                                                             (1, TERMS, -1, 2, ALL, None), (-1, TERMS, abi.WIN_RANK, 2, ALL, None), (4, TERMS, abi.WIN_RANK, 2, ALL, None),
                                                             (0, TERMS, abi.WIN_RANK, 2, ALL, 0), (1, [TERMS[0]] * 9, abi.WIN_RANK, 2, ALL, None),
                                                             (1, [(P, 1, False, False)], abi.WIN_RANK, 2, ALL, None), (1, [(V, 0, False, True, 2, 0, 0, None)], abi.WIN_RANK, 2, ALL, None)):
            assert _raw(ctx, t, 1, npart, terms, kind, per_limit, limit, 700, keys, nterms=nterms) == (abi.ERR_INVALID, -7), (npart, kind, per_limit, limit)
            assert (keys == -7).all()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window(t, 1, 1, TERMS, abi.WIN_RANK, 0, ALL, 64)
        assert e.value.code == abi.ERR_INVALID
        assert _check(ctx, t, TERMS, 1, "after the errors", per_limits=(2,))[0] == 3 * 3      # the context still works
    finally:
        t.free()


# 7. through the engine and the decorator -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0.01, 0.05])
def db(request):
    qs = ["q3", "q15", "q16"]
    return tpch.generate(request.param, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))


@pytest.fixture()
def on_the_decorator(hip_lib):
    from sdqlpy_amd import sdql_lib
    eng = engine.Engine(hip_lib.context(device=0))
    engine.use_engine(eng)
    sdql_lib._state.update(mode=sdql_lib.MODE_HIP, runner=None, device=0)
    yield eng
    engine.reset_default_engine()
    sdql_lib._state.update(mode=None)


def _close(a, b):
    return a == b if not isinstance(a, float) else abs(a - b) <= 1e-10 * max(abs(a), abs(b))


def _numpy_window(res, by, order, kind, per_limit):
    """(row indices, ranks) of a result set's own rows, by numpy: numeric columns through the bit map, text through np.unique."""
    cols = []
    for name, d in [(b, "asc") for b in by] + list(order):
        a = np.asarray(res.column(name))
        if a.dtype.kind not in "if":
            a = np.unique(a, return_inverse=True)[1].reshape(-1).astype(np.int64)
        u = _sort_bits(a.astype(np.float64 if a.dtype.kind == "f" else np.int64), a.dtype.kind == "f", d == "desc")
        cols.append((u ^ (np.uint64(1) << np.uint64(63))).view(np.int64))                # the image as the signed integer that orders like it
    rows = (np.arange(len(res)), cols, None, None)
    ref = Ranked(rows, [(P, i, False, False) for i in range(len(cols))], len(by))
    sel = ref.kept(kind, per_limit)
    return ref.order[sel], ref.ranks[kind][sel]


def _same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and all(_close(p, q) for p, q in zip(x, y)), (x, y)


def test_q3_and_q15_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    everything = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    assert len(everything) > 100
    for run in range(3):
        top = Q.q3.top_per(3, by, order)(*args)
        assert eng.stats()["order_routes"][-1] == {"route": "window", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "kind": "row_number", "per_limit": 3}
        idx, _ = _numpy_window(everything, by, order, abi.WIN_ROW_NUMBER, 3)
        assert top.columns == everything.columns
        _same_rows(top.ordered_rows(), [everything.ordered_rows()[i] for i in idx])
        num = Q.q3.numbered(by, order, kind="dense_rank", name="nth")(*args)
        assert eng.stats()["order_routes"][-1]["route"] == "window" and eng.stats()["order_routes"][-1]["kind"] == "dense_rank"
        assert num.columns == everything.columns + ["nth"] and num.column("nth").dtype == np.int64
        idx, rank = _numpy_window(num, by, order, abi.WIN_DENSE_RANK, ALL)              # on its own rows: exact
        assert (idx == np.arange(len(num))).all() and (num.column("nth") == rank).all() and len(num) == len(everything)
    monkeypatch.setattr(eng, "device_window", False)
    host = Q.q3.top_per(3, by, order)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["per"] == by
    _same_rows(host.ordered_rows(), top.ordered_rows())
    _same_rows(Q.q3.numbered(by, order, kind="dense_rank", name="nth")(*args).ordered_rows(), num.ordered_rows())
    monkeypatch.setattr(eng, "device_window", True)
    # q15: the suppliers whose revenue is the maximum, ties kept = q15_max
    args = [db[t] for t in Q.QUERY_TABLES["q15"]]
    best = Q.q15.top_per(1, [], [("total_revenue", "desc")], ties=True)(*args)
    assert eng.stats()["order_routes"][-1]["kind"] == "rank" and eng.stats()["order_routes"][-1]["per"] == []
    want = Q.q15_max(*args)
    assert len(best) >= 1 and sorted(best.column("s_suppkey").tolist()) == sorted(want.column("s_suppkey").tolist())
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*[db[t] for t in Q.QUERY_TABLES["q3"]])
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_the_switch_forces_the_host_route(hip_lib, db, monkeypatch):
    monkeypatch.setenv("SDQLPY_AMD_DEVICE_WINDOW", "0")
    eng = engine.Engine(hip_lib.context(device=0))
    try:
        assert eng.device_window is False
        plan = frontend.lower_function(Q.QUERIES["q3"])
        from sdqlpy_amd.result import window_request
        req = window_request(engine.result_columns(plan), ["o_orderdate"], [("revenue", "desc")], "row_number", 2)
        res = engine.execute_plan(eng, plan, [db[t] for t in Q.QUERY_TABLES["q3"]], req)
        assert eng.stats()["order_routes"][-1]["route"] == "host" and len(res) > 0
    finally:
        eng.close()


def test_text_and_radix_fields_on_the_decorator(on_the_decorator, db, monkeypatch):
    """q16's result — text fields in a mixed-radix key: PARTITION BY brand ORDER BY count desc on the device, and a request of more
    than SORT_MAX_KEYS terms on the host, both equal to numpy on the result's own rows and to each other."""
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q16"]]
    by, order = ["p_brand"], [("supplier_cnt", "desc")]
    dev = Q.q16.numbered(by, order, kind="rank", name="r")(*args)
    route = eng.stats()["order_routes"][-1]
    assert route["route"] == "window" and route["per"] == by and route["order"] == ["supplier_cnt"]
    idx, rank = _numpy_window(dev, by, order, abi.WIN_RANK, ALL)           # on its own rows (sorted already: a stable sort leaves them)
    assert len(dev) > 100 and (idx == np.arange(len(dev))).all() and (dev.column("r") == rank).all()
    # (what is left of a tie is the order of the group table's entries, which one run need not share with the next: between runs the
    # rows compare as sets and the (brand, count) pairs as sequences — RANK keeps whole ties, so both are determined)
    pairs = lambda rows: [(r[0], r[3]) for r in rows]
    top = Q.q16.top_per(2, by, order, ties=True)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "window" and top.columns == dev.columns[:4] == ["p_brand", "p_type", "p_size", "supplier_cnt"]
    kept = [r[:4] for r, k in zip(dev.ordered_rows(), dev.column("r") <= 2) if k]
    assert sorted(top.ordered_rows()) == sorted(kept) and pairs(top.ordered_rows()) == pairs(kept) and 0 < len(kept) < len(dev)
    monkeypatch.setattr(eng, "device_window", False)
    host = Q.q16.top_per(2, by, order, ties=True)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    assert sorted(host.ordered_rows()) == sorted(top.ordered_rows()) and pairs(host.ordered_rows()) == pairs(top.ordered_rows())
    monkeypatch.setattr(eng, "device_window", True)
    # nine terms: beyond SDQH_SORT_MAX_KEYS, so on the host
    long_order = [("supplier_cnt", "desc"), ("p_type", "asc"), ("p_size", "asc"), ("p_brand", "desc"), ("p_size", "desc"), ("p_type", "desc"), ("supplier_cnt", "asc"), ("p_size", "asc")]
    wide = Q.q16.numbered(by, long_order, name="r")(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and len(eng.stats()["order_routes"][-1]["order"]) == 8
    idx, rank = _numpy_window(wide, by, long_order, abi.WIN_ROW_NUMBER, ALL)
    assert (idx == np.arange(len(wide))).all() and (wide.column("r") == rank).all() and len(wide) == len(dev)
