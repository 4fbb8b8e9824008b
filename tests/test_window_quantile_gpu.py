"""Functions of the partition's size on the MI355X (run with -m gpu): sdqh_table_window_quantile (include/sdqh_sort_quantile.h) against
numpy at every size at which the sort or the tile scan takes another path — the smallest shapes at which a partition's end or a tie
run's end must come from a later tile —, on partition patterns that exercise the carries between tiles in both directions, on every
table layout, over derived terms, on edge values, against sdqh_table_window / _window_agg / _window_slide / _sorted_by where they
overlap, its argument errors, what it launches, and through the engine and the decorator.

The expected rows are the table's own K-F rows reordered by a stable numpy lexsort (test_window_gpu's Ranked, test_window_slide_gpu's
Slid for the partitions' ends).  The values are restated here from the header: for sorted row j in the partition [s, e], m = e - s + 1,
i = j - s, [f, l] its tie run's offsets; NTILE in int64 arithmetic, the ranks as one float64 division, the percentiles with one IEEE
operation per numpy call.  Nothing is imported from the product's host route.  Comparison is bit for bit, except that a NaN
PERCENTILE_CONT is compared as NaN-ness only."""
import ctypes as C
import struct

import numpy as np
import pytest

from sdqlpy_amd import abi, engine
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import ResultSet
from test_window_gpu import (EDGE_DOUBLES, EDGE_INTS, PATTERNS, TERMS, Ranked, _pattern, _probed_table, _runs, _sizes as _window_sizes, _sort_bits, _stage_rows, _table, _under,
                             db, hip_engine, on_the_decorator)     # noqa: F401 (fixtures)
from test_window_slide_gpu import Slid, _last_of

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
NTILE, PRANK, CDIST, NTH, DISC, CONT = abi.WQ_NTILE, abi.WQ_PERCENT_RANK, abi.WQ_CUME_DIST, abi.WQ_NTH, abi.WQ_PERCENTILE_DISC, abi.WQ_PERCENTILE_CONT
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
PS = [0.0, 5e-324, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.7, float(np.nextafter(1.0, 0.0)), 1.0]
MEASURES = [(V, 0, True), (H, 0, False), (P, 0, False)]                    # value 0 (a double), the hit count, an integer payload
NAN_BITS = struct.unpack("<q", struct.pack("<d", float("nan")))[0]
EMPTIES = (0, -1, I_MIN, NAN_BITS)


def _col(fn, measure=(K, 0, False), arg=0, p=0.0, empty=0):
    return (fn,) + tuple(measure) + (arg, p, empty)


def _sizes(ctx):
    T, S, sizes = _window_sizes(ctx)
    assert ctx.window_quantile_geometry() == ctx.window_geometry() == T     # one tile for ranks, aggregates, slides and quantiles
    return T, S, sizes


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
class Quant(Slid):
    """A table's rows in the order of `terms`, and the expected value of every column at every sorted position as int64 bit patterns."""

    def __init__(self, rows, terms, npart, rank_tables=None):
        Slid.__init__(self, rows, terms, npart, rank_tables)
        self.m, self.i = self.end - self.start + 1, self.pos - self.start
        self.f = (np.maximum.accumulate(np.where(self.ref.tie_head, self.pos, 0)) if self.n else self.pos) - self.start
        self.l = _last_of(self.ref.tie_head) - self.start
        if 0 < self.n <= 300:                                              # the same once more, walking the sorted rows
            a = 0
            for j in range(1, self.n + 1):
                if j == self.n or self.ref.part_head[j]:
                    assert (self.start[a:j] == a).all() and (self.end[a:j] == j - 1).all()
                    p = a
                    for q in range(a + 1, j + 1):
                        if q == j or self.ref.tie_head[q]:
                            assert (self.f[p:q] == p - a).all() and (self.l[p:q] == q - 1 - a).all()
                            p = q
                    a = j

    def sizes(self):
        """a few partition sizes to take b and k from: the smallest, the largest, the median"""
        if not self.n:
            return [1]
        ms = np.sort(self.m[self.ref.part_head])
        return sorted({int(ms[0]), int(ms[-1]), int(ms[len(ms) // 2])})

    def want(self, col):
        fn, kind, index, is_f64, arg, p, empty = col
        m, i, s, e = self.m, self.i, self.start, self.end
        if fn == NTILE:
            q, r = m // arg, m % arg
            big = r * (q + 1)
            return np.where(i < big, i // (q + 1) + 1, r + (i - big) // np.maximum(q, 1) + 1).astype(np.int64)
        if fn == PRANK:
            return _bits(np.where(m == 1, 0.0, self.f.astype(np.float64) / np.maximum(m - 1, 1).astype(np.float64)))
        if fn == CDIST:
            return _bits((self.l + 1).astype(np.float64) / m.astype(np.float64))
        raw = self.raw(kind, index)
        if fn == NTH:
            ak = min(abs(arg), self.n + 1)                                 # (beyond n: outside every partition)
            inside = ak <= m
            src = np.where(inside, s + ak - 1 if arg > 0 else e + 1 - ak, self.pos)
            return np.where(inside, raw[src], np.int64(empty))
        if fn == DISC:
            up = np.ceil(np.float64(p) * m.astype(np.float64))
            return raw[s + np.maximum(up.astype(np.int64) - 1, 0)]
        is_f64 = kind == V or (kind == P and bool(is_f64))
        x = np.float64(p) * (m - 1).astype(np.float64)
        lo, hi = np.floor(x), np.ceil(x)
        va, vb = raw[s + lo.astype(np.int64)], raw[s + hi.astype(np.int64)]
        a, b = (va.view(np.float64), vb.view(np.float64)) if is_f64 else (va.astype(np.float64), vb.astype(np.float64))
        with np.errstate(invalid="ignore", over="ignore"):
            d = b - a
            w = x - lo
            t = d * w
            y = a + t
        return _bits(np.where(lo == hi, a, y))


def _is_f64(col):
    fn, kind, _, is_f64 = col[:4]
    return fn in (PRANK, CDIST, CONT) or (fn in (NTH, DISC) and (kind == V or (kind == P and bool(is_f64))))


def _same_col(col, got, want, what):
    assert got.dtype == (np.float64 if _is_f64(col) else np.int64), (what, col, got.dtype)
    g = _bits(got)
    assert len(g) == len(want), (what, col, len(g), len(want))
    ok = g == want
    if col[0] == CONT:
        ok |= np.isnan(g.view(np.float64)) & np.isnan(want.view(np.float64))
    bad = np.nonzero(~ok)[0]
    assert len(bad) == 0, (what, col, bad[:5], g[bad[:5]], want[bad[:5]])


def _same_rows(got, rows, idx, what):
    gk, gp, gv, gh = got[:4]
    keys, payload, values, hits = rows
    assert len(gk) == len(idx) and (gk == keys[idx]).all(), what
    if payload is not None:
        for p in range(len(payload)):
            assert (gp[p] == payload[p][idx]).all(), (what, "payload", p)
    if values is not None:
        assert (_bits(gv[0]) == _bits(values[0][idx])).all(), (what, "value")
    if hits is not None and gh is not None:
        assert (gh == hits[idx]).all(), (what, "hits")


def _column_lists(ref, measures=MEASURES, shift=0):
    """Calls of four columns each that together hold every function with every argument of the lists — b in {1, 2, 3, m - 1, m, m + 1,
    2^63 - 1}, k in {1, 2, -1, m, m + 1, -m, -m - 1, +-(2^63 - 1), INT64_MIN}, every p of PS, m taken from the partitions at hand —
    in mixed combinations, after three fixed ones: no measure (nothing gathered), no PERCENT_RANK / CUME_DIST (no tie ends), both."""
    ms = ref.sizes()
    bs = sorted({1, 2, 3, I_MAX} | {b for m in ms for b in (m - 1, m, m + 1) if b >= 1})
    ks = sorted({1, 2, -1, I_MAX, -I_MAX, I_MIN} | {k for m in ms for k in (m, m + 1, -m, -m - 1)})
    pick = lambda j: measures[(j + shift) % len(measures)]
    flat = [_col(NTILE, arg=b) for b in bs]
    flat += [_col(NTH, pick(j), arg=k, empty=EMPTIES[j % len(EMPTIES)]) for j, k in enumerate(ks)]
    flat += [_col(DISC, pick(j), p=p) for j, p in enumerate(PS)] + [_col(CONT, pick(j + 1), p=p) for j, p in enumerate(PS)]
    flat += [_col(PRANK), _col(CDIST)] * 3
    stride = (len(flat) + 3) // 4                                           # columns `stride` apart share a call: the functions mix
    mixed = [[flat[j] for j in range(c, len(flat), stride)][:4] for c in range(stride)]
    fixed = [[_col(NTILE, arg=4), _col(PRANK), _col(CDIST), _col(NTILE, arg=ms[-1])],
             [_col(NTH, pick(0), arg=-1, empty=-9), _col(DISC, pick(1), p=0.9), _col(CONT, pick(0), p=0.5), _col(NTILE, arg=4)],
             [_col(CONT, pick(0), p=0.5), _col(CDIST), _col(PRANK), _col(DISC, pick(1), p=0.9)]]
    assert all(1 <= len(cols) <= abi.WQUANT_MAX_COLS for cols in fixed + mixed) and sum(len(c) for c in mixed) == len(flat)
    return fixed, mixed


def _check(ctx, t, terms, npart, what, min_hits=1, rank_tables=None, measures=MEASURES, per_limits=(1, 2, ALL), full=True):
    """Every column list with every row kept and no limit; the three fixed lists again under per_limit x limit — the rows those of
    sdqh_table_window(ROW_NUMBER, per_limit), bit for bit — with a limit below n so that values depend on rows beyond it; the
    count-only call; two calls, the same bits."""
    rows = _stage_rows(ctx, t, min_hits)
    ref = Quant(rows, terms, npart, rank_tables)
    fixed, mixed = _column_lists(ref, measures)
    want = {}

    def expect(col):
        if col not in want:
            want[col] = ref.want(col)
        return want[col]
    done = 0
    for cols in fixed + (mixed if full else mixed[:2]):
        got = ctx.table_window_quantile(t, min_hits, npart, terms, cols, ALL, ALL, 64, want_hits=t.accumulate)
        _same_rows(got, rows, ref.order, (what, cols))
        for col, a in zip(cols, got[4]):
            _same_col(col, a, expect(col), what)
        done += 1
    if ref.n:                                                              # the skips take the same values: a column is the same whatever shares its call
        again = ctx.table_window_quantile(t, min_hits, npart, terms, fixed[2], ALL, ALL, ref.n, want_hits=t.accumulate)
        assert all((_bits(a) == expect(col)).all() or col[0] == CONT for col, a in zip(fixed[2], again[4]))
        twice = ctx.table_window_quantile(t, min_hits, npart, terms, fixed[2], ALL, ALL, ref.n, want_hits=t.accumulate)
        assert all((_bits(a) == _bits(b)).all() for a, b in zip(again[4], twice[4])), (what, "two calls")
    for per_limit in per_limits:
        sel = np.nonzero(ref.i < per_limit)[0]
        for limit in sorted({1, max(1, len(sel) // 2), ALL}):
            keep = sel[:limit]
            win = ctx.table_window(t, min_hits, npart, terms, abi.WIN_ROW_NUMBER, per_limit, limit, 64, want_hits=t.accumulate, want_rank=False)
            for cols in fixed:
                got = ctx.table_window_quantile(t, min_hits, npart, terms, cols, per_limit, limit, 64, want_hits=t.accumulate)
                _same_rows(got, rows, ref.order[keep], (what, per_limit, limit))
                assert all(g is None and w is None or (_bits(g) == _bits(w)).all() for g, w in zip(got[:4], win[:4])), (what, per_limit, limit, "the window's rows")
                for col, a in zip(cols, got[4]):
                    _same_col(col, a, expect(col)[keep], (what, per_limit, limit))
                done += 1
        assert _raw(ctx, t, min_hits, npart, terms, fixed[1], per_limit, ALL, 0) == (abi.OK, len(sel)), (what, per_limit, "count")
    return done, ref


def _marshal(cols):
    arr = (abi.WindowQuantile * max(1, len(cols)))()
    for i, (fn, kind, index, is_f64, arg, p, empty) in enumerate(cols):
        arr[i].fn, arr[i].kind, arr[i].index, arr[i].is_f64, arr[i].arg, arr[i].p, arr[i].empty = fn, kind, index, 1 if is_f64 else 0, arg, p, empty
    return arr


def _raw(ctx, t, min_hits, npart, terms, cols, per_limit, limit, capacity, keys=None, out=None, nterms=None, ncols=None):
    got = C.c_int64(-7)
    rc = ctx.lib.sdqh_table_window_quantile(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms),
                                            abi._marshal_sort_terms(terms), C.c_int(len(cols) if ncols is None else ncols), _marshal(cols), C.c_int64(per_limit),
                                            C.c_int64(limit), C.c_int64(capacity), None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                            None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value


# 1. partition patterns x sizes x functions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    for n in sizes:
        t = _table(ctx, *_pattern(pattern, n, T, rng))
        try:
            done, ref = _check(ctx, t, TERMS, 1, (pattern, n), full=n <= 2 * T + 1 or n == 70001)
            assert done >= 5 + 3 * 1 * 3 and ref.n == n
            if pattern == "a long partition" and n == 70001:              # tiles wholly inside a tie run: both ends come from other tiles
                tiles = ref.ref.tie_head[:(n // T) * T].reshape(-1, T)
                assert (~tiles.any(axis=1)).sum() >= 2 and ref.m.max() >= 3 * T and (ref.l - ref.f + 1).max() >= 3 * T
            if pattern == "one partition" and n == 70001:                 # tiles with tie heads but no partition head
                assert ref.ref.part_head.sum() == 1 and ref.ref.tie_head[T:2 * T].any()
            if n:                                                          # a capacity one too small: the needed count, nothing written
                cols = [_col(NTILE, arg=2), _col(CONT, MEASURES[0], p=0.5)]
                kept = int((ref.i < 2).sum())
                keys, out = np.full(n, -7, np.int64), np.full((2, n), -7, np.int64)
                assert _raw(ctx, t, 1, 1, TERMS, cols, 2, ALL, kept - 1, keys, out) == (abi.ERR_OVERFLOW, kept)
                assert _raw(ctx, t, 1, 1, TERMS, cols, ALL, ALL, n - 1, keys, out) == (abi.ERR_OVERFLOW, n)
                assert _raw(ctx, t, 1, 1, TERMS, cols, ALL, 7, min(n, 7) - 1, keys, out) == (abi.ERR_OVERFLOW, min(n, 7))
                assert (keys == -7).all() and (out == -7).all()
                assert _raw(ctx, t, 1, 1, TERMS, cols, ALL, ALL, 0) == (abi.OK, n) and _raw(ctx, t, 1, 1, TERMS, cols, ALL, 5, 0) == (abi.OK, min(n, 5))
            else:
                assert _raw(ctx, t, 1, 1, TERMS, [_col(NTILE, arg=2)], 1, ALL, 0, np.zeros(1, np.int64), np.zeros((1, 1), np.int64)) == (abi.OK, 0)
        finally:
            t.free()


def test_values_depend_on_rows_beyond_the_limit(hip_engine):
    """One partition of 70001 rows, the first 10 returned: the median, the last value and CUME_DIST are those of the whole partition."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 70001
    t = _table(ctx, *_pattern("one partition", n, T, np.random.default_rng(1)))
    try:
        rows = _stage_rows(ctx, t, 1)
        ref = Quant(rows, TERMS, 1)
        cols = [_col(CONT, MEASURES[0], p=0.5), _col(NTH, MEASURES[0], arg=-1), _col(CDIST), _col(NTILE, arg=7)]
        got = ctx.table_window_quantile(t, 1, 1, TERMS, cols, ALL, 10, 10)
        assert len(got[0]) == 10
        x = ref.column(V, 0)
        assert (got[4][0] == x[(n - 1) // 2]).all() and (got[4][1] == x[-1]).all() and x[-1] != x[9] and x[(n - 1) // 2] != x[9]
        for col, a in zip(cols, got[4]):
            _same_col(col, a, ref.want(col)[:10], "limit 10")
    finally:
        t.free()


def test_heads_on_wave_and_tile_boundaries(hip_engine):
    """Partitions that start exactly on wave and tile boundaries, end exactly before them, and cover whole tiles: the next head of
    a batch's or a tile's last position is the first position of the one after."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 6 * T + 1
    rng = np.random.default_rng(8)
    part = _runs(n, [64, 64, T - 128, T, 2 * T, 1, 63, T - 64])
    value, hits, mix = rng.integers(-3, 3, n).astype(np.float64), rng.integers(1, 3, n), rng.permutation(n)
    t = _table(ctx, part[mix], value[mix], hits[mix])
    try:
        done, ref = _check(ctx, t, TERMS, 1, "aligned")
        heads = np.nonzero(ref.ref.part_head)[0]
        assert {0, 64, 128, T, 2 * T, 4 * T, 4 * T + 1, 4 * T + 64, 5 * T, 6 * T} <= set(heads.tolist()) and (ref.l > ref.f).any() and done > 20
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
            return sum(_check(ctx, t, TERMS, 1, ("layout", dups, mh), min_hits=mh, per_limits=(1, ALL), full=False)[0] for mh in (0, 1, 2))
        finally:
            t.free()
    assert run(0) >= 3 * (5 + 2 * 2 * 3)
    assert run(200) >= 3 * (5 + 2 * 2 * 3)
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) >= 3 * (5 + 2 * 2 * 3)
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
            assert _check(ctx, t, terms, 1, ("xbuild", mh), min_hits=mh, measures=[(V, 0, True), (H, 0, False), (K, 0, False)], per_limits=(2, ALL), full=False)[0] >= 5 + 2 * 2 * 3
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
                done, ref = _check(ctx, t, terms, 1, ("derived", n), min_hits=0, rank_tables={id(ct): want}, measures=[(K, 0, False), (P, 0, False)], full=False)
                assert done >= 5 + 3 * 2 * 3 and (ref.l > ref.f).any()
                bad = terms[:2] + [(P, 0, False, False, 0, 0, 0, short)]
                keys_out, out = np.full(len(keys), -7, np.int64), np.full((2, len(keys)), -7, np.int64)
                assert _raw(ctx, t, 0, 1, bad, [_col(NTILE, arg=2), _col(CDIST)], ALL, ALL, len(keys), keys_out, out) == (abi.ERR_INVALID, -7)
                assert (keys_out == -7).all() and (out == -7).all() and b"term 2" in ctx.lib.sdqh_last_error(ctx.handle)
            finally:
                t.free()
    finally:
        ct.free(); short.free()


# 4. edge values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 2600])
def test_edge_values(hip_engine, n):
    """+-0.0, +-inf, two NaN bit patterns, DBL_MAX and the int64 extremes as measures: NTH and PERCENTILE_DISC copy them bit for bit;
    PERCENTILE_CONT over integers beyond 2^53 (one rounding each, then four operations) and over inf neighbours (inf - inf: a NaN)."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) * 3 - n
    ints = np.resize(np.concatenate([EDGE_INTS, [(1 << 53) + 1, -(1 << 53) - 3, (1 << 62) + 12345]]), n)[rng.permutation(n)]
    dbls = np.resize(np.concatenate([EDGE_DOUBLES, [-np.finfo(np.float64).max, 5e-324, 9007199254740994.0]]), n)[rng.permutation(n)]
    group = rng.integers(0, 9, n).astype(np.int64)
    t = ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ints), ctx.upload(dbls.view(np.int64)), ctx.upload(group)], accumulate=False)
    try:
        measures = [(P, 0, False), (P, 1, True)]
        done = 0
        for terms, npart in (([(P, 2, False, False), (K, 0, False, False)], 1), ([(P, 2, True, False), (P, 1, False, True)], 1), ([(P, 1, False, True), (P, 0, True, False)], 1),
                             ([(P, 0, False, False)], 0), ([(P, 2, False, False), (P, 0, True, False)], 1)):
            d, ref = _check(ctx, t, terms, npart, ("edge", terms, npart), min_hits=0, measures=measures)
            done += d
            for measure in measures:                                       # every row's own value and its partition's first and last, bit for bit
                raw = ref.raw(measure[0], measure[1])
                got = ctx.table_window_quantile(t, 0, npart, terms, [_col(NTH, measure, arg=1), _col(NTH, measure, arg=-1), _col(DISC, measure, p=0.0), _col(DISC, measure, p=1.0)],
                                                ALL, ALL, n)[4]
                assert (_bits(got[0]) == raw[ref.start]).all() and (_bits(got[1]) == raw[ref.end]).all()
                assert (_bits(got[2]) == raw[ref.start]).all() and (_bits(got[3]) == raw[ref.end]).all()
        assert done >= 5 * (5 + 3 * 2 * 3)
    finally:
        t.free()


def test_cont_on_inf_neighbours_and_wide_integers(hip_engine):
    """The median of two rows is a + (b - a) * 0.5 in four operations, whatever they overflow into: -inf and inf give inf - inf, a
    NaN; 1 and inf give inf; -DBL_MAX and DBL_MAX give inf (b - a overflows first); 2^53 + 1 and 2^53 + 3 round to 2^53 and 2^53 + 4
    before anything is subtracted; INT64_MIN and INT64_MAX give -2^63 + 2^64 * 0.5 = 0; 5 and 6 give 5.5."""
    ctx = hip_engine.ctx
    big = np.finfo(np.float64).max
    group = np.array([0, 0, 1, 1, 2, 2], np.int64)
    dbls = np.array([np.inf, -np.inf, np.inf, 1.0, -big, big], np.float64)
    ints = np.array([(1 << 53) + 3, (1 << 53) + 1, I_MAX, I_MIN, 6, 5], np.int64)
    t = ctx.hash_build_unique(6, abi.make_filter(), [], ctx.upload(np.arange(6, dtype=np.int64) + 10), [ctx.upload(ints), ctx.upload(dbls.view(np.int64)), ctx.upload(group)],
                              accumulate=False)
    try:
        got = ctx.table_window_quantile(t, 0, 1, [(P, 2, False, False), (P, 1, False, True)], [_col(CONT, (P, 1, True), p=0.5)], 1, ALL, 8)
        assert got[1][2].tolist() == [0, 1, 2] and np.isnan(got[4][0][0]) and got[4][0][1:].tolist() == [np.inf, np.inf]
        got = ctx.table_window_quantile(t, 0, 1, [(P, 2, False, False), (P, 0, False, False)], [_col(CONT, (P, 0, False), p=0.5), _col(CONT, (P, 0, False), p=0.0),
                                                                                              _col(CONT, (P, 0, False), p=1.0)], 1, ALL, 8)
        assert got[4][0].tolist() == [2.0 ** 53 + 2, 0.0, 5.5] and got[4][1].tolist() == [2.0 ** 53, -2.0 ** 63, 5.0] and got[4][2].tolist() == [2.0 ** 53 + 4, 2.0 ** 63, 6.0]
    finally:
        t.free()


# 5. agreement -----------------------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_siblings(hip_engine):
    """NTH(1) / NTH(-1) are sdqh_table_window_slide's FIRST / LAST over the unbounded frame; CUME_DIST x m is sdqh_table_window_agg's
    COUNT over RANGE; PERCENT_RANK is (RANK - 1) / (m - 1) from sdqh_table_window; per_limit = ALL with no columns returns exactly
    sdqh_table_sorted_by's rows."""
    from test_order_by_gpu import SPECS
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    UP, UF = abi.SLIDE_UNBOUNDED_PRECEDING, abi.SLIDE_UNBOUNDED_FOLLOWING
    done = 0
    for n in (S - 1, 5 * T + 17):
        t = _probed_table(ctx, n)
        try:
            for spec in SPECS:
                for min_hits in (0, 2):
                    want = ctx.table_sorted_by(t, min_hits, ALL, spec, n)
                    for npart in sorted({0, 1, len(spec)}):
                        got = ctx.table_window_quantile(t, min_hits, npart, spec, [_col(NTH, (V, 0, True), arg=1, empty=-1), _col(NTH, (P, 1, True), arg=-1, empty=-1), _col(CDIST),
                                                                                  _col(PRANK)], ALL, ALL, n)
                        assert all((_bits(g) == _bits(w)).all() for g, w in zip(got[:4], want))
                        bare = ctx.table_window_quantile(t, min_hits, npart, spec, [_col(NTILE, arg=3)], ALL, ALL, n, want_cols=False)
                        assert bare[4] is None and all((_bits(g) == _bits(w)).all() for g, w in zip(bare[:4], want))
                        slide = ctx.table_window_slide(t, min_hits, npart, spec, [(abi.WSLIDE_FIRST, V, 0, True, UP, UF, -1), (abi.WSLIDE_LAST, P, 1, True, UP, UF, -1),
                                                                                 (abi.WAGG_COUNT, K, 0, False, UP, UF, 0)], ALL, n)[4]
                        assert (_bits(got[4][0]) == _bits(slide[0])).all() and (_bits(got[4][1]) == _bits(slide[1])).all()
                        m = slide[2]
                        upto = ctx.table_window_agg(t, min_hits, npart, spec, [(abi.WAGG_COUNT, abi.FRAME_RANGE, K, 0, False)], ALL, n)[4][0]
                        assert (_bits(got[4][2]) == _bits(upto.astype(np.float64) / m.astype(np.float64))).all()      # CUME_DIST x m, as the one division it is
                        rank = ctx.table_window(t, min_hits, npart, spec, abi.WIN_RANK, ALL, ALL, n)[4]
                        assert (_bits(got[4][3]) == _bits(np.where(m == 1, 0.0, (rank - 1).astype(np.float64) / np.maximum(m - 1, 1).astype(np.float64)))).all()
                        done += 1
        finally:
            t.free()
    assert done >= 2 * 5 * 2 * 2


# 6. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(hip_engine):
    ctx = hip_engine.ctx
    t = _table(ctx, *_pattern("runs", 700, 512, np.random.default_rng(3)))
    m = MEASURES[0]
    ok = [_col(CONT, m, p=0.5)]
    try:
        keys, out = np.full(700, -7, np.int64), np.full((5, 700), -7, np.int64)
        for npart, terms, cols, per_limit, limit, nterms, ncols in (
                (1, TERMS, ok, ALL, 0, None, None), (1, TERMS, ok, 0, ALL, None, None), (1, TERMS, ok, -1, ALL, None, None), (-1, TERMS, ok, ALL, ALL, None, None),
                (4, TERMS, ok, ALL, ALL, None, None), (0, TERMS, ok, ALL, ALL, 0, None), (1, [TERMS[0]] * 9, ok, ALL, ALL, None, None), (1, [(P, 1, False, False)], ok, ALL, ALL, None, None),
                (1, [(V, 0, False, True, 2, 0, 0, None)], ok, ALL, ALL, None, None), (1, TERMS, ok, ALL, ALL, None, 0), (1, TERMS, ok * 5, ALL, ALL, None, None),
                (1, TERMS, [_col(6, m)], ALL, ALL, None, None), (1, TERMS, [_col(-1, m)], ALL, ALL, None, None), (1, TERMS, [_col(NTILE, arg=0)], ALL, ALL, None, None),
                (1, TERMS, [_col(NTILE, arg=I_MIN)], ALL, ALL, None, None), (1, TERMS, [_col(NTH, m, arg=0)], ALL, ALL, None, None), (1, TERMS, [_col(DISC, m, p=-5e-324)], ALL, ALL, None, None),
                (1, TERMS, [_col(DISC, m, p=float(np.nextafter(1.0, 2.0)))], ALL, ALL, None, None), (1, TERMS, [_col(CONT, m, p=float("nan"))], ALL, ALL, None, None),
                (1, TERMS, [_col(CONT, m, p=float("inf"))], ALL, ALL, None, None), (1, TERMS, ok + [_col(NTH, m, arg=0)], ALL, ALL, None, None),
                (1, TERMS, [_col(NTH, (V, 1, True), arg=1)], ALL, ALL, None, None), (1, TERMS, [_col(DISC, (P, 1, False), p=0.5)], ALL, ALL, None, None),
                (1, TERMS, [_col(CONT, (9, 0, False), p=0.5)], ALL, ALL, None, None), (1, TERMS, [_col(NTH, (K, 0, True), arg=1)], ALL, ALL, None, None),
                (1, TERMS, [_col(DISC, (H, 0, True), p=0.5)], ALL, ALL, None, None)):
            assert _raw(ctx, t, 1, npart, terms, cols, per_limit, limit, 700, keys, out, nterms=nterms, ncols=ncols) == (abi.ERR_INVALID, -7), (npart, cols, per_limit, limit, nterms, ncols)
            assert (keys == -7).all() and (out == -7).all()
            good = ctx.table_window_quantile(t, 1, 1, TERMS, ok, 1, ALL, 64)   # a good call succeeds after every one of them
            assert len(good[0]) > 3 and not np.isnan(good[4][0]).any()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_quantile(t, 1, 1, TERMS, [_col(NTILE, arg=0)], ALL, ALL, 64)
        assert e.value.code == abi.ERR_INVALID
        # the functions without a measure ignore whatever theirs names, and arg / p they do not read
        got = ctx.table_window_quantile(t, 1, 1, TERMS, [_col(NTILE, (P, 3, True), arg=2, p=float("nan")), _col(CDIST, (9, 9, True), arg=0, p=7.0)], ALL, ALL, 64)
        assert got[4][0].dtype == np.int64 and set(got[4][0].tolist()) == {1, 2} and got[4][1].max() == 1.0
        assert _check(ctx, t, TERMS, 1, "after the errors", full=False)[0] >= 5      # the context still works
    finally:
        t.free()


# 7. launches ----------------------------------------------------------------------------------------------------------------------------
def test_what_is_launched(hip_engine):
    """A quantile call launches k_wq_* kernels — the tie pass only with CUME_DIST, the RANK pass only with PERCENT_RANK, the place step
    only when per_limit filters — and the six other entry points launch none."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    t = _table(ctx, *_pattern("runs", 2 * T + 1, T, np.random.default_rng(3)))
    m = MEASURES[0]
    ctx.set_profiling(1)
    try:
        def launched(call):
            call()
            return [nm for nm, _ in ctx.profile()]
        q = lambda cols, per_limit=ALL: launched(lambda: ctx.table_window_quantile(t, 1, 1, TERMS, cols, per_limit, ALL, 4096))
        ks = q([_col(CONT, m, p=0.5), _col(NTILE, arg=4)])
        assert [k for k in ks if k.startswith("k_w")] == ["k_win_heads", "k_win_scan", "k_wsl_rows", "k_wagg_next", "k_wq_stage", "k_wq_value"]
        ks = q([_col(CDIST), _col(NTILE, arg=4)])
        assert [k for k in ks if k.startswith("k_w")] == ["k_win_heads", "k_win_scan", "k_wsl_rows", "k_wq_ties", "k_wagg_next", "k_wq_stage", "k_wq_value"]
        ks = q([_col(PRANK)])
        assert [k for k in ks if k.startswith("k_w")] == ["k_win_heads", "k_win_scan", "k_wsl_rows", "k_wagg_next", "k_win_rank", "k_wq_stage", "k_wq_value"]
        ks = q([_col(DISC, m, p=0.9)], 1)
        assert [k for k in ks if k.startswith("k_w")] == ["k_win_heads", "k_win_scan", "k_win_rank", "k_win_place", "k_wsl_rows", "k_wagg_next", "k_wq_stage", "k_wq_value"]
        assert ks.count("k_sort_scan") == 2 and ks[-1] == "k_sort_emit"
        ks = launched(lambda: ctx.table_window_quantile(t, 1, 1, TERMS, [_col(NTILE, arg=4)], ALL, ALL, 4096, want_cols=False))      # rows only, nothing filtered: a plain sort
        assert not [k for k in ks if k.startswith("k_w")] and ks[-1] == "k_sort_emit"
        UP, UF = abi.SLIDE_UNBOUNDED_PRECEDING, abi.SLIDE_UNBOUNDED_FOLLOWING
        others = {
            "sorted": lambda: ctx.table_sorted(t, 1, ALL, TERMS, 4096),
            "sorted_by": lambda: ctx.table_sorted_by(t, 1, ALL, TERMS, 4096),
            "window": lambda: ctx.table_window(t, 1, 1, TERMS, abi.WIN_RANK, 2, ALL, 4096),
            "window_agg": lambda: ctx.table_window_agg(t, 1, 1, TERMS, [(abi.WAGG_SUM, abi.FRAME_RANGE) + m], ALL, 4096),
            "window_slide": lambda: ctx.table_window_slide(t, 1, 1, TERMS, [(abi.WAGG_SUM,) + m + (-2, 0, 0), (abi.WSLIDE_LAST,) + m + (UP, UF, 0)], ALL, 4096),
            "window_range": lambda: ctx.table_window_range(t, 1, 1, TERMS[:2], [(abi.WAGG_SUM,) + m + (abi.WRANGE_VALUE, -2.0, 2.0, 0), (abi.WAGG_COUNT,) + m + (abi.WRANGE_GROUPS, -1, 1, 0)],
                                                           ALL, 4096)}
        for name, call in others.items():
            ks = launched(call)
            assert ks and not [k for k in ks if k.startswith("k_wq")], (name, ks)
    finally:
        ctx.set_profiling(0)
        t.free()


# 8. through the engine and the decorator -------------------------------------------------------------------------------------------------
Q3_COLS = {"med": ("median", "revenue"), "p90": ("percentile_disc", "revenue", 0.9), "q": ("ntile", 4), "cd": ("cume_dist",)}
Q3_NOTE = [["med", "percentile_cont", "revenue", None, 0.5, None], ["p90", "percentile_disc", "revenue", None, 0.9, None], ["q", "ntile", None, 4, None, None],
           ["cd", "cume_dist", None, None, None, None]]
RUN_TO_RUN = 1e-10      # two runs of a query accumulate its sums in another order: what test_window_gpu allows between two runs' rows


def _numpy_q3(dates, x):
    """The four columns of Q3_COLS for rows ordered by (date asc, revenue asc) already, and the partition starts, by numpy."""
    n = len(x)
    pos = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = dates[1:] != dates[:-1]
    tie = head.copy()
    tie[1:] |= x[1:] != x[:-1]
    start, end = np.maximum.accumulate(np.where(head, pos, 0)), _last_of(head)
    m, i = end - start + 1, pos - start
    t = np.float64(0.5) * (m - 1).astype(np.float64)
    lo, hi = np.floor(t), np.ceil(t)
    a, b = x[start + lo.astype(np.int64)], x[start + hi.astype(np.int64)]
    d = b - a
    w = t - lo
    med = np.where(lo == hi, a, a + d * w)
    p90 = x[start + np.maximum(np.ceil(np.float64(0.9) * m.astype(np.float64)).astype(np.int64) - 1, 0)]
    q, r = m // 4, m % 4
    big = r * (q + 1)
    tile = np.where(i < big, i // (q + 1) + 1, r + (i - big) // np.maximum(q, 1) + 1)
    cd = (_last_of(tie) - start + 1).astype(np.float64) / m.astype(np.float64)
    return {"med": med, "p90": p90, "q": tile, "cd": cd}, start


def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    """The revenue of an order is a sum of doubles whose order two runs of the query need not share (RUN_TO_RUN), so between two runs
    — the device route, the host route forced by the switch, order_by + numpy — the measure-valued columns compare within that and the
    rank-valued ones exactly; on the SAME rows (every row returned: the result carries its own measure) device, host route and numpy
    agree bit for bit."""
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "asc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    want_plain, start_plain = _numpy_q3(np.asarray(plain.column("o_orderdate")), np.asarray(plain.column("revenue")))
    firsts = np.nonzero(start_plain == np.arange(len(plain)))[0]

    def close(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return bool(np.allclose(a, b, rtol=RUN_TO_RUN, atol=0.0, equal_nan=True)) if a.dtype.kind == "f" else bool((a == b).all())

    def compare(res, per, route):
        assert eng.stats()["order_routes"][-1] == {"route": route, "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "per_limit": ALL if per is None else per,
                                                   "quantiles": Q3_NOTE}
        assert res.columns == plain.columns + list(Q3_COLS) and [res.column(c).dtype for c in Q3_COLS] == [np.float64, np.float64, np.int64, np.float64]
        rows = np.arange(len(plain)) if per is None else firsts
        assert len(res) == len(rows) > (100 if per is None else 10)
        for c in plain.columns:
            assert close(res.column(c), np.asarray(plain.column(c))[rows]), c
        for c in Q3_COLS:
            assert close(res.column(c), want_plain[c][rows]), (c, per, route)
        if per is None:                                                    # on its own rows: bit for bit, against numpy and against the host route's code
            own, _ = _numpy_q3(np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue")))
            again = ResultSet(plain.columns, [np.asarray(res.column(c)) for c in plain.columns]).quantiles(by, order, Q3_COLS)
            for c in Q3_COLS:
                assert (_bits(res.column(c)) == _bits(own[c].astype(res.column(c).dtype))).all(), (c, route)
                assert (_bits(res.column(c)) == _bits(again.column(c))).all(), (c, route, "host route on the same rows")

    results = {}
    for per in (None, 1):
        results[per] = Q.q3.quantiles(by, order, Q3_COLS, per=per)(*args)
        compare(results[per], per, "window_quantile")
    monkeypatch.setattr(eng, "device_window_quantile", False)
    for per in (None, 1):
        host = Q.q3.quantiles(by, order, Q3_COLS, per=per)(*args)
        compare(host, per, "host")
        for c in host.columns:
            assert close(host.column(c), results[per].column(c)), c
    monkeypatch.setattr(eng, "device_window_quantile", True)
    # a fifth column: on the host, with equal values
    five = dict(Q3_COLS, last=("nth", "revenue", -1))
    wide = Q.q3.quantiles(by, order, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == plain.columns + list(five)
    assert all(close(wide.column(c), results[None].column(c)) for c in Q3_COLS)
    # q16: text fields in a mixed-radix key partition; the count is the measure: exact, whichever run
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    cols16 = {"top": ("nth", "supplier_cnt", 1), "third": ("nth", "supplier_cnt", 3, -1), "mid": ("percentile_disc", "supplier_cnt", 0.5), "avg2": ("median", "supplier_cnt")}
    res = Q.q16.quantiles(["p_brand"], [("supplier_cnt", "desc")], cols16)(*args16)
    route = eng.stats()["order_routes"][-1]
    assert route["route"] == "window_quantile" and route["per"] == ["p_brand"] and route["order"] == ["supplier_cnt"]
    assert [res.column(c).dtype for c in cols16] == [np.int64, np.int64, np.int64, np.float64] and len(res) > 100
    cnt, n = np.asarray(res.column("supplier_cnt")), len(res)
    head = np.ones(n, bool)
    brand = np.asarray(res.column("p_brand"))
    head[1:] = brand[1:] != brand[:-1]
    pos = np.arange(n)
    start, end = np.maximum.accumulate(np.where(head, pos, 0)), _last_of(head)
    m = end - start + 1
    assert (res.column("top") == cnt[start]).all() and (res.column("third") == np.where(m >= 3, cnt[np.minimum(start + 2, n - 1)], -1)).all()
    assert (res.column("mid") == cnt[start + np.maximum(np.ceil(0.5 * m.astype(np.float64)).astype(np.int64) - 1, 0)]).all()
    lo, hi = start + (m - 1) // 2, start + m // 2
    assert (res.column("avg2") == cnt[lo] + (cnt[hi] - cnt[lo]) * np.where(lo == hi, 0.0, 0.5)).all()
    monkeypatch.setattr(eng, "device_window_quantile", False)
    host = Q.q16.quantiles(["p_brand"], [("supplier_cnt", "desc")], cols16)(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    assert all((np.asarray(host.column(c)) == np.asarray(res.column(c))).all() for c in ["p_brand", "supplier_cnt"] + list(cols16))
    monkeypatch.setattr(eng, "device_window_quantile", True)
    # a default no double holds, for a count the table may keep as a double: exact all the same, whichever route takes it
    far = Q.q16.quantiles(["p_brand"], [("supplier_cnt", "desc")], {"x": ("nth", "supplier_cnt", 10 ** 6, (1 << 62) + 1)})(*args16)
    assert (far.column("x") == (1 << 62) + 1).all()
    with pytest.raises(ValueError):                                       # ... and one that does not fit an int64 column is refused by the call
        Q.q16.quantiles(["p_brand"], [("supplier_cnt", "desc")], {"x": ("nth", "supplier_cnt", 1, 0.5)})(*args16)
    with pytest.raises(ValueError):                                       # a text measure: on the host (and refused there: not numeric)
        Q.q16.quantiles(["p_brand"], [("supplier_cnt", "desc")], {"x": ("median", "p_type")})(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_the_switch_forces_the_host_route(hip_lib, db, monkeypatch):
    monkeypatch.setenv("SDQLPY_AMD_DEVICE_WINDOW_QUANTILE", "0")
    eng = engine.Engine(hip_lib.context(device=0))
    try:
        assert eng.device_window_quantile is False
        from sdqlpy_amd import frontend
        from sdqlpy_amd.result import quantile_request
        plan = frontend.lower_function(Q.QUERIES["q3"])
        req = quantile_request(engine.result_columns(plan), ["o_orderdate"], [("revenue", "asc")], Q3_COLS, per=1)
        res = engine.execute_plan(eng, plan, [db[t] for t in Q.QUERY_TABLES["q3"]], req)
        assert eng.stats()["order_routes"][-1]["route"] == "host" and len(res) > 0 and res.columns[-4:] == list(Q3_COLS)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def suppliers():
    from sdqlpy_amd import tpch
    from order_terms_queries import SUPPLIER_COLUMNS, shuffled_suppliers
    plain = tpch.generate(0.05, tables=["supplier"], columns={"supplier": SUPPLIER_COLUMNS})["supplier"]
    return {"plain": plain, "shuffled": shuffled_suppliers(plain)}


def test_a_text_term_goes_through_its_rank_column(on_the_decorator, suppliers):
    """A unique build finished directly whose text payload is row references into s_name: in the generated table they increase with
    the text and the device orders by them as plain numbers, in the shuffled one through a rank table (Engine.rank_column)."""
    from order_terms_queries import suppliers_by_name
    eng = on_the_decorator
    tables = suppliers
    for which, ranked in (("plain", []), ("shuffled", ["s_name"])):
        res = suppliers_by_name.quantiles(["s_nationkey"], [("s_name", "desc")], {"q": ("ntile", 3), "pr": ("percent_rank",), "low": ("nth", "s_suppkey", -1)})(tables[which])
        route = eng.stats()["order_routes"][-1]
        assert route["route"] == "window_quantile" and route["ranked"] == ranked and route["per"] == ["s_nationkey"], (which, route)
        nation, names, key = (np.asarray(res.column(c)) for c in ("s_nationkey", "s_name", "s_suppkey"))
        n = len(res)
        head = np.concatenate(([True], nation[1:] != nation[:-1]))
        pos = np.arange(n)
        start, end = np.maximum.accumulate(np.where(head, pos, 0)), _last_of(head)
        m, i = end - start + 1, pos - start
        assert n > 100 and (names[1:] <= names[:-1])[~head[1:]].all() and (res.column("low") == key[end]).all()
        tie = head.copy()
        tie[1:] |= names[1:] != names[:-1]
        f = np.maximum.accumulate(np.where(tie, pos, 0)) - start
        assert (_bits(res.column("pr")) == _bits(np.where(m == 1, 0.0, f.astype(np.float64) / np.maximum(m - 1, 1).astype(np.float64)))).all()
        q, r = m // 3, m % 3
        big = r * (q + 1)
        assert (res.column("q") == np.where(i < big, i // (q + 1) + 1, r + (i - big) // np.maximum(q, 1) + 1)).all()
