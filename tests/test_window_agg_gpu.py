"""Aggregates over window frames on the MI355X (run with -m gpu): sdqh_table_window_agg (include/sdqh_sort_frames.h) against numpy at
every size at which the sort or the tile scan takes another path, on partition patterns that exercise the carries between tiles in
both directions, on every table layout, over derived terms, on values that would betray a prefix-sum-and-subtract, on general
doubles against the header's error bound, on edge values, against sdqh_table_window and sdqh_table_sorted_by where they overlap,
its argument errors, and through the engine and the decorator.

The expected rows are the table's own K-F rows reordered by a stable numpy lexsort (test_window_gpu's Ranked: order, partition heads,
tie heads).  The aggregates are restated here in numpy: per partition a running fold (int64 cumsum, a running maximum of the
order-preserving images), the ROWS value; RANGE / PARTITION values are the ROWS value of the last row of the tie run / partition.
Nothing is imported from the product's aggregation code."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from test_window_gpu import (EDGE_DOUBLES, EDGE_INTS, PATTERNS, TERMS, Ranked, _pattern, _probed_table, _same, _sizes as _window_sizes, _sort_bits,
                             _stage_rows, _table, _under, db, hip_engine, on_the_decorator)     # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
SUM, COUNT, MIN, MAX = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX
ROWS, RANGE, PARTITION = abi.FRAME_ROWS, abi.FRAME_RANGE, abi.FRAME_PARTITION
OPS, FRAME_KINDS = (SUM, COUNT, MIN, MAX), (ROWS, RANGE, PARTITION)
QNAN = np.uint64(0x7FF8000000000000)
TOP = np.uint64(1) << np.uint64(63)
MEASURES = [(V, 0, True), (H, 0, False), (P, 0, False)]                    # value 0 (a double), the hit count, an integer payload


def _sizes(ctx):
    T, S, sizes = _window_sizes(ctx)
    assert ctx.window_agg_geometry() == T                                  # one tile for ranks and aggregates: the sizes of test_window_gpu are the sizes here
    return T, S, sizes


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _last_of(head):
    """per sorted position: the last position of the run (of `head`s) it lies in"""
    n = len(head)
    at = np.nonzero(head)[0]
    return (np.append(at[1:], n) - 1)[np.cumsum(head) - 1] if n else np.zeros(0, np.int64)


def _seg_cummax(v, start):
    """running maximum of v inside every partition (start: the position its partition starts at), by doubling: after the step of
    distance d a position holds the maximum over the 2d positions ending at it, cut at its partition's start"""
    n, pos, d = len(v), np.arange(len(v)), 1
    while d < n:
        src = v[np.maximum(pos - d, 0)]
        v = np.where((pos - d >= start) & (src > v), src, v)
        d *= 2
    return v


class Framed:
    """A table's rows in the order of `terms`, and the expected aggregates of every sorted position as int64 bit patterns."""

    def __init__(self, rows, terms, npart, rank_tables=None):
        self.rows, self.ref = rows, Ranked(rows, terms, npart, rank_tables)
        self.n, self.order = self.ref.n, self.ref.order
        pos = np.arange(self.n, dtype=np.int64)
        self.start = np.maximum.accumulate(np.where(self.ref.part_head, pos, 0)) if self.n else pos
        self.ends = {RANGE: _last_of(self.ref.tie_head), PARTITION: _last_of(self.ref.part_head)}
        self._memo = {}

    def column(self, kind, index):
        keys, payload, values, hits = self.rows
        return np.asarray({K: lambda: keys, P: lambda: payload[index], V: lambda: values[index], H: lambda: hits}[kind]())[self.order]

    def rows_value(self, op, kind, index, is_f64):
        """The ROWS value of every position.  A SUM of doubles here is of integer-valued doubles below 2^53: exact, through int64."""
        key = (op, kind, index, is_f64) if op != COUNT else (COUNT,)
        if key in self._memo:
            return self._memo[key]
        pos = np.arange(self.n, dtype=np.int64)
        if op == COUNT:
            out = pos - self.start + 1
        elif op == SUM:
            x = self.column(kind, index)
            if is_f64:
                x = x.view(np.float64) if x.dtype != np.float64 else x
                xi = x.astype(np.int64)
                assert (xi == x).all() and (np.abs(xi) < 1 << 40).all()
                x = xi
            c = np.cumsum(x.astype(np.int64)) if self.n else x.astype(np.int64)
            out = c - c[self.start] + x[self.start] if self.n else c         # (int64 wraps: exact modulo 2^64)
            if is_f64:
                out = out.astype(np.float64).view(np.int64)
        else:
            x = self.column(kind, index)
            raw = x.view(np.int64) if x.dtype == np.float64 else x.astype(np.int64)
            img = _sort_bits(raw, is_f64, op == MIN)
            if is_f64:
                img = np.where(np.isnan(raw.view(np.float64)), np.uint64(0), img)
            e = _seg_cummax(img, self.start)
            u = ~e if op == MIN else e
            if is_f64:
                out = np.where(e == 0, QNAN, np.where(u >> np.uint64(63) != 0, u ^ TOP, ~u)).view(np.int64)
            else:
                out = (u ^ TOP).view(np.int64)
        self._memo[key] = out
        return out

    def want(self, agg):
        op, frame, kind, index, is_f64 = agg
        rows = self.rows_value(op, kind, index, is_f64)
        return rows if frame == ROWS else rows[self.ends[frame]]


def _agg(op, frame, measure):
    return (op, frame) + tuple(measure)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _is_f64(agg):
    op, _, kind, _, is_f64 = agg
    return op != COUNT and (kind == V or (kind == P and bool(is_f64)))


def _check(ctx, t, terms, npart, what, aggs_lists, min_hits=1, rank_tables=None, limits=None):
    """Every list of aggregates in one call each: rows and aggregates against numpy, exact by bits; dtypes; the count-only call."""
    rows = _stage_rows(ctx, t, min_hits)
    ref = Framed(rows, terms, npart, rank_tables)
    done = 0
    for i, aggs in enumerate(aggs_lists):
        for limit in (limits(ref.n) if limits and (i == 0 or len(aggs) == 1) else (ALL,)):      # the limits: on the first call of four and on one alone
            got = ctx.table_window_agg(t, min_hits, npart, terms, aggs, limit, 64, want_hits=t.accumulate)
            m = min(limit, ref.n)
            _same(got, rows, ref.order[:m], (what, aggs, limit))
            assert len(got[4]) == len(aggs)
            for a, agg in zip(got[4], aggs):
                assert a.dtype == (np.float64 if _is_f64(agg) else np.int64) and len(a) == m, (what, agg)
                bad = np.nonzero(_bits(a) != ref.want(agg)[:m])[0]
                assert len(bad) == 0, (what, agg, limit, bad[:5], _bits(a)[bad[:5]], ref.want(agg)[bad[:5]])
                done += 1
    assert _raw(ctx, t, min_hits, npart, terms, aggs_lists[0], ALL, 0) == (abi.OK, ref.n), (what, "count")
    return done, ref


def _marshal_aggs(aggs):
    arr = (abi.WindowAgg * max(1, len(aggs)))()
    for a, (op, frame, kind, index, is_f64) in zip(arr, aggs):
        a.op, a.frame, a.kind, a.index, a.is_f64 = op, frame, kind, index, int(bool(is_f64))
    return arr


def _raw(ctx, t, min_hits, npart, terms, aggs, limit, capacity, keys=None, out=None, nterms=None, naggs=None):
    got = C.c_int64(-7)
    rc = ctx.lib.sdqh_table_window_agg(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms),
                                       abi._marshal_sort_terms(terms), C.c_int(len(aggs) if naggs is None else naggs), _marshal_aggs(aggs),
                                       C.c_int64(limit), C.c_int64(capacity), None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                       None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value


def _all_combinations():
    """every op x frame x measure (COUNT once per frame), four to a call, and one alone"""
    combos = [_agg(op, fr, m) for op in (SUM, MIN, MAX) for fr in FRAME_KINDS for m in MEASURES] + [_agg(COUNT, fr, MEASURES[0]) for fr in FRAME_KINDS]
    lists = [combos[i:i + 4] for i in range(0, len(combos), 4)]
    return lists + [[_agg(SUM, RANGE, MEASURES[0])]], len(combos) + 1


def _limits(n):
    return sorted({1, max(1, n // 2), ALL})


# 1. partition patterns x sizes x ops x frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    lists, ncombos = _all_combinations()
    assert ncombos == 3 * 3 * 3 + 3 + 1 and all(1 <= len(l) <= abi.WAGG_MAX_AGGS for l in lists) and len(lists[0]) == 4
    for n in sizes:
        t = _table(ctx, *_pattern(pattern, n, T, rng))
        try:
            done, ref = _check(ctx, t, TERMS, 1, (pattern, n), lists, limits=_limits)
            assert done >= ncombos and ref.n == n
            if pattern == "a long partition" and n == 70001:              # a tile with no head of either kind: the carry passes through, forwards and backwards
                tiles = ref.ref.tie_head[:(n // T) * T].reshape(-1, T)
                assert (~tiles.any(axis=1)).any()
            if pattern == "one partition" and n == 70001:                 # ... and tiles with tie heads but no partition head
                assert ref.ref.part_head.sum() == 1 and ref.ref.tie_head[T:2 * T].any()
            if n:                                                          # a capacity one too small: the needed count, nothing written
                keys, out = np.full(n, -7, np.int64), np.full((4, n), -7, np.int64)
                assert _raw(ctx, t, 1, 1, TERMS, lists[0], ALL, n - 1, keys, out) == (abi.ERR_OVERFLOW, n)
                assert (keys == -7).all() and (out == -7).all()
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
    lists = [[_agg(SUM, RANGE, MEASURES[0]), _agg(MAX, ROWS, MEASURES[1]), _agg(COUNT, PARTITION, MEASURES[0]), _agg(MIN, PARTITION, MEASURES[2])]]

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        try:
            return sum(_check(ctx, t, TERMS, 1, ("layout", dups, mh), lists, min_hits=mh, limits=_limits)[0] for mh in (0, 1, 2))
        finally:
            t.free()
    assert run(0) >= 3 * 4 * 2
    assert run(200) >= 3 * 4 * 2
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) >= 3 * 4 * 2
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
        xl = [[_agg(SUM, RANGE, (V, 0, True)), _agg(SUM, ROWS, (K, 0, False)), _agg(MAX, PARTITION, (H, 0, False)), _agg(MIN, RANGE, (K, 0, False))]]
        for mh in (0, 1, 2):
            assert _check(ctx, t, terms, 1, ("xbuild", mh), xl, min_hits=mh)[0] >= 4
    finally:
        t.free()


# 3. derived terms -----------------------------------------------------------------------------------------------------------------------
def test_derived_terms(hip_engine):
    """PARTITION BY the high half of a packed key ORDER BY its low half descending, then a text-ranked payload; the measure is the plain
    payload (a measure has no derivation: sdqh_window_agg has no field for one).  A ranks column too short is SDQH_ERR_INVALID
    naming the term, with nothing written, *out_n included."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    assert [f for f, _ in abi.WindowAgg._fields_] == ["op", "frame", "kind", "index", "is_f64", "_pad"]
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    short = ctx.upload(want[:20])
    m = (P, 0, False)
    lists = [[_agg(SUM, ROWS, m), _agg(MIN, RANGE, m), _agg(MAX, PARTITION, m), _agg(COUNT, RANGE, m)], [_agg(SUM, PARTITION, (K, 0, False))]]
    try:
        for n in (T + 1, S + 1, 5 * T + 17):
            a = rng.integers(0, n // 90 + 2, n).astype(np.int64)
            b = rng.integers(0, 3000, n).astype(np.int64)
            keys = np.unique((a << 32) | b)
            keys = keys[rng.permutation(len(keys))]
            ref_col = rng.integers(0, len(text), len(keys)).astype(np.int64)
            t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ref_col)], accumulate=False)
            try:
                terms = [(K, 0, False, False, 1 << 32, 0, 0, None), (K, 0, True, False, 16, 1 << 28, 0, None), (P, 0, False, False, 0, 0, 0, ct)]
                assert _check(ctx, t, terms, 1, ("derived", n), lists, min_hits=0, rank_tables={id(ct): want}, limits=_limits)[0] >= 5
                bad = terms[:2] + [(P, 0, False, False, 0, 0, 0, short)]
                out, aggs = np.full(len(keys), -7, np.int64), np.full((4, len(keys)), -7, np.int64)
                assert _raw(ctx, t, 0, 1, bad, lists[0], ALL, len(keys), out, aggs) == (abi.ERR_INVALID, -7) and (out == -7).all() and (aggs == -7).all()
                assert b"term 2" in ctx.lib.sdqh_last_error(ctx.handle)
            finally:
                t.free()
    finally:
        ct.free(); short.free()


# 4. nothing leaks across partitions, nothing is subtracted --------------------------------------------------------------------------------
def _payload_table(ctx, part, dbls, ints=None, seed=3):
    """entries with payload 0 = part, payload 1 = the bits of dbls (and payload 2 = ints), in random build order"""
    n = len(part)
    keys = np.random.default_rng(seed + n).permutation(n).astype(np.int64) * 3 - n
    cols = [ctx.upload(np.asarray(part, np.int64)), ctx.upload(np.ascontiguousarray(dbls, np.float64).view(np.int64))] + ([] if ints is None else [ctx.upload(ints)])
    return ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), cols, accumulate=False)


def test_no_leak_and_no_subtraction(hip_engine):
    """Partitions alternate between values near +-1e300 and small integers.  A sum that carried anything over a partition head, or
    that took a global prefix sum and subtracted the partition's start, loses the small values (1e300 + 3 - 1e300 = 0): every small
    partition's sums must be exact, in every frame."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    for n in (2 * T + 1, 5 * T + 17):
        rng = np.random.default_rng(n)
        part = np.arange(n) // 37
        small = part % 2 == 1
        dbls = np.where(small, rng.integers(-9, 10, n).astype(np.float64), rng.choice([-1.0, 1.0], n) * (1e300 + rng.integers(0, 1000, n) * 1e290))
        mix = rng.permutation(n)
        t = _payload_table(ctx, part[mix], dbls[mix])
        try:
            terms = [(P, 0, False, False), (K, 0, False, False)]
            rows = _stage_rows(ctx, t, 0)
            ref = Framed(rows, terms, 1)
            x = ref.column(P, 1).view(np.float64)
            sm = (ref.column(P, 0) % 2 == 1)
            assert sm.any() and (~sm).any() and (np.abs(x[~sm]) >= 1e300).all()
            xi = np.where(sm, x, 0.0).astype(np.int64)                     # the small partitions' sums, exactly
            c = np.cumsum(xi)
            want_rows = (c - c[ref.start] + xi[ref.start]).astype(np.float64)
            m = (P, 1, True)
            got = ctx.table_window_agg(t, 0, 1, terms, [_agg(SUM, ROWS, m), _agg(SUM, RANGE, m), _agg(SUM, PARTITION, m)], ALL, n, want_hits=False)
            _same(got, rows, ref.order, ("leak", n))
            for a, want in zip(got[4], (want_rows, want_rows[ref.ends[RANGE]], want_rows[ref.ends[PARTITION]])):
                assert a.dtype == np.float64 and (a[sm] == want[sm]).all(), (n, np.nonzero(a[sm] != want[sm])[0][:5])
            assert np.isfinite(got[4][0]).all() and (np.abs(got[4][0][~sm]) >= 1e299).any()
        finally:
            t.free()


# 5. general doubles -----------------------------------------------------------------------------------------------------------------------
def _frame_guarantees(ref, rows, rng_, part, what):
    """all rows of a tie run share one RANGE value = the ROWS value at the run's last row; all rows of a partition share one PARTITION
    value = the ROWS value at the partition's last row: bit for bit"""
    assert (_bits(rng_) == _bits(rows)[ref.ends[RANGE]]).all(), (what, "range")
    assert (_bits(part) == _bits(rows)[ref.ends[PARTITION]]).all(), (what, "partition")


def test_general_doubles_within_the_bound(hip_engine):
    """Values k * 2^-20 with |value| < 2^40: exact sums are integer sums of the k.  Every SUM lies within the header's bound
    gamma * sum|v|, gamma = (m - 1) u / (1 - (m - 1) u), u = 2^-53, m the frame's rows; the four frame guarantees hold bit for bit for
    every op; two calls return identical bits."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    u = Fraction(1, 1 << 53)
    for n, lengths in ((2 * T + 1, [200, 3, 64, 65, 1]), (5 * T + 17, [5 * T + 17]), (S + 1, [T + 9, 7])):
        rng = np.random.default_rng(n)
        k = rng.integers(-(1 << 59), 1 << 59, n)
        k[rng.integers(0, n, n // 3)] >>= 30                                # magnitudes spread over thirty binades: sums that round
        dbls = k.astype(np.float64) / float(1 << 20)
        assert (dbls * float(1 << 20) == k.astype(np.float64)).all() and (np.abs(dbls) < float(1 << 40)).all()
        part = np.zeros(n, np.int64)
        at = g = 0
        while at < n:
            part[at:at + lengths[g % len(lengths)]] = g
            at += lengths[g % len(lengths)]; g += 1
        tie = rng.integers(0, max(2, n // 3), n)                            # order by this: ties of about three rows
        mix = rng.permutation(n)
        t = _payload_table(ctx, part[mix], dbls[mix], tie[mix])
        try:
            terms = [(P, 0, False, False), (P, 2, True, False)]
            rows = _stage_rows(ctx, t, 0)
            ref = Framed(rows, terms, 1)
            assert (ref.ends[RANGE] > np.arange(n)).any() and (ref.ends[RANGE] < ref.ends[PARTITION]).any()
            m = (P, 1, True)
            calls = [[_agg(op, fr, m) for fr in FRAME_KINDS] for op in OPS]
            for aggs in calls:
                got = ctx.table_window_agg(t, 0, 1, terms, aggs, ALL, n, want_hits=False)
                again = ctx.table_window_agg(t, 0, 1, terms, aggs, ALL, 64, want_hits=False)
                _same(got, rows, ref.order, ("general", n))
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(got[4], again[4])), (n, aggs[0][0], "two calls differ")
                _frame_guarantees(ref, got[4][0], got[4][1], got[4][2], (n, aggs[0][0]))
                if aggs[0][0] in (MIN, MAX, COUNT):                         # exact
                    assert (_bits(got[4][0]) == ref.want(aggs[0])).all(), (n, aggs[0][0])
            # SUM / ROWS against the exact sums (Python integers), within gamma * sum|v|; the other frames are copies of these (above)
            sums = ctx.table_window_agg(t, 0, 1, terms, calls[0], ALL, n, want_hits=False)[4][0]
            ks = np.rint(ref.column(P, 1).view(np.float64) * float(1 << 20)).astype(np.int64).tolist()
            exact = mag = cnt = 0
            worst = Fraction(0)
            for i in range(n):
                if ref.ref.part_head[i]:
                    exact = mag = cnt = 0
                exact += ks[i]; mag += abs(ks[i]); cnt += 1
                gamma = (cnt - 1) * u / (1 - (cnt - 1) * u)
                err = abs(Fraction(float(sums[i])) * (1 << 20) - exact)
                assert err <= gamma * mag, (n, i, cnt, float(err), float(gamma * mag))
                worst = max(worst, err / mag if mag else Fraction(0))
            print("general doubles n=%d: worst |err| / sum|v| = %.3g (bound at the longest frame %.3g)" % (n, float(worst), float((max(lengths) - 1) * u)))
        finally:
            t.free()


# 6. edge values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 2600])
def test_edge_values(hip_engine, n):
    """+-0.0, +-inf, two NaN bit patterns, DBL_MAX, INT64_MIN / MAX as measures and as partition terms.  MIN / MAX exact by bits (-0.0
    below +0.0, NaNs skipped, a frame of NaNs only: the quiet NaN); integer SUM wraps like numpy's int64; double SUM: the frame
    guarantees, and partitions without inf / NaN exact — their values are +-0.0, 1.0 and DBL_MAX, all of one sign or zero, whose sum
    is the same in every association (DBL_MAX absorbs the ones; two DBL_MAX overflow to inf whatever the order), so numpy's cumsum
    in row order is the expected value bit for bit."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) * 3 - n
    ints = np.resize(EDGE_INTS, n)[rng.permutation(n)]
    dbls = np.resize(EDGE_DOUBLES, n)[rng.permutation(n)]
    t = ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ints), ctx.upload(dbls.view(np.int64))], accumulate=False)
    mi, md = (P, 0, False), (P, 1, True)
    exact = [[_agg(MIN, fr, md) for fr in FRAME_KINDS] + [_agg(SUM, RANGE, mi)], [_agg(MAX, fr, md) for fr in FRAME_KINDS] + [_agg(SUM, ROWS, mi)],
             [_agg(MIN, ROWS, mi), _agg(MAX, RANGE, mi), _agg(SUM, PARTITION, mi), _agg(COUNT, RANGE, mi)], [_agg(MAX, PARTITION, mi), _agg(MIN, PARTITION, mi)]]
    try:
        done = 0
        for terms, npart in (([(P, 1, False, True), (P, 0, True, False)], 1), ([(P, 0, False, False), (P, 1, True, True)], 1),
                             ([(P, 1, True, True), (P, 0, False, False)], 2), ([(P, 1, False, True)], 0), ([(P, 0, True, False)], 0),
                             ([(K, 0, False, False, 0, 5, 0, None), (P, 0, False, False)], 1)):
            with np.errstate(over="ignore"):
                d, ref = _check(ctx, t, terms, npart, ("edge", terms, npart), exact, min_hits=0)
            done += d
            if terms[0][:2] == (P, 1) and npart == 1:                       # eight different doubles under the total order: a partition of NaNs only exists
                x = ref.column(P, 1).view(np.float64)
                assert ref.ref.part_head.sum() == 8 and np.isnan(x[ref.ends[PARTITION] == ref.ends[PARTITION][np.nonzero(np.isnan(x))[0][0]]]).all()
            got = ctx.table_window_agg(t, 0, npart, terms, [_agg(SUM, fr, md) for fr in FRAME_KINDS], ALL, n, want_hits=False)
            _frame_guarantees(ref, got[4][0], got[4][1], got[4][2], ("edge sum", terms))
            x = ref.column(P, 1).view(np.float64)
            starts = np.nonzero(ref.ref.part_head)[0]
            checked = 0
            for a, b in zip(starts, np.append(starts[1:], n)):
                if np.isfinite(x[a:b]).all():
                    with np.errstate(over="ignore"):
                        assert (_bits(got[4][0][a:b]) == _bits(np.cumsum(x[a:b]))).all(), ("edge sum", terms, a, b)
                    checked += 1
            assert checked or npart == 0 or terms[0][:2] != (P, 1)
        assert done >= 6 * 14
    finally:
        t.free()


# 7. agreement -------------------------------------------------------------------------------------------------------------------------
def test_agreement_with_window_and_sorted_by(hip_engine):
    """COUNT / ROWS is sdqh_table_window's ROW_NUMBER; COUNT / RANGE minus the tie run's length plus 1 is its RANK; the rows are
    sdqh_table_sorted_by's rows bit for bit."""
    from test_order_by_gpu import SPECS
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    done = 0
    for n in (S - 1, 5 * T + 17):
        t = _probed_table(ctx, n)
        try:
            for spec in SPECS:
                for min_hits in (0, 2):
                    want = ctx.table_sorted_by(t, min_hits, ALL, spec, n)
                    for npart in sorted({0, 1, len(spec)}):
                        got = ctx.table_window_agg(t, min_hits, npart, spec, [_agg(COUNT, ROWS, MEASURES[0]), _agg(COUNT, RANGE, MEASURES[0])], ALL, n)
                        assert all((_bits(g) == _bits(w)).all() for g, w in zip(got[:4], want))
                        rn = ctx.table_window(t, min_hits, npart, spec, abi.WIN_ROW_NUMBER, ALL, ALL, n)[4]
                        rk = ctx.table_window(t, min_hits, npart, spec, abi.WIN_RANK, ALL, ALL, n)[4]
                        assert (got[4][0] == rn).all()
                        head = np.nonzero(rn == rk)[0]                      # a tie run's first row: its row number is its rank
                        run = np.append(head[1:], len(rn)) - head           # ... and the run ends where the next starts
                        assert (got[4][1][head] - run + 1 == rk[head]).all() and (got[4][1] - np.repeat(run, run) + 1 == rk).all()
                        done += 1
        finally:
            t.free()
    assert done >= 2 * 5 * 2 * 2


# 8. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(hip_engine):
    ctx = hip_engine.ctx
    t = _table(ctx, *_pattern("runs", 700, 512, np.random.default_rng(3)))
    ok = [_agg(SUM, RANGE, MEASURES[0])]
    try:
        keys, out = np.full(700, -7, np.int64), np.full((5, 700), -7, np.int64)
        for npart, terms, aggs, limit, nterms, naggs in (
                (1, TERMS, ok, 0, None, None), (-1, TERMS, ok, ALL, None, None), (4, TERMS, ok, ALL, None, None), (0, TERMS, ok, ALL, 0, None),
                (1, [TERMS[0]] * 9, ok, ALL, None, None), (1, [(P, 1, False, False)], ok, ALL, None, None), (1, [(V, 0, False, True, 2, 0, 0, None)], ok, ALL, None, None),
                (1, TERMS, ok, ALL, None, 0), (1, TERMS, ok * 5, ALL, None, None), (1, TERMS, [(7, RANGE, V, 0, True)], ALL, None, None),
                (1, TERMS, [(-1, RANGE, V, 0, True)], ALL, None, None), (1, TERMS, [(SUM, 3, V, 0, True)], ALL, None, None), (1, TERMS, [(SUM, -1, V, 0, True)], ALL, None, None),
                (1, TERMS, [(SUM, ROWS, V, 1, True)], ALL, None, None), (1, TERMS, [(MAX, ROWS, P, 1, False)], ALL, None, None), (1, TERMS, [(MIN, ROWS, 9, 0, False)], ALL, None, None),
                (1, TERMS, [(SUM, ROWS, K, 0, True)], ALL, None, None), (1, TERMS, [(MAX, RANGE, H, 0, True)], ALL, None, None)):
            assert _raw(ctx, t, 1, npart, terms, aggs, limit, 700, keys, out, nterms=nterms, naggs=naggs) == (abi.ERR_INVALID, -7), (npart, aggs, limit, nterms, naggs)
            assert (keys == -7).all() and (out == -7).all()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_agg(t, 1, 1, TERMS, [(7, RANGE, V, 0, True)], ALL, 64)
        assert e.value.code == abi.ERR_INVALID
        # COUNT ignores its measure, whatever it names
        got = ctx.table_window_agg(t, 1, 1, TERMS, [(COUNT, PARTITION, P, 3, True)], ALL, 64)
        assert got[4][0].dtype == np.int64 and got[4][0].min() >= 1
        lists, ncombos = _all_combinations()
        assert _check(ctx, t, TERMS, 1, "after the errors", lists)[0] == ncombos      # the context still works
    finally:
        t.free()


# 9. through the engine and the decorator -------------------------------------------------------------------------------------------------
def _numpy_over(res, by, order, aggs):
    """The aggregate columns of a result set's own rows (which must be in order already), by numpy: {name: (values, exact?)} — sums of
    doubles are np.cumsum per partition in row order (not exact: compared within the header's bound), everything else is exact."""
    cols = []
    for name, d in [(b, "asc") for b in by] + list(order):
        a = np.asarray(res.column(name))
        if a.dtype.kind not in "if":
            a = np.unique(a, return_inverse=True)[1].reshape(-1).astype(np.int64)
        u = _sort_bits(a.astype(np.float64 if a.dtype.kind == "f" else np.int64), a.dtype.kind == "f", d == "desc")
        cols.append((u ^ TOP).view(np.int64))
    n = len(res)
    ref = Framed((np.arange(n), cols, None, None), [(P, i, False, False) for i in range(len(cols))], len(by))
    assert (ref.order == np.arange(n)).all()                               # sorted already: a stable sort leaves the rows
    starts = np.nonzero(ref.ref.part_head)[0]
    out = {}
    for name, (op, col, frame) in aggs.items():
        x = None if col is None else np.asarray(res.column(col))
        if op == "count":
            rows = np.arange(n) - ref.start + 1
        elif op == "sum":
            rows = np.empty(n, x.dtype if x.dtype.kind == "f" else np.int64)
            for a, b in zip(starts, np.append(starts[1:], n)):
                rows[a:b] = np.cumsum(x[a:b])
        else:                                                              # (a query result holds no NaN and no -0.0: numpy's own order will do)
            assert not (x.dtype.kind == "f" and (np.isnan(x).any() or (np.signbit(x) & (x == 0)).any()))
            rows = np.empty_like(x)
            for a, b in zip(starts, np.append(starts[1:], n)):
                rows[a:b] = (np.minimum if op == "min" else np.maximum).accumulate(x[a:b])
        frame_id = {"rows": ROWS, "range": RANGE, "partition": PARTITION}[frame]
        out[name] = (rows if frame_id == ROWS else rows[ref.ends[frame_id]], not (op == "sum" and x.dtype.kind == "f"), ref)
    return out


RUN_TO_RUN = 1e-10      # two runs of a query accumulate its sums in another order: what test_window_gpu allows between two runs' rows


def _within_bound(got, want, x, ref, slack=0.0):
    """|got - want| <= 2 * gamma * sum|v| over the partition: both sides are IEEE sums of the frame's rows, each within gamma * sum|v| of
    exact (slack: what the measure itself may differ by, relative, when the two sides come from two runs of the query)"""
    starts = np.nonzero(ref.ref.part_head)[0]
    mag = np.empty(len(x))
    for a, b in zip(starts, np.append(starts[1:], len(x))):
        mag[a:b] = np.abs(x[a:b]).sum()
    m = (ref.ends[PARTITION] - ref.start + 1).astype(np.float64)
    u = 2.0 ** -53
    return (np.abs(got - want) <= (2 * (m * u / (1 - m * u)) + slack) * mag).all()


Q3_AGGS = {"running": ("sum", "revenue"), "day_total": ("sum", "revenue", "partition"), "n": ("count", None, "partition"), "best": ("max", "revenue", "rows")}


def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    full = {k: (v + ("range",))[:3] for k, v in Q3_AGGS.items()}

    def compare(res):
        assert res.columns == plain.columns + list(Q3_AGGS) and len(res) == len(plain) > 100
        assert [res.column(c).dtype for c in Q3_AGGS] == [np.float64, np.float64, np.int64, np.float64]
        want = _numpy_over(res, by, order, full)
        for name, (w, exact, ref) in want.items():
            g = res.column(name)
            assert (g == w).all() if exact else _within_bound(g, w, np.asarray(res.column("revenue")), ref), name
        ref = want["running"][2]
        assert (_bits(res.column("running")) == _bits(res.column("running"))[ref.ends[RANGE]]).all()      # peers are equal
        assert (_bits(res.column("day_total")) == _bits(res.column("day_total"))[ref.ends[PARTITION]]).all()
        return want

    dev = Q.q3.over(by, order, Q3_AGGS)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "window_agg", "k": ALL, "order": ["revenue"], "ranked": [], "per": by,
                                               "aggs": [[k] + list(v) for k, v in full.items()]}
    compare(dev)
    monkeypatch.setattr(eng, "device_window_agg", False)
    host = Q.q3.over(by, order, Q3_AGGS)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["aggs"] == [[k] + list(v) for k, v in full.items()]
    want = compare(host)
    def close(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return bool(np.allclose(a, b, rtol=RUN_TO_RUN, atol=0.0)) if a.dtype.kind == "f" else bool((a == b).all())
    for c in plain.columns:
        assert close(host.column(c), dev.column(c)), c
    for name, (_, exact, ref) in want.items():
        g, h = dev.column(name), host.column(name)
        assert close(g, h) if exact else _within_bound(g, h, np.asarray(host.column("revenue")), ref, RUN_TO_RUN), name
    monkeypatch.setattr(eng, "device_window_agg", True)
    # more than four aggregates: on the host
    five = dict(Q3_AGGS, least=("min", "revenue", "rows"))
    wide = Q.q3.over(by, order, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == plain.columns + list(five)
    assert close(wide.column("n"), dev.column("n")) and close(wide.column("best"), dev.column("best"))
    # q16: text fields in a mixed-radix key partition, the count is the measure: exact
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    res = Q.q16.over(["p_brand"], [("supplier_cnt", "desc")], {"brand_total": ("sum", "supplier_cnt", "partition")})(*args16)
    route = eng.stats()["order_routes"][-1]
    assert route["route"] == "window_agg" and route["per"] == ["p_brand"] and route["aggs"] == [["brand_total", "sum", "supplier_cnt", "partition"]]
    assert res.column("brand_total").dtype == np.int64 and len(res) > 100
    w, exact, _ = _numpy_over(res, ["p_brand"], [("supplier_cnt", "desc")], {"brand_total": ("sum", "supplier_cnt", "partition")})["brand_total"]
    assert exact and (res.column("brand_total") == w).all()
    # a text measure: on the host (and refused there: not numeric)
    with pytest.raises(ValueError):
        Q.q16.over(["p_brand"], [("supplier_cnt", "desc")], {"x": ("max", "p_type")})(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]
