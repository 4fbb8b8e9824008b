"""Sliding window frames on the MI355X (run with -m gpu): sdqh_table_window_slide (include/sdqh_sort_slide.h) against numpy at every
size at which the sort or the tile scan takes another path, at frame widths around the wave, the tile and the table, on partition
patterns that exercise the carries between tiles in both directions, on every table layout, over derived terms, on values that would
betray a prefix-sum-and-subtract, on general doubles against the header's error bound, on edge values, against
sdqh_table_window_agg / sdqh_table_window / sdqh_table_sorted_by where they overlap, at extreme offsets, its argument errors, and
through the engine and the decorator.

The expected rows are the table's own K-F rows reordered by a stable numpy lexsort (test_window_gpu's Ranked).  The values are restated
here in numpy: the frame of position j in the partition [s, e] is [max(j + lo, s), min(j + hi, e)]; COUNT is arithmetic, FIRST / LAST
gather, an integer SUM is a difference of wrapping prefix sums (fine in a reference), MIN / MAX query a doubling table of the
order-preserving images.  Nothing is imported from the product's fold code."""
import ctypes as C
import struct
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
SUM, COUNT, MIN, MAX, FIRST, LAST = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WSLIDE_FIRST, abi.WSLIDE_LAST
OPS = (SUM, COUNT, MIN, MAX, FIRST, LAST)
UP, UF = abi.SLIDE_UNBOUNDED_PRECEDING, abi.SLIDE_UNBOUNDED_FOLLOWING
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
QNAN = np.uint64(0x7FF8000000000000)
TOP = np.uint64(1) << np.uint64(63)
MEASURES = [(V, 0, True), (H, 0, False), (P, 0, False)]                    # value 0 (a double), the hit count, an integer payload
NAN_BITS = struct.unpack("<q", struct.pack("<d", float("nan")))[0]
NEG_ZERO_BITS = I_MIN                                                      # the bits of -0.0
EMPTIES = (0, -1, I_MIN, NAN_BITS, NEG_ZERO_BITS)


def _sizes(ctx):
    T, S, sizes = _window_sizes(ctx)
    tile, narrow = ctx.window_slide_geometry()
    assert tile == ctx.window_geometry() == T and narrow >= 0              # one tile for ranks, aggregates and slides
    return T, S, sizes, narrow


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _last_of(head):
    n = len(head)
    at = np.nonzero(head)[0]
    return (np.append(at[1:], n) - 1)[np.cumsum(head) - 1] if n else np.zeros(0, np.int64)


class Slid:
    """A table's rows in the order of `terms`, and the expected value of every slide at every sorted position as int64 bit patterns."""

    def __init__(self, rows, terms, npart, rank_tables=None):
        self.rows, self.ref = rows, Ranked(rows, terms, npart, rank_tables)
        self.n, self.order = self.ref.n, self.ref.order
        self.pos = np.arange(self.n, dtype=np.int64)
        self.start = np.maximum.accumulate(np.where(self.ref.part_head, self.pos, 0)) if self.n else self.pos
        self.end = _last_of(self.ref.part_head)
        self._tables = {}

    def column(self, kind, index):
        keys, payload, values, hits = self.rows
        return np.asarray({K: lambda: keys, P: lambda: payload[index], V: lambda: values[index], H: lambda: hits}[kind]())[self.order]

    def raw(self, kind, index):
        x = self.column(kind, index)
        return np.ascontiguousarray(x).view(np.int64) if x.dtype == np.float64 else x.astype(np.int64)

    def frame(self, lo, hi):
        """(first position, last position, empty?) of every position's frame; offsets beyond the table reach outside every partition"""
        lo, hi = max(-self.n - 1, min(self.n + 1, lo)), max(-self.n - 1, min(self.n + 1, hi))
        left, right = np.maximum(self.pos + lo, self.start), np.minimum(self.pos + hi, self.end)
        return left, right, left > right

    def _levels(self, op, kind, index, is_f64):
        """level t, position i: the unsigned maximum of the images of positions [i, i + 2^t) (cut at the table's end)"""
        key = (op, kind, index, is_f64)
        if key not in self._tables:
            raw = self.raw(kind, index)
            img = _sort_bits(raw, is_f64, op == MIN)
            if is_f64:
                img = np.where(np.isnan(raw.view(np.float64)), np.uint64(0), img)
            levels, d = [img], 1
            while d < self.n:
                prev = levels[-1]
                levels.append(np.maximum(prev, prev[np.minimum(self.pos + d, self.n - 1)]))
                d *= 2
            self._tables[key] = np.stack(levels) if self.n else np.zeros((1, 0), np.uint64)
        return self._tables[key]

    def want(self, slide):
        op, kind, index, is_f64, lo, hi, empty = slide
        left, right, emp = self.frame(lo, hi)
        if op == COUNT:
            return np.where(emp, 0, right - left + 1).astype(np.int64)
        is_f64 = kind == V or (kind == P and bool(is_f64))
        a, b = np.where(emp, self.pos, left), np.where(emp, self.pos, right)
        raw = self.raw(kind, index)
        if op in (FIRST, LAST):
            v = raw[a] if op == FIRST else raw[b]
        elif op == SUM:                                                    # a SUM of doubles here is of integer-valued doubles below 2^53: exact, through int64
            x = raw
            if is_f64:
                xf = raw.view(np.float64)
                x = xf.astype(np.int64)
                assert (x == xf).all() and (np.abs(x) < 1 << 40).all()
            c = np.concatenate((np.zeros(1, np.uint64), np.cumsum(x.view(np.uint64), dtype=np.uint64)))
            v = (c[b + 1] - c[a]).view(np.int64)                           # (wraps: exact modulo 2^64)
            if is_f64:
                v = v.astype(np.float64).view(np.int64)
        else:
            levels = self._levels(op, kind, index, is_f64)
            k = np.frexp((b - a + 1).astype(np.float64))[1] - 1            # floor(log2(rows in the frame))
            e = np.maximum(levels[k, a], levels[k, b - (np.int64(1) << k) + 1]) if self.n else np.zeros(0, np.uint64)
            u = ~e if op == MIN else e
            if is_f64:
                v = np.where(e == 0, QNAN, np.where(u >> np.uint64(63) != 0, u ^ TOP, ~u)).view(np.int64)
            else:
                v = (u ^ TOP).view(np.int64)
        return np.where(emp, np.int64(empty), v)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _is_f64(slide):
    op, kind, _, is_f64 = slide[:4]
    return op != COUNT and (kind == V or (kind == P and bool(is_f64)))


def _widths(n, T, narrow):
    return [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, max(n, 1) + 2] + ([narrow, narrow + 1] if narrow > 0 else [])


def _frames(n, T, narrow):
    """every width ending at the row, starting at it, centred, all preceding and all following; LAG / LEAD as one-row frames"""
    out = []
    for w in _widths(n, T, narrow):
        p = w - 1
        out += [(-p, 0), (0, p), (-(p // 2), p - p // 2), (-p - 2, -2), (3, p + 3)]
    return out + [(-d, -d) for d in (1, 63, 64, T, T + 1)] + [(d, d) for d in (1, 63, 64, T, T + 1)]


def _slide_lists(n, T, narrow, shift=0):
    """Every frame of _frames once, the ops, measures and defaults rotating over them (`shift` moves the rotation: over the sizes of
    a test every op meets every kind of frame), four to a call, and one alone; LAG / LEAD are FIRST.

    This is a reduction of the full product ops x frames at every size, which would be some 400 slides per size and pattern: at one
    size a frame is folded by ONE op over one measure with one default.  What is kept: every frame (every width in all five
    positions, every LAG / LEAD distance) at every size and pattern; every op on every kind of frame over the sizes of a pattern
    (asserted: `met`); and, since the op only selects the fold while the frame arithmetic, the block heads and the carries are
    shared by all ops, every path through the kernels at every size.  What is not: each op at each width at each size."""
    frames = _frames(n, T, narrow)
    slides = []
    for i, (lo, hi) in enumerate(frames):
        op = FIRST if lo == hi and lo != 0 else OPS[(i + shift) % len(OPS)]
        slides.append((op,) + MEASURES[(i // 2 + shift) % len(MEASURES)] + (lo, hi, EMPTIES[(i + shift) % len(EMPTIES)]))
    lists = [slides[i:i + 4] for i in range(0, len(slides), 4)]
    return lists + [[(SUM,) + MEASURES[0] + (-2, 0, -1)]], len(slides) + 1


LIMITS_EVERYWHERE = 1100      # rows up to which _check runs every limit on every call (all sizes of _sizes but the largest)


def _limits(n):
    return sorted({1, max(1, n // 2), ALL})


def _check(ctx, t, terms, npart, what, slide_lists, min_hits=1, rank_tables=None, limits=None):
    """Every list of slides in one call each: rows and values against numpy, exact by bits; dtypes; the count-only call.  A limit cuts
    the rows returned, never the frames: the expected values are the first m of the whole table's."""
    rows = _stage_rows(ctx, t, min_hits)
    ref = Slid(rows, terms, npart, rank_tables)
    done = 0
    for i, slides in enumerate(slide_lists):
        # the limits: on every call while the table is small (a few tiles), beyond that on the first call of four and on one alone
        for limit in (limits(ref.n) if limits and (i == 0 or len(slides) == 1 or ref.n <= LIMITS_EVERYWHERE) else (ALL,)):
            got = ctx.table_window_slide(t, min_hits, npart, terms, slides, limit, 64, want_hits=t.accumulate)
            m = min(limit, ref.n)
            _same(got, rows, ref.order[:m], (what, slides, limit))
            assert len(got[4]) == len(slides)
            for a, slide in zip(got[4], slides):
                assert a.dtype == (np.float64 if _is_f64(slide) else np.int64) and len(a) == m, (what, slide)
                want = ref.want(slide)[:m]
                bad = np.nonzero(_bits(a) != want)[0]
                assert len(bad) == 0, (what, slide, limit, bad[:5], _bits(a)[bad[:5]], want[bad[:5]])
                done += 1
    assert _raw(ctx, t, min_hits, npart, terms, slide_lists[0], ALL, 0) == (abi.OK, ref.n), (what, "count")
    return done, ref


def _marshal(slides):
    arr = (abi.WindowSlide * max(1, len(slides)))()
    for a, (op, kind, index, is_f64, lo, hi, empty) in zip(arr, slides):
        a.op, a.kind, a.index, a.is_f64, a.lo, a.hi, a.empty = op, kind, index, int(bool(is_f64)), lo, hi, empty
    return arr


def _raw(ctx, t, min_hits, npart, terms, slides, limit, capacity, keys=None, out=None, nterms=None, nslides=None):
    got = C.c_int64(-7)
    rc = ctx.lib.sdqh_table_window_slide(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms),
                                         abi._marshal_sort_terms(terms), C.c_int(len(slides) if nslides is None else nslides), _marshal(slides),
                                         C.c_int64(limit), C.c_int64(capacity), None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                         None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value


# 1. partition patterns x sizes x ops x frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes, narrow = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    met = set()
    for at, n in enumerate(sizes):
        lists, nslides = _slide_lists(n, T, narrow, shift=at)
        assert nslides >= 11 * 5 + 10 + 1 and all(1 <= len(l) <= abi.WSLIDE_MAX_AGGS for l in lists) and len(lists[0]) == 4 and len(lists[-1]) == 1
        met |= {(s[0], i % 5) for i, s in enumerate(sum(lists[:-1], [])) if i < 5 * len(_widths(n, T, narrow))}
        t = _table(ctx, *_pattern(pattern, n, T, rng))
        try:
            done, ref = _check(ctx, t, TERMS, 1, (pattern, n), lists, limits=_limits)
            assert done >= nslides and ref.n == n
            if n > 3:                                                      # frames that follow the row look past the limit: row 0 of m = 1 counts rows that are not returned
                got = ctx.table_window_slide(t, 1, 0, TERMS, [(COUNT,) + MEASURES[0] + (0, 2, 0), (SUM, H, 0, False, 1, 3, 0)], 1, 64)
                hits = _stage_rows(ctx, t, 1)[3][Ranked(_stage_rows(ctx, t, 1), TERMS, 0).order]
                assert len(got[0]) == 1 and got[4][0][0] == 3 and got[4][1][0] == hits[1:4].sum()
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
    assert met == {(op, kind) for op in OPS for kind in range(5)}          # every op met every kind of frame


# 2. layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True])
def test_layouts(hip_engine, big):
    """The direct layout, the open-addressing layout, a table with duplicate build keys (owner rows only), a row-program build, each
    with min_hits in {0, 1, 2}."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    n = 70001 if big else T + 1
    rng = np.random.default_rng(n)
    part, value, _ = _pattern("runs", n, T, rng)
    hits = rng.integers(0, 4, n)                                           # some entries never probed: min_hits selects
    lists = [[(SUM,) + MEASURES[0] + (-2, 64, 0), (MAX,) + MEASURES[1] + (-T, 0, -1), (FIRST,) + MEASURES[2] + (-1, -1, I_MIN), (MIN,) + MEASURES[2] + (1, T + 1, 5)]]

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
        xl = [[(SUM, V, 0, True, -65, 0, 0), (SUM, K, 0, False, 0, 3, 0), (LAST, H, 0, False, 2, 70, -1), (MIN, K, 0, False, -T - 1, 1, 0)]]
        for mh in (0, 1, 2):
            assert _check(ctx, t, terms, 1, ("xbuild", mh), xl, min_hits=mh)[0] >= 4
    finally:
        t.free()


# 3. derived terms -----------------------------------------------------------------------------------------------------------------------
def test_derived_terms(hip_engine):
    """PARTITION BY the high half of a packed key ORDER BY its low half descending, then a text-ranked payload; the measure is the plain
    payload.  A ranks column too short is SDQH_ERR_INVALID naming the term, with nothing written, *out_n included."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    short = ctx.upload(want[:20])
    m = (P, 0, False)
    lists = [[(SUM,) + m + (-3, 3, 0), (MIN,) + m + (-64, 0, 0), (LAST,) + m + (1, 1, -1), (COUNT,) + m + (-T, T, 0)], [(SUM, K, 0, False, 0, 65, 0)]]
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
                out, vals = np.full(len(keys), -7, np.int64), np.full((4, len(keys)), -7, np.int64)
                assert _raw(ctx, t, 0, 1, bad, lists[0], ALL, len(keys), out, vals) == (abi.ERR_INVALID, -7) and (out == -7).all() and (vals == -7).all()
                assert b"term 2" in ctx.lib.sdqh_last_error(ctx.handle)
            finally:
                t.free()
    finally:
        ct.free(); short.free()


# 4. nothing subtracted, nothing leaked ---------------------------------------------------------------------------------------------------
def _payload_table(ctx, part, dbls, ints=None, seed=3):
    """entries with payload 0 = part, payload 1 = the bits of dbls (and payload 2 = ints), in random build order"""
    n = len(part)
    keys = np.random.default_rng(seed + n).permutation(n).astype(np.int64) * 3 - n
    cols = [ctx.upload(np.asarray(part, np.int64)), ctx.upload(np.ascontiguousarray(dbls, np.float64).view(np.int64))] + ([] if ints is None else [ctx.upload(np.asarray(ints, np.int64))])
    return ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), cols, accumulate=False)


@pytest.mark.parametrize("alternating", [False, True])
def test_nothing_subtracted_nothing_leaked(hip_engine, alternating):
    """Runs of 40 rows near +-1e300 alternate with runs of 40 small integers, in one long partition or a partition each.  A sum that
    took a prefix sum and subtracted (1e300 + 3 - 1e300 = 0), or that let a row outside the frame or the partition in, loses the small
    values: every frame all of whose rows are small must be exact."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    for n in (2 * T + 1, 5 * T + 17):
        rng = np.random.default_rng(n)
        run = np.arange(n) // 40
        small = run % 2 == 1
        dbls = np.where(small, rng.integers(-9, 10, n).astype(np.float64), rng.choice([-1.0, 1.0], n) * (1e300 + rng.integers(0, 1000, n) * 1e290))
        part = run if alternating else np.zeros(n, np.int64)
        mix = rng.permutation(n)
        t = _payload_table(ctx, part[mix], dbls[mix], np.arange(n)[mix])
        try:
            terms = [(P, 0, False, False), (P, 2, False, False)]           # the sorted order is the order the runs were laid out in
            rows = _stage_rows(ctx, t, 0)
            ref = Slid(rows, terms, 1)
            x = ref.column(P, 1).view(np.float64)
            assert (x == dbls).all() and (np.abs(x[~small]) >= 1e300).all()
            xi = np.where(small, x, 0.0).astype(np.int64)
            c, big = np.concatenate(([0], np.cumsum(xi))), np.concatenate(([0], np.cumsum(~small)))
            frames = [(-5, 0), (0, 5), (-3, 3), (-T - 1, 0)]
            got = ctx.table_window_slide(t, 0, 1, terms, [(SUM, P, 1, True, lo, hi, 0) for lo, hi in frames], ALL, n, want_hits=False)
            _same(got, rows, ref.order, ("subtract", n))
            for a, (lo, hi) in zip(got[4], frames):
                left, right, emp = ref.frame(lo, hi)
                assert not emp.any() and a.dtype == np.float64
                pure = big[right + 1] - big[left] == 0                     # frames that hold small rows only
                want = (c[right + 1] - c[left]).astype(np.float64)
                assert (a[pure] == want[pure]).all(), (n, lo, hi, np.nonzero(a[pure] != want[pure])[0][:5])
                if alternating or hi - lo < 40:                            # such frames exist on both sides of a tile boundary — and, in the longer table, across one
                    assert (pure & (right < T)).any() and (pure & (left >= T)).any(), (n, lo, hi)
                    assert n < 5 * T or (pure & (left < 2 * T) & (right >= 2 * T)).any(), (n, lo, hi)
                assert np.isfinite(a).all() and (np.abs(a[~pure]) >= 1e299).any()
        finally:
            t.free()


# 5. general doubles -----------------------------------------------------------------------------------------------------------------------
def test_general_doubles_within_the_bound(hip_engine):
    """Values k * 2^-20 with |value| < 2^40: exact sums are integer sums of the k.  Every SUM lies within the header's bound
    gamma * sum|v|, gamma = (m - 1) u / (1 - (m - 1) u), u = 2^-53, m the frame's own row count; MIN / MAX / FIRST / LAST / COUNT are
    exact; two calls return identical bits."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
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
        tie = rng.integers(0, max(2, n // 3), n)
        mix = rng.permutation(n)
        t = _payload_table(ctx, part[mix], dbls[mix], tie[mix])
        try:
            terms = [(P, 0, False, False), (P, 2, True, False)]
            rows = _stage_rows(ctx, t, 0)
            ref = Slid(rows, terms, 1)
            m = (P, 1, True)
            frames = [f for w in (3, 65, T + 1) for f in ((-(w - 1), 0), (0, w - 1), (-(w // 2), w - 1 - w // 2), (-w - 1, -2))]
            ks = np.rint(ref.column(P, 1).view(np.float64) * float(1 << 20)).astype(np.int64).tolist()
            cs, ms = [0], [0]
            for v in ks:
                cs.append(cs[-1] + v); ms.append(ms[-1] + abs(v))
            worst = Fraction(0)
            for i in range(0, len(frames), 4):
                sums = [(SUM,) + m + f + (NAN_BITS,) for f in frames[i:i + 4]]
                got = ctx.table_window_slide(t, 0, 1, terms, sums, ALL, n, want_hits=False)
                again = ctx.table_window_slide(t, 0, 1, terms, sums, ALL, 64, want_hits=False)
                _same(got, rows, ref.order, ("general", n))
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(got[4], again[4])), (n, "two calls differ")
                for a, (lo, hi) in zip(got[4], frames[i:i + 4]):
                    left, right, emp = ref.frame(lo, hi)
                    assert (_bits(a)[emp] == NAN_BITS).all()
                    for j in np.nonzero(~emp)[0].tolist():
                        l, r = int(left[j]), int(right[j])
                        cnt, exact, mag = r - l + 1, cs[r + 1] - cs[l], ms[r + 1] - ms[l]
                        gamma = (cnt - 1) * u / (1 - (cnt - 1) * u)
                        err = abs(Fraction(float(a[j])) * (1 << 20) - exact)
                        assert err <= gamma * mag, (n, lo, hi, j, cnt, float(err), float(gamma * mag))
                        worst = max(worst, err / mag if mag else Fraction(0))
                for op in (MIN, MAX, FIRST, LAST):                          # exact
                    others = [(op,) + m + f + (-1,) for f in frames[i:i + 4]]
                    got = ctx.table_window_slide(t, 0, 1, terms, others, ALL, n, want_hits=False)
                    again = ctx.table_window_slide(t, 0, 1, terms, others, ALL, 64, want_hits=False)
                    for a, b, s in zip(got[4], again[4], others):
                        assert (_bits(a) == ref.want(s)).all() and (_bits(a) == _bits(b)).all(), (n, s)
                counts = [(COUNT,) + m + f + (0,) for f in frames[i:i + 4]]
                for a, s in zip(ctx.table_window_slide(t, 0, 1, terms, counts, ALL, n, want_hits=False)[4], counts):
                    assert a.dtype == np.int64 and (a == ref.want(s)).all(), (n, s)
            print("general doubles n=%d: worst |err| / sum|v| = %.3g (bound at the widest frame %.3g)" % (n, float(worst), float(T * u)))
        finally:
            t.free()


# 6. edge values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 2600])
def test_edge_values(hip_engine, n):
    """+-0.0, +-inf, two NaN bit patterns, DBL_MAX, INT64_MIN / MAX as measures and as partition terms.  MIN / MAX / FIRST / LAST exact
    by bits (-0.0 below +0.0, NaNs skipped by MIN / MAX — nothing but NaNs: the quiet NaN — and copied with their payload by FIRST /
    LAST); integer SUM wraps like numpy's; an empty frame gives `empty` whatever its bits, and COUNT gives 0."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) * 3 - n
    ints = np.resize(EDGE_INTS, n)[rng.permutation(n)]
    dbls = np.resize(EDGE_DOUBLES, n)[rng.permutation(n)]
    t = ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ints), ctx.upload(dbls.view(np.int64))], accumulate=False)
    mi, md = (P, 0, False), (P, 1, True)
    frames = [(-2, 0), (0, 3), (-1, 1), (-5, -3), (2, 6), (-70, 0), (UP, UF), (-1, -1), (1, 1)]
    lists = []
    for i, (lo, hi) in enumerate(frames):
        e = EMPTIES[i % len(EMPTIES)]
        lists += [[(MIN,) + md + (lo, hi, e), (MAX,) + md + (lo, hi, e), (FIRST,) + md + (lo, hi, e), (LAST,) + md + (lo, hi, e)],
                  [(SUM,) + mi + (lo, hi, e), (MIN,) + mi + (lo, hi, e), (MAX,) + mi + (lo, hi, e), (COUNT,) + mi + (lo, hi, e)],
                  [(FIRST,) + mi + (lo, hi, EMPTIES[(i + 1) % 5]), (LAST,) + mi + (lo, hi, EMPTIES[(i + 2) % 5])]]
    try:
        done = 0
        for terms, npart in (([(P, 1, False, True), (P, 0, True, False)], 1), ([(P, 0, False, False), (P, 1, True, True)], 1),
                             ([(P, 1, True, True), (P, 0, False, False)], 2), ([(P, 1, False, True)], 0), ([(P, 0, True, False)], 0),
                             ([(K, 0, False, False, 0, 5, 0, None), (P, 0, False, False)], 1)):
            with np.errstate(over="ignore"):
                d, ref = _check(ctx, t, terms, npart, ("edge", terms, npart), lists, min_hits=0)
            done += d
            x = ref.column(P, 1).view(np.float64)
            if terms[0][:2] == (P, 1) and npart == 1:                       # eight different doubles under the total order: a partition of NaNs only exists
                assert ref.ref.part_head.sum() == 8
                got = ctx.table_window_slide(t, 0, npart, terms, [(MIN,) + md + (-2, 0, 0), (FIRST,) + md + (0, 0, 0), (LAST,) + md + (-1, 0, 0)], ALL, n, want_hits=False)[4]
                nan = np.isnan(x)
                assert nan.any() and (_bits(got[0])[nan] == NAN_BITS).all() and (_bits(got[1]) == _bits(x)).all() and len(set(_bits(got[1])[nan].tolist())) == 2
                assert (_bits(got[2])[nan] == _bits(x)[nan]).all()           # (a partition holds one NaN bit pattern: the last of the frame is it)
            left, right, emp = ref.frame(-5, -3)
            assert emp.any() and not emp.all()
            for e in EMPTIES:                                               # every default comes back bit for bit; a count of nothing is 0
                got = ctx.table_window_slide(t, 0, npart, terms, [(FIRST,) + md + (-5, -3, e), (SUM,) + mi + (-5, -3, e), (COUNT,) + mi + (-5, -3, e), (MAX,) + md + (-5, -3, e)], ALL, n, want_hits=False)[4]
                assert all((_bits(a)[emp] == e).all() for a in (got[0], got[1], got[3])) and (got[2][emp] == 0).all() and (got[2][~emp] >= 1).all()
            neg_zero = np.signbit(x) & (x == 0)
            assert neg_zero.any()
            got = ctx.table_window_slide(t, 0, npart, terms, [(FIRST,) + md + (0, 0, 0)], ALL, n, want_hits=False)[4][0]
            assert np.signbit(got[neg_zero]).all() and (got[neg_zero] == 0).all()
        assert done >= 6 * len(frames) * 10
    finally:
        t.free()


# 7. agreement -------------------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_siblings(hip_engine):
    """(UNBOUNDED, 0) and (UNBOUNDED, UNBOUNDED) are sdqh_table_window_agg's ROWS and PARTITION frames: bit for bit for COUNT, integer
    SUM, MIN, MAX, within the header's bound for a double SUM; COUNT over (UNBOUNDED, 0) is sdqh_table_window's ROW_NUMBER; FIRST = LAST
    over (0, 0) = the measure of the emitted rows; the rows are sdqh_table_sorted_by's; LAG(k) of row j is the measure of row j - k
    wherever both lie in one partition."""
    from test_order_by_gpu import SPECS
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    done = 0
    uf = 2.0 ** -53
    for n in (S - 1, 5 * T + 17):
        t = _probed_table(ctx, n)
        try:
            for spec in SPECS:
                for min_hits in (0, 2):
                    want = ctx.table_sorted_by(t, min_hits, ALL, spec, n)
                    for npart in sorted({0, 1, len(spec)}):
                        for lo, hi, frame in ((UP, 0, abi.FRAME_ROWS), (UP, UF, abi.FRAME_PARTITION)):
                            got = ctx.table_window_slide(t, min_hits, npart, spec, [(COUNT, K, 0, False, lo, hi, 0), (SUM, P, 0, False, lo, hi, 0), (MIN, P, 1, True, lo, hi, 0),
                                                                                    (MAX, V, 0, True, lo, hi, 0)], ALL, n)
                            sib = ctx.table_window_agg(t, min_hits, npart, spec, [(COUNT, frame, K, 0, False), (SUM, frame, P, 0, False), (MIN, frame, P, 1, True),
                                                                                  (MAX, frame, V, 0, True)], ALL, n)
                            assert all((_bits(g) == _bits(w)).all() for g, w in zip(got[:4], want))
                            assert all((_bits(a) == _bits(b)).all() for a, b in zip(got[4], sib[4])), (n, spec, npart, frame)
                            full = ctx.table_window_slide(t, min_hits, npart, spec, [(SUM, P, 1, True, lo, hi, 0), (SUM, V, 0, True, lo, hi, 0), (COUNT, K, 0, False, lo, hi, 0),
                                                                                     (COUNT, K, 0, False, UP, 0, 0)], ALL, n)
                            fsum = full[4]
                            ssum = ctx.table_window_agg(t, min_hits, npart, spec, [(abi.WAGG_SUM, frame, P, 1, True), (abi.WAGG_SUM, frame, V, 0, True)], ALL, n)[4]
                            # Both are IEEE sums of the frame's rows, each within gamma(m) sum|v| of exact — m the frame's own row count (a
                            # COUNT over the same frame), sum|v| over the frame from the emitted measure columns: the frame starts at the
                            # partition's start (row number 1) and holds m rows.  The |v| are multiples of 1/4 with small sums: their prefix
                            # sums, and the differences of two of them, are exact in doubles.
                            m, first = fsum[2], np.arange(len(fsum[2])) - fsum[3] + 1
                            assert (m >= 1).all() and (first >= 0).all() and (first + m <= len(m)).all()
                            gamma = (m - 1) * uf / (1 - (m - 1) * uf)
                            for a, b, v in ((fsum[0], ssum[0], full[1][1].view(np.float64)), (fsum[1], ssum[1], full[2][0])):
                                c = np.concatenate(([0.0], np.cumsum(np.abs(v))))
                                mag = c[first + m] - c[first]
                                assert (c * 4 == np.rint(c * 4)).all() and c[-1] < 2.0 ** 50 and (mag >= np.abs(v)).all()
                                bad = np.nonzero(~(np.abs(a - b) <= 2 * gamma * mag))[0]
                                assert len(bad) == 0, (n, spec, npart, frame, bad[:5], a[bad[:5]], b[bad[:5]], (2 * gamma * mag)[bad[:5]])
                        rn = ctx.table_window(t, min_hits, npart, spec, abi.WIN_ROW_NUMBER, ALL, ALL, n)[4]
                        got = ctx.table_window_slide(t, min_hits, npart, spec, [(COUNT, K, 0, False, UP, 0, 0), (FIRST, V, 0, True, 0, 0, -1), (LAST, V, 0, True, 0, 0, -1),
                                                                                (FIRST, V, 0, True, -3, -3, NAN_BITS)], ALL, n)
                        assert (got[4][0] == rn).all()
                        assert (_bits(got[4][1]) == _bits(got[2][0])).all() and (_bits(got[4][2]) == _bits(got[2][0])).all()
                        inside = rn > 3                                     # row j - 3 lies in j's partition
                        assert (_bits(got[4][3])[inside] == _bits(got[2][0])[np.nonzero(inside)[0] - 3]).all() and (_bits(got[4][3])[~inside] == NAN_BITS).all()
                        done += 1
        finally:
            t.free()
    assert done >= 2 * 5 * 2 * 2


# 8. extreme offsets and argument errors -----------------------------------------------------------------------------------------------------
def test_extreme_offsets_and_argument_errors(hip_engine):
    ctx = hip_engine.ctx
    t = _table(ctx, *_pattern("runs", 700, 512, np.random.default_rng(3)))
    m = MEASURES[0]
    ok = [(SUM,) + m + (-2, 0, 0)]
    try:
        rows = _stage_rows(ctx, t, 1)
        ref = Slid(rows, TERMS, 1)
        size = ref.end - ref.start + 1
        for lo, hi in ((I_MIN + 1, I_MAX - 1), (UP, UF), (I_MIN + 1, UF), (UP, I_MAX - 1)):      # every one of them: the whole partition
            got = ctx.table_window_slide(t, 1, 1, TERMS, [(COUNT,) + m + (lo, hi, 0), (SUM,) + m + (lo, hi, 0), (MAX, H, 0, False, lo, hi, 0), (LAST, P, 0, False, lo, hi, 0)], ALL, 64)[4]
            assert (got[0] == size).all()
            for a, s in zip(got[1:], ((SUM,) + m + (UP, UF, 0), (MAX, H, 0, False, UP, UF, 0), (LAST, P, 0, False, UP, UF, 0))):
                assert (_bits(a) == ref.want(s)).all(), (lo, hi, s)
        for lo, hi in ((I_MAX - 1, I_MAX - 1), (I_MIN + 1, I_MIN + 1), (I_MAX - 1, UF), (UP, I_MIN + 1), (I_MAX, I_MAX), (I_MIN, I_MIN)):      # every frame is empty
            got = ctx.table_window_slide(t, 1, 1, TERMS, [(COUNT,) + m + (lo, hi, 5), (SUM,) + m + (lo, hi, NAN_BITS), (FIRST, H, 0, False, lo, hi, -9)], ALL, 64)[4]
            assert (got[0] == 0).all() and (_bits(got[1]) == NAN_BITS).all() and (got[2] == -9).all(), (lo, hi)
        lists, _ = _slide_lists(700, 512, 0)
        half = ctx.table_window_slide(t, 1, 1, TERMS, [(COUNT,) + m + (I_MIN + 1, 0, 0), (COUNT,) + m + (0, I_MAX - 1, 0)], ALL, 64)[4]
        assert (half[0] == ref.pos - ref.start + 1).all() and (half[1] == ref.end - ref.pos + 1).all()
        keys, out = np.full(700, -7, np.int64), np.full((5, 700), -7, np.int64)
        for npart, terms, slides, limit, nterms, nslides in (
                (1, TERMS, ok, 0, None, None), (-1, TERMS, ok, ALL, None, None), (4, TERMS, ok, ALL, None, None), (0, TERMS, ok, ALL, 0, None),
                (1, [TERMS[0]] * 9, ok, ALL, None, None), (1, [(P, 1, False, False)], ok, ALL, None, None), (1, [(V, 0, False, True, 2, 0, 0, None)], ok, ALL, None, None),
                (1, TERMS, ok, ALL, None, 0), (1, TERMS, ok * 5, ALL, None, None), (1, TERMS, [(6, V, 0, True, -1, 1, 0)], ALL, None, None),
                (1, TERMS, [(-1, V, 0, True, -1, 1, 0)], ALL, None, None), (1, TERMS, [(SUM, V, 0, True, 1, 0, 0)], ALL, None, None), (1, TERMS, [(COUNT, V, 0, True, 0, -1, 0)], ALL, None, None),
                (1, TERMS, [(FIRST, V, 0, True, UF, UP, 0)], ALL, None, None), (1, TERMS, [(SUM, V, 1, True, -1, 1, 0)], ALL, None, None), (1, TERMS, [(LAST, P, 1, False, -1, 1, 0)], ALL, None, None),
                (1, TERMS, [(MIN, 9, 0, False, -1, 1, 0)], ALL, None, None), (1, TERMS, [(SUM, K, 0, True, -1, 1, 0)], ALL, None, None), (1, TERMS, [(FIRST, H, 0, True, -1, 1, 0)], ALL, None, None)):
            assert _raw(ctx, t, 1, npart, terms, slides, limit, 700, keys, out, nterms=nterms, nslides=nslides) == (abi.ERR_INVALID, -7), (npart, slides, limit, nterms, nslides)
            assert (keys == -7).all() and (out == -7).all()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_slide(t, 1, 1, TERMS, [(6, V, 0, True, 0, 0, 0)], ALL, 64)
        assert e.value.code == abi.ERR_INVALID
        # COUNT ignores its measure, whatever it names
        got = ctx.table_window_slide(t, 1, 1, TERMS, [(COUNT, P, 3, True, -1, 1, 7)], ALL, 64)
        assert got[4][0].dtype == np.int64 and got[4][0].min() >= 1 and got[4][0].max() == 3
        assert _check(ctx, t, TERMS, 1, "after the errors", lists)[0] >= 60      # the context still works
    finally:
        t.free()


# 9. through the engine and the decorator -------------------------------------------------------------------------------------------------
Q3_SLIDES = {"prev": ("lag", "revenue", 1), "ma3": ("sum", "revenue", -2, 0), "n3": ("count", None, -2, 0), "best3": ("max", "revenue", -1, 1)}
Q3_NOTE = [["prev", "first", "revenue", -1, -1, None], ["ma3", "sum", "revenue", -2, 0, None], ["n3", "count", None, -2, 0, None], ["best3", "max", "revenue", -1, 1, None]]
RUN_TO_RUN = 1e-10      # two runs of a query accumulate its sums in another order: what test_window_gpu allows between two runs' rows


def _partitions(res, by):
    """(start, end) of every row's partition in a result whose rows are in order already"""
    n = len(res)
    head = np.zeros(n, bool)
    head[0] = True
    for b in by:
        a = np.asarray(res.column(b))
        head[1:] |= a[1:] != a[:-1]
    pos = np.arange(n)
    return np.maximum.accumulate(np.where(head, pos, 0)), _last_of(head)


def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "desc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    uf = 2.0 ** -53

    def compare(res):
        """the four columns against numpy on the returned rows: exact, but the sum of three doubles — within the header's bound, m = 3"""
        assert res.columns == plain.columns + list(Q3_SLIDES) and len(res) == len(plain) > 100
        assert [res.column(c).dtype for c in Q3_SLIDES] == [np.float64, np.float64, np.int64, np.float64]
        n, x = len(res), np.asarray(res.column("revenue"))
        start, end = _partitions(res, by)
        pos = np.arange(n)
        assert (x[1:] <= x[:-1])[start[1:] != pos[1:]].all()
        prev = res.column("prev")
        assert np.isnan(prev[start == pos]).all() and (prev[start != pos] == x[pos[start != pos] - 1]).all()
        assert (res.column("n3") == np.minimum(pos - start + 1, 3)).all()
        pad = np.concatenate(([0.0, 0.0], x))
        parts = [np.where(pos - d >= start, pad[pos - d + 2], 0.0) for d in (2, 1, 0)]
        mag = sum(np.abs(p) for p in parts)
        assert (np.abs(res.column("ma3") - (parts[0] + parts[1] + parts[2])) <= 2 * (2 * uf / (1 - 2 * uf)) * mag).all()
        best = np.maximum(x, np.maximum(np.where(pos - 1 >= start, x[np.maximum(pos - 1, 0)], -np.inf), np.where(pos + 1 <= end, x[np.minimum(pos + 1, n - 1)], -np.inf)))
        assert (res.column("best3") == best).all()
        return mag

    dev = Q.q3.sliding(by, order, Q3_SLIDES)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "window_slide", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "slides": Q3_NOTE}
    compare(dev)
    monkeypatch.setattr(eng, "device_window_slide", False)
    host = Q.q3.sliding(by, order, Q3_SLIDES)(*args)
    assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "slides": Q3_NOTE}
    mag = compare(host)

    def close(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return bool(np.allclose(a, b, rtol=RUN_TO_RUN, atol=0.0, equal_nan=True)) if a.dtype.kind == "f" else bool((a == b).all())
    for c in plain.columns + ["prev", "n3", "best3"]:
        assert close(host.column(c), dev.column(c)), c
    assert (np.abs(dev.column("ma3") - host.column("ma3")) <= (2 * (2 * uf / (1 - 2 * uf)) + RUN_TO_RUN) * mag).all()
    monkeypatch.setattr(eng, "device_window_slide", True)
    # more than four: on the host
    five = dict(Q3_SLIDES, nxt=("lead", "revenue", 1, 0.0))
    wide = Q.q3.sliding(by, order, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == plain.columns + list(five)
    assert close(wide.column("n3"), dev.column("n3")) and close(wide.column("best3"), dev.column("best3"))
    # q16: text fields in a mixed-radix key partition, the count is the measure: exact
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    slides16 = {"above": ("lag", "supplier_cnt", 1, -1), "pair": ("sum", "supplier_cnt", 0, 1), "low": ("min", "supplier_cnt", -2, 2)}
    res = Q.q16.sliding(["p_brand"], [("supplier_cnt", "desc")], slides16)(*args16)
    route = eng.stats()["order_routes"][-1]
    assert route["route"] == "window_slide" and route["per"] == ["p_brand"]
    assert route["slides"] == [["above", "first", "supplier_cnt", -1, -1, -1], ["pair", "sum", "supplier_cnt", 0, 1, None], ["low", "min", "supplier_cnt", -2, 2, None]]
    assert [res.column(c).dtype for c in slides16] == [np.int64] * 3 and len(res) > 100
    cnt, n = np.asarray(res.column("supplier_cnt")), len(res)
    start, end = _partitions(res, ["p_brand"])
    pos = np.arange(n)
    assert (res.column("above") == np.where(pos == start, -1, cnt[np.maximum(pos - 1, 0)])).all()
    assert (res.column("pair") == cnt + np.where(pos + 1 <= end, cnt[np.minimum(pos + 1, n - 1)], 0)).all()
    assert (res.column("low") == cnt[np.minimum(pos + 2, end)]).all()      # (descending: the lowest of the frame is its last row)
    # a default no double holds, for a count the table may keep as a double: exact all the same, whichever route takes it
    far = Q.q16.sliding(["p_brand"], [("supplier_cnt", "desc")], {"above": ("lag", "supplier_cnt", 1, (1 << 62) + 1), "below": ("lead", "supplier_cnt", 1, I_MIN)})(*args16)
    assert eng.stats()["order_routes"][-1]["slides"][0] == ["above", "first", "supplier_cnt", -1, -1, (1 << 62) + 1]
    assert (far.column("above") == np.where(pos == start, (1 << 62) + 1, cnt[np.maximum(pos - 1, 0)])).all()
    assert (far.column("below") == np.where(pos == end, I_MIN, cnt[np.minimum(pos + 1, n - 1)])).all()
    with pytest.raises(ValueError):                                       # ... and one that does not fit an int64 column is refused by the call
        Q.q16.sliding(["p_brand"], [("supplier_cnt", "desc")], {"above": ("lag", "supplier_cnt", 1, 0.5)})(*args16)
    # a text measure: on the host (and refused there: not numeric)
    with pytest.raises(ValueError):
        Q.q16.sliding(["p_brand"], [("supplier_cnt", "desc")], {"x": ("first", "p_type", 0, 0)})(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]
