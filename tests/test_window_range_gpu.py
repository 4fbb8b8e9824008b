"""Value and group window frames on the MI355X (run with -m gpu): sdqh_table_window_range (include/sdqh_sort_range.h) against numpy at
every size at which the sort, the tile passes or the fold tree take another path, at offsets around the wave, the tile and the table,
on partition patterns that exercise the carries between tiles and value patterns that give frames of data-dependent width, on every
table layout, over derived terms, on double order values at their edges, on values that would betray a prefix-sum-and-subtract, on
general doubles against the header's error bound, against sdqh_table_window_agg / sdqh_table_window_slide / sdqh_table_sorted_by where
they overlap, its argument errors, and through the engine and the decorator.

The expected rows are the table's own K-F rows reordered by a stable numpy lexsort (test_window_gpu's Ranked).  The frame's ends are
restated here: one ordered image per sorted position (the ORDER BY value, or the dense rank), bounds computed in Python integers
(object arrays) and clipped to int64 — for doubles the one np.float64 add — and np.searchsorted over (partition, image); for n <= 300
those ends are checked once more against an O(n^2) membership walk by the header's definition.  The values of a frame [l, r] are
computed as test_window_slide_gpu's Slid computes them.  Nothing is imported from the product's fold code."""
import ctypes as C
import struct
from fractions import Fraction

import numpy as np
import pytest

from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from test_window_gpu import (PATTERNS, TERMS, Ranked, _pattern, _same, _sizes as _window_sizes, _sort_bits, _stage_rows, _table, _under, db, hip_engine,
                             on_the_decorator)     # noqa: F401 (fixtures)
from test_window_slide_gpu import EMPTIES, NAN_BITS, RUN_TO_RUN, Slid, _bits, _partitions

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
SUM, COUNT, MIN, MAX, FIRST, LAST = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WSLIDE_FIRST, abi.WSLIDE_LAST
OPS = (SUM, COUNT, MIN, MAX, FIRST, LAST)
VAL, GRP = abi.WRANGE_VALUE, abi.WRANGE_GROUPS
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
NAN_A = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]
RM = [(P, 2, True), (P, 3, False), (P, 0, False)]                          # _range_table's measures: a double, an integer, the partition id
VALUE_PATTERNS = ["dense", "gaps", "heavy ties", "one value", "wide"]


def _sizes(ctx):
    T, S, sizes = _window_sizes(ctx)
    tile, narrow = ctx.window_range_geometry()
    assert tile == ctx.window_geometry() == T and narrow >= 0              # one tile for ranks, aggregates, slides and ranges
    return T, S, sorted(set(sizes) | {4095, 4096, 4097, 65537}), narrow    # ... and the edges of the padded tree


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _neg(x):
    return None if x is None else -x


def _ends_ascending(part, v, is_f, lo, hi, start, end):
    """(first position, last position, empty?) of every position's frame where v ascends inside every partition (part: the partition's
    number, ascending): the rows i of j's partition with lo <= v(i) - v(j) <= hi."""
    n = len(v)
    img = _sort_bits(np.ascontiguousarray(v), is_f, False)
    never, always = np.zeros(n, bool), np.ones(n, bool)
    if is_f:
        nan = np.isnan(v)
        with np.errstate(over="ignore", invalid="ignore"):
            tl = None if lo is None else v + np.float64(lo)                # the one IEEE addition
            tr = None if hi is None else v + np.float64(hi)
        if tl is not None and tr is not None:
            tl, tr = np.minimum(tl, tr), np.maximum(tl, tr)

        def side(t, lower):                                                # IEEE comparison: a zero bound takes both zeros; a NaN row its own tie run
            if t is None:
                return img, always, never
            z = np.where(t == 0.0, -0.0 if lower else 0.0, np.where(nan, 0.0, t))
            return np.where(nan, img, _sort_bits(z, True, False)), never, never
        (kl, all_l, none_l), (kr, all_r, none_r) = side(tl, True), side(tr, False)
    else:
        def side(off, lower):                                              # Python integers: nothing wraps
            if off is None:
                return img, always, never
            u, inv = np.unique(v, return_inverse=True)                     # (a bound depends on the row's value alone: once per distinct value)
            t = u.astype(object) + int(off)
            over, under = (t > I_MAX).astype(bool)[inv], (t < I_MIN).astype(bool)[inv]
            k = _sort_bits(np.clip(t, I_MIN, I_MAX).astype(np.int64)[inv], False, False)
            return (k, under, over) if lower else (k, over, under)
        (kl, all_l, none_l), (kr, all_r, none_r) = side(lo, True), side(hi, False)
    uniq = np.unique(img)
    U = np.int64(len(uniq) + 1)
    c = part * U + np.searchsorted(uniq, img, "left")
    left = np.searchsorted(c, part * U + np.searchsorted(uniq, kl, "left"), "left")
    right = np.searchsorted(c, part * U + np.searchsorted(uniq, kr, "right") - 1, "right") - 1
    left, right = np.where(all_l, start, left), np.where(all_r, end, right)
    empty = none_l | none_r | (left > right)
    if 0 < n <= 300:
        _walk(v, is_f, lo, hi, start, end, left, right, empty)
    return left, right, empty


def _walk(v, is_f, lo, hi, start, end, left, right, empty):
    """the same by the header's definition, every row of the partition tested for every row"""
    vals = v.tolist()
    bits = np.ascontiguousarray(v).view(np.int64).tolist()
    for j in range(len(vals)):
        s, e, vj = int(start[j]), int(end[j]), vals[j]
        if not is_f:
            inside = [i for i in range(s, e + 1) if (lo is None or vals[i] - vj >= lo) and (hi is None or vals[i] - vj <= hi)]
        elif vj != vj:                                                     # a NaN row: each bounded side ends with its own tie run
            same = [i for i in range(s, e + 1) if bits[i] == bits[j]]
            inside = [i for i in range(s, e + 1) if (lo is None or i >= same[0]) and (hi is None or i <= same[-1])]
        else:
            with np.errstate(over="ignore"):
                a = None if lo is None else float(np.float64(vj) + np.float64(lo))
                b = None if hi is None else float(np.float64(vj) + np.float64(hi))
            inside = []
            for i in range(s, e + 1):
                x = vals[i]
                if x != x:                                                 # a NaN: only through an unbounded side (negative NaNs come first, positive ones last)
                    ok = (lo is None) if bits[i] < 0 else (hi is None)
                elif a is not None and b is not None:
                    ok = min(a, b) <= x <= max(a, b)
                else:
                    ok = (a is None or x >= a) and (b is None or x <= b)
                if ok:
                    inside.append(i)
        if inside:
            assert not empty[j] and (int(left[j]), int(right[j])) == (inside[0], inside[-1]) and inside == list(range(inside[0], inside[-1] + 1)), (j, lo, hi)
        else:
            assert empty[j], (j, lo, hi)


class Ranged(Slid):
    """Slid with the frame of a value / group range in the place of the positional one: `unit` is set by want_range."""

    def __init__(self, rows, terms, npart, rank_tables=None):
        Slid.__init__(self, rows, terms, npart, rank_tables)
        self.terms, self.npart, self.unit, self._ends = terms, npart, None, {}
        self.part = (np.cumsum(self.ref.part_head) - 1).astype(np.int64)
        self.group = np.asarray(self.ref.ranks[abi.WIN_DENSE_RANK], np.int64)

    def value(self):
        """(v of every sorted position before the descending reversal, is it a double, descending?) of the one ORDER BY term"""
        assert len(self.terms) == self.npart + 1
        t = self.terms[self.npart]
        kind, index, desc, is_f64 = t[:4]
        src = self.column(kind, index)
        if len(t) > 4:
            div, mod, add, ranks = t[4:]
            assert ranks is None
            f = np.ascontiguousarray(src).view(np.uint64)
            f = f // np.uint64(div) if div > 1 else f
            f = f % np.uint64(mod) if mod else f
            return f.astype(np.int64) + np.int64(add), False, bool(desc)
        if kind == V or (kind == P and is_f64):
            return np.ascontiguousarray(src).view(np.float64), True, bool(desc)
        return np.asarray(src, np.int64), False, bool(desc)

    def ends(self, unit, lo, hi):
        key = (unit, lo, hi)
        if key not in self._ends:
            n = self.n
            if n == 0:
                self._ends[key] = (self.pos, self.pos, np.zeros(0, bool))
            else:
                v, is_f, desc = (self.group, False, False) if unit == GRP else self.value()
                if not desc:
                    self._ends[key] = _ends_ascending(self.part, v, is_f, lo, hi, self.start, self.end)
                else:                                                      # read backwards the order ascends: (lo, hi) becomes (-hi, -lo)
                    l2, r2, e2 = _ends_ascending((self.part[-1] - self.part)[::-1], v[::-1], is_f, _neg(hi), _neg(lo), (n - 1 - self.end)[::-1], (n - 1 - self.start)[::-1])
                    self._ends[key] = ((n - 1 - r2)[::-1], (n - 1 - l2)[::-1], e2[::-1])
        return self._ends[key]

    def frame(self, lo, hi):
        return self.ends(self.unit, lo, hi)

    def want_range(self, rg):
        op, kind, index, is_f64, unit, lo, hi, empty = rg
        self.unit = unit
        return self.want((op, kind, index, is_f64, lo, hi, empty))


def _is_f64(rg):
    op, kind, _, is_f64 = rg[:4]
    return op != COUNT and (kind == V or (kind == P and bool(is_f64)))


def _marshal(ranges):
    arr = (abi.WindowRange * max(1, len(ranges)))()
    for a, (op, kind, index, is_f64, unit, lo, hi, empty) in zip(arr, ranges):
        a.op, a.kind, a.index, a.is_f64, a.unit, a.empty = op, kind, index, int(bool(is_f64)), unit, empty
        a.flags = (abi.WRANGE_LO_UNBOUNDED if lo is None else 0) | (abi.WRANGE_HI_UNBOUNDED if hi is None else 0)
        a.lo, a.hi = abi._range_offset(lo), abi._range_offset(hi)
    return arr


def _raw(ctx, t, min_hits, npart, terms, ranges, limit, capacity, keys=None, out=None, nterms=None, nranges=None, flags=None):
    got = C.c_int64(-7)
    arr = _marshal(ranges)
    if flags is not None:
        arr[0].flags = flags
    rc = ctx.lib.sdqh_table_window_range(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms),
                                         abi._marshal_sort_terms(terms), C.c_int(len(ranges) if nranges is None else nranges), arr,
                                         C.c_int64(limit), C.c_int64(capacity), None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                         None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(got))
    return rc, got.value


LIMITS_EVERYWHERE = 1100      # rows up to which _check runs every limit on every call


def _limits(n):
    return sorted({1, max(1, n // 2), ALL})


def _check(ctx, t, terms, npart, what, range_lists, min_hits=1, rank_tables=None, limits=None, ref=None):
    """Every list of ranges in one call each: rows and values against numpy, exact by bits; dtypes; the count-only call.  A limit cuts
    the rows returned, never the frames: the expected values are the first m of the whole table's."""
    rows = _stage_rows(ctx, t, min_hits)
    ref = ref or Ranged(rows, terms, npart, rank_tables)
    done = 0
    for i, ranges in enumerate(range_lists):
        for limit in (limits(ref.n) if limits and (i == 0 or ref.n <= LIMITS_EVERYWHERE) else (ALL,)):
            got = ctx.table_window_range(t, min_hits, npart, terms, ranges, limit, 64, want_hits=t.accumulate)
            m = min(limit, ref.n)
            _same(got, rows, ref.order[:m], (what, ranges, limit))
            assert len(got[4]) == len(ranges)
            for a, rg in zip(got[4], ranges):
                assert a.dtype == (np.float64 if _is_f64(rg) else np.int64) and len(a) == m, (what, rg)
                want = ref.want_range(rg)[:m]
                bad = np.nonzero(_bits(a) != want)[0]
                assert len(bad) == 0, (what, rg, limit, bad[:5], _bits(a)[bad[:5]], want[bad[:5]])
                done += 1
    assert _raw(ctx, t, min_hits, npart, terms, range_lists[0], ALL, 0) == (abi.OK, ref.n), (what, "count")
    return done, ref


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def _range_table(ctx, part, order, dbls, ints, seed=3):
    """entries with payload 0 = part, payload 1 = order (int64, or the bits of doubles), payload 2 = the bits of dbls, payload 3 = ints,
    in the build order given"""
    n = len(part)
    keys = np.random.default_rng(seed + n).permutation(n).astype(np.int64) * 3 - n
    order = np.ascontiguousarray(order)
    cols = [np.asarray(part, np.int64), order.view(np.int64) if order.dtype == np.float64 else order.astype(np.int64), np.ascontiguousarray(dbls, np.float64).view(np.int64), np.asarray(ints, np.int64)]
    return ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(c) for c in cols], accumulate=False)


def _order_values(name, part, rng):
    """int64 order values, by the pattern, per row (rows in any order; what matters is the values inside a partition)"""
    n = len(part)
    if name in ("dense", "gaps"):
        by = np.lexsort((rng.random(n), part))
        pos = np.arange(n)
        head = np.ones(n, bool)
        head[1:] = part[by][1:] != part[by][:-1]
        start = np.maximum.accumulate(np.where(head, pos, 0)) if n else pos
        run = pos if name == "dense" else np.cumsum(rng.integers(0, 6, n))
        v = np.zeros(n, np.int64)
        v[by] = run - run[start] if n else run
        return v
    if name == "heavy ties":
        return rng.integers(0, 5, n).astype(np.int64) * 3
    if name == "one value":
        return np.full(n, 7, np.int64)
    return rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)


def _offset_frames(widths):
    """every width ending at the row, starting at it, centred, wholly preceding and wholly following"""
    out = []
    for w in widths:
        out += [(-w, 0), (0, w), (-(w // 2), w - w // 2), (-w - 2, -2), (3, w + 3)]
    return out


def _range_lists(frames, shift, unit_of):
    """Every frame once, the ops, measures and defaults rotating over them (`shift` moves the rotation: over the sizes of a test every op
    meets every kind of frame), four to a call.

    This is a reduction of the full product ops x frames x units at every size: at one size a frame is folded by ONE op over one measure
    with one default in one unit.  What is kept: every frame (every width in all five positions) at every size and pattern; every op on
    every kind of frame over the sizes of a pattern (asserted: `met`); both units in every call; and, since the op only selects what is
    read off the two ends, every path through the search and the tree at every size."""
    ranges = []
    for i, (lo, hi) in enumerate(frames):
        ranges.append((OPS[(i + shift) % len(OPS)],) + RM[(i // 2 + shift) % len(RM)] + (unit_of(i), lo, hi, EMPTIES[(i + shift) % len(EMPTIES)]))
    return [ranges[i:i + 4] for i in range(0, len(ranges), 4)]


# 1. partition patterns x value patterns x sizes, both units ------------------------------------------------------------------------------
@pytest.mark.parametrize("values", VALUE_PATTERNS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern, values):
    ctx = hip_engine.ctx
    T, S, sizes, narrow = _sizes(ctx)
    case = PATTERNS.index(pattern) * len(VALUE_PATTERNS) + VALUE_PATTERNS.index(values)
    rng = np.random.default_rng(case)
    met = set()
    for at, n in enumerate(sizes):
        part = _pattern(pattern, n, T, rng)[0]
        order = _order_values(values, part, rng)
        desc = (at + case) % 2 == 1                                        # ascending and descending alternate over the sizes
        span = int(order.max()) - int(order.min()) if n else 0
        widths = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, min(span + 2, I_MAX - 4)] + ([narrow, narrow + 1] if narrow > 0 else [])
        frames = _offset_frames(widths)
        if values == "wide":                                               # offsets at the ends of int64: every bounded side is unbounded or empty, as Python integers say
            frames += [(I_MIN + 1, 0), (0, I_MAX - 1), (I_MIN + 1, I_MAX - 1), (I_MAX - 1, I_MAX - 1), (I_MIN + 1, I_MIN + 1), (I_MIN + 1, None), (None, I_MAX - 1), (I_MAX - 1, None)]
        lists = _range_lists(frames, at, lambda i: (i + at) % 2)
        assert len(frames) >= 55 and all(1 <= len(l) <= abi.WRANGE_MAX_AGGS for l in lists)
        met |= {(r[0], i % 5) for i, r in enumerate(sum(lists, [])) if i < 55}
        terms = [(P, 0, False, False), (P, 1, desc, False)]
        t = _range_table(ctx, part, order, rng.integers(-50, 50, n).astype(np.float64), rng.integers(-1000, 1000, n))
        try:
            done, ref = _check(ctx, t, terms, 1, (pattern, values, n, desc), lists, min_hits=0, limits=_limits)
            assert done >= len(frames) and ref.n == n
            if values == "dense" and n:                                    # v = the row number: the three kinds of frame are one
                for lo, hi in ((-2, 0), (0, T + 1), (-65, 64), (-T - 2, -2), (3, 5)):
                    for ms in ([(SUM, P, 3, False), (COUNT, P, 0, False), (MIN, P, 2, True), (MAX, P, 3, False)], [(FIRST, P, 2, True), (LAST, P, 3, False)]):
                        rows = ctx.table_window_slide(t, 0, 1, terms, [m + (lo, hi, -1) for m in ms], ALL, 64, want_hits=False)[4]
                        for unit in (VAL, GRP):
                            got = ctx.table_window_range(t, 0, 1, terms, [m + (unit, lo, hi, -1) for m in ms], ALL, 64, want_hits=False)[4]
                            assert all((_bits(a) == _bits(b)).all() for a, b in zip(got, rows)), (n, lo, hi, unit)
            if values == "gaps" and n >= T and pattern != "every row its own":      # ties and holes: a frame wholly behind the row is empty for some rows and not for others
                _, _, emp = ref.ends(VAL, 3, 3)
                assert emp.any() and not emp.all()
            if values == "wide" and n > 2:                                 # nothing wraps
                for lo, hi, whole in ((I_MIN + 1, I_MAX - 1, True), (I_MAX - 1, I_MAX - 1, False), (I_MIN + 1, I_MIN + 1, False)):
                    left, right, emp = ref.ends(VAL, lo, hi)
                    assert ((left == ref.start) & (right == ref.end)).all() if whole else emp.sum() >= n - 2, (n, lo, hi)
            if n > 3:                                                      # frames look past the limit: row 0 of m = 1 counts rows that are not returned
                got = ctx.table_window_range(t, 0, 0, [(P, 0, False, False), (P, 1, desc, False)], [(COUNT, P, 0, False, GRP, 0, None, 0)], 1, 64, want_hits=False)
                assert len(got[0]) == 1 and got[4][0][0] == n
            if n:                                                          # a capacity one too small: the needed count, nothing written
                keys, out = np.full(n, -7, np.int64), np.full((4, n), -7, np.int64)
                assert _raw(ctx, t, 0, 1, terms, lists[0], ALL, n - 1, keys, out) == (abi.ERR_OVERFLOW, n)
                assert (keys == -7).all() and (out == -7).all()
        finally:
            t.free()
    assert met == {(op, kind) for op in OPS for kind in range(5)}          # every op met every kind of frame


# 2. layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [False, True])
def test_layouts(hip_engine, big):
    """The direct layout, the open-addressing layout, a table with duplicate build keys (owner rows only), a row-program build, each
    with min_hits in {0, 1, 2}.  The order term is a double column of integer values: offsets are doubles."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    n = 70001 if big else T + 1
    rng = np.random.default_rng(n)
    part, value, _ = _pattern("runs", n, T, rng)
    hits = rng.integers(0, 4, n)                                           # some entries never probed: min_hits selects
    terms = [(P, 0, False, False), (V, 0, True, True)]
    lists = [[(SUM, V, 0, True, VAL, -2.0, 64.0, 0), (MAX, H, 0, False, GRP, -T, 0, -1), (FIRST, P, 0, False, VAL, -1.0, -1.0, I_MIN), (MIN, P, 0, False, GRP, 1, T + 1, 5)]]

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        try:
            return sum(_check(ctx, t, terms, 1, ("layout", dups, mh), lists, min_hits=mh, limits=_limits)[0] for mh in (0, 1, 2))
        finally:
            t.free()
    assert run(0) >= 3 * 4 * 2
    assert run(200) >= 3 * 4 * 2
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) >= 3 * 4 * 2
    # a row-program build (sdqh_xbuild): the key is its only integer column — partition by key % 7, order by the sum
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
        xterms = [(K, 0, True, False, 0, 7, 0, None), (V, 0, False, True)]
        xl = [[(SUM, V, 0, True, VAL, -1.0, 0.0, 0), (SUM, K, 0, False, GRP, 0, 3, 0), (LAST, H, 0, False, VAL, 1.0, 2.0, -1), (MIN, K, 0, False, GRP, -2, 1, 0)]]
        for mh in (0, 1, 2):
            assert _check(ctx, t, xterms, 1, ("xbuild", mh), xl, min_hits=mh)[0] >= 4
    finally:
        t.free()


# 3. derived terms -----------------------------------------------------------------------------------------------------------------------
def test_derived_terms(hip_engine):
    """PARTITION BY the high half of a packed key; VALUE over its low half (mod 2^32) descending; GROUPS over that term and a text-ranked
    payload.  VALUE over the text-ranked term is SDQH_ERR_INVALID (text has no arithmetic); a ranks column too short is
    SDQH_ERR_INVALID naming the term, with nothing written, *out_n included."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    short = ctx.upload(want[:20])
    m = (P, 0, False)
    try:
        for n in (T + 1, S + 1, 5 * T + 17):
            a = rng.integers(0, n // 90 + 2, n).astype(np.int64)
            b = rng.integers(0, 3000, n).astype(np.int64)
            keys = np.unique((a << 32) | b)
            keys = keys[rng.permutation(len(keys))]
            ref_col = rng.integers(0, len(text), len(keys)).astype(np.int64)
            t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ref_col)], accumulate=False)
            try:
                hi_half, lo_half = (K, 0, False, False, 1 << 32, 0, 0, None), (K, 0, True, False, 0, 1 << 32, 0, None)
                vlists = [[(SUM,) + m + (VAL, -30, 30, 0), (MIN,) + m + (VAL, -640, 0, 0), (LAST,) + m + (VAL, 1, 100, -1), (COUNT,) + m + (VAL, -T, T, 0)], [(SUM, K, 0, False, VAL, 0, 65, 0)]]
                assert _check(ctx, t, [hi_half, lo_half], 1, ("derived value", n), vlists, min_hits=0, limits=_limits)[0] >= 5
                terms = [hi_half, lo_half, (P, 0, False, False, 0, 0, 0, ct)]
                glists = [[(SUM,) + m + (GRP, -3, 3, 0), (MAX,) + m + (GRP, -64, 0, 0), (FIRST,) + m + (GRP, 1, 1, -1), (COUNT,) + m + (GRP, -T, T, 0)]]
                assert _check(ctx, t, terms, 1, ("derived groups", n), glists, min_hits=0, rank_tables={id(ct): want}, limits=_limits)[0] >= 4
                out, vals = np.full(len(keys), -7, np.int64), np.full((4, len(keys)), -7, np.int64)
                assert _raw(ctx, t, 0, 1, [hi_half, (P, 0, False, False, 0, 0, 0, ct)], vlists[0], ALL, len(keys), out, vals) == (abi.ERR_INVALID, -7)
                assert (out == -7).all() and (vals == -7).all()
                bad = terms[:2] + [(P, 0, False, False, 0, 0, 0, short)]
                assert _raw(ctx, t, 0, 1, bad, glists[0], ALL, len(keys), out, vals) == (abi.ERR_INVALID, -7) and (out == -7).all() and (vals == -7).all()
                assert b"term 2" in ctx.lib.sdqh_last_error(ctx.handle)
            finally:
                t.free()
    finally:
        ct.free(); short.free()


# 4. double order values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 2600])
def test_double_order_values(hip_engine, n):
    """+-0.0, +-inf, two NaN bit patterns, DBL_MAX, denormals and ordinary values as order values, ascending and descending, with
    offsets 0.0, 0.5, 1e308 and one so small that v + lo == v: every op but SUM exact by bits (the measures are integers and
    integer-valued doubles: SUM is exact too); the NaN rule, the zero rule and the inf rule of the header."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(n)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, NAN_A, NAN_B, np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324, -5e-324, 2.5e-310, 1.0, 1.5, 2.0, -1.0, 1e308, 3.0, 1e-5])
    order = np.resize(edge, n)[rng.permutation(n)]
    part = rng.integers(0, 3, n)
    t = _range_table(ctx, part, order, rng.integers(-50, 50, n).astype(np.float64), rng.integers(-1000, 1000, n))
    frames = [(0.0, 0.0), (-0.5, 0.5), (-1e308, 1e308), (-1e-300, 1e-300), (0.5, 1.0), (-1.0, -0.5), (None, 0.0), (0.0, None), (None, -0.5), (0.5, None), (None, None), (0.0, 1e308)]
    try:
        done = 0
        for desc in (False, True):
            terms = [(P, 0, False, False), (P, 1, desc, True)]
            lists = _range_lists(frames, int(desc), lambda i: VAL) + _range_lists(frames, 3 + int(desc), lambda i: VAL)
            d, ref = _check(ctx, t, terms, 1, ("doubles", n, desc), lists, min_hits=0, limits=_limits)
            done += d
            v = ref.value()[0]
            bits = _bits(v)
            got = ctx.table_window_range(t, 0, 1, terms, [(COUNT, P, 0, False, VAL, 0.0, 0.0, 0), (COUNT, P, 0, False, VAL, -0.5, 0.5, 0), (COUNT, P, 0, False, VAL, -1e308, 1e308, 0),
                                                         (COUNT, P, 0, False, VAL, -1e-300, 1e-300, 0)], ALL, 64, want_hits=False)[4]
            same_bits = np.array([np.count_nonzero((ref.part == ref.part[j]) & (bits == bits[j])) for j in range(n)])
            same_value = np.array([np.count_nonzero((ref.part == ref.part[j]) & (v == v[j])) for j in range(n)])
            nan, zero, inf = np.isnan(v), v == 0.0, np.isinf(v)
            assert nan.any() and zero.any() and inf.any() and len(set(bits[nan].tolist())) == 2 and len(set(bits[zero].tolist())) == 2
            for a in got:                                                  # a NaN row: its own tie run, whatever the offset
                assert (a[nan] == same_bits[nan]).all()
            assert (got[0][~nan] == same_value[~nan]).all() and (got[0][zero] > same_bits[zero]).all()      # both zeros enter together
            assert (got[2][inf] == same_value[inf]).all() and (got[1][inf] == same_value[inf]).all()         # inf + x = inf: its equals alone
            ordinary = (v == 1.0) | (v == 1.5) | (v == 2.0)
            assert (got[3][ordinary] == same_value[ordinary]).all() and (got[1][v == 1.5] > same_value[v == 1.5]).all()
        assert done >= 2 * 2 * len(frames)
    finally:
        t.free()


# 5. nothing subtracted, nothing leaked ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alternating", [False, True])
def test_nothing_subtracted_nothing_leaked(hip_engine, alternating):
    """Runs of 40 rows near +-1e300 alternate with runs of 40 small integers, in one long partition or a partition each; the order value
    steps by 1 inside a run and by 8 between runs, so a value frame's width depends on where the row lies.  A sum that took a prefix
    sum and subtracted (1e300 + 3 - 1e300 = 0), or that let a row outside the frame or the partition in, loses the small values: every
    frame all of whose rows are small must be exact."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    for n in (2 * T + 1, 5 * T + 17):
        rng = np.random.default_rng(n)
        run = np.arange(n) // 40
        small = run % 2 == 1
        dbls = np.where(small, rng.integers(-9, 10, n).astype(np.float64), rng.choice([-1.0, 1.0], n) * (1e300 + rng.integers(0, 1000, n) * 1e290))
        part = run if alternating else np.zeros(n, np.int64)
        order = np.arange(n) + 7 * run
        mix = rng.permutation(n)
        t = _range_table(ctx, part[mix], order[mix], dbls[mix], np.arange(n)[mix])
        try:
            terms = [(P, 0, False, False), (P, 1, False, False)]           # the sorted order is the order the runs were laid out in
            rows = _stage_rows(ctx, t, 0)
            ref = Ranged(rows, terms, 1)
            x = ref.column(P, 2).view(np.float64)
            assert (x == dbls).all() and (np.abs(x[~small]) >= 1e300).all()
            xi = np.where(small, x, 0.0).astype(np.int64)
            c, big = np.concatenate(([0], np.cumsum(xi))), np.concatenate(([0], np.cumsum(~small)))
            frames = [(VAL, -5, 0), (VAL, 0, 5), (GRP, -3, 3), (VAL, -T - 1, 0)]
            got = ctx.table_window_range(t, 0, 1, terms, [(SUM, P, 2, True, unit, lo, hi, 0) for unit, lo, hi in frames], ALL, n, want_hits=False)
            _same(got, rows, ref.order, ("subtract", n))
            widths = set()
            for a, (unit, lo, hi) in zip(got[4], frames):
                left, right, emp = ref.ends(unit, lo, hi)
                assert not emp.any() and a.dtype == np.float64
                widths |= set((right - left + 1).tolist())
                pure = big[right + 1] - big[left] == 0                     # frames that hold small rows only
                want = (c[right + 1] - c[left]).astype(np.float64)
                assert (a[pure] == want[pure]).all(), (n, unit, lo, hi, np.nonzero(a[pure] != want[pure])[0][:5])
                if alternating or hi - lo < 40:                            # such frames exist on both sides of a tile boundary — and, in the longer table, across one
                    assert (pure & (right < T)).any() and (pure & (left >= T)).any(), (n, lo, hi)
                    assert n < 5 * T or (pure & (left < 2 * T) & (right >= 2 * T)).any(), (n, lo, hi)
                assert np.isfinite(a).all() and (np.abs(a[~pure]) >= 1e299).any()
            assert len(widths) > 6                                         # widths that depend on the data
        finally:
            t.free()


# 6. general doubles -----------------------------------------------------------------------------------------------------------------------
def test_general_doubles_within_the_bound(hip_engine):
    """Values k * 2^-20 with |value| < 2^40: exact sums are integer sums of the k.  Every SUM lies within the header's bound
    gamma * sum|v|, gamma = (m - 1) u / (1 - (m - 1) u), u = 2^-53, m the frame's own row count; MIN / MAX / FIRST / LAST / COUNT are
    exact; two calls return identical bits."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    u = Fraction(1, 1 << 53)
    for n, lengths in ((2 * T + 1, [200, 3, 64, 65, 1]), (5 * T + 17, [5 * T + 17])):
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
        t = _range_table(ctx, part[mix], tie[mix], dbls[mix], np.arange(n)[mix])
        try:
            terms = [(P, 0, False, False), (P, 1, True, False)]
            rows = _stage_rows(ctx, t, 0)
            ref = Ranged(rows, terms, 1)
            m = (P, 2, True)
            frames = [(VAL, -2, 0), (GRP, 0, 64), (VAL, -(T // 6), T // 6), (GRP, -T - 3, -2), (GRP, -1, 1), (VAL, 0, T), (VAL, None, 0), (GRP, None, None)]
            ks = np.rint(ref.column(P, 2).view(np.float64) * float(1 << 20)).astype(np.int64).tolist()
            cs, ms = [0], [0]
            for v in ks:
                cs.append(cs[-1] + v); ms.append(ms[-1] + abs(v))
            worst = Fraction(0)
            for i in range(0, len(frames), 4):
                sums = [(SUM,) + m + f + (NAN_BITS,) for f in frames[i:i + 4]]
                got = ctx.table_window_range(t, 0, 1, terms, sums, ALL, n, want_hits=False)
                again = ctx.table_window_range(t, 0, 1, terms, sums, ALL, 64, want_hits=False)
                _same(got, rows, ref.order, ("general", n))
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(got[4], again[4])), (n, "two calls differ")
                for a, (unit, lo, hi) in zip(got[4], frames[i:i + 4]):
                    left, right, emp = ref.ends(unit, lo, hi)
                    assert (_bits(a)[emp] == NAN_BITS).all()
                    for j in np.nonzero(~emp)[0].tolist():
                        l, r = int(left[j]), int(right[j])
                        cnt, exact, mag = r - l + 1, cs[r + 1] - cs[l], ms[r + 1] - ms[l]
                        gamma = (cnt - 1) * u / (1 - (cnt - 1) * u)
                        err = abs(Fraction(float(a[j])) * (1 << 20) - exact)
                        assert err <= gamma * mag, (n, unit, lo, hi, j, cnt, float(err), float(gamma * mag))
                        worst = max(worst, err / mag if mag else Fraction(0))
                for op in (MIN, MAX, FIRST, LAST, COUNT):                   # exact
                    others = [(op,) + m + f + (-1,) for f in frames[i:i + 4]]
                    got = ctx.table_window_range(t, 0, 1, terms, others, ALL, n, want_hits=False)
                    again = ctx.table_window_range(t, 0, 1, terms, others, ALL, 64, want_hits=False)
                    for a, b, s in zip(got[4], again[4], others):
                        assert (_bits(a) == ref.want_range(s)).all() and (_bits(a) == _bits(b)).all(), (n, s)
            print("general doubles n=%d: worst |err| / sum|v| = %.3g (u = %.3g)" % (n, float(worst), float(u)))
        finally:
            t.free()


# 7. agreement -------------------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_siblings(hip_engine):
    """(unbounded, 0) in either unit is sdqh_table_window_agg's RANGE frame, (unbounded, unbounded) its PARTITION frame: bit for bit for
    COUNT, integer SUM, MIN, MAX, within 2 gamma sum|v| for a double SUM; all rows of a tie run share every value bit for bit; the
    rows are sdqh_table_sorted_by's."""
    ctx = hip_engine.ctx
    T, S, _, _ = _sizes(ctx)
    uf = 2.0 ** -53
    done = 0
    for n in (S - 1, 5 * T + 17):
        rng = np.random.default_rng(n)
        part, value, hits = _pattern("heavy ties", n, T, rng)
        value = value + rng.integers(0, 4, n) / 4.0                        # quarters: sums of them are exact in doubles
        t = _table(ctx, part, value, hits)
        try:
            for terms, units in (([(P, 0, False, False), (V, 0, True, True)], (VAL, GRP)), (TERMS, (GRP,)), ([(P, 0, True, False), (H, 0, False, False)], (VAL, GRP))):
                rows = _stage_rows(ctx, t, 1)
                ref = Ranged(rows, terms, 1)
                want = ctx.table_sorted_by(t, 1, ALL, terms, n)
                is_f = terms[1][0] == V
                zero = 0.0 if is_f else 0
                for unit in units:
                    for lo, hi, frame in ((None, zero, abi.FRAME_RANGE), (None, None, abi.FRAME_PARTITION)):
                        got = ctx.table_window_range(t, 1, 1, terms, [(COUNT, K, 0, False, unit, lo, hi, 0), (SUM, P, 0, False, unit, lo, hi, 0), (MIN, V, 0, True, unit, lo, hi, 0),
                                                                     (MAX, H, 0, False, unit, lo, hi, 0)], ALL, n)
                        sib = ctx.table_window_agg(t, 1, 1, terms, [(COUNT, frame, K, 0, False), (SUM, frame, P, 0, False), (MIN, frame, V, 0, True), (MAX, frame, H, 0, False)], ALL, n)
                        assert (got[0] == want[0]).all() and (got[3] == want[3]).all()
                        _same(got, rows, ref.order, ("agreement", n, unit))
                        assert all((_bits(a) == _bits(b)).all() for a, b in zip(got[4], sib[4])), (n, terms, unit, frame)
                        fsum = ctx.table_window_range(t, 1, 1, terms, [(SUM, V, 0, True, unit, lo, hi, 0), (COUNT, K, 0, False, unit, lo, hi, 0)], ALL, n)
                        ssum = ctx.table_window_agg(t, 1, 1, terms, [(SUM, frame, V, 0, True)], ALL, n)[4][0]
                        left, right, emp = ref.ends(unit, lo, hi)
                        assert not emp.any() and (fsum[4][1] == right - left + 1).all()
                        v = np.abs(fsum[2][0])
                        c = np.concatenate(([0.0], np.cumsum(v)))
                        assert (c * 4 == np.rint(c * 4)).all() and c[-1] < 2.0 ** 50      # prefix sums of |v| and their differences are exact
                        m = (right - left + 1).astype(np.float64)
                        gamma = (m - 1) * uf / (1 - (m - 1) * uf)
                        assert (np.abs(fsum[4][0] - ssum) <= 2 * gamma * (c[right + 1] - c[left])).all(), (n, terms, unit, frame)
                        done += 1
                    # all rows of a tie run share every value, whatever the frame
                    frames = [(-1, 1), (0, 2), (-3, -1), (None, 1)]
                    for op, ms in ((SUM, (V, 0, True)), (MIN, (V, 0, True)), (LAST, (H, 0, False)), (COUNT, (K, 0, False)), (FIRST, (P, 0, False))):
                        got = ctx.table_window_range(t, 1, 1, terms, [(op,) + ms + (unit, float(lo) if is_f and unit == VAL and lo is not None else lo,
                                                                                  float(hi) if is_f and unit == VAL else hi, 0) for lo, hi in frames], ALL, n)[4]
                        follower = ~ref.ref.tie_head
                        for a in got:
                            assert (_bits(a)[follower] == _bits(a)[np.nonzero(follower)[0] - 1]).all(), (n, terms, unit, op)
        finally:
            t.free()
    assert done >= 2 * 5 * 2


# 8. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors(hip_engine):
    ctx = hip_engine.ctx
    T = _sizes(ctx)[0]
    rng = np.random.default_rng(3)
    part = _pattern("runs", 700, T, rng)[0]
    t = _range_table(ctx, part, _order_values("gaps", part, rng), rng.integers(-50, 50, 700).astype(np.float64), rng.integers(-1000, 1000, 700))
    terms, fterms = [(P, 0, False, False), (P, 1, True, False)], [(P, 0, False, False), (P, 2, True, True)]
    m = RM[0]
    ok = [(SUM,) + m + (VAL, -2, 0, 0)]
    try:
        ct, _ = ctx.text_ranks(ctx.upload(np.array(["a", "b"])), 2)
        keys, out = np.full(700, -7, np.int64), np.full((5, 700), -7, np.int64)
        for npart, tm, ranges, limit, nterms, nranges, flags in (
                (1, terms, ok, 0, None, None, None), (-1, terms, ok, ALL, None, None, None), (3, terms, ok, ALL, None, None, None), (0, terms, ok, ALL, 0, None, None),
                (1, [terms[0]] * 9, ok, ALL, None, None, None), (1, [terms[0], (P, 4, False, False)], ok, ALL, None, None, None), (1, [terms[0], (P, 2, False, True, 2, 0, 0, None)], ok, ALL, None, None, None),
                (1, terms, ok, ALL, None, 0, None), (1, terms, ok * 5, ALL, None, None, None), (1, terms, [(6,) + m + (VAL, -1, 1, 0)], ALL, None, None, None),
                (1, terms, [(-1,) + m + (VAL, -1, 1, 0)], ALL, None, None, None), (1, terms, [(SUM,) + m + (2, -1, 1, 0)], ALL, None, None, None), (1, terms, [(SUM,) + m + (-1, -1, 1, 0)], ALL, None, None, None),
                (1, terms, ok, ALL, None, None, 4), (1, terms, ok, ALL, None, None, 8 | 1), (1, terms, [(SUM,) + m + (VAL, 1, 0, 0)], ALL, None, None, None),
                (1, terms, [(COUNT,) + m + (GRP, 0, -1, 0)], ALL, None, None, None), (1, fterms, [(SUM,) + m + (VAL, 0.5, 0.25, 0)], ALL, None, None, None),
                (1, fterms, [(SUM,) + m + (VAL, -1.0, -2.0, 0)], ALL, None, None, None), (1, fterms, [(SUM,) + m + (VAL, float("-inf"), 0.0, 0)], ALL, None, None, None),
                (1, fterms, [(SUM,) + m + (VAL, 0.0, float("nan"), 0)], ALL, None, None, None), (0, terms, ok, ALL, None, None, None), (2, terms, ok, ALL, None, None, None),
                (1, [terms[0], (P, 3, False, False, 0, 0, 0, ct)], ok, ALL, None, None, None),
                (1, terms, [(SUM, P, 4, True, VAL, -1, 1, 0)], ALL, None, None, None), (1, terms, [(MIN, 9, 0, False, GRP, -1, 1, 0)], ALL, None, None, None),
                (1, terms, [(SUM, K, 0, True, VAL, -1, 1, 0)], ALL, None, None, None), (1, terms, [(FIRST, V, 0, True, GRP, -1, 1, 0)], ALL, None, None, None)):
            assert _raw(ctx, t, 0, npart, tm, ranges, limit, 700, keys, out, nterms=nterms, nranges=nranges, flags=flags) == (abi.ERR_INVALID, -7), (npart, tm, ranges, limit, nterms, nranges, flags)
            assert (keys == -7).all() and (out == -7).all()
        ct.free()
        with pytest.raises(abi.SdqhError) as e:
            ctx.table_window_range(t, 0, 1, terms, [(6,) + m + (VAL, 0, 0, 0)], ALL, 64)
        assert e.value.code == abi.ERR_INVALID
        # an unbounded side ignores its offset, whatever it holds; COUNT ignores its measure, whatever it names
        assert _raw(ctx, t, 0, 1, terms, [(COUNT,) + m + (VAL, 5, -5, 0)], ALL, 0, flags=3) == (abi.OK, 700)
        got = ctx.table_window_range(t, 0, 1, terms, [(COUNT, P, 9, True, VAL, 0, 0, 7)], ALL, 64, want_hits=False)
        assert got[4][0].dtype == np.int64 and got[4][0].min() >= 1
        lists = _range_lists(_offset_frames([0, 1, 2, 63, 64, 65, T - 1, T, T + 1]), 0, lambda i: i % 2)
        assert _check(ctx, t, terms, 1, "after the errors", lists, min_hits=0)[0] >= 45      # the context still works
    finally:
        t.free()


# 9. through the engine and the decorator -------------------------------------------------------------------------------------------------
Q3_GROUPS = {"week": ("sum", "revenue", -6, 0), "n": ("count", None, -6, 0)}
Q3_VALUE = {"near": ("count", None, -1000.0, 1000.0), "best": ("max", "revenue", -1000.0, 1000.0)}


def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    uf = 2.0 ** -53

    def close(a, b):
        a, b = np.asarray(a), np.asarray(b)
        return bool(np.allclose(a, b, rtol=RUN_TO_RUN, atol=0.0, equal_nan=True)) if a.dtype.kind == "f" else bool((a == b).all())

    # this order date and the six distinct dates before it
    def groups(res):
        assert res.columns[-2:] == list(Q3_GROUPS) and [res.column(c).dtype for c in Q3_GROUPS] == [np.float64, np.int64] and len(res) > 100
        dates, rev = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
        start, end = _partitions(res, ["o_shippriority"])
        assert (dates[1:] >= dates[:-1])[start[1:] != np.arange(1, len(res))].all()
        head = np.ones(len(res), bool)
        head[1:] = (dates[1:] != dates[:-1]) | (start[1:] != start[:-1])
        g = np.cumsum(head)
        first_of = np.nonzero(head)[0]                                     # the first row of every tie run, by its number - 1
        lo_run = np.maximum(g - 6, g[start])
        left, right = first_of[lo_run - 1], np.append(first_of[1:], len(res))[g - 1] - 1
        assert (res.column("n") == right - left + 1).all()
        u = Fraction(1, 1 << 53)
        for j in range(0, len(res), 17):                                   # the header's bound, m the frame's own row count, in exact arithmetic
            vals = [Fraction(float(x)) for x in rev[left[j]:right[j] + 1]]
            m = len(vals)
            assert abs(Fraction(float(res.column("week")[j])) - sum(vals)) <= (m - 1) * u / (1 - (m - 1) * u) * sum(abs(x) for x in vals), j
        m = (right - left + 1).astype(np.float64)
        mag = np.concatenate(([0.0], np.cumsum(np.abs(rev))))
        return (m - 1) * uf / (1 - (m - 1) * uf), mag[right + 1] - mag[left]

    by, order = ["o_shippriority"], [("o_orderdate", "asc")]
    dev = Q.q3.ranged(by, order, Q3_GROUPS, unit="groups")(*args)
    note = {"k": ALL, "order": ["o_orderdate"], "ranked": [], "per": by, "unit": "groups", "ranges": [["week", "sum", "revenue", -6, 0, None], ["n", "count", None, -6, 0, None]]}
    assert eng.stats()["order_routes"][-1] == dict(note, route="window_range")
    groups(dev)
    monkeypatch.setattr(eng, "device_window_range", False)
    host = Q.q3.ranged(by, order, Q3_GROUPS, unit="groups")(*args)
    assert eng.stats()["order_routes"][-1] == dict(note, route="host")
    gamma, mag = groups(host)
    for c in ("o_orderdate", "o_shippriority", "n"):
        assert close(host.column(c), dev.column(c)), c
    assert (np.abs(dev.column("week") - host.column("week")) <= (2 * gamma + RUN_TO_RUN) * mag).all()
    monkeypatch.setattr(eng, "device_window_range", True)

    # every order whose revenue lies within 1000 of this one's, per order date
    def value(res):
        assert res.columns[-2:] == list(Q3_VALUE) and [res.column(c).dtype for c in Q3_VALUE] == [np.int64, np.float64]
        x = np.asarray(res.column("revenue"))
        start, end = _partitions(res, ["o_orderdate"])
        n = len(res)
        pos = np.arange(n)
        assert (x[1:] <= x[:-1])[start[1:] != pos[1:]].all()
        for j in range(0, n, 3):
            s, e = start[j], end[j]
            inside = (x[s:e + 1] >= x[j] - 1000.0) & (x[s:e + 1] <= x[j] + 1000.0)
            assert res.column("near")[j] == inside.sum() and res.column("best")[j] == x[s:e + 1][inside].max(), j

    by, order = ["o_orderdate"], [("revenue", "desc")]
    dev = Q.q3.ranged(by, order, Q3_VALUE)(*args)
    note = {"k": ALL, "order": ["revenue"], "ranked": [], "per": by, "unit": "value", "ranges": [["near", "count", None, -1000.0, 1000.0, None], ["best", "max", "revenue", -1000.0, 1000.0, None]]}
    assert eng.stats()["order_routes"][-1] == dict(note, route="window_range")
    value(dev)
    monkeypatch.setattr(eng, "device_window_range", False)
    host = Q.q3.ranged(by, order, Q3_VALUE)(*args)
    assert eng.stats()["order_routes"][-1] == dict(note, route="host")
    value(host)
    for c in ("o_orderdate", "revenue", "near", "best"):                     # the exact columns exactly (revenue: two runs of the query sum in another order)
        assert close(host.column(c), dev.column(c)), c
    monkeypatch.setattr(eng, "device_window_range", True)
    # more than four: on the host
    five = {"a%d" % i: ("count", None, -float(i), float(i)) for i in range(5)}
    wide = Q.q3.ranged(by, order, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns[-5:] == list(five) and (wide.column("a0") >= 1).all()
    # q16: text fields in a mixed-radix key partition; the order column is a count the table keeps as integer-valued doubles: exact
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    res = Q.q16.ranged(["p_brand"], [("supplier_cnt", "desc")], {"n": ("count", None, -2, 2), "low": ("min", "supplier_cnt", -2, 2)}, unit="value")(*args16)
    route = eng.stats()["order_routes"][-1]
    assert route["route"] == "window_range" and route["per"] == ["p_brand"] and route["unit"] == "value"
    assert route["ranges"] == [["n", "count", None, -2, 2, None], ["low", "min", "supplier_cnt", -2, 2, None]]
    assert [res.column(c).dtype for c in ("n", "low")] == [np.int64] * 2 and len(res) > 100
    cnt = np.asarray(res.column("supplier_cnt"))
    start, end = _partitions(res, ["p_brand"])
    for j in range(0, len(res), 5):
        x = cnt[start[j]:end[j] + 1]
        inside = np.abs(x - cnt[j]) <= 2
        assert res.column("n")[j] == inside.sum() and res.column("low")[j] == x[inside].min(), j
    # an offset no int64 holds: the host saturates it (every row of the brand lies within 10^30 of every other)
    far = Q.q16.ranged(["p_brand"], [("supplier_cnt", "desc")], {"n": ("count", None, -10 ** 30, 10 ** 30), "g": ("count", None, -10 ** 30, 0)}, unit="value")(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    s16, e16 = _partitions(far, ["p_brand"])
    assert (far.column("n") == e16 - s16 + 1).all()
    far = Q.q16.ranged(["p_brand"], [("supplier_cnt", "desc")], {"g": ("count", None, -10 ** 30, 0)}, unit="groups")(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and (far.column("g")[s16 == np.arange(len(far))] >= 1).all()
    # a value frame over a text column has no arithmetic, whatever the device orders it by (a sorted dictionary's code is a plain
    # number there): the host's to refuse.  A group frame over the same column counts brands, on the device.
    with pytest.raises(ValueError):
        Q.q16.ranged(["p_size"], [("p_brand", "asc")], {"x": ("count", None, -1, 1)}, unit="value")(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    with pytest.raises(ValueError):
        Q.q16.ranged(["p_size"], [("p_type", "desc")], {"x": ("sum", "supplier_cnt", None, 0)}, unit="value")(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    res = Q.q16.ranged(["p_size"], [("p_brand", "asc")], {"n": ("count", None, -1, 1)}, unit="groups")(*args16)
    assert eng.stats()["order_routes"][-1]["route"] == "window_range" and eng.stats()["order_routes"][-1]["unit"] == "groups"
    brand = np.asarray(res.column("p_brand"))
    start, end = _partitions(res, ["p_size"])
    for j in range(0, len(res), 7):
        b = brand[start[j]:end[j] + 1]
        names = np.unique(b)
        at = np.searchsorted(names, brand[j])
        assert res.column("n")[j] == np.isin(b, names[max(0, at - 1):at + 2]).sum(), j
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


@pytest.fixture(scope="module")
def db22():
    from sdqlpy_amd import tpch
    return tpch.generate(0.05, tables=sorted(tpch.columns_for(["q22"])), columns=tpch.columns_for(["q22"]))


def test_a_value_frame_over_a_substr_part_is_refused(on_the_decorator, db22):
    """q22 groups by substr(c_phone, 0, 1): in a device table the country code is a number made of the text's code units, on the host
    it is text.  VALUE over it is a ValueError whichever way the result is ordered (test_window_range_cpu checks the routing decision
    for a substr part of a mixed-radix key by itself); GROUPS over it counts codes."""
    eng = on_the_decorator
    args = [db22[t] for t in Q.QUERY_TABLES["q22"]]
    plain = Q.q22.order_by([("cntrycode", "asc")])(*args)
    assert len(plain) == 7 and np.asarray(plain.column("cntrycode")).dtype.kind == "U"
    with pytest.raises(ValueError):
        Q.q22.ranged([], [("cntrycode", "asc")], {"x": ("count", None, -1, 1)}, unit="value")(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host"
    res = Q.q22.ranged([], [("cntrycode", "asc")], {"n": ("count", None, -1, 1), "cust": ("sum", "numcust", -1, 0)}, unit="groups")(*args)
    assert (np.asarray(res.column("cntrycode")) == np.asarray(plain.column("cntrycode"))).all()
    cust = np.asarray(res.column("numcust"))
    assert res.column("n").tolist() == [2, 3, 3, 3, 3, 3, 2] and (res.column("cust") == cust + np.concatenate(([0], cust[:-1]))).all()


@pytest.fixture(scope="module")
def suppliers():
    from sdqlpy_amd import tpch
    from order_terms_queries import SUPPLIER_COLUMNS, shuffled_suppliers
    plain = tpch.generate(0.05, tables=["supplier"], columns={"supplier": SUPPLIER_COLUMNS})["supplier"]
    return {"plain": plain, "shuffled": shuffled_suppliers(plain)}


def test_value_frames_over_the_columns_of_a_built_table(on_the_decorator, suppliers):
    """A unique build finished directly (no aggregation: the other way a result reaches the host).  Its text payload is row references
    into s_name: in the generated table they increase with the text and the device orders by them as plain numbers, in the shuffled
    one through a rank table.  Either way the column is text: a value frame over it is the host's ValueError, a group frame runs on
    the device.  The halves of a packed key are numbers: value frames over them run on the device."""
    from order_terms_queries import suppliers_by_name, suppliers_by_pair
    eng = on_the_decorator
    for which, ranked in (("plain", []), ("shuffled", ["s_name"])):
        table = suppliers[which]
        with pytest.raises(ValueError):
            suppliers_by_name.ranged([], [("s_name", "asc")], {"x": ("count", None, -1, 1)}, unit="value")(table)
        assert eng.stats()["order_routes"][-1]["route"] == "host", which
        with pytest.raises(ValueError):
            suppliers_by_name.ranged(["s_nationkey"], [("s_name", "desc")], {"x": ("sum", "s_suppkey", None, 0)}, unit="value")(table)
        assert eng.stats()["order_routes"][-1]["route"] == "host", which
        res = suppliers_by_name.ranged([], [("s_name", "asc")], {"n": ("count", None, -1, 1), "first": ("first", "s_suppkey", 0, 0)}, unit="groups")(table)
        route = eng.stats()["order_routes"][-1]
        assert route["route"] == "window_range" and route["ranked"] == ranked and route["unit"] == "groups", (which, route)
        names = np.asarray(res.column("s_name"))
        assert len(res) > 100 and (names[1:] >= names[:-1]).all()
        uniq, at, per = np.unique(names, return_inverse=True, return_counts=True)
        at = at.reshape(-1)
        pad = np.concatenate(([0], per, [0]))
        assert (res.column("n") == pad[at] + pad[at + 1] + pad[at + 2]).all(), which
        head = np.concatenate(([True], names[1:] != names[:-1]))
        assert (res.column("first") == np.asarray(res.column("s_suppkey"))[np.maximum.accumulate(np.where(head, np.arange(len(res)), 0))]).all(), which
    res = suppliers_by_pair.ranged(["s_nationkey"], [("s_suppkey", "desc")], {"n": ("count", None, -5, 5), "top": ("max", "s_acctbal", -5, 5)}, unit="value")(suppliers["plain"])
    route = eng.stats()["order_routes"][-1]
    assert route["route"] == "window_range" and route["unit"] == "value" and route["per"] == ["s_nationkey"], route
    nation, key, bal = (np.asarray(res.column(c)) for c in ("s_nationkey", "s_suppkey", "s_acctbal"))
    assert len(res) > 100 and (nation[1:] >= nation[:-1]).all()
    for j in range(0, len(res), 3):
        inside = (nation == nation[j]) & (np.abs(key - key[j]) <= 5)
        assert res.column("n")[j] == inside.sum() and res.column("top")[j] == bal[inside].max(), j
