"""GROUP BY ROLLUP / CUBE / GROUPING SETS over the entries of a table on the MI355X (run with -m gpu): sdqh_table_grouping_sets
(include/sdqh_sort_groups.h) against numpy at every size at which the sort, the wave batches or the tile carries take another path, on
group patterns that put group ends on those edges, at every mask of levels, against exact rational sums, against its sibling
sdqh_table_window_agg, on every table layout, over derived and text-ranked terms, and its contract.

The expected groups are the table's own rows (sdqh_table_compact) in the order of a STABLE numpy lexsort over the documented
order-preserving map (test_window_gpu.Ranked), cut where the images of neighbours differ in one of the level's first L terms and
folded with numpy's reduceat.  Nothing is imported from the product's fold code.  Doubles in exact comparisons are integer-valued
and below 2^40, so their sums are exact in any association."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from test_window_gpu import Ranked, _images, _probed_table, _same, _sort_bits, _stage_rows, _table, _under, db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)
from test_window_range_gpu import _range_table

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
SUM, COUNT, MIN, MAX, AVG = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WEX_AVG
OPS = (SUM, COUNT, MIN, MAX, AVG)
I_MIN, I_MAX = abi.INT64_MIN, abi.INT64_MAX
TOP = np.uint64(1) << np.uint64(63)
QNAN = 0x7FF8000000000000
UF = 2.0 ** -53
PACK = 1 << 20                                                              # payload 0 of the pattern tables = a * PACK + b
MEASURES = [(P, 3, False), (P, 2, True), (K, 0, False)]                    # _range_table's integers, its doubles, the key
COMBOS = [(op,) + m for op in OPS for m in MEASURES]


def _terms(desc):
    """(a, b, c): the two halves of payload 0 — derived terms — and payload 1"""
    return [(P, 0, desc, False, PACK, 0, 0, None), (P, 0, desc, False, 1, PACK, 0, None), (P, 1, desc, False)]


def _column(rows, kind, index):
    keys, payload, values, hits = rows
    return keys if kind == K else payload[index] if kind == P else values[index] if kind == V else hits


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Grouped:
    """The groups of every level 0 .. nterms of the rows in the order of `terms`, and aggregates over them, by numpy."""

    def __init__(self, rows, terms, rank_tables=None):
        self.rows, self.nterms = rows, len(terms)
        self.ranked = Ranked(rows, terms, len(terms), rank_tables)
        self.n, self.order = self.ranked.n, self.ranked.order
        imgs = _images(rows, terms, rank_tables)
        differ = np.zeros(self.n, bool)
        self.heads = []
        for L in range(self.nterms + 1):
            h = differ.copy()
            if self.n:
                h[0] = True
            self.heads.append(h)
            if L < self.nterms and self.n:
                s = imgs[L][self.order]
                differ[1:] |= s[1:] != s[:-1]
        self.starts = [np.nonzero(h)[0] for h in self.heads]

    def levels(self, mask):
        return [L for L in range(self.nterms, -1, -1) if (mask >> L) & 1]

    def level_rows(self, mask):
        out = np.zeros(abi.SORT_MAX_KEYS + 1, np.int64)
        for L in self.levels(mask):
            out[L] = len(self.starts[L])
        return out

    def positions(self, mask):
        """sorted positions of the representatives, in output order"""
        return np.concatenate([self.starts[L] for L in self.levels(mask)] + [np.zeros(0, np.int64)]).astype(np.int64)

    def sizes(self, L):
        return np.diff(np.concatenate([self.starts[L], [self.n]]))

    def value(self, L, agg):
        """aggregate `agg` = (op, kind, index, is_f64) of every level-L group: an int64 or float64 array"""
        op, kind, index, is_f64 = agg
        st = self.starts[L]
        f64 = op != COUNT and (kind == V or (kind == P and is_f64))
        if not self.n:
            return np.zeros(0, np.float64 if (f64 or op == AVG) else np.int64)
        cnt = self.sizes(L).astype(np.int64)
        if op == COUNT:
            return cnt
        src = np.ascontiguousarray(_column(self.rows, kind, index))[self.order]
        src = src.view(np.float64) if f64 and src.dtype != np.float64 else src
        if op in (SUM, AVG):
            s = np.add.reduceat(src, st) if f64 else np.add.reduceat(src.view(np.uint64), st).view(np.int64)
            return s if op == SUM else s.astype(np.float64) / cnt.astype(np.float64)
        img = _sort_bits(src, f64, op == MIN)                               # MIN: the complement, so that both are an unsigned maximum
        if f64:
            img = np.where(np.isnan(src), np.uint64(0), img)
        e = np.maximum.reduceat(img, st)
        u = ~e if op == MIN else e
        if not f64:
            return (u ^ TOP).view(np.int64)
        out = np.where(u >> np.uint64(63) != 0, u ^ TOP, ~u)
        return np.where(e == 0, np.uint64(QNAN), out).view(np.float64)

    def column(self, mask, agg):
        return np.concatenate([self.value(L, agg) for L in self.levels(mask)])


def _expect_dtype(agg):
    op, kind, _, is_f64 = agg
    return np.float64 if op == AVG or (op != COUNT and (kind == V or (kind == P and is_f64))) else np.int64


def _check(ctx, t, ref, terms, mask, aggs, what, limit=ALL, want_hits=False, min_hits=0):
    got = ctx.table_grouping_sets(t, min_hits, terms, mask, aggs, limit, 64, want_hits=want_hits)
    pos = ref.positions(mask)[:limit]
    _same(got, ref.rows, ref.order[pos], what)
    assert (got[5] == ref.level_rows(mask)).all(), (what, "level rows", got[5])
    assert len(got[4]) == len(aggs)
    for a, agg in enumerate(aggs):
        want = ref.column(mask, agg)[:limit]
        assert got[4][a].dtype == _expect_dtype(agg) == want.dtype, (what, agg, got[4][a].dtype, want.dtype)
        same = _bits(got[4][a]) == _bits(want)
        assert same.all(), (what, agg, int(np.argmin(same)), got[4][a][~same][:4], want[~same][:4])
    return got


def _sizes(ctx):
    T = ctx.window_geometry()
    S = ctx.sort_geometry()[0]
    assert ctx.grouping_sets_geometry() == T
    return T, S, sorted({0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, S - 1, S, S + 1, 4095, 4096, 4097, 65537})


PATTERNS = ["nested runs", "every row alone", "one group", "a finest group over three tiles", "edges", "same groups at two levels"]


def _pattern(name, n, T):
    """(a, b, c) by sorted position, each non-decreasing"""
    pos = np.arange(n, dtype=np.int64)
    a, b, c = pos // (T + 37), pos // 67, pos // 3
    if name == "every row alone":
        c = pos
    elif name == "one group":
        a, b, c = pos * 0, pos * 0, pos * 0
    elif name == "a finest group over three tiles":
        a = pos * 0
        lo, hi = T - 10, min(n, 3 * T + 6)
        if lo < n:
            b[lo:hi], c[lo:hi] = b[lo], c[lo]
    elif name == "edges":
        starts = np.array([63, 64, 65, T - 1, T, T + 1])
        c = np.searchsorted(starts, pos, side="right").astype(np.int64)
        a, b = c // 4, c // 2
    elif name == "same groups at two levels":
        b = pos * 0
    return a, b, c


def _pattern_table(ctx, name, n, T, desc, rng):
    a, b, c = _pattern(name, n, T)
    if desc and n:
        a, b, c = a.max() - a, b.max() - b, c.max() - c
    ints = rng.integers(-1000, 1000, n).astype(np.int64)
    if n > 2:
        ints[rng.integers(0, n, 2)] = [I_MIN, I_MAX]
    if n > 70:
        ints[[61, 62, 63, 64]] = [I_MAX, I_MAX, I_MIN, I_MIN]
    dbls = rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64)
    mix = rng.permutation(n)                                                # rows in random build order
    return _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], ints[mix])


# 1. patterns x sizes x levels, exact by bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_numpy(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S, sizes = _sizes(ctx)
    rng = np.random.default_rng(PATTERNS.index(pattern))
    for i, n in enumerate(sizes):
        desc = bool(i & 1)
        terms = _terms(desc)
        t = _pattern_table(ctx, pattern, n, T, desc, rng)
        try:
            rows = _stage_rows(ctx, t, 0)
            ref = Grouped(rows, terms)
            assert ref.n == n
            for k, mask in enumerate((0b1111, 0b0001, 0b1000, 0b0101, 0b1010)):
                at = (i * 5 + k) * 4
                aggs = [COMBOS[(at + j) % len(COMBOS)] for j in range(4)] if k else [(COUNT, K, 0, False)] + [COMBOS[(at + j) % len(COMBOS)] for j in range(3)]
                what = (pattern, n, bin(mask))
                got = _check(ctx, t, ref, terms, mask, aggs, what)
                g = int(ref.level_rows(mask).sum())
                assert ctx.table_grouping_sets_count(t, 0, terms, mask)[0] == g == len(got[0]), what
                assert (ctx.table_grouping_sets_count(t, 0, terms, mask)[1] == ref.level_rows(mask)).all(), what
                again = ctx.table_grouping_sets(t, 0, terms, mask, aggs, ALL, g)
                assert all((_bits(x) == _bits(y)).all() for x, y in zip(got[4], again[4])), what
                if not k and n:                                            # the COUNTs of every level add up to n
                    at0 = 0
                    for L in ref.levels(mask):
                        m = int(ref.level_rows(mask)[L])
                        assert int(got[4][0][at0:at0 + m].sum()) == n, (what, L)
                        at0 += m
            if n > 1:                                                       # limit cuts the output, not the groups; a capacity too small
                _check(ctx, t, ref, terms, 0b1111, [COMBOS[0], COMBOS[13]], (pattern, n, "limit"), limit=max(1, len(ref.positions(0b1111)) // 2))
        finally:
            t.free()
    if pattern == "a finest group over three tiles":
        assert (ref.sizes(3) > 2 * T).any() and len(ref.starts[2]) > 20
    if pattern == "edges":
        assert set(ref.starts[3]) == {0, 63, 64, 65, T - 1, T, T + 1}


# 2. eight terms, nine levels ------------------------------------------------------------------------------------------------------------
def test_eight_terms_nine_levels(hip_engine):
    ctx = hip_engine.ctx
    T, _, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(8)
    pos = np.arange(n, dtype=np.int64)
    divs = [T + 37, 300, 130, 67, 31, 9, 4, 2]                              # term i = position // divs[i]: nested divisions
    assert abi.SORT_MAX_KEYS == len(divs) and n // 2 < 1024
    ints = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    mix = rng.permutation(n)
    # payload 0 .. 1 carry the eight digits (10 bits each: five in one word, three in the other)
    hi, lo = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for d in divs[:5]:
        hi = hi * 1024 + (pos // d) % 1024
    for d in divs[5:]:
        lo = lo * 1024 + (pos // d) % 1024
    t = _range_table(ctx, hi[mix], lo[mix], rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64)[mix], ints[mix])
    terms = [(P, 0, False, False, 1024 ** (4 - i), 1024, 0, None) for i in range(5)] + [(P, 1, bool(i & 1), False, 1024 ** (2 - i), 1024, 0, None) for i in range(3)]
    try:
        ref = Grouped(_stage_rows(ctx, t, 0), terms)
        aggs = [(SUM, P, 3, False), (MIN, P, 3, False), (MAX, P, 2, True), (AVG, P, 2, True)]
        got = _check(ctx, t, ref, terms, 0b111111111, aggs, "eight terms")
        counts = ref.level_rows(0b111111111)
        assert counts[0] == 1 and counts[8] > counts[4] > counts[1] > 1
        # nesting: a level's groups fold into the groups of the level below it
        off = {L: int(counts[L + 1:].sum()) for L in range(9)}
        for L in range(8, 0, -1):
            fine = slice(off[L], off[L] + int(counts[L]))
            parent = np.cumsum(ref.heads[L - 1][ref.starts[L]]) - 1
            coarse = slice(off[L - 1], off[L - 1] + int(counts[L - 1]))
            s = np.zeros(int(counts[L - 1]), np.uint64)
            np.add.at(s, parent, got[4][0][fine].view(np.uint64))
            assert (s.view(np.int64) == got[4][0][coarse]).all(), L
            lo_, hi_ = np.full(len(s), I_MAX, np.int64), np.full(len(s), -np.inf)
            np.minimum.at(lo_, parent, got[4][1][fine])
            np.maximum.at(hi_, parent, got[4][2][fine])
            assert (lo_ == got[4][1][coarse]).all() and (hi_ == got[4][2][coarse]).all(), L
    finally:
        t.free()


# 3. nothing is subtracted and nothing leaks -------------------------------------------------------------------------------------------
def test_nothing_is_subtracted_and_nothing_leaks(hip_engine):
    ctx = hip_engine.ctx
    T, _, _ = _sizes(ctx)
    n = 2 * T + 50
    rng = np.random.default_rng(3)
    pos = np.arange(n, dtype=np.int64)
    a, b, c = pos // (T + 37), pos // 50, pos // 5
    assert (T - 1) // 5 == T // 5                                           # the finest group of position T - 1 crosses the tile edge
    dbls = rng.integers(-9, 10, n).astype(np.float64)
    dbls[T - 1], dbls[(T // 5 + 1) * 5 + 1] = 1e300, -1e300                 # ... in two neighbouring finest groups
    mix = rng.permutation(n)
    t = _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], pos[mix])
    terms = _terms(False)
    try:
        ref = Grouped(_stage_rows(ctx, t, 0), terms)
        aggs = [(SUM, P, 2, True), (AVG, P, 2, True), (COUNT, K, 0, False), (MAX, P, 2, True)]
        got = ctx.table_grouping_sets(t, 0, terms, 0b1111, aggs, ALL, 64)
        assert (got[5] == ref.level_rows(0b1111)).all()
        sorted_d = dbls                                                      # (a, b, c) are functions of the position: sorted position = pos
        at = 0
        seen = {"none": 0, "one": 0, "both": 0}
        for L in ref.levels(0b1111):
            st, size = ref.starts[L], ref.sizes(L)
            for j in range(len(st)):
                v = sorted_d[st[j]:st[j] + size[j]]
                huge = int((np.abs(v) > 1e200).sum())
                assert got[4][2][at + j] == size[j] and got[4][3][at + j] == v.max(), (L, j)
                if huge == 0:
                    assert got[4][0][at + j] == v.sum() and got[4][1][at + j] == v.sum() / size[j], (L, j)
                elif huge == 1:                                            # the small ones vanish beside it, in any order
                    assert abs(got[4][0][at + j]) == 1e300, (L, j)
                seen[("none", "one", "both")[huge]] += 1
            at += len(st)
        assert seen["none"] > 100 and seen["one"] == 2 and seen["both"] >= 3
    finally:
        t.free()


# 4. general doubles within the header's bound -------------------------------------------------------------------------------------------
def test_general_doubles_within_the_bound(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    for n in (S + 1, 4097):
        rng = np.random.default_rng(n)
        pos = np.arange(n, dtype=np.int64)
        a, b, c = pos // (T + 37), pos // 67, pos // 3
        dbls = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)
        mix = rng.permutation(n)
        t = _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], pos[mix])
        terms = _terms(False)
        try:
            ref = Grouped(_stage_rows(ctx, t, 0), terms)
            aggs = [(SUM, P, 2, True), (COUNT, K, 0, False), (AVG, P, 2, True)]
            got = ctx.table_grouping_sets(t, 0, terms, 0b1111, aggs, ALL, 64)
            again = ctx.table_grouping_sets(t, 0, terms, 0b1111, aggs, ALL, 64)
            assert all((_bits(x) == _bits(y)).all() for x, y in zip(got[4], again[4]))
            assert (_bits(got[4][2]) == _bits(got[4][0] / got[4][1].astype(np.float64))).all()
            at = checked = 0
            for L in ref.levels(0b1111):
                st, size = ref.starts[L], ref.sizes(L)
                assert (got[4][1][at:at + len(st)] == size).all()
                for j in range(0, len(st), 37):
                    v = dbls[st[j]:st[j] + size[j]]
                    m = int(size[j])
                    exact = sum((Fraction(float(x)) for x in v), Fraction(0))
                    gamma = Fraction((m - 1) * UF) / (1 - Fraction((m - 1) * UF))
                    assert abs(Fraction(float(got[4][0][at + j])) - exact) <= gamma * sum(Fraction(abs(float(x))) for x in v), (n, L, j)
                    checked += 1
                at += len(st)
            assert checked >= 10
        finally:
            t.free()


# 5. agreement with the sibling ---------------------------------------------------------------------------------------------------------
def test_agreement_with_window_agg(hip_engine):
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 2 * T + 77
    rng = np.random.default_rng(5)
    pos = np.arange(n, dtype=np.int64)
    a, b, c = pos // (T + 37), pos // 67, pos // 3
    wild = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-20, 20, n)
    mix = rng.permutation(n)
    terms = _terms(True)
    for dbls, exact in ((rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64), True), (wild, False)):
        t = _range_table(ctx, (a * PACK + b)[mix], c[mix], dbls[mix], rng.integers(-(1 << 62), 1 << 62, n)[mix])
        try:
            ref = Grouped(_stage_rows(ctx, t, 0), terms)
            aggs = [(COUNT, K, 0, False), (MIN, P, 2, True), (SUM, P, 3, False), (SUM, P, 2, True)]
            got = ctx.table_grouping_sets(t, 0, terms, 0b1111, aggs, ALL, 64)
            at = 0
            for L in ref.levels(0b1111):
                sib = ctx.table_window_agg(t, 0, L, terms, [(op, abi.FRAME_PARTITION, k, i, f) for op, k, i, f in aggs], ALL, n, want_hits=False)
                st = ref.starts[L]
                assert (got[0][at:at + len(st)] == sib[0][st]).all(), L
                for x in range(3):
                    assert (_bits(got[4][x][at:at + len(st)]) == _bits(sib[4][x][st])).all(), (L, x)
                mine, theirs = got[4][3][at:at + len(st)], sib[4][3][st]
                if exact:
                    assert (_bits(mine) == _bits(theirs)).all(), L
                else:
                    sorted_abs = np.abs(np.ascontiguousarray(ref.rows[1][2]).view(np.float64)[ref.order])
                    mass = np.add.reduceat(sorted_abs, st)
                    m = ref.sizes(L).astype(np.float64)
                    g = (m - 1) * UF / (1 - (m - 1) * UF)
                    assert (np.abs(mine - theirs) <= 2 * g * mass * (1 + 1e-9)).all(), L
                at += len(st)
            # the distinct combinations alone: no aggregates
            only = ctx.table_grouping_sets(t, 0, terms, 0b1000, [], ALL, 64)
            _same(only, ref.rows, ref.order[ref.starts[3]], "distinct")
            assert only[4] == [] and only[5][3] == len(ref.starts[3]) == len(only[0])
            dense = ctx.table_window(t, 0, 3, terms, abi.WIN_ROW_NUMBER, 1, ALL, 64, want_hits=False)
            assert (dense[0] == only[0]).all()
        finally:
            t.free()


# 6. layouts, derived terms and text -------------------------------------------------------------------------------------------------------
def test_layouts(hip_engine):
    """The direct layout, a table with duplicate build keys (owner rows only), the open-addressing layout, the probed table of the
    ordering tests, each with min_hits 0 and 2; VALUE and HITS as terms and as measures — every op over HITS."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    n = 2 * T + 1
    rng = np.random.default_rng(n)
    part = rng.integers(0, 9, n).astype(np.int64)
    value = rng.integers(-50, 50, n).astype(np.float64)
    hits = rng.integers(0, 4, n)                                           # some entries never probed: min_hits selects
    term_lists = [[(P, 0, True, False), (H, 0, False, False)], [(H, 0, True, False), (P, 0, False, False), (V, 0, False, True)]]
    agg_lists = [[(SUM, V, 0, True), (MAX, H, 0, False), (AVG, H, 0, False), (MIN, V, 0, True)],
                 [(SUM, H, 0, False), (MIN, H, 0, False), (COUNT, H, 0, False), (AVG, V, 0, True)]]

    def run(dups):
        t = _table(ctx, part, value, hits, dups=dups)
        done = 0
        try:
            for mh in (0, 2):
                rows = _stage_rows(ctx, t, mh)
                for terms in term_lists:
                    ref = Grouped(rows, terms)
                    assert 0 < ref.n < n + 1 and (mh == 0 or ref.n < n)
                    for aggs in agg_lists:
                        _check(ctx, t, ref, terms, (1 << (len(terms) + 1)) - 1, aggs, ("layout", dups, mh), want_hits=True, min_hits=mh)
                        done += 1
        finally:
            t.free()
        return done
    assert run(0) == 8
    assert run(200) == 8
    assert _under(hip_engine, {"direct_index": 0, "row_index": 0, "grouped_index": 0}, lambda: run(200)) == 8
    t = _probed_table(ctx, S + 1)
    try:
        pt = [(P, 0, False, False), (V, 0, False, True)]
        pa = [(AVG, P, 1, True), (MAX, P, 1, True), (COUNT, K, 0, False), (SUM, H, 0, False)]      # (the double payload counts in quarters: its sums are exact)
        for mh in (0, 2):
            ref = Grouped(_stage_rows(ctx, t, mh), pt)
            _check(ctx, t, ref, pt, 0b111, pa, ("probed", mh), want_hits=True, min_hits=mh)
            _check(ctx, t, ref, pt, 0b010, pa[::-1], ("probed", mh, "one level"), want_hits=True, min_hits=mh)
    finally:
        t.free()


def test_text_ranked_terms_and_nans_beside_them(hip_engine):
    """GROUP BY the high half of a packed key, a text behind a payload of row references (its ranks column) and the key's low half;
    a double measure with NaNs beside them; a ranks column too short for the references is the error of sdqh_table_window."""
    ctx = hip_engine.ctx
    T, S, _ = _sizes(ctx)
    rng = np.random.default_rng(5)
    words = np.array(["pear", "apple", "fig", "apple ", "Fig", "quince", "plum", "pea", "", "zz"])
    text = words[rng.integers(0, len(words), 41)]
    ct, distinct = ctx.text_ranks(ctx.upload(text), len(text))
    want = np.unique(text, return_inverse=True)[1].reshape(-1).astype(np.int64)
    short = ctx.upload(want[:20])
    try:
        for n in (T + 1, S + 1):
            a = rng.integers(0, n // 90 + 2, n).astype(np.int64)
            b = rng.integers(0, 40, n).astype(np.int64)
            keys = np.unique((a << 32) | b)
            keys = keys[rng.permutation(len(keys))]
            ref_col = rng.integers(0, len(text), len(keys)).astype(np.int64)
            dbls = rng.integers(-9, 9, len(keys)).astype(np.float64)
            dbls[rng.integers(0, len(keys), len(keys) // 3)] = np.nan
            dbls[:4] = [-0.0, 0.0, np.inf, -np.inf]
            t = ctx.hash_build_unique(len(keys), abi.make_filter(), [], ctx.upload(keys), [ctx.upload(ref_col), ctx.upload(dbls.view(np.int64))], accumulate=False)
            try:
                terms = [(K, 0, False, False, 1 << 32, 0, 0, None), (P, 0, True, False, 0, 0, 0, ct), (K, 0, False, False, 0, 1 << 32, 0, None)]
                ref = Grouped(_stage_rows(ctx, t, 0), terms, {id(ct): want})
                assert ref.n == len(keys) and len(ref.starts[1]) < len(ref.starts[2]) < len(ref.starts[3]) == ref.n
                aggs = [(MIN, P, 1, True), (MAX, P, 1, True), (COUNT, K, 0, False), (SUM, P, 0, False)]
                for mask in (0b0100, 0b0110, 0b1111):
                    got = _check(ctx, t, ref, terms, mask, aggs, ("text", n, bin(mask)))
                assert np.isnan(got[4][0]).any() and not np.isnan(got[4][0]).all()      # groups of nothing but NaNs, and others
                bad = [terms[0], (P, 0, True, False, 0, 0, 0, short), terms[2]]
                keys_out, out, lr = np.full(len(keys), -7, np.int64), np.full(len(keys), -7, np.int64), np.full(9, -7, np.int64)
                assert _raw(ctx, t, bad, 0b1111, aggs[2:3], ALL, len(keys), keys_out, out, lr) == (abi.ERR_INVALID, -7)
                assert (keys_out == -7).all() and (out == -7).all() and (lr == -7).all()
                assert b"term 1" in ctx.lib.sdqh_last_error(ctx.handle)
                _check(ctx, t, ref, terms, 0b1111, aggs, ("text", n, "usable after the error"))
            finally:
                t.free()
    finally:
        ct.free(); short.free()


def test_nan_extrema(hip_engine):
    ctx = hip_engine.ctx
    n = 700
    pos = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(7)
    dbls = rng.integers(-5, 5, n).astype(np.float64)
    dbls[rng.integers(0, n, 200)] = np.nan
    dbls[3:9] = np.nan                                                       # finest groups with nothing but NaNs
    dbls[[20, 21]] = [-0.0, 0.0]
    dbls[[30, 33]] = [np.inf, -np.inf]
    t = _range_table(ctx, (pos // 100) * PACK + pos // 30, pos // 3, dbls, pos)
    terms = _terms(False)
    try:
        ref = Grouped(_stage_rows(ctx, t, 0), terms)
        got = _check(ctx, t, ref, terms, 0b1111, [(MIN, P, 2, True), (MAX, P, 2, True), (COUNT, K, 0, False)], "nan")
        assert np.isnan(got[4][0]).any() and not np.isnan(got[4][0]).all()
    finally:
        t.free()


# 7. the contract ------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, t, terms, levels, aggs, limit, capacity, keys=None, out=None, level_rows=None, nterms=None, naggs=None, got=None):
    arr = (abi.GroupAgg * max(1, len(aggs)))()
    for i, (op, kind, index, is_f64) in enumerate(aggs):
        arr[i].op, arr[i].kind, arr[i].index, arr[i].is_f64 = op, kind, index, int(is_f64)
    got = got if got is not None else C.c_int64(-7)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = ctx.lib.sdqh_table_grouping_sets(ctx.handle, t.handle, C.c_int64(0), C.c_int(len(terms) if nterms is None else nterms), abi._marshal_sort_terms(terms),
                                          C.c_uint32(levels), C.c_int(len(aggs) if naggs is None else naggs), arr, C.c_int64(limit), C.c_int64(capacity),
                                          ptr(keys), None, None, None, ptr(out), ptr(level_rows), C.byref(got))
    return rc, got.value


def test_sizes_errors_and_empties(hip_engine):
    ctx = hip_engine.ctx
    T, _, _ = _sizes(ctx)
    n = T + 9
    pos = np.arange(n, dtype=np.int64)
    t = _range_table(ctx, (pos // 100) * PACK + pos // 10, pos // 2, pos.astype(np.float64), pos)
    empty = _range_table(ctx, pos[:0], pos[:0], pos[:0].astype(np.float64), pos[:0])
    terms = _terms(False)
    try:
        ref = Grouped(_stage_rows(ctx, t, 0), terms)
        g = int(ref.level_rows(0b1111).sum())
        aggs = [(SUM, P, 3, False)]
        keys, out, lr = np.full(g, -7, np.int64), np.full(g, -7, np.int64), np.full(9, -7, np.int64)
        assert _raw(ctx, t, terms, 0b1111, aggs, ALL, g - 1, keys, out, lr) == (abi.ERR_OVERFLOW, g)
        assert (keys == -7).all() and (out == -7).all()
        assert _raw(ctx, t, terms, 0b1111, aggs, 5, 5, keys, out, lr) == (abi.OK, 5) and (keys[5:] == -7).all() and (out[5:] == -7).all()
        assert (lr == ref.level_rows(0b1111)).all()
        assert _raw(ctx, t, terms, 0b1111, aggs, ALL, 0, None, None, lr) == (abi.OK, g)              # count only
        assert _raw(ctx, t, terms, 0b0110, aggs, ALL, g, keys, None, lr) == (abi.OK, int(ref.level_rows(0b0110).sum()))      # rows only
        assert (lr == ref.level_rows(0b0110)).all()
        lr[:] = -7
        assert _raw(ctx, empty, terms, 0b1111, aggs, ALL, 4, keys, out, lr) == (abi.OK, 0) and (lr == 0).all()
        for bad in (dict(levels=0), dict(levels=0b10000), dict(aggs=[(7, P, 3, False)]), dict(aggs=[(4, P, 3, False)]), dict(aggs=[(SUM, P, 9, False)]),
                    dict(aggs=[(SUM, K, 0, True)]), dict(aggs=[(SUM, H, 0, False)]), dict(naggs=-1), dict(naggs=5), dict(nterms=0), dict(nterms=9), dict(limit=0), dict(capacity=-1)):
            args = dict(levels=0b1111, aggs=aggs, limit=ALL, capacity=g, nterms=None, naggs=None)
            args.update(bad)
            keys[:], out[:], lr[:] = -7, -7, -7
            rc = _raw(ctx, t, terms, args["levels"], args["aggs"], args["limit"], args["capacity"], keys, out, lr, nterms=args["nterms"], naggs=args["naggs"])
            assert rc == (abi.ERR_INVALID, -7), (bad, rc)
            assert (keys == -7).all() and (out == -7).all() and (lr == -7).all(), bad
        _check(ctx, t, ref, terms, 0b1111, aggs, "usable after the errors")
    finally:
        t.free()
        empty.free()


# 8. through the engine and the decorator --------------------------------------------------------------------------------------------------
def test_q3_and_q16_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by = ["o_orderdate", "o_shippriority"]
    aggs = {"total": ("sum", "revenue"), "n": ("count", None), "best": ("max", "revenue"), "mean": ("avg", "revenue")}

    def both(run, calls):
        dev = run()
        note = eng.stats()["order_routes"][-1]
        assert note["route"] == "grouping_sets" and note["calls"] == calls, note
        monkeypatch.setattr(eng, "device_grouping_sets", False)
        host = run()
        assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["calls"] == 0
        monkeypatch.setattr(eng, "device_grouping_sets", True)
        assert dev.columns == host.columns and len(dev) == len(host) > 3
        return dev, host, note
    dev, host, note = both(lambda: Q.q3.rollup(by, aggs)(*args), 1)
    assert note["per"] == by and note["sets"] == [by, by[:1], []] and note["aggs"] == [[k] + list(v) for k, v in aggs.items()]
    assert dev.columns == by + list(aggs) + ["grouping"]
    assert [dev.column(c).dtype for c in aggs] == [host.column(c).dtype for c in aggs] == [np.float64, np.int64, np.float64, np.float64]
    for c in by + ["n", "best", "grouping"]:
        assert (np.asarray(dev.column(c)) == np.asarray(host.column(c))).all(), c
    n = np.asarray(dev.column("n")).astype(np.float64)
    for c in ("total", "mean"):                                             # double sums of one group's rows in two associations, and two runs of the query
        a, b = np.asarray(dev.column(c)), np.asarray(host.column(c))
        assert (np.abs(a - b) <= (2 * n * UF / (1 - n * UF) + 1e-12) * np.abs(b) * (1 if c == "total" else 2)).all(), c      # (revenues are positive: sum|v| = the sum)
    g = np.asarray(dev.column("grouping"))
    assert (g[:-1] <= g[1:]).all() and g[-1] == 3 and (g == 3).sum() == 1 and int(np.asarray(dev.column("n"))[-1]) == int(np.asarray(dev.column("n"))[g == 0].sum())
    # a cube: two chains, the sets back in listed order
    dev, host, note = both(lambda: Q.q3.cube(by, {"n": ("count", None)})(*args), 2)
    for c in dev.columns:
        assert (np.asarray(dev.column(c)) == np.asarray(host.column(c))).all(), c
    assert sorted(set(np.asarray(dev.column("grouping")).tolist())) == [0, 1, 2, 3]
    # text grouping columns go through their ranks; integer-valued sums come back as the integers they are
    args16 = [db[t] for t in Q.QUERY_TABLES["q16"]]
    sets16 = [("p_brand", "p_type"), ("p_brand",), ()]
    aggs16 = {"suppliers": ("sum", "supplier_cnt"), "most": ("max", "supplier_cnt"), "mean": ("avg", "supplier_cnt")}
    dev, host, note = both(lambda: Q.q16.grouping_sets(sets16, aggs16)(*args16), 1)
    assert [dev.column(c).dtype for c in aggs16] == [host.column(c).dtype for c in aggs16]
    for c in dev.columns:
        a, b = np.asarray(dev.column(c)), np.asarray(host.column(c))
        assert (a == b).all() if a.dtype.kind != "f" else (_bits(a) == _bits(b)).all(), c
    assert "" in np.asarray(dev.column("p_type")).tolist()
    # more than four aggregates: on the host
    five = dict(aggs, lo=("min", "revenue"))
    wide = Q.q3.rollup(by, five)(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == by + list(five) + ["grouping"]
    Q.q3.top(10, [("revenue", "desc")])(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]
