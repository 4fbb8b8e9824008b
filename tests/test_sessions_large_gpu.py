"""Sessions past 256 tiles on the MI355X (run with -m gpu): sdqh_table_sessions (include/sdqh_sort_sessions.h) against whole-array numpy
(sessions_numpy_reference) at the sizes at which a thread of the one-workgroup scans folds MORE THAN ONE tile.  test_sessions_gpu stops
at one such case (257 T + 3 rows, the gap rule ascending, four columns); test_window_large_gpu and test_group_large_gpu do not reach
sessions by reuse, because k_ss_heads writes the inputs of those scans itself:

    carryA   win_step(runA, partition heads, session heads): k_win_scan and a dense rank over it give SDQH_SS_NUMBER
    carryB   win_step(runB, session heads, session heads): a row number over it gives SDQH_SS_ROW and the session's start that FIRST
             and the per-row AVG use
    tfirst   the tile's first session head: k_wagg_scan's, and k_wagg_next scanned backwards gives tnext, the end of a session that
             runs on into later tiles — k_ss_rows reads it, over the tiles below `limit` only
    tcount   the session heads per tile: k_sort_bins' offsets, from which k_gs_run places the per-session shape's slots

    rows          tiles  per  runs at
    W T + 1       257    2    everything, ascending (a ragged last thread: thread 128 holds one tile)
    2 W T + T + 1 514    3    everything, descending (per does not divide the tiles)
    W T - 1, W T, 2 W T, 2 W T + 1   one call per output shape, on one pattern

A pattern is (cut, ph) by sorted position: where the rule cuts and where a partition starts (_large).  The tables are
test_sessions_gpu's (_ss_table, _pattern_columns): the order value moves on by GAP + 1 exactly at a cut and by GAP or 1 elsewhere, the
marker changes exactly at the cuts, the doubles are multiples of 0.25 of small magnitude, so every partial sum is exact in every
association: everything is compared bit for bit.  Each pattern's structural claims (_claims; test_sessions_large_cpu asserts them on
synthetic flags) are asserted on the reference built from the DEVICE's staged rows.  Failure messages name the first differing slot,
the sorted position it stands for, its tile and its thread run.

"mixed" is test_past_256_tiles' pattern.  That test runs at per = 2, so its multiples of T are multiples of half a thread run; here
each of them is scaled by per — it becomes that many half thread runs, per T / 2 positions each — so that at every size the pattern
keeps its place against the seams and fits below n.

CPU time of the reference at 262 657 rows on one core without a GPU (test_sessions_large_cpu prints it): the order 0.03 s, the order
and the heads 0.04 s, a set of four columns 0.01 s to 0.03 s ("every row its own session", the slowest).  Python loops run only over
the sampled sessions of the general-doubles test."""
from fractions import Fraction

import numpy as np
import pytest

import large_patterns as LP
import sessions_numpy_reference as nref
from sdqlpy_amd import abi
from test_sessions_gpu import GAP, MQ, MT, MX, OP, _field, _pattern_columns, _ss_table
from test_window_gpu import _images, _pattern as _window_pattern, _same, _stage_rows, _table, hip_engine      # noqa: F401 (fixture)
from test_window_large_gpu import FULL, LIGHT, W, _geometry, _rows_of, _thread_runs

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
U = Fraction(1, 1 << 53)
ONE, EACH, PARTS, S_SEAMS, P_SEAMS, MIXED = ("one session", "every row its own session", "every row its own partition", "session seams", "partition seams",
                                             "mixed")
PATTERNS = [ONE, EACH, PARTS, S_SEAMS, P_SEAMS, MIXED]
TAIL = [60, 1, 63, 64, 65, 200]
NUMBER, ROW, COUNT = (OP["number"], K, 0, False), (OP["row"], K, 0, False), (OP["count"], K, 0, False)
SETS = ([(OP["sum"],) + MX, (OP["avg"],) + MQ, NUMBER, ROW],               # test_exact_by_bits' three sets: all nine ops, on the integer, the
        [(OP["min"],) + MQ, (OP["max"],) + MX, (OP["first"],) + MT, (OP["last"],) + MT],      # double and the order column
        [(OP["sum"],) + MQ, COUNT, (OP["avg"],) + MX, (OP["last"],) + MQ])


# ---- patterns ----------------------------------------------------------------------------------------------------------------------------
def _large(name, n, T):
    """(cut, ph) by sorted position: where the rule cuts, where a partition starts"""
    per = _geometry(n, T)[1]
    pos = np.arange(n)
    cut, ph = np.zeros(n, bool), np.zeros(n, bool)
    ph[0] = True
    if name == EACH:
        cut[:] = True
    elif name == PARTS:
        ph[:] = True
    elif name == S_SEAMS:
        cut = LP.seam_heads(n, T, TAIL)
    elif name == P_SEAMS:
        ph = LP.seam_heads(n, T, TAIL)
        cut = LP.cyc_heads(n, [3, 1, 5, 2, 64, 65])
    elif name == MIXED:
        h = per * T // 2                                                    # half a thread run: T where test_past_256_tiles runs
        cut[pos % 3 == 0] = True
        cut[5 * h + 7:9 * h + 1] = False                                    # a session over two thread runs
        cut[20 * h:150 * h + 5] = False                                     # ... and 65 thread runs that only the partition heads cut: sessions of 20
        cut[200 * h + 3:200 * h + 3 + 3 * h:5] = True
        ph = pos % (40 * h + 11) == 0
    else:
        assert name == ONE
    return cut, ph


def _claims(name, sh, ph, n, T):
    """the structural claims of a pattern on head flags by sorted position (sh: session heads, ph: partition heads), n > W T"""
    ntiles, per, _ = _geometry(n, T)
    L = per * T
    assert n > W * T and per >= 2 and len(sh) == len(ph) == n and sh[0] and ph[0] and not (ph & ~sh).any()
    length = np.diff(np.append(np.nonzero(sh)[0], n))
    if name == ONE:
        assert sh.sum() == 1 and not _thread_runs(sh, n, T)[1:].any()      # every carry passes through every later thread's partial
    if name == EACH:
        assert sh.all() and ph.sum() == 1                                   # NUMBER climbs to n > W T: the per-session shape has n slots
    if name == PARTS:
        assert ph.all()
    if name == S_SEAMS:
        assert ph.sum() == 1
        on, before, after, swallowed, only_last = LP.seam_rule(sh, T, name)
        assert on >= 3 and swallowed >= 3 and only_last >= 3 and not _thread_runs(sh, n, T)[14:17].any()
        assert sh[14 * L - 5] and sh[17 * L + 3] and not sh[14 * L - 4:17 * L + 3].any()      # the session that swallows the thread runs 14 .. 16
    if name == P_SEAMS:
        LP.seam_rule(ph, T, name)
        assert not _thread_runs(ph, n, T)[14:17].any() and _thread_runs(sh, n, T).all()      # session heads go on where no partition starts
        assert (sh & ~ph)[14 * L:17 * L].sum() > 3 * L // 64
    if name == MIXED:
        assert (length == 1).sum() >= 10 and (length == 3).sum() > n // 16 and ((length >= 2 * L - 8) & (length < 3 * L)).any()
        assert length.max() == 20 * L + 11 and (length > 15 * L).sum() >= 2 and ph.sum() >= 5 and (sh & ~ph).any()      # (partition heads cut the 65 thread runs)
    return length


class Sessions:
    """The sessions of a table's staged rows under terms / npart / rule by sessions_numpy_reference: idx (the rows' order), heads,
    part_heads, starts."""

    def __init__(self, rows, terms, npart, rule):
        self.rows, self.n = rows, len(rows[0])
        self.idx = nref.order(rows, terms)
        part = [u[self.idx] for u in _images(rows, terms[:npart])]
        if rule[0] == abi.SS_GAP:
            kind, index, desc, is_f64 = terms[npart]
            f = bool(is_f64) or kind == V
            self.heads, self.part_heads = nref.heads(part, np.ascontiguousarray(_field(rows, kind, index, f))[self.idx], bool(desc), rule[1], f)
        else:
            marker = nref.bits(_field(rows, rule[1], rule[2]))[self.idx]
            self.heads, self.part_heads = nref.heads(part, None, False, None, False, marker_bits=marker)
        self.starts = np.nonzero(self.heads)[0]

    def columns(self, cols, per):
        spec = []
        for op, kind, index, is_f64 in cols:
            name = nref.OPS[op]
            if name in ("count", "number", "row"):
                spec.append((name, None, False))
            else:
                f = bool(is_f64) or kind == V
                spec.append((name, np.ascontiguousarray(_field(self.rows, kind, index, f))[self.idx], f))
        return nref.columns(self.heads, self.part_heads, spec, per)

    def order(self, per):
        return self.idx[self.starts] if per else self.idx


def _first_bad(got, want, where, n, T, what):
    """bit for bit; the message names the first differing slot, the sorted position it stands for (where[slot]: a session's first
    row; None: the slot itself), its tile and its thread run (seam)"""
    got, want = nref.bits(got), nref.bits(want)
    assert len(got) == len(want), (what, "rows", len(got), len(want))
    same = got == want
    if not same.all():
        j = int(np.argmin(same))
        at = int(where[j]) if where is not None else j
        L = _geometry(n, T)[1] * T
        raise AssertionError((what, "slot", j, "position", at, "tile", at // T, "thread run", at // L, "at", at % L, got[j:j + 3], want[j:j + 3]))


def _check(ctx, t, exp, terms, npart, rule, cols, what, T, min_hits=0, limit=ALL, pers=(False, True)):
    """one call per output shape against the reference: rows and columns by bits, the count-only call"""
    for per in pers:
        asked = [c for c in cols if not (per and c[0] == OP["row"])]
        order = exp.order(per)[:limit]
        shape = "per session" if per else "per row"
        got = ctx.table_sessions(t, min_hits, npart, terms, rule, asked, limit, len(order), per_session=per, want_hits=t.accumulate)
        _same(got, exp.rows, order, (what, shape))
        want = exp.columns(asked, per)
        assert len(got[4]) == len(asked)
        for c, a, w in zip(asked, got[4], want):
            f = c[0] == OP["avg"] or (c[0] in (OP["sum"], OP["min"], OP["max"], OP["first"], OP["last"]) and (bool(c[3]) or c[1] == V))
            assert a.dtype == (np.float64 if f else np.int64), (what, shape, c)
            _first_bad(a, w[:limit], exp.starts if per else None, exp.n, T, (what, shape, nref.OPS[c[0]], c[1:], "limit", limit))
        assert ctx.table_sessions_count(t, min_hits, npart, terms, rule, per_session=per, limit=limit) == len(order), (what, shape, "count")


def _columns_of(pattern, n, T, desc):
    """(cut, ph, (p, t, x, q)): the pattern and test_sessions_gpu's columns of it by sorted position"""
    rng = np.random.default_rng(PATTERNS.index(pattern) * 1000003 + n)
    cut, ph = _large(pattern, n, T)
    p, t, x, q = _pattern_columns(cut, ph, desc, rng)
    return cut, ph, (p, t, x, q)


# 0. the sizes reach what the file says they reach -------------------------------------------------------------------------------------------
def test_geometry(hip_engine):
    ctx = hip_engine.ctx
    T = ctx.window_geometry()
    assert ctx.sessions_geometry() == ctx.window_geometry() == 512
    assert [_geometry(_rows_of(s, T), T)[:2] for s in FULL] == [(257, 2), (514, 3)] and all(LP.ragged(_rows_of(s, T), T) for s in FULL)
    assert [_geometry(_rows_of(s, T), T)[1] for s in LIGHT] == [1, 1, 2, 3]


# 1. every pattern, both rules, all nine ops, both shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sessions(hip_engine, pattern, size):
    """The gap rule and the change rule, each on a table of its own, ascending at W T + 1 and descending at 2 W T + T + 1 (the other
    arm of ss_continues' unsigned difference); three sets of four columns in both shapes; the count-only calls."""
    ctx = hip_engine.ctx
    T = ctx.sessions_geometry()
    n = _rows_of(size, T)
    desc = size == FULL[1]
    cut, ph, (p, t, x, q) = _columns_of(pattern, n, T, desc)
    terms = [(P, 0, desc, False), (P, 1, desc, False)]
    for rule, third in (((abi.SS_GAP, GAP), x), ((abi.SS_CHANGE, P, 2, False), x // 1000)):
        tab = _ss_table(ctx, p, t, third, q)
        try:
            exp = Sessions(_stage_rows(ctx, tab, 0), terms, 1, rule)
            assert exp.n == n and (exp.heads == (cut | ph)).all() and (exp.part_heads == ph).all(), (pattern, n, rule[0])      # the pattern lies where it was placed
            _claims(pattern, exp.heads, exp.part_heads, n, T)
            if pattern == EACH:
                assert len(exp.starts) == n > W * T
            for cols in SETS:
                _check(ctx, tab, exp, terms, 1, rule, cols, (pattern, n, "desc" if desc else "asc", "gap" if rule[0] == abi.SS_GAP else "change"), T)
        finally:
            tab.free()


# 2. a limit inside a session that runs on over three seams ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FULL)
def test_limit_inside_a_swallowing_session(hip_engine, size):
    """k_ss_rows runs over the tiles below `limit` only, but reads tnext, scanned backwards over ALL tiles: with limit = 15 L + 5 the
    rows from 14 L - 5 on belong to a session whose last row, 17 L + 2, lies past the limit, in a tile no wave of the launch holds.
    SUM, LAST, AVG and COUNT are the whole session's."""
    ctx = hip_engine.ctx
    T = ctx.sessions_geometry()
    n = _rows_of(size, T)
    ntiles, per, _ = _geometry(n, T)
    L = per * T
    desc = size == FULL[1]
    terms = [(P, 0, desc, False), (P, 1, desc, False)]
    rule = (abi.SS_GAP, GAP)
    cols = [(OP["sum"],) + MQ, (OP["last"],) + MT, (OP["avg"],) + MX, COUNT]
    cut, ph, (p, t, x, q) = _columns_of(S_SEAMS, n, T, desc)
    tab = _ss_table(ctx, p, t, x, q)
    try:
        exp = Sessions(_stage_rows(ctx, tab, 0), terms, 1, rule)
        _claims(S_SEAMS, exp.heads, exp.part_heads, n, T)
        limit = 15 * L + 5
        j = int(np.searchsorted(exp.starts, limit - 1, side="right")) - 1   # the session of the last row below the limit
        start, last = int(exp.starts[j]), int(exp.starts[j + 1]) - 1
        assert (start, last) == (14 * L - 5, 17 * L + 2) and last > limit and last // L - start // L >= 3 and last // L - (limit - 1) // L == 2
        assert -(-limit // T) < ntiles and last // T >= -(-limit // T)       # mtiles < ntiles: the session ends in a tile the launch does not hold
        count = nref.columns(exp.heads, exp.part_heads, [("count", None, False)], False)[0]
        assert (count[start:limit] == last - start + 1).all()
        _check(ctx, tab, exp, terms, 1, rule, cols, (S_SEAMS, n, "limit 15 L + 5"), T, limit=limit, pers=(False,))
        _check(ctx, tab, exp, terms, 1, rule, cols, (S_SEAMS, n, "limit T - 1"), T, limit=T - 1, pers=(False,))
        half = len(exp.starts) // 2
        assert half > 100
        _check(ctx, tab, exp, terms, 1, rule, cols, (S_SEAMS, n, "half the sessions"), T, limit=half, pers=(True,))
        _check(ctx, tab, exp, terms, 1, rule, cols, (S_SEAMS, n, "one session of many"), T, limit=1, pers=(True,))
    finally:
        tab.free()
    cut, ph, (p, t, x, q) = _columns_of(ONE, n, T, desc)
    tab = _ss_table(ctx, p, t, x, q)
    try:
        exp = Sessions(_stage_rows(ctx, tab, 0), terms, 1, rule)
        assert len(exp.starts) == 1
        _check(ctx, tab, exp, terms, 1, rule, cols, (ONE, n, "limit L + 1"), T, limit=L + 1, pers=(False,))
    finally:
        tab.free()


# 3. a double gap term -------------------------------------------------------------------------------------------------------------------------
def test_double_gap_term(hip_engine):
    """The order column holds doubles — the integer pattern's values times 0.5 — with gap 1.5, descending, on "partition seams":
    1.5 or 0.5 continues, 2.0 cuts; a = v + 1.5 is exact."""
    ctx = hip_engine.ctx
    T = ctx.sessions_geometry()
    n = _rows_of(FULL[1], T)
    cut, ph, (p, t, x, q) = _columns_of(P_SEAMS, n, T, True)
    tab = _ss_table(ctx, p, t.astype(np.float64) * 0.5, x, q)
    terms = [(P, 0, True, False), (P, 1, True, True)]
    rule = (abi.SS_GAP, GAP * 0.5)
    try:
        exp = Sessions(_stage_rows(ctx, tab, 0), terms, 1, rule)
        assert (exp.heads == (cut | ph)).all() and (exp.part_heads == ph).all()
        _claims(P_SEAMS, exp.heads, exp.part_heads, n, T)
        _check(ctx, tab, exp, terms, 1, rule, [(OP["sum"],) + MQ, (OP["first"], P, 1, True), (OP["max"], P, 1, True), NUMBER], (P_SEAMS, n, "double gap term"), T)
    finally:
        tab.free()


# 4. a selection through min_hits ----------------------------------------------------------------------------------------------------------------
def test_min_hits_selects_past_256_tiles(hip_engine):
    """About 2.2 (W T + 1) entries with hits in 1 .. 3, min_hits = 2: the selection, not the table, is what passes 256 tiles.  The heads
    are found by the reference from the data (a double gap term: the aggregated value), not placed."""
    ctx = hip_engine.ctx
    T = ctx.sessions_geometry()
    entries = (W * T + 1) * 22 // 10
    rng = np.random.default_rng(entries)
    part, value, hits = _window_pattern("runs", entries, T, rng)
    tab = _table(ctx, part, value, hits)
    terms = [(P, 0, False, False), (V, 0, False, True)]
    rule = (abi.SS_GAP, 1.0)
    try:
        rows = _stage_rows(ctx, tab, 2)
        exp = Sessions(rows, terms, 1, rule)
        ntiles, per, _ = _geometry(exp.n, T)
        assert W * T < exp.n < entries and per >= 2 and ntiles > W and (rows[3] >= 2).all() and set(np.unique(hits)) == {1, 2, 3}
        length = np.diff(np.append(exp.starts, exp.n))
        assert len(exp.starts) > exp.part_heads.sum() > 1000 and length.max() > 8 and (length == 1).any()
        _check(ctx, tab, exp, terms, 1, rule, [COUNT, (OP["max"], H, 0, False), NUMBER, ROW], ("min_hits 2", exp.n), T, min_hits=2)
    finally:
        tab.free()


# 5. the other sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", LIGHT)
def test_one_call_per_size(hip_engine, size):
    ctx = hip_engine.ctx
    T = ctx.sessions_geometry()
    n = _rows_of(size, T)
    cut, ph, (p, t, x, q) = _columns_of(MIXED, n, T, False)
    tab = _ss_table(ctx, p, t, x, q)
    terms = [(P, 0, False, False), (P, 1, False, False)]
    rule = (abi.SS_GAP, GAP)
    try:
        exp = Sessions(_stage_rows(ctx, tab, 0), terms, 1, rule)
        assert (exp.heads == (cut | ph)).all() and (exp.part_heads == ph).all()
        _check(ctx, tab, exp, terms, 1, rule, [(OP["sum"],) + MQ, (OP["max"],) + MX, NUMBER, ROW], (MIXED, n), T, pers=(False,))
        _check(ctx, tab, exp, terms, 1, rule, [(OP["avg"],) + MQ, (OP["first"],) + MT, NUMBER, COUNT], (MIXED, n), T, pers=(True,))
    finally:
        tab.free()


# 6. general doubles ---------------------------------------------------------------------------------------------------------------------------
def _exact(xs):
    """(the exact sum, the exact sum of magnitudes) of doubles, as Fractions: integers over the largest denominator"""
    pairs = [float(v).as_integer_ratio() for v in xs]
    den = max(d for _, d in pairs)
    return Fraction(sum(a * (den // d) for a, d in pairs), den), Fraction(sum(abs(a) * (den // d) for a, d in pairs), den)


def _sample(starts, length, n, L):
    """at most forty sessions: the longest, those whose first or last row lies on or next to a seam between thread runs, some of one row"""
    last = starts + length - 1
    near = lambda at: (at > 1) & ((at % L <= 1) | (at % L == L - 1))        # noqa: E731
    seam = np.nonzero(near(starts) | near(last))[0]
    ones = np.nonzero(length == 1)[0]
    picked = list(np.argsort(length)[-4:]) + list(seam[::max(1, len(seam) // 24)][:24]) + list(ones[::max(1, len(ones) // 8)][:8])
    return sorted(set(int(i) for i in picked)), len(seam), len(ones)


def test_general_doubles_past_256_tiles(hip_engine):
    """262 657 rows of "mixed", the measure standard_normal * 10^U{-30 .. 29} as in test_sessions_gpu: SUM and AVG in both shapes against
    exact rational sums within the header's bound g(m) sum|v|, g(m) = (m - 1) u / (1 - (m - 1) u), u = 2^-53, on a sample of at most
    forty sessions — the longest (20 thread runs each: their sums reach their rows only through the carries), those that begin or end on or
    next to a seam, some of one row.  One-row sessions are equal by bits; every row of a session carries the same bits; an AVG is one
    IEEE division of the SUM beside it.
    PRINTED sessions, large: the worst error / bound — measured on the MI355X: 0.5819 (profiles/sessions_device.txt)."""
    ctx = hip_engine.ctx
    T = ctx.sessions_geometry()
    n = _rows_of(FULL[1], T)
    L = _geometry(n, T)[1] * T
    rng = np.random.default_rng(n)
    cut, ph = _large(MIXED, n, T)
    p, t, x, _ = _pattern_columns(cut, ph, False, rng)
    q = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
    tab = _ss_table(ctx, p, t, x, q)
    terms = [(P, 0, False, False), (P, 1, False, False)]
    rule = (abi.SS_GAP, GAP)
    cols = [(OP["sum"],) + MQ, (OP["avg"],) + MQ]
    worst = Fraction(0)
    try:
        exp = Sessions(_stage_rows(ctx, tab, 0), terms, 1, rule)
        assert (exp.heads == (cut | ph)).all()
        length = _claims(MIXED, exp.heads, exp.part_heads, n, T)
        qs = np.ascontiguousarray(_field(exp.rows, P, 3, True))[exp.idx]
        picked, nseam, nones = _sample(exp.starts, length, n, L)
        assert len(picked) <= 40 and nseam >= 10 and nones >= 8 and int(np.argmax(length)) in picked
        ones = length == 1
        for per in (False, True):
            order = exp.order(per)
            got = ctx.table_sessions(tab, 0, 1, terms, rule, cols, ALL, len(order), per_session=per, want_hits=False)
            _same(got, exp.rows, order, ("general doubles", per))
            s_col, a_col = got[4]
            assert s_col.dtype == a_col.dtype == np.float64 and len(s_col) == len(order)
            m_of = length if per else np.repeat(length, length)
            assert (nref.bits(a_col) == nref.bits(s_col / m_of.astype(np.float64))).all()      # one IEEE division of that sum
            at = np.arange(len(exp.starts)) if per else exp.starts
            assert (nref.bits(s_col[at[ones]]) == nref.bits(qs[exp.starts[ones]])).all()       # a session of one row: the row's bits
            if not per:
                first = np.repeat(nref.bits(s_col)[exp.starts], length)
                _first_bad(s_col, first.view(np.float64), None, n, T, "every row of a session: the same bits")
            for i in picked:
                a, m = int(exp.starts[i]), int(length[i])
                exact, mag = _exact(qs[a:a + m])
                g = (m - 1) * U / (1 - (m - 1) * U)
                s = float(s_col[i if per else a])
                err = abs(Fraction(s) - exact)
                assert err <= g * mag, ("general doubles", per, "session", i, "position", a, "rows", m, s, float(exact))
                if m > 1 and mag > 0:
                    worst = max(worst, err / (g * mag))
    finally:
        tab.free()
    print("PRINTED sessions, large, general doubles n=%d: worst observed error / bound = %.4f" % (n, float(worst)))
    assert worst > 0
