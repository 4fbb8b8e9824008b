"""Sessions (gaps and islands) on the MI355X (run with -m gpu): sdqh_table_sessions (include/sdqh_sort_sessions.h) by bits on data whose
every partial sum is exact — both output shapes, both rules, both directions, boundary patterns placed by sorted position —, on the
integer and double edges of the gap rule, within the header's bound against math.fsum / Fraction on general doubles, its contract,
one case past 256 tiles, and through the decorator against the host route.

The expected rows are the table's own rows (sdqh_table_compact) ordered and cut by sessions_reference: a Python loop with int and
Fraction that shares no code with the product.  PRINTED: the general-doubles test prints its worst error / bound ratio."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import sessions_reference as ref
from sdqlpy_amd import abi
from sdqlpy_amd import tpch_queries as Q
from test_window_gpu import _same, _stage_rows, _table, db, hip_engine, on_the_decorator      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
U = 2.0 ** -53
OP = {name: i for i, name in enumerate(ref.OPS)}
MX, MQ, MT = (P, 2, False), (P, 3, True), (P, 1, False)                   # the tables' integer measure, their double one, the order column as a measure


def _sizes(ctx):
    T, S = ctx.window_geometry(), ctx.sort_geometry()[0]
    assert ctx.sessions_geometry() == ctx.window_geometry() == T
    return T, S


def _ss_table(ctx, p, t, x, q, seed=5):
    """entries with payload 0 = p, payload 1 = t (an int64 array, or a float64 one: its bits), payload 2 = x, payload 3 = the bits of the
    doubles q, built in a shuffled order"""
    n = len(p)
    rng = np.random.default_rng(seed + n)
    keys = rng.permutation(n).astype(np.int64) * 3 - n
    sh = rng.permutation(n)
    t = np.ascontiguousarray(t)
    cols = [np.asarray(p, np.int64), t.view(np.int64) if t.dtype == np.float64 else t.astype(np.int64), np.asarray(x, np.int64), np.ascontiguousarray(q, np.float64).view(np.int64)]
    return ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(np.ascontiguousarray(c[sh])) for c in cols], accumulate=False)


def _field(rows, kind, index, is_f64=False):
    keys, payload, values, hits = rows
    src = keys if kind == K else payload[index] if kind == P else values[index] if kind == V else hits
    src = np.ascontiguousarray(src)
    return src.view(np.float64) if (is_f64 and src.dtype != np.float64) else src


def _term_values(rows, term):
    """a term's value before the descending reversal, as a list of Python numbers: the column, or the derived field"""
    kind, index, _, is_f64 = term[:4]
    v = _field(rows, kind, index, is_f64)
    if len(term) > 4:                                                    # field = (uint64(source) / div) % mod + add
        div, mod, add, _ = term[4:]
        out = []
        for u in np.ascontiguousarray(v).view(np.uint64):
            f = int(u) // div if div > 1 else int(u)
            out.append((f % mod if mod else f) + add)
        return out, False
    is_f = bool(is_f64) or kind == V
    return [u.item() for u in v], is_f


class Expected:
    """The sessions of a table's rows under terms / npart / rule, by sessions_reference: idx (the rows' order), heads, part_heads."""

    def __init__(self, rows, terms, npart, rule):
        self.rows = rows
        vals = [_term_values(rows, t) for t in terms]
        self.idx = ref.sort_index([v for v, _ in vals], ["desc" if t[2] else "asc" for t in terms], [f for _, f in vals])
        pk = [tuple(ref.total_key(v[i], f) for v, f in vals[:npart]) for i in self.idx]
        self.part_heads = [j == 0 or pk[j] != pk[j - 1] for j in range(len(pk))]
        if rule[0] == abi.SS_GAP:
            v, f = vals[npart]
            self.heads = ref.session_heads(pk, [v[i] for i in self.idx], bool(terms[npart][2]), rule[1], f)
        else:
            m = _field(rows, rule[1], rule[2])
            self.heads = ref.session_heads(pk, None, False, None, False, marker_bits=[ref.i_bits(m.view(np.int64)[i] if m.dtype != np.int64 else m[i]) for i in self.idx])
        self.starts = [j for j, h in enumerate(self.heads) if h]

    def columns(self, cols, per):
        spec = []
        for op, kind, index, is_f64 in cols:
            name = ref.OPS[op]
            if name in ("count", "number", "row"):
                spec.append((name, None, False))
            else:
                f = bool(is_f64) or kind == V
                m = _field(self.rows, kind, index, f)
                spec.append((name, [m[i].item() for i in self.idx], f))
        return ref.columns(self.heads, self.part_heads, spec, per)[0]

    def order(self, per):
        return np.array([self.idx[s] for s in self.starts] if per else self.idx, np.int64)


def _compare(ctx, t, terms, npart, rule, cols, what, min_hits=0, exp=None, limit=ALL, pers=(False, True)):
    """both shapes of one call against the reference, rows and columns by bits; returns the Expected"""
    exp = exp or Expected(_stage_rows(ctx, t, min_hits), terms, npart, rule)
    for per in pers:
        asked = [c for c in cols if not (per and c[0] == abi.SS_ROW)]
        got = ctx.table_sessions(t, min_hits, npart, terms, rule, asked, limit, 64, per_session=per, want_hits=t.accumulate)
        order = exp.order(per)[:limit]
        _same(got, exp.rows, order, (what, per))
        want = exp.columns(asked, per)
        assert len(got[4]) == len(asked)
        for c, (a, w) in enumerate(zip(got[4], want)):
            bits = [int(u) for u in np.ascontiguousarray(a).view(np.uint64)]
            assert bits == w[:limit], (what, "per session" if per else "per row", ref.OPS[asked[c][0]], [j for j in range(len(bits)) if bits[j] != w[j]][:5])
        assert ctx.table_sessions_count(t, min_hits, npart, terms, rule, per_session=per, limit=limit) == len(order)
    return exp


# 1. exact by bits -------------------------------------------------------------------------------------------------------------------------
PATTERNS = ["one session", "every row its own session", "edges", "a session over three tiles", "partitions and gaps"]
GAP = 3


def _pattern(name, n, T):
    """(cut, ph) by sorted position: where the rule cuts, where a partition starts"""
    pos = np.arange(n)
    cut, ph = np.zeros(n, bool), np.zeros(n, bool)
    ph[0] = True
    if name == "every row its own session":
        cut[:] = True
    elif name == "edges":
        for s in (63, 64, 65, T - 1, T, T + 1):
            if s < n:
                cut[s] = True
    elif name == "a session over three tiles":
        cut[pos % 4 == 0] = True
        cut[T - 9:min(n, 3 * T + 6)] = False
    elif name == "partitions and gaps":
        ph[pos % 37 == 0] = True                                           # a partition head where the gap alone would not cut ...
        cut[pos % 11 == 5] = True                                          # ... a gap cut that is no partition head, and (at 16 * 37 + ... ) both at once
        cut[pos % 407 == 0] = True
    return cut, ph


def _pattern_columns(cut, ph, desc, rng):
    """p, t, marker-bearing x and q by sorted position: t moves on by GAP + 1 at a cut (one more than continues) and by GAP or 1 elsewhere
    (exactly the gap continues) — at a partition head that is no cut too —; the marker x // 1000 changes exactly at the cuts"""
    n = len(cut)
    step = np.where(cut, GAP + 1, np.where(np.arange(n) % 2 == 0, GAP, 1))
    t = np.cumsum(step) - step[0]
    p = np.cumsum(ph) - 1
    marker = np.cumsum(cut) % 5
    x = marker * 1000 + rng.integers(0, 100, n)
    q = rng.integers(-40, 40, n) * 0.25                                     # multiples of 0.25 of small magnitude: every partial sum is exact
    sign = -1 if desc else 1
    return sign * p, sign * t, x, q


@pytest.mark.parametrize("pattern", PATTERNS)
def test_exact_by_bits(hip_engine, pattern):
    ctx = hip_engine.ctx
    T, S = _sizes(ctx)
    rng = np.random.default_rng(3)
    sets = ([(OP["sum"],) + MX, (OP["avg"],) + MQ, (OP["number"], K, 0, False), (OP["row"], K, 0, False)],
            [(OP["min"],) + MQ, (OP["max"],) + MX, (OP["first"],) + MT, (OP["last"],) + MT],
            [(OP["sum"],) + MQ, (OP["count"], K, 0, False), (OP["avg"],) + MX, (OP["last"],) + MQ])
    for n in (1, 2, 64, 66, T, T + 2, 2 * T + 2, S + 2, 3 * T + 5):
        cut, ph = _pattern(pattern, n, T)
        for desc in (False, True):
            p, t, x, q = _pattern_columns(cut, ph, desc, rng)
            tab = _ss_table(ctx, p, t, x, q)
            terms = [(P, 0, desc, False), (P, 1, desc, False)]
            try:
                exp = Expected(_stage_rows(ctx, tab, 0), terms, 1, (abi.SS_GAP, GAP))
                assert exp.heads == list(cut | ph), (pattern, n, desc)      # the pattern lies where it was placed
                for cols in sets:
                    _compare(ctx, tab, terms, 1, (abi.SS_GAP, GAP), cols, (pattern, n, desc, "gap"), exp=exp)
            finally:
                tab.free()
            # the change rule over the same positions: the marker x // 1000 in payload 2
            mtab = _ss_table(ctx, p, t, x // 1000, q)
            try:
                rule = (abi.SS_CHANGE, P, 2, False)
                exp = Expected(_stage_rows(ctx, mtab, 0), terms, 1, rule)
                assert exp.heads == list(cut | ph), (pattern, n, desc, "change")
                for cols in sets[1:]:
                    _compare(ctx, mtab, terms, 1, rule, cols, (pattern, n, desc, "change"), exp=exp)
            finally:
                mtab.free()


# 2. integer edges -------------------------------------------------------------------------------------------------------------------------
def test_int64_extremes_adjacent(hip_engine):
    ctx = hip_engine.ctx
    t = np.array([I_MAX, -1, I_MIN, 0, I_MAX, I_MIN, I_MAX, I_MIN], np.int64)
    p = np.array([0, 0, 0, 0, 0, 0, 1, 1])                                  # partition 1: INT64_MIN next to INT64_MAX, a difference of 2^64 - 1
    tab = _ss_table(ctx, p, t, np.array([I_MAX, I_MAX, 1, I_MIN, -1, 7, 3, 4], np.int64), np.arange(8) * 0.5)
    cols = [(OP["sum"],) + MX, (OP["first"],) + MT, (OP["last"],) + MT, (OP["number"], K, 0, False)]
    try:
        for desc in (False, True):
            terms = [(P, 0, False, False), (P, 1, desc, False)]
            for gap, sessions in ((0, 6), (1, 5), (I_MAX - 1, 5), (I_MAX, 3)):
                exp = _compare(ctx, tab, terms, 1, (abi.SS_GAP, gap), cols, ("extremes", desc, gap))
                assert sum(exp.heads) == sessions, (desc, gap)              # partition 1 is two sessions under every gap
    finally:
        tab.free()


def test_a_hits_gap_term_and_a_derived_one(hip_engine):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    n = T + 70
    rng = np.random.default_rng(8)
    PACK = 1 << 20
    a, b = np.arange(n) // 90, np.cumsum(rng.choice([0, 1, 2, 5], n))      # the packed halves: b the gap term's field
    tab = _table(ctx, a * PACK + (b % PACK), rng.integers(0, 1000, n), 1 + np.cumsum(rng.choice([0, 1, 3], n)) % 40)
    cols = [(OP["sum"], V, 0, True), (OP["count"], K, 0, False), (OP["max"], H, 0, False), (OP["number"], K, 0, False)]
    try:
        for desc in (False, True):
            _compare(ctx, tab, [(P, 0, False, False, PACK, 0, 0, None), (H, 0, desc, False), (K, 0, False, False)], 1, (abi.SS_GAP, 1), cols, ("hits", desc), min_hits=1)
            for gap in (0, 1, 4):
                _compare(ctx, tab, [(P, 0, False, False, PACK, 0, 0, None), (P, 0, desc, False, 1, PACK, 0, None)], 1, (abi.SS_GAP, gap), cols, ("derived", desc, gap), min_hits=1)
    finally:
        tab.free()


# 3. a double gap term ---------------------------------------------------------------------------------------------------------------------
def test_a_double_gap_term_takes_one_addition(hip_engine):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    nan1, nan2 = np.array([0x7FF8000000000001, 0xFFF8000000000002], np.uint64).view(np.float64)
    v = np.array([0.1 * i for i in range(T + 40)])                          # (0.0 among them) neighbours a rounding apart: 0.1 * i - 0.1 against 0.1 * (i - 1)
    t = np.concatenate([v, [-0.0, 0.0, -0.0, nan1, nan1, nan2, nan2, nan1, -np.inf, np.inf, 1e308, -1e308, 5e-324, -5e-324]])
    n = len(t)
    rng = np.random.default_rng(2)
    tab = _ss_table(ctx, np.zeros(n, np.int64), t, rng.integers(-9, 9, n), rng.integers(-9, 9, n) * 0.5)
    cols = [(OP["count"], K, 0, False), (OP["first"], P, 1, True), (OP["last"], P, 1, True), (OP["sum"],) + MQ]
    try:
        for desc in (False, True):
            terms = [(P, 1, desc, True), (K, 0, False, False)]
            for gap in (0.1, 0.0, 0.09999999999999999, 0.5, 1e308):
                exp = _compare(ctx, tab, terms, 0, (abi.SS_GAP, gap), cols, ("doubles", desc, gap))
                s = np.array([t_ for t_ in _field(exp.rows, P, 1, True)[exp.idx]])
                with np.errstate(invalid="ignore", over="ignore"):
                    a = s[1:] + np.float64(gap if desc else -gap)           # the same single numpy addition
                    inside = (np.minimum(a, s[1:]) <= s[:-1]) & (s[:-1] <= np.maximum(a, s[1:]))
                same = s[1:].view(np.uint64) == s[:-1].view(np.uint64)
                assert exp.heads[1:] == list(~np.where(np.isnan(s[1:]), same, inside & ~np.isnan(s[:-1]))), (desc, gap)
                if gap == 0.0:
                    zeros = [j for j in range(n) if s[j] == 0.0]
                    assert len(zeros) == 4 and exp.heads[zeros[0]] and not any(exp.heads[j] for j in zeros[1:])      # -0.0 and +0.0 are one value
                    nans = [j for j in range(n) if s[j] != s[j]]
                    assert len(nans) == 5 and sum(exp.heads[j] for j in nans) == 2      # two payloads, two sessions
        exp = Expected(_stage_rows(ctx, tab, 0), [(P, 1, False, True), (K, 0, False, False)], 0, (abi.SS_GAP, 0.1))
        assert 10 < sum(exp.heads[:T + 40]) < T                             # multiples of 0.1: some neighbours continue, some do not
    finally:
        tab.free()


# 4. general doubles -----------------------------------------------------------------------------------------------------------------------
def test_general_doubles_within_the_bound(hip_engine):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    worst = 0.0
    for n, run in ((T + 1, 3), (4 * T + 1, 300), (2 * T + 7, 2 * T + 7)):
        rng = np.random.default_rng(n)
        q = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
        tpos = np.cumsum(np.where(np.arange(n) % run == 0, 5, 1))
        tab = _ss_table(ctx, np.zeros(n, np.int64), tpos, rng.integers(-9, 9, n), q)
        terms = [(P, 1, False, False)]
        try:
            exp = Expected(_stage_rows(ctx, tab, 0), terms, 0, (abi.SS_GAP, 1))
            qs = _field(exp.rows, P, 3, True)[exp.idx]
            stops = exp.starts[1:] + [n]
            for per in (False, True):
                got = ctx.table_sessions(tab, 0, 0, terms, (abi.SS_GAP, 1), [(OP["sum"],) + MQ, (OP["avg"],) + MQ], ALL, 64, per_session=per, want_hits=False)
                assert [a.dtype for a in got[4]] == [np.float64, np.float64]
                for i, (a, b) in enumerate(zip(exp.starts, stops)):
                    m = b - a
                    exact = sum((Fraction(float(x)) for x in qs[a:b]), Fraction(0))
                    mag = math.fsum(abs(float(x)) for x in qs[a:b])
                    g = (m - 1) * U / (1 - (m - 1) * U)
                    for j in ([i] if per else [a, b - 1]):
                        s, avg = float(got[4][0][j]), float(got[4][1][j])
                        err = abs(Fraction(s) - exact)
                        assert err <= Fraction(g) * Fraction(mag), (n, per, i, s, float(exact))
                        if mag > 0 and g > 0:
                            worst = max(worst, float(err / (Fraction(g) * Fraction(mag))))
                        assert abs(Fraction(avg) - exact / m) <= (Fraction(g) * Fraction(mag) * (1 + Fraction(U)) + Fraction(U) * abs(exact)) / m, (n, per, i)
                        assert avg == s / float(m)                          # one IEEE division of that sum
                    if not per:
                        assert len(set(ref.f_bits(x) for x in got[4][0][a:b])) == 1      # every row of a session: the same bits
        finally:
            tab.free()
    print("sessions, general doubles: worst observed error / bound = %.4f" % worst)
    assert worst > 0.0


# 5. the change rule, the tie-breaking term -----------------------------------------------------------------------------------------------
def test_the_change_rule_over_an_integer_and_a_double_marker(hip_engine):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    n = 2 * T + 9
    rng = np.random.default_rng(4)
    q = np.where(rng.integers(0, 4, n) == 0, -0.0, rng.integers(0, 2, n) * 1.0)      # -0.0 and +0.0 differ as stored bits
    tab = _ss_table(ctx, np.arange(n) // 200, np.arange(n), rng.integers(0, 3, n), q)
    ptab = _table(ctx, rng.integers(0, 3, n), np.repeat(rng.integers(0, 4, n // 3 + 1), 3)[:n], rng.integers(1, 4, n))
    cols = [(OP["count"], K, 0, False), (OP["number"], K, 0, False), (OP["first"],) + MT, (OP["last"],) + MT]
    try:
        for desc in (False, True):
            terms = [(P, 0, False, False), (P, 1, desc, False)]
            _compare(ctx, tab, terms, 1, (abi.SS_CHANGE, P, 2, False), cols, ("integer marker", desc))
            _compare(ctx, tab, terms, 1, (abi.SS_CHANGE, P, 3, True), cols, ("double marker", desc))
            _compare(ctx, tab, terms[:1], 1, (abi.SS_CHANGE, P, 2, False), cols[:2], ("no order term", desc))
            _compare(ctx, ptab, [(P, 0, desc, False), (K, 0, False, False)], 1, (abi.SS_CHANGE, V, 0, True), [(OP["sum"], V, 0, True), (OP["max"], H, 0, False)], ("value marker", desc), min_hits=1)
    finally:
        tab.free()
        ptab.free()


def test_a_tie_breaking_term_orders_inside_equal_gap_values(hip_engine):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    n = T + 33
    rng = np.random.default_rng(6)
    t = rng.integers(0, n // 6, n) * 2                                      # many ties, and differences of 0, 2, 4 ...
    tab = _ss_table(ctx, rng.integers(0, 3, n), t, rng.permutation(n), rng.integers(-9, 9, n) * 0.25)
    cols = [(OP["first"],) + MX, (OP["last"],) + MX, (OP["sum"],) + MQ, (OP["row"], K, 0, False)]
    try:
        for desc in (False, True):
            for tie_desc in (False, True):                                  # payload 2 is a permutation: the order is total, whatever the stored order
                terms = [(P, 0, False, False), (P, 1, desc, False), (P, 2, tie_desc, False)]
                _compare(ctx, tab, terms, 1, (abi.SS_GAP, 2), cols, ("tie term", desc, tie_desc))
            _compare(ctx, tab, [(P, 0, False, False), (P, 1, desc, False)], 1, (abi.SS_GAP, 2), cols, ("stable", desc))      # ties keep the stored order, as the host route's
    finally:
        tab.free()


# 6. the contract ----------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, t, terms, npart, rule, cols, limit, capacity, keys=None, out=None, per=0, min_hits=0, nterms=None, ncols=None, null_cols=False, null_rule=False, no_n=False):
    got = C.c_int64(-7)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    r = abi._marshal_session_rule(rule)
    rc = ctx.lib.sdqh_table_sessions(ctx.handle, t.handle, C.c_int64(min_hits), C.c_int(npart), C.c_int(len(terms) if nterms is None else nterms), abi._marshal_sort_terms(terms),
                                     None if null_rule else C.byref(r), C.c_int(per), C.c_int(len(cols) if ncols is None else ncols), None if null_cols else abi._marshal_session_cols(cols),
                                     C.c_int64(limit), C.c_int64(capacity), ptr(keys), None, None, None, ptr(out), None if no_n else C.byref(got))
    return rc, got.value


def test_sizes_errors_and_empties(hip_engine, hip_lib):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    n = T + 9
    pos = np.arange(n, dtype=np.int64)
    tab = _ss_table(ctx, pos // 100, pos * 2 + (pos % 10 == 0) * 5, pos % 7, (pos % 5) * 0.5)
    empty = _ss_table(ctx, pos[:0], pos[:0], pos[:0], pos[:0].astype(np.float64))
    terms, gap = [(P, 0, False, False), (P, 1, False, False)], (abi.SS_GAP, 2)
    cols = [(OP["sum"],) + MX, (OP["avg"],) + MQ]
    try:
        exp = Expected(_stage_rows(ctx, tab, 0), terms, 1, gap)
        ns = len(exp.starts)
        assert 50 < ns < n
        for per, total in ((0, n), (1, ns)):
            keys, out = np.full(total, -7, np.int64), np.full((2, total), -7, np.int64)
            assert _raw(ctx, tab, terms, 1, gap, cols, ALL, total - 1, keys, out, per=per) == (abi.ERR_OVERFLOW, total)      # the count needed, nothing written
            assert (keys == -7).all() and (out == -7).all()
            assert _raw(ctx, tab, terms, 1, gap, cols, 5, total, keys, out, per=per) == (abi.OK, 5) and (keys[5:] == -7).all() and (out[:, 5:] == -7).all() and (out[:, :5] != -7).all()
            assert _raw(ctx, tab, terms, 1, gap, cols, ALL, 0, per=per) == (abi.OK, total)                                    # count only: every out array NULL
            assert _raw(ctx, tab, terms, 1, gap, [], ALL, 0, per=per, null_cols=True) == (abi.OK, total)
            keys[:], out[:] = -7, -7
            assert _raw(ctx, tab, terms, 1, gap, cols, ALL, total, keys, None, per=per) == (abi.OK, total)                    # rows only
            assert (keys == exp.rows[0][exp.order(per)]).all()
            first = keys.copy()
            keys[:] = -7
            assert _raw(ctx, tab, terms, 1, gap, [], ALL, total, keys, out, per=per) == (abi.OK, total) and (keys == first).all() and (out == -7).all()      # no column
            assert _raw(ctx, tab, terms, 1, gap, cols, ALL, total, None, out, per=per) == (abi.OK, total) and (out != -7).all()                              # columns only
            again = np.full((2, total), -7, np.int64)
            assert _raw(ctx, tab, terms, 1, gap, cols, ALL, total, None, again, per=per) == (abi.OK, total) and (again == out).all()                        # two calls: identical bits
            assert _raw(ctx, empty, terms, 1, gap, cols, ALL, 4, keys, out, per=per) == (abi.OK, 0)
        # a session straddling the limit: its columns still cover the whole session
        a, b = next((a, b) for a, b in zip(exp.starts, exp.starts[1:]) if b - a >= 4)
        _compare(ctx, tab, terms, 1, gap, cols + [(OP["count"], K, 0, False), (OP["last"],) + MT], "straddling the limit", exp=exp, limit=a + 2, pers=(False,))
        _compare(ctx, tab, terms, 1, gap, cols, "the first sessions", exp=exp, limit=3, pers=(True,))
        keys, out = np.full(n, -7, np.int64), np.full((4, n), -7, np.int64)
        x9, k_f, h_f = (P, 9, False), (K, 0, True), (H, 0, True)
        bads = [dict(rule=(2, 0)), dict(rule=(-1, 0)), dict(null_rule=True), dict(per=2), dict(per=-1),
                dict(cols=[(-1,) + MX]), dict(cols=[(9,) + MX]), dict(ncols=-1), dict(ncols=5), dict(null_cols=True), dict(cols=[(OP["row"], K, 0, False)], per=1),
                dict(rule=(abi.SS_GAP, -1)), dict(npart=2), dict(nterms=0), dict(nterms=9), dict(limit=0), dict(capacity=-1),
                dict(cols=[(OP["sum"],) + x9]), dict(cols=[(OP["min"],) + k_f]), dict(cols=[(OP["first"],) + h_f]), dict(cols=[(OP["max"], H, 0, False)]),      # (a table without hits)
                dict(rule=(abi.SS_CHANGE, P, 9, False)), dict(rule=(abi.SS_CHANGE, K, 0, True)), dict(terms=[(P, 0, False, False), (P, 9, False, False)])]
        for bad in bads:
            args = dict(terms=terms, npart=1, rule=gap, cols=cols, limit=ALL, capacity=n, per=0, nterms=None, ncols=None, null_cols=False, null_rule=False)
            args.update(bad)
            keys[:], out[:] = -7, -7
            rc = _raw(ctx, tab, args["terms"], args["npart"], args["rule"], args["cols"], args["limit"], args["capacity"], keys, out, per=args["per"], nterms=args["nterms"],
                      ncols=args["ncols"], null_cols=args["null_cols"], null_rule=args["null_rule"])
            assert rc == (abi.ERR_INVALID, -7), (bad, rc)
            assert (keys == -7).all() and (out == -7).all(), bad
        assert _raw(ctx, tab, terms, 1, gap, cols, ALL, n, keys, out, no_n=True)[0] == abi.ERR_INVALID and (keys == -7).all()
        for bad_t in ([(P, 1, False, True)], [(P, 3, False, True)]):       # a double gap term: a negative and a non-finite gap
            for g in (-0.5, float("inf"), float("nan")):
                assert _raw(ctx, tab, bad_t, 0, (abi.SS_GAP, g), cols, ALL, n, keys, out) == (abi.ERR_INVALID, -7)
        # the order of the checks: on a compile-only context the struct checks answer first, SDQH_ERR_UNSUPPORTED next, the table's never
        cctx = hip_lib.context(device=-1)
        try:
            prog = abi.Program()
            prog.key = prog.op(abi.X_COL, abi.T_I64, col=cctx.wrap(0x10000, 64, abi.I64))
            ctab = cctx.xbuild(64, prog, 0, 100, accumulate=True)
            one = [(K, 0, False, False)]
            assert _raw(cctx, ctab, one, 0, (abi.SS_GAP, -1), cols, ALL, n, keys, out) == (abi.ERR_INVALID, -7)
            assert _raw(cctx, ctab, one, 0, gap, [(9,) + MX], ALL, n, keys, out) == (abi.ERR_INVALID, -7)
            assert _raw(cctx, ctab, one, 0, gap, [(OP["sum"],) + x9], ALL, n, keys, out) == (abi.ERR_UNSUPPORTED, -7)
            assert _raw(cctx, ctab, one, 0, gap, cols, ALL, n, keys, out) == (abi.ERR_UNSUPPORTED, -7) and (keys == -7).all() and (out == -7).all()
        finally:
            cctx.close()
        _compare(ctx, tab, terms, 1, gap, cols, "usable after the errors", exp=exp)
    finally:
        tab.free()
        empty.free()


def test_min_hits_selects_before_the_sessions_are_cut(hip_engine):
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    n = T + 50
    rng = np.random.default_rng(12)
    tab = _table(ctx, np.arange(n) // 2, rng.integers(0, 50, n), rng.integers(0, 4, n), dups=20)      # payload 0 = the gap term: a row left out widens a gap
    cols = [(OP["count"], K, 0, False), (OP["sum"], V, 0, True), (OP["first"], P, 0, False), (OP["last"], P, 0, False)]
    try:
        counts = set()
        for min_hits in (0, 1, 2, 3):
            exp = _compare(ctx, tab, [(P, 0, False, False), (K, 0, False, False)], 0, (abi.SS_GAP, 1), cols, ("min_hits", min_hits), min_hits=min_hits)
            counts.add((len(exp.idx), len(exp.starts)))
        assert len(counts) == 4
    finally:
        tab.free()


# 7. past 256 tiles ------------------------------------------------------------------------------------------------------------------------
def test_past_256_tiles(hip_engine):
    """n = 257 T + 3: the one-workgroup scans (k_win_scan, k_wagg_scan, k_wagg_next, k_sort_bins) fold several tiles per thread, with sessions
    of mixed lengths — single rows, a few rows, several tiles, most of the input."""
    ctx = hip_engine.ctx
    T, _ = _sizes(ctx)
    n = 257 * T + 3
    pos = np.arange(n)
    rng = np.random.default_rng(257)
    cut = np.zeros(n, bool)
    cut[pos % 3 == 0] = True
    cut[5 * T + 7:9 * T + 1] = False                                        # a session over four tiles
    cut[20 * T:150 * T + 5] = False                                         # ... and one over 130
    cut[200 * T + 3:200 * T + 3 + 3 * T:5] = True
    ph = pos % (40 * T + 11) == 0
    p, t, x, q = _pattern_columns(cut, ph, False, rng)
    tab = _ss_table(ctx, p, t, x % 1000 - 50, q)
    terms = [(P, 0, False, False), (P, 1, False, False)]
    try:
        exp = Expected(_stage_rows(ctx, tab, 0), terms, 1, (abi.SS_GAP, GAP))
        assert exp.heads == list(cut | ph)
        _compare(ctx, tab, terms, 1, (abi.SS_GAP, GAP), [(OP["sum"],) + MQ, (OP["max"],) + MX, (OP["number"], K, 0, False), (OP["row"], K, 0, False)], "257 tiles", exp=exp)
    finally:
        tab.free()


# 8. through the engine and the decorator ---------------------------------------------------------------------------------------------------
def test_q3_on_the_decorator(on_the_decorator, db, monkeypatch):
    eng = on_the_decorator
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_shippriority"], [("o_orderdate", "asc")]
    cols = {"from": ("first", "o_orderdate"), "to": ("last", "o_orderdate"), "orders": ("count",), "revenue_sum": ("sum", "revenue")}
    more = {"k": ("number",), "r": ("row",), "avg_rev": ("avg", "revenue"), "best": ("max", "revenue")}

    def both(run, per):
        dev = run()
        note = eng.stats()["order_routes"][-1]
        assert note["route"] == "sessions" and note["calls"] == 1 and note["per_session"] is per and note["rule"] == "gap" and note["gap"] == 1, note
        monkeypatch.setattr(eng, "device_sessions", False)
        host = run()
        assert eng.stats()["order_routes"][-1]["route"] == "host" and eng.stats()["order_routes"][-1]["calls"] == 0
        monkeypatch.setattr(eng, "device_sessions", True)
        assert dev.columns == host.columns and len(dev) == len(host) > 3
        assert [np.asarray(a).dtype for a in dev.arrays] == [np.asarray(a).dtype for a in host.arrays]
        return dev, host

    rows = Q.q3.order_by([("o_shippriority", "asc"), ("o_orderdate", "asc")])(*args)
    dates, prio = np.asarray(rows.column("o_orderdate")), np.asarray(rows.column("o_shippriority"))
    head = np.ones(len(rows), bool)
    head[1:] = (prio[1:] != prio[:-1]) | (dates[1:] - dates[:-1] > 1)
    size = np.diff(np.append(np.nonzero(head)[0], len(rows)))             # every session's row count, by numpy over the order_by rows
    for wanted, per in ((cols, None), (cols, "session"), (more, None), ({k: v for k, v in more.items() if k != "r"}, "session")):
        dev, host = both(lambda: Q.q3.sessions(by, order, gap=1, cols=wanted, per=per)(*args), per == "session")
        assert dev.columns == rows.columns + list(wanted)
        assert len(dev) == (len(rows) if per is None else len(size))
        m = (size if per == "session" else size[np.cumsum(head) - 1]).astype(np.float64)
        for c in dev.columns:
            d, h = np.asarray(dev.column(c)), np.asarray(host.column(c))
            if c in ("revenue_sum", "avg_rev"):                            # revenues are positive: sum|v| is the sum itself; both sides lie within g(m) of it
                assert d.dtype == np.float64 and (np.abs(d - h) <= (2 * (m - 1) * U / (1 - (m - 1) * U) + 2 * U) * np.abs(h)).all(), c
            elif d.dtype.kind == "f":
                assert (d.view(np.int64) == h.view(np.int64)).all(), c
            else:
                assert (d.astype(str) == h.astype(str)).all(), c
    # more than four columns: on the host
    wide = Q.q3.sessions(by, order, gap=1, cols=dict(cols, **{"k": ("number",)}))(*args)
    assert eng.stats()["order_routes"][-1]["route"] == "host" and wide.columns == rows.columns + list(cols) + ["k"]
