"""The test's own half of the sessions tests past 256 tiles (test_sessions_large_gpu), without a GPU.  There is no CPU implementation of
sdqh_table_sessions, so what can be checked here is the reference and the patterns:

    reference against reference   sessions_numpy_reference (whole-array numpy) equals sessions_reference (a Python loop with int and
        Fraction) by bits on random inputs of 1 .. 200 rows and on every pattern of test_sessions_gpu at its sizes up to 3 T + 5: both
        rules, both directions, the integer and the double gap term, all nine ops, both shapes, -0.0 measures, int64 sums that wrap,
        sessions of one row; and its order equals sessions_reference.sort_index on rows with ties;
    pattern claims   each pattern of test_sessions_large_gpu is built at both full sizes as the rows _stage_rows would return, in a
        shuffled order, found again by the reference, and its structural claims are asserted (the GPU test asserts the same claims,
        through the same checker, on the device's rows);
    time   the reference's calls at 262 657 rows are timed and printed (pytest -s); the figures stand in the GPU file's docstring."""
import time

import numpy as np
import pytest

import large_patterns as LP
import sessions_numpy_reference as nref
import sessions_reference as ref
from sdqlpy_amd import abi
from test_sessions_gpu import GAP, PATTERNS as SMALL_PATTERNS, _pattern, _pattern_columns
from test_sessions_large_gpu import EACH, MIXED, ONE, P_SEAMS, PATTERNS, S_SEAMS, SETS, Sessions, _claims, _columns_of, _sample
from test_window_large_gpu import FULL, W, _geometry, _rows_of, _thread_runs

T = 512
N = 2 * W * T + T + 1
P = abi.SORT_PAYLOAD
I_MAX = (1 << 63) - 1


def _words(col):
    return [int(u) for u in col]


def _both(part, values, desc, gap, is_f64, marker, measures, what):
    """heads and all nine ops over each measure, both shapes: the two references agree by bits.  Everything by sorted position."""
    pk = [tuple(int(c[j]) for c in part) for j in range(len(part[0]))]
    if marker is None:
        want_heads = ref.session_heads(pk, [v.item() for v in values], desc, gap, is_f64)
        sh, ph = nref.heads(part, values, desc, gap, is_f64)
    else:
        want_heads = ref.session_heads(pk, None, False, None, False, marker_bits=_words(nref.bits(marker)))
        sh, ph = nref.heads(part, None, False, None, False, marker_bits=nref.bits(marker))
    want_part = [j == 0 or pk[j] != pk[j - 1] for j in range(len(pk))]
    assert list(sh) == want_heads and list(ph) == want_part, what
    for per in (False, True):
        for xs, f in measures:
            names = [op for op in nref.OPS if not (per and op == "row")]
            got = nref.columns(sh, ph, [(op, xs, f) for op in names], per)
            want, starts = ref.columns(want_heads, want_part, [(op, [x.item() for x in xs], f) for op in names], per)
            assert starts == list(np.nonzero(sh)[0])
            for op, g, w in zip(names, got, want):
                assert g.dtype == np.uint64 and _words(g) == w, (what, per, op, f)
    return sh, ph


def _random_case(rng):
    n = int(rng.integers(1, 201))
    nparts = int(rng.integers(1, 5))
    part = [np.sort(rng.integers(0, nparts, n)).astype(np.int64), np.zeros(n, np.int64)]
    desc = bool(rng.integers(0, 2))
    kind = ("int", "double", "change int", "change double")[int(rng.integers(0, 4))]
    step = rng.choice(np.array([0, 0, 1, 2, 3, 7]), n)
    climb = np.cumsum(step) * (-1 if desc else 1)                           # along the order inside a partition, and across them: the partition heads cut anyway
    ints = rng.integers(-(1 << 62), 1 << 62, n)
    ints[rng.integers(0, n, n // 3)] = rng.integers(-9, 9, n // 3)
    if rng.integers(0, 4) == 0:
        ints[:] = I_MAX - rng.integers(0, 3, n)                             # every sum of two rows wraps
    dbls = rng.integers(-40, 40, n) * 0.25
    dbls[rng.integers(0, n, n // 4)] = -0.0
    if rng.integers(0, 4) == 0:
        dbls[:] = np.where(rng.integers(0, 2, n) == 0, -0.0, 0.0)           # sessions of -0.0 alone, and of both zeros
    measures = [(ints, False), (dbls, True)]
    if kind == "int":
        return part, climb.astype(np.int64), desc, int(rng.integers(0, 4)), False, None, measures
    if kind == "double":
        return part, climb * 0.1, desc, float(rng.choice(np.array([0.0, 0.1, 0.2, 0.30000000000000004, 0.5]))), True, None, measures
    marker = rng.integers(0, 3, n).astype(np.int64) if kind == "change int" else np.where(rng.integers(0, 3, n) == 0, -0.0, rng.integers(0, 2, n) * 1.0)
    return part, None, False, None, False, marker, measures


def test_reference_against_reference_on_random_inputs():
    rng = np.random.default_rng(20)
    seen, single, wrapped = set(), 0, 0
    for i in range(320):
        part, values, desc, gap, is_f64, marker, measures = _random_case(rng)
        sh, _ = _both(part[:1 + i % 2], values, desc, gap, is_f64, marker, measures, i)
        seen.add((marker is None, desc, is_f64))
        length = np.diff(np.append(np.nonzero(sh)[0], len(sh)))
        single += int((length == 1).sum())
        with np.errstate(over="ignore"):
            sums = np.add.reduceat(measures[0][0], np.nonzero(sh)[0])
        exact = [sum(int(x) for x in measures[0][0][a:a + m]) for a, m in zip(np.nonzero(sh)[0], length)]
        wrapped += sum(1 for s, e in zip(sums, exact) if int(s) != e)
    assert len(seen) >= 5 and single > 300 and wrapped > 100, (seen, single, wrapped)


@pytest.mark.parametrize("pattern", SMALL_PATTERNS)
def test_reference_against_reference_on_the_small_patterns(pattern):
    """test_sessions_gpu's patterns at its sizes (its S + 2 is 2 T + 2 with the library's SORT_SMALL = 1024), both directions, both rules,
    and a double gap term: the integer one's values times 0.5 with gap 1.5"""
    rng = np.random.default_rng(3)
    for n in (1, 2, 64, 66, T, T + 2, 2 * T + 2, 3 * T + 5):
        assert n <= 3 * T + 5
        cut, ph = _pattern(pattern, n, T)
        for desc in (False, True):
            p, t, x, q = _pattern_columns(cut, ph, desc, rng)
            measures = [(x.astype(np.int64), False), (q, True)]
            for what, values, gap, f, marker in (("gap", t.astype(np.int64), GAP, False, None), ("double gap", t * 0.5, GAP * 0.5, True, None),
                                                 ("change", None, None, False, (x // 1000).astype(np.int64))):
                sh, got_ph = _both([np.asarray(p, np.int64)], values, desc, gap, f, marker, measures, (pattern, n, desc, what))
                assert (sh == (cut | ph)).all() and (got_ph == ph).all(), (pattern, n, desc, what)


def test_order_is_the_stable_order():
    rng = np.random.default_rng(5)
    for n in (1, 2, 77, 300):
        a, b = rng.integers(-3, 3, n), rng.choice(np.array([-1.5, -0.0, 0.0, 2.0, 1e300]), n)
        rows = LP.synthetic_rows([a, b])
        for da in (False, True):
            for db in (False, True):
                terms = [(P, 0, da, False), (P, 1, db, True)]
                want = ref.sort_index([[int(v) for v in a], [float(v) for v in b]], ["desc" if da else "asc", "desc" if db else "asc"], [False, True])
                assert list(nref.order(rows, terms)) == want, (n, da, db)


def _synthetic(pattern, n, desc, change=False):
    """the rows _stage_rows would return for the pattern's table, in a shuffled order, and the pattern"""
    cut, ph, (p, t, x, q) = _columns_of(pattern, n, T, desc)
    mix = np.random.default_rng(n).permutation(n)
    cols = [np.asarray(p, np.int64)[mix], np.asarray(t, np.int64)[mix], np.asarray(x // 1000 if change else x, np.int64)[mix], q[mix]]
    return LP.synthetic_rows(cols), cut, ph


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pattern_claims(pattern, size):
    n = _rows_of(size, T)
    ntiles, per, _ = _geometry(n, T)
    L = per * T
    assert (ntiles, per) == {FULL[0]: (257, 2), FULL[1]: (514, 3)}[size] and LP.ragged(n, T)
    desc = size == FULL[1]
    terms = [(P, 0, desc, False), (P, 1, desc, False)]
    for rule in ((abi.SS_GAP, GAP), (abi.SS_CHANGE, P, 2, False)):
        rows, cut, ph = _synthetic(pattern, n, desc, change=rule[0] == abi.SS_CHANGE)
        exp = Sessions(rows, terms, 1, rule)
        assert (exp.heads == (cut | ph)).all() and (exp.part_heads == ph).all(), (pattern, n, rule[0])      # found again where it was placed
        length = _claims(pattern, exp.heads, exp.part_heads, n, T)
    counts = LP.seam_counts(exp.heads, T)
    if pattern == ONE:
        assert counts[3] == n // L - 1                                      # no head behind the first thread run
    if pattern == EACH:
        assert len(exp.starts) == n > W * T and _geometry(len(exp.starts), T)[1] == per      # the sessions' slots pass 256 tiles too
    if pattern == S_SEAMS:
        assert LP.seam_rule(exp.heads, T, pattern) == counts and counts[3] == 3
        limit = 15 * L + 5                                                  # test_limit_inside_a_swallowing_session's
        assert 14 * L - 5 < limit < 17 * L + 2 and -(-limit // T) < ntiles and length[np.searchsorted(exp.starts, limit, side="right") - 1] == 3 * L + 8
    if pattern == P_SEAMS:
        assert LP.seam_rule(exp.part_heads, T, pattern) == LP.seam_counts(exp.part_heads, T)
        number = nref.columns(exp.heads, exp.part_heads, [("number", None, False)], False)[0].astype(np.int64)
        assert (number[exp.part_heads] == 1).all() and number[17 * L + 2] > number[15 * L] > 1 and _thread_runs(exp.heads, n, T).all()
    if pattern == MIXED:
        picked, nseam, nones = _sample(exp.starts, length, n, L)
        assert len(picked) <= 40 and nseam >= 10 and nones >= 8 and int(np.argmax(length)) in picked
    for cols in SETS:                                                       # the columns exist in both shapes
        for per_session in (False, True):
            asked = [c for c in cols if not (per_session and nref.OPS[c[0]] == "row")]
            assert all(len(a) == (len(exp.starts) if per_session else n) for a in exp.columns(asked, per_session))


def test_the_reference_is_quick_at_262657_rows():
    slowest = ("", 0.0)
    for pattern in (EACH, MIXED):
        rows, cut, ph = _synthetic(pattern, N, True)
        terms = [(P, 0, True, False), (P, 1, True, False)]
        t0 = time.perf_counter()
        idx = nref.order(rows, terms)
        t1 = time.perf_counter()
        exp = Sessions(rows, terms, 1, (abi.SS_GAP, GAP))
        t2 = time.perf_counter()
        took = {"order": t1 - t0, "Sessions (order and heads)": t2 - t1}
        assert len(idx) == N
        for cols in SETS:
            for per_session in (False, True):
                asked = [c for c in cols if not (per_session and nref.OPS[c[0]] == "row")]
                t3 = time.perf_counter()
                exp.columns(asked, per_session)
                took["%d columns of %s, %s" % (len(asked), [nref.OPS[c[0]] for c in asked], "per session" if per_session else "per row")] = time.perf_counter() - t3
        worst = max(took, key=took.get)
        print("PRINTED sessions reference %r n=%d: order %.3f s, Sessions %.3f s, slowest column set %.3f s" % (pattern, N, took["order"], took["Sessions (order and heads)"],
                                                                                                          max(v for k, v in took.items() if "columns" in k)))
        if took[worst] > slowest[1]:
            slowest = (pattern + ": " + worst, took[worst])
    print("PRINTED sessions reference, slowest call at %d rows: %s, %.3f s" % (N, slowest[0], slowest[1]))
    assert slowest[1] < 5.0                                                 # whole-array numpy: a Python loop over rows would not get here
