"""The whole-array numpy restatement of the pinned fold (window_moments_numpy_reference) against the Python one
(window_moments_reference.Tree / finish), bit for bit: on every case of test_window_moments_cpu, every frame, every row, and on random
frames — empty, single-row and whole-array ones included.  And, without a GPU, the claims about the inputs of
test_window_moments_frames_gpu: on tied orders its VALUE and GROUPS frames are not the ROWS frames of the same offsets.

The cases of test_window_moments_frames_gpu and test_window_large_gpu's test_moments (patterns, sizes, frames, columns, the expected
bits of a column) are defined here once; the GPU tests import them."""
import numpy as np
import pytest

import window_moments_numpy_reference as npref
import window_moments_reference as ref
from sdqlpy_amd import abi
from test_window_exclude_gpu import EX_PATTERNS, GRP, ROWS, VAL, Excluded, _ex_pattern, _frames
from test_window_gpu import PATTERNS, _pattern
from test_window_moments_cpu import CASES, COLUMNS, TILE, data, frame_ends, frames, partition_column, restated
from test_window_range_gpu import _order_values

K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
UNITS = (VAL, GRP, ROWS)
MD, MI = (P, 2, True), (P, 3, False)                                       # _range_table's measures: a double, an integer
NOPS = len(npref.OPS)
FAR = 10 ** 18
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------
ORDERS = ["gaps", "heavy ties", "one value", "wide"]                       # test_window_range_gpu's order patterns but "dense" (consecutive, unique: a ROWS frame)
OWN = "its own"                                                            # the two patterns of test_window_exclude_gpu place their tie runs themselves
FRAME_CASES = [(p, o) for p in PATTERNS for o in ORDERS] + [(p, OWN) for p in EX_PATTERNS[len(PATTERNS):]]


def frame_sizes(T):
    """a partial tile, a tile boundary, a tile with ragged upper levels, the first size above SORT_TILE blocks"""
    return [2, 65, T - 1, T, T + 1, 3 * T + 5, 4097]


def tied(pattern, order):
    return order != "wide" and pattern != "every row its own"


def frame_case(pattern, order, at, n, T):
    """-> (partition ids, int64 order values, descending?, doubles, integers) of the table of a case at its at-th size, rows in
    random build order.  The doubles are general ones: nothing in the fold is exact, so the bits tell the leaf order inside ties."""
    case = FRAME_CASES.index((pattern, order))
    rng = np.random.default_rng(7000 + 100 * case + at)
    if order == OWN:
        part, values = _ex_pattern(pattern, n, T, rng)
    else:
        part = _pattern(pattern, n, T, rng)[0]
        values = _order_values(order, part, rng)
    if order != "wide":
        values = _twins_at_the_ends(part, values)
    return part, values, (at + case) % 2 == 1, 1e6 + rng.standard_normal(n), rng.integers(-1000, 1000, n)


def _twins_at_the_ends(part, values):
    """In every partition of four rows or more the smallest and the largest order value come twice at least: the first and the last
    tie run of the partition hold two rows, so a frame wholly before or behind the row is empty for a row that a ROWS frame gives a
    neighbour (where the tie runs at a partition's ends are single rows, "empty" cannot tell GROUPS from ROWS)."""
    n = len(part)
    values = values.copy()
    by = np.lexsort((values, part))
    p = part[by]
    pos = np.arange(n)
    head, last = np.ones(n, bool), np.ones(n, bool)
    head[1:], last[:-1] = p[1:] != p[:-1], p[1:] != p[:-1]
    size = (np.append(np.nonzero(head)[0][1:], n) - np.nonzero(head)[0])[np.cumsum(head) - 1] if n else pos
    first, final = np.nonzero(head & (size >= 4))[0], np.nonzero(last & (size >= 4))[0]
    values[by[first + 1]] = values[by[first]]
    values[by[final - 1]] = values[by[final]]
    return values


def case_frames(order, n, T):
    """test_window_exclude_gpu's 24 frames; on "wide" — order values all over +-2^62 — eight more with offsets of +-10^18 and at the ends
    of int64, where value + offset passes 2^63: nothing wraps"""
    far = [(-FAR, FAR), (-FAR, -1), (1, FAR), (FAR, FAR), (I_MIN + 1, I_MAX - 1), (I_MAX - 1, I_MAX - 1), (I_MIN + 1, I_MIN + 1), (I_MIN + 1, 0)]
    return _frames(n, T) + (far if order == "wide" else [])


def moment_columns(fl, at):
    """Every frame once, four to a call: (op, Y, X, unit, lo, hi) as table_window_moments takes them.  The unit turns with the frame
    and moves by one from size to size, the op by two: over three consecutive sizes every op meets every unit.  The measures rotate
    over the double and the integer payload, alone and in both orders."""
    cols = []
    for i, (lo, hi) in enumerate(fl):
        y, x = [(MD, MI), (MI, MD), (MD, MD), (MI, MI)][(i + at) % 4]
        cols.append(((i + 2 * at) % NOPS,) + y + x + (UNITS[(i + at) % 3], lo, hi))
    return [cols[i:i + 4] for i in range(0, len(cols), 4)]


def rows_of_case(part, values, dbls, ints):
    """what _stage_rows returns for _range_table(ctx, part, values, dbls, ints)"""
    import large_patterns as LP                                            # (it imports test_window_large_gpu, which imports this module)
    return LP.synthetic_rows([part, values, dbls, ints])


def case_terms(desc):
    return [(P, 0, False, False), (P, 1, desc, False)]


class Expected:
    """The expected bits of a column of sdqh_table_window_moments over `ref` (an Excluded of the table's rows): the frame's ends from
    ref.base, the leaves in ref.order — the measures as doubles, an integer one converted once —, the fold from the numpy
    restatement.  A tree per (Y, X) is built once."""

    def __init__(self, exc):
        self.ref, self.trees, self.states = exc, {}, {}

    def leaves(self, m):
        kind, index, is_f64 = m
        return npref.leaf(self.ref.raw(kind, index), kind == V or (kind == P and bool(is_f64)))

    def ends(self, unit, lo, hi):
        """(l, r) per sorted position; l > r: empty"""
        left, right, emp = self.ref.base(unit, lo, hi)
        return np.where(emp, 1, left), np.where(emp, 0, right)

    def column(self, col):
        op, y, x, (unit, lo, hi) = col[0], tuple(col[1:4]), tuple(col[4:7]), col[7:]
        name = npref.OPS[op]
        if name in npref.UNI:
            x = y                                                          # (VAR_* and STDDEV_* ignore the second measure)
        if (y, x) not in self.trees:
            self.trees[(y, x)] = npref.Tree(self.leaves(y), None if x == y else self.leaves(x))
        key = (y, x, unit, lo, hi)
        if key not in self.states:
            self.states = {key: self.trees[(y, x)].query(*self.ends(unit, lo, hi))}      # (the last one: the columns of a call often share a frame)
        return npref.finish(name, self.states[key])


def differs_from_rows(exc, fl, cols):
    """Per unit VALUE / GROUPS of the columns `cols` over the frames fl: (a bounded frame whose l differs from the ROWS frame's with the
    same offsets on some row where both hold rows, one whose r does, a frame that is empty where the ROWS frame is not or the reverse)"""
    out = {VAL: [False] * 3, GRP: [False] * 3}
    for col in cols:
        unit, lo, hi = col[7:]
        if unit == ROWS:
            continue
        l, r, e = exc.base(unit, lo, hi)
        l0, r0, e0 = exc.base(ROWS, lo, hi)
        both = ~e & ~e0
        if lo is not None and hi is not None:
            out[unit][0] |= bool((l != l0)[both].any())
            out[unit][1] |= bool((r != r0)[both].any())
        out[unit][2] |= bool((e != e0).any())
    return out


# ---- the restatement against the restatement ---------------------------------------------------------------------------------------------
def _numpy_columns(tree, l, r):
    """{column of test_window_moments_cpu.COLUMNS: its values at every row}"""
    s = tree.query(l, r)
    sx = npref.swapped(s)
    return {(op, which): npref.finish(op, sx if which == "x" else s) for op, which in COLUMNS}


def test_the_names_are_the_header_s():
    assert npref.OPS == ref.OPS and npref.NULL_BITS == ref.NULL_BITS and (npref.UNI, npref.BI) == (ref.UNI, ref.BI)
    assert [getattr(abi, "GM_" + op.upper()) for op in npref.OPS] == list(range(NOPS))


@pytest.mark.parametrize("n,kind", CASES)
def test_bits_on_every_case_frame_and_row(n, kind):
    T = TILE
    part = partition_column(kind, n, T)
    y, x = data(n)
    tree, mine = ref.Tree(y, x), npref.Tree(y, x)
    rows = np.arange(n)
    empties = 0
    for unit, lo, hi in frames(T):
        l, r = frame_ends(part, lo, hi)
        empties += int((l > r).sum())
        want, got = restated(tree, rows, l, r), _numpy_columns(mine, l, r)
        for col in COLUMNS:
            same = npref.bits(got[col]) == npref.bits(want[col])
            assert same.all(), (n, kind, unit, lo, hi, col, rows[~same][:5], got[col][~same][:5], want[col][~same][:5])
    assert n == 0 or empties > 0


@pytest.mark.parametrize("n", [1, 2, 3, TILE - 1, TILE + 1, 3 * TILE + 5])
def test_bits_on_random_frames(n):
    """states and all nine finishes; general doubles, a constant stretch (Q = 0: the NULLs of CORR / REGR) and an integer measure"""
    rng = np.random.default_rng(n)
    y = 1e6 + rng.standard_normal(n)
    x = npref.leaf(rng.integers(-8, 8, n), False)
    y[n // 3:n // 3 + 5] = 7.0
    x[n // 3:n // 3 + 5] = 3.0
    m = 3000
    l = rng.integers(0, n, m)
    r = np.minimum(n - 1, l + rng.integers(-1, n + 1, m) // rng.integers(1, 50, m))
    l[:4], r[:4] = (0, n - 1, n // 2, n - 1), (n - 1, 0 if n > 1 else -1, n // 2, n - 2)      # the whole array, an empty frame, a single row, another empty one
    assert (l > r).any() and (l == r).any() and ((l == 0) & (r == n - 1)).any()
    tree, mine = ref.Tree(y, x), npref.Tree(y, x)
    got = mine.query(l, r)
    want = [tree.query(int(a), int(b)) if a <= b else ref.EMPTY for a, b in zip(l, r)]
    assert (got[0] == np.array([w[0] for w in want])).all()
    for k in range(1, 6):
        assert (npref.bits(got[k]) == npref.bits(np.array([w[k] for w in want]))).all(), (n, k)
    for op in npref.OPS:
        for state, swap in ((got, False), (npref.swapped(got), True)):
            a = npref.finish(op, state)
            b = np.array([ref.finish(op, (w[0], w[3], w[4], w[1], w[2], w[5]) if swap else w) for w in want])
            assert (npref.bits(a) == npref.bits(b)).all(), (n, op, swap)
    alone = npref.Tree(y)                                                  # x = None: C is Qy, bit for bit
    s = alone.query(l, r)
    assert (npref.bits(s[5]) == npref.bits(s[2])).all() and (npref.bits(s[2]) == npref.bits(got[2])).all()
    assert (npref.bits(npref.leaf(np.array([3, -4], np.int64), False)) == npref.bits(np.array([3.0, -4.0]))).all()
    assert (npref.bits(npref.leaf(npref.bits(y).view(np.int64), True)) == npref.bits(y)).all()


# ---- the inputs of test_window_moments_frames_gpu ----------------------------------------------------------------------------------------------
def test_every_op_meets_every_unit_over_the_sizes():
    T = TILE
    for order in ("gaps", "wide"):
        met = set()
        for at, n in enumerate(frame_sizes(T)):
            fl = case_frames(order, n, T)
            lists = moment_columns(fl, at)
            here = [c for cols in lists for c in cols]
            assert [(c[8], c[9]) for c in here] == fl and all(1 <= len(cols) <= abi.WM_MAX_COLS for cols in lists)
            met |= {(c[0], c[7]) for c in here}
        assert met == {(op, u) for op in range(NOPS) for u in UNITS}


@pytest.mark.parametrize("pattern,order", [c for c in FRAME_CASES if tied(*c)])
def test_tied_frames_are_not_rows_frames(pattern, order):
    """For every tied pattern, size >= T — ascending and descending alternate over them — and each of VALUE and GROUPS: a bounded frame
    whose first row is not the ROWS frame's, one whose last row is not, and a frame that is empty where the ROWS frame is not (or the
    reverse).  A library that read every unit as ROWS could not pass test_window_moments_frames_gpu at any of these sizes."""
    T = TILE
    directions = set()
    for at, n in enumerate(frame_sizes(T)):
        if n < T:
            continue
        part, values, desc, dbls, ints = frame_case(pattern, order, at, n, T)
        exc = Excluded(rows_of_case(part, values, dbls, ints), case_terms(desc), 1)
        assert exc.n == n and (~exc.ref.tie_head).any()                    # ties exist
        fl = case_frames(order, n, T)
        got = differs_from_rows(exc, fl, [c for cols in moment_columns(fl, at) for c in cols])
        assert got == {VAL: [True] * 3, GRP: [True] * 3}, (pattern, order, n, desc, got)
        directions.add(desc)
    assert directions == {False, True}
