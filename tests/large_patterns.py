"""The patterns of the tests past 256 tiles of the grouping extensions (test_group_large_gpu, test_large_patterns_cpu), and the checkers of
their structural claims: importable without a GPU.  A pattern is a tuple of term columns BY SORTED POSITION, each non-decreasing; the
tables are built from them in a random row order, and the references (Grouped, Distinct — whole-array numpy) find the positions again.

A FOLD ARRAY is an array that a one-workgroup scan (k_wagg_scan, k_sort_bins) runs over: thread t of its W = 256 threads folds the tiles
[t per, (t + 1) per) of T positions each, per = ceil(tiles / W) — one THREAD RUN of L = per T positions.  The SEAM RULE for the head
flags of such an array, of more than W T positions (seam_rule):
    heads exactly on a seam t L, one before and one after it, for several t;
    at least two whole thread runs in a row with no head (a group swallows them: the carry passes through a thread's partial);
    a thread run whose only head lies in its last tile;
and, at one of the sizes, a ragged last thread: per does not divide the tiles (ragged).
Geometry, the thread runs and the two row patterns SWALLOW / SEAMS are test_window_large_gpu's."""
import numpy as np

from test_window_large_gpu import SEAMS, SWALLOW, W, _geometry, _large_pattern, _thread_runs

ROW_SEAMS, GROUP_SEAMS = "row seams", "group seams"
GROUPING = ["one group", "every row alone", "halving", ROW_SEAMS, GROUP_SEAMS]
OWN_VALUE, RUNS_OF_2, ONE_VALUE, LONG_RUN, RUN_SEAMS, MODE_TIES = ("every row its own value", "runs of 2", "one group with one value",
                                                                   "a value run that swallows thread runs", "group seams in run space", "mode ties across a seam")
DISTINCT = [OWN_VALUE, RUNS_OF_2, ONE_VALUE, LONG_RUN, RUN_SEAMS, MODE_TIES]
FINER = "b finer than a"
MOMENTS = ["one group", "groups of 2", SWALLOW, SEAMS, ROW_SEAMS, FINER]
DEV = 1 << 16                                                              # the moments' deviations: |d| < 2^16, see moments_cap


# ---- head flags ------------------------------------------------------------------------------------------------------------------------
def cyc_heads(m, lengths):
    """head flags of m positions in runs of the given lengths, over and over"""
    lengths = np.asarray(lengths, np.int64)
    starts = np.concatenate(([0], np.cumsum(np.tile(lengths, m // int(lengths.sum()) + 1))[:-1]))
    flag = np.zeros(m, bool)
    flag[starts[starts < m]] = True
    return flag


def seam_heads(m, T, tail):
    """Head flags over an array of m > W T positions that obey the seam rule: the heads of test_window_large_gpu's SEAMS (on the seams
    1 .. 3, one before the seams 5 and 6, one after the seams 8 and 9, five before the end of the thread runs 11 .. 13 — their only
    head, in their last tile), then no head over the thread runs 14 .. 16, then runs of the lengths `tail`."""
    L = _geometry(m, T)[1] * T
    flag = np.zeros(m, bool)
    flag[[0] + [t * L for t in (1, 2, 3)] + [t * L - 1 for t in (5, 6)] + [t * L + 1 for t in (8, 9)] + [(t + 1) * L - 5 for t in (11, 12, 13)]] = True
    at = 17 * L + 3
    flag[at:] = cyc_heads(m - at, tail)
    return flag


def ids(flag):
    return (np.cumsum(flag) - 1).astype(np.int64)


def heads_of(col):
    """head flags of the runs of equal neighbours"""
    flag = np.ones(len(col), bool)
    flag[1:] = col[1:] != col[:-1]
    return flag


# ---- claims ----------------------------------------------------------------------------------------------------------------------------
def seam_counts(flag, T):
    """(heads on a seam, one before, one after, the longest stretch of whole thread runs with no head, thread runs whose only head lies
    in their last tile) of the head flags of a fold array"""
    m = len(flag)
    L = _geometry(m, T)[1] * T
    whole = m // L
    seams = np.arange(1, whole) * L                                        # (seam + 1 < m: a whole run follows every one of them)
    has = _thread_runs(flag, m, T)
    assert len(has) == whole
    gaps = np.diff(np.nonzero(np.concatenate(([True], has, [True])))[0]) - 1
    runs = flag[:whole * L].reshape(whole, L)
    only_last = (runs.sum(axis=1) == 1) & runs[:, L - T:].any(axis=1)
    return int(flag[seams].sum()), int(flag[seams - 1].sum()), int(flag[seams + 1].sum()), int(gaps.max()), int(only_last.sum())


def seam_rule(flag, T, what):
    m = len(flag)
    ntiles, per, _ = _geometry(m, T)
    assert m > W * T and ntiles > W and per >= 2 and flag[0], (what, m, per)
    on, before, after, swallowed, only_last = seam_counts(np.asarray(flag, bool), T)
    assert on >= 2 and before >= 2 and after >= 2 and swallowed >= 2 and only_last >= 1, (what, on, before, after, swallowed, only_last)
    return on, before, after, swallowed, only_last


def ragged(m, T):
    ntiles, per, _ = _geometry(m, T)
    return per >= 2 and ntiles % per != 0


def synthetic_rows(cols, seed=3):
    """what _stage_rows returns for a table without values and hits whose payloads are `cols` (doubles as their bits): keys, payload,
    None, None — the keys are test_window_range_gpu._range_table's"""
    n = len(cols[0])
    keys = np.random.default_rng(seed + n).permutation(n).astype(np.int64) * 3 - n
    return keys, [np.ascontiguousarray(c).view(np.int64) if np.asarray(c).dtype == np.float64 else np.asarray(c, np.int64) for c in cols], None, None


# ---- grouping sets: (a, b, c) ----------------------------------------------------------------------------------------------------------
def grouping_pattern(name, n, T):
    pos = np.arange(n, dtype=np.int64)
    if name == "one group":
        return pos * 0, pos * 0, pos * 0
    if name == "every row alone":                                           # every level has n groups: every lower fold runs over an n-long array
        return pos, pos, pos
    if name == "halving":
        return pos // (3 * T + 5), pos // 2, pos
    if name == ROW_SEAMS:                                                   # the level-2 heads obey the seam rule in the rows; c is finer
        b = ids(seam_heads(n, T, [60, 1, 63, 64, 65, 200]))
        return b // 7, b, pos // 3
    assert name == GROUP_SEAMS                                              # c = pos: level 3's group array is the positions
    b = ids(seam_heads(n, T, [1, 2]))                                       # level 2's heads obey the rule in it
    m2 = int(b[-1]) + 1
    if m2 > W * T:                                                          # ... and level 1's heads obey it in level 2's group array
        return ids(seam_heads(m2, T, [3, 1, 5, 2]))[b], b, pos
    return b // 9, b, pos


def grouping_columns(name, n, T, desc, rng, i_min, i_max, pack):
    """-> ([payload 0 = a * pack + b, payload 1 = c, doubles, integers] in a random build order, the seam positions that hold int64's ends)"""
    a, b, c = grouping_pattern(name, n, T)
    assert b.max() < pack and (np.diff(a) >= 0).all() and (np.diff(b) >= 0).all() and (np.diff(c) >= 0).all()
    L = _geometry(n, T)[1] * T
    ints = rng.integers(-1000, 1000, n).astype(np.int64)
    ends = np.array([L - 1, L, 2 * L, 2 * L + 1, 5 * L - 1, 5 * L, 8 * L, 8 * L + 1])
    ints[ends] = [i_max, i_min, i_min, i_max, i_max, i_max, i_min, i_min]
    if desc:                                                                # descending terms over mirrored values: the same sorted order
        a, b, c = a.max() - a, b.max() - b, c.max() - c
    dbls = rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64)
    mix = rng.permutation(n)
    return [(a * pack + b)[mix], c[mix], dbls[mix], ints[mix]], ends


def grouping_claims(name, ref, T):
    """the structural claims of a grouping pattern on its reference (test_grouping_sets_gpu.Grouped): the fold arrays are the rows (for
    the highest level asked for) and, for a lower level, the group array of the level it is folded from.  Returns the fold arrays, as
    (from level or "rows", to level, length), that obey the whole seam rule."""
    n = ref.n
    counts = [len(s) for s in ref.starts]
    ruled = []
    assert n > W * T and _geometry(n, T)[1] >= 2
    if name == "one group":
        assert counts == [1, 1, 1, 1] and not _thread_runs(ref.heads[3], n, T)[1:].any()
    if name == "every row alone":
        assert counts == [1, n, n, n]
    if name == "halving":
        split = len(range(3 * T + 5, n, 2 * (3 * T + 5)))                   # 3 T + 5 is odd: every other head of a cuts a pair of b in two
        assert counts[3] == n and counts[2] == (n + 1) // 2 + split and counts[1] == -(-n // (3 * T + 5))
        if n == 2 * W * T + T + 1:                                          # level 2 is folded over 514 tiles of groups, per 3; level 1 over 257 tiles, per 2, ragged
            assert counts[3] == 262657 and _geometry(counts[3], T)[:2] == (514, 3)
            assert (n + 1) // 2 == 131329 and split == 85 and counts[2] == 131414 and _geometry(counts[2], T)[:2] == (257, 2) and ragged(counts[2], T)
    if name == ROW_SEAMS:
        seam_rule(ref.heads[2], T, (name, "level 2 in the rows"))
        ruled.append(("rows", 2, n))
        assert counts[3] > counts[2] > counts[1] > 1
    if name == GROUP_SEAMS:
        assert counts[3] == n
        seam_rule(ref.heads[2], T, (name, "level 2 in level 3's groups"))   # (level 3's groups are the positions)
        ruled.append((3, 2, n))
        if n == 2 * W * T + T + 1:
            assert counts[2] > W * T and _geometry(counts[2], T)[1] == 2 and ragged(counts[2], T), counts
            seam_rule(ref.heads[1][ref.starts[2]], T, (name, "level 1 in level 2's groups"))
            ruled.append((2, 1, counts[2]))
    return ruled


# ---- group distinct: (a, b, c), (a, b) the group, c the value --------------------------------------------------------------------------
def mode_tie_runs(n, T):
    """run lengths (all 1 but three pairs of 3) and the groups cut around the pairs: -> (lengths, [(first run, end run)] per pair).  The
    pairs lie either side of a thread seam of the run array (where the run array has thread runs of more than one tile; of a tile edge
    otherwise), of a tile edge inside a thread run of the run array, and of a thread seam of the rows."""
    nr = n - 12
    lens = np.ones(nr, np.int64)
    Lr, Lrow = _geometry(nr, T)[1] * T, _geometry(n, T)[1] * T
    s1, e2, p3 = 2 * Lr, 4 * Lr + T, 7 * Lrow
    r3 = p3 - 5 - 8                                                         # (the two pairs before it moved every start by 8)
    lens[[s1 - 3, s1 + 2, e2 - 2, e2 + 1, r3, r3 + 5]] = 3
    return lens, [(s1 - 20, s1 + 20), (e2 - 20, e2 + 20), (r3 - 20, r3 + 25)]


def distinct_pattern(name, n, T):
    pos = np.arange(n, dtype=np.int64)
    per = _geometry(n, T)[1]
    if name == OWN_VALUE:                                                   # as many runs as rows
        return pos * 0, pos // (T + 188), pos
    if name == RUNS_OF_2:
        return pos * 0, (pos // 2) // (T + 188), pos // 2
    if name == ONE_VALUE:
        return pos * 0, pos * 0, pos * 0
    if name == LONG_RUN:                                                    # T + 7 runs of one row: the long one starts off every seam
        lead, tie = T + 7, (4 * per + 1) * T + 5
        flag = np.ones(n, bool)
        flag[lead + 1:lead + tie] = False
        flag[lead + tie:] = cyc_heads(n - lead - tie, [3, 1, 5, 2])
        c = ids(flag)
        return pos * 0, c // 50, c
    if name == RUN_SEAMS:                                                   # the group heads obey the seam rule in the run array
        c = pos if n <= 2 * W * T else ids(cyc_heads(n, [1, 1, 2]))
        return pos * 0, ids(seam_heads(int(c[-1]) + 1, T, [3, 1, 5, 2]))[c], c
    assert name == MODE_TIES
    lens, groups = mode_tie_runs(n, T)
    head = np.arange(len(lens)) % 67 == 0
    for lo, hi in groups:
        head[lo + 1:hi] = False
        head[[lo, hi]] = True
    c = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    return pos * 0, ids(head)[c], c


def distinct_columns(name, n, T, desc, rng, i_min, i_max, pack):
    a, b, c = distinct_pattern(name, n, T)
    assert len(c) == n and b.max() < pack and (np.diff(b) >= 0).all() and (np.diff(c) >= 0).all()
    L = _geometry(n, T)[1] * T
    ints = rng.integers(-1000, 1000, n).astype(np.int64)
    ints[[L - 1, L, 2 * L, 2 * L + 1]] = [i_max, i_min, i_min, i_max]
    if desc:
        a, b, c = a.max() - a, b.max() - b, c.max() - c
    dbls = rng.integers(-(1 << 30), 1 << 30, n).astype(np.float64)
    mix = rng.permutation(n)
    return [(a * pack + b)[mix], c[mix], dbls[mix], ints[mix]]


def distinct_claims(name, ref, T):
    """the structural claims of a distinct pattern on its reference (test_group_distinct_gpu.Distinct, ngroup = 2): the fold arrays are
    the rows (k_sort_bins' tile offsets) and the value runs (the upper stage)"""
    n, nr = ref.n, ref.nruns
    group_head = np.zeros(nr, bool)
    group_head[ref.gfirst] = True
    assert n > W * T
    if name == OWN_VALUE:
        assert nr == n and ref.g > 100 and (n != 2 * W * T + T + 1 or _geometry(nr, T)[:2] == (514, 3))
    if name == RUNS_OF_2:
        assert nr == (n + 1) // 2 and (n != 2 * W * T + T + 1 or (_geometry(nr, T)[:2] == (257, 2) and ragged(nr, T)))
    if name == ONE_VALUE:
        assert nr == ref.g == 1
    if name == LONG_RUN:
        per = _geometry(n, T)[1]
        j = int(np.argmax(ref.rlen))
        assert ref.rlen[j] == (4 * per + 1) * T + 5 > (1 << 11) * per and ref.rstart[j] % T != 0
        run_head = np.zeros(n, bool)
        run_head[ref.rstart] = True
        assert seam_counts(run_head, T)[3] >= 2                             # it swallows whole thread runs of the rows
        assert ref.longest.max() == ref.rlen[j] and ref.runs[np.argmax(ref.longest)] > 1      # MODE_COUNT above 2^11 per, in a group of several runs
    if name == RUN_SEAMS:
        assert nr > W * T and ragged(nr, T) and (n != 2 * W * T + T + 1 or (n > nr and _geometry(nr, T)[1] == 2))
        seam_rule(group_head, T, (name, "the group heads in the run array"))
    if name == MODE_TIES:
        Lr, Lrow = _geometry(nr, T)[1] * T, _geometry(n, T)[1] * T
        met = set()
        for j in np.nonzero(ref.longest == 3)[0]:                           # (three groups)
            r1, r2 = (ref.gfirst[j] + np.nonzero(ref.tied[ref.gfirst[j]:ref.gfirst[j] + ref.runs[j]])[0])
            assert ref.winner[j] == r1 < r2                                 # two longest runs of equal length: the earlier one wins
            if r1 // Lr != r2 // Lr:
                met.add("a seam of the run array")
            elif r1 // T != r2 // T:
                met.add("a tile edge of the run array")
            if ref.rstart[r1] // Lrow != ref.rstart[r2] // Lrow:
                met.add("a seam of the rows")
        assert met >= {"a seam of the run array", "a seam of the rows"} and (nr <= W * T or "a tile edge of the run array" in met), met
        assert nr <= W * T or _geometry(nr, T)[1] >= 2


# ---- group moments: (a, b) -------------------------------------------------------------------------------------------------------------
def moments_pattern(name, n, T, rng):
    pos = np.arange(n, dtype=np.int64)
    if name == "one group":
        return pos * 0, pos * 0
    if name == "groups of 2":
        return pos // (T + 38), pos // 2
    if name == SWALLOW:                                                     # the partitions of the window tests' pattern lie in the order of their ids
        b = np.sort(_large_pattern(SWALLOW, n, T, rng)[0])
        return b // 5, b
    if name == SEAMS:
        b = np.sort(_large_pattern(SEAMS, n, T, rng)[0])
        return b // 3, b
    if name == ROW_SEAMS:
        b = ids(seam_heads(n, T, [60, 1, 63, 64, 65, 200]))
        return b // 7, b
    assert name == FINER                                                    # level 1 differs from level 2
    return pos // (3 * T + 5), pos // 7


def moments_claims(name, ref, T):
    """the structural claims of a moments pattern on its reference (Grouped over the two terms): every level is folded over the rows"""
    n = ref.n
    assert n > W * T and _geometry(n, T)[1] >= 2
    on, before, after, swallowed, only_last = seam_counts(ref.heads[2], T)
    if name == "one group":
        assert len(ref.starts[2]) == 1 and swallowed == n // (_geometry(n, T)[1] * T) - 1
    if name == "groups of 2":
        assert len(ref.starts[2]) == (n + 1) // 2 and len(ref.starts[1]) == -(-n // (T + 38))
    if name == SWALLOW:
        assert swallowed >= 2
    if name == SEAMS:
        assert on >= 3 and before >= 2 and after >= 2 and only_last >= 3
    if name == ROW_SEAMS:
        seam_rule(ref.heads[2], T, (name, "level 2 in the rows"))
        assert seam_counts(ref.heads[1], T)[3] >= 2
    if name == FINER:
        assert len(ref.starts[2]) > 4 * len(ref.starts[1]) > 4
    return name == ROW_SEAMS


def moments_cap(n):
    """|d| < DEV = 2^16: a group of n <= 2^18 + 2^10 rows has Q, |C| <= n * 2^32 < 2^51, far below 2^53"""
    assert n * DEV * DEV < 1 << 53
    return n * DEV * DEV


def moments_columns(name, n, T, desc, rng, pack, kx, ky):
    """-> [payload 0 = a * pack + b, x, y, integers] in a random build order: x = kx + d, y = ky + d' with the deviations of every finest
    group symmetric about 0 (test_group_moments_gpu._symmetric) and below DEV"""
    from test_group_moments_gpu import _symmetric
    a, b = moments_pattern(name, n, T, rng)
    assert b.max() < pack and (np.diff(a) >= 0).all() and (np.diff(b) >= 0).all()
    finest = ids(heads_of(a) | heads_of(b))                                 # the level-2 groups: a head of a may cut a run of b
    x, y = _symmetric(finest, rng, kx, DEV), _symmetric(finest, rng, ky, DEV)
    if desc:
        a, b = a.max() - a, b.max() - b
    mix = rng.permutation(n)
    return [(a * pack + b)[mix], x[mix], y[mix], mix]
