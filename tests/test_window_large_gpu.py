"""The window entry points past 256 tiles on the MI355X (run with -m gpu): sdqh_table_window, _window_agg, _window_slide, _window_range,
_window_quantile, _window_exclude and _window_moments against numpy at the sizes at which a thread of the one-workgroup tile scans (k_win_scan, k_wagg_scan, k_wsl_scan in
both directions, k_wagg_next, k_sort_scan over tile_kept) folds MORE THAN ONE tile, k_wrg_upper's stride loop iterates more than once
and the fold tree grows levels above cap = 131072.  With T = 512 positions per tile and W = 256 threads in the scan workgroup, thread t
takes the tiles [t * per, (t + 1) * per), per = ceil(ntiles / W); every other window test stops at 137 tiles, where per = 1.

    rows          tiles  per  cap     what it reaches
    W T - 1, W T  256    1    131072  the last sizes with per = 1
    W T + 1       257    2    262144  a ragged last thread (thread 128 holds one tile, threads 129 .. 255 none)
    2 W T         512    2    262144
    2 W T + 1     513    3    524288
    2 W T + T + 1 514    3    524288  per does not divide the tiles; 257 live nodes at k_wrg_upper's first level
    2 W T + 2 T   514    3    524288  (ranges only) ... the 257th of which lies wholly below n, so that a query reads it

    entry point            W T + 1 and 2 W T + T + 1, six patterns         the other four sizes
    _window                test_ranks                                      test_one_call_per_entry_point
    _window_agg            test_frames                                     "
    _window_slide          test_slides                                     "
    _window_range          test_ranges (and 2 W T + 2 T)                   "
    _window_quantile       test_quantiles                                  "
    _window_exclude        test_exclusions: 24 frames, 3 units x 4 ways    test_exclusions_one_call (SWALLOW)
    _window_moments        test_moments: 8 / 4 columns (and 2 W T + 2 T)   test_moments_one_call ("one partition", SWALLOW)

Everything runs at W T + 1 and at 2 W T + T + 1 (262 657) on six partition patterns; the other four sizes take one call of four columns
per entry point.  Beside four patterns of test_window_gpu there are two of this file's own, because test_window_gpu's long tie run
(3 T + 5 rows) is shorter than one thread's run once per = 3: a tie run that swallows whole thread runs (no head of either kind in
them: the carry passes through a thread's partial untouched, forwards and backwards), followed by a stretch of distinct values longer
than a thread's run (tie heads, no partition head), and partition heads exactly on, one before and one after the seams between thread
runs, with other thread runs whose only head lies in their last tile.  Each structural claim is asserted on the reference.

The references are the sibling files' (Ranked, Framed, Slid, the range test's frame ends, the quantile test's Quant): all of them are
whole-array numpy, none loops over partitions or rows in Python at these sizes.  Values are integer-valued doubles below 2^40, so every
expected value is exact and compared bit for bit; general doubles are checked against exact int64 sums within the headers' bound.
Nothing is imported from the product's fold code.

CPU time of the references at 262 657 rows, "every row its own" (262 657 partitions), on one core without a GPU: Ranked 0.11 s, Framed
and its 31 columns 0.4 s, Quant's 50 columns 0.25 s, Slid's 56 slides 0.7 s; the slowest is Ranged's 56 ranges, 0.8 s — and 2.4 s on
"one partition", whose 220 000 distinct order values pass through Python integers once per bounded side of a frame.  A table, its
staged rows and their Ranked are built once per (pattern, size) and shared; Framed, Slid, Ranged and Quant each sort the rows once more
when a test makes one (the 0.1 s of Ranked above).  Excluded (test_window_exclude_gpu's, a Ranged) and its 24 columns: 0.9 s on "heavy
ties" up to 2.2 s on "one partition" (test_large_patterns_cpu prints them).

The window moments (k_wmo_tiles over 257 and 514 tiles, k_wmo_upper's stride loop, k_wmo_fold's queries above cap = 131072) are general
sums of squares, exact in no association: they are compared BY BITS ON EVERY ROW with the header's pinned fold restated in whole-array
numpy (window_moments_numpy_reference; test_window_moments_numpy_cpu holds it against the Python restatement bit for bit), over the frame
ends of Excluded.base.  That reference costs, on the same core: the tree 0.04 s, a column of 262 657 rows 0.1 s ("heavy ties": few
distinct frames) to 0.7 s ("one partition": a frame per row); the four columns of test_moments at 262 657 rows 0.3 s to 2.0 s, the
eight at 131 073 rows 0.4 s to 1.4 s, the one call at 263 168 rows 2.5 s.  On the MI355X's host a test_moments id takes 0.2 s to 0.8 s,
a test_moments_one_call id 0.3 s to 0.9 s, test_moments_read_the_upper_levels_second_stride 0.9 s."""
import numpy as np
import pytest

import window_moments_numpy_reference as npref
from sdqlpy_amd import abi
from test_window_moments_numpy_cpu import Expected
from test_window_gpu import KINDS, TERMS, Ranked, _pattern, _raw as _raw_window, _runs, _same, _stage_rows, _table, hip_engine     # noqa: F401 (fixture)
from test_window_agg_gpu import MEASURES, Framed, _agg, _all_combinations, _raw as _raw_agg
from test_window_slide_gpu import NAN_BITS, Slid, _bits, _last_of
from test_window_range_gpu import RM, Ranged, _order_values, _range_table
from test_window_quantile_gpu import Quant, _col, _column_lists, _same_col, _same_rows
from test_window_exclude_gpu import AVG, CUR, GROUP, NO, TIES, Excluded, _col_lists, _frames, _is_f64 as _ex_is_f64, _raw as _raw_exclude

pytestmark = pytest.mark.gpu

W = 256      # threads of the one-workgroup tile scans: TPB in sdqlpy_amd/csrc/sdqh_kernels.hpp (tests/test_abi_cpu.py guards W * T == 131072)

ALL = abi.SORT_ALL
K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
SUM, COUNT, MIN, MAX, FIRST, LAST = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WSLIDE_FIRST, abi.WSLIDE_LAST
ROWS, RANGE, PARTITION = abi.FRAME_ROWS, abi.FRAME_RANGE, abi.FRAME_PARTITION
UP, UF = abi.SLIDE_UNBOUNDED_PRECEDING, abi.SLIDE_UNBOUNDED_FOLLOWING
VAL, GRP = abi.WRANGE_VALUE, abi.WRANGE_GROUPS
NTILE, PRANK, CDIST, NTH, DISC, CONT = abi.WQ_NTILE, abi.WQ_PERCENT_RANK, abi.WQ_CUME_DIST, abi.WQ_NTH, abi.WQ_PERCENTILE_DISC, abi.WQ_PERCENTILE_CONT
MD, MH, MI = MEASURES                                                      # value 0 (a double), the hit count, an integer payload

SWALLOW, SEAMS = "a tie run that swallows thread runs", "heads at the seams"
PATTERNS = ["one partition", "every row its own", "runs", "heavy ties", SWALLOW, SEAMS]
FULL = ["W*T+1", "2*W*T+T+1"]                                              # everything runs here
LIGHT = ["W*T-1", "W*T", "2*W*T", "2*W*T+1"]                               # one call per entry point


def _rows_of(size, T):
    return {"W*T-1": W * T - 1, "W*T": W * T, "W*T+1": W * T + 1, "2*W*T": 2 * W * T, "2*W*T+1": 2 * W * T + 1, "2*W*T+T+1": 2 * W * T + T + 1,
            "2*W*T+2*T": 2 * W * T + 2 * T}[size]


def _geometry(n, T):
    """(tiles, tiles per thread of the scan workgroup, leaves of the padded fold tree) — restated from the kernels' comments"""
    ntiles = -(-n // T)
    return ntiles, -(-ntiles // W), 1 << (n - 1).bit_length()


def _upper_levels(n, T):
    """k_wrg_upper's levels above the tiles, bottom up: (live nodes, does the last live node lack its right child?).  A node of the
    level `up` above the tiles covers 2^up tiles; node i's right child starts at tile (2 i + 1) << (up - 1)."""
    ntiles, _, cap = _geometry(n, T)
    out, up = [], 1
    while cap // (T << up) >= 1:
        live = min(cap // (T << up), ((ntiles - 1) >> up) + 1)
        out.append((live, ((2 * (live - 1) + 1) << (up - 1)) >= ntiles))
        up += 1
    return out


# ---- patterns ----------------------------------------------------------------------------------------------------------------------
def _large_pattern(name, n, T, rng):
    """-> (partition ids, values, hits), rows in random build order.  The sorted order is by partition id, then value descending, then
    hits: the partitions lie in the order of their ids, so their lengths place the heads."""
    if name not in (SWALLOW, SEAMS):
        return _pattern(name, n, T, rng)
    per = _geometry(n, T)[1]
    L = per * T                                                            # positions of one thread's run
    value = rng.integers(-50, 50, n).astype(np.float64)
    hits = rng.integers(1, 4, n)
    if name == SWALLOW:
        lead, tie, climb = T + 7, (4 * per + 1) * T + 5, 2 * L + 11        # T + 7 partitions of one row: the long one starts off every seam
        rest = n - lead - tie - climb
        part = np.concatenate([np.arange(lead), np.full(tie + climb, lead), lead + 1 + _runs(rest, [3, 1, 5, 2])]).astype(np.int64)
        value[lead:lead + tie], hits[lead:lead + tie] = 7.0, 2             # one tie run ...
        value[lead + tie:lead + tie + climb] = -100.0 - np.arange(climb)   # ... then distinct values below it, in this order (value descends)
    else:
        heads = [0] + [t * L for t in (1, 2, 3)] + [t * L - 1 for t in (5, 6)] + [t * L + 1 for t in (8, 9)] + [(t + 1) * L - 5 for t in (11, 12, 13)]
        tail = 15 * L
        flag = np.zeros(tail, np.int64)
        flag[heads] = 1
        part = np.concatenate([np.cumsum(flag) - 1, len(heads) + _runs(n - tail, [60, 1, 63, 64, 65, 200])]).astype(np.int64)
    assert len(part) == n
    mix = rng.permutation(n)
    return part[mix], value[mix], hits[mix]


def _thread_runs(flag, n, T, backward=False):
    """Per thread of the scan workgroup whose run holds `per` whole tiles: does any position of the run carry the flag?  Forwards
    thread t folds the tiles [t per, (t + 1) per); backwards (k_wsl_scan's second direction) the tiles [ntiles - (t + 1) per,
    ntiles - t per), met from the last one down."""
    ntiles, per, _ = _geometry(n, T)
    L = per * T
    if not backward:
        return flag[:(n // L) * L].reshape(-1, L).any(axis=1)
    padded = np.concatenate([flag, np.zeros(ntiles * T - n, bool)])
    return padded[(ntiles % per) * T:].reshape(-1, L).any(axis=1)[::-1]


def _structure(pattern, ref, T):
    """the structural claims of the pattern, on the reference's heads"""
    n = ref.n
    ntiles, per, _ = _geometry(n, T)
    L = per * T
    assert per >= 2 and ntiles > W
    part_last, tie_last = np.append(ref.part_head[1:], True), np.append(ref.tie_head[1:], True)
    if pattern == "one partition":
        assert ref.part_head.sum() == 1 and _thread_runs(ref.tie_head, n, T).all()
    if pattern == "every row its own":
        assert ref.part_head.all()
    if pattern == SWALLOW:
        ph, th = _thread_runs(ref.part_head, n, T), _thread_runs(ref.tie_head, n, T)
        assert (~th).sum() >= 2                                            # whole thread runs with no head of either kind: the carry passes through
        assert (th & ~ph).sum() >= 1                                       # ... and one with tie heads but no partition head
        assert (~_thread_runs(tie_last, n, T, backward=True)).sum() >= 2   # the same met backwards: no run of either kind ends in them
        assert (~_thread_runs(part_last, n, T, backward=True) & _thread_runs(tie_last, n, T, backward=True)).sum() >= 1
        first = np.nonzero(~th)[0][0]
        start = np.nonzero(ref.tie_head[:first * L])[0][-1]                # the long tie run's head: off every seam
        assert start % L != 0 and start % T != 0 and _last_of(ref.tie_head)[start] - start + 1 == (4 * per + 1) * T + 5
    if pattern == SEAMS:
        heads = np.nonzero(ref.part_head)[0]
        on, before, after = (sum(1 for t in range(1, 15) if ref.part_head[t * L + d]) for d in (0, -1, 1))
        assert on >= 3 and before >= 2 and after >= 2, (on, before, after)
        only_last = 0
        for t in range(1, 15):                                             # thread runs whose only head lies in their last tile
            inside = heads[(heads >= t * L) & (heads < (t + 1) * L)]
            only_last += len(inside) == 1 and inside[0] >= (t + 1) * L - T
        assert only_last >= 3
        assert any(ref.part_head[t * L:t * L + T].any() for t in range(1, 15))      # ... and heads in the first tile of a run


def _ranged_columns(pattern, part, value, rng):
    """-> (order values, descending?, doubles, integers) of the range tests' table of a pattern"""
    order = value.astype(np.int64) if pattern in (SWALLOW, "heavy ties") else _order_values("gaps", part, rng)
    return order, pattern in ("runs", SWALLOW), rng.integers(-50, 50, len(part)).astype(np.float64), rng.integers(-1000, 1000, len(part))


# ---- shared tables -----------------------------------------------------------------------------------------------------------------
class Case:
    """one table of a (pattern, size), its staged rows and their Ranked, built once and shared by the tests of the module"""

    def __init__(self, ctx, pattern, n, T, ranged):
        rng = np.random.default_rng(PATTERNS.index(pattern) * 1000003 + n)
        part, value, hits = _large_pattern(pattern, n, T, rng)
        self.ctx, self.pattern, self.n, self.T = ctx, pattern, n, T
        if ranged:                                                         # the range test's table: payloads part, order, a double, an integer
            order, self.desc, dbls, ints = _ranged_columns(pattern, part, value, rng)
            self.terms, self.min_hits = [(P, 0, False, False), (P, 1, self.desc, False)], 0
            self.t = _range_table(ctx, part, order, dbls, ints)
        else:
            self.terms, self.min_hits = TERMS, 1
            self.t = _table(ctx, part, value, hits)
        self.rows = _stage_rows(ctx, self.t, self.min_hits)
        self.ref = Ranked(self.rows, self.terms, 1)
        assert self.ref.n == n
        if n > W * T:
            _structure(pattern, self.ref, T)


@pytest.fixture(scope="module")
def cases(hip_engine):
    ctx = hip_engine.ctx
    T = ctx.window_geometry()
    made = {}

    def get(pattern, size, ranged=False):
        key = (pattern, size, ranged)
        if key not in made:
            made[key] = Case(ctx, pattern, _rows_of(size, T), T, ranged)
        return made[key]
    yield get
    for c in made.values():
        c.t.free()


def _equal(got, want, what):
    assert np.shape(got) == np.shape(want), (what, np.shape(got), np.shape(want))
    bad = np.nonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))[0]
    assert len(bad) == 0, (what, bad[:5], _bits(got).reshape(-1)[bad[:5]], _bits(want).reshape(-1)[bad[:5]])


# 0. the sizes reach what the file says they reach ---------------------------------------------------------------------------------------
def test_geometry(hip_engine):
    ctx = hip_engine.ctx
    T = ctx.window_geometry()
    assert T == 512 and ctx.window_agg_geometry() == T and ctx.window_slide_geometry()[0] == T and ctx.window_range_geometry()[0] == T and ctx.window_quantile_geometry() == T
    geo = {s: _geometry(_rows_of(s, T), T) for s in LIGHT + FULL}
    assert geo == {"W*T-1": (256, 1, 131072), "W*T": (256, 1, 131072), "W*T+1": (257, 2, 262144), "2*W*T": (512, 2, 262144), "2*W*T+1": (513, 3, 524288),
                   "2*W*T+T+1": (514, 3, 524288)}
    # the ragged case: per = 2 over 257 tiles — threads 0 .. 127 hold two tiles, thread 128 one, threads 129 .. 255 none
    ntiles, per, _ = geo["W*T+1"]
    held = [max(0, min(ntiles, (t + 1) * per) - min(ntiles, t * per)) for t in range(W)]
    assert held[:128] == [2] * 128 and held[128] == 1 and held[129:] == [0] * 127
    # per = 3 does not divide 514 tiles: thread 171 holds one tile
    ntiles, per, _ = geo["2*W*T+T+1"]
    assert ntiles % per == 1 and min(ntiles, 172 * per) - 171 * per == 1
    # k_wrg_upper: 257 live nodes at the first level above the tiles (its stride loop of W threads iterates twice) ...
    assert _upper_levels(_rows_of("2*W*T+T+1", T), T)[0][0] == 257 and _upper_levels(_rows_of("2*W*T+1", T), T)[0][0] == 257
    assert all(live <= W for s in ("W*T-1", "W*T", "W*T+1", "2*W*T") for live, _ in _upper_levels(_rows_of(s, T), T))
    # ... and at every size above W T a live node whose right child does not exist (at W T + 1 and 2 W T + 1 at the first level:
    # (ntiles - 1) >> 1 is even)
    for s in ("W*T+1", "2*W*T+1", "2*W*T+T+1"):
        assert any(missing for _, missing in _upper_levels(_rows_of(s, T), T)), s
    assert _upper_levels(_rows_of("W*T+1", T), T)[0] == (129, True) and ((257 - 1) >> 1) % 2 == 0
    # levels above cap = 131072 leaves exist from W T + 1 on
    assert len(_upper_levels(_rows_of("W*T", T), T)) == 8 and len(_upper_levels(_rows_of("W*T+1", T), T)) == 9 and len(_upper_levels(_rows_of("2*W*T+1", T), T)) == 10


# 1. ranks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_ranks(cases, pattern, size):
    """ROW_NUMBER, RANK, DENSE_RANK with every row kept; per_limit in {1, 3}: few rows kept, so k_sort_scan over tile_kept runs with
    per >= 2 on sparse counts; per_limit = 1 with a limit below the kept count; the count-only call; a capacity one too small."""
    c = cases(pattern, size)
    ctx, t, rows, ref, n = c.ctx, c.t, c.rows, c.ref, c.n
    for kind in KINDS:
        for per_limit in (ALL, 1, 3):
            sel = ref.kept(kind, per_limit)
            assert per_limit == ALL or pattern not in ("one partition", "runs", SEAMS) or len(sel) < n // 8      # far below n: most tiles keep nothing
            got = ctx.table_window(t, 1, 1, TERMS, kind, per_limit, ALL, len(sel), want_hits=True)
            _same(got, rows, ref.order[sel], (pattern, n, kind, per_limit))
            assert got[4].dtype == np.int64 and (got[4] == ref.ranks[kind][sel]).all(), (pattern, n, kind, per_limit, "ranks")
            assert _raw_window(ctx, t, 1, 1, TERMS, kind, per_limit, ALL, 0) == (abi.OK, len(sel)), (pattern, n, kind, per_limit, "count")
        sel = ref.kept(kind, 1)
        limit = max(1, len(sel) // 2)
        got = ctx.table_window(t, 1, 1, TERMS, kind, 1, limit, limit, want_hits=True)
        _same(got, rows, ref.order[sel[:limit]], (pattern, n, kind, "limit", limit))
        assert (got[4] == ref.ranks[kind][sel[:limit]]).all()
    kept = len(ref.kept(abi.WIN_RANK, 3))
    keys, rank = np.full(n, -7, np.int64), np.full(n, -7, np.int64)
    assert _raw_window(ctx, t, 1, 1, TERMS, abi.WIN_RANK, 3, ALL, kept - 1, keys, rank) == (abi.ERR_OVERFLOW, kept)
    assert _raw_window(ctx, t, 1, 1, TERMS, abi.WIN_ROW_NUMBER, ALL, ALL, n - 1, keys, rank) == (abi.ERR_OVERFLOW, n)
    assert (keys == -7).all() and (rank == -7).all()


# 2. frames --------------------------------------------------------------------------------------------------------------------------------
def _check_frames(c, ref, lists, limits):
    ctx, t, rows, n = c.ctx, c.t, c.rows, c.n
    done = 0
    for i, aggs in enumerate(lists):
        for limit in (limits if i == 0 or len(aggs) == 1 else (ALL,)):
            m = min(limit, n)
            got = ctx.table_window_agg(t, 1, 1, TERMS, aggs, limit, m, want_hits=True)
            _same(got, rows, ref.order[:m], (c.pattern, n, aggs, limit))
            assert len(got[4]) == len(aggs)
            for a, agg in zip(got[4], aggs):
                assert a.dtype == (np.float64 if agg[0] != COUNT and agg[2] == V else np.int64), (c.pattern, n, agg)
                _equal(a, ref.want(agg)[:m], (c.pattern, n, agg, limit))
                done += 1
    return done


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_frames(cases, pattern, size):
    """SUM, COUNT, MIN, MAX over ROWS, RANGE and PARTITION of the double, the hit count and the integer payload; limits 1, n / 2,
    W T + 1 (k_wagg_ends walks 257 of the tiles, tnext was built over all of them) and ALL."""
    c = cases(pattern, size)
    ref = Framed(c.rows, TERMS, 1)
    lists, ncombos = _all_combinations()
    assert _check_frames(c, ref, lists, sorted({1, c.n // 2, W * c.T + 1, ALL})) >= ncombos
    assert _raw_agg(c.ctx, c.t, 1, 1, TERMS, lists[0], ALL, 0) == (abi.OK, c.n)
    keys, out = np.full(c.n, -7, np.int64), np.full((4, c.n), -7, np.int64)
    assert _raw_agg(c.ctx, c.t, 1, 1, TERMS, lists[0], ALL, c.n - 1, keys, out) == (abi.ERR_OVERFLOW, c.n) and (keys == -7).all() and (out == -7).all()


# 3. slides --------------------------------------------------------------------------------------------------------------------------------
def _slide_calls(n, T, per):
    """Widths 1, 3, 64, T, T + 1, per T, per T + 1 and beyond n, each looking back only, ahead only and both ways, and frames with an
    unbounded side: block heads on tile seams, on thread-run seams and on neither.  Two frames to a call of four slides; every call
    folds a SUM and a MAX (every folded slide is scanned in both directions), the fourth slide rotates over the other ops."""
    frames = []
    for w in (1, 3, 64, T, T + 1, per * T, per * T + 1, n + 2):
        p = w - 1
        frames += [(-p, 0), (0, p), (-(p // 2), p - p // 2)]
    frames = list(dict.fromkeys(frames + [(UP, 0), (0, UF), (UP, UF), (UP, 5), (-T, UF)]))
    fourth = [(MIN,) + MD, (COUNT,) + MD, (FIRST,) + MI, (LAST,) + MD, (MAX,) + MH, (MIN,) + MI]
    calls = []
    for i in range(0, len(frames), 2):
        a, b = frames[i], frames[(i + 1) % len(frames)]
        calls.append([(SUM,) + MD + a + (0,), (MAX,) + MI + a + (-1,), (SUM,) + MH + b + (NAN_BITS,), fourth[(i // 2) % len(fourth)] + b + (-9,)])
    return calls


def _check_slides(c, ref, calls):
    ctx, t, rows, n = c.ctx, c.t, c.rows, c.n
    done = 0
    for slides in calls:
        got = ctx.table_window_slide(t, 1, 1, TERMS, slides, ALL, n, want_hits=True)
        _same(got, rows, ref.order, (c.pattern, n, slides))
        assert len(got[4]) == len(slides)
        for a, s in zip(got[4], slides):
            assert a.dtype == (np.float64 if s[0] != COUNT and s[1] == V else np.int64), (c.pattern, n, s)
            _equal(a, ref.want(s), (c.pattern, n, s))
            done += 1
    return done


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_slides(cases, pattern, size):
    c = cases(pattern, size)
    per = _geometry(c.n, c.T)[1]
    ref = Slid(c.rows, TERMS, 1)
    calls = _slide_calls(c.n, c.T, per)
    assert _check_slides(c, ref, calls) == 4 * len(calls) >= 4 * 13
    # LAG / LEAD alone: nothing is folded, no scan is launched — the control
    control = [(FIRST,) + MD + (-1, -1, NAN_BITS), (FIRST,) + MI + (c.T + 1, c.T + 1, -9), (FIRST,) + MH + (-per * c.T, -per * c.T, 0), (LAST,) + MD + (1, 1, -1)]
    assert _check_slides(c, ref, [control]) == 4
    # a limit: frames that follow the row look past it
    got = c.ctx.table_window_slide(c.t, 1, 1, TERMS, calls[0], W * c.T + 1, W * c.T + 1, want_hits=True)
    for a, s in zip(got[4], calls[0]):
        _equal(a, ref.want(s)[:W * c.T + 1], (pattern, c.n, s, "limit"))


# 4. ranges --------------------------------------------------------------------------------------------------------------------------------
def _range_calls(T):
    """VALUE and GROUPS frames of a few rows, of about T rows and the whole partition (and each half of it): a tree query joins nodes
    below the tile level, above it, and both.  SUM, MIN, MAX, COUNT, FIRST, LAST."""
    frames = [(-2, 1), (-T, T), (None, None), (None, 0), (0, None), (-3 * T, -2), (5, 2 * T)]
    ops = ([(SUM,) + RM[0], (MIN,) + RM[1], (MAX,) + RM[0], (COUNT,) + RM[2]], [(SUM,) + RM[1], (FIRST,) + RM[0], (LAST,) + RM[1], (MAX,) + RM[1]])
    calls = []
    for i, (lo, hi) in enumerate(frames):
        for unit in (VAL, GRP):
            calls.append([m + (unit, lo, hi, e) for m, e in zip(ops[(i + unit) % 2], (0, -1, NAN_BITS, -9))])
    return calls


def _check_ranges(c, ref, calls, limit=ALL):
    ctx, t, rows, n = c.ctx, c.t, c.rows, c.n
    done, m = 0, min(limit, n)
    for ranges in calls:
        got = ctx.table_window_range(t, 0, 1, c.terms, ranges, limit, m, want_hits=False)
        _same(got, rows, ref.order[:m], (c.pattern, n, ranges))
        assert len(got[4]) == len(ranges)
        for a, rg in zip(got[4], ranges):
            assert a.dtype == (np.float64 if rg[0] != COUNT and rg[3] else np.int64), (c.pattern, n, rg)
            _equal(a, ref.want_range(rg)[:m], (c.pattern, n, rg, limit))
            done += 1
    return done


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_ranges(cases, pattern, size):
    c = cases(pattern, size, ranged=True)
    ref = Ranged(c.rows, c.terms, 1)
    calls = _range_calls(c.T)
    assert _check_ranges(c, ref, calls) == 4 * len(calls) == 4 * 14
    if pattern == "one partition":                                         # frames of every scale exist: a few rows, about a tile, everything
        for unit in (VAL, GRP):
            left, right, emp = ref.ends(unit, -2, 1)
            assert not emp.any() and (right - left + 1).max() < 64
            left, right, emp = ref.ends(unit, -c.T, c.T)
            assert np.median(right - left + 1) > c.T // 2 and (right - left + 1).max() < 4 * c.T
            left, right, emp = ref.ends(unit, None, None)
            assert (left == 0).all() and (right == c.n - 1).all()
        assert any(missing for _, missing in _upper_levels(c.n, c.T))      # the whole-table query passes a node whose right child does not exist
    assert _check_ranges(c, ref, calls[:2], limit=W * c.T + 1) == 8


def test_ranges_read_the_upper_levels_second_stride(cases):
    """At 262 657 rows k_wrg_upper's first level has 257 live nodes, but the 257th covers positions beyond n, and a node that does is
    never read by a query: a wrong second iteration of the stride loop cannot show there.  At 2 W T + 2 T rows the node lies wholly
    below n — it covers the last two tiles — and the iterative query of a frame that ends at the table's last row reads it: at level
    h it takes node ((cap + r + 1) >> h) - 1 whenever (cap + r + 1) >> h is odd, and at h = 10, r = n - 1 that is node 512 + 256."""
    c = cases("one partition", "2*W*T+2*T", ranged=True)
    n, T = c.n, c.T
    ntiles, per, cap = _geometry(n, T)
    assert (ntiles, per, cap) == (514, 3, 524288) and _upper_levels(n, T)[0][0] == 257 > W and n >= 257 * 2 * T
    assert all(((cap + n) >> h) % 2 == 0 for h in range(10)) and ((cap + n) >> 10) % 2 == 1 and ((cap + n) >> 10) - 1 == (cap >> 10) + 256
    ref = Ranged(c.rows, c.terms, 1)
    calls = _range_calls(T)
    for unit in (VAL, GRP):                                                # frames that end at the last row exist for many rows
        left, right, emp = ref.ends(unit, 0, None)
        assert (right == n - 1).all() and (left < 2 * W * T).sum() > 2 * W * T - 8
    assert _check_ranges(c, ref, calls) == 4 * len(calls)


# 5. quantiles -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_quantiles(cases, pattern, size):
    """NTILE, PERCENT_RANK, CUME_DIST, NTH(+-k), PERCENTILE_DISC / CONT and the median, for every row and with per_limit = 1.  In the
    tie run that swallows thread runs both the tie run's end and the partition's end come from k_wagg_next, several threads away."""
    c = cases(pattern, size)
    ctx, t, rows, n = c.ctx, c.t, c.rows, c.n
    ref = Quant(rows, TERMS, 1)
    fixed, mixed = _column_lists(ref)
    want = {}

    def expect(col):
        if col not in want:
            want[col] = ref.want(col)
        return want[col]
    for cols in fixed + mixed:
        got = ctx.table_window_quantile(t, 1, 1, TERMS, cols, ALL, ALL, n, want_hits=True)
        _same_rows(got, rows, ref.order, (pattern, n, cols))
        for col, a in zip(cols, got[4]):
            _same_col(col, a, expect(col), (pattern, n))
    assert any(col[0] == CONT and col[5] == 0.5 for cols in fixed for col in cols)       # the median
    sel = np.nonzero(ref.i < 1)[0]
    for cols in fixed:
        got = ctx.table_window_quantile(t, 1, 1, TERMS, cols, 1, ALL, len(sel), want_hits=True)
        _same_rows(got, rows, ref.order[sel], (pattern, n, cols, "per_limit 1"))
        for col, a in zip(cols, got[4]):
            _same_col(col, a, expect(col)[sel], (pattern, n, "per_limit 1"))
    if pattern == SWALLOW:
        far = (ref.l - ref.i) // c.T                                       # tiles between a row and its tie run's end
        assert far.max() >= 4 * _geometry(n, c.T)[1] and ((ref.m - 1 - ref.i) // c.T).max() >= 6 * _geometry(n, c.T)[1]


# 6. the other sizes: one call of four columns per entry point ------------------------------------------------------------------------------
@pytest.mark.parametrize("size", LIGHT)
@pytest.mark.parametrize("pattern", ["one partition", SWALLOW])
def test_one_call_per_entry_point(cases, pattern, size):
    """An integer sum, a double sum, an extremum and a count or a first in every call; the range call runs at every edge of cap."""
    c = cases(pattern, size)
    ctx, t, rows, ref, n, T = c.ctx, c.t, c.rows, c.ref, c.n, c.T
    per = _geometry(n, T)[1]
    got = ctx.table_window(t, 1, 1, TERMS, abi.WIN_DENSE_RANK, ALL, ALL, n, want_hits=True)
    _same(got, rows, ref.order, (pattern, n, "ranks"))
    assert (got[4] == ref.ranks[abi.WIN_DENSE_RANK]).all()
    sel = ref.kept(abi.WIN_RANK, 3)
    got = ctx.table_window(t, 1, 1, TERMS, abi.WIN_RANK, 3, ALL, len(sel), want_hits=True)
    _same(got, rows, ref.order[sel], (pattern, n, "rank <= 3"))
    assert (got[4] == ref.ranks[abi.WIN_RANK][sel]).all()
    assert _check_frames(c, Framed(rows, TERMS, 1), [[_agg(SUM, ROWS, MH), _agg(SUM, RANGE, MD), _agg(MAX, PARTITION, MI), _agg(COUNT, RANGE, MD)]], (ALL,)) == 4
    assert _check_slides(c, Slid(rows, TERMS, 1), [[(SUM,) + MH + (-per * T, 0, 0), (SUM,) + MD + (0, T + 1, 0), (MIN,) + MI + (UP, UF, 0), (FIRST,) + MD + (-1, -1, NAN_BITS)]]) == 4
    quant = Quant(rows, TERMS, 1)
    cols = [_col(CONT, MD, p=0.5), _col(CDIST), _col(PRANK), _col(DISC, MH, p=0.9)]
    got = ctx.table_window_quantile(t, 1, 1, TERMS, cols, ALL, ALL, n, want_hits=True)
    _same_rows(got, rows, quant.order, (pattern, n, "quantiles"))
    for col, a in zip(cols, got[4]):
        _same_col(col, a, quant.want(col), (pattern, n))
    r = cases(pattern, size, ranged=True)
    ranges = [(SUM,) + RM[1] + (GRP, -2, 1, 0), (SUM,) + RM[0] + (VAL, -T, T, 0), (MAX,) + RM[1] + (VAL, None, None, 0), (COUNT,) + RM[2] + (VAL, 0, None, 0)]
    assert _check_ranges(r, Ranged(r.rows, r.terms, 1), [ranges]) == 4


# 6b. exclusions ----------------------------------------------------------------------------------------------------------------------------
def _query_heights(a, b, cap):
    """Per query [a, b] of the fold tree over cap leaves the set, as a bit mask, of the heights h whose nodes (2^h leaves each) the
    bottom-up walk takes: p = cap + a, q = cap + b + 1; while p < q: an odd p takes node p and steps right, an odd q steps left and
    takes node q; both halve.  Restated from include/sdqh_sort_exclude.h; tile nodes have height log2 T, k_wrg_upper's lie above."""
    p, q = np.asarray(a, np.int64) + cap, np.asarray(b, np.int64) + cap + 1
    mask, h = np.zeros(len(p), np.int64), 0
    while (p < q).any():
        live = p < q
        left, right = live & (p & 1 == 1), live & (q & 1 == 1)
        mask |= (left | right).astype(np.int64) << h
        p, q = (p + left) >> 1, (q - right) >> 1
        h += 1
    return mask


def _exclude_reach(ref, T):
    """On SWALLOW: some row's GROUP / TIES exclusion leaves a left and a right piece whose tree queries, together, take a node of every
    level of k_wrg_upper from which a node fits between the ends of the longest partition — a frame never leaves its partition, so no
    query can take a node that does not — and no higher one; among them the first level above the tiles, the one with 257 live nodes
    at 262 657 rows.  (The levels above that are reached by "one partition": asserted there.)  On the reference's piece ends."""
    n = ref.n
    cap = _geometry(n, T)[2]
    base = T.bit_length() - 1                                               # the tiles' height
    longest = int(np.argmax(ref.end - ref.start))
    lo, hi = int(ref.start[longest]), int(ref.end[longest])
    fits = [up for up in range(1, len(_upper_levels(n, T)) + 1) if (-(-lo // (T << up)) + 1) * (T << up) <= hi + 1]
    assert fits and fits == list(range(1, len(fits) + 1)), fits
    need = sum(1 << (base + up) for up in fits)
    upper = sum(1 << (base + up) for up in range(1, len(_upper_levels(n, T)) + 1))
    for exclude in (GROUP, TIES):
        (p1, a1, b1), _, (p3, a3, b3) = ref.pieces((SUM,) + RM[0] + (abi.WEX_ROWS, None, None, 0, exclude))[0]
        both = np.nonzero(p1 & p3)[0]
        assert len(both) > T
        took = _query_heights(a1[both], b1[both], cap) | _query_heights(a3[both], b3[both], cap)
        assert ((took & upper) == need).any(), (exclude, fits)
    return fits


def _check_exclusions(c, ref, lists, limit=ALL):
    ctx, t, rows, n = c.ctx, c.t, c.rows, c.n
    done, m = 0, min(limit, n)
    for cols in lists:
        got = ctx.table_window_exclude(t, 0, 1, c.terms, cols, limit, m, want_hits=False)
        _same(got, rows, ref.order[:m], (c.pattern, n, cols))
        assert len(got[4]) == len(cols)
        for a, col in zip(got[4], cols):
            assert a.dtype == (np.float64 if _ex_is_f64(col) else np.int64) and len(a) == m, (c.pattern, n, col)
            want = ref.want_col(col)[:m]
            bad = np.nonzero(_bits(a) != want)[0]
            assert len(bad) == 0, (c.pattern, n, col, limit, "first slot", bad[:5], "tile", bad[:5] // c.T, "thread run", bad[:5] // (_geometry(n, c.T)[1] * c.T),
                                   _bits(a)[bad[:5]], want[bad[:5]])
            done += 1
    return done


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_exclusions(cases, pattern, size):
    """test_window_exclude_gpu's 24 frames — offsets around the wave, the tile and the table, unbounded sides, frames that do not hold
    their own row — in all three units and under all four exclusions, four columns to a call; k_wex_ties takes the end of a tie run
    from k_wagg_next's tnext, several thread runs away on SWALLOW; k_wex_fold asks the tree once per piece."""
    c = cases(pattern, size, ranged=True)
    ref = Excluded(c.rows, c.terms, 1)
    frames = _frames(c.n, c.T)
    lists = _col_lists(frames, PATTERNS.index(pattern) + FULL.index(size))
    here = [col for cols in lists for col in cols]
    assert [(col[5], col[6]) for col in here] == frames and {(col[4], col[8]) for col in here} == {(u, x) for u in (VAL, GRP, abi.WEX_ROWS) for x in (NO, CUR, GROUP, TIES)}
    assert any(lo is not None and hi is not None and (lo > 0 or hi < 0) for lo, hi in frames)      # frames that do not hold their own row
    assert _check_exclusions(c, ref, lists) == 24
    assert _raw_exclude(c.ctx, c.t, 0, 1, c.terms, lists[0], ALL, 0) == (abi.OK, c.n)
    assert _check_exclusions(c, ref, lists[:1], limit=W * c.T + 1) == 4
    if pattern == SWALLOW:
        far = (ref.tie_b - ref.pos) // c.T                                  # tiles between a row and its tie run's end
        assert far.max() >= 4 * _geometry(c.n, c.T)[1]
        fits = _exclude_reach(ref, c.T)
        assert 1 in fits and (size != "2*W*T+T+1" or _upper_levels(c.n, c.T)[0][0] == 257)
    if pattern == "one partition":                                          # pieces long enough for every level below the two highest
        (p1, a1, b1), _, (p3, a3, b3) = ref.pieces((SUM,) + RM[0] + (abi.WEX_ROWS, None, None, 0, CUR))[0]
        cap, base, ups = _geometry(c.n, c.T)[2], c.T.bit_length() - 1, len(_upper_levels(c.n, c.T))
        took = np.bitwise_or.reduce(np.where(p1, _query_heights(a1, b1, cap), 0) | np.where(p3, _query_heights(a3, b3, cap), 0))
        assert all((took >> (base + up)) & 1 for up in range(1, ups - 1)), bin(took)


@pytest.mark.parametrize("size", LIGHT)
def test_exclusions_one_call(cases, size):
    """a double sum without the row, an integer maximum without its tie run, an average with the row alone of its run, a count"""
    c = cases(SWALLOW, size, ranged=True)
    T = c.T
    cols = [(SUM,) + RM[0] + (abi.WEX_ROWS, -T, T, 0, CUR), (MAX,) + RM[1] + (GRP, None, 1, -1, GROUP), (AVG,) + RM[0] + (VAL, -2, None, NAN_BITS, TIES),
            (COUNT,) + RM[2] + (abi.WEX_ROWS, None, None, 0, GROUP)]
    assert _check_exclusions(c, Excluded(c.rows, c.terms, 1), [cols]) == 4


# 6c. second moments --------------------------------------------------------------------------------------------------------------------------
def _moment_columns(pattern, size, n, T):
    """The columns of test_moments at a (pattern, size): one call of four at 262 657 rows, two at 131 073 (the reference costs about a
    second per column and 262 657 rows).  The frames are test_window_exclude_gpu's 24, rotated by the pattern; the unit turns with the
    column, the op moves on by one, the measures are the double and the integer payload, alone and in both orders."""
    fl = _frames(n, T)
    pi, big = PATTERNS.index(pattern), size == FULL[1]
    cols = []
    for k in range(4 if big else 8):
        lo, hi = fl[(4 * pi + 5 * k + (2 if big else 0)) % len(fl)]
        y, x = [(RM[0], RM[1]), (RM[1], RM[0]), (RM[0], RM[0]), (RM[1], RM[1])][(k + pi) % 4]
        cols.append(((3 * pi + k + (4 if big else 0)) % len(npref.OPS),) + y + x + ((VAL, GRP, abi.WEX_ROWS)[(k + pi) % 3], lo, hi))
    return [cols[i:i + 4] for i in range(0, len(cols), 4)]


def _check_moments(c, exc, lists):
    """every column float64 and equal BY BITS ON EVERY ROW to the numpy restatement of the pinned fold (window_moments_numpy_reference)
    over the reference's frame ends, the leaves in the reference's row order (the device's is asserted equal to it)"""
    ctx, t, rows, n = c.ctx, c.t, c.rows, c.n
    want = Expected(exc)
    done = 0
    for cols in lists:
        got = ctx.table_window_moments(t, 0, 1, c.terms, cols, ALL, n, want_hits=False)
        _same(got, rows, exc.order, (c.pattern, n, cols))
        assert len(got[4]) == len(cols)
        for a, col in zip(got[4], cols):
            assert a.dtype == np.float64 and len(a) == n, (c.pattern, n, col)
            w = want.column(col)
            bad = np.nonzero(npref.bits(a) != npref.bits(w))[0]
            assert len(bad) == 0, (c.pattern, n, col, len(bad), "first slot", bad[:5], "tile", bad[:5] // c.T, "thread run", bad[:5] // (_geometry(n, c.T)[1] * c.T), a[bad[:5]], w[bad[:5]])
            done += 1
    return done


def test_moment_columns_meet_every_unit_and_op():
    met = [col for p in PATTERNS for s in FULL for cols in _moment_columns(p, s, _rows_of(s, 512), 512) for col in cols]
    assert {col[7] for col in met} == {VAL, GRP, abi.WEX_ROWS} and {col[0] for col in met} == set(range(len(npref.OPS))) and len(met) == 6 * (4 + 8)
    assert {(col[0], col[7]) for col in met} >= {(op, u) for op in range(len(npref.OPS)) for u in (VAL, GRP)}      # every op under both units that are not ROWS
    assert len({(col[8], col[9]) for col in met}) >= 20                     # ... over most of the 24 frames


@pytest.mark.parametrize("size", FULL)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_moments(cases, pattern, size):
    """VAR / STDDEV / COVAR / CORR / REGR over VALUE, GROUPS and ROWS frames on the tables of test_ranges — ties, heads at the seams,
    descending on "runs" and SWALLOW —: k_wmo_tiles over 257 and 514 tiles, k_wmo_upper's stride loop, k_wmo_fold's queries above
    cap = 131072, by bits on every row."""
    c = cases(pattern, size, ranged=True)
    exc = Excluded(c.rows, c.terms, 1)
    lists = _moment_columns(pattern, size, c.n, c.T)
    assert _check_moments(c, exc, lists) == (4 if size == FULL[1] else 8)
    if pattern == "one partition":                                          # a frame that passes a node whose right child does not exist
        assert any(missing for _, missing in _upper_levels(c.n, c.T))


@pytest.mark.parametrize("size", LIGHT)
@pytest.mark.parametrize("pattern", ["one partition", SWALLOW])
def test_moments_one_call(cases, pattern, size):
    """a sample deviation behind the row, a correlation over the tie runs around it, a slope over the values from it on, a covariance over
    the partition up to it"""
    c = cases(pattern, size, ranged=True)
    T = c.T
    cols = [(abi.GM_STDDEV_SAMP,) + RM[0] + RM[0] + (abi.WEX_ROWS, -T, 0), (abi.GM_CORR,) + RM[0] + RM[1] + (GRP, -1, 1), (abi.GM_REGR_SLOPE,) + RM[1] + RM[0] + (VAL, 0, None),
            (abi.GM_COVAR_POP,) + RM[1] + RM[0] + (abi.WEX_ROWS, None, 0)]
    assert _check_moments(c, Excluded(c.rows, c.terms, 1), [cols]) == 4


def test_moments_read_the_upper_levels_second_stride(cases):
    """test_ranges_read_the_upper_levels_second_stride for k_wmo_upper: at 2 W T + 2 T rows the 257th live node of its first level lies
    wholly below n, and the query of a frame that ends at the table's last row reads it (node 512 + 256 at h = 10).  Over the rows
    compared — all of them — some frame reads a node on every level above the tiles but the root, which no frame shorter than cap can."""
    c = cases("one partition", "2*W*T+2*T", ranged=True)
    n, T = c.n, c.T
    ntiles, per, cap = _geometry(n, T)
    assert (ntiles, per, cap) == (514, 3, 524288) and _upper_levels(n, T)[0][0] == 257 > W
    assert all(((cap + n) >> h) % 2 == 0 for h in range(10)) and ((cap + n) >> 10) % 2 == 1 and ((cap + n) >> 10) - 1 == (cap >> 10) + 256
    exc = Excluded(c.rows, c.terms, 1)
    cols = [(abi.GM_VAR_SAMP,) + RM[0] + RM[0] + (GRP, 0, None), (abi.GM_REGR_INTERCEPT,) + RM[0] + RM[1] + (abi.WEX_ROWS, None, 0), (abi.GM_CORR,) + RM[1] + RM[0] + (VAL, None, None),
            (abi.GM_COVAR_SAMP,) + RM[0] + RM[1] + (VAL, -T, T)]
    left, right, emp = exc.base(GRP, 0, None)
    assert not emp.any() and (right == n - 1).all() and (left < 2 * W * T).sum() > 2 * W * T - 8      # frames that end at the last row: they read node 512 + 256
    base, ups = T.bit_length() - 1, len(_upper_levels(n, T))
    took = 0
    for col in cols:
        l, r, e = exc.base(*col[7:])
        took |= int(np.bitwise_or.reduce(_query_heights(l[~e], r[~e], cap)))
    assert all((took >> (base + up)) & 1 for up in range(1, ups)) and not (took >> (base + ups)) & 1, bin(took)
    assert _check_moments(c, exc, [cols]) == 4


# 7. general doubles -----------------------------------------------------------------------------------------------------------------------
def _within_the_bound(a, left, right, emp, cs, ma, what):
    """Every sum of a non-empty frame [left, right] within gamma_m * sum|v| of the exact sum, gamma_m = (m - 1) u / (1 - (m - 1) u),
    u = 2^-53, m the frame's row count — in exact integer arithmetic on the k = v * 2^20: err * (2^53 - (m - 1)) <= (m - 1) * sum|k|.
    (cs, ma: prefix sums of k and |k|, int64: n * 2^40 < 2^63.)  Empty frames hold the default.  Returns the worst err / sum|k|."""
    assert (_bits(a)[emp] == NAN_BITS).all(), what
    l, r = left[~emp], right[~emp]
    scaled = a[~emp] * float(1 << 20)                                      # a power of two: exact
    got = scaled.astype(np.int64)
    assert (np.abs(scaled) < float(1 << 62)).all() and (got.astype(np.float64) == scaled).all(), what      # an integer that int64 holds
    exact, mag, m = cs[r + 1] - cs[l], ma[r + 1] - ma[l], r - l + 1
    err = np.abs(got - exact)
    off = np.nonzero(err > 0)[0]                                           # (products beyond 64 bits: Python integers, on the rows that rounded at all)
    lhs = err[off].astype(object) * ((1 << 53) - (m[off] - 1).astype(object))
    rhs = (m[off] - 1).astype(object) * mag[off].astype(object)
    bad = off[np.nonzero((lhs > rhs).astype(bool))[0]] if len(off) else off
    assert len(bad) == 0, (what, bad[:5], err[bad[:5]], m[bad[:5]], mag[bad[:5]])
    return float((err[off] / mag[off]).max()) if len(off) else 0.0


def _same_frame_same_bits(a, left, right, emp, what):
    same = (left[1:] == left[:-1]) & (right[1:] == right[:-1]) & ~emp[1:] & ~emp[:-1]
    assert same.any() and (_bits(a)[1:][same] == _bits(a)[:-1][same]).all(), what


def test_general_doubles_within_the_bound(hip_engine):
    """262 657 rows in three partitions — longer than a thread's run, shorter than a tile, and the rest —, values k * 2^-20 with
    |k| < 2^40 spread over thirty binades: the exact frame sums are int64 sums of the k.  One SUM through each of the frame, slide and
    range calls lies within the headers' bound gamma_m * sum|v|; the same call twice gives the same bits; rows with the same frame get
    the same bits."""
    ctx = hip_engine.ctx
    T = ctx.window_geometry()
    n = 2 * W * T + T + 1
    per = _geometry(n, T)[1]
    rng = np.random.default_rng(n)
    sizes = [per * T + 77, T - 9]
    part = np.repeat(np.arange(3), sizes + [n - sum(sizes)])
    k = rng.integers(-(1 << 40) + 1, 1 << 40, n)
    k[rng.integers(0, n, n // 3)] >>= 30                                    # magnitudes spread over thirty binades
    lean = rng.random(n) < 0.75                                             # three in four positive: a long frame's sum drifts past 2^53 ulps of
    k[lean] = np.abs(k[lean])                                               # the small values, so sums round (balanced signs would stay exact)
    dbls = k.astype(np.float64) / float(1 << 20)
    assert (dbls * float(1 << 20) == k.astype(np.float64)).all() and (np.abs(k) < 1 << 40).all()
    tie = rng.integers(0, n // 3, n)                                        # order by this: ties of about three rows
    mix = rng.permutation(n)
    t = _range_table(ctx, part[mix], tie[mix], dbls[mix], np.arange(n)[mix])
    try:
        terms = [(P, 0, False, False), (P, 1, True, False)]
        rows = _stage_rows(ctx, t, 0)
        ref = Ranged(rows, terms, 1)
        assert sorted((ref.end - ref.start + 1)[ref.ref.part_head].tolist()) == sorted(sizes + [n - sum(sizes)])
        ks = np.rint(ref.column(P, 2).view(np.float64) * float(1 << 20)).astype(np.int64)
        cs, ma = np.concatenate(([0], np.cumsum(ks))), np.concatenate(([0], np.cumsum(np.abs(ks))))
        none = np.zeros(n, bool)
        m = (P, 2, True)
        worst = 0.0
        # frames: ROWS, RANGE, PARTITION
        aggs = [(SUM, ROWS) + m, (SUM, RANGE) + m, (SUM, PARTITION) + m]
        got = ctx.table_window_agg(t, 0, 1, terms, aggs, ALL, n, want_hits=False)
        again = ctx.table_window_agg(t, 0, 1, terms, aggs, ALL, n, want_hits=False)
        _same(got, rows, ref.order, "general frames")
        for a, b, right in zip(got[4], again[4], (ref.pos, _last_of(ref.ref.tie_head), ref.end)):
            _equal(a, b, "two frame calls differ")
            worst = max(worst, _within_the_bound(a, ref.start, right, none, cs, ma, "frames"))
            if right is not ref.pos:
                _same_frame_same_bits(a, ref.start, right, none, "frames")
        # slides
        frames = [(-per * T, 3), (UP, 0), (UP, UF), (-2, 2)]
        slides = [(SUM,) + m + f + (NAN_BITS,) for f in frames]
        got = ctx.table_window_slide(t, 0, 1, terms, slides, ALL, n, want_hits=False)
        again = ctx.table_window_slide(t, 0, 1, terms, slides, ALL, n, want_hits=False)
        for a, b, (lo, hi) in zip(got[4], again[4], frames):
            _equal(a, b, "two slide calls differ")
            left, right, emp = Slid.frame(ref, lo, hi)
            worst = max(worst, _within_the_bound(a, left, right, emp, cs, ma, ("slides", lo, hi)))
            if (lo, hi) == (UP, UF):
                _same_frame_same_bits(a, left, right, emp, "slides")
        # value and group ranges
        frames = [(VAL, -5, 5), (GRP, -T, 0), (GRP, None, None), (VAL, None, 0)]
        ranges = [(SUM,) + m + f + (NAN_BITS,) for f in frames]
        got = ctx.table_window_range(t, 0, 1, terms, ranges, ALL, n, want_hits=False)
        again = ctx.table_window_range(t, 0, 1, terms, ranges, ALL, n, want_hits=False)
        for a, b, (unit, lo, hi) in zip(got[4], again[4], frames):
            _equal(a, b, "two range calls differ")
            left, right, emp = ref.ends(unit, lo, hi)
            worst = max(worst, _within_the_bound(a, left, right, emp, cs, ma, ("ranges", unit, lo, hi)))
            _same_frame_same_bits(a, left, right, emp, ("ranges", unit, lo, hi))
        assert worst > 0.0                                                  # some sum rounded: the bound was exercised
        print("general doubles n=%d: worst |err| / sum|v| = %.3g (u = %.3g)" % (n, worst, 2.0 ** -53))
    finally:
        t.free()


# 8. agreement where the entry points overlap --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["runs", SWALLOW])
def test_the_entry_points_agree(cases, pattern):
    """At 262 657 rows, bit for bit (the sums are of integer-valued doubles: exact in every association): a ROWS frame and a slide over
    (unbounded, 0); a PARTITION frame, a slide and a group range unbounded both ways; sdqh_table_window with every row kept and
    sdqh_table_sorted_by."""
    c = cases(pattern, "2*W*T+T+1")
    ctx, t, n = c.ctx, c.t, c.n
    measures = [(SUM,) + MD, (SUM,) + MH, (MAX,) + MI, (MIN,) + MD]

    def same(x, y, what):                                                  # the rows' four arrays and the value columns
        pairs = list(zip(x[:4], y[:4])) + (list(zip(x[4], y[4])) if len(x) > 4 and len(y) > 4 else [])
        assert len(pairs) >= 4 and all((a is None) == (b is None) for a, b in pairs), what
        for a, b in pairs:
            if a is not None:
                _equal(np.asarray(a), np.asarray(b), (pattern, what))
    for frame, lo, hi in ((ROWS, UP, 0), (PARTITION, UP, UF)):
        frames = ctx.table_window_agg(t, 1, 1, TERMS, [(op, frame, kind, index, f) for op, kind, index, f in measures], ALL, n)
        slides = ctx.table_window_slide(t, 1, 1, TERMS, [m + (lo, hi, 0) for m in measures], ALL, n)
        assert len(frames[4]) == len(slides[4]) == 4
        same(frames, slides, (frame, "frames and slides"))
    ranges = ctx.table_window_range(t, 1, 1, TERMS, [m + (GRP, None, None, 0) for m in measures], ALL, n)
    assert len(ranges[4]) == 4
    same(frames, ranges, "the partition frame and the range unbounded both ways")
    window = ctx.table_window(t, 1, 1, TERMS, abi.WIN_ROW_NUMBER, ALL, ALL, n)
    same(window[:4], ctx.table_sorted_by(t, 1, ALL, TERMS, n), "the window's rows and the sorted rows")
    _same(window, c.rows, c.ref.order, (pattern, "the window's rows"))
    assert (window[4] == c.ref.ranks[abi.WIN_ROW_NUMBER]).all() and len(window[0]) == n
