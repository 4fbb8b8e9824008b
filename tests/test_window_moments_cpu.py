"""VAR / STDDEV / COVAR / CORR / REGR over window frames, the part that needs no GPU: the pinned fold of include/sdqh_sort_wmoments.h
restated in Python (window_moments_reference) against exact rationals within the header's bound on the cases the GPU tests run — and
the textbook formula missing that bound —, ResultSet.rolling against the definition, the request's checks and messages, the route on
a stub engine, dist.refuse_window, and the struct's layout against the header.

The cases (sizes, partitions, frames, data) are defined here once; test_window_moments_gpu imports them."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import moments_reference as mref
import window_moments_reference as ref
from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import dist as sdist
from sdqlpy_amd.result import MOMENT_OPS, ResultSet, RollingRequest, WindowRequest, rolling_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
TILE = 512                                   # window_moments_geometry() today; the GPU tests take the device's
OFFSET = float(1 << 30)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def sizes(T):
    return [0, 1, 2, T - 1, T, T + 1, 3 * T + 5]


def large(T):
    return 257 * T + 3


PARTITIONS = ("one", "ones", "tile end", "seam")


def partition_column(kind, n, T):
    """the partition of every sorted position, non-decreasing"""
    pos = np.arange(n, dtype=np.int64)
    if kind == "one":
        return pos * 0
    if kind == "ones":
        return pos
    if kind == "tile end":                   # [0, T / 3), [T / 3, T) — it ends on tile 0's last position —, [T, 2 T + 7), the rest
        return np.searchsorted(np.array([T // 3, T, 2 * T + 7]), pos, side="right").astype(np.int64)
    seam = 256 * T                           # "seam": a partition over the 256-tile seam, one before it and one behind
    return np.searchsorted(np.array([seam - 300, seam + 200]), pos, side="right").astype(np.int64)


def frames(T):
    """(unit, lo, hi) of the frames under test; the order values are consecutive integers and unique keys, so a VALUE or GROUPS frame
    holds the rows of the ROWS frame with the same offsets"""
    return [("rows", -19, 0), ("rows", -2, 2), ("rows", -(T + 7), 3), ("rows", None, 0), ("rows", None, None), ("rows", 2, 5), ("value", -6, 6), ("groups", -3, 1)]


def data(n, seed=0):
    """(y: doubles — quarters beside 2^30 —, x: integers beside 2^30, as doubles) by sorted position"""
    rng = np.random.default_rng(1000 + seed + n)
    return OFFSET + rng.integers(0, 64, n) / 4.0, OFFSET + rng.integers(-8, 8, n).astype(np.float64)


def sample_rows(n, part, T, every=97):
    """the rows checked of a case too large to check row by row: every 97th, and two on either side of every tile, partition and
    256-tile seam"""
    pos = np.arange(n)
    head = np.ones(n, bool)
    head[1:] = part[1:] != part[:-1]
    marks = np.unique(np.concatenate((np.arange(0, n, T), np.nonzero(head)[0], [n])))
    near = (marks[:, None] + np.arange(-2, 3)[None, :]).ravel()
    return np.unique(np.concatenate((pos[::every], near[(near >= 0) & (near < n)])))


def frame_ends(part, lo, hi):
    starts, ends = ref.partition_ends(part)
    return ref.rows_frames(len(part), starts, ends, lo, hi)


# every column of a case: (op, the measures read — "y" the double one, "x" the integer one); all nine ops, each kind of measure under
# the ops of one measure, the double one as Y and the integer one as X under the others
COLUMNS = [(op, "y") for op in ref.UNI] + [(op, "x") for op in ref.UNI] + [(op, "yx") for op in ref.BI]


def restated(tree, rows, l, r):
    """{column: its values by the pinned fold at `rows`} — NaN (the NULL bits) on an empty frame"""
    out = {col: np.empty(len(rows)) for col in COLUMNS}
    seen = {}                                                              # (rows with one frame have one state: the association is l's and r's alone)
    for i, j in enumerate(rows):
        ends = (int(l[j]), int(r[j]))
        if ends not in seen:
            s = tree.query(*ends) if ends[0] <= ends[1] else ref.EMPTY
            sx = (s[0], s[3], s[4], s[1], s[2], s[5])
            seen[ends] = [ref.finish(op, sx if which == "x" else s) for op, which in COLUMNS]
        for col, v in zip(COLUMNS, seen[ends]):
            out[col][i] = v
    return out


def check_bound(ex, cols, rows, l, r, what):
    """every column of `cols` (at `rows`) against exact within the header's bound; an empty frame is NULL by bits.  -> the worst ratio"""
    live = l[rows] <= r[rows]
    worst = 0.0
    for col, got in cols.items():
        assert (mref.bits(got[~live]) == ref.NULL_BITS).all(), (what, col, "empty frames")
    if live.any():
        ends, inv = np.unique(np.stack((l[rows][live], r[rows][live]), 1), axis=0, return_inverse=True)      # every distinct frame once
        f = ex.frames(ends[:, 0], ends[:, 1], abs_c=True).take(inv.ravel())
        fx = f.swapped()
        for (op, which), got in cols.items():
            worst = max(worst, ref.check_column(op, got[live], fx if which == "x" else f, (what, op, which)))
    return worst


CASES = [(n, kind) for n in sizes(TILE) for kind in PARTITIONS[:3]] + [(large(TILE), "seam")]


@pytest.mark.parametrize("n,kind", CASES)
def test_the_restatement_meets_the_bound(n, kind):
    """No row is skipped, past 256 tiles either."""
    T = TILE
    part = partition_column(kind, n, T)
    y, x = data(n)
    ex, tree = ref.Exact(y, x), ref.Tree(y, x)
    rows = np.arange(n)
    worst = 0.0
    for unit, lo, hi in frames(T):
        l, r = frame_ends(part, lo, hi)
        worst = max(worst, check_bound(ex, restated(tree, rows, l, r), rows, l, r, (n, kind, unit, lo, hi)))
    print("PRINTED window moments restated: worst error / bound at n = %d, %s = %.4f" % (n, kind, worst))
    assert worst < 1.0


def test_the_vector_propagation_is_moments_reference_s():
    n = 300
    y, x = data(n, 3)
    l, r = frame_ends(partition_column("tile end", n, 90), -19, 2)
    f = ref.Exact(y, x).frames(l, r, abs_c=True)
    for op in ref.OPS:
        want, bound, null = ref.values(op, f)
        for j in range(0, n, 7):
            w, b = f.exact(j, True).value(op)
            assert (w is None) == bool(null[j])
            if w is not None:
                assert abs(w - want[j]) <= 4 * np.spacing(abs(w)) and abs(b - bound[j]) <= 1e-9 * b, (op, j, w, want[j], b, bound[j])


def test_the_textbook_formula_misses_the_bound():
    """sum x^2 - (sum x)^2 / m in doubles on the 2^30-offset data, frames of 20 rows: were this ever to pass, the bound would be too
    loose to tell a wrong fold from a right one."""
    n = 400
    y, _ = data(n, 1)
    l, r = frame_ends(partition_column("one", n, TILE), -19, 0)
    assert (r - l + 1).max() <= 60
    f = ref.Exact(y).frames(l, r)
    bound = ref._q_bound(f, f.qy, f.ay)
    text = np.array([ref.textbook_q(y[a:b + 1]) for a, b in zip(l, r)])
    tree = ref.Tree(y)
    ours = np.array([tree.query(int(a), int(b))[2] for a, b in zip(l, r)])
    miss = np.abs(text - f.qy) / bound
    print("PRINTED window moments: the textbook formula's worst error / bound = %.3g, the fold's = %.3g" % (miss.max(), (np.abs(ours - f.qy) / bound).max()))
    assert (miss > 1.0).any() and (np.abs(ours - f.qy) <= bound).all()


# ---- the host route ----------------------------------------------------------------------------------------------------------------
def test_resultset_rolling_against_exact():
    """by the definition's two passes: within the two-pass bound of sdqh_sort_moments.h (moments_reference), NULLs by bits"""
    n = 160
    rng = np.random.default_rng(7)
    part = rng.integers(0, 3, n)
    day = rng.integers(0, 25, n)                                           # ties: a VALUE / GROUPS frame holds whole tie runs
    y, x = data(n, 2)
    rows = ResultSet(["p", "d", "y", "x", "i"], [part, day, y, x.astype(np.int64), np.arange(n)])
    aggs = {}
    for k, (unit, lo, hi) in enumerate([("rows", -5, 0), ("rows", 1, 3), ("value", -2, 2), ("groups", None, 0), ("rows", None, None)]):
        for op in MOMENT_OPS:
            aggs["%s_%d" % (op, k)] = (op, "y", lo, hi, unit) if op in ref.UNI else (op, "y", "x", lo, hi, unit)
    got = rows.rolling(["p"], [("d", "asc")], aggs)
    assert got.columns == rows.columns + list(aggs) and all(got.column(c).dtype == np.float64 for c in aggs) and len(got) == n
    order = np.asarray(got.column("i"))
    assert (np.lexsort((np.arange(n), day, part)) == order).all()
    ps, ds, ys, xs = part[order], day[order], y[order], x[order]
    empties = 0
    for k, (unit, lo, hi) in enumerate([("rows", -5, 0), ("rows", 1, 3), ("value", -2, 2), ("groups", None, 0), ("rows", None, None)]):
        for j in range(n):
            same = np.nonzero(ps == ps[j])[0]
            if unit == "rows":
                members = same[(same >= j + (-n if lo is None else lo)) & (same <= j + (n if hi is None else hi))]
            elif unit == "value":
                members = same[(ds[same] >= ds[j] + lo) & (ds[same] <= ds[j] + hi)]
            else:
                members = same[ds[same] <= ds[j]]
            if len(members) == 0:
                empties += 1
                assert all(int(mref.bits(got.column("%s_%d" % (op, k))[j:j + 1])[0]) == ref.NULL_BITS for op in MOMENT_OPS), (k, j)
                continue
            exact = mref.Exact(ys[members], xs[members])
            for op in MOMENT_OPS:
                mref.check(op, got.column("%s_%d" % (op, k))[j], None, None, (k, j, op), exact=exact)
    assert empties > 0
    assert len(ResultSet(["p", "d", "y"], [part[:0], day[:0], y[:0]]).rolling(["p"], ["d"], {"v": ("var_pop", "y", -1, 0)})) == 0


# ---- the request -------------------------------------------------------------------------------------------------------------------
COLS = ["grp", "ord", "val", "oth"]


def test_rolling_request_checks_and_messages():
    req = rolling_request(COLS, ["grp"], [("ord", "desc")], {"v": ("stddev_samp", "val", -19, 0), "b": ("regr_slope", "val", "oth", None, 2, "groups"), "c": ("corr", "val", "oth", -1.5, 1, "value")})
    assert isinstance(req, RollingRequest) and isinstance(req, WindowRequest) and req.method == "rolling" and req.served_by == "rolled"
    assert req.aggs == [("v", "stddev_samp", "val", None, "rows", -19, 0), ("b", "regr_slope", "val", "oth", "groups", None, 2), ("c", "corr", "val", "oth", "value", -1.5, 1)]
    assert req.items == req.aggs and req[0] == ALL and req[1] == [("grp", "asc"), ("ord", "desc")] and req.npartition == 1
    assert req.renamed([("g", "asc"), ("o", "desc")], {"val": "v2", "oth": "o2"}).aggs[1] == ("b", "regr_slope", "v2", "o2", "groups", None, 2)
    ops = ", ".join(MOMENT_OPS)
    units = "value, groups, rows"
    shape = "(op, y, lo, hi[, unit]) or (op, y, x, lo, hi[, unit])"
    bad = [
        (dict(aggs={"v": ("variance", "val", -1, 0)}), ValueError, "rolling: op is one of %s, not 'variance'" % ops),
        (dict(aggs={"v": ("var_pop", "val", "oth", -1, 0, "rows", 1)}), ValueError, "rolling: var_pop takes one column: (op, y, lo, hi[, unit])"),
        (dict(aggs={"v": ("var_pop", "val", -1)}), ValueError, "rolling: var_pop takes one column: (op, y, lo, hi[, unit])"),
        (dict(aggs={"v": ("corr", "val", -1, 0)}), ValueError, "rolling: corr takes two columns: (op, y, x, lo, hi[, unit])"),
        (dict(aggs={"v": ("corr", "val", 3, -1, 0)}), ValueError, "rolling: a measure is a column name"),
        (dict(aggs={"v": ("var_pop", "val", 2, 1)}), ValueError, "rolling: the frame (2, 1) ends before it starts"),
        (dict(aggs={"v": ("var_pop", "val", -1.5, 0)}), ValueError, "rolling: a bound is an integer, not -1.5"),
        (dict(aggs={"v": ("var_pop", "val", "a", 0, "value")}), ValueError, "rolling: a bound is an integer or a finite float, not 'a'"),
        (dict(aggs={"v": ("var_pop", "val", -1, 0, "days")}), ValueError, "rolling: a column's unit is one of %s, not 'days'" % units),
        (dict(aggs={"v": ("var_pop", "val", -1, 0)}, unit="range"), ValueError, "rolling: unit is one of %s, not 'range'" % units),
        (dict(aggs={"v": ("var_pop", "val", -1, 0, "value")}, order=[("ord", "asc"), ("val", "asc")]), ValueError, "rolling: a value frame is ordered by exactly one column, not 2"),
        (dict(aggs={}), ValueError, "rolling: aggs is a non-empty dict {new column: %s}" % shape),
        (dict(aggs={"v": "var_pop"}), ValueError, "rolling: an aggregate is name: %s" % shape),
        (dict(aggs={"v": ("var_pop", "nope", -1, 0)}), KeyError, "rolling: the result has no column 'nope'"),
        (dict(aggs={"v": ("covar_pop", "val", "nope", -1, 0)}), KeyError, "rolling: the result has no column 'nope'"),
        (dict(aggs={"val": ("var_pop", "val", -1, 0)}), KeyError, "rolling: the result already has a column 'val'"),
        (dict(aggs={"v": ("var_pop", "val", -1, 0)}, by=["nope"]), KeyError, "window: the result has no column 'nope'"),
        (dict(aggs={"v": ("var_pop", "val", -1, 0)}, order=[("ord", "up")]), ValueError, "window: directions are 'asc' or 'desc'"),
    ]
    for how, error, message in bad:
        args = dict(by=["grp"], order=[("ord", "desc")], unit="rows")
        args.update(how)
        with pytest.raises(error) as e:
            rolling_request(COLS, args["by"], args["order"], args["aggs"], args["unit"])
        assert e.value.args[0] == message, how
    with pytest.raises(ValueError) as e:
        RollingRequest(ALL, [("grp", "asc")], 1, [("v", "var_pop", "val", "oth", "rows", -1, 0)])
    assert e.value.args[0] == "rolling: bad aggregate"
    late = rolling_request(None, ["grp"], ["ord"], {"v": ("var_pop", "nope", -1, 0)})        # unchecked until the result is known
    with pytest.raises(KeyError) as e:
        ResultSet(COLS, [np.arange(3)] * 4).windowed(late)
    assert e.value.args[0] == "rolling: the result has no column 'nope'"


# ---- the route ---------------------------------------------------------------------------------------------------------------------
K, V = abi.SORT_KEY, abi.SORT_VALUE


class _Recorder:
    """A context whose table_* calls are written down and answered with three rows and one array of doubles per column asked for
    (test_request_routes_cpu's stub, for this request)."""

    def __init__(self):
        self.calls = []
        self.library = SimpleNamespace(has_sort=True, has_sort_terms=True, **{flag: True for flag in abi.WINDOW_EXTENSIONS})

    def __getattr__(self, name):
        if not name.startswith("table_"):
            raise AttributeError(name)

        def call(table, *args, **kwargs):
            self.calls.append((name, args, kwargs))
            return np.arange(1, 4, dtype=np.int64), None, np.array([[10.0, 20.0, 30.0], [3.0, 2.0, 1.0]]), None, [np.array([2.0, 4.0, 6.0]) for _ in args[3]]
        return call


def _run(aggs, **switches):
    ctx = _Recorder()
    eng = SimpleNamespace(ctx=ctx, device_sort=True, order_routes=[], compact_hints={}, lazy_results=False, **switches)
    bt = SimpleNamespace(agg=([("p", "key")], ["x", "k"], None, True, True, 2), shared_groups=False, agg_fields={}, int_values=("x",), table=object(), key_radix=None,
                         key_parts=None, key_decoder=None, decoder_of=lambda field, src: None, payload_dtypes={})
    op = SimpleNamespace(source="groups", out="result", lineno=1, fields=[("grp", 0, "p"), ("ord", 1, "k"), ("val", 1, "x")])
    rs = engine._finalize(eng, op, {"groups": ("aggregated", "bt"), "bt": bt}, rolling_request(["grp", "ord", "val"], ["grp"], [("ord", "desc")], aggs))
    assert len(eng.order_routes) == 1
    return eng.order_routes[0], ctx.calls, rs


def test_route_note_call_and_result():
    aggs = {"vol": ("stddev_samp", "val", -19, 0), "beta": ("regr_slope", "val", "ord", None, 2, "groups"), "c": ("covar_pop", "ord", "val", -1.5, 1, "value")}
    note, calls, rs = _run(aggs)
    listed = [["vol", "stddev_samp", "val", None, "rows", -19, 0], ["beta", "regr_slope", "val", "ord", "groups", None, 2], ["c", "covar_pop", "ord", "val", "value", -1.5, 1]]
    assert note == {"route": "window_moments", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"], "aggs": listed, "calls": 1}
    X, O = (V, 0, True), (V, 1, True)
    terms = [(K, 0, False, False), (V, 1, True, True)]
    assert calls == [("table_window_moments", (1, 1, terms, [(abi.GM_STDDEV_SAMP,) + X + X + (abi.WEX_ROWS, -19, 0), (abi.GM_REGR_SLOPE,) + X + O + (abi.WRANGE_GROUPS, None, 2),
                                                             (abi.GM_COVAR_POP,) + O + X + (abi.WRANGE_VALUE, -1.5, 1.0)], ALL, 4096), {"want_hits": False})]
    assert [(nm, a.dtype.str) for nm, a in zip(rs.columns, rs.arrays)] == [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("vol", "<f8"), ("beta", "<f8"), ("c", "<f8")]
    assert engine._route_of(rolling_request(None, [], ["ord"], aggs)).env == "SDQLPY_AMD_DEVICE_WINDOW_MOMENTS"
    # the routing decision alone: the switch, the library's flag, and more columns than a call takes (the host's, as every window route's)
    req = rolling_request(None, ["grp"], [("ord", "desc")], aggs)
    spec = engine._FrameSpec(terms)
    spec.measures = [[X], [X, O], [O, X]]

    def route(req, spec, switch=True, flag=True):
        lib = SimpleNamespace(has_sort=True, has_sort_terms=True, **{f: True for f in abi.WINDOW_EXTENSIONS})
        lib.has_window_moments = flag
        return engine._order_route(SimpleNamespace(ctx=SimpleNamespace(library=lib), device_sort=True, device_window_moments=switch), req, spec)
    assert route(req, spec) == "window_moments" and route(req, spec, switch=False) == "host" and route(req, spec, flag=False) == "host"
    five = rolling_request(None, ["grp"], [("ord", "desc")], {"v%d" % i: ("var_pop", "val", -i, 0) for i in range(abi.WM_MAX_COLS + 1)})
    wide = engine._FrameSpec(terms)
    wide.measures = [[X]] * (abi.WM_MAX_COLS + 1)
    assert route(five, wide) == "host"
    far = rolling_request(None, ["grp"], [("ord", "desc")], {"v": ("var_pop", "val", -1, 1 << 60)})      # a column ends in `hi`, not in a default: no 2^53 rule
    kept = engine._FrameSpec(terms)
    kept.measures, kept.int_values = [[X]], ("val",)
    assert route(far, kept) == "window_moments"
    text = rolling_request(None, ["grp"], [("ord", "desc")], {"v": ("var_pop", "val", -1, 0)})      # a measure the device cannot read as numbers: spec.measures None
    assert route(text, engine._FrameSpec(terms)) == "host"


def test_the_multi_gpu_runner_refuses_it():
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(rolling_request(None, ["grp"], ["ord"], {"v": ("var_pop", "val", -1, 0)}))
    assert str(e.value) == "rolling runs on one GPU: the multi-GPU runner has no exchange by partition key"


# ---- the binding -------------------------------------------------------------------------------------------------------------------
def test_the_struct_is_the_header_s():
    text = open(os.path.join(ROOT, "include", "sdqh_sort_wmoments.h")).read()
    body = re.search(r"typedef struct sdqh_window_moment \{(.*?)\} sdqh_window_moment;", text, re.S).group(1)
    at, want = 0, []
    for ctype, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        size = 4 if ctype == "int32_t" else 8
        for name in (s.strip() for s in names.split(",")):
            at = (at + size - 1) // size * size
            want.append((name, at, size))
            at += size
    assert [(name, getattr(abi.WindowMoment, name).offset, getattr(abi.WindowMoment, name).size) for name, _ in abi.WindowMoment._fields_] == want
    assert C.sizeof(abi.WindowMoment) == 56 == (at + 7) // 8 * 8 and [n for n, _, _ in want] == ["op", "kind", "index", "is_f64", "kind2", "index2", "is_f64_2", "unit", "flags", "_pad", "lo", "hi"]
    assert re.search(r"#define\s+SDQH_WM_MAX_COLS\s+%d\b" % abi.WM_MAX_COLS, text) and abi.WM_MAX_COLS == 4
    assert abi.WINDOW_EXTENSIONS["has_window_moments"] == (abi.WINDOW_MOMENTS_EXPORTS, "sdqh_sort_wmoments.h", "window moments", "has_window_exclude")
    assert abi.WINDOW_MOMENTS_EXPORTS == ["sdqh_table_window_moments", "sdqh_window_moments_geometry"]
    for s in abi.WINDOW_MOMENTS_EXPORTS:
        assert re.search(r"\bint %s\(" % s, text), s
    assert '#include "sdqh_sort_exclude.h"' in text and '#include "sdqh_sort_moments.h"' in text
    assert "sdqh_sort_wmoments.h" in open(os.path.join(ROOT, "include", "sdqh_sort_moments.h")).read()


def test_a_compile_only_context_refuses_after_the_struct_checks_and_before_the_table_checks(hip_lib):
    """the order of the errors is sdqh_table_window_exclude's: what reads the caller's structs alone is SDQH_ERR_INVALID first, then
    SDQH_ERR_UNSUPPORTED, and what needs the table (a measure it lacks) is never looked at"""
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.window_moments_geometry() == ctx.window_exclude_geometry()[0] == TILE
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context: a key, hits, no payload
        Kk, H, P = abi.SORT_KEY, abi.SORT_HITS, abi.SORT_PAYLOAD
        key, hits = (Kk, 0, False, False), (H, 0, True, False)
        ky, hx, rows, value, groups = (Kk, 0, False), (H, 0, False), abi.WEX_ROWS, abi.WRANGE_VALUE, abi.WRANGE_GROUPS
        good = (abi.GM_VAR_POP,) + ky + ky + (rows, -1, 0)
        unsupported = [
            (1, [key, hits], [good, (abi.GM_CORR,) + ky + hx + (value, -2, 2), (abi.GM_REGR_INTERCEPT,) + hx + ky + (groups, None, None)]),
            (0, [key], [(abi.GM_STDDEV_SAMP,) + ky + (P, 9, True) + (rows, None, 3)]),        # VAR / STDDEV do not read X: unchecked
            (0, [key], [(abi.GM_VAR_POP, P, 3, False) + ky + (rows, -1, 0)]),                 # a measure the table lacks: the table's business, behind the refusal
            (0, [key], [(abi.GM_COVAR_POP,) + ky + (Kk, 0, True) + (rows, -1, 0)]),           # is_f64 on a key: likewise
            (0, [key], [(abi.GM_VAR_POP,) + ky + ky + (rows, 1 << 40, 1 << 41)]),
        ]
        for npart, terms, cols in unsupported:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_moments(table, 0, npart, terms, cols, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED and "compile-only" in str(e.value), (npart, terms, cols)
        invalid = [
            (0, [key], [(-1,) + good[1:]]), (0, [key], [(9,) + good[1:]]), (0, [key], [good, (abi.GM_REGR_INTERCEPT + 1,) + good[1:]]),      # an op outside SDQH_GM_*
            (0, [key], [good[:7] + (3, -1, 0)]), (0, [key], [good[:7] + (-1, -1, 0)]),        # an unknown unit
            (0, [key], [good[:7] + (rows, 1, 0)]), (0, [key], [good[:7] + (groups, 5, 4)]), (0, [(abi.SORT_VALUE, 0, False, True)], [good[:7] + (value, 0.5, 0.25)]),      # lo > hi
            (0, [(abi.SORT_VALUE, 0, False, True)], [good[:7] + (value, float("inf"), None)]),   # a non-finite offset of a double VALUE frame
            (0, [key, hits], [good[:7] + (value, -1, 1)]), (1, [key], [good[:7] + (value, -1, 1)]),      # a VALUE frame wants exactly one ORDER BY term
            (0, [key], []), (0, [key], [good] * 5),                                           # ncols < 1, > SDQH_WM_MAX_COLS
            (0, [], [good]), (0, [key] * 9, [good]), (2, [key], [good]), (-1, [key], [good]),
        ]
        for npart, terms, cols in invalid:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_moments(table, 0, npart, terms, cols, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, (npart, terms, cols)
        # flags and _pad are not the binding's to set wrong: through the struct
        for field, val in (("flags", 4), ("flags", -1), ("_pad", 1)):
            arr = (abi.WindowMoment * 1)()
            arr[0].op, arr[0].unit, arr[0].lo = abi.GM_VAR_POP, rows, -1
            setattr(arr[0], field, val)
            got = C.c_int64(-7)
            rc = ctx.lib.sdqh_table_window_moments(ctx.handle, table.handle, C.c_int64(0), C.c_int(0), C.c_int(1), abi._marshal_sort_terms([key]), C.c_int(1), arr,
                                                   C.c_int64(ALL), C.c_int64(16), None, None, None, None, None, C.byref(got))
            assert (rc, got.value) == (abi.ERR_INVALID, -7), (field, val)
        table.free()
    finally:
        ctx.close()


def test_the_library_exports_the_extension(hip_lib, oracle_lib):
    for s in abi.WINDOW_MOMENTS_EXPORTS:
        assert hasattr(hip_lib.cdll, s) and not hasattr(oracle_lib.cdll, s), s
    assert hip_lib.has_window_moments and hip_lib.has_window_exclude and oracle_lib.has_window_moments is False
