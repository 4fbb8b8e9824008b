#!/usr/bin/env python3
"""Golden fixture for the step behind the sort: what the five window entry points launched and returned at commit fda5743 ("Add
NTILE, PERCENT_RANK, CUME_DIST, NTH_VALUE and percentiles per group"), the parent of the change that gave them one step type and one
partition pass.  Run on an MI355X AT THAT COMMIT; tests/test_window_gpu.py (test_window_paths_launch_what_they_launched) replays
run_cases() on the tree and compares.

Tables: test_window_gpu._probed_table(ctx, n) for n in (0, 1, S, S + 1, tile + 1, 3 tile + 5) — S the largest n of the
single-workgroup sort, tile the rows per tile of the scans (sort_geometry(), recorded and asserted) — with min_hits in (0, 2): the sizes
at which the single-workgroup sort, the tile scans, k_wrg_upper (n > tile) and the carries across tiles switch on.  PARTITION BY payload
0 ORDER BY value desc, hits asc (the VALUE / GROUP frames: value desc alone, a VALUE frame takes one ORDER BY term).

Per call: the return code, *out_n, every kernel launched (the call's profile), a SHA-256 of the first *out_n rows of each returned
array.  The digests are reproducible: every measure of that table is an integer or a multiple of 0.25 of small magnitude, so every
partial sum is exact in a double in any order, and the window kernels use no floating-point atomics.  main() runs everything twice,
tables rebuilt, and refuses to write if any case differs between the two.

    python tests/golden/make_window_path_golden.py        # rewrites tests/golden/window_path_kernels.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "window_path_kernels.json")
PARENT = "fda5743"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(got):
    """{array name: SHA-256} of a wrapper's (keys, payload, values, hits, extra) — extra None, one array or a list of them."""
    out = {}
    for name, a in zip(("keys", "payload", "values", "hits"), got[:4]):
        if a is not None:
            out[name] = _sha(a)
    extra = got[4]
    if isinstance(extra, list):
        for i, a in enumerate(extra):
            out["col%d" % i] = _sha(a)
    elif extra is not None:
        out["rank"] = _sha(extra)
    return out


def _structs(abi, family, cols):
    """The family's argument array, filled as abi.Context's wrapper fills it (for the raw calls)."""
    if family == "agg":
        arr = (abi.WindowAgg * len(cols))()
        for a, (op, frame, kind, index, is_f64) in zip(arr, cols):
            a.op, a.frame, a.kind, a.index, a.is_f64 = op, frame, kind, index, int(is_f64)
    elif family == "slide":
        arr = (abi.WindowSlide * len(cols))()
        for a, (op, kind, index, is_f64, lo, hi, empty) in zip(arr, cols):
            a.op, a.kind, a.index, a.is_f64, a.lo, a.hi, a.empty = op, kind, index, int(is_f64), lo, hi, empty
    elif family == "range":
        arr = (abi.WindowRange * len(cols))()
        for a, (op, kind, index, is_f64, unit, lo, hi, empty) in zip(arr, cols):
            a.op, a.kind, a.index, a.is_f64, a.unit, a.flags = op, kind, index, int(is_f64), unit, 0
            a.lo, a.hi, a.empty = abi._range_offset(lo), abi._range_offset(hi), empty
    else:
        arr = (abi.WindowQuantile * len(cols))()
        for a, (fn, kind, index, is_f64, arg, p, empty) in zip(arr, cols):
            a.fn, a.kind, a.index, a.is_f64, a.arg, a.p, a.empty = fn, kind, index, int(is_f64), arg, p, empty
    return arr


def run_cases(ctx, abi, probed_table):
    """{"geometry": [S, tile], "calls": {case: {"rc", "n", "kernels", "sha"}}} of every call of the module's docstring on `ctx`."""
    ALL = abi.SORT_ALL
    K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
    SUM, COUNT, MIN = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN
    FIRST, LAST = abi.WSLIDE_FIRST, abi.WSLIDE_LAST
    UP, UF = abi.SLIDE_UNBOUNDED_PRECEDING, abi.SLIDE_UNBOUNDED_FOLLOWING
    VALUE, GROUPS = abi.WRANGE_VALUE, abi.WRANGE_GROUPS
    TERMS = [(P, 0, False, False), (V, 0, True, True), (H, 0, False, False)]
    PAY_F, PAY_I, VAL = (P, 1, True), (P, 0, False), (V, 0, True)          # the double payload, the integer payload, value 0 (a double)
    S, tile, _ = ctx.sort_geometry()
    calls = {}

    def record(case, rc, n, sha):
        assert case not in calls, case
        calls[case] = {"rc": int(rc), "n": int(n), "kernels": " ".join(nm for nm, _ in ctx.profile()), "sha": sha}

    def wrapped(case, call):
        got = call()
        record(case, abi.OK, len(got[0]), _digests(got))

    def raw(case, t, name, lead, cap, last):
        """The raw C call over a keys array of max(cap, 1) rows filled with -7 (cap None: no array at all — the count-only call), and
        `last` (the rank / columns pointer the entry point takes after the four row arrays, or None) -> *out_n."""
        keys = None if cap is None else np.full(max(cap, 1), -7, np.int64)
        got = C.c_int64(-7)
        rc = getattr(ctx.lib, "sdqh_" + name)(ctx.handle, t.handle, *lead, C.c_int64(cap or 0), None if keys is None else keys.ctypes.data_as(C.c_void_p), None, None, None,
                                              last, C.byref(got))
        record(case, rc, got.value, {} if keys is None else {"keys": _sha(keys[:max(0, min(got.value, cap))] if rc == abi.OK else keys)})
        return got.value

    for n in (0, 1, S, S + 1, tile + 1, 3 * tile + 5):
        t = probed_table(ctx, n)
        try:
            for mh in (0, 2):
                at = "n=%d min_hits=%d " % (n, mh)
                cap = n + 8                                                # (every row fits: no wrapper repeats its call)
                head = lambda terms: (C.c_int64(mh), C.c_int(1), C.c_int(len(terms)), abi._marshal_sort_terms(terms))
                # ranks
                for kind, nm in ((abi.WIN_ROW_NUMBER, "row_number"), (abi.WIN_RANK, "rank"), (abi.WIN_DENSE_RANK, "dense_rank")):
                    wrapped(at + "window " + nm, lambda: ctx.table_window(t, mh, 1, TERMS, kind, ALL, ALL, cap))
                wrapped(at + "window rank per_limit=2", lambda: ctx.table_window(t, mh, 1, TERMS, abi.WIN_RANK, 2, ALL, cap))
                wrapped(at + "window row_number no rank column", lambda: ctx.table_window(t, mh, 1, TERMS, abi.WIN_ROW_NUMBER, ALL, ALL, cap, want_rank=False))
                for pl, nm in ((ALL, "every row"), (2, "per_limit=2")):
                    lead = head(TERMS) + (C.c_int(abi.WIN_RANK), C.c_int64(pl), C.c_int64(ALL))
                    m = raw(at + "window count only, " + nm, t, "table_window", lead, None, None)
                    raw(at + "window capacity below the count, " + nm, t, "table_window", lead, max(0, m - 1), None)
                # the four families with columns: (name, terms, {case: columns}, the columns of the two raw calls)
                families = (
                    ("agg", TERMS, {"rows only": [(SUM, abi.FRAME_ROWS) + PAY_F, (COUNT, abi.FRAME_ROWS) + PAY_I],
                                    "rows, range, partition": [(SUM, abi.FRAME_ROWS) + PAY_F, (MIN, abi.FRAME_RANGE) + PAY_I, (SUM, abi.FRAME_PARTITION) + PAY_F,
                                                               (MIN, abi.FRAME_ROWS) + PAY_I]}),
                    ("slide", TERMS, {"sum(-2, 0), last(unbounded)": [(SUM,) + PAY_F + (-2, 0, 0), (LAST,) + PAY_F + (UP, UF, 0)],
                                      "first, count": [(FIRST,) + PAY_I + (-1, 1, -1), (COUNT,) + PAY_I + (-2, 0, 0)]}),
                    ("range", TERMS[:2], {"value sum(-2.0, 2.0)": [(SUM,) + PAY_F + (VALUE, -2.0, 2.0, 0)],
                                          "groups count(-1, 1), value sum": [(COUNT,) + PAY_I + (GROUPS, -1, 1, 0), (SUM,) + PAY_F + (VALUE, -2.0, 2.0, 0)],
                                          "first, count": [(FIRST,) + PAY_I + (VALUE, -2.0, 2.0, -1), (COUNT,) + PAY_I + (GROUPS, -1, 1, 0)]}),
                )
                for family, terms, sets in families:
                    name = "table_window_" + family
                    for nm, cols in sets.items():
                        wrapped(at + family + " " + nm, lambda: getattr(ctx, name)(t, mh, 1, terms, cols, ALL, cap))
                    cols = next(iter(sets.values()))
                    lead = head(terms) + (C.c_int(len(cols)), _structs(abi, family, cols), C.c_int64(ALL))
                    m = raw(at + family + " count only", t, name, lead, None, None)
                    out = np.full((len(cols), max(m, 1)), -7, np.int64)
                    raw(at + family + " capacity below the count", t, name, lead, max(0, m - 1), out.ctypes.data_as(C.c_void_p))
                    assert (out == -7).all() or m == 0, (at, family)
                # functions of the partition's size
                q = lambda fn, measure=(K, 0, False), arg=0, p=0.0: (fn,) + measure + (arg, p, 0)
                quants = {"cont, ntile": [q(abi.WQ_PERCENTILE_CONT, VAL, p=0.5), q(abi.WQ_NTILE, arg=4)], "cume_dist, ntile": [q(abi.WQ_CUME_DIST), q(abi.WQ_NTILE, arg=4)],
                          "percent_rank": [q(abi.WQ_PERCENT_RANK)], "disc per_limit=1": [q(abi.WQ_PERCENTILE_DISC, VAL, p=0.9)]}
                for nm, cols in quants.items():
                    wrapped(at + "quantile " + nm, lambda: ctx.table_window_quantile(t, mh, 1, TERMS, cols, 1 if "per_limit=1" in nm else ALL, ALL, cap))
                wrapped(at + "quantile rows only per_limit=1", lambda: ctx.table_window_quantile(t, mh, 1, TERMS, [q(abi.WQ_NTILE, arg=4)], 1, ALL, cap, want_cols=False))
                cols = quants["cont, ntile"]
                for pl, nm in ((ALL, "every row"), (1, "per_limit=1")):
                    lead = head(TERMS) + (C.c_int(len(cols)), _structs(abi, "quantile", cols), C.c_int64(pl), C.c_int64(ALL))
                    m = raw(at + "quantile count only, " + nm, t, "table_window_quantile", lead, None, None)
                    out = np.full((len(cols), max(m, 1)), -7, np.int64)
                    raw(at + "quantile capacity below the count, " + nm, t, "table_window_quantile", lead, max(0, m - 1), out.ctypes.data_as(C.c_void_p))
                    assert (out == -7).all() or m == 0, (at, "quantile")
        finally:
            t.free()
    return {"geometry": [S, tile], "calls": calls}


def main():
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
    from sdqlpy_amd import abi, engine
    from test_window_gpu import _probed_table
    ctx = engine.load_hip_library().context(device=0)
    ctx.set_profiling(1)
    try:
        first, second = run_cases(ctx, abi, _probed_table), run_cases(ctx, abi, _probed_table)
    finally:
        ctx.set_profiling(0)
        ctx.close()
    differ = [case for case in first["calls"] if first["calls"][case] != second["calls"][case]]
    if differ or first["geometry"] != second["geometry"]:
        sys.exit("not written: %d cases differ between two runs on the same commit: %s" % (len(differ), differ[:8]))
    first["commit"] = PARENT
    with open(OUT, "w") as fh:
        json.dump(first, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %d calls" % (OUT, len(first["calls"])))


if __name__ == "__main__":
    main()
