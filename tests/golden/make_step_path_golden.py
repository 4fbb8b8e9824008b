#!/usr/bin/env python3
"""Golden fixture for the six newer steps behind the sort: what sdqh_table_window_exclude, _grouping_sets, _group_distinct,
_group_moments, _sessions and _window_moments launched and returned at commit 954f75f ("Test window moments on tied, descending, double
orders and wide calls"), the parent of the change that gave their host code one level pass, one frame pass and one tile fold.  Run on
an MI355X AT THAT COMMIT; tests/test_step_paths_gpu.py replays run_cases() on the tree and compares.  The older five families have
make_window_path_golden.py beside this file.

Tables: test_window_gpu._probed_table(ctx, n) for n in (0, 1, S, S + 1, tile + 1, 3 tile + 5) — S the largest n of the
single-workgroup sort, tile the rows per tile of the scans (sort_geometry(), recorded and asserted) — with min_hits in (0, 2): the sizes
at which the single-workgroup sort, the tile scans, the upper tree levels (k_wrg_upper, k_wmo_upper: n > tile), the carries across
tiles and a lower level with more than one tile of groups switch on.

Per call: the return code, *out_n, every kernel launched (the call's profile), a SHA-256 of the first *out_n rows of each returned
array, and for the two level families the level_rows array.  The kernels use no floating-point atomics and every fold runs in a fixed
order, so the digests of doubles reproduce.  main() runs everything twice, tables rebuilt, and refuses to write if any case differs
between the two.

Every family: wrapped calls, a raw count-only call (no output array at all) and a raw call with capacity = count - 1, after which
nothing may be written.  The cases switch every optional launch of the six steps on and off at least once — see run_cases.  A
sessions call takes at most SS_MAX_COLS = 4 columns, so NUMBER, ROW, FIRST, AVG and a SUM are two calls: both k_win_scan / k_win_rank
pairs and the fold run in each.

    python tests/golden/make_step_path_golden.py        # rewrites tests/golden/step_path_kernels.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "step_path_kernels.json")
PARENT = "954f75f"


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(got):
    """{array name: SHA-256} of a wrapper's (keys, payload, values, hits, columns[, level_rows]) — columns None or a list of arrays."""
    out = {}
    for name, a in zip(("keys", "payload", "values", "hits"), got[:4]):
        if a is not None:
            out[name] = _sha(a)
    for i, a in enumerate(got[4] or []):
        out["col%d" % i] = _sha(a)
    return out


def write_golden(result, path=OUT):
    """run_cases()' result on disk.  Many calls launch the same kernels and return the same arrays (the rows of one table, the empty
    array), so the file holds each distinct kernel sequence and each distinct digest once — "kernels", "sha" — and a call as [rc, n,
    index of its kernels, {array: index of its digest}] with its level_rows behind them; one call per line.  load_golden() undoes it."""
    calls = result["calls"]
    kernels = sorted({c["kernels"] for c in calls.values()})
    sha = sorted({h for c in calls.values() for h in c["sha"].values()})
    ki, si = {k: i for i, k in enumerate(kernels)}, {h: i for i, h in enumerate(sha)}
    line = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as fh:
        fh.write('{"commit":%s,"geometry":%s,\n"kernels":[\n%s],\n' % (line(result["commit"]), line(result["geometry"]), ",\n".join(line(k) for k in kernels)))
        fh.write('"sha":[\n%s],\n"calls":{\n' % ",\n".join(",".join(line(h) for h in sha[i:i + 4]) for i in range(0, len(sha), 4)))
        rows = []
        for case in sorted(calls):
            c = calls[case]
            rows.append("%s:%s" % (line(case), line([c["rc"], c["n"], ki[c["kernels"]], {a: si[h] for a, h in c["sha"].items()}] + ([c["level_rows"]] if "level_rows" in c else []))))
        fh.write(",\n".join(rows) + "}}\n")


def load_golden(path=OUT):
    """What write_golden() wrote, in run_cases()' form (and "commit")."""
    with open(path) as fh:
        packed = json.load(fh)
    calls = {}
    for case, (rc, n, k, sha, *level_rows) in packed["calls"].items():
        calls[case] = {"rc": rc, "n": n, "kernels": packed["kernels"][k], "sha": {a: packed["sha"][i] for a, i in sha.items()}}
        if level_rows:
            calls[case]["level_rows"] = level_rows[0]
    return {"commit": packed["commit"], "geometry": packed["geometry"], "calls": calls}


def _exclude_structs(abi, cols):
    arr = (abi.WindowExclude * len(cols))()
    for a, (op, kind, index, is_f64, unit, lo, hi, empty, exclude) in zip(arr, cols):
        a.op, a.kind, a.index, a.is_f64, a.unit, a.exclude = op, kind, index, int(is_f64), unit, exclude
        a.flags = (abi.WRANGE_LO_UNBOUNDED if lo is None else 0) | (abi.WRANGE_HI_UNBOUNDED if hi is None else 0)
        a.lo, a.hi, a.empty = abi._range_offset(lo), abi._range_offset(hi), empty
    return arr


def _wmoment_structs(abi, cols):
    arr = (abi.WindowMoment * len(cols))()
    for a, (op, kind, index, is_f64, kind2, index2, is_f64_2, unit, lo, hi) in zip(arr, cols):
        a.op, a.kind, a.index, a.is_f64, a.kind2, a.index2, a.is_f64_2, a.unit = op, kind, index, int(is_f64), kind2, index2, int(is_f64_2), unit
        a.flags = (abi.WRANGE_LO_UNBOUNDED if lo is None else 0) | (abi.WRANGE_HI_UNBOUNDED if hi is None else 0)
        a.lo, a.hi = abi._range_offset(lo), abi._range_offset(hi)
    return arr


def _group_structs(abi, aggs):
    arr = (abi.GroupAgg * max(1, len(aggs)))()
    for a, (op, kind, index, is_f64) in zip(arr, aggs):
        a.op, a.kind, a.index, a.is_f64 = op, kind, index, int(is_f64)
    return arr


def run_cases(ctx, abi, probed_table):
    """{"geometry": [S, tile], "calls": {case: {"rc", "n", "kernels", "sha"[, "level_rows"]}}} of every call of the module's docstring on `ctx`."""
    ALL = abi.SORT_ALL
    K, P, V, H = abi.SORT_KEY, abi.SORT_PAYLOAD, abi.SORT_VALUE, abi.SORT_HITS
    SUM, COUNT, MIN, MAX, AVG = abi.WAGG_SUM, abi.WAGG_COUNT, abi.WAGG_MIN, abi.WAGG_MAX, abi.WEX_AVG
    FIRST, LAST = abi.WSLIDE_FIRST, abi.WSLIDE_LAST
    VALUE, GROUPS, ROWS = abi.WRANGE_VALUE, abi.WRANGE_GROUPS, abi.WEX_ROWS
    NONE, CURRENT, GROUP, TIES = abi.WEX_NO_OTHERS, abi.WEX_CURRENT_ROW, abi.WEX_GROUP, abi.WEX_TIES
    TERMS = [(P, 0, False, False), (V, 0, True, True), (H, 0, False, False)]
    PAY_F, PAY_I, VAL, KEY = (P, 1, True), (P, 0, False), (V, 0, True), (K, 0, False)      # the double payload, the integer payload, value 0 (a double), the key
    NO2 = (K, 0, False)                                                     # the second measure of an op that reads one
    FAR = 10 ** 12                                                          # a ROWS offset beyond every n: the clamp
    S, tile, _ = ctx.sort_geometry()
    calls = {}

    def record(case, rc, n, sha, level_rows=None):
        assert case not in calls, case
        calls[case] = {"rc": int(rc), "n": int(n), "kernels": " ".join(nm for nm, _ in ctx.profile()), "sha": sha}
        if level_rows is not None:
            calls[case]["level_rows"] = [int(x) for x in level_rows]

    def wrapped(case, call):
        got = call()
        record(case, abi.OK, len(got[0]), _digests(got), got[5] if len(got) > 5 else None)

    def raw(case, t, name, lead, cap, ncols, level_rows=False, want_level_rows=True):
        """The raw C call sdqh_<name>: cap None — no array at all, the count-only call —, else a keys array and an ncols x cap columns
        array, both filled with -7; a level family takes its level_rows array (or None) behind the columns.  -> *out_n."""
        keys = None if cap is None else np.full(max(cap, 1), -7, np.int64)
        out = None if cap is None or not ncols else np.full((ncols, max(cap, 1)), -7, np.int64)
        lrows = np.full(abi.SORT_MAX_KEYS + 1, -7, np.int64) if level_rows and want_level_rows else None
        got = C.c_int64(-7)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        trail = (ptr(lrows),) if level_rows else ()
        rc = getattr(ctx.lib, "sdqh_" + name)(ctx.handle, t.handle, *lead, C.c_int64(cap or 0), ptr(keys), None, None, None, ptr(out), *trail, C.byref(got))
        sha = {}
        if rc == abi.OK:
            m = max(0, min(got.value, cap or 0))
            if keys is not None:
                sha["keys"] = _sha(keys[:m])
            if out is not None:
                sha.update({"col%d" % i: _sha(out[i, :m]) for i in range(ncols)})
        else:                                                              # nothing may have been written
            assert keys is None or (keys == -7).all(), case
            assert out is None or (out == -7).all(), case
        record(case, rc, got.value, sha, lrows)
        return got.value

    def three(at, family, t, name, lead, ncols, level_rows=False):
        """The two raw calls every family gets — count-only, capacity = count - 1 — and, for a level family, the full raw call without level_rows."""
        m = raw(at + family + " count only", t, name, lead, None, ncols, level_rows)
        raw(at + family + " capacity below the count", t, name, lead, max(0, m - 1), ncols, level_rows)      # (nothing selected: capacity 0 holds the 0 rows)
        if level_rows:
            raw(at + family + " no level_rows", t, name, lead, max(m, 1), ncols, level_rows, want_level_rows=False)

    for n in (0, 1, S, S + 1, tile + 1, 3 * tile + 5):
        t = probed_table(ctx, n)
        try:
            for mh in (0, 2):
                at = "n=%d min_hits=%d " % (n, mh)
                cap = n + 8                                                # (every row fits: no wrapper repeats its call)
                gcap = 4 * n + 8                                           # ... and every group of at most four levels
                mt = abi._marshal_sort_terms
                head = lambda terms, npart=1: (C.c_int64(mh), C.c_int(npart), C.c_int(len(terms)), mt(terms))
                ghead = lambda terms: (C.c_int64(mh), C.c_int(len(terms)), mt(terms))

                # exclude: ties (k_wq_ties / k_wex_ties) on and off, the dense rank on and off, VALUE / ROWS beyond n, folded / raw / COUNT alone
                ex = {"value sum, nothing excluded": (TERMS[:2], [(SUM,) + PAY_F + (VALUE, -2.0, 2.0, 0, NONE)]),
                      "groups avg exclude group, rows first exclude ties": (TERMS, [(AVG,) + PAY_F + (GROUPS, -1, 1, 0, GROUP), (FIRST,) + PAY_I + (ROWS, -FAR, FAR, -1, TIES)]),
                      "rows count alone, current row": (TERMS, [(COUNT,) + PAY_I + (ROWS, -FAR, 1, 0, CURRENT)]),
                      "value last exclude ties, value sum": (TERMS[:2], [(LAST,) + PAY_F + (VALUE, -2.0, None, 0, TIES), (SUM,) + PAY_I + (VALUE, None, 2.0, 0, NONE)]),
                      "groups count, rows min": (TERMS, [(COUNT,) + PAY_I + (GROUPS, -1, 1, 0, NONE), (MIN,) + PAY_I + (ROWS, -2, 2, 0, NONE)])}
                for nm, (terms, cols) in ex.items():
                    wrapped(at + "exclude " + nm, lambda: ctx.table_window_exclude(t, mh, 1, terms, cols, ALL, cap))
                terms, cols = ex["groups avg exclude group, rows first exclude ties"]
                three(at, "exclude", t, "table_window_exclude", head(terms) + (C.c_int(len(cols)), _exclude_structs(abi, cols), C.c_int64(ALL)), len(cols))

                # window moments: the three units, one measure / a distinct pair (k_wmo_upper twice) / a measure with itself
                wm = {"rows var": (TERMS, [(abi.GM_VAR_SAMP,) + PAY_F + NO2 + (ROWS, -3, 3)]),
                      "value corr of a pair, groups covar of a measure with itself": (TERMS[:2], [(abi.GM_CORR,) + PAY_F + PAY_I + (VALUE, -2.0, 2.0),
                                                                                                   (abi.GM_COVAR_POP,) + PAY_F + PAY_F + (GROUPS, -1, 1)]),
                      "groups regr, rows stddev beyond n": (TERMS, [(abi.GM_REGR_SLOPE,) + PAY_I + VAL + (GROUPS, -2, 0), (abi.GM_STDDEV_POP,) + VAL + NO2 + (ROWS, -FAR, FAR)])}
                for nm, (terms, cols) in wm.items():
                    wrapped(at + "window_moments " + nm, lambda: ctx.table_window_moments(t, mh, 1, terms, cols, ALL, cap))
                terms, cols = wm["value corr of a pair, groups covar of a measure with itself"]
                three(at, "window_moments", t, "table_window_moments", head(terms) + (C.c_int(len(cols)), _wmoment_structs(abi, cols), C.c_int64(ALL)), len(cols))

                # grouping sets: one level / ROLLUP / a mask below the top level; an AVG (k_gs_avg) and none; no aggregate; level_rows given and null
                gs = {"one level, sum": (1 << 3, [(SUM,) + PAY_F]),
                      "rollup, avg count min": (0b1111, [(AVG,) + PAY_F, (COUNT,) + PAY_I, (MIN,) + PAY_I]),
                      "levels 0 and 1, max": (0b0011, [(MAX,) + PAY_F]),
                      "levels 1 and 3, rows only": (0b1010, [])}
                for nm, (levels, aggs) in gs.items():
                    wrapped(at + "grouping_sets " + nm, lambda: ctx.table_grouping_sets(t, mh, TERMS, levels, aggs, ALL, gcap))
                levels, aggs = gs["rollup, avg count min"]
                three(at, "grouping_sets", t, "table_grouping_sets", ghead(TERMS) + (C.c_uint32(levels), C.c_int(len(aggs)), _group_structs(abi, aggs), C.c_int64(ALL)),
                      len(aggs), level_rows=True)

                # group distinct: ngroup 0 and 1; COUNT_DISTINCT with MODE, SUM / AVG_DISTINCT; rows only
                gd = {"ngroup=1 count_distinct, mode, mode_count, count": (TERMS[:2], 1, [(abi.GD_COUNT_DISTINCT,) + VAL, (abi.GD_MODE,) + VAL, (abi.GD_MODE_COUNT,) + VAL,
                                                                                           (abi.GD_COUNT,) + VAL], True),
                      "ngroup=0 sum_distinct, avg_distinct": (TERMS[:1], 0, [(abi.GD_SUM_DISTINCT,) + PAY_I, (abi.GD_AVG_DISTINCT,) + PAY_I], True),
                      "ngroup=1 sum_distinct, rows only": (TERMS[:2], 1, [(abi.GD_SUM_DISTINCT,) + VAL], False)}
                for nm, (terms, ngroup, aggs, want) in gd.items():
                    wrapped(at + "group_distinct " + nm, lambda: ctx.table_group_distinct(t, mh, terms, ngroup, aggs, ALL, gcap, want_aggs=want))
                terms, ngroup, aggs, _ = gd["ngroup=1 count_distinct, mode, mode_count, count"]
                three(at, "group_distinct", t, "table_group_distinct", ghead(terms) + (C.c_int(ngroup), C.c_int(len(aggs)), _group_structs(abi, aggs), C.c_int64(ALL)), len(aggs))

                # group moments: one VAR; CORR with REGR on two measures; GM_MAX_AGGS aggregates whose pass 2 folds seven centred columns
                # (more than SDQH_WAGG_MAX_AGGS = 4: the fold loops twice); a ROLLUP mask
                assert abi.GM_MAX_AGGS == 4 and abi.WAGG_MAX_AGGS == 4
                gm = {"one level, one var": (1 << 3, [(abi.GM_VAR_POP,) + PAY_F]),
                      "rollup, corr and regr": (0b1111, [(abi.GM_CORR,) + PAY_F + PAY_I, (abi.GM_REGR_INTERCEPT,) + PAY_F + PAY_I]),
                      "levels 0 and 2, four aggregates over seven products": (0b0101, [(abi.GM_CORR,) + PAY_F + PAY_I, (abi.GM_CORR,) + PAY_F + VAL, (abi.GM_CORR,) + PAY_I + VAL,
                                                                                      (abi.GM_STDDEV_SAMP,) + KEY])}
                for nm, (levels, aggs) in gm.items():
                    wrapped(at + "group_moments " + nm, lambda: ctx.table_group_moments(t, mh, TERMS, levels, aggs, ALL, gcap))
                levels, aggs = gm["rollup, corr and regr"]
                three(at, "group_moments", t, "table_group_moments", ghead(TERMS) + (C.c_uint32(levels), C.c_int(len(aggs)), abi._marshal_moment_aggs(aggs), C.c_int64(ALL)),
                      len(aggs), level_rows=True)

                # sessions: the GAP and the CHANGE rule; per row with both rank pairs and the fold, with a COUNT alone, with no column;
                # per session with and without columns
                GAP, CHANGE = (abi.SS_GAP, 50.0), (abi.SS_CHANGE, P, 0, False)
                ss = {"gap, per row: number row first avg": (GAP, False, [(abi.SS_NUMBER,) + KEY, (abi.SS_ROW,) + KEY, (abi.SS_FIRST,) + PAY_I, (abi.SS_AVG,) + PAY_F]),
                      "change, per row: sum last max number": (CHANGE, False, [(abi.SS_SUM,) + PAY_F, (abi.SS_LAST,) + PAY_I, (abi.SS_MAX,) + PAY_I, (abi.SS_NUMBER,) + KEY]),
                      "gap, per row: count alone": (GAP, False, [(abi.SS_COUNT,) + KEY]),
                      "change, per row: no column": (CHANGE, False, []),
                      "gap, per session: sum number avg first": (GAP, True, [(abi.SS_SUM,) + PAY_I, (abi.SS_NUMBER,) + KEY, (abi.SS_AVG,) + PAY_F, (abi.SS_FIRST,) + PAY_F]),
                      "change, per session: count alone": (CHANGE, True, [(abi.SS_COUNT,) + KEY]),
                      "gap, per session: no column": (GAP, True, [])}
                for nm, (rule, per, cols) in ss.items():
                    wrapped(at + "sessions " + nm, lambda: ctx.table_sessions(t, mh, 1, TERMS, rule, cols, ALL, cap, per_session=per))
                for key, fam in (("gap, per row: number row first avg", "sessions per row"), ("gap, per session: sum number avg first", "sessions per session")):
                    rule, per, cols = ss[key]
                    lead = head(TERMS) + (C.byref(abi._marshal_session_rule(rule)), C.c_int(int(per)), C.c_int(len(cols)), abi._marshal_session_cols(cols), C.c_int64(ALL))
                    three(at, fam, t, "table_sessions", lead, len(cols))
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
    write_golden(first)
    assert load_golden() == first
    print("%s: %d calls" % (OUT, len(first["calls"])))


if __name__ == "__main__":
    main()
