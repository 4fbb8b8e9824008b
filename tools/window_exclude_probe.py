#!/usr/bin/env python3
"""q3 at a given SF finished with values over frames with rows taken out: `excluding(["o_orderdate"], [("revenue", "desc")], aggs,
exclude=...)` — q3 per order date by revenue descending — with one column and with four of three units, against:

    (a) the device route (sdqh_table_window_exclude): wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one
        call — one folded column (the average of the 103 orders on either side, without the row itself), the same column with
        nothing excluded and excluding the group, and four columns: that average (ROWS -103..103 excluding the current row), a VALUE
        +-20000 sum, a GROUPS -3..3 count and a ROWS running maximum, each also with its own exclusion where the call takes one
    (b) in the same run, `ranged` and `sliding` with the same base frames (one column each): what one folded column costs there —
        run them alone on the parent commit with --no-excluding: they launch what they launched
    (c) what a caller did before there was a device route: `order_by` of the same terms (every row copied to the host) followed by
        ResultSet.excluding

    window_exclude_probe.py [SF] [calls] [--no-excluding]     medians of `calls` calls (default 30) after 5 warm-up calls"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

import numpy as np

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
have_excluding = "--no-excluding" not in sys.argv
sf = float(argv[0]) if len(argv) > 0 else 10.0
runs = int(argv[1]) if len(argv) > 1 else 30
sdqlpy_init(3, 1, device=0)
eng = engine.default_engine()


def median_ms(call, warm, runs):
    for _ in range(warm):
        call()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_wsl", "k_wrg", "k_wq", "k_wex", "k_compact", "topk")):
    eng.ctx.set_profiling(True)                                        # (starts an empty log, shared with the lanes)
    call()
    log = list(eng.ctx.kernel_log)
    eng.ctx.set_profiling(False)
    times = {}
    for k, ms in log:
        if any(nm in k for nm in names):
            n, t = times.get(k, (0, 0.0))
            times[k] = (n + 1, t + ms)
    return [(k, n, round(t, 4)) for k, (n, t) in times.items()]


db = tpch.generate(sf, tables=["lineitem", "customer", "orders"], columns=tpch.columns_for(("q3",)))
args = [db[t] for t in Q.QUERY_TABLES["q3"]]
by, order = ["o_orderdate"], [("revenue", "desc")]
ordered = Q.q3.order_by([(b, "asc") for b in by] + order)


def timed(what, leg):
    def call():
        r = leg()
        r.size()                                                        # (the rows are on the host)
        return r
    med, lo, hi = median_ms(call, 5, runs)
    r = call()
    route = [x for x in eng.stats()["order_routes"] if x][-1]
    print("q3 SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, med, runs, lo, hi, r.size(), route["route"]), flush=True)
    print("   ", kernel_times(call), flush=True)
    return r


timed("sliding rows -103..103, 1 sum (b)", lambda: Q.q3.sliding(by, order, {"near": ("sum", "revenue", -103, 103)})(*args))
timed("ranged value +-20000, 1 sum (b)", lambda: Q.q3.ranged(by, order, {"near": ("sum", "revenue", -20000.0, 20000.0)})(*args))
timed("ranged groups -3..3, 1 sum (b)", lambda: Q.q3.ranged(by, order, {"near": ("sum", "revenue", -3, 3)}, unit="groups")(*args))
if have_excluding:
    one = {"others": ("avg", "revenue", -103, 103)}
    four = {"others": ("avg", "revenue", -103, 103), "near": ("sum", "revenue", -20000.0, 20000.0, None, "value"), "peers": ("count", None, -3, 3, None, "groups"),
            "best": ("max", "revenue", None, 0)}
    timed("excluding no others, rows -103..103, 1 avg (a) device", lambda: Q.q3.excluding(by, order, one, exclude="no others")(*args))
    timed("excluding current row, rows -103..103, 1 avg (a) device", lambda: Q.q3.excluding(by, order, one)(*args))
    timed("excluding group, rows -103..103, 1 avg (a) device", lambda: Q.q3.excluding(by, order, one, exclude="group")(*args))
    timed("excluding current row, value +-20000, 1 sum (a) device", lambda: Q.q3.excluding(by, order, {"near": ("sum", "revenue", -20000.0, 20000.0)}, unit="value")(*args))
    timed("excluding ties, groups -3..3, 1 sum (a) device", lambda: Q.q3.excluding(by, order, {"near": ("sum", "revenue", -3, 3)}, exclude="ties", unit="groups")(*args))
    a4 = {}
    for exclude in ("current row", "group", "ties", "no others"):
        a4[exclude] = timed("excluding %s, 4 columns of 3 units (a) device" % exclude, lambda: Q.q3.excluding(by, order, four, exclude=exclude)(*args))
    c1 = timed("excluding current row, 1 avg (c) order_by + ResultSet.excluding", lambda: ordered(*args).excluding(by, order, one))
    c4 = timed("excluding current row, 4 columns (c) order_by + ResultSet.excluding", lambda: ordered(*args).excluding(by, order, four))
    a = a4["current row"]
    # two runs of the query sum the revenues in another order: doubles are compared within 1e-10, as the tests do
    rel = lambda x, y: float(np.nanmax(np.abs(np.asarray(x) - np.asarray(y)) / np.maximum(np.abs(np.asarray(y)), 1e-300))) if len(x) else 0.0      # noqa: E731
    same = {"columns": a.columns == c4.columns, "orders": [x[0] for x in a.ordered_rows()] == [x[0] for x in c4.ordered_rows()],
            "peers": bool((a.column("peers") == c4.column("peers")).all()), "nan": all(bool((np.isnan(a.column(c)) == np.isnan(c4.column(c))).all()) for c in ("others", "near", "best"))}
    print("q3 SF=%g excluding current row, 4 columns: (a) and (c) agree: %s; largest relative difference: revenue %.3g, best %.3g, near %.3g, others %.3g" %
          (sf, same, rel(a.column("revenue"), c4.column("revenue")), rel(a.column("best"), c4.column("best")), rel(a.column("near"), c4.column("near")), rel(a.column("others"), c4.column("others"))), flush=True)
