#!/usr/bin/env python3
"""q3 at a given SF finished with aggregates over window frames: `over(["o_orderdate"], [("revenue", "desc")], aggs)` with one
aggregate (a running sum, RANGE) and with four (running sum, the day's total, the day's size, a running maximum), three ways:

    (a) the device route (sdqh_table_window_agg): wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call
    (b) `numbered` of the same terms — the nearest route there was before: the same selection and order, the rank passes where (a)
        has its scans
    (c) what a caller did before there was a device route: `order_by` of the same terms (every row copied to the host) followed by
        the numpy folds of ResultSet.over on the ordered rows

    window_agg_probe.py SF [runs]          medians of `runs` calls (default 30) after 5 warm-up calls"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

sf = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 30
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_compact", "topk")):
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
one = {"running": ("sum", "revenue")}
four = {"running": ("sum", "revenue"), "day_total": ("sum", "revenue", "partition"), "n": ("count", None, "partition"), "best": ("max", "revenue", "rows")}
legs = [
    ("over, 1 aggregate (a) device", lambda: Q.q3.over(by, order, one)(*args)),
    ("over, 4 aggregates (a) device", lambda: Q.q3.over(by, order, four)(*args)),
    ("numbered (b) rank passes", lambda: Q.q3.numbered(by, order)(*args)),
    ("over, 1 aggregate (c) order_by + numpy", lambda: ordered(*args).over(by, order, one)),
    ("over, 4 aggregates (c) order_by + numpy", lambda: ordered(*args).over(by, order, four)),
]
for what, leg in legs:
    def call(leg=leg):
        r = leg()
        r.size()                                                        # (the rows are on the host)
        return r
    med, lo, hi = median_ms(call, 5, runs)
    r = call()
    route = [x for x in eng.stats()["order_routes"] if x][-1]
    print("q3 SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, med, runs, lo, hi, r.size(), route["route"]), flush=True)
    print("   ", kernel_times(call), flush=True)
a, c = legs[1][1](), legs[4][1]()
same = a.columns == c.columns and [x[0] for x in a.ordered_rows()] == [x[0] for x in c.ordered_rows()] and (a.column("n") == c.column("n")).all()
print("q3 SF=%g over, 4 aggregates: (a) and (c) give the same orders in the same sequence and the same counts: %s" % (sf, same), flush=True)
