#!/usr/bin/env python3
"""q3 at a given SF finished with values over VALUE and GROUP frames: `ranged(["o_orderdate"], [("revenue", "desc")], aggs)` with one
range (the sum of the revenues within `span` of the row's) and with four (that sum, the frame's row count, its maximum, the revenue
of its first row), against:

    (a) the device route (sdqh_table_window_range): wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call,
        the same with unit "groups" (the row's tie run and the three runs on either side)
    (b) `sliding` with positional frames of the same average width on the same result (the frame's width is read off (a)'s count
        column), one slide and four — and `sliding` with one 3-row moving sum and `over` with one ROWS sum, the siblings' own
        probes (they launch what they launched before this route existed: run them on both commits with --no-ranged)
    (c) what a caller did before there was a device route: `order_by` of the same terms (every row copied to the host) followed by
        ResultSet.ranged

    window_range_probe.py SF [runs] [span] [--no-ranged]     medians of `runs` calls (default 30) after 5 warm-up calls"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

import numpy as np

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
have_ranged = "--no-ranged" not in sys.argv
sf = float(argv[0]) if len(argv) > 0 else 10.0
runs = int(argv[1]) if len(argv) > 1 else 30
span = float(argv[2]) if len(argv) > 2 else 20000.0
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_wsl", "k_wrg", "k_compact", "topk")):
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


timed("over, 1 ROWS sum: the forward scan", lambda: Q.q3.over(by, order, {"running": ("sum", "revenue", "rows")})(*args))
timed("sliding, 1 moving sum of 3 rows", lambda: Q.q3.sliding(by, order, {"ma3": ("sum", "revenue", -2, 0)})(*args))
if have_ranged:
    def frames(lo, hi):
        one = {"near": ("sum", "revenue", lo, hi)}
        return one, dict(one, n=("count", None, lo, hi), best=("max", "revenue", lo, hi), first=("first", "revenue", lo, hi))
    one, four = frames(-span, span)
    a1 = timed("ranged value +-%g, 1 range (a) device" % span, lambda: Q.q3.ranged(by, order, one)(*args))
    a4 = timed("ranged value +-%g, 4 ranges (a) device" % span, lambda: Q.q3.ranged(by, order, four)(*args))
    width = np.asarray(a4.column("n"))
    print("q3 SF=%g the value frames hold %.1f rows on average (min %d, max %d)" % (sf, width.mean(), width.min(), width.max()), flush=True)
    g1, g4 = frames(-3, 3)
    timed("ranged groups -3..3, 1 range (a) device", lambda: Q.q3.ranged(by, order, g1, unit="groups")(*args))
    timed("ranged groups -3..3, 4 ranges (a) device", lambda: Q.q3.ranged(by, order, g4, unit="groups")(*args))
    half = max(0, int(round((width.mean() - 1) / 2)))
    s1, s4 = frames(-half, half)
    timed("sliding rows -%d..%d (the same average width), 1 slide (b)" % (half, half), lambda: Q.q3.sliding(by, order, s1)(*args))
    timed("sliding rows -%d..%d (the same average width), 4 slides (b)" % (half, half), lambda: Q.q3.sliding(by, order, s4)(*args))
    c1 = timed("ranged value, 1 range (c) order_by + ResultSet.ranged", lambda: ordered(*args).ranged(by, order, one))
    c4 = timed("ranged value, 4 ranges (c) order_by + ResultSet.ranged", lambda: ordered(*args).ranged(by, order, four))
    same = a4.columns == c4.columns and [x[0] for x in a4.ordered_rows()] == [x[0] for x in c4.ordered_rows()] and (a4.column("n") == c4.column("n")).all() \
        and (a4.column("best") == c4.column("best")).all() and np.allclose(a4.column("near"), c4.column("near"), rtol=1e-12, atol=0.0)
    print("q3 SF=%g ranged, 4 ranges: (a) and (c) give the same orders in the same sequence, the same counts, maxima and sums: %s" % (sf, same), flush=True)
