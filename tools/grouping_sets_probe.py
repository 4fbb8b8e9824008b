#!/usr/bin/env python3
"""q3 at a given SF finished with GROUP BY ROLLUP: `rollup(["o_orderdate", "o_shippriority"], aggs)` with one aggregate (the revenue's
sum) and with four (sum, count, max, avg), three ways:

    (a) the device route (sdqh_table_grouping_sets): one sort, the levels folded from the finest down; wall ms, the route
        Engine.stats() reports, per-kernel HIP-event times of one call
    (b) what a caller did before there was a device route: `order_by` of the same columns (every row copied to the host) followed by
        the numpy folds of ResultSet.rollup
    (c) the nearest device route there was: one `over(by[:L], by[L:], aggs over "partition")` per level — sdqh_table_window_agg: a full
        sort and a fold over all n rows for every level, all n rows copied out each time

    grouping_sets_probe.py SF [runs]          medians of `runs` calls (default 30) after 5 warm-up calls"""
import os
import sys
import time

import numpy as np

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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_gs", "k_compact", "topk")):
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
by = ["o_orderdate", "o_shippriority"]
ordered = Q.q3.order_by([(b, "asc") for b in by])
one = {"total": ("sum", "revenue")}
four = {"total": ("sum", "revenue"), "n": ("count", None), "best": ("max", "revenue"), "mean": ("avg", "revenue")}


def per_level(aggs):
    """a window call per level: the level's value beside every row (an average is not an op there: its sum and the count are)"""
    frames = {k: (("sum" if op == "avg" else op), col, "partition") for k, (op, col) in aggs.items()}
    out = [Q.q3.over(by[:L], [(b, "asc") for b in by[L:]] , frames)(*args) for L in range(len(by), 0, -1)]
    out.append(Q.q3.over([], [(b, "asc") for b in by], frames)(*args))
    return out


legs = [
    ("rollup, 1 aggregate (a) device", lambda: Q.q3.rollup(by, one)(*args)),
    ("rollup, 4 aggregates (a) device", lambda: Q.q3.rollup(by, four)(*args)),
    ("rollup, 1 aggregate (b) order_by + numpy", lambda: ordered(*args).rollup(by, one)),
    ("rollup, 4 aggregates (b) order_by + numpy", lambda: ordered(*args).rollup(by, four)),
    ("rollup, 1 aggregate (c) a window call per level", lambda: per_level(one)),
    ("rollup, 4 aggregates (c) a window call per level", lambda: per_level(four)),
]
for what, leg in legs:
    def call(leg=leg):
        r = leg()
        for x in (r if isinstance(r, list) else [r]):
            x.size()                                                    # (the rows are on the host)
        return r
    med, lo, hi = median_ms(call, 5, runs)
    r = call()
    rows = sum(x.size() for x in r) if isinstance(r, list) else r.size()
    route = [x for x in eng.stats()["order_routes"] if x][-1]
    print("q3 SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, med, runs, lo, hi, rows, route["route"]), flush=True)
    print("   ", kernel_times(call), flush=True)
a, b = legs[1][1](), legs[3][1]()
same = a.columns == b.columns and all((np.asarray(a.column(c)) == np.asarray(b.column(c))).all() for c in by + ["n", "best", "grouping"])
close = bool(np.allclose(a.column("total"), b.column("total"), rtol=1e-12, atol=0.0))
print("q3 SF=%g rollup, 4 aggregates: (a) and (b) give the same groups, counts and maxima: %s; sums within 1e-12: %s" % (sf, same, close), flush=True)
