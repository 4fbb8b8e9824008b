#!/usr/bin/env python3
"""q3 at a given SF finished with second moments over window frames — `rolling(["o_shippriority"], [("o_orderdate", "asc"),
("l_orderkey", "asc")], aggs)`: a 20-row volatility, a rolling slope, a running variance — with one column and with four, three ways:

    (a) the device route (sdqh_table_window_moments): one sort, the component trees, a query per row and column; wall ms, the route
        Engine.stats() reports, per-kernel HIP-event times of one call
    (b) the host route, what a caller did before there was a device route: `order_by` of the same columns (every row copied to the
        host) followed by ResultSet.rolling — two passes per frame in numpy, a Python loop over the rows: `host_runs` calls only
    (c) the yardstick: `excluding` with an `avg` over the same frames and exclude="no others" (sdqh_table_window_exclude) — the same
        sort, partitions and frame ends, ONE 64-bit tree per column in the place of the (S, Q[, S, Q, C]) states

and the agreement of (a) and (b): the same rows, NaN in the same places, the largest relative difference of the columns.

    window_moments_probe.py SF [runs [host_runs]]          medians of `runs` calls (default 30) after 5 warm-up calls"""
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
host_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_wsl", "k_wrg", "k_wex", "k_wmo", "k_compact", "topk")):
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


db = tpch.generate(sf, tables=sorted(tpch.columns_for(["q3"])), columns=tpch.columns_for(["q3"]))
args = [db[t] for t in Q.QUERY_TABLES["q3"]]
q = Q.q3
by, order = ["o_shippriority"], [("o_orderdate", "asc"), ("l_orderkey", "asc")]
one = {"vol": ("stddev_samp", "revenue", -19, 0)}
four = {"vol": ("stddev_samp", "revenue", -19, 0), "beta": ("regr_slope", "revenue", "l_orderkey", -19, 0), "running": ("var_pop", "revenue", None, 0),
        "around": ("corr", "revenue", "l_orderkey", -50, 50)}
avg_one = {"mean": ("avg", "revenue", -19, 0)}
avg_four = {"mean": ("avg", "revenue", -19, 0), "key": ("avg", "l_orderkey", -19, 0), "running": ("avg", "revenue", None, 0), "around": ("avg", "revenue", -50, 50)}
ordered = q.order_by([(b, "asc") for b in by] + order)

legs = [
    ("rolling, 1 column (a) device", lambda: q.rolling(by, order, one)(*args), runs),
    ("rolling, 4 columns (a) device", lambda: q.rolling(by, order, four)(*args), runs),
    ("rolling, 1 column (b) order_by + ResultSet.rolling", lambda: ordered(*args).rolling(by, order, one), host_runs),
    ("rolling, 4 columns (b) order_by + ResultSet.rolling", lambda: ordered(*args).rolling(by, order, four), host_runs),
    ("excluding avg, 1 column (c) the yardstick", lambda: q.excluding(by, order, avg_one, exclude="no others")(*args), runs),
    ("excluding avg, 4 columns (c) the yardstick", lambda: q.excluding(by, order, avg_four, exclude="no others")(*args), runs),
]
medians = {}
for what, leg, count in legs:
    def call(leg=leg):
        r = leg()
        r.size()                                                        # (the rows are on the host)
        return r
    med, lo, hi = median_ms(call, 5 if count == runs else 1, count)
    medians[what] = med
    r = call()
    routes = [x for x in eng.stats()["order_routes"] if x]
    print("q3 SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, med, count, lo, hi, r.size(), routes[-1]["route"] if routes else None), flush=True)
    print("   ", kernel_times(call), flush=True)

for a, b in ((0, 2), (1, 3)):
    print("q3 SF=%g %s: device / host = %.4f" % (sf, legs[a][0].split(" (a)")[0], medians[legs[a][0]] / medians[legs[b][0]]), flush=True)
for a, c in ((0, 4), (1, 5)):
    print("q3 SF=%g %s: device / yardstick = %.3f" % (sf, legs[a][0].split(" (a)")[0], medians[legs[a][0]] / medians[legs[c][0]]), flush=True)

# (a) against (b): the same rows, NaN (SQL's NULL) in the same places, the columns' largest relative difference
dev, host = legs[1][1](), legs[3][1]()
same = dev.columns == host.columns and len(dev) == len(host) and all((np.asarray(dev.column(c)).astype(str) == np.asarray(host.column(c)).astype(str)).all() for c in dev.columns if c not in four)
for c in four:
    d, h = np.asarray(dev.column(c)), np.asarray(host.column(c))
    live = np.isfinite(d) & np.isfinite(h)
    with np.errstate(all="ignore"):
        rel = np.abs(d[live] - h[live]) / np.maximum(np.abs(h[live]), np.finfo(np.float64).tiny)
    print("q3 SF=%g rolling %s: NaN in the same places: %s; largest |device - host| / |host| over %d rows: %.3g" % (sf, c, bool((np.isnan(d) == np.isnan(h)).all()), int(live.sum()), float(rel.max()) if live.any() else 0.0), flush=True)
print("q3 SF=%g rolling: (a) and (b) give the same rows: %s" % (sf, same), flush=True)
