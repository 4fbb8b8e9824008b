#!/usr/bin/env python3
"""q3 at a given SF finished with second moments per group — `moments(["o_orderdate"], aggs)` with one aggregate (a STDDEV_SAMP) and with
four, two of them bivariate, plain and with rollup=True over ["o_orderdate", "o_shippriority"] — three ways:

    (a) the device route (sdqh_table_group_moments): one sort, then per level two fold rounds over the rows (the sums, then the centred
        squares and products); wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call
    (b) what a caller did before there was a device route: `order_by` of the same columns (every row copied to the host) followed by
        the numpy two-pass of ResultSet.moments
    (c) the yardstick: one `rollup` call with an `avg` over the same columns (sdqh_table_grouping_sets) — one fold round over the rows
        and one per coarser level over the groups; the moments are about two of its row rounds per level

and the agreement of (a) and (b): the largest difference of an aggregate in units of the header's bound on Q (both sides meet it, in
different associations), over the groups of more than one row.

    group_moments_probe.py SF [runs]          medians of `runs` calls (default 30) after 5 warm-up calls"""
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_gs", "k_gd", "k_mo", "k_compact", "topk")):
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
one = {"spread": ("stddev_samp", "revenue")}
four = {"spread": ("stddev_samp", "revenue"), "var": ("var_pop", "revenue"), "trend": ("regr_slope", "revenue", "l_orderkey"), "r": ("corr", "revenue", "l_orderkey")}
by1, by2 = ["o_orderdate"], ["o_orderdate", "o_shippriority"]
ordered = q.order_by([(b, "asc") for b in by2])
legs = [
    ("moments, 1 aggregate (a) device", lambda: q.moments(by1, one)(*args)),
    ("moments, 4 aggregates (a) device", lambda: q.moments(by1, four)(*args)),
    ("moments, 1 aggregate, rollup (a) device", lambda: q.moments(by2, one, rollup=True)(*args)),
    ("moments, 4 aggregates, rollup (a) device", lambda: q.moments(by2, four, rollup=True)(*args)),
    ("moments, 1 aggregate (b) order_by + numpy", lambda: ordered(*args).moments(by1, one)),
    ("moments, 4 aggregates (b) order_by + numpy", lambda: ordered(*args).moments(by1, four)),
    ("moments, 4 aggregates, rollup (b) order_by + numpy", lambda: ordered(*args).moments(by2, four, rollup=True)),
    ("rollup, 1 avg (c) the yardstick", lambda: q.rollup(by2, {"mean": ("avg", "revenue")})(*args)),
    ("rollup, 4 aggregates (c) the yardstick", lambda: q.rollup(by2, {"mean": ("avg", "revenue"), "total": ("sum", "revenue"), "keys": ("avg", "l_orderkey"), "n": ("count", None)})(*args)),
]
for what, leg in legs:
    def call(leg=leg):
        r = leg()
        r.size()                                                        # (the rows are on the host)
        return r
    med, lo, hi = median_ms(call, 5, runs)
    r = call()
    routes = [x for x in eng.stats()["order_routes"] if x]
    print("q3 SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, med, runs, lo, hi, r.size(), routes[-1]["route"] if routes else None), flush=True)
    print("   ", kernel_times(call), flush=True)

# (a) against (b): the same rows; the aggregates within twice the header's bound on Q, taken relative (the groups are small: a few
# hundred rows at most, revenues of one magnitude) — printed in units of that bound
for name, a, b in (("plain", legs[1][1](), legs[5][1]()), ("rollup", legs[3][1](), legs[6][1]())):
    same = a.columns == b.columns and len(a) == len(b) and all((np.asarray(a.column(c)).astype(str) == np.asarray(b.column(c)).astype(str)).all() for c in a.columns if c not in four)
    counts = q.rollup(by2, {"n": ("count", None)})(*args) if name == "rollup" else q.rollup(by1, {"n": ("count", None)})(*args)
    m = np.asarray(counts.column("n"), np.float64)[:len(a)]
    u = 2.0 ** -53
    bound = 2 * ((m + 2 * np.sqrt(m) + 6) * u + 4 * m ** 3 * u * u)
    worst = {}
    for c in four:
        x, y = np.asarray(a.column(c)), np.asarray(b.column(c))
        live = np.isfinite(x) & np.isfinite(y) & (y != 0)
        nulls = bool((np.isnan(x) == np.isnan(y)).all())
        worst[c] = (round(float(np.max(np.abs(x[live] - y[live]) / np.abs(y[live]) / bound[live])) if live.any() else 0.0, 4), nulls)
    print("q3 SF=%g moments, 4 aggregates, %s: (a) and (b) give the same groups: %s; per aggregate (largest relative difference / the relative bound on Q, NULLs in the same rows): %s"
          % (sf, name, same, worst), flush=True)
