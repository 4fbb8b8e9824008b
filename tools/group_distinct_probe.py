#!/usr/bin/env python3
"""q3 and q16 at a given SF finished with aggregates over the distinct values of a group — q3 `distincts(["o_shippriority"], aggs)` over
o_orderdate, q16 `distincts(["p_brand"], aggs)` over p_type / p_size / supplier_cnt — with one aggregate (a COUNT(DISTINCT)) and with
four, three ways:

    (a) the device route (sdqh_table_group_distinct): one sort per value column, the rows folded to value runs and the runs to groups;
        wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call
    (b) what a caller did before there was a device route: `order_by` of the same columns (every row copied to the host) followed by
        the numpy folds of ResultSet.distincts
    (c) where the question allows it — a COUNT(DISTINCT) alone — two chained grouping calls: the distinct (group, value) combinations
        on the device (sdqh_table_grouping_sets), then a second GROUP BY over those rows, which are a result set on the host

    group_distinct_probe.py SF [runs]          medians of `runs` calls (default 30) after 5 warm-up calls"""
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_gs", "k_gd", "k_compact", "topk")):
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


qs = ("q3", "q16")
db = tpch.generate(sf, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
cases = {
    "q3": (Q.q3, ["o_shippriority"], {"days": ("count_distinct", "o_orderdate")},
           {"days": ("count_distinct", "o_orderdate"), "busiest": ("mode", "o_orderdate"), "that_day": ("mode_count", "o_orderdate"), "orders": ("count", None)}),
    "q16": (Q.q16, ["p_brand"], {"types": ("count_distinct", "p_type")},
            {"types": ("count_distinct", "p_type"), "commonest": ("mode_count", "p_type"), "usual_size": ("mode", "p_size"), "suppliers": ("sum_distinct", "supplier_cnt")}),
}
for name, (q, by, one, four) in cases.items():
    args = [db[t] for t in Q.QUERY_TABLES[name]]
    value = list(one.values())[0][1]
    ordered = q.order_by([(b, "asc") for b in by])
    combos = q.grouping_sets([tuple(by) + (value,)], {})                # the distinct (group, value) combinations, on the device
    legs = [
        ("distincts, 1 aggregate (a) device", lambda: q.distincts(by, one)(*args)),
        ("distincts, 4 aggregates (a) device", lambda: q.distincts(by, four)(*args)),
        ("distincts, 1 aggregate (b) order_by + numpy", lambda: ordered(*args).distincts(by, one)),
        ("distincts, 4 aggregates (b) order_by + numpy", lambda: ordered(*args).distincts(by, four)),
        ("distincts, 1 aggregate (c) two chained grouping calls", lambda: combos(*args).grouping_sets([tuple(by)], {list(one)[0]: ("count", None)})),
    ]
    for what, leg in legs:
        def call(leg=leg):
            r = leg()
            r.size()                                                    # (the rows are on the host)
            return r
        med, lo, hi = median_ms(call, 5, runs)
        r = call()
        routes = [x for x in eng.stats()["order_routes"] if x]
        print("%s SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (name, sf, what, med, runs, lo, hi, r.size(), routes[-1]["route"] if routes else None), flush=True)
        print("   ", kernel_times(call), flush=True)
    a, b, c = legs[1][1](), legs[3][1](), legs[4][1]()
    same = a.columns == b.columns and all((np.asarray(a.column(col)) == np.asarray(b.column(col))).all() for col in a.columns)
    agree = bool((np.asarray(a.column(list(one)[0])) == np.asarray(c.column(list(one)[0]))).all())
    print("%s SF=%g distincts, 4 aggregates: (a) and (b) give the same rows: %s; the chained calls (c) count the same distinct values: %s" % (name, sf, same, agree), flush=True)
