#!/usr/bin/env python3
"""q3 at a given SF finished with ORDER BY ... LIMIT per group: `top_per(3, ["o_orderdate"], [("revenue", "desc")])` and `numbered` of the
same terms (every row plus its row_number), each two ways:

    (a) the device route (sdqh_table_window): wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call
    (b) what a caller did before there was one: `order_by` of the same terms (sdqh_table_sorted_by / _sorted with SORT_ALL, every row
        copied to the host) followed by the numpy ranking of ResultSet.window_index on the ordered rows

    window_probe.py SF [runs]              medians of `runs` calls (default 30) after 5 warm-up calls"""
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


def kernel_times(call, names=("k_sort", "k_win", "k_compact", "topk")):
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
legs = [
    ("top_per(3)", lambda: Q.q3.top_per(3, by, order)(*args), lambda: ordered(*args).top_per(3, by, order)),
    ("numbered", lambda: Q.q3.numbered(by, order)(*args), lambda: ordered(*args).numbered(by, order)),
]
for what, device, before in legs:
    for label, leg in (("(a) device", device), ("(b) order_by + numpy", before)):
        def call(leg=leg):
            r = leg()
            r.size()                                                    # (the rows are on the host)
            return r
        med, lo, hi = median_ms(call, 5, runs)
        r = call()
        route = [x for x in eng.stats()["order_routes"] if x][-1]
        print("q3 SF=%g %s %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, label, med, runs, lo, hi, r.size(), route["route"]), flush=True)
        print("   ", kernel_times(call), flush=True)
    a, b = device(), before()
    same = a.columns == b.columns and [x[0] for x in a.ordered_rows()] == [x[0] for x in b.ordered_rows()]
    print("q3 SF=%g %s: both ways give the same orders in the same sequence: %s" % (sf, what, same), flush=True)
