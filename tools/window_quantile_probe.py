#!/usr/bin/env python3
"""q3 at a given SF finished with functions of the size of the row's group: `quantiles(["o_orderdate"], [("revenue", "asc")], cols)` with
one column (the median revenue) and with four (median, the 90th percentile by PERCENTILE_DISC, NTILE(4), CUME_DIST), for every row
and with per=1 (one row per order date: the GROUP BY form), against:

    (a) the device route (sdqh_table_window_quantile): wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call
    (b) `numbered` (ROW_NUMBER as a column) and `sliding` with one 3-row moving sum on the same result, the siblings' own probes (they
        launch what they launched before this route existed: run them on both commits with --no-quantiles)
    (c) what a caller did before there was a device route: `order_by` of the same terms (every row copied to the host) followed by
        ResultSet.quantiles

    window_quantile_probe.py SF [runs] [--no-quantiles]     medians of `runs` calls (default 30) after 5 warm-up calls"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

import numpy as np

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
have_quantiles = "--no-quantiles" not in sys.argv
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_wsl", "k_wq", "k_compact", "topk")):
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
by, order = ["o_orderdate"], [("revenue", "asc")]
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


timed("numbered, ROW_NUMBER as a column", lambda: Q.q3.numbered(by, order, name="rn")(*args))
timed("sliding, 1 moving sum of 3 rows", lambda: Q.q3.sliding(by, order, {"ma3": ("sum", "revenue", -2, 0)})(*args))
if have_quantiles:
    one = {"med": ("median", "revenue")}
    four = dict(one, p90=("percentile_disc", "revenue", 0.9), q=("ntile", 4), cd=("cume_dist",))
    timed("quantiles, 1 column, every row (a) device", lambda: Q.q3.quantiles(by, order, one)(*args))
    a4 = timed("quantiles, 4 columns, every row (a) device", lambda: Q.q3.quantiles(by, order, four)(*args))
    timed("quantiles, 1 column, per=1 (a) device", lambda: Q.q3.quantiles(by, order, one, per=1)(*args))
    g4 = timed("quantiles, 4 columns, per=1 (a) device", lambda: Q.q3.quantiles(by, order, four, per=1)(*args))
    timed("quantiles, 1 column, every row (c) order_by + ResultSet.quantiles", lambda: ordered(*args).quantiles(by, order, one))
    c4 = timed("quantiles, 4 columns, every row (c) order_by + ResultSet.quantiles", lambda: ordered(*args).quantiles(by, order, four))
    h4 = timed("quantiles, 4 columns, per=1 (c) order_by + ResultSet.quantiles", lambda: ordered(*args).quantiles(by, order, four, per=1))
    for what, a, c in (("every row", a4, c4), ("per=1", g4, h4)):
        same = a.columns == c.columns and [x[0] for x in a.ordered_rows()] == [x[0] for x in c.ordered_rows()] and (a.column("q") == c.column("q")).all() \
            and (a.column("cd") == c.column("cd")).all() and np.allclose(a.column("med"), c.column("med"), rtol=1e-12, atol=0.0) \
            and np.allclose(a.column("p90"), c.column("p90"), rtol=1e-12, atol=0.0)
        print("q3 SF=%g quantiles, 4 columns, %s: (a) and (c) give the same orders in the same sequence, the same tiles, distributions, medians and percentiles: %s"
              % (sf, what, same), flush=True)
