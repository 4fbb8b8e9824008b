#!/usr/bin/env python3
"""q3 at a given SF finished with sessions — `sessions(["o_shippriority"], [("o_orderdate", "asc")], gap=1, cols)`: the runs of
consecutive order dates (yyyymmdd integers: a month's end is a gap) per ship priority — per row with four columns, and per session
with one column and with four, four ways:

    (a) the device route (sdqh_table_sessions): one sort, the boundary pass, the folds over its cuts; wall ms, the route
        Engine.stats() reports, per-kernel HIP-event times of one call
    (b) the host route, what a caller did before there was a device route: `order_by` of the same columns (every row copied to the
        host) followed by ResultSet.sessions
    (c) the best composition of existing device calls: `sliding` with a LAG of the order column on the device (every row copied to the
        host with its predecessor's date), then a comparison, a cumsum and np.add.reduceat on the host
    (d) the yardstick: one `rollup` call over the same columns (sdqh_table_grouping_sets) — about the same number of passes

and the agreement of (a) and (b): the same rows and integer columns, the double sums within twice g(m) * sum|v|.

    sessions_probe.py SF [runs]          medians of `runs` calls (default 30) after 5 warm-up calls"""
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_wsl", "k_gs", "k_gd", "k_ss", "k_compact", "topk")):
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
by, order, gap = ["o_shippriority"], [("o_orderdate", "asc")], 1
one = {"revenue_sum": ("sum", "revenue")}
four = {"from": ("first", "o_orderdate"), "to": ("last", "o_orderdate"), "orders": ("count",), "revenue_sum": ("sum", "revenue")}
ordered = q.order_by([(b, "asc") for b in by] + order)
lagged = q.sliding(by, order, {"prev": ("lag", "o_orderdate", 1, -(1 << 40))})


class _Rows:
    """what leg (c) leaves: the sessions' columns as arrays"""

    def __init__(self, cols):
        self.cols = cols

    def size(self):
        return len(next(iter(self.cols.values())))


def composed(cols):
    """(c): the device's LAG, then the cuts, a cumsum's worth of positions and one reduceat per column on the host — one row per session"""
    r = lagged(*args)
    date, prev, prio, rev = (np.asarray(r.column(c)) for c in ("o_orderdate", "prev", "o_shippriority", "revenue"))
    head = date - prev > gap                                           # (the first row of a partition: the default, far below every date)
    head[1:] |= prio[1:] != prio[:-1]
    starts = np.nonzero(head)[0]
    stops = np.append(starts[1:], len(date))
    out = {"o_shippriority": prio[starts]}
    for name, (op, *measure) in cols.items():
        out[name] = np.add.reduceat(rev, starts) if op == "sum" else date[starts] if op == "first" else date[stops - 1] if op == "last" else stops - starts
    return _Rows(out)


legs = [
    ("sessions per row, 4 columns (a) device", lambda: q.sessions(by, order, gap=gap, cols=four)(*args)),
    ("sessions per session, 1 column (a) device", lambda: q.sessions(by, order, gap=gap, cols=one, per="session")(*args)),
    ("sessions per session, 4 columns (a) device", lambda: q.sessions(by, order, gap=gap, cols=four, per="session")(*args)),
    ("sessions per row, 4 columns (b) order_by + ResultSet.sessions", lambda: ordered(*args).sessions(by, order, gap=gap, cols=four)),
    ("sessions per session, 1 column (b) order_by + ResultSet.sessions", lambda: ordered(*args).sessions(by, order, gap=gap, cols=one, per="session")),
    ("sessions per session, 4 columns (b) order_by + ResultSet.sessions", lambda: ordered(*args).sessions(by, order, gap=gap, cols=four, per="session")),
    ("sessions per session, 1 column (c) sliding LAG + numpy", lambda: composed(one)),
    ("sessions per session, 4 columns (c) sliding LAG + numpy", lambda: composed(four)),
    ("rollup, 1 sum (d) the yardstick", lambda: q.rollup(["o_orderdate", "o_shippriority"], {"total": ("sum", "revenue")})(*args)),
    ("rollup, 4 aggregates (d) the yardstick", lambda: q.rollup(["o_orderdate", "o_shippriority"], {"mean": ("avg", "revenue"), "total": ("sum", "revenue"), "hi": ("max", "revenue"), "n": ("count", None)})(*args)),
]
medians = {}
for what, leg in legs:
    def call(leg=leg):
        r = leg()
        r.size()                                                        # (the rows are on the host)
        return r
    med, lo, hi = median_ms(call, 5, runs)
    medians[what] = med
    r = call()
    routes = [x for x in eng.stats()["order_routes"] if x]
    print("q3 SF=%g %s: median %.3f ms of %d (min %.3f, max %.3f), %d rows, route %s" % (sf, what, med, runs, lo, hi, r.size(), routes[-1]["route"] if routes else None), flush=True)
    print("   ", kernel_times(call), flush=True)

for a, b in ((0, 3), (1, 4), (2, 5)):
    print("q3 SF=%g %s: device / host = %.3f" % (sf, legs[a][0].split(" (a)")[0], medians[legs[a][0]] / medians[legs[b][0]]), flush=True)
for a, c in ((1, 6), (2, 7)):
    print("q3 SF=%g %s: device / composition = %.3f" % (sf, legs[a][0].split(" (a)")[0], medians[legs[a][0]] / medians[legs[c][0]]), flush=True)

# (a) against (b): the same rows and integer columns; the double sums within twice the bound g(m) * sum|v| (revenues are positive: the
# sum itself), printed in units of that bound
u = 2.0 ** -53
for name, a, b in (("per row", legs[0][1](), legs[3][1]()), ("per session", legs[2][1](), legs[5][1]())):
    same = a.columns == b.columns and len(a) == len(b) and all((np.asarray(a.column(c)) == np.asarray(b.column(c))).all() for c in a.columns if c not in ("revenue", "revenue_sum"))
    m = np.asarray(a.column("orders"), np.float64)
    x, y = np.asarray(a.column("revenue_sum")), np.asarray(b.column("revenue_sum"))
    live = m > 1
    g = (m - 1) * u / (1 - (m - 1) * u)
    worst = float(np.max(np.abs(x[live] - y[live]) / (g[live] * np.abs(y[live])))) if live.any() else 0.0
    print("q3 SF=%g sessions %s: (a) and (b) give the same rows and integer columns: %s; sessions %d, the longest %d rows; largest |sum difference| / (g(m) * sum|v|): %.4f; single-row sessions equal by bits: %s"
          % (sf, name, same, len(m) if name == "per session" else int((np.asarray(a.column("from")) != np.roll(np.asarray(a.column("from")), 1)).sum()), int(m.max()), worst,
             bool((x[~live].view(np.int64) == y[~live].view(np.int64)).all())), flush=True)
