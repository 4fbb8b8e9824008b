#!/usr/bin/env python3
"""q3 at a given SF finished with values over sliding frames: `sliding(["o_orderdate"], [("revenue", "desc")], aggs)` with one slide
(a 3-row moving sum) and with four (LAG 1, the moving sum, the frame's row count, a centred 3-row maximum), three ways:

    (a) the device route (sdqh_table_window_slide): wall ms, the route Engine.stats() reports, per-kernel HIP-event times of one call
    (b) `over` with one ROWS sum of the same terms — the nearest route there was before: the same selection and order, one forward
        scan where (a) has two and a fold (it launches what it launched before this route existed: run it on both commits)
    (c) what a caller did before there was a device route: `order_by` of the same terms (every row copied to the host) followed by
        numpy on the ordered rows (ResultSet.sliding, or with --no-sliding a hand-written numpy moving sum: what runs on a commit
        that has no `sliding`)

    window_slide_probe.py SF [runs] [--no-sliding]     medians of `runs` calls (default 30) after 5 warm-up calls"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

import numpy as np

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
have_sliding = "--no-sliding" not in sys.argv
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


def kernel_times(call, names=("k_sort", "k_win", "k_wagg", "k_wsl", "k_compact", "topk")):
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
one = {"ma3": ("sum", "revenue", -2, 0)}
four = {"prev": ("lag", "revenue", 1), "ma3": ("sum", "revenue", -2, 0), "n3": ("count", None, -2, 0), "best3": ("max", "revenue", -1, 1)}


def by_hand(res):
    """the 3-row moving sum of an ordered result, per order date, in numpy: what a caller writes where there is no `sliding`"""
    d, x = np.asarray(res.column("o_orderdate")), np.asarray(res.column("revenue"))
    pos = np.arange(len(x))
    head = np.concatenate(([True], d[1:] != d[:-1]))
    start = np.maximum.accumulate(np.where(head, pos, 0))
    pad = np.concatenate(([0.0, 0.0], x))
    return np.where(pos - 2 >= start, pad[pos], 0.0) + np.where(pos - 1 >= start, pad[pos + 1], 0.0) + x


legs = [("over, 1 ROWS sum (b) the forward scan", lambda: Q.q3.over(by, order, {"running": ("sum", "revenue", "rows")})(*args))]
if have_sliding:
    legs += [
        ("sliding, 1 slide (a) device", lambda: Q.q3.sliding(by, order, one)(*args)),
        ("sliding, 4 slides (a) device", lambda: Q.q3.sliding(by, order, four)(*args)),
        ("sliding, 1 slide (c) order_by + numpy", lambda: ordered(*args).sliding(by, order, one)),
        ("sliding, 4 slides (c) order_by + numpy", lambda: ordered(*args).sliding(by, order, four)),
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


def hand():
    r = ordered(*args)
    return r, by_hand(r)


med, lo, hi = median_ms(hand, 5, runs)
print("q3 SF=%g moving sum (c) order_by + numpy by hand: median %.3f ms of %d (min %.3f, max %.3f)" % (sf, med, runs, lo, hi), flush=True)
if have_sliding:
    a, c = legs[2][1](), legs[4][1]()
    same = a.columns == c.columns and [x[0] for x in a.ordered_rows()] == [x[0] for x in c.ordered_rows()] and (a.column("n3") == c.column("n3")).all() \
        and np.allclose(a.column("ma3"), hand()[1], rtol=1e-12, atol=0.0)
    print("q3 SF=%g sliding, 4 slides: (a) and (c) give the same orders in the same sequence, the same counts and the same moving sums: %s" % (sf, same), flush=True)
