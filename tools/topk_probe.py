#!/usr/bin/env python3
"""q3 at a given SF: full result vs ORDER BY revenue desc, o_orderdate asc LIMIT k (wall ms + top-k / sort kernel times).
k <= 128 is sdqh_table_topk; top(1000) and order_by (no limit) are the device ORDER BY (sdqh_table_sorted) — SDQLPY_AMD_DEVICE_SORT=0 in
the environment sends those two to compact + host lexsort instead, for an A/B.

    topk_probe.py SF                       the q3 legs above
    topk_probe.py SF q16 q2 q2_min ...     instead: order_by and top(100) with TPC-H's own order for the named queries — text, packed and
                                           mixed-radix order columns (sdqh_table_sorted_by; SDQLPY_AMD_DEVICE_SORT=0: the host route) —
                                           median wall ms of 30 calls after 5, the route Engine.stats() reports, the sort kernels' times
    topk_probe.py SF ranks                 the one-time cost of ranking supplier.s_name and customer.c_name (upload + sdqh_text_ranks),
                                           median of 20 fresh columns, and the radix passes each took"""
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

sf = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
sdqlpy_init(3, 1, device=0)


def median_ms(call, warm, runs):
    for _ in range(warm):
        call()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2]


def kernel_times(eng, call, names=("topk", "k_sort", "k_compact", "k_text", "k_rank")):
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


def probe_terms(names):
    eng = engine.default_engine()
    db = tpch.generate(sf, tables=sorted(tpch.columns_for(names)), columns=tpch.columns_for(names))
    for name in names:
        query = Q.QUERIES.get(name) or Q.EXTREMA_QUERIES[name]
        order = Q.TPCH_ORDER[name][1]
        args = [db[t] for t in Q.QUERY_TABLES[name]]
        for what, leg in (("order_by", query.order_by(order)), ("top 100", query.top(100, order))):
            def call(leg=leg):
                r = leg(*args)
                r.size()                                                # (the rows are on the host)
                return r
            ms = median_ms(call, 5, 30)
            r = call()
            print("%s %s: %.3f ms (median of 30), %d rows, route %s" % (name, what, ms, r.size(), eng.stats()["order_routes"][-1]), r.ordered_rows()[:1], flush=True)
            print("   ", kernel_times(eng, call), flush=True)


def probe_ranks():
    import numpy as np
    eng = engine.default_engine()
    db = tpch.generate(sf, tables=["supplier", "customer"], columns={"supplier": ["s_name"], "customer": ["c_name"]})
    for table, column in (("supplier", "s_name"), ("customer", "c_name")):
        c = db[table].getContainer()
        text = c["data"][c["headers"].index(column)]
        shuffled = np.ascontiguousarray(text[np.random.default_rng(1).permutation(len(text))])      # (the generator's names come sorted)

        def call(text=shuffled):
            col = eng.ctx.upload(text)
            ranks, distinct = eng.ctx.text_ranks(col, len(text))
            ranks.free(); col.free()
            return distinct
        ms = median_ms(call, 3, 20)
        up = median_ms(lambda: eng.ctx.upload(shuffled).free(), 3, 20)
        kt = kernel_times(eng, call)
        print("%s.%s: %d rows of %s, %d distinct: upload + ranks %.3f ms, upload alone %.3f ms (medians of 20); %d radix passes" %
              (table, column, len(text), text.dtype, call(), ms, up, sum(n for k, n, _ in kt if k == "k_sort_scatter")), flush=True)
        print("   ", kt, flush=True)


if len(sys.argv) > 2:
    names = [a for a in sys.argv[2:] if a != "ranks"]
    if names:
        probe_terms(names)
    if "ranks" in sys.argv[2:]:
        probe_ranks()
    sys.exit(0)
db = tpch.generate(sf, tables=["lineitem", "customer", "orders"], columns=tpch.columns_for(("q3",)))
order = Q.TPCH_ORDER["q3"][1]
args = [db[t] for t in Q.QUERY_TABLES["q3"]]
legs = [("all rows, no order", lambda: Q.q3(*args)), ("top 10", Q.q3.top(10, order)), ("top 100", Q.q3.top(100, order)),
        ("top 1000", Q.q3.top(1000, order)), ("order_by", Q.q3.order_by(order))]
for what, leg in legs:
    call = leg if what.startswith("all") else (lambda leg=leg: leg(*args))
    for _ in range(5):
        r = call()
    t0 = time.perf_counter()
    for _ in range(50):
        r = call()
        r.size()                                                    # (the rows are on the host)
    print("q3 %s: %.3f ms, %d rows" % (what, (time.perf_counter() - t0) * 20, r.size()), "" if what.startswith("all") else r.ordered_rows()[:2], flush=True)
    print("q3 %s: median of 30 calls %.3f ms" % (what, median_ms(lambda: call().size(), 0, 30)), flush=True)
eng = engine.default_engine()
eng.ctx.set_profiling(True)
for what, leg in legs[1:]:
    eng.ctx.kernel_log = []
    leg(*args)
    times = {}
    for k, ms in eng.ctx.kernel_log:
        if "topk" in k or "k_sort" in k or "k_compact" in k:
            n, t = times.get(k, (0, 0.0))
            times[k] = (n + 1, t + ms)
    print(what, [(k, n, round(t, 4)) for k, (n, t) in times.items()], flush=True)
