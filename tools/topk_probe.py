#!/usr/bin/env python3
"""q3 at a given SF: full result vs ORDER BY revenue desc, o_orderdate asc LIMIT k (wall ms + top-k / sort kernel times).
k <= 128 is sdqh_table_topk; top(1000) and order_by (no limit) are the device ORDER BY (sdqh_table_sorted) — SDQLPY_AMD_DEVICE_SORT=0 in
the environment sends those two to compact + host lexsort instead, for an A/B."""
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import engine, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import sdqlpy_init

sf = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
sdqlpy_init(3, 1, device=0)
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
