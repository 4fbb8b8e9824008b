#!/usr/bin/env python3
"""The extrema extension (include/sdqh_extrema.h) at a given SF, in one process: kernel times of
  - the fold over (l_orderkey, l_extendedprice) — clustered runs: one atomic per run —,
  - the same over a shuffled copy of the rows — one atomic per row —,
  - sdqh_column_extrema over l_extendedprice (a pure read: rows x 8 bytes),
  - and, as the yardstick, sdqh_groupby_key with TUPLE_A on the same two columns (the sum per l_orderkey: Q18's loop).
Three runs each: median and range, in ms, from the per-launch event pairs (ctx.set_profiling).  Compare column_extrema's rate with the
copy rate tools/stream_shapes.hip prints on the same machine.
    python tools/extrema_probe.py [SF, default 10] [--shuffled-rows N]"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdqlpy_amd import abi, engine, tpch

sf = float(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 10.0
eng = engine.Engine(engine.load_hip_library().context(device=0))
ctx = eng.ctx
li = tpch.generate(sf, tables=["lineitem"], columns={"lineitem": ["l_orderkey", "l_extendedprice"]})["lineitem"]
key, price = tpch.column(li, "l_orderkey"), tpch.column(li, "l_extendedprice")
n = len(key)
perm = np.random.default_rng(1).permutation(n)
kc, pc = ctx.upload(key), ctx.upload(price)
ks, ps = ctx.upload(key[perm]), ctx.upload(price[perm])
print("SF %g: %d rows, %d keys, rows per step %d" % (sf, n, len(np.unique(key)), ctx.extrema_geometry()), flush=True)


def kernels(run, names):
    """[(sum of the named kernels' ms; None: of every kernel)] of three profiled runs after two warm-up runs."""
    out = []
    for i in range(5):
        ctx.kernel_log = []
        run()
        ctx.synchronize()
        if i >= 2:
            out.append(sum(ms for k, ms in ctx.kernel_log if names is None or k in names))
    return out


def report(what, ms, bytes_moved=None):
    med = statistics.median(ms)
    rate = "" if bytes_moved is None else ", %.2f TB/s of streamed bytes at the median" % (bytes_moved / med / 1e9)
    print("%-58s median %.4f ms, range %.4f - %.4f%s" % (what, med, min(ms), max(ms), rate), flush=True)


tup = abi.make_tuple(abi.TUPLE_A, [pc])
table = ctx.groupby_key(n, abi.make_filter(), kc, tup)              # the entries the folds go into (built once, unprofiled)
ctx.synchronize()
ctx.set_profiling(True)


def groupby():
    ctx.groupby_key(n, abi.make_filter(), kc, tup).free()


def fold(k, v):
    def run():
        ctx.table_extrema(table, k, n, [(0, abi.EXT_MAX, v, True)])
    return run


report("sdqh_groupby_key TUPLE_A, k_probe_agg alone", kernels(groupby, {"k_probe_agg"}), 16 * n)
report("sdqh_groupby_key TUPLE_A, all its kernels", kernels(groupby, None))
report("k_ext_fold (l_orderkey, l_extendedprice), clustered", kernels(fold(kc, pc), {"k_ext_fold"}), 16 * n)
report("k_ext_fold, shuffled rows", kernels(fold(ks, ps), {"k_ext_fold"}), 16 * n)
report("k_ext_begin + k_ext_end (the slots of every entry)", kernels(fold(kc, pc), {"k_ext_begin", "k_ext_end"}))
report("k_col_extrema l_extendedprice", kernels(lambda: ctx.column_extrema(pc, n), {"k_col_extrema"}), 8 * n)
got = ctx.column_extrema(pc, n)
assert got == (float(price.min()), float(price.max()), n), got
keys, _, values, _ = ctx.table_compact(table, 0, ctx.table_compact_count(table, 0))
want = np.zeros(int(key.max()) + 1)
np.maximum.at(want, key, price)
assert (values[0] == want[keys]).all()
print("results checked against numpy", flush=True)
table.free()
eng.close()
