#!/usr/bin/env python3
"""Which table should the one-pass distinct count of a dictionary of sets (engine._prepare_distinct, SDQH_X_RUNNEW) aggregate into,
and in which order should its gates stand?  Per-call and per-kernel device times (HIP events) of Q21's two set-building loops over
lineitem, each into three tables: a fixed build from l_orderkey itself, a fixed build over the key range lo..hi, a program build of the
keys.  Tuning aid: python tools/distinct_tables.py [SF]   (recorded in profiles/q21_distinct_routes.txt)"""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from sdqlpy_amd import abi, engine, tpch
from sdqlpy_amd.sdql_lib import sdqlpy_init
sdqlpy_init(3, 1, device=0)
eng = engine.default_engine(device=0)
ctx = eng.ctx
sf = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
db = tpch.generate(sf, tables=["lineitem"], columns={"lineitem": ["l_orderkey", "l_suppkey", "l_commitdate", "l_receiptdate"]})
K, V, C, R = (tpch.column(db["lineitem"], c) for c in ("l_orderkey", "l_suppkey", "l_commitdate", "l_receiptdate"))
n = len(K)
ck, cv, cc, cr = (eng.column(a) for a in (K, V, C, R))
lo, hi = int(K.min()), int(K.max())
print("rows", n, "key range", lo, hi, flush=True)

def program(late, table, lookup_first):
    P = abi.Program()
    gates = []
    inner = -1
    if late:
        inner = P.op(abi.X_GT, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=cr), b=P.op(abi.X_COL, abi.T_I64, col=cc))
        gates.append(inner)
    new = P.op(abi.X_RUNNEW, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=cv), b=inner, col=ck)
    look = P.op(abi.X_LOOKUP, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=ck), table=table)
    P.gates = gates + ([look, new] if lookup_first else [new, look])
    return P, look

def timed(name, fn, iters=5):
    fn()
    ctx.set_profiling(True)
    per = []
    for _ in range(iters):
        ctx.kernel_log, ctx.device_log = [], []
        out = fn()
        per.append((list(ctx.kernel_log), list(ctx.device_log)))
        if hasattr(out, "free"):
            out.free()
    ctx.set_profiling(False)
    calls = ", ".join("%s %.3f" % (per[0][1][i][0], statistics.median(p[1][i][1] for p in per)) for i in range(len(per[0][1])))
    kernels = ", ".join("%s %.3f" % (per[0][0][i][0], statistics.median(p[0][i][1] for p in per)) for i in range(len(per[0][0])))
    print("%-44s calls: %s\n%-44s kernels: %s" % (name, calls, "", kernels), flush=True)

def check(table, late):
    kcol, _, _, hcol, nent = ctx.table_columns(table, 1)
    hits = hcol.download()[:nent]
    return int(nent), int(hits.sum())

def from_key_column():
    return ctx.hash_build_unique(n, abi.make_filter(), [], ck, [], accumulate=True)

iota = eng.iota_column(lo, hi - lo + 1)
def from_iota():
    return ctx.hash_build_unique(hi - lo + 1, abi.make_filter(), [], iota, [], accumulate=True)

def from_program():
    P = abi.Program()
    P.key = P.op(abi.X_COL, abi.T_I64, col=ck)
    return ctx.xbuild(n, P, lo, hi, accumulate=True)

for name, make in (("fixed build from the key column", from_key_column), ("fixed build over lo..hi", from_iota), ("program build from the key column", from_program)):
    try:
        timed("TABLE " + name, make)
    except abi.SdqhError as exc:
        print("TABLE", name, "refused:", exc, flush=True)
        continue
    for late in (False, True):
        for lookup_first in (False, True):
            def run():
                t = make()
                P, look = program(late, t, lookup_first)
                ctx.xprobe_aggregate(n, P, look, t)
                return t
            timed("  %s, %s" % ("late rows" if late else "every row", "lookup first" if lookup_first else "first-of-run first"), run)
        t = make(); P, look = program(late, t, False); ctx.xprobe_aggregate(n, P, look, t)
        print("   entries with rows, sum of counts:", check(t, late), flush=True)
        t.free()
