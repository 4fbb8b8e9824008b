"""TPCH q21 on the MI355X: the reference's rows on both routes of the dictionaries of sets, and the run-aware row-program operation
(SDQH_X_RUNNEW, include/sdqh.h) against numpy.  The CPU half is tests/test_q21_cpu.py."""
import json
import os

import numpy as np
import pytest

import helpers
from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_q21():
    with open(os.path.join(ROOT, "tests", "golden", "tpch_golden_q21.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def hip_engine(hip_lib):
    eng = engine.Engine(hip_lib.context(device=0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oracle_engine(oracle_lib):
    eng = engine.Engine(oracle_lib.context(threads=min(16, os.cpu_count() or 1)))
    yield eng
    eng.close()


def _routes(eng):
    return {l["result"]: l["route"] for l in eng.stats()["distinct_loops"]}


BOTH = {"suppliers_of_order", "late_suppliers_of_order"}


# ---- the query ------------------------------------------------------------------------------------------------------------
def test_goldens_on_the_default_route(hip_engine, golden_q21):
    """Every case, five times (the second run of a plan takes its deferred route, later ones launch its recording where one can be
    made), then under strict_device: generated lineitem is stored in l_orderkey order, so both set-building loops take the one-pass route."""
    hip_engine.distinct_loops.clear()
    for strict in (False, True):
        hip_engine.strict_device = strict
        try:
            for case in golden_q21["cases"]:
                db = helpers.case_db(case)
                for run in range(5):
                    res = helpers.run_query(hip_engine, "q21", db)
                    helpers.check_against_golden(res, case["results"]["q21"], 0.0, "hip/%s/q21 run %d strict %s" % (case["name"], run, strict))
        finally:
            hip_engine.strict_device = False
    assert _routes(hip_engine) == dict.fromkeys(BOTH, "fast"), hip_engine.stats()["distinct_loops"]
    assert hip_engine.stats()["host_loops"] == []


def test_goldens_without_the_direct_layouts(hip_engine, golden_q21):
    try:
        for k in ("direct_index", "row_index", "grouped_index"):
            hip_engine.ctx.set_option(k, 0)
        hip_engine.clear()
        for case in golden_q21["cases"]:
            db = helpers.case_db(case)
            for run in range(2):
                helpers.check_against_golden(helpers.run_query(hip_engine, "q21", db), case["results"]["q21"], 0.0, "hip/hash layouts/%s/q21 run %d" % (case["name"], run))
    finally:
        for k in ("direct_index", "row_index", "grouped_index"):
            hip_engine.ctx.set_option(k, 1)
        hip_engine.clear()


def test_generic_route_on_permuted_rows_and_on_request(hip_engine, golden_q21):
    """Lineitem in no order: the library refuses the run-aware operation (its key column decreases somewhere) and the loops take the
    generic route; the same route on request (Engine.distinct_fast) on the rows as generated.  The reference's rows both times."""
    for case in golden_q21["cases"][:2]:
        db = helpers.case_db(case)
        c = db["lineitem"].getContainer()
        perm = np.random.default_rng(5).permutation(len(c["data"][0]))
        shuffled = dict(db)
        shuffled["lineitem"] = tpch.table_from_columns(c["headers"], [np.ascontiguousarray(a[perm]) for a in c["data"]])
        hip_engine.distinct_loops.clear()
        for run in range(2):
            helpers.check_against_golden(helpers.run_query(hip_engine, "q21", shuffled), case["results"]["q21"], 0.0, "hip/permuted/%s/q21" % case["name"])
        loops = hip_engine.stats()["distinct_loops"]
        assert _routes(hip_engine) == dict.fromkeys(BOTH, "generic") and all("non-decreasing" in l["why"] for l in loops), loops
        hip_engine.invalidate(shuffled["lineitem"])
    hip_engine.distinct_fast = False
    try:
        hip_engine.clear()
        hip_engine.distinct_loops.clear()
        for case in golden_q21["cases"]:
            helpers.check_against_golden(helpers.run_query(hip_engine, "q21", helpers.case_db(case)), case["results"]["q21"], 0.0, "hip/generic/%s/q21" % case["name"])
        assert _routes(hip_engine) == dict.fromkeys(BOTH, "generic")
    finally:
        hip_engine.distinct_fast = True
        hip_engine.clear()


def test_sf10_against_the_cpu_checker(hip_engine, oracle_engine):
    db = tpch.generate(10, tables=sorted(tpch.columns_for(["q21"])), columns=tpch.columns_for(["q21"]))
    want = helpers.run_query(oracle_engine, "q21", db)
    want = helpers.result_rows(want, want.columns)
    oracle_engine.clear()
    assert len(want) > 1000
    hip_engine.distinct_loops.clear()
    for run in range(2):
        got = helpers.run_query(hip_engine, "q21", db)
        helpers.assert_rows_match(helpers.result_rows(got, got.columns), want, 0.0, "sf=10/q21 run %d" % run)
    assert _routes(hip_engine) == dict.fromkeys(BOTH, "fast")
    k, order = Q.TPCH_ORDER["q21"]
    plan = frontend.lower_function(Q.QUERIES["q21"])
    top = engine.execute_plan(hip_engine, plan, [db[t] for t in Q.QUERY_TABLES["q21"]], top=(k, order)).ordered_rows()
    assert [tuple(r) for r in top] == sorted(want, key=lambda r: (-r[1], r[0]))[:k]
    hip_engine.clear()


# ---- the operation --------------------------------------------------------------------------------------------------------
def _runs(n, seed):
    """Key, value, condition columns of n rows (n a multiple of no tile): runs of 1, 2, 7, 63, 64, 65, 300 and 5000 equal keys in random
    order (so that runs end and straddle at every row offset of a tile), keys from below zero upwards with gaps, values drawn from few
    enough numbers that most runs repeat some."""
    rng = np.random.default_rng(seed)
    lengths = []
    while sum(lengths) < n:
        lengths.append(int(rng.choice([1, 2, 7, 63, 64, 65, 300, 5000], p=[0.3, 0.25, 0.2, 0.07, 0.07, 0.07, 0.035, 0.005])))
    lengths[0] = 5000                                               # (one long run from row 0: across the first tiles' ends)
    key = np.repeat(np.cumsum(rng.integers(1, 4, len(lengths))) - 40000, lengths)[:n].astype(np.int64)
    val = rng.integers(0, 40, n).astype(np.int64) * 1000003 - 7
    g = np.round(rng.random(n), 3)
    f = rng.integers(1, 100, n).astype(np.float64)
    return key, val, g, f


def _first_of_run(key, val, passes):
    """numpy restatement: row r is new iff no r' < r has key[r'] = key[r], val[r'] = val[r] and passes[r']."""
    n = len(key)
    order = np.lexsort((np.arange(n), val, key))
    k, v, p = key[order], val[order], passes[order]
    start = np.ones(n, bool)
    start[1:] = (k[1:] != k[:-1]) | (v[1:] != v[:-1])
    group = np.cumsum(start) - 1
    seen_before = np.zeros(n, bool)                                 # within a (key, value) group, in row order: has a passing row come before?
    cum = np.cumsum(p) - p                                          # passing rows strictly before, overall
    base = cum[np.nonzero(start)[0]][group]
    seen_before = (cum - base) > 0
    out = np.empty(n, bool)
    out[order] = ~seen_before
    return out


@pytest.mark.parametrize("n,seed", [(70001, 1), (1300007, 2)])
def test_runnew_against_numpy(hip_engine, n, seed):
    ctx = hip_engine.ctx
    key, val, g, f = _runs(n, seed)
    assert key.min() < 0 and n % 64 != 0 and (np.diff(key) >= 0).all()
    ck, cv, cg, cf = ctx.upload(key), ctx.upload(val), ctx.upload(g), ctx.upload(f)
    passes = g > 0.5

    def program(with_cond, gate_cond):
        P = abi.Program()
        xv = P.op(abi.X_COL, abi.T_I64, col=cv)
        inner = P.op(abi.X_GT, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_F64, col=cg), b=P.op(abi.X_CONST, abi.T_F64, imm_f=0.5)) if with_cond else -1
        new = P.op(abi.X_RUNNEW, abi.T_BOOL, a=xv, b=inner, col=ck)
        P.gates = ([inner] if gate_cond else []) + [new]
        return P, new

    checks = 0
    for with_cond, gate_cond in ((False, False), (True, True), (True, False)):
        new = _first_of_run(key, val, passes if with_cond else np.ones(n, bool))
        keep = new & (passes if gate_cond else True)
        # a scalar sum
        P, _ = program(with_cond, gate_cond)
        P.vals = [P.op(abi.X_COL, abi.T_F64, col=cf)]
        vals, cnt = ctx.xscan_sum(n, P)
        assert cnt == int(keep.sum()) and vals[0] == float(f[keep].sum()), (with_cond, gate_cond, cnt, int(keep.sum()))
        if not with_cond:
            assert cnt == len(np.unique(np.stack([key, val]), axis=1).T)        # the number of distinct (key, value) pairs
        # a small group-by: per residue of the value
        P, _ = program(with_cond, gate_cond)
        xv = P.op(abi.X_COL, abi.T_I64, col=cv)
        P.key = P.op(abi.X_MODI, abi.T_I64, a=P.op(abi.X_ADD, abi.T_I64, a=xv, b=P.op(abi.X_CONST, abi.T_I64, imm_i=7)), imm_i=5)
        P.vals = [P.op(abi.X_COL, abi.T_F64, col=cf)]
        gk, gv, gc = ctx.xgroupby(n, P)
        want_key = (val + 7) % 5
        assert sorted(gk.tolist()) == sorted(np.unique(want_key[keep]).tolist())
        for k_, v_, c_ in zip(gk.tolist(), gv, gc.tolist()):
            sel = keep & (want_key == k_)
            assert c_ == int(sel.sum()) and v_[0] == float(f[sel].sum()), (with_cond, gate_cond, k_)
        # the dense-domain group-by Q21 uses: a count per key into the key's own table = the number of distinct values per key
        ukeys = np.unique(key)
        cu = ctx.upload(ukeys)
        table = ctx.hash_build_unique(len(ukeys), abi.make_filter(), [], cu, [], accumulate=True)
        P, _ = program(with_cond, gate_cond)
        look = P.op(abi.X_LOOKUP, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=ck), table=table)
        P.gates = list(P.gates) + [look]
        ctx.xprobe_aggregate(n, P, look, table)
        kcol, _, _, hcol, nent = ctx.table_columns(table, 0)
        got = dict(zip(kcol.download()[:nent].tolist(), hcol.download()[:nent].tolist()))
        want = dict(zip(ukeys.tolist(), [0] * len(ukeys)))
        uk, cnts = np.unique(key[keep], return_counts=True)
        want.update(zip(uk.tolist(), cnts.tolist()))
        assert got == want, (with_cond, gate_cond)
        del kcol, hcol
        table.free()
        checks += 3
    assert checks == 9
    # where the operation is refused: a key column that decreases somewhere; builds and key sets
    shuffled = ctx.upload(np.ascontiguousarray(key[::-1]))
    P = abi.Program()
    P.gates = [P.op(abi.X_RUNNEW, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=cv), b=-1, col=shuffled)]
    with pytest.raises(abi.SdqhError) as e:
        ctx.xscan_sum(n, P)
    assert e.value.code == abi.ERR_UNSUPPORTED and "non-decreasing" in str(e.value)
    P, _ = program(False, False)
    P.key = P.op(abi.X_COL, abi.T_I64, col=ck)
    for call in (lambda: ctx.xbuild(n, P), lambda: ctx.xkey_set(n, P, int(key.min()), int(key.max()))):
        with pytest.raises(abi.SdqhError) as e:
            call()
        assert e.value.code == abi.ERR_UNSUPPORTED and "RUNNEW" in str(e.value)
    # an inner condition that cannot be evaluated at another row is invalid
    t = ctx.hash_build_unique(len(ukeys), abi.make_filter(), [], cu, [])
    P = abi.Program()
    bad = P.op(abi.X_LOOKUP, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=ck), table=t)
    P.gates = [P.op(abi.X_RUNNEW, abi.T_BOOL, a=P.op(abi.X_COL, abi.T_I64, col=cv), b=bad, col=ck)]
    with pytest.raises(abi.SdqhError) as e:
        ctx.xscan_sum(n, P)
    assert e.value.code == abi.ERR_INVALID
    t.free()
    for c in (ck, cv, cg, cf, cu, shuffled):
        c.free()
