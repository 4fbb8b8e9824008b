"""Parity of the HIP path (libsdqlhip.so, gfx950 kernels) — the tests proper, run with -m gpu.

Every query goes decorator -> front end -> planner -> C ABI -> HIP kernels; nothing here can pass
on a CPU fall-back because there is none (sdqh_create fails without a GPU).

Bars (BASELINE.json north_star): COUNT / integer keys / row selection bit-exact; SUM(double)
within 1e-6 relative of the reference.  The assertions below use 1e-10, far inside that bar — the
only difference from the reference is the order in which doubles are added.
"""
import numpy as np
import pytest

import exact_reference as X
import helpers
from sdqlpy_amd import engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q

pytestmark = pytest.mark.gpu
REL = 1e-10
SUPPORTED = ("q1", "q3", "q5", "q6", "q9")


_MODULE_ENGINES = []                                    # engines the module's fixtures made: _need_memory trims their pools


@pytest.fixture(scope="module")
def hip_engine(hip_lib):
    eng = engine.Engine(hip_lib.context(device=0))
    _MODULE_ENGINES.append(eng)
    yield eng
    _MODULE_ENGINES.remove(eng)
    eng.close()


@pytest.fixture(scope="module")
def oracle_engine(oracle_lib):
    import os
    eng = engine.Engine(oracle_lib.context(threads=min(16, os.cpu_count() or 1)))
    yield eng
    eng.close()


def _need_memory(host_gib, hbm_gib, *engines):
    """The SF=100 tests' guard.  A box that HAS the memory (an MI355X: >= 256 GiB of HBM in total, and enough host memory in total)
    must run them: the pools of engines used earlier in the module are trimmed first, and if the memory is still not free the test
    FAILS — a BASELINE-sized test that is silently skipped has not run (round-5 review).  A smaller box skips, visibly."""
    import psutil
    import torch
    for eng in engines:
        eng.clear()
        eng.trim()
    torch.cuda.empty_cache()
    free_hbm, total_hbm = torch.cuda.mem_get_info(0)
    vm = psutil.virtual_memory()
    need_host, need_hbm = host_gib * (1 << 30), hbm_gib * (1 << 30)
    if vm.available >= need_host and free_hbm >= need_hbm:
        return
    msg = "needs ~%d GiB of host memory (available %.0f of %.0f) and ~%d GiB of HBM free (free %.0f of %.0f)" % (
        host_gib, vm.available / 2**30, vm.total / 2**30, hbm_gib, free_hbm / 2**30, total_hbm / 2**30)
    if total_hbm >= 256 * (1 << 30) and vm.total >= need_host + 32 * (1 << 30):
        pytest.fail("this box has the memory, something is holding it: " + msg)
    pytest.skip(msg)


# ---- SF=100 against an exact reference (tests/exact_reference.py: int64 cents, plain numpy) --------------------------------------------
# The exact results per query, computed once per session from the generated columns (the generator is deterministic: the row counts are
# asserted), and used by all five SF=100 tests.  Figures the tests measure are printed as "sf100-exact:" lines (pytest -s shows them;
# profiles/sf100_exact_reference.txt is a copy of one run).
_SF100_ROWS = {"lineitem": 600_018_671, "orders": 150_000_000, "customer": 15_000_000, "supplier": 1_000_000, "part": 20_000_000,
               "partsupp": 80_000_000, "nation": 25, "region": 5}
_EXACT_SF100 = {}


def _figure(text):
    import resource
    print("sf100-exact: %s | host peak of this process %.1f GiB" % (text, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20), flush=True)


def _exact_sf100(db, qs):
    """{query: exact result} at SF=100 for `qs`, which `db` holds the columns of: those not computed yet in one pass over lineitem."""
    import time
    for t, table in db.items():
        assert len(table.getContainer()["data"][0]) == _SF100_ROWS[t], t
    missing = [q for q in qs if q not in _EXACT_SF100]
    if missing:
        t0 = time.perf_counter()
        _EXACT_SF100.update(X.exact_results(db, missing))
        _figure("exact reference of %s in one pass: %.1f s; %s" % ("+".join(missing), time.perf_counter() - t0, "; ".join(
            "%s %d groups, %d of one row" % (q, _EXACT_SF100[q].size(), _EXACT_SF100[q].one_row_groups()) for q in missing)))
    return {q: _EXACT_SF100[q] for q in qs}


def _close_to_exact_sf100(got, q, db, what):
    worst = X.assert_close_to_exact(got, _exact_sf100(db, (q,))[q], "sf100/%s/%s" % (what, q))
    _figure("%s %s: largest err/bound %.3g" % (what, q, worst))
    return worst


def _cpu_leg_sf100(oracle_lib, got, q, db):
    """The CPU implementation on the same SF=100 tables (16 threads at most; its engine lives for this one query): the HIP result against
    it at REL — sharp on q1's groups of 10^7 - 10^8 rows, where the exact reference's worst-case bound is about 1e-8 — and the CPU
    implementation itself against the exact reference."""
    import os
    import time
    import bench
    cpu = engine.Engine(oracle_lib.context(threads=min(16, os.cpu_count() or 1)))
    try:
        t0 = time.perf_counter()
        want = helpers.run_query(cpu, q, db)
        want = want.wait() if hasattr(want, "wait") else want
        _figure("CPU implementation %s: %.1f s" % (q, time.perf_counter() - t0))
        got = got.wait() if hasattr(got, "wait") else got
        cmp = bench.compare_results(got, want)
        assert cmp["rows_equal"] and cmp["counts_equal"] and cmp["max_rel"] <= REL, (q, cmp)
        if not isinstance(want, float):
            assert cmp["rows"] > 0
        _figure("HIP against the CPU implementation %s: largest relative difference %.3e" % (q, cmp["max_rel"]))
        _close_to_exact_sf100(want, q, db, "CPU implementation")
    finally:
        cpu.close()


def test_backend_is_hip(hip_lib):
    assert hip_lib.backend_name() == "hip-gfx950"


def test_golden_vectors(hip_engine, golden):
    """Every golden vector of the reference (tiny / small / medium + edge-case variants)."""
    n = 0
    for case in golden["cases"]:
        db = helpers.case_db(case)
        for q in case["results"]:
            if q not in SUPPORTED:
                continue
            res = helpers.run_query(hip_engine, q, db)
            helpers.check_against_golden(res, case["results"][q], REL, "%s/%s/hip" % (case["name"], q))
            n += 1
        hip_engine.clear()
    assert n >= 21


def test_sf1_goldens_with_the_size_dependent_paths_on_and_off(hip_engine, golden_sf1):
    """Round 6: the REFERENCE's results at SF=1 (all 21 queries) and with keys beyond 2^40 at SF=0.1 / SF=1 — where twins, delta
    twins, walks, clustered packs, layout choices and device loops over result dictionaries engage — on the default options, with
    the orders the library keeps beside the data off, with the direct layouts off (open addressing everywhere), with result
    dictionaries looped over on the host, and with every feature forced on at every size.  Twice each (the second run takes the
    prepared paths); ints, keys and row sets exact, sums within REL."""
    variants = [
        ("default", {}, {}),
        ("no walks / delta twins / clustered pack", {"x_driven": 0, "delta8": 0, "cluster_pack": 0}, {}),
        ("open addressing behind its hashed filter", {"direct_index": 0, "row_index": 0, "grouped_index": 0}, {}),
        ("open addressing, no filter", {"direct_index": 0, "row_index": 0, "grouped_index": 0, "hash_filter": 0}, {}),
        ("host dictionary loops", {}, {"dict_programs": False}),
        ("every feature at every size", {"feature_min_rows": 0, "coarse_kb": 1}, {}),
    ]
    defaults = {"x_driven": 64, "delta8": 1, "cluster_pack": 1, "direct_index": 1, "row_index": 1, "grouped_index": 1, "feature_min_rows": 1 << 20, "coarse_kb": 64, "hash_filter": 1}
    for name, opts, attrs in variants:
        saved = {k: getattr(hip_engine, k) for k in attrs}
        for k, v in opts.items():
            hip_engine.ctx.set_option(k, v)
        for k, v in attrs.items():
            setattr(hip_engine, k, v)
        hip_engine.clear()
        try:
            for again in range(2):
                assert helpers.check_all_goldens(hip_engine, [golden_sf1], REL, REL, "hip/sf1/%s/%d" % (name, again)) == 23
        finally:
            for k in opts:
                hip_engine.ctx.set_option(k, defaults[k])
            for k, v in saved.items():
                setattr(hip_engine, k, v)
            hip_engine.clear()


def test_every_query_runs_with_the_host_loops_refused(hip_lib, golden_sf1):
    """Round 6: all 21 queries under Engine.strict_device (no numpy loop over a result dictionary on the product path: such a loop
    raises) — Q8's two-row share was the last one — at SF=1, against the REFERENCE's results.  (At the small goldens' sizes a handful
    of groups comes back to the host and is walked there; that is counted and refusable, not silent: Engine.stats().)"""
    eng = engine.Engine(hip_lib.context(device=0))
    eng.strict_device = True
    try:
        assert helpers.check_all_goldens(eng, [golden_sf1], REL, REL, "hip/strict") == 23
        assert eng.stats()["host_loops"] == []
    finally:
        eng.close()


def test_reference_results_at_baseline_size(hip_engine, oracle_lib, golden_sf10):
    """BASELINE.json's configs at their own size against the REFERENCE itself: q1 (configs[1]), q3 (configs[2]), q5, q6, q9 at SF=10 —
    the reference's Python-mode results on these very inputs (tests/golden/tpch_golden_sf10.json.gz: the interpreter's hour, once) —
    on the HIP path (twice: the second run takes the settled routes, recorded plans included) and on the CPU checker with every host
    thread.  Rows, keys and counts exact, sums within REL."""
    import os
    (case,) = golden_sf10["cases"]
    assert case["sf"] == 10.0 and case["rows"]["lineitem"] > 59_000_000 and set(case["results"]) == set(SUPPORTED)
    for again in range(2):
        assert helpers.check_all_goldens(hip_engine, [golden_sf10], REL, REL, "hip/sf10/%d" % again) == 5
    cpu = engine.Engine(oracle_lib.context(threads=os.cpu_count() or 1))
    try:
        assert helpers.check_all_goldens(cpu, [golden_sf10], REL, REL, "oracle/sf10") == 5
    finally:
        cpu.close()
    hip_engine.clear()


def test_decorated_queries_through_public_api(golden, golden_more, golden_wide):
    """The user-facing route: sdqlpy_init(3) + @sdql_compile functions.  The decorator keeps a query's plan, so the second
    and third run of a query on the same tables take the cached paths (prepared plan, marshalled calls per layout
    signature, compiled row programs): every query of every small / medium case three times, each run checked."""
    from sdqlpy_amd.sdql_lib import sdqlpy_init
    sdqlpy_init(3, 1)
    n = 0
    for gold in (golden, golden_more, golden_wide):
        for case in gold["cases"]:
            if case["name"] not in ("small", "medium"):
                continue
            db = helpers.case_db(case)
            for q, want in case["results"].items():
                for run in range(3):
                    res = Q.run(q, db)
                    if q == "q15" and want["rows"]:
                        res = res.top(1, [("total_revenue", "desc")])
                    helpers.check_against_golden(res, want, REL, "%s/%s/api run %d" % (case["name"], q, run))
                n += 1
    assert n >= 40


@pytest.mark.parametrize("sf", [1.0])
def test_against_oracle_sf1(hip_engine, oracle_engine, sf):
    """Same seeded inputs through both implementations of the ABI at SF=1 (the reference's own
    CPU-runnable scale, BASELINE.json configs[0])."""
    db = tpch.generate(sf, tables=sorted(tpch.columns_for(SUPPORTED)), columns=tpch.columns_for(SUPPORTED))
    for q in SUPPORTED:
        got = helpers.run_query(hip_engine, q, db)
        want = helpers.run_query(oracle_engine, q, db)
        if q == "q6":
            assert abs(got - want) <= REL * abs(want)
        else:
            assert sorted(got.columns) == sorted(want.columns)
            helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "sf1/" + q)
    hip_engine.clear()
    oracle_engine.clear()


def test_q1_q6_are_bit_reproducible(hip_engine):
    """K-A / K-C small reduce in a fixed order: two runs must agree to the last bit."""
    db = tpch.generate(0.2, tables=("lineitem",), columns=tpch.columns_for(["q1", "q6"]))
    a, b = helpers.run_query(hip_engine, "q6", db), helpers.run_query(hip_engine, "q6", db)
    assert a == b
    r1, r2 = helpers.run_query(hip_engine, "q1", db), helpers.run_query(hip_engine, "q1", db)
    assert r1.rows() == r2.rows()
    hip_engine.clear()


def test_every_table_layout_gives_the_same_rows(hip_engine, oracle_engine):
    """A drained row's lookups are compiled for the LAYOUT of the table they read (csrc/sdqh_xkernels.hpp x_lookup_l: dense array,
    bitmap + rank, row index, linearised rectangle, grouped runs, open addressing behind a bitmap or bare), which the build chooses from
    the data: the join queries with each family of direct layouts switched off in turn — down to every table an open-addressing one —
    and with the run-time form of the lookups (SDQLPY_AMD_X_NOLAYOUT is read once per process, so that leg is the options' only) give
    the rows of the CPU implementation."""
    qs = ["q3", "q5", "q9", "q10", "q2", "q7", "q12"]
    db = tpch.generate(0.5, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    want = {}
    for q in qs:
        r = helpers.run_query(oracle_engine, q, db)
        want[q] = helpers.result_rows(r, r.columns)
    oracle_engine.clear()
    configs = [{}, {"row_index": 0}, {"grouped_index": 0}, {"row_index": 0, "grouped_index": 0}, {"direct_index": 0, "row_index": 0, "grouped_index": 0}]
    try:
        for cfg in configs:
            for k, v in cfg.items():
                hip_engine.ctx.set_option(k, v)
            hip_engine.clear()
            for q in qs:
                for _ in range(2):                                   # (the second run of a plan takes its deferred / recorded route)
                    r = helpers.run_query(hip_engine, q, db)
                    helpers.assert_rows_match(helpers.result_rows(r, r.columns), want[q], 1e-9, "%s under %r" % (q, cfg))
            for k in cfg:
                hip_engine.ctx.set_option(k, 1)
    finally:
        for k in ("direct_index", "row_index", "grouped_index"):
            hip_engine.ctx.set_option(k, 1)
        hip_engine.clear()


def test_dictionary_passes_started_with_the_plan_change_no_row(hip_engine):
    """Engine.prefetch_dicts on the HIP engine (where Q1's flag columns ARE coded: the tight kernels stream their codes): the rows with
    the passes started in the background when the plan is bound are the rows with every pass made on demand, bit for bit (Q1, Q4: fixed
    orders of addition), and nothing started is left behind."""
    qs = ["q1", "q4", "q12"]
    db = tpch.generate(0.3, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    rows = {}
    saved = hip_engine.__dict__.get("prefetch_dict_rows")
    try:
        for min_rows in (-1, 0):
            hip_engine.prefetch_dict_rows = min_rows
            for q in qs:
                r = helpers.run_query(hip_engine, q, db)
                rows.setdefault(q, []).append(helpers.result_rows(r, r.columns))
            if min_rows == 0:
                li = dict(zip(db["lineitem"].getContainer()["headers"], db["lineitem"].getContainer()["data"]))
                assert id(li["l_returnflag"]) in hip_engine._dicts and id(li["l_returnflag"]) not in hip_engine._dict_futures
            hip_engine.clear()
            assert not hip_engine.__dict__.get("_dict_futures")
        for q in qs:
            assert rows[q][0] == rows[q][1], q
    finally:
        if saved is None:
            hip_engine.__dict__.pop("prefetch_dict_rows", None)
        else:
            hip_engine.prefetch_dict_rows = saved
        hip_engine.clear()


def test_narrow_twins_change_no_bit(hip_engine, oracle_engine):
    """Streamed columns are read through 4-byte twins only when every row of the twin decodes to the
    column's value bit for bit.  (1) TPCH data: every query that streams through twins returns the SAME bits with
    the twins switched off.  (2) Columns the twins cannot hold — prices with more than two decimals, a negative
    zero, a value beyond int32 cents, keys beyond int32 — silently keep their 8-byte form: same bits again, and
    the CPU implementation agrees."""
    qs = ["q1", "q6", "q3", "q5", "q14", "q10", "q4"]
    db = tpch.generate(2.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))

    def run_all(database, names):
        out = {}
        for q in names:
            r = helpers.run_query(hip_engine, q, database)
            out[q] = r if isinstance(r, float) else helpers.result_rows(r, r.columns)
        return out

    with_twins = run_all(db, qs)
    hip_engine.ctx.set_option("narrow", 0)
    hip_engine.clear()
    try:
        without = run_all(db, qs)
    finally:
        hip_engine.ctx.set_option("narrow", 1)
        hip_engine.clear()
    # q5 (LDS group table) and q10 (the orders of one customer) add with f64 atomics in no fixed order: equal to rounding, not to
    # the bit, with or without twins; the register / fixed-order reductions (q1, q6, q14) and q3's one atomic per group are exact
    for q in ("q5", "q10"):
        helpers.assert_rows_match(with_twins.pop(q), without.pop(q), 1e-12, "twins/" + q)
    assert with_twins == without
    # (2) awkward columns
    li = db["lineitem"].getContainer()
    cols = {h: c.copy() for h, c in zip(li["headers"], li["data"])}
    cols["l_extendedprice"][::7] += 1e-7                      # more than two decimals
    cols["l_discount"][5] = -0.0                              # the twin would decode to +0.0
    cols["l_quantity"][11] = 3.0e9                            # beyond int32 hundredths
    cols["l_tax"][3::1000] = 1.0 / 3.0
    cols["l_shipdate"][17] = 1 << 40                          # beyond int32
    awkward = dict(db)
    awkward["lineitem"] = tpch.table_from_columns(li["headers"], [cols[h] for h in li["headers"]])
    a = run_all(awkward, ["q1", "q6", "q14"])
    hip_engine.ctx.set_option("narrow", 0)
    hip_engine.clear()
    try:
        b = run_all(awkward, ["q1", "q6", "q14"])
    finally:
        hip_engine.ctx.set_option("narrow", 1)
        hip_engine.clear()
    assert a == b
    want6 = helpers.run_query(oracle_engine, "q6", awkward)
    assert abs(a["q6"] - want6) <= REL * abs(want6)
    want1 = helpers.run_query(oracle_engine, "q1", awkward)
    helpers.assert_rows_match(a["q1"], helpers.result_rows(want1, want1.columns), REL, "awkward/q1")
    oracle_engine.clear()


def test_row_order_invariance(hip_engine):
    """Size-independent property: a permutation of the probe-side rows leaves every result
    unchanged (exactly for counts and keys, to rounding for sums)."""
    db = tpch.generate(0.05, tables=sorted(tpch.columns_for(SUPPORTED)), columns=tpch.columns_for(SUPPORTED))
    li = db["lineitem"].getContainer()
    perm = np.random.default_rng(7).permutation(len(li["data"][0]))
    shuffled = dict(db)
    shuffled["lineitem"] = tpch.table_from_columns(li["headers"], [c[perm] for c in li["data"]])
    for q in SUPPORTED:
        a, b = helpers.run_query(hip_engine, q, db), helpers.run_query(hip_engine, q, shuffled)
        if q == "q6":
            assert abs(a - b) <= REL * abs(a)
        else:
            helpers.assert_rows_match(helpers.result_rows(a, a.columns), helpers.result_rows(b, a.columns), REL, "perm/" + q)
    hip_engine.clear()


def test_full_size_properties_sf10(hip_engine):
    """BASELINE.json's full size (SF=10, 60 M lineitem rows), where the CPU oracle is too slow for a
    test: properties that hold at any size.  Totals against numpy reductions of the same columns,
    additivity over a split of the probe side (q(A) + q(B) == q(A ∪ B) group by group), counts exact,
    a second run identical."""
    qs = ("q1", "q3", "q5", "q6")
    db = tpch.generate(10, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    li = db["lineitem"].getContainer()
    col = dict(zip(li["headers"], li["data"]))
    n = len(col["l_shipdate"])
    assert n > 59_000_000
    # q6: the scalar against numpy
    m = (col["l_shipdate"] >= 19940101) & (col["l_shipdate"] < 19950101) & (col["l_discount"] >= 0.05) & (col["l_discount"] <= 0.07) & (col["l_quantity"] < 24.0)
    want6 = float(np.sum(col["l_extendedprice"][m] * col["l_discount"][m]))
    got6 = helpers.run_query(hip_engine, "q6", db)
    assert abs(got6 - want6) <= 1e-9 * abs(want6)
    # q1: counts exact and totals against numpy; bit-identical when run again
    q1 = helpers.run_query(hip_engine, "q1", db)
    m1 = col["l_shipdate"] <= 19980902
    assert int(q1.column("count_order").sum()) == int(m1.sum())
    assert abs(float(q1.column("sum_qty").sum()) - float(col["l_quantity"][m1].sum())) <= 1e-9 * float(col["l_quantity"][m1].sum())
    base = float((col["l_extendedprice"][m1] * (1.0 - col["l_discount"][m1])).sum())
    assert abs(float(q1.column("sum_disc_price").sum()) - base) <= 1e-9 * base
    again = helpers.run_query(hip_engine, "q1", db)
    assert again.rows() == q1.rows()
    del m, m1
    # q3 / q5 / q1: additive over a split of lineitem at an odd row (not a tile boundary)
    cut = n // 2 + 333
    halves = []
    for lo, hi in ((0, cut), (cut, n)):
        part = dict(db)
        part["lineitem"] = tpch.table_from_columns(li["headers"], [c[lo:hi] for c in li["data"]])
        halves.append(part)
    for q in ("q1", "q3", "q5"):
        whole = helpers.run_query(hip_engine, q, db)
        value_cols = [c for c in whole.columns if whole.column(c).dtype.kind == "f" or c.startswith("count")]
        key_cols = [c for c in whole.columns if c not in value_cols]
        sums = {}
        for part in halves:
            r = helpers.run_query(hip_engine, q, part)
            for row in zip(*[r.column(c).tolist() for c in key_cols + value_cols]):
                k, v = row[:len(key_cols)], row[len(key_cols):]
                sums[k] = [a + b for a, b in zip(sums.get(k, [0] * len(v)), v)]
        want = {row[:len(key_cols)]: row[len(key_cols):] for row in zip(*[whole.column(c).tolist() for c in key_cols + value_cols])}
        assert sums.keys() == want.keys() and len(want) > 0, q
        for k, v in want.items():
            for c, a, b in zip(value_cols, sums[k], v):
                if isinstance(b, int):
                    assert a == b, (q, k, c)
                elif not c.startswith("avg"):                  # averages are not additive
                    assert abs(a - b) <= 1e-9 * abs(b), (q, k, c, a, b)
    hip_engine.clear()


def test_full_size_sf10_against_the_cpu_implementation(hip_engine, oracle_lib):
    """BASELINE.json's full size against the ORACLE itself, not only through properties: q1, q3, q5 (the timed step), q6 and q9 at
    SF=10 on the HIP path and on the CPU restatement with every host thread (the GPU box's 256 threads take 0.05-0.2 s per query;
    a small host takes a few seconds).  Row sets, keys and counts exact; sums within 1e-10 relative (contract: 1e-6).  The same
    comparison is printed by bench.py's cpu_baseline leg as `parity_at_bench_size`."""
    import os
    import bench
    qs = ("q1", "q3", "q5", "q6", "q9")
    db = tpch.generate(10, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    cpu = engine.Engine(oracle_lib.context(threads=os.cpu_count() or 1))
    try:
        for q in qs:
            got = helpers.run_query(hip_engine, q, db)
            want = helpers.run_query(cpu, q, db)
            if q == "q6":
                assert want != 0.0 and abs(got - want) <= REL * abs(want), (got, want)
                continue
            cmp = bench.compare_results(got.wait() if hasattr(got, "wait") else got, want)
            assert cmp["rows_equal"] and cmp["counts_equal"], (q, cmp)
            assert cmp["rows"] > 0 and cmp["max_rel"] <= REL, (q, cmp)
            if q == "q3":
                assert cmp["rows"] > 100_000
    finally:
        cpu.close()
        hip_engine.clear()


def test_sf100_on_one_gpu_q3_q6(hip_engine, oracle_lib):
    """BASELINE configs[3]'s data size (SF=100: 600 M lineitem rows, 150 M orders) on ONE device — what every rank of the 8-GPU
    configuration holds an eighth of, and the size at which bitmaps stop fitting LDS / L2 and 32-bit offsets start to matter.
    Q6 against a numpy reduction of the same columns; Q3 additive over a split of lineitem at an odd row, counts of groups exact,
    ORDER BY ... LIMIT on the device equal to ordering the full result, a second run bit-identical.
    And against references that are not the HIP path: Q6, EVERY Q3 group, the top 10 and Q1 (600 M rows through the tight encodings)
    against the exact integer reference (tests/exact_reference.py) under its derived bound, one-row groups bit for bit; and against the
    CPU implementation on the same tables at REL, which is itself held to the exact reference."""
    import psutil
    import torch
    _need_memory(150, 120, *_MODULE_ENGINES)
    qs = ("q1", "q3", "q6")
    db = tpch.generate(100, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    exact = _exact_sf100(db, qs)
    li = db["lineitem"].getContainer()
    col = dict(zip(li["headers"], li["data"]))
    n = len(col["l_shipdate"])
    assert n > 599_000_000
    m = (col["l_shipdate"] >= 19940101) & (col["l_shipdate"] < 19950101)
    m &= (col["l_discount"] >= 0.05) & (col["l_discount"] <= 0.07)
    m &= col["l_quantity"] < 24.0
    want6 = float(np.sum(col["l_extendedprice"][m] * col["l_discount"][m]))
    del m
    got6 = helpers.run_query(hip_engine, "q6", db)
    assert abs(got6 - want6) <= 1e-9 * abs(want6), (got6, want6)
    _close_to_exact_sf100(got6, "q6", db, "HIP")
    _cpu_leg_sf100(oracle_lib, got6, "q6", db)
    got1 = helpers.run_query(hip_engine, "q1", db)
    _close_to_exact_sf100(got1, "q1", db, "HIP")
    assert len(exact["q1"].m) == 4 and max(exact["q1"].m) > 100_000_000   # (groups the bound alone is loose on: the CPU leg below is sharp there)
    _cpu_leg_sf100(oracle_lib, got1, "q1", db)
    del got1
    whole = helpers.run_query(hip_engine, "q3", db)
    assert whole.size() > 1_000_000
    _close_to_exact_sf100(whole, "q3", db, "HIP")
    _cpu_leg_sf100(oracle_lib, whole, "q3", db)
    again = helpers.run_query(hip_engine, "q3", db)
    assert again.size() == whole.size() and all(np.array_equal(again.column(c), whole.column(c)) for c in whole.columns)
    del again
    order_by = Q.TPCH_ORDER["q3"][1]
    plan = frontend.lower_function(Q.QUERIES["q3"])
    got = engine.execute_plan(hip_engine, plan, [db[t] for t in Q.QUERY_TABLES["q3"]], top=(10, order_by)).ordered_rows()
    want_rows = whole.top(10, order_by).ordered_rows()
    assert [r[0] for r in got] == [r[0] for r in want_rows]
    helpers.assert_rows_match(got, want_rows, 1e-10, "q3 top 10 at SF=100")
    assert [r[0] for r in got] == X.top_keys(exact["q3"], 10)                  # ... and the exact reference's own ordering
    # additivity over a split of the probe side, group by group (keys: l_orderkey)
    cut = n // 2 + 777
    keys = whole.column("l_orderkey")
    order = np.argsort(keys, kind="stable")
    total = np.zeros(len(keys))
    for lo, hi in ((0, cut), (cut, n)):
        part = dict(db)
        part["lineitem"] = tpch.table_from_columns(li["headers"], [c[lo:hi] for c in li["data"]])
        r = helpers.run_query(hip_engine, "q3", part)
        pos = np.searchsorted(keys[order], r.column("l_orderkey"))
        assert np.array_equal(keys[order][pos], r.column("l_orderkey"))           # every group of a half is a group of the whole
        np.add.at(total, order[pos], r.column("revenue"))
        hip_engine.invalidate(part["lineitem"])
        del part, r
    rev = whole.column("revenue")
    assert np.all(np.abs(total - rev) <= 1e-9 * np.abs(rev))
    hip_engine.clear()


def test_full_size_q9_and_topk_sf10(hip_engine):
    """The two size holes of the SF=10 suite: q9 (composite-key probe + dense order lookup, 60 M probe rows)
    through additivity over a lineitem split and a numpy total, and ORDER BY ... LIMIT on the device
    against ordering the full SF=10 result on the host."""
    qs = ("q3", "q9")
    db = tpch.generate(10, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    li = db["lineitem"].getContainer()
    n = len(li["data"][0])
    whole = helpers.run_query(hip_engine, "q9", db)
    assert 100 <= whole.size() <= 175 and sorted(whole.columns) == ["nation", "o_year", "sum_profit"]
    again = helpers.run_query(hip_engine, "q9", db)
    helpers.assert_rows_match(helpers.result_rows(again, whole.columns), helpers.result_rows(whole, whole.columns), 1e-10, "q9 rerun")
    cut = n // 3 + 77
    sums = {}
    for lo, hi in ((0, cut), (cut, n)):
        part = dict(db)
        part["lineitem"] = tpch.table_from_columns(li["headers"], [c[lo:hi] for c in li["data"]])
        r = helpers.run_query(hip_engine, "q9", part)
        for nat, yr, v in zip(r.column("nation").tolist(), r.column("o_year").tolist(), r.column("sum_profit").tolist()):
            sums[(nat, yr)] = sums.get((nat, yr), 0.0) + v
    want = dict(zip(zip(whole.column("nation").tolist(), whole.column("o_year").tolist()), whole.column("sum_profit").tolist()))
    assert sums.keys() == want.keys()
    for k, v in want.items():
        assert abs(sums[k] - v) <= 1e-9 * abs(v), (k, sums[k], v)
    # grand total against numpy: rows whose part is green (name contains the word) — every (part, supplier)
    # pair of lineitem exists in partsupp, so the join drops nothing else
    pa = db["part"].getContainer(); pcol = dict(zip(pa["headers"], pa["data"]))
    ps = db["partsupp"].getContainer(); pscol = dict(zip(ps["headers"], ps["data"]))
    green = np.zeros(int(pcol["p_partkey"].max()) + 1, bool)
    green[pcol["p_partkey"][np.char.find(pcol["p_name"], "green") >= 0]] = True
    col = dict(zip(li["headers"], li["data"]))
    m = green[col["l_partkey"]]
    nsupp = int(pscol["ps_suppkey"].max()) + 1
    order = np.argsort(pscol["ps_partkey"] * nsupp + pscol["ps_suppkey"], kind="stable")
    skeys = (pscol["ps_partkey"] * nsupp + pscol["ps_suppkey"])[order]
    lk = col["l_partkey"][m] * nsupp + col["l_suppkey"][m]
    pos = np.searchsorted(skeys, lk)
    assert (skeys[pos] == lk).all()
    sc = pscol["ps_supplycost"][order][pos]
    total = float(np.sum(col["l_extendedprice"][m] * (1.0 - col["l_discount"][m]) - sc * col["l_quantity"][m]))
    got_total = float(whole.column("sum_profit").sum())
    assert abs(got_total - total) <= 1e-9 * abs(total), (got_total, total)
    del m, lk, pos, sc, green
    # top-k on the device == ordering the full result
    full = helpers.run_query(hip_engine, "q3", db)
    assert full.size() > 100000
    for k in (1, 10, 100):
        order_by = Q.TPCH_ORDER["q3"][1]
        plan = frontend.lower_function(Q.QUERIES["q3"])
        got = engine.execute_plan(hip_engine, plan, [db[t] for t in Q.QUERY_TABLES["q3"]], top=(k, order_by)).ordered_rows()
        want_rows = full.top(k, order_by).ordered_rows()
        assert [r[0] for r in got] == [r[0] for r in want_rows], k
        helpers.assert_rows_match(got, want_rows, 1e-10, "q3 top %d" % k)
    hip_engine.clear()


def test_open_vocabulary_queries_against_the_reference(hip_engine, golden_wide, oracle_engine):
    """q2, q7, q8, q11, q12, q13, q15, q16, q17, q19, q20, q22 through kernels specialised on their own conditions and values
    (row programs), against the reference's results; then at SF 1 against the CPU implementation."""
    assert helpers.check_wide_goldens(hip_engine, golden_wide, REL, "hip") >= 36
    qs = ("q2", "q7", "q8", "q11", "q12", "q13", "q15", "q16", "q17", "q19", "q20", "q22")
    db = tpch.generate(1.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    for q in qs:
        got, want = helpers.run_query(hip_engine, q, db), helpers.run_query(oracle_engine, q, db)
        if isinstance(want, float):
            assert abs(got - want) <= REL * abs(want), (q, got, want)
        else:
            assert want.size() > 0, q
            helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "sf1/" + q)
    hip_engine.clear()
    oracle_engine.clear()


def test_plans_the_reference_text_lowers_to(hip_engine, golden_wide, oracle_engine):
    """Round 5: the loops a user of the REFERENCE's script launches.  For q2, q7, q8, q11, q12, q16, q19, q20 the reference's own text
    lowers to other loops than the shipped formulation (other build order, payloads carried as records, another table as the probed
    index); its text never travels, so tests/reference_shapes.py restates those plans in this package's spelling — the CPU suite
    pins their plan digests to the ones recorded for the reference's text (tests/test_frontend_cpu.py) — and here they run on the GPU:
    against the reference's golden results, at SF 1 against the CPU implementation, and timed beside the shipped formulation at SF 1
    (printed; the figures at SF=10 are in profiles/)."""
    import time
    import reference_shapes as shapes
    plans = {q: frontend.lower_function(fn) for q, fn in shapes.QUERIES.items()}
    n = 0
    for case in golden_wide["cases"]:
        db = helpers.case_db(case)
        for q, plan in plans.items():
            if q in case["results"]:
                for again in range(2):                              # the second run takes the prepared, cached paths
                    res = engine.execute_plan(hip_engine, plan, [db[t] for t in shapes.TABLES[q]])
                    helpers.check_against_golden(res, case["results"][q], REL, "reference shape/%s/%s" % (case["name"], q))
                n += 1
        hip_engine.clear()
    assert n >= 3 * len(plans) - 3
    qs = tuple(sorted(plans))
    db = tpch.generate(1.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    for q in qs:
        args = [db[t] for t in shapes.TABLES[q]]
        got = engine.execute_plan(hip_engine, plans[q], args)
        want = engine.execute_plan(oracle_engine, plans[q], args)
        assert want.size() > 0, q
        helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "reference shape sf1/" + q)
        shipped = helpers.run_query(hip_engine, q, db)
        helpers.assert_rows_match(helpers.result_rows(shipped, want.columns), helpers.result_rows(want, want.columns), REL, "shipped sf1/" + q)
        times = {}
        for label, run in (("reference shape", lambda: engine.execute_plan(hip_engine, plans[q], args)), ("shipped", lambda: helpers.run_query(hip_engine, q, db))):
            for _ in range(3):
                r = run(); r.wait() if hasattr(r, "wait") else None
            t0 = time.perf_counter()
            for _ in range(10):
                r = run(); r.wait() if hasattr(r, "wait") else None
            times[label] = (time.perf_counter() - t0) * 100
        print("%s at SF=1: reference-shaped plan %.3f ms, shipped formulation %.3f ms" % (q, times["reference shape"], times["shipped"]))
    hip_engine.clear()
    oracle_engine.clear()


def test_sums_over_result_dictionaries_run_as_device_loops(hip_engine, golden_wide, oracle_engine):
    """frontend.HostDictOp on the device (xplan.prepare_dict_scan: the entries of a table as resident columns — sdqh_table_columns
    hands out the table's own K-F buffers — packed keys unpacked with DIVI / MODI): q16, q15 (with and without ORDER BY / LIMIT
    on the device), q11 against the reference's results and against the host evaluation of the same plans; then q16 at SF 1
    against the CPU implementation, where its source dictionary has some hundred thousand entries."""
    n, on_device = 0, {}
    for case in golden_wide["cases"]:
        k, used = helpers.dict_loop_cases(hip_engine, case, REL)
        n += k
        for q, c in used.items():
            on_device[q] = on_device.get(q, 0) + c
    assert n >= 12 and all(on_device.get(q, 0) >= 2 for q in ("q16", "q15", "q11")), on_device
    qs = ("q16", "q15", "q11", "q2")                        # (q2's 470 offers at SF 1 are a table; at the golden sizes they come back as host groups)
    db = tpch.generate(1.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    with helpers.spy_calls("table_columns") as calls:
        for q in qs:
            got = helpers.run_query(hip_engine, q, db)
            assert calls, q
            del calls[:]
            want = helpers.run_query(oracle_engine, q, db)
            assert want.size() > 0, q
            helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "sf1 dict loop/" + q)
            del calls[:]
    hip_engine.clear()
    oracle_engine.clear()


def test_dense_group_domain_keeps_unreached_keys_out_of_the_dictionary(hip_engine):
    """xplan's one-pass group-by over a dense key domain (Q13's shape) on the device: the dense build with accumulators
    (sdqh_hash_build_unique), the probe-aggregate into it, and a later loop's membership test, against numpy."""
    helpers.dense_domain_case(hip_engine)
    helpers.dense_domain_case(hip_engine, ncust=70000, nord=400000, seed=6)
    helpers.dense_domain_case(hip_engine, ncust=1500000, nord=6000000, seed=7)
    hip_engine.clear()


def test_results_launched_and_not_waited_for(hip_engine, golden, golden_more, golden_wide):
    """Engine.deferred_results on the device: sdqh_xgroupby_async / _collect and sdqh_table_compact_deferred — the plan's last call
    queued, the host free to queue the next query — against the waited-for results of the same plans and the reference's; queries
    launched back to back and read in reverse, results dropped unread, a group table that overflows found at collection; then the
    timed step of the bench at SF 1: three queries launched, then their results read."""
    n, seen = helpers.deferred_result_cases(hip_engine, [golden, golden_more, golden_wide], REL)
    assert n >= 40 and {"q1", "q3", "q5"} <= seen, (n, seen)
    from sdqlpy_amd.result import DeferredResultSet
    qs = ("q1", "q3", "q5")
    db = tpch.generate(1.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    plans = {q: frontend.lower_function(Q.QUERIES[q]) for q in qs}
    hip_engine.deferred_results = False
    want = {q: engine.execute_plan(hip_engine, plans[q], [db[t] for t in Q.QUERY_TABLES[q]]).rows() for q in qs}
    hip_engine.deferred_results = True
    try:
        for _ in range(4):
            rs = [engine.execute_plan(hip_engine, plans[q], [db[t] for t in Q.QUERY_TABLES[q]]) for q in qs]
            assert all(isinstance(r, DeferredResultSet) for r in rs)
            for q, r in zip(qs, rs):
                helpers.assert_rows_match(r.wait().rows(), want[q], REL, "deferred step " + q)
    finally:
        hip_engine.deferred_results = hip_engine.ctx.library.backend_name() == "hip-gfx950"
    hip_engine.clear()


def test_every_golden_vector_through_specialised_kernels(hip_engine, golden, golden_more, golden_wide):
    """All reference results again with every table loop forced through a run-time specialised kernel
    (no ahead-of-time kernel shape): the general path must agree with the tuned one on its home turf."""
    assert helpers.check_all_goldens_as_programs(hip_engine, [golden, golden_more, golden_wide], REL, 1e-10, "hip") >= 82
    hip_engine.clear()


def test_row_programs_specialised_kernels(hip_engine):
    """ABI 4: every sdqh_x* entry point — kernels specialised at run time (hiprtc) on the program —
    against numpy, on the cases the CPU implementation is pinned with; at three sizes around the
    queue / tile boundaries, and once more from the code-object cache."""
    ctx = hip_engine.ctx
    for n in (300, 20000, 70001):
        assert helpers.xprogram_cases(ctx, n) > 40
    before = ctx.jit_stats()
    assert before[0] + before[1] > 0                    # something was specialised (compiled now, or loaded from the disk cache)
    assert helpers.xprogram_cases(ctx, 4097, seed=9) > 40
    assert ctx.jit_stats() == before                    # same program structures: nothing new to compile


def test_hash_layout_at_scale(hip_engine):
    """The open-addressing layout (k_clear / k_insert / hash probes) at 12 M build keys: keys spread
    over 2^44 so no bitmap / direct index applies.  Join + aggregation against numpy."""
    helpers.hash_layout_case(hip_engine.ctx, 12_000_000, 40_000_000)


@pytest.mark.gpu
def test_text_tables_to_query_results_match_the_reference(hip_engine):
    """.tbl -> read_csv -> HIP kernels against the reference's own load + query of the same files."""
    helpers.check_tbl_queries(hip_engine, REL, 1e-10)
    hip_engine.clear()


def test_ragged_sizes(hip_engine, oracle_engine):
    """Row counts around the tile (1024), sub-tile (512), wave (64) and pair (2) boundaries, and empty."""
    base = tpch.generate(0.002, tables=sorted(tpch.columns_for(SUPPORTED)), columns=tpch.columns_for(SUPPORTED))
    li = base["lineitem"].getContainer()
    total = len(li["data"][0])
    for n in [0, 1, 2, 3, 63, 64, 65, 127, 129, 511, 513, 1023, 1024, 1025, 2047, 2049, 4097, total]:
        db = dict(base)
        db["lineitem"] = tpch.table_from_columns(li["headers"], [np.ascontiguousarray(c[:n]) for c in li["data"]])
        for q in SUPPORTED:
            got = helpers.run_query(hip_engine, q, db)
            want = helpers.run_query(oracle_engine, q, db)
            if q == "q6":
                assert abs(got - want) <= REL * max(abs(want), 1e-300), (n, got, want)
            else:
                helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "n=%d/%s" % (n, q))
    hip_engine.clear()
    oracle_engine.clear()


def test_large_scan_instances_on_small_and_ragged_inputs(hip_engine, oracle_engine, golden, golden_more, golden_wide):
    """The instances that large scans select — narrow twins (NW kernels incl. their tail paths), the row pack, the coarse
    key filter in its 1024-thread workgroup, the pipelined streaming steps — are chosen from 1 M / 4 M rows up, where only
    the full-size tests reach them.  With `feature_min_rows` 0 (and a 1 KiB coarse filter) they run on every golden
    vector, on row counts around every tile / wave / pair boundary, and in the differential fuzz."""
    from helpers import fuzz_case
    opts = {"feature_min_rows": 0, "coarse_kb": 1, "lookup_pipeline": 1, "probe_pipeline": 1}
    for k, v in opts.items():
        hip_engine.ctx.set_option(k, v)
    hip_engine.clear()
    try:
        assert helpers.check_all_goldens(hip_engine, [golden, golden_more, golden_wide], REL, 1e-10, "hip/large-scan instances") >= 82
        hip_engine.clear()
        base = tpch.generate(0.002, tables=sorted(tpch.columns_for(SUPPORTED)), columns=tpch.columns_for(SUPPORTED))
        li = base["lineitem"].getContainer()
        total = len(li["data"][0])
        # (520, 521, 1032, 1033, 8200, 8201: a last step of 8 / 9 rows — the delta twin's 12-byte group records behind the last row, round-5 advice)
        for n in [0, 1, 2, 3, 63, 65, 127, 129, 511, 513, 520, 521, 1023, 1025, 1032, 1033, 2047, 2049, 4097, 8191, 8193, 8200, 8201, total]:
            db = dict(base)
            db["lineitem"] = tpch.table_from_columns(li["headers"], [np.ascontiguousarray(c[:n]) for c in li["data"]])
            for q in SUPPORTED:
                got = helpers.run_query(hip_engine, q, db)
                want = helpers.run_query(oracle_engine, q, db)
                if q == "q6":
                    assert abs(got - want) <= REL * max(abs(want), 1e-300), (n, got, want)
                else:
                    helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "n=%d/%s" % (n, q))
        # the same around the ORDERS table's end: the value-queue build streams o_orderkey through its delta twin
        od = base["orders"].getContainer()
        for n in [1, 8, 9, 65, 513, 520, 521, 1025, 1032, 1033, 2049, 2056, 2057]:
            db = dict(base)
            db["orders"] = tpch.table_from_columns(od["headers"], [np.ascontiguousarray(c[:n]) for c in od["data"]])
            for q in ("q3", "q5", "q9"):
                got = helpers.run_query(hip_engine, q, db)
                want = helpers.run_query(oracle_engine, q, db)
                helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "orders n=%d/%s" % (n, q))
        for seed in (11, 12, 13):
            assert fuzz_case(hip_engine.ctx, oracle_engine.ctx, seed) == 12
    finally:
        hip_engine.ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.ctx.set_option("coarse_kb", 64)
        hip_engine.ctx.set_option("lookup_pipeline", -1)
        hip_engine.ctx.set_option("probe_pipeline", 0)
        hip_engine.clear()
        oracle_engine.clear()


def test_many_groups_fallback_and_overflow(hip_engine, oracle_engine):
    """9..64 groups take the LDS kernel; more than 64 is reported, not mis-aggregated."""
    from sdqlpy_amd import abi
    rng = np.random.default_rng(3)
    n = 50000
    for ngroups in (1, 8, 9, 40, 64):
        keys = rng.integers(0, ngroups, n).astype(np.int64) * 7 + 1
        vals = rng.random(n)
        res = {}
        for name, eng in (("hip", hip_engine), ("cpu", oracle_engine)):
            ctx = eng.ctx
            kc, vc = ctx.upload(keys), ctx.upload(vals)
            k, v, c = ctx.groupby_small(n, abi.make_filter(), [kc], abi.make_tuple(abi.TUPLE_A, [vc]))
            order = np.argsort(k[:, 0])
            res[name] = (k[order, 0], v[order, 0], c[order])
        assert (res["hip"][0] == res["cpu"][0]).all() and (res["hip"][2] == res["cpu"][2]).all()
        assert np.allclose(res["hip"][1], res["cpu"][1], rtol=REL, atol=0)
    keys = np.arange(n, dtype=np.int64) % 65
    ctx = hip_engine.ctx
    kc, vc = ctx.upload(keys), ctx.upload(rng.random(n))
    with pytest.raises(abi.SdqhError) as exc:
        ctx.groupby_small(n, abi.make_filter(), [kc], abi.make_tuple(abi.TUPLE_A, [vc]))
    assert exc.value.code == abi.ERR_OVERFLOW


def test_duplicate_build_keys_first_row_wins(hip_engine, oracle_engine):
    """A unique build that meets a duplicate key keeps the lowest row, as emplace/insert(range) do
    in row order (reference generator 366-367, 766-773)."""
    from sdqlpy_amd import abi
    rng = np.random.default_rng(11)
    n = 20000
    keys = rng.integers(0, 3000, n).astype(np.int64)            # heavy duplication
    keys[17] = np.iinfo(np.int64).min                          # the sentinel value itself is a legal key
    keys[9000] = np.iinfo(np.int64).min
    pay = np.arange(n, dtype=np.int64)
    out = {}
    for name, eng in (("hip", hip_engine), ("cpu", oracle_engine)):
        ctx = eng.ctx
        t = ctx.hash_build_unique(n, abi.make_filter(), [], ctx.upload(keys), [ctx.upload(pay)])
        k, p, _, _ = ctx.table_compact(t, 0, t.size())
        order = np.argsort(k)
        out[name] = (k[order], p[0][order])
        t.free()
    assert (out["hip"][0] == out["cpu"][0]).all()
    assert (out["hip"][1] == out["cpu"][1]).all()
    first = {}
    for i, k in enumerate(keys.tolist()):
        first.setdefault(k, i)
    assert dict(zip(out["hip"][0].tolist(), out["hip"][1].tolist())) == first
    # the same on the direct layouts: a key range of one rank block with many workgroups of rows (rank + insert in one launch,
    # k_index_medium), of several rank blocks (k_rank_words + k_insert_direct), and one workgroup of rows (k_index_small / in the build kernel)
    for n2, span in ((20000, 3000), (400000, 300000), (300, 40), (150000, 131000)):
        keys2 = rng.integers(5, 5 + span, n2).astype(np.int64)
        pay2 = np.arange(n2, dtype=np.int64)
        got = {}
        for name, eng in (("hip", hip_engine), ("cpu", oracle_engine)):
            ctx = eng.ctx
            ck, cp = ctx.upload(keys2), ctx.upload(pay2)
            t = ctx.hash_build_unique(n2, abi.make_filter(), [], ck, [cp])
            k, p, _, _ = ctx.table_compact(t, 0, t.size())
            got[name] = dict(zip(k.tolist(), p[0].tolist()))
            t.free(); ck.free(); cp.free()
        first2 = {}
        for i, k in enumerate(keys2.tolist()):
            first2.setdefault(k, i)
        assert got["hip"] == first2 and got["cpu"] == first2, (n2, span)


def test_compaction_into_device_writable_blocks(hip_engine, oracle_engine):
    """K-F through sdqh_host_alloc blocks: rows the kernel wrote into the caller's block, the
    overflow -> retry path, and the pageable-array path all return the same rows, in build order."""
    from helpers import compaction_block_case
    hip, cpu = compaction_block_case(hip_engine.ctx), compaction_block_case(oracle_engine.ctx)
    assert (hip[0] == cpu[0]).all() and (hip[1] == cpu[1]).all() and (hip[3] == cpu[3]).all()
    np.testing.assert_allclose(hip[2], cpu[2], rtol=1e-12)


def test_string_predicates_all_widths(hip_engine):
    """The LDS-staged string predicate of the staging kernel (64- and 32-row staging, the global
    fallback beyond 128 units, equality / inequality / substring with needles up to and beyond 8
    units) against the Python restatement of VarChar semantics."""
    from helpers import string_predicate_case
    assert string_predicate_case(hip_engine.ctx) > 400


def test_text_byte_twins_change_no_result(hip_engine, oracle_engine, golden, golden_more, golden_wide):
    """A text column whose code units are all below 256 is scanned through a one-byte-per-unit twin: the
    staging kernels copy a quarter of the bytes and scan the fields as whole words.  (1) Every predicate mode over many
    widths, through both staging kernels, on a column that has a twin and on one that cannot (a CJK unit).  (2) The
    queries with text conditions on small tables with the twins forced on, against the CPU implementation; the same tables
    with a few fields made non-Latin (the twin is refused: 4-byte units again)."""
    from helpers import string_predicate_case
    hip_engine.ctx.set_option("feature_min_rows", 0)
    hip_engine.clear()
    try:
        for key_set in (False, True):
            assert string_predicate_case(hip_engine.ctx, widths=(1, 2, 3, 7, 10, 25, 33, 55, 79, 100, 128, 129), rows=3000, latin=True, key_set=key_set) > 300
            assert string_predicate_case(hip_engine.ctx, widths=(3, 10, 55, 79), rows=3000, latin=False, key_set=key_set) > 100
        qs = ["q3", "q9", "q13", "q16", "q2", "q20", "q22", "q14", "q19", "q12"]
        db = tpch.generate(0.03, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
        wide = dict(db)
        for table, field in (("part", "p_name"), ("customer", "c_mktsegment"), ("orders", "o_comment")):
            cont = db[table].getContainer()
            cols = {h: c.copy() for h, c in zip(cont["headers"], cont["data"])}
            cols[field][3] = "\u65e5" + str(cols[field][3])[1:]
            wide[table] = tpch.table_from_columns(cont["headers"], [cols[h] for h in cont["headers"]])
        for tag, database in (("latin", db), ("wide", wide)):
            for q in qs:
                got, want = helpers.run_query(hip_engine, q, database), helpers.run_query(oracle_engine, q, database)
                if isinstance(want, float):
                    assert abs(got - want) <= REL * max(abs(want), 1e-300), (tag, q, got, want)
                else:
                    helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "%s/%s" % (tag, q))
            hip_engine.clear(); oracle_engine.clear()
    finally:
        hip_engine.ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()
        oracle_engine.clear()


def test_fill_ahead_changes_nothing(hip_engine, oracle_engine):
    """A fill launch also clears the free pool blocks later builds habitually need cleared, and their own fills are then
    skipped.  Queries interleaved so that blocks change hands between plans and purposes, every run
    against the CPU implementation; the same sequence with `fill_ahead` 0 must give the same rows."""
    qs = ["q5", "q3", "q9", "q18", "q5", "q13", "q9", "q3", "q4", "q22", "q3", "q5", "q9", "q16", "q5", "q3"]
    db = tpch.generate(0.2, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    want = {}
    for q in set(qs):
        r = helpers.run_query(oracle_engine, q, db)
        want[q] = (r.columns, helpers.result_rows(r, r.columns))
    oracle_engine.clear()
    try:
        for ahead in (1, 0, 1):
            hip_engine.ctx.set_option("fill_ahead", ahead)
            for rep in range(2):
                for q in qs:
                    r = helpers.run_query(hip_engine, q, db)
                    helpers.assert_rows_match(helpers.result_rows(r, want[q][0]), want[q][1], REL, "fill_ahead=%d/%s" % (ahead, q))
    finally:
        hip_engine.ctx.set_option("fill_ahead", 1)
        hip_engine.clear()


def test_key_sets_on_unordered_keys(hip_engine):
    """Membership builds on keys in no row order go through bitmaps in LDS (one per workgroup, folded afterwards) instead of one
    device-scope atomic per row: ranges below and above one pass of 2^20 keys, short bitmaps (the fold split over chunks of
    slices), duplicates, a filter; against numpy and against the atomic kernel (`lds_key_set` 0)."""
    from sdqlpy_amd import abi
    ctx = hip_engine.ctx
    rng = np.random.default_rng(5)
    ctx.set_option("feature_min_rows", 0)
    try:
        for n, span in ((5000, 3000), (300000, 2500000), (70001, 1 << 20), (200000, 40000), (70000, 4100000)):
            keys = rng.integers(10, 10 + span, n).astype(np.int64)
            keys[0], keys[1] = 10, 10 + span - 1
            other = rng.integers(0, 100, n).astype(np.int64)
            ck, co = ctx.upload(keys), ctx.upload(other)
            probe = np.arange(0, span + 20, dtype=np.int64)
            cp = ctx.upload(probe)
            for use_filter in (False, True):
                want = np.unique(keys[other <= 29] if use_filter else keys)
                for lds in (1, 0):
                    ctx.set_option("lds_key_set", lds)
                    flt = abi.make_filter(ipreds=[(co, 0, 29)]) if use_filter else abi.make_filter()
                    t = ctx.build_key_set(n, flt, [], ck)
                    (hit,), nh = ctx.scan_compact(len(probe), abi.make_filter(), [(t, cp)], [cp])
                    got = np.sort(hit.download(0, nh)) if nh else np.zeros(0, np.int64)
                    t.free()
                    assert np.array_equal(got, want), (n, span, use_filter, lds, len(got), len(want))
    finally:
        ctx.set_option("lds_key_set", 1)
        ctx.set_option("feature_min_rows", 1 << 20)


def test_membership_only_builds(hip_engine):
    """sdqh_build_key_set (bitmap-only build used for `tbl[k] != None`) against numpy."""
    from helpers import key_set_case
    assert key_set_case(hip_engine.ctx) == 5
    assert key_set_case(hip_engine.ctx, n=1000, seed=2) == 5


def test_share_groups(hip_engine):
    """sdqh_table_share_groups: groups named by fields of the matched entry (Q10)."""
    from helpers import share_groups_case
    assert share_groups_case(hip_engine.ctx) == 6
    assert share_groups_case(hip_engine.ctx, n_build=700, n_probe=5000, seed=4) == 6


def test_groupby_key_and_having(hip_engine):
    """sdqh_groupby_key (dense-range layout and the staged fallback) and sdqh_table_select_keys."""
    from helpers import groupby_key_case
    assert groupby_key_case(hip_engine.ctx) == 3
    assert groupby_key_case(hip_engine.ctx, n=900, seed=3) == 3


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_differential_fuzz_against_the_cpu_implementation(hip_engine, oracle_engine, seed):
    from helpers import fuzz_case
    assert fuzz_case(hip_engine.ctx, oracle_engine.ctx, seed) == 12


def test_empty_inputs(hip_engine):
    """Zero-row tables and filters that pass nothing through the newer entry points (key sets,
    row-keyed group-by, HAVING, top-k, probe sums)."""
    from helpers import empty_input_case
    assert empty_input_case(hip_engine.ctx)


def test_column_comparisons(hip_engine):
    """a op b on two columns (Q4's `l_commitdate < l_receiptdate`): every operator, ints and
    doubles, in the scan, group-by and staging kernels (generic filter instances)."""
    from helpers import column_compare_case
    assert column_compare_case(hip_engine.ctx) == 16


def test_queries_beyond_the_configured_five(hip_engine, oracle_engine, golden_more):
    """q4, q10, q14 and q18: the reference's golden results, then SF=1 against the oracle."""
    import helpers
    from sdqlpy_amd import tpch
    for case in golden_more["cases"]:
        for q in case["results"]:
            res = helpers.run_query(hip_engine, q, helpers.case_db(case))
            helpers.check_against_golden(res, case["results"][q], 1e-10, "%s/%s" % (case["name"], q))
    qs = ("q4", "q10", "q14", "q18")
    db = tpch.generate(1.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    got10, want10 = helpers.run_query(hip_engine, "q10", db), helpers.run_query(oracle_engine, "q10", db)
    helpers.assert_rows_match(got10.rows(), want10.rows(), 1e-10, "sf1/q10")
    assert got10.size() > 10000
    got18, want18 = helpers.run_query(hip_engine, "q18", db), helpers.run_query(oracle_engine, "q18", db)
    assert got18.rows() == want18.rows() and got18.size() > 0
    got4, want4 = helpers.run_query(hip_engine, "q4", db), helpers.run_query(oracle_engine, "q4", db)
    assert got4.rows() == want4.rows() and got4.size() == 5
    got14, want14 = helpers.run_query(hip_engine, "q14", db), helpers.run_query(oracle_engine, "q14", db)
    assert abs(got14 - want14) <= 1e-10 * abs(want14) and 10.0 < got14 < 25.0


def test_table_topk_matches_numpy_and_oracle(hip_engine, oracle_engine):
    """sdqh_table_topk (multi-level selection on the device) against a numpy restatement and the CPU
    implementation: same rows in the same order for every sort spec of the shared case."""
    from helpers import topk_case
    hip, cpu = topk_case(hip_engine.ctx), topk_case(oracle_engine.ctx)
    for (hk, hv), (ck, cv) in zip(hip, cpu):
        assert hk.tolist() == ck.tolist() and hv.tolist() == cv.tolist()
    topk_case(hip_engine.ctx, n=3000, seed=4)                 # fewer segments than CUs: single-level path


def test_query_top_k_through_the_api(hip_engine, oracle_engine):
    """q.top(k, order)(tables): device ORDER BY ... LIMIT on the HIP backend equals ordering the
    oracle's full result (q3: device operator; q1/q5/q9: ≤256 groups ordered on the host)."""
    from sdqlpy_amd import engine, frontend, tpch
    from sdqlpy_amd import tpch_queries as Q
    qs = ("q1", "q3", "q5", "q9")
    db = tpch.generate(0.2, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    for q in qs:
        plan = frontend.lower_function(Q.QUERIES[q].__sdql_func__, Q.QUERIES[q].__sdql_in_type__)
        args = [db[t] for t in Q.QUERY_TABLES[q]]
        k, order = Q.TPCH_ORDER[q]
        want = engine.execute_plan(oracle_engine, plan, args).top(k, order)
        got = engine.execute_plan(hip_engine, plan, args, top=(k, order))
        assert got.columns == want.columns and got.size() == want.size()
        for a, b in zip(got.ordered_rows(), want.ordered_rows()):
            for x, y in zip(a, b):
                assert (abs(x - y) <= 1e-10 * max(abs(x), abs(y))) if isinstance(y, float) else x == y, (q, a, b)


@pytest.mark.parametrize("sf", [0.03, 0.37, 1.3])
def test_every_query_across_sizes(hip_engine, oracle_engine, sf):
    """All seven queries and their top-k variants (k on both sides of the selection / sorting
    switch and of the per-workgroup buffer) at sizes that move every segment, tile and level
    boundary: HIP against the oracle on the same generated database."""
    import helpers
    from sdqlpy_amd import engine, frontend, tpch
    from sdqlpy_amd import tpch_queries as Q
    qs = sorted(Q.QUERIES)
    db = tpch.generate(sf, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
    for q in qs:
        got, want = helpers.run_query(hip_engine, q, db), helpers.run_query(oracle_engine, q, db)
        if isinstance(want, float):
            assert abs(got - want) <= 1e-10 * abs(want), (sf, q, got, want)
            continue
        helpers.assert_rows_match(got.rows(), want.rows(), 1e-10, "sf=%g/%s" % (sf, q))
        if q not in Q.TPCH_ORDER:
            continue
        plan = frontend.lower_function(Q.QUERIES[q])
        args = [db[t] for t in Q.QUERY_TABLES[q]]
        for k in (1, 7, 16, 17, 100, 128):
            t = engine.execute_plan(hip_engine, plan, args, top=(k, Q.TPCH_ORDER[q][1])).ordered_rows()
            w = want.top(k, Q.TPCH_ORDER[q][1]).ordered_rows()
            assert len(t) == len(w), (sf, q, k)
            for a, b in zip(t, w):
                for x, y in zip(a, b):
                    assert (abs(x - y) <= 1e-10 * max(abs(x), abs(y))) if isinstance(y, float) else x == y, (sf, q, k, a, b)


def test_redistribution_helpers_match_oracle(hip_engine, oracle_engine):
    """scan_compact / partition_by_key (hash and range) / bitmap export-import / column copies:
    same multisets of rows from both implementations of the ABI."""
    from sdqlpy_amd import abi
    rng = np.random.default_rng(21)
    n = 70001
    key = rng.integers(0, 5000, n).astype(np.int64) * 3 + 7
    date = rng.integers(19920101, 19981231, n).astype(np.int64)
    val = rng.random(n)
    out = {}
    for name, eng in (("hip", hip_engine), ("cpu", oracle_engine)):
        ctx = eng.ctx
        kc, dc, vc = ctx.upload(key), ctx.upload(date), ctx.upload(val)
        flt = abi.make_filter([(dc, 19950101, 19961231)])
        cols, m = ctx.scan_compact(n, flt, [], [kc, vc])
        rows = sorted(zip(cols[0].download(0, m).tolist(), cols[1].download(0, m).tolist()))
        parts_h, counts_h = ctx.partition_by_key(m, cols[0], 5, cols)
        upper = np.array([2000, 6000, 9000, 12000], np.int64)
        parts_r, counts_r = ctx.partition_by_key(m, cols[0], 5, cols, range_upper=upper)
        kh, vh = parts_h[0].download(0, m), parts_h[1].download(0, m)
        kr = parts_r[0].download(0, m)
        # every partition holds exactly the rows the partition function sends there
        off = np.concatenate([[0], np.cumsum(counts_h)])
        per_part = [sorted(zip(kh[off[p]:off[p + 1]].tolist(), vh[off[p]:off[p + 1]].tolist())) for p in range(5)]
        offr = np.concatenate([[0], np.cumsum(counts_r)])
        for p in range(5):
            seg = kr[offr[p]:offr[p + 1]]
            lo = -1 if p == 0 else upper[p - 1]
            assert ((seg > lo) & ((seg <= upper[p]) if p < 4 else True)).all()
        t = ctx.hash_build_unique(n, abi.make_filter(), [], kc, [])
        words = ctx.table_export_bitmap(t, 7, 7 + 3 * 5000)
        t2 = ctx.table_from_bitmap(words, 7, 7 + 3 * 5000)
        probe = ctx.upload(np.arange(0, 16000, dtype=np.int64))
        (hit,), nh = ctx.scan_compact(16000, abi.make_filter(), [(t2, probe)], [probe])
        out[name] = (m, rows, counts_h.tolist(), per_part, counts_r.tolist(), sorted(hit.download(0, nh).tolist()))
    assert out["hip"] == out["cpu"]
    assert out["hip"][5] == sorted(set(key.tolist()))


def test_packed_exchange_helpers_match_oracle(hip_engine, oracle_engine):
    """Round 4: the partitioning pass that writes the all-to-all's own buffer, its inverse, packed-key splitting and bitmap export
    from key sets / direct-layout tables (what the multi-GPU runner's redistribution steps are made of), against numpy inside the
    helper and against the CPU implementation's digest."""
    got = helpers.redistribution_pack_case(hip_engine.ctx)
    want = helpers.redistribution_pack_case(oracle_engine.ctx)
    assert got["hash"][0] == want["hash"][0] and got["range"][0] == want["range"][0]
    assert got["range"][1] == want["range"][1] and got["hash"][1] == want["hash"][1]
    for n in (70001, 1, 300, 2_000_003):                          # sdqh_xcompact: checked row by row against numpy inside the helper
        assert helpers.xcompact_case(hip_engine.ctx, n=n) == 8
    hip_engine.ctx.set_option("feature_min_rows", 0)             # ... and with the tight encodings on at every size
    try:
        assert helpers.xcompact_case(hip_engine.ctx, n=70001, seed=4) == 8
    finally:
        hip_engine.ctx.set_option("feature_min_rows", 1 << 20)


def test_tight_encodings_on_small_inputs(hip_engine, oracle_engine):
    """Round 3: register row programs stream their columns at the tightest exact encoding — sorted-dictionary codes of 1 / 2 bytes
    (csrc/sdqh_codes.hip), 4-byte twins — 8 rows per lane (x_tight), queue programs test their leading conditions the same way
    (x_queue8).  From 1 M rows up by default; with feature_min_rows 0: every row-program case against numpy at sizes around the
    tile / step boundaries, the code-space comparison edge cases, and q1 / q6 / q3 / q5 with the encodings on and off."""
    ctx = hip_engine.ctx
    ctx.set_option("feature_min_rows", 0)
    hip_engine.clear()
    try:
        for n in (300, 4097, 20000, 70001):
            assert helpers.xprogram_cases(ctx, n) > 40
        assert helpers.xcode_edge_cases(ctx) > 500
        assert helpers.xcode_edge_cases(ctx, n=2047, seed=5) > 500
        qs = ["q1", "q6", "q3", "q5", "q14"]
        db = tpch.generate(0.05, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
        res = {}
        for tight in (1, 0):
            ctx.set_option("tight", tight)
            hip_engine.clear()
            for q in qs:
                r = helpers.run_query(hip_engine, q, db)
                res[(tight, q)] = r if isinstance(r, float) else helpers.result_rows(r, r.columns)
        ctx.set_option("tight", 1)
        for q in qs:
            want = helpers.run_query(oracle_engine, q, db)
            for tight in (1, 0):
                got = res[(tight, q)]
                if isinstance(want, float):
                    assert abs(got - want) <= REL * abs(want), (q, tight)
                else:
                    helpers.assert_rows_match(got, helpers.result_rows(want, want.columns), REL, "tight=%d/%s" % (tight, q))
    finally:
        ctx.set_option("tight", 1)
        ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()
        oracle_engine.clear()


def test_result_rows_delivered_behind_the_call(hip_engine, oracle_engine):
    """K-F's rows reach the host by a copy queued behind the query's kernels (sdqh_table_compact_async); the ResultSet waits for
    them on first read.  Same rows as the synchronous path, also when results are dropped unread and their blocks reused, when
    several results are pending at once, and with the option off."""
    db = tpch.generate(0.3, tables=sorted(tpch.columns_for(["q3", "q18"])), columns=tpch.columns_for(["q3", "q18"]))
    want = helpers.run_query(oracle_engine, "q3", db)
    want_rows = helpers.result_rows(want, want.columns)
    assert hip_engine.lazy_results
    pending = [helpers.run_query(hip_engine, "q3", db) for _ in range(4)]          # four results in flight, none read yet
    for _ in range(6):
        helpers.run_query(hip_engine, "q3", db)                                    # dropped unread: their blocks go round
    for r in pending + [helpers.run_query(hip_engine, "q3", db)]:
        assert r.size() == want.size()
        helpers.assert_rows_match(helpers.result_rows(r, want.columns), want_rows, REL, "lazy q3")
    hip_engine.ctx.set_option("async_result", 0)
    try:
        r = helpers.run_query(hip_engine, "q3", db)
        helpers.assert_rows_match(helpers.result_rows(r, want.columns), want_rows, REL, "synchronous q3")
    finally:
        hip_engine.ctx.set_option("async_result", 1)
    hip_engine.lazy_results = False
    try:
        r = helpers.run_query(hip_engine, "q3", db)
        helpers.assert_rows_match(helpers.result_rows(r, want.columns), want_rows, REL, "eager q3")
    finally:
        hip_engine.lazy_results = True
    hip_engine.clear()
    oracle_engine.clear()


def test_coarse_filter_left_out_when_it_passes_most_rows(hip_engine, oracle_engine):
    """A first lookup on keys in no order whose exact bitmap (3 MB: 24 M keys) dwarfs the LDS budget of the coarse filter: at
    5 % of the keys set, a 64 KiB filter (one bit per 46 keys) passes ~90 % of the rows — Q9 at SF=100.  The library measures the
    filter's density when it builds it (k_coarsen counts the set bits, read at the next call) and leaves a filter that passes more
    than half the rows out: the exact bitmap is then tested straight from L2.  Same groups as the CPU implementation with the
    filter (first call), without it (later calls), and with a sparse set that keeps it."""
    from sdqlpy_amd import abi as A
    rng = np.random.default_rng(17)
    nkeys, nprobe = 24_000_000, 6_000_000
    probe_key = rng.integers(0, nkeys, nprobe).astype(np.int64)
    val = np.round(rng.random(nprobe) * 100.0, 2)
    group = rng.integers(0, 7, nprobe).astype(np.int64)
    results = {}
    for name, eng in (("hip", hip_engine), ("cpu", oracle_engine)):
        ctx = eng.ctx
        ck, cv, cg = ctx.upload(probe_key), ctx.upload(val), ctx.upload(group)
        out = []
        for density in (0.05, 0.02):
            if density == 0.05:                                           # 5 % of the keys, anywhere: nearly every coarse bit is set
                members = np.flatnonzero(np.random.default_rng(3).random(nkeys) < density).astype(np.int64)
            else:                                                         # 2 % of the keys in 24 dense blocks: 2 % of the coarse bits are set
                members = np.concatenate([np.arange(i * 1_000_000, i * 1_000_000 + 20_000, dtype=np.int64) for i in range(24)])
            cm = ctx.upload(members)
            logs = []
            for _ in range(3):
                table = ctx.build_key_set(len(members), A.make_filter(), [], cm)
                if name == "hip":
                    ctx.set_profiling(True); ctx.kernel_log = []
                keys, vals, cnts = ctx.lookup_aggregate(nprobe, A.make_filter(), [(table, [A.src_col(ck)])], [A.src_col(cg)], A.TUPLE_A, [A.src_col(cv)])
                if name == "hip":
                    logs.append([k for k, _ in ctx.kernel_log]); ctx.set_profiling(False)
                order = np.argsort(keys[:, 0])
                out.append((keys[order, 0].tolist(), vals[order, 0].tolist(), cnts[order].tolist()))
                table.free()
            if name == "hip":
                assert "k_coarsen" in logs[0], logs[0]                       # the first call builds and uses the filter
                if density == 0.05:
                    assert "k_coarsen" not in logs[1] and "k_coarsen" not in logs[2], logs       # found dense: left out
                else:
                    assert "k_coarsen" in logs[2], logs                        # sparse: kept
            cm.free()
        results[name] = out
        for c in (ck, cv, cg):
            c.free()
    for got, want in zip(results["hip"], results["cpu"]):
        assert got[0] == want[0] and got[2] == want[2] and len(want[0]) == 7
        assert all(abs(x - y) <= REL * abs(y) for x, y in zip(got[1], want[1]))
    member = np.zeros(nkeys, bool); member[np.flatnonzero(np.random.default_rng(3).random(nkeys) < 0.05)] = True
    hit = member[probe_key]
    assert results["cpu"][0][2] == np.bincount(group[hit], minlength=7).tolist()


def test_distributed_runner_world1_nccl(hip_lib, golden, golden_more):
    """The distributed plan end to end on one GPU (RCCL group of size 1).  The tables carry row-shard marks
    (shard 0 of 1), so the runner takes the PARTITIONED plans — an unmarked table is "whole" and would send every
    query down the single-GPU plan with no collective at all (round 2's hole).  Asserted, not assumed: q3 is
    partitioned, rows go through the exchange, and all_to_all_single / all_gather / all_reduce run on DEVICE
    tensors (torch.distributed wrapped); then SF=1 against the single-GPU plan."""
    import torch
    import torch.distributed as dist
    from sdqlpy_amd import dist as sdist
    from sdqlpy_amd.sdql_lib import shard_rows
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29591", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    calls = []
    real = {n: getattr(dist, n) for n in ("all_to_all_single", "all_gather_into_tensor", "all_reduce")}

    def spy(name):
        def wrapped(*a, **kw):
            t = next(x for x in a if isinstance(x, torch.Tensor))
            calls.append((name, bool(t.is_cuda), int(t.numel())))
            return real[name](*a, **kw)
        return wrapped
    for n in real:
        setattr(dist, n, spy(n))

    def marked(db):
        return {t: (tbl if t in ("region", "nation") else shard_rows(tbl, 0, 1)) for t, tbl in db.items()}
    eng = engine.Engine(hip_lib.context(device=0))
    runners = []
    _new = sdist.DistributedRunner

    def make_runner(*a, **kw):
        kw.setdefault("skip_trivial", False)                 # a group of one still ISSUES its collectives here (the default skips what moves nothing)
        runners.append(_new(*a, **kw))
        return runners[-1]
    try:
        case = next(c for c in golden["cases"] if c["name"] == "small")
        db = marked(helpers.case_db(case))
        for part in ("auto", "hash"):
            runner = make_runner(eng, 0, 1, partition=part)
            for q in SUPPORTED:
                del calls[:]
                helpers.check_against_golden(runner.run(q, db), case["results"][q], REL, "dist1/%s/%s" % (part, q))
                assert calls and all(dev for _, dev, _ in calls), (q, part, calls)       # collectives ran, on device memory
                if q == "q3":
                    assert runner.last_partitioning == {"auto": "range", "hash": "hash"}[part]
                    a2a = [c for c in calls if c[0] == "all_to_all_single"]
                    if part == "hash":
                        assert runner.exchanged_rows["build"] > 0 and runner.exchanged_rows["probe_sent"] > 0, runner.exchanged_rows
                        assert runner.exchanged_rows["probe_received"] == runner.exchanged_rows["probe_sent"]
                        assert len(a2a) >= 2 and sum(n for _, _, n in a2a) >= runner.exchanged_rows["probe_sent"], a2a
                        assert runner.collectives["all_to_all"][1] == runner.collectives["all_to_all"][0] > 0
                        # the join again: device-sized exchanges (chunks through an equal-split all-to-all, the status all-reduced), the
                        # result launched and collected later — same rows, same exchange
                        first = dict(runner.exchanged_rows)
                        for again in range(2):
                            del calls[:]
                            res = runner.run(q, db)
                            helpers.check_against_golden(res, case["results"][q], REL, "dist1/hash/q3 device-sized %d" % again)
                            assert runner.fast_runs == again + 1 and runner.fast_retries == 0
                            assert runner.exchanged_rows == first, (runner.exchanged_rows, first)
                            assert len([c for c in calls if c[0] == "all_to_all_single"]) == 2 and all(dev for _, dev, _ in calls), calls
                    else:
                        assert runner.exchanged_rows == {"build": 0, "probe_sent": 0, "probe_received": 0} and not a2a
            if part == "hash":
                # the default for a group of one: collectives that move nothing are skipped — the same plan, the same rows, no RCCL call
                quiet = make_runner(eng, 0, 1, partition=part, skip_trivial=True)
                for q in SUPPORTED:
                    for again in range(3 if q == "q3" else 1):
                        del calls[:]
                        helpers.check_against_golden(quiet.run(q, db), case["results"][q], REL, "dist1/quiet/%s" % q)
                        assert not calls, (q, calls)
                assert quiet.fast_runs == 2
        more = next(c for c in golden_more["cases"] if c["name"] == "small")
        db = marked(helpers.case_db(more))
        runner = make_runner(eng, 0, 1)
        for q in ("q4", "q14"):                              # the chain executor beyond q5 / q9
            del calls[:]
            helpers.check_against_golden(runner.run(q, db), more["results"][q], REL, "dist1/%s" % q)
            assert calls, q
        # q18: row-keyed group-by, HAVING key set and a local probe-aggregate; customer (text payload) held whole
        helpers.check_against_golden(runner.run("q18", db, whole_tables=("region", "nation", "customer")), more["results"]["q18"], REL, "dist1/q18")
        top = runner.run("q3", marked(helpers.case_db(case)), top=(10, [("revenue", "desc"), ("o_orderdate", "asc")]))
        assert top.size() == 10 and top.column("revenue").tolist() == sorted(top.column("revenue").tolist(), reverse=True)
        # unmarked tables are whole: the single-GPU plan, no collective (and that is the ONLY way to get none)
        del calls[:]
        runner.run("q3", helpers.case_db(case))
        assert not calls and runner.last_partitioning == "range"      # last_partitioning is of the last PARTITIONED run

        # SF=1: the hash-partitioned and the range plan against the single-GPU plan on the same tables
        qs = ("q1", "q3", "q5", "q6", "q9")
        cols = tpch.columns_for(qs)
        big = tpch.generate(1.0, tables=sorted(cols), columns=cols, shard=(0, 1))
        assert big["lineitem"].shard == (0, 1) and getattr(big["nation"], "shard", None) is None
        for part in ("hash", "auto"):
            runner = make_runner(eng, 0, 1, partition=part)
            for q in qs:
                del calls[:]
                got = runner.run(q, big)
                want = helpers.run_query(eng, q, big)
                assert calls, (q, part)
                if q == "q6":
                    assert abs(got - want) <= REL * abs(want)
                    continue
                g, w = sorted(got.rows()), sorted(want.rows())
                assert len(g) == len(w) and len(w) > 0, (q, len(g), len(w))
                for a, b in zip(g, w):
                    for x, y in zip(a, b):
                        assert (abs(x - y) <= REL * max(abs(x), abs(y))) if isinstance(y, float) else x == y, (q, part, a, b)
                if q == "q3" and part == "hash":
                    # the replicated bitmap of all build keys (one all-reduce) lets only the probe rows that will hit travel
                    assert 0 < runner.exchanged_rows["probe_sent"] < 100000 and runner.exchanged_bytes == 0       # all of it to itself
                    assert any(nm == "all_reduce" for nm, _, _ in calls)
                    moved = sum(n for nm, _, n in calls if nm == "all_to_all_single")
                    assert moved >= 3 * runner.exchanged_rows["probe_sent"], (moved, runner.exchanged_rows)   # key + two operands
                    plain = make_runner(eng, 0, 1, partition="hash", prefilter=False)
                    del calls[:]
                    again = plain.run(q, big)
                    assert plain.exchanged_rows["probe_sent"] > 3000000                                       # every filtered probe row, without it
                    assert sorted(again.rows()) == g or all(abs(x - y) <= REL * max(abs(x), abs(y)) if isinstance(y, float) else x == y
                                                            for a, b in zip(sorted(again.rows()), g) for x, y in zip(a, b))
    finally:
        for n in real:
            setattr(dist, n, real[n])
        for obj in runners:                                    # buffers released before the engine's stream goes
            obj.close()
        torch.cuda.synchronize()
        dist.destroy_process_group()
        eng.close()


def _rows_match(got, want, what):
    g, w = sorted(got.rows()), sorted(want.rows())
    assert len(g) == len(w) and len(w) > 0, (what, len(g), len(w))
    for a, b in zip(g, w):
        for x, y in zip(a, b):
            assert (abs(x - y) <= REL * max(abs(x), abs(y))) if isinstance(y, float) else x == y, (what, a, b)


def test_distributed_plans_world1_full_size(hip_lib):
    """The distributed plans at BASELINE's sizes on one GPU (RCCL group of one, tables marked as row shards so that the partitioned
    plans and their collectives really run): q1 / q3 (range and hash) / q5 / q9 / q6 at SF=10 against the single-GPU plan on the same
    tables; the hash-partitioned q3 at SF=100 (32-bit offsets in the partitioning pass, a 75 MB bitmap through the all-reduce) when the
    box has the memory.  N > 1 needs more GPUs than this box has: the same code path under gloo with 2 and 4 ranks is
    tests/test_dist_cpu.py."""
    import psutil
    import torch
    import torch.distributed as dist
    from sdqlpy_amd import dist as sdist
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29593", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    eng = engine.Engine(hip_lib.context(device=0))
    runners = []
    try:
        qs = ("q1", "q3", "q5", "q6", "q9")
        cols = tpch.columns_for(qs)
        db = tpch.generate(10.0, tables=sorted(cols), columns=cols, shard=(0, 1))
        want = {q: helpers.run_query(eng, q, db) for q in qs}
        want = {q: (r.wait() if hasattr(r, "wait") else r) for q, r in want.items()}
        for part in ("hash", "auto"):
            for trivial in (False, True):
                runner = sdist.DistributedRunner(eng, 0, 1, partition=part, skip_trivial=trivial)
                runners.append(runner)
                for q in qs:
                    for again in range(5 if q == "q3" else 1):         # q3's later runs: device-sized exchanges, nothing waited for; from the fourth on one recorded launch
                        got = runner.run(q, db)
                        if q == "q6":
                            assert abs(got - want[q]) <= REL * abs(want[q])
                            continue
                        _rows_match(got, want[q], "sf10/%s/%s/%d" % (part, q, again))
                    if q == "q3":
                        assert runner.last_partitioning == {"auto": "range", "hash": "hash"}[part]
                        if part == "hash":
                            assert runner.exchanged_rows["build"] > 1_000_000 and 100_000 < runner.exchanged_rows["probe_sent"] < 1_000_000, runner.exchanged_rows
                            assert runner.fast_runs == 4 and runner.fast_retries == 0
                            if not trivial:
                                assert runner.collectives["all_to_all"][0] == runner.collectives["all_to_all"][1] >= 6      # one packed all-to-all per exchange, on device memory
                                assert runner.graph_recordings >= 1 and runner.graph_launches >= 2, (runner.graph_recordings, runner.graph_launches)      # (round 6: recorded with its collectives)
                            else:
                                assert not runner.collectives
    finally:
        for obj in runners:
            obj.close()
        torch.cuda.synchronize()
        dist.destroy_process_group()
        eng.close()


def test_groups_of_many_ranks_folded_on_the_device(hip_engine):
    """sdqh_xgroupby_fold by itself (round 6): up to 64 ranks' group tables — laid out like the device result block: 512 key slots, four
    sums and a count per slot, flags — folded by key, block after block.  Against numpy folding the same blocks in the same order: the
    same BITS (a group's sums are ((block 0 + block 1) + block 2) ...), whatever slot a key sits in in each block; groups whose count is
    zero are no groups; more than 256 distinct keys over all blocks, or a block that reported an overflow itself: SDQH_ERR_OVERFLOW
    when the result is collected."""
    import ctypes as C
    from sdqlpy_amd import abi
    ctx = hip_engine.ctx
    nbytes = ctx.xgroupby_block_bytes()
    words, slots = nbytes // 8, 512
    assert slots * 48 + 8 <= nbytes
    rng = np.random.default_rng(21)
    EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

    def make_blocks(nblocks, universe, per_block, flags=None):
        raw = np.zeros((nblocks, words), np.uint64)
        folded = {}
        for b in range(nblocks):
            keys = rng.choice(universe, size=min(per_block, len(universe)), replace=False)
            at = rng.choice(slots, size=len(keys), replace=False)                      # any slot: the fold goes by key
            blk = raw[b]
            blk[:slots] = EMPTY
            acc = blk[slots:slots * 5].view(np.float64).reshape(slots, 4)
            cnt = blk[slots * 5:slots * 6].view(np.int64)
            for k, s_ in zip(keys, at):
                v = rng.normal(size=4) * 10.0 ** rng.integers(-3, 9)
                c = int(rng.integers(0, 5))                                               # (a slot whose count is 0 holds no group)
                blk[s_] = np.uint64(k); acc[s_] = v; cnt[s_] = c
                if c > 0:
                    cur = folded.get(int(k))
                    folded[int(k)] = (v.copy(), c) if cur is None else (cur[0] + v, cur[1] + c)
            if flags is not None:
                blk[slots * 6:slots * 6 + 1].view(np.int32)[0] = flags[b]
        return raw, folded

    def fold(raw):
        col = ctx.upload(np.ascontiguousarray(raw.reshape(-1).view(np.int64)))
        buf = ctx.host_block(nbytes)
        ctx._check(ctx.lib.sdqh_xgroupby_fold(ctx.handle, C.c_void_p(col.data_ptr()), C.c_int(raw.shape[0]), C.addressof(buf)))
        keys, vals, cnts, ng = np.zeros(256, np.int64), np.zeros((256, 4), np.float64), np.zeros(256, np.int64), C.c_int32()
        rc = ctx.lib.sdqh_xgroupby_collect(ctx.handle, C.addressof(buf), C.c_int(4), C.c_int(256), keys.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p),
                                           cnts.ctypes.data_as(C.c_void_p), C.byref(ng))
        col.free()
        return rc, keys[:ng.value], vals[:ng.value], cnts[:ng.value]

    for nblocks, nuniverse, per_block in ((1, 40, 40), (2, 6, 4), (8, 200, 120), (64, 256, 256), (64, 5, 5), (33, 250, 17)):
        universe = rng.choice(1 << 40, size=nuniverse, replace=False).astype(np.int64)
        raw, want = make_blocks(nblocks, universe, per_block)
        rc, keys, vals, cnts = fold(raw)
        assert rc == abi.OK, (nblocks, rc)
        assert sorted(keys.tolist()) == sorted(want), (nblocks, len(keys), len(want))
        for k, v, c in zip(keys.tolist(), vals, cnts.tolist()):
            assert c == want[k][1] and np.array_equal(v, want[k][0]), (nblocks, k, v, want[k])      # the same bits: the same order of adds
    # more than 256 groups over all blocks; a block that overflowed by itself
    universe = np.arange(1000, 1000 + 400, dtype=np.int64)
    raw, _ = make_blocks(4, universe, 200)
    assert fold(raw)[0] == abi.ERR_OVERFLOW
    raw, _ = make_blocks(3, universe[:10], 5, flags=[0, 1, 0])
    assert fold(raw)[0] == abi.ERR_OVERFLOW


def test_one_part_pack_keeps_the_build_order(hip_engine):
    """sdqh_table_partition_pack with ONE part (round 6: the send buffer of an all-gather): the chunk holds the table's entries in the
    order the build met them — key, then every payload column, `chunk_rows` apart behind the two header words — the same bytes run
    after run; the header counts every entry even when the chunk is too small to hold them all (the overflow the receiver reports)."""
    from sdqlpy_amd import abi
    ctx = hip_engine.ctx
    rng = np.random.default_rng(8)
    for n, keep in ((1, 1.0), (777, 0.5), (300_000, 0.3), (2_000_001, 0.02)):
        keys = np.sort(rng.choice(1 << 40, size=n, replace=False)).astype(np.int64)
        p0, p1 = rng.integers(-1 << 50, 1 << 50, size=n), rng.integers(0, 100, size=n)
        gate = rng.random(n) < keep
        gate[0] = True
        ck, c0, c1, cg = ctx.upload(keys), ctx.upload(p0), ctx.upload(p1), ctx.upload(gate.astype(np.int64))
        table = ctx.hash_build_unique(n, abi.make_filter([(cg, 1, 1)], [], []), [], ck, [c0, c1])
        want = [keys[gate], p0[gate], p1[gate]]
        m = int(gate.sum())
        for cap in (m + 10, max(1, m // 2)):
            cw = ctx.chunk_words(3, cap)
            raws = []
            for again in range(2):
                buf = ctx.alloc(cw, abi.I64)
                ctx.table_partition_pack(table, 1, cap, buf.data_ptr())
                ctx.synchronize()
                raws.append(buf.download())
                buf.free()
            raw = raws[0]
            assert int(raw[0]) == m and int(raw[1]) == 0, (n, cap, raw[:2])
            stored = min(m, cap)
            for c, w in enumerate(want):
                assert np.array_equal(raw[2 + c * cap: 2 + c * cap + stored], w[:stored]), (n, cap, c)
                assert np.array_equal(raws[1][2 + c * cap: 2 + c * cap + stored], w[:stored])
        table.free()
        for c in (ck, c0, c1, cg):
            c.free()


def test_multi_part_pack_is_deterministic(hip_engine):
    """sdqh_table_partition_pack with several parts (the send buffer of the hash-partitioned join's all-to-all): every chunk holds exactly
    the entries whose key hashes to its part (mix64(key) % nparts), its header their count — and, round 6, the SAME BYTES run after run:
    rows are placed from per-wave cursors that a scan of per-wave counts fixes, not by racing atomics (option "pack_ordered"; with it
    off the same rows arrive in whatever order)."""
    from sdqlpy_amd import abi
    ctx = hip_engine.ctx
    rng = np.random.default_rng(12)

    def mix64(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
        return x

    try:
        for n, nparts in ((5, 2), (70_000, 3), (1_500_000, 8), (400_000, 64)):
            keys = np.sort(rng.choice(1 << 44, size=n, replace=False)).astype(np.int64)
            p0 = rng.integers(-1 << 40, 1 << 40, size=n)
            ck, c0 = ctx.upload(keys), ctx.upload(p0)
            table = ctx.hash_build_unique(n, abi.make_filter(), [], ck, [c0])
            part = (mix64(keys) % np.uint64(nparts)).astype(np.int64)
            cap = int(np.bincount(part, minlength=nparts).max()) + 7
            cw = ctx.chunk_words(2, cap)
            runs = {}
            for ordered in (1, 1, 0):
                ctx.set_option("pack_ordered", ordered)
                buf = ctx.alloc(nparts * cw, abi.I64)
                ctx.table_partition_pack(table, nparts, cap, buf.data_ptr())
                ctx.synchronize()
                runs.setdefault(ordered, []).append(buf.download())
                buf.free()
            assert np.array_equal(runs[1][0], runs[1][1]) or _same_chunks(runs[1][0], runs[1][1], nparts, cw, cap, exact=True), (n, nparts)
            for raw in (runs[1][0], runs[0][0]):
                for p in range(nparts):
                    chunk = raw[p * cw:(p + 1) * cw]
                    m = int(chunk[0])
                    want = keys[part == p]
                    assert m == len(want), (n, nparts, p, m, len(want))
                    got_k, got_p = chunk[2:2 + m], chunk[2 + cap:2 + cap + m]
                    order = np.argsort(got_k, kind="stable")
                    assert np.array_equal(got_k[order], want) and np.array_equal(got_p[order], p0[part == p]), (n, nparts, p)
            table.free(); ck.free(); c0.free()
    finally:
        ctx.set_option("pack_ordered", 1)


def _same_chunks(a, b, nparts, cw, cap, exact):
    """The live words of two packed buffers (headers and the rows they count; the words behind a chunk's last row are whatever the pool held)."""
    for p in range(nparts):
        ca, cb = a[p * cw:(p + 1) * cw], b[p * cw:(p + 1) * cw]
        m = int(ca[0])
        if m != int(cb[0]):
            return False
        for c in range((cw - 2) // cap):
            if not np.array_equal(ca[2 + c * cap:2 + c * cap + m], cb[2 + c * cap:2 + c * cap + m]):
                return False
    return True


def test_settled_chains_world1_wait_for_nothing(hip_lib):
    """Round 6: the chain plans (q1, q5, q9) at SF=10 on an RCCL group of one whose collectives are ISSUED, from their second run on: a
    replicated table travels as one fixed-capacity chunk behind one all-gather (sdqh_table_partition_pack with one part /
    sdqh_unpack_chunks), the partial groups are folded on the device behind one more (sdqh_xgroupby_partial / _fold) — at most three
    collectives per query, all on device tensors, and the seams say that this is what ran.  Against the single-GPU plan on the same
    tables; then q5 with its chunk bounds cut to two rows: noticed when the result is collected, the chain repeated with exact sizes."""
    import torch
    import torch.distributed as dist
    from sdqlpy_amd import dist as sdist
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29599", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    eng = engine.Engine(hip_lib.context(device=0))
    runner = sdist.DistributedRunner(eng, 0, 1, skip_trivial=False)
    try:
        qs = ("q1", "q5", "q9")
        cols = tpch.columns_for(qs)
        db = tpch.generate(10.0, tables=sorted(cols), columns=cols, shard=(0, 1))
        want = {q: helpers.run_query(eng, q, db) for q in qs}
        want = {q: (r.wait() if hasattr(r, "wait") else r) for q, r in want.items()}
        for q in qs:
            _rows_match(runner.run(q, db), want[q], "settled/%s/first (exact sizes)" % q)
            for again in range(3):
                runner.reset_collectives()
                runner.last_chain = None
                got = runner.run(q, db)
                seams = dict(runner.last_chain or {})
                calls = {k: v[:2] for k, v in runner.collectives.items()}
                _rows_match(got, want[q], "settled/%s/%d" % (q, again))
                assert seams.get("plan") == q, (q, seams)
                assert sum(c[0] for c in calls.values()) <= 3 and all(c[0] == c[1] for c in calls.values()), (q, calls)
                if q == "q9":
                    # (its replicated (part, supplier) table is keyed by pairs that do NOT increase row after row in partsupp — the suppliers of
                    #  a part come in the generator's order — but no pair comes twice, which the library checks once per column pair: the
                    #  stage travels as one chunk.  Its last loop is the fixed-shape lookup kernel, its partial groups left in a device
                    #  block and folded like a program's: sdqh_lookup_aggregate_block, ABI 7)
                    assert seams["replicated"] == ["green_costs"], seams
                assert bool(seams.get("recorded")) == (again == 2), (q, again, seams)      # (two settled runs with the calls issued, then the chain — its collectives inside — is ONE recorded launch)
                if q in ("q1", "q5", "q9"):
                    assert seams["folded"] and not seams["merged_on_host"], (q, seams)
                if q == "q5":
                    assert seams["replicated"] == ["supplier_nations"], seams        # (on a group of one the customers' join is co-partitioned)
        assert runner.fast_runs >= 9 and runner.fast_retries == 0
        assert runner.graph_recordings == 3 and runner.graph_launches == 3, (runner.graph_recordings, runner.graph_launches)
        for again in range(4):                                       # ... and replayed: the same rows from the same recording
            _rows_match(runner.run("q5", db), want["q5"], "settled/q5/replay %d" % again)
            _rows_match(runner.run("q1", db), want["q1"], "settled/q1/replay %d" % again)
        assert runner.graph_recordings == 3 and runner.graph_launches == 11
        fn5, plan5, _ = runner._resolve("q5", db)
        st5 = [st for key, st in plan5.__dict__["_dist_chain"].items() if key[0] == id(runner)][0]
        for name in st5.caps:
            st5.caps[name] = 2
        _rows_match(runner.run("q5", db), want["q5"], "settled/q5/after an overflow")
        assert runner.fast_retries == 1 and all(v > 2 for v in st5.caps.values()), (runner.fast_retries, st5.caps)
        _rows_match(runner.run("q5", db), want["q5"], "settled/q5/settled again")
        assert runner.fast_retries == 1
    finally:
        runner.close()
        torch.cuda.synchronize()
        dist.destroy_process_group()
        eng.close()


def test_recordings_survive_the_collective_watchdog(hip_engine):
    """A recording of a settled distributed plan while torch's collective watchdog polls (tests/dist_record_race_worker.py): in a process
    of its own — what this guards against is a core dump (tools/exp_watchdog_capture.py `same`)."""
    import os
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_record_race_worker.py")
    p = subprocess.run([sys.executable, worker, str(port), "1.0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "ok recordings=" in p.stdout, p.stdout[-4000:]


@pytest.mark.parametrize("world,shuffled", [(2, False), (3, False), (2, True)])
def test_ranks_share_one_gpu(hip_engine, tmp_path, world, shuffled):
    """Round 6: N > 1 ON THE HARDWARE, as far as one GPU allows.  RCCL refuses two ranks on one device, so the ranks talk through gloo and
    the runner's HYBRID mode (sdqlpy_amd/dist.py): collective buffers in pinned host memory that the HIP kernels read and write through
    their device-visible addresses.  Everything but the transport is the N > 1 GPU path: the hash-partitioning pack into `world` chunks,
    chunks of several sources taken apart, replicated tables rebuilt from several ranks' entries, partial groups of several ranks folded
    on the device, bitmaps of several ranks reduced — on `world` processes with a HIP context each.  Every query three times per
    partitioning (exact sizes, then twice settled) against the single-process HIP result on the whole database.  shuffled: every table's
    rows dealt to the ranks at random — overlapping key ranges, nothing co-partitioned: every looked-up build replicated, the join
    hash-partitioned whatever was asked for."""
    import json
    import os
    import socket
    import subprocess
    import sys
    sf = 1.0
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "ranks.json")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_gpu_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), str(sf), out] + (["", "auto", "", "shuffled"] if shuffled else []),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = [p.communicate(timeout=900)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    with open(out) as fh:
        got = json.load(fh)
    qs = ["q6", "q1", "q5", "q9", "q4", "q14", "q3"]
    cols = tpch.columns_for(qs)
    db = tpch.generate(sf, tables=sorted(cols), columns=cols)
    want = {}
    for q in qs:
        r = helpers.run_query(hip_engine, q, db)
        want[q] = r.wait() if hasattr(r, "wait") else r
    n = 0
    for tag, res in got["runs"].items():
        part, q, again = tag.split("/")
        assert "unsupported" not in res, (tag, res)
        if "scalar" in res:
            assert abs(res["scalar"] - want[q]) <= REL * abs(want[q]), (tag, res["scalar"], want[q])
        else:
            helpers.assert_rows_match(sorted(tuple(r) for r in res["rows"]), helpers.result_rows(want[q], res["columns"]), REL, "world %d/%s" % (world, tag))
            if q == "q3":
                assert res["partitioning"] == ("hash" if shuffled else {"hash": "hash", "auto": "range"}[part]), (tag, res["partitioning"])
                if res["partitioning"] == "hash":
                    assert res["exchanged"]["build"] > 30_000 and res["exchanged"]["probe_sent"] > 5_000, (tag, res["exchanged"])
            if q == "q1" and again != "0":
                assert res["seams"].get("plan") == q and res["seams"]["folded"] and not res["seams"]["merged_on_host"], (tag, res["seams"])
            if q == "q5" and again != "0" and not shuffled:
                assert res["seams"].get("plan") == q and res["seams"]["folded"] and not res["seams"]["merged_on_host"], (tag, res["seams"])
                assert "supplier_nations" in res["seams"]["replicated"] and "asian_customers" in res["seams"]["replicated"], (tag, res["seams"])
        n += 1
    # the hash-partitioned join's settled runs: the same BITS (the pack places every row deterministically — round-5 advice — so the received
    # probe rows meet the sink's f64 atomics in the same arrangement run after run)
    # (clustered shards: an order's lines reach the sink in neighbouring lanes and are summed before the one atomic that adds them; dealt at
    #  random they arrive apart, three or more atomics of different waves may add to one group, and no placement fixes THEIR order)
    if not shuffled:
        assert got["runs"]["hash/q3/1"]["rows"] == got["runs"]["hash/q3/2"]["rows"]
    parts = ("auto",) if shuffled else ("hash", "auto")
    assert n == len(parts) * len(qs) * 3
    for part in parts:
        assert got[part]["fast_retries"] == 0 and got[part]["fast_runs"] >= (4 if shuffled else 8), got[part]
    hip_engine.clear()


def test_eight_ranks_share_one_gpu_at_sf100(hip_lib, tmp_path):
    """BASELINE configs[3] and [4] at their GLOBAL size and rank count — TPCH Q3 hash-partitioned on o_orderkey, and the Q5 / Q9 chains, at
    SF=100 over EIGHT ranks — with the eight ranks sharing the one GPU that is here (gloo between the processes, pinned host buffers: the
    runner's hybrid mode; RCCL over xGMI is what an 8-GPU node adds).  Each rank holds an SF=12.5 row shard; every query three times
    (exact sizes, then twice with device-sized exchanges / folded groups) against the single-process plan on the whole SF=100 database:
    Q5 / Q9 row for row, Q3's 1.1 M rows through a digest that adds up over the ranks' key partitions (rows, key / date sums exact,
    revenue to 1e-9).  Every Q5 / Q9 row, and every Q3 group of every rank (the ranks write their rows as .npy files; the union of their
    keys is the reference's key set), also against the exact integer reference (tests/exact_reference.py) under its derived bound.
    Needs ~150 GiB of host memory and ~120 GiB of HBM: fails, not skips, on a box that has them."""
    import json
    import os
    import socket
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dist_gpu_worker
    _need_memory(150, 120, *_MODULE_ENGINES)
    world, sf = 8, 100.0
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "ranks8.json")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_gpu_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), str(sf), out, "q5,q9,q3", "hash", "digest+rows"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = [p.communicate(timeout=1500)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    with open(out) as fh:
        got = json.load(fh)
    eng = engine.Engine(hip_lib.context(device=0))
    try:
        for q in ("q5", "q9", "q3"):
            cols = tpch.columns_for((q,))
            db = tpch.generate(sf, tables=sorted(cols), columns=cols)
            want = helpers.run_query(eng, q, db)
            want = want.wait() if hasattr(want, "wait") else want
            for again in range(3):
                res = got["runs"]["hash/%s/%d" % (q, again)]
                if q == "q3":
                    assert res["partitioning"] == "hash" and res["exchanged"]["build"] > 1_000_000, res["exchanged"]
                    wd, gd = dist_gpu_worker.result_digest(want), res["digest"]
                    assert gd[0] == wd[0] > 1_000_000, (gd[0], wd[0])
                    for name, a, b in zip(want.columns, gd[1:], wd[1:]):
                        assert abs(a - b) <= 1e-9 * max(abs(b), 1.0), (q, again, name, a, b)
                    # every group of every rank against the exact reference, and the union of the ranks' keys against its key set
                    ranks = [{c: np.load(str(tmp_path / ("q3_hash_run%d_rank%d_%s.npy" % (again, r, c)))) for c in res["columns"]} for r in range(world)]
                    assert all(len(rk["l_orderkey"]) > 0 for rk in ranks) and sum(len(rk["l_orderkey"]) for rk in ranks) == wd[0]
                    _close_to_exact_sf100({c: np.concatenate([rk[c] for rk in ranks]) for c in res["columns"]}, q, db, "8 ranks, run %d" % again)
                else:
                    helpers.assert_rows_match(sorted(tuple(r) for r in res["rows"]), helpers.result_rows(want, res["columns"]), REL, "8 ranks/%s/%d" % (q, again))
                    _close_to_exact_sf100(dict(zip(res["columns"], zip(*res["rows"]))), q, db, "8 ranks, run %d" % again)
            eng.clear()
            del db, want
        assert got["hash"]["fast_retries"] == 0 and got["hash"]["fast_runs"] >= 4, got["hash"]
    finally:
        eng.close()


def test_distributed_hash_join_world1_sf100(hip_lib):
    """BASELINE configs[3]'s data size on one device: the hash-partitioned q3 at SF=100 (32-bit offsets in the partitioning pass, a
    75 MB bitmap through the all-reduce, 15 M build rows and 3 M probe rows through the all-to-all of an RCCL group of one), its first
    run with exact sizes and its second with device-sized chunks, against the single-GPU plan.  Skipped — visibly — on a box
    without the memory."""
    import psutil
    import torch
    import torch.distributed as dist
    from sdqlpy_amd import dist as sdist
    _need_memory(96, 120, *_MODULE_ENGINES)
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29595", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    eng = engine.Engine(hip_lib.context(device=0))
    runners = []
    try:
        cols3 = tpch.columns_for(("q3",))
        big = tpch.generate(100.0, tables=sorted(cols3), columns=cols3, shard=(0, 1))
        single = helpers.run_query(eng, "q3", big).wait()
        runner = sdist.DistributedRunner(eng, 0, 1, partition="hash", skip_trivial=False)
        runners.append(runner)
        import bench
        for again in range(2):
            got = runner.run("q3", big)
            assert got.size() == single.size() > 1_000_000
            cmp = bench.compare_results(got.wait() if hasattr(got, "wait") else got, single)
            assert cmp["rows_equal"] and cmp["max_rel"] <= REL, cmp
            assert runner.exchanged_rows["build"] > 10_000_000
            _close_to_exact_sf100(got, "q3", big, "distributed hash join, world 1, run %d" % again)
        assert runner.fast_runs == 1 and runner.fast_retries == 0
    finally:
        for obj in runners:
            obj.close()
        torch.cuda.synchronize()
        dist.destroy_process_group()
        eng.close()


def test_sf100_on_one_gpu_q5_q9(hip_engine, oracle_lib):
    """BASELINE configs[4]'s data size (Q5 / Q9 at SF=100) on ONE device: totals against numpy reductions of the same columns where the
    query allows, additivity over a split of lineitem at an odd row group by group, a second run identical.  Every group of both queries
    against the exact integer reference under its derived bound, and against the CPU implementation on the same tables at REL."""
    import psutil
    import torch
    _need_memory(150, 150, *_MODULE_ENGINES)
    for q in ("q5", "q9"):
        cols = tpch.columns_for((q,))
        db = tpch.generate(100, tables=sorted(cols), columns=cols)
        li = db["lineitem"].getContainer()
        n = len(li["data"][0])
        assert n > 599_000_000
        whole = helpers.run_query(hip_engine, q, db)
        whole = whole.wait() if hasattr(whole, "wait") else whole
        assert whole.size() > 0
        _close_to_exact_sf100(whole, q, db, "HIP")
        _cpu_leg_sf100(oracle_lib, whole, q, db)
        again = helpers.run_query(hip_engine, q, db)
        _rows_match(again, whole, "sf100/%s/again" % q)                  # (group sums through LDS atomics: the order of the adds is not fixed)
        value_cols = [c for c in whole.columns if whole.column(c).dtype.kind == "f"]
        key_cols = [c for c in whole.columns if c not in value_cols]
        cut = n // 2 + 333
        sums = {}
        for lo, hi in ((0, cut), (cut, n)):
            part = dict(db)
            part["lineitem"] = tpch.table_from_columns(li["headers"], [c[lo:hi] for c in li["data"]])
            r = helpers.run_query(hip_engine, q, part)
            for row in zip(*[r.column(c).tolist() for c in key_cols + value_cols]):
                k, v = row[:len(key_cols)], row[len(key_cols):]
                sums[k] = [a + b for a, b in zip(sums.get(k, [0.0] * len(v)), v)]
            hip_engine.invalidate(part["lineitem"])
        want = {row[:len(key_cols)]: row[len(key_cols):] for row in zip(*[whole.column(c).tolist() for c in key_cols + value_cols])}
        assert sums.keys() == want.keys(), q
        for k, v in want.items():
            for a, b in zip(sums[k], v):
                assert abs(a - b) <= 1e-9 * max(abs(a), abs(b), 1.0), (q, k, a, b)
        hip_engine.clear()
        del db, li, whole, again


@pytest.mark.gpu
def test_distributed_chain_world1_sf100(hip_lib):
    """BASELINE configs[4] on what is here: Q5 and Q9 at SF=100 through the DISTRIBUTED chain plan (builds over sharded tables
    replicated — entries all-gathered on the device, key sets as bitmaps — the co-partitioned orders <-> lineitem join local, partial
    groups merged) on an RCCL group of ONE whose collectives are ISSUED, against the single-GPU plan on the same tables.  Eight GPUs
    are not here; the same plan at world 2 / 4 on gloo is tests/test_dist_cpu.py.  Skipped — visibly — on a box without the memory."""
    import psutil
    import torch
    import torch.distributed as dist
    from sdqlpy_amd import dist as sdist
    _need_memory(110, 150, *_MODULE_ENGINES)
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29597", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    eng = engine.Engine(hip_lib.context(device=0))
    runner = sdist.DistributedRunner(eng, 0, 1, skip_trivial=False)
    try:
        for q in ("q5", "q9"):
            cols = tpch.columns_for((q,))
            db = tpch.generate(100, tables=sorted(cols), columns=cols, shard=(0, 1))
            assert len(db["lineitem"].getContainer()["data"][0]) > 599_000_000 and db["lineitem"].shard == (0, 1)
            single = helpers.run_query(eng, q, db)
            single = single.wait() if hasattr(single, "wait") else single
            runner.reset_collectives()
            for again in range(2):
                got = runner.run(q, db)
                _rows_match(got, single, "sf100 distributed chain/%s/%d" % (q, again))
                _close_to_exact_sf100(got, q, db, "distributed chain, world 1, run %d" % again)
            assert runner.collectives.get("all_gather", [0, 0])[1] > 0, runner.collectives      # replicas and partial groups really travelled, on device tensors
            eng.clear()
            del db, single, got
    finally:
        runner.close()
        torch.cuda.synchronize()
        dist.destroy_process_group()
        eng.close()


@pytest.mark.gpu
def test_lanes_give_the_rows_one_stream_gives(hip_lib):
    """Round 4: an engine runs its plans on three lanes — contexts of one family (sdqh_fork), a stream, a pool and result blocks each,
    the resident columns shared — so that queries launched together share the chip.  Seven queries in flight at once, round after
    round, against one lane: the same rows (sums within REL: atomics order); with the tight encodings on at every size the twins and
    dictionaries are built by whichever lane first needs them and used by the others; at SF=1 the kernels are long enough to
    overlap for real."""
    assert helpers.lanes_case(hip_lib, sf=0.05, rounds=6, rel=REL) == {0, 1, 2}
    assert helpers.lanes_case(hip_lib, sf=0.05, rounds=6, rel=REL, tight=True) == {0, 1, 2}
    assert helpers.lanes_case(hip_lib, sf=1.0, rounds=8, rel=REL, queries=("q1", "q3", "q5", "q9", "q18", "q10")) == {0, 1, 2}


@pytest.mark.gpu
def test_plan_graphs_give_the_rows_the_calls_give(hip_lib):
    """Round 5: a settled plan whose last call is deferred is recorded into a graph (sdqh_graph_begin / _end: HIP stream capture; the
    memory its calls allocate stays with the recording) and launched by one call from then on.  Same rows as the calls give, with
    several results of a query in flight, results dropped unread, an option flipped, the columns re-uploaded; plans that wait for
    the device in the middle (q6's scalar, q9's ... none of the configured ones' LAST loops, but q18's HAVING size read-back) are
    refused once and keep issuing their calls."""
    stats = helpers.plan_graphs_case(hip_lib, sf=0.05, rounds=8, rel=REL)
    assert stats["recorded"] >= 6 and stats["launched"] >= 20, stats
    big = helpers.plan_graphs_case(hip_lib, sf=1.0, rounds=6, rel=REL, queries=("q1", "q3", "q5", "q9", "q10"))
    assert big["recorded"] >= 4 and big["launched"] >= 12, big


@pytest.mark.gpu
def test_grouped_layout_for_composite_keys(hip_engine, oracle_engine):
    """Round 4: a composite-key build over a table stored in the order of the key's first part gets the GROUPED layout (one stage row
    per first-part value, written while staging; a lookup walks the run): against numpy inside the helper and against the CPU
    implementation's digest, with the layout on and off, at sizes where runs cross wave segments, with almost every row filtered
    out (single-entry segments, empty segments), with one row per first part, and with the tight encodings forced on."""
    ctx = hip_engine.ctx
    cases = [dict(n=200000, nprobe=500000), dict(n=2000003, nprobe=3000000, seed=5, keep=0.05), dict(n=70001, nprobe=100000, keep=0.002, per_a=1),
             dict(n=300, nprobe=1000, keep=0.9, per_a=50), dict(n=1000000, nprobe=1000000, seed=9, keep=1.0, per_a=2000),
             dict(n=51200, nprobe=100000, seed=3, keep=1.0, per_a=3), dict(n=512, nprobe=2000, seed=4, keep=1.0, per_a=600)]      # (every segment full, the last one too)
    try:
        for kw in cases:
            want = helpers.grouped_index_case(oracle_engine.ctx, **kw)
            for grouped in (1, 0):
                ctx.set_option("grouped_index", grouped)
                assert helpers.grouped_index_case(ctx, **kw) == want, (kw, grouped)
        ctx.set_option("grouped_index", 1)
        ctx.set_option("feature_min_rows", 0)
        assert helpers.grouped_index_case(ctx, **cases[0]) == helpers.grouped_index_case(oracle_engine.ctx, **cases[0])
    finally:
        ctx.set_option("grouped_index", 1)
        ctx.set_option("feature_min_rows", 1 << 20)


@pytest.mark.gpu
def test_row_pack_clustered_by_the_first_lookups_key(hip_engine, oracle_engine):
    """Round 5: Q9's loop shape with its row pack in the order of the first lookup's key (stable radix order of the unordered probe
    key: sdqh_aux.hip) against numpy (inside the helper), against the CPU implementation, and against the pack in row order — same
    groups and counts, sums to 1e-10; sizes around the sort's
    wave tile (4096 rows) and the loop's tile, one row, keys spanning one and three radix digits."""
    ctx = hip_engine.ctx
    cases = [dict(), dict(nprobe=4096), dict(nprobe=4097, seed=2), dict(nprobe=1, seed=3), dict(nprobe=65, seed=4), dict(nprobe=1 << 20, seed=5, nparts=200),
             dict(n=400000, nprobe=2000003, seed=6, nparts=90000, keep=0.05), dict(nprobe=70001, seed=7, nparts=70000, n=70000, keep=0.5)]
    try:
        ctx.set_option("feature_min_rows", 0)
        for kw in cases:
            want = helpers.cluster_pack_case(oracle_engine.ctx, **kw)
            runs = {}
            for cluster in (1, 0, 1):
                ctx.set_option("cluster_pack", 2 * cluster)              # (2: also where the probe key is short or near-sorted by chance)
                ctx.set_profiling(True); ctx.kernel_log = []
                got = helpers.cluster_pack_case(ctx, **kw)
                names = [k for k, _ in ctx.kernel_log]
                ctx.set_profiling(False)
                clustered = bool(cluster) and kw.get("nprobe", 2) >= 2            # (one row has no twin, so no order to be put in)
                assert ("k_rs_scatter" in names) == clustered and ("k_interleave_perm" in names) == clustered, (kw, cluster, names)
                assert ("k_interleave" in names) == (not clustered), (kw, cluster, names)
                assert got[0] == want[0] and got[1] == want[1], (kw, cluster)
                assert all(abs(x - y) <= REL * max(abs(y), 1.0) for x, y in zip(got[2], want[2])), (kw, cluster)
                runs[cluster] = got                                      # (group sums are LDS atomics of many waves: their last bits are not pinned in any order)
    finally:
        ctx.set_option("cluster_pack", 1)
        ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()


@pytest.mark.gpu
def test_driven_walk_of_loops_keyed_by_the_stored_order(hip_engine, oracle_engine):
    """Round 5: a final loop whose first lookup is keyed by the column its table is stored in the order of (Q5: l_orderkey against the
    orders of one year and region) walks the looked-up table's KEYS and their row runs (the column's run index) instead of streaming
    the column, when the table holds few of the keys (x_queue8's driven walk, option "x_driven": 0 never, 1 whenever the table has
    fewer keys than the loop rows, 64 the default ratio).  Same rows as the CPU implementation either way — at sizes where the walk is
    and is not chosen, with the lineitem rows cut around wave / step boundaries (runs cut in the middle, the last run ending at the
    last row), and for the other configured queries with the option at its most eager."""
    ctx = hip_engine.ctx
    try:
        ctx.set_option("feature_min_rows", 0)
        for sf in (0.02, 0.3):
            db = tpch.generate(sf, tables=sorted(tpch.columns_for(SUPPORTED)), columns=tpch.columns_for(SUPPORTED))
            want = {q: helpers.run_query(oracle_engine, q, db) for q in ("q5", "q9", "q3")}
            for ratio in (1, 0, 64):
                ctx.set_option("x_driven", ratio)
                hip_engine.clear()
                ctx.set_profiling(True); ctx.kernel_log = []
                for q in ("q5", "q9", "q3"):
                    for _ in range(2):
                        got = helpers.run_query(hip_engine, q, db)
                        helpers.assert_rows_match(helpers.result_rows(got, want[q].columns), helpers.result_rows(want[q], want[q].columns), REL, "sf=%s x_driven=%d %s" % (sf, ratio, q))
                names = [k for k, _ in ctx.kernel_log]
                ctx.set_profiling(False)
                assert "xk_group_tight" in names, (sf, ratio, sorted(set(names)))      # (Q5's final loop: the skeleton that has the walk)
            oracle_engine.clear()
        ctx.set_option("x_driven", 1)
        base = tpch.generate(0.01, tables=sorted(tpch.columns_for(SUPPORTED)), columns=tpch.columns_for(SUPPORTED))
        li = base["lineitem"].getContainer()
        total = len(li["data"][0])
        for n in [0, 1, 2, 7, 8, 9, 63, 65, 511, 513, 1023, 1025, 4097, 8191, 20001, total - 1, total]:
            db = dict(base)
            db["lineitem"] = tpch.table_from_columns(li["headers"], [np.ascontiguousarray(c[:n]) for c in li["data"]])
            got = helpers.run_query(hip_engine, "q5", db)
            wantq = helpers.run_query(oracle_engine, "q5", db)
            helpers.assert_rows_match(helpers.result_rows(got, wantq.columns), helpers.result_rows(wantq, wantq.columns), REL, "n=%d/q5 driven" % n)
    finally:
        ctx.set_option("x_driven", 64)
        ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()
        oracle_engine.clear()


@pytest.mark.gpu
def test_delta_twins_change_no_bit(hip_engine, oracle_engine):
    """Round 5: a queue program streams its prefilter's key column — a key the table is stored in the order of (l_orderkey, o_orderkey) —
    through its DELTA twin: 12 bytes per aligned group of 8 rows (the group's smallest value and eight one-byte offsets), verified
    group by group when built.  The rows a loop meets and their order do not depend on the encoding, so q3 (its probe streams l_orderkey
    that way) returns the SAME bits with the option off, q4 / q10 / q12 the same rows; a key column whose groups span more than 255
    somewhere keeps its 4-byte twin (orders cut out of the middle: one group straddles the gap) and nothing changes either; sizes
    around the 8-row group and the skeleton's 512-row step."""
    ctx = hip_engine.ctx
    qs = ["q3", "q4", "q10", "q12", "q5"]
    db = tpch.generate(1.0, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))

    def run_all(database, names):
        out = {}
        for q in names:
            r = helpers.run_query(hip_engine, q, database)
            out[q] = helpers.result_rows(r, r.columns)
        return out
    try:
        ctx.set_option("delta8", 1)
        hip_engine.clear()
        on = run_all(db, qs)
        ctx.set_option("delta8", 0)
        hip_engine.clear()
        off = run_all(db, qs)
        assert on["q3"] == off["q3"]
        for q in qs:
            helpers.assert_rows_match(on[q], off[q], 1e-12, "delta twins/" + q)
        want = helpers.run_query(oracle_engine, "q3", db)
        helpers.assert_rows_match(on["q3"], helpers.result_rows(want, want.columns), REL, "delta twins/q3 against the CPU implementation")
        # a gap in the key: the lineitems of the orders 200 001 .. 4 000 000 removed — the group that straddles the gap spans millions
        li = db["lineitem"].getContainer()
        ok = li["data"][li["headers"].index("l_orderkey")]
        keep = (ok <= 200000) | (ok > 4000000)
        ctx.set_option("feature_min_rows", 0)
        for n in (None, 7, 8, 9, 511, 513, 4097):
            cols = [np.ascontiguousarray(c[keep] if n is None else c[:n]) for c in li["data"]]
            cut = dict(db)
            cut["lineitem"] = tpch.table_from_columns(li["headers"], cols)
            ctx.set_option("delta8", 1)
            hip_engine.clear()
            a = run_all(cut, ["q3"])
            ctx.set_option("delta8", 0)
            hip_engine.clear()
            b = run_all(cut, ["q3"])
            assert a == b, n
            w = helpers.run_query(oracle_engine, "q3", cut)
            helpers.assert_rows_match(a["q3"], helpers.result_rows(w, w.columns), REL, "delta twins/cut %r" % (n,))
    finally:
        ctx.set_option("delta8", 1)
        ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()
        oracle_engine.clear()


@pytest.mark.gpu
def test_word_pairs_of_the_rank_is_row_layout(hip_engine, oracle_engine):
    """Whole-table builds keyed by a strictly increasing column over a wide range (Q9's orders) may keep { first row, bits } pairs per bitmap
    word beside the bitmap and the row-per-word array, so that a lookup's two requests are one line (option "word_pairs", off by default:
    what the final loop gains the build loses).  Same rows as the CPU implementation with the pairs on — at a size where the layout is
    chosen by itself and, with `feature_min_rows` 0, on small and ragged tables where waves share boundary words."""
    ctx = hip_engine.ctx
    qs = ("q9", "q5", "q3")
    try:
        ctx.set_option("word_pairs", 1)
        for sf, fmr in ((2.0, 1 << 20), (0.03, 0), (0.3, 0)):
            ctx.set_option("feature_min_rows", fmr)
            hip_engine.clear()
            db = tpch.generate(sf, tables=sorted(tpch.columns_for(qs)), columns=tpch.columns_for(qs))
            for q in qs:
                want = helpers.run_query(oracle_engine, q, db)
                for _ in range(2):
                    got = helpers.run_query(hip_engine, q, db)
                    helpers.assert_rows_match(helpers.result_rows(got, want.columns), helpers.result_rows(want, want.columns), REL, "word pairs sf=%s %s" % (sf, q))
            oracle_engine.clear()
    finally:
        ctx.set_option("word_pairs", 0)
        ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()


@pytest.mark.gpu
def test_delta_twins_and_walks_on_awkward_key_columns(hip_engine, oracle_engine):
    """The ABI-level loop `if set[key] != None: out[g] += v` over key columns chosen against the round's encodings and walks: negative
    keys, keys next to the int32 limits (a delta twin's base + offset must not wrap), groups of 8 rows that are narrow but not in order
    (the base is the group's SMALLEST value), one group 256 wide (no delta twin: the 4-byte twin serves), runs longer than a wave's 8-row
    rounds (thousands of rows of one key), keys the set holds that the column does not and the other way round, a set of ONE key, a set of
    every key, row counts off the 8-row and 512-row grids — with the walk at its most eager, at its default, and off; numpy inside the
    helper, the CPU implementation beside."""
    ctx = hip_engine.ctx
    rng = np.random.default_rng(41)

    def runs(values, lens):
        return np.repeat(np.asarray(values, np.int64), np.asarray(lens, np.int64))
    n = 300007
    sorted_keys = np.sort(rng.integers(-5000, 200000, n)).astype(np.int64)
    cases = [
        ("negative, in order", sorted_keys, rng.choice(np.unique(sorted_keys), 900, replace=False)),
        ("next to the upper int32 limit", np.repeat(np.arange(2**31 - 40002, 2**31 - 1, dtype=np.int64), 3), np.array([2**31 - 2, 2**31 - 40002, 2**31 - 20000, 2**31 - 9], np.int64)),
        ("next to the lower int32 limit", np.repeat(np.arange(-2**31 + 1, -2**31 + 40001, dtype=np.int64), 2), np.array([-2**31 + 1, -2**31 + 7, -2**31 + 40000], np.int64)),
        ("narrow groups, not in order", (np.arange(n, dtype=np.int64) // 8) * 200 + rng.integers(0, 200, n), np.arange(0, n * 25, 1013, dtype=np.int64)),
        ("one group 256 wide", np.where(np.arange(n) == 4011, 4011 // 8 * 200 + 256 + 255, (np.arange(n, dtype=np.int64) // 8) * 200 + rng.integers(0, 56, n)), np.arange(0, n * 25, 511, dtype=np.int64)),
        ("long runs", runs(np.arange(10, 10 + 60) * 3, rng.integers(1, 9000, 60)), np.array([10 * 3, 11 * 3, 40 * 3, 69 * 3, 5, 1000], np.int64)),
        ("a set of one key", sorted_keys, np.array([int(sorted_keys[n // 2])], np.int64)),
        ("a set of every key", sorted_keys[:70001], np.unique(sorted_keys[:70001])),
        ("seven rows", np.arange(7, dtype=np.int64) * 2, np.array([0, 4, 12, 13], np.int64)),
        ("513 rows", np.arange(513, dtype=np.int64) // 3, np.arange(0, 171, 7, dtype=np.int64)),
    ]
    try:
        ctx.set_option("feature_min_rows", 0)
        for name, keys, members in cases:
            want = helpers.keyed_probe_case(oracle_engine.ctx, keys, members)
            for ratio, d8 in ((1, 1), (64, 1), (0, 1), (0, 0)):
                ctx.set_option("x_driven", ratio); ctx.set_option("delta8", d8)
                got = helpers.keyed_probe_case(ctx, keys, members)
                assert got[0] == want[0] and got[1] == want[1], (name, ratio, d8)
                assert all(abs(x - y) <= REL * max(abs(y), 1.0) for x, y in zip(got[2], want[2])), (name, ratio, d8)
    finally:
        ctx.set_option("x_driven", 64); ctx.set_option("delta8", 1)
        ctx.set_option("feature_min_rows", 1 << 20)
        hip_engine.clear()
