"""tests/exact_reference.py pinned: the exact integer results of q1 / q3 / q5 / q6 / q9 against the reference's own results (the goldens
at SF=1 and SF=10) and against the CPU implementation, chunked against unchunked, and the comparator against corrupted results it must
reject.  Runs without a GPU; the SF=100 tests of tests/test_hip_parity.py use the same module on the GPU box."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_reference as X
import helpers
from sdqlpy_amd import engine, tpch

REL = 1e-10                                              # tests/test_hip_parity.py's figure for HIP against the CPU implementation
ODD_CHUNK = 100_003                                      # a multiple of nothing: seams fall inside key runs


def _generate(sf, qs=X.QUERIES):
    cols = tpch.columns_for(qs)
    return tpch.generate(sf, tables=sorted(cols), columns=cols, threads=4)


@pytest.fixture(scope="module")
def cpu_engine(oracle_lib):
    eng = engine.Engine(oracle_lib.context(threads=4))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def db037():
    return _generate(0.37)


@pytest.fixture(scope="module")
def exact037(db037):
    return X.exact_results(db037, X.QUERIES)


def _against_golden(case, qs, chunk_rows=X.DEFAULT_CHUNK_ROWS):
    db = helpers.case_db(case)
    exact = X.exact_results(db, qs, chunk_rows)
    worst = {}
    for q in qs:
        gold = case["results"][q]
        got = helpers.dec(gold["value"]) if gold["kind"] == "scalar" else gold
        worst[q] = X.assert_close_to_exact(got, exact[q], "%s/%s" % (case["name"], q))
        assert exact[q].size() > 0 and worst[q] <= 1.0
    return exact, worst


def test_exact_results_against_the_reference_at_sf1(golden_sf1):
    """The reference's own q1 / q3 / q5 / q6 / q9 at SF=1: keys and counts exact, every value of every group inside the derived bound,
    one-row groups bit for bit (11 301 q3 groups of at most 7 rows: the bound is a few ulps there)."""
    case = next(c for c in golden_sf1["cases"] if c["name"] == "sf1")
    exact, worst = _against_golden(case, X.QUERIES)
    assert exact["q3"].size() > 10_000 and exact["q3"].one_row_groups() > 1000
    assert int(np.max(exact["q3"].m)) <= 7 and exact["q6"].m[0] > 100_000
    assert sum(exact["q1"].m) == sum(exact["q1"].counts["count_order"]) > 5_800_000


def test_exact_results_against_the_reference_at_sf10(golden_sf10):
    """The same at BASELINE.json's size, for the queries the SF=10 golden file holds."""
    (case,) = golden_sf10["cases"]
    qs = tuple(q for q in X.QUERIES if q in case["results"])
    assert len(qs) >= 3
    try:
        exact, worst = _against_golden(case, qs)
        if "q3" in qs:
            assert exact["q3"].size() > 100_000
    finally:
        helpers._db_cache.clear()                                # (5 GB of generated columns: not kept for the rest of the session)


@pytest.mark.parametrize("sf", [0.37, 1.3])
def test_exact_results_against_the_cpu_implementation(cpu_engine, sf):
    """The CPU implementation at two odd scale factors: inside the derived bound of the exact result, group by group."""
    db = _generate(sf)
    exact = X.exact_results(db, X.QUERIES)
    for q in X.QUERIES:
        got = helpers.run_query(cpu_engine, q, db)
        assert X.assert_close_to_exact(got, exact[q], "cpu/sf%s/%s" % (sf, q)) <= 1.0
    cpu_engine.clear()


def _same(a, b):
    assert a.query == b.query and list(a.keys) == list(b.keys) and list(a.values) == list(b.values)
    for k in a.keys:
        assert np.array_equal(np.asarray(a.keys[k]), np.asarray(b.keys[k])), (a.query, k)
    assert np.array_equal(np.asarray(a.m), np.asarray(b.m)) and a.counts == b.counts
    for name in a.values:
        va, vb = a.values[name], b.values[name]
        assert va["D"] == vb["D"]
        for f in ("N", "S", "plain"):
            assert np.asarray(va[f]).tolist() == np.asarray(vb[f]).tolist(), (a.query, name, f)


def test_chunked_results_equal_unchunked_ones(db037, exact037):
    """Seams of a 100 003-row chunking fall inside q3's key runs and inside every group of the other queries; one chunk holds all rows."""
    n = len(X.columns(db037["lineitem"])["l_orderkey"])
    chunked = X.exact_results(db037, X.QUERIES, chunk_rows=ODD_CHUNK)
    whole = X.exact_results(db037, X.QUERIES, chunk_rows=n)
    ok = X.columns(db037["lineitem"])["l_orderkey"]
    seams = np.arange(ODD_CHUNK, n, ODD_CHUNK)
    assert len(seams) > 10 and np.count_nonzero(ok[seams] == ok[seams - 1]) > 5
    for q in X.QUERIES:
        _same(chunked[q], whole[q])
        _same(exact037[q], whole[q])


def _fma(a, b, c):
    """a * b + c with one rounding."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))            # (int / int true division rounds correctly)


def _without_row(db, row):
    c = db["lineitem"].getContainer()
    out = dict(db)
    out["lineitem"] = tpch.table_from_columns(c["headers"], [np.delete(a, row) for a in c["data"]])
    return out


def _rejected(got, exact, what):
    with pytest.raises(AssertionError):
        X.assert_close_to_exact(got, exact, what)


def test_the_comparator_rejects_corrupted_results(cpu_engine, db037, exact037):
    """Each corruption a kernel or a plan could produce at a seam, a tile edge or through a fused multiply-add, and the leg that catches it.
    The clean result passes first, so that a rejection is the corruption's."""
    li = X.columns(db037["lineitem"])
    clean = {q: helpers.run_query(cpu_engine, q, db037) for q in ("q1", "q3", "q5")}
    clean = {q: X.as_columns(r) for q, r in clean.items()}
    for q in clean:
        assert X.assert_close_to_exact(clean[q], exact037[q], q) <= 1.0
    e3 = exact037["q3"]
    keys3, m3 = e3.keys["l_orderkey"], np.asarray(e3.m)
    in_q3 = (li["l_shipdate"] > 19950315) & np.isin(li["l_orderkey"], keys3)

    # one row dropped from a large group: the count says so (and the sums: one row of 2e5 is far outside (m + 6) ulps)
    row = int(np.flatnonzero(li["l_shipdate"] <= 19980902)[12345])
    assert min(exact037["q1"].m) > 10_000
    short = _without_row(db037, row)
    _rejected(helpers.run_query(cpu_engine, "q1", short), exact037["q1"], "q1 without one row")
    got = dict(clean["q1"])
    got["count_order"] = np.asarray(got["count_order"]).copy()
    got["count_order"][0] -= 1
    _rejected(got, exact037["q1"], "q1 with one count less")

    # one row dropped from a q3 group of several rows
    key = int(keys3[np.flatnonzero(m3 >= 3)[7]])
    row = int(np.flatnonzero(in_q3 & (li["l_orderkey"] == key))[1])
    _rejected(helpers.run_query(cpu_engine, "q3", _without_row(db037, row)), e3, "q3 without one row")
    cpu_engine.clear()

    # one one-row q3 group computed as fma(p, -d, p): one rounding instead of two, a last-bit difference the bound alone would let through
    order = np.argsort(np.asarray(clean["q3"]["l_orderkey"]), kind="stable")
    rev = np.asarray(clean["q3"]["revenue"], np.float64)
    fused = 0
    for g in np.flatnonzero(m3 == 1):
        (row,) = np.flatnonzero(in_q3 & (li["l_orderkey"] == keys3[g]))
        p, d = float(li["l_extendedprice"][row]), float(li["l_discount"][row])
        assert rev[order[g]] == p * (1.0 - d)
        f = _fma(p, -d, p)
        if f != p * (1.0 - d):
            got = dict(clean["q3"])
            got["revenue"] = rev.copy()
            got["revenue"][order[g]] = f
            assert abs(Fraction(f) - Fraction(int(e3.values["revenue"]["N"][g]), 10 ** 4)) <= X.bound_of(1, int(e3.values["revenue"]["S"][g]), 10 ** 4)
            _rejected(got, e3, "q3 with one fused row")
            fused += 1
            if fused == 3:
                break
    assert fused == 3

    # a group's sum in which the last row before a chunk seam is counted twice
    # (few of the 100 003-row seams cut a q3 run at this size, so the chunk size is chosen to put its first seam inside one; the
    #  exact reference itself, chunked there, still gives the unchunked result)
    inside = np.flatnonzero(in_q3[1:] & in_q3[:-1] & (li["l_orderkey"][1:] == li["l_orderkey"][:-1])) + 1
    s = int(inside[len(inside) // 2])
    assert s > 100_000 and s % 2 ** 10
    _same(X.q3(db037, chunk_rows=s), e3)
    g = int(np.searchsorted(keys3, li["l_orderkey"][s]))
    twice = int(e3.values["revenue"]["N"][g]) + int(X.cents(li["l_extendedprice"][s - 1:s])[0] * (100 - X.cents(li["l_discount"][s - 1:s])[0]))
    got = dict(clean["q3"])
    got["revenue"] = rev.copy()
    got["revenue"][order[g]] = twice / 1e4
    _rejected(got, e3, "q3 with a seam row counted twice")

    # a q5 group sum off by 1e-9 relative.  At this size (m of a few hundred rows) the derived bound rejects it, as does REL against the
    # CPU implementation.  The bound grows with m: for the same group with every row repeated k times until m is 10^8 (the exact result
    # is N*k, S*k, m*k) it is about 1e-8 relative and lets 1e-9 through — REL against the CPU implementation does not.  That is why the
    # SF=100 tests keep both legs: q1's groups there hold 10^7 - 10^8 rows.
    e5 = exact037["q5"]
    names = list(clean["q5"]["n_name"])
    name = e5.keys["n_name"][0]
    i = names.index(name)
    value = float(clean["q5"]["revenue"][i])
    got = dict(clean["q5"])
    got["revenue"] = np.asarray(got["revenue"], np.float64).copy()
    got["revenue"][i] = value * (1.0 + 1e-9)
    assert abs(got["revenue"][i] - value) > REL * abs(value)
    _rejected(got, e5, "q5 off by 1e-9")
    k = 10 ** 8 // e5.m[0] + 1
    v = e5.values["revenue"]
    repeated = X.Exact("q5", {"n_name": [name]}, [e5.m[0] * k], {"revenue": {"N": [v["N"][0] * k], "S": [v["S"][0] * k], "D": v["D"], "plain": [None]}})
    big = float(Fraction(v["N"][0] * k, v["D"]))
    assert X.assert_close_to_exact({"n_name": [name], "revenue": [big]}, repeated, "q5 repeated") <= 1.0
    off = big * (1.0 + 1e-9)
    assert 0.01 < X.assert_close_to_exact({"n_name": [name], "revenue": [off]}, repeated, "q5 repeated, off by 1e-9") <= 1.0
    assert abs(off - big) > REL * abs(big)
