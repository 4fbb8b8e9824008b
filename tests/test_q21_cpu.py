"""TPCH q21 and the loop shape only it uses: dictionaries of sets, `{key: vector({value})}` read back as `dictSize(tbl[key])`.

Everything here runs without a GPU: the front end, the generator's o_orderstatus, and the executor's GENERIC route on the CPU
implementation of the ABI, which does not have the run-aware row-program operation (SDQH_X_RUNNEW) and says so with
SDQH_ERR_UNSUPPORTED — the refusal that moves the engine from its fast route to the generic one.  Expected rows come from the
reference itself (tests/golden/make_golden_q21.py), whose Python mode keeps vectors as sets.
"""
import collections
import json
import os

import numpy as np
import pytest

import helpers
from sdqlpy_amd import abi, engine, frontend, tpch
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.sdql_lib import *      # noqa: F401,F403
from sdqlpy_amd.tpch import lineitem_type

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden_q21():
    with open(os.path.join(ROOT, "tests", "golden", "tpch_golden_q21.json")) as fh:
        return json.load(fh)


@pytest.fixture()
def oracle_engine(oracle_lib):
    eng = engine.Engine(oracle_lib.context(threads=8))
    yield eng
    eng.close()


def _small_db():
    return tpch.generate(0.01, tables=["lineitem", "nation", "orders", "supplier"], columns=tpch.columns_for(["q21"]), threads=4)


# ---- generator -----------------------------------------------------------------------------------------------------------
def test_orderstatus_only_when_named():
    """generate() without `columns`, and every column list that does not name it, return what they returned before the column existed."""
    plain = tpch.generate(0.001, tables=["orders"])["orders"].getContainer()["headers"]
    assert plain == ["o_orderkey", "o_custkey", "o_totalprice", "o_orderdate", "o_orderpriority", "o_shippriority", "o_comment"]
    assert "o_orderstatus" not in tpch.columns_for([q for q in tpch.QUERY_COLUMNS if q != "q21"]).get("orders", [])
    assert tpch.columns_for(["q21"])["orders"] == ["o_orderkey", "o_orderstatus"]
    assert tpch.QUERY_COLUMNS["q21"] == {"supplier": ["s_suppkey", "s_name", "s_nationkey"], "lineitem": ["l_orderkey", "l_suppkey", "l_commitdate", "l_receiptdate"],
                                         "orders": ["o_orderkey", "o_orderstatus"], "nation": ["n_nationkey", "n_name"]}
    named = tpch.generate(0.001, tables=["orders"], columns={"orders": ["o_orderkey", "o_orderstatus"]})["orders"].getContainer()
    assert named["headers"] == ["o_orderkey", "o_orderstatus"]


def test_orderstatus_follows_the_lines(tmp_path):
    """Derived from o_orderdate so that it agrees with dbgen's rule on the generator's own lineitem: every line of an 'F' order is 'F',
    every line of an 'O' order 'O', and every order with lines of both kinds is 'P'; about half 'F' and a few per cent 'P'; the same
    for the same seed; written to text as it is."""
    cols = {"orders": ["o_orderkey", "o_orderstatus", "o_orderdate"], "lineitem": ["l_orderkey", "l_linestatus"]}
    db = tpch.generate(0.01, tables=["orders", "lineitem"], columns=cols)
    again = tpch.generate(0.01, tables=["orders"], columns=cols)
    status = tpch.column(db["orders"], "o_orderstatus")
    assert (status == tpch.column(again["orders"], "o_orderstatus")).all()
    shipped = collections.defaultdict(set)
    for k, s in zip(tpch.column(db["lineitem"], "l_orderkey").tolist(), tpch.column(db["lineitem"], "l_linestatus").tolist()):
        shipped[k].add(s)
    mixed = 0
    for k, s in zip(tpch.column(db["orders"], "o_orderkey").tolist(), status.tolist()):
        lines = shipped[k]
        assert lines == {s} if s in "FO" else lines <= {"F", "O"}, (k, s, lines)      # (an order dated inside the window CAN ship all its lines on one side)
        mixed += len(lines) == 2
        assert s == "P" or len(lines) == 1
    assert mixed > 0
    share = {c: float((status == c).mean()) for c in "FOP"}
    assert 0.4 < share["F"] < 0.6 and 0.01 < share["P"] < 0.1 and abs(sum(share.values()) - 1.0) < 1e-12, share
    path = tpch.write_tbl(str(tmp_path), {"orders": db["orders"]})["orders"]
    with open(path) as fh:
        written = [line.split("|")[2] for line in fh]
    assert written == status.tolist()


# ---- front end -----------------------------------------------------------------------------------------------------------
def test_q21_lowers_to_distinct_ops():
    plan = frontend.lower_function(Q.QUERIES["q21"])
    distinct = [op for op in plan.ops if isinstance(op, frontend.DistinctOp)]
    assert [op.out for op in distinct] == ["suppliers_of_order", "late_suppliers_of_order"]
    assert all(op.table == "lineitem" and repr(op.key) == "Col(l_orderkey)" and repr(op.value) == "Col(l_suppkey)" for op in distinct)
    assert distinct[0].conds == [] and repr(distinct[1].conds) == "[(Col(l_receiptdate) > Col(l_commitdate))]"
    final = [op for op in plan.ops if isinstance(op, frontend.ScanOp)][-1]
    counts = [c.left for c in final.conds if isinstance(c, frontend.Cmp) and isinstance(c.left, frontend.DistinctCount)]
    assert [c.lookup.dict_name for c in counts] == ["suppliers_of_order", "late_suppliers_of_order"]
    assert Q.QUERY_TABLES["q21"] == ["supplier", "lineitem", "orders", "nation"]
    assert Q.TPCH_ORDER["q21"] == (100, [("numwait", "desc"), ("s_name", "asc")])
    assert "DistinctOp" in plan.fingerprint()


@pytest.mark.parametrize("key", ["l[0].l_orderkey", "unique(l[0].l_orderkey)", "dense(6000000, l[0].l_orderkey)", "dense(6000000, unique(l[0].l_orderkey))"])
@pytest.mark.parametrize("cond", ["", " if l[0].l_receiptdate > l[0].l_commitdate else None"])
def test_vector_sum_spellings(key, cond):
    src = ("def f(lineitem):\n"
           "    s = lineitem.sum(lambda l: {%s: vector({l[0].l_suppkey})}%s)\n"
           "    n = lineitem.sum(lambda l: 1.0 if dictSize(s[l[0].l_orderkey]) > 1 else 0.0)\n"
           "    return n\n" % (key, cond))
    plan = frontend.lower_source(src)
    assert isinstance(plan.ops[0], frontend.DistinctOp) and len(plan.ops[0].conds) == (1 if cond else 0)
    assert repr(plan.ops[0].key) == "Col(l_orderkey)"


REFUSED = [
    ("returned", "    return s\n", 3, "cannot be returned"),
    ("summed over", "    t = s.sum(lambda g: {unique(g[0]): True})\n    return t\n", 3, "cannot be summed over"),
    ("read without dictSize", "    t = lineitem.sum(lambda l: 1.0 if s[l[0].l_orderkey] != None else 0.0)\n    return t\n", 3, "only its size can be read"),
    ("as a joinProbe index", "    t = lineitem.joinProbe(s, 'l_orderkey', lambda l: True, lambda e, r: 1.0)\n    return t\n", 3, "cannot be a joinProbe index"),
    ("dictSize of a plain dictionary", "    u = lineitem.sum(lambda l: {l[0].l_orderkey: 1})\n    t = lineitem.sum(lambda l: 1.0 if dictSize(u[l[0].l_orderkey]) > 1 else 0.0)\n    return t\n", 4, "dictSize is only supported"),
    ("dictSize of a column", "    t = lineitem.sum(lambda l: 1.0 if dictSize(l[0].l_orderkey) > 1 else 0.0)\n    return t\n", 3, "dictSize is only supported"),
    ("a vector inside an expression", "    t = lineitem.sum(lambda l: {l[0].l_orderkey: record({'v': vector({l[0].l_suppkey})})})\n    return t\n", 3, "vector({...}) is only supported"),
    ("a vector of two values", "    t = lineitem.sum(lambda l: {l[0].l_orderkey: vector({l[0].l_suppkey, l[0].l_partkey})})\n    return t\n", 3, "vector({...}) is only supported"),
]


@pytest.mark.parametrize("what,tail,line,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_other_uses_of_a_dictionary_of_sets_are_refused_with_their_line(what, tail, line, text):
    src = "def f(lineitem):\n    s = lineitem.sum(lambda l: {l[0].l_orderkey: vector({l[0].l_suppkey})})\n" + tail
    with pytest.raises(frontend.UnsupportedQuery) as e:
        frontend.lower_source(src, first_line=1)
    assert text in str(e.value), str(e.value)
    assert "f, line %d:" % line in str(e.value), str(e.value)


# ---- executor, generic route --------------------------------------------------------------------------------------------
def test_oracle_reproduces_the_reference(oracle_engine, golden_q21):
    """Every case, SF=1 included: names and counts exact."""
    assert [c["sf"] for c in golden_q21["cases"]] == [0.01, 0.1, 1.0]
    for case in golden_q21["cases"]:
        want = case["results"]["q21"]
        assert want["columns"] == ["s_name", "numwait"] and len(want["rows"]) >= 1 and "reference_seconds" in want
        res = helpers.run_query(oracle_engine, "q21", helpers.case_db(case))
        helpers.check_against_golden(res, want, 0.0, "oracle/%s/q21" % case["name"])
    loops = oracle_engine.stats()["distinct_loops"]
    assert [(l["result"], l["route"]) for l in loops] == [("suppliers_of_order", "generic"), ("late_suppliers_of_order", "generic")]
    assert all("unknown operation code %d" % abi.X_RUNNEW in l["why"] and l["runs"] == 3 for l in loops)
    assert oracle_engine.stats()["host_loops"] == []


def test_strict_device_and_top(oracle_engine, golden_q21):
    case = golden_q21["cases"][1]
    db = helpers.case_db(case)
    oracle_engine.strict_device = True
    res = helpers.run_query(oracle_engine, "q21", db)
    helpers.check_against_golden(res, case["results"]["q21"], 0.0, "oracle/strict/q21")
    assert oracle_engine.stats()["host_loops"] == []
    k, order = Q.TPCH_ORDER["q21"]
    plan = frontend.lower_function(Q.QUERIES["q21"])
    top = engine.execute_plan(oracle_engine, plan, [db[t] for t in Q.QUERY_TABLES["q21"]], top=(7, order)).ordered_rows()
    want = sorted(helpers.golden_rows(case["results"]["q21"]), key=lambda r: (-r[1], r[0]))[:7]
    assert [tuple(r) for r in top] == want


def test_same_rows_with_lineitem_permuted(oracle_engine, golden_q21):
    case = golden_q21["cases"][0]
    db = helpers.case_db(case)
    c = db["lineitem"].getContainer()
    perm = np.random.default_rng(5).permutation(len(c["data"][0]))
    shuffled = dict(db)
    shuffled["lineitem"] = tpch.table_from_columns(c["headers"], [np.ascontiguousarray(a[perm]) for a in c["data"]])
    assert not (np.diff(tpch.column(shuffled["lineitem"], "l_orderkey")) >= 0).all()
    helpers.check_against_golden(helpers.run_query(oracle_engine, "q21", shuffled), case["results"]["q21"], 0.0, "oracle/permuted/q21")


def test_no_qualifying_nation_gives_the_empty_set(oracle_engine):
    db = _small_db()
    names = tpch.column(db["nation"], "n_name").copy()
    names[names == "SAUDI ARABIA"] = "ATLANTIS"
    res = helpers.run_query(oracle_engine, "q21", helpers.make_golden._replace(db, "nation", n_name=names))
    assert res.size() == 0 and res.columns == ["s_name", "numwait"]


def test_scalar_payload_spelling_gives_the_same_rows(oracle_engine, golden_q21):
    """The reference's own spelling keeps the supplier's name as the build's scalar value and groups by the looked-up value itself:
    with more suppliers than a small group table holds that is a large group-by keyed by one text value, whose keys must come back
    as the text."""
    @sdql_compile({"supplier": tpch.supplier_type, "lineitem": lineitem_type, "orders": tpch.order_type, "nation": tpch.nation_type})
    def spelled(supplier, lineitem, orders, nation):
        saudi = nation.joinBuild("n_nationkey", lambda n: n[0].n_name == "SAUDI ARABIA", [])
        names = supplier.joinProbe(saudi, "s_nationkey", lambda s: True, lambda e, s: {s.s_suppkey: s.s_name}, False)
        failed = orders.sum(lambda o: {dense(6000000, unique(o[0].o_orderkey)): True} if o[0].o_orderstatus == "F" else None)
        every = lineitem.sum(lambda l: {dense(6000000, l[0].l_orderkey): vector({l[0].l_suppkey})})
        late = lineitem.sum(lambda l: {dense(6000000, l[0].l_orderkey): vector({l[0].l_suppkey})} if l[0].l_receiptdate > l[0].l_commitdate else None)
        waits = lineitem.sum(
            lambda l: {record({"s_name": names[l[0].l_suppkey]}): record({"numwait": 1})}
            if l[0].l_receiptdate > l[0].l_commitdate and names[l[0].l_suppkey] != None and failed[l[0].l_orderkey] != None      # noqa: E711
            and dictSize(every[l[0].l_orderkey]) > 1
            and ((dictSize(late[l[0].l_orderkey]) > 0) and (dictSize(late[l[0].l_orderkey]) > 1)) == False      # noqa: E712
            else None)
        out = waits.sum(lambda g: {unique(g[0].concat(g[1])): True})
        return out

    case = golden_q21["cases"][2]
    db = helpers.case_db(case)
    plan = frontend.lower_function(spelled)
    res = engine.execute_plan(oracle_engine, plan, [db[t] for t in ("supplier", "lineitem", "orders", "nation")])
    helpers.check_against_golden(res, case["results"]["q21"], 0.0, "oracle/spelled/q21")


def test_sizes_against_python_sets(oracle_engine):
    """dictSize per row against Python sets; a text value; a condition that nothing passes (every size reads 0: the absent key)."""
    db = tpch.generate(0.01, tables=["lineitem"], columns={"lineitem": ["l_orderkey", "l_suppkey", "l_shipmode", "l_receiptdate", "l_commitdate"]})

    @sdql_compile({"lineitem": lineitem_type})
    def sizes(lineitem):
        sups = lineitem.sum(lambda l: {l[0].l_orderkey: vector({l[0].l_suppkey})})
        modes = lineitem.sum(lambda l: {l[0].l_orderkey: vector({l[0].l_shipmode})} if l[0].l_receiptdate > l[0].l_commitdate else None)
        never = lineitem.sum(lambda l: {l[0].l_orderkey: vector({l[0].l_suppkey})} if l[0].l_receiptdate > 99999999 else None)
        # (one size per histogram: the parts of a several-part group key need known value ranges, and a size has none)
        hist = lineitem.sum(lambda l: {dictSize(sups[l[0].l_orderkey]) * 100 + dictSize(modes[l[0].l_orderkey]) * 10 + dictSize(never[l[0].l_orderkey]): 1})
        out = hist.sum(lambda g: {unique(record({"sizes": g[0], "rows": g[1]})): True})
        return out

    res = engine.execute_plan(oracle_engine, frontend.lower_function(sizes), [db["lineitem"]])
    li = db["lineitem"]
    ok, sk, sm = (tpch.column(li, c).tolist() for c in ("l_orderkey", "l_suppkey", "l_shipmode"))
    late = (tpch.column(li, "l_receiptdate") > tpch.column(li, "l_commitdate")).tolist()
    sups, modes = collections.defaultdict(set), collections.defaultdict(set)
    for k, s, m, is_late in zip(ok, sk, sm, late):
        sups[k].add(s)
        if is_late:
            modes[k].add(m)
    want = collections.Counter((len(sups[k]), len(modes[k]), 0) for k in ok)
    assert sorted(tuple(r) for r in res.rows()) == sorted((k[0] * 100 + k[1] * 10 + k[2], n) for k, n in want.items())
    assert any(k[1] == 0 for k in want) and any(k[0] != k[1] for k in want)


def test_pairs_too_wide_for_the_generic_route_are_refused(oracle_engine):
    db = _small_db()
    wide = helpers.make_golden._replace(db, "lineitem", l_orderkey=tpch.column(db["lineitem"], "l_orderkey") + (np.int64(1) << 40))
    with pytest.raises(frontend.UnsupportedQuery) as e:
        helpers.run_query(oracle_engine, "q21", wide)
    assert "pair packing" in str(e.value) and "line " in str(e.value)


def test_cpu_checker_refuses_the_operation(oracle_lib):
    ctx = oracle_lib.context(threads=1)
    try:
        key, val = ctx.upload(np.array([1, 1, 2, 2, 2], np.int64)), ctx.upload(np.array([7, 7, 8, 9, 8], np.int64))
        prog = abi.Program()
        first = prog.op(abi.X_RUNNEW, abi.T_BOOL, a=prog.op(abi.X_COL, abi.T_I64, col=val), b=-1, col=key)
        prog.gates = [first]
        with pytest.raises(abi.SdqhError) as e:
            ctx.xscan_sum(5, prog)
        assert e.value.code == abi.ERR_UNSUPPORTED and "unknown operation code 43" in str(e.value)
    finally:
        ctx.close()
