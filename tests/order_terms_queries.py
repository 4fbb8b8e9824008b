"""What tests/test_order_terms_cpu.py and tests/test_order_terms_gpu.py share: two purpose-made queries over supplier whose results are
ordered by text behind row references and by the halves of a packed key, and a supplier table in which a name neither sorts with its
row nor comes once."""
import numpy as np

from sdqlpy_amd.sdql_lib import *      # noqa: F401,F403  (the DSL of the queries)
from sdqlpy_amd.sdql_lib import table_from_columns
from sdqlpy_amd.tpch import supplier_type

SUPPLIER_COLUMNS = ["s_suppkey", "s_name", "s_nationkey", "s_acctbal"]


@sdql_compile({"supplier": supplier_type})
def suppliers_by_name(supplier):
    """A unique build with a text payload (row references into s_name) and an integer one."""
    built = supplier.sum(lambda s: {unique(s[0].s_suppkey): record({"s_name": s[0].s_name, "s_nationkey": s[0].s_nationkey})})
    listed = built.sum(lambda g: {unique(record({"s_suppkey": g[0], "s_name": g[1].s_name, "s_nationkey": g[1].s_nationkey})): True})
    return listed


@sdql_compile({"supplier": supplier_type})
def suppliers_by_pair(supplier):
    """A unique build keyed by the packed pair (s_nationkey, s_suppkey)."""
    built = supplier.sum(lambda s: {unique(record({"s_nationkey": s[0].s_nationkey, "s_suppkey": s[0].s_suppkey})):
                                    record({"s_name": s[0].s_name, "s_acctbal": s[0].s_acctbal})})
    listed = built.sum(lambda g: {unique(g[0].concat(g[1])): True})
    return listed


BY_NAME_ORDER = [("s_name", "desc")]
BY_PAIR_ORDER = [("s_nationkey", "desc"), ("s_suppkey", "asc")]
BY_PAIR_ORDER_2 = [("s_suppkey", "desc"), ("s_nationkey", "asc")]


@sdql_compile({"supplier": supplier_type})
def balance_by_name(supplier):
    """A group-by keyed by one text column: beyond 4096 distinct names the key travels as a row reference into s_name (key_decoder),
    one entry per row — entries that hold equal names are merged on the host when the result is read."""
    sums = supplier.sum(lambda s: {s[0].s_name: s[0].s_acctbal})
    listed = sums.sum(lambda g: {unique(record({"s_name": g[0], "balance": g[1]})): True})
    return listed


@sdql_compile({"supplier": supplier_type})
def balance_by_name_and_nation(supplier):
    """A group-by keyed by the packed pair (s_name, s_nationkey): the first half is a row reference behind a part decoder."""
    sums = supplier.sum(lambda s: {record({"s_name": s[0].s_name, "s_nationkey": s[0].s_nationkey}): s[0].s_acctbal})
    listed = sums.sum(lambda g: {unique(record({"s_name": g[0].s_name, "s_nationkey": g[0].s_nationkey, "balance": g[1]})): True})
    return listed


BY_TEXT_KEY_ORDERS = [[("s_name", "asc")], [("balance", "desc"), ("s_name", "desc")]]
BY_TEXT_PART_ORDERS = [[("s_name", "desc"), ("s_nationkey", "asc")], [("s_nationkey", "desc"), ("s_name", "asc")]]


def permuted_suppliers(supplier, seed=7):
    """The supplier table in a random row order: s_name does not sort with its row, and no name comes twice."""
    c = supplier.getContainer()
    perm = np.random.default_rng(seed).permutation(len(c["data"][0]))
    return table_from_columns(list(c["headers"]), [np.ascontiguousarray(a[perm]) for a in c["data"]])


def shuffled_suppliers(supplier, seed=5):
    """The supplier table in a random row order, every name given to three rows: s_name is neither sorted nor free of repeats, so a
    row reference into it does not order as the text and ties on it fall through to build-row order."""
    c = supplier.getContainer()
    n = len(c["data"][0])
    perm = np.random.default_rng(seed).permutation(n)
    cols = {h: np.ascontiguousarray(a[perm]) for h, a in zip(c["headers"], c["data"])}
    cols["s_name"] = np.ascontiguousarray(cols["s_name"][np.arange(n) % max(1, n // 3)])
    return table_from_columns(list(c["headers"]), [cols[h] for h in c["headers"]])
