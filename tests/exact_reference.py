"""Exact results of TPCH q1, q3, q5, q6 and q9 in integer arithmetic — plain numpy, no project kernel, no CPU implementation.

TPCH money columns are two-decimal and quantities are whole numbers, so every sum of sdqlpy_amd/tpch_queries.py's q1 / q3 / q5 / q6 /
q9 has an exact rational value: an integer numerator N over a fixed power of ten D.  This module restates the five queries on a
generated database (a dict of columnar tables) and returns, per group,

    the key, the exact row count m, the exact numerator N (D = 10^4 for price*(1-disc), price*disc and q9's profit, 10^6 for q1's
    sum_charge, 10^2 for sums of one column), S = the same sum over the absolute values of the parts (q9: |a| + |b| per row of a - b;
    everywhere else the terms are positive and S = N), and the plain double evaluation of the group's first row (what a one-row group
    must be, bit for bit).

The values do not depend on summation order, on the HIP path or on the CPU implementation.  `assert_close_to_exact` compares a computed
result with them under the worst-case bound of double arithmetic

    |got - N/D| <= 1.01 * (m + 6) * 2^-53 * S/D

(the two decimal inputs of a term carry at most u = 2^-53 relative representation error each, each of the at most three multiplies /
subtracts of a term adds u, any summation order adds (m-1) * u * sum|x_i|, and 1.01 covers the second-order terms at m*u <= 1e-7).

lineitem is walked in row chunks (`chunk_rows`), so SF=100 needs no second copy of it; a chunk's int64 sums are asserted to stay below
2^63 and are accumulated across chunks in Python ints (q1's sum_charge numerator reaches 6e21 over 600 M rows).
"""
from fractions import Fraction

import numpy as np

QUERIES = ("q1", "q3", "q5", "q6", "q9")
DEFAULT_CHUNK_ROWS = 1 << 22
U = Fraction(1, 2 ** 53)
SLACK = Fraction(101, 100)


def cents(col, whole=False):
    """A two-decimal double column as int64 hundredths; the column must BE two-decimal (whole=True: a whole number), bit for bit."""
    col = np.asarray(col, np.float64)
    c = np.rint(col * 100).astype(np.int64)
    assert np.array_equal(c / 100.0, col), "a money column is not two-decimal: the exact reference does not apply to this input"
    if whole:
        assert not np.any(c % 100), "a quantity is not a whole number: the exact reference does not apply to this input"
    return c


def columns(table):
    """name -> numpy array of a columnar table."""
    c = table.getContainer()
    return dict(zip(c["headers"], c["data"]))


class Exact:
    """The exact result of one query.  keys: {column: array or list} in result-column order; m: rows per group; values:
    {column: {"N", "S", "D", "plain"}}; counts: {column: exact integers}.  A scalar query (q6) is one group without keys.
    Large results (q3) hold N / S as int64 arrays below 2^53, small ones as lists of Python ints."""

    def __init__(self, query, keys, m, values, counts=None, scalar=False):
        self.query, self.keys, self.m, self.values, self.counts, self.scalar = query, keys, m, values, counts or {}, scalar

    def size(self):
        return len(self.m)

    def one_row_groups(self):
        return int(np.count_nonzero(np.asarray(self.m) == 1))

    def key_rows(self):
        cols = [np.asarray(v).tolist() for v in self.keys.values()]
        return [tuple(r) for r in zip(*cols)]


# ---- per-chunk state shared by the queries of one pass ------------------------------------------------------------------------------
class _Chunk:
    def __init__(self, li, lo, hi):
        self.li, self.lo, self.hi, self._cents, self._rev = li, lo, hi, {}, None

    def __len__(self):
        return self.hi - self.lo

    def col(self, name):
        return self.li[name][self.lo:self.hi]

    def cents(self, name):
        if name not in self._cents:
            self._cents[name] = cents(self.col(name), whole=name == "l_quantity")
        return self._cents[name]

    def revenue(self):
        """l_extendedprice * (1 - l_discount) in 10^-4: price cents times (100 - discount cents)."""
        if self._rev is None:
            self._rev = self.cents("l_extendedprice") * (100 - self.cents("l_discount"))
        return self._rev


def _check_chunk_sum(absterm, rows):
    """A chunk's int64 sum cannot wrap: rows * (largest |term|) stays below 2^63."""
    if len(absterm):
        assert int(absterm.max()) * int(rows) < 2 ** 63, "chunk too large for int64 sums: lower chunk_rows"


class _Groups:
    """Exact sums for a small number of groups (group ids 0 .. ngroups-1), accumulated across chunks in Python ints."""

    def __init__(self, ngroups, names):
        self.G = ngroups
        self.m = [0] * ngroups
        self.N = {n: [0] * ngroups for n in names}
        self.S = {n: [0] * ngroups for n in names}
        self.plain = {n: [None] * ngroups for n in names}

    def add(self, gid, terms, plain):
        """gid: group of each selected row; terms: {name: (term, |parts| summed, or None when term >= 0)} as int64 arrays;
        plain(rows) -> {name: doubles}: the query's own double expression on the given selected rows."""
        if len(gid) == 0:
            return
        gid = gid.astype(np.int16 if self.G <= 32767 else np.int64)
        cnt = np.bincount(gid, minlength=self.G)
        present = np.flatnonzero(cnt)
        order = np.argsort(gid, kind="stable")
        starts = (np.cumsum(cnt) - cnt)[present]
        groups = present.tolist()
        new = [i for i, g in enumerate(groups) if self.m[g] == 0]
        if new:
            first = plain(order[starts[new]])                   # (stable sort: a group's first entry is its first row)
            for name, v in first.items():
                for i, x in zip(new, v.tolist()):
                    self.plain[name][groups[i]] = x
        for g, c in zip(groups, cnt[present].tolist()):
            self.m[g] += c
        for name, (t, a) in terms.items():
            if a is None:
                assert t.min() >= 0
            _check_chunk_sum(t if a is None else a, len(t))
            sums = np.add.reduceat(t[order], starts).tolist()
            sums_abs = sums if a is None else np.add.reduceat(a[order], starts).tolist()
            for g, s, b in zip(groups, sums, sums_abs):
                self.N[name][g] += s
                self.S[name][g] += b

    def present(self):
        return [g for g in range(self.G) if self.m[g]]

    def values(self, name, D):
        g = self.present()
        return {"N": [self.N[name][i] for i in g], "S": [self.S[name][i] for i in g], "D": D,
                "plain": [self.plain[name][i] for i in g]}


def _strictly_increasing(a):
    return bool(np.all(a[1:] > a[:-1]))


def _dense(size, keys, values, default, dtype):
    out = np.full(size, default, dtype)
    out[keys] = values
    return out


def _max_key(*arrays):
    return max(int(a.max()) for a in arrays if len(a))


# ---- the five queries: prepare (small tables), chunk (a row range of lineitem), finish ----------------------------------------------
class _Q6:
    def __init__(self, db, li):
        self.g = _Groups(1, ["gain"])

    def chunk(self, ck):
        d, q, ship = ck.cents("l_discount"), ck.cents("l_quantity"), ck.col("l_shipdate")
        idx = np.flatnonzero((ship >= 19940101) & (ship < 19950101) & (d >= 5) & (d <= 7) & (q < 2400))
        p, dd = ck.col("l_extendedprice"), ck.col("l_discount")
        self.g.add(np.zeros(len(idx), np.int16), {"gain": (ck.cents("l_extendedprice")[idx] * d[idx], None)},
                   lambda r: {"gain": p[idx[r]] * dd[idx[r]]})

    def finish(self):
        if not self.g.m[0]:
            return Exact("q6", {}, [0], {"gain": {"N": [0], "S": [0], "D": 10 ** 4, "plain": [0.0]}}, scalar=True)
        return Exact("q6", {}, list(self.g.m), {"gain": self.g.values("gain", 10 ** 4)}, scalar=True)


class _Q1:
    NAMES = {"sum_qty": 10 ** 2, "sum_base_price": 10 ** 2, "sum_disc_price": 10 ** 4, "sum_charge": 10 ** 6}

    def __init__(self, db, li):
        self.g = _Groups(128 * 128, list(self.NAMES))

    def chunk(self, ck):
        rf, ls = ck.col("l_returnflag").view(np.uint32), ck.col("l_linestatus").view(np.uint32)
        assert rf.max() < 128 and ls.max() < 128
        idx = np.flatnonzero(ck.col("l_shipdate") <= 19980902)
        gid = (rf[idx] * 128 + ls[idx]).astype(np.int16)
        rev, t = ck.revenue()[idx], ck.cents("l_tax")[idx]
        p, d, tax, q = (ck.col(c) for c in ("l_extendedprice", "l_discount", "l_tax", "l_quantity"))

        def plain(r):
            i = idx[r]
            return {"sum_qty": q[i], "sum_base_price": p[i], "sum_disc_price": p[i] * (1.0 - d[i]),
                    "sum_charge": (p[i] * (1.0 - d[i])) * (1.0 + tax[i])}
        self.g.add(gid, {"sum_qty": (ck.cents("l_quantity")[idx], None), "sum_base_price": (ck.cents("l_extendedprice")[idx], None),
                         "sum_disc_price": (rev, None), "sum_charge": (rev * (100 + t), None)}, plain)

    def finish(self):
        g = self.g.present()
        keys = {"l_returnflag": [chr(i // 128) for i in g], "l_linestatus": [chr(i % 128) for i in g]}
        m = [self.g.m[i] for i in g]
        return Exact("q1", keys, m, {n: self.g.values(n, D) for n, D in self.NAMES.items()}, counts={"count_order": list(m)})


class _Q3:
    CUTOFF = 19950315

    def __init__(self, db, li):
        cu, od = columns(db["customer"]), columns(db["orders"])
        assert _strictly_increasing(np.sort(cu["c_custkey"])) and _strictly_increasing(od["o_orderkey"])
        building = np.zeros(_max_key(cu["c_custkey"], od["o_custkey"]) + 1, bool)
        building[cu["c_custkey"][cu["c_mktsegment"] == "BUILDING"]] = True
        is_open = (od["o_orderdate"] < self.CUTOFF) & building[od["o_custkey"]]
        self.open = np.zeros(_max_key(od["o_orderkey"], li["l_orderkey"][-1:]) + 1, bool)
        self.open[od["o_orderkey"][is_open]] = True
        self.od, self.last, self.parts = od, -1, []

    def chunk(self, ck):
        ok = ck.col("l_orderkey")
        # lineitem is stored in l_orderkey order: a group is a run of rows, summed by reduceat on int64 — no float accumulates
        assert len(ok) == 0 or (ok[0] >= self.last and bool(np.all(ok[1:] >= ok[:-1]))), "lineitem is not in l_orderkey order"
        if len(ok):
            self.last = int(ok[-1])
        idx = np.flatnonzero((ck.col("l_shipdate") > self.CUTOFF) & self.open[ok])
        if not len(idx):
            return
        k, r = ok[idx], ck.revenue()[idx]
        _check_chunk_sum(r, len(r))
        starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
        first = idx[starts]
        self.parts.append((k[starts], np.add.reduceat(r, starts), np.diff(np.r_[starts, len(k)]),
                           ck.col("l_extendedprice")[first] * (1.0 - ck.col("l_discount")[first])))

    def finish(self):
        if not self.parts:
            k = np.zeros(0, np.int64)
            return Exact("q3", {"l_orderkey": k, "o_orderdate": k, "o_shippriority": k}, k,
                         {"revenue": {"N": k, "S": k, "D": 10 ** 4, "plain": np.zeros(0)}})
        k, s, c, pl = (np.concatenate(x) for x in zip(*self.parts))
        assert bool(np.all(k[1:] >= k[:-1]))                       # a run cut by a chunk seam: its two pieces are neighbours
        starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
        assert int(s.max()) * int(np.diff(np.r_[starts, len(k)]).max()) < 2 ** 53
        keys, N, m = k[starts], np.add.reduceat(s, starts), np.add.reduceat(c, starts)
        assert int(N.max()) < 2 ** 53
        pos = np.searchsorted(self.od["o_orderkey"], keys)
        assert np.array_equal(self.od["o_orderkey"][pos], keys)
        return Exact("q3", {"l_orderkey": keys, "o_orderdate": self.od["o_orderdate"][pos], "o_shippriority": self.od["o_shippriority"][pos]},
                     m, {"revenue": {"N": N, "S": N, "D": 10 ** 4, "plain": pl[starts]}})


class _Q5:
    def __init__(self, db, li):
        re, na, cu, od, su = (columns(db[t]) for t in ("region", "nation", "customer", "orders", "supplier"))
        asia = re["r_regionkey"][re["r_name"] == "ASIA"]
        asian = np.isin(na["n_regionkey"], asia)
        assert _strictly_increasing(np.sort(na["n_nationkey"])) and na["n_nationkey"].max() < 127
        self.names = {int(k): str(n) for k, n in zip(na["n_nationkey"][asian], na["n_name"][asian])}
        assert len(set(self.names.values())) == len(self.names)
        assert _strictly_increasing(np.sort(cu["c_custkey"])) and _strictly_increasing(od["o_orderkey"]) and _strictly_increasing(np.sort(su["s_suppkey"]))
        is_asian = np.isin(cu["c_nationkey"], list(self.names))
        cust_nation = _dense(_max_key(cu["c_custkey"], od["o_custkey"]) + 1, cu["c_custkey"][is_asian], cu["c_nationkey"][is_asian], -1, np.int8)
        on = cust_nation[od["o_custkey"]]
        in_1994 = (od["o_orderdate"] >= 19940101) & (od["o_orderdate"] < 19950101) & (on >= 0)
        self.order_nation = _dense(_max_key(od["o_orderkey"], li["l_orderkey"][-1:]) + 1, od["o_orderkey"][in_1994], on[in_1994], -1, np.int8)
        self.supp_nation = _dense(_max_key(su["s_suppkey"], li["l_suppkey"]) + 1, su["s_suppkey"], su["s_nationkey"], -2, np.int8)
        self.g = _Groups(128, ["revenue"])

    def chunk(self, ck):
        on = self.order_nation[ck.col("l_orderkey")]
        cand = np.flatnonzero(on >= 0)
        idx = cand[self.supp_nation[ck.col("l_suppkey")[cand]] == on[cand]]
        p, d = ck.col("l_extendedprice"), ck.col("l_discount")
        self.g.add(on[idx], {"revenue": (ck.revenue()[idx], None)}, lambda r: {"revenue": p[idx[r]] * (1.0 - d[idx[r]])})

    def finish(self):
        g = self.g.present()
        return Exact("q5", {"n_name": [self.names[i] for i in g]}, [self.g.m[i] for i in g], {"revenue": self.g.values("revenue", 10 ** 4)})


class _Q9:
    def __init__(self, db, li):
        na, su, pa, ps, od = (columns(db[t]) for t in ("nation", "supplier", "part", "partsupp", "orders"))
        assert _strictly_increasing(np.sort(na["n_nationkey"])) and _strictly_increasing(np.sort(su["s_suppkey"]))
        assert _strictly_increasing(np.sort(pa["p_partkey"])) and _strictly_increasing(od["o_orderkey"])
        self.names = {int(k): str(n) for k, n in zip(na["n_nationkey"], na["n_name"])}
        assert len(set(self.names.values())) == len(self.names) and na["n_nationkey"].max() < 127
        assert bool(np.all(np.isin(su["s_nationkey"], na["n_nationkey"])))
        self.width = _max_key(su["s_suppkey"], ps["ps_suppkey"], li["l_suppkey"]) + 1
        supp_nation = _dense(self.width, su["s_suppkey"], su["s_nationkey"], -1, np.int8)
        self.green = np.zeros(_max_key(pa["p_partkey"], ps["ps_partkey"], li["l_partkey"]) + 1, bool)
        self.green[pa["p_partkey"][np.char.find(pa["p_name"], "green") >= 0]] = True
        sel = np.flatnonzero(self.green[ps["ps_partkey"]])
        packed = ps["ps_partkey"][sel] * self.width + ps["ps_suppkey"][sel]               # the composite (part, supplier) key as one int64
        assert self.green.size * self.width < 2 ** 62
        order = np.argsort(packed, kind="stable")
        self.packed = packed[order]
        assert _strictly_increasing(self.packed)
        self.cost = cents(ps["ps_supplycost"][sel][order])
        self.cost_plain = ps["ps_supplycost"][sel][order]
        self.nation = supp_nation[ps["ps_suppkey"][sel][order]]
        assert len(self.nation) == 0 or self.nation.min() >= 0
        self.od = od
        years = od["o_orderdate"] // 10000
        self.y0, self.ny = int(years.min()), int(years.max() - years.min()) + 1
        self.g = _Groups(128 * self.ny, ["sum_profit"])

    def chunk(self, ck):
        cand = np.flatnonzero(self.green[ck.col("l_partkey")])
        if not len(cand) or not len(self.packed):
            return
        key = ck.col("l_partkey")[cand] * self.width + ck.col("l_suppkey")[cand]
        pos = np.minimum(np.searchsorted(self.packed, key), len(self.packed) - 1)
        hit = self.packed[pos] == key
        idx, pos = cand[hit], pos[hit]
        ok = ck.col("l_orderkey")[idx]
        opos = np.searchsorted(self.od["o_orderkey"], ok)
        assert np.array_equal(self.od["o_orderkey"][np.minimum(opos, len(self.od["o_orderkey"]) - 1)], ok), "a lineitem row without its order"
        year = self.od["o_orderdate"][opos] // 10000
        gid = self.nation[pos].astype(np.int64) * self.ny + (year - self.y0)
        a, b = ck.revenue()[idx], self.cost[pos] * ck.cents("l_quantity")[idx]
        assert (len(a) == 0) or (a.min() >= 0 and b.min() >= 0)
        p, d, q, c = ck.col("l_extendedprice"), ck.col("l_discount"), ck.col("l_quantity"), self.cost_plain
        self.g.add(gid, {"sum_profit": (a - b, a + b)}, lambda r: {"sum_profit": p[idx[r]] * (1.0 - d[idx[r]]) - c[pos[r]] * q[idx[r]]})

    def finish(self):
        g = self.g.present()
        keys = {"nation": [self.names[i // self.ny] for i in g], "o_year": [self.y0 + i % self.ny for i in g]}
        return Exact("q9", keys, [self.g.m[i] for i in g], {"sum_profit": self.g.values("sum_profit", 10 ** 4)})


_STATES = {"q1": _Q1, "q3": _Q3, "q5": _Q5, "q6": _Q6, "q9": _Q9}


def exact_results(db, queries, chunk_rows=DEFAULT_CHUNK_ROWS):
    """{query: Exact} for the given queries in ONE pass over lineitem: the cents of a chunk's columns are taken once for all of them."""
    li = columns(db["lineitem"])
    states = {q: _STATES[q](db, li) for q in queries}
    n = len(next(iter(li.values())))
    for lo in range(0, n, int(chunk_rows)):
        ck = _Chunk(li, lo, min(n, lo + int(chunk_rows)))
        for st in states.values():
            st.chunk(ck)
    return {q: st.finish() for q, st in states.items()}


def q1(db, chunk_rows=DEFAULT_CHUNK_ROWS):
    return exact_results(db, ("q1",), chunk_rows)["q1"]


def q3(db, chunk_rows=DEFAULT_CHUNK_ROWS):
    return exact_results(db, ("q3",), chunk_rows)["q3"]


def q5(db, chunk_rows=DEFAULT_CHUNK_ROWS):
    return exact_results(db, ("q5",), chunk_rows)["q5"]


def q6(db, chunk_rows=DEFAULT_CHUNK_ROWS):
    return exact_results(db, ("q6",), chunk_rows)["q6"]


def q9(db, chunk_rows=DEFAULT_CHUNK_ROWS):
    return exact_results(db, ("q9",), chunk_rows)["q9"]


# ---- the comparator --------------------------------------------------------------------------------------------------------------------
def as_columns(res):
    """{column: values} of a result: a result set (.columns / .column), a golden entry ({"columns", "rows"}, doubles as {"f": hex})
    or a mapping that is one already."""
    if hasattr(res, "columns") and hasattr(res, "column"):
        res = res.wait() if hasattr(res, "wait") else res
        return {c: res.column(c) for c in res.columns}
    if isinstance(res, dict) and "rows" in res and "columns" in res:
        dec = lambda v: float.fromhex(v["f"]) if isinstance(v, dict) else v
        cols = list(zip(*[[dec(x) for x in row] for row in res["rows"]])) or [()] * len(res["columns"])
        return {c: list(v) for c, v in zip(res["columns"], cols)}
    return dict(res)


def bound_of(m, S, D):
    """1.01 * (m + 6) * 2^-53 * S/D, exactly."""
    return SLACK * (m + 6) * U * Fraction(S, D)


def _ratio(got, N, S, D, m, what):
    err, bound = abs(Fraction(float(got)) - Fraction(N, D)), bound_of(m, S, D)
    assert err <= bound, "%s: %r is %.3e from the exact %s/%d, bound %.3e (m = %d)" % (what, got, float(err), N, D, float(bound), m)
    return float(err / bound) if bound else 0.0


def assert_close_to_exact(got, exact, what=""):
    """`got` (a result of the query, see as_columns; q6: a float) against the exact result: key columns, the set of rows and integer
    columns exact; every sum of every group within the bound; a one-row group bit-equal to the plain double evaluation of its row.
    No group is left out.  Returns the largest err / bound seen."""
    worst = 0.0
    if exact.scalar:
        (name, v), = exact.values.items()
        got = float(got)
        if exact.m[0] == 1:
            assert got == v["plain"][0], "%s: one row, %r != %r" % (what, got, v["plain"][0])
        return _ratio(got, v["N"][0], v["S"][0], v["D"], exact.m[0], what)
    cols = as_columns(got)
    want_cols = list(exact.keys) + list(exact.values) + list(exact.counts)
    assert sorted(cols) == sorted(want_cols), "%s: columns %s, expected %s" % (what, sorted(cols), sorted(want_cols))
    n = len(cols[want_cols[0]])
    assert n == exact.size(), "%s: %d rows, the exact result has %d" % (what, n, exact.size())
    first = next(iter(exact.values.values()))
    if isinstance(first["N"], np.ndarray):
        # a large result keyed by one increasing integer column (q3): vectorised.  N < 2^53, so N / D in doubles is correctly rounded
        # and the comparison against it gets one ulp of slack for that rounding
        kname = next(iter(exact.keys))
        gk = np.asarray(cols[kname])
        order = np.argsort(gk, kind="stable")
        for name, want in exact.keys.items():
            assert np.array_equal(np.asarray(cols[name])[order], want), "%s: key column %s differs from the exact result" % (what, name)
        m = np.asarray(exact.m)
        for name, v in exact.values.items():
            g = np.asarray(cols[name], np.float64)[order]
            assert int(v["N"].max(initial=0)) < 2 ** 53
            ref = v["N"].astype(np.float64) / float(v["D"])
            bound = 1.01 * (m + 6) * 2.0 ** -53 * (v["S"].astype(np.float64) / float(v["D"]))
            err = np.abs(g - ref)
            bad = np.flatnonzero(~(err <= bound + np.spacing(ref)))
            assert not len(bad), "%s: %d of %d groups outside the bound, first: key %r got %r exact %r (m = %d)" % (
                what, len(bad), n, exact.keys[kname][bad[0]], g[bad[0]], ref[bad[0]], m[bad[0]])
            one = m == 1
            bad = np.flatnonzero(one & (g != v["plain"]))
            assert not len(bad), "%s: %d one-row groups differ from the plain double evaluation of their row, first: key %r got %r plain %r" % (
                what, len(bad), exact.keys[kname][bad[0]], g[bad[0]], v["plain"][bad[0]])
            if n:
                worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))))
        for name, want in exact.counts.items():
            assert np.array_equal(np.asarray(cols[name])[order], want), "%s: %s" % (what, name)
        return worst
    knames = list(exact.keys)
    got_keys = [tuple(r) for r in zip(*[np.asarray(cols[k]).tolist() for k in knames])]
    assert len(set(got_keys)) == len(got_keys) and set(got_keys) == set(exact.key_rows()), \
        "%s: groups %s, the exact result has %s" % (what, sorted(got_keys)[:8], sorted(exact.key_rows())[:8])
    at = {k: i for i, k in enumerate(got_keys)}
    for j, key in enumerate(exact.key_rows()):
        i, m = at[key], exact.m[j]
        for name, want in exact.counts.items():
            assert int(np.asarray(cols[name]).tolist()[i]) == want[j], "%s: %s of %r is %r, exactly %d" % (what, name, key, cols[name][i], want[j])
        for name, v in exact.values.items():
            g = float(np.asarray(cols[name]).tolist()[i])
            if m == 1:
                assert g == v["plain"][j], "%s: one-row group %r: %s = %r, its row gives %r" % (what, key, name, g, v["plain"][j])
            worst = max(worst, _ratio(g, v["N"][j], v["S"][j], v["D"], m, "%s: %s of %r" % (what, name, key)))
    return worst


def top_keys(exact, k):
    """q3's ORDER BY revenue DESC, o_orderdate ASC LIMIT k on the exact values: the l_orderkey of the first k groups."""
    assert exact.query == "q3"
    N = exact.values["revenue"]["N"]
    order = np.lexsort((exact.keys["o_orderdate"], -N))[:k]
    return exact.keys["l_orderkey"][order].tolist()
