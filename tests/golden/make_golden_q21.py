#!/usr/bin/env python3
"""Golden fixture for TPCH q21, made like the others: the REFERENCE itself (Python mode) on this repository's generated data.

q21 is the one query of the reference's TPCH script that reads o_orderstatus, a column the generator produces only when it is
named (sdqlpy_amd/tpch.py: NAMED_ONLY), so it has a fixture of its own and the input fingerprints of the older fixtures stay as
they are.  The reference's interpreter keeps `vector({x})` values as Python sets (`vector.__add__` is a set union), so
`dictSize(l2[k])` is the number of DISTINCT suppliers of order k; that is the meaning these expected rows pin.

The reference raises AttributeError on its last line when no row qualifies (no SAUDI ARABIA supplier below SF ~ 0.002), so every
case here has at least one result row; the empty case is tested against the empty set in tests/test_q21_cpu.py.

    python tests/golden/make_golden_q21.py [--jobs 3]        # rewrites tests/golden/tpch_golden_q21.json
"""
import json
import multiprocessing as mp
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from sdqlpy_amd import tpch  # noqa: E402

QUERY = "q21"
ARG_TABLES = ["supplier", "lineitem", "orders", "nation"]       # positional order of the reference's q21 (test/test_all.py:1032)
CASES = [("small", 0.01), ("medium", 0.1), ("sf1", 1.0)]


def _inputs(sf, threads):
    return tpch.generate(sf, tpch.DEFAULT_SEED, tables=sorted(ARG_TABLES), columns=tpch.columns_for([QUERY]), threads=threads)


def _one(job):
    name, sf = job
    mg.WIDE_QUERIES.append(QUERY)                                # load_reference() picks the functions to exec from these lists
    ref, queries = mg.load_reference()
    db = _inputs(sf, 2)
    t0 = time.time()
    res = queries[QUERY](*[mg.to_ref_table(ref, db[t]) for t in ARG_TABLES])
    r = mg.encode_result(ref, res)
    r["reference_seconds"] = round(time.time() - t0, 1)
    if not r["rows"]:
        raise SystemExit("%s: the reference returned no row; choose a size with at least one" % name)
    case = {"name": name, "sf": sf, "seed": tpch.DEFAULT_SEED, "variant": "base", "tables": sorted(ARG_TABLES),
            "fingerprint": tpch.fingerprint(db), "rows": {t: len(db[t].getContainer()["data"][0]) for t in sorted(ARG_TABLES)},
            "results": {QUERY: r}}
    print("%-8s %s  %7.1fs  %d rows" % (name, QUERY, time.time() - t0, len(r["rows"])), flush=True)
    return case


def main():
    jobs_n = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else len(CASES)
    with mp.get_context("spawn").Pool(jobs_n, maxtasksperchild=1) as pool:
        cases = pool.map(_one, CASES, chunksize=1)
    out = {"meta": {"generator_seed": tpch.DEFAULT_SEED,
                    "reference": "edin-dal/sdqlpy Python mode (sdqlpy_init(0,1)), q21 from test/test_all.py",
                    "made_by": "tests/golden/make_golden_q21.py"},
           "cases": cases}
    path = os.path.join(HERE, "tpch_golden_q21.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
