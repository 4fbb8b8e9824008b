"""Functions of the partition's size (quantiles), the part that needs no GPU: the window quantile extension's symbols
(include/sdqh_sort_quantile.h, abi.WINDOW_QUANTILE_EXPORTS) in the cross-compiled library and nowhere else, the CPU implementation
without them, a compile-only context, the request's checks, ResultSet.quantiles against an independent restatement (sort a list of
tuples, walk it; Python integers and fractions.Fraction for NTILE and the ranks, np.float64 scalar operations for the four-operation
PERCENTILE_CONT expression), the routing decision on a stub engine, and the decorator surface on the CPU implementation's engine."""
import math
import os
import re
import struct
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import tpch_queries as Q
from sdqlpy_amd.result import QUANTILE_FNS, FrameRequest, QuantileRequest, ResultSet, SlideRequest, WindowRequest, quantile_request
from test_window_cpu import NAN_A, NAN_B, SHAPES, _cases, _declared, _image, db, on_the_decorator      # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.SORT_ALL
I_MIN, I_MAX = -(1 << 63), (1 << 63) - 1
PS = [0.0, 5e-324, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.7, float(np.nextafter(1.0, 0.0)), 1.0]
K_TERM = (abi.SORT_KEY, 0, False, False)


# ---- symbols -----------------------------------------------------------------------------------------------------------------------
def test_extension_symbols_are_exported_and_stay_out_of_the_other_boundaries(hip_lib):
    assert sorted(abi.WINDOW_QUANTILE_EXPORTS) == _declared("sdqh_sort_quantile.h") == ["sdqh_table_window_quantile", "sdqh_window_quantile_geometry"]
    for s in abi.WINDOW_QUANTILE_EXPORTS:
        assert hasattr(hip_lib.cdll, s), s
        for other in (abi.EXPORTS, abi.SORT_EXPORTS, abi.SORT_TERMS_EXPORTS, abi.WINDOW_EXPORTS, abi.WINDOW_AGG_EXPORTS, abi.WINDOW_SLIDE_EXPORTS, abi.WINDOW_RANGE_EXPORTS,
                      abi.EXTREMA_EXPORTS):
            assert s not in other
        for header in ("sdqh.h", "sdqh_sort.h", "sdqh_sort_terms.h", "sdqh_sort_window.h", "sdqh_sort_frames.h", "sdqh_sort_slide.h", "sdqh_sort_range.h", "sdqh_extrema.h"):
            assert s not in _declared(header), (s, header)
    assert hip_lib.has_window_quantile and hip_lib.has_window_slide and abi.ABI_VERSION == 7
    text = open(os.path.join(ROOT, "include", "sdqh_sort_quantile.h")).read()
    assert '#include "sdqh_sort_slide.h"' in text
    names = ("NTILE", "PERCENT_RANK", "CUME_DIST", "NTH", "PERCENTILE_DISC", "PERCENTILE_CONT")
    values = (abi.WQ_NTILE, abi.WQ_PERCENT_RANK, abi.WQ_CUME_DIST, abi.WQ_NTH, abi.WQ_PERCENTILE_DISC, abi.WQ_PERCENTILE_CONT)
    assert values == (0, 1, 2, 3, 4, 5) and abi.WQUANT_MAX_COLS == 4
    for name, value in zip(names, values):
        assert re.search(r"#define\s+SDQH_WQ_%s\s+%d\b" % (name, value), text), name
    assert re.search(r"#define\s+SDQH_WQUANT_MAX_COLS\s+4\b", text)
    assert QUANTILE_FNS == tuple(n.lower() for n in names)                  # positions = the constants
    import ctypes as C
    assert C.sizeof(abi.WindowQuantile) == 40 and [f for f, _ in abi.WindowQuantile._fields_] == ["fn", "kind", "index", "is_f64", "arg", "p", "empty"]
    assert "SDQH_ABI_VERSION 7" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sdqh.h")).read())
    assert "sdqh_sort_quantile.h" not in open(os.path.join(ROOT, "include", "sdqh.h")).read()


def test_cpu_implementation_loads_without_the_extension(oracle_lib):
    assert oracle_lib.has_window_quantile is False
    ctx = oracle_lib.context(threads=1)
    try:
        k = ctx.upload(np.arange(10, dtype=np.int64))
        t = ctx.hash_build_unique(10, abi.make_filter(), [], k, [], accumulate=True)
        call = lambda: ctx.table_window_quantile(t, 0, 0, [K_TERM], [(abi.WQ_NTILE, abi.SORT_KEY, 0, False, 2, 0.0, 0)], ALL, ALL, 16)
        for f in (call, ctx.window_quantile_geometry):
            with pytest.raises(abi.SdqhError) as e:
                f()
            assert e.value.code == abi.ERR_UNSUPPORTED and "has no window quantile extension (include/sdqh_sort_quantile.h)" in str(e.value) and "libsdqloracle" in str(e.value)
        t.free()
    finally:
        ctx.close()


def test_a_compile_only_context_refuses(hip_lib):
    ctx = hip_lib.context(device=-1)
    try:
        assert ctx.window_quantile_geometry() == ctx.window_geometry() >= 64       # (asks nothing of a device)
        prog = abi.Program()
        prog.key = prog.op(abi.X_COL, abi.T_I64, col=ctx.wrap(0x10000, 64, abi.I64))
        table = ctx.xbuild(64, prog, 0, 100, accumulate=True)             # the placeholder table of a compile-only context
        K = abi.SORT_KEY
        good = [[(abi.WQ_NTILE, K, 0, False, 4, 0.0, 0)], [(abi.WQ_PERCENT_RANK, K, 0, False, 0, 0.0, 0), (abi.WQ_CUME_DIST, K, 0, False, 0, 0.0, 0)],
                [(abi.WQ_NTH, K, 0, False, I_MIN, 0.0, 7)], [(abi.WQ_PERCENTILE_DISC, K, 0, False, 0, 1.0, 0), (abi.WQ_PERCENTILE_CONT, K, 0, False, 0, 0.0, 0)]]
        for cols in good:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_quantile(table, 0, 0, [K_TERM], cols, ALL, ALL, 16)
            assert e.value.code == abi.ERR_UNSUPPORTED, cols
        one = good[0][0]
        bad = [[], [one] * 5, [(6, K, 0, False, 1, 0.5, 0)], [(-1, K, 0, False, 1, 0.5, 0)], [(abi.WQ_NTILE, K, 0, False, 0, 0.0, 0)], [(abi.WQ_NTILE, K, 0, False, -3, 0.0, 0)],
               [(abi.WQ_NTH, K, 0, False, 0, 0.0, 0)], [(abi.WQ_PERCENTILE_DISC, K, 0, False, 0, -0.25, 0)], [(abi.WQ_PERCENTILE_DISC, K, 0, False, 0, float(np.nextafter(1.0, 2.0)), 0)],
               [(abi.WQ_PERCENTILE_CONT, K, 0, False, 0, math.nan, 0)], [(abi.WQ_PERCENTILE_CONT, K, 0, False, 0, math.inf, 0)], [one, (abi.WQ_NTH, K, 0, False, 0, 0.0, 0)]]
        for cols in bad:
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_quantile(table, 0, 0, [K_TERM], cols, ALL, ALL, 16)
            assert e.value.code == abi.ERR_INVALID, cols                   # the argument checks come first
        for per_limit in (0, -1):
            with pytest.raises(abi.SdqhError) as e:
                ctx.table_window_quantile(table, 0, 0, [K_TERM], good[0], per_limit, ALL, 16)
            assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.SdqhError) as e:                            # the binding never cuts an argument to 64 bits
            ctx.table_window_quantile(table, 0, 0, [K_TERM], [(abi.WQ_NTILE, K, 0, False, 1 << 63, 0.0, 0)], ALL, ALL, 16)
        assert e.value.code == abi.ERR_INVALID
    finally:
        ctx.close()


# ---- the request -------------------------------------------------------------------------------------------------------------------------
def test_the_request_checks_and_travels_as_a_window():
    cols = {"t": ("ntile", 4), "pr": ("percent_rank",), "cd": ("cume_dist",), "n2": ("nth", "b", 2), "last": ("nth", "b", -1, 1.5), "d": ("percentile_disc", "b", 0.9),
            "c": ("percentile_cont", "b", 0.25), "med": ("median", "b")}
    req = quantile_request(None, ["a"], [("b", "desc")], cols, per=1)
    assert isinstance(req, QuantileRequest) and isinstance(req, WindowRequest) and not isinstance(req, (FrameRequest, SlideRequest)) and isinstance(req, tuple) and len(req) == 2
    assert (req[0], req[1]) == (ALL, [("a", "asc"), ("b", "desc")]) and req.by == [("a", "asc")] and req.order == [("b", "desc")] and req.npartition == 1
    assert (req.kind, req.per_limit, req.name) == (abi.WIN_ROW_NUMBER, 1, None)
    assert req.quants == [("t", "ntile", None, 4, None, None), ("pr", "percent_rank", None, None, None, None), ("cd", "cume_dist", None, None, None, None),
                          ("n2", "nth", "b", 2, None, None), ("last", "nth", "b", -1, None, 1.5), ("d", "percentile_disc", "b", None, 0.9, None),
                          ("c", "percentile_cont", "b", None, 0.25, None), ("med", "percentile_cont", "b", None, 0.5, None)]
    assert len(req.quants) > abi.WQUANT_MAX_COLS                           # more columns than the device takes is a request like any other
    assert quantile_request(None, ["a"], [], {"x": ("ntile", I_MAX)}).per_limit == ALL and quantile_request(None, ["a"], [], {"x": ("nth", "b", I_MIN)}, per=2).per_limit == 2
    again = req.renamed([("x", "asc"), ("y", "desc")], {"b": "y"})
    assert isinstance(again, QuantileRequest) and again[1] == [("x", "asc"), ("y", "desc")] and again.per_limit == 1
    assert again.quants[3] == ("n2", "nth", "y", 2, None, None) and again.quants[0] == req.quants[0] and req.renamed(req[1]).quants == req.quants
    ok = {"x": ("ntile", 2)}
    bad = [{"x": ("mode", "b")}, {"x": ("ntile", 0)}, {"x": ("ntile", -1)}, {"x": ("ntile", 2.0)}, {"x": ("ntile", True)}, {"x": ("ntile", 1 << 63)}, {"x": ("ntile",)},
           {"x": ("nth", "b", 0)}, {"x": ("nth", "b", 1.0)}, {"x": ("nth", "b", 1 << 63)}, {"x": ("nth", "b", -(1 << 63) - 1)}, {"x": ("nth", None, 1)}, {"x": ("nth", "b", 1, "zero")},
           {"x": ("nth", "b")}, {"x": ("percentile_disc", "b", -0.1)}, {"x": ("percentile_disc", "b", 1.0000001)}, {"x": ("percentile_cont", "b", math.nan)},
           {"x": ("percentile_cont", "b", "half")}, {"x": ("percentile_cont", "b")}, {"x": ("percentile_cont", 3, 0.5)}, {"x": ("median", "b", 0.5)}, {"x": ("percent_rank", "b")},
           {"x": ("cume_dist", 1)}, {"x": ()}, {"x": "ntile"}, {3: ("ntile", 2)}, {}]
    for cols in bad:
        with pytest.raises(ValueError):
            quantile_request(["a", "b"], ["a"], [("b", "desc")], cols)
    for per in (0, -1, 1.0, True, "1"):
        with pytest.raises(ValueError):
            quantile_request(None, ["a"], [("b", "desc")], ok, per=per)
    for call in (lambda: quantile_request(None, ["a"], [("b", "down")], ok), lambda: quantile_request(None, [], [], ok)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: quantile_request(["a", "b"], ["nope"], [("b", "desc")], ok), lambda: quantile_request(["a", "b"], ["a"], [("nope", "desc")], ok),
                 lambda: quantile_request(["a", "b"], ["a"], [("b", "desc")], {"x": ("median", "nope")}), lambda: quantile_request(["a", "b"], ["a"], [("b", "desc")], {"b": ("ntile", 2)})):
        with pytest.raises(KeyError):
            call()
    from sdqlpy_amd import dist as sdist
    with pytest.raises(frontend.UnsupportedQuery) as e:
        sdist.refuse_window(req)
    assert "quantiles" in str(e.value)
    sdist.refuse_window((10, [("b", "desc")]))                             # a plain top passes


# ---- ResultSet.quantiles against a walk over sorted tuples ---------------------------------------------------------------------------------
def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _walk(columns, rows, by, order):
    """rows: list of tuples.  -> [(row index, partition start a, partition end b (exclusive), tie run [f, l] as offsets from a)] in
    sorted order: sort (term images..., row index) tuples, walk them."""
    terms = [(b, "asc") if isinstance(b, str) else b for b in by] + list(order)
    text_rank = {}
    for name, _ in terms:
        j = columns.index(name)
        if rows and isinstance(rows[0][j], str):
            text_rank[name] = {s: i for i, s in enumerate(sorted({r[j] for r in rows}))}
    keyed = sorted((tuple(_image(text_rank[nm][r[columns.index(nm)]] if nm in text_rank else r[columns.index(nm)], d == "desc") for nm, d in terms), i)
                   for i, r in enumerate(rows))
    n, out, a = len(keyed), [], 0
    while a < n:
        b = a + 1
        while b < n and keyed[b][0][:len(by)] == keyed[a][0][:len(by)]:
            b += 1
        p = a
        while p < b:
            q = p + 1
            while q < b and keyed[q][0] == keyed[p][0]:
                q += 1
            out += [(keyed[j][1], a, b, p - a, q - 1 - a) for j in range(p, q)]
            p = q
        a = b
    return out


def _ntile(i, m, b):
    """SQL's NTILE by its definition: m rows dealt into b buckets in order, sizes differing by at most one, the larger ones first."""
    if b > m:
        return i + 1
    q, r = divmod(m, b)
    sizes_before = 0
    for bucket in range(1, b + 1):
        sizes_before += q + 1 if bucket <= r else q
        if i < sizes_before:
            return bucket
    raise AssertionError


def _as_f64(v):
    return np.float64(v)                                                   # (an int by one round-to-nearest conversion)


def _want(fn, vals, i, m, f, l, arg, p, default):
    """The value of one function at offset i of a partition whose measure values are vals (None: no measure)."""
    if fn == "ntile":
        return _ntile(i, m, arg)
    if fn == "percent_rank":
        return 0.0 if m == 1 else float(Fraction(f, m - 1))               # (a Fraction rounds correctly)
    if fn == "cume_dist":
        return float(Fraction(l + 1, m))
    if fn == "nth":
        if abs(arg) > m:
            return default
        return vals[arg - 1] if arg > 0 else vals[m + arg]
    if fn == "percentile_disc":
        return vals[max(math.ceil(np.float64(p) * np.float64(m)) - 1, 0)]
    x = np.float64(p) * np.float64(m - 1)
    lo, hi = math.floor(x), math.ceil(x)
    a, b = _as_f64(vals[lo]), _as_f64(vals[hi])
    if lo == hi:
        return float(a)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        w = x - np.float64(lo)
        t = d * w
        return float(a + t)


def _same(fn, got, want):
    if isinstance(want, float):
        if fn == "percentile_cont" and math.isnan(want):
            return math.isnan(got)
        return _bits(got) == _bits(want)
    return type(got) is int and got == want


def _quant_cases():
    cases = dict(_cases())
    columns, arrays = cases["plain"]
    n = len(arrays[0])
    rng = np.random.default_rng(5)
    big = np.resize(np.array([0, I_MAX, -1, I_MIN, 1, I_MIN, I_MAX, 0, I_MIN + 1, I_MAX - 1, (1 << 53) + 1, -(1 << 53) - 3], np.int64), n)[rng.permutation(n)]
    wide = np.resize(np.array([1.7976931348623157e308, -1.7976931348623157e308, np.inf, -np.inf, 0.0, -0.0, 5e-324, 1.5, NAN_A, NAN_B, 9007199254740993.0]), n)[rng.permutation(n)]
    cases["plain"] = (columns + ["big", "wide"], arrays + [big, wide])
    cases["empty"] = (columns + ["big", "wide"], [a[:0] for a in cases["plain"][1]])
    cases["one row"] = (columns + ["big", "wide"], [a[:1] for a in cases["plain"][1]])
    return cases


def _cols_of(measure, sizes):
    """Every function with every argument of the issue's lists, m taken from the sizes of the partitions at hand."""
    ms = sorted({min(sizes), max(sizes), sorted(sizes)[len(sizes) // 2]}) if sizes else [1]
    bs = sorted({1, 2, 3, I_MAX} | {b for m in ms for b in (m - 1, m, m + 1) if b >= 1})
    ks = sorted({1, 2, -1, I_MAX, -I_MAX, I_MIN} | {k for m in ms for k in (m, m + 1, -m, -m - 1)})
    cols = {"pr": ("percent_rank",), "cd": ("cume_dist",), "med": ("median", measure)}
    for b in bs:
        cols["tile_%d" % b] = ("ntile", b)
    for j, k in enumerate(ks):
        cols["nth_%d" % j] = ("nth", measure, k) if j % 2 else ("nth", measure, k, -7)
    for j, p in enumerate(PS):
        cols["disc_%d" % j] = ("percentile_disc", measure, p)
        cols["cont_%d" % j] = ("percentile_cont", measure, p)
    return cols


@pytest.mark.parametrize("case", ["plain", "empty", "one row"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_quantiles_against_a_walk(case, shape):
    """Integers (with INT64_MIN / MAX and values beyond 2^53), integer-valued doubles, +-0.0 / NaN / inf / DBL_MAX, text partition and
    order columns, by = [], every function x argument, per in {None, 1, 2}, and a limit on the whole result."""
    columns, arrays = _quant_cases()[case]
    rs = ResultSet(columns, arrays)
    rows = list(zip(*[a.tolist() for a in arrays]))
    by, order = SHAPES[shape]
    if not by and not order:
        return
    walked = _walk(columns, rows, by, order)
    sizes = sorted({b - a for _, a, b, _, _ in walked})
    done = 0
    for measure in ("v", "h", "e", "big", "wide"):
        is_f = arrays[columns.index(measure)].dtype.kind == "f"
        cols = _cols_of(measure, sizes)
        assert len(cols) > 30 > abi.WQUANT_MAX_COLS
        req_all = quantile_request(columns, by, order, cols)
        part = {}                                                          # partition start -> its measure values in order
        for pos, (i, a, b, _, _) in enumerate(walked):
            part.setdefault(a, []).append(rows[i][columns.index(measure)])
        want = {}
        for name, fn, col, arg, p, default in req_all.quants:
            fill = None
            if fn == "nth":
                fill = (NAN_A if default is None else float(default)) if is_f else (0 if default is None else default)
            want[name] = [_want(fn, part[a], pos - a, b - a, f, l, arg, p, fill) for pos, (_, a, b, f, l) in enumerate(walked)]
        for per in (None, 1, 2):
            kept = [pos for pos, (_, a, _, _, _) in enumerate(walked) if per is None or pos - a < per]
            for k in sorted({1, max(1, len(kept) // 2), ALL}):
                res = rs.quantiled(quantile_request(columns, by, order, cols, per, k=k))
                keep = kept[:k]
                assert res.columns == columns + list(cols) and len(res) == len(keep)
                for c, a in zip(columns, arrays):
                    got = res.column(c)
                    assert got.dtype == a.dtype and [x if not isinstance(x, float) else _bits(x) for x in got.tolist()] == \
                        [v if not isinstance(v, float) else _bits(v) for v in (rows[walked[pos][0]][columns.index(c)] for pos in keep)], c
                for name, fn, _, arg, p, _ in req_all.quants:
                    got = res.column(name)
                    want_dtype = np.int64 if fn == "ntile" else (np.float64 if fn in ("percent_rank", "cume_dist", "percentile_cont") or is_f else np.int64)
                    assert got.dtype == want_dtype, (name, got.dtype)
                    bad = [(pos, x, want[name][pos]) for x, pos in zip(got.tolist(), keep) if not _same(fn, x, want[name][pos])]
                    assert not bad, (by, order, measure, name, fn, arg, p, per, k, bad[:3])
                    done += 1
    assert done >= 5 * 30 * 3


def test_quantiles_on_a_result_set():
    columns, arrays = _quant_cases()["plain"]
    rs = ResultSet(columns, arrays)
    by, order = ["g"], [("v", "asc")]
    res = rs.quantiles(by, order, {"med": ("median", "v"), "p90": ("percentile_disc", "v", 0.9), "q": ("ntile", 4), "cd": ("cume_dist",), "hmax": ("nth", "h", -1)}, per=1)
    g = arrays[0]
    assert res.columns == columns + ["med", "p90", "q", "cd", "hmax"] and len(res) == len(np.unique(g))
    assert [res.column(c).dtype for c in ("med", "p90", "q", "cd", "hmax")] == [np.float64, np.float64, np.int64, np.float64, np.int64]
    for row, grp in enumerate(np.unique(g)):
        x = np.sort(arrays[1][g == grp])
        assert res.column("g")[row] == grp and res.column("med")[row] == np.percentile(x, 50) and res.column("q")[row] == 1       # (integer-valued halves: exact)
        assert res.column("p90")[row] == x[max(math.ceil(0.9 * len(x)) - 1, 0)]
        assert res.column("cd")[row] == np.count_nonzero(x == x[0]) / len(x)
    every = rs.quantiles(by, order, {"q": ("ntile", 4)})
    assert len(every) == len(rs) and sorted(np.unique(every.column("q")).tolist()) == [1, 2, 3, 4]
    for call, exc in ((lambda: rs.quantiles(by, order, {"x": ("median", "s")}), ValueError), (lambda: rs.quantiles(by, order, {"x": ("nth", "s", 1)}), ValueError),
                      (lambda: rs.quantiles(by, order, {"x": ("nth", "h", 1, 0.5)}), ValueError), (lambda: rs.quantiles(by, order, {"x": ("nth", "h", 1, 1 << 63)}), ValueError),
                      (lambda: rs.quantiles(by, order, {"h": ("ntile", 2)}), KeyError), (lambda: rs.quantiles(by, order, {"x": ("median", "nope")}), KeyError)):
        with pytest.raises(exc):
            call()
    assert rs.quantiles(by, order, {"x": ("nth", "v", 1000, 3)}).column("x").tolist() == [3.0] * len(rs)      # (an int default fits a float64 column)


# ---- the routing decision ------------------------------------------------------------------------------------------------------------
def test_the_route_on_a_stub_engine():
    V = (abi.SORT_VALUE, 0, False, True)

    def eng(switch=True, ext=True, terms=True):
        return SimpleNamespace(device_window_quantile=switch, device_sort=True, ctx=SimpleNamespace(library=SimpleNamespace(has_window_quantile=ext, has_sort_terms=terms)))

    def spec_of(req, measures="plain", terms=None):
        spec = engine._FrameSpec(terms or [K_TERM, V])
        spec.measures = [None if q[2] is None else V for q in req.quants] if measures == "plain" else measures
        return spec
    four = quantile_request(None, ["d"], [("r", "asc")], {"med": ("median", "r"), "p90": ("percentile_disc", "r", 0.9), "q": ("ntile", 4), "cd": ("cume_dist",)}, per=1)
    bare = quantile_request(None, ["d"], [("r", "asc")], {"q": ("ntile", 4), "pr": ("percent_rank",)})
    five = quantile_request(None, ["d"], [("r", "asc")], dict({"x%d" % i: ("ntile", i + 1) for i in range(5)}))
    for req in (four, bare):
        assert engine._order_route(eng(), req, spec_of(req)) == "window_quantile"
        assert engine._order_route(eng(switch=False), req, spec_of(req)) == "host" and engine._order_route(eng(ext=False), req, spec_of(req)) == "host"
        assert engine._order_route(eng(), req, None) == "host"
    assert engine._order_route(eng(), five, spec_of(five)) == "host"       # a fifth column goes to the host: no error
    assert engine._order_route(eng(), four, spec_of(four, measures=None)) == "host"        # a derived or text measure
    ranked = [K_TERM, (abi.SORT_KEY, 0, False, False, 1, 0, 0, "text")]
    assert engine._order_route(eng(), bare, spec_of(bare, terms=ranked)) == "window_quantile" and engine._order_route(eng(terms=False), bare, spec_of(bare, terms=ranked)) == "host"
    # the spec: measures through the plain mapping, None where a function has none, None as a whole where the mapping refuses one
    made = engine._order_spec(four, lambda order, derive: [K_TERM] * len(order), lambda nm: False)
    assert isinstance(made, engine._FrameSpec) and made.measures == [K_TERM, K_TERM, None, None]
    assert engine._order_spec(bare, lambda order, derive: [K_TERM] * len(order) if derive else None, lambda nm: False).measures == [None, None]
    assert engine._order_spec(four, lambda order, derive: [K_TERM] * len(order) if derive else None, lambda nm: False).measures is None
    # an integer-valued double column takes NTH's default as a double: one no double holds stays on the host
    far = quantile_request(None, ["d"], [("r", "asc")], {"x": ("nth", "r", 2, (1 << 53) + 1)})
    near = quantile_request(None, ["d"], [("r", "asc")], {"x": ("nth", "r", 2, 1 << 53)})
    for req, route in ((far, "host"), (near, "window_quantile")):
        spec = spec_of(req)
        spec.int_values = ("r",)
        assert engine._order_route(eng(), req, spec) == route
    assert engine._order_route(eng(), far, spec_of(far)) == "window_quantile"


# ---- through the decorator on the CPU implementation's engine: the host route -------------------------------------------------------
Q3_COLS = {"med": ("median", "revenue"), "p90": ("percentile_disc", "revenue", 0.9), "q": ("ntile", 4), "cd": ("cume_dist",)}
Q3_NOTE = [["med", "percentile_cont", "revenue", None, 0.5, None], ["p90", "percentile_disc", "revenue", None, 0.9, None], ["q", "ntile", None, 4, None, None],
           ["cd", "cume_dist", None, None, None, None]]


def test_q3_on_the_host_route(on_the_decorator, db):
    eng = on_the_decorator
    assert eng.device_window_quantile is True
    args = [db[t] for t in Q.QUERY_TABLES["q3"]]
    by, order = ["o_orderdate"], [("revenue", "asc")]
    plain = Q.q3.order_by([("o_orderdate", "asc")] + order)(*args)
    dates, rev = np.asarray(plain.column("o_orderdate")), np.asarray(plain.column("revenue"))
    assert len(plain) > 300
    for per, per_limit in ((None, ALL), (1, 1)):
        res = Q.q3.quantiles(by, order, Q3_COLS, per=per)(*args)
        assert eng.stats()["order_routes"][-1] == {"route": "host", "k": ALL, "order": ["revenue"], "ranked": [], "per": by, "per_limit": per_limit, "quantiles": Q3_NOTE}
        assert res.columns == plain.columns + list(Q3_COLS) and [res.column(c).dtype for c in Q3_COLS] == [np.float64, np.float64, np.int64, np.float64]
        assert len(res) == (len(plain) if per is None else len(np.unique(dates)))
        at = 0
        for d in np.unique(dates):
            x = rev[dates == d]
            m = len(x)
            rows = range(at, at + (m if per is None else 1))
            assert (np.asarray(res.column("o_orderdate"))[list(rows)] == d).all() and (np.asarray(res.column("revenue"))[list(rows)] == x[:len(rows)]).all()
            t = np.float64(0.5) * np.float64(m - 1)
            lo, hi = math.floor(t), math.ceil(t)
            med = x[lo] if lo == hi else x[lo] + (x[hi] - x[lo]) * (t - np.float64(lo))
            for i, row in enumerate(rows):
                assert res.column("med")[row] == med and res.column("p90")[row] == x[max(math.ceil(np.float64(0.9) * np.float64(m)) - 1, 0)]
                assert res.column("q")[row] == _ntile(i, m, 4)
                assert res.column("cd")[row] == float(Fraction(int(np.count_nonzero(x <= x[i])), m))
            at += len(rows)
        assert at == len(res)
    # a plain top afterwards: today's keys only
    Q.q3.top(10, order)(*args)
    assert sorted(eng.stats()["order_routes"][-1]) == ["k", "order", "ranked", "route"]


def test_argument_errors_come_before_anything_is_launched(on_the_decorator, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("launched")
    monkeypatch.setattr(engine, "execute_plan", never)
    by, order, ok = ["o_orderdate"], [("revenue", "asc")], {"x": ("median", "revenue")}
    for call, exc in ((lambda: Q.q3.quantiles(by, order, {"x": ("mode", "revenue")}), ValueError), (lambda: Q.q3.quantiles(by, order, {"x": ("ntile", 0)}), ValueError),
                      (lambda: Q.q3.quantiles(by, order, {"x": ("nth", "revenue", 0)}), ValueError), (lambda: Q.q3.quantiles(by, order, {"x": ("percentile_cont", "revenue", 1.5)}), ValueError),
                      (lambda: Q.q3.quantiles(by, order, {"x": ("percentile_disc", "revenue", math.nan)}), ValueError), (lambda: Q.q3.quantiles(by, order, ok, per=0), ValueError),
                      (lambda: Q.q3.quantiles(by, order, {}), ValueError), (lambda: Q.q3.quantiles(by, [("revenue", "down")], ok), ValueError),
                      (lambda: Q.q3.quantiles(by, order, {"revenue": ("ntile", 2)}), KeyError), (lambda: Q.q3.quantiles(by, order, {"x": ("median", "revenu")}), KeyError),
                      (lambda: Q.q3.quantiles(["o_orderdat"], order, ok), KeyError), (lambda: Q.q3.quantiles(by, [("revenu", "asc")], ok), KeyError)):
        with pytest.raises(exc):
            call()
    assert callable(Q.q3.quantiles(by, order, ok, per=1)) and callable(Q.q3.quantiles([], order, dict(ok, n=("ntile", 3))))      # nothing runs until it is called
