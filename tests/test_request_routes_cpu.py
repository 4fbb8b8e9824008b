"""The eight requests with partitions (top_per / numbered, over, sliding, ranged, excluding, quantiles, grouping_sets, distincts), one of
each kind through its public builder and through engine._finalize on a stub engine: the route, the entry of Engine.order_routes, the
abi.Context.table_* call with its marshalled columns, the columns and dtypes of the result, the KeyErrors' messages and
dist.refuse_window's — all against literals, so that whoever tells the kinds apart keeps telling them apart the same way.  No GPU and
no library: the stub context records its calls and hands back three rows (one per group for grouping_sets), every device column as
doubles — whatever comes out int64 was rounded back by the engine, for a measure the table keeps as integer-valued doubles."""
from types import SimpleNamespace

import numpy as np
import pytest

from sdqlpy_amd import abi, engine, frontend
from sdqlpy_amd import dist as sdist
from sdqlpy_amd.result import (ResultSet, distinct_request, exclude_request, frame_request, grouping_request, quantile_request, range_request, slide_request,
                               window_request)

ALL = abi.SORT_ALL
K, V = abi.SORT_KEY, abi.SORT_VALUE
COLS = ["grp", "ord", "val"]                 # the result's columns: aliases of the table's key p and of its values k and x
TERMS = [(K, 0, False, False), (V, 1, True, True)]      # PARTITION BY grp ORDER BY ord DESC, as the device takes them
X = (V, 0, True)                             # the measure val = x, a value column: (kind, index, is_f64)


def _f64_bits(x):
    return int(np.array(np.float64(x)).view(np.int64))


# kind (the method's name in the messages; "window": top_per / numbered) -> its request over the result columns `cols` (None: unchecked)
REQUESTS = {
    "window": lambda cols: window_request(cols, ["grp"], [("ord", "desc")], "dense_rank", 2, name="r"),
    "over": lambda cols: frame_request(cols, ["grp"], [("ord", "desc")], {"s": ("sum", "val"), "n": ("count", None, "partition"), "lo": ("min", "val", "rows")}),
    "sliding": lambda cols: slide_request(cols, ["grp"], [("ord", "desc")], {"ma": ("sum", "val", -2, 0, 7), "prev": ("lag", "val", 1), "n": ("count", None, None, 0)}),
    "ranged": lambda cols: range_request(cols, ["grp"], [("ord", "desc")], {"near": ("sum", "val", -1.5, None, 7), "c": ("count", None, -1, 1.0), "f": ("first", "val", None, 0)}),
    "excluding": lambda cols: exclude_request(cols, ["grp"], [("ord", "desc")], {"a": ("avg", "val", -3, 3, 5), "s": ("sum", "val", -1.5, 2, 7, "value"),
                                                                               "c": ("count", None, None, 1, None, "groups"), "m": ("max", "val", None, 0)}, exclude="ties"),
    "quantiles": lambda cols: quantile_request(cols, ["grp"], [("ord", "desc")], {"t": ("ntile", 3), "nth": ("nth", "val", -2, 7), "pd": ("percentile_disc", "val", 0.9),
                                                                                 "med": ("median", "val")}, per=2),
    "grouping_sets": lambda cols: grouping_request(cols, [("grp", ("ord", "desc")), ("grp",), ("ord",)],
                                                   {"s": ("sum", "val"), "n": ("count", None), "a": ("avg", "val"), "h": ("max", "val")}),
    "distincts": lambda cols: distinct_request(cols, [("grp", "desc")], {"m": ("mode", "val"), "s": ("sum_distinct", "val"), "a": ("avg_distinct", "val"),
                                                                        "d": ("count_distinct", "ord"), "n": ("count", None)}),
}


class _Recorder:
    """A context whose table_* calls are written down — (method, the arguments behind the table, keywords) — and answered with three
    rows: keys, no payload, the two value columns, no hits, and one array of doubles per column asked for."""

    def __init__(self):
        self.calls = []
        self.library = SimpleNamespace(has_sort=True, has_sort_terms=True, **{flag: True for flag in abi.WINDOW_EXTENSIONS})

    @staticmethod
    def _rows(n):
        return np.arange(1, n + 1, dtype=np.int64), None, np.array([[10.0, 20.0, 30.0][:n], [3.0, 2.0, 1.0][:n]]), None

    def __getattr__(self, name):
        if not name.startswith("table_"):
            raise AttributeError(name)

        def call(table, *args, **kwargs):
            self.calls.append((name, args, kwargs))
            if name == "table_window":
                return self._rows(3) + (np.array([1, 1, 2], np.int64),)
            if name == "table_grouping_sets":                # one group per level asked for, the levels from the highest down
                levels = [length for length in range(abi.SORT_MAX_KEYS, -1, -1) if args[2] >> length & 1]
                level_rows = np.zeros(abi.SORT_MAX_KEYS + 1, np.int64)
                level_rows[levels] = 1
                return self._rows(len(levels)) + ([np.array([2.0, 4.0, 6.0][:len(levels)]) for _ in args[3]], level_rows)
            return self._rows(3) + ([np.array([2.0, 4.0, 6.0]) for _ in args[3]],)
        return call


def _run(kind):
    """(the order_routes entry, the recorded calls, the ResultSet) of the request `kind` finished by engine._finalize over a table
    keyed by p with the summed values x (integer-valued, kept as doubles) and k, the result's columns their aliases grp, val, ord."""
    ctx = _Recorder()
    eng = SimpleNamespace(ctx=ctx, device_sort=True, order_routes=[], compact_hints={}, lazy_results=False)
    bt = SimpleNamespace(agg=([("p", "key")], ["x", "k"], None, True, True, 2), shared_groups=False, agg_fields={}, int_values=("x",), table=object(), key_radix=None,
                         key_parts=None, key_decoder=None, decoder_of=lambda field, src: None, payload_dtypes={})
    op = SimpleNamespace(source="groups", out="result", lineno=1, fields=[("grp", 0, "p"), ("ord", 1, "k"), ("val", 1, "x")])
    rs = engine._finalize(eng, op, {"groups": ("aggregated", "bt"), "bt": bt}, REQUESTS[kind](COLS))
    assert len(eng.order_routes) == 1
    return eng.order_routes[0], ctx.calls, rs


def _shape(rs):
    return [(name, a.dtype.str) for name, a in zip(rs.columns, rs.arrays)]


SEVEN, FIVE = _f64_bits(7), _f64_bits(5)     # an integer default over a column kept as doubles travels as the double it is there
WANT = {"want_hits": False}
# kind -> (the order_routes entry, the device calls, the result's columns and dtypes)
EXPECTED = {
    "window": (
        {"route": "window", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"], "kind": "dense_rank", "per_limit": 2},
        [("table_window", (1, 1, TERMS, 2, 2, ALL, 4096), {"want_hits": False, "want_rank": True})],
        [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("r", "<i8")]),
    "over": (
        {"route": "window_agg", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"],
         "aggs": [["s", "sum", "val", "range"], ["n", "count", None, "partition"], ["lo", "min", "val", "rows"]]},
        [("table_window_agg", (1, 1, TERMS, [(abi.WAGG_SUM, abi.FRAME_RANGE) + X, (abi.WAGG_COUNT, abi.FRAME_PARTITION, K, 0, False), (abi.WAGG_MIN, abi.FRAME_ROWS) + X], ALL, 4096), WANT)],
        [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("s", "<i8"), ("n", "<f8"), ("lo", "<i8")]),
    "sliding": (
        {"route": "window_slide", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"],
         "slides": [["ma", "sum", "val", -2, 0, 7], ["prev", "first", "val", -1, -1, None], ["n", "count", None, None, 0, None]]},
        [("table_window_slide", (1, 1, TERMS, [(abi.WAGG_SUM,) + X + (-2, 0, SEVEN), (abi.WSLIDE_FIRST,) + X + (-1, -1, 0),
                                               (abi.WAGG_COUNT, K, 0, False, abi.SLIDE_UNBOUNDED_PRECEDING, 0, 0)], ALL, 4096), WANT)],
        [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("ma", "<i8"), ("prev", "<i8"), ("n", "<f8")]),
    "ranged": (
        {"route": "window_range", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"], "unit": "value",
         "ranges": [["near", "sum", "val", -1.5, None, 7], ["c", "count", None, -1, 1.0, None], ["f", "first", "val", None, 0, None]]},
        [("table_window_range", (1, 1, TERMS, [(abi.WAGG_SUM,) + X + (abi.WRANGE_VALUE, -1.5, None, SEVEN), (abi.WAGG_COUNT, K, 0, False, abi.WRANGE_VALUE, -1.0, 1.0, 0),
                                               (abi.WSLIDE_FIRST,) + X + (abi.WRANGE_VALUE, None, 0.0, 0)], ALL, 4096), WANT)],
        [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("near", "<i8"), ("c", "<f8"), ("f", "<i8")]),
    "excluding": (
        {"route": "window_exclude", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"], "exclude": "ties",
         "frames": [["a", "avg", "val", "rows", -3, 3, 5], ["s", "sum", "val", "value", -1.5, 2, 7], ["c", "count", None, "groups", None, 1, None], ["m", "max", "val", "rows", None, 0, None]]},
        [("table_window_exclude", (1, 1, TERMS, [(abi.WEX_AVG,) + X + (abi.WEX_ROWS, -3, 3, FIVE, abi.WEX_TIES), (abi.WAGG_SUM,) + X + (abi.WRANGE_VALUE, -1.5, 2.0, SEVEN, abi.WEX_TIES),
                                                 (abi.WAGG_COUNT, K, 0, False, abi.WRANGE_GROUPS, None, 1, 0, abi.WEX_TIES), (abi.WAGG_MAX,) + X + (abi.WEX_ROWS, None, 0, 0, abi.WEX_TIES)],
                                   ALL, 4096), WANT)],
        [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("a", "<f8"), ("s", "<i8"), ("c", "<f8"), ("m", "<i8")]),
    "quantiles": (
        {"route": "window_quantile", "k": ALL, "order": ["ord"], "ranked": [], "per": ["grp"], "per_limit": 2,
         "quantiles": [["t", "ntile", None, 3, None, None], ["nth", "nth", "val", -2, None, 7], ["pd", "percentile_disc", "val", None, 0.9, None],
                       ["med", "percentile_cont", "val", None, 0.5, None]]},
        [("table_window_quantile", (1, 1, TERMS, [(abi.WQ_NTILE, K, 0, False, 3, 0.0, 0), (abi.WQ_NTH,) + X + (-2, 0.0, SEVEN), (abi.WQ_PERCENTILE_DISC,) + X + (0, 0.9, 0),
                                                  (abi.WQ_PERCENTILE_CONT,) + X + (0, 0.5, 0)], 2, ALL, 4096), WANT)],
        [("grp", "<i8"), ("ord", "<f8"), ("val", "<i8"), ("t", "<f8"), ("nth", "<i8"), ("pd", "<i8"), ("med", "<f8")]),
    "grouping_sets": (
        {"route": "grouping_sets", "k": ALL, "order": [], "ranked": [], "per": ["grp", "ord"], "sets": [["grp", "ord"], ["grp"], ["ord"]],
         "aggs": [["s", "sum", "val"], ["n", "count", None], ["a", "avg", "val"], ["h", "max", "val"]], "calls": 2},
        [("table_grouping_sets", (1, terms, levels, [(abi.WAGG_SUM,) + X, (abi.WAGG_COUNT, K, 0, False), (abi.WEX_AVG,) + X, (abi.WAGG_MAX,) + X], ALL, 4096), WANT)
         for terms, levels in ((TERMS, 0b110), (TERMS[1:], 0b10))],         # the chain (grp, ord) > (grp), and (ord) on its own
        [("grp", "<i8"), ("ord", "<f8"), ("s", "<i8"), ("n", "<f8"), ("a", "<f8"), ("h", "<i8"), ("grouping", "<i8")]),
    "distincts": (                                           # ("aggs" names the table's own columns x and k under aliases: as it always has)
        {"route": "group_distinct", "k": ALL, "order": ["val", "ord"], "ranked": [], "per": ["grp"],
         "aggs": [["m", "mode", "x"], ["s", "sum_distinct", "x"], ["a", "avg_distinct", "x"], ["d", "count_distinct", "k"], ["n", "count", None]], "calls": 2, "host_measures": False},
        [("table_group_distinct", (1, [(K, 0, True, False), (V, 0, False, True)], 1, [(abi.GD_MODE,) + X, (abi.GD_SUM_DISTINCT,) + X, (abi.GD_AVG_DISTINCT,) + X, (abi.GD_COUNT, K, 0, False)],
                                   ALL, 4096), WANT),               # the count rides with the first value column
         ("table_group_distinct", (1, [(K, 0, True, False), (V, 1, False, True)], 1, [(abi.GD_COUNT_DISTINCT, K, 0, False)], ALL, 4096), WANT)],
        [("grp", "<i8"), ("m", "<i8"), ("s", "<i8"), ("a", "<f8"), ("d", "<f8"), ("n", "<f8")]),
}


@pytest.mark.parametrize("kind", list(REQUESTS))
def test_route_note_call_and_result(kind):
    note, calls, rs = _run(kind)
    want_note, want_calls, want_shape = EXPECTED[kind]
    assert note == want_note and list(note) == list(want_note)            # (the keys in their order too)
    assert calls == want_calls
    assert _shape(rs) == want_shape and len(rs) == 3
    if kind == "grouping_sets":                                            # the sets back in listed order, a rolled-up column 0 / NaN
        assert rs.column("grouping").tolist() == [0, 1, 2] and rs.column("grp").tolist() == [1, 2, 0] and np.isnan(rs.column("ord")[1])
    elif kind == "window":
        assert rs.column("r").tolist() == [1, 1, 2]


def test_the_columns_rounded_back_to_int64():
    """What takes its measure's dtype, per kind — for a measure the table keeps as integer-valued doubles the device's doubles are
    rounded back: every op of over / sliding / ranged but count; of excluding / grouping_sets but count and avg; nth and
    percentile_disc of quantiles; sum_distinct and mode of distincts.  (The stub answers every column with doubles.)"""
    rounded = {kind: [name for name, dtype in _shape(_run(kind)[2]) if name not in COLS and dtype == "<i8"] for kind in REQUESTS}
    assert rounded == {"window": ["r"], "over": ["s", "lo"], "sliding": ["ma", "prev"], "ranged": ["near", "f"], "excluding": ["s", "m"], "quantiles": ["nth", "pd"],
                       "grouping_sets": ["s", "h", "grouping"], "distincts": ["m", "s"]}


FIRST_NEW = {"window": "r", "over": "s", "sliding": "ma", "ranged": "near", "excluding": "a", "quantiles": "t", "grouping_sets": "s", "distincts": "m"}


@pytest.mark.parametrize("kind", list(REQUESTS))
def test_column_errors(kind):
    with pytest.raises(KeyError) as e:                                     # a column the result lacks: an order column of a plain window, the measure of the others
        REQUESTS[kind](["grp"] if kind == "window" else ["grp", "ord"])
    assert e.value.args[0] == "%s: the result has no column %r" % (kind, "ord" if kind == "window" else "val")
    with pytest.raises(KeyError) as e:                                     # a new column it has already
        REQUESTS[kind](COLS + [FIRST_NEW[kind]])
    assert e.value.args[0] == "%s: the result already has a column %r" % (kind, FIRST_NEW[kind])
    req = REQUESTS[kind](None)                                             # unchecked until the result is known: the host's methods check
    rows = ResultSet(COLS + [FIRST_NEW[kind]], [np.arange(3), np.arange(3.0), np.arange(3), np.arange(3)])
    with pytest.raises(KeyError) as e:
        rows.windowed(req)
    assert e.value.args[0] == "%s: the result already has a column %r" % (kind, FIRST_NEW[kind])
    if kind not in ("grouping_sets", "distincts"):                         # ... and so does the last mile behind the device (those two build their result anew)
        with pytest.raises(KeyError) as e:
            engine._finish_top(rows, engine._Ranked([np.arange(3)] * 4), req)
        assert e.value.args[0] == "%s: the result already has a column %r" % (kind, FIRST_NEW[kind])


def test_grouping_sets_refuses_a_column_named_grouping():
    with pytest.raises(KeyError) as e:
        grouping_request(COLS, [("grp",)], {"grouping": ("count", None)})
    assert e.value.args[0] == "grouping_sets: the result already has a column 'grouping'"


def test_the_host_serves_every_kind():
    rows = ResultSet(COLS, [np.array([1, 1, 2]), np.array([3.0, 2.0, 1.0]), np.array([10, 20, 30])])
    got = {kind: [c for c in _shape(rows.windowed(REQUESTS[kind](COLS))) if c[0] not in COLS] for kind in REQUESTS}
    assert got == {"window": [("r", "<i8")], "over": [("s", "<i8"), ("n", "<i8"), ("lo", "<i8")], "sliding": [("ma", "<i8"), ("prev", "<i8"), ("n", "<i8")],
                   "ranged": [("near", "<i8"), ("c", "<i8"), ("f", "<i8")], "excluding": [("a", "<f8"), ("s", "<i8"), ("c", "<i8"), ("m", "<i8")],
                   "quantiles": [("t", "<i8"), ("nth", "<i8"), ("pd", "<i8"), ("med", "<f8")], "grouping_sets": [("s", "<i8"), ("n", "<i8"), ("a", "<f8"), ("h", "<i8"), ("grouping", "<i8")],
                   "distincts": [("m", "<i8"), ("s", "<i8"), ("a", "<f8"), ("d", "<i8"), ("n", "<i8")]}


def test_the_multi_gpu_runner_refuses_every_kind():
    said = {}
    for kind in REQUESTS:
        with pytest.raises(frontend.UnsupportedQuery) as e:
            sdist.refuse_window(REQUESTS[kind](None))
        said[kind] = str(e.value)
    tail = ": the multi-GPU runner has no exchange by partition key"
    assert said == {"window": "top_per / numbered run on one GPU" + tail, "over": "over runs on one GPU" + tail, "sliding": "sliding runs on one GPU" + tail,
                    "ranged": "ranged runs on one GPU" + tail, "excluding": "excluding runs on one GPU" + tail, "quantiles": "quantiles runs on one GPU" + tail,
                    "grouping_sets": "grouping_sets runs on one GPU" + tail, "distincts": "distincts runs on one GPU" + tail}
    sdist.refuse_window((10, [("val", "desc")]))                           # a plain top passes
    sdist.refuse_window(None)
