"""Result containers handed back by compiled queries.

The reference returns `sdqlpy.fastd.fastd` around a generated `FastDict_<abbr>_b` object — a
phmap set of result records with size() / to_dict() / print (reference src/sdqlpy/fastd.py:31-51,
src/sdqlpy/lib/fast_dict_generator.py:203-356).  Here a result is struct-of-arrays: one numpy
array per record field, rows in unspecified order (the reference's set is unordered too), with the
same size() / to_dict() surface.
"""
import numpy as np

from .sdql_lib import record, sr_dict


class Dictionary(np.ndarray):
    """The distinct values of a dictionary-coded text column (engine.dict_column): a decoder whose entries are
    pairwise different, so equal codes <=> equal text and grouping can stay on the integer codes."""


class TextRefs:
    """A text column of a large result, not decoded yet: row references (or dictionary codes) as they
    came from the device, and the host array they index.  The reference's result object defers its
    Python conversion to `to_dict()` in the same way (src/sdqlpy/fastd.py:31-51); here K-F's transfer is
    done when the query returns and only the gather of the (wide, UCS-4) strings waits for the first
    read — a 389 K-row Q10 result spends 70 of its 72 ms in that gather."""

    def __init__(self, refs, decoder):
        # own copy of the references: the array handed in may view the pinned result block of the call
        # that produced it, and a lazy column must not keep that block out of the pool
        self.refs, self.decoder = np.array(refs, copy=True), decoder

    dtype = property(lambda self: self.decoder.dtype)
    shape = property(lambda self: self.refs.shape)
    distinct = property(lambda self: isinstance(self.decoder, Dictionary))     # equal references <=> equal text

    def __len__(self):
        return len(self.refs)

    def __array__(self, dtype=None, copy=None):
        a = np.asarray(self.decoder)[self.refs]
        return a if dtype is None else a.astype(dtype)

    def __getitem__(self, idx):
        if isinstance(idx, (int, np.integer)):
            return np.asarray(self.decoder)[self.refs[idx]]
        out = TextRefs.__new__(TextRefs)                          # slices / index arrays stay references
        out.refs, out.decoder = self.refs[idx], self.decoder
        return out

    def tolist(self):
        return np.asarray(self.decoder)[self.refs].tolist()

    # comparisons are element-wise on the decoded text, as for an ndarray (identity comparison of two
    # lazy columns would silently yield one bool)
    def __eq__(self, other):
        return np.asarray(self) == (np.asarray(other) if isinstance(other, TextRefs) else other)

    def __ne__(self, other):
        return np.asarray(self) != (np.asarray(other) if isinstance(other, TextRefs) else other)

    __hash__ = None

    def astype(self, dtype):
        return np.asarray(self).astype(dtype)


LAZY_TEXT_ROWS = 4096        # results with at least this many rows keep their text columns as TextRefs


def decode_text(refs, decoder):
    """decoder[refs], deferred for large results."""
    return TextRefs(refs, decoder) if len(refs) >= LAZY_TEXT_ROWS else np.asarray(decoder)[refs]


WINDOW_KINDS = ("row_number", "rank", "dense_rank")      # their positions are abi.WIN_ROW_NUMBER / WIN_RANK / WIN_DENSE_RANK
WINDOW_ALL = 1 << 62                                      # abi.SORT_ALL: no limit


class WindowRequest(tuple):
    """ORDER BY ... LIMIT per group, travelling where a (k, order) of `top` travels: [0] = the limit on the whole result, [1] = the
    PARTITION BY terms followed by the ORDER BY terms — code that only orders reads it as a plain `top` — and beside them how many of
    the terms partition (npartition), the rank wanted (kind: a position in WINDOW_KINDS), the largest rank kept (per_limit) and the
    name of the rank column the result gets (None: none).

    The requests that travel the same way are its subclasses.  What tells them apart is said here once and declared by each: `method`,
    its name as the user knows it and the prefix of its messages (`terms_method`: the one a missing PARTITION BY / ORDER BY column is
    reported under — a window's, for every kind that keeps the rows); `items_attr`, the attribute that lists its new columns, a tuple
    each with the column's name at [0] and its measure column (or None) at [2] — `items` reads it, () for a plain window; `served_by`,
    the ResultSet method that serves it on the host; `reserved`, names its result takes for itself."""
    method = terms_method = "window"
    items_attr = None
    served_by = "ranked"
    reserved = ()

    def __new__(cls, k, terms, npartition, kind, per_limit, name=None):
        self = tuple.__new__(cls, (int(k), [(str(n), str(d)) for n, d in terms]))
        self.npartition, self.kind, self.per_limit, self.name = int(npartition), int(kind), int(per_limit), name
        if not 0 <= self.npartition <= len(self[1]) or self.kind not in (0, 1, 2):
            raise ValueError("window: bad partition count or kind")
        return self

    by = property(lambda self: self[1][:self.npartition])
    order = property(lambda self: self[1][self.npartition:])

    items = property(lambda self: getattr(self, self.items_attr) if self.items_attr else ())

    def _with(self, terms, items):
        """The request of the same class and settings over `terms` and the columns `items`."""
        return WindowRequest(self[0], terms, self.npartition, self.kind, self.per_limit, self.name)

    def renamed(self, terms, names=None):
        """The same request over other column names: the terms term for term (aliases of the same columns), the measures through
        `names` (old name -> new)."""
        names = names or {}
        return self._with(terms, [item[:2] + (names.get(item[2], item[2]),) + item[3:] for item in self.items])

    def check_columns(self, columns):
        """KeyError for a column the result (its column names: `columns`) lacks, or a new column it has already."""
        for nm, _ in self[1]:
            if nm not in columns:
                raise KeyError("%s: the result has no column %r" % (self.terms_method, nm))
        if self.name is not None and self.name in columns:
            raise KeyError("window: the result already has a column %r" % self.name)
        for item in self.items:                                  # (the value columns of `distincts` are terms: checked above)
            if item[2] is not None and item[2] not in columns:
                raise KeyError("%s: the result has no column %r" % (self.method, item[2]))
            if item[0] in columns or item[0] in self.reserved:
                raise KeyError("%s: the result already has a column %r" % (self.method, item[0]))

    def host(self, rs):
        """The request served on the host: the ResultSet it makes of `rs`."""
        return getattr(rs, self.served_by)(self)


def window_request(columns, by, order, kind, per_limit, k=WINDOW_ALL, name=None):
    """The checked WindowRequest of top_per / numbered: by = names or (name, "asc" | "desc"), order = [(name, "asc" | "desc")], kind a
    name of WINDOW_KINDS.  columns: the result's column names when they are known (None: checked when the result is).  KeyError for a
    column the result lacks or a rank column it has already, ValueError for everything else."""
    if kind not in WINDOW_KINDS:
        raise ValueError("window: kind is one of %s, not %r" % (", ".join(WINDOW_KINDS), kind))
    if int(per_limit) < 1 or int(k) < 1:
        raise ValueError("window: k must be at least 1")
    terms = [(b, "asc") if isinstance(b, str) else (b[0], b[1]) for b in by]
    npartition = len(terms)
    terms += [(o, "asc") if isinstance(o, str) else (o[0], o[1]) for o in order]
    if any(d not in ("asc", "desc") for _, d in terms):
        raise ValueError("window: directions are 'asc' or 'desc'")
    if not terms:
        raise ValueError("window: nothing to partition or order by")
    if name is not None and not isinstance(name, str):
        raise ValueError("window: the rank column's name is a string")
    req = WindowRequest(k, terms, npartition, WINDOW_KINDS.index(kind), min(int(per_limit), WINDOW_ALL), name)
    if columns is not None:
        req.check_columns(columns)
    return req


def _aggs_dict(who, aggs, shape, what="aggs", empty_ok=False):
    """The dict a builder takes its new columns from, {new column: `shape`}: ValueError (under the method's name `who`) for anything else."""
    if not isinstance(aggs, dict) or not (aggs or empty_ok):
        raise ValueError("%s: %s is a %sdict {new column: %s}" % (who, what, "" if empty_ok else "non-empty ", shape))


def _agg_spec(who, name, spec, shape, fits, what="an aggregate"):
    """One entry of that dict: a name and a tuple or list whose length fits(len)."""
    if not isinstance(name, str) or not isinstance(spec, (tuple, list)) or not fits(len(spec)):
        raise ValueError("%s: %s is name: %s" % (who, what, shape))


def _agg_measure(who, op, col):
    """An aggregate's measure: a column name, or None for a count."""
    if col is None and op != "count":
        raise ValueError("%s: %s needs a measure column" % (who, op))
    if col is not None and not isinstance(col, str):
        raise ValueError("%s: a measure is a column name" % who)


def _agg_default(who, default):
    if default is not None and (isinstance(default, bool) or not isinstance(default, (int, float, np.integer, np.floating))):
        raise ValueError("%s: a default is a number, not %r" % (who, default))


def _agg_frame(who, lo, hi):
    if lo is not None and hi is not None and lo > hi:
        raise ValueError("%s: the frame (%r, %r) ends before it starts" % (who, lo, hi))


WAGG_OPS = ("sum", "count", "min", "max")                 # their positions are abi.WAGG_SUM / WAGG_COUNT / WAGG_MIN / WAGG_MAX
FRAMES = ("rows", "range", "partition")                   # ... abi.FRAME_ROWS / FRAME_RANGE / FRAME_PARTITION


class FrameRequest(WindowRequest):
    """Aggregates over window frames, travelling where a WindowRequest travels (every row is kept: it reads as ROW_NUMBER with no
    per-group limit and no rank column): [0] = the limit on the whole result, [1] = the PARTITION BY terms followed by the ORDER BY
    terms, npartition, and aggs = [(name of the new column, op: a name of WAGG_OPS, measure column or None for a count, frame: a
    name of FRAMES)] in the order the columns are appended."""
    method, items_attr, served_by = "over", "aggs", "framed"

    def __new__(cls, k, terms, npartition, aggs):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, WINDOW_ALL, None)
        self.aggs = [(str(n), str(op), None if col is None else str(col), str(fr)) for n, op, col, fr in aggs]
        if not self.aggs or any(op not in WAGG_OPS or fr not in FRAMES or (col is None and op != "count") for _, op, col, fr in self.aggs):
            raise ValueError("over: bad aggregate")
        return self

    def _with(self, terms, items):
        return FrameRequest(self[0], terms, self.npartition, items)


def frame_request(columns, by, order, aggs, frame="range", k=WINDOW_ALL):
    """The checked FrameRequest of `over`: by / order as window_request takes them; aggs = {new column: (op, measure column or None)
    or (op, measure, frame)} with op a name of WAGG_OPS and frame a name of FRAMES (default: `frame`).  columns: the result's column
    names when they are known (None: checked when the result is).  KeyError for a column the result lacks or a new column it has
    already, ValueError for everything else."""
    req = window_request(None, by, order, "row_number", WINDOW_ALL, k=k)     # (its checks of by / order / k)
    _aggs_dict("over", aggs, "(op, measure[, frame])")
    if frame not in FRAMES:
        raise ValueError("over: frame is one of %s, not %r" % (", ".join(FRAMES), frame))
    out = []
    for name, spec in aggs.items():
        _agg_spec("over", name, spec, "(op, measure[, frame])", lambda n: n in (2, 3))
        op, col, fr = spec[0], spec[1], (spec[2] if len(spec) == 3 else frame)
        if op not in WAGG_OPS:
            raise ValueError("over: op is one of %s, not %r" % (", ".join(WAGG_OPS), op))
        if fr not in FRAMES:
            raise ValueError("over: frame is one of %s, not %r" % (", ".join(FRAMES), fr))
        _agg_measure("over", op, col)
        out.append((name, op, col, fr))
    req = FrameRequest(req[0], req[1], req.npartition, out)
    if columns is not None:
        req.check_columns(columns)
    return req


SLIDE_OPS = ("sum", "count", "min", "max", "first", "last")      # their positions are abi.WAGG_SUM .. WAGG_MAX, WSLIDE_FIRST, WSLIDE_LAST


class SlideRequest(WindowRequest):
    """Values over sliding window frames, travelling where a FrameRequest travels (every row is kept): [0] = the limit on the whole
    result, [1] = the PARTITION BY terms followed by the ORDER BY terms, npartition, and slides = [(name of the new column, op: a name
    of SLIDE_OPS, measure column or None for a count, lo, hi: the frame's offsets from the row — negative = preceding, None =
    unbounded —, default: what an empty frame gives, None = 0 for an int64 measure and NaN for a float64 one)] in the order the
    columns are appended.  lag / lead are `first` over (-k, -k) / (k, k) by the time they are here."""
    method, items_attr, served_by = "sliding", "slides", "slid"

    def __new__(cls, k, terms, npartition, slides):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, WINDOW_ALL, None)
        self.slides = [(str(n), str(op), None if col is None else str(col), lo, hi, default) for n, op, col, lo, hi, default in slides]
        if not self.slides or any(op not in SLIDE_OPS or (col is None and op != "count") or (lo is not None and hi is not None and lo > hi)
                                  for _, op, col, lo, hi, _ in self.slides):
            raise ValueError("sliding: bad aggregate")
        return self

    def _with(self, terms, items):
        return SlideRequest(self[0], terms, self.npartition, items)


def _slide_int(x, what, who="sliding"):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise ValueError("%s: %s is an integer, not %r" % (who, what, x))
    return int(x)


def slide_request(columns, by, order, aggs, k=WINDOW_ALL):
    """The checked SlideRequest of `sliding`: by / order as window_request takes them; aggs = {new column: (op, measure column or None,
    lo, hi[, default])} with op a name of SLIDE_OPS and lo / hi ints relative to the row (negative = preceding, None = unbounded), or
    ("lag" | "lead", measure, k[, default]) with k >= 0: `first` over (-k, -k) / (k, k).  columns: the result's column names when they
    are known (None: checked when the result is).  KeyError for a column the result lacks or a new column it has already, ValueError
    for everything else (a default that does not fit its column is found when the column is known: slide_empty)."""
    req = window_request(None, by, order, "row_number", WINDOW_ALL, k=k)     # (its checks of by / order / k)
    _aggs_dict("sliding", aggs, "(op, measure, lo, hi[, default])")
    out = []
    for name, spec in aggs.items():
        _agg_spec("sliding", name, spec, "(op, measure, lo, hi[, default]) or (lag | lead, measure, k[, default])", lambda n: n >= 2)
        op, col = spec[0], spec[1]
        if op in ("lag", "lead"):
            if len(spec) not in (3, 4):
                raise ValueError("sliding: %s is (%s, measure, k[, default])" % (op, op))
            back = _slide_int(spec[2], "k")
            if back < 0:
                raise ValueError("sliding: k is at least 0")
            lo = hi = -back if op == "lag" else back
            op, default = "first", (spec[3] if len(spec) == 4 else None)
        else:
            if op not in SLIDE_OPS:
                raise ValueError("sliding: op is one of %s, lag, lead, not %r" % (", ".join(SLIDE_OPS), op))
            _agg_spec("sliding", name, spec, "(op, measure, lo, hi[, default])", lambda n: n in (4, 5))
            lo = None if spec[2] is None else _slide_int(spec[2], "a bound")
            hi = None if spec[3] is None else _slide_int(spec[3], "a bound")
            default = spec[4] if len(spec) == 5 else None
            _agg_frame("sliding", lo, hi)
        _agg_measure("sliding", op, col)
        _agg_default("sliding", default)
        out.append((name, op, col, lo, hi, default))
    req = SlideRequest(req[0], req[1], req.npartition, out)
    if columns is not None:
        req.check_columns(columns)
    return req


RANGE_UNITS = ("value", "groups")       # their positions are abi.WRANGE_VALUE / WRANGE_GROUPS


class RangeRequest(WindowRequest):
    """Values over value and group window frames, travelling where a SlideRequest travels (every row is kept): [0] = the limit on the
    whole result, [1] = the PARTITION BY terms followed by the ORDER BY terms, npartition, unit (a name of RANGE_UNITS) and ranges =
    [(name of the new column, op: a name of SLIDE_OPS, measure column or None for a count, lo, hi: the frame's offsets along the order
    — of the ORDER BY value (unit "value": ints or floats) or in tie runs (unit "groups": ints), negative = preceding, None = unbounded
    —, default: what an empty frame gives, None = 0 for an int64 measure and NaN for a float64 one)] in the order the columns are
    appended."""
    method, items_attr, served_by = "ranged", "ranges", "ranged_by"

    def __new__(cls, k, terms, npartition, unit, ranges):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, WINDOW_ALL, None)
        self.unit = str(unit)
        self.ranges = [(str(n), str(op), None if col is None else str(col), lo, hi, default) for n, op, col, lo, hi, default in ranges]
        if self.unit not in RANGE_UNITS or not self.ranges or any(op not in SLIDE_OPS or (col is None and op != "count") or (lo is not None and hi is not None and lo > hi)
                                                                   for _, op, col, lo, hi, _ in self.ranges):
            raise ValueError("ranged: bad aggregate")
        if self.unit == "value" and len(terms) != npartition + 1:
            raise ValueError("ranged: a value frame is ordered by exactly one column")
        return self

    def _with(self, terms, items):
        return RangeRequest(self[0], terms, self.npartition, self.unit, items)


def _range_offset(x, unit, who="ranged"):
    """A frame offset of `ranged` (or `excluding`): an int, or — unit "value" only — a finite float."""
    if not isinstance(x, bool) and isinstance(x, (int, np.integer)):
        return int(x)
    if unit == "value" and isinstance(x, (float, np.floating)) and np.isfinite(x):
        return float(x)
    raise ValueError("%s: a bound is %s, not %r" % (who, "an integer or a finite float" if unit == "value" else "an integer", x))


def range_request(columns, by, order, aggs, unit="value", k=WINDOW_ALL):
    """The checked RangeRequest of `ranged`: by / order as window_request takes them; unit a name of RANGE_UNITS; aggs = {new column:
    (op, measure column or None, lo, hi[, default])} with op a name of SLIDE_OPS and lo / hi offsets along the order (negative =
    preceding, None = unbounded): ints, or floats as well for unit "value".  columns: the result's column names when they are known
    (None: checked when the result is).  KeyError for a column the result lacks or a new column it has already, ValueError for
    everything else (a default that does not fit its column, or an order column without arithmetic, is found when the column is
    known)."""
    req = window_request(None, by, order, "row_number", WINDOW_ALL, k=k)     # (its checks of by / order / k)
    if unit not in RANGE_UNITS:
        raise ValueError("ranged: unit is one of %s, not %r" % (", ".join(RANGE_UNITS), unit))
    if unit == "value" and len(req[1]) != req.npartition + 1:
        raise ValueError("ranged: a value frame is ordered by exactly one column, not %d" % (len(req[1]) - req.npartition))
    _aggs_dict("ranged", aggs, "(op, measure, lo, hi[, default])")
    out = []
    for name, spec in aggs.items():
        _agg_spec("ranged", name, spec, "(op, measure, lo, hi[, default])", lambda n: n in (4, 5))
        op, col = spec[0], spec[1]
        if op not in SLIDE_OPS:
            raise ValueError("ranged: op is one of %s, not %r" % (", ".join(SLIDE_OPS), op))
        lo = None if spec[2] is None else _range_offset(spec[2], unit)
        hi = None if spec[3] is None else _range_offset(spec[3], unit)
        default = spec[4] if len(spec) == 5 else None
        _agg_frame("ranged", lo, hi)
        _agg_measure("ranged", op, col)
        _agg_default("ranged", default)
        out.append((name, op, col, lo, hi, default))
    req = RangeRequest(req[0], req[1], req.npartition, unit, out)
    if columns is not None:
        req.check_columns(columns)
    return req


def _range_int_offset(x):
    """A frame offset over an integer order column as an int: an int as it is, an integral float converted; ValueError otherwise."""
    if x is None or isinstance(x, (int, np.integer)):
        return x if x is None else int(x)
    if float(x) != int(x):
        raise ValueError("ranged: the offset %r over an integer column is not an integer" % (x,))
    return int(x)


EXCLUDES = ("no others", "current row", "group", "ties")      # their positions are abi.WEX_NO_OTHERS .. WEX_TIES
EXCLUDE_UNITS = ("value", "groups", "rows")                   # ... abi.WRANGE_VALUE / WRANGE_GROUPS / WEX_ROWS
EXCLUDE_OPS = SLIDE_OPS + ("avg",)                            # ... abi.WAGG_SUM .. WSLIDE_LAST, WEX_AVG


class ExcludeRequest(WindowRequest):
    """Values over window frames with rows taken out, travelling where a RangeRequest travels (every row is kept): [0] = the limit on
    the whole result, [1] = the PARTITION BY terms followed by the ORDER BY terms, npartition, exclude (a name of EXCLUDES: what is cut
    out of every frame) and frames = [(name of the new column, op: a name of EXCLUDE_OPS, measure column or None for a count, unit: a
    name of EXCLUDE_UNITS — the column's own —, lo, hi: the frame's offsets in that unit, negative = preceding, None = unbounded,
    default: what a column gives where nothing remains, None = 0 for an int64 column and NaN for a float64 one)] in the order the
    columns are appended."""
    method, items_attr, served_by = "excluding", "frames", "excluded"

    def __new__(cls, k, terms, npartition, exclude, frames):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, WINDOW_ALL, None)
        self.exclude = str(exclude)
        self.frames = [(str(n), str(op), None if col is None else str(col), str(unit), lo, hi, default) for n, op, col, unit, lo, hi, default in frames]
        if self.exclude not in EXCLUDES or not self.frames or any(op not in EXCLUDE_OPS or unit not in EXCLUDE_UNITS or (col is None and op != "count") or
                                                                   (lo is not None and hi is not None and lo > hi) for _, op, col, unit, lo, hi, _ in self.frames):
            raise ValueError("excluding: bad aggregate")
        if any(unit == "value" for _, _, _, unit, _, _, _ in self.frames) and len(terms) != npartition + 1:
            raise ValueError("excluding: a value frame is ordered by exactly one column")
        return self

    def _with(self, terms, items):
        return ExcludeRequest(self[0], terms, self.npartition, self.exclude, items)


def exclude_request(columns, by, order, aggs, exclude="current row", unit="rows", k=WINDOW_ALL):
    """The checked ExcludeRequest of `excluding`: by / order as window_request takes them; exclude a name of EXCLUDES; unit a name of
    EXCLUDE_UNITS, the unit of every column that names none; aggs = {new column: (op, measure column or None, lo, hi[, default]) or
    (op, measure, lo, hi, default, unit)} with op a name of EXCLUDE_OPS and lo / hi offsets in the column's unit (negative =
    preceding, None = unbounded): ints, or floats as well for unit "value".  columns: the result's column names when they are known
    (None: checked when the result is).  The checks and their errors are range_request's: KeyError for a column the result lacks or
    a new column it has already, ValueError for everything else."""
    req = window_request(None, by, order, "row_number", WINDOW_ALL, k=k)     # (its checks of by / order / k)
    if exclude not in EXCLUDES:
        raise ValueError("excluding: exclude is one of %s, not %r" % (", ".join(EXCLUDES), exclude))
    if unit not in EXCLUDE_UNITS:
        raise ValueError("excluding: unit is one of %s, not %r" % (", ".join(EXCLUDE_UNITS), unit))
    _aggs_dict("excluding", aggs, "(op, measure, lo, hi[, default[, unit]])")
    out = []
    for name, spec in aggs.items():
        _agg_spec("excluding", name, spec, "(op, measure, lo, hi[, default[, unit]])", lambda n: n in (4, 5, 6))
        op, col = spec[0], spec[1]
        own = spec[5] if len(spec) == 6 else unit
        if op not in EXCLUDE_OPS:
            raise ValueError("excluding: op is one of %s, not %r" % (", ".join(EXCLUDE_OPS), op))
        if own not in EXCLUDE_UNITS:
            raise ValueError("excluding: a column's unit is one of %s, not %r" % (", ".join(EXCLUDE_UNITS), own))
        if own == "value" and len(req[1]) != req.npartition + 1:
            raise ValueError("excluding: a value frame is ordered by exactly one column, not %d" % (len(req[1]) - req.npartition))
        lo = None if spec[2] is None else _range_offset(spec[2], own, "excluding")
        hi = None if spec[3] is None else _range_offset(spec[3], own, "excluding")
        default = spec[4] if len(spec) >= 5 else None
        _agg_frame("excluding", lo, hi)
        _agg_measure("excluding", op, col)
        _agg_default("excluding", default)
        out.append((name, op, col, own, lo, hi, default))
    req = ExcludeRequest(req[0], req[1], req.npartition, exclude, out)
    if columns is not None:
        req.check_columns(columns)
    return req


QUANTILE_FNS = ("ntile", "percent_rank", "cume_dist", "nth", "percentile_disc", "percentile_cont")     # their positions are abi.WQ_NTILE .. WQ_PERCENTILE_CONT


class QuantileRequest(WindowRequest):
    """Functions of the partition's size, travelling where a WindowRequest travels — and filtering as one: it reads as ROW_NUMBER with
    per_limit (the rows whose row number in their group is at most per_limit are kept; WINDOW_ALL: every row) and no rank column.
    quants = [(name of the new column, fn: a name of QUANTILE_FNS, measure column or None, arg: NTILE's b / NTH's k or None, p: a
    percentile's or None, default: what NTH gives beyond the group, None = 0 for an int64 measure and NaN for a float64 one)] in the
    order the columns are appended.  median is percentile_cont at 0.5 by the time it is here."""
    method, items_attr, served_by = "quantiles", "quants", "quantiled"

    def __new__(cls, k, terms, npartition, per_limit, quants):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, per_limit, None)
        self.quants = [(str(n), str(fn), None if col is None else str(col), arg, p, default) for n, fn, col, arg, p, default in quants]
        if not self.quants or self.per_limit < 1 or any(fn not in QUANTILE_FNS or ((col is None) != (fn in QUANTILE_FNS[:3])) for _, fn, col, _, _, _ in self.quants):
            raise ValueError("quantiles: bad column")
        return self

    def _with(self, terms, items):
        return QuantileRequest(self[0], terms, self.npartition, self.per_limit, items)


def quantile_request(columns, by, order, cols, per=None, k=WINDOW_ALL):
    """The checked QuantileRequest of `quantiles`: by / order as window_request takes them; cols = {new column: ("ntile", b) |
    ("percent_rank",) | ("cume_dist",) | ("nth", measure, k[, default]) | ("percentile_disc", measure, p) | ("percentile_cont",
    measure, p) | ("median", measure)} with 1 <= b < 2^63, k != 0 inside int64 (negative: from the group's end), 0 <= p <= 1; per: only
    the first `per` rows of every group are returned (None: all; 1: one row per group).  columns: the result's column names when they
    are known (None: checked when the result is).  KeyError for a column the result lacks or a new column it has already, ValueError
    for everything else (a default that does not fit its column is found when the column is known: slide_empty)."""
    if per is not None and (isinstance(per, bool) or not isinstance(per, (int, np.integer)) or int(per) < 1):
        raise ValueError("quantiles: per is None or an integer of at least 1, not %r" % (per,))
    req = window_request(None, by, order, "row_number", WINDOW_ALL if per is None else int(per), k=k)     # (its checks of by / order / k)
    _aggs_dict("quantiles", cols, "(function, ...)", what="cols")
    shapes = {"ntile": (2,), "percent_rank": (1,), "cume_dist": (1,), "nth": (3, 4), "percentile_disc": (3,), "percentile_cont": (3,), "median": (2,)}
    out = []
    for name, spec in cols.items():
        _agg_spec("quantiles", name, spec, "(function, ...)", lambda n: n >= 1, what="a column")
        fn = spec[0]
        if not isinstance(fn, str) or fn not in shapes:
            raise ValueError("quantiles: the function is one of %s, median, not %r" % (", ".join(QUANTILE_FNS), fn))
        if len(spec) not in shapes[fn]:
            raise ValueError("quantiles: %s takes %s arguments, not %d" % (fn, " or ".join(str(s - 1) for s in shapes[fn]), len(spec) - 1))
        col = arg = p = default = None
        if fn == "ntile":
            arg = _slide_int(spec[1], "b", "quantiles")
            if not 1 <= arg < (1 << 63):
                raise ValueError("quantiles: ntile's b is at least 1 and fits int64, not %d" % arg)
        elif fn in ("nth", "percentile_disc", "percentile_cont", "median"):
            col = spec[1]
            if not isinstance(col, str):
                raise ValueError("quantiles: a measure is a column name, not %r" % (col,))
            if fn == "nth":
                arg = _slide_int(spec[2], "k", "quantiles")
                if arg == 0 or not -(1 << 63) <= arg < (1 << 63):
                    raise ValueError("quantiles: nth's k is not 0 and fits int64, not %d" % arg)
                default = spec[3] if len(spec) == 4 else None
                _agg_default("quantiles", default)
            else:
                p = 0.5 if fn == "median" else spec[2]
                if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:      # (a NaN fails both)
                    raise ValueError("quantiles: p lies in [0, 1], not %r" % (p,))
                p = float(p)
                fn = "percentile_cont" if fn == "median" else fn
        out.append((name, fn, col, arg, p, default))
    req = QuantileRequest(req[0], req[1], req.npartition, req.per_limit, out)
    if columns is not None:
        req.check_columns(columns)
    return req


GROUP_OPS = ("sum", "count", "min", "max", "avg")          # abi.WAGG_SUM / WAGG_COUNT / WAGG_MIN / WAGG_MAX, and abi.WEX_AVG


class GroupingRequest(WindowRequest):
    """GROUP BY GROUPING SETS over a result, travelling where a WindowRequest travels (it reads as an ORDER BY of every grouping
    column): [1] = `by`, the union of the sets' columns in order of first appearance with their directions; sets = the column tuples
    in the order listed; aggs = [(name of the new column, op: a name of GROUP_OPS, measure column or None for a count)].  The result
    holds `by`, the aggregates and an int64 column "grouping" (SQL's GROUPING(by...): bit len(by) - 1 - i set where by[i] is rolled
    up in the row; such a column holds 0 / NaN / ""); every other column of the query's result is dropped.  The sets come in the
    order listed, inside a set the rows are ordered by the set's columns as the set lists them."""
    method = terms_method = "grouping_sets"
    items_attr, served_by, reserved = "aggs", "grouped", ("grouping",)

    def __new__(cls, terms, sets, aggs):
        self = WindowRequest.__new__(cls, WINDOW_ALL, terms, len(terms), 0, WINDOW_ALL, None)
        self.sets = [tuple(str(c) for c in s) for s in sets]
        self.aggs = [(str(n), str(op), None if col is None else str(col)) for n, op, col in aggs]
        names = [nm for nm, _ in self[1]]
        if not self.sets or len(set(self.sets)) != len(self.sets) or any(len(set(s)) != len(s) or any(c not in names for c in s) for s in self.sets):
            raise ValueError("grouping_sets: bad sets")
        if any(op not in GROUP_OPS or (col is None and op != "count") for _, op, col in self.aggs):
            raise ValueError("grouping_sets: bad aggregate")
        return self

    def _with(self, terms, items):
        to = {old: new for (old, _), (new, _) in zip(self[1], terms)}      # (the sets follow `by`)
        return GroupingRequest(terms, [tuple(to[c] for c in s) for s in self.sets], items)

    def chains(self):
        """The sets as the device serves them: [(the chain's column tuple, {level: index of the set it serves})].  A set rides in
        another set's chain iff its tuple is a prefix of that set's; a chain is one call over its longest tuple, `levels` = the
        members' lengths.  Every set is served exactly once."""
        out = []
        for i in sorted(range(len(self.sets)), key=lambda i: -len(self.sets[i])):      # (stable: longest first, then as listed)
            s = self.sets[i]
            for head, members in out:
                if head[:len(s)] == s and len(s) not in members:
                    members[len(s)] = i
                    break
            else:
                out.append((s, {len(s): i}))
        return out

    def masks(self):
        """the `grouping` value of every set's rows"""
        names = [nm for nm, _ in self[1]]
        return [sum(1 << (len(names) - 1 - i) for i, nm in enumerate(names) if nm not in s) for s in self.sets]


def grouping_request(columns, sets, aggs):
    """The checked GroupingRequest of rollup / cube / grouping_sets: sets = a list of column tuples, a column `name` or (name, "asc" |
    "desc"); aggs = {new column: (op, measure column or None)} with op a name of GROUP_OPS (an empty dict: the distinct combinations
    alone).  columns: the result's column names when they are known (None: checked when the result is).  KeyError for a column the
    result lacks or a new column it has already, ValueError for everything else."""
    if not isinstance(sets, (list, tuple)) or not sets:
        raise ValueError("grouping_sets: sets is a non-empty list of column tuples")
    direction, listed = {}, []
    for s in sets:
        if isinstance(s, str) or not isinstance(s, (list, tuple)):
            raise ValueError("grouping_sets: a set is a tuple of columns")
        cols = []
        for c in s:
            name, d = (c, None) if isinstance(c, str) else (c[0], c[1]) if isinstance(c, (list, tuple)) and len(c) == 2 else (None, None)
            if not isinstance(name, str) or d not in (None, "asc", "desc"):
                raise ValueError("grouping_sets: a column is a name or (name, 'asc' | 'desc')")
            if name in cols:
                raise ValueError("grouping_sets: column %r comes twice in one set" % name)
            if d is not None and direction.get(name, d) != d:
                raise ValueError("grouping_sets: column %r has two directions" % name)
            if d is not None or name not in direction:
                direction[name] = d
            cols.append(name)
        if tuple(cols) in listed:
            raise ValueError("grouping_sets: the set %r comes twice" % (tuple(cols),))
        listed.append(tuple(cols))
    _aggs_dict("grouping_sets", aggs, "(op, measure)", empty_ok=True)
    out = []
    for name, spec in aggs.items():
        _agg_spec("grouping_sets", name, spec, "(op, measure)", lambda n: n == 2)
        op, col = spec
        if op not in GROUP_OPS:
            raise ValueError("grouping_sets: op is one of %s, not %r" % (", ".join(GROUP_OPS), op))
        _agg_measure("grouping_sets", op, col)
        out.append((name, op, col))
    req = GroupingRequest([(nm, d or "asc") for nm, d in direction.items()], listed, out)
    if columns is not None:
        req.check_columns(columns)
    return req


def rollup_sets(by):
    """by[:d], by[:d - 1], ..., ()"""
    by = list(by)
    return [tuple(by[:d]) for d in range(len(by), -1, -1)]


def cube_sets(by):
    """every subset of `by`, in by's order, by ascending `grouping` mask (bit len(by) - 1 - i: by[i] is rolled up)"""
    by = list(by)
    return [tuple(c for i, c in enumerate(by) if not (mask >> (len(by) - 1 - i)) & 1) for mask in range(1 << len(by))]


def _rolled_up(a, n):
    """n values of what a rolled-up column of a's dtype holds: 0, NaN or the empty text"""
    a = np.asarray(a)
    return np.full(n, np.nan, a.dtype) if a.dtype.kind == "f" else np.zeros(n, a.dtype if a.dtype.kind in "iubU" else object)


def grouped_result(req, column_of, pieces):
    """The ResultSet of a GroupingRequest out of its sets' rows, whoever grouped them: pieces[s] = ({column of set s: its groups'
    values}, [one array per aggregate], the number of groups) for every set; column_of(name): the source column (for the dtype of what a rolled-up column
    holds).  The sets in the order listed, rolled-up columns filled, the `grouping` column last."""
    names = [nm for nm, _ in req[1]]
    masks = req.masks()
    sizes = [m for _, _, m in pieces]
    cols = []
    for nm in names:
        src = column_of(nm)
        parts = [np.asarray(by[nm]) if nm in by else _rolled_up(src, m) for (by, _, _), m in zip(pieces, sizes)]
        cols.append(np.concatenate(parts) if parts else np.asarray(src)[:0])
    for a in range(len(req.aggs)):
        cols.append(np.concatenate([np.asarray(aggs[a]) for _, aggs, _ in pieces]))
    cols.append(np.concatenate([np.full(m, mask, np.int64) for m, mask in zip(sizes, masks)]))
    return ResultSet(names + [n for n, _, _ in req.aggs] + ["grouping"], cols)


DISTINCT_OPS = ("count_distinct", "sum_distinct", "avg_distinct", "mode", "mode_count", "count")      # their positions are abi.GD_COUNT_DISTINCT .. GD_COUNT
DISTINCT_MEASURED = ("sum_distinct", "avg_distinct", "mode")      # the ops that read their value column's values, not only its runs
DISTINCT_MAX_AGGS = 4                                      # abi.GD_MAX_AGGS: the aggregates of one device call


class DistinctRequest(WindowRequest):
    """Aggregates over the distinct values of a group, travelling where a WindowRequest travels: [1] = the grouping columns `by` with
    their directions (npartition of them) followed by the value columns, ascending, in order of first appearance; aggs = [(name of
    the new column, op: a name of DISTINCT_OPS, value column or None for a count)].  The result holds `by` and the aggregates, one row
    per group, ordered by `by`; every other column of the query's result is dropped."""
    method = terms_method = "distincts"
    items_attr, served_by = "aggs", "distincted"

    def __new__(cls, by, aggs):
        aggs = [(str(n), str(op), None if col is None else str(col)) for n, op, col in aggs]
        values = list(dict.fromkeys(col for _, _, col in aggs if col is not None))
        self = WindowRequest.__new__(cls, WINDOW_ALL, list(by) + [(v, "asc") for v in values], len(by), 0, WINDOW_ALL, None)
        self.aggs = aggs
        names = [nm for nm, _ in self.by]
        if not aggs or len(set(names)) != len(names) or any(v in names for v in values):
            raise ValueError("distincts: bad columns")
        if any(op not in DISTINCT_OPS or (col is None) != (op == "count") for _, op, col in aggs):
            raise ValueError("distincts: bad aggregate")
        return self

    values = property(lambda self: [nm for nm, _ in self.order])

    def renamed(self, terms, names=None):
        """The same request over other column names: the terms one for one, the value columns with them."""
        to = {old: new for (old, _), (new, _) in zip(self[1], terms)}
        return DistinctRequest(terms[:self.npartition], [(n, op, to.get(col, col)) for n, op, col in self.aggs])

    def calls(self):
        """The aggregates as the device serves them: [(value column, [indices into aggs])], one call per value column in order of
        first appearance, a `count` riding in the first call that has room — or None where the device cannot: no value column at
        all, or more than DISTINCT_MAX_AGGS aggregates in one call."""
        out = [(v, [i for i, (_, _, col) in enumerate(self.aggs) if col == v]) for v in self.values]
        for i, (_, _, col) in enumerate(self.aggs):
            if col is None:
                room = [idx for _, idx in out if len(idx) < DISTINCT_MAX_AGGS]
                if not room:
                    return None
                room[0].append(i)
        return out if out and all(len(idx) <= DISTINCT_MAX_AGGS for _, idx in out) else None


def distinct_request(columns, by, aggs):
    """The checked DistinctRequest of distincts: by = a list of columns, a column `name` or (name, "asc" | "desc") (an empty list: the
    whole result is one group); aggs = {new column: (op, value column)} with op a name of DISTINCT_OPS — "count" takes None, every
    other op a column name.  columns: the result's column names when they are known (None: checked when the result is).  KeyError for
    a column the result lacks or a new column it has already, ValueError for everything else."""
    if isinstance(by, str) or not isinstance(by, (list, tuple)):
        raise ValueError("distincts: by is a list of columns")
    terms = []
    for c in by:
        name, d = (c, "asc") if isinstance(c, str) else (c[0], c[1]) if isinstance(c, (list, tuple)) and len(c) == 2 else (None, None)
        if not isinstance(name, str) or d not in ("asc", "desc"):
            raise ValueError("distincts: a column is a name or (name, 'asc' | 'desc')")
        if name in [nm for nm, _ in terms]:
            raise ValueError("distincts: column %r comes twice in by" % name)
        terms.append((name, d))
    _aggs_dict("distincts", aggs, "(op, value column)")
    out = []
    for name, spec in aggs.items():
        _agg_spec("distincts", name, spec, "(op, value column)", lambda n: n == 2)
        op, col = spec
        if op not in DISTINCT_OPS:
            raise ValueError("distincts: op is one of %s, not %r" % (", ".join(DISTINCT_OPS), op))
        if op == "count":
            if col is not None:
                raise ValueError("distincts: count takes no value column (None)")
        elif not isinstance(col, str):
            raise ValueError("distincts: %s needs a value column, a column name" % op)
        elif col in [nm for nm, _ in terms]:
            raise ValueError("distincts: the value column %r is a grouping column" % col)
        out.append((name, op, col))
    if len(set(n for n, _, _ in out) | set(nm for nm, _ in terms)) != len(out) + len(terms):
        raise ValueError("distincts: a new column has the name of a grouping column")
    req = DistinctRequest(terms, out)
    if columns is not None:
        req.check_columns(columns)
    return req


MOMENT_OPS = ("var_pop", "var_samp", "stddev_pop", "stddev_samp", "covar_pop", "covar_samp", "corr", "regr_slope", "regr_intercept")      # their positions are abi.GM_VAR_POP .. GM_REGR_INTERCEPT
MOMENT_UNIVARIATE = MOMENT_OPS[:4]                         # the ops of one column; the others take (y, x)
MOMENT_NULL = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]      # what stands for SQL's NULL: the device's quiet NaN, bit for bit


class MomentsRequest(WindowRequest):
    """The second moments per group, travelling where a WindowRequest travels: [1] = the grouping columns `by` with their directions
    (all of them partition); aggs = [(name of the new column, op: a name of MOMENT_OPS, y, x or None)] — a univariate op reads y alone, a
    bivariate one y (the dependent measure, as in SQL's REGR_SLOPE(Y, X)) and x; rollup: the sets are rollup_sets(by), not `by` alone.
    The result holds `by` and a float64 column per aggregate, one row per group, ordered by `by`; with rollup the sets one after the
    other, rolled-up columns filled and an int64 column "grouping" last, as a GroupingRequest's.  Every other column is dropped."""
    method = terms_method = "moments"
    items_attr, served_by = "aggs", "momented"

    def __new__(cls, by, aggs, rollup=False):
        self = WindowRequest.__new__(cls, WINDOW_ALL, list(by), len(by), 0, WINDOW_ALL, None)
        self.aggs = [(str(n), str(op), str(y), None if x is None else str(x)) for n, op, y, x in aggs]
        self.rollup = bool(rollup)
        names = [nm for nm, _ in self[1]]
        if not names or len(set(names)) != len(names) or not self.aggs:
            raise ValueError("moments: bad columns")
        if any(op not in MOMENT_OPS or (x is None) != (op in MOMENT_UNIVARIATE) or y in names or x in names for _, op, y, x in self.aggs):
            raise ValueError("moments: bad aggregate")
        return self

    reserved = property(lambda self: ("grouping",) if self.rollup else ())
    sets = property(lambda self: rollup_sets([nm for nm, _ in self[1]]) if self.rollup else [tuple(nm for nm, _ in self[1])])

    def masks(self):
        """the `grouping` value of every set's rows (GroupingRequest.masks)"""
        names = [nm for nm, _ in self[1]]
        return [sum(1 << (len(names) - 1 - i) for i, nm in enumerate(names) if nm not in s) for s in self.sets]

    def renamed(self, terms, names=None):
        """The same request over other column names: the terms term for term, both measures through `names` (old name -> new)."""
        names = names or {}
        return MomentsRequest(terms, [(n, op, names.get(y, y), names.get(x, x)) for n, op, y, x in self.aggs], self.rollup)

    def check_columns(self, columns):
        WindowRequest.check_columns(self, columns)               # (the terms, y and the new names)
        for _, _, _, x in self.aggs:
            if x is not None and x not in columns:
                raise KeyError("moments: the result has no column %r" % x)


def moments_request(columns, by, aggs, rollup=False):
    """The checked MomentsRequest of moments: by = a non-empty list of columns, a column `name` or (name, "asc" | "desc"); aggs = {new
    column: (op, y) | (op, y, x)} with op a name of MOMENT_OPS — "var_pop" .. "stddev_samp" take one column, "covar_pop" ..
    "regr_intercept" two, y first.  columns: the result's column names when they are known (None: checked when the result is).
    KeyError for a column the result lacks or a new column it has already, ValueError for everything else."""
    if isinstance(by, str) or not isinstance(by, (list, tuple)) or not by:
        raise ValueError("moments: by is a non-empty list of columns")
    terms = []
    for c in by:
        name, d = (c, "asc") if isinstance(c, str) else (c[0], c[1]) if isinstance(c, (list, tuple)) and len(c) == 2 else (None, None)
        if not isinstance(name, str) or d not in ("asc", "desc"):
            raise ValueError("moments: a column is a name or (name, 'asc' | 'desc')")
        if name in [nm for nm, _ in terms]:
            raise ValueError("moments: column %r comes twice in by" % name)
        terms.append((name, d))
    _aggs_dict("moments", aggs, "(op, y) or (op, y, x)")
    out = []
    for name, spec in aggs.items():
        _agg_spec("moments", name, spec, "(op, y) or (op, y, x)", lambda n: n in (2, 3))
        op, y, x = spec[0], spec[1], spec[2] if len(spec) == 3 else None
        if op not in MOMENT_OPS:
            raise ValueError("moments: op is one of %s, not %r" % (", ".join(MOMENT_OPS), op))
        if op in MOMENT_UNIVARIATE and x is not None:
            raise ValueError("moments: %s takes one column" % op)
        if op not in MOMENT_UNIVARIATE and x is None:
            raise ValueError("moments: %s takes two columns, (y, x)" % op)
        for col in (y,) if x is None else (y, x):
            if not isinstance(col, str):
                raise ValueError("moments: a measure is a column name")
            if col in [nm for nm, _ in terms]:
                raise ValueError("moments: the measure %r is a grouping column" % col)
        out.append((name, op, y, x))
    if len(set(n for n, _, _, _ in out) | set(nm for nm, _ in terms)) != len(out) + len(terms):
        raise ValueError("moments: a new column has the name of a grouping column")
    if rollup and "grouping" in [n for n, _, _, _ in out]:
        raise ValueError("moments: with rollup the result's own column is named 'grouping'")
    req = MomentsRequest(terms, out, rollup)
    if columns is not None:
        req.check_columns(columns)
    return req


def moments_result(req, column_of, pieces):
    """The ResultSet of a MomentsRequest out of its sets' rows, whoever took the moments: pieces[s] = ({column of set s: its groups'
    values}, [one float64 array per aggregate], the number of groups).  Without rollup the one set's columns and the aggregates; with
    it grouped_result's layout: the sets in order, rolled-up columns filled, the `grouping` column last."""
    names = [nm for nm, _ in req[1]]
    sizes = [m for _, _, m in pieces]
    cols = []
    for nm in names:
        src = column_of(nm)
        cols.append(np.concatenate([np.asarray(by[nm]) if nm in by else _rolled_up(src, m) for (by, _, _), m in zip(pieces, sizes)]))
    for a in range(len(req.aggs)):
        cols.append(np.concatenate([np.asarray(aggs[a], np.float64) for _, aggs, _ in pieces]))
    out = names + [n for n, _, _, _ in req.aggs]
    if req.rollup:
        cols.append(np.concatenate([np.full(m, mask, np.int64) for m, mask in zip(sizes, req.masks())]))
        out.append("grouping")
    return ResultSet(out, cols)


def moment_finish(op, count, qy, qx, c, muy, mux):
    """An op of MOMENT_OPS out of its group's centred sums, in the order of operations include/sdqh_sort_moments.h states: count the
    groups' sizes as doubles, qy / qx / c the sums of squares and products (what the op does not read: None), muy / mux the means."""
    with np.errstate(all="ignore"):
        if op in ("var_pop", "stddev_pop", "covar_pop"):
            v = (c if op == "covar_pop" else qy) / count
            return np.sqrt(v) if op == "stddev_pop" else v
        if op in ("var_samp", "stddev_samp", "covar_samp"):
            v = (c if op == "covar_samp" else qy) / (count - 1.0)
            return np.where(count > 1.0, np.sqrt(v) if op == "stddev_samp" else v, MOMENT_NULL)
        if op == "corr":
            t = c / (np.sqrt(qx) * np.sqrt(qy))
            t = np.where(t > 1.0, 1.0, np.where(t < -1.0, -1.0, t))
            return np.where((qx != 0.0) & (qy != 0.0), t, MOMENT_NULL)
        slope = c / qx
        return np.where(qx != 0.0, slope if op == "regr_slope" else muy - slope * mux, MOMENT_NULL)


class RollingRequest(WindowRequest):
    """The second moments over window frames, travelling where an ExcludeRequest travels (every row is kept): [0] = the limit on the
    whole result, [1] = the PARTITION BY terms followed by the ORDER BY terms, npartition, and aggs = [(name of the new column, op: a
    name of MOMENT_OPS, y, x or None — a univariate op reads y alone —, unit: a name of EXCLUDE_UNITS, the column's own, lo, hi: the
    frame's offsets in that unit, negative = preceding, None = unbounded)] in the order the columns are appended.  Every new column
    is float64, NaN where SQL has NULL (an empty frame among them)."""
    method, items_attr, served_by = "rolling", "aggs", "rolled"

    def __new__(cls, k, terms, npartition, aggs):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, WINDOW_ALL, None)
        self.aggs = [(str(n), str(op), str(y), None if x is None else str(x), str(unit), lo, hi) for n, op, y, x, unit, lo, hi in aggs]
        if not self.aggs or any(op not in MOMENT_OPS or (x is None) != (op in MOMENT_UNIVARIATE) or unit not in EXCLUDE_UNITS or
                                (lo is not None and hi is not None and lo > hi) for _, op, _, x, unit, lo, hi in self.aggs):
            raise ValueError("rolling: bad aggregate")
        if any(unit == "value" for _, _, _, _, unit, _, _ in self.aggs) and len(terms) != npartition + 1:
            raise ValueError("rolling: a value frame is ordered by exactly one column")
        return self

    def _with(self, terms, items):
        return RollingRequest(self[0], terms, self.npartition, items)

    def renamed(self, terms, names=None):
        """The same request over other column names: the terms term for term, both measures through `names` (old name -> new)."""
        names = names or {}
        return self._with(terms, [(n, op, names.get(y, y), names.get(x, x), unit, lo, hi) for n, op, y, x, unit, lo, hi in self.aggs])

    def check_columns(self, columns):
        WindowRequest.check_columns(self, columns)               # (the terms, y and the new names)
        for _, _, _, x, _, _, _ in self.aggs:
            if x is not None and x not in columns:
                raise KeyError("rolling: the result has no column %r" % x)


def rolling_request(columns, by, order, aggs, unit="rows", k=WINDOW_ALL):
    """The checked RollingRequest of `rolling`: by / order as window_request takes them; unit a name of EXCLUDE_UNITS, the unit of every
    column that names none; aggs = {new column: (op, y, lo, hi[, unit]) | (op, y, x, lo, hi[, unit])} with op a name of MOMENT_OPS —
    "var_pop" .. "stddev_samp" take the first form, "covar_pop" .. "regr_intercept" the second, y first — and lo / hi offsets in the
    column's unit (negative = preceding, None = unbounded): ints, or floats as well for unit "value".  columns: the result's column
    names when they are known (None: checked when the result is).  KeyError for a column the result lacks or a new column it has
    already, ValueError for everything else."""
    req = window_request(None, by, order, "row_number", WINDOW_ALL, k=k)     # (its checks of by / order / k)
    if unit not in EXCLUDE_UNITS:
        raise ValueError("rolling: unit is one of %s, not %r" % (", ".join(EXCLUDE_UNITS), unit))
    shape = "(op, y, lo, hi[, unit]) or (op, y, x, lo, hi[, unit])"
    _aggs_dict("rolling", aggs, shape)
    out = []
    for name, spec in aggs.items():
        _agg_spec("rolling", name, spec, shape, lambda n: n >= 1)
        op = spec[0]
        if op not in MOMENT_OPS:
            raise ValueError("rolling: op is one of %s, not %r" % (", ".join(MOMENT_OPS), op))
        nm = 1 if op in MOMENT_UNIVARIATE else 2                 # the measures come first, then lo, hi and perhaps the unit
        if len(spec) not in (nm + 3, nm + 4):
            raise ValueError("rolling: %s takes %s" % (op, "one column: (op, y, lo, hi[, unit])" if nm == 1 else "two columns: (op, y, x, lo, hi[, unit])"))
        y, x = spec[1], spec[2] if nm == 2 else None
        for col in (y,) if x is None else (y, x):
            if not isinstance(col, str):
                raise ValueError("rolling: a measure is a column name")
        own = spec[nm + 3] if len(spec) == nm + 4 else unit
        if own not in EXCLUDE_UNITS:
            raise ValueError("rolling: a column's unit is one of %s, not %r" % (", ".join(EXCLUDE_UNITS), own))
        if own == "value" and len(req[1]) != req.npartition + 1:
            raise ValueError("rolling: a value frame is ordered by exactly one column, not %d" % (len(req[1]) - req.npartition))
        lo = None if spec[nm + 1] is None else _range_offset(spec[nm + 1], own, "rolling")
        hi = None if spec[nm + 2] is None else _range_offset(spec[nm + 2], own, "rolling")
        _agg_frame("rolling", lo, hi)
        out.append((name, op, y, x, own, lo, hi))
    req = RollingRequest(req[0], req[1], req.npartition, out)
    if columns is not None:
        req.check_columns(columns)
    return req


SESSION_OPS = ("sum", "count", "min", "max", "first", "last", "avg", "number", "row")      # their positions are abi.SS_SUM .. SS_ROW
SESSION_UNMEASURED = ("count", "number", "row")            # the ops that read no measure
SESSION_HOST_MAX_COLS = 64                                 # the columns of one request (the device takes abi.SS_MAX_COLS a call; the rest is the host's)


class SessionRequest(WindowRequest):
    """Sessions (gaps and islands), travelling where a WindowRequest travels (no rank column): [0] = the limit on the whole result,
    [1] = the PARTITION BY terms followed by the ORDER BY terms, npartition; rule "gap" — a new session where the first ORDER BY
    column moves on by more than `gap`, an int or a float >= 0 — or "change" — where the column `marker` changes; cols = [(name of the
    new column, op: a name of SESSION_OPS, measure column or None)] in the order the columns are appended, each over the row's whole
    session; per None: every row, "session": one row per session — its first row."""
    method, items_attr, served_by = "sessions", "cols", "sessioned"

    def __new__(cls, k, terms, npartition, rule, gap, marker, cols, per=None):
        self = WindowRequest.__new__(cls, k, terms, npartition, 0, WINDOW_ALL, None)
        self.rule, self.gap, self.marker, self.per = str(rule), gap, None if marker is None else str(marker), per
        self.cols = [(str(n), str(op), None if col is None else str(col)) for n, op, col in cols]
        if self.rule not in ("gap", "change") or self.per not in (None, "session") or (self.rule == "gap") != (self.marker is None) or (self.rule == "gap") == (gap is None):
            raise ValueError("sessions: bad rule")
        if self.rule == "gap" and (len(self[1]) < self.npartition + 1 or isinstance(gap, bool) or not isinstance(gap, (int, float, np.integer, np.floating)) or not gap >= 0 or gap == float("inf")):
            raise ValueError("sessions: bad gap")
        if any(op not in SESSION_OPS or (col is None) != (op in SESSION_UNMEASURED) or (op == "row" and self.per == "session") for _, op, col in self.cols):
            raise ValueError("sessions: bad column")
        return self

    def _with(self, terms, items):
        return SessionRequest(self[0], terms, self.npartition, self.rule, self.gap, self.marker, items, self.per)

    def renamed(self, terms, names=None):
        """The same request over other column names: the terms term for term, the measures and the marker through `names`."""
        req = WindowRequest.renamed(self, terms, names)
        req.marker = None if self.marker is None else (names or {}).get(self.marker, self.marker)
        return req

    def check_columns(self, columns):
        WindowRequest.check_columns(self, columns)               # (the terms, the measures and the new names)
        if self.marker is not None and self.marker not in columns:
            raise KeyError("sessions: the result has no column %r" % self.marker)


def sessions_request(columns, partition, order, gap=None, change=None, cols=None, per=None, k=WINDOW_ALL):
    """The checked SessionRequest of `sessions`: partition / order as window_request takes by / order; exactly one of gap — a new
    session where the first order column moves on by more than gap along the order: an int or a finite float >= 0 (a date column counts
    in its yyyymmdd units) — and change — the name of a column: a new session where it changes —; cols = {new column: (op, measure) |
    ("count",) | ("number",) | ("row",)} with op a name of SESSION_OPS, at most SESSION_HOST_MAX_COLS of them (an empty dict: the rows
    alone); per None or "session".  columns: the result's column names when they are known (None: checked when the result is).
    KeyError for a column the result lacks or a new column it has already, ValueError for everything else (an order column without
    arithmetic is found when the column is known)."""
    if (gap is None) == (change is None):
        raise ValueError("sessions: exactly one of gap and change says where a session starts")
    if per not in (None, "session"):
        raise ValueError("sessions: per is None or 'session', not %r" % (per,))
    if gap is not None:
        if isinstance(gap, bool) or not isinstance(gap, (int, float, np.integer, np.floating)) or not np.isfinite(float(gap) if isinstance(gap, (float, np.floating)) else 0.0) or not gap >= 0:
            raise ValueError("sessions: gap is an integer or a finite float, at least 0, not %r" % (gap,))
        if not order:
            raise ValueError("sessions: a gap is a difference of the first order column: order is empty")
        gap = float(gap) if isinstance(gap, (float, np.floating)) else int(gap)
    elif not isinstance(change, str):
        raise ValueError("sessions: change is a column name, not %r" % (change,))
    req = window_request(None, partition, order, "row_number", WINDOW_ALL, k=k)     # (its checks of by / order / k)
    cols = {} if cols is None else cols
    _aggs_dict("sessions", cols, "(op, measure)", what="cols", empty_ok=True)
    if len(cols) > SESSION_HOST_MAX_COLS:
        raise ValueError("sessions: at most %d columns, not %d" % (SESSION_HOST_MAX_COLS, len(cols)))
    out = []
    for name, spec in cols.items():
        _agg_spec("sessions", name, spec, "(op, measure)", lambda n: n in (1, 2), what="a column")
        op, col = spec[0], spec[1] if len(spec) == 2 else None
        if op not in SESSION_OPS:
            raise ValueError("sessions: op is one of %s, not %r" % (", ".join(SESSION_OPS), op))
        if op in SESSION_UNMEASURED and col is not None and op != "count":
            raise ValueError("sessions: %s takes no measure" % op)
        if op not in SESSION_UNMEASURED and not isinstance(col, str):
            raise ValueError("sessions: %s needs a measure column" % op)
        if op == "row" and per == "session":
            raise ValueError("sessions: a row's number in its session is no column of one row per session")
        out.append((name, op, None if op in SESSION_UNMEASURED else col))
    req = SessionRequest(req[0], req[1], req.npartition, "gap" if gap is not None else "change", gap, change, out, per)
    if columns is not None:
        req.check_columns(columns)
    return req


def session_continues(v, desc, gap):
    """Per sorted row but the first: does it continue its predecessor's session under the gap rule of include/sdqh_sort_sessions.h?  v:
    the order column along the order, int64 or float64.  Integers by the unsigned 64-bit difference of the two order-adjacent values
    (exact: nothing wraps); doubles by ONE IEEE addition, a = v(j) + d * (-gap), and min(a, v(j)) <= v(j - 1) <= max(a, v(j)) — -0.0
    and +0.0 are one value, a NaN row continues only a row with the same bits."""
    prev, cur = v[:-1], v[1:]
    if v.dtype.kind != "f":
        a, b = np.ascontiguousarray(prev, np.int64).view(np.uint64), np.ascontiguousarray(cur, np.int64).view(np.uint64)
        return (a - b if desc else b - a) <= np.uint64(min(int(gap), (1 << 64) - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        a = cur + np.float64(gap if desc else -gap)
        inside = (np.where(a < cur, a, cur) <= prev) & (prev <= np.where(a < cur, cur, a))
    same = np.ascontiguousarray(prev).view(np.uint64) == np.ascontiguousarray(cur).view(np.uint64)
    return np.where(np.isnan(cur), same, inside & ~np.isnan(prev))


def slide_empty(default, is_f64, what="sliding"):
    """What an empty frame gives for a measure of dtype float64 (is_f64) or int64: `default`, or with None NaN / 0.  ValueError for a
    default that does not fit the dtype: a float for an int64 column, an int outside int64."""
    if is_f64:
        return np.float64(np.nan if default is None else default)
    if default is None:
        return np.int64(0)
    if isinstance(default, (float, np.floating)) or not -(1 << 63) <= int(default) < (1 << 63):
        raise ValueError("%s: the default %r does not fit an int64 column" % (what, default))
    return np.int64(int(default))


def order_image(a, descending):
    """The order-preserving unsigned 64-bit image of a column under the total order of the device's ORDER BY (sdqh_sort.h): integers
    as signed values, doubles by sign and magnitude through their bits (-0.0 before +0.0, NaNs by their bits), text by its dense rank
    (numpy's order of '<U' arrays); a descending column is the complement.  Equal images <=> equal values under that order."""
    a = np.asarray(a)
    top = np.uint64(1) << np.uint64(63)
    if a.dtype.kind == "f":
        u = np.ascontiguousarray(a, np.float64).view(np.uint64)
        u = np.where(u >> np.uint64(63) != 0, ~u, u | top)
    else:
        if a.dtype.kind not in "iub":                        # text (or anything else numpy orders): its dense rank
            a = np.unique(a, return_inverse=True)[1].reshape(-1)
        u = np.ascontiguousarray(a, np.int64).view(np.uint64) ^ top
    return ~u if descending else u


class ResultSet:
    """Set of records: {record(field...): True}."""

    def __init__(self, columns, arrays, ready=None):
        """ready: a callable to run before the arrays are first read — the rows of a K-F result reach the host by a copy
        queued behind the query's kernels (sdqh_table_compact_async); the row count is known, the rows are waited for when
        something looks at them, as the reference's result object converts on `to_dict()` (src/sdqlpy/fastd.py:31-51)."""
        self.columns = list(columns)
        self._cols = [a if isinstance(a, TextRefs) else np.asarray(a) for a in arrays]
        n = len(self._cols[0]) if self._cols else 0
        for a in self._cols:
            if len(a) != n:
                raise ValueError("ragged result")
        self._n = n
        self._ready = ready

    def _wait(self):
        if self._ready is not None:
            ready, self._ready = self._ready, None
            ready()

    def wait(self):
        """Block until every row is on the host (a no-op for results that are complete already)."""
        self._wait()
        return self

    @property
    def arrays(self):
        """One numpy array per column (text columns of a large result are decoded on first use)."""
        self._wait()
        for i, a in enumerate(self._cols):
            if isinstance(a, TextRefs):
                self._cols[i] = np.asarray(a)
        return self._cols

    @arrays.setter
    def arrays(self, value):
        self._cols = list(value)

    def size(self):
        return self._n

    def __len__(self):
        return self._n

    def column(self, name):
        self._wait()
        i = self.columns.index(name)
        if isinstance(self._cols[i], TextRefs):
            self._cols[i] = np.asarray(self._cols[i])
        return self._cols[i]

    def rows(self):
        """Sorted list of plain-Python tuples (ints, floats, strs) — for comparisons."""
        cols = [a.tolist() for a in self.arrays]
        return sorted(zip(*cols)) if cols else []

    def ordered_rows(self):
        """Rows as plain-Python tuples in the order they are stored (the order of a top-k result)."""
        return list(zip(*[a.tolist() for a in self.arrays])) if self.arrays else []

    def top(self, k, order):
        self._wait()
        idx = self.top_index(k, order)
        return ResultSet(self.columns, [a[idx] for a in self._cols])     # undecoded text stays undecoded

    def top_index(self, k, order):
        """ORDER BY ... LIMIT k on the host: order = [(column, "asc" | "desc")], ties keep the stored
        row order (for K-F results that is build-row order, the same total order the device
        operator sdqh_table_topk uses).  Used for results that are small or not device tables."""
        keys = []
        for name, direction in reversed(list(order)):
            if name not in self.columns:
                raise KeyError("top: the result has no column %r" % name)
            a = self.column(name)
            if direction == "desc":
                if a.dtype.kind in "iuf":
                    a = -a if a.dtype.kind == "f" else ~a
                else:                                        # strings: rank them, then negate the rank
                    a = -np.unique(a, return_inverse=True)[1]
            keys.append(a)
        idx = np.lexsort(keys) if keys else np.arange(self._n)         # lexsort is stable
        return idx[:max(0, int(k))]

    def window_index(self, by, order, kind, per_limit, k=WINDOW_ALL):
        """Ranks inside partitions on the host, what sdqh_table_window does on the device (include/sdqh_sort_window.h): rows ordered by
        `by` then `order` (names or (name, "asc" | "desc")), ties in stored row order; a partition = rows equal in every `by` column,
        a tie = rows equal in every column, both under the device's total order (order_image: -0.0 != +0.0, NaNs equal bit for
        bit).  kind: a name of WINDOW_KINDS (or its position).  Returns (indices of the first k rows whose rank is <= per_limit, in
        order; their ranks, int64).  Used for results that are not device tables."""
        kind = WINDOW_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        if kind not in (0, 1, 2):
            raise ValueError("window: unknown kind")
        if int(per_limit) < 1 or int(k) < 1:
            raise ValueError("window: k must be at least 1")
        idx, part_head, tie_head = self._window_heads(by, order)
        n = self._n
        if n == 0:
            return idx[:0], np.zeros(0, np.int64)
        pos = np.arange(n, dtype=np.int64)
        part_start = np.maximum.accumulate(np.where(part_head, pos, 0))
        if kind == 0:
            rank = pos - part_start + 1
        elif kind == 1:
            rank = np.maximum.accumulate(np.where(tie_head, pos, 0)) - part_start + 1
        else:
            heads = np.cumsum(tie_head)
            rank = heads - heads[part_start] + 1
        keep = rank <= int(per_limit)
        return idx[keep][:int(k)], rank[keep][:int(k)].astype(np.int64)

    def _window_heads(self, by, order):
        """(the stored rows' indices in the order of `by` then `order`, ties in stored order; per sorted position: does a partition
        start here, does a tie run start here) — the order, partitions and ties of sdqh_table_window."""
        terms = [(b, "asc") if isinstance(b, str) else (b[0], b[1]) for b in by]
        npartition = len(terms)
        terms += [(o, "asc") if isinstance(o, str) else (o[0], o[1]) for o in order]
        images = []
        for name, direction in terms:
            if name not in self.columns:
                raise KeyError("window: the result has no column %r" % name)
            if direction not in ("asc", "desc"):
                raise ValueError("window: directions are 'asc' or 'desc'")
            images.append(order_image(self.column(name), direction == "desc"))
        n = self._n
        idx = np.lexsort(images[::-1]) if images else np.arange(n)      # lexsort is stable: ties keep the stored order
        part_head = np.zeros(n, bool)
        tie_head = np.zeros(n, bool)
        if n:
            part_head[0] = tie_head[0] = True
        for i, u in enumerate(images):
            differ = u[idx][1:] != u[idx][:-1]
            tie_head[1:] |= differ
            if i < npartition:
                part_head[1:] |= differ
        return idx, part_head, tie_head

    def framed(self, req):
        """Every row in a FrameRequest's order (the first req[0] of them) with its aggregate columns appended: what
        sdqh_table_window_agg does on the device (include/sdqh_sort_frames.h), on the host.  Per partition a running fold in row
        order — np.cumsum for SUM (int64 wraps), a running maximum of the order-preserving images for MIN / MAX (NaNs skipped, -0.0
        below +0.0, nothing but NaNs: NaN) — which is the ROWS value; RANGE / PARTITION rows take the ROWS value of the last row of
        their tie run / partition.  int64 for COUNT and integer measures, float64 otherwise."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, tie_head = self._window_heads(req.by, req.order)
        n = self._n
        starts = np.nonzero(part_head)[0]
        stops = np.append(starts[1:], n)

        def last_of(head):                                           # per position: the last position of its run of `head`
            at = np.nonzero(head)[0]
            return (np.append(at[1:], n) - 1)[np.cumsum(head) - 1] if n else np.zeros(0, np.int64)
        ends = {"range": last_of(tie_head), "partition": last_of(part_head)}
        top = np.uint64(1) << np.uint64(63)
        new = []
        for name, op, col, frame in req.aggs:
            x = None if op == "count" else self.column(col)[idx]
            if x is not None and x.dtype.kind not in "iubf":
                raise ValueError("over: %s of column %r: the measure is not numeric" % (op, col))
            is_f = x is not None and x.dtype.kind == "f"
            if op in ("count", "sum"):
                v = np.ones(n, np.int64) if op == "count" else np.ascontiguousarray(x, np.float64 if is_f else np.int64)
                fold = np.add
            else:                                                    # the images of sdqh_extrema.h: unsigned maximum, reversed for MIN, NaN = 0
                v = order_image(x, op == "min")
                if is_f:
                    v = np.where(np.isnan(x), np.uint64(0), v)
                fold = np.maximum
            rows = np.empty_like(v)
            for a, b in zip(starts, stops):
                fold.accumulate(v[a:b], out=rows[a:b])
            if op in ("min", "max"):
                u = ~rows if op == "min" else rows
                if is_f:
                    bits = np.where(u >> np.uint64(63) != 0, u ^ top, ~u)
                    rows = np.where(rows == 0, np.uint64(0x7FF8000000000000), bits).view(np.float64)
                else:
                    rows = (u ^ top).view(np.int64)
            new.append((name, rows if frame == "rows" else rows[ends[frame]]))
        k = max(0, min(int(req[0]), n))
        cols = [a[idx[:k]] for a in self._cols]                          # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [a[:k] for _, a in new])

    def slid(self, req):
        """Every row in a SlideRequest's order (the first req[0] of them) with its columns appended: what sdqh_table_window_slide does on
        the device (include/sdqh_sort_slide.h), on the host.  The frame of sorted row j in a partition [s, e] is [max(j + lo, s),
        min(j + hi, e)].  COUNT is arithmetic, FIRST / LAST gather, an integer SUM is a difference of wrapping prefix sums (exact
        mod 2^64); a double SUM and MIN / MAX (on the images of sdqh_extrema.h) fold exactly the frame's rows, nothing is subtracted:
        row by row for narrow frames, else through prefix and suffix folds of blocks of the frame's width, as the device does."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, _ = self._window_heads(req.by, req.order)
        n = self._n
        pos = np.arange(n, dtype=np.int64)
        start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos
        heads = np.nonzero(part_head)[0]
        end = (np.append(heads[1:], n) - 1)[np.cumsum(part_head) - 1] if n else pos
        top = np.uint64(1) << np.uint64(63)
        new = []
        for name, op, col, lo, hi, default in req.slides:
            x = None if op == "count" else self.column(col)[idx]
            if x is not None and x.dtype.kind not in "iubf":
                raise ValueError("sliding: %s of column %r: the measure is not numeric" % (op, col))
            is_f = x is not None and x.dtype.kind == "f"
            fill = None if op == "count" else slide_empty(default, is_f)
            lo_c = -n if lo is None else max(-n, min(n, lo))             # an offset of n or more leaves every partition
            hi_c = n if hi is None else max(-n, min(n, hi))
            left, right = np.maximum(pos + lo_c, start), np.minimum(pos + hi_c, end)
            empty = left > right
            a, b = np.where(empty, pos, left), np.where(empty, pos, right)       # (an empty frame reads its own row, then takes the default)
            if op == "count":
                new.append((name, np.where(empty, 0, right - left + 1).astype(np.int64)))
                continue
            x = np.ascontiguousarray(x, np.float64 if is_f else np.int64)
            if op in ("first", "last"):
                v = x[a] if op == "first" else x[b]
            elif op == "sum" and not is_f:
                c = np.concatenate((np.zeros(1, np.uint64), np.cumsum(x.view(np.uint64), dtype=np.uint64)))
                v = (c[b + 1] - c[a]).view(np.int64)
            else:
                if op == "sum":
                    e, fold = x, np.add
                else:                                                    # unsigned maximum of the images, reversed for MIN, NaN = 0
                    e, fold = order_image(x, op == "min"), np.maximum
                    e = np.where(np.isnan(x), np.uint64(0), e) if is_f else e
                v = _slide_fold(e, fold, a, b, start, end, max(1, min(hi_c - lo_c + 1, n)))
                if op != "sum":
                    u = ~v if op == "min" else v
                    if is_f:
                        v = np.where(v == 0, np.uint64(0x7FF8000000000000), np.where(u >> np.uint64(63) != 0, u ^ top, ~u)).view(np.float64)
                    else:
                        v = (u ^ top).view(np.int64)
            bits = np.where(empty, np.array(fill).view(np.uint64), np.ascontiguousarray(v).view(np.uint64))      # (by bits: a NaN default keeps its payload)
            new.append((name, bits.view(np.float64 if is_f else np.int64)))
        k = max(0, min(int(req[0]), n))
        cols = [c[idx[:k]] for c in self._cols]                          # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [c[:k] for _, c in new])

    def ranged_by(self, req):
        """Every row in a RangeRequest's order (the first req[0] of them) with its columns appended: what sdqh_table_window_range does on
        the device (include/sdqh_sort_range.h), on the host.  Per sorted position one ordered key — the order_image of the one ORDER BY
        column (unit "value"), the tie run's number inside the partition (unit "groups") — and per row two np.searchsorted over its
        partition's keys for the frame's ends, against bounds made without a wrapping add (integers: saturating; doubles: the one IEEE
        add, -0.0 / +0.0 as one value, NaN rows their own tie run).  COUNT is arithmetic, FIRST / LAST gather, an integer SUM is a
        difference of wrapping prefix sums (exact mod 2^64); a double SUM and MIN / MAX (on the images of sdqh_extrema.h) fold exactly
        the frame's rows through a binary fold tree over the sorted positions, lower positions on the left: nothing is subtracted."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, tie_head = self._window_heads(req.by, req.order)
        n = self._n
        pos = np.arange(n, dtype=np.int64)
        start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos
        heads = np.nonzero(part_head)[0]
        stops = np.append(heads[1:], n)
        end = (stops - 1)[np.cumsum(part_head) - 1] if n else pos
        top = np.uint64(1) << np.uint64(63)
        keys = self._range_keys(req.unit, req.order, idx, start, tie_head, "ranged")
        new = []
        for name, op, col, lo, hi, default in req.ranges:
            x = None if op == "count" else self.column(col)[idx]
            if x is not None and x.dtype.kind not in "iubf":
                raise ValueError("ranged: %s of column %r: the measure is not numeric" % (op, col))
            is_f = x is not None and x.dtype.kind == "f"
            fill = None if op == "count" else slide_empty(default, is_f, "ranged")
            left, right, empty = _range_ends(req.unit, keys, lo, hi, heads, stops, start, end)
            a, b = np.where(empty, pos, left), np.where(empty, pos, right)       # (an empty frame reads its own row, then takes the default)
            if op == "count":
                new.append((name, np.where(empty, 0, right - left + 1).astype(np.int64)))
                continue
            x = np.ascontiguousarray(x, np.float64 if is_f else np.int64)
            if op in ("first", "last"):
                val = x[a] if op == "first" else x[b]
            elif op == "sum" and not is_f:
                c = np.concatenate((np.zeros(1, np.uint64), np.cumsum(x.view(np.uint64), dtype=np.uint64)))
                val = (c[b + 1] - c[a]).view(np.int64)
            elif op == "sum":
                val = _tree_fold(x, np.add, np.float64(-0.0), a, b)
            else:                                                        # unsigned maximum of the images, reversed for MIN, NaN = 0
                e = order_image(x, op == "min")
                e = np.where(np.isnan(x), np.uint64(0), e) if is_f else e
                val = _tree_fold(e, np.maximum, np.uint64(0), a, b)
                u = ~val if op == "min" else val
                if is_f:
                    val = np.where(val == 0, np.uint64(0x7FF8000000000000), np.where(u >> np.uint64(63) != 0, u ^ top, ~u)).view(np.float64)
                else:
                    val = (u ^ top).view(np.int64)
            bits = np.where(empty, np.array(fill).view(np.uint64), np.ascontiguousarray(val).view(np.uint64))      # (by bits: a NaN default keeps its payload)
            new.append((name, bits.view(np.float64 if is_f else np.int64)))
        k = max(0, min(int(req[0]), n))
        cols = [c[idx[:k]] for c in self._cols]                          # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [c[:k] for _, c in new])

    def _range_keys(self, unit, order, idx, start, tie_head, who):
        """What the ends of a value or group frame are searched in: (one ordered uint64 key per sorted position — the order_image of
        the one ORDER BY column (unit "value"), the image of the tie run's number inside the partition (unit "groups") —, the order
        values themselves, is the order descending, are the values doubles)."""
        n = self._n
        top = np.uint64(1) << np.uint64(63)
        if unit == "groups":
            g = np.cumsum(tie_head).astype(np.int64)
            key = (g - g[start] + 1 if n else g).view(np.uint64) ^ top
            return key, key, False, False
        (name, direction), = order
        col = self.column(name)
        if col.dtype.kind not in "iubf":
            raise ValueError("%s: a value frame over column %r: the order column is not numeric" % (who, name))
        desc, is_fv = direction == "desc", col.dtype.kind == "f"
        v = np.ascontiguousarray(col[idx], np.float64 if is_fv else np.int64)
        return order_image(v, desc), v, desc, is_fv

    def excluded(self, req):
        """Every row in an ExcludeRequest's order (the first req[0] of them) with its columns appended: what sdqh_table_window_exclude
        does on the device (include/sdqh_sort_exclude.h), on the host.  The base frame's ends as slid (unit "rows") or ranged_by
        ("value", "groups") find them; then the excluded interval around the row — the row itself, or its tie run with or without
        it — cuts the frame into at most three pieces in position order.  COUNT adds their lengths, FIRST / LAST gather at the first
        / last remaining position, an integer SUM adds the pieces' differences of wrapping prefix sums (exact mod 2^64); a double
        SUM and MIN / MAX fold every piece through ranged_by's fold tree and join the pieces left to right: nothing is subtracted.
        AVG is that SUM as a float64 divided by the count as a float64, one division."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, tie_head = self._window_heads(req.by, req.order)
        n = self._n
        pos = np.arange(n, dtype=np.int64)
        start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos
        heads = np.nonzero(part_head)[0]
        stops = np.append(heads[1:], n)
        end = (stops - 1)[np.cumsum(part_head) - 1] if n else pos
        tie_a = np.maximum.accumulate(np.where(tie_head, pos, 0)) if n else pos         # the tie run [tie_a, tie_b] of every position
        ties = np.nonzero(tie_head)[0]
        tie_b = (np.append(ties[1:], n) - 1)[np.cumsum(tie_head) - 1] if n else pos
        top = np.uint64(1) << np.uint64(63)
        keys = {}
        new = []
        for name, op, col, unit, lo, hi, default in req.frames:
            x = None if op == "count" else self.column(col)[idx]
            if x is not None and x.dtype.kind not in "iubf":
                raise ValueError("excluding: %s of column %r: the measure is not numeric" % (op, col))
            is_f = x is not None and x.dtype.kind == "f"
            fill = None if op == "count" else slide_empty(default, is_f or op == "avg", "excluding")
            if unit == "rows":
                lo_c = -n if lo is None else max(-n, min(n, lo))         # an offset of n or more leaves every partition
                hi_c = n if hi is None else max(-n, min(n, hi))
                left, right = np.maximum(pos + lo_c, start), np.minimum(pos + hi_c, end)
                empty = left > right
            else:
                if unit not in keys:
                    keys[unit] = self._range_keys(unit, req.order, idx, start, tie_head, "excluding")
                left, right, empty = _range_ends(unit, keys[unit], lo, hi, heads, stops, start, end)
            # the hull [x0, x1] of what is taken out, and the pieces [a1, b1], {pos} (mid), [a3, b3] that remain
            if req.exclude == "no others":
                x0, x1 = right + 1, right
            elif req.exclude == "current row":
                x0, x1 = pos, pos
            else:
                x0, x1 = tie_a, tie_b
            a1, b1, a3, b3 = left, np.minimum(right, x0 - 1), np.maximum(left, x1 + 1), right
            p1, p3 = ~empty & (a1 <= b1), ~empty & (a3 <= b3)
            mid = ~empty & (left <= pos) & (pos <= right) if req.exclude == "ties" else np.zeros(n, bool)
            count = (np.where(p1, b1 - a1 + 1, 0) + mid + np.where(p3, b3 - a3 + 1, 0)).astype(np.int64)
            if op == "count":
                new.append((name, count))
                continue
            none = count == 0
            x = np.ascontiguousarray(x, np.float64 if is_f else np.int64)
            pieces = [(p1, np.where(p1, a1, pos), np.where(p1, b1, pos)), (mid, pos, pos), (p3, np.where(p3, a3, pos), np.where(p3, b3, pos))]      # (an empty piece reads its own row and is left out)
            if op in ("first", "last"):
                at = np.where(p1, a1, np.where(mid, pos, a3)) if op == "first" else np.where(p3, b3, np.where(mid, pos, b1))
                val = x[np.where(none, pos, at)]
            else:
                if op in ("sum", "avg") and not is_f:
                    c = np.concatenate((np.zeros(1, np.uint64), np.cumsum(x.view(np.uint64), dtype=np.uint64)))
                    val = np.zeros(n, np.uint64)
                    for has, a, b in pieces:
                        val = val + np.where(has, c[b + 1] - c[a], np.uint64(0))
                    val = val.view(np.int64)
                else:
                    if op in ("sum", "avg"):
                        e, fold, identity = x, np.add, np.float64(-0.0)
                    else:                                                # unsigned maximum of the images, reversed for MIN, NaN = 0
                        e, fold, identity = order_image(x, op == "min"), np.maximum, np.uint64(0)
                        e = np.where(np.isnan(x), np.uint64(0), e) if is_f else e
                    val, have = np.full(n, identity, e.dtype), np.zeros(n, bool)
                    with np.errstate(invalid="ignore", over="ignore"):
                        for has, a, b in pieces:
                            if has.any():
                                q = _tree_fold(e, fold, identity, a, b)
                                val = np.where(has, np.where(have, fold(val, q), q), val)
                                have = have | has
                    if op in ("min", "max"):
                        u = ~val if op == "min" else val
                        if is_f:
                            val = np.where(val == 0, np.uint64(0x7FF8000000000000), np.where(u >> np.uint64(63) != 0, u ^ top, ~u)).view(np.float64)
                        else:
                            val = (u ^ top).view(np.int64)
                if op == "avg":
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        val = val.astype(np.float64) / np.where(none, 1, count).astype(np.float64)
            out_f = is_f or op == "avg"
            bits = np.where(none, np.array(fill).view(np.uint64), np.ascontiguousarray(val).view(np.uint64))      # (by bits: a NaN default keeps its payload)
            new.append((name, bits.view(np.float64 if out_f else np.int64)))
        k = max(0, min(int(req[0]), n))
        cols = [c[idx[:k]] for c in self._cols]                          # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [c[:k] for _, c in new])

    def excluding(self, by, order, aggs, exclude="current row", unit="rows"):
        """Every row, ordered by `by` then `order`, plus one column per aggregate over a frame inside the row's group of `by` with rows
        taken out of it: aggs = {new column: (op, measure column or None, lo, hi[, default])}, op in EXCLUDE_OPS ("avg" among them),
        the frame in `unit` — "rows" (the rows [row + lo, row + hi]), "value" or "groups" (ranged's frames) — or a 6-tuple (op,
        measure, lo, hi, default, unit) for a column with a unit of its own.  exclude: "current row", "group" (the row and the rows
        tied with it), "ties" (those rows but not the row itself) or "no others".  Nothing left gives `default` (0 / NaN), a count 0;
        an avg is float64."""
        return self.excluded(exclude_request(self.columns, by, order, aggs, exclude, unit))

    def rolled(self, req):
        """Every row in a RollingRequest's order (the first req[0] of them) with its columns appended: what sdqh_table_window_moments
        gives on the device (include/sdqh_sort_wmoments.h), on the host — by the definition, not by the device's tree: the frame's
        ends as `excluded` finds them with nothing taken out, then per row two passes over the frame's rows as float64: the means,
        then the sums of the centred squares and products, and the op's formula (moment_finish).  NaN where SQL has NULL: an empty
        frame, *_samp of one row, corr with a constant column, regr_* with a constant x."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, tie_head = self._window_heads(req.by, req.order)
        n = self._n
        pos = np.arange(n, dtype=np.int64)
        start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos
        heads = np.nonzero(part_head)[0]
        stops = np.append(heads[1:], n)
        end = (stops - 1)[np.cumsum(part_head) - 1] if n else pos
        measures, keys, frames, sums = {}, {}, {}, {}
        new = []
        for name, op, y, x, unit, lo, hi in req.aggs:
            for col in (y, x):
                if col is not None and col not in measures:
                    v = self.column(col)
                    if v.dtype.kind not in "iubf":
                        raise ValueError("rolling: %s of column %r: the measure is not numeric" % (op, col))
                    measures[col] = np.ascontiguousarray(v[idx], np.float64)
            if (unit, lo, hi) not in frames:
                if unit == "rows":
                    lo_c = -n if lo is None else max(-n, min(n, lo))     # an offset of n or more leaves every partition
                    hi_c = n if hi is None else max(-n, min(n, hi))
                    left, right = np.maximum(pos + lo_c, start), np.minimum(pos + hi_c, end)
                    empty = left > right
                else:
                    if unit not in keys:
                        keys[unit] = self._range_keys(unit, req.order, idx, start, tie_head, "rolling")
                    left, right, empty = _range_ends(unit, keys[unit], lo, hi, heads, stops, start, end)
                frames[(unit, lo, hi)] = (left, right, np.asarray(empty, bool))
            left, right, empty = frames[(unit, lo, hi)]
            if (unit, lo, hi, y, x) not in sums:                         # [count, qy, qx, c, muy, mux] per row; an empty frame counts one row of zeros
                s = np.zeros((6, n), np.float64)
                s[0] = 1.0
                vy, vx = measures[y], measures[x if x is not None else y]
                with np.errstate(all="ignore"):
                    for j in np.nonzero(~empty)[0]:
                        a, b = left[j], right[j] + 1
                        m = np.float64(b - a)
                        muy, mux = vy[a:b].sum() / m, vx[a:b].sum() / m
                        dy, dx = vy[a:b] - muy, vx[a:b] - mux
                        s[:, j] = (m, (dy * dy).sum(), (dx * dx).sum(), (dx * dy).sum(), muy, mux)
                sums[(unit, lo, hi, y, x)] = s
            count, qy, qx, c, muy, mux = sums[(unit, lo, hi, y, x)]
            new.append((name, np.where(empty, MOMENT_NULL, moment_finish(op, count, qy, qx, c, muy, mux)) if n else np.zeros(0, np.float64)))
        k = max(0, min(int(req[0]), n))
        cols = [c[idx[:k]] for c in self._cols]                          # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [np.ascontiguousarray(c[:k], np.float64) for _, c in new])

    def rolling(self, by, order, aggs, unit="rows"):
        """Every row, ordered by `by` then `order`, plus one float64 column per aggregate over a frame inside the row's group of `by`:
        aggs = {new column: (op, y, lo, hi[, unit]) | (op, y, x, lo, hi[, unit])}, op in MOMENT_OPS — a moving standard deviation, a
        rolling correlation, a rolling regression slope.  The frame in `unit` — "rows" (the rows [row + lo, row + hi]), "value" or
        "groups" (ranged's frames) — or in the column's own; None: unbounded.  NaN where SQL has NULL, an empty frame included."""
        return self.rolled(rolling_request(self.columns, by, order, aggs, unit))

    def ranged(self, by, order, aggs, unit="value"):
        """Every row, ordered by `by` then `order`, plus one column per aggregate over a value or group frame inside the row's group of
        `by`: aggs = {new column: (op, measure column or None, lo, hi[, default])}, op in SLIDE_OPS.  unit "value": the rows whose
        (one, numeric) order column lies within [lo, hi] of this row's, along the order (RANGE BETWEEN); unit "groups": the rows whose
        tie run lies within [lo, hi] runs of this row's (GROUPS BETWEEN).  None: unbounded.  An empty frame gives `default` (0 / NaN),
        a count 0."""
        return self.ranged_by(range_request(self.columns, by, order, aggs, unit))

    def quantiled(self, req):
        """The rows a QuantileRequest keeps, in its order (the first req[0] of them), with its columns appended: what
        sdqh_table_window_quantile does on the device (include/sdqh_sort_quantile.h), on the host, under the same key images
        (order_image) and with the same IEEE expressions, so that both agree bit for bit on every value that is not a NaN.  For sorted
        row j in a partition [s, e]: m = e - s + 1, i = j - s, [f, l] the offsets of its tie run; every function looks at the whole
        partition, per_limit and the limit cut the rows off afterwards."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, tie_head = self._window_heads(req.by, req.order)
        n = self._n
        pos = np.arange(n, dtype=np.int64)
        start = np.maximum.accumulate(np.where(part_head, pos, 0)) if n else pos
        heads = np.nonzero(part_head)[0]
        end = (np.append(heads[1:], n) - 1)[np.cumsum(part_head) - 1] if n else pos
        m, i = end - start + 1, pos - start
        new = []
        for name, fn, col, arg, p, default in req.quants:
            x = None if col is None else self.column(col)[idx]
            if x is not None and x.dtype.kind not in "iubf":
                raise ValueError("quantiles: %s of column %r: the measure is not numeric" % (fn, col))
            is_f = x is not None and x.dtype.kind == "f"
            if x is not None:
                x = np.ascontiguousarray(x, np.float64 if is_f else np.int64)
            if fn == "ntile":
                q, r = m // arg, m % arg                                 # (b > m: q = 0 and r = m, every row takes the first arm)
                big = r * (q + 1)
                v = np.where(i < big, i // (q + 1) + 1, r + (i - big) // np.maximum(q, 1) + 1).astype(np.int64)
            elif fn == "percent_rank":
                f = (np.maximum.accumulate(np.where(tie_head, pos, 0)) if n else pos) - start
                v = np.where(m == 1, np.float64(0.0), f.astype(np.float64) / np.maximum(m - 1, 1).astype(np.float64))
            elif fn == "cume_dist":
                ties = np.nonzero(tie_head)[0]
                last = (np.append(ties[1:], n) - 1)[np.cumsum(tie_head) - 1] if n else pos
                v = (last - start + 1).astype(np.float64) / m.astype(np.float64)
            elif fn == "nth":
                fill = slide_empty(default, is_f, "quantiles")
                ak = min(abs(arg), n + 1)                                # (a k beyond n lies outside every partition: no wide arithmetic)
                inside = ak <= m
                src = np.where(inside, start + ak - 1 if arg > 0 else end + 1 - ak, pos)
                bits = np.where(inside, x[src].view(np.uint64), np.array(fill).view(np.uint64))      # (by bits: a NaN keeps its payload)
                v = bits.view(np.float64 if is_f else np.int64)
            elif fn == "percentile_disc":
                up = np.ceil(np.float64(p) * m.astype(np.float64))
                at = np.minimum(np.where(up >= 1.0, up - 1.0, 0.0).astype(np.int64), m - 1)
                v = x[start + at]
            else:
                t = np.float64(p) * (m - 1).astype(np.float64)
                lo, hi = np.floor(t), np.ceil(t)
                al, ah = np.minimum(lo.astype(np.int64), m - 1), np.minimum(hi.astype(np.int64), m - 1)
                a, b = x[start + al].astype(np.float64), x[start + ah].astype(np.float64)     # (an int64 by one round-to-nearest conversion)
                with np.errstate(invalid="ignore", over="ignore"):
                    v = np.where(al == ah, a, a + (b - a) * (t - lo))    # four IEEE operations, each a ufunc of its own: nothing is fused
            new.append((name, np.ascontiguousarray(v)))
        keep = np.nonzero(i < req.per_limit)[0][:max(0, int(req[0]))]
        cols = [c[idx[keep]] for c in self._cols]                        # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [c[keep] for _, c in new])

    def quantiles(self, by, order, cols, per=None):
        """The rows ordered by `by` then `order` — every row, or with `per` the first `per` of every group of `by` (1: one row per
        group) — plus one column per function of the group's size: cols = {new column: ("ntile", b) | ("percent_rank",) |
        ("cume_dist",) | ("nth", measure, k[, default]) | ("percentile_disc", measure, p) | ("percentile_cont", measure, p) |
        ("median", measure)}.  Every function sees its whole group, whatever `per` keeps."""
        return self.quantiled(quantile_request(self.columns, by, order, cols, per))

    def grouped(self, req):
        """The groups of a GroupingRequest, what sdqh_table_grouping_sets does on the device (include/sdqh_sort_groups.h), on the host:
        per set a stable lexsort by the set's columns (order_image: the device's total order), a group wherever a neighbour differs
        in one of them, and np.ufunc.reduceat over the groups — SUM of integers wraps, MIN / MAX are the unsigned maximum of the
        order-preserving images (NaNs skipped, -0.0 below +0.0, nothing but NaNs: NaN), AVG the SUM as a double over the count.
        sum / min / max take the measure's dtype (int64 or float64), count is int64, avg float64.  An empty result has no groups, not
        even the grand total."""
        self._wait()
        req.check_columns(self.columns)
        n = self._n
        direction = dict(req[1])
        top = np.uint64(1) << np.uint64(63)
        measures = {}
        for name, op, col in req.aggs:
            if col is not None and col not in measures:
                x = self.column(col)
                if x.dtype.kind not in "iubf":
                    raise ValueError("grouping_sets: %s of column %r: the measure is not numeric" % (op, col))
                measures[col] = np.ascontiguousarray(x, np.float64 if x.dtype.kind == "f" else np.int64)
        pieces = []
        for s in req.sets:
            images = [order_image(self.column(c), direction[c] == "desc") for c in s]
            idx = np.lexsort(images[::-1]) if images else np.arange(n)    # stable: ties keep the stored order
            head = np.zeros(n, bool)
            if n:
                head[0] = True
            for u in images:
                head[1:] |= u[idx][1:] != u[idx][:-1]
            starts = np.nonzero(head)[0]
            m = len(starts)
            count = np.diff(np.append(starts, n)).astype(np.int64)
            aggs = []
            for name, op, col in req.aggs:
                if op == "count":
                    aggs.append(count)
                    continue
                x = measures[col][idx]
                is_f = x.dtype.kind == "f"
                if not m:
                    aggs.append(np.zeros(0, np.float64 if is_f or op == "avg" else np.int64))
                elif op in ("sum", "avg"):
                    v = np.add.reduceat(x, starts) if is_f else np.add.reduceat(x.view(np.uint64), starts).view(np.int64)
                    aggs.append(v if op == "sum" else v.astype(np.float64) / count.astype(np.float64))
                else:                                                # the images of sdqh_extrema.h: unsigned maximum, reversed for MIN, NaN = 0
                    v = order_image(x, op == "min")
                    if is_f:
                        v = np.where(np.isnan(x), np.uint64(0), v)
                    e = np.maximum.reduceat(v, starts)
                    u = ~e if op == "min" else e
                    if is_f:
                        aggs.append(np.where(e == 0, np.uint64(0x7FF8000000000000), np.where(u >> np.uint64(63) != 0, u ^ top, ~u)).view(np.float64))
                    else:
                        aggs.append((u ^ top).view(np.int64))
            pieces.append(({c: self.column(c)[idx[starts]] for c in s}, aggs, m))
        return grouped_result(req, self.column, pieces)

    def grouping_sets(self, sets, aggs):
        """GROUP BY GROUPING SETS over the rows: one row per group of every set in `sets` (column tuples; a column is a name or (name,
        "asc" | "desc")), aggs = {new column: (op, measure column or None)}, op in GROUP_OPS.  The result holds the sets' columns, the
        aggregates and `grouping` (see GroupingRequest)."""
        return self.grouped(grouping_request(self.columns, sets, aggs))

    def rollup(self, by, aggs):
        """GROUP BY ROLLUP(by): the sets by[:d], by[:d - 1], ..., () — every prefix's subtotals down to the grand total."""
        return self.grouping_sets(rollup_sets(by), aggs)

    def cube(self, by, aggs):
        """GROUP BY CUBE(by): every subset of `by`, by ascending `grouping` mask."""
        return self.grouping_sets(cube_sets(by), aggs)

    def distincted(self, req):
        """The groups of a DistinctRequest, what sdqh_table_group_distinct does on the device (include/sdqh_sort_distinct.h), on the
        host: per value column a stable lexsort by `by` and the column (order_image: the device's total order, so -0.0 and +0.0 are two
        values and NaNs are equal only bit for bit), a group wherever a neighbour differs in `by`, a value run wherever it differs at
        all, and np.ufunc.reduceat of the runs over the groups.  count_distinct / mode_count / count are int64, sum_distinct and mode
        take the column's dtype (a sum of integers wraps; mode may be text), avg_distinct is float64: the sum as a double over the
        number of runs.  Among runs of equal length the mode is the first in order.  An empty result has no groups."""
        self._wait()
        req.check_columns(self.columns)
        n = self._n
        by = [(nm, d == "desc") for nm, d in req.by]
        by_images = [order_image(self.column(nm), desc) for nm, desc in by]
        out, first_rows = {}, None
        for v in req.values or [None]:
            images = by_images + ([order_image(self.column(v), False)] if v is not None else [])
            idx = np.lexsort(images[::-1]) if images else np.arange(n)    # stable: ties keep the stored order
            ghead, rhead = np.zeros(n, bool), np.zeros(n, bool)
            if n:
                ghead[0] = rhead[0] = True
            for i, u in enumerate(images):
                diff = u[idx][1:] != u[idx][:-1]
                rhead[1:] |= diff
                if i < len(by_images):
                    ghead[1:] |= diff
            rstart = np.nonzero(rhead)[0]                                 # the runs' first sorted positions
            rlen = np.diff(np.append(rstart, n)).astype(np.int64)
            gfirst = np.nonzero(ghead[rstart])[0]                         # per group its first run
            g = len(gfirst)
            runs = np.diff(np.append(gfirst, len(rstart))).astype(np.int64)
            if first_rows is None:
                first_rows = idx[rstart[gfirst]] if g else np.zeros(0, np.int64)
            for name, op, col in req.aggs:
                if col != v and not (col is None and name not in out):
                    continue
                if op == "count":
                    out[name] = np.add.reduceat(rlen, gfirst) if g else np.zeros(0, np.int64)
                    continue
                x = self.column(col)
                if op == "count_distinct":
                    out[name] = runs
                elif op in ("mode", "mode_count"):
                    if not g:
                        out[name] = np.zeros(0, np.int64) if op == "mode_count" else x[:0]
                        continue
                    longest = np.maximum.reduceat(rlen, gfirst)
                    group_of = np.repeat(np.arange(g), runs)
                    winner = np.minimum.reduceat(np.where(rlen == longest[group_of], np.arange(len(rstart)), len(rstart)), gfirst)
                    out[name] = longest if op == "mode_count" else x[idx[rstart[winner]]]
                else:
                    if x.dtype.kind not in "iubf":
                        raise ValueError("distincts: %s of column %r: the column is not numeric" % (op, col))
                    is_f = x.dtype.kind == "f"
                    r = np.ascontiguousarray(x, np.float64 if is_f else np.int64)[idx[rstart]]
                    if not g:
                        out[name] = np.zeros(0, np.float64 if is_f or op == "avg_distinct" else np.int64)
                        continue
                    total = np.add.reduceat(r, gfirst) if is_f else np.add.reduceat(r.view(np.uint64), gfirst).view(np.int64)
                    out[name] = total if op == "sum_distinct" else total.astype(np.float64) / runs.astype(np.float64)
        names = [nm for nm, _ in req.by]
        return ResultSet(names + [nm for nm, _, _ in req.aggs], [self.column(nm)[first_rows] for nm in names] + [out[nm] for nm, _, _ in req.aggs])

    def distincts(self, by, aggs):
        """Aggregates over the distinct values of every group of `by` (a list of columns, a column a name or (name, "asc" | "desc")):
        aggs = {new column: (op, value column)}, op in DISTINCT_OPS — COUNT(DISTINCT x), SUM / AVG(DISTINCT x), the most frequent x
        and how often it comes, and ("count", None), the group's rows.  The result holds `by` and the aggregates, one row per group,
        ordered by `by` (see DistinctRequest)."""
        return self.distincted(distinct_request(self.columns, by, aggs))

    def momented(self, req):
        """The groups of a MomentsRequest, what sdqh_table_group_moments does on the device (include/sdqh_sort_moments.h), on the host:
        the two-pass algorithm in numpy.  Per set a stable lexsort by the set's columns (order_image: the device's total order), a
        group wherever a neighbour differs; every measure as float64 minus its group's first sorted row's, np.add.reduceat for the
        sums, np.repeat of the means back to the rows, reduceat again over the centred squares and products, and the op's formula
        (moment_finish).  The exact cases are the device's: a constant group has Q = 0.0, *_samp of one row, corr with a constant
        column and regr_* with a constant x are NaN.  An empty result has no groups, not even the grand total."""
        self._wait()
        req.check_columns(self.columns)
        n = self._n
        direction = dict(req[1])
        measures = {}
        for name, op, y, x in req.aggs:
            for col in (y, x):
                if col is not None and col not in measures:
                    v = self.column(col)
                    if v.dtype.kind not in "iubf":
                        raise ValueError("moments: %s of column %r: the measure is not numeric" % (op, col))
                    measures[col] = np.ascontiguousarray(v, np.float64)
        pieces = []
        for s in req.sets:
            images = [order_image(self.column(c), direction[c] == "desc") for c in s]
            idx = np.lexsort(images[::-1]) if images else np.arange(n)    # stable: ties keep the stored order
            head = np.zeros(n, bool)
            if n:
                head[0] = True
            for u in images:
                head[1:] |= u[idx][1:] != u[idx][:-1]
            starts = np.nonzero(head)[0]
            m = len(starts)
            rows = np.diff(np.append(starts, n))
            count = rows.astype(np.float64)
            shifted, centred, mean = {}, {}, {}
            with np.errstate(all="ignore"):
                for col, v in measures.items() if m else ():
                    v = v[idx]
                    shifted[col] = v - np.repeat(v[starts], rows)             # the shift by the representative
                    mu = np.add.reduceat(shifted[col], starts) / count
                    centred[col] = shifted[col] - np.repeat(mu, rows)
                    mean[col] = v[starts] + mu
                aggs = []
                for name, op, y, x in req.aggs:
                    if not m:
                        aggs.append(np.zeros(0, np.float64))
                        continue
                    qy = np.add.reduceat(centred[y] * centred[y], starts)
                    qx = np.add.reduceat(centred[x] * centred[x], starts) if x is not None else None
                    c = np.add.reduceat(centred[x] * centred[y], starts) if x is not None else None
                    aggs.append(moment_finish(op, count, qy, qx, c, mean[y], mean.get(x)))
            pieces.append(({c: self.column(c)[idx[starts]] for c in s}, aggs, m))
        return moments_result(req, self.column, pieces)

    def moments(self, by, aggs, rollup=False):
        """VAR / STDDEV / COVAR / CORR / REGR per group of `by` (a non-empty list of columns, a column a name or (name, "asc" |
        "desc")): aggs = {new column: (op, y) | (op, y, x)}, op in MOMENT_OPS.  The result holds `by` and a float64 column per
        aggregate, one row per group, ordered by `by`; rollup=True: every prefix of `by` down to the grand total, with `grouping`
        (see MomentsRequest)."""
        return self.momented(moments_request(self.columns, by, aggs, rollup))

    def sessioned(self, req):
        """The rows of a SessionRequest in its order (the first req[0] of them) with its columns appended, or with per "session" one
        row per session: what sdqh_table_sessions does on the device (include/sdqh_sort_sessions.h), on the host.  The order,
        partitions and ties are sdqh_table_window's (_window_heads); a session starts at a partition's head and wherever the rule
        says so about two neighbours — the gap rule by session_continues (the unsigned integer difference, the one IEEE addition), the
        change rule by the marker's order_image.  Every column is folded per session by np.ufunc.reduceat — an integer SUM wraps, MIN /
        MAX are the unsigned maximum of the images with a NaN left out, AVG is the sum as float64 by the count, one division — and
        handed back to the session's rows; a double SUM is numpy's association, not the device's."""
        self._wait()
        req.check_columns(self.columns)
        idx, part_head, _ = self._window_heads(req.by, req.order)
        n = self._n
        if req.rule == "gap":
            name, direction = req.order[0]
            col = self.column(name)
            if col.dtype.kind not in "iubf":
                raise ValueError("sessions: a gap over column %r: the order column is not numeric" % name)
            is_fv = col.dtype.kind == "f"
            gap = req.gap
            if not is_fv:
                if isinstance(gap, (float, np.floating)) and float(gap) != int(gap):
                    raise ValueError("sessions: the gap %r over an integer column is not an integer" % (gap,))
                gap = int(gap)
            cont = session_continues(np.ascontiguousarray(col[idx], np.float64 if is_fv else np.int64), direction == "desc", gap) if n else np.zeros(0, bool)
        else:
            u = order_image(self.column(req.marker), False)[idx]
            cont = u[1:] == u[:-1]
        head = part_head.copy()
        if n:
            head[1:] |= ~cont
        starts = np.nonzero(head)[0]
        stops = np.append(starts[1:], n)
        ns = len(starts)
        sid = np.cumsum(head) - 1                                        # every position's session
        rows = (stops - starts).astype(np.int64)
        top = np.uint64(1) << np.uint64(63)
        new = []
        for name, op, col in req.cols:
            x = None if col is None else self.column(col)[idx]
            if x is not None and x.dtype.kind not in "iubf":
                raise ValueError("sessions: %s of column %r: the measure is not numeric" % (op, col))
            is_f = x is not None and x.dtype.kind == "f"
            if x is not None:
                x = np.ascontiguousarray(x, np.float64 if is_f else np.int64)
            if op == "row":
                new.append((name, (np.arange(n, dtype=np.int64) - starts[sid] + 1) if n else np.zeros(0, np.int64)))
                continue
            if not ns:
                s = np.zeros(0, np.float64 if (is_f or op == "avg") else np.int64)
            elif op == "count":
                s = rows
            elif op == "number":
                at = np.arange(ns, dtype=np.int64)
                s = at - np.maximum.accumulate(np.where(part_head[starts], at, 0)) + 1
            elif op == "first":
                s = x[starts]
            elif op == "last":
                s = x[stops - 1]
            elif op in ("sum", "avg"):
                with np.errstate(invalid="ignore", over="ignore"):
                    s = np.add.reduceat(x, starts) if is_f else np.add.reduceat(x.view(np.uint64), starts).view(np.int64)
                    if op == "avg":
                        s = s.astype(np.float64) / rows.astype(np.float64)
            else:                                                        # unsigned maximum of the images, reversed for MIN, NaN = 0
                e = order_image(x, op == "min")
                e = np.where(np.isnan(x), np.uint64(0), e) if is_f else e
                val = np.maximum.reduceat(e, starts)
                u = ~val if op == "min" else val
                if is_f:
                    s = np.where(val == 0, np.uint64(0x7FF8000000000000), np.where(u >> np.uint64(63) != 0, u ^ top, ~u)).view(np.float64)
                else:
                    s = (u ^ top).view(np.int64)
            new.append((name, np.ascontiguousarray(s) if req.per == "session" else np.ascontiguousarray(s[sid])))
        keep = (starts if req.per == "session" else np.arange(n))[:max(0, int(req[0]))]
        cols = [c[idx[keep]] for c in self._cols]                        # undecoded text stays undecoded
        return ResultSet(self.columns + [nm for nm, _ in new], cols + [c[:len(keep)] for _, c in new])

    def sessions(self, partition, order, gap=None, change=None, cols=None, per=None):
        """Sessions (gaps and islands) inside every group of `partition`, the rows ordered by `partition` then `order`: a new session
        where the first order column moves on by more than `gap` (gap=...), or where the column `change` changes (change=...).  cols =
        {new column: (op, measure) | ("count",) | ("number",) | ("row",)}, op in SESSION_OPS, each over the row's whole session:
        "first" / "last" of the order column are the session's start and end, "number" counts the sessions of a group from 1, "row"
        the rows of a session.  per=None: every row with its columns; per="session": one row per session, its first row."""
        return self.sessioned(sessions_request(self.columns, partition, order, gap, change, cols, per))

    def sliding(self, by, order, aggs):
        """Every row, ordered by `by` then `order`, plus one column per aggregate over a sliding frame inside the row's group of `by`:
        aggs = {new column: (op, measure column or None, lo, hi[, default])}, op in SLIDE_OPS, the frame rows [row + lo, row + hi] of
        the group (None: unbounded), or ("lag" | "lead", measure, k[, default]).  An empty frame gives `default` (0 / NaN), a count 0."""
        return self.slid(slide_request(self.columns, by, order, aggs))

    def over(self, by, order, aggs, frame="range"):
        """Every row, ordered by `by` then `order`, plus one column per aggregate over the row's frame inside its group of `by`:
        aggs = {new column: (op, measure column or None[, frame])}, op in WAGG_OPS, frame in FRAMES ("rows": group start .. this
        row; "range": .. the last row tied with this one, SQL's default; "partition": the whole group)."""
        return self.framed(frame_request(self.columns, by, order, aggs, frame))

    def windowed(self, req):
        """A WindowRequest of any kind served on the host, by the method its class names (WindowRequest.served_by)."""
        return req.host(self)

    def ranked(self, req):
        """The rows a plain WindowRequest keeps, in its order, with its rank column when it names one."""
        self._wait()
        req.check_columns(self.columns)
        idx, rank = self.window_index(req.by, req.order, req.kind, req.per_limit, req[0])
        cols = [a[idx] for a in self._cols]                              # undecoded text stays undecoded
        return ResultSet(self.columns + ([req.name] if req.name is not None else []), cols + ([rank] if req.name is not None else []))

    def top_per(self, k, by, order, ties=False):
        """The first k rows of every group of `by` in the order of `order`; ties=True keeps every row tied with the k-th (RANK)."""
        return self.windowed(window_request(self.columns, by, order, "rank" if ties else "row_number", k))

    def numbered(self, by, order, kind="row_number", name="rank"):
        """Every row, ordered by `by` then `order`, plus an int64 column `name`: its row_number / rank / dense_rank inside its group."""
        return self.windowed(window_request(self.columns, by, order, kind, WINDOW_ALL, name=name))

    def to_dict(self):
        out = {}
        cols = [a.tolist() for a in self.arrays]
        for row in zip(*cols):
            out[record(dict(zip(self.columns, row)))] = True
        return sr_dict(out)

    def __str__(self):
        return str(self.to_dict())

    # -- the rest of the reference container's surface (reference src/sdqlpy/fastd.py:31-51) --------
    def _row_of(self, key):
        fields = key.getContainer() if hasattr(key, "getContainer") else dict(key)
        if set(fields) != set(self.columns):
            raise KeyError("record fields %s do not match the result columns %s" % (sorted(fields), self.columns))
        return tuple(fields[c] for c in self.columns)

    def get(self, key):
        """True if the record is in the set, else None (`fastd.get`)."""
        if getattr(self, "_index", None) is None:
            self._index = set(zip(*[a.tolist() for a in self.arrays])) if self.arrays else set()
        return True if self._row_of(key) in self._index else None

    def set(self, key, value=True):
        """Add a record to the set (`fastd.set`; the value of a result set entry is always True)."""
        if value is not True:
            raise ValueError("a result set maps records to True")
        if self.get(key) is None:
            row = self._row_of(key)
            self.arrays = [np.append(a, np.array([v], dtype=a.dtype)) for a, v in zip(self.arrays, row)]
            self._n += 1
            self._index.add(row)

    def from_dict(self, data):
        """Replace the contents with {record: True, ...} (`fastd.from_dict`)."""
        recs = list((data.getContainer() if hasattr(data, "getContainer") else data).keys())
        rows = [self._row_of(r) for r in recs]
        self.arrays = [np.array([r[j] for r in rows], dtype=self.arrays[j].dtype) for j in range(len(self.columns))]
        self._n, self._index = len(rows), None
        return self

    def print(self):
        print(str(self.to_dict()))


class DictResult:
    """Dictionary from key record (or scalar) to value record (or scalar), struct-of-arrays."""

    def __init__(self, key_fields, val_fields, key_is_record=True, val_is_record=True):
        self.key_fields = list(key_fields)      # [(name, array)]
        self.val_fields = list(val_fields)
        self.key_is_record, self.val_is_record = key_is_record, val_is_record

    def size(self):
        fields = self.key_fields or self.val_fields
        return len(fields[0][1]) if fields else 0

    def __len__(self):
        return self.size()

    def to_dict(self):
        out = {}
        kcols = [a.tolist() for _, a in self.key_fields]
        vcols = [a.tolist() for _, a in self.val_fields]
        knames = [n for n, _ in self.key_fields]
        vnames = [n for n, _ in self.val_fields]
        for i in range(self.size()):
            k = record({n: c[i] for n, c in zip(knames, kcols)}) if self.key_is_record else kcols[0][i]
            v = record({n: c[i] for n, c in zip(vnames, vcols)}) if self.val_is_record else (vcols[0][i] if vcols else True)
            out[k] = v
        return sr_dict(out)

    def __str__(self):
        return str(self.to_dict())


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SLIDE_WALK_MAX = 32          # frames at most this wide are folded row by row on the host


def _slide_fold(e, fold, a, b, start, end, w):
    """fold over e[a[j] .. b[j]] for every j (a <= b, both inside j's partition [start, end], b - a < w): left to right row by row
    for w <= SLIDE_WALK_MAX; else the partitions are cut into blocks of w positions from their start, every block is folded from its
    first position (prefix) and up to its last (suffix), and a frame — it spans at most two adjacent blocks — is suffix[a] then
    prefix[b], or whichever of the two covers it alone.  The two folds are segmented scans by doubling over the whole array (after the
    step of distance d a position holds the fold of the min(2d, its distance into the block) positions ending at it): log2(w) numpy
    passes whatever the number of partitions, every row of a block entering once, the lower positions on the left."""
    n = len(e)
    if n == 0:
        return e.copy()
    if w <= SLIDE_WALK_MAX:
        v = e[a]
        for d in range(1, w):
            at = a + d
            inside = at <= b
            v = np.where(inside, fold(v, e[np.where(inside, at, a)]), v)
        return v
    pos = np.arange(n, dtype=np.int64)
    first = start + (pos - start) // w * w                               # the block's first and last position
    last = np.minimum(first + w - 1, end)
    pre, suf, d = e, e, 1
    while d < min(w, n):
        pre = np.where(pos - d >= first, fold(pre[np.maximum(pos - d, 0)], pre), pre)
        suf = np.where(pos + d <= last, fold(suf, suf[np.minimum(pos + d, n - 1)]), suf)
        d *= 2
    ra, rb = a - start, b - start
    two = ra // w != rb // w
    return np.where(two, fold(suf[a], pre[b]), np.where(ra % w == 0, pre[b], suf[a]))


def _range_int_bound(v, off, desc, lo_side):
    """One side of an integer value / group frame for every row: (the key to search for, all: every row of the partition lies inside
    this bound, none: no row does).  The target v + d * off is made in Python integers, once per distinct value: nothing wraps, and
    beyond int64 it is a bound that no value reaches."""
    n = len(v)
    if off is None:
        return np.zeros(n, np.uint64), np.ones(n, bool), np.zeros(n, bool)
    u, inv = np.unique(v, return_inverse=True)
    inv = inv.reshape(-1)
    t = u.astype(object) + (-int(off) if desc else int(off))
    over, under = (t > INT64_MAX).astype(bool)[inv], (t < INT64_MIN).astype(bool)[inv]
    key = order_image(np.clip(t, INT64_MIN, INT64_MAX).astype(np.int64)[inv], desc)
    out = over | under
    every = (over != desc) != lo_side
    return key, out & every, out & ~every


def _range_ends(unit, keys, lo, hi, heads, stops, start, end):
    """(first position, last position, is it empty) of every row's value or group frame [lo, hi] inside its partition — heads / stops:
    the partitions [a, b); start / end: per position — by two np.searchsorted over the partition's keys (keys: ResultSet._range_keys')
    against bounds made without a wrapping add."""
    key, v, desc, is_fv = keys
    n = len(key)
    top = np.uint64(1) << np.uint64(63)
    # per side: the key searched for, and where no search is needed whether every row of the partition lies inside (all) or none
    if is_fv:
        sides = _range_f64_bounds(v, key, None if lo is None else float(lo), None if hi is None else float(hi), desc)
    else:
        vj = (key ^ top).view(np.int64) if unit == "groups" else v
        sides = (_range_int_bound(vj, _range_int_offset(lo), desc, True), _range_int_bound(vj, _range_int_offset(hi), desc, False))
    (kl, all_l, none_l), (kr, all_r, none_r) = sides
    left, right = np.empty(n, np.int64), np.empty(n, np.int64)
    for a, b in zip(heads, stops):                              # the ends of every row's frame inside its partition [a, b)
        left[a:b] = a + np.searchsorted(key[a:b], kl[a:b], "left")
        right[a:b] = a + np.searchsorted(key[a:b], kr[a:b], "right") - 1
    left, right = np.where(all_l, start, left), np.where(all_r, end, right)
    return left, right, none_l | none_r | (left > right)


def _range_f64_bounds(v, key, lo, hi, desc):
    """Both sides of a double value frame for every row, as _range_int_bound gives one: the bounds a = v + d * lo, b = v + d * hi (one
    IEEE addition each) as keys of the total order — the lower end of the IEEE comparison takes -0.0 for a zero, the upper end +0.0 —
    and a NaN row its own key on every bounded side."""
    n = len(v)
    nan = np.isnan(v)
    with np.errstate(over="ignore", invalid="ignore"):
        fa = None if lo is None else v + (-lo if desc else lo)
        fb = None if hi is None else v + (-hi if desc else hi)
    x, y = (fb, fa) if desc else (fa, fb)                            # the lower and the upper value bound
    if x is not None and y is not None:
        x, y = np.minimum(x, y), np.maximum(x, y)

    def side(bound, lower):
        if bound is None:
            return np.zeros(n, np.uint64), np.ones(n, bool), np.zeros(n, bool)
        z = np.where(bound == 0.0, -0.0 if lower else 0.0, np.where(nan, 0.0, bound))
        return np.where(nan, key, order_image(z, desc)), np.zeros(n, bool), np.zeros(n, bool)
    return (side(y, False), side(x, True)) if desc else (side(x, True), side(y, False))


def _tree_fold(e, fold, identity, a, b):
    """fold over e[a[j] .. b[j]] for every j (a <= b) through a bottom-up binary fold tree over the positions, as the device's range
    frames are folded: node k = node 2k then node 2k + 1, the leaves padded to a power of two with the identity; the iterative query
    keeps a left and a right accumulator and reads at most 2 log2(width) + 2 nodes, the lower positions on the left."""
    n = len(e)
    if n == 0:
        return e.copy()
    cap = 1
    while cap < n:
        cap *= 2
    t = np.full(2 * cap, identity, e.dtype)
    t[cap:cap + n] = e
    width = cap
    while width > 1:
        half = width // 2
        t[half:width] = fold(t[width:2 * width:2], t[width + 1:2 * width:2])
        width = half
    p, q = a.astype(np.int64) + cap, b.astype(np.int64) + 1 + cap
    left, right = np.full(len(a), identity, e.dtype), np.full(len(a), identity, e.dtype)
    while np.any(p < q):
        m = (p < q) & ((p & 1) == 1)
        left = np.where(m, fold(left, t[np.where(m, p, 1)]), left)
        p = p + m
        m = (p < q) & ((q & 1) == 1)
        q = q - m
        right = np.where(m, fold(t[np.where(m, q, 1)], right), right)
        p, q = p >> 1, q >> 1
    return fold(left, right)


class Pending:
    """The outcome of a plan step whose device call was launched and not waited for: resolve() — after the context has been
    synchronised — collects it and returns what the step would have returned (engine.PreparedPlan.run)."""
    __slots__ = ("resolve",)

    def __init__(self, resolve):
        self.resolve = resolve


class DeferredResultSet(ResultSet):
    """A result set whose query has been LAUNCHED but not waited for: the plan's last device call was queued and the call returned
    (engine.PreparedPlan.run with Engine.deferred_results) — the host goes on to queue the next query while this one runs, as a CUDA /
    HIP program overlaps launches with execution.  Everything that looks at the result — its size, its columns, its rows —
    first runs `thunk`, which synchronises the context, collects the device's output and finishes the plan's host-side steps;
    errors the data decides (more groups than the kernel holds ...) surface there, where the plan is re-run synchronously on its
    other path.  The reference's result object defers its conversion in the same spirit (src/sdqlpy/fastd.py:31-51)."""

    _launched = 0

    def __init__(self, thunk):
        self._thunk = thunk
        DeferredResultSet._launched += 1
        self._seq = DeferredResultSet._launched                 # launch order (engine.finish_outstanding finishes results in it)

    def _force(self):
        err = self.__dict__.get("_error")
        if err is not None:                                      # the thunk failed once: every later look at the result says so again
            raise err
        thunk = self.__dict__.pop("_thunk", None)
        if thunk is not None:
            try:
                rs = thunk()
                if not isinstance(rs, ResultSet):
                    raise TypeError("a deferred query finished with %r, not a result set" % type(rs).__name__)
                if isinstance(rs, DeferredResultSet):
                    rs._force()
            except BaseException as exc:
                self.__dict__["_error"] = exc
                raise
            self.__dict__.update(rs.__dict__)

    def __getattr__(self, name):                                 # only reached for attributes not set yet: columns, _cols, _n, _ready
        if name in ("_thunk", "_error"):
            raise AttributeError(name)
        if "_error" in self.__dict__:
            raise self.__dict__["_error"]
        if "_thunk" not in self.__dict__:
            raise AttributeError(name)
        self._force()
        return getattr(self, name)

    def wait(self):
        """Finish the query now (the result is complete and on the host when this returns)."""
        self._force()
        self._wait()
        return self

