"""A whole-array reference for sessions (include/sdqh_sort_sessions.h) at the sizes past 256 tiles, where sessions_reference's Python
loop over rows is too slow: numpy over the sorted rows, nothing loops over rows or sessions in Python.  Importable without a GPU.  It
shares no code with sdqlpy_amd.result and none with sessions_reference's folds (test_sessions_large_cpu compares the two by bits on
small inputs): the heads come from neighbour differences, the folds from ufunc.reduceat over the sessions' first positions.

Narrower than sessions_reference on purpose — the small tests own these —: an integer gap term below 2^40 in magnitude (plain int64
subtraction, nothing wraps), no NaN in a double gap term or under a double MIN / MAX, no derived gap term.  Double sums are additions in
row order: exact, and so independent of the association, on the tests' data (multiples of 0.25 of small magnitude).

Columns come back as uint64 arrays — the bits of the int64 or the double the column holds."""
import numpy as np

from test_window_gpu import _images

OPS = ("sum", "count", "min", "max", "first", "last", "avg", "number", "row")
TOP = np.uint64(1) << np.uint64(63)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def order(rows, terms):
    """The stable sorted index of the staged rows (keys, payload, values, hits) under the terms: a lexsort over the terms' ordered
    64-bit images, ties in stored order."""
    n = len(rows[0])
    return np.lexsort(_images(rows, terms)[::-1]) if n else np.zeros(0, np.int64)


def heads(part_cols, order_values, desc, gap, is_f64, marker_bits=None):
    """-> (session heads, partition heads), bool by sorted position.  part_cols: the partition terms' columns along the order (any
    dtype, compared by !=); order_values: the gap term's values along the order, int64 or float64 (gap rule), or marker_bits: the
    marker's stored 64 bits as uint64 (change rule)."""
    n = len(marker_bits) if marker_bits is not None else len(order_values)
    ph = np.zeros(n, bool)
    if n == 0:
        return ph, ph.copy()
    ph[0] = True
    for c in part_cols:
        c = np.asarray(c)
        assert len(c) == n
        ph[1:] |= c[1:] != c[:-1]
    if marker_bits is not None:
        m = np.asarray(marker_bits, np.uint64)
        goes_on = m[1:] == m[:-1]
    elif not is_f64:
        v = np.asarray(order_values)
        assert v.dtype == np.int64 and ((v > -(1 << 40)) & (v < 1 << 40)).all() and 0 <= int(gap) < 1 << 40      # nothing wraps
        d = (v[:-1] - v[1:]) if desc else (v[1:] - v[:-1])
        goes_on = (d >= 0) & (d <= np.int64(gap))
    else:
        v = np.asarray(order_values)
        assert v.dtype == np.float64 and not np.isnan(v).any()
        a = v[1:] + np.float64(gap if desc else -gap)                       # the header's one IEEE addition: v(j) + d * (-gap)
        goes_on = (np.minimum(a, v[1:]) <= v[:-1]) & (v[:-1] <= np.maximum(a, v[1:]))
    sh = ph.copy()
    sh[1:] |= ~goes_on
    return sh, ph


def _total_key(u):
    """double bits -> the total-order key of sdqh_sort.h: ~bits if the sign is set, else bits | 2^63"""
    return np.where(u >> np.uint64(63) != 0, ~u, u | TOP)


def _from_key(k):
    return np.where(k >> np.uint64(63) != 0, k ^ TOP, ~k)


def columns(session_heads, part_heads, cols, per_session):
    """cols: [(op name, the measure along the order (int64, or float64 with is_f64) or None, is_f64)] -> one uint64 array per column:
    per sorted row, or per session.  'row' exists per row only."""
    sh, ph = np.asarray(session_heads, bool), np.asarray(part_heads, bool)
    n = len(sh)
    if n == 0:
        return [np.zeros(0, np.uint64) for _ in cols]
    assert sh[0] and ph[0] and not (ph & ~sh).any()
    starts = np.nonzero(sh)[0]
    length = np.diff(np.append(starts, n))
    seen = np.cumsum(sh)                                                    # sessions up to and including the position
    pos = np.arange(n, dtype=np.int64)
    pstart = np.maximum.accumulate(np.where(ph, pos, 0))
    out = []
    for op, xs, is_f64 in cols:
        if op == "row":
            assert not per_session
            out.append(bits(pos - starts[seen - 1] + 1))
            continue
        if op == "count":
            per = length.astype(np.int64)
        elif op == "number":
            per = (seen[starts] - seen[pstart[starts]] + 1).astype(np.int64)
        else:
            x = np.ascontiguousarray(xs)
            assert len(x) == n and x.dtype == (np.float64 if is_f64 else np.int64)
            if op == "first":
                per = x[starts]
            elif op == "last":
                per = x[starts + length - 1]
            elif op in ("sum", "avg"):
                with np.errstate(over="ignore"):
                    per = np.add.reduceat(x, starts)                        # int64 wraps, as the header says
                if op == "avg":
                    per = per.astype(np.float64) / length.astype(np.float64)      # one conversion, one IEEE division
            else:
                fold = np.minimum if op == "min" else np.maximum
                if is_f64:
                    assert not np.isnan(x).any()
                    per = _from_key(fold.reduceat(_total_key(bits(x)), starts))
                else:
                    per = fold.reduceat(x, starts)
        per = bits(per)
        out.append(per if per_session else np.repeat(per, length))
    return out
