"""A brute-force reference for sessions (include/sdqh_sort_sessions.h): a plain Python loop over the sorted rows, with `int` for
integers (nothing wraps until a result is stored) and `fractions.Fraction` for sums of doubles (exact).  It shares no code with
sdqlpy_amd.result: the order is Python's `sorted` under a key of its own, the rule and the folds are written out row by row.

Columns come back as lists of unsigned 64-bit words — the bits of the int64 or the double the column holds — so that a comparison
is by bits."""
import struct
from fractions import Fraction

OPS = ("sum", "count", "min", "max", "first", "last", "avg", "number", "row")
QNAN = 0x7FF8000000000000
M64 = (1 << 64) - 1


def f_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def bits_f(u):
    return struct.unpack("<d", struct.pack("<Q", u & M64))[0]


def i_bits(x):
    return int(x) & M64


def total_key(x, is_f64):
    """The device's total order (sdqh_sort.h): integers as they are; doubles by sign and magnitude through their bits, -0.0 before
    +0.0, NaNs by their bits."""
    if not is_f64:
        return int(x)
    u = f_bits(x)
    return (M64 ^ u) if u >> 63 else (u | (1 << 63))


def sort_index(columns, directions, is_f64):
    """The stored rows' indices ordered by the columns (lists) in the directions ("asc" / "desc"), ties in stored order."""
    n = len(columns[0]) if columns else 0

    def key(i):
        out = []
        for col, d, f in zip(columns, directions, is_f64):
            k = total_key(col[i], f)
            out.append(-k if d == "desc" else k)
        return tuple(out)
    return sorted(range(n), key=key)                                     # (stable)


def continues_gap(prev, cur, desc, gap, is_f64):
    """Does the row with order value `cur` continue the session of its predecessor `prev`?  prev lies in cur's frame RANGE BETWEEN gap
    PRECEDING AND CURRENT ROW."""
    if not is_f64:
        d = (int(prev) - int(cur)) if desc else (int(cur) - int(prev))     # mathematical integers
        return 0 <= d <= int(gap)
    prev, cur, gap = float(prev), float(cur), float(gap)
    if cur != cur:
        return f_bits(prev) == f_bits(cur)
    if prev != prev:
        return False
    a = cur + (gap if desc else -gap)                                    # ONE IEEE addition: v(j) + d * (-gap)
    return min(a, cur) <= prev <= max(a, cur)


def session_heads(part_keys, values, desc, gap, is_f64, marker_bits=None):
    """Per sorted row: does a session start here?  part_keys: the row's partition key (any comparable), values: the gap term's values
    along the order (gap rule), or marker_bits: the marker's stored 64 bits (change rule)."""
    heads = []
    for j in range(len(part_keys)):
        if j == 0 or part_keys[j] != part_keys[j - 1]:
            heads.append(True)
        elif marker_bits is not None:
            heads.append(marker_bits[j] != marker_bits[j - 1])
        else:
            heads.append(not continues_gap(values[j - 1], values[j], desc, gap, is_f64))
    return heads


def wrap(x):
    """A mathematical integer as the int64 two's complement leaves."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def fold(op, xs, is_f64):
    """One session's column as 64 bits: xs its rows' measures along the order (count: anything of the right length)."""
    m = len(xs)
    if op == "count":
        return i_bits(m)
    if op == "first":
        return f_bits(xs[0]) if is_f64 else i_bits(xs[0])
    if op == "last":
        return f_bits(xs[-1]) if is_f64 else i_bits(xs[-1])
    if op in ("sum", "avg"):
        if is_f64:
            if any(x != x or x in (float("inf"), float("-inf")) for x in xs):
                s = sum(xs)
            else:
                exact = sum((Fraction(x) for x in xs), Fraction(0))
                s = float(exact)                                         # (the tests' measures: every partial sum is a double)
                if exact == 0 and all(f_bits(x) == f_bits(-0.0) for x in xs):
                    s = -0.0
        else:
            s = wrap(sum(int(x) for x in xs))
        if op == "avg":
            return f_bits(float(s) / float(m))                           # one conversion, one IEEE division
        return f_bits(s) if is_f64 else i_bits(s)
    live = [x for x in xs if not (is_f64 and x != x)]                    # MIN / MAX: NaNs are left out; nothing left: the quiet NaN
    if not live:
        return QNAN
    best = (min if op == "min" else max)(live, key=lambda x: total_key(x, is_f64))
    return f_bits(best) if is_f64 else i_bits(best)


def columns(heads, part_heads, cols, per_session):
    """cols: [(op, measures along the order or None, is_f64)] -> one list of 64-bit words per column: per row, or per session.  heads:
    session_heads' flags; part_heads: the partition heads among them."""
    n = len(heads)
    starts = [j for j in range(n) if heads[j]]
    stops = starts[1:] + [n]
    number, k = [], 0
    for s in starts:
        k = 1 if part_heads[s] else k + 1
        number.append(k)
    out = []
    for op, xs, is_f64 in cols:
        if op == "row":
            col, r = [], 0
            for j in range(n):
                r = 1 if heads[j] else r + 1
                col.append(i_bits(r))
            out.append(col)
            continue
        per = []
        for i, (a, b) in enumerate(zip(starts, stops)):
            per.append(i_bits(number[i]) if op == "number" else fold(op, xs[a:b] if xs is not None else [0] * (b - a), is_f64))
        if per_session:
            out.append(per)
        else:
            out.append([v for v, a, b in zip(per, starts, stops) for _ in range(b - a)])
    return out, starts
