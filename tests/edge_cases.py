"""Edge values against exact sums: row programs (the sdqh_xop vocabulary) and the fixed tuple shapes on columns built to
reach the run-time specialisations (integer widths from column ranges, code-space comparisons, narrow twins) and the
f64 accumulators (NaN, +-inf, -0.0, subnormal values, values near DBL_MAX, heavy cancellation).

The reference is plain Python with the C semantics include/sdqh.h states: i64 arithmetic on Python ints (a row that leaves
int64 is flagged: C is undefined there), DIVI / MODI / YEAR truncate toward zero, I2F rounds to nearest even, f64 arithmetic
on IEEE doubles one operation at a time (no FMA), every comparison with NaN false except NE.  Sums are checked by
`Checker.sum`:
- a group of one row equals the row's double bit for bit (order-free: catches a contraction or a changed association);
- a group of m rows is within (m-1) * 2^-53 * sum|x| of math.fsum (holds for any order of additions, atomics included);
- NaN when a NaN or both infinities are summed, else the matching infinity;
- a group of subnormal values only equals the exact sum bit for bit (sums of values <= 2^-1060 stay exact in any order);
- a group of zeros only is +0.0: the reference's sums start from the literal 0.0 (src/sdqlpy/lib/sdql_ir_cpp_generator_par.py:688),
  and 0.0 + -0.0 is +0.0.
"""
import math
import struct

import numpy as np

from sdqlpy_amd import abi as A

I64_LO, I64_HI = -(1 << 63), (1 << 63) - 1
SIZES = (1, 63, 65, 513, 4097, 70001)
DBL_MAX = 1.7976931348623157e308
LARGE_SCAN_OPTIONS = {"feature_min_rows": 0, "coarse_kb": 1}
DEFAULT_OPTIONS = {"feature_min_rows": 1 << 20, "coarse_kb": 64}


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def from_bits(i):
    return struct.unpack("<d", struct.pack("<q", int(i)))[0]


def _trunc_div(x, d):
    q = abs(x) // d
    return q if x >= 0 else -q


# ---- 1(a): the evaluator ------------------------------------------------------------------------------------------------------
class RefTable:
    """A unique build as a Python dict (first passing row wins): key -> entry; per entry its payload as raw 8-byte integers,
    its accumulators and its row count, and the per-row doubles summed into each accumulator."""

    def __init__(self, nfields):
        self.index, self.payload, self.acc, self.hits, self.parts = {}, [], [], [], []
        self.nfields = nfields

    def add(self, key, payload):
        if key in self.index:
            return
        self.index[key] = len(self.payload)
        self.payload.append(list(payload))
        self.acc.append([0.0] * A.TUPLE_MAX_VALUES)
        self.hits.append(0)
        self.parts.append([[] for _ in range(A.TUPLE_MAX_VALUES)])


class Eval:
    """What a program computes on every row: `passing` (bool), `key` (object array of ints or None), `vals` (float64 arrays for
    F64 values, object arrays of ints for I64 ones), `flagged` (rows that leave int64 while they are evaluated), `bad` (rows whose
    PACK2 part is outside [0, 2^32)) and `ent` (entry index per row of every LOOKUP operation)."""


def evaluate(prog, n, host, tables=None):
    """Evaluate an abi.Program on n rows.  host: id(Column) -> numpy array; tables: id(Table) -> RefTable."""
    tables = tables or {}
    ops = prog.ops
    val, oob, bad, ent = [None] * len(ops), [None] * len(ops), [None] * len(ops), {}
    zero_b = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for k, o in enumerate(ops):
            code, typ = o["code"], o["type"]
            a = val[o["a"]] if o["a"] >= 0 else None
            b = val[o["b"]] if o["b"] >= 0 else None
            dep = [j for j in (o["a"], o["b"], o["c"] if code == A.X_SELECT else -1) if j >= 0]
            of = zero_b.copy()
            bd = zero_b.copy()
            for j in dep:
                of |= oob[j]
                bd |= bad[j]
            fa = o["a"] >= 0 and ops[o["a"]]["type"] == A.T_F64
            if code == A.X_COL:
                arr = host[id(o["col"])][:n]
                r = arr.astype(object) if typ == A.T_I64 else arr.astype(np.float64)
            elif code == A.X_ROWID:
                r = np.arange(n).astype(object)
            elif code == A.X_CONST:
                r = np.full(n, float(o["imm_f"])) if typ == A.T_F64 else np.array([int(o["imm_i"])] * n, dtype=object)
                if typ == A.T_BOOL:
                    r = np.full(n, bool(o["imm_i"]))
            elif code == A.X_LOOKUP:
                t = tables[id(o["table"])]
                e = np.array([t.index.get(int(x), -1) if not bd[i] else -1 for i, x in enumerate(a)], np.int64) if n else np.zeros(0, np.int64)
                ent[k] = e
                r = e >= 0
            elif code in (A.X_FIELD, A.X_ACC):
                t, e = tables[id(ops[o["a"]]["table"])], ent[o["a"]]
                if code == A.X_FIELD:
                    raw = [t.payload[x][o["aux"]] if x >= 0 else 0 for x in e.tolist()]
                    r = np.array([from_bits(x) for x in raw], np.float64) if typ == A.T_F64 else np.array(raw, dtype=object)
                elif o["aux"] < 0:
                    r = np.array([t.hits[x] if x >= 0 else 0 for x in e.tolist()], dtype=object)
                else:
                    r = np.array([t.acc[x][o["aux"]] if x >= 0 else 0.0 for x in e.tolist()], np.float64)
            elif code in (A.X_ADD, A.X_SUB, A.X_MUL):
                r = a + b if code == A.X_ADD else a - b if code == A.X_SUB else a * b
            elif code == A.X_DIV:
                r = a / b
            elif code == A.X_NEG:
                r = -a
            elif code == A.X_I2F:
                r = np.array([float(x) for x in a], np.float64)          # int -> float: round to nearest, ties to even
            elif code in (A.X_YEAR, A.X_DIVI, A.X_MODI):
                d = 10000 if code == A.X_YEAR else int(o["imm_i"])
                q = np.array([_trunc_div(int(x), d) for x in a], dtype=object)
                r = q if code != A.X_MODI else a - q * d
            elif code == A.X_PACK2:
                lo_ok = np.array([0 <= int(x) <= 0xFFFFFFFF for x in a], bool) & np.array([0 <= int(x) <= 0xFFFFFFFF for x in b], bool)
                bd = bd | ~lo_ok
                packed = [((int(x) & 0xFFFFFFFF) << 32) | (int(y) & 0xFFFFFFFF) for x, y in zip(a, b)]
                r = np.array([p - (1 << 64) if p > I64_HI else p for p in packed], dtype=object)
            elif A.X_LT <= code <= A.X_NE:
                if fa:
                    r = [a < b, a <= b, a > b, a >= b, a == b, a != b][code - A.X_LT]
                else:
                    r = np.array([[x < y, x <= y, x > y, x >= y, x == y, x != y][code - A.X_LT] for x, y in zip(a, b)], bool)
            elif code == A.X_AND:
                r = a & b
            elif code == A.X_OR:
                r = a | b
            elif code == A.X_NOT:
                r = ~a
            elif code == A.X_SELECT:
                c = val[o["c"]]
                r = np.where(a, b, c)
                if typ == A.T_I64:
                    r = r.astype(object)
            elif code in (A.X_STR, A.X_STRIDX, A.X_CHAR):
                texts = host[id(o["col"])][:n].tolist()                  # the field up to its first NUL
                if code == A.X_CHAR:
                    r = np.array([ord(s[o["aux"]]) if 0 <= o["aux"] < len(s) else 0 for s in texts], dtype=object)
                elif code == A.X_STRIDX:
                    r = np.array([s.find(o["text"]) for s in texts], dtype=object)
                else:
                    t, mode = o["text"], o["aux"]
                    f = {A.STR_EQ: lambda s: s == t, A.STR_NE: lambda s: s != t, A.STR_CONTAINS: lambda s: t in s,
                         A.STR_PREFIX: lambda s: s.startswith(t), A.STR_SUFFIX: lambda s: s.endswith(t)}[mode]
                    r = np.array([f(s) for s in texts], bool)
            else:
                raise AssertionError("operation %d not in the vocabulary" % code)
            if typ == A.T_I64:
                of = of | np.array([not (I64_LO <= int(x) <= I64_HI) for x in r], bool)
            val[k], oob[k], bad[k] = r, of, bd
    alive = np.ones(n, bool)
    flagged, failed = zero_b.copy(), zero_b.copy()
    for g in prog.gates:
        flagged |= alive & oob[g]
        failed |= alive & bad[g]
        alive &= val[g].astype(bool)
    for j in ([prog.key] if prog.key >= 0 else []) + list(prog.vals):
        flagged |= alive & oob[j]
        failed |= alive & bad[j]
    ev = Eval()
    ev.passing, ev.flagged, ev.bad, ev.ent = alive, flagged, failed, ent
    ev.key = val[prog.key] if prog.key >= 0 else None
    ev.vals = [val[j] for j in prog.vals]
    ev.types = [ops[j]["type"] for j in prog.vals]
    return ev


# ---- 1(b): comparison rules -----------------------------------------------------------------------------------------------
def _tiny(x):
    return x == 0.0 or abs(x) <= 2.0 ** -1060


class Checker:
    """Applies the rules of the module docstring; `records` keeps (what, rows, got) of every sum for a bitwise comparison
    of two implementations."""

    def __init__(self):
        self.checks, self.records = 0, []

    def sum(self, got, xs, what):
        got = float(got)
        xs = [float(x) for x in xs]
        m = len(xs)
        self.checks += 1
        self.records.append((what, m, got, all(x == 0.0 for x in xs)))
        if any(math.isnan(x) for x in xs) or (math.inf in xs and -math.inf in xs):
            assert math.isnan(got), "%s: %r, expected NaN" % (what, got)
            return
        if math.inf in xs or -math.inf in xs:
            want = math.inf if math.inf in xs else -math.inf
            assert got == want, "%s: %r, expected %r" % (what, got, want)
            return
        if all(x == 0.0 for x in xs):
            assert bits(got) == 0, "%s: %r (%s), expected +0.0 (the reference sums from 0.0)" % (what, got, got.hex())
            return
        if m == 1:
            assert bits(got) == bits(xs[0]), "%s: one row: %s, expected %s bit for bit" % (what, got.hex(), xs[0].hex())
            return
        exact = math.fsum(xs)
        if all(_tiny(x) for x in xs):
            assert bits(got) == bits(exact + 0.0), "%s: subnormal sum %s, exact %s" % (what, got.hex(), exact.hex())
            return
        bound = (m - 1) * 2.0 ** -53 * math.fsum(abs(x) for x in xs) + math.ulp(exact)
        assert abs(got - exact) <= bound, "%s: %r vs exact %r (m=%d, bound %r)" % (what, got, exact, m, bound)

    def equal(self, got, want, what):
        self.checks += 1
        assert got == want, "%s: %r != %r" % (what, got, want)


# ---- 1(c): column families --------------------------------------------------------------------------------------------------
TEXTS = ["ABCDEFGH", "", "\U0001F600\U00010348xy", "xyABCDEF", "ABCDEFGx", "a\U0001F600", "GH", "HABCDEFG", "ABCDEFG", "zzzzzzGH"]
F_GROUPS = 16


def families(n, seed):
    """Named numpy columns of n rows.  Integer columns are sized for the specialisations: i8 (<= 256 distinct, mixed sign: 1-byte
    codes), i16 (<= 65 536 distinct: 2-byte codes), b24 / b24x (the 24-bit multiply's range and one past it: 4-byte twins),
    b32 / b32x (INT32_MIN..INT32_MAX and one past it), b62 (+-2^62), imin (minimum INT64_MIN: NEG's interval), w64 (wide, unique),
    big (beyond 2^53 for I2F).  fx holds the special doubles, laid out by the group key gk: group 0 only -0.0, 1 +-0.0, 2 subnormal
    values, 3 heavy cancellation, 4 +inf, 5 -inf, 6 NaN, 7 both infinities, 8 near DBL_MAX, 9 three decimals, 10-15 mixed.
    fy / fz are tuple operands (fy is 0.5 wherever fx is near DBL_MAX, so no product or sum overflows); txt the text edges."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    pick = lambda vals: np.array(vals, np.int64)[rng.integers(0, len(vals), n)]
    c = {}
    c["i8"] = (rng.integers(-100, 100, n) * 3 - 7).astype(np.int64)
    c["i16"] = rng.integers(-30000, 30000, n).astype(np.int64)
    c["b24"] = pick([-(1 << 23), (1 << 23) - 1, 0, -1, 1, 12345, -777])
    c["b24x"] = pick([-(1 << 23), 1 << 23, 0, -1, 3])
    c["b32"] = pick([-(1 << 31), (1 << 31) - 1, 0, -1, 7, 1 << 30])
    c["b32x"] = pick([-(1 << 31), 1 << 31, 0, 5])
    c["b62"] = pick([1 << 62, -(1 << 62), (1 << 62) - 1, -(1 << 62) + 1, 0, 3])
    c["imin"] = pick([I64_LO, -(1 << 40), -(1 << 31) - 1, -1, 0, 5])
    c["w64"] = (rng.permutation(n).astype(np.int64) * 7919 + rng.integers(-(1 << 40), 1 << 40)).astype(np.int64)
    c["big"] = pick([(1 << 53) + 1, (1 << 53) + 3, (1 << 60) + 1, I64_HI, -I64_HI, (1 << 62) + (1 << 9) + 1, -(1 << 53) - 1, 7])
    for k in ("b24", "b24x", "b32", "b32x", "b62", "imin", "big"):     # both ends present whenever the column has two rows
        vals = {"b24": [-(1 << 23), (1 << 23) - 1], "b24x": [-(1 << 23), 1 << 23], "b32": [-(1 << 31), (1 << 31) - 1], "b32x": [-(1 << 31), 1 << 31],
                "b62": [-(1 << 62), 1 << 62], "imin": [I64_LO, 5], "big": [(1 << 53) + 1, I64_HI]}[k]
        c[k][: min(n, 2)] = vals[: min(n, 2)]
    gk = (i * 7 + (i // F_GROUPS)) % F_GROUPS
    c["gk"] = gk.astype(np.int64)
    fx = np.round(rng.standard_normal(n) * 1000.0, 2)
    fx = np.where(gk == 0, -0.0, fx)
    fx = np.where(gk == 1, np.where(i % 2 == 0, 0.0, -0.0), fx)
    fx = np.where(gk == 2, rng.integers(-(1 << 14), 1 << 14, n) * 2.0 ** -1074, fx)
    canc = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 16, n)
    fx = np.where(gk == 3, np.where(i % 4 < 2, canc, -np.roll(canc, 2)) + rng.integers(-9, 9, n) * 1e-3, fx)
    fx = np.where((gk == 4) & (i % 5 == 0), np.inf, fx)
    fx = np.where((gk == 5) & (i % 5 == 1), -np.inf, fx)
    fx = np.where((gk == 6) & (i % 3 == 0), np.nan, fx)
    fx = np.where((gk == 7) & (i % 4 == 0), np.inf, np.where((gk == 7) & (i % 4 == 2), -np.inf, fx))
    fx = np.where((gk == 8) & (i % 997 == 8), np.where(i % 2 == 0, DBL_MAX / 16, -DBL_MAX / 16), fx)
    fx = np.where(gk == 9, np.round(rng.random(n) * 1000.0, 3), fx)
    fx = np.where((gk >= 10) & (i % 11 == 3), rng.integers(1, 99, n) * 2.0 ** -1070, fx)
    fx = np.where((gk >= 10) & (i % 13 == 4), -0.0, fx)
    c["fx"] = fx.astype(np.float64)
    fy = np.round(rng.random(n) * 1.5 - 0.25, 7)
    fy = np.where(i % 17 == 5, 1.0, np.where(i % 19 == 6, -0.0, np.where(i % 23 == 7, 1e-300, fy)))
    c["fy"] = np.where(gk == 8, 0.5, fy).astype(np.float64)
    c["fz"] = np.where(gk == 8, 0.25, np.round(rng.standard_normal(n) * 3.0, 9)).astype(np.float64)
    c["fsub"] = (rng.integers(-(1 << 14), 1 << 14, n) * 2.0 ** -1074).astype(np.float64)
    c["txt"] = np.array(TEXTS, "<U8")[rng.integers(0, len(TEXTS), n)]
    return c


class Bound:
    """The families of one size uploaded to one context: `col[name]` (Column), `host` (id(Column) -> numpy array)."""

    def __init__(self, ctx, cols):
        self.ctx, self.arr, self.col, self.host = ctx, cols, {}, {}
        for name, a in cols.items():
            self.col[name] = ctx.upload(np.ascontiguousarray(a))
            self.host[id(self.col[name])] = a


# ---- 1(d): typed program templates --------------------------------------------------------------------------------------------
def _row_window(P, B):
    """Gates lo <= w64 <= hi (w64 is unique): the whole column, or one row when lo = hi = its value.  Returns (lo op, hi op)."""
    w = P.op(A.X_COL, A.T_I64, col=B.col["w64"])
    lo = P.op(A.X_CONST, A.T_I64, imm_i=I64_LO)
    hi = P.op(A.X_CONST, A.T_I64, imm_i=I64_HI)
    P.gates += [P.op(A.X_GE, A.T_BOOL, a=w, b=lo), P.op(A.X_LE, A.T_BOOL, a=w, b=hi)]
    return lo, hi


def t_int_widths(B, rng):
    """xscan_sum: integer arithmetic whose operands sit on the irange boundaries (the 24-bit multiply's operands at -2^23 and
    2^23-1, results exactly at INT32_MAX and INT32_MAX+1), NEG of the INT64_MIN column under SELECT and under an add, I2F
    beyond 2^53."""
    P = A.Program()
    col = lambda name: P.op(A.X_COL, A.T_I64, col=B.col[name])
    cst = lambda v: P.op(A.X_CONST, A.T_I64, imm_i=int(v))
    i8, b24, b24x, b32, imin, big = col("i8"), col("b24"), col("b24x"), col("b32"), col("imin"), col("big")
    P.gates = [P.op(A.X_GT, A.T_BOOL, a=imin, b=cst(I64_LO)), P.op(A.X_GE, A.T_BOOL, a=i8, b=cst(int(rng.integers(-310, -250))))]
    lo, hi = _row_window(P, B)
    m24 = P.op(A.X_MUL, A.T_I64, a=b24, b=cst(255))                                      # __mul24 operands at both ends
    at_max = P.op(A.X_ADD, A.T_I64, a=b24, b=cst((1 << 31) - 1 - ((1 << 23) - 1)))         # lands on INT32_MAX exactly
    past_max = P.op(A.X_ADD, A.T_I64, a=b24, b=cst((1 << 31) - ((1 << 23) - 1)))           # ... and on INT32_MAX + 1
    m24x = P.op(A.X_SUB, A.T_I64, a=P.op(A.X_MUL, A.T_I64, a=b24x, b=cst(255)), b=b32)
    neg = P.op(A.X_NEG, A.T_I64, a=imin)
    sel = P.op(A.X_ADD, A.T_I64, a=P.op(A.X_SELECT, A.T_I64, a=P.op(A.X_LT, A.T_BOOL, a=i8, b=cst(0)), b=neg, c=cst(0)), b=cst(1))
    f = lambda k: P.op(A.X_I2F, A.T_F64, a=k)
    P.vals = [f(P.op(A.X_ADD, A.T_I64, a=m24, b=at_max)), f(P.op(A.X_SUB, A.T_I64, a=past_max, b=m24x)), f(sel),
              P.op(A.X_ADD, A.T_F64, a=f(P.op(A.X_ADD, A.T_I64, a=neg, b=cst(1))), b=f(big))]
    return P, (lo, hi)


def t_float_specials(B, rng):
    """xscan_sum: f64 arithmetic on the special values (products in the header's association, a division, comparisons against
    NaN / -0.0 / nextafter bounds, NE with NaN), text predicates at the field's edges, CHAR past the text."""
    P = A.Program()
    fx, fy, fz = (P.op(A.X_COL, A.T_F64, col=B.col[k]) for k in ("fx", "fy", "fz"))
    one = P.op(A.X_CONST, A.T_F64, imm_f=1.0)
    cut = P.op(A.X_CONST, A.T_F64, imm_f=float(rng.choice([-0.0, 0.0, math.nextafter(0.5, 1.0), -math.inf])))
    txt = B.col["txt"]
    needle = str(rng.choice(["ABCDEFGH", "GH", "\U0001F600", "H"]))
    P.gates = [P.op(A.X_OR, A.T_BOOL, a=P.op(A.X_NE, A.T_BOOL, a=fy, b=cut), b=P.op(A.X_STR, A.T_BOOL, col=txt, aux=A.STR_CONTAINS, text=needle))]
    lo, hi = _row_window(P, B)
    omb = P.op(A.X_SUB, A.T_F64, a=one, b=fy)
    v0 = P.op(A.X_SUB, A.T_F64, a=P.op(A.X_MUL, A.T_F64, a=fx, b=omb), b=P.op(A.X_MUL, A.T_F64, a=fz, b=fy))
    v1 = P.op(A.X_SELECT, A.T_F64, a=P.op(A.X_LE, A.T_BOOL, a=fx, b=cut), b=P.op(A.X_NEG, A.T_F64, a=fx), c=P.op(A.X_DIV, A.T_F64, a=fz, b=fy))
    idx = P.op(A.X_STRIDX, A.T_I64, col=txt, text="GH")
    ch = P.op(A.X_ADD, A.T_I64, a=P.op(A.X_CHAR, A.T_I64, col=txt, aux=7), b=P.op(A.X_CHAR, A.T_I64, col=txt, aux=0))
    suf = P.op(A.X_STR, A.T_BOOL, col=txt, aux=A.STR_SUFFIX, text="GH")
    v2 = P.op(A.X_I2F, A.T_F64, a=P.op(A.X_ADD, A.T_I64, a=P.op(A.X_MUL, A.T_I64, a=idx, b=P.op(A.X_CONST, A.T_I64, imm_i=1 << 22)), b=ch))
    v3 = P.op(A.X_SELECT, A.T_F64, a=P.op(A.X_AND, A.T_BOOL, a=suf, b=P.op(A.X_STR, A.T_BOOL, col=txt, aux=A.STR_PREFIX, text="ABCDEFG")),
              b=P.op(A.X_COL, A.T_F64, col=B.col["fsub"]), c=P.op(A.X_MUL, A.T_F64, a=fx, b=fx))
    P.vals = [v0, v1, v2, v3]
    return P, (lo, hi)


def t_group_trunc(B, rng):
    """xgroupby: the key from MODI / DIVI of a mixed-sign column (C truncation: a floor would move rows between groups) and the
    f64 values of the special layout, summed per group through the group accumulators."""
    P = A.Program()
    i8 = P.op(A.X_COL, A.T_I64, col=B.col["i8"])
    cst = lambda v: P.op(A.X_CONST, A.T_I64, imm_i=int(v))
    P.gates = [P.op(A.X_NE, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["b32"]), b=cst(int(rng.choice([7, 0, -1]))))]
    m = P.op(A.X_ADD, A.T_I64, a=P.op(A.X_MODI, A.T_I64, a=i8, imm_i=8), b=cst(7))
    d = P.op(A.X_ADD, A.T_I64, a=P.op(A.X_DIVI, A.T_I64, a=i8, imm_i=50), b=cst(6))
    P.key = P.op(A.X_ADD, A.T_I64, a=P.op(A.X_MUL, A.T_I64, a=m, b=cst(12)), b=d)
    P.vals = [P.op(A.X_COL, A.T_F64, col=B.col["fsub"]), P.op(A.X_I2F, A.T_F64, a=P.op(A.X_COL, A.T_I64, col=B.col["big"]))]
    return P


def t_group_special(B, rng):
    """xgroupby on the special layout's own group key: each group's f64 sums follow its rule (zeros, subnormal, NaN, inf...)."""
    P = A.Program()
    fx, fy = P.op(A.X_COL, A.T_F64, col=B.col["fx"]), P.op(A.X_COL, A.T_F64, col=B.col["fy"])
    P.gates = [P.op(A.X_GE, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["i16"]), b=P.op(A.X_CONST, A.T_I64, imm_i=int(rng.integers(-30001, -20000))))]
    P.key = P.op(A.X_COL, A.T_I64, col=B.col["gk"])
    P.vals = [fx, P.op(A.X_MUL, A.T_F64, a=fx, b=P.op(A.X_SUB, A.T_F64, a=P.op(A.X_CONST, A.T_F64, imm_f=1.0), b=fy)),
              P.op(A.X_NEG, A.T_F64, a=fx)]
    return P


def t_build_neg(B, rng):
    """xbuild keyed by NEG of the INT64_MIN column (that row gated out), payload i64 and f64: the queue words' width follows the
    key's interval."""
    P = A.Program()
    imin = P.op(A.X_COL, A.T_I64, col=B.col["imin"])
    P.gates = [P.op(A.X_GT, A.T_BOOL, a=imin, b=P.op(A.X_CONST, A.T_I64, imm_i=I64_LO)),
               P.op(A.X_LE, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["i8"]), b=P.op(A.X_CONST, A.T_I64, imm_i=int(rng.integers(200, 300))))]
    P.key = P.op(A.X_NEG, A.T_I64, a=imin)
    P.vals = [P.op(A.X_COL, A.T_I64, col=B.col["i8"]), P.op(A.X_COL, A.T_F64, col=B.col["fz"])]
    return P


def t_build_w(B, rng):
    """xbuild keyed by the unique wide column with its f64 payload: the table the probe templates look up."""
    P = A.Program()
    P.gates = [P.op(A.X_GE, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["i8"]), b=P.op(A.X_CONST, A.T_I64, imm_i=int(rng.integers(-200, 100))))]
    P.key = P.op(A.X_COL, A.T_I64, col=B.col["w64"])
    P.vals = [P.op(A.X_COL, A.T_F64, col=B.col["fz"]), P.op(A.X_COL, A.T_I64, col=B.col["b32"])]
    return P


def t_probe(B, rng, table, neg_table):
    """xscan_sum of fields of two lookups: one by the wide key, one by NEG of the INT64_MIN column (the key a lookup takes)."""
    P = A.Program()
    lk = P.op(A.X_LOOKUP, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["w64"]), table=table)
    imin = P.op(A.X_COL, A.T_I64, col=B.col["imin"])
    ln = P.op(A.X_LOOKUP, A.T_BOOL, a=P.op(A.X_NEG, A.T_I64, a=imin), table=neg_table)
    P.gates = [P.op(A.X_NE, A.T_BOOL, a=imin, b=P.op(A.X_CONST, A.T_I64, imm_i=I64_LO)), lk]
    P.vals = [P.op(A.X_FIELD, A.T_F64, a=lk, aux=0), P.op(A.X_I2F, A.T_F64, a=P.op(A.X_FIELD, A.T_I64, a=lk, aux=1)),
              P.op(A.X_SELECT, A.T_F64, a=ln, b=P.op(A.X_FIELD, A.T_F64, a=ln, aux=1), c=P.op(A.X_CONST, A.T_F64, imm_f=0.0)),
              P.op(A.X_I2F, A.T_F64, a=P.op(A.X_FIELD, A.T_I64, a=ln, aux=0))]
    return P, lk


def t_probe_agg(B, rng, table):
    """xprobe_aggregate into the wide-keyed table: the special doubles summed into the HBM accumulators of the matched entries."""
    P = A.Program()
    lk = P.op(A.X_LOOKUP, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["w64"]), table=table)
    P.gates = [lk, P.op(A.X_LT, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col["gk"]), b=P.op(A.X_CONST, A.T_I64, imm_i=int(rng.integers(8, 17))))]
    P.vals = [P.op(A.X_COL, A.T_F64, col=B.col["fx"]), P.op(A.X_COL, A.T_F64, col=B.col["fsub"])]
    return P, lk


def t_acc_read(B, rng, table, lk_table_key="w64"):
    """xscan_sum reading ACC (sum and row count) of the table the probe-aggregate filled."""
    P = A.Program()
    lk = P.op(A.X_LOOKUP, A.T_BOOL, a=P.op(A.X_COL, A.T_I64, col=B.col[lk_table_key]), table=table)
    P.gates = [lk, P.op(A.X_GT, A.T_BOOL, a=P.op(A.X_ACC, A.T_I64, a=lk, aux=-1), b=P.op(A.X_CONST, A.T_I64, imm_i=0))]
    P.vals = [P.op(A.X_ACC, A.T_F64, a=lk, aux=1), P.op(A.X_I2F, A.T_F64, a=P.op(A.X_ACC, A.T_I64, a=lk, aux=-1))]
    return P


def t_key_set(B, rng):
    """xkey_set keyed by NEG of a mixed-sign coded column plus a constant, gated by a text predicate."""
    P = A.Program()
    P.gates = [P.op(A.X_STR, A.T_BOOL, col=B.col["txt"], aux=int(rng.choice([A.STR_NE, A.STR_PREFIX])), text=str(rng.choice(["ABCDEFGH", "xy"])))]
    P.key = P.op(A.X_ADD, A.T_I64, a=P.op(A.X_NEG, A.T_I64, a=P.op(A.X_COL, A.T_I64, col=B.col["i8"])), b=P.op(A.X_CONST, A.T_I64, imm_i=400))
    return P


def _no_overflow(ev, what):
    assert not ev.flagged.any(), "%s: the draw leaves int64 on a row that reaches a value" % what
    assert not ev.bad.any(), "%s: a PACK2 part out of range" % what


def _check_scan(ctx, chk, B, n, P, window, what, tables=None, singles=3, rng=None):
    ev = evaluate(P, n, B.host, tables)
    _no_overflow(ev, what)
    vals, cnt = ctx.xscan_sum(n, P)
    chk.equal(cnt, int(ev.passing.sum()), what + " count")
    for v in range(len(P.vals)):
        chk.sum(vals[v], ev.vals[v][ev.passing], "%s v%d" % (what, v))
    if window is None or not singles:
        return
    lo, hi = window
    rows = np.nonzero(ev.passing)[0]
    w = B.arr["w64"]
    for r in (rng.choice(rows, min(singles, len(rows)), replace=False).tolist() if len(rows) else []):
        P.set_const(lo, int(w[r])); P.set_const(hi, int(w[r]))
        vals, cnt = ctx.xscan_sum(n, P)
        chk.equal(cnt, 1, "%s row %d count" % (what, r))
        for v in range(len(P.vals)):
            chk.sum(vals[v], [ev.vals[v][r]], "%s row %d v%d" % (what, r, v))
    P.set_const(lo, I64_LO); P.set_const(hi, I64_HI)


def _check_groups(chk, keys, vals, cnts, ev, what):
    want = {}
    for r in np.nonzero(ev.passing)[0].tolist():
        want.setdefault(int(ev.key[r]), []).append(r)
    chk.equal(sorted(int(k) for k in keys), sorted(want), what + " keys")
    order = np.argsort(np.asarray(keys, np.int64), kind="stable")
    for g in order.tolist():
        k = int(keys[g])
        rows = want[k]
        chk.equal(int(cnts[g]), len(rows), "%s key %d count" % (what, k))
        for v in range(len(ev.vals)):
            chk.sum(vals[g][v], ev.vals[v][rows].tolist(), "%s key %d v%d" % (what, k, v))


def program_case(ctx, n, seed, chk=None):
    """Every template once on the families of n rows: xscan_sum (all rows and single rows), xgroupby, xbuild followed by
    LOOKUP / FIELD / ACC, xprobe_aggregate, xkey_set.  A draw whose evaluation would leave int64 on a row that reaches a key or a
    value is drawn again (such rows may only appear gated out).  Returns the Checker."""
    chk = chk or Checker()
    rng = np.random.default_rng(seed)
    B = Bound(ctx, families(n, seed))
    for make, tag in ((t_int_widths, "int widths"), (t_float_specials, "float specials")):
        for _ in range(8):
            P, window = make(B, rng)
            if not evaluate(P, n, B.host).flagged.any():
                break
        _check_scan(ctx, chk, B, n, P, window, "%s n=%d" % (tag, n), rng=rng)
    for make, tag in ((t_group_trunc, "group trunc"), (t_group_special, "group special")):
        P = make(B, rng)
        ev = evaluate(P, n, B.host)
        _no_overflow(ev, tag)
        keys, vals, cnts = ctx.xgroupby(n, P)
        _check_groups(chk, keys.tolist(), vals.tolist(), cnts.tolist(), ev, "%s n=%d" % (tag, n))
    # builds: one keyed by NEG(imin) (no bounds known: open addressing), one by the unique wide key with accumulators
    tables = {}
    built = []
    for make, acc in ((t_build_neg, False), (t_build_w, True)):
        P = make(B, rng)
        ev = evaluate(P, n, B.host)
        _no_overflow(ev, make.__name__)
        ref = RefTable(len(P.vals))
        for r in np.nonzero(ev.passing)[0].tolist():
            ref.add(int(ev.key[r]), [int(x[r]) if t == A.T_I64 else bits(x[r]) for x, t in zip(ev.vals, ev.types)])
        t = ctx.xbuild(n, P, accumulate=acc)
        chk.equal(t.size(), len(ref.index), "%s n=%d entries" % (make.__name__, n))
        kcol, pcols, _, _, ne = ctx.table_columns(t, 0)
        got = {int(k): [int(p.download()[i]) for p in pcols] for i, k in enumerate(kcol.download().tolist())} if ne else {}
        chk.equal(got, {k: ref.payload[e] for k, e in ref.index.items()}, "%s n=%d entries" % (make.__name__, n))
        del kcol, pcols
        tables[id(t)] = ref
        built.append(t)
    t_neg, t_w = built
    P, _ = t_probe(B, rng, t_w, t_neg)
    _check_scan(ctx, chk, B, n, P, None, "probe n=%d" % n, tables)
    P, lk = t_probe_agg(B, rng, t_w)
    ev = evaluate(P, n, B.host, tables)
    _no_overflow(ev, "probe-aggregate")
    ctx.xprobe_aggregate(n, P, lk, t_w)
    ref = tables[id(t_w)]
    for r in np.nonzero(ev.passing)[0].tolist():
        e = int(ev.ent[lk][r])
        ref.hits[e] += 1
        for v in range(len(P.vals)):
            ref.parts[e][v].append(float(ev.vals[v][r]))
    for e in range(len(ref.hits)):
        for v in range(len(P.vals)):
            ref.acc[e][v] = math.fsum(ref.parts[e][v]) if ref.parts[e][v] else 0.0
    kcol, _, acols, hcol, ne = ctx.table_columns(t_w, 1)
    ks = kcol.download().tolist() if ne else []
    hs = hcol.download().tolist() if ne else []
    accs = [a.download().tolist() if ne else [] for a in acols]
    chk.equal(sorted(ks), sorted(k for k, e in ref.index.items() if ref.hits[e]), "probe-aggregate n=%d entries" % n)
    got_acc = {}
    for i, k in enumerate(ks):
        e = ref.index[k]
        chk.equal(hs[i], ref.hits[e], "probe-aggregate n=%d key %d hits" % (n, k))
        for v in range(len(P.vals)):
            chk.sum(accs[v][i], ref.parts[e][v], "probe-aggregate n=%d key %d v%d" % (n, k, v))
            got_acc[(e, v)] = accs[v][i]
    for (e, v), x in got_acc.items():                               # later loops read what the device accumulated
        ref.acc[e][v] = x
    del kcol, acols, hcol
    P = t_acc_read(B, rng, t_w)
    _check_scan(ctx, chk, B, n, P, None, "acc read n=%d" % n, tables)
    P = t_key_set(B, rng)
    ev = evaluate(P, n, B.host)
    _no_overflow(ev, "key set")
    ts = ctx.xkey_set(n, P, 0, 1000)
    want = set(int(k) for k in ev.key[ev.passing])
    chk.equal(ts.size(), len(want), "key set n=%d size" % n)
    Q = A.Program()
    lk = Q.op(A.X_LOOKUP, A.T_BOOL, a=Q.op(A.X_ADD, A.T_I64, a=Q.op(A.X_COL, A.T_I64, col=B.col["i16"]), b=Q.op(A.X_CONST, A.T_I64, imm_i=0)), table=ts)
    Q.gates = [lk]
    Q.vals = [Q.op(A.X_COL, A.T_F64, col=B.col["fz"])]
    hit = np.array([int(x) in want for x in B.arr["i16"][:n].tolist()], bool)
    vals, cnt = ctx.xscan_sum(n, Q)
    chk.equal(cnt, int(hit.sum()), "key set n=%d probe count" % n)
    chk.sum(vals[0], B.arr["fz"][:n][hit].tolist(), "key set n=%d probe" % n)
    for t in built + [ts]:
        t.free()
    return chk


def changed_contents_case(ctx, chk=None):
    """One program run, then values outside the column's earlier range copied in (sdqh_column_copy_in), then the same Program
    again: the answer follows the new contents (the cached minimum / maximum and codes feed the integer widths)."""
    chk = chk or Checker()
    n = 4097
    rng = np.random.default_rng(77)
    small = rng.integers(-100, 100, n).astype(np.int64)
    col = ctx.upload(small.copy())
    host = {id(col): small}
    P = A.Program()
    x = P.op(A.X_COL, A.T_I64, col=col)
    cst = lambda v: P.op(A.X_CONST, A.T_I64, imm_i=v)
    P.gates = [P.op(A.X_GT, A.T_BOOL, a=x, b=cst(I64_LO))]
    P.vals = [P.op(A.X_I2F, A.T_F64, a=P.op(A.X_ADD, A.T_I64, a=P.op(A.X_MUL, A.T_I64, a=x, b=cst(3)), b=cst(1))),
              P.op(A.X_I2F, A.T_F64, a=P.op(A.X_NEG, A.T_I64, a=x))]
    for stage in range(2):
        ev = evaluate(P, n, host)
        _no_overflow(ev, "changed contents")
        vals, cnt = ctx.xscan_sum(n, P)
        chk.equal(cnt, int(ev.passing.sum()), "changed contents stage %d count" % stage)
        for v in range(len(P.vals)):
            chk.sum(vals[v], ev.vals[v][ev.passing].tolist(), "changed contents stage %d v%d" % (stage, v))
        if stage == 0:
            new = small.copy()
            new[::7] = np.array([1 << 40, -(1 << 40), (1 << 31), -(1 << 31) - 1, 1 << 23], np.int64)[np.arange(len(new[::7])) % 5]
            src = np.ascontiguousarray(new)
            ctx.copy_in(col, 0, n, src.ctypes.data)
            ctx.synchronize()
            small[:] = new
    return chk


# ---- 2: the fixed tuple shapes --------------------------------------------------------------------------------------------
SHAPES = (A.TUPLE_A, A.TUPLE_AB, A.TUPLE_A_1MB, A.TUPLE_PRICING, A.TUPLE_A_1MB_M_CD, A.TUPLE_COUNT)
SHAPE_NAMES = {A.TUPLE_A: "A", A.TUPLE_AB: "AB", A.TUPLE_A_1MB: "A_1MB", A.TUPLE_PRICING: "PRICING", A.TUPLE_A_1MB_M_CD: "A_1MB_M_CD", A.TUPLE_COUNT: "COUNT"}
SHAPE_OPERANDS = {A.TUPLE_A: ("fx",), A.TUPLE_AB: ("fx", "fy"), A.TUPLE_A_1MB: ("fx", "fy"), A.TUPLE_PRICING: ("fz", "fx", "fy", "fy"),
                  A.TUPLE_A_1MB_M_CD: ("fx", "fy", "fz", "fy"), A.TUPLE_COUNT: ()}


def tuple_rows(shape, a=None, b=None, c=None, d=None):
    """The tuple's per-row doubles in the header's association (include/sdqh.h), one numpy operation at a time."""
    with np.errstate(all="ignore"):
        if shape == A.TUPLE_A:
            return [a]
        if shape == A.TUPLE_AB:
            return [a * b]
        if shape == A.TUPLE_A_1MB:
            return [a * (1.0 - b)]
        if shape == A.TUPLE_PRICING:
            dp = b * (1.0 - c)
            return [a, b, dp, dp * (1.0 + d)]
        if shape == A.TUPLE_A_1MB_M_CD:
            return [a * (1.0 - b) - c * d]
        return []


def float_filters(fx):
    """(lo, hi) ranges on the special column: bounds at +-inf, +-0.0 and nextafter of a value in it; NaN fails every one."""
    finite = fx[np.isfinite(fx) & (fx != 0.0)]
    v = float(finite[len(finite) // 2]) if len(finite) else 1.5
    return [(-math.inf, math.inf), (-0.0, 0.0), (0.0, math.inf), (-math.inf, -0.0), (v, math.nextafter(v, math.inf)),
            (math.nextafter(v, -math.inf), v), (math.nextafter(v, math.inf), math.inf), (math.inf, math.inf)]


def shape_case(ctx, n, seed, chk=None, filters=None):
    """Every SDQH_TUPLE_* shape through scan_filter_sum, groupby_small, groupby_key, hash_probe_aggregate and lookup_aggregate on
    the families of n rows, with f64 range filters on the special column.  Single-row groups (groupby_key by the unique column, the
    probe by unique keys) are bitwise against the per-row formula."""
    chk = chk or Checker()
    rng = np.random.default_rng(seed)
    B = Bound(ctx, families(n, seed))
    arr = {k: v[:n] for k, v in B.arr.items()}
    fx = arr["fx"]
    flts = filters if filters is not None else float_filters(fx)
    gk = arr["gk"]
    w = arr["w64"]
    # a unique-keyed build of every row (the probes' table) with one f64 payload
    tb = ctx.hash_build_unique(n, A.make_filter(), [], B.col["w64"], [B.col["fz"]], accumulate=True)
    for shape in SHAPES:
        name = SHAPE_NAMES[shape]
        ops = SHAPE_OPERANDS[shape]
        per_row = tuple_rows(shape, *[arr[k] for k in ops])
        tup = A.make_tuple(shape, [B.col[k] for k in ops])
        for fi, (lo, hi) in enumerate(flts):
            m = (fx >= lo) & (fx <= hi)
            what = "%s n=%d filter %d [%r, %r]" % (name, n, fi, lo, hi)
            flt = A.make_filter(fpreds=[(B.col["fx"], lo, hi)])
            vals, cnt = ctx.scan_filter_sum(n, flt, tup)
            chk.equal(cnt, int(m.sum()), what + " scan count")
            for v, x in enumerate(per_row):
                chk.sum(vals[v], x[m].tolist(), what + " scan v%d" % v)
            keys, gv, gc = ctx.groupby_small(n, flt, [B.col["gk"]], tup, max_groups=64)
            _check_keyed(chk, keys[:, 0].tolist(), gv.tolist(), gc.tolist(), gk, m, per_row, what + " groupby_small")
        # one row per group: groupby_key by the unique column, inside a window of rows
        sel = rng.choice(n, min(n, 300), replace=False)
        lo_w = int(np.sort(w[sel])[0]); hi_w = int(np.sort(w[sel])[-1])
        m = (w >= lo_w) & (w <= hi_w)
        flt = A.make_filter(ipreds=[(B.col["w64"], lo_w, hi_w)])
        t = ctx.groupby_key(n, flt, B.col["w64"], tup)
        _check_table(ctx, chk, t, w, m, per_row, "%s n=%d groupby_key" % (name, n))
        t.free()
        # probe-aggregate into the unique build: every entry gets one row
        t2 = ctx.hash_build_unique(n, A.make_filter(), [], B.col["w64"], [B.col["fz"]], accumulate=True)
        ctx.hash_probe_aggregate(n, A.make_filter(fpreds=[(B.col["fx"], -math.inf, math.inf)]), t2, B.col["w64"], tup)
        _check_table(ctx, chk, t2, w, ~np.isnan(fx), per_row, "%s n=%d probe" % (name, n))
        t2.free()
        # lookup_aggregate: operands through the lookup's payload bits (fz) and columns, keyed by the special groups
        ops_src = [A.src_lookup(0, 0) if k == "fz" else A.src_col(B.col[k]) for k in ops]
        for fi, (lo, hi) in enumerate(flts[:3]):
            m = (fx >= lo) & (fx <= hi)
            flt = A.make_filter(fpreds=[(B.col["fx"], lo, hi)])
            keys, gv, gc = ctx.lookup_aggregate(n, flt, [(tb, [A.src_col(B.col["w64"])])], [A.src_col(B.col["gk"])], shape, ops_src)
            _check_keyed(chk, keys[:, 0].tolist(), gv.tolist(), gc.tolist(), gk, m, per_row, "%s n=%d filter %d lookup_aggregate" % (name, n, fi))
    tb.free()
    return chk


def _check_keyed(chk, keys, vals, cnts, key_arr, m, per_row, what):
    want = {}
    for r in np.nonzero(m)[0].tolist():
        want.setdefault(int(key_arr[r]), []).append(r)
    chk.equal(sorted(keys), sorted(want), what + " keys")
    for g in np.argsort(np.asarray(keys, np.int64), kind="stable").tolist():
        rows = want[int(keys[g])]
        chk.equal(int(cnts[g]), len(rows), "%s key %d count" % (what, keys[g]))
        for v, x in enumerate(per_row):
            chk.sum(vals[g][v], x[rows].tolist(), "%s key %d v%d" % (what, keys[g], v))


def _check_table(ctx, chk, t, key_arr, m, per_row, what):
    kcol, _, acols, hcol, ne = ctx.table_columns(t, 1)
    ks = kcol.download().tolist() if ne else []
    hs = hcol.download().tolist() if ne else []
    accs = [a.download().tolist() if ne else [] for a in acols]
    del kcol, acols, hcol
    row_of = {}
    for r in np.nonzero(m)[0].tolist():
        row_of.setdefault(int(key_arr[r]), []).append(r)
    chk.equal(sorted(ks), sorted(row_of), what + " keys")
    for i in np.argsort(np.asarray(ks, np.int64), kind="stable").tolist():
        rows = row_of[ks[i]]
        chk.equal(hs[i], len(rows), "%s key %d hits" % (what, ks[i]))
        for v, x in enumerate(per_row):
            chk.sum(accs[v][i], x[rows].tolist(), "%s key %d v%d" % (what, ks[i], v))


def all_cases(ctx, sizes=SIZES, seeds=(1,)):
    """The program templates (per seed) and the tuple shapes at every size, then the changed-contents case: one Checker."""
    chk = Checker()
    for n in sizes:
        for seed in seeds:
            program_case(ctx, n, seed * 1000 + n, chk)
        shape_case(ctx, n, 500 + n, chk)
    changed_contents_case(ctx, chk)
    return chk
