"""What the tests of the window-moments extension (include/sdqh_sort_wmoments.h) compare against.  Nothing here reads the product's
fold code.

EXACT.  The inputs are dyadic doubles — integers or quarters, possibly offset by 2^30 — so scaled by SCALE they are Python integers, and
the prefix sums of x, x^2, xy and |x| give every frame's means, Q, C and A exactly — ratios of Python integers, fractions.Fraction for one
frame (Frames.exact) — in O(1) per frame (Exact.frames).  The header's two bounds are q_bound / c_bound.  What the ops make of Q^ and
C^ is bounded by the propagation of tests/moments_reference.py (Exact.value there) with these bounds in the place of the two-pass ones
— a frame's mean is off by at most L u A <= m u A, which is what that propagation allows for: FrameExact inherits it, `values` is the
same propagation formula by formula over arrays (the tests hold the two against each other).  The one quantity of the bounds that
prefix sums do not give, sum|dx dy|, is evaluated in doubles after an exact shift of the columns and the means by the first row's values
(the inputs are dyadic and small beside 2^53): its relative error of a few m u is nothing beside the bound's constant.  Wide frames
over columns of few distinct values take it from prefix counts of the value pairs (Exact._abs_c), not row by row.

THE PINNED FOLD.  Tree / finish restate the header's leaf, merge, tree and query in Python floats — IEEE doubles, one operation per
step, no FMA — and the finish with math.sqrt (correctly rounded)."""
import math
from fractions import Fraction

import numpy as np

import moments_reference as mref

U = mref.U
NULL_BITS = mref.NULL_BITS
OPS = mref.OPS
UNI, BI = OPS[:4], OPS[4:]
SCALE = 4                                    # the inputs are multiples of 1 / SCALE
C_BOUND = 8.0                                # the header's constant c (DESIGN.md section 4o derives it)
NAN = float(np.array([NULL_BITS], np.uint64).view(np.float64)[0])


def levels(m):
    """L = ceil(log2 m) + 1 (1 for m = 1)"""
    return 1 if m <= 1 else (m - 1).bit_length() + 1


def q_bound(m, q, a):
    """the header's |Q^ - Q|"""
    lu = levels(m) * U
    q = float(q)
    return C_BOUND * (lu * q + lu * a * math.sqrt(m * q) + m * (lu * a) ** 2)


def c_bound(m, abs_c, ax, ay, qx, qy):
    """the header's |C^ - C|"""
    lu = levels(m) * U
    return C_BOUND * (lu * abs_c + lu * (ax * math.sqrt(m * float(qy)) + ay * math.sqrt(m * float(qx))) + m * (lu * ax) * (lu * ay))


class FrameExact(mref.Exact):
    """One frame's exact moments with the bounds of sdqh_sort_wmoments.h; value(op) is moments_reference's propagation over them."""

    def __init__(self, m, muy, qy, ay, mux=None, qx=None, c=None, ax=None, abs_c=None):
        self.m, self.muy, self.qy, self.ay = m, muy, qy, ay
        self.mux, self.qx, self.c, self.ax, self.abs_c = mux, qx, c, ax, abs_c

    def q_bound(self, q, a):
        return q_bound(self.m, q, a)

    def c_bound(self):
        return c_bound(self.m, self.abs_c, self.ax, self.ay, self.qx, self.qy)


def _obj(a):
    out = np.empty(len(a), object)
    out[:] = [int(t) for t in a]
    return out


def _f64(a):
    return np.array([float(t) for t in a], np.float64)


class Frames:
    """The exact moments of many frames at once, each a ratio of Python integers (object arrays: no rounding, no overflow), and their
    correctly rounded doubles: m; muy, qy, ay — with x: mux, qx, c, ax, abs_c (see the module's docstring for abs_c)."""

    def exact(self, j, two=False):
        """frame j as a FrameExact of fractions.Fraction: moments_reference's propagation applies to it as it stands"""
        m, d1, d2 = int(self.m[j]), int(self.m[j]) * SCALE, int(self.m[j]) * SCALE * SCALE
        fe = FrameExact(m, Fraction(int(self.sy[j]), d1), Fraction(int(self.qy_num[j]), d2), float(self.ay[j]))
        if two:
            fe.mux, fe.qx, fe.c = Fraction(int(self.sx[j]), d1), Fraction(int(self.qx_num[j]), d2), Fraction(int(self.c_num[j]), d2)
            fe.ax, fe.abs_c = float(self.ax[j]), float(self.abs_c[j])
        return fe

    def take(self, idx):
        """the frames idx[0], idx[1], ... of these (a frame may come many times)"""
        out = Frames()
        out.__dict__.update({k: v[idx] if isinstance(v, np.ndarray) else v for k, v in self.__dict__.items()})
        return out

    def swapped(self):
        """the same frames with the measures' roles exchanged (for the ops of one measure over x)"""
        out = Frames()
        out.__dict__.update(self.__dict__)
        out.sy, out.sx, out.qy_num, out.qx_num, out.muy, out.mux, out.qy, out.qx, out.ay, out.ax = self.sx, self.sy, self.qx_num, self.qy_num, self.mux, self.muy, self.qx, self.qy, self.ax, self.ay
        return out


class Exact:
    """The definition over every frame of the sorted columns y and x (x = None: y again): dyadic doubles, multiples of 1 / SCALE."""

    def __init__(self, y, x=None):
        self.y = np.ascontiguousarray(y, np.float64)
        self.x = self.y if x is None else np.ascontiguousarray(x, np.float64)

        def scaled(v):
            out = _obj((v * SCALE).tolist())
            assert all(float(t) / SCALE == float(u) for t, u in zip(out, v.tolist())), "the inputs are multiples of 1 / SCALE"
            return out

        def prefix(vals):
            out = np.empty(len(vals) + 1, object)
            out[0] = 0
            out[1:] = np.cumsum(vals) if len(vals) else []
            return out
        ys, xs = scaled(self.y), scaled(self.x)
        self.y0s, self.x0s = (int(ys[0]), int(xs[0])) if len(ys) else (0, 0)
        self.py, self.pyy, self.pay = prefix(ys), prefix(ys * ys), prefix(abs(ys))
        self.px, self.pxx, self.pax, self.pxy = prefix(xs), prefix(xs * xs), prefix(abs(xs)), prefix(xs * ys)

    def frames(self, l, r, abs_c=False):
        """the Frames of the positions [l[j], r[j]] (l <= r)"""
        l, r = np.asarray(l, np.int64), np.asarray(r, np.int64) + 1
        f = Frames()
        m = f.m = _obj(r - l)
        d1, d2 = m * SCALE, m * (SCALE * SCALE)
        f.sy, f.sx = self.py[r] - self.py[l], self.px[r] - self.px[l]
        f.qy_num, f.qx_num = m * (self.pyy[r] - self.pyy[l]) - f.sy * f.sy, m * (self.pxx[r] - self.pxx[l]) - f.sx * f.sx
        f.c_num = m * (self.pxy[r] - self.pxy[l]) - f.sx * f.sy
        f.muy, f.mux, f.qy, f.qx, f.c = _f64(f.sy / d1), _f64(f.sx / d1), _f64(f.qy_num / d2), _f64(f.qx_num / d2), _f64(f.c_num / d2)
        f.ay, f.ax = _f64((self.pay[r] - self.pay[l]) / d1), _f64((self.pax[r] - self.pax[l]) / d1)
        f.mf = _f64(m)
        # REGR_INTERCEPT = muy - (C / Qx) mux as one ratio: the difference cancels, so it is not formed in doubles
        den = d1 * f.qx_num
        live = den != 0
        f.intercept = np.full(len(m), np.nan)
        f.intercept[live] = _f64((f.sy * f.qx_num - f.c_num * f.sx)[live] / den[live])
        if abs_c:
            f.abs_c = self._abs_c(l, r, _f64((f.sx - m * self.x0s) / d1), _f64((f.sy - m * self.y0s) / d1))      # the means beside the first row's values: exact, rounded once
        return f


ABS_C_ALPHABET = 4096                        # at most so many distinct (x, y) pairs: sum|dx dy| of wide frames goes through prefix counts


def _abs_c_method(self, l, r, mx, my):
    """sum|(x_i - mux)(y_i - muy)| over [l, r) per frame, in doubles after an exact shift of the columns and of the means (mx, my) by
    the first row's values (the inputs are dyadic and of one magnitude).  Narrow frames: row by row.  Wide ones — an unbounded side makes the row-by-row sum quadratic —, where the columns
    take few distinct (x, y) pairs: sum over the pairs of (how often the pair lies in the frame) * |dx dy|, the counts from prefix
    counts walked in blocks of positions; the same sum in another order."""
    n, nf = len(self.y), len(l)
    out = np.zeros(nf, np.float64)
    if nf == 0:
        return out
    xs, ys = self.x - self.x[0], self.y - self.y[0]
    pairs, code = np.unique(np.stack((xs, ys), 1), axis=0, return_inverse=True)
    code = code.ravel()
    if int((r - l).sum()) <= 4 * len(pairs) * nf or len(pairs) > ABS_C_ALPHABET:      # (the counts cost a frame about as much as 4 K of its rows)
        for j in range(nf):
            a, b = int(l[j]), int(r[j])
            out[j] = np.abs((xs[a:b] - mx[j]) * (ys[a:b] - my[j])).sum()
        return out
    K, block = len(pairs), 2048
    for sign, at in ((1.0, r), (-1.0, l)):                                  # counts(r) - counts(l), each against the frame's own means
        order = np.argsort(at, kind="stable")
        run = np.zeros(K, np.int64)
        lo = 0
        for p0 in range(0, n + 1, block):                                   # prefix positions [p0, p0 + block): counts of the rows before each
            hi = np.searchsorted(at[order], p0 + block, "left")
            if hi > lo:
                onehot = np.zeros((block, K), np.int64)
                rows = np.arange(p0, min(p0 + block, n))
                onehot[rows - p0, code[rows]] = 1
                cnt = run + np.concatenate((np.zeros((1, K), np.int64), np.cumsum(onehot, 0)[:-1]))
                js = order[lo:hi]
                w = np.abs((pairs[None, :, 0] - mx[js, None]) * (pairs[None, :, 1] - my[js, None]))
                out[js] += sign * (cnt[at[js] - p0] * w).sum(1)
            run += np.bincount(code[p0:p0 + block], minlength=K)
            lo = hi
    return out


Exact._abs_c = _abs_c_method


def _levels(mf):
    return np.where(mf <= 1.0, 1.0, np.frexp(mf - 1.0)[1] + 1.0)


def _q_bound(f, q, a):
    lu = _levels(f.mf) * U
    return C_BOUND * (lu * q + lu * a * np.sqrt(f.mf * q) + f.mf * (lu * a) ** 2)


def _c_bound(f):
    lu = _levels(f.mf) * U
    return C_BOUND * (lu * f.abs_c + lu * (f.ax * np.sqrt(f.mf * f.qy) + f.ay * np.sqrt(f.mf * f.qx)) + f.mf * (lu * f.ax) * (lu * f.ay))


def values(op, f):
    """(want, bound, null) per frame of f: moments_reference.Exact.value — its propagation formula by formula — over arrays"""
    m = f.mf
    null = np.zeros(len(m), bool)
    with np.errstate(all="ignore"):
        if op in UNI or op in ("covar_pop", "covar_samp"):
            d = m if op.endswith("pop") else m - 1.0
            null = d == 0.0
            if op in UNI:
                v, b = f.qy / d, _q_bound(f, f.qy, f.ay) / d
                if op.startswith("var"):
                    return v, b + 2 * U * np.abs(v), null
                s = np.sqrt(v)
                return s, np.where(v == 0.0, 0.0, 1.01 * s * (b / v) / 2 + 3 * U * s), null
            v = f.c / d
            return v, _c_bound(f) / d + 2 * U * np.abs(v), null
        null = (f.qx == 0.0) | ((f.qy == 0.0) if op == "corr" else False)
        rx = _q_bound(f, f.qx, f.ax) / f.qx
        if op == "corr":
            ry = _q_bound(f, f.qy, f.ay) / f.qy
            sxy = np.sqrt(f.qx) * np.sqrt(f.qy)
            v = f.c / sxy
            return v, _c_bound(f) / sxy + 1.01 * np.abs(v) * (rx + ry) / 2 + 6 * U, null
        slope = f.c / f.qx
        eslope = _c_bound(f) / f.qx + 1.01 * np.abs(slope) * rx + 2 * U * np.abs(slope)
        if op == "regr_slope":
            return slope, eslope, null
        return f.intercept, 1.01 * eslope * np.abs(f.mux) + 2 * m * U * (f.ay + np.abs(slope) * f.ax) + 4 * U * (np.abs(f.muy) + np.abs(slope * f.mux)), null


def check_column(op, got, f, what=None):
    """Assert a computed column against the definition of every frame of f within its bound; NULL where SQL has it, by bits.  Returns
    the worst error / bound."""
    want, bound, null = values(op, f)
    got = np.ascontiguousarray(got, np.float64)
    assert (got.view(np.uint64)[null] == NULL_BITS).all(), (what, op, "NULL")
    live = ~null
    err = np.abs(got[live] - want[live])
    bad = ~(np.isfinite(got[live]) & (err <= bound[live]))
    assert not bad.any(), (what, op, np.nonzero(live)[0][bad][:5], got[live][bad][:5], want[live][bad][:5], err[bad][:5], bound[live][bad][:5])
    with np.errstate(all="ignore"):
        ratio = np.where(bound[live] > 0, err / bound[live], 0.0)
    return float(ratio.max()) if len(ratio) else 0.0


def check(op, got, fe, what=None):
    """Assert one computed value against a FrameExact within its bound (moments_reference.check); returns error / bound."""
    return mref.check(op, got, None, None, what, exact=fe)


# ---- the pinned fold ------------------------------------------------------------------------------------------------------------------
def merge(a, b):
    """merge(a, b), a's positions before b's; a state is (n, Sy, Qy, Sx, Qx, C), the empty one has n = 0"""
    if a[0] == 0:
        return b
    if b[0] == 0:
        return a
    na, nb = float(a[0]), float(b[0])
    w = (na * nb) / float(a[0] + b[0])
    dy = b[1] / nb - a[1] / na
    dx = b[3] / nb - a[3] / na
    return (a[0] + b[0], a[1] + b[1], (a[2] + b[2]) + (dy * dy) * w, a[3] + b[3], (a[4] + b[4]) + (dx * dx) * w, (a[5] + b[5]) + (dx * dy) * w)


EMPTY = (0, 0.0, 0.0, 0.0, 0.0, 0.0)


class Tree:
    """The tree over the sorted columns y, x (x = None: y again): node k = merge(node 2k, node 2k + 1), the leaves at cap + position,
    padded to a power of two with leaves of 0.0 — a query never reads a node that holds one."""

    def __init__(self, y, x=None):
        y = [float(v) for v in y]
        x = y if x is None else [float(v) for v in x]
        n = len(y)
        cap = 1
        while cap < n:
            cap <<= 1
        self.cap = cap
        node = [None] * (2 * cap)
        for i in range(cap):
            node[cap + i] = (1, y[i], 0.0, x[i], 0.0, 0.0) if i < n else (1, 0.0, 0.0, 0.0, 0.0, 0.0)
        for k in range(cap - 1, 0, -1):
            node[k] = merge(node[2 * k], node[2 * k + 1])
        self.node = node

    def query(self, l, r):
        """the state of the positions [l, r]: the iterative query"""
        left = right = EMPTY
        p, q = self.cap + l, self.cap + r + 1
        while p < q:
            if p & 1:
                left = merge(left, self.node[p])
                p += 1
            if q & 1:
                q -= 1
                right = merge(self.node[q], right)
            p >>= 1
            q >>= 1
        return merge(left, right)


def finish(op, state):
    """THE FINISH over a frame's state; NAN (the NULL bits) where SQL has NULL.  An empty frame: state[0] == 0."""
    m, sy, qy, sx, qx, c = state
    if m == 0:
        return NAN
    M = float(m)
    if op in ("var_pop", "stddev_pop", "covar_pop"):
        v = (c if op == "covar_pop" else qy) / M
        return math.sqrt(v) if op == "stddev_pop" else v
    if op in ("var_samp", "stddev_samp", "covar_samp"):
        if m == 1:
            return NAN
        v = (c if op == "covar_samp" else qy) / (M - 1.0)
        return math.sqrt(v) if op == "stddev_samp" else v
    if op == "corr":
        if qx == 0.0 or qy == 0.0:
            return NAN
        t = c / (math.sqrt(qx) * math.sqrt(qy))
        return 1.0 if t > 1.0 else -1.0 if t < -1.0 else t
    if qx == 0.0:
        return NAN
    b = c / qx
    return b if op == "regr_slope" else sy / M - b * (sx / M)


def textbook_q(y):
    """sum y^2 - (sum y)^2 / m in doubles, left to right: the formula DESIGN.md rules out"""
    s = s2 = 0.0
    for v in y:
        v = float(v)
        s += v
        s2 += v * v
    return s2 - (s * s) / float(len(y))


def rows_frames(n, starts, ends, lo, hi):
    """the ROWS frame [l, r] of every position (l > r: empty) inside its partition [starts[j], ends[j]]; lo / hi None: unbounded"""
    pos = np.arange(n, dtype=np.int64)
    l = starts if lo is None else np.maximum(pos + lo, starts)
    r = ends if hi is None else np.minimum(pos + hi, ends)
    return np.asarray(l, np.int64), np.asarray(r, np.int64)


def partition_ends(part):
    """(first position, last position) of every position's partition; part: the sorted partition column"""
    n = len(part)
    pos = np.arange(n, dtype=np.int64)
    head = np.ones(n, bool)
    head[1:] = part[1:] != part[:-1]
    starts = np.maximum.accumulate(np.where(head, pos, 0)) if n else pos
    heads = np.nonzero(head)[0]
    ends = (np.append(heads[1:], n) - 1)[np.cumsum(head) - 1] if n else pos
    return starts, ends
