"""Exact second moments and the bounds of include/sdqh_sort_moments.h, restated for the tests of the group-moments extension: every
double is an exact fractions.Fraction, so Q, C and the means are the definition's, to the last bit.  Nothing here reads the product's
fold code.

The header bounds Q^ and C^.  What the ops make of them is bounded here by first-order propagation, written down once:
  a quotient Q^ / d (d exact):        the sum's bound / d, and one rounding
  a square root:                      half the relative error of its argument, and one rounding
  CORR = C / (sx * sy):               C's bound / (sx sy) + |corr| * (relQx + relQy) / 2, and four roundings
  REGR_SLOPE = C / Qx:                C's bound / Qx + |slope| * relQx, and one rounding
  REGR_INTERCEPT = muy - slope mux:   the slope's error * |mux|, each mean off by m u A (pass 1's bound and a division) and three roundings
Each relative term carries the factor 1.01 for the second order — the cases keep the relative bounds below 1e-3."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
NULL_BITS = 0x7FF8000000000000
OPS = ("var_pop", "var_samp", "stddev_pop", "stddev_samp", "covar_pop", "covar_samp", "corr", "regr_slope", "regr_intercept")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ulps(a, b):
    """the distance of two finite doubles of one sign in units in the last place"""
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


class Exact:
    """The definition over one group: y (and x) as sequences of finite doubles."""

    def __init__(self, y, x=None):
        self.m = m = len(y)
        fy = [Fraction(float(v)) for v in y]
        self.muy = sum(fy) / m
        self.dy = [v - self.muy for v in fy]
        self.qy = sum(d * d for d in self.dy)
        self.ay = float(sum(abs(v) for v in fy) / m)
        if x is not None:
            fx = [Fraction(float(v)) for v in x]
            self.mux = sum(fx) / m
            self.dx = [v - self.mux for v in fx]
            self.qx = sum(d * d for d in self.dx)
            self.c = sum(a * b for a, b in zip(self.dx, self.dy))
            self.ax = float(sum(abs(v) for v in fx) / m)
            self.abs_c = float(sum(abs(a * b) for a, b in zip(self.dx, self.dy)))

    def q_bound(self, q, a):
        """the header's |Q^ - Q|"""
        m, q = self.m, float(q)
        if q == 0.0:
            return 0.0
        return 2.0 * ((m + 2.0 * math.sqrt(m) + 6.0) * U + max(m * (m * U * a) ** 2 / q, 4.0 * m ** 3 * U * U)) * q

    def c_bound(self):
        """the header's |C^ - C|"""
        m = self.m
        return 2.0 * ((m + 2.0 * math.sqrt(m) + 6.0) * U * self.abs_c + m * (m * U * self.ax) * (m * U * self.ay) + 4.0 * m ** 3 * U * U * math.sqrt(float(self.qx) * float(self.qy)))

    def value(self, op):
        """(the op's exact value as a float — None where SQL has NULL —, the bound on |computed - exact|)"""
        m = self.m
        if op in ("var_pop", "var_samp", "stddev_pop", "stddev_samp"):
            d = m if op.endswith("pop") else m - 1
            if d == 0:
                return None, 0.0
            v, b = float(self.qy / d), self.q_bound(self.qy, self.ay) / d
            if op.startswith("var"):
                return v, b + 2 * U * abs(v)
            if v == 0.0:
                return 0.0, 0.0
            s = math.sqrt(self.qy / d)
            return s, 1.01 * s * (b / v) / 2 + 3 * U * s
        if op in ("covar_pop", "covar_samp"):
            d = m if op.endswith("pop") else m - 1
            if d == 0:
                return None, 0.0
            v = float(self.c / d)
            return v, self.c_bound() / d + 2 * U * abs(v)
        if self.qx == 0 or (op == "corr" and self.qy == 0):
            return None, 0.0
        rx = self.q_bound(self.qx, self.ax) / float(self.qx)
        if op == "corr":
            ry = self.q_bound(self.qy, self.ay) / float(self.qy)
            sxy = math.sqrt(self.qx) * math.sqrt(self.qy)
            v = float(self.c) / sxy
            return v, self.c_bound() / sxy + 1.01 * abs(v) * (rx + ry) / 2 + 6 * U
        slope = float(self.c / self.qx)
        eslope = self.c_bound() / float(self.qx) + 1.01 * abs(slope) * rx + 2 * U * abs(slope)
        if op == "regr_slope":
            return slope, eslope
        muy, mux = float(self.muy), float(self.mux)
        v = float(self.muy - self.c / self.qx * self.mux)
        return v, 1.01 * eslope * abs(mux) + 2 * m * U * (self.ay + abs(slope) * self.ax) + 4 * U * (abs(muy) + abs(slope * mux))


def check(op, got, y, x=None, what=None, exact=None):
    """Assert one computed value against the definition within its bound; returns error / bound (0 where the value is exact).  exact: the
    Exact of these y (and x), where a caller checks several ops of one group."""
    want, bound = (exact or Exact(y, x)).value(op)
    got = np.float64(got)
    if want is None:
        assert int(got.view(np.uint64)) == NULL_BITS, (what, op, got)
        return 0.0
    err = abs(float(got) - want)
    assert np.isfinite(got) and err <= bound, (what, op, float(got), want, err, bound)
    return err / bound if bound else 0.0


def naive_variance(x):
    """sum x^2 - (sum x)^2 / m over m, in doubles: the formula the header rules out"""
    x = np.asarray(x, np.float64)
    m = len(x)
    return float((np.add.reduce(x * x) - np.add.reduce(x) ** 2 / m) / m)
