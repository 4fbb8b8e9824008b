"""The pinned fold of include/sdqh_sort_wmoments.h once more, as whole-array numpy: the tree built level by level, the iterative
query over an array of frames [l, r] at once, and THE FINISH of all nine ops as array code.  One IEEE operation per numpy elementwise
operation (numpy contracts nothing into an FMA; np.sqrt and the division are correctly rounded), in the header's order, so the bits are
those of window_moments_reference.Tree / finish — test_window_moments_numpy_cpu holds the two against each other — at a cost that lets
a test compare every row at 262 657 rows: 0.04 s for the tree, about a second for a frame of every row.

Nothing is imported from the product, nor from window_moments_reference.

A state is (n, Sy, Qy, Sx, Qx, C): n an int64 array (0: the empty state), the others float64 arrays, one entry per frame."""
import numpy as np

OPS = ("var_pop", "var_samp", "stddev_pop", "stddev_samp", "covar_pop", "covar_samp", "corr", "regr_slope", "regr_intercept")
UNI, BI = OPS[:4], OPS[4:]
NULL_BITS = 0x7FF8000000000000
NAN = np.array([NULL_BITS], np.uint64).view(np.float64)[0]
COMPONENTS = ("sy", "qy", "sx", "qx", "c")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def leaf(raw, is_f64):
    """a measure's leaves: the stored 64 bits as the doubles they are, or the integers they are converted to double — once, here"""
    raw = np.ascontiguousarray(raw)
    if raw.dtype == np.float64:
        return raw
    return raw.view(np.float64) if is_f64 else raw.astype(np.int64).astype(np.float64)


def merge(a, b):
    """merge(a, b) per entry, a's positions before b's; merging with the empty state returns the other one unchanged"""
    both = (a[0] > 0) & (b[0] > 0)
    na, nb = np.where(both, a[0], 1).astype(np.float64), np.where(both, b[0], 1).astype(np.float64)      # (an empty side: any divisor, the lane is not taken)
    with np.errstate(all="ignore"):
        w = (na * nb) / (na + nb)                                          # (n_a + n_b is exact in a double either way)
        dy = b[1] / nb - a[1] / na
        dx = b[3] / nb - a[3] / na
        merged = (a[0] + b[0], a[1] + b[1], (a[2] + b[2]) + (dy * dy) * w, a[3] + b[3], (a[4] + b[4]) + (dx * dx) * w, (a[5] + b[5]) + (dx * dy) * w)
    only_a = a[0] > 0
    return tuple(np.where(both, m, np.where(only_a, x, y)) for m, x, y in zip(merged, a, b))


def empty(m):
    return (np.zeros(m, np.int64),) + tuple(np.zeros(m) for _ in COMPONENTS)


class Tree:
    """The tree over the sorted columns y, x (x = None: y again, and then C has the bits of Qy): node k = merge(node 2k, node 2k + 1),
    the leaves at cap + position, padded to a power of two with leaves of 0.0.  A node of height h holds 2^h rows: its n is not stored."""

    def __init__(self, y, x=None):
        y = np.ascontiguousarray(y, np.float64)
        x = y if x is None else np.ascontiguousarray(x, np.float64)
        n = len(y)
        cap = 1
        while cap < n:
            cap <<= 1
        self.n, self.cap = n, cap
        s = {k: np.zeros(2 * cap) for k in COMPONENTS}
        s["sy"][cap:cap + n], s["sx"][cap:cap + n] = y, x
        cnt, h = cap >> 1, 1
        with np.errstate(all="ignore"):
            while cnt >= 1:
                a, b, o = slice(2 * cnt, 4 * cnt, 2), slice(2 * cnt + 1, 4 * cnt, 2), slice(cnt, 2 * cnt)
                nh = np.float64(1 << (h - 1))                              # a child's rows
                w = (nh * nh) / (nh + nh)
                dy = s["sy"][b] / nh - s["sy"][a] / nh
                dx = s["sx"][b] / nh - s["sx"][a] / nh
                s["qy"][o] = (s["qy"][a] + s["qy"][b]) + (dy * dy) * w
                s["qx"][o] = (s["qx"][a] + s["qx"][b]) + (dx * dx) * w
                s["c"][o] = (s["c"][a] + s["c"][b]) + (dx * dy) * w
                s["sy"][o] = s["sy"][a] + s["sy"][b]
                s["sx"][o] = s["sx"][a] + s["sx"][b]
                cnt >>= 1
                h += 1
        self.s = s

    def _nodes(self, take, at, h):
        idx = np.where(take, at, 0)
        return (np.where(take, np.int64(1) << h, 0),) + tuple(np.where(take, self.s[k][idx], 0.0) for k in COMPONENTS)

    def query(self, l, r):
        """the states of the frames [l[j], r[j]] — l[j] > r[j]: the empty state —: the iterative query, every distinct frame once"""
        l, r = np.asarray(l, np.int64), np.asarray(r, np.int64)
        if len(l) == 0:
            return empty(0)
        none = l > r
        assert (none | ((l >= 0) & (r < self.n))).all()
        code = np.where(none, np.int64(0), l * np.int64(self.n + 1) + r + 1)
        uniq, inv = np.unique(code, return_inverse=True)
        inv = inv.reshape(-1)
        ul, ur = np.where(uniq == 0, 1, (uniq - 1) // (self.n + 1)), np.where(uniq == 0, 0, (uniq - 1) % (self.n + 1))
        left, right = empty(len(uniq)), empty(len(uniq))
        p, q = self.cap + ul, self.cap + ur + 1
        h = 0
        while (p < q).any():
            live = p < q
            tl = live & (p & 1 == 1)                                       # p & 1: left = merge(left, node p), p += 1
            left = merge(left, self._nodes(tl, p, h))
            p = p + tl
            tr = live & (q & 1 == 1)                                       # q & 1: q -= 1, right = merge(node q, right)
            q = q - tr
            right = merge(self._nodes(tr, q, h), right)
            p, q = np.where(live, p >> 1, p), np.where(live, q >> 1, q)
            h += 1
        return tuple(c[inv] for c in merge(left, right))


def swapped(state):
    """the same frames with the measures' roles exchanged"""
    n, sy, qy, sx, qx, c = state
    return n, sx, qx, sy, qy, c


def finish(op, state):
    """THE FINISH per entry; the NULL bits on an empty frame, on a single row under *_SAMP, where Qx^ (CORR: or Qy^) is 0"""
    n, sy, qy, sx, qx, c = state
    m = n.astype(np.float64)
    with np.errstate(all="ignore"):
        if op in ("var_pop", "stddev_pop", "covar_pop"):
            v = (c if op == "covar_pop" else qy) / m
            v = np.sqrt(v) if op == "stddev_pop" else v
            null = n == 0
        elif op in ("var_samp", "stddev_samp", "covar_samp"):
            v = (c if op == "covar_samp" else qy) / (m - 1.0)
            v = np.sqrt(v) if op == "stddev_samp" else v
            null = n <= 1
        elif op == "corr":
            t = c / (np.sqrt(qx) * np.sqrt(qy))
            v = np.where(t > 1.0, 1.0, np.where(t < -1.0, -1.0, t))
            null = (n == 0) | (qx == 0.0) | (qy == 0.0)
        else:
            b = c / qx
            v = b if op == "regr_slope" else sy / m - b * (sx / m)
            null = (n == 0) | (qx == 0.0)
    return np.where(null, NAN, v)
