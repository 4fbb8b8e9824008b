/* sdqh_sort_wmoments.h — the HIP library's thirteenth ordering extension: the second-moment aggregates over window frames —
 * VAR_POP / VAR_SAMP, STDDEV_POP / STDDEV_SAMP, COVAR_POP / COVAR_SAMP, CORR, REGR_SLOPE and REGR_INTERCEPT (measures) OVER
 * (PARTITION BY ... ORDER BY ... ROWS | RANGE | GROUPS BETWEEN lo AND hi), the frame's unit chosen per column: a moving standard
 * deviation, a rolling correlation, a rolling regression slope behind one sort.
 *
 * Like its twelve siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * folds such frames on the device, one without them leaves it to the caller (the binding: abi.WINDOW_MOMENTS_EXPORTS,
 * Library.has_window_moments).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection, the order of the rows, partitions, ties, derived terms, the base frame F = [l, r] per unit (VALUE's demands on the
 * terms included), unbounded sides, limit / capacity / the count-only call / SDQH_ERR_OVERFLOW, the bounds check of a term's ranks
 * column, the order of the errors (argument checks before SDQH_ERR_UNSUPPORTED) and the wait for the stream are exactly those of
 * sdqh_table_window_exclude with exclude = SDQH_WEX_NO_OTHERS, declared in sdqh_sort_exclude.h.  Frames look past `limit`.
 *
 * Not here: EXCLUDE clauses, third and fourth moments, weights, text measures, a row-by-row two-pass for narrow ROWS frames, more
 * than SDQH_WM_MAX_COLS columns per call, and the multi-GPU runner. */
#ifndef SDQH_SORT_WMOMENTS_H
#define SDQH_SORT_WMOMENTS_H

#include "sdqh_sort_exclude.h"
#include "sdqh_sort_moments.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WM_MAX_COLS 4
/* 56 bytes; op: SDQH_GM_* (sdqh_sort_moments.h); kind / index / is_f64: the first measure, Y; kind2 / index2 / is_f64_2: the
 * second, X (ignored, unchecked, by VAR_* and STDDEV_*); unit: SDQH_WRANGE_VALUE / SDQH_WRANGE_GROUPS / SDQH_WEX_ROWS; flags:
 * SDQH_WRANGE_LO_UNBOUNDED | SDQH_WRANGE_HI_UNBOUNDED; lo / hi as sdqh_window_exclude's */
typedef struct sdqh_window_moment { int32_t op, kind, index, is_f64, kind2, index2, is_f64_2, unit, flags, _pad; int64_t lo, hi; } sdqh_window_moment;

/* The first min(limit, n) of the n selected rows in sorted order, and beside row j the value of every column over row j's frame:
 * out_cols[c * capacity + j], the 64 bits of a double (out_cols may be NULL: rows only).
 *
 * MEASURES AND RESULTS.  A measure is what sdqh_sort_frames.h calls one.  An integer measure is converted to double once, at the
 * leaf, and is a double from then on.  Every result is a double.  An empty frame gives the quiet NaN 0x7FF8000000000000, standing
 * for SQL's NULL; there is no `empty` field.  The definition of the nine ops is sdqh_sort_moments.h's DEFINITION over the rows of
 * the frame.
 *
 * THE FOLD, operation by operation (the unit is built without FMA contraction; every step below is one IEEE operation).  A STATE
 * over a run of positions is (n, S, Q) per measure plus C per measure pair.  A leaf is (1, x, +0.0, +0.0).  The empty state has
 * n = 0 and merging with it returns the other state unchanged.  merge(a, b), a's positions before b's:
 *
 *     delta = S_b / (double)n_b - S_a / (double)n_a          w = ((double)n_a * (double)n_b) / (double)(n_a + n_b)
 *     S = S_a + S_b        Q = (Q_a + Q_b) + (delta * delta) * w        C = (C_a + C_b) + (delta_x * delta_y) * w
 *
 * A node of the tree is merge(left child, right child) over an aligned block of 2^h positions of the sorted order.  A frame's
 * state is the tree's iterative query over [l, r]: left = merge(left, node) going up from l, right = merge(node, right) going down
 * from r + 1, then merge(left, right).  The association is a function of l and r alone — not of the unit, the tree's capacity, the
 * tile or the call: two rows with the same frame, two calls, and one frame spelled in ROWS, VALUE or GROUPS give the same bits.  No
 * atomics, nothing added and later subtracted, no row outside the frame enters.
 *
 * THE FINISH is sdqh_sort_moments.h's THE FINISH with M = (double)(r - l + 1), the frame's Q^ and C^, and
 * REGR_INTERCEPT = Sy^ / M - b * (Sx^ / M).  Kept from there: m = 1 gives +0.0 for VAR_POP / STDDEV_POP / COVAR_POP and the NULL
 * NaN for *_SAMP; CORR is that NaN when Qx^ = 0 or Qy^ = 0 exactly, REGR_SLOPE and REGR_INTERCEPT when Qx^ = 0; CORR's clamp; COVAR_*
 * and CORR give the same bits with the measures swapped, and COVAR_POP(x, x) the bits of VAR_POP(x).  The device's double
 * division and square root are correctly rounded: STDDEV_* and CORR match a restatement with a correctly rounded sqrt bit for bit.
 *
 * WHAT DOES NOT CARRY OVER.  There is no shift by a representative: a partition's head may lie far from a frame's values and would
 * destroy them.  "Data far from zero loses nothing" becomes the bound below.  A frame of equal non-integer doubles may give a tiny
 * Q^ > 0 (0.1 three times: S = fl(0.3), S / 3 != 0.1), so the constant-column NULL of CORR / REGR is guaranteed only where the
 * sums are exact: m = 1, and equal integer-valued doubles with m * |x| < 2^53.  A NaN or an infinity poisons exactly the frames
 * that contain its position (as NaN or +-inf, as IEEE arithmetic falls).
 *
 * ACCURACY.  u = 2^-53, m the frame's rows, A = sum|x_i| / m over the frame, L = ceil(log2 m) + 1 (L = 1 for m = 1):
 *
 *     |Q^ - Q| <= 8 * [ L u Q  +  L u A sqrt(m Q)  +  m (L u A)^2 ]
 *     |C^ - C| <= 8 * [ L u sum|dx_i dy_i|  +  L u (Ax sqrt(m Qy) + Ay sqrt(m Qx))  +  m (L u Ax)(L u Ay) ]
 *
 * The middle term is the price of merged states: a merge sees its halves' means, each off by about L u A, so the relative error
 * grows like (A / sigma) u L, not like u.  DESIGN.md (section 4o) derives the constant.
 *
 * SCRATCH, from the context's pool, beside sdqh_table_window_exclude's partition arrays and keys: (2 per distinct measure + 1 per
 * distinct unordered pair of different measures) * 2 * cap doubles, cap the power of two at or above max(n, tile_rows).
 *
 * ERRORS.  An op outside SDQH_GM_*, an unknown unit or flag bit, _pad != 0, both sides bounded with lo > hi (sdqh_window_exclude's
 * rule), ncols < 1 or > SDQH_WM_MAX_COLS, cols NULL, a measure the table lacks or is_f64 on SDQH_SORT_KEY / SDQH_SORT_HITS (either
 * measure of an op that reads it): SDQH_ERR_INVALID with the argument errors of sdqh_table_window_exclude, nothing written, *out_n
 * included. */
int sdqh_table_window_moments(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                              int ncols, const sdqh_window_moment* cols, int64_t limit, int64_t capacity,
                              int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                              int64_t* out_cols /* ncols x capacity, 64 bits each */, int64_t* out_n);
/* What the tests size their cases from: the tile every window pass shares. */
int sdqh_window_moments_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
