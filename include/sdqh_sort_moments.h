/* sdqh_sort_moments.h — the HIP library's eleventh ordering extension: the second-moment aggregates per group — VAR_POP / VAR_SAMP,
 * STDDEV_POP / STDDEV_SAMP, COVAR_POP / COVAR_SAMP, CORR, REGR_SLOPE and REGR_INTERCEPT over the ordered entries of a table
 * re-grouped at several nested levels of one key list, behind one sort.
 *
 * Like its ten siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * takes moments on the device, one without them leaves it to the caller (the binding: abi.GROUP_MOMENTS_EXPORTS,
 * Library.has_group_moments).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection, the order of the rows, derived terms, the ranks-column check, `levels`, the output layout (levels from the highest
 * asked for down, sorted order inside a level, the representative's row columns, out_level_rows), the count-only call,
 * SDQH_ERR_OVERFLOW with the needed count, SDQH_ERR_INVALID before SDQH_ERR_UNSUPPORTED, "nothing written on an error, *out_n
 * included" and the empty selection's 0 rows are sdqh_table_grouping_sets', declared in sdqh_sort_groups.h, word for word.
 *
 * Not here: moments over window frames (they are sdqh_sort_wmoments.h's, the thirteenth extension), third and fourth moments,
 * weighted moments, text measures, more than SDQH_GM_MAX_AGGS aggregates per call, and the multi-GPU runner. */
#ifndef SDQH_SORT_MOMENTS_H
#define SDQH_SORT_MOMENTS_H

#include "sdqh_sort_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_GM_MAX_AGGS 4
#define SDQH_GM_VAR_POP        0
#define SDQH_GM_VAR_SAMP       1
#define SDQH_GM_STDDEV_POP     2
#define SDQH_GM_STDDEV_SAMP    3
#define SDQH_GM_COVAR_POP      4
#define SDQH_GM_COVAR_SAMP     5
#define SDQH_GM_CORR           6
#define SDQH_GM_REGR_SLOPE     7
#define SDQH_GM_REGR_INTERCEPT 8
/* 32 bytes; op: SDQH_GM_*; kind / index / is_f64: the first measure, Y — the dependent one, as in SQL's REGR_SLOPE(Y, X);
 * kind2 / index2 / is_f64_2: the second, X */
typedef struct sdqh_moment_agg { int32_t op, kind, index, is_f64, kind2, index2, is_f64_2, _pad; } sdqh_moment_agg;

/* MEASURES.  A measure is what sdqh_sort_frames.h calls one, with its validity rules.  VAR_* and STDDEV_* read the first measure
 * only and ignore the second (it is not checked); the other ops read both.  An integer measure is converted to double by one
 * conversion and is a double from then on.  Every result is a double; out_aggs[a * capacity + j] holds its 64 bits.
 *
 * DEFINITION.  For a group of m rows, their doubles x_i, y_i, in exact arithmetic: mux = sum x / m, Qx = sum (x_i - mux)^2, Qy
 * likewise, C = sum (x_i - mux)(y_i - muy).  With Q the first measure's:
 *   VAR_POP = Q / m            VAR_SAMP = Q / (m - 1)          STDDEV_* = sqrt of that variance
 *   COVAR_POP = C / m          COVAR_SAMP = C / (m - 1)
 *   CORR = C / (sqrt(Qx) * sqrt(Qy)), clamped to [-1, 1]       (two square roots: sqrt(Qx * Qy) overflows at Q ~ 1e155)
 *   REGR_SLOPE = C / Qx        REGR_INTERCEPT = muy - REGR_SLOPE * mux
 *
 * HOW IT IS COMPUTED: two passes over the group's rows, per level asked for.  With r the group's representative (its first sorted
 * row) every row is staged as s_i = x_i - x_r, one IEEE subtraction.  Pass 1 sums the s_i (S^) and forms the shifted mean
 * mu^ = S^ / (double)m, one division.  Every row is then centred, d_i = s_i - mu^, and pass 2 sums d_i * d_i (Q^) and dx_i * dy_i
 * (C^), each term one rounding.  Both sums are sums in the sense of sdqh_sort_groups.h: IEEE additions of exactly the group's rows
 * in an association fixed for a given input, geometry and `levels`, no atomics (two calls give the same bits), nothing added and
 * later subtracted, no row of another group enters, |sum^ - sum| <= g(m) * sum|v|.  A coarser level's Q is taken over the rows
 * again, not folded from a finer level's (the means differ).  sum x^2 - (sum x)^2 / m and merged (n, mean, M2) states are not used.
 *
 * ACCURACY.  u = 2^-53, A = sum|x_i| / m:
 *   |Q^ - Q| <= 2 * [(m + 2 sqrt m + 6) u + max(m (m u A)^2 / Q, 4 m^3 u^2)] * Q
 *   |C^ - C| <= 2 * [(m + 2 sqrt m + 6) u * sum|dx_i dy_i| + m (m u Ax)(m u Ay) + 4 m^3 u^2 sqrt(Qx Qy)]
 * (pass 1's mean is off by at most about m u A — g(m) and one division —, which adds m delta^2 to Q; each d_i and d_i^2 costs one
 * rounding, the non-negative sum g(m); the shift by a group member at most 2 u (1 + sqrt m); the factor 2 covers the second-order
 * terms dropped.)
 *
 * THE FINISH, in this order, every step one IEEE operation, M = (double)m:
 *   VAR_POP    Q^ / M                                COVAR_POP    C^ / M
 *   VAR_SAMP   Q^ / (M - 1.0)                        COVAR_SAMP   C^ / (M - 1.0)
 *   STDDEV_*   sqrt(the variance above)
 *   CORR       t = C^ / (sqrt(Qx^) * sqrt(Qy^)); t > 1.0 gives 1.0, t < -1.0 gives -1.0
 *   REGR_SLOPE b = C^ / Qx^
 *   REGR_INTERCEPT  (y_r + Sy^ / M) - b * (x_r + Sx^ / M)
 *
 * EXACT CASES.  A group whose x are all the same double has Qx = +0.0 (every s_i is +0.0).  m = 1: VAR_POP = STDDEV_POP =
 * COVAR_POP = +0.0, and *_SAMP is the quiet NaN 0x7FF8000000000000, standing for SQL's NULL.  CORR is that NaN when Qx^ = 0 or
 * Qy^ = 0, REGR_SLOPE and REGR_INTERCEPT when Qx^ = 0.  A group that holds a NaN or an infinity gives NaN or +-inf as IEEE
 * arithmetic falls; the groups beside it are unaffected.  COVAR_* and CORR give the same bits with the measures swapped, and
 * COVAR_POP(x, x) the bits of VAR_POP(x).
 *
 * ERRORS.  An op outside SDQH_GM_*, a measure the table lacks or is_f64 on SDQH_SORT_KEY / SDQH_SORT_HITS (either measure of an op
 * that reads it), naggs < 1 or > SDQH_GM_MAX_AGGS, aggs NULL: SDQH_ERR_INVALID, with those of sdqh_table_grouping_sets.  out_aggs
 * NULL: rows only. */
int sdqh_table_group_moments(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits,
                             int nterms, const sdqh_sort_term* terms, uint32_t levels,
                             int naggs, const sdqh_moment_agg* aggs, int64_t limit, int64_t capacity,
                             int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                             int64_t* out_aggs      /* naggs x capacity, 64 bits each; may be NULL */,
                             int64_t* out_level_rows /* SDQH_SORT_MAX_KEYS + 1 counts; may be NULL */,
                             int64_t* out_n);
/* What the tests size their cases from: the tile both passes share with the window passes. */
int sdqh_group_moments_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
