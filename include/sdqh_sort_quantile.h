/* sdqh_sort_quantile.h — the HIP library's seventh ordering extension: the window functions that need the SIZE of the row's partition
 * — NTILE, PERCENT_RANK, CUME_DIST, NTH_VALUE from either end, PERCENTILE_DISC and PERCENTILE_CONT (the median among them) OVER
 * (PARTITION BY ... ORDER BY ...) — beside the ordered entries of a table, every row or the first per_limit rows of every partition
 * (per_limit = 1: one row per group, the GROUP BY form of a percentile).
 *
 * Like its six siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * computes them on the device, one without them leaves it to the caller (the binding: abi.WINDOW_QUANTILE_EXPORTS,
 * Library.has_window_quantile).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection, the order of the rows, partitions, ties, derived terms, measures (kind / index / is_f64, an underived column), outputs,
 * limit / capacity / the count-only call / SDQH_ERR_OVERFLOW, the bounds check of a term's ranks column and its error,
 * SDQH_ERR_UNSUPPORTED for a bitmap-only table or a compile-only context (argument checks first) and the wait for the stream are
 * exactly those of sdqh_table_window_slide, declared in sdqh_sort_slide.h.  per_limit is sdqh_table_window's with kind ROW_NUMBER
 * (sdqh_sort_window.h): only the rows whose row number inside their partition is <= per_limit are returned (SDQH_SORT_ALL: every
 * row), *out_n and the second wait for the kept count are as there, and per_limit >= n skips the rank, scan and place steps.
 *
 * Not here: weighted percentiles, several p of one measure in one pass (ask for several columns), MODE, text measures, and the
 * multi-GPU runner. */
#ifndef SDQH_SORT_QUANTILE_H
#define SDQH_SORT_QUANTILE_H

#include "sdqh_sort_slide.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WQ_NTILE           0   /* arg = b >= 1            -> int64                     */
#define SDQH_WQ_PERCENT_RANK    1   /*                         -> double                    */
#define SDQH_WQ_CUME_DIST       2   /*                         -> double                    */
#define SDQH_WQ_NTH             3   /* measure, arg = k != 0   -> the measure's 64 bits     */
#define SDQH_WQ_PERCENTILE_DISC 4   /* measure, p in [0, 1]    -> the measure's 64 bits     */
#define SDQH_WQ_PERCENTILE_CONT 5   /* measure, p in [0, 1]    -> double                    */
#define SDQH_WQUANT_MAX_COLS    4
typedef struct sdqh_window_quantile { int32_t fn, kind, index, is_f64; int64_t arg; double p; int64_t empty; } sdqh_window_quantile;  /* 40 bytes; kind/index/is_f64: the measure */

/* The returned rows in sorted order — of the n selected rows those whose row number inside their partition is <= per_limit, the
 * first min(limit, kept) of them — and beside the i-th returned row the value of every column: out_cols[c * capacity + i], 64 bits
 * each (out_cols may be NULL: rows only).
 *
 * For sorted row j let its partition occupy the sorted positions [s, e]: m = e - s + 1, i = j - s, and [f, l] the offsets from s of
 * the first and last row of j's tie run (a tie: all nterms keys equal, as everywhere).  Every function looks at the WHOLE partition,
 * whether or not its rows are returned: limit and per_limit cut the result off afterwards.
 *
 *   NTILE(b)          q = m / b, r = m % b (integers): i / (q + 1) + 1 if i < r * (q + 1), else r + (i - r * (q + 1)) / q + 1.
 *                     Positional: ties play no part.  b > m gives i + 1.  Any b in [1, INT64_MAX] is valid and overflows nowhere.
 *   PERCENT_RANK      0.0 when m = 1, else (double)f / (double)(m - 1): one correctly rounded IEEE division.
 *   CUME_DIST         (double)(l + 1) / (double)m.
 *   NTH(measure, k)   the measure's 64 bits, copied (NaN payloads, -0.0): k >= 1 from position s + k - 1, k <= -1 from position
 *                     e + k + 1; |k| > m gives the 64 bits of `empty`.  INT64_MIN is handled without overflow.
 *   PERCENTILE_DISC(measure, p)
 *                     the measure's 64 bits at position s + max(ceil(p * (double)m) - 1, 0), the product one IEEE multiplication.
 *                     Positional; with the measure equal to the ORDER BY column this is SQL's PERCENTILE_DISC(p) WITHIN GROUP.
 *   PERCENTILE_CONT(measure, p)
 *                     x = p * (double)(m - 1), lo = floor(x), hi = ceil(x); a and b the measure at s + lo and s + hi as doubles (an
 *                     int64 measure by one round-to-nearest conversion).  a if lo = hi, else a + (b - a) * (x - lo): four IEEE
 *                     operations in exactly that order, no FMA.  A NaN result is some NaN: its payload is unspecified.
 *
 * ncols < 1 or > SDQH_WQUANT_MAX_COLS, an unknown fn, b < 1, k = 0, p < 0, p > 1 or NaN, per_limit < 1, and the measure and
 * argument errors of sdqh_table_window_agg: SDQH_ERR_INVALID, nothing written, *out_n included.  arg is read by NTILE and NTH, p by
 * the percentiles, the measure by NTH and the percentiles, empty by NTH; the others ignore them. */
int sdqh_table_window_quantile(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                               int ncols, const sdqh_window_quantile* cols, int64_t per_limit, int64_t limit, int64_t capacity,
                               int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                               int64_t* out_cols /* ncols x capacity, 64 bits each; may be NULL */, int64_t* out_n);
/* What the tests size their cases from: tile_rows — the tile, the one the window, frame and slide passes share. */
int sdqh_window_quantile_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
