/* sdqh_sort_frames.h — the HIP library's fourth ordering extension: aggregates over window frames of the ordered entries of a
 * table — SUM / COUNT / MIN / MAX (measure) OVER (PARTITION BY ... ORDER BY ... <frame>): running totals, a row's share of its
 * group's total, the group's size beside every row, running extrema.
 *
 * Like sdqh_sort.h, sdqh_sort_terms.h and sdqh_sort_window.h it is not part of the boundary every implementation provides
 * (sdqh.h): a library that has these symbols aggregates on the device, one without them leaves the aggregation to the caller (the
 * binding: abi.WINDOW_AGG_EXPORTS, Library.has_window_agg).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection (min_hits, owner rows only), the order of the rows, PARTITIONS (maximal runs of ordered rows whose first npartition
 * keys are equal), TIES (all nterms keys equal; what is left of a tie is build-row order) and derived terms are exactly those of
 * sdqh_table_window, declared in sdqh_sort_window.h.  Every selected row is kept: there is no per_limit. */
#ifndef SDQH_SORT_FRAMES_H
#define SDQH_SORT_FRAMES_H

#include "sdqh_sort_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WAGG_SUM 0
#define SDQH_WAGG_COUNT 1
#define SDQH_WAGG_MIN 2
#define SDQH_WAGG_MAX 3
#define SDQH_FRAME_ROWS      0   /* partition start .. this row                                   */
#define SDQH_FRAME_RANGE     1   /* partition start .. the last row tied with this one (SQL default) */
#define SDQH_FRAME_PARTITION 2   /* the whole partition                                            */
#define SDQH_WAGG_MAX_AGGS 4
typedef struct sdqh_window_agg { int32_t op, frame, kind, index, is_f64, _pad; } sdqh_window_agg;   /* kind/index/is_f64: the measure, as sdqh_sort_key names a column */

/* The first min(limit, n) of the n selected rows in sorted order, and beside row j the value of every aggregate over row j's frame:
 * out_aggs[a * capacity + j] is aggregate a of row j, 64 bits each (out_aggs may be NULL: rows only).
 *
 * A MEASURE is an underived column: SDQH_SORT_KEY, an integer or double (is_f64) SDQH_SORT_PAYLOAD, SDQH_SORT_VALUE i, or
 * SDQH_SORT_HITS.  SDQH_WAGG_COUNT ignores its measure: the number of rows in the frame, as int64.
 *   Integer measures: results are int64.  SUM wraps around in two's complement, so it is exact in any association; MIN / MAX are signed.
 *   Double measures: results are the double's bits in the int64 slot.  MIN / MAX follow the total order and the NaN rule of
 *     sdqh_extrema.h: -0.0 is below +0.0, NaNs are skipped, a frame with no non-NaN value gives the quiet NaN.  SUM is IEEE addition
 *     of exactly the frame's rows, in an association this header leaves unspecified but which is fixed for a given input and
 *     geometry (no atomics: two calls give the same bits).  Nothing is ever added and later subtracted, and rows of other
 *     partitions never enter a sum.  So for a frame of m finite rows |result - exact| <= g * sum|v| with g = (m-1)u / (1 - (m-1)u),
 *     u = 2^-53, and sums of integer-valued doubles that stay below 2^53 in magnitude are exact.
 * For every op, bit for bit: all rows of a tie run share one RANGE value; all rows of a partition share one PARTITION value; the
 * ROWS value at the last row of a tie run is that run's RANGE value; the ROWS value at the last row of a partition is the
 * partition's PARTITION value.
 *
 * The bounds check of a term's ranks column and its error, the limit of SDQH_SORT_MAX_KEYS terms, SDQH_ERR_UNSUPPORTED for a
 * bitmap-only table or a compile-only context, and the wait for the stream are those of sdqh_table_window.  Outputs and capacity as
 * sdqh_table_sorted: all of out_keys / out_payload / out_values / out_hits / out_aggs NULL: count only (*out_n = min(limit, n), no
 * pass runs); min(limit, n) > capacity: SDQH_ERR_OVERFLOW, *out_n = the capacity needed, nothing written.
 * naggs < 1 or > SDQH_WAGG_MAX_AGGS, an unknown op or frame, a measure column the table lacks, is_f64 on SDQH_SORT_KEY or
 * SDQH_SORT_HITS, and the argument errors of sdqh_table_window: SDQH_ERR_INVALID, nothing written, *out_n included. */
int sdqh_table_window_agg(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                          int naggs, const sdqh_window_agg* aggs, int64_t limit, int64_t capacity,
                          int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                          int64_t* out_aggs /* naggs x capacity, 64 bits each */, int64_t* out_n);
/* What the tests size their cases from: the sorted positions one wave aggregates per step of the tile scan (a tile; a carry crosses
 * from one tile to the next, forwards for the values and backwards for the frame ends).  One form for every n. */
int sdqh_window_agg_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
