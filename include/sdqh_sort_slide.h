/* sdqh_sort_slide.h — the HIP library's fifth ordering extension: aggregates and values over SLIDING window frames of the ordered
 * entries of a table — SUM / COUNT / MIN / MAX / FIRST_VALUE / LAST_VALUE (measure) OVER (PARTITION BY ... ORDER BY ... ROWS BETWEEN
 * lo AND hi): moving sums and extrema, "this row and the next two", LAG and LEAD.
 *
 * Like its four siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * slides on the device, one without them leaves it to the caller (the binding: abi.WINDOW_SLIDE_EXPORTS, Library.has_window_slide).
 * SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection, the order of the rows, partitions, ties, derived terms, measures (kind / index / is_f64), outputs, limit / capacity /
 * the count-only call / SDQH_ERR_OVERFLOW, the bounds check of a term's ranks column and its error, SDQH_ERR_UNSUPPORTED for a
 * bitmap-only table or a compile-only context (argument checks first) and the wait for the stream are exactly those of
 * sdqh_table_window_agg, declared in sdqh_sort_frames.h.  What differs is the frame.
 *
 * Not here: text measures and the multi-GPU runner.  AVG, and ROWS frames with an EXCLUDE clause, are the eighth extension's: sdqh_sort_exclude.h.  Value-based frames (RANGE BETWEEN x
 * PRECEDING ...) and GROUPS frames are the sixth extension's: sdqh_sort_range.h.  NTILE, PERCENT_RANK, CUME_DIST, NTH_VALUE and the
 * percentiles are the seventh's: sdqh_sort_quantile.h. */
#ifndef SDQH_SORT_SLIDE_H
#define SDQH_SORT_SLIDE_H

#include "sdqh_sort_frames.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WSLIDE_FIRST 4            /* ops 0..3 are SDQH_WAGG_SUM / COUNT / MIN / MAX */
#define SDQH_WSLIDE_LAST  5
#define SDQH_SLIDE_UNBOUNDED_PRECEDING INT64_MIN   /* as lo */
#define SDQH_SLIDE_UNBOUNDED_FOLLOWING INT64_MAX   /* as hi */
#define SDQH_WSLIDE_MAX_AGGS 4
typedef struct sdqh_window_slide { int32_t op, kind, index, is_f64; int64_t lo, hi, empty; } sdqh_window_slide;   /* 40 bytes; kind/index/is_f64: the measure */

/* The first min(limit, n) of the n selected rows in sorted order, and beside row j the value of every slide over row j's frame:
 * out_aggs[a * capacity + j], 64 bits each (out_aggs may be NULL: rows only).
 *
 * THE FRAME of sorted row j, in a partition that occupies the sorted positions [s, e], is the positions [max(j + lo, s),
 * min(j + hi, e)]: ROWS BETWEEN with signed offsets, negative = preceding, positive = following.  It is EMPTY when that interval is
 * (LAG before the partition's start, LEAD after its end, (-5, -3) on the second row).  lo > hi: SDQH_ERR_INVALID; every other pair of
 * int64 values is valid and overflows nowhere.  (SDQH_SLIDE_UNBOUNDED_PRECEDING, 0) is sdqh_table_window_agg's ROWS frame,
 * (SDQH_SLIDE_UNBOUNDED_PRECEDING, SDQH_SLIDE_UNBOUNDED_FOLLOWING) its PARTITION frame.  Frames are positional: ties play no part
 * (what is left of a tie is build-row order, as everywhere), and a frame reaches past `limit` — row j < min(limit, n) with hi > 0
 * folds rows at later positions whether they are returned or not.
 *
 *   COUNT          the frame's row count as int64, 0 for an empty frame; ignores its measure and `empty`.
 *   SUM, MIN, MAX  the rules of sdqh_sort_frames.h: integer SUM wraps; MIN / MAX follow the total order and the NaN rule of
 *                  sdqh_extrema.h; double SUM is IEEE addition of exactly the frame's rows in an association that is unspecified but
 *                  fixed for a given input and geometry (no atomics), nothing is ever added and later subtracted — the bound of
 *                  that header holds with m = the frame's row count, and sums of integer-valued doubles below 2^53 are exact.
 *   FIRST, LAST    the measure's 64 bits at the frame's first / last row, copied (NaN payloads, -0.0).  LAG(k) is FIRST over
 *                  (-k, -k), LEAD(k) is FIRST over (k, k).
 * For every op but COUNT an empty frame gives the 64 bits of `empty` (the caller's default: SQL's third argument of LAG).
 *
 * nslides < 1 or > SDQH_WSLIDE_MAX_AGGS, an unknown op, lo > hi, and the measure and argument errors of sdqh_table_window_agg:
 * SDQH_ERR_INVALID, nothing written, *out_n included. */
int sdqh_table_window_slide(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                            int nslides, const sdqh_window_slide* slides, int64_t limit, int64_t capacity,
                            int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                            int64_t* out_aggs /* nslides x capacity, 64 bits each */, int64_t* out_n);
/* What the tests size their cases from: tile_rows — the tile, the one the window and frame passes share — and narrow_max_width — the
 * largest frame width (hi - lo + 1) a kernel walks row by row; 0: no kernel ever does, the work per row does not depend on the width. */
int sdqh_window_slide_geometry(sdqh_ctx* ctx, int64_t* tile_rows, int64_t* narrow_max_width);

#ifdef __cplusplus
}
#endif
#endif
