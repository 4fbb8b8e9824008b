/* sdqh_sort_range.h — the HIP library's sixth ordering extension: aggregates and values over VALUE and GROUP window frames of the
 * ordered entries of a table — SUM / COUNT / MIN / MAX / FIRST_VALUE / LAST_VALUE (measure) OVER (PARTITION BY ... ORDER BY ...
 * RANGE | GROUPS BETWEEN lo AND hi): "every order whose revenue lies within 1000 of this one's", "this order date and the six
 * distinct dates before it".
 *
 * Like its five siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * folds such frames on the device, one without them leaves it to the caller (the binding: abi.WINDOW_RANGE_EXPORTS,
 * Library.has_window_range).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * The six ops, the measure (kind / index / is_f64), `empty` and COUNT's 0 for an empty frame, the rules for integer and double SUM,
 * MIN / MAX and NaN, selection, the order of the rows, partitions, ties, derived terms, outputs, limit / capacity / the count-only
 * call / SDQH_ERR_OVERFLOW, the bounds check of a term's ranks column and its error, SDQH_ERR_UNSUPPORTED for a bitmap-only table or
 * a compile-only context (argument checks first) and the wait for the stream are exactly those of sdqh_table_window_slide, declared
 * in sdqh_sort_slide.h.  Frames look past `limit`, as they do there.  What differs is the frame.
 *
 * These two frame units were the first entries of sdqh_sort_slide.h's "Not here" list.  EXCLUDE clauses, AVG and frames of different
 * units in one call are the eighth extension's: sdqh_sort_exclude.h.  Not here: text measures; calendar arithmetic — dates are stored as yyyymmdd integers, so a VALUE offset on a
 * date column counts in those units (GROUPS counts distinct dates); and the multi-GPU runner. */
#ifndef SDQH_SORT_RANGE_H
#define SDQH_SORT_RANGE_H

#include "sdqh_sort_slide.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WRANGE_VALUE  0          /* offsets are differences of the ORDER BY value      */
#define SDQH_WRANGE_GROUPS 1          /* offsets count tie runs (peer groups)               */
#define SDQH_WRANGE_LO_UNBOUNDED 1    /* flags: lo is ignored, the side is UNBOUNDED PRECEDING */
#define SDQH_WRANGE_HI_UNBOUNDED 2    /*        hi is ignored, UNBOUNDED FOLLOWING             */
#define SDQH_WRANGE_MAX_AGGS 4
typedef struct sdqh_window_range { int32_t op, kind, index, is_f64, unit, flags; int64_t lo, hi, empty; } sdqh_window_range;   /* 48 bytes; kind/index/is_f64: the measure */

/* The first min(limit, n) of the n selected rows in sorted order, and beside row j the value of every range over row j's frame:
 * out_aggs[a * capacity + j], 64 bits each (out_aggs may be NULL: rows only).
 *
 * THE FRAME.  Sorted row j lies in a partition at the sorted positions [s, e].  Offsets are signed along the order, as in
 * sdqh_table_window_slide: negative = preceding.  A side whose UNBOUNDED flag is set reaches s (lo) or e (hi).
 *
 *   unit = GROUPS   g(i) = the number of tie heads in [s, i]; a tie is all nterms keys equal.  The frame is
 *                   {i in [s, e] : g(j) + lo <= g(i) <= g(j) + hi}, taken in mathematical integers.  Valid for any nterms >=
 *                   npartition; with no ORDER BY term a partition is one group.
 *   unit = VALUE    requires nterms == npartition + 1 — exactly one ORDER BY term, as SQL demands — and that term to have ranks ==
 *                   NULL (text has no arithmetic): anything else is SDQH_ERR_INVALID.  v(i) is the term's value before the descending
 *                   reversal: the derived `field` of sdqh_sort_terms.h, or the column itself.  d = +1 ascending, -1 descending.
 *     integer term  (KEY, integer PAYLOAD, HITS, derived.)  lo and hi are int64.  The frame is {i : lo <= d * (v(i) - v(j)) <= hi} in
 *                   mathematical integers: nothing wraps, v(j) + lo beyond int64 behaves as a bound that no value reaches.
 *     double term   (is_f64 PAYLOAD, VALUE.)  lo and hi hold the bits of finite doubles; a non-finite offset is SDQH_ERR_INVALID.
 *                   The bounds are a = v(j) + d * lo and b = v(j) + d * hi, each ONE IEEE addition rounded to nearest, and the frame
 *                   is the non-NaN rows with min(a, b) <= v(i) <= max(a, b) under IEEE comparison: -0.0 and +0.0 enter or stay out
 *                   together.  IEEE addition is monotone, so the frame is an interval of the total order of sdqh_sort.h.  A row whose
 *                   own v(j) is a NaN ends each bounded side at the end of its own tie run (the rows with the same bits), whatever
 *                   the offset.  A NaN row never enters a bounded side of a non-NaN row's frame; an unbounded side still reaches s
 *                   or e, NaN rows included.
 *
 * Both sides bounded with lo > hi (compared as integers, or as doubles for a double term), an unknown unit, unknown flag bits,
 * nranges < 1 or > SDQH_WRANGE_MAX_AGGS, and the argument errors of sdqh_table_window_slide: SDQH_ERR_INVALID, nothing written, *out_n
 * included.  These read the caller's structs alone and come before SDQH_ERR_UNSUPPORTED.  What needs the table — a term or a measure
 * that names a field the table does not have, an is_f64 KEY / HITS measure, a term that derives from a double — is SDQH_ERR_INVALID
 * too, but is looked at after it, as in sdqh_table_window_slide: a compile-only context answers SDQH_ERR_UNSUPPORTED for those.
 *
 * THE VALUES.  Rows with the same frame [l, r] get the same bits for every op — in particular all rows of a tie run do — and two
 * calls give the same bits: no atomics on the value path.  Exactly the frame's rows enter a SUM, once each, in an association that is
 * a function of (l, r) and the geometry alone; nothing is added and later subtracted; the bound of sdqh_sort_frames.h holds with m =
 * the frame's row count. */
int sdqh_table_window_range(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                            int nranges, const sdqh_window_range* ranges, int64_t limit, int64_t capacity,
                            int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                            int64_t* out_aggs /* nranges x capacity, 64 bits each */, int64_t* out_n);
/* What the tests size their cases from: tile_rows — the tile, the one the window, frame and slide passes share — and
 * narrow_max_width — the largest frame width a kernel walks row by row; 0: no kernel ever does. */
int sdqh_window_range_geometry(sdqh_ctx* ctx, int64_t* tile_rows, int64_t* narrow_max_width);

#ifdef __cplusplus
}
#endif
#endif
