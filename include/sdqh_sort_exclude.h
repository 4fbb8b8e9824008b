/* sdqh_sort_exclude.h — the HIP library's eighth ordering extension: window frames with rows taken out — SUM / COUNT / MIN / MAX /
 * FIRST_VALUE / LAST_VALUE / AVG (measure) OVER (PARTITION BY ... ORDER BY ... ROWS | RANGE | GROUPS BETWEEN lo AND hi EXCLUDE
 * CURRENT ROW | GROUP | TIES | NO OTHERS), the frame's unit chosen per column: "the average of the other orders of that day", "the
 * best price among the rows that are not my peers", a moving ROWS average beside a RANGE count behind one sort.
 *
 * Like its seven siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * folds such frames on the device, one without them leaves it to the caller (the binding: abi.WINDOW_EXCLUDE_EXPORTS,
 * Library.has_window_exclude).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection, the order of the rows, partitions, ties, derived terms, the measure (kind / index / is_f64), outputs, limit / capacity /
 * the count-only call / SDQH_ERR_OVERFLOW, the bounds check of a term's ranks column and its error, the order of the argument checks
 * against SDQH_ERR_UNSUPPORTED for a bitmap-only table or a compile-only context (argument checks first) and the wait for the stream
 * are exactly those of sdqh_table_window_range, declared in sdqh_sort_range.h.  Frames look past `limit`, as they do there.  What
 * differs is the frame: its unit is a column's own, rows are taken out of it, and AVG is an op.
 *
 * Not here: text measures, weighted frames, more than SDQH_WEX_MAX_COLS columns per call, and the multi-GPU runner. */
#ifndef SDQH_SORT_EXCLUDE_H
#define SDQH_SORT_EXCLUDE_H

#include "sdqh_sort_range.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WEX_ROWS        2   /* unit; 0 / 1 are SDQH_WRANGE_VALUE / SDQH_WRANGE_GROUPS with their meaning */
#define SDQH_WEX_AVG         6   /* op; 0..5 are SUM COUNT MIN MAX FIRST LAST as in sdqh_sort_slide.h */
#define SDQH_WEX_NO_OTHERS   0   /* exclude */
#define SDQH_WEX_CURRENT_ROW 1
#define SDQH_WEX_GROUP       2
#define SDQH_WEX_TIES        3
#define SDQH_WEX_MAX_COLS    4
typedef struct sdqh_window_exclude { int32_t op, kind, index, is_f64, unit, flags, exclude, _pad; int64_t lo, hi, empty; } sdqh_window_exclude;   /* 56 bytes; kind/index/is_f64: the measure */

/* The first min(limit, n) of the n selected rows in sorted order, and beside row j the value of every column over what is left of
 * row j's frame: out_cols[c * capacity + j], 64 bits each (out_cols may be NULL: rows only).
 *
 * THE BASE FRAME F = [l, r] of sorted row j, inside its partition at the sorted positions [s, e].  `unit` is the column's own: one
 * call may mix the three.
 *
 *   unit = VALUE, GROUPS   the frame of sdqh_table_window_range, word for word: VALUE's demand for nterms == npartition + 1 and a
 *                   term without ranks (a call with any VALUE column), the 128-bit integer bounds, the one IEEE addition per bound of
 *                   a double term, the NaN and -0.0 / +0.0 rules, GROUPS' count of tie heads.
 *   unit = ROWS     the frame of sdqh_table_window_slide: [max(j + lo, s), min(j + hi, e)] in mathematical integers.
 *
 * All three units mark an unbounded side in `flags` (SDQH_WRANGE_LO_UNBOUNDED / SDQH_WRANGE_HI_UNBOUNDED: lo / hi is ignored, the
 * side reaches s / e).  Both sides bounded with lo > hi (as integers, or as doubles for a VALUE column over a double term, where a
 * non-finite offset is an error too), an unknown unit / op / exclude / flag bit, _pad != 0, ncols < 1 or > SDQH_WEX_MAX_COLS, and
 * the argument errors of sdqh_table_window_range: SDQH_ERR_INVALID, nothing written, *out_n included.  These read the caller's
 * structs alone and come before SDQH_ERR_UNSUPPORTED; what needs the table is looked at after it, as there.
 *
 * THE EXCLUSION.  [a, b] is row j's tie run: the positions around j whose nterms keys all equal j's (with no ORDER BY term the
 * partition is one run).  The removed set X is nothing (NO_OTHERS), {j} (CURRENT_ROW), [a, b] (GROUP) or [a, b] \ {j} (TIES).  X is
 * cut out after the base frame was found: what remains, F \ X, is at most three pieces in position order —
 *
 *       [l, min(r, x0 - 1)]      {j}, only under TIES and only if j lies in F      [max(l, x1 + 1), r]
 *
 * with [x0, x1] the hull of X.  A row outside its own base frame is never added.
 *
 * THE VALUES.  COUNT is the number of remaining rows, 0 if none.  FIRST / LAST copy the measure's 64 bits at the first / last
 * remaining position.  SUM / MIN / MAX follow the rules of sdqh_sort_frames.h over exactly the remaining rows: every piece is folded
 * by the iterative query of the fold tree sdqh_table_window_range reads, the pieces are joined left to right; nothing is added and
 * later subtracted, there are no atomics, and the association is a function of the pieces' ends and the geometry alone — two
 * calls, and two rows with the same pieces, give the same bits; with NO_OTHERS a VALUE or GROUPS column has the bits of
 * sdqh_table_window_range.  The bound of sdqh_sort_frames.h holds with m = the number of remaining rows.  AVG returns a double: the
 * column's own SUM converted to double — the wrapping int64 sum of an integer measure by one round-to-nearest conversion, the SUM
 * op's bits of a double measure — divided by (double)COUNT in one IEEE division.  Nothing remaining: the 64 bits of `empty` for every
 * op but COUNT. */
int sdqh_table_window_exclude(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                              int ncols, const sdqh_window_exclude* cols, int64_t limit, int64_t capacity,
                              int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                              int64_t* out_cols /* ncols x capacity, 64 bits each */, int64_t* out_n);
/* What the tests size their cases from: tile_rows — the tile every window pass shares — and narrow_max_width — the largest frame
 * width a kernel walks row by row; 0: no kernel ever does. */
int sdqh_window_exclude_geometry(sdqh_ctx* ctx, int64_t* tile_rows, int64_t* narrow_max_width);

#ifdef __cplusplus
}
#endif
#endif
