/* sdqh_sort_groups.h — the HIP library's ninth ordering extension: the ordered entries of a table re-grouped — GROUP BY ROLLUP /
 * CUBE / GROUPING SETS over a result: one row per group at several nested levels of one key list behind one sort, with SUM / COUNT /
 * MIN / MAX / AVG per group: subtotals per prefix of the keys, the grand total, the distinct key combinations.
 *
 * Like its eight siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * groups on the device, one without them leaves it to the caller (the binding: abi.GROUPING_SETS_EXPORTS,
 * Library.has_grouping_sets).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection (min_hits, owner rows only), the order of the rows, derived terms, the bounds check of a term's ranks column and its
 * error are exactly those of sdqh_table_window, declared in sdqh_sort_window.h.  There is no npartition: all nterms terms
 * (1 .. SDQH_SORT_MAX_KEYS) are grouping terms, and a term's direction only decides the order in which the groups come.
 *
 * Not here: text measures, HAVING on the groups, more than SDQH_GS_MAX_AGGS aggregates per call, and the multi-GPU runner. */
#ifndef SDQH_SORT_GROUPS_H
#define SDQH_SORT_GROUPS_H

#include "sdqh_sort_exclude.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_GS_MAX_AGGS 4
typedef struct sdqh_group_agg { int32_t op, kind, index, is_f64; } sdqh_group_agg;   /* 16 bytes; op: SDQH_WAGG_SUM/COUNT/MIN/MAX or SDQH_WEX_AVG; kind/index/is_f64: the measure */

/* LEVELS.  Bit L of `levels`, 0 <= L <= nterms, asks for the groups of level L: the maximal runs of sorted rows whose first L keys
 * are equal.  Level 0 is the whole selection, one group; level nterms is the distinct key combinations.  levels == 0 or a bit above
 * nterms: SDQH_ERR_INVALID.
 *
 * OUTPUT.  One row per group.  The levels come one after the other, from the highest L asked for down to the lowest; inside a level
 * the rows are in sorted order.  Row j carries the key / payload / values / hits of its group's first sorted row, the
 * representative: the columns that are not among the level's first L terms are that row's own and carry no meaning.
 * out_aggs[a * capacity + j], 64 bits each, is aggregate a over exactly the rows of row j's group (out_aggs may be NULL with
 * naggs > 0: rows only; naggs == 0 with out_aggs NULL: the distinct combinations and their counts alone).  out_level_rows[L]
 * (SDQH_SORT_MAX_KEYS + 1 counts; may be NULL) is the number of groups of level L, before `limit`, and 0 for a level not asked for:
 * the caller reads a row's level off these counts.  With g the sum of the level counts, *out_n = min(limit, g).
 *
 * VALUES.  The rules of sdqh_sort_frames.h, word for word: integer SUM wraps around in two's complement, MIN / MAX are signed;
 * double MIN / MAX follow the total order and the NaN rule of sdqh_extrema.h; a double SUM is IEEE addition of exactly the group's
 * rows in an association that is fixed for a given input, geometry and `levels` (no atomics: two calls give the same bits), nothing
 * is added and later subtracted, no row of another group enters a sum, and |result - exact| <= g(m) * sum|v| with
 * g(m) = (m-1)u / (1 - (m-1)u), u = 2^-53, m the group's size.  A coarser level may be folded from the finer level's group values or
 * from the rows: the bound holds either way, and which it is is left open.  A measure (kind / index / is_f64) is what
 * sdqh_sort_frames.h calls one; COUNT ignores it and is int64.  SDQH_WEX_AVG returns a double by the rule of sdqh_sort_exclude.h: the
 * column's own SUM converted to double, divided by (double)COUNT in one IEEE division.
 *
 * SIZES, ERRORS, WAITS.  The number of groups is known only after the sort, so the call has the shape of a filtering sibling
 * (sdqh_table_window with a per_limit): one read-back of the level counts, then the ways out.  All of out_keys / out_payload /
 * out_values / out_hits / out_aggs NULL: the count-only call — the sort and the level pass run, *out_n and out_level_rows are
 * returned.  min(limit, g) > capacity: SDQH_ERR_OVERFLOW, *out_n = the count needed, no row array is written.  An empty selection
 * gives 0 rows and level counts of 0: this call invents no grand-total row for it.
 * An unknown op, a measure the table lacks, is_f64 on SDQH_SORT_KEY / SDQH_SORT_HITS, naggs < 0 or > SDQH_GS_MAX_AGGS, naggs > 0
 * without aggs, a bad `levels` and the argument errors of sdqh_table_window: SDQH_ERR_INVALID, nothing written, *out_n included.
 * Those named here — the measures' among them — and those of sdqh_table_window that read the caller's arguments alone come before
 * SDQH_ERR_UNSUPPORTED for a bitmap-only table or a compile-only context; a term naming a field the table lacks comes after it, as
 * it does there.  More than 2^32 - 1 groups over the levels asked for: SDQH_ERR_UNSUPPORTED. */
int sdqh_table_grouping_sets(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits,
                             int nterms, const sdqh_sort_term* terms, uint32_t levels,
                             int naggs, const sdqh_group_agg* aggs, int64_t limit, int64_t capacity,
                             int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                             int64_t* out_aggs      /* naggs x capacity, 64 bits each; may be NULL */,
                             int64_t* out_level_rows /* SDQH_SORT_MAX_KEYS + 1 counts; may be NULL */,
                             int64_t* out_n);
/* What the tests size their cases from: the tile every level's pass shares with the window passes. */
int sdqh_grouping_sets_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
