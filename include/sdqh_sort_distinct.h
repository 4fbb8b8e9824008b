/* sdqh_sort_distinct.h — the HIP library's tenth ordering extension: aggregates over the DISTINCT values of a group — COUNT(DISTINCT x),
 * SUM / AVG(DISTINCT x) and MODE per group of the ordered entries of a table, behind one sort.
 *
 * Like its nine siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * folds distinct values on the device, one without them leaves it to the caller (the binding: abi.GROUP_DISTINCT_EXPORTS,
 * Library.has_group_distinct).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection (min_hits, owner rows only), the order of the rows, derived terms, the bounds check of a term's ranks column and its
 * error are exactly those of sdqh_table_window, declared in sdqh_sort_window.h, and of sdqh_table_grouping_sets.
 *
 * Not here: DISTINCT over window frames; several levels per call (a distinct count does not fold from a finer level's counts, so
 * one call serves one grouping); more than SDQH_GD_MAX_AGGS aggregates per call; and the multi-GPU runner. */
#ifndef SDQH_SORT_DISTINCT_H
#define SDQH_SORT_DISTINCT_H

#include "sdqh_sort_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_GD_MAX_AGGS 4
#define SDQH_GD_COUNT_DISTINCT 0
#define SDQH_GD_SUM_DISTINCT   1
#define SDQH_GD_AVG_DISTINCT   2
#define SDQH_GD_MODE           3
#define SDQH_GD_MODE_COUNT     4
#define SDQH_GD_COUNT          5
typedef struct sdqh_distinct_agg { int32_t op, kind, index, is_f64; } sdqh_distinct_agg;   /* 16 bytes; op: SDQH_GD_*; kind/index/is_f64: the measure */

/* GROUPS AND VALUE RUNS.  The first ngroup terms (0 <= ngroup <= nterms - 1; 0: the whole selection is one group) group, the other
 * nterms - ngroup >= 1 terms are "the value".  A GROUP is a maximal run of sorted rows equal in the first ngroup terms, a VALUE RUN a
 * maximal run equal in all nterms terms.  Equality is the rule of sdqh_sort_window.h, equality under the total order: -0.0 and +0.0
 * are two values, NaNs are equal only bit for bit.  A run's REPRESENTATIVE is its first sorted row.
 *
 * OUTPUT.  One row per group, in sorted order.  Row j carries the key / payload / values / hits of its group's first sorted row, as
 * at one level of sdqh_table_grouping_sets: the columns that are not among the first ngroup terms are that row's own and carry no
 * meaning.  out_aggs[a * capacity + j], 64 bits each, is aggregate a of group j (out_aggs may be NULL: rows only).  With g the
 * number of groups, *out_n = min(limit, g).
 *
 * OPS.  A measure (kind / index / is_f64) is what sdqh_sort_frames.h calls one.
 *   SDQH_GD_COUNT_DISTINCT  the number of value runs in the group (int64; the measure is ignored).
 *   SDQH_GD_SUM_DISTINCT    the measure read at every run's representative, summed.  Integers wrap around in two's complement; doubles
 *                           are IEEE additions of exactly the group's representatives in an association that is fixed for a given
 *                           input and geometry (no atomics: two calls give the same bits), nothing is added and later subtracted, no
 *                           row of another group enters a sum, and |result - exact| <= g(m) * sum|v| with g(m) = (m-1)u / (1 - (m-1)u),
 *                           u = 2^-53, m the group's number of runs — the bound of sdqh_sort_groups.h.  For SQL's SUM(DISTINCT x) the
 *                           caller passes x both as the value term and as the measure.
 *   SDQH_GD_AVG_DISTINCT    that sum converted to double, divided by (double)COUNT_DISTINCT in one IEEE division: the rule of
 *                           sdqh_sort_exclude.h.  Always a double.
 *   SDQH_GD_MODE            the 64 bits of the measure at the representative of the group's longest value run, copied (NaN payloads
 *                           and -0.0 included).  Among runs of equal length the first in sorted order wins.
 *   SDQH_GD_MODE_COUNT      that run's length (int64; the measure is ignored).
 *   SDQH_GD_COUNT           the group's rows (int64; the measure is ignored), so that a distinct ratio needs no second call.
 *
 * SIZES, ERRORS, WAITS.  Those of sdqh_table_grouping_sets with one level.  The number of groups is known only after the sort: one
 * read-back of the run and group counts, then the ways out.  All of out_keys / out_payload / out_values / out_hits / out_aggs NULL:
 * the count-only call — the sort and the depth pass run, *out_n is returned.  min(limit, g) > capacity: SDQH_ERR_OVERFLOW, *out_n =
 * the count needed, no array is written.  An empty selection gives 0 rows.
 * An unknown op, a measure the table lacks, is_f64 on SDQH_SORT_KEY / SDQH_SORT_HITS, naggs < 1 or > SDQH_GD_MAX_AGGS, aggs NULL,
 * ngroup < 0 or ngroup >= nterms and the argument errors of sdqh_table_window: SDQH_ERR_INVALID, nothing written, *out_n included.
 * Those named here — the measures' among them — and those of sdqh_table_window that read the caller's arguments alone come before
 * SDQH_ERR_UNSUPPORTED for a bitmap-only table or a compile-only context; a term naming a field the table lacks comes after it, as
 * it does there. */
int sdqh_table_group_distinct(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits,
                              int nterms, const sdqh_sort_term* terms, int ngroup,
                              int naggs, const sdqh_distinct_agg* aggs, int64_t limit, int64_t capacity,
                              int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                              int64_t* out_aggs      /* naggs x capacity, 64 bits each; may be NULL */,
                              int64_t* out_n);
/* What the tests size their cases from: the tile both stages' passes share with the window passes — rows per tile at the lower
 * stage, value runs per tile at the upper one. */
int sdqh_group_distinct_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
