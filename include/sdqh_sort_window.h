/* sdqh_sort_window.h — the HIP library's third ordering extension: ranks inside partitions of the ordered entries of a table, and
 * the first k rows of every partition — ROW_NUMBER() / RANK() / DENSE_RANK() OVER (PARTITION BY ... ORDER BY ...), usually under
 * a `<= k` filter ("ORDER BY ... LIMIT k per group").
 *
 * Like sdqh_sort.h and sdqh_sort_terms.h it is not part of the boundary every implementation provides (sdqh.h): a library that has
 * these symbols ranks on the device, one without them leaves the ranking to the caller (the binding: abi.WINDOW_EXPORTS,
 * Library.has_window).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * The entries are ordered by all nterms terms (sdqh_sort_terms.h), ties by build-row order; each term becomes an order-preserving
 * 64-bit key (the total order of sdqh_table_topk: integers as signed values, doubles by sign and magnitude, a descending term
 * reversed).  A PARTITION is a maximal run of ordered rows whose first npartition keys are equal; two rows TIE when all nterms
 * keys are equal.  Equality is equality of those keys, that is equality under the total order: -0.0 and +0.0 are different values,
 * NaNs are equal only bit for bit. */
#ifndef SDQH_SORT_WINDOW_H
#define SDQH_SORT_WINDOW_H

#include "sdqh_sort_terms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_WIN_ROW_NUMBER 0   /* 1, 2, 3, ... in order; what is left of a tie is build-row order        */
#define SDQH_WIN_RANK       1   /* 1 + rows of the partition that sort strictly before (ties share)     */
#define SDQH_WIN_DENSE_RANK 2   /* 1 + distinct order values of the partition that sort strictly before */

/* The rows whose rank (of `kind`) inside their partition is <= per_limit (SDQH_SORT_ALL: every row), in sorted order, the first
 * min(limit, kept) of them; out_rank (may be NULL) receives the rank of every row written.
 *
 * Selection (min_hits, owner rows only), the total order of every term, derivations, the bounds check of a term's ranks column
 * and its error (SDQH_ERR_INVALID naming the term, nothing written, *out_n included) and the limit of SDQH_SORT_MAX_KEYS terms are
 * those of sdqh_table_sorted_by.  The first npartition terms are PARTITION BY (their direction only decides in which order the
 * partitions come).  npartition == 0: the whole selection is one partition (SDQH_WIN_RANK with per_limit = k is then "top k with
 * ties").  npartition == nterms: SDQH_WIN_ROW_NUMBER counts in build-row order, the other two kinds give 1 everywhere.
 *
 * Outputs and capacity as sdqh_table_compact; all of out_keys / out_payload / out_values / out_hits / out_rank NULL: count only
 * (*out_n = min(limit, kept); unlike sdqh_table_sorted this runs the passes, because the count depends on the ranks).  If
 * min(limit, kept) > capacity: SDQH_ERR_OVERFLOW, *out_n = the capacity needed, nothing written.
 * per_limit < 1, limit < 1, an unknown kind, npartition < 0, npartition > nterms, nterms < 1 (or > SDQH_SORT_MAX_KEYS):
 * SDQH_ERR_INVALID, nothing written.  A bitmap-only table or a compile-only context: SDQH_ERR_UNSUPPORTED.  Waits for the stream. */
int sdqh_table_window(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits,
                      int npartition, int nterms, const sdqh_sort_term* terms,
                      int kind, int64_t per_limit, int64_t limit, int64_t capacity,
                      int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                      int64_t* out_rank, int64_t* out_n);
/* What the tests size their cases from: the sorted positions one wave ranks per step of the tile scan (a tile; a carry crosses
 * from one tile to the next).  One form for every n. */
int sdqh_window_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
