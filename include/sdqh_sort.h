/* sdqh_sort.h — the HIP library's ordering extension: ORDER BY over the entries of a table, any number of rows.
 *
 * Not part of the boundary every implementation provides (that is sdqh.h, whose entry points the CPU implementation
 * exports one for one): a library that has these symbols orders results on the device, one without them leaves the
 * ordering to the caller (the binding: abi.SORT_EXPORTS, Library.has_sort).  SDQH_ABI_VERSION is not affected.
 *
 * The order is the total order sdqh_table_topk defines (sdqh.h): the sort columns in turn — integers as signed
 * values, doubles by sign and magnitude (-0.0 before +0.0, NaNs by their bits), a descending column reversed — and
 * ties by build-row order.  The reference has no such operator (its results are unordered sets). */
#ifndef SDQH_SORT_H
#define SDQH_SORT_H

#include "sdqh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_SORT_MAX_KEYS 8
#define SDQH_SORT_ALL ((int64_t)1 << 62)
/* ORDER BY over the entries with at least min_hits rows, first min(limit, n) of them; order and tie-break as sdqh_table_topk.
 * Outputs and capacity as sdqh_table_compact; all four out_* NULL: count only.  *out_n = rows written; if min(limit, n) > capacity:
 * SDQH_ERR_OVERFLOW and *out_n = the capacity needed, nothing written. */
int sdqh_table_sorted(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int64_t limit, int nsort, const sdqh_sort_key* sort,
                      int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_n);
/* What the tests size their cases from: largest n of the single-workgroup path, rows per tile of the radix path, and the smallest n
 * at which the scan takes a second level (0: one form for every n). */
int sdqh_sort_geometry(sdqh_ctx* ctx, int64_t* single_wg_max, int64_t* tile_rows, int64_t* second_level_rows);

#ifdef __cplusplus
}
#endif
#endif
