/* sdqh_sort_terms.h — the HIP library's second ordering extension: ORDER BY over DERIVED columns of a table's entries
 * (the halves of a packed key, the digits of a mixed-radix key, text that travels as row references or dictionary codes),
 * and the ranking of a text column that makes the last of these possible.
 *
 * Like sdqh_sort.h it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * orders such results on the device, one without them leaves them to the caller (the binding: abi.SORT_TERMS_EXPORTS,
 * Library.has_sort_terms).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * A sort TERM is a sort column of sdqh_table_sorted plus a derivation of the value that is ordered:
 *
 *     field = (uint64(source) / div) % mod + add          div <= 1: no division; mod == 0: no modulo
 *     value = ranks ? ranks[field] : field                 ordered as a signed 64-bit integer, reversed when descending
 *
 * (key >> 32 is div = 2^32; key & 0xFFFFFFFF is mod = 2^32; digit i of a mixed-radix key is div = the product of the spans
 * below it, mod = its span, add = its lowest value.)  A derivation applies to integer sources only: SDQH_SORT_KEY, an integer
 * SDQH_SORT_PAYLOAD, SDQH_SORT_HITS; on a double (is_f64 != 0, SDQH_SORT_VALUE) it is SDQH_ERR_INVALID.  A term with
 * div <= 1, mod == 0, add == 0 and ranks == NULL is underived: exactly the column sdqh_table_sorted orders by. */
#ifndef SDQH_SORT_TERMS_H
#define SDQH_SORT_TERMS_H

#include "sdqh_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_TEXT_RANK_MAX_WIDTH 128      /* code units per row sdqh_text_ranks takes */

typedef struct sdqh_sort_term {
    int32_t kind, index, descending, is_f64;     /* as sdqh_sort_key */
    int64_t div, mod, add;
    const sdqh_column* ranks;                    /* NULL, or an I64 column indexed by the field */
} sdqh_sort_term;

/* Dense ranks of the rows of a text column: *out_ranks = a new resident I64 column of nrows ranks in [0, *out_distinct) with
 * rank[r] < rank[s] iff text r sorts before text s and rank[r] == rank[s] iff they are equal.  The order is that of numpy's
 * '<U' arrays: code units compared as unsigned 32-bit values position by position, the zero padding first ("ab" < "abc").
 * nrows = 0 launches nothing (*out_distinct = 0).  A column that is not SDQH_STR or does not cover nrows: SDQH_ERR_INVALID;
 * wider than SDQH_TEXT_RANK_MAX_WIDTH code units: SDQH_ERR_UNSUPPORTED.  Waits for the stream.  Free the column with
 * sdqh_column_free. */
int sdqh_text_ranks(sdqh_ctx* ctx, const sdqh_column* text, int64_t nrows, sdqh_column** out_ranks, int64_t* out_distinct);

/* sdqh_table_sorted over terms: selection, tie-break by build-row order, outputs, capacity / overflow contract, the count-only call
 * and the limit of SDQH_SORT_MAX_KEYS columns are its own; underived terms only give exactly its rows.  A field of a selected
 * entry outside [0, rows of the term's ranks column) is never read through: SDQH_ERR_INVALID naming the term, and nothing —
 * not even *out_n — is written. */
int sdqh_table_sorted_by(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int64_t limit, int nterms, const sdqh_sort_term* terms,
                         int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_n);

#ifdef __cplusplus
}
#endif
#endif
