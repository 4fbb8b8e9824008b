/* sdqh_extrema.h — the HIP library's extrema extension: MIN / MAX per entry of an accumulating table, and over a column.
 *
 * Not part of the boundary every implementation provides (that is sdqh.h): a library that has these symbols folds
 * minima and maxima on the device, one without them has no MIN / MAX (the binding: abi.EXTREMA_EXPORTS,
 * Library.has_extrema).  SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Order: the total order sdqh_table_topk defines (sdqh.h) — doubles by sign and magnitude, -0.0 below +0.0 — so
 * min{+0.0, -0.0} is -0.0 and max is +0.0 whatever the row order.  A NaN value is skipped (as SQL skips NULL) but its
 * row still counts as a hit; a slot no non-NaN value reached reads as a quiet NaN.  Integer values are folded as
 * doubles (the accumulators are doubles): one with |v| > 2^53 is never rounded silently — SDQH_ERR_UNSUPPORTED.
 *
 * Encoding: between _begin and _end a slot holds e(v) = the order-preserving uint64 of v's bits (reversed for MIN),
 * folded by an unsigned 64-bit maximum.  With NaNs skipped no value encodes to 0: 0 is the identity of both
 * operations (_begin writes it, _end reads it as the quiet NaN).  Unsigned max is associative, commutative and
 * idempotent: any number of _fold calls between _begin and _end equals one fold of the concatenated rows, bit for bit. */
#ifndef SDQH_EXTREMA_H
#define SDQH_EXTREMA_H

#include "sdqh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_EXT_MIN 0
#define SDQH_EXT_MAX 1
/* Mark accumulator slots of an accumulating table as extrema slots: from here to _end they hold ENCODED values and must not be read.
 * Slots not named, payload and hits keep their bits.  A table without accumulators, a slot >= the entries' room or named twice, an
 * unknown op: SDQH_ERR_INVALID; a membership-only table: SDQH_ERR_UNSUPPORTED. */
int sdqh_table_extrema_begin(sdqh_ctx* ctx, sdqh_table* table, int nslots, const int32_t* slots, const int32_t* ops);
/* For every row r < nrows whose key[r] is in the table: slot s of the matched entry = op_s(slot, vals[s][r]) (entries that share
 * their accumulators — sdqh_table_share_groups — share these too).  vals: I64 or F64 columns; val_is_f64[s] != 0 says an I64-typed
 * column holds the raw bits of doubles (as sdqh_xcompact returns them).  count_hits != 0: hits += 1 per matched row, NaN rows included.
 * Every slot must have been named by _begin (else, or without _begin: SDQH_ERR_INVALID).  nrows = 0 launches nothing. */
int sdqh_table_extrema_fold(sdqh_ctx* ctx, sdqh_table* table, int64_t nrows, const sdqh_column* key, int nslots, const int32_t* slots,
                            const sdqh_column* const* vals, const int32_t* val_is_f64, int count_hits);
/* Decode the slots back to doubles.  Waits for the stream (so it cannot be recorded into a plan graph).  SDQH_ERR_UNSUPPORTED when an
 * integer value beyond +-2^53 was folded: the slots are unspecified until the next _begin. */
int sdqh_table_extrema_end(sdqh_ctx* ctx, sdqh_table* table);
/* Minimum, maximum (as doubles) and the number of non-NaN values of a column; nrows = 0 or all NaN: count 0, min = max = quiet NaN.
 * An I64 column with is_f64 != 0 holds the raw bits of doubles.  An integer beyond +-2^53: SDQH_ERR_UNSUPPORTED.  Waits for the stream. */
int sdqh_column_extrema(sdqh_ctx* ctx, int64_t nrows, const sdqh_column* col, int is_f64, double* out_min, double* out_max, int64_t* out_count);
/* What the tests size their cases from: rows one workgroup takes per step of the fold. */
int sdqh_extrema_geometry(sdqh_ctx* ctx, int64_t* rows_per_step);

#ifdef __cplusplus
}
#endif
#endif
