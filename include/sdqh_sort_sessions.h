/* sdqh_sort_sessions.h — the HIP library's twelfth ordering extension: sessions (gaps and islands) inside the partitions of the
 * ordered entries of a table — a new group wherever the ORDER BY value moves on by more than a gap ("visits separated by more than
 * 30 minutes") or wherever a marker column changes ("runs of consecutive days with the same ship priority") — with columns over the
 * row's whole session, for every row or as one row per session, behind one sort.
 *
 * Like its eleven siblings it is not part of the boundary every implementation provides (sdqh.h): a library that has these symbols
 * cuts sessions on the device, one without them leaves it to the caller (the binding: abi.SESSIONS_EXPORTS, Library.has_sessions).
 * SDQH_ABI_VERSION is not affected.  The reference has no such operator.
 *
 * Selection, the order of the rows, partitions (the first `npartition` terms), ties, derived terms, the bounds check of a term's
 * ranks column and its error, and the wait for the stream are sdqh_table_window's (sdqh_sort_window.h).  What a value offset means
 * for an integer and for a double term is sdqh_sort_range.h's VALUE frame; the ops SUM / COUNT / MIN / MAX / FIRST / LAST are
 * sdqh_sort_slide.h's, AVG is sdqh_sort_exclude.h's, a measure (kind / index / is_f64) and its validity rules sdqh_sort_frames.h's,
 * and what a SUM, a MIN / MAX and an AVG over a group give is sdqh_sort_groups.h's.
 *
 * Not here: calendar arithmetic — dates are stored as yyyymmdd integers, so a gap on a date column counts in those units —, a rule on
 * two columns at once, a cap on a session's length or duration, text measures, more than SDQH_SS_MAX_COLS columns per call, and the
 * multi-GPU runner. */
#ifndef SDQH_SORT_SESSIONS_H
#define SDQH_SORT_SESSIONS_H

#include "sdqh_sort_range.h"
#include "sdqh_sort_exclude.h"
#include "sdqh_sort_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDQH_SS_GAP    0      /* a new session where the ORDER BY value moves on by more than `gap` */
#define SDQH_SS_CHANGE 1      /* a new session where the marker's stored 64 bits change            */
/* 24 bytes; rule: SDQH_SS_*; kind / index / is_f64: the marker of SDQH_SS_CHANGE, named as a measure is; gap: SDQH_SS_GAP's, an
 * int64 for an integer gap term, the bits of a double for a double one */
typedef struct sdqh_session_rule { int32_t rule, kind, index, is_f64; int64_t gap; } sdqh_session_rule;
#define SDQH_SS_NUMBER 7      /* ops 0..5: SUM COUNT MIN MAX FIRST LAST (sdqh_sort_slide.h), 6: SDQH_WEX_AVG */
#define SDQH_SS_ROW    8
#define SDQH_SS_MAX_COLS 4
/* 16 bytes; op: one of the nine; kind / index / is_f64: the measure (COUNT, NUMBER and ROW ignore it: it is not checked) */
typedef struct sdqh_session_col { int32_t op, kind, index, is_f64; } sdqh_session_col;

/* WHERE A SESSION STARTS.  Sorted row j starts a session iff it is the head of its partition or the rule says so about rows j - 1
 * and j of the same partition.
 *
 *   SDQH_SS_GAP     needs nterms >= npartition + 1; the gap term is terms[npartition] and must have ranks == NULL (text has no
 *                   arithmetic); later terms only break ties.  Row j CONTINUES row j - 1's session iff row j - 1 lies in row j's
 *                   frame RANGE BETWEEN gap PRECEDING AND CURRENT ROW as sdqh_sort_range.h defines a VALUE frame (lo = -gap, hi =
 *                   0), v being the term's value before the descending reversal — the derived `field`, or the column itself.
 *     integer term  taken in mathematical integers: nothing wraps.  INT64_MIN next to INT64_MAX is a difference of 2^64 - 1 and a
 *                   new session for every gap.  gap is an int64 >= 0.
 *     double term   gap holds the bits of a finite double >= 0.  The bound is ONE IEEE addition a = v(j) + d * (-gap), d = +1
 *                   ascending, -1 descending; row j continues iff min(a, v(j)) <= v(j - 1) <= max(a, v(j)) under IEEE comparison,
 *                   so -0.0 and +0.0 are the same value.  A NaN row continues only a row with the same bits, and no other row
 *                   continues a NaN row.
 *                   A negative gap, a non-finite double gap, or a ranks column on the gap term: SDQH_ERR_INVALID.  rule->kind, index
 *                   and is_f64 are ignored.
 *   SDQH_SS_CHANGE  reads a marker: any field of the table, named by kind / index / is_f64 the way a measure names one.  Row j
 *                   continues iff its marker and row j - 1's would tie as a sort term on that field under the total order of
 *                   sdqh_sort.h — their stored 64 bits are equal (-0.0 and +0.0 differ, as they do there).  nterms >= npartition;
 *                   gap is ignored.
 *
 * THE COLUMNS.  Every column is over the row's WHOLE session, look-ahead included: every row of a session gets the same bits
 * (SDQH_SS_ROW apart), and sessions look past `limit`, as frames do.  SUM, COUNT, MIN, MAX and AVG follow the rules of
 * sdqh_sort_groups.h word for word, a session in the place of a group: integer sums wrap in two's complement, COUNT is int64, the
 * NaN rule for MIN / MAX holds, a double SUM is IEEE additions of exactly the session's rows in one association fixed for a given
 * input, geometry and output shape — no atomics, two calls give identical bits, nothing is added and later subtracted, no row of
 * another session enters — within |sum^ - sum| <= g(m) * sum|v|, m the session's rows.  AVG is that sum (an integer one converted
 * once) divided by the row count, one IEEE division, as in sdqh_sort_exclude.h.  FIRST and LAST are the measure's 64 bits at the
 * session's first and last sorted row: of the order column they are the session's start and end.  SDQH_SS_NUMBER is the session's
 * 1-based number inside its partition, SDQH_SS_ROW the row's 1-based number inside its session, both int64.
 *
 * TWO OUTPUT SHAPES.
 *   per_session == 0   the first min(limit, n) of the n selected rows in sorted order, out_cols[c * capacity + j] beside row j.
 *                      Sizes, the count-only call (every out array NULL: *out_n = min(limit, n), nothing is sorted) and
 *                      SDQH_ERR_OVERFLOW are sdqh_table_window_slide's; there is no read-back beyond that call's.
 *   per_session == 1   one row per session, in sorted order: the session's first row's key / payload / values / hits — its
 *                      representative, as in sdqh_table_grouping_sets — and its columns.  *out_n = min(limit, sessions).  The count
 *                      is known only behind the sort (one more read-back, as there): the count-only call works with every out
 *                      array NULL, a capacity below the count is SDQH_ERR_OVERFLOW with the count in *out_n and no array
 *                      written, more than 2^32 - 1 sessions SDQH_ERR_UNSUPPORTED.  SDQH_SS_ROW is SDQH_ERR_INVALID in this shape.
 * out_cols NULL: rows only, no column is computed.  ncols == 0 is allowed: the sorted rows, or the sessions' representatives.
 * Slots at or past *out_n are not written.  An empty selection gives 0 rows.
 *
 * ERRORS, in this order.  Read off the caller's structs alone, SDQH_ERR_INVALID: rule NULL or an unknown rule, per_session outside
 * 0 / 1, ncols < 0 or > SDQH_SS_MAX_COLS, ncols > 0 without cols, an unknown op, SDQH_SS_ROW with per_session == 1, for SDQH_SS_GAP
 * nterms < npartition + 1, a ranks column on the gap term, a negative or non-finite gap, and the argument errors of
 * sdqh_table_window.  Then SDQH_ERR_UNSUPPORTED for a bitmap-only table or a compile-only context.  Then what needs the table,
 * SDQH_ERR_INVALID again: a term, a measure or the marker naming a field the table does not have, is_f64 on a SDQH_SORT_KEY /
 * SDQH_SORT_HITS measure or marker, a term that derives from a double.  On any error nothing is written, *out_n included (the
 * overflow's count apart). */
int sdqh_table_sessions(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* terms,
                        const sdqh_session_rule* rule, int per_session, int ncols, const sdqh_session_col* cols, int64_t limit, int64_t capacity,
                        int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits,
                        int64_t* out_cols /* ncols x capacity, 64 bits each; may be NULL */, int64_t* out_n);
/* What the tests size their cases from: the tile every pass shares with the window passes. */
int sdqh_sessions_geometry(sdqh_ctx* ctx, int64_t* tile_rows);

#ifdef __cplusplus
}
#endif
#endif
