// sdqh_extrema.hip — MIN / MAX per entry of an accumulating table and over a column (include/sdqh_extrema.h).
//
// The accumulators of a table are doubles summed with atomic adds.  An extremum reuses the same 8 bytes between
// sdqh_table_extrema_begin and _end as a uint64 holding sort_bits(value) — the order-preserving map sdqh_table_topk and the
// ordering extension use, reversed for MIN — folded with an unsigned 64-bit atomic maximum (native on gfx950, no CAS loop):
//
//   k_ext_slots<false>  _begin: the named slots of every staged entry = 0, the identity (no non-NaN value encodes to 0)
//   k_ext_fold<NS>      the hot path: key column and NS value columns streamed with 16-byte loads (two rows per lane, 512 per
//                       workgroup step, grid-stride); per row table_find -> entry -> encoded values; then the device probe_drain uses
//                       for sums: rows of one entry standing next to one another (lineitem by order key) are combined by a
//                       segmented scan over head flags — max instead of add, the hit count still added — and only the last row of
//                       a run issues the atomics.  A lane holds two consecutive rows: the scan runs over the lanes' CARRIES (the run
//                       that ends at a lane's second row), a lane's first row takes the carry of the lane below, so the scan is in
//                       row order and a run costs one atomic per slot wherever it starts and ends inside a wave.
//   k_ext_slots<true>   _end: the slots decoded back to doubles (0 -> quiet NaN)
//   k_col_extrema       both extrema and the count of non-NaN values of a column: per lane, per wave (shuffles), one atomic pair per
//                       workgroup into a block the host reads
//
// Nothing here has a counterpart in the reference (its aggregates are sums).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#define SDQH_DECLS_ONLY 1            // argument structs and device helpers of the kernel header, not a second copy of its kernels
#include "sdqh_host.hpp"
#include "sdqh_extrema.h"

using namespace sdqh_host;


namespace {

constexpr int EXT_ROWS = TPB * ROWS_PER_LOAD;                  // rows a workgroup takes per step: one 16-byte load per lane and column
constexpr int64_t EXT_INT_EXACT = (int64_t)1 << 53;            // integers up to here are doubles exactly
constexpr unsigned long long EXT_QNAN = 0x7FF8000000000000ull;

struct DevExtSlots { int32_t slot[SDQH_TUPLE_MAX_VALUES], is_min[SDQH_TUPLE_MAX_VALUES]; int32_t n, _pad; };
struct DevExtVals { const int64_t* col[SDQH_TUPLE_MAX_VALUES]; int32_t slot[SDQH_TUPLE_MAX_VALUES], is_min[SDQH_TUPLE_MAX_VALUES], is_int[SDQH_TUPLE_MAX_VALUES]; int32_t count_hits, aligned; };

// e(v): 0 for a NaN (skipped: the identity), else sort_bits of the double's bits, reversed for MIN; an integer is taken as the double it equals
__device__ __forceinline__ uint64_t ext_encode(int64_t raw, int is_int, int is_min, bool& big) {
    if (is_int) { big |= (raw > EXT_INT_EXACT) | (raw < -EXT_INT_EXACT); raw = __double_as_longlong((double)raw); }
    const double d = __longlong_as_double(raw);
    return d != d ? 0ull : sort_bits(raw, 1, is_min);
}
__device__ __forceinline__ unsigned long long ext_decode(uint64_t e, int is_min) {
    if (e == 0) return EXT_QNAN;
    const uint64_t u = is_min ? ~e : e;
    return (u >> 63) ? (u ^ (1ull << 63)) : ~u;
}
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int off) { return (uint64_t)__shfl_up((long long)v, off, WAVE); }

// _begin (DECODE false) / _end (DECODE true): the named slots of every staged entry, a wave per stage segment
template <bool DECODE>
__global__ __launch_bounds__(TPB) void k_ext_slots(DevStage st, DevExtSlots es, unsigned long long* __restrict__ status) {
    if (!DECODE && blockIdx.x == 0 && threadIdx.x == 0) *status = 0ull;
    const int seg = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
    if (seg >= st.nseg) return;
    const int64_t base = (int64_t)seg * st.seg_rows;
    const uint32_t count = st.seg_count[seg];
    unsigned long long* __restrict__ acc = reinterpret_cast<unsigned long long*>(st.sacc);
    for (uint32_t i = lane_id(); i < count; i += WAVE) {
        const size_t at = (size_t)(base + i) * st.acc_stride;
#pragma unroll
        for (int s = 0; s < SDQH_TUPLE_MAX_VALUES; ++s) {
            if (s >= es.n) break;
            if (DECODE) acc[at + es.slot[s]] = ext_decode(acc[at + es.slot[s]], es.is_min[s]); else acc[at + es.slot[s]] = 0ull;
        }
    }
}

// the entry (stage row whose accumulators it uses) of a row's key, NO_ROW: the key is not in the table
__device__ __forceinline__ uint32_t ext_entry(const DevTable& tb, int64_t key, uint64_t mask, bool inside) {
    if (!inside) return NO_ROW;
    const int64_t pos = table_find(tb, key, mask);
    if (pos < 0) return NO_ROW;
    uint32_t idx = table_ref(tb, pos);
    if (tb.alias) idx = tb.alias[idx];                     // entries of one group share the first one's accumulators
    return idx;
}

template <int NS>
__global__ __launch_bounds__(TPB) void k_ext_fold(DevTable tb, const int64_t* __restrict__ keycol, DevExtVals ev, int64_t nrows, unsigned long long* __restrict__ status) {
    const int lane = lane_id();
    const uint64_t mask = table_is_direct(tb) ? 0 : tb.hdr->cap_mask;
    const int64_t ntiles = (nrows + EXT_ROWS - 1) / EXT_ROWS;
    unsigned long long* __restrict__ acc = reinterpret_cast<unsigned long long*>(tb.sacc);
    bool big = false;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * EXT_ROWS + (int64_t)threadIdx.x * ROWS_PER_LOAD;
        Pair<int64_t> k, v[NS];
        if (ev.aligned && (tile + 1) * EXT_ROWS <= nrows) {                 // workgroup-uniform: whole tile inside, 16-byte loads
            k = load2<false>(keycol, r, nrows);
#pragma unroll
            for (int s = 0; s < NS; ++s) v[s] = load2<false>(ev.col[s], r, nrows);
        } else {
            k = load2<true>(keycol, r, nrows);
#pragma unroll
            for (int s = 0; s < NS; ++s) v[s] = load2<true>(ev.col[s], r, nrows);
        }
        const uint32_t i0 = ext_entry(tb, k.x, mask, r < nrows), i1 = ext_entry(tb, k.y, mask, r + 1 < nrows);
        const uint32_t c0 = i0 != NO_ROW ? 1u : 0u, c1 = i1 != NO_ROW ? 1u : 0u;
        uint64_t e0[NS], e1[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            e0[s] = c0 ? ext_encode(v[s].x, ev.is_int[s], ev.is_min[s], big) : 0ull;
            e1[s] = c1 ? ext_encode(v[s].y, ev.is_int[s], ev.is_min[s], big) : 0ull;
        }
        // head flags in row order: the lane's first row against the second row of the lane below, its second row against its first
        const uint32_t below1 = __shfl_up(i1, 1, WAVE);
        const bool head0 = lane == 0 || below1 != i0, head1 = i1 != i0;
        // the lane's carry = the run that ends at its second row, scanned over the lanes
        uint32_t ch = (head0 || head1) ? 1u : 0u, cc = head1 ? c1 : c0 + c1;
        uint64_t cv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) cv[s] = head1 ? e1[s] : umax64(e0[s], e1[s]);
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const uint32_t oc = __shfl_up(cc, off, WAVE), oh = __shfl_up(ch, off, WAVE);
            uint64_t ov[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) ov[s] = shfl_up64(cv[s], off);
            if (lane >= off && !ch) {
                cc += oc;
#pragma unroll
                for (int s = 0; s < NS; ++s) cv[s] = umax64(cv[s], ov[s]);
                ch |= oh;
            }
        }
        // what the lane below carries into this lane's first row
        const uint32_t pc = __shfl_up(cc, 1, WAVE);
        uint64_t pv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) pv[s] = shfl_up64(cv[s], 1);
        const uint32_t above0 = __shfl_down(i0, 1, WAVE);
        const bool tail0 = i0 != NO_ROW && head1;                                             // the run ends at the first row
        const bool tail1 = i1 != NO_ROW && (lane == WAVE - 1 || above0 != i1);                // ... at the second
        if (tail0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint64_t e = head0 ? e0[s] : umax64(e0[s], pv[s]);
                if (e) atomicMax(&acc[(size_t)i0 * tb.acc_stride + ev.slot[s]], (unsigned long long)e);
            }
            if (ev.count_hits) atomicAdd(&tb.shits[i0], head0 ? c0 : c0 + pc);
        }
        if (tail1) {
#pragma unroll
            for (int s = 0; s < NS; ++s) if (cv[s]) atomicMax(&acc[(size_t)i1 * tb.acc_stride + ev.slot[s]], (unsigned long long)cv[s]);
            if (ev.count_hits) atomicAdd(&tb.shits[i1], cc);
        }
    }
    if (big) atomicOr(status, 1ull);
}

// out[0] = max e_min(v), out[1] = max e_max(v), out[2] = non-NaN values, out[3] |= 1: an integer beyond +-2^53
__global__ __launch_bounds__(TPB) void k_col_extrema(const int64_t* __restrict__ col, int64_t nrows, int is_int, int aligned, unsigned long long* __restrict__ out) {
    __shared__ uint64_t s_lo[TPB / WAVE], s_hi[TPB / WAVE];
    __shared__ unsigned long long s_n[TPB / WAVE];
    const int64_t ntiles = (nrows + EXT_ROWS - 1) / EXT_ROWS;
    uint64_t lo = 0, hi = 0;
    unsigned long long n = 0;
    bool big = false;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r = tile * EXT_ROWS + (int64_t)threadIdx.x * ROWS_PER_LOAD;
        Pair<int64_t> v;
        if (aligned && (tile + 1) * EXT_ROWS <= nrows) v = load2<false>(col, r, nrows); else v = load2<true>(col, r, nrows);
        if (r < nrows) { const uint64_t a = ext_encode(v.x, is_int, 1, big); if (a) { lo = umax64(lo, a); hi = umax64(hi, ext_encode(v.x, is_int, 0, big)); ++n; } }
        if (r + 1 < nrows) { const uint64_t a = ext_encode(v.y, is_int, 1, big); if (a) { lo = umax64(lo, a); hi = umax64(hi, ext_encode(v.y, is_int, 0, big)); ++n; } }
    }
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        lo = umax64(lo, (uint64_t)__shfl_xor((long long)lo, off, WAVE));
        hi = umax64(hi, (uint64_t)__shfl_xor((long long)hi, off, WAVE));
        n += (unsigned long long)__shfl_xor((long long)n, off, WAVE);
    }
    if (lane_id() == 0) { s_lo[threadIdx.x / WAVE] = lo; s_hi[threadIdx.x / WAVE] = hi; s_n[threadIdx.x / WAVE] = n; }
    if (big) atomicOr(&out[3], 1ull);
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TPB / WAVE; ++w) { lo = umax64(lo, s_lo[w]); hi = umax64(hi, s_hi[w]); n += s_n[w]; }
        if (n) { atomicMax(&out[0], (unsigned long long)lo); atomicMax(&out[1], (unsigned long long)hi); atomicAdd(&out[2], n); }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline unsigned tile_grid(sdqh_ctx* ctx, int64_t nrows) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((nrows + EXT_ROWS - 1) / EXT_ROWS, (int64_t)ctx->num_cu * 8));
}
inline int slot_of(const sdqh_table* t, int32_t slot) { for (int i = 0; i < t->ext_nslots; ++i) if (t->ext_slot[i] == slot) return i; return -1; }
int check_table(sdqh_ctx* ctx, const sdqh_table* table, const char* what) {
    if (table->bitmap_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, std::string(what) + ": membership-only table");
    if (!table->accumulate || !table->stage.sacc) return fail(ctx, SDQH_ERR_INVALID, std::string(what) + ": the table carries no accumulators");
    return SDQH_OK;
}

}  // namespace

extern "C" {

int sdqh_extrema_geometry(sdqh_ctx* ctx, int64_t* rows_per_step) {
    if (!ctx || !rows_per_step) return fail(ctx, SDQH_ERR_INVALID, "extrema_geometry: bad arguments");
    *rows_per_step = EXT_ROWS;
    return SDQH_OK;
}

int sdqh_table_extrema_begin(sdqh_ctx* ctx, sdqh_table* table, int nslots, const int32_t* slots, const int32_t* ops) {
    if (!ctx || !table || !slots || !ops || nslots < 1 || nslots > SDQH_TUPLE_MAX_VALUES) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_begin: bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_extrema_begin: compile-only context");
    if (int rc = check_table(ctx, table, "table_extrema_begin")) return rc;
    DevExtSlots es; std::memset(&es, 0, sizeof(es));
    int top = 0;
    for (int i = 0; i < nslots; ++i) {
        if (slots[i] < 0 || slots[i] >= table->stage.acc_stride) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_begin: the table's entries have no such slot");
        if (ops[i] != SDQH_EXT_MIN && ops[i] != SDQH_EXT_MAX) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_begin: unknown operation");
        for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_begin: a slot named twice");
        es.slot[i] = slots[i]; es.is_min[i] = ops[i] == SDQH_EXT_MIN ? 1 : 0;
        top = std::max(top, slots[i] + 1);
    }
    es.n = nslots;
    (void)hipSetDevice(ctx->device);
    if (!table->ext_status) {
        table->ext_status = static_cast<unsigned long long*>(tb_alloc(ctx, table, 64));
        if (!table->ext_status) return fail(ctx, SDQH_ERR_NOMEM, "table_extrema_begin: out of device memory");
    }
    call_begin(ctx);
    if (int rc = index_ensure(ctx, table)) return rc;
    table->compact_valid = false;
    table->nv = std::max(table->nv, top);
    const unsigned grid = (unsigned)std::max(1, (table->stage.nseg + TPB / WAVE - 1) / (TPB / WAVE));
    LAUNCH(ctx, "k_ext_begin", k_ext_slots<false>, grid, table->stage, es, table->ext_status);
    call_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SDQH_ERR_DEVICE, std::string("table_extrema_begin launch: ") + hipGetErrorString(e));
    table->ext_open = true; table->ext_nslots = nslots;
    for (int i = 0; i < nslots; ++i) { table->ext_slot[i] = slots[i]; table->ext_op[i] = ops[i]; }
    return SDQH_OK;
}

int sdqh_table_extrema_fold(sdqh_ctx* ctx, sdqh_table* table, int64_t nrows, const sdqh_column* key, int nslots, const int32_t* slots,
                            const sdqh_column* const* vals, const int32_t* val_is_f64, int count_hits) {
    if (!ctx || !table || nrows < 0 || !slots || !vals || !val_is_f64 || nslots < 1 || nslots > SDQH_TUPLE_MAX_VALUES) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_fold: bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_extrema_fold: compile-only context");
    if (int rc = check_table(ctx, table, "table_extrema_fold")) return rc;
    if (!table->ext_open) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_fold: no sdqh_table_extrema_begin on this table");
    if (!key || key->dtype != SDQH_I64 || key->nrows < nrows) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_fold: the key must be an I64 column of at least nrows rows");
    DevExtVals ev; std::memset(&ev, 0, sizeof(ev));
    bool aligned = aligned16(key->data);
    for (int i = 0; i < nslots; ++i) {
        const int at = slot_of(table, slots[i]);
        if (at < 0) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_fold: a slot sdqh_table_extrema_begin did not name");
        for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_fold: a slot named twice");
        const sdqh_column* c = vals[i];
        if (!c || (c->dtype != SDQH_I64 && c->dtype != SDQH_F64) || c->nrows < nrows) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_fold: values must be I64 or F64 columns of at least nrows rows");
        ev.col[i] = static_cast<const int64_t*>(c->data);
        ev.slot[i] = slots[i]; ev.is_min[i] = table->ext_op[at] == SDQH_EXT_MIN ? 1 : 0;
        ev.is_int[i] = (c->dtype == SDQH_I64 && !val_is_f64[i]) ? 1 : 0;
        aligned = aligned && aligned16(c->data);
    }
    ev.count_hits = (count_hits && table->dev.shits) ? 1 : 0; ev.aligned = aligned ? 1 : 0;
    table->compact_valid = false;
    if (nrows == 0) return SDQH_OK;
    (void)hipSetDevice(ctx->device);
    call_begin(ctx);
    const unsigned grid = tile_grid(ctx, nrows);
    const int64_t* kc = static_cast<const int64_t*>(key->data);
    ctx->next_model_bytes = nrows * 8 * (1 + nslots);
    switch (nslots) {
        case 1: LAUNCH(ctx, "k_ext_fold", k_ext_fold<1>, grid, table->dev, kc, ev, nrows, table->ext_status); break;
        case 2: LAUNCH(ctx, "k_ext_fold", k_ext_fold<2>, grid, table->dev, kc, ev, nrows, table->ext_status); break;
        case 3: LAUNCH(ctx, "k_ext_fold", k_ext_fold<3>, grid, table->dev, kc, ev, nrows, table->ext_status); break;
        default: LAUNCH(ctx, "k_ext_fold", k_ext_fold<4>, grid, table->dev, kc, ev, nrows, table->ext_status); break;
    }
    call_end(ctx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SDQH_ERR_DEVICE, std::string("table_extrema_fold launch: ") + hipGetErrorString(e));
    return SDQH_OK;
}

int sdqh_table_extrema_end(sdqh_ctx* ctx, sdqh_table* table) {
    if (!ctx || !table) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_end: bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_extrema_end: compile-only context");
    if (int rc = check_table(ctx, table, "table_extrema_end")) return rc;
    if (!table->ext_open) return fail(ctx, SDQH_ERR_INVALID, "table_extrema_end: no sdqh_table_extrema_begin on this table");
    if (ctx->capturing) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_extrema_end: waits for the device, cannot be recorded into a plan graph");
    DevExtSlots es; std::memset(&es, 0, sizeof(es));
    es.n = table->ext_nslots;
    for (int i = 0; i < es.n; ++i) { es.slot[i] = table->ext_slot[i]; es.is_min[i] = table->ext_op[i] == SDQH_EXT_MIN ? 1 : 0; }
    (void)hipSetDevice(ctx->device);
    table->ext_open = false;
    table->compact_valid = false;
    call_begin(ctx);
    const unsigned grid = (unsigned)std::max(1, (table->stage.nseg + TPB / WAVE - 1) / (TPB / WAVE));
    LAUNCH(ctx, "k_ext_end", k_ext_slots<true>, grid, table->stage, es, table->ext_status);
    call_end(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->result_host, table->ext_status, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    unsigned long long status = 0;
    std::memcpy(&status, ctx->result_host, 8);
    if (status) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_extrema_end: an integer value beyond +-2^53 is not a double exactly");
    return SDQH_OK;
}

int sdqh_column_extrema(sdqh_ctx* ctx, int64_t nrows, const sdqh_column* col, int is_f64, double* out_min, double* out_max, int64_t* out_count) {
    if (!ctx || nrows < 0 || !out_min || !out_max || !out_count) return fail(ctx, SDQH_ERR_INVALID, "column_extrema: bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "column_extrema: compile-only context");
    if (!col || (col->dtype != SDQH_I64 && col->dtype != SDQH_F64) || col->nrows < nrows) return fail(ctx, SDQH_ERR_INVALID, "column_extrema: needs an I64 or F64 column of at least nrows rows");
    if (ctx->capturing) return fail(ctx, SDQH_ERR_UNSUPPORTED, "column_extrema: waits for the device, cannot be recorded into a plan graph");
    unsigned long long h[4] = {0, 0, 0, 0};
    if (nrows > 0) {
        (void)hipSetDevice(ctx->device);
        unsigned long long* out = static_cast<unsigned long long*>(pool_alloc(ctx, 256));
        if (!out) return fail(ctx, SDQH_ERR_NOMEM, "column_extrema: out of device memory");
        call_begin(ctx);
        hipError_t e = hipMemsetAsync(out, 0, 32, ctx->stream);
        if (e == hipSuccess) {
            const int is_int = (col->dtype == SDQH_I64 && !is_f64) ? 1 : 0;
            ctx->next_model_bytes = nrows * 8;
            LAUNCH(ctx, "k_col_extrema", k_col_extrema, tile_grid(ctx, nrows), static_cast<const int64_t*>(col->data), nrows, is_int, aligned16(col->data) ? 1 : 0, out);
            call_end(ctx);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->result_host, out, 32, hipMemcpyDeviceToHost, ctx->stream);
        const int rc = e == hipSuccess ? sync_stream(ctx) : fail(ctx, SDQH_ERR_DEVICE, std::string("column_extrema: ") + hipGetErrorString(e));
        pool_free(ctx, out);
        if (rc) return rc;
        std::memcpy(h, ctx->result_host, sizeof(h));
    }
    if (h[3]) return fail(ctx, SDQH_ERR_UNSUPPORTED, "column_extrema: an integer value beyond +-2^53 is not a double exactly");
    const unsigned long long qnan = EXT_QNAN;
    unsigned long long lo = qnan, hi = qnan;
    if (h[2]) {                                                   // (the decode of k_ext_slots, on the host)
        const uint64_t a = ~h[0], b = h[1];
        lo = (a >> 63) ? (a ^ (1ull << 63)) : ~a;
        hi = (b >> 63) ? (b ^ (1ull << 63)) : ~b;
    }
    std::memcpy(out_min, &lo, 8); std::memcpy(out_max, &hi, 8);
    *out_count = (int64_t)h[2];
    return SDQH_OK;
}

}  // extern "C"
