// sdqh_sort.hip — ORDER BY over the entries of a table (include/sdqh_sort.h): a stable LSD radix sort on the device.
//
// sdqh_table_topk (sdqh_hip.hip) selects at most 128 rows by at most three columns through a 1024-slot LDS buffer; everything
// beyond that used to be compacted, copied out and ordered on the host.  Here the whole selection is ordered where it lies:
//
//   k_sort_count / k_sort_scan / k_sort_gather / k_sort_keys
//                     the selected entries (hits >= min_hits, owner rows only — the predicate of k_compact_count / k_topk_scan) as
//                     32-bit stage-row references IN STAGE ORDER (count per segment -> exclusive scan -> place: no atomic cursor,
//                     because stage order = build-row order is the tie-break), the transformed uint64 key of every sort column
//                     beside them (top_sort_value: the order-preserving map sdqh_table_topk uses), and per column the AND and the OR
//                     of its keys: OR & ~AND = the bits that differ between any two entries (= the OR over entries of key ^ first key)
//   (host)            one small copy: n and those masks.  An 8-bit digit none of whose bits varies orders nothing: its pass is
//                     skipped — hit counts, date codes and small integers cost one or two passes, not eight
//   k_sort_small      n <= SORT_SMALL: every pass in LDS by one workgroup, one launch
//   k_sort_hist / k_sort_bins / k_sort_scatter
//                     larger n, per pass: a wave owns a tile of SORT_TILE consecutive positions; 256 digit counts per tile ->
//                     exclusive scan over (digit, tile), digit-major (one workgroup per digit, then the 256 digit totals inside the
//                     scatter) -> every wave places its tile 64 positions at a time in order: a lane's place = its digit's cursor (LDS,
//                     per wave) + the lanes below it holding the same digit (eight 64-bit ballots).  Equal digits keep their order
//                     across lanes (lane mask), batches (the cursor), tiles and workgroups (the scan): the sort is stable, so passes
//                     run from the last sort column to the first, low digit to high, and what is left of every tie is stage order.
//                     One form for every n a stage can hold (references are 32 bits): no second scan level.
//   k_sort_emit       the first min(limit, n) rows in order, columns as sdqh_table_compact lays them out
//
// What is sorted is a permutation of the gathered positions; a pass reads its digit through it (8-byte gathers from arrays that
// stay in L2 / Infinity Cache at the sizes a query result has) and moves 4 bytes per entry, whatever the number of sort columns.
// Nothing here has a counterpart in the reference, whose results are unordered sets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#define SDQH_DECLS_ONLY 1            // argument structs and device helpers of the kernel header, not a second copy of its kernels
#include "sdqh_host.hpp"
#include "sdqh_sort.h"

using namespace sdqh_host;

#define HIP_TRYS(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return fail(ctx, SDQH_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define LAUNCH(ctx, name, kernel, grid, ...)                                         \
    do { KernelScope _ks(ctx, name); hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(TPB), 0, (ctx)->stream, __VA_ARGS__); } while (0)

namespace {

constexpr int SORT_SMALL = 1024;                     // largest n the single-workgroup kernel takes
constexpr int SORT_SMALL_WAVE = SORT_SMALL / (TPB / WAVE);
constexpr int SORT_TILE = 512;                       // positions a wave counts / places per pass (a result of 100 K rows still spreads over 200 waves)
constexpr int SORT_INFO = 1 + 2 * SDQH_SORT_MAX_KEYS;      // [n | AND of the keys per column | OR of the keys per column]

struct DevSortSpec { DevSortKey key[SDQH_SORT_MAX_KEYS]; int32_t nsort, _pad; };
struct DevSortOut { int64_t* keys; int64_t* pay[SDQH_MAX_PAYLOAD]; double* val[SDQH_TUPLE_MAX_VALUES]; int64_t* hits; int32_t npay, nval; };

// the selection predicate of k_compact_count / k_topk_scan
__device__ __forceinline__ bool sort_keeps(const DevTable& t, const DevStage& st, int64_t idx, bool inside, uint32_t min_hits, bool dups, uint64_t mask, uint32_t& hits) {
    hits = 0;
    if (!inside) return false;
    hits = st.shits ? st.shits[idx] : 0u;
    if (hits < min_hits) return false;
    return !dups || stage_row_owns(st, t, idx, mask);
}

// inclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); every thread calls it
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* s_part) {
    s_part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {
        const uint32_t a = (int)threadIdx.x >= off ? s_part[threadIdx.x - off] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += a;
        __syncthreads();
    }
    return s_part[threadIdx.x];
}

// 1. selected entries per segment
__global__ __launch_bounds__(TPB) void k_sort_count(DevTable t, DevStage st, uint32_t min_hits, uint32_t* __restrict__ seg_kept) {
    const int seg = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
    if (seg >= st.nseg) return;
    const bool dups = t.hdr->has_dups != 0;
    const uint64_t mask = (table_is_direct(t) || !dups) ? 0 : t.hdr->cap_mask;
    const int64_t base = (int64_t)seg * st.seg_rows;
    const uint32_t count = st.seg_count[seg];
    uint32_t n = 0;
    for (uint32_t i0 = 0; i0 < count; i0 += WAVE) {
        const uint32_t i = i0 + lane_id();
        uint32_t hits;
        const bool keep = sort_keeps(t, st, base + i, i < count, min_hits, dups, mask, hits);
        n += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane_id() == 0) seg_kept[seg] = n;
}
// 2. one workgroup: exclusive scan of the per-segment counts, in place; info = [n | ~0 x 8 | 0 x 8]
__global__ __launch_bounds__(TPB) void k_sort_scan(uint32_t* __restrict__ seg_kept, int nseg, unsigned long long* __restrict__ info) {
    __shared__ uint32_t s_part[TPB];
    const int per = (nseg + TPB - 1) / TPB;
    const int b0 = threadIdx.x * per, b1 = min(nseg, b0 + per);
    uint32_t sum = 0;                                                 // (a build side holds at most 2^32 - 2 rows: 32 bits are enough)
    for (int b = b0; b < b1; ++b) sum += seg_kept[b];
    const uint32_t incl = block_scan_incl(sum, s_part);
    if (threadIdx.x == TPB - 1) info[0] = incl;
    if (threadIdx.x < SDQH_SORT_MAX_KEYS) { info[1 + threadIdx.x] = ~0ull; info[1 + SDQH_SORT_MAX_KEYS + threadIdx.x] = 0ull; }
    uint32_t run = incl - sum;
    for (int b = b0; b < b1; ++b) { const uint32_t v = seg_kept[b]; seg_kept[b] = run; run += v; }
}
// 3. place: the references in stage order
__global__ __launch_bounds__(TPB) void k_sort_gather(DevTable t, DevStage st, uint32_t min_hits, const uint32_t* __restrict__ seg_off, uint32_t* __restrict__ refs) {
    const int seg = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
    if (seg >= st.nseg) return;
    const bool dups = t.hdr->has_dups != 0;
    const uint64_t mask = (table_is_direct(t) || !dups) ? 0 : t.hdr->cap_mask;
    const int64_t base = (int64_t)seg * st.seg_rows;
    const uint32_t count = st.seg_count[seg];
    const uint64_t lt = lanemask_lt();
    size_t at0 = seg_off[seg];
    for (uint32_t i0 = 0; i0 < count; i0 += WAVE) {
        const uint32_t i = i0 + lane_id();
        uint32_t hits;
        const bool keep = sort_keeps(t, st, base + i, i < count, min_hits, dups, mask, hits);
        const uint64_t b = __ballot(keep);
        if (keep) refs[at0 + (size_t)__popcll(b & lt)] = (uint32_t)(base + i);
        at0 += (size_t)__popcll(b);
    }
}
// 4. one sort column's transformed keys beside the references (a launch per column), and the AND / OR of them — the order of those
// does not matter: atomics.  n is the device's (info[0]).
__global__ __launch_bounds__(TPB) void k_sort_keys(DevStage st, DevSortKey sk, const uint32_t* __restrict__ refs, uint64_t* __restrict__ key, unsigned long long* __restrict__ info, int col) {
    const uint64_t n = info[0];
    uint64_t all = ~0ull, any = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
        const int64_t idx = (int64_t)refs[i];
        const uint64_t k = top_sort_value(sk, st, idx, st.shits ? st.shits[idx] : 0u);
        key[i] = k; all &= k; any |= k;
    }
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { all &= (uint64_t)__shfl_xor((long long)all, off, WAVE); any |= (uint64_t)__shfl_xor((long long)any, off, WAVE); }
    if (lane_id() == 0 && (all != ~0ull || any != 0ull)) { atomicAnd(&info[1 + col], (unsigned long long)all); atomicOr(&info[1 + SDQH_SORT_MAX_KEYS + col], (unsigned long long)any); }
}

// One wave's 64 positions of a pass placed: lane's place = cursor of its digit + lanes below it with the same digit; the lowest lane
// of each digit then moves the cursor (a wave's LDS accesses keep their order).  at: this wave's 256 cursors.
__device__ __forceinline__ uint32_t wave_place(uint32_t* at, bool live, uint32_t d, uint64_t lt) {
    uint64_t same = __ballot(live);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) { const uint64_t m = __ballot((d >> bit) & 1u); same &= ((d >> bit) & 1u) ? m : ~m; }
    uint32_t place = 0;
    if (live) place = at[d] + (uint32_t)__popcll(same & lt);
    if (live && !(same & lt)) at[d] += (uint32_t)__popcll(same);
    return place;
}

// n <= SORT_SMALL: all passes by one workgroup, the permutation in LDS.  The passes are read off the masks in `info` (the host
// launches this kernel only when at least one digit varies); wave w owns positions [w * 256, w * 256 + 256).
__global__ __launch_bounds__(TPB) void k_sort_small(const uint64_t* __restrict__ keys, size_t key_stride, int nsort, uint32_t n,
                                                   const unsigned long long* __restrict__ info, uint32_t* __restrict__ perm_out) {
    __shared__ uint32_t s_perm[2][SORT_SMALL];
    __shared__ uint32_t s_at[TPB / WAVE][256];
    __shared__ uint32_t s_part[TPB];
    const int wv = (int)(threadIdx.x / WAVE), lane = lane_id();
    const uint64_t lt = lanemask_lt();
    const int r0 = wv * SORT_SMALL_WAVE, r1 = min((int)n, r0 + SORT_SMALL_WAVE);
    for (int i = threadIdx.x; i < (int)n; i += TPB) s_perm[0][i] = (uint32_t)i;
    int cur = 0;
    __syncthreads();
    for (int c = nsort - 1; c >= 0; --c) {
        const uint64_t vary = info[1 + SDQH_SORT_MAX_KEYS + c] & ~info[1 + c];
        const uint64_t* __restrict__ key = keys + (size_t)c * key_stride;
        for (int shift = 0; shift < 64; shift += 8) {
            if (((vary >> shift) & 255ull) == 0) continue;                    // uniform: every thread reads the same words
            s_at[wv][lane] = 0; s_at[wv][lane + 64] = 0; s_at[wv][lane + 128] = 0; s_at[wv][lane + 192] = 0;
            __syncthreads();
            for (int r = r0 + lane; r < r1; r += WAVE) atomicAdd(&s_at[wv][(uint32_t)(key[s_perm[cur][r]] >> shift) & 255u], 1u);
            __syncthreads();
            // thread d: digit d's count in every wave -> its cursors, digit-major
            uint32_t cnt[TPB / WAVE], tot = 0;
#pragma unroll
            for (int w = 0; w < TPB / WAVE; ++w) { cnt[w] = s_at[w][threadIdx.x]; tot += cnt[w]; }
            uint32_t run = block_scan_incl(tot, s_part) - tot;
#pragma unroll
            for (int w = 0; w < TPB / WAVE; ++w) { s_at[w][threadIdx.x] = run; run += cnt[w]; }
            __syncthreads();
            for (int b = r0; b < r1; b += WAVE) {
                const int r = b + lane;
                const bool live = r < r1;
                const uint32_t g = live ? s_perm[cur][r] : 0u;
                const uint32_t d = live ? (uint32_t)(key[g] >> shift) & 255u : 0u;
                const uint32_t place = wave_place(s_at[wv], live, d, lt);
                if (live && place < (uint32_t)SORT_SMALL) s_perm[cur ^ 1][place] = g;
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    for (int i = threadIdx.x; i < (int)n; i += TPB) perm_out[i] = s_perm[cur][i];
}

// larger n, per pass.  perm == nullptr: the identity (the first pass).  hist[d * ntiles + tile].
__global__ __launch_bounds__(TPB) void k_sort_hist(const uint64_t* __restrict__ key, const uint32_t* __restrict__ perm, uint32_t n, int shift,
                                                  uint32_t* __restrict__ hist, uint32_t ntiles) {
    __shared__ uint32_t s_cnt[TPB / WAVE][256];
    const int wv = (int)(threadIdx.x / WAVE), lane = lane_id();
    for (int d = lane; d < 256; d += WAVE) s_cnt[wv][d] = 0;
    const uint32_t w = blockIdx.x * (TPB / WAVE) + wv;
    if (w >= ntiles) return;
    const uint64_t r0 = (uint64_t)w * SORT_TILE, r1 = min((uint64_t)n, r0 + SORT_TILE);
    for (uint64_t r = r0 + lane; r < r1; r += WAVE) { const uint32_t g = perm ? perm[r] : (uint32_t)r; atomicAdd(&s_cnt[wv][g < n ? (uint32_t)(key[g] >> shift) & 255u : 0u], 1u); }
    for (int d = lane; d < 256; d += WAVE) hist[(size_t)d * ntiles + w] = s_cnt[wv][d];
}
// workgroup d: exclusive scan of digit d's counts over the tiles, in place; its total -> bin_total[d]
__global__ __launch_bounds__(TPB) void k_sort_bins(uint32_t* __restrict__ hist, uint32_t ntiles, uint32_t* __restrict__ bin_total) {
    __shared__ uint32_t s_part[TPB];
    uint32_t* __restrict__ row = hist + (size_t)blockIdx.x * ntiles;
    const uint32_t per = (ntiles + TPB - 1) / TPB;
    const uint64_t b0 = (uint64_t)threadIdx.x * per, b1 = min((uint64_t)ntiles, b0 + per);
    uint32_t sum = 0;
    for (uint64_t b = b0; b < b1; ++b) sum += row[b];
    const uint32_t incl = block_scan_incl(sum, s_part);
    if (threadIdx.x == TPB - 1) bin_total[blockIdx.x] = incl;
    uint32_t run = incl - sum;
    for (uint64_t b = b0; b < b1; ++b) { const uint32_t v = row[b]; row[b] = run; run += v; }
}
__global__ __launch_bounds__(TPB) void k_sort_scatter(const uint64_t* __restrict__ key, const uint32_t* __restrict__ perm, uint32_t n, int shift,
                                                     const uint32_t* __restrict__ hist, const uint32_t* __restrict__ bin_total, uint32_t ntiles,
                                                     uint32_t* __restrict__ perm_out) {
    __shared__ uint32_t s_at[TPB / WAVE][256];
    __shared__ uint32_t s_part[TPB];
    const int wv = (int)(threadIdx.x / WAVE), lane = lane_id();
    const uint32_t total = bin_total[threadIdx.x];
    const uint32_t first = block_scan_incl(total, s_part) - total;            // where digit threadIdx.x starts
    __syncthreads();
    s_part[threadIdx.x] = first;
    __syncthreads();
    const uint32_t w = blockIdx.x * (TPB / WAVE) + wv;
    if (w >= ntiles) return;
    for (int d = lane; d < 256; d += WAVE) s_at[wv][d] = s_part[d] + hist[(size_t)d * ntiles + w];
    const uint64_t lt = lanemask_lt();
    const uint64_t r0 = (uint64_t)w * SORT_TILE, r1 = min((uint64_t)n, r0 + SORT_TILE);
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const uint32_t g = live ? (perm ? perm[r] : (uint32_t)r) : 0u;
        const uint32_t d = live && g < n ? (uint32_t)(key[g] >> shift) & 255u : 0u;
        const uint32_t place = wave_place(s_at[wv], live, d, lt);
        if (live && place < n) perm_out[place] = g;
    }
}

// rows perm[0 .. m) of the gathered entries (perm == nullptr: the gathered order itself); o's arrays hold m rows each
__global__ __launch_bounds__(TPB) void k_sort_emit(DevStage st, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, uint32_t n, uint32_t m, DevSortOut o) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t g = perm ? perm[j] : (uint32_t)j;
        if (g >= n) continue;                                            // (a permutation of [0, n): never taken)
        const int64_t idx = (int64_t)refs[g];
        if (o.keys) o.keys[j] = st.key[idx];
#pragma unroll
        for (int p = 0; p < SDQH_MAX_PAYLOAD; ++p) if (p < o.npay && o.pay[p]) o.pay[p][j] = st.pay[p][idx];
#pragma unroll
        for (int v = 0; v < SDQH_TUPLE_MAX_VALUES; ++v) if (v < o.nval && o.val[v]) o.val[v][j] = st.sacc[(size_t)idx * st.acc_stride + v];
        if (o.hits) o.hits[j] = st.shits ? (int64_t)st.shits[idx] : 0;
    }
}

struct Scratch {                                     // pool blocks of one call, returned on every way out
    sdqh_ctx* ctx; void* p[3] = {nullptr, nullptr, nullptr};
    explicit Scratch(sdqh_ctx* c) : ctx(c) {}
    ~Scratch() { for (void* q : p) if (q) pool_free(ctx, q); }
};
inline size_t round_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int sdqh_sort_geometry(sdqh_ctx* ctx, int64_t* single_wg_max, int64_t* tile_rows, int64_t* second_level_rows) {
    if (!ctx || !single_wg_max || !tile_rows || !second_level_rows) return fail(ctx, SDQH_ERR_INVALID, "sort_geometry: bad arguments");
    *single_wg_max = SORT_SMALL; *tile_rows = SORT_TILE; *second_level_rows = 0;
    return SDQH_OK;
}

int sdqh_table_sorted(sdqh_ctx* ctx, const sdqh_table* ctable, int64_t min_hits, int64_t limit, int nsort, const sdqh_sort_key* sort,
                      int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_n) {
    sdqh_table* table = const_cast<sdqh_table*>(ctable);
    if (!ctx || !table || !out_n || !sort || nsort < 1 || nsort > SDQH_SORT_MAX_KEYS || limit < 1 || capacity < 0)
        return fail(ctx, SDQH_ERR_INVALID, "table_sorted: bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_sorted: compile-only context");
    if (table->bitmap_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "table_sorted: bitmap-only table");
    (void)hipSetDevice(ctx->device);
    DevSortSpec spec; std::memset(&spec, 0, sizeof(spec));
    spec.nsort = nsort;
    const int nv = table->accumulate ? table->nv : 0;
    for (int i = 0; i < nsort; ++i) {
        const sdqh_sort_key& sk = sort[i];
        const bool ok = (sk.kind == SDQH_SORT_KEY) || (sk.kind == SDQH_SORT_PAYLOAD && sk.index >= 0 && sk.index < table->npay) ||
                        (sk.kind == SDQH_SORT_VALUE && sk.index >= 0 && sk.index < nv) || (sk.kind == SDQH_SORT_HITS && table->accumulate);
        if (!ok) return fail(ctx, SDQH_ERR_INVALID, "table_sorted: sort key names a field the table does not have");
        spec.key[i].kind = sk.kind; spec.key[i].index = sk.index; spec.key[i].desc = sk.descending ? 1 : 0;
        spec.key[i].is_f64 = sk.kind == SDQH_SORT_VALUE ? 1 : (sk.kind == SDQH_SORT_PAYLOAD ? (sk.is_f64 ? 1 : 0) : 0);
    }
    call_begin(ctx);
    if (int rc = index_ensure(ctx, table)) return rc;
    Scratch scratch(ctx);
    // block 0: [segment offsets | info | references | keys per column], sized for every staged row (the count is the device's)
    const size_t rows = (size_t)std::max<int64_t>(table->nrows_build, 1) + 1;
    const int nseg = table->stage.nseg;
    const size_t seg_bytes = round_up((size_t)std::max(nseg, 1) * 4), info_bytes = round_up(SORT_INFO * 8), ref_bytes = round_up(rows * 4), key_bytes = round_up(rows * 8);
    char* blob = static_cast<char*>(scratch.p[0] = pool_alloc(ctx, seg_bytes + info_bytes + ref_bytes + key_bytes * (size_t)nsort));
    if (!blob) return fail(ctx, SDQH_ERR_NOMEM, "table_sorted: out of device memory");
    uint32_t* seg_off = reinterpret_cast<uint32_t*>(blob);
    unsigned long long* info = reinterpret_cast<unsigned long long*>(blob + seg_bytes);
    uint32_t* refs = reinterpret_cast<uint32_t*>(blob + seg_bytes + info_bytes);
    uint64_t* keys = reinterpret_cast<uint64_t*>(blob + seg_bytes + info_bytes + ref_bytes);
    const size_t key_stride = key_bytes / 8;
    const uint32_t mh = (uint32_t)std::min<int64_t>(std::max<int64_t>(min_hits, 0), 0xFFFFFFFFll);
    const unsigned seg_grid = (unsigned)std::max(1, (nseg + TPB / WAVE - 1) / (TPB / WAVE));
    LAUNCH(ctx, "k_sort_count", k_sort_count, seg_grid, table->dev, table->stage, mh, seg_off);
    LAUNCH(ctx, "k_sort_scan", k_sort_scan, 1, seg_off, nseg, info);
    LAUNCH(ctx, "k_sort_gather", k_sort_gather, seg_grid, table->dev, table->stage, mh, seg_off, refs);
    const unsigned key_grid = (unsigned)std::max<size_t>(1, std::min<size_t>((rows + TPB - 1) / TPB, (size_t)ctx->num_cu * 8));
    for (int c = 0; c < nsort; ++c) LAUNCH(ctx, "k_sort_keys", k_sort_keys, key_grid, table->stage, spec.key[c], refs, keys + (size_t)c * key_stride, info, c);
    HIP_TRYS(ctx, hipMemcpyAsync(ctx->result_host, info, SORT_INFO * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    unsigned long long h[SORT_INFO];
    std::memcpy(h, ctx->result_host, sizeof(h));
    const int64_t n = (int64_t)h[0], m = std::min<int64_t>(limit, n);
    *out_n = m;
    if (!out_keys && !out_payload && !out_values && !out_hits) { call_end(ctx); return SDQH_OK; }      // count-only call
    if (m > capacity) { call_end(ctx); return fail(ctx, SDQH_ERR_OVERFLOW, "table_sorted: capacity too small"); }
    if (m == 0) { call_end(ctx); return SDQH_OK; }
    // the passes: last column first, low digit first; a digit whose bits are the same in every key orders nothing
    int pass_col[8 * SDQH_SORT_MAX_KEYS], pass_shift[8 * SDQH_SORT_MAX_KEYS], npass = 0;
    if (n > 1) for (int c = nsort - 1; c >= 0; --c) {
        const uint64_t vary = h[1 + SDQH_SORT_MAX_KEYS + c] & ~h[1 + c];
        for (int shift = 0; shift < 64; shift += 8) if ((vary >> shift) & 255ull) { pass_col[npass] = c; pass_shift[npass] = shift; ++npass; }
    }
    // block 1: [permutation x 2 | digit counts per tile | digit totals]; block 2: the result rows
    const uint32_t un = (uint32_t)n, um = (uint32_t)m;
    const uint32_t ntiles = (uint32_t)((n + SORT_TILE - 1) / SORT_TILE);
    const bool small = n <= SORT_SMALL;
    const uint32_t* perm = nullptr;
    if (npass) {
        const size_t perm_bytes = round_up((size_t)n * 4), hist_bytes = small ? 0 : round_up((size_t)ntiles * 256 * 4);
        char* b1 = static_cast<char*>(scratch.p[1] = pool_alloc(ctx, perm_bytes * (small ? 1 : 2) + hist_bytes + 1024));
        if (!b1) return fail(ctx, SDQH_ERR_NOMEM, "table_sorted: out of device memory");
        uint32_t* pa = reinterpret_cast<uint32_t*>(b1);
        if (small) {
            LAUNCH(ctx, "k_sort_small", k_sort_small, 1, keys, key_stride, nsort, un, info, pa);
            perm = pa;
        } else {
            uint32_t* pb = reinterpret_cast<uint32_t*>(b1 + perm_bytes);
            uint32_t* hist = reinterpret_cast<uint32_t*>(b1 + 2 * perm_bytes);
            uint32_t* bin_total = reinterpret_cast<uint32_t*>(b1 + 2 * perm_bytes + hist_bytes);
            const unsigned tgrid = (ntiles + TPB / WAVE - 1) / (TPB / WAVE);
            for (int p = 0; p < npass; ++p) {
                const uint64_t* key = keys + (size_t)pass_col[p] * key_stride;
                LAUNCH(ctx, "k_sort_hist", k_sort_hist, tgrid, key, perm, un, pass_shift[p], hist, ntiles);
                LAUNCH(ctx, "k_sort_bins", k_sort_bins, 256, hist, ntiles, bin_total);
                LAUNCH(ctx, "k_sort_scatter", k_sort_scatter, tgrid, key, perm, un, pass_shift[p], hist, bin_total, ntiles, pa);
                perm = pa; std::swap(pa, pb);
            }
        }
    }
    const int npay = out_payload ? table->npay : 0, nval = out_values ? nv : 0;
    const int narr = (out_keys ? 1 : 0) + npay + nval + (out_hits ? 1 : 0);
    const size_t nb = (size_t)m * 8, need = nb * (size_t)narr;
    if (narr) {
        char* dev = static_cast<char*>(scratch.p[2] = pool_alloc(ctx, need + 64));
        if (!dev) return fail(ctx, SDQH_ERR_NOMEM, "table_sorted: out of device memory");
        DevSortOut o; std::memset(&o, 0, sizeof(o));
        size_t at = 0;
        if (out_keys) { o.keys = reinterpret_cast<int64_t*>(dev + at); at += nb; }
        for (int p = 0; p < npay; ++p) { o.pay[p] = reinterpret_cast<int64_t*>(dev + at); at += nb; }
        for (int v = 0; v < nval; ++v) { o.val[v] = reinterpret_cast<double*>(dev + at); at += nb; }
        if (out_hits) { o.hits = reinterpret_cast<int64_t*>(dev + at); at += nb; }
        o.npay = npay; o.nval = nval;
        const unsigned egrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + TPB - 1) / TPB, (int64_t)ctx->num_cu * 8));
        LAUNCH(ctx, "k_sort_emit", k_sort_emit, egrid, table->stage, refs, perm, un, um, o);
        call_end(ctx);
        // the rows land in pinned memory in one copy (a copy into pageable memory is several times slower), then one memcpy per array
        if (need > ctx->bulk_bytes && need <= ((size_t)1 << 30)) {
            if (ctx->bulk_host) (void)hipHostFree(ctx->bulk_host);
            ctx->bulk_host = nullptr; ctx->bulk_bytes = 0;
            const size_t want = std::max<size_t>(need * 2, (size_t)8 << 20);
            if (hipHostMalloc(&ctx->bulk_host, want, hipHostMallocDefault) == hipSuccess) ctx->bulk_bytes = want; else (void)hipGetLastError();
        }
        const bool pinned = need <= ctx->bulk_bytes;
        int64_t* dst[2 + SDQH_MAX_PAYLOAD + SDQH_TUPLE_MAX_VALUES]; int nd = 0;
        if (out_keys) dst[nd++] = out_keys;
        for (int p = 0; p < npay; ++p) dst[nd++] = out_payload + (size_t)p * (size_t)capacity;
        for (int v = 0; v < nval; ++v) dst[nd++] = reinterpret_cast<int64_t*>(out_values + (size_t)v * (size_t)capacity);
        if (out_hits) dst[nd++] = out_hits;
        if (pinned) HIP_TRYS(ctx, hipMemcpyAsync(ctx->bulk_host, dev, need, hipMemcpyDeviceToHost, ctx->stream));
        else for (int a = 0; a < nd; ++a) HIP_TRYS(ctx, hipMemcpyAsync(dst[a], dev + (size_t)a * nb, nb, hipMemcpyDeviceToHost, ctx->stream));
        if (int rc = sync_stream(ctx)) return rc;
        if (pinned) for (int a = 0; a < nd; ++a) std::memcpy(dst[a], static_cast<const char*>(ctx->bulk_host) + (size_t)a * nb, nb);
    }
    if (out_values) for (int v = nval; v < SDQH_TUPLE_MAX_VALUES; ++v) std::memset(out_values + (size_t)v * (size_t)capacity, 0, nb);
    return SDQH_OK;
}

}  // extern "C"
