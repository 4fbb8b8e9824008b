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
// One path behind the table entry points — sdqh_table_sorted, sdqh_table_sorted_by (include/sdqh_sort_terms.h), sdqh_table_window
// (include/sdqh_sort_window.h), sdqh_table_window_agg (include/sdqh_sort_frames.h), sdqh_table_window_slide
// (include/sdqh_sort_slide.h), sdqh_table_window_range (include/sdqh_sort_range.h), sdqh_table_window_quantile
// (include/sdqh_sort_quantile.h), sdqh_table_window_exclude (include/sdqh_sort_exclude.h), sdqh_table_grouping_sets
// (include/sdqh_sort_groups.h), sdqh_table_group_distinct (include/sdqh_sort_distinct.h), sdqh_table_group_moments
// (include/sdqh_sort_moments.h), sdqh_table_sessions (include/sdqh_sort_sessions.h) and sdqh_table_window_moments
// (include/sdqh_sort_wmoments.h): select -> passes -> step -> emit -> fetch (ordered_impl, the spine).  What differs between them
// is data, not code: their terms, and ONE step description (SortStep) that the spine hands to one dispatch.  On the host the step
// is a few shared pieces — each a small struct whose take() lays its arrays into the family's scratch block, and a function that
// launches — and the family steps.  The pieces: Tiles (the tiles of a count and the grid that gives each a wave: the one place that
// arithmetic is written), the partition pass (Partitions + partition_pass: the arrays every window family reads its partitions from,
// k_win_heads and of k_win_scan / k_wsl_rows / k_wagg_next those the family names), the filter (rank_filter: k_win_rank ->
// k_sort_scan -> the kept count to the host -> the ways out -> k_win_place; a window filters on its own ranks, quantiles on row
// numbers), the tile fold (tile_fold: k_wagg_tiles -> k_wagg_scan -> k_wagg_run, over partitions, groups or sessions), the frame
// pass (Frames + frame_pass / frame_trees: where ranges, excludes and moments over frames find their data-dependent frames and
// build their fold trees) and the level pass (Levels + level_pass / level_counts / level_sets: the heads and counts of every
// grouping level, the count to the host and the ways out of the steps that return one row per group).  The family steps (step_ranks
// / _frames / _slides / _ranges / _quantiles / _excludes / _groups / _distincts / _moments / _sessions / _wmoments) each lay out
// their scratch blocks, run the pieces above and their own kernels and say where each output column lies.  In front of them the
// entry points share window_enter, measure_set, fold_class, frame_bounds_ok, frame_image and measure_slot.  On the device:
//
//   a TERM            every sort column is a DevSortTerm.  k_sort_keys reads the column (sort_raw) and, for a DERIVED term, takes
//                     field = (uint64(source) / div) % mod + add and a bounds-checked gather through a ranks column in front of
//                     sort_bits; sdqh_table_sorted's keys are terms with no derivation.  sdqh_text_ranks makes such a ranks column of
//                     a text column (k_text_masks / k_text_pack, the passes above, k_rank_count / k_rank_place: see there).
//   a WINDOW          optional (STEP_RANKS).  sdqh_table_window ranks the ordered entries inside PARTITIONS (maximal runs of sorted
//                     positions whose first npartition keys are equal) and keeps the rows whose rank is <= per_limit — ROW_NUMBER /
//                     RANK / DENSE_RANK OVER (PARTITION BY ... ORDER BY ...).  Without one the rank step launches nothing, allocates
//                     nothing, and the emit reads the permutation directly.  With one, between the passes and the emit:
//
//   k_win_heads       a wave owns a tile of SORT_TILE sorted positions: position i reads its keys and those of i - 1 through the
//                     permutation and sets two flags (a byte per position) — part_head: a partition key differs, tie_head: any key
//                     differs, position 0 both — and the wave folds its ballots into the tile's CARRY: {a partition head seen,
//                     positions since the last partition head (no head: the tile's length), position of the last tie head relative
//                     to the partition start, tie heads since the last partition head}
//   k_win_scan        one workgroup: exclusive scan of the carries over the tiles with the segmented-scan operator (win_join: a
//                     right side with a partition head wins, one without adds its length and tie heads to the left side — a tile
//                     with no head at all passes the incoming carry through, longer), in place
//   k_win_rank        the tile again with its carry-in, 64 positions at a time: the three ranks are read off the two ballots and
//                     the running carry (row_number = distance to the last partition head + 1, rank = distance of the last tie head
//                     to it + 1, dense_rank = tie heads between them); the kind asked for is stored per position (32 bits) and
//                     the positions with rank <= per_limit are counted per tile
//   k_sort_scan / k_win_place
//                     those counts scanned over the tiles, then the kept positions placed in order (ballot + lanes below: no atomic
//                     cursor, because order is the contract).  per_limit >= n keeps everything: both are skipped
//   k_sort_emit       then goes through the kept positions and writes the rank column beside the others
//   FRAMES            in a window's place (STEP_FRAMES).  sdqh_table_window_agg (include/sdqh_sort_frames.h) folds a measure column over
//                     frames of the same partitions — SUM / COUNT / MIN / MAX OVER (PARTITION BY ... ORDER BY ... ROWS | RANGE | the
//                     whole partition) — and keeps every row.  Behind k_win_heads, in place of the rank step:
//
//   k_wagg_tiles      a wave per tile: every aggregate's 64-bit element of every position (the measure read through perm -> refs ->
//                     stage once), the tile's carry {the elements folded since its last partition head, or over the whole tile} per
//                     aggregate, and the tile's first partition head and tie head
//   k_wagg_scan       a workgroup per aggregate: exclusive segmented scan of the carries over the tiles (win_join's rule)
//   k_wagg_run        the tile again with its carry-in: a segmented inclusive scan across the lanes (a lane never reaches below its
//                     partition head's lane), the running carry folded in — the ROWS value of every position, 8 bytes
//   k_wagg_next / k_wagg_ends
//                     only for RANGE / PARTITION frames, backwards: the first heads of the later tiles (suffix minimum), then per
//                     position the last row of its tie run / partition, whose ROWS value is copied: the frames agree bit for bit.
//                     Row j is sorted position j: the first m values are the output, k_sort_emit writes the rows as for a plain sort
//   SLIDES            in their place (STEP_SLIDES).  sdqh_table_window_slide (include/sdqh_sort_slide.h) takes SUM / COUNT / MIN / MAX /
//                     FIRST / LAST over ROWS BETWEEN lo AND hi of the same partitions.  Behind k_win_heads and k_win_scan:
//
//   k_wsl_rows        the row number of every position in its partition (k_win_rank's ROW_NUMBER arm), the tile's first partition head
//   k_wagg_next / k_wsl_blocks
//                     backwards: per position its partition's last position, every slide's element (perm -> refs -> stage, once) and
//                     a byte of block-head flags — a slide of width w cuts the partitions into blocks of w positions
//   k_wsl_tiles / k_wsl_scan / k_wsl_run
//                     the tile scan of the frames, restarted at block heads, forwards (prefix folds) and backwards (suffix folds)
//   k_wsl_fold        row j's frame [l, r] spans at most two blocks: suffix[l] (+) prefix[r], or one of them — see the section
//   RANGES            in their place (STEP_RANGES).  sdqh_table_window_range (include/sdqh_sort_range.h) takes the same six ops over VALUE
//                     and GROUP frames, whose width depends on the data.  Behind k_win_heads, k_win_scan, k_wsl_rows and k_wagg_next:
//
//   k_win_rank        only with a GROUPS range: the dense rank of every position (every row kept)
//   k_wrg_stage       backwards: per position its partition's last position, one ordered 64-bit key (the ORDER BY term's sort key /
//                     the rank's image) and every range's element — raw, or as a leaf of the range's fold tree
//   k_wrg_tiles / k_wrg_upper
//                     the fold trees bottom-up: nine levels inside the wave that owns a tile, the rest in one workgroup per range
//   k_wrg_fold        per row two binary searches of its partition for the frame's ends, then the tree's iterative query — see the section
//   QUANTILES         in their place (STEP_QUANTILES).  sdqh_table_window_quantile (include/sdqh_sort_quantile.h) takes NTILE / PERCENT_RANK /
//                     CUME_DIST / NTH / PERCENTILE_DISC / PERCENTILE_CONT — everything that needs the partition's size — and keeps the
//                     rows whose row number is <= per_limit (k_win_rank / k_sort_scan / k_win_place, as a window does).  Behind k_win_heads,
//                     k_win_scan, k_wsl_rows and k_wagg_next:
//
//   k_wq_ties         only with a CUME_DIST column: the first tie head of every tile, for k_wagg_next to scan
//   k_win_rank        only with a PERCENT_RANK column: the RANK of every position = its tie run's first offset + 1 (every row kept)
//   k_wq_stage        backwards: per position its partition's and its tie run's last position, every distinct measure's element once
//   k_wq_value        per returned row the indices, one or two gathers and the arithmetic — see the section
//   EXCLUDES          in their place (STEP_EXCLUDES).  sdqh_table_window_exclude (include/sdqh_sort_exclude.h) takes the six ops of the
//                     slides and AVG over ROWS, VALUE and GROUP frames — the unit a column's own — out of which the row, its tie run
//                     or its ties are taken.  Behind k_win_heads, k_win_scan, k_wsl_rows and k_wagg_next, and the ranges' k_win_rank
//                     (a GROUPS column), k_wrg_stage, k_wrg_tiles and k_wrg_upper over the columns' image as ranges:
//
//   k_wq_ties / k_win_rank / k_wex_ties
//                     only with a GROUP / TIES column: the first tie head of every tile for k_wagg_next to scan, the RANK of every
//                     position (its tie run's first offset + 1) and, backwards, its tie run's last position
//   k_wex_fold        per row and column the base frame's ends, the cut into at most three pieces, a tree query per piece — see the section
//   GROUPS            in their place (STEP_GROUPS).  sdqh_table_grouping_sets (include/sdqh_sort_groups.h) returns one row per GROUP at
//                     several nested levels of the terms — GROUP BY ROLLUP / CUBE / GROUPING SETS — with SUM / COUNT / MIN / MAX / AVG:
//
//   k_gs_depth        per position the number of leading terms equal to its predecessor's (the heads of every level in one byte), per
//                     tile and level the heads; k_sort_bins scans them, the level counts go to the host (the count is known only now)
//   k_wagg_tiles / k_wagg_scan / k_gs_run
//                     the highest level over the rows: the frames' tile scan, the value at a group's last row kept in the group's slot
//   k_gs_tiles / k_wagg_scan / k_sort_bins / k_gs_run
//                     every lower level over the groups of the level above it; k_gs_avg divides the sums of an AVG — see the section
//   DISTINCTS         in their place (STEP_DISTINCTS).  sdqh_table_group_distinct (include/sdqh_sort_distinct.h) returns one row per group of
//                     the first ngroup terms with COUNT / SUM / AVG over the DISTINCT values of the other terms, MODE and COUNT:
//
//   k_gs_depth / k_sort_bins
//                     as for GROUPS: a head of level nterms opens a value run, one of level ngroup a group; both counts go to the host
//   k_gd_heads / k_gd_elems
//                     the rows to value runs: a run's sorted position, depth and length, per aggregate the element the groups fold
//   k_gs_tiles / k_wagg_scan / k_sort_bins / k_gs_run
//                     the runs folded into groups, as a lower level of GROUPS; k_gd_finish unpacks MODE and divides an AVG — see the section
//   MOMENTS           in their place (STEP_MOMENTS).  sdqh_table_group_moments (include/sdqh_sort_moments.h) returns the rows of GROUPS with
//                     VAR / STDDEV / COVAR / CORR / REGR_SLOPE / REGR_INTERCEPT per group, two passes over the rows per level:
//
//   k_gs_depth / k_sort_bins
//                     as for GROUPS: the heads of every level, the level counts to the host
//   k_gd_heads / k_mo_stage
//                     per level: its groups' sorted positions, then per row every distinct measure as a double minus its representative's
//   k_gs_tiles / k_wagg_scan / k_gs_run
//                     pass 1, over the rows at that level: the groups' sums; k_mo_center hands every row its group's mean and writes the
//                     centred squares and products; the same three again, pass 2; k_mo_finish applies the ops — see the section
//   SESSIONS          in their place (STEP_SESSIONS).  sdqh_table_sessions (include/sdqh_sort_sessions.h) cuts every partition where the
//                     ORDER BY value jumps by more than a gap or a marker column changes, and returns columns over the row's session:
//
//   k_ss_heads        the boundary pass: each position against its predecessor BY VALUE (through refs, before the keys' encoding);
//                     the cuts as two flag bytes and a depth byte, the tile carries and counts the passes below expect
//   k_win_scan / k_win_rank
//                     the session's number in its partition (a dense rank), the row's number in its session (a row number)
//   k_wagg_tiles / k_wagg_scan / k_wagg_run / k_wagg_next, k_ss_rows
//                     per row: SUM / COUNT / MIN / MAX over sessions as over partitions; every row takes the value at its session's end
//   k_sort_bins, k_wagg_tiles / k_wagg_scan / k_gs_run, k_ss_sessions
//                     per session: the count to the host, the folds kept in the session's slot as a level of GROUPS — see the section
//   WMOMENTS          in their place (STEP_WMOMENTS).  sdqh_table_window_moments (include/sdqh_sort_wmoments.h) takes the nine ops of MOMENTS
//                     over ROWS, VALUE and GROUP frames.  Behind k_win_heads, k_win_scan, k_wsl_rows, k_wagg_next, the ranges' k_win_rank
//                     (a GROUPS column) and k_wrg_stage (the partitions' ends and the frames' keys alone):
//
//   k_wmo_stage       per position every distinct measure as a double: the leaves of the component trees (S, Q per measure, C per pair)
//   k_wmo_tiles / k_wmo_upper
//                     the trees' nodes: merged (n, S, Q, C) states over aligned blocks of 2^h positions, n never stored
//   k_wmo_fold        per row and column the frame's ends, the iterative query over the states, the op's formula — see the section
//
// What is sorted is a permutation of the gathered positions; a pass reads its digit through it (8-byte gathers from arrays that
// stay in L2 / Infinity Cache at the sizes a query result has) and moves 4 bytes per entry, whatever the number of sort columns.
// Nothing here has a counterpart in the reference, whose results are unordered sets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#define SDQH_DECLS_ONLY 1            // argument structs and device helpers of the kernel header, not a second copy of its kernels
#include "sdqh_host.hpp"
#include "sdqh_sort_range.h"
#include "sdqh_sort_quantile.h"
#include "sdqh_sort_exclude.h"
#include "sdqh_sort_groups.h"
#include "sdqh_sort_distinct.h"
#include "sdqh_sort_moments.h"
#include "sdqh_sort_sessions.h"
#include "sdqh_sort_wmoments.h"

using namespace sdqh_host;


namespace {

constexpr int SORT_SMALL = 1024;                     // largest n the single-workgroup kernel takes
constexpr int SORT_SMALL_WAVE = SORT_SMALL / (TPB / WAVE);
constexpr int SORT_TILE = 512;                       // positions a wave counts / places per pass (a result of 100 K rows still spreads over 200 waves)
constexpr int SORT_INFO = 2 + 2 * SDQH_SORT_MAX_KEYS;      // [n | AND of the keys per column | OR of the keys per column | terms whose field fell outside its ranks column, a bit each]
constexpr int SORT_INFO_BAD = 1 + 2 * SDQH_SORT_MAX_KEYS;
constexpr int TEXT_WORD_BYTES = 8;                   // varying bytes of a text row packed into one 64-bit sort key

// a sort column with its derivation (include/sdqh_sort_terms.h); nranks = rows of `ranks`
struct DevSortTerm { DevSortKey sk; uint64_t div, mod; int64_t add; const int64_t* ranks; int64_t nranks; };
__host__ __device__ inline bool term_derived(const DevSortTerm& t) { return t.div > 1 || t.mod != 0 || t.add != 0 || t.ranks != nullptr; }
// the bytes of a text row that make up one 64-bit key, most significant first: byte (24 - 8 * part) of code unit `unit`
struct DevTextWord { uint16_t unit[TEXT_WORD_BYTES]; uint8_t shift[TEXT_WORD_BYTES]; int32_t nbytes, _pad; };
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

// the tile of SORT_TILE consecutive positions of [0, n) the calling wave owns: tile w = [r0, r1); false: there is no such tile
__device__ __forceinline__ bool tile_range(uint32_t ntiles, uint32_t n, uint32_t& w, uint64_t& r0, uint64_t& r1) {
    w = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
    if (w >= ntiles) return false;
    r0 = (uint64_t)w * SORT_TILE; r1 = min((uint64_t)n, r0 + SORT_TILE);
    return true;
}

// the AND / OR of a column's keys, one pair per lane, folded over the wave and into info — the order does not matter: atomics
__device__ __forceinline__ void fold_masks(uint64_t all, uint64_t any, unsigned long long* __restrict__ info, int col) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) { all &= (uint64_t)__shfl_xor((long long)all, off, WAVE); any |= (uint64_t)__shfl_xor((long long)any, off, WAVE); }
    if (lane_id() == 0 && (all != ~0ull || any != 0ull)) { atomicAnd(&info[1 + col], (unsigned long long)all); atomicOr(&info[1 + SDQH_SORT_MAX_KEYS + col], (unsigned long long)any); }
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
// 2. one workgroup: exclusive scan of the per-segment counts, in place; info = [n | ~0 x 8 | 0 x 8 | 0]
__global__ __launch_bounds__(TPB) void k_sort_scan(uint32_t* __restrict__ seg_kept, int nseg, unsigned long long* __restrict__ info) {
    __shared__ uint32_t s_part[TPB];
    const int per = (nseg + TPB - 1) / TPB;
    const int b0 = threadIdx.x * per, b1 = min(nseg, b0 + per);
    uint32_t sum = 0;                                                 // (a build side holds at most 2^32 - 2 rows: 32 bits are enough)
    for (int b = b0; b < b1; ++b) sum += seg_kept[b];
    const uint32_t incl = block_scan_incl(sum, s_part);
    if (threadIdx.x == TPB - 1) info[0] = incl;
    if (threadIdx.x < SDQH_SORT_MAX_KEYS) { info[1 + threadIdx.x] = ~0ull; info[1 + SDQH_SORT_MAX_KEYS + threadIdx.x] = 0ull; }
    if (threadIdx.x == SDQH_SORT_MAX_KEYS) info[SORT_INFO_BAD] = 0ull;
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
// 4. one term's transformed keys beside the references (a launch per term), and the AND / OR of them.  n is the device's (info[0]).
// A derived term (uniform over the launch): field = (uint64(source) / div) % mod + add, then — if the term has a ranks column —
// ranks[field], read only after field was found inside [0, nranks): an entry whose field lies outside raises the term's bit in
// info[SORT_INFO_BAD] (the host reads the block anyway and fails the call) and takes key 0.
__global__ __launch_bounds__(TPB) void k_sort_keys(DevStage st, DevSortTerm tm, const uint32_t* __restrict__ refs, uint64_t* __restrict__ key, unsigned long long* __restrict__ info, int col) {
    const uint64_t n = info[0];
    const bool derived = term_derived(tm);
    uint64_t all = ~0ull, any = 0ull;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
        const int64_t idx = (int64_t)refs[i];
        const uint32_t hits = st.shits ? st.shits[idx] : 0u;
        uint64_t k = 0ull;
        if (!derived) k = top_sort_value(tm.sk, st, idx, hits);
        else {
            uint64_t f = (uint64_t)sort_raw(tm.sk, st, idx, hits);
            if (tm.div > 1) f /= tm.div;
            if (tm.mod) f %= tm.mod;
            const int64_t v = (int64_t)(f + (uint64_t)tm.add);
            if (!tm.ranks) k = sort_bits(v, 0, tm.sk.desc);
            else if (v >= 0 && v < tm.nranks) k = sort_bits(tm.ranks[v], 0, tm.sk.desc);
            else bad = true;
        }
        key[i] = k; all &= k; any |= k;
    }
    fold_masks(all, any, info, col);
    if (__ballot(bad) && lane_id() == 0) atomicOr(&info[SORT_INFO_BAD], 1ull << col);
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
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
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
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    for (int d = lane; d < 256; d += WAVE) s_at[wv][d] = s_part[d] + hist[(size_t)d * ntiles + w];
    const uint64_t lt = lanemask_lt();
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const uint32_t g = live ? (perm ? perm[r] : (uint32_t)r) : 0u;
        const uint32_t d = live && g < n ? (uint32_t)(key[g] >> shift) & 255u : 0u;
        const uint32_t place = wave_place(s_at[wv], live, d, lt);
        if (live && place < n) perm_out[place] = g;
    }
}

// ---- text ranking (sdqh_text_ranks) ----------------------------------------------------------------------------------------------
// A text column is nrows x width 32-bit code units.  (a) k_text_masks: per position the AND and the OR of the unit over all rows —
// OR & ~AND = the bits that differ between any two rows; the host reads the block and lists the BYTES that vary at all, most
// significant first ("Supplier#000012345": the low byte of six to nine positions out of 25).  (b) k_text_pack: up to eight of those
// bytes of every row as one uint64.  (c) the stable LSD passes above (k_sort_hist / _bins / _scatter) over that word, last word
// first, one key buffer reused; every packed byte varies, so every pass is needed and none is looked for.  (d) dense ranks in the
// count -> scan -> place shape: a sorted row that differs from its predecessor (compared on the text itself) opens a new rank;
// k_rank_count counts those per tile, k_sort_scan scans the tiles, k_rank_place writes ranks[perm[i]].  One form for every n.
constexpr int TEXT_MAX_WIDTH = SDQH_TEXT_RANK_MAX_WIDTH;
static_assert(TEXT_MAX_WIDTH <= TPB, "a workgroup holds at least one row of code units");

__global__ __launch_bounds__(TPB) void k_text_masks(const uint32_t* __restrict__ text, uint64_t nrows, int width, uint32_t* __restrict__ masks) {
    __shared__ uint32_t s_and[TEXT_MAX_WIDTH], s_or[TEXT_MAX_WIDTH];
    if (threadIdx.x < TEXT_MAX_WIDTH) { s_and[threadIdx.x] = ~0u; s_or[threadIdx.x] = 0u; }
    __syncthreads();
    const int rows_per = TPB / width;                                 // whole rows a workgroup reads per step: consecutive threads, consecutive units
    const int p = (int)threadIdx.x % width, sub = (int)threadIdx.x / width;
    if (sub < rows_per) {
        uint32_t all = ~0u, any = 0u;
        for (uint64_t r = (uint64_t)blockIdx.x * rows_per + sub; r < nrows; r += (uint64_t)gridDim.x * rows_per) { const uint32_t u = text[r * (uint64_t)width + p]; all &= u; any |= u; }
        atomicAnd(&s_and[p], all); atomicOr(&s_or[p], any);
    }
    __syncthreads();
    if ((int)threadIdx.x < width) { atomicAnd(&masks[threadIdx.x], s_and[threadIdx.x]); atomicOr(&masks[TEXT_MAX_WIDTH + threadIdx.x], s_or[threadIdx.x]); }
}
__global__ __launch_bounds__(TPB) void k_text_pack(const uint32_t* __restrict__ text, uint64_t nrows, int width, DevTextWord w, uint64_t* __restrict__ key) {
    for (uint64_t r = (uint64_t)blockIdx.x * TPB + threadIdx.x; r < nrows; r += (uint64_t)gridDim.x * TPB) {
        const uint32_t* __restrict__ row = text + r * (uint64_t)width;
        uint64_t k = 0ull;
#pragma unroll
        for (int b = 0; b < TEXT_WORD_BYTES; ++b) if (b < w.nbytes && (int)w.unit[b] < width) k |= (uint64_t)((row[w.unit[b]] >> w.shift[b]) & 255u) << (56 - 8 * b);
        key[r] = k;
    }
}
// does the row at sorted position r (>= 1) differ from the one before it?
__device__ __forceinline__ bool text_head(const uint32_t* __restrict__ text, int width, const uint32_t* __restrict__ perm, uint64_t r, uint32_t n, uint32_t& g) {
    g = perm ? perm[r] : (uint32_t)r;
    if (r == 0) return false;
    const uint32_t h = perm ? perm[r - 1] : (uint32_t)(r - 1);
    if (g >= n || h >= n) return false;                              // (a permutation of [0, n): never taken)
    const uint32_t* __restrict__ a = text + (uint64_t)g * width;
    const uint32_t* __restrict__ b = text + (uint64_t)h * width;
    bool differ = false;
    for (int p = 0; p < width; ++p) differ |= a[p] != b[p];
    return differ;
}
__global__ __launch_bounds__(TPB) void k_rank_count(const uint32_t* __restrict__ text, int width, const uint32_t* __restrict__ perm, uint32_t n, uint32_t* __restrict__ tile_heads, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    uint32_t heads = 0;
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane_id();
        uint32_t g = 0;
        const bool head = r < r1 && text_head(text, width, perm, r, n, g);
        heads += (uint32_t)__popcll(__ballot(head));
    }
    if (lane_id() == 0) tile_heads[w] = heads;
}
__global__ __launch_bounds__(TPB) void k_rank_place(const uint32_t* __restrict__ text, int width, const uint32_t* __restrict__ perm, uint32_t n, const uint32_t* __restrict__ tile_off, uint32_t ntiles,
                                                   int64_t* __restrict__ ranks) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint64_t le = lanemask_lt() | (1ull << lane_id());
    uint32_t run = tile_off[w];                                       // ranks opened before this tile
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane_id();
        uint32_t g = 0;
        const bool live = r < r1;
        const bool head = live && text_head(text, width, perm, r, n, g);
        const uint64_t m = __ballot(head);
        if (live && g < n) ranks[g] = (int64_t)(run + (uint32_t)__popcll(m & le));
        run += (uint32_t)__popcll(m);
    }
}

// ---- ranks inside partitions (sdqh_table_window) ---------------------------------------------------------------------------------
// The carry of a run of sorted positions [a, b).  cnt: positions since the last partition head, that head included (none in the
// run: b - a).  tie_off: the last tie head's distance from that partition head (no partition head: from a); only meaningful with
// WIN_TIE.  ties: tie heads since the last partition head, itself included (none: in the whole run).  A partition head is a tie head.
constexpr uint32_t WIN_PART = 1u, WIN_TIE = 2u;
struct WinCarry { uint32_t flags, cnt, tie_off, ties; };
static_assert(sizeof(WinCarry) == 16, "a carry is one 16-byte load");

// the carry of [a, b) followed by [b, c): the segmented-scan operator (associative; {0, 0, 0, 0} is its left identity)
__device__ __forceinline__ WinCarry win_join(const WinCarry& l, const WinCarry& r) {
    if (r.flags & WIN_PART) return r;
    WinCarry o;
    o.flags = l.flags | r.flags;
    o.cnt = l.cnt + r.cnt;
    o.tie_off = (r.flags & WIN_TIE) ? l.cnt + r.tie_off : l.tie_off;
    o.ties = l.ties + r.ties;
    return o;
}
// `run` moved over one wave's batch of `live` positions (lanes [0, live)) with partition heads mp and tie heads mt
__device__ __forceinline__ void win_step(WinCarry& run, uint64_t mp, uint64_t mt, uint32_t live) {
    if (mp) {
        const uint32_t p = 63u - (uint32_t)__clzll((long long)mp);
        run.flags = WIN_PART | WIN_TIE;
        run.cnt = live - p;
        run.tie_off = (63u - (uint32_t)__clzll((long long)mt)) - p;         // (mt has bit p: the distance is >= 0)
        run.ties = (uint32_t)__popcll(mt >> p);
    } else {
        if (mt) { run.flags |= WIN_TIE; run.tie_off = run.cnt + (63u - (uint32_t)__clzll((long long)mt)); }
        run.ties += (uint32_t)__popcll(mt);
        run.cnt += live;
    }
}

// 1. heads + the carry of every tile.  keys[c * key_stride + g]: term c's key of gathered entry g.
__global__ __launch_bounds__(TPB) void k_win_heads(const uint64_t* __restrict__ keys, size_t key_stride, int npart, int nterms, const uint32_t* __restrict__ perm, uint32_t n,
                                                  uint8_t* __restrict__ heads, WinCarry* __restrict__ carry, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    WinCarry run = {0u, 0u, 0u, 0u};
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane_id();
        const bool live = r < r1;
        bool ph = false, th = false;
        if (live) {
            if (r == 0) ph = th = true;
            else {
                const uint32_t g = perm ? perm[r] : (uint32_t)r, h = perm ? perm[r - 1] : (uint32_t)(r - 1);
                if (g < n && h < n)                                      // (a permutation of [0, n): always)
                    for (int c = 0; c < nterms; ++c) {
                        const bool differ = keys[(size_t)c * key_stride + g] != keys[(size_t)c * key_stride + h];
                        th |= differ;
                        ph |= differ && c < npart;
                    }
            }
            heads[r] = (uint8_t)((ph ? WIN_PART : 0u) | (th ? WIN_TIE : 0u));
        }
        win_step(run, __ballot(ph), __ballot(th), (uint32_t)min((uint64_t)WAVE, r1 - b));
    }
    if (lane_id() == 0) carry[w] = run;
}
// 2. one workgroup: exclusive scan of the tile carries under win_join, in place (thread t folds a run of consecutive tiles, the runs
// are scanned in LDS — Hillis-Steele, the operator is not commutative: left operand = lower tiles — and each run is then rewritten)
__global__ __launch_bounds__(TPB) void k_win_scan(WinCarry* __restrict__ carry, uint32_t ntiles) {
    __shared__ WinCarry s_c[TPB];
    const uint32_t per = (ntiles + TPB - 1) / TPB;
    const uint64_t b0 = (uint64_t)threadIdx.x * per, b1 = min((uint64_t)ntiles, b0 + per);
    WinCarry sum = {0u, 0u, 0u, 0u};
    for (uint64_t b = b0; b < b1; ++b) sum = win_join(sum, carry[b]);
    s_c[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {
        WinCarry a = {0u, 0u, 0u, 0u};
        if ((int)threadIdx.x >= off) a = s_c[threadIdx.x - off];
        __syncthreads();
        s_c[threadIdx.x] = win_join(a, s_c[threadIdx.x]);
        __syncthreads();
    }
    WinCarry run = {0u, 0u, 0u, 0u};
    if (threadIdx.x > 0) run = s_c[threadIdx.x - 1];
    for (uint64_t b = b0; b < b1; ++b) { const WinCarry v = carry[b]; carry[b] = run; run = win_join(run, v); }
}
// 3. the rank of `kind` of every position, and per tile the positions with rank <= per_limit
__global__ __launch_bounds__(TPB) void k_win_rank(const uint8_t* __restrict__ heads, const WinCarry* __restrict__ carry, uint32_t n, int kind, uint64_t per_limit,
                                                 uint32_t* __restrict__ rank, uint32_t* __restrict__ tile_kept, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    WinCarry run = carry[w];
    uint32_t kept = 0;
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const uint32_t f = live ? heads[r] : 0u;
        const uint64_t mp = __ballot(f & WIN_PART), mt = __ballot(f & WIN_TIE);
        const uint64_t pl = mp & le, tl = mt & le;
        uint32_t v;
        if (pl) {                                                       // the partition starts in this batch, at lane p
            const uint32_t p = 63u - (uint32_t)__clzll((long long)pl);
            if (kind == SDQH_WIN_ROW_NUMBER) v = lane - p + 1u;
            else if (kind == SDQH_WIN_RANK) v = (63u - (uint32_t)__clzll((long long)tl)) - p + 1u;
            else v = (uint32_t)__popcll(tl >> p);
        } else {                                                        // ... before it: the carry knows where
            if (kind == SDQH_WIN_ROW_NUMBER) v = run.cnt + lane + 1u;
            else if (kind == SDQH_WIN_RANK) v = (tl ? run.cnt + (63u - (uint32_t)__clzll((long long)tl)) : run.tie_off) + 1u;
            else v = run.ties + (uint32_t)__popcll(tl);
        }
        if (live) rank[r] = v;
        kept += (uint32_t)__popcll(__ballot(live && (uint64_t)v <= per_limit));
        win_step(run, mp, mt, (uint32_t)min((uint64_t)WAVE, r1 - b));
    }
    if (lane == 0) tile_kept[w] = kept;
}
// 4. the kept positions, in order: sel[0 .. kept) (tile_off: k_sort_scan of tile_kept); only the first m are asked for
__global__ __launch_bounds__(TPB) void k_win_place(const uint32_t* __restrict__ rank, uint32_t n, uint64_t per_limit, const uint32_t* __restrict__ tile_off, uint32_t ntiles,
                                                  uint32_t* __restrict__ sel, uint32_t m) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint64_t lt = lanemask_lt();
    uint64_t at0 = tile_off[w];
    for (uint64_t b = r0; b < r1 && at0 < m; b += WAVE) {
        const uint64_t r = b + lane_id();
        const bool keep = r < r1 && (uint64_t)rank[r] <= per_limit;
        const uint64_t k = __ballot(keep);
        const uint64_t at = at0 + (uint64_t)__popcll(k & lt);
        if (keep && at < m) sel[at] = (uint32_t)r;
        at0 += (uint64_t)__popcll(k);
    }
}
// ---- aggregates over window frames (sdqh_table_window_agg) -----------------------------------------------------------------------
// Every aggregate is a 64-bit ELEMENT per position folded by one of three associative operators (its class): SUM of an integer
// measure and COUNT add uint64 (two's complement: exact in any association), SUM of a double measure adds doubles, MIN / MAX take the
// unsigned maximum of the order-preserving image (reversed for MIN; a NaN is 0, which no other double encodes to — the rule of
// sdqh_extrema.hip).  Each class has a left and right identity: 0, -0.0 (x + -0.0 = x for every x, -0.0 included), 0.
constexpr int WAGG_ADD_I = 0, WAGG_ADD_F = 1, WAGG_UMAX = 2;
constexpr unsigned long long WAGG_QNAN = 0x7FF8000000000000ull;
struct DevWagg { DevSortKey sk; int32_t op, frame, cls, _pad; };      // sk: the measure (desc unused)
struct DevWaggs { DevWagg a[SDQH_WAGG_MAX_AGGS]; int32_t n, _pad; };
struct WaggHeads { uint32_t part, tie; };            // positions of a partition head and of a tie head (n: none)

__device__ __forceinline__ uint64_t wagg_identity(int cls) { return cls == WAGG_ADD_F ? (1ull << 63) : 0ull; }
// left (lower positions) joined with right
__device__ __forceinline__ uint64_t wagg_join(int cls, uint64_t l, uint64_t r) {
    if (cls == WAGG_ADD_I) return l + r;
    if (cls == WAGG_UMAX) return l > r ? l : r;
    return (uint64_t)__double_as_longlong(__longlong_as_double((long long)l) + __longlong_as_double((long long)r));
}
// the element of staged row idx
__device__ __forceinline__ uint64_t wagg_element(const DevWagg& g, const DevStage& st, int64_t idx, uint32_t hits) {
    if (g.op == SDQH_WAGG_COUNT) return 1ull;
    const int64_t raw = sort_raw(g.sk, st, idx, hits);
    if (g.op == SDQH_WAGG_SUM) return (uint64_t)raw;
    if (g.sk.is_f64) { const double d = __longlong_as_double(raw); if (d != d) return 0ull; }
    return sort_bits(raw, g.sk.is_f64, g.op == SDQH_WAGG_MIN);
}
// a folded element as the caller reads it: sums and counts as they are, an image decoded (a double frame nothing reached: the quiet NaN)
__device__ __forceinline__ uint64_t wagg_result(const DevWagg& g, uint64_t e) {
    if (g.cls != WAGG_UMAX) return e;
    if (g.sk.is_f64 && e == 0ull) return WAGG_QNAN;
    const uint64_t u = g.op == SDQH_WAGG_MIN ? ~e : e;
    if (!g.sk.is_f64) return u ^ (1ull << 63);
    return (u >> 63) ? (u ^ (1ull << 63)) : ~u;
}
// Inclusive scan of one element per lane, restarted at partition heads (Hillis-Steele over the wave): `first` = the lane of the
// last partition head at or below this lane (none: 0).  A lane takes from lane - d only when that lane is not below `first`; by
// then it holds everything from max(first, lane - d + 1) on, so nothing is taken twice and nothing of another partition at all.
__device__ __forceinline__ uint64_t wagg_wave_scan(int cls, uint64_t v, uint32_t lane, uint32_t first) {
#pragma unroll
    for (uint32_t d = 1; d < (uint32_t)WAVE; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)v, d, WAVE);
        if (lane >= first + d) v = wagg_join(cls, o, v);
    }
    return v;
}
// what a wave's batch at [b, ..) knows of lane's partition: the two head ballots, and `first` for wagg_wave_scan
struct WaggBatch { uint64_t mp, mt, pl; uint32_t first; };
__device__ __forceinline__ WaggBatch wagg_batch(const uint8_t* __restrict__ heads, uint64_t r, bool live, uint64_t le) {
    const uint32_t f = live ? heads[r] : 0u;
    WaggBatch h;
    h.mp = __ballot(f & WIN_PART); h.mt = __ballot(f & WIN_TIE);
    h.pl = h.mp & le;
    h.first = h.pl ? 63u - (uint32_t)__clzll((long long)h.pl) : 0u;
    return h;
}

// 1. the element of every position and aggregate (elem[a * stride + r], read through perm -> refs -> stage once: the later passes
// stay on these arrays), per tile and aggregate the carry — the elements folded since the tile's last partition head, or over the
// whole tile — and per tile the position of its first partition head and first tie head.  heads: k_win_heads'.
__global__ __launch_bounds__(TPB) void k_wagg_tiles(DevStage st, DevWaggs ag, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ heads,
                                                   uint32_t n, size_t stride, uint64_t* __restrict__ elem, uint64_t* __restrict__ tval, WaggHeads* __restrict__ tfirst, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint64_t run[SDQH_WAGG_MAX_AGGS];
#pragma unroll
    for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) run[a] = wagg_identity(ag.a[a].cls);
    WaggHeads fh = {n, n};
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        if (h.mp && fh.part == n) fh.part = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (h.mt && fh.tie == n) fh.tie = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mt);
        const uint32_t g = live ? (perm ? perm[r] : (uint32_t)r) : n;
        const bool ok = g < n;                                           // (a permutation of [0, n): every live lane)
        const int64_t idx = ok ? (int64_t)refs[g] : 0;
        const uint32_t hits = ok && st.shits ? st.shits[idx] : 0u;
        const int last = (int)min((uint64_t)WAVE, r1 - b) - 1;
#pragma unroll
        for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n) {
            const int cls = ag.a[a].cls;
            const uint64_t e = ok ? wagg_element(ag.a[a], st, idx, hits) : wagg_identity(cls);
            if (live) elem[(size_t)a * stride + r] = e;
            const uint64_t s = wagg_wave_scan(cls, e, lane, h.first);
            const uint64_t tail = (uint64_t)__shfl((long long)s, last, WAVE);          // since the batch's last head, or the whole batch
            run[a] = h.mp ? tail : wagg_join(cls, run[a], tail);
        }
    }
    if (lane == 0) {
        tfirst[w] = fh;
#pragma unroll
        for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n) tval[(size_t)a * ntiles + w] = run[a];
    }
}
// 2. workgroup a: exclusive segmented scan of aggregate a's tile carries, in place — k_win_scan's shape and win_join's rule (a right
// side with a partition head wins); the operator is not commutative where it matters (doubles): left operand = lower tiles
__global__ __launch_bounds__(TPB) void k_wagg_scan(DevWaggs ag, const WaggHeads* __restrict__ tfirst, uint32_t n, uint64_t* __restrict__ tval, uint32_t ntiles) {
    __shared__ uint64_t s_v[TPB];
    __shared__ uint32_t s_f[TPB];
    const int cls = ag.a[blockIdx.x].cls;
    const uint64_t id = wagg_identity(cls);
    uint64_t* __restrict__ v = tval + (size_t)blockIdx.x * ntiles;
    const uint32_t per = (ntiles + TPB - 1) / TPB;
    const uint64_t b0 = (uint64_t)threadIdx.x * per, b1 = min((uint64_t)ntiles, b0 + per);
    uint64_t sum = id; uint32_t f = 0u;
    for (uint64_t b = b0; b < b1; ++b) { const bool hf = tfirst[b].part < n; sum = hf ? v[b] : wagg_join(cls, sum, v[b]); f |= hf ? 1u : 0u; }
    s_v[threadIdx.x] = sum; s_f[threadIdx.x] = f;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {
        uint64_t av = id; uint32_t af = 0u;
        if ((int)threadIdx.x >= off) { av = s_v[threadIdx.x - off]; af = s_f[threadIdx.x - off]; }
        __syncthreads();
        if (!s_f[threadIdx.x]) { s_v[threadIdx.x] = wagg_join(cls, av, s_v[threadIdx.x]); s_f[threadIdx.x] = af; }
        __syncthreads();
    }
    uint64_t run = threadIdx.x > 0 ? s_v[threadIdx.x - 1] : id;
    for (uint64_t b = b0; b < b1; ++b) { const uint64_t x = v[b]; v[b] = run; run = tfirst[b].part < n ? x : wagg_join(cls, run, x); }
}
// 3. the tile again with its carry-in, 64 positions at a time: the segmented scan across the lanes, the running carry folded into
// the lanes whose partition started before the batch; elem[a * stride + r] becomes aggregate a's ROWS value of position r, decoded
__global__ __launch_bounds__(TPB) void k_wagg_run(DevWaggs ag, const uint8_t* __restrict__ heads, uint32_t n, size_t stride, uint64_t* __restrict__ elem,
                                                 const uint64_t* __restrict__ tval, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint64_t run[SDQH_WAGG_MAX_AGGS];
#pragma unroll
    for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) run[a] = a < ag.n ? tval[(size_t)a * ntiles + w] : 0ull;
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        const int last = (int)min((uint64_t)WAVE, r1 - b) - 1;
#pragma unroll
        for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n) {
            const int cls = ag.a[a].cls;
            const uint64_t e = live ? elem[(size_t)a * stride + r] : wagg_identity(cls);
            const uint64_t s = wagg_wave_scan(cls, e, lane, h.first);
            const uint64_t v = h.pl ? s : wagg_join(cls, run[a], s);
            if (live) elem[(size_t)a * stride + r] = wagg_result(ag.a[a], v);
            run[a] = (uint64_t)__shfl((long long)v, last, WAVE);        // (the last live lane has seen every head of the batch)
        }
    }
}
// 4. one workgroup: for every tile the first partition head and the first tie head of the tiles AFTER it (n: none) — an exclusive
// suffix minimum of tfirst over the tiles (positions grow with the tile, "none" is n, the largest)
__device__ __forceinline__ WaggHeads wagg_min(const WaggHeads& a, const WaggHeads& b) { return WaggHeads{min(a.part, b.part), min(a.tie, b.tie)}; }
__global__ __launch_bounds__(TPB) void k_wagg_next(const WaggHeads* __restrict__ tfirst, uint32_t n, WaggHeads* __restrict__ tnext, uint32_t ntiles) {
    __shared__ WaggHeads s_h[TPB];
    const uint32_t per = (ntiles + TPB - 1) / TPB;
    const uint64_t b0 = min((uint64_t)ntiles, (uint64_t)threadIdx.x * per), b1 = min((uint64_t)ntiles, b0 + per);
    WaggHeads mine = {n, n};
    for (uint64_t b = b0; b < b1; ++b) mine = wagg_min(mine, tfirst[b]);
    s_h[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {
        WaggHeads o = {n, n};
        if ((int)threadIdx.x + off < TPB) o = s_h[threadIdx.x + off];
        __syncthreads();
        s_h[threadIdx.x] = wagg_min(s_h[threadIdx.x], o);
        __syncthreads();
    }
    WaggHeads run = {n, n};
    if (threadIdx.x + 1 < TPB) run = s_h[threadIdx.x + 1];
    for (uint64_t b = b1; b > b0; --b) { const WaggHeads x = tfirst[b - 1]; tnext[b - 1] = run; run = wagg_min(run, x); }
}
// 5. the RANGE and PARTITION values of the first m positions (only launched when some aggregate asks for one): a tile walked
// backwards, the next tie head / partition head after a position read off the ballots above its lane, else off the batches and
// tiles behind; the value is the ROWS value of the position before that head — a copy, so the frames agree bit for bit
__global__ __launch_bounds__(TPB) void k_wagg_ends(DevWaggs ag, const uint8_t* __restrict__ heads, const WaggHeads* __restrict__ tnext, uint32_t n, uint32_t m, size_t stride,
                                                  const uint64_t* __restrict__ rows, uint64_t* __restrict__ fin, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;                       // ntiles: the tiles that hold a position below m
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    WaggHeads next = tnext[w];
    for (uint64_t b = r0 + ((r1 - r0 - 1) / WAVE) * WAVE; ; b -= WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        const uint64_t pg = h.mp & ~le, tg = h.mt & ~le;
        const uint32_t pe = (pg ? (uint32_t)b + (uint32_t)__builtin_ctzll(pg) : next.part) - 1u;
        const uint32_t te = (tg ? (uint32_t)b + (uint32_t)__builtin_ctzll(tg) : next.tie) - 1u;
        if (live && r < m) {
#pragma unroll
            for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n && ag.a[a].frame != SDQH_FRAME_ROWS) {
                const uint32_t e = ag.a[a].frame == SDQH_FRAME_RANGE ? te : pe;
                if (e < n) fin[(size_t)a * stride + r] = rows[(size_t)a * stride + e];     // (r <= e < n: always)
            }
        }
        if (h.mp) next.part = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (h.mt) next.tie = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mt);
        if (b == r0) break;
    }
}

// ---- sliding frames (sdqh_table_window_slide) ------------------------------------------------------------------------------------
// The frame of sorted row j is [l, r] = [max(j + lo, s), min(j + hi, e)] inside its partition [s, e].  COUNT is arithmetic on l and
// r, FIRST / LAST gather the raw element at l / r.  SUM / MIN / MAX of width w = hi - lo + 1 (an unbounded side, or w >= n: w = n, a
// block is the partition) cut every partition into BLOCKS of w positions aligned at the partition's start and fold every block
// twice — an inclusive prefix from its first position, an inclusive suffix up to its last — so that a frame, which spans at most
// two adjacent blocks, is suffix[l] (+) prefix[r], or one of the two alone: the work per row does not depend on w, exactly the
// frame's rows enter, nothing is added and later subtracted.  The two folds are the tile scan of the frames above (tile carries ->
// scan over the tiles -> the tile again) with block heads in the place of partition heads, once forwards and once backwards.
constexpr int WSL_NONE = 3;                          // a slide's class when nothing is folded (COUNT, FIRST, LAST); else WAGG_*
constexpr int WSL_FWD = 0, WSL_BWD = 1;
struct DevWslide { DevWagg g; uint32_t w, _pad; int64_t lo, hi; uint64_t empty; };     // g.frame unused; lo / hi clamped to [-n, n]; 1 <= w <= n
struct DevWslides { DevWslide a[SDQH_WSLIDE_MAX_AGGS]; int32_t n, _pad; };
static_assert(SDQH_WSLIDE_MAX_AGGS * 2 <= 8, "a byte per position holds every slide's two block-head flags");

// the batch of 64 positions at [b, ..) as one direction walks it: forwards lane i holds position b + i, backwards b + 63 - i, so
// that "a lower lane" is "earlier in the fold" either way and wagg_wave_scan's lane rule holds unchanged
__device__ __forceinline__ uint64_t wsl_pos(int dir, uint64_t b, uint32_t lane) { return dir == WSL_BWD ? b + (uint64_t)(WAVE - 1) - lane : b + lane; }
// wagg_wave_scan with the operands in position order: backwards the lower lane is the higher position, the right operand
__device__ __forceinline__ uint64_t wsl_wave_scan(int cls, int dir, uint64_t v, uint32_t lane, uint32_t first) {
#pragma unroll
    for (uint32_t d = 1; d < (uint32_t)WAVE; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)v, d, WAVE);
        if (lane >= first + d) v = dir == WSL_BWD ? wagg_join(cls, v, o) : wagg_join(cls, o, v);
    }
    return v;
}
__device__ __forceinline__ uint64_t wsl_join(int cls, int dir, uint64_t before, uint64_t after) { return dir == WSL_BWD ? wagg_join(cls, after, before) : wagg_join(cls, before, after); }

// 1. the row number of every position inside its partition, from 0 (k_win_rank's ROW_NUMBER arm: carry = k_win_scan's), and per
// tile the position of its first partition head (n: none; what k_wagg_next scans)
__global__ __launch_bounds__(TPB) void k_wsl_rows(const uint8_t* __restrict__ heads, const WinCarry* __restrict__ carry, uint32_t n, uint32_t* __restrict__ rown,
                                                 WaggHeads* __restrict__ tfirst, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    WinCarry run = carry[w];
    WaggHeads fh = {n, n};
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        if (h.mp && fh.part == n) fh.part = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (live) rown[r] = h.pl ? lane - h.first : run.cnt + lane;
        win_step(run, h.mp, h.mt, (uint32_t)min((uint64_t)WAVE, r1 - b));
    }
    if (lane == 0) tfirst[w] = fh;
}
// 2. a tile walked backwards (k_wagg_ends' shape): per position the last position of its partition, every slide's element (the
// measure read through perm -> refs -> stage once: raw for SUM / FIRST / LAST, the image for MIN / MAX, none for COUNT) and the
// block-head flags of the folded slides, a byte: bit 2a = position opens a block of slide a, bit 2a + 1 = it closes one
__global__ __launch_bounds__(TPB) void k_wsl_blocks(DevStage st, DevWslides sl, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ heads,
                                                   const WaggHeads* __restrict__ tnext, const uint32_t* __restrict__ rown, uint32_t n, size_t stride,
                                                   uint32_t* __restrict__ pend, uint8_t* __restrict__ bh, uint64_t* __restrict__ elem, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint32_t next = tnext[w].part;
    for (uint64_t b = r0 + ((r1 - r0 - 1) / WAVE) * WAVE; ; b -= WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        const uint64_t pg = h.mp & ~le;
        const uint32_t pe = (pg ? (uint32_t)b + (uint32_t)__builtin_ctzll(pg) : next) - 1u;
        if (live) {
            const uint32_t rn = rown[r];
            const uint32_t g = perm ? perm[r] : (uint32_t)r;
            const bool ok = g < n;                                       // (a permutation of [0, n): always)
            const int64_t idx = ok ? (int64_t)refs[g] : 0;
            const uint32_t hits = ok && st.shits ? st.shits[idx] : 0u;
            uint32_t flags = 0u;
#pragma unroll
            for (int a = 0; a < SDQH_WSLIDE_MAX_AGGS; ++a) if (a < sl.n) {
                const DevWslide& s = sl.a[a];
                if (s.g.cls != WSL_NONE) {
                    if (rn % s.w == 0u) flags |= 1u << (2 * a);
                    if ((uint32_t)r == pe || (rn + 1u) % s.w == 0u) flags |= 2u << (2 * a);
                }
                if (s.g.op != SDQH_WAGG_COUNT) {
                    uint64_t e = 0ull;
                    if (ok) e = s.g.cls == WSL_NONE ? (uint64_t)sort_raw(s.g.sk, st, idx, hits) : wagg_element(s.g, st, idx, hits);
                    elem[(size_t)a * stride + r] = e;
                }
            }
            pend[r] = pe;
            bh[r] = (uint8_t)flags;
        }
        if (h.mp) next = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (b == r0) break;
    }
}
// One direction of one tile, 64 positions at a time — the segmented scan across the lanes restarted at block heads, the running
// carry folded into the lanes whose block began before the batch.  `run` comes in as the tile's carry-in and leaves as its carry-out
// (the elements folded since the tile's last head, or carry-in and whole tile); out != nullptr: the fold of every position is stored.
// Returns whether the tile holds a head.  Dead lanes (past the tile's end) hold the identity and no head.
__device__ __forceinline__ bool wsl_tile_fold(int cls, int dir, int a, const uint8_t* __restrict__ bh, const uint64_t* in, uint64_t* out,
                                              uint64_t r0, uint64_t r1, uint32_t lane, uint64_t le, uint64_t& run) {
    const uint32_t nb = (uint32_t)((r1 - r0 + WAVE - 1) / WAVE);
    bool seen = false;
    for (uint32_t k = 0; k < nb; ++k) {
        const uint64_t b = r0 + (uint64_t)(dir == WSL_BWD ? nb - 1u - k : k) * WAVE;
        const uint64_t r = wsl_pos(dir, b, lane);
        const bool live = r < r1;
        const uint32_t f = live ? bh[r] : 0u;
        const uint64_t mh = __ballot((f >> (2 * a + dir)) & 1u);
        const uint64_t hl = mh & le;
        const uint64_t e = live ? in[r] : wagg_identity(cls);
        const uint64_t s = wsl_wave_scan(cls, dir, e, lane, hl ? 63u - (uint32_t)__clzll((long long)hl) : 0u);
        const uint64_t v = hl ? s : wsl_join(cls, dir, run, s);
        if (out && live) out[r] = v;
        const int last = dir == WSL_BWD ? WAVE - 1 : (int)min((uint64_t)WAVE, r1 - b) - 1;      // the lane that has seen the whole batch
        run = (uint64_t)__shfl((long long)v, last, WAVE);
        seen |= mh != 0ull;
    }
    return seen;
}
// 3. per tile, folded slide and direction the carry and whether the tile holds a block head: tval / thead[(dir * MAX_AGGS + a) * ntiles + tile]
__global__ __launch_bounds__(TPB) void k_wsl_tiles(DevWslides sl, const uint8_t* __restrict__ bh, uint32_t n, size_t stride, const uint64_t* __restrict__ elem,
                                                  uint64_t* __restrict__ tval, uint8_t* __restrict__ thead, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
#pragma unroll
    for (int a = 0; a < SDQH_WSLIDE_MAX_AGGS; ++a) if (a < sl.n && sl.a[a].g.cls != WSL_NONE) {
        const int cls = sl.a[a].g.cls;
        for (int dir = WSL_FWD; dir <= WSL_BWD; ++dir) {
            uint64_t run = wagg_identity(cls);
            const bool seen = wsl_tile_fold(cls, dir, a, bh, elem + (size_t)a * stride, nullptr, r0, r1, lane, le, run);
            if (lane == 0) { const size_t at = (size_t)(dir * SDQH_WSLIDE_MAX_AGGS + a) * ntiles + w; tval[at] = run; thead[at] = seen ? 1u : 0u; }
        }
    }
}
// 4. workgroup dir * MAX_AGGS + a: exclusive segmented scan of those carries over the tiles in the direction's order, in place —
// k_wagg_scan's shape (a later side with a head wins; the operands stay in position order)
__global__ __launch_bounds__(TPB) void k_wsl_scan(DevWslides sl, const uint8_t* __restrict__ thead, uint64_t* __restrict__ tval, uint32_t ntiles) {
    __shared__ uint64_t s_v[TPB];
    __shared__ uint32_t s_f[TPB];
    const int dir = (int)blockIdx.x / SDQH_WSLIDE_MAX_AGGS, a = (int)blockIdx.x % SDQH_WSLIDE_MAX_AGGS;
    if (a >= sl.n || sl.a[a].g.cls == WSL_NONE) return;
    const int cls = sl.a[a].g.cls;
    const uint64_t id = wagg_identity(cls);
    uint64_t* __restrict__ v = tval + (size_t)blockIdx.x * ntiles;
    const uint8_t* __restrict__ hd = thead + (size_t)blockIdx.x * ntiles;
    const uint32_t per = (ntiles + TPB - 1) / TPB;
    const uint64_t b0 = min((uint64_t)ntiles, (uint64_t)threadIdx.x * per), b1 = min((uint64_t)ntiles, b0 + per);
    const auto tile = [&](uint64_t b) { return dir == WSL_BWD ? (uint64_t)ntiles - 1u - b : b; };      // the b-th tile the direction meets
    uint64_t sum = id; uint32_t f = 0u;
    for (uint64_t b = b0; b < b1; ++b) { const uint64_t t = tile(b); const bool hf = hd[t] != 0; sum = hf ? v[t] : wsl_join(cls, dir, sum, v[t]); f |= hf ? 1u : 0u; }
    s_v[threadIdx.x] = sum; s_f[threadIdx.x] = f;
    __syncthreads();
    for (int off = 1; off < TPB; off <<= 1) {
        uint64_t av = id; uint32_t af = 0u;
        if ((int)threadIdx.x >= off) { av = s_v[threadIdx.x - off]; af = s_f[threadIdx.x - off]; }
        __syncthreads();
        if (!s_f[threadIdx.x]) { s_v[threadIdx.x] = wsl_join(cls, dir, av, s_v[threadIdx.x]); s_f[threadIdx.x] = af; }
        __syncthreads();
    }
    uint64_t run = threadIdx.x > 0 ? s_v[threadIdx.x - 1] : id;
    for (uint64_t b = b0; b < b1; ++b) { const uint64_t t = tile(b); const uint64_t x = v[t]; v[t] = run; run = hd[t] ? x : wsl_join(cls, dir, run, x); }
}
// 5. the tile again with its carries-in: pre[a * stride + r] = the fold of r's block from its first position to r; then, in place,
// elem[a * stride + r] = the fold from r to the block's last position (the forward walk has read the tile's elements by then, and no
// other wave touches them)
__global__ __launch_bounds__(TPB) void k_wsl_run(DevWslides sl, const uint8_t* __restrict__ bh, uint32_t n, size_t stride, uint64_t* __restrict__ elem, uint64_t* __restrict__ pre,
                                                const uint64_t* __restrict__ tval, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
#pragma unroll
    for (int a = 0; a < SDQH_WSLIDE_MAX_AGGS; ++a) if (a < sl.n && sl.a[a].g.cls != WSL_NONE) {
        const int cls = sl.a[a].g.cls;
        uint64_t* __restrict__ e = elem + (size_t)a * stride;
        for (int dir = WSL_FWD; dir <= WSL_BWD; ++dir) {
            uint64_t run = tval[(size_t)(dir * SDQH_WSLIDE_MAX_AGGS + a) * ntiles + w];
            (void)wsl_tile_fold(cls, dir, a, bh, e, dir == WSL_BWD ? e : pre + (size_t)a * stride, r0, r1, lane, le, run);
        }
    }
}
// 6. the value of every slide at the first m positions: fin[a * stride + j].  suf: elem after k_wsl_run (raw for FIRST / LAST)
__global__ __launch_bounds__(TPB) void k_wsl_fold(DevWslides sl, const uint32_t* __restrict__ rown, const uint32_t* __restrict__ pend, uint32_t n, uint32_t m, size_t stride,
                                                 const uint64_t* __restrict__ suf, const uint64_t* __restrict__ pre, uint64_t* __restrict__ fin) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t rn = rown[j];
        const int64_t e = (int64_t)pend[j], s = (int64_t)j - (int64_t)rn;
        if (s < 0 || e < (int64_t)j || e >= (int64_t)n) continue;           // (s <= j <= e < n: never taken)
#pragma unroll
        for (int a = 0; a < SDQH_WSLIDE_MAX_AGGS; ++a) if (a < sl.n) {
            const DevWslide& d = sl.a[a];
            const int64_t l = max((int64_t)j + d.lo, s), r = min((int64_t)j + d.hi, e);      // (|lo|, |hi| <= n < 2^32: no overflow)
            uint64_t v;
            if (d.g.op == SDQH_WAGG_COUNT) v = l > r ? 0ull : (uint64_t)(r - l + 1);
            else if (l > r) v = d.empty;
            else if (d.g.op == SDQH_WSLIDE_FIRST) v = suf[(size_t)a * stride + (size_t)l];
            else if (d.g.op == SDQH_WSLIDE_LAST) v = suf[(size_t)a * stride + (size_t)r];
            else {
                const uint32_t rl = (uint32_t)(l - s), rr = (uint32_t)(r - s);           // row numbers of the frame's ends
                const uint32_t bl = rl / d.w, br = rr / d.w;
                const uint64_t p = pre[(size_t)a * stride + (size_t)r], q = suf[(size_t)a * stride + (size_t)l];
                // two blocks: the tail of l's and the head of r's; one: l opens it, or else r closes it (a frame shorter than w that
                // does not start at a block's first position was cut at the partition's end, which is its last block's end)
                v = wagg_result(d.g, bl != br ? wagg_join(d.g.cls, q, p) : (rl == bl * d.w ? p : q));
            }
            fin[(size_t)a * stride + j] = v;
        }
    }
}

// ---- value and group frames (sdqh_table_window_range) ----------------------------------------------------------------------------
// The frame of sorted row j is an interval [l, r] of its partition [s, e] whose ends depend on the data: the positions whose ORDER
// BY value (VALUE) or tie-run number (GROUPS) lies within the offsets of row j's.  Both are found by binary search over one ordered
// 64-bit KEY per sorted position — VALUE: the sort key of the one ORDER BY term (the order-preserving image k_sort_keys made,
// ascending with the position whatever the term's direction, from which v(j) is decoded again); GROUPS: the image of the dense rank
// k_win_rank stored — against bounds made without a wrapping add (128-bit integers) or with the one IEEE add (doubles).  COUNT is
// r - l + 1, FIRST / LAST gather the raw element at l / r.  SUM / MIN / MAX read a bottom-up binary FOLD TREE over the sorted
// positions (node k = node 2k (+) node 2k + 1, the leaves at [cap, cap + n), cap = the power of two at or above n): the iterative
// query keeps a left and a right accumulator, joins at most 2 log2(r - l + 1) + 2 nodes in position order, and its association is a
// function of (l, r) and cap alone — rows with the same frame get the same bits, nothing is subtracted, no atomics.  A node that
// covers a position >= n is never read by a query (r < n) and stands for the identity wherever a parent is made of it.
constexpr int WRG_TILE_LEVELS = 9;
static_assert((1 << WRG_TILE_LEVELS) == SORT_TILE && SORT_TILE == 8 * WAVE, "a wave folds its tile's nine levels: three in a lane's registers, six by shuffles");
// g.frame unused; g.cls: WSL_NONE when nothing is folded; slot: which fold tree (a folded range) / raw element array (FIRST, LAST) is
// this range's — each kind numbered from 0 on its own, so a COUNT takes neither and memory is one tree per FOLDED range
struct DevWrange { DevWagg g; int32_t unit, flags; int64_t lo, hi; uint64_t empty; int32_t slot, _pad; };
struct DevWranges { DevWrange a[SDQH_WRANGE_MAX_AGGS]; int32_t n, vcol, vdesc, vf64; };   // vcol: the ORDER BY term of the VALUE ranges (-1: none), its direction and type

// One bounded side of an integer frame: the key a position's key is searched against.  Returns 0: `key` is set; 1: every row of the
// partition lies inside this bound; 2: none does.  tv = v(j) + d * off in 128 bits; beyond int64 it is a bound that no value reaches.
__device__ __forceinline__ int wrg_int_bound(int64_t vj, int64_t off, bool desc, bool lo_side, uint64_t& key) {
    const __int128 tv = (__int128)vj + (desc ? -(__int128)off : (__int128)off);
    const bool over = tv > (__int128)INT64_MAX, under = tv < (__int128)INT64_MIN;
    if (over || under) return ((over != desc) != lo_side) ? 1 : 2;
    key = sort_bits((int64_t)tv, 0, desc ? 1 : 0);
    return 0;
}
// a double bound as a key: the lower end of an IEEE comparison takes -0.0 for a zero, the upper end +0.0, so both zeros are in or out
__device__ __forceinline__ uint64_t wrg_f64_key(double x, bool lower, bool desc) {
    if (x == 0.0) x = lower ? -0.0 : 0.0;
    return sort_bits(__double_as_longlong(x), 1, desc ? 1 : 0);
}
// the first position of [a, b) whose key is >= k (b: none) / > k
__device__ __forceinline__ uint32_t wrg_lower(const uint64_t* __restrict__ key, uint32_t a, uint32_t b, uint64_t k) {
    while (a < b) { const uint32_t mid = a + (b - a) / 2u; if (key[mid] < k) a = mid + 1u; else b = mid; }
    return a;
}
__device__ __forceinline__ uint32_t wrg_upper(const uint64_t* __restrict__ key, uint32_t a, uint32_t b, uint64_t k) {
    while (a < b) { const uint32_t mid = a + (b - a) / 2u; if (key[mid] <= k) a = mid + 1u; else b = mid; }
    return a;
}

// 1. a tile walked backwards (k_wsl_blocks' shape): per position the last position of its partition, the key of the VALUE ranges
// (vkey[r] = the ORDER BY term's sort key of the entry at r; vkey == nullptr: no VALUE range) and of the GROUPS ranges (gkey[r] = the
// image of the dense rank; nullptr: none), and every range's element — raw for FIRST / LAST into elem[slot * stride + r], the fold's
// element for SUM / MIN / MAX into its tree's leaf tree[slot * tstride + cap + r], none for COUNT (perm -> refs -> stage once)
__global__ __launch_bounds__(TPB) void k_wrg_stage(DevStage st, DevWranges rg, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ heads,
                                                  const WaggHeads* __restrict__ tnext, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, uint32_t n, size_t stride,
                                                  size_t tstride, uint64_t cap, uint32_t* __restrict__ pend, uint64_t* __restrict__ vkey, uint64_t* __restrict__ gkey,
                                                  uint64_t* __restrict__ elem, uint64_t* __restrict__ tree, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint32_t next = tnext[w].part;
    for (uint64_t b = r0 + ((r1 - r0 - 1) / WAVE) * WAVE; ; b -= WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        const uint64_t pg = h.mp & ~le;
        const uint32_t pe = (pg ? (uint32_t)b + (uint32_t)__builtin_ctzll(pg) : next) - 1u;
        if (live) {
            const uint32_t g = perm ? perm[r] : (uint32_t)r;
            const bool ok = g < n;                                       // (a permutation of [0, n): always)
            const int64_t idx = ok ? (int64_t)refs[g] : 0;
            const uint32_t hits = ok && st.shits ? st.shits[idx] : 0u;
#pragma unroll
            for (int a = 0; a < SDQH_WRANGE_MAX_AGGS; ++a) if (a < rg.n) {
                const DevWrange& d = rg.a[a];
                if (d.g.op == SDQH_WAGG_COUNT) continue;
                if (d.g.cls == WSL_NONE) elem[(size_t)d.slot * stride + r] = ok ? (uint64_t)sort_raw(d.g.sk, st, idx, hits) : 0ull;
                else tree[(size_t)d.slot * tstride + cap + r] = ok ? wagg_element(d.g, st, idx, hits) : wagg_identity(d.g.cls);
            }
            pend[r] = pe;
            if (vkey) vkey[r] = ok ? keys[g] : 0ull;
            if (gkey) gkey[r] = sort_bits((int64_t)rank[r], 0, 0);
        }
        if (h.mp) next = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (b == r0) break;
    }
}
// 2. the lowest nine levels of every folded range's tree, a wave per tile of SORT_TILE leaves: lane i takes the eight leaves
// [8i, 8i + 8) of the tile (past n: the identity) and folds three levels in its registers, the wave folds six more by shuffles —
// the lane whose number is a multiple of 2^k holds the node over lanes [lane, lane + 2^k) — and every node is stored at its level:
// node (cap >> h) + ((first leaf) >> h) covers 2^h leaves.  Operands stay in position order.
__global__ __launch_bounds__(TPB) void k_wrg_tiles(DevWranges rg, uint32_t n, size_t tstride, uint64_t cap, uint64_t* __restrict__ tree, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
#pragma unroll
    for (int a = 0; a < SDQH_WRANGE_MAX_AGGS; ++a) if (a < rg.n && rg.a[a].g.cls != WSL_NONE) {
        const int cls = rg.a[a].g.cls;
        const uint64_t id = wagg_identity(cls);
        uint64_t* __restrict__ t = tree + (size_t)rg.a[a].slot * tstride;
        const uint64_t p0 = r0 + 8ull * lane;                            // this lane's first leaf
        uint64_t v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p0 + i < r1 ? t[cap + p0 + i] : id;
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = wagg_join(cls, v[2 * i], v[2 * i + 1]); t[(cap >> 1) + (p0 >> 1) + i] = v[i]; }
#pragma unroll
        for (int i = 0; i < 2; ++i) { v[i] = wagg_join(cls, v[2 * i], v[2 * i + 1]); t[(cap >> 2) + (p0 >> 2) + i] = v[i]; }
        uint64_t x = wagg_join(cls, v[0], v[1]);
        t[(cap >> 3) + (p0 >> 3)] = x;
#pragma unroll
        for (int k = 1; k <= WRG_TILE_LEVELS - 3; ++k) {
            const uint64_t o = (uint64_t)__shfl_down((long long)x, 1u << (k - 1), WAVE);
            if ((lane & ((1u << k) - 1u)) == 0u) { x = wagg_join(cls, x, o); t[(cap >> (3 + k)) + (p0 >> (3 + k))] = x; }
        }
    }
}
// 3. workgroup b: the levels above the tiles of tree b (the folded range whose slot is b), one level at a time (a workgroup barrier between two levels:
// every node is written by one thread and read by another of this workgroup).  Level h has cap >> h nodes; node i of it covers the
// tiles from i << (h - 9) on, and one whose first tile is not below ntiles was never written: the identity.
__global__ __launch_bounds__(TPB) void k_wrg_upper(DevWranges rg, size_t tstride, uint64_t cap, uint64_t* __restrict__ tree, uint32_t ntiles) {
    int a = 0;
    while (a < rg.n && !(rg.a[a].g.cls != WSL_NONE && rg.a[a].slot == (int)blockIdx.x)) ++a;
    if (a >= rg.n) return;
    const int cls = rg.a[a].g.cls;
    const uint64_t id = wagg_identity(cls);
    uint64_t* t = tree + (size_t)blockIdx.x * tstride;
    for (int h = WRG_TILE_LEVELS + 1; (cap >> h) >= 1ull; ++h) {
        const uint64_t cnt = cap >> h;                                   // nodes of this level: [cnt, 2 cnt)
        const int up = h - WRG_TILE_LEVELS;                              // a node of it covers 2^up tiles
        const uint64_t live = min(cnt, (((uint64_t)ntiles - 1ull) >> up) + 1ull);      // those whose first tile exists
        for (uint64_t i = threadIdx.x; i < live; i += TPB) {
            const uint64_t right_first = (2ull * i + 1ull) << (up - 1);
            const uint64_t l = t[2ull * (cnt + i)], r = right_first < (uint64_t)ntiles ? t[2ull * (cnt + i) + 1ull] : id;
            t[cnt + i] = wagg_join(cls, l, r);
        }
        __syncthreads();
    }
}
// 4. the value of every range at the first m positions: fin[a * stride + j] — the two ends of the frame searched in [s, e], then
// COUNT / FIRST / LAST off the ends or the tree's iterative query.  rown: k_wsl_rows' (s = j - rown[j]); pend: k_wrg_stage's (e).
__global__ __launch_bounds__(TPB) void k_wrg_fold(DevWranges rg, const uint32_t* __restrict__ rown, const uint32_t* __restrict__ pend, const uint64_t* __restrict__ vkey,
                                                 const uint64_t* __restrict__ gkey, uint32_t n, uint32_t m, size_t stride, size_t tstride, uint64_t cap,
                                                 const uint64_t* __restrict__ elem, const uint64_t* __restrict__ tree, uint64_t* __restrict__ fin) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t rn = rown[j], e = pend[j];
        if ((uint64_t)rn > j || (uint64_t)e < j || e >= n) continue;       // (s <= j <= e < n: never taken)
        const uint32_t s = (uint32_t)j - rn;
#pragma unroll
        for (int a = 0; a < SDQH_WRANGE_MAX_AGGS; ++a) if (a < rg.n) {
            const DevWrange& d = rg.a[a];
            const bool groups = d.unit == SDQH_WRANGE_GROUPS;
            const uint64_t* __restrict__ key = groups ? gkey : vkey;
            const bool desc = !groups && rg.vdesc != 0, f64 = !groups && rg.vf64 != 0;
            const uint64_t kj = key[j];
            // each side: 0 = search for `kl` / `kr`, 1 = the partition's end, 2 = no row at all
            int sl = (d.flags & SDQH_WRANGE_LO_UNBOUNDED) ? 1 : 0, sr = (d.flags & SDQH_WRANGE_HI_UNBOUNDED) ? 1 : 0;
            uint64_t kl = kj, kr = kj;
            if (!f64) {
                const int64_t vj = (int64_t)((desc ? ~kj : kj) ^ (1ull << 63));
                if (sl == 0) sl = wrg_int_bound(vj, d.lo, desc, true, kl);
                if (sr == 0) sr = wrg_int_bound(vj, d.hi, desc, false, kr);
            } else {
                const uint64_t u = desc ? ~kj : kj;
                const double vj = __longlong_as_double((long long)((u >> 63) ? (u ^ (1ull << 63)) : ~u));
                if (vj == vj) {                                          // a NaN row: its own tie run on every bounded side (kl = kr = kj)
                    const double lo = __longlong_as_double(d.lo), hi = __longlong_as_double(d.hi);
                    const double fa = vj + (desc ? -lo : lo), fb = vj + (desc ? -hi : hi);
                    // ascending the lo side is the lower value bound, descending the upper one; with both sides the smaller bounds below
                    double x = desc ? fb : fa, y = desc ? fa : fb;
                    if (sl == 0 && sr == 0 && x > y) { const double t = x; x = y; y = t; }
                    if (desc) { kl = wrg_f64_key(y, false, true); kr = wrg_f64_key(x, true, true); }
                    else { kl = wrg_f64_key(x, true, false); kr = wrg_f64_key(y, false, false); }
                }
            }
            const uint32_t l = sl == 1 ? s : wrg_lower(key, s, e + 1u, kl);
            const uint32_t r1 = sr == 1 ? e + 1u : wrg_upper(key, s, e + 1u, kr);       // one past the frame's last position
            const bool none = sl == 2 || sr == 2 || l >= r1;
            uint64_t v;
            if (d.g.op == SDQH_WAGG_COUNT) v = none ? 0ull : (uint64_t)(r1 - l);
            else if (none) v = d.empty;
            else if (d.g.op == SDQH_WSLIDE_FIRST) v = elem[(size_t)d.slot * stride + l];
            else if (d.g.op == SDQH_WSLIDE_LAST) v = elem[(size_t)d.slot * stride + (r1 - 1u)];
            else {
                const int cls = d.g.cls;
                const uint64_t* __restrict__ t = tree + (size_t)d.slot * tstride;
                uint64_t left = wagg_identity(cls), right = left;
                for (uint64_t p = cap + l, q = cap + r1; p < q; p >>= 1, q >>= 1) {
                    if (p & 1ull) left = wagg_join(cls, left, t[p++]);
                    if (q & 1ull) right = wagg_join(cls, t[--q], right);
                }
                v = wagg_result(d.g, wagg_join(cls, left, right));
            }
            fin[(size_t)a * stride + j] = v;
        }
    }
}

// ---- functions of the partition's size (sdqh_table_window_quantile) --------------------------------------------------------------
// Sorted position j lies in a partition [s, e] of m = e - s + 1 rows at offset i = j - s, inside a tie run [s + f, s + l].  Every
// column is arithmetic on (i, m, f, l) and at most two gathers at positions that arithmetic names: NTILE from i and m; PERCENT_RANK
// f / (m - 1); CUME_DIST (l + 1) / m; NTH, PERCENTILE_DISC and PERCENTILE_CONT read the measure at s + an offset computed from k or
// p and m.  i is k_wsl_rows' row number, e and l come from one backwards pass over the tile (k_wq_stage), f from k_win_rank's RANK
// arm; nothing walks a partition, the work per row does not depend on m.  Columns that name the same measure share one element
// array (a SLOT), so a median and a p90 of one column gather it once.
struct DevWquant { int32_t fn, slot, is_f64, _pad; int64_t arg; double p; uint64_t empty; };     // slot: the element array of the measure (-1: none)
struct DevWquants { DevWquant a[SDQH_WQUANT_MAX_COLS]; DevSortKey slot[SDQH_WQUANT_MAX_COLS]; int32_t n, nslots; };      // slot[k]: measure k (desc unused)

// 1. only with a CUME_DIST column: the first tie head of every tile into tfirst[w].tie, beside the first partition head k_wsl_rows
// left there (it sets .tie to n: none) — what k_wagg_next then scans into the next tie head of the later tiles
__global__ __launch_bounds__(TPB) void k_wq_ties(const uint8_t* __restrict__ heads, uint32_t n, WaggHeads* __restrict__ tfirst, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    uint32_t tie = n;
    for (uint64_t b = r0; b < r1 && tie == n; b += WAVE) {
        const uint64_t r = b + lane_id();
        const uint64_t mt = __ballot(r < r1 && (heads[r] & WIN_TIE));
        if (mt) tie = (uint32_t)b + (uint32_t)__builtin_ctzll(mt);
    }
    if (lane_id() == 0) tfirst[w].tie = tie;
}
// 2. a tile walked backwards (k_wsl_blocks' shape): per position the last position of its partition (pend), of its tie run (tend;
// nullptr: no column asks) — the next head read off the ballots above the lane, else off the batches and tiles behind — and the 64
// bits of every measure (elem[slot * stride + r], read through perm -> refs -> stage exactly once; no slot: nothing is gathered)
__global__ __launch_bounds__(TPB) void k_wq_stage(DevStage st, DevWquants q, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ heads,
                                                 const WaggHeads* __restrict__ tnext, uint32_t n, size_t stride, uint32_t* __restrict__ pend, uint32_t* __restrict__ tend,
                                                 uint64_t* __restrict__ elem, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    WaggHeads next = tnext[w];
    for (uint64_t b = r0 + ((r1 - r0 - 1) / WAVE) * WAVE; ; b -= WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        const uint64_t pg = h.mp & ~le, tg = h.mt & ~le;
        const uint32_t pe = (pg ? (uint32_t)b + (uint32_t)__builtin_ctzll(pg) : next.part) - 1u;
        const uint32_t te = (tg ? (uint32_t)b + (uint32_t)__builtin_ctzll(tg) : next.tie) - 1u;
        if (live) {
            pend[r] = pe;
            if (tend) tend[r] = te;
            if (q.nslots > 0) {
                const uint32_t g = perm ? perm[r] : (uint32_t)r;
                const bool ok = g < n;                                   // (a permutation of [0, n): always)
                const int64_t idx = ok ? (int64_t)refs[g] : 0;
                const uint32_t hits = ok && st.shits ? st.shits[idx] : 0u;
#pragma unroll
                for (int k = 0; k < SDQH_WQUANT_MAX_COLS; ++k) if (k < q.nslots) elem[(size_t)k * stride + r] = ok ? (uint64_t)sort_raw(q.slot[k], st, idx, hits) : 0ull;
            }
        }
        if (h.mp) next.part = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (h.mt) next.tie = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mt);
        if (b == r0) break;
    }
}
// the measure at a position as a double: its bits, or an int64 by one round-to-nearest conversion
__device__ __forceinline__ double wq_f64(uint64_t bits, bool is_f64) { return is_f64 ? __longlong_as_double((long long)bits) : (double)(int64_t)bits; }
// 3. the value of every column at the first m returned rows: fin[c * stride + j], row j = sorted position sel[j] (nullptr: j itself).
// rown: k_wsl_rows' (i); pend / tend: k_wq_stage's (e, s + l); frank: k_win_rank's RANK (f + 1; nullptr: no PERCENT_RANK column)
__global__ __launch_bounds__(TPB) void k_wq_value(DevWquants q, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ rown, const uint32_t* __restrict__ pend,
                                                 const uint32_t* __restrict__ tend, const uint32_t* __restrict__ frank, uint32_t n, uint32_t m, size_t stride,
                                                 const uint64_t* __restrict__ elem, uint64_t* __restrict__ fin) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t pos = sel ? sel[j] : (uint32_t)j;
        if (pos >= n) continue;                                          // (kept positions are positions: never taken)
        const uint32_t rn = rown[pos], e = pend[pos];
        if (rn > pos || e < pos || e >= n) continue;                     // (s <= pos <= e < n: never taken)
        const uint64_t s = (uint64_t)(pos - rn), i = rn, size = (uint64_t)e - s + 1ull;      // the partition's start, the row's offset, m
#pragma unroll
        for (int c = 0; c < SDQH_WQUANT_MAX_COLS; ++c) if (c < q.n) {
            const DevWquant& d = q.a[c];
            const uint64_t* __restrict__ x = elem + (size_t)(d.slot < 0 ? 0 : d.slot) * stride;
            uint64_t v = 0ull;
            if (d.fn == SDQH_WQ_NTILE) {
                const uint64_t b = (uint64_t)d.arg, qq = size / b, r = size % b, big = r * (qq + 1ull);      // (b > m: qq = 0, big = m > i; else big < 2 m)
                v = i < big ? i / (qq + 1ull) + 1ull : r + (i - big) / qq + 1ull;
            } else if (d.fn == SDQH_WQ_PERCENT_RANK) {
                const uint32_t f = frank[pos] - 1u;
                v = (uint64_t)__double_as_longlong(size == 1ull ? 0.0 : (double)f / (double)(size - 1ull));
            } else if (d.fn == SDQH_WQ_CUME_DIST) {
                const uint64_t l1 = (uint64_t)tend[pos] - s + 1ull;     // l + 1: the rows up to the end of the tie run
                v = (uint64_t)__double_as_longlong((double)l1 / (double)size);
            } else if (d.fn == SDQH_WQ_NTH) {
                const uint64_t ak = d.arg < 0 ? 0ull - (uint64_t)d.arg : (uint64_t)d.arg;      // |k|, INT64_MIN included
                v = ak > size ? d.empty : x[d.arg > 0 ? s + ak - 1ull : (uint64_t)e + 1ull - ak];
            } else if (d.fn == SDQH_WQ_PERCENTILE_DISC) {
                const double up = ceil(d.p * (double)size);             // (0 <= p <= 1: 0 <= up <= m)
                const uint64_t at = up >= 1.0 ? min((uint64_t)up - 1ull, size - 1ull) : 0ull;
                v = x[s + at];
            } else {
                const double t = d.p * (double)(size - 1ull), lo = floor(t), hi = ceil(t);      // (0 <= lo <= hi <= m - 1)
                const uint64_t al = min((uint64_t)lo, size - 1ull), ah = min((uint64_t)hi, size - 1ull);
                const double a = wq_f64(x[s + al], d.is_f64 != 0), b = wq_f64(x[s + ah], d.is_f64 != 0);
                // four IEEE operations in this order: the unit is built with -ffp-contract=off, so (b - a) * (t - lo) is not fused into the sum
                const double y = al == ah ? a : a + (b - a) * (t - lo);
                v = (uint64_t)__double_as_longlong(y);
            }
            fin[(size_t)c * stride + j] = v;
        }
    }
}

// ---- frames with rows taken out (sdqh_table_window_exclude) ------------------------------------------------------------------------
// The base frame of sorted row j is an interval [l, r] of its partition [s, e] in the column's own unit — ROWS: arithmetic on j;
// VALUE / GROUPS: the two binary searches of k_wrg_fold over the same keys — and what EXCLUDE removes is an interval around j too:
// {j}, or j's tie run [a, b] (a from k_win_rank's RANK arm, b from k_wex_ties), with or without j itself.  What remains is at most
// three pieces in position order, [l, min(r, x0 - 1)], {j}, [max(l, x1 + 1), r]: COUNT adds their lengths, FIRST / LAST gather at
// the first / last remaining position, SUM / MIN / MAX / AVG ask the fold tree of the ranges (k_wrg_stage / _tiles / _upper build
// it from the columns' DevWranges image, an AVG staged as the SUM it divides) once per piece with k_wrg_fold's iterative query and
// join the answers left to right: exactly the remaining rows enter, once each, nothing is subtracted, and the association is a
// function of the pieces' ends and cap alone.  With nothing excluded the one piece is the frame and the bits are k_wrg_fold's.
struct DevWexs { DevWranges rg; int32_t exclude[SDQH_WEX_MAX_COLS]; int32_t avg[SDQH_WEX_MAX_COLS]; };      // rg: the image (a[c].unit may be SDQH_WEX_ROWS: lo / hi clamped to [-n, n]; an AVG has op SUM there)
static_assert(SDQH_WEX_MAX_COLS == SDQH_WRANGE_MAX_AGGS, "the columns of an exclude call are the ranges of its image");

// 1. only with a GROUP / TIES column: a tile walked backwards (k_wq_stage's shape), per position the last position of its tie run —
// the next tie head read off the ballots above the lane, else off the batches and tiles behind (tnext: k_wagg_next's, over the
// first tie heads k_wq_ties left)
__global__ __launch_bounds__(TPB) void k_wex_ties(const uint8_t* __restrict__ heads, const WaggHeads* __restrict__ tnext, uint32_t n, uint32_t* __restrict__ tend, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint32_t next = tnext[w].tie;
    for (uint64_t b = r0 + ((r1 - r0 - 1) / WAVE) * WAVE; ; b -= WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(heads, r, live, le);
        const uint64_t tg = h.mt & ~le;
        if (live) tend[r] = (tg ? (uint32_t)b + (uint32_t)__builtin_ctzll(tg) : next) - 1u;
        if (h.mt) next = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mt);
        if (b == r0) break;
    }
}
// the base frame [l, r1) of row j in [s, e] (false: no row): ROWS by arithmetic, VALUE / GROUPS as k_wrg_fold finds it
__device__ __forceinline__ bool wex_ends(const DevWrange& d, const DevWranges& rg, const uint64_t* __restrict__ vkey, const uint64_t* __restrict__ gkey,
                                         uint64_t j, uint32_t s, uint32_t e, uint32_t& l, uint32_t& r1) {
    if (d.unit == SDQH_WEX_ROWS) {                                       // (|lo|, |hi| <= n < 2^32: no overflow)
        const int64_t a = (d.flags & SDQH_WRANGE_LO_UNBOUNDED) ? (int64_t)s : max((int64_t)j + d.lo, (int64_t)s);
        const int64_t b = (d.flags & SDQH_WRANGE_HI_UNBOUNDED) ? (int64_t)e : min((int64_t)j + d.hi, (int64_t)e);
        if (a > b) return false;
        l = (uint32_t)a; r1 = (uint32_t)b + 1u;
        return true;
    }
    const bool groups = d.unit == SDQH_WRANGE_GROUPS;
    const uint64_t* __restrict__ key = groups ? gkey : vkey;
    const bool desc = !groups && rg.vdesc != 0, f64 = !groups && rg.vf64 != 0;
    const uint64_t kj = key[j];
    int sl = (d.flags & SDQH_WRANGE_LO_UNBOUNDED) ? 1 : 0, sr = (d.flags & SDQH_WRANGE_HI_UNBOUNDED) ? 1 : 0;      // k_wrg_fold's sides
    uint64_t kl = kj, kr = kj;
    if (!f64) {
        const int64_t vj = (int64_t)((desc ? ~kj : kj) ^ (1ull << 63));
        if (sl == 0) sl = wrg_int_bound(vj, d.lo, desc, true, kl);
        if (sr == 0) sr = wrg_int_bound(vj, d.hi, desc, false, kr);
    } else {
        const uint64_t u = desc ? ~kj : kj;
        const double vj = __longlong_as_double((long long)((u >> 63) ? (u ^ (1ull << 63)) : ~u));
        if (vj == vj) {
            const double lo = __longlong_as_double(d.lo), hi = __longlong_as_double(d.hi);
            const double fa = vj + (desc ? -lo : lo), fb = vj + (desc ? -hi : hi);
            double x = desc ? fb : fa, y = desc ? fa : fb;
            if (sl == 0 && sr == 0 && x > y) { const double t = x; x = y; y = t; }
            if (desc) { kl = wrg_f64_key(y, false, true); kr = wrg_f64_key(x, true, true); }
            else { kl = wrg_f64_key(x, true, false); kr = wrg_f64_key(y, false, false); }
        }
    }
    l = sl == 1 ? s : wrg_lower(key, s, e + 1u, kl);
    r1 = sr == 1 ? e + 1u : wrg_upper(key, s, e + 1u, kr);
    return sl != 2 && sr != 2 && l < r1;
}
// the fold of tree t over the positions [a, b] (a <= b < n): k_wrg_fold's iterative query
__device__ __forceinline__ uint64_t wex_query(int cls, const uint64_t* __restrict__ t, uint64_t cap, int64_t a, int64_t b) {
    uint64_t left = wagg_identity(cls), right = left;
    for (uint64_t p = cap + (uint64_t)a, q = cap + (uint64_t)b + 1ull; p < q; p >>= 1, q >>= 1) {
        if (p & 1ull) left = wagg_join(cls, left, t[p++]);
        if (q & 1ull) right = wagg_join(cls, t[--q], right);
    }
    return wagg_join(cls, left, right);
}
// 2. the value of every column at the first m positions: fin[c * stride + j].  rown: k_wsl_rows' (s = j - rown[j]); pend, vkey, gkey,
// elem, tree: k_wrg_stage's; frank: k_win_rank's RANK (a = s + frank[j] - 1) and tend: k_wex_ties' (b) — both nullptr when no column
// excludes GROUP or TIES
__global__ __launch_bounds__(TPB) void k_wex_fold(DevWexs ex, const uint32_t* __restrict__ rown, const uint32_t* __restrict__ pend, const uint32_t* __restrict__ frank,
                                                 const uint32_t* __restrict__ tend, const uint64_t* __restrict__ vkey, const uint64_t* __restrict__ gkey, uint32_t n, uint32_t m,
                                                 size_t stride, size_t tstride, uint64_t cap, const uint64_t* __restrict__ elem, const uint64_t* __restrict__ tree,
                                                 uint64_t* __restrict__ fin) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t rn = rown[j], e = pend[j];
        if ((uint64_t)rn > j || (uint64_t)e < j || e >= n) continue;       // (s <= j <= e < n: never taken)
        const uint32_t s = (uint32_t)j - rn;
        int64_t ta = (int64_t)j, tb = (int64_t)j;                         // the tie run [ta, tb]
        if (frank) {
            const int64_t a = (int64_t)s + (int64_t)frank[j] - 1, b = (int64_t)tend[j];
            if (a >= (int64_t)s && a <= (int64_t)j && b >= (int64_t)j && b <= (int64_t)e) { ta = a; tb = b; }      // (s <= a <= j <= b <= e: always)
        }
#pragma unroll
        for (int c = 0; c < SDQH_WEX_MAX_COLS; ++c) if (c < ex.rg.n) {
            const DevWrange& d = ex.rg.a[c];
            const int x = ex.exclude[c];
            uint32_t l = 0u, r1 = 0u;
            const bool any = wex_ends(d, ex.rg, vkey, gkey, j, s, e, l, r1);
            // the pieces [a1, b1], {j} (mid), [a3, b3]; an empty one has its end below its start
            int64_t a1 = 0, b1 = -1, a3 = 0, b3 = -1;
            bool mid = false;
            if (any) {
                const int64_t fl = (int64_t)l, fr = (int64_t)r1 - 1;
                const int64_t x0 = x == SDQH_WEX_NO_OTHERS ? fr + 1 : (x == SDQH_WEX_CURRENT_ROW ? (int64_t)j : ta);
                const int64_t x1 = x == SDQH_WEX_NO_OTHERS ? fr : (x == SDQH_WEX_CURRENT_ROW ? (int64_t)j : tb);
                a1 = fl; b1 = min(fr, x0 - 1); a3 = max(fl, x1 + 1); b3 = fr;
                mid = x == SDQH_WEX_TIES && fl <= (int64_t)j && (int64_t)j <= fr;
            }
            const bool p1 = a1 <= b1, p3 = a3 <= b3;
            const uint64_t count = (p1 ? (uint64_t)(b1 - a1 + 1) : 0ull) + (mid ? 1ull : 0ull) + (p3 ? (uint64_t)(b3 - a3 + 1) : 0ull);
            uint64_t v;
            if (d.g.op == SDQH_WAGG_COUNT) v = count;
            else if (count == 0ull) v = d.empty;
            else if (d.g.op == SDQH_WSLIDE_FIRST) v = elem[(size_t)d.slot * stride + (size_t)(p1 ? a1 : (mid ? (int64_t)j : a3))];
            else if (d.g.op == SDQH_WSLIDE_LAST) v = elem[(size_t)d.slot * stride + (size_t)(p3 ? b3 : (mid ? (int64_t)j : b1))];
            else {
                const int cls = d.g.cls;
                const uint64_t* __restrict__ t = tree + (size_t)d.slot * tstride;
                uint64_t acc = 0ull;
                bool have = false;
                if (p1) { acc = wex_query(cls, t, cap, a1, b1); have = true; }
                if (mid) { const uint64_t q = wex_query(cls, t, cap, (int64_t)j, (int64_t)j); acc = have ? wagg_join(cls, acc, q) : q; have = true; }
                if (p3) { const uint64_t q = wex_query(cls, t, cap, a3, b3); acc = have ? wagg_join(cls, acc, q) : q; }
                if (ex.avg[c]) {                                         // the column's own SUM as a double, one division
                    const double sum = d.g.sk.is_f64 ? __longlong_as_double((long long)acc) : (double)(int64_t)acc;
                    v = (uint64_t)__double_as_longlong(sum / (double)count);
                } else v = wagg_result(d.g, acc);
            }
            fin[(size_t)c * stride + j] = v;
        }
    }
}

// ---- groups at nested levels (sdqh_table_grouping_sets) ---------------------------------------------------------------------------
// The DEPTH of sorted position r is the number of leading terms whose keys equal those of r - 1 (position 0: 0).  r opens a level-L
// group iff r == 0 or depth[r] < L, so one byte per position holds the heads of every level.  The levels asked for are folded from
// the highest down: the highest over the rows (k_wagg_tiles' elements and tile carries, k_wagg_scan, then k_gs_run in the place of
// k_wagg_run: the value at a group's last row goes to the group's slot), every lower one over the GROUPS of the level above it, which
// carry their first row's depth and sorted position along — the same three passes (k_gs_tiles / k_wagg_scan / k_gs_run) over an
// array as long as that level's group count, not n.  All levels write into one set of arrays, highest level first: the positions
// are the emit's `sel`, the values the call's columns.  COUNT is a sum of ones, an AVG is folded as its SUM and divided at the end
// by the count read off the positions (k_gs_avg).  No atomics: a group's slot is its head's rank among the heads.
struct DevGsLevels { uint32_t off[SDQH_SORT_MAX_KEYS + 2]; int32_t n, _pad; };      // level k's groups are rows [off[k], off[k + 1]) of the output
struct DevGsAvg { int32_t avg[SDQH_GS_MAX_AGGS], is_f64[SDQH_GS_MAX_AGGS]; };
static_assert(SDQH_GS_MAX_AGGS == SDQH_WAGG_MAX_AGGS, "the groups' folds are the frames'");

// a group's value as k_gs_run left it (wagg_result) back as an element of its class
__device__ __forceinline__ uint64_t gs_element(const DevWagg& g, uint64_t v) {
    if (g.cls != WAGG_UMAX) return v;
    if (g.sk.is_f64) { const double d = __longlong_as_double((long long)v); if (d != d) return 0ull; }
    return sort_bits((int64_t)v, g.sk.is_f64, g.op == SDQH_WAGG_MIN);
}
// the heads of level L among 64 items at [b, ..): item j is one iff j == 0 or depth[j] < L
struct GsBatch { uint64_t mh, hl; uint32_t first, d; bool head, last; };
__device__ __forceinline__ GsBatch gs_batch(const uint8_t* __restrict__ depth, int L, uint64_t j, uint64_t r1, uint32_t n, uint64_t le) {
    GsBatch h;
    const bool live = j < r1;
    h.d = live ? depth[j] : 255u;
    h.head = live && (j == 0 || (int)h.d < L);
    h.last = live && (j + 1 >= n || (int)depth[j + 1] < L);              // the item closes its group
    h.mh = __ballot(h.head);
    h.hl = h.mh & le;
    h.first = h.hl ? 63u - (uint32_t)__clzll((long long)h.hl) : 0u;
    return h;
}

// 1. the depth of every position, the head flags of level `top` as k_wagg_tiles reads them, and per tile and level 0 .. nterms the
// number of heads: tcount[L * ntiles + tile]
__global__ __launch_bounds__(TPB) void k_gs_depth(const uint64_t* __restrict__ keys, size_t key_stride, int nterms, int top, const uint32_t* __restrict__ perm, uint32_t n,
                                                 uint8_t* __restrict__ depth, uint8_t* __restrict__ heads, uint32_t* __restrict__ tcount, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    uint32_t cnt[SDQH_SORT_MAX_KEYS + 1];
#pragma unroll
    for (int L = 0; L <= SDQH_SORT_MAX_KEYS; ++L) cnt[L] = 0u;
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane_id();
        const bool live = r < r1;
        int d = 0;
        if (live && r > 0) {
            const uint32_t g = perm ? perm[r] : (uint32_t)r, h = perm ? perm[r - 1] : (uint32_t)(r - 1);
            if (g < n && h < n)                                          // (a permutation of [0, n): always)
                while (d < nterms && keys[(size_t)d * key_stride + g] == keys[(size_t)d * key_stride + h]) ++d;
        }
        if (live) {
            depth[r] = (uint8_t)d;
            heads[r] = (uint8_t)((r == 0 || d < top) ? (WIN_PART | WIN_TIE) : 0u);
        }
#pragma unroll
        for (int L = 0; L <= SDQH_SORT_MAX_KEYS; ++L) cnt[L] += (uint32_t)__popcll(__ballot(live && (r == 0 || d < L)));
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int L = 0; L <= SDQH_SORT_MAX_KEYS; ++L) if (L <= nterms) tcount[(size_t)L * ntiles + w] = cnt[L];
    }
}
// 2. a lower level over the n groups of the level above it (depth / val: theirs): per tile and aggregate the carry — the elements
// folded since the tile's last head of level L, or over the whole tile — the tile's first head (what k_wagg_scan reads) and its
// number of heads
__global__ __launch_bounds__(TPB) void k_gs_tiles(DevWaggs ag, int L, const uint8_t* __restrict__ depth, const uint64_t* __restrict__ val, size_t stride, uint32_t n,
                                                 uint64_t* __restrict__ tval, WaggHeads* __restrict__ tfirst, uint32_t* __restrict__ tcnt, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint64_t run[SDQH_WAGG_MAX_AGGS];
#pragma unroll
    for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) run[a] = wagg_identity(ag.a[a].cls);
    WaggHeads fh = {n, n};
    uint32_t cnt = 0u;
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t j = b + lane;
        const GsBatch h = gs_batch(depth, L, j, r1, n, le);
        if (h.mh && fh.part == n) fh.part = fh.tie = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mh);
        cnt += (uint32_t)__popcll(h.mh);
        const int last = (int)min((uint64_t)WAVE, r1 - b) - 1;
#pragma unroll
        for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n) {
            const int cls = ag.a[a].cls;
            const uint64_t e = j < r1 ? gs_element(ag.a[a], val[(size_t)a * stride + j]) : wagg_identity(cls);
            const uint64_t s = wagg_wave_scan(cls, e, lane, h.first);
            const uint64_t tail = (uint64_t)__shfl((long long)s, last, WAVE);
            run[a] = h.mh ? tail : wagg_join(cls, run[a], tail);
        }
    }
    if (lane == 0) {
        tfirst[w] = fh; tcnt[w] = cnt;
#pragma unroll
        for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n) tval[(size_t)a * ntiles + w] = run[a];
    }
}
// 3. the tile again with its carry-in (tval: k_wagg_scan's) and the number of heads before it (toff): k_wagg_run's scan, but only
// the value at a group's last item is kept — in slot toff + heads up to the item - 1 of the level's part of the output, where the
// group's head leaves its depth and sorted position.  elems: val holds elements (the rows', k_wagg_tiles'), not group values;
// pos == nullptr: item j is sorted position j.  A slot at or past `ng` is not written.
__global__ __launch_bounds__(TPB) void k_gs_run(DevWaggs ag, int L, int elems, const uint8_t* __restrict__ depth, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ val, size_t stride,
                                               uint32_t n, const uint64_t* __restrict__ tval, const uint32_t* __restrict__ toff, uint32_t ntiles,
                                               uint64_t* __restrict__ oval, size_t ostride, uint8_t* __restrict__ odepth, uint32_t* __restrict__ opos, uint32_t ng) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint64_t run[SDQH_WAGG_MAX_AGGS];
#pragma unroll
    for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) run[a] = a < ag.n ? tval[(size_t)a * ntiles + w] : 0ull;
    uint32_t at0 = toff[w];
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t j = b + lane;
        const bool live = j < r1;
        const GsBatch h = gs_batch(depth, L, j, r1, n, le);
        const uint32_t slot = at0 + (uint32_t)__popcll(h.hl) - 1u;       // (position 0 is a head: at least one lies at or below every item)
        const bool ok = slot < ng;
        if (h.head && ok) { odepth[slot] = (uint8_t)(j == 0 ? 0u : h.d); opos[slot] = pos ? pos[j] : (uint32_t)j; }
        const int last = (int)min((uint64_t)WAVE, r1 - b) - 1;
#pragma unroll
        for (int a = 0; a < SDQH_WAGG_MAX_AGGS; ++a) if (a < ag.n) {
            const int cls = ag.a[a].cls;
            uint64_t e = wagg_identity(cls);
            if (live) { e = val[(size_t)a * stride + j]; if (!elems) e = gs_element(ag.a[a], e); }
            const uint64_t s = wagg_wave_scan(cls, e, lane, h.first);
            const uint64_t v = h.hl ? s : wagg_join(cls, run[a], s);
            if (h.last && ok) oval[(size_t)a * ostride + slot] = wagg_result(ag.a[a], v);
            run[a] = (uint64_t)__shfl((long long)v, last, WAVE);
        }
        at0 += (uint32_t)__popcll(h.mh);
    }
}
// 4. the averages of the first m output rows, in place: the SUM in the slot converted to double and divided by the group's size —
// the distance to the next representative of its level, or to n
__global__ __launch_bounds__(TPB) void k_gs_avg(DevGsAvg av, DevGsLevels lv, const uint32_t* __restrict__ pos, uint32_t n, uint32_t m, size_t stride, uint64_t* __restrict__ val) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        int k = 0;
        while (k + 1 < lv.n && j >= lv.off[k + 1]) ++k;
        const uint32_t next = j + 1 < lv.off[k + 1] ? pos[j + 1] : n;
        const double cnt = (double)(next - pos[j]);
#pragma unroll
        for (int a = 0; a < SDQH_GS_MAX_AGGS; ++a) if (av.avg[a]) {
            const uint64_t s = val[(size_t)a * stride + j];
            const double sum = av.is_f64[a] ? __longlong_as_double((long long)s) : (double)(int64_t)s;
            val[(size_t)a * stride + j] = (uint64_t)__double_as_longlong(sum / cnt);
        }
    }
}

// ---- aggregates over the distinct values of a group (sdqh_table_group_distinct) ----------------------------------------------------
// The first ngroup terms group, all nterms terms make the value: a VALUE RUN is a level-nterms group, a GROUP a level-ngroup one, and
// k_gs_depth's byte holds the heads of both.  Two stages.  The lower one turns the rows into runs: a run's slot is its head's rank
// among the run heads (k_gd_heads), its length the distance to the next run's head, and per aggregate it leaves the element the upper
// stage folds (k_gd_elems) — 1 for COUNT_DISTINCT, the length for COUNT, the measure's bits at the run's first row for SUM / AVG, and
// for MODE / MODE_COUNT one word, (length << 32) | (0xFFFFFFFF - sorted position), whose unsigned maximum is the longest and then the
// earliest run.  The upper one is the grouping sets' "a lower level over the groups of the level above it", unchanged: k_gs_tiles /
// k_wagg_scan / k_sort_bins / k_gs_run at level ngroup over an array as long as the number of runs.  The MODE word is folded by
// WAGG_UMAX as it stands — as the signed image of a MAX over int64, which those passes encode to the word and decode again — so no
// new fold class is needed.  k_gd_finish then gives every group its sorted position, unpacks the MODE word (the measure gathered
// through the permutation at the winning position) and divides an AVG by the group's own number of runs.  No atomics.
struct DevGdAggs { DevSortKey sk[SDQH_GD_MAX_AGGS]; int32_t op[SDQH_GD_MAX_AGGS]; int32_t n, _pad; };      // sk: the measure (desc unused)
static_assert(SDQH_GD_MAX_AGGS == SDQH_WAGG_MAX_AGGS, "the distinct folds are the frames'");
constexpr unsigned long long GD_SIGN = 1ull << 63;

// the 64 bits of measure sk at sorted position p (p < n)
__device__ __forceinline__ uint64_t gd_measure(const DevSortKey& sk, const DevStage& st, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, uint32_t p, uint32_t n) {
    const uint32_t g = perm ? perm[p] : p;
    if (g >= n) return 0ull;                                             // (a permutation of [0, n): never taken)
    const int64_t idx = (int64_t)refs[g];
    const uint32_t hits = st.shits ? st.shits[idx] : 0u;
    return (uint64_t)sort_raw(sk, st, idx, hits);
}

// 1. a wave per tile of sorted positions: the head of value run s (its rank among the level-`top` heads: toff — k_sort_bins' — plus
// the heads up to it in the tile) leaves its sorted position and its depth in slot s.  A slot at or past nr is not written.
__global__ __launch_bounds__(TPB) void k_gd_heads(int top, const uint8_t* __restrict__ depth, uint32_t n, const uint32_t* __restrict__ toff, uint32_t ntiles,
                                                 uint32_t* __restrict__ rpos, uint8_t* __restrict__ rdepth, uint32_t nr) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint64_t le = lanemask_lt() | (1ull << (uint32_t)lane_id());
    uint32_t at0 = toff[w];
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t j = b + (uint32_t)lane_id();
        const GsBatch h = gs_batch(depth, top, j, r1, n, le);
        const uint32_t slot = at0 + (uint32_t)__popcll(h.hl) - 1u;
        if (h.head && slot < nr) { rpos[slot] = (uint32_t)j; rdepth[slot] = (uint8_t)(j == 0 ? 0u : h.d); }
        at0 += (uint32_t)__popcll(h.mh);
    }
}
// 2. a thread per value run: its length and every aggregate's element, as a group value of the aggregate's fold class (what
// k_gs_tiles and k_gs_run read with elems == 0)
__global__ __launch_bounds__(TPB) void k_gd_elems(DevStage st, DevGdAggs gd, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ rpos,
                                                 uint32_t n, uint32_t nr, size_t stride, uint64_t* __restrict__ elem) {
    for (uint64_t s = (uint64_t)blockIdx.x * TPB + threadIdx.x; s < nr; s += (uint64_t)gridDim.x * TPB) {
        const uint32_t p = rpos[s];
        const uint32_t next = s + 1 < nr ? rpos[s + 1] : n;
        const uint64_t len = (uint64_t)(next - p);
#pragma unroll
        for (int a = 0; a < SDQH_GD_MAX_AGGS; ++a) if (a < gd.n) {
            const int op = gd.op[a];
            uint64_t e;
            if (op == SDQH_GD_COUNT_DISTINCT) e = 1ull;
            else if (op == SDQH_GD_COUNT) e = len;
            else if (op == SDQH_GD_MODE || op == SDQH_GD_MODE_COUNT) e = ((len << 32) | (uint64_t)(0xFFFFFFFFu - p)) ^ GD_SIGN;
            else e = p < n ? gd_measure(gd.sk[a], st, refs, perm, p, n) : 0ull;
            elem[(size_t)a * stride + s] = e;
        }
    }
}
// 3. a thread per returned group: gfirst[j] (k_gs_run's positions over the runs) is the group's first run — its sorted position
// goes to sel, the distance to the next group's first run (or to nr) is its number of runs; MODE / MODE_COUNT are unpacked and an
// AVG divided, in place
__global__ __launch_bounds__(TPB) void k_gd_finish(DevStage st, DevGdAggs gd, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ rpos,
                                                  const uint32_t* __restrict__ gfirst, uint32_t n, uint32_t nr, uint32_t ng, uint32_t m, size_t stride,
                                                  uint64_t* __restrict__ val, uint32_t* __restrict__ sel) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t f = gfirst[j];
        const uint32_t next = j + 1 < ng ? gfirst[j + 1] : nr;
        if (f >= nr) continue;                                           // (a run index: never taken)
        sel[j] = rpos[f];
        const double runs = (double)(next - f);
#pragma unroll
        for (int a = 0; a < SDQH_GD_MAX_AGGS; ++a) if (a < gd.n) {
            const int op = gd.op[a];
            const uint64_t v = val[(size_t)a * stride + j];
            if (op == SDQH_GD_MODE_COUNT) val[(size_t)a * stride + j] = (v ^ GD_SIGN) >> 32;
            else if (op == SDQH_GD_MODE) {
                const uint32_t p = 0xFFFFFFFFu - (uint32_t)((v ^ GD_SIGN) & 0xFFFFFFFFull);
                val[(size_t)a * stride + j] = p < n ? gd_measure(gd.sk[a], st, refs, perm, p, n) : 0ull;
            } else if (op == SDQH_GD_AVG_DISTINCT) {
                const double sum = gd.sk[a].is_f64 ? __longlong_as_double((long long)v) : (double)(int64_t)v;
                val[(size_t)a * stride + j] = (uint64_t)__double_as_longlong(sum / runs);
            }
        }
    }
}

// ---- second moments per group (sdqh_table_group_moments) ---------------------------------------------------------------------------
// VAR / STDDEV / COVAR / CORR / REGR per group at the levels of GROUPS, by the two-pass algorithm (include/sdqh_sort_moments.h).  A
// variance is no fold of one 64-bit element per row: sum x^2 - (sum x)^2 / m cancels, merged (n, mean, M2) states are a multi-word
// operator and less accurate.  Two folds of doubles are: per level L asked for, over the ROWS (a coarser level's mean is another
// mean, so nothing folds from the level above),
//   k_gd_heads        the level's groups: slot = the head's rank among the level-L heads, its sorted position — the representative
//   k_mo_stage        per position the call's distinct measures (at most two per aggregate; aggregates naming the same measure share
//                     a column) read through perm -> refs -> stage once, converted to double, minus the representative's: s = x - x_r
//   k_gs_tiles / k_wagg_scan / k_gs_run
//                     pass 1: the s folded per group as WAGG_ADD_F elements, at most SDQH_WAGG_MAX_AGGS columns a launch
//   k_mo_center       per position its group's slot again, mu = S / m (m off the positions), d = s - mu per measure, and the
//                     elements of pass 2: d * d per measure an aggregate needs a Q of, dx * dy per pair
//   k_gs_tiles / k_wagg_scan / k_gs_run
//                     pass 2: those folded per group, the same way
// and at the end k_mo_finish, a thread per returned group, applies the op's formula.  A wave's lanes mostly share a slot, so the
// loads of the representative and of the group's sums broadcast.  No atomics; the level's tile offsets are k_sort_bins' (tcount).
constexpr int MO_MAX_MEAS = 2 * SDQH_GM_MAX_AGGS, MO_MAX_CEN = 3 * SDQH_GM_MAX_AGGS;
struct DevMoAggs {
    DevSortKey sk[MO_MAX_MEAS];                                       // the distinct measures (desc unused)
    int32_t ci[MO_MAX_CEN], cj[MO_MAX_CEN];                           // pass 2's column c: d of measure ci[c] times d of measure cj[c]
    int32_t op[SDQH_GM_MAX_AGGS], my[SDQH_GM_MAX_AGGS], mx[SDQH_GM_MAX_AGGS];                  // per aggregate: the op, its measures
    int32_t qy[SDQH_GM_MAX_AGGS], qx[SDQH_GM_MAX_AGGS], cc[SDQH_GM_MAX_AGGS];                  // ... and its columns of pass 2 (-1: not read)
    int32_t nmeas, ncen, n, _pad;
};

__device__ __forceinline__ double mo_f64(uint64_t bits) { return __longlong_as_double((long long)bits); }
__device__ __forceinline__ uint64_t mo_bits(double d) { return (uint64_t)__double_as_longlong(d); }
// measure sk of staged row idx as a double: an integer by one conversion
__device__ __forceinline__ double mo_value(const DevSortKey& sk, const DevStage& st, int64_t idx, uint32_t hits) {
    const int64_t raw = sort_raw(sk, st, idx, hits);
    return sk.is_f64 ? __longlong_as_double(raw) : (double)raw;
}

// 1. a wave per tile of sorted positions: elem[k * stride + r] = measure k at position r minus measure k at the representative of
// r's level-L group.  toff: the level-L heads before the tile, lpos: the sorted position of every level-L group (ng of them).
__global__ __launch_bounds__(TPB) void k_mo_stage(DevStage st, DevMoAggs mo, int L, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ depth,
                                                 const uint32_t* __restrict__ toff, const uint32_t* __restrict__ lpos, uint32_t ng, uint32_t n, size_t stride,
                                                 uint64_t* __restrict__ elem, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint64_t le = lanemask_lt() | (1ull << (uint32_t)lane_id());
    uint32_t at0 = toff[w];
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t j = b + (uint32_t)lane_id();
        const bool live = j < r1;
        const GsBatch h = gs_batch(depth, L, j, r1, n, le);
        const uint32_t slot = at0 + (uint32_t)__popcll(h.hl) - 1u;       // (position 0 is a head: at least one lies at or below every item)
        const uint32_t rp = (live && slot < ng) ? lpos[slot] : n;
        const uint32_t g = live ? (perm ? perm[j] : (uint32_t)j) : n;
        const uint32_t gr = rp < n ? (perm ? perm[rp] : rp) : n;
        const bool ok = g < n && gr < n;                                 // (positions and a permutation of [0, n): every live lane)
        const int64_t idx = ok ? (int64_t)refs[g] : 0, idr = ok ? (int64_t)refs[gr] : 0;
        const uint32_t hits = ok && st.shits ? st.shits[idx] : 0u, hitr = ok && st.shits ? st.shits[idr] : 0u;
#pragma unroll
        for (int k = 0; k < MO_MAX_MEAS; ++k) if (k < mo.nmeas) {
            const double s = ok ? mo_value(mo.sk[k], st, idx, hits) - mo_value(mo.sk[k], st, idr, hitr) : 0.0;
            if (live) elem[(size_t)k * stride + j] = mo_bits(s);
        }
        at0 += (uint32_t)__popcll(h.mh);
    }
}
// 2. the tile again: position r's group is slot toff + heads up to r - 1, its size the distance to the next group's position (or to
// n), its shifted means sums / size; cen[c * stride + r] = d_ci * d_cj with d_k = elem[k] - mean_k.  sums: pass 1's, gstride apart.
__global__ __launch_bounds__(TPB) void k_mo_center(DevMoAggs mo, int L, const uint8_t* __restrict__ depth, const uint32_t* __restrict__ toff, const uint32_t* __restrict__ lpos,
                                                  uint32_t ng, uint32_t n, size_t stride, const uint64_t* __restrict__ elem, size_t gstride, const uint64_t* __restrict__ sums,
                                                  uint64_t* __restrict__ cen, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint64_t le = lanemask_lt() | (1ull << (uint32_t)lane_id());
    uint32_t at0 = toff[w];
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t j = b + (uint32_t)lane_id();
        const GsBatch h = gs_batch(depth, L, j, r1, n, le);
        const uint32_t slot = at0 + (uint32_t)__popcll(h.hl) - 1u;
        if (j < r1 && slot < ng) {
            const uint32_t next = slot + 1u < ng ? lpos[slot + 1u] : n;
            const double size = (double)(next - lpos[slot]);
#pragma unroll
            for (int c = 0; c < MO_MAX_CEN; ++c) if (c < mo.ncen) {
                const int ki = mo.ci[c], kj = mo.cj[c];
                const double di = mo_f64(elem[(size_t)ki * stride + j]) - mo_f64(sums[(size_t)ki * gstride + slot]) / size;
                const double dj = mo_f64(elem[(size_t)kj * stride + j]) - mo_f64(sums[(size_t)kj * gstride + slot]) / size;
                cen[(size_t)c * stride + j] = mo_bits(di * dj);
            }
        }
        at0 += (uint32_t)__popcll(h.mh);
    }
}
// 3. a thread per returned group: the op's formula, in the header's order of operations, on pass 2's sums (cen), pass 1's (sums),
// the representative's measures and the group's size — the distance to the next representative of its level, or to n
__global__ __launch_bounds__(TPB) void k_mo_finish(DevStage st, DevMoAggs mo, DevGsLevels lv, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pos,
                                                  uint32_t n, uint32_t m, size_t gstride, const uint64_t* __restrict__ sums, const uint64_t* __restrict__ cen, uint64_t* __restrict__ val) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        int k = 0;
        while (k + 1 < lv.n && j >= lv.off[k + 1]) ++k;
        const uint32_t p = pos[j];
        const uint32_t next = j + 1 < lv.off[k + 1] ? pos[j + 1] : n;
        const uint32_t rows = next - p;
        const double size = (double)rows;
        const uint32_t g = p < n ? (perm ? perm[p] : p) : n;
        if (g >= n) continue;                                            // (a position and a permutation of [0, n): never taken)
        const int64_t idx = (int64_t)refs[g];
        const uint32_t hits = st.shits ? st.shits[idx] : 0u;
#pragma unroll
        for (int a = 0; a < SDQH_GM_MAX_AGGS; ++a) if (a < mo.n) {
            const int op = mo.op[a];
            const double qy = mo.qy[a] >= 0 ? mo_f64(cen[(size_t)mo.qy[a] * gstride + j]) : 0.0;
            const double qx = mo.qx[a] >= 0 ? mo_f64(cen[(size_t)mo.qx[a] * gstride + j]) : 0.0;
            const double c = mo.cc[a] >= 0 ? mo_f64(cen[(size_t)mo.cc[a] * gstride + j]) : 0.0;
            uint64_t out = WAGG_QNAN;
            if (op == SDQH_GM_VAR_POP) out = mo_bits(qy / size);
            else if (op == SDQH_GM_STDDEV_POP) out = mo_bits(sqrt(qy / size));
            else if (op == SDQH_GM_COVAR_POP) out = mo_bits(c / size);
            else if (op == SDQH_GM_VAR_SAMP) { if (rows > 1u) out = mo_bits(qy / (size - 1.0)); }
            else if (op == SDQH_GM_STDDEV_SAMP) { if (rows > 1u) out = mo_bits(sqrt(qy / (size - 1.0))); }
            else if (op == SDQH_GM_COVAR_SAMP) { if (rows > 1u) out = mo_bits(c / (size - 1.0)); }
            else if (op == SDQH_GM_CORR) {
                if (qx != 0.0 && qy != 0.0) {
                    double t = c / (sqrt(qx) * sqrt(qy));
                    if (t > 1.0) t = 1.0;
                    if (t < -1.0) t = -1.0;
                    out = mo_bits(t);
                }
            } else if (qx != 0.0) {                                      // REGR_SLOPE, REGR_INTERCEPT
                const double slope = c / qx;
                if (op == SDQH_GM_REGR_SLOPE) out = mo_bits(slope);
                else {
                    const double muy = mo_value(mo.sk[mo.my[a]], st, idx, hits) + mo_f64(sums[(size_t)mo.my[a] * gstride + j]) / size;
                    const double mux = mo_value(mo.sk[mo.mx[a]], st, idx, hits) + mo_f64(sums[(size_t)mo.mx[a] * gstride + j]) / size;
                    out = mo_bits(muy - slope * mux);
                }
            }
            val[(size_t)a * gstride + j] = out;
        }
    }
}

// ---- second moments over window frames (sdqh_table_window_moments) ------------------------------------------------------------------
// VAR / STDDEV / COVAR / CORR / REGR over the frame [l, r] of every row (include/sdqh_sort_wmoments.h).  A frame per row rules the two
// passes of the section above out — O(n * width) — so the fold here is the one that section put off: merged states.  A state over a
// run of positions is (n, S, Q) per measure and C per measure pair; wmo_delta / wmo_weight / wmo_second are the header's merge, and
// every kernel below goes through them, so a node and a query associate and round alike wherever they are computed.  The states lie
// in component trees of the ranges' layout (tree[slot * tstride + node], leaves at cap + r): S of distinct measure k in slot 2k, its
// Q in slot 2k + 1, C of distinct pair c in slot 2 nmeas + c.  A node of level h covers 2^h positions — its n is never stored — and
// one that straddles n or a partition's end is never read by a query: what is folded into it is zeros or a neighbour's rows.
//   k_wmo_stage       the leaves: perm -> refs -> stage once per row, every distinct measure as a double into its S leaf, +0.0 into
//                     the Q and C leaves (pend / vkey / gkey are k_wrg_stage's, launched over an image of COUNT ranges)
//   k_wmo_tiles       a wave per tile, k_wrg_tiles' shape: three levels in a lane's registers, six by shuffles; a measure travels as
//                     (S, Q), a pair as (Sx, Sy, C) — its sums are added again, to the same bits as the measures' trees hold
//   k_wmo_upper       the levels above the tiles, a workgroup per measure; launched again, a workgroup per pair, once the S trees stand
//   k_wmo_fold        per row and column the frame's ends (wex_ends), the iterative query carrying the level, the finish
constexpr int WMO_MAX_MEAS = 2 * SDQH_WM_MAX_COLS, WMO_MAX_PAIRS = SDQH_WM_MAX_COLS;
struct DevWmoCol { int32_t op, my, mx, pair; };                       // the measures Y and X among the distinct ones; pair: its C tree (-1: none — one measure, or my == mx: my's Q)
struct DevWmos {
    DevWranges rg;                                                    // the frames, as an image of COUNT ranges (a[c].unit may be SDQH_WEX_ROWS: lo / hi clamped to [-n, n])
    DevSortKey sk[WMO_MAX_MEAS];                                      // the distinct measures (desc unused)
    int32_t pi[WMO_MAX_PAIRS], pj[WMO_MAX_PAIRS];                     // the distinct pairs, pi < pj
    DevWmoCol a[SDQH_WM_MAX_COLS];
    int32_t nmeas, npairs;
};
static_assert(SDQH_WM_MAX_COLS == SDQH_WRANGE_MAX_AGGS, "the columns of a moments call are the ranges of its image");

// merge(a, b), a's positions first: the difference of the means, the weight, and a second-order component (Q: dx = dy)
__device__ __forceinline__ double wmo_delta(double na, double sa, double nb, double sb) { return sb / nb - sa / na; }
__device__ __forceinline__ double wmo_weight(double na, double nb) { return (na * nb) / (na + nb); }
__device__ __forceinline__ double wmo_second(double a, double b, double dx, double dy, double w) { return (a + b) + (dx * dy) * w; }

// 1. a wave per tile: the leaves of every component tree
__global__ __launch_bounds__(TPB) void k_wmo_stage(DevStage st, DevWmos mo, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, uint32_t n, size_t tstride, uint64_t cap,
                                                  uint64_t* __restrict__ tree, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    for (uint64_t r = r0 + (uint32_t)lane_id(); r < r1; r += WAVE) {
        const uint32_t g = perm ? perm[r] : (uint32_t)r;
        const bool ok = g < n;                                           // (a permutation of [0, n): always)
        const int64_t idx = ok ? (int64_t)refs[g] : 0;
        const uint32_t hits = ok && st.shits ? st.shits[idx] : 0u;
        for (int k = 0; k < mo.nmeas; ++k) {
            tree[(size_t)(2 * k) * tstride + cap + r] = mo_bits(ok ? mo_value(mo.sk[k], st, idx, hits) : 0.0);
            tree[(size_t)(2 * k + 1) * tstride + cap + r] = mo_bits(0.0);
        }
        for (int c = 0; c < mo.npairs; ++c) tree[(size_t)(2 * mo.nmeas + c) * tstride + cap + r] = mo_bits(0.0);
    }
}
// 2. the lowest nine levels, a wave per tile (k_wrg_tiles' walk: lane i takes the leaves [8i, 8i + 8), past n a zero; the lane whose
// number is a multiple of 2^k holds the node over lanes [lane, lane + 2^k)).  unit u < nmeas: measure u's S and Q; above: a pair's C.
__global__ __launch_bounds__(TPB) void k_wmo_tiles(DevWmos mo, uint32_t n, size_t tstride, uint64_t cap, uint64_t* __restrict__ tree, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t p0 = r0 + 8ull * lane;                                // this lane's first leaf
    for (int u = 0; u < mo.nmeas + mo.npairs; ++u) {
        const bool pair = u >= mo.nmeas;
        const int ki = pair ? mo.pi[u - mo.nmeas] : u, kj = pair ? mo.pj[u - mo.nmeas] : u;
        const uint64_t* __restrict__ li = tree + (size_t)(2 * ki) * tstride + cap;      // the leaves of S_i, S_j
        const uint64_t* __restrict__ lj = tree + (size_t)(2 * kj) * tstride + cap;
        uint64_t* __restrict__ ts = tree + (size_t)(2 * ki) * tstride;                  // where S (a measure alone) and the second-order component go
        uint64_t* __restrict__ t2 = tree + (size_t)(pair ? 2 * mo.nmeas + (u - mo.nmeas) : 2 * ki + 1) * tstride;
        double si[8], sj[8], q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const bool in = p0 + i < r1; si[i] = in ? mo_f64(li[p0 + i]) : 0.0; sj[i] = in ? mo_f64(lj[p0 + i]) : 0.0; q[i] = 0.0; }
#pragma unroll
        for (int h = 1; h <= 3; ++h) {
            const double nh = (double)(1u << (h - 1));                   // a child's rows
            const double wt = wmo_weight(nh, nh);
#pragma unroll
            for (int i = 0; i < (8 >> h); ++i) {
                const double di = wmo_delta(nh, si[2 * i], nh, si[2 * i + 1]), dj = wmo_delta(nh, sj[2 * i], nh, sj[2 * i + 1]);
                const double nq = wmo_second(q[2 * i], q[2 * i + 1], di, dj, wt);
                const double ni = si[2 * i] + si[2 * i + 1], nj = sj[2 * i] + sj[2 * i + 1];
                si[i] = ni; sj[i] = nj; q[i] = nq;
                const uint64_t at = (cap >> h) + (p0 >> h) + (uint64_t)i;
                if (!pair) ts[at] = mo_bits(ni);
                t2[at] = mo_bits(nq);
            }
        }
        double xi = si[0], xj = sj[0], xq = q[0];
#pragma unroll
        for (int k = 1; k <= WRG_TILE_LEVELS - 3; ++k) {
            const double oi = __shfl_down(xi, 1u << (k - 1), WAVE), oj = __shfl_down(xj, 1u << (k - 1), WAVE), oq = __shfl_down(xq, 1u << (k - 1), WAVE);
            if ((lane & ((1u << k) - 1u)) == 0u) {
                const double nh = (double)(1u << (2 + k));
                const double wt = wmo_weight(nh, nh);
                const double di = wmo_delta(nh, xi, nh, oi), dj = wmo_delta(nh, xj, nh, oj);
                xq = wmo_second(xq, oq, di, dj, wt);
                xi = xi + oi; xj = xj + oj;
                const uint64_t at = (cap >> (3 + k)) + (p0 >> (3 + k));
                if (!pair) ts[at] = mo_bits(xi);
                t2[at] = mo_bits(xq);
            }
        }
    }
}
// 3. the levels above the tiles, one at a time (k_wrg_upper's walk and barrier).  pairs == 0: workgroup b takes measure b's S and Q;
// pairs == 1, launched behind it: workgroup b takes pair b's C and reads the S trees that launch left.  A child whose first tile
// does not exist was never written: zeros.
__global__ __launch_bounds__(TPB) void k_wmo_upper(DevWmos mo, int pairs, size_t tstride, uint64_t cap, uint64_t* __restrict__ tree, uint32_t ntiles) {
    const int b = (int)blockIdx.x;
    if (b >= (pairs ? mo.npairs : mo.nmeas)) return;
    const int ki = pairs ? mo.pi[b] : b, kj = pairs ? mo.pj[b] : b;
    uint64_t* si = tree + (size_t)(2 * ki) * tstride;
    const uint64_t* sj = tree + (size_t)(2 * kj) * tstride;
    uint64_t* t2 = tree + (size_t)(pairs ? 2 * mo.nmeas + b : 2 * ki + 1) * tstride;
    for (int h = WRG_TILE_LEVELS + 1; (cap >> h) >= 1ull; ++h) {
        const uint64_t cnt = cap >> h;                                   // nodes of this level: [cnt, 2 cnt)
        const int up = h - WRG_TILE_LEVELS;                              // a node of it covers 2^up tiles
        const uint64_t live = min(cnt, (((uint64_t)ntiles - 1ull) >> up) + 1ull);      // those whose first tile exists
        const double nh = (double)(1ull << (h - 1));
        const double wt = wmo_weight(nh, nh);
        for (uint64_t i = threadIdx.x; i < live; i += TPB) {
            const uint64_t l = 2ull * (cnt + i), r = l + 1ull;
            const bool has = ((2ull * i + 1ull) << (up - 1)) < (uint64_t)ntiles;
            const double ai = mo_f64(si[l]), aj = mo_f64(sj[l]), aq = mo_f64(t2[l]);
            const double bi = has ? mo_f64(si[r]) : 0.0, bj = has ? mo_f64(sj[r]) : 0.0, bq = has ? mo_f64(t2[r]) : 0.0;
            const double di = wmo_delta(nh, ai, nh, bi), dj = wmo_delta(nh, aj, nh, bj);
            t2[cnt + i] = mo_bits(wmo_second(aq, bq, di, dj, wt));
            if (!pairs) si[cnt + i] = mo_bits(ai + bi);
        }
        __syncthreads();
    }
}
// a frame's state under the query: the rows it holds so far (0: the empty state) and the components a column reads
struct WmoState { uint64_t n; double sy, qy, sx, qx, c; };
// the node at index p of level h; two: the column reads a second measure
__device__ __forceinline__ WmoState wmo_node(const uint64_t* __restrict__ ty, const uint64_t* __restrict__ tx, const uint64_t* __restrict__ tc, size_t tstride, uint64_t p, int h, bool two) {
    WmoState v;
    v.n = 1ull << h;
    v.sy = mo_f64(ty[p]); v.qy = mo_f64(ty[tstride + p]);
    v.sx = two ? mo_f64(tx[p]) : v.sy; v.qx = two ? mo_f64(tx[tstride + p]) : v.qy; v.c = two ? mo_f64(tc[p]) : v.qy;
    return v;
}
__device__ __forceinline__ WmoState wmo_merge(const WmoState& a, const WmoState& b, bool two) {
    if (a.n == 0ull) return b;
    if (b.n == 0ull) return a;
    const double na = (double)a.n, nb = (double)b.n;
    const double wt = wmo_weight(na, nb);
    const double dy = wmo_delta(na, a.sy, nb, b.sy);
    WmoState v;
    v.n = a.n + b.n;
    v.sy = a.sy + b.sy; v.qy = wmo_second(a.qy, b.qy, dy, dy, wt);
    if (two) {
        const double dx = wmo_delta(na, a.sx, nb, b.sx);
        v.sx = a.sx + b.sx; v.qx = wmo_second(a.qx, b.qx, dx, dx, wt); v.c = wmo_second(a.c, b.c, dx, dy, wt);
    } else { v.sx = v.sy; v.qx = v.qy; v.c = v.qy; }
    return v;
}
// 4. the value of every column at the first m positions: fin[c * stride + j].  rown: k_wsl_rows' (s = j - rown[j]); pend, vkey, gkey:
// k_wrg_stage's.  (wmo_weight's n_a + n_b is exact in a double either way: n < 2^32.)
__global__ __launch_bounds__(TPB) void k_wmo_fold(DevWmos mo, const uint32_t* __restrict__ rown, const uint32_t* __restrict__ pend, const uint64_t* __restrict__ vkey,
                                                 const uint64_t* __restrict__ gkey, uint32_t n, uint32_t m, size_t stride, size_t tstride, uint64_t cap,
                                                 const uint64_t* __restrict__ tree, uint64_t* __restrict__ fin) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t rn = rown[j], e = pend[j];
        if ((uint64_t)rn > j || (uint64_t)e < j || e >= n) continue;       // (s <= j <= e < n: never taken)
        const uint32_t s = (uint32_t)j - rn;
        for (int c = 0; c < mo.rg.n; ++c) {
            const DevWmoCol& a = mo.a[c];
            uint32_t l = 0u, r1 = 0u;
            uint64_t out = WAGG_QNAN;
            if (wex_ends(mo.rg.a[c], mo.rg, vkey, gkey, j, s, e, l, r1)) {
                const int op = a.op;
                const bool two = op >= SDQH_GM_COVAR_POP;
                const uint64_t* __restrict__ ty = tree + (size_t)(2 * a.my) * tstride;
                const uint64_t* __restrict__ tx = tree + (size_t)(2 * a.mx) * tstride;
                const uint64_t* __restrict__ tc = a.pair >= 0 ? tree + (size_t)(2 * mo.nmeas + a.pair) * tstride : ty + tstride;
                WmoState left, right;
                left.n = 0ull; left.sy = left.qy = left.sx = left.qx = left.c = 0.0;
                right = left;
                int h = 0;
                for (uint64_t p = cap + l, q = cap + r1; p < q; p >>= 1, q >>= 1, ++h) {
                    if (p & 1ull) left = wmo_merge(left, wmo_node(ty, tx, tc, tstride, p++, h, two), two);
                    if (q & 1ull) right = wmo_merge(wmo_node(ty, tx, tc, tstride, --q, h, two), right, two);
                }
                const WmoState f = wmo_merge(left, right, two);
                const uint32_t rows = r1 - l;
                const double size = (double)rows;
                // a pair stored as (pi < pj) holds C whichever of the two is Y: dx * dy commutes
                if (op == SDQH_GM_VAR_POP) out = mo_bits(f.qy / size);
                else if (op == SDQH_GM_STDDEV_POP) out = mo_bits(sqrt(f.qy / size));
                else if (op == SDQH_GM_COVAR_POP) out = mo_bits(f.c / size);
                else if (op == SDQH_GM_VAR_SAMP) { if (rows > 1u) out = mo_bits(f.qy / (size - 1.0)); }
                else if (op == SDQH_GM_STDDEV_SAMP) { if (rows > 1u) out = mo_bits(sqrt(f.qy / (size - 1.0))); }
                else if (op == SDQH_GM_COVAR_SAMP) { if (rows > 1u) out = mo_bits(f.c / (size - 1.0)); }
                else if (op == SDQH_GM_CORR) {
                    if (f.qx != 0.0 && f.qy != 0.0) {
                        double t = f.c / (sqrt(f.qx) * sqrt(f.qy));
                        if (t > 1.0) t = 1.0;
                        if (t < -1.0) t = -1.0;
                        out = mo_bits(t);
                    }
                } else if (f.qx != 0.0) {                                // REGR_SLOPE, REGR_INTERCEPT
                    const double slope = f.c / f.qx;
                    out = mo_bits(op == SDQH_GM_REGR_SLOPE ? slope : f.sy / size - slope * (f.sx / size));
                }
            }
            fin[(size_t)c * stride + j] = out;
        }
    }
}

// ---- sessions inside partitions (sdqh_table_sessions) -----------------------------------------------------------------------------
// Every pass above cuts where the KEYS decide; a session is cut where the data along the order decide (include/sdqh_sort_sessions.h):
// sorted position r opens one iff it opens its partition or the rule says so about the raw values at r - 1 and r.  k_ss_heads makes
// that comparison once and leaves the cuts in the three encodings the passes above read, so that they run over sessions unchanged:
//   headsA            WIN_PART on partition heads, WIN_TIE on session heads: a dense rank over it (k_win_scan / k_win_rank) numbers the
//                     sessions of a partition — SDQH_SS_NUMBER
//   headsB            WIN_PART | WIN_TIE on every session head: a row number over it is SDQH_SS_ROW, and the frames' passes
//                     (k_wagg_tiles / _scan / _run / _next) fold SUM / COUNT / MIN / MAX over sessions as they fold over partitions
//   depth             0 partition head, 1 session head, 2 neither: level 2 of the grouping sets' passes is "sessions" — k_sort_bins
//                     counts them, k_gs_run keeps the value at a session's last row in the session's slot
// Per row, k_ss_rows walks a tile backwards (k_wagg_ends' shape): the session's last position is read off the ballots and the tiles
// behind, its first off the row number; a fold's value is the running value at the last position, an AVG divides it by the length,
// FIRST / LAST gather the measure there.  Per session, k_ss_sessions does the same from the sessions' positions.  No atomics.
struct DevSsRule { DevSortTerm tm; int64_t gap; int32_t rule, _pad; };      // tm: the gap term, or the marker as a term with no derivation
struct DevSsCols { DevSortKey sk[SDQH_SS_MAX_COLS]; int32_t op[SDQH_SS_MAX_COLS], slot[SDQH_SS_MAX_COLS]; int32_t n, _pad; };      // slot: the column's fold among the call's folds (-1: none)
static_assert(SDQH_SS_MAX_COLS == SDQH_WAGG_MAX_AGGS, "the sessions' folds are the frames'");

// the rule's value at gathered entry g: the stored 64 bits, a derived term's `field` (k_sort_keys' derivation, before sort_bits)
__device__ __forceinline__ int64_t ss_value(const DevSortTerm& tm, const DevStage& st, const uint32_t* __restrict__ refs, uint32_t g) {
    const int64_t idx = (int64_t)refs[g];
    const uint32_t hits = st.shits ? st.shits[idx] : 0u;
    const int64_t raw = sort_raw(tm.sk, st, idx, hits);
    if (!term_derived(tm)) return raw;
    uint64_t f = (uint64_t)raw;
    if (tm.div > 1) f /= tm.div;
    if (tm.mod) f %= tm.mod;
    return (int64_t)(f + (uint64_t)tm.add);
}
// does the row with value `cur` continue the session of its predecessor in the order, `prev`?  An integer gap by the unsigned
// difference of the two order-adjacent values (prev <= cur ascending, >= descending: exact, nothing wraps), a double gap by one
// IEEE addition and two comparisons
__device__ __forceinline__ bool ss_continues(const DevSsRule& ru, int64_t prev, int64_t cur) {
    if (ru.rule == SDQH_SS_CHANGE) return prev == cur;
    if (!ru.tm.sk.is_f64) {
        const uint64_t d = ru.tm.sk.desc ? (uint64_t)prev - (uint64_t)cur : (uint64_t)cur - (uint64_t)prev;
        return d <= (uint64_t)ru.gap;
    }
    const double vp = __longlong_as_double(prev), vc = __longlong_as_double(cur), gap = __longlong_as_double(ru.gap);
    if (vc != vc) return prev == cur;
    if (vp != vp) return false;
    const double a = vc + (ru.tm.sk.desc ? gap : -gap);
    return (a < vc ? a : vc) <= vp && vp <= (a < vc ? vc : a);
}

// 1. a wave per tile of sorted positions: the two flag bytes and the depth of every position, per tile the carries of both flag
// arrays (k_win_scan's), the first session head (what k_wagg_scan and k_wagg_next read) and the heads of levels 0 .. 2
// (tcount[L * ntiles + tile], k_sort_bins').  keys: the staged keys of the npart partition terms.
__global__ __launch_bounds__(TPB) void k_ss_heads(DevStage st, DevSsRule ru, const uint64_t* __restrict__ keys, size_t key_stride, int npart, const uint32_t* __restrict__ refs,
                                                 const uint32_t* __restrict__ perm, uint32_t n, uint8_t* __restrict__ headsA, uint8_t* __restrict__ headsB, uint8_t* __restrict__ depth,
                                                 WinCarry* __restrict__ carryA, WinCarry* __restrict__ carryB, WaggHeads* __restrict__ tfirst, uint32_t* __restrict__ tcount, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    WinCarry runA = {0u, 0u, 0u, 0u}, runB = {0u, 0u, 0u, 0u};
    WaggHeads fh = {n, n};
    uint32_t cp = 0u, cs = 0u;
    for (uint64_t b = r0; b < r1; b += WAVE) {
        const uint64_t r = b + lane_id();
        const bool live = r < r1;
        bool ph = false, sh = false;
        if (live) {
            if (r == 0) ph = sh = true;
            else {
                const uint32_t g = perm ? perm[r] : (uint32_t)r, h = perm ? perm[r - 1] : (uint32_t)(r - 1);
                if (g < n && h < n) {                                    // (a permutation of [0, n): always)
                    for (int c = 0; c < npart; ++c) ph |= keys[(size_t)c * key_stride + g] != keys[(size_t)c * key_stride + h];
                    sh = ph || !ss_continues(ru, ss_value(ru.tm, st, refs, h), ss_value(ru.tm, st, refs, g));
                }
            }
            headsA[r] = (uint8_t)((ph ? WIN_PART : 0u) | (sh ? WIN_TIE : 0u));
            headsB[r] = (uint8_t)(sh ? (WIN_PART | WIN_TIE) : 0u);
            depth[r] = (uint8_t)(ph ? 0u : (sh ? 1u : 2u));
        }
        const uint64_t mp = __ballot(ph), ms = __ballot(sh);
        const uint32_t cnt = (uint32_t)min((uint64_t)WAVE, r1 - b);
        win_step(runA, mp, ms, cnt);
        win_step(runB, ms, ms, cnt);
        if (ms && fh.part == n) fh.part = fh.tie = (uint32_t)b + (uint32_t)__builtin_ctzll(ms);
        cp += (uint32_t)__popcll(mp); cs += (uint32_t)__popcll(ms);
    }
    if (lane_id() == 0) {
        carryA[w] = runA; carryB[w] = runB; tfirst[w] = fh;
        tcount[w] = w == 0 ? 1u : 0u; tcount[(size_t)ntiles + w] = cp; tcount[(size_t)2 * ntiles + w] = cs;
    }
}
// an AVG: the session's sum (an integer one converted once) by its number of rows, one IEEE division — k_gs_avg's
__device__ __forceinline__ uint64_t ss_avg(uint64_t s, int is_f64, uint32_t rows) {
    const double sum = is_f64 ? __longlong_as_double((long long)s) : (double)(int64_t)s;
    return (uint64_t)__double_as_longlong(sum / (double)rows);
}
// 2a. per row: the columns of the first m positions.  A tile walked backwards; `se` is the last position of lane's session — the
// position before the next session head above the lane, in the batches behind or in the tiles behind (tnext) —, its first the row's
// own position minus its row number (rowb, from 1; nullptr: no column reads it).  rows: k_wagg_run's running values over headsB,
// numb: the dense ranks over headsA.  ntiles: the tiles that hold a position below m.
__global__ __launch_bounds__(TPB) void k_ss_rows(DevStage st, DevSsCols sc, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint8_t* __restrict__ headsB,
                                                const WaggHeads* __restrict__ tnext, const uint32_t* __restrict__ numb, const uint32_t* __restrict__ rowb, uint32_t n, uint32_t m,
                                                size_t stride, const uint64_t* __restrict__ rows, uint64_t* __restrict__ fin, uint32_t ntiles) {
    uint32_t w; uint64_t r0, r1;
    if (!tile_range(ntiles, n, w, r0, r1)) return;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t le = lanemask_lt() | (1ull << lane);
    uint32_t next = tnext[w].part;
    for (uint64_t b = r0 + ((r1 - r0 - 1) / WAVE) * WAVE; ; b -= WAVE) {
        const uint64_t r = b + lane;
        const bool live = r < r1;
        const WaggBatch h = wagg_batch(headsB, r, live, le);
        const uint64_t pg = h.mp & ~le;
        const uint32_t se = (pg ? (uint32_t)b + (uint32_t)__builtin_ctzll(pg) : next) - 1u;
        if (live && r < m && se < n && se >= r) {                        // (r <= se < n: always)
            const uint32_t rn = rowb ? rowb[r] : 1u;
            const uint32_t s0 = (uint32_t)r - (rn - 1u);                 // (a row number is at most r + 1)
#pragma unroll
            for (int c = 0; c < SDQH_SS_MAX_COLS; ++c) if (c < sc.n) {
                const int op = sc.op[c];
                uint64_t v;
                if (op == SDQH_SS_NUMBER) v = (uint64_t)numb[r];
                else if (op == SDQH_SS_ROW) v = (uint64_t)rn;
                else if (op == SDQH_WSLIDE_FIRST) v = gd_measure(sc.sk[c], st, refs, perm, s0, n);
                else if (op == SDQH_WSLIDE_LAST) v = gd_measure(sc.sk[c], st, refs, perm, se, n);
                else {
                    v = sc.slot[c] >= 0 ? rows[(size_t)sc.slot[c] * stride + se] : 0ull;      // (every other op folds: always)
                    if (op == SDQH_WEX_AVG) v = ss_avg(v, sc.sk[c].is_f64, se - s0 + 1u);
                }
                fin[(size_t)c * stride + r] = v;
            }
        }
        if (h.mp) next = (uint32_t)b + (uint32_t)__builtin_ctzll(h.mp);
        if (b == r0) break;
    }
}
// 2b. per session: a thread per returned session j.  pos: the sessions' sorted positions (k_gs_run's, all ng of them), sums: the
// folds' values in the sessions' slots (gstride apart); the session's rows are [pos[j], pos[j + 1]) or up to n
__global__ __launch_bounds__(TPB) void k_ss_sessions(DevStage st, DevSsCols sc, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ pos,
                                                    const uint32_t* __restrict__ numb, uint32_t n, uint32_t ng, uint32_t m, size_t gstride, const uint64_t* __restrict__ sums,
                                                    uint64_t* __restrict__ val) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t p = pos[j];
        const uint32_t next = j + 1 < ng ? pos[j + 1] : n;
        if (p >= n || next <= p || next > n) continue;                   // (positions in order, below n: never taken)
#pragma unroll
        for (int c = 0; c < SDQH_SS_MAX_COLS; ++c) if (c < sc.n) {
            const int op = sc.op[c];
            uint64_t v;
            if (op == SDQH_SS_NUMBER) v = (uint64_t)numb[p];
            else if (op == SDQH_WSLIDE_FIRST) v = gd_measure(sc.sk[c], st, refs, perm, p, n);
            else if (op == SDQH_WSLIDE_LAST) v = gd_measure(sc.sk[c], st, refs, perm, next - 1u, n);
            else {
                v = sc.slot[c] >= 0 ? sums[(size_t)sc.slot[c] * gstride + j] : 0ull;          // (every other op folds: always)
                if (op == SDQH_WEX_AVG) v = ss_avg(v, sc.sk[c].is_f64, next - p);
            }
            val[(size_t)c * gstride + j] = v;
        }
    }
}

// The emit of every entry point: row j of the result = the entry at sorted position sel[j] (sel == nullptr: every position is
// kept, j itself), which is gathered entry perm[position] (perm == nullptr: the gathered order itself).  o's arrays and out_rank
// hold m rows each; a null array is not written, and rank is read only for out_rank.
__global__ __launch_bounds__(TPB) void k_sort_emit(DevStage st, const uint32_t* __restrict__ refs, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ sel,
                                                  const uint32_t* __restrict__ rank, uint32_t n, uint32_t m, DevSortOut o, int64_t* __restrict__ out_rank) {
    for (uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x; j < m; j += (uint64_t)gridDim.x * TPB) {
        const uint32_t i = sel ? sel[j] : (uint32_t)j;
        if (i >= n) continue;                                            // (kept positions are positions: never taken)
        const uint32_t g = perm ? perm[i] : i;
        if (g >= n) continue;                                            // (a permutation of [0, n): never taken)
        const int64_t idx = (int64_t)refs[g];
        if (o.keys) o.keys[j] = st.key[idx];
#pragma unroll
        for (int p = 0; p < SDQH_MAX_PAYLOAD; ++p) if (p < o.npay && o.pay[p]) o.pay[p][j] = st.pay[p][idx];
#pragma unroll
        for (int v = 0; v < SDQH_TUPLE_MAX_VALUES; ++v) if (v < o.nval && o.val[v]) o.val[v][j] = st.sacc[(size_t)idx * st.acc_stride + v];
        if (o.hits) o.hits[j] = st.shits ? (int64_t)st.shits[idx] : 0;
        if (out_rank) out_rank[j] = (int64_t)rank[i];
    }
}

struct Scratch {                                     // pool blocks of one call, returned on every way out
    sdqh_ctx* ctx; void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    explicit Scratch(sdqh_ctx* c) : ctx(c) {}
    ~Scratch() { for (void* q : p) if (q) pool_free(ctx, q); }
};
inline size_t round_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// A scratch block carved into typed arrays, each starting on a 256-byte boundary.  A block's layout is ONE sequence of take() calls
// (a lambda), run twice: over Carver(nullptr) it sums the sizes — bytes() is what to allocate — and over Carver(block) it hands out the
// arrays, so no array can be left out of the sum.  The sums are byte for byte those the hand-written offsets gave (the slack a
// block carried is taken as an array of its own): the pool hands a freed block to the next request of its size.
struct Carver {
    uintptr_t base; size_t at = 0;
    explicit Carver(void* block) : base(reinterpret_cast<uintptr_t>(block)) {}
    template <class T> T* take(size_t count) { T* p = reinterpret_cast<T*>(base + at); at += round_up(count * sizeof(T)); return p; }
    size_t bytes() const { return at; }
};
// the block of `layout` from the pool into `slot` and carved; false: out of device memory
template <class Layout> bool carve(sdqh_ctx* ctx, void*& slot, Layout layout) {
    Carver sum(nullptr);
    layout(sum);
    if (!(slot = pool_alloc(ctx, sum.bytes()))) return false;
    Carver c(slot);
    layout(c);
    return true;
}

// A wave owns a tile of SORT_TILE consecutive positions: the tiles of `count` positions and the grid that gives each a wave.
struct Tiles {
    uint32_t ntiles = 0; unsigned tgrid = 0;
    Tiles() = default;
    explicit Tiles(int64_t count) : ntiles((uint32_t)((count + SORT_TILE - 1) / SORT_TILE)), tgrid((ntiles + TPB / WAVE - 1) / (TPB / WAVE)) {}
};

}  // namespace

extern "C" {

int sdqh_sort_geometry(sdqh_ctx* ctx, int64_t* single_wg_max, int64_t* tile_rows, int64_t* second_level_rows) {
    if (!ctx || !single_wg_max || !tile_rows || !second_level_rows) return fail(ctx, SDQH_ERR_INVALID, "sort_geometry: bad arguments");
    *single_wg_max = SORT_SMALL; *tile_rows = SORT_TILE; *second_level_rows = 0;
    return SDQH_OK;
}

// one pass of the radix path over `key` at `shift`: perm (nullptr: the identity) -> out
static void radix_pass(sdqh_ctx* ctx, const uint64_t* key, const uint32_t* perm, uint32_t n, int shift, uint32_t* hist, uint32_t* bin_total, const Tiles& t, uint32_t* out) {
    LAUNCH(ctx, "k_sort_hist", k_sort_hist, t.tgrid, key, perm, n, shift, hist, t.ntiles);
    LAUNCH(ctx, "k_sort_bins", k_sort_bins, 256, hist, t.ntiles, bin_total);
    LAUNCH(ctx, "k_sort_scatter", k_sort_scatter, t.tgrid, key, perm, n, shift, hist, bin_total, t.ntiles, out);
}

// What the first half of an ORDER BY leaves on the device — the references of the selected entries in stage order, the keys of every
// term beside them, the permutation that orders them (nullptr: stage order is the order) — and what the host knows of it.
struct SortState {
    unsigned long long h[SORT_INFO];                 // the info block: n, the AND / OR masks
    unsigned long long* info = nullptr;
    uint32_t* refs = nullptr;
    uint64_t* keys = nullptr;
    size_t key_stride = 0;
    const uint32_t* perm = nullptr;
    int64_t n = 0;
};

// first half, (a): selection, keys, the info block read (one wait).  Opens the call (call_begin); blocks go to scratch.p[0].
static int sort_select(sdqh_ctx* ctx, sdqh_table* table, const std::string& me, int64_t min_hits, int nsort, const DevSortTerm* terms, Scratch& scratch, SortState& s) {
    call_begin(ctx);
    if (int rc = index_ensure(ctx, table)) return rc;
    // block 0: [segment offsets | info | references | keys per column], sized for every staged row (the count is the device's)
    const size_t rows = (size_t)std::max<int64_t>(table->nrows_build, 1) + 1;
    const int nseg = table->stage.nseg;
    const size_t key_stride = s.key_stride = round_up(rows * 8) / 8;
    uint32_t* seg_off = nullptr;
    if (!carve(ctx, scratch.p[0], [&](Carver& c) {
            seg_off = c.take<uint32_t>((size_t)std::max(nseg, 1));
            s.info = c.take<unsigned long long>(SORT_INFO);
            s.refs = c.take<uint32_t>(rows);
            s.keys = c.take<uint64_t>(key_stride * (size_t)nsort);
        })) return fail(ctx, SDQH_ERR_NOMEM, me + ": out of device memory");
    const uint32_t mh = (uint32_t)std::min<int64_t>(std::max<int64_t>(min_hits, 0), 0xFFFFFFFFll);
    const unsigned seg_grid = (unsigned)std::max(1, (nseg + TPB / WAVE - 1) / (TPB / WAVE));
    LAUNCH(ctx, "k_sort_count", k_sort_count, seg_grid, table->dev, table->stage, mh, seg_off);
    LAUNCH(ctx, "k_sort_scan", k_sort_scan, 1, seg_off, nseg, s.info);
    LAUNCH(ctx, "k_sort_gather", k_sort_gather, seg_grid, table->dev, table->stage, mh, seg_off, s.refs);
    const unsigned key_grid = (unsigned)std::max<size_t>(1, std::min<size_t>((rows + TPB - 1) / TPB, (size_t)ctx->num_cu * 8));
    for (int c = 0; c < nsort; ++c) LAUNCH(ctx, "k_sort_keys", k_sort_keys, key_grid, table->stage, terms[c], s.refs, s.keys + (size_t)c * key_stride, s.info, c);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->result_host, s.info, SORT_INFO * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    std::memcpy(s.h, ctx->result_host, sizeof(s.h));
    if (s.h[SORT_INFO_BAD]) {                                         // before anything is written, *out_n included
        int c = 0;
        while (c < nsort - 1 && !((s.h[SORT_INFO_BAD] >> c) & 1ull)) ++c;
        call_end(ctx);
        return fail(ctx, SDQH_ERR_INVALID, me + ": term " + std::to_string(c) + " derives a field outside its ranks column (" + std::to_string((long long)terms[c].nranks) + " rows)");
    }
    s.n = (int64_t)s.h[0];
    return SDQH_OK;
}

// first half, (b): the passes (n >= 1) — last column first, low digit first; a digit whose bits are the same in every key orders
// nothing.  Leaves s.perm; block 1 = [permutation x 2 | digit counts per tile | digit totals] goes to scratch.p[1].
static int sort_passes(sdqh_ctx* ctx, const std::string& me, int nsort, Scratch& scratch, SortState& s) {
    const int64_t n = s.n;
    int pass_col[8 * SDQH_SORT_MAX_KEYS], pass_shift[8 * SDQH_SORT_MAX_KEYS], npass = 0;
    if (n > 1) for (int c = nsort - 1; c >= 0; --c) {
        const uint64_t vary = s.h[1 + SDQH_SORT_MAX_KEYS + c] & ~s.h[1 + c];
        for (int shift = 0; shift < 64; shift += 8) if ((vary >> shift) & 255ull) { pass_col[npass] = c; pass_shift[npass] = shift; ++npass; }
    }
    const uint32_t un = (uint32_t)n;
    const Tiles t(n);
    const bool small = n <= SORT_SMALL;
    s.perm = nullptr;
    if (npass) {
        uint32_t *pa = nullptr, *pb = nullptr, *hist = nullptr, *bin_total = nullptr;       // (the single-workgroup kernel uses pa alone)
        if (!carve(ctx, scratch.p[1], [&](Carver& c) {
                pa = c.take<uint32_t>((size_t)n);
                pb = c.take<uint32_t>(small ? 0 : (size_t)n);
                hist = c.take<uint32_t>(small ? 0 : (size_t)t.ntiles * 256);
                bin_total = c.take<uint32_t>(256);
            })) return fail(ctx, SDQH_ERR_NOMEM, me + ": out of device memory");
        if (small) {
            LAUNCH(ctx, "k_sort_small", k_sort_small, 1, s.keys, s.key_stride, nsort, un, s.info, pa);
            s.perm = pa;
        } else {
            for (int p = 0; p < npass; ++p) {
                radix_pass(ctx, s.keys + (size_t)pass_col[p] * s.key_stride, s.perm, un, pass_shift[p], hist, bin_total, t, pa);
                s.perm = pa; std::swap(pa, pb);
            }
        }
    }
    return SDQH_OK;
}

// second half: the arrays of a result of m rows on the device (block 2: scratch.p[2]; each array m x 8 bytes, in the order keys,
// payload columns, value columns, hits, extra) ...
struct SortRows { char* dev = nullptr; DevSortOut o; int64_t* extra = nullptr; int npay = 0, nval = 0, narr = 0; size_t nb = 0, need = 0; };
static int sort_rows_alloc(sdqh_ctx* ctx, sdqh_table* table, const std::string& me, int64_t m, bool keys, bool payload, bool values, bool hits, bool extra, Scratch& scratch, SortRows& r) {
    const int nv = table->accumulate ? table->nv : 0;
    r.npay = payload ? table->npay : 0; r.nval = values ? nv : 0;
    r.narr = (keys ? 1 : 0) + r.npay + r.nval + (hits ? 1 : 0) + (extra ? 1 : 0);
    r.nb = (size_t)m * 8; r.need = r.nb * (size_t)r.narr;
    std::memset(&r.o, 0, sizeof(r.o));
    if (!r.narr) return SDQH_OK;
    char* dev = r.dev = static_cast<char*>(scratch.p[2] = pool_alloc(ctx, r.need + 64));
    if (!dev) return fail(ctx, SDQH_ERR_NOMEM, me + ": out of device memory");
    size_t at = 0;
    if (keys) { r.o.keys = reinterpret_cast<int64_t*>(dev + at); at += r.nb; }
    for (int p = 0; p < r.npay; ++p) { r.o.pay[p] = reinterpret_cast<int64_t*>(dev + at); at += r.nb; }
    for (int v = 0; v < r.nval; ++v) { r.o.val[v] = reinterpret_cast<double*>(dev + at); at += r.nb; }
    if (hits) { r.o.hits = reinterpret_cast<int64_t*>(dev + at); at += r.nb; }
    if (extra) { r.extra = reinterpret_cast<int64_t*>(dev + at); at += r.nb; }
    r.o.npay = r.npay; r.o.nval = r.nval;
    return SDQH_OK;
}
// ... and their way to the caller's arrays (after call_end; waits for the stream)
static int sort_rows_fetch(sdqh_ctx* ctx, const SortRows& r, int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_extra) {
    const size_t nb = r.nb, need = r.need;
    // the rows land in pinned memory in one copy (a copy into pageable memory is several times slower), then one memcpy per array
    if (need > ctx->bulk_bytes && need <= ((size_t)1 << 30)) {
        if (ctx->bulk_host) (void)hipHostFree(ctx->bulk_host);
        ctx->bulk_host = nullptr; ctx->bulk_bytes = 0;
        const size_t want = std::max<size_t>(need * 2, (size_t)8 << 20);
        if (hipHostMalloc(&ctx->bulk_host, want, hipHostMallocDefault) == hipSuccess) ctx->bulk_bytes = want; else (void)hipGetLastError();
    }
    const bool pinned = need <= ctx->bulk_bytes;
    int64_t* dst[3 + SDQH_MAX_PAYLOAD + SDQH_TUPLE_MAX_VALUES]; int nd = 0;
    if (out_keys) dst[nd++] = out_keys;
    for (int p = 0; p < r.npay; ++p) dst[nd++] = out_payload + (size_t)p * (size_t)capacity;
    for (int v = 0; v < r.nval; ++v) dst[nd++] = reinterpret_cast<int64_t*>(out_values + (size_t)v * (size_t)capacity);
    if (out_hits) dst[nd++] = out_hits;
    if (out_extra) dst[nd++] = out_extra;
    if (pinned) HIP_TRY(ctx, hipMemcpyAsync(ctx->bulk_host, r.dev, need, hipMemcpyDeviceToHost, ctx->stream));
    else for (int a = 0; a < nd; ++a) HIP_TRY(ctx, hipMemcpyAsync(dst[a], r.dev + (size_t)a * nb, nb, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    if (pinned) for (int a = 0; a < nd; ++a) std::memcpy(dst[a], static_cast<const char*>(ctx->bulk_host) + (size_t)a * nb, nb);
    return SDQH_OK;
}

// ---- the step behind the sort ------------------------------------------------------------------------------------------------------
// What an entry point asks for between the passes and the emit.  kind: nothing (the two plain sorts), ranks inside partitions or, in
// their place, columns over the same partitions (frames, slides, ranges, quantiles).  The first npart terms are PARTITION BY.  The
// filter: only the rows whose rank of `rank_kind` is <= per_limit are returned (filters false: the entry point has no such argument).
// out: the rank column, or out[a * capacity + j] = column a beside returned row j — nullptr: rows only, no column is computed.  Then
// the family's device arguments (a slide's lo / hi: the caller's).
// STEP_GROUPS (sdqh_table_grouping_sets) returns one row per group: `levels` of the nsort terms, their counts to level_rows; its
// aggregates are `aggs` (an AVG as the SUM it divides: avg), and like a filter it knows its count only behind the sort.
// STEP_DISTINCTS (sdqh_table_group_distinct) returns one row per group of the first `ngroup` terms; `aggs` are the folds of the upper
// stage, `gd` the ops and measures as the caller named them.
// STEP_MOMENTS (sdqh_table_group_moments) returns the rows of STEP_GROUPS — `levels`, level_rows —; `mo` holds its aggregates, the
// distinct measures they read and the columns its second pass folds.
// STEP_SESSIONS (sdqh_table_sessions) cuts the partitions of the first npart terms by `ssr` and returns every row (per_session 0) or
// one row per session — then it filters as STEP_GROUPS does; `ss` are its columns, `aggs` the folds among them.
// STEP_WMOMENTS (sdqh_table_window_moments) returns every row with `wm`'s columns: frames as STEP_EXCLUDES finds them, moments in them.
// Behind the dispatch a step is built from shared pieces: the partition pass (Partitions), the filter (rank_filter), the tile fold
// (tile_fold), the frame pass of `rg` / `ex.rg` / `wm.rg` (Frames) and the level pass of `levels` / `ngroup` (Levels); see each.
enum StepKind { STEP_NONE, STEP_RANKS, STEP_FRAMES, STEP_SLIDES, STEP_RANGES, STEP_QUANTILES, STEP_EXCLUDES, STEP_GROUPS, STEP_DISTINCTS, STEP_MOMENTS, STEP_SESSIONS, STEP_WMOMENTS };
struct SortStep {
    StepKind kind; int npart;
    bool filters; int rank_kind; int64_t per_limit;
    int64_t* out;
    union { DevWaggs aggs; DevWslides sl; DevWranges rg; DevWquants q; DevWexs ex; };
    uint32_t levels; int64_t* level_rows; DevGsAvg avg;
    int ngroup; DevGdAggs gd;
    DevMoAggs mo;
    int per_session; DevSsRule ssr; DevSsCols ss;
    DevWmos wm;
};
static_assert(SDQH_WSLIDE_MAX_AGGS == SDQH_WAGG_MAX_AGGS && SDQH_WRANGE_MAX_AGGS == SDQH_WAGG_MAX_AGGS && SDQH_WQUANT_MAX_COLS == SDQH_WAGG_MAX_AGGS,
              "one list of result arrays serves frames, slides, ranges and quantiles");
static SortStep sort_step(StepKind kind, int npart, int64_t* out) {
    SortStep st; std::memset(&st, 0, sizeof(st));
    st.kind = kind; st.npart = npart; st.out = out; st.rank_kind = SDQH_WIN_ROW_NUMBER; st.per_limit = INT64_MAX;
    return st;
}

// One call between the passes and the emit: what the pieces of its step read, and what they leave for the emit and the fetch.
struct StepRun {
    sdqh_ctx* ctx; sdqh_table* table; const std::string& me; const SortStep& step; const SortState& s; Scratch& scratch;
    int nsort; int64_t n, limit, capacity; bool count_only, all_kept; int64_t* out_n;
    uint32_t un; size_t stride;                                       // n as the kernels take it; column a's values start at a * stride
    int64_t m;                                                        // rows returned: min(limit, kept)
    const uint32_t* sel = nullptr;                                    // their sorted positions (nullptr: the first m)
    const uint32_t* rank = nullptr;                                   // the ranks the emit writes beside them (nullptr: no rank column)
    const uint64_t* col_src[SDQH_WAGG_MAX_AGGS] = {nullptr, nullptr, nullptr, nullptr};      // where each of the ncols columns lies once the step ran
    int ncols = 0;
    bool ended = false;                                               // a way out was taken: *out_n is set and the call closed
    unsigned row_grid() const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + TPB - 1) / TPB, (int64_t)ctx->num_cu * 8)); }      // a thread per returned row
    void columns(const uint64_t* first, int count) { for (ncols = 0; ncols < count; ++ncols) col_src[ncols] = first + (size_t)ncols * stride; }
    int done(int64_t rows) { *out_n = rows; call_end(ctx); ended = true; return SDQH_OK; }
    int overflow(int64_t rows) { *out_n = rows; call_end(ctx); ended = true; return fail(ctx, SDQH_ERR_OVERFLOW, me + ": capacity too small"); }
    int nomem() const { return fail(ctx, SDQH_ERR_NOMEM, me + ": out of device memory"); }
    // a step that returns groups knows its count only now: m, and the ways out again (taken: `ended`)
    int counted(int64_t rows) {
        m = std::min<int64_t>(limit, rows);
        if (count_only) return done(m);
        return m > capacity ? overflow(m) : SDQH_OK;
    }
};

// The partition pass: the arrays every family reads its partitions from — out of the family's block 3 (take() inside its layout):
// head flags and tile carries always, the others as its kernels read them (an array not asked for takes no bytes) — and the kernels
// that fill them: `what` of the four, in this order.  A family whose own kernels come in between asks twice: frames fill the first
// heads themselves (k_wagg_tiles), quantiles filter behind PP_SCAN and mark tie heads (k_wq_ties) in front of PP_NEXT.
struct Partitions : Tiles {                                           // (the tiles of the n sorted positions)
    uint8_t* heads = nullptr; WinCarry* carry = nullptr; uint32_t* rown = nullptr; WaggHeads *tfirst = nullptr, *tnext = nullptr;
    void take(Carver& c, int64_t n, bool rows, bool firsts, bool nexts) {
        static_cast<Tiles&>(*this) = Tiles(n);
        heads = c.take<uint8_t>((size_t)n);
        carry = c.take<WinCarry>(ntiles);
        rown = c.take<uint32_t>(rows ? (size_t)n : 0);
        tfirst = c.take<WaggHeads>(firsts ? ntiles : 0);
        tnext = c.take<WaggHeads>(nexts ? ntiles : 0);
    }
};
enum { PP_HEADS = 1, PP_SCAN = 2, PP_ROWS = 4, PP_NEXT = 8 };
static void partition_pass(const StepRun& r, const Partitions& p, int what) {
    if (what & PP_HEADS) LAUNCH(r.ctx, "k_win_heads", k_win_heads, p.tgrid, r.s.keys, r.s.key_stride, r.step.npart, r.nsort, r.s.perm, r.un, p.heads, p.carry, p.ntiles);
    if (what & PP_SCAN) LAUNCH(r.ctx, "k_win_scan", k_win_scan, 1, p.carry, p.ntiles);
    if (what & PP_ROWS) LAUNCH(r.ctx, "k_wsl_rows", k_wsl_rows, p.tgrid, p.heads, p.carry, r.un, p.rown, p.tfirst, p.ntiles);
    if (what & PP_NEXT) LAUNCH(r.ctx, "k_wagg_next", k_wagg_next, 1, p.tfirst, r.un, p.tnext, p.ntiles);
}

// The tile fold of the frames, over whatever head flags cut the rows (partitions, the highest level's groups, sessions): every
// fold's element of every position and the tiles' carries and first heads, the carries scanned and — `run` — the running value of
// every position in place of its element.  Without `run` the carries are left for k_gs_run, which keeps a group's last value.
static void tile_fold(const StepRun& r, const Tiles& t, const DevWaggs& ag, const uint8_t* heads, uint64_t* elem, uint64_t* tval, WaggHeads* tfirst, bool run) {
    LAUNCH(r.ctx, "k_wagg_tiles", k_wagg_tiles, t.tgrid, r.table->stage, ag, r.s.refs, r.s.perm, heads, r.un, r.stride, elem, tval, tfirst, t.ntiles);
    LAUNCH(r.ctx, "k_wagg_scan", k_wagg_scan, (unsigned)ag.n, ag, tfirst, r.un, tval, t.ntiles);
    if (run) LAUNCH(r.ctx, "k_wagg_run", k_wagg_run, t.tgrid, ag, heads, r.un, r.stride, elem, tval, t.ntiles);
}

// The filter (behind PP_SCAN): the step's rank of every position into `rank`, the positions with rank <= per_limit counted per tile;
// then, unless every row is kept, the count to the host (a second wait), the ways out again — a filtering call knows its count only
// here — and the kept positions placed in order.  Leaves r.m and r.sel.
static int rank_filter(StepRun& r, const Partitions& p, uint32_t* rank, uint32_t* tile_kept, uint32_t* sel) {
    sdqh_ctx* ctx = r.ctx;
    const uint64_t pl = (uint64_t)r.step.per_limit;
    LAUNCH(ctx, "k_win_rank", k_win_rank, p.tgrid, p.heads, p.carry, r.un, r.step.rank_kind, pl, rank, tile_kept, p.ntiles);
    if (r.all_kept) return SDQH_OK;
    LAUNCH(ctx, "k_sort_scan", k_sort_scan, 1, tile_kept, (int)p.ntiles, r.s.info);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->result_host, r.s.info, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    unsigned long long kept;
    std::memcpy(&kept, ctx->result_host, 8);
    r.m = std::min<int64_t>(r.limit, (int64_t)kept);
    if (r.count_only || r.m == 0) return r.done(r.m);
    if (r.m > r.capacity) return r.overflow(r.m);
    LAUNCH(ctx, "k_win_place", k_win_place, p.tgrid, rank, r.un, pl, tile_kept, p.ntiles, sel, (uint32_t)r.m);
    r.sel = sel;
    return SDQH_OK;
}

// The frame pass: where the data-dependent frames of ranges, excludes and moments over frames are found.  Its constructor reads the
// family's DevWranges image — a folded column's tree slot, a FIRST / LAST column's element slot, is there a GROUPS column, does a
// column exclude its GROUP or TIES (`exclude`: excludes alone have one), a ROWS offset clamped as a slide's is — take() lays
// [partition pass | partition ends | dense ranks | kept per tile | tie-run ranks | kept per tile of that pass | tie-run ends | VALUE
// keys | GROUPS keys] in front of the family's own arrays (an array nobody asked for takes no bytes and is null), and frame_pass fills
// them; frame_trees builds the fold trees of the folded columns bottom-up.
struct Frames {
    Partitions p;
    int nfold = 0, nraw = 0; bool groups = false, ties = false;
    uint64_t cap = SORT_TILE;                                          // the trees' leaf count: the power of two at or above n
    size_t tstride = 0;                                                // a fold tree: nodes [1, cap), leaves [cap, 2 cap)
    uint32_t *pend = nullptr, *dense = nullptr, *tile_kept = nullptr, *frank = nullptr, *fkept = nullptr, *tend = nullptr;
    uint64_t *vkey = nullptr, *gkey = nullptr;
    Frames(DevWranges& rg, int64_t n, const int32_t* exclude) {
        for (int a = 0; a < rg.n; ++a) {
            DevWrange& d = rg.a[a];
            d.slot = d.g.cls != WSL_NONE ? nfold++ : (d.g.op != SDQH_WAGG_COUNT ? nraw++ : 0);
            groups |= d.unit == SDQH_WRANGE_GROUPS;
            ties |= exclude && (exclude[a] == SDQH_WEX_GROUP || exclude[a] == SDQH_WEX_TIES);
            if (d.unit == SDQH_WEX_ROWS) {                             // an offset of n or more reaches outside every partition: clamped, as a slide's is
                d.lo = std::max<int64_t>(std::min<int64_t>(d.lo, n), -n);
                d.hi = std::max<int64_t>(std::min<int64_t>(d.hi, n), -n);
            }
        }
        while (cap < (uint64_t)n) cap <<= 1;
        tstride = nfold ? (size_t)(2 * cap) : 0;
    }
    void take(Carver& c, int64_t n, const DevWranges& rg) {
        p.take(c, n, true, true, true);
        pend = c.take<uint32_t>((size_t)n);
        dense = c.take<uint32_t>(groups ? (size_t)n : 0);
        tile_kept = c.take<uint32_t>(groups ? p.ntiles : 0);
        frank = c.take<uint32_t>(ties ? (size_t)n : 0);
        fkept = c.take<uint32_t>(ties ? p.ntiles : 0);
        tend = c.take<uint32_t>(ties ? (size_t)n : 0);
        vkey = c.take<uint64_t>(rg.vcol >= 0 ? (size_t)n : 0);
        gkey = c.take<uint64_t>(groups ? (size_t)n : 0);
        if (rg.vcol < 0) vkey = nullptr;
        if (!groups) { dense = nullptr; gkey = nullptr; }
        if (!ties) { frank = nullptr; tend = nullptr; }
    }
};
// partitions, rows and ends; with ties the first tie heads, tie-run ranks and ends; with a GROUPS column the dense ranks; then
// k_wrg_stage: the partitions' ends, the frames' keys, and the columns' elements — raw into `elem`, leaves into `tree` (both null: none)
static void frame_pass(const StepRun& r, const Frames& f, const DevWranges& rg, uint64_t* elem, uint64_t* tree) {
    const Partitions& p = f.p;
    partition_pass(r, p, PP_HEADS | PP_SCAN | PP_ROWS);
    if (f.ties) LAUNCH(r.ctx, "k_wq_ties", k_wq_ties, p.tgrid, p.heads, r.un, p.tfirst, p.ntiles);
    partition_pass(r, p, PP_NEXT);
    if (f.groups) LAUNCH(r.ctx, "k_win_rank", k_win_rank, p.tgrid, p.heads, p.carry, r.un, (int)SDQH_WIN_DENSE_RANK, ~0ull, f.dense, f.tile_kept, p.ntiles);
    if (f.ties) {
        LAUNCH(r.ctx, "k_win_rank", k_win_rank, p.tgrid, p.heads, p.carry, r.un, (int)SDQH_WIN_RANK, ~0ull, f.frank, f.fkept, p.ntiles);
        LAUNCH(r.ctx, "k_wex_ties", k_wex_ties, p.tgrid, p.heads, p.tnext, r.un, f.tend, p.ntiles);
    }
    LAUNCH(r.ctx, "k_wrg_stage", k_wrg_stage, p.tgrid, r.table->stage, rg, r.s.refs, r.s.perm, p.heads, p.tnext, rg.vcol >= 0 ? r.s.keys + (size_t)rg.vcol * r.s.key_stride : nullptr, f.dense, r.un,
           r.stride, f.tstride, f.cap, f.pend, f.vkey, f.gkey, elem, tree, p.ntiles);
}
static void frame_trees(const StepRun& r, const Frames& f, const DevWranges& rg, uint64_t* tree) {
    if (!f.nfold) return;
    LAUNCH(r.ctx, "k_wrg_tiles", k_wrg_tiles, f.p.tgrid, rg, r.un, f.tstride, f.cap, tree, f.p.ntiles);
    if (f.cap > (uint64_t)SORT_TILE) LAUNCH(r.ctx, "k_wrg_upper", k_wrg_upper, (unsigned)f.nfold, rg, f.tstride, f.cap, tree, f.p.ntiles);
}

// The family steps.  Each carves block 3 (scratch.p[3]: one pool block per call, the partition pass's arrays and its own in one
// layout), runs the partition pass and its own kernels, and leaves what the emit and the fetch need in the StepRun.
// Ranks (sdqh_table_window): block 3 = [partition pass | ranks | kept per tile | kept positions | slack].  The emit writes the ranks.
static int step_ranks(StepRun& r) {
    Partitions p;
    uint32_t *rank = nullptr, *tile_kept = nullptr, *sel = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            p.take(c, r.n, false, false, false);
            rank = c.take<uint32_t>((size_t)r.n);
            tile_kept = c.take<uint32_t>(p.ntiles);
            sel = c.take<uint32_t>(r.all_kept ? 0 : (size_t)r.n);
            (void)c.take<char>(256);
        })) return r.nomem();
    partition_pass(r, p, PP_HEADS | PP_SCAN);
    r.rank = rank;
    return rank_filter(r, p, rank, tile_kept, sel);
}

// Aggregates over frames (sdqh_table_window_agg): block 3 = [partition pass | ROWS values | RANGE / PARTITION values | value carries].
// Every position is kept: row j is sorted position j, the first m values are the output.
static int step_frames(StepRun& r) {
    const DevWaggs& ag = r.step.aggs;
    const size_t na = (size_t)ag.n;
    bool ends = false;                                                // does some aggregate ask for RANGE or PARTITION?
    for (size_t a = 0; a < na; ++a) ends |= ag.a[a].frame != SDQH_FRAME_ROWS;
    Partitions p;
    uint64_t *elem = nullptr, *fin = nullptr, *tval = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            p.take(c, r.n, false, true, ends);
            elem = c.take<uint64_t>(r.stride * na);
            fin = c.take<uint64_t>(ends ? r.stride * na : 0);
            tval = c.take<uint64_t>((size_t)p.ntiles * na);
        })) return r.nomem();
    partition_pass(r, p, PP_HEADS);
    tile_fold(r, p, ag, p.heads, elem, tval, p.tfirst, true);
    if (ends) {
        const Tiles mt(r.m);                                          // (the returned rows' tiles)
        partition_pass(r, p, PP_NEXT);
        LAUNCH(r.ctx, "k_wagg_ends", k_wagg_ends, mt.tgrid, ag, p.heads, p.tnext, r.un, (uint32_t)r.m, r.stride, elem, fin, mt.ntiles);
    }
    r.columns(elem, ag.n);                                            // each from the array its frame left it in
    for (int a = 0; a < ag.n; ++a) if (ag.a[a].frame != SDQH_FRAME_ROWS) r.col_src[a] = fin + (size_t)a * r.stride;
    return SDQH_OK;
}

// Values over sliding frames (sdqh_table_window_slide): block 3 = [partition pass | partition ends | block-head flags | elements, then
// suffix folds | prefix folds | values | fold carries | their head flags]
static int step_slides(StepRun& r) {
    const int64_t n = r.n;
    DevWslides sl = r.step.sl;
    const size_t na = (size_t)sl.n;
    bool folds = false;                                               // does some slide fold (SUM / MIN / MAX)?
    for (size_t a = 0; a < na; ++a) {
        // an offset of n or more reaches outside every partition, whichever it is: clamped, the arithmetic stays far inside 64 bits
        DevWslide& d = sl.a[a];
        d.lo = std::max<int64_t>(std::min<int64_t>(d.lo, n), -n);
        d.hi = std::max<int64_t>(std::min<int64_t>(d.hi, n), -n);
        d.w = (uint32_t)std::min<int64_t>(d.hi - d.lo + 1, n);
        folds |= d.g.cls != WSL_NONE;
    }
    Partitions p;
    uint8_t *bh = nullptr, *thead = nullptr; uint32_t* pend = nullptr;
    uint64_t *elem = nullptr, *pre = nullptr, *fin = nullptr, *tval = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            p.take(c, n, true, true, true);
            pend = c.take<uint32_t>((size_t)n);
            bh = c.take<uint8_t>((size_t)n);
            elem = c.take<uint64_t>(r.stride * na);
            pre = c.take<uint64_t>(folds ? r.stride * na : 0);
            fin = c.take<uint64_t>(r.stride * na);
            tval = c.take<uint64_t>(folds ? (size_t)p.ntiles * 2 * SDQH_WSLIDE_MAX_AGGS : 0);
            thead = c.take<uint8_t>(folds ? (size_t)p.ntiles * 2 * SDQH_WSLIDE_MAX_AGGS : 0);
        })) return r.nomem();
    partition_pass(r, p, PP_HEADS | PP_SCAN | PP_ROWS | PP_NEXT);
    LAUNCH(r.ctx, "k_wsl_blocks", k_wsl_blocks, p.tgrid, r.table->stage, sl, r.s.refs, r.s.perm, p.heads, p.tnext, p.rown, r.un, r.stride, pend, bh, elem, p.ntiles);
    if (folds) {
        LAUNCH(r.ctx, "k_wsl_tiles", k_wsl_tiles, p.tgrid, sl, bh, r.un, r.stride, elem, tval, thead, p.ntiles);
        LAUNCH(r.ctx, "k_wsl_scan", k_wsl_scan, 2 * SDQH_WSLIDE_MAX_AGGS, sl, thead, tval, p.ntiles);
        LAUNCH(r.ctx, "k_wsl_run", k_wsl_run, p.tgrid, sl, bh, r.un, r.stride, elem, pre, tval, p.ntiles);
    }
    LAUNCH(r.ctx, "k_wsl_fold", k_wsl_fold, r.row_grid(), sl, p.rown, pend, r.un, (uint32_t)r.m, r.stride, elem, pre, fin);
    r.columns(fin, sl.n);
    return SDQH_OK;
}

// Values over value and group frames (sdqh_table_window_range): block 3 = [frame pass | raw elements, an array per FIRST / LAST
// range | fold trees, one per folded range (SUM / MIN / MAX) | values]
static int step_ranges(StepRun& r) {
    DevWranges rg = r.step.rg;
    Frames f(rg, r.n, nullptr);
    uint64_t *elem = nullptr, *tree = nullptr, *fin = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            f.take(c, r.n, rg);
            elem = c.take<uint64_t>(r.stride * (size_t)f.nraw);
            tree = c.take<uint64_t>(f.tstride * (size_t)f.nfold);
            fin = c.take<uint64_t>(r.stride * (size_t)rg.n);
        })) return r.nomem();
    frame_pass(r, f, rg, elem, tree);
    frame_trees(r, f, rg, tree);
    LAUNCH(r.ctx, "k_wrg_fold", k_wrg_fold, r.row_grid(), rg, f.p.rown, f.pend, f.vkey, f.gkey, r.un, (uint32_t)r.m, r.stride, f.tstride, f.cap, elem, tree, fin);
    r.columns(fin, rg.n);
    return SDQH_OK;
}

// Functions of the partition's size (sdqh_table_window_quantile): block 3 = [partition pass | partition ends | tie-run ends | tie-run
// ranks | kept per tile of that pass | row numbers from 1 | kept per tile | kept positions | measure elements, an array per distinct
// measure | values] — the tie arrays only with a CUME_DIST / PERCENT_RANK column, the three kept arrays only when per_limit filters,
// the rest (row numbers, first and next heads among them) only when columns are asked for
static int step_quantiles(StepRun& r) {
    const int64_t n = r.n;
    const DevWquants& q = r.step.q;
    const bool cols = r.step.out != nullptr;
    bool need_f = false, need_l = false;                              // does some column read the tie run's first / last position?
    for (int c = 0; cols && c < q.n; ++c) { need_f |= q.a[c].fn == SDQH_WQ_PERCENT_RANK; need_l |= q.a[c].fn == SDQH_WQ_CUME_DIST; }
    Partitions p;
    uint32_t *pend = nullptr, *tend = nullptr, *frank = nullptr, *fkept = nullptr, *rank = nullptr, *tile_kept = nullptr, *sel = nullptr;
    uint64_t *elem = nullptr, *fin = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            p.take(c, n, cols, cols, cols);
            pend = c.take<uint32_t>(cols ? (size_t)n : 0);
            tend = c.take<uint32_t>(need_l ? (size_t)n : 0);
            frank = c.take<uint32_t>(need_f ? (size_t)n : 0);
            fkept = c.take<uint32_t>(need_f ? p.ntiles : 0);
            rank = c.take<uint32_t>(r.all_kept ? 0 : (size_t)n);
            tile_kept = c.take<uint32_t>(r.all_kept ? 0 : p.ntiles);
            sel = c.take<uint32_t>(r.all_kept ? 0 : (size_t)n);
            elem = c.take<uint64_t>(cols ? r.stride * (size_t)q.nslots : 0);
            fin = c.take<uint64_t>(cols ? r.stride * (size_t)q.n : 0);
        })) return r.nomem();
    if (!need_l) tend = nullptr;
    if (!need_f) frank = nullptr;
    partition_pass(r, p, PP_HEADS | PP_SCAN);
    if (!r.all_kept) {                                                // sdqh_table_window's filter on ROW_NUMBER, its ranks the filter's own
        const int rc = rank_filter(r, p, rank, tile_kept, sel);
        if (rc || r.ended) return rc;
    }
    if (!cols) return SDQH_OK;
    partition_pass(r, p, PP_ROWS);
    if (need_l) LAUNCH(r.ctx, "k_wq_ties", k_wq_ties, p.tgrid, p.heads, r.un, p.tfirst, p.ntiles);
    partition_pass(r, p, PP_NEXT);
    if (need_f) LAUNCH(r.ctx, "k_win_rank", k_win_rank, p.tgrid, p.heads, p.carry, r.un, (int)SDQH_WIN_RANK, ~0ull, frank, fkept, p.ntiles);
    LAUNCH(r.ctx, "k_wq_stage", k_wq_stage, p.tgrid, r.table->stage, q, r.s.refs, r.s.perm, p.heads, p.tnext, r.un, r.stride, pend, tend, elem, p.ntiles);
    LAUNCH(r.ctx, "k_wq_value", k_wq_value, r.row_grid(), q, r.sel, p.rown, pend, tend, frank, r.un, (uint32_t)r.m, r.stride, elem, fin);
    r.columns(fin, q.n);
    return SDQH_OK;
}

// Values over frames with rows taken out (sdqh_table_window_exclude): block 3 = [frame pass, its tie arrays when some column excludes
// GROUP or TIES | raw elements, an array per FIRST / LAST column | fold trees, one per folded column (SUM / MIN / MAX / AVG) | values].
// The trees and the keys are the ranges': the frame pass over the columns' DevWranges image.
static int step_excludes(StepRun& r) {
    DevWexs ex = r.step.ex;
    DevWranges& rg = ex.rg;
    Frames f(rg, r.n, ex.exclude);
    uint64_t *elem = nullptr, *tree = nullptr, *fin = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            f.take(c, r.n, rg);
            elem = c.take<uint64_t>(r.stride * (size_t)f.nraw);
            tree = c.take<uint64_t>(f.tstride * (size_t)f.nfold);
            fin = c.take<uint64_t>(r.stride * (size_t)rg.n);
        })) return r.nomem();
    frame_pass(r, f, rg, elem, tree);
    frame_trees(r, f, rg, tree);
    LAUNCH(r.ctx, "k_wex_fold", k_wex_fold, r.row_grid(), ex, f.p.rown, f.pend, f.frank, f.tend, f.vkey, f.gkey, r.un, (uint32_t)r.m, r.stride, f.tstride, f.cap, elem, tree, fin);
    r.columns(fin, rg.n);
    return SDQH_OK;
}

// The level pass: the steps that return one row per group find the heads of every level of the nsort terms at once.  Block 3 =
// [depths | head flags of level `top` | heads per tile and level | level counts], laid out and filled by level_pass: k_gs_depth, then
// level_counts — the tiles' heads scanned per level in place (k_sort_bins, a workgroup a level: a level's tile offsets), the level
// counts to the host (the call's second wait, as a filter's) into tot[].  level_sets is what groups and moments make of them.
struct Levels : Tiles {                                               // (the tiles of the n sorted positions)
    int nl = 0, top = 0;                                              // nsort + 1 levels; the highest one the call reads
    uint8_t *depth = nullptr, *heads = nullptr; uint32_t *tcount = nullptr, *ltot = nullptr;
    uint32_t tot[SDQH_SORT_MAX_KEYS + 1];                             // level L's groups
    DevGsLevels lv; int lvl[SDQH_SORT_MAX_KEYS + 1]; int64_t g = 0;   // level_sets: the levels asked for, highest first; their groups in all
    const uint32_t* offsets(int L) const { return tcount + (size_t)L * ntiles; }
};
static int level_counts(StepRun& r, uint32_t* tcount, uint32_t ntiles, uint32_t* ltot, int nl, uint32_t* tot) {
    sdqh_ctx* ctx = r.ctx;
    LAUNCH(ctx, "k_sort_bins", k_sort_bins, (unsigned)nl, tcount, ntiles, ltot);      // per level: the tiles' offsets in place, the level's count
    HIP_TRY(ctx, hipMemcpyAsync(ctx->result_host, ltot, (size_t)nl * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    std::memcpy(tot, ctx->result_host, (size_t)nl * 4);
    return SDQH_OK;
}
static int level_pass(StepRun& r, Levels& p, int top) {
    static_cast<Tiles&>(p) = Tiles(r.n);
    p.nl = r.nsort + 1; p.top = top;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            p.depth = c.take<uint8_t>((size_t)r.n);
            p.heads = c.take<uint8_t>((size_t)r.n);
            p.tcount = c.take<uint32_t>((size_t)p.ntiles * (size_t)p.nl);
            p.ltot = c.take<uint32_t>(SDQH_SORT_MAX_KEYS + 1);
        })) return r.nomem();
    LAUNCH(r.ctx, "k_gs_depth", k_gs_depth, p.tgrid, r.s.keys, r.s.key_stride, r.nsort, top, r.s.perm, r.un, p.depth, p.heads, p.tcount, p.ntiles);
    return level_counts(r, p.tcount, p.ntiles, p.ltot, p.nl, p.tot);
}
// The level pass up to the highest of the step's `levels`, then the levels asked for from the highest down — lvl[k], its groups rows
// [lv.off[k], lv.off[k + 1]) of the output, g in all —, their counts to level_rows, and the ways out (r.counted).
static int level_sets(StepRun& r, Levels& p) {
    const uint32_t levels = r.step.levels;
    int top = r.nsort;
    while (!((levels >> top) & 1u)) --top;                            // (levels != 0 and no bit above nsort: the entry point's check)
    if (int rc = level_pass(r, p, top)) return rc;
    std::memset(&p.lv, 0, sizeof(p.lv));
    for (int L = top; L >= 0; --L) if ((levels >> L) & 1u) { p.lvl[p.lv.n] = L; p.g += (int64_t)p.tot[L]; p.lv.off[++p.lv.n] = (uint32_t)p.g; }
    if (p.g > 0xFFFFFFFFll) return fail(r.ctx, SDQH_ERR_UNSUPPORTED, r.me + ": more than 2^32 - 1 groups over the levels asked for");
    if (r.step.level_rows) for (int L = 0; L <= SDQH_SORT_MAX_KEYS; ++L) r.step.level_rows[L] = (L < p.nl && ((levels >> L) & 1u)) ? (int64_t)p.tot[L] : 0;
    return r.counted(p.g);
}

// Groups at nested levels (sdqh_table_grouping_sets).  Block 3 is the level pass's; only behind its ways out is the output's size
// known: block 4 = [representatives' positions | their depths | group values | the rows' elements | value carries | first heads |
// heads per tile | their total], the first three over all g groups, highest level first.
static int step_groups(StepRun& r) {
    sdqh_ctx* ctx = r.ctx;
    Levels p;
    const int rc = level_sets(r, p);
    if (rc || r.ended) return rc;
    const DevGsLevels& lv = p.lv;
    DevWaggs ag = r.step.aggs;
    if (!r.step.out) ag.n = 0;                                        // rows only: nothing is folded
    const size_t na = (size_t)ag.n, gstride = round_up((size_t)p.g * 8) / 8;
    uint32_t *sel = nullptr, *tcnt = nullptr, *tot1 = nullptr; uint8_t* gdepth = nullptr;
    uint64_t *fin = nullptr, *elem = nullptr, *tval = nullptr; WaggHeads* tfirst = nullptr;
    if (!carve(ctx, r.scratch.p[4], [&](Carver& c) {
            sel = c.take<uint32_t>((size_t)p.g);
            gdepth = c.take<uint8_t>((size_t)p.g);
            fin = c.take<uint64_t>(gstride * na);
            elem = c.take<uint64_t>(r.stride * na);
            tval = c.take<uint64_t>((size_t)p.ntiles * na);
            tfirst = c.take<WaggHeads>(p.ntiles);
            tcnt = c.take<uint32_t>(p.ntiles);
            tot1 = c.take<uint32_t>(1);
        })) return r.nomem();
    // the highest level, over the rows
    if (na) tile_fold(r, p, ag, p.heads, elem, tval, tfirst, false);
    LAUNCH(ctx, "k_gs_run", k_gs_run, p.tgrid, ag, p.top, 1, p.depth, (const uint32_t*)nullptr, elem, r.stride, r.un, tval, p.offsets(p.top), p.ntiles,
           fin, gstride, gdepth, sel, p.tot[p.top]);
    // every lower level, over the groups of the one above it
    for (int k = 1; k < lv.n; ++k) {
        const uint32_t nf = p.tot[p.lvl[k - 1]], from = lv.off[k - 1], to = lv.off[k];
        const Tiles ft(nf);                                           // SORT_TILE groups of the level above each
        LAUNCH(ctx, "k_gs_tiles", k_gs_tiles, ft.tgrid, ag, p.lvl[k], gdepth + from, fin + from, gstride, nf, tval, tfirst, tcnt, ft.ntiles);
        if (na) LAUNCH(ctx, "k_wagg_scan", k_wagg_scan, (unsigned)na, ag, tfirst, nf, tval, ft.ntiles);
        LAUNCH(ctx, "k_sort_bins", k_sort_bins, 1, tcnt, ft.ntiles, tot1);
        LAUNCH(ctx, "k_gs_run", k_gs_run, ft.tgrid, ag, p.lvl[k], 0, gdepth + from, sel + from, fin + from, gstride, nf, tval, tcnt, ft.ntiles,
               fin + to, gstride, gdepth + to, sel + to, p.tot[p.lvl[k]]);
    }
    bool avg = false;
    for (size_t a = 0; a < na; ++a) avg |= r.step.avg.avg[a] != 0;
    if (avg) LAUNCH(ctx, "k_gs_avg", k_gs_avg, r.row_grid(), r.step.avg, lv, sel, r.un, (uint32_t)r.m, gstride, fin);
    r.sel = sel;
    for (r.ncols = 0; r.ncols < ag.n; ++r.ncols) r.col_src[r.ncols] = fin + (size_t)r.ncols * gstride;
    return SDQH_OK;
}

// Aggregates over the distinct values of a group (sdqh_table_group_distinct).  Block 3 is the level pass's, up to level nsort.  Of
// its counts the step reads two, the runs' (level nsort) and the groups' (level ngroup), and takes the ways out.  Block 4 = [runs:
// positions | depths | elements] [groups: first runs | depths | values | positions] [the upper stage's value carries | first heads |
// heads per tile | their total].
static int step_distincts(StepRun& r) {
    sdqh_ctx* ctx = r.ctx;
    const int top = r.nsort, L = r.step.ngroup;
    Levels p;
    if (int rc = level_pass(r, p, top)) return rc;
    const uint32_t nr = p.tot[top], ng = p.tot[L];                    // value runs, groups: 1 <= ng <= nr <= n
    const int rc = r.counted((int64_t)ng);
    if (rc || r.ended) return rc;
    DevWaggs ag = r.step.aggs;
    DevGdAggs gd = r.step.gd;
    if (!r.step.out) ag.n = gd.n = 0;                                 // rows only: nothing is folded
    const size_t na = (size_t)ag.n, rstride = round_up((size_t)nr * 8) / 8, gstride = round_up((size_t)ng * 8) / 8;
    const Tiles ft(nr);                                               // the upper stage's tiles: SORT_TILE runs each
    const uint32_t nt = ft.ntiles;
    uint32_t *rpos = nullptr, *gfirst = nullptr, *sel = nullptr, *tcnt = nullptr, *tot1 = nullptr; uint8_t *rdepth = nullptr, *gdepth = nullptr;
    uint64_t *elem = nullptr, *fin = nullptr, *tval = nullptr; WaggHeads* tfirst = nullptr;
    if (!carve(ctx, r.scratch.p[4], [&](Carver& c) {
            rpos = c.take<uint32_t>((size_t)nr);
            rdepth = c.take<uint8_t>((size_t)nr);
            elem = c.take<uint64_t>(rstride * na);
            gfirst = c.take<uint32_t>((size_t)ng);
            gdepth = c.take<uint8_t>((size_t)ng);
            fin = c.take<uint64_t>(gstride * na);
            sel = c.take<uint32_t>((size_t)ng);
            tval = c.take<uint64_t>((size_t)nt * na);
            tfirst = c.take<WaggHeads>(nt);
            tcnt = c.take<uint32_t>(nt);
            tot1 = c.take<uint32_t>(1);
        })) return r.nomem();
    // the lower stage: rows -> value runs
    const unsigned rgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)nr + TPB - 1) / TPB, (int64_t)ctx->num_cu * 8));
    LAUNCH(ctx, "k_gd_heads", k_gd_heads, p.tgrid, top, p.depth, r.un, p.offsets(top), p.ntiles, rpos, rdepth, nr);
    if (na) LAUNCH(ctx, "k_gd_elems", k_gd_elems, rgrid, r.table->stage, gd, r.s.refs, r.s.perm, rpos, r.un, nr, rstride, elem);
    // the upper stage: value runs -> groups, a lower level of the grouping sets over the runs (positions: run indices)
    LAUNCH(ctx, "k_gs_tiles", k_gs_tiles, ft.tgrid, ag, L, rdepth, elem, rstride, nr, tval, tfirst, tcnt, nt);
    if (na) LAUNCH(ctx, "k_wagg_scan", k_wagg_scan, (unsigned)na, ag, tfirst, nr, tval, nt);
    LAUNCH(ctx, "k_sort_bins", k_sort_bins, 1, tcnt, nt, tot1);
    LAUNCH(ctx, "k_gs_run", k_gs_run, ft.tgrid, ag, L, 0, rdepth, (const uint32_t*)nullptr, elem, rstride, nr, tval, tcnt, nt, fin, gstride, gdepth, gfirst, ng);
    LAUNCH(ctx, "k_gd_finish", k_gd_finish, r.row_grid(), r.table->stage, gd, r.s.refs, r.s.perm, rpos, gfirst, r.un, nr, ng, (uint32_t)r.m, gstride, fin, sel);
    r.sel = sel;
    for (r.ncols = 0; r.ncols < ag.n; ++r.ncols) r.col_src[r.ncols] = fin + (size_t)r.ncols * gstride;
    return SDQH_OK;
}

// Second moments per group (sdqh_table_group_moments).  Block 3 is the level pass's, the levels and the ways out step_groups'.
// Block 4 = [groups: positions | depths | pass 1's sums | pass 2's sums | results] [rows: staged measures | centred products] [value
// carries | first heads | heads per tile].  Every level asked for is folded over the rows, its tile offsets the level pass's.
static int step_moments(StepRun& r) {
    sdqh_ctx* ctx = r.ctx;
    Levels p;
    const int rc = level_sets(r, p);
    if (rc || r.ended) return rc;
    const DevGsLevels& lv = p.lv;
    const uint32_t ntiles = p.ntiles; const unsigned tgrid = p.tgrid; const int64_t g = p.g;
    const uint8_t* depth = p.depth;
    DevMoAggs mo = r.step.mo;
    if (!r.step.out) mo.n = mo.nmeas = mo.ncen = 0;                   // rows only: nothing is folded
    const size_t na = (size_t)mo.n, nm = (size_t)mo.nmeas, nc = (size_t)mo.ncen, gstride = round_up((size_t)g * 8) / 8;
    uint32_t *sel = nullptr, *tcnt = nullptr; uint8_t* gdepth = nullptr;
    uint64_t *sums = nullptr, *cens = nullptr, *fin = nullptr, *elem = nullptr, *cen = nullptr, *tval = nullptr; WaggHeads* tfirst = nullptr;
    if (!carve(ctx, r.scratch.p[4], [&](Carver& c) {
            sel = c.take<uint32_t>((size_t)g);
            gdepth = c.take<uint8_t>((size_t)g);
            sums = c.take<uint64_t>(gstride * nm);
            cens = c.take<uint64_t>(gstride * nc);
            fin = c.take<uint64_t>(gstride * na);
            elem = c.take<uint64_t>(r.stride * nm);
            cen = c.take<uint64_t>(r.stride * nc);
            tval = c.take<uint64_t>((size_t)ntiles * SDQH_WAGG_MAX_AGGS);
            tfirst = c.take<WaggHeads>(ntiles);
            tcnt = c.take<uint32_t>(ntiles);
        })) return r.nomem();
    for (int k = 0; k < lv.n; ++k) {
        const int L = p.lvl[k];
        const uint32_t from = lv.off[k], ng = p.tot[L];
        const uint32_t* toff = p.offsets(L);
        LAUNCH(ctx, "k_gd_heads", k_gd_heads, tgrid, L, depth, r.un, toff, ntiles, sel + from, gdepth + from, ng);
        if (!na) continue;
        // `cols` columns of doubles at `src`, one per row, summed per level-L group into `dst`: the frames' folds, four columns a launch
        auto fold = [&](const uint64_t* src, size_t cols, uint64_t* dst) {
            for (size_t c0 = 0; c0 < cols; c0 += SDQH_WAGG_MAX_AGGS) {
                DevWaggs ag; std::memset(&ag, 0, sizeof(ag));
                ag.n = (int32_t)std::min<size_t>(SDQH_WAGG_MAX_AGGS, cols - c0);
                for (int a = 0; a < ag.n; ++a) { ag.a[a].op = SDQH_WAGG_SUM; ag.a[a].frame = SDQH_FRAME_ROWS; ag.a[a].cls = WAGG_ADD_F; ag.a[a].sk.is_f64 = 1; }
                LAUNCH(ctx, "k_gs_tiles", k_gs_tiles, tgrid, ag, L, depth, src + c0 * r.stride, r.stride, r.un, tval, tfirst, tcnt, ntiles);
                LAUNCH(ctx, "k_wagg_scan", k_wagg_scan, (unsigned)ag.n, ag, tfirst, r.un, tval, ntiles);
                LAUNCH(ctx, "k_gs_run", k_gs_run, tgrid, ag, L, 1, depth, (const uint32_t*)nullptr, src + c0 * r.stride, r.stride, r.un, tval, toff, ntiles,
                       dst + c0 * gstride, gstride, gdepth + from, sel + from, ng);
            }
        };
        LAUNCH(ctx, "k_mo_stage", k_mo_stage, tgrid, r.table->stage, mo, L, r.s.refs, r.s.perm, depth, toff, sel + from, ng, r.un, r.stride, elem, ntiles);
        fold(elem, nm, sums + from);
        LAUNCH(ctx, "k_mo_center", k_mo_center, tgrid, mo, L, depth, toff, sel + from, ng, r.un, r.stride, elem, gstride, sums + from, cen, ntiles);
        fold(cen, nc, cens + from);
    }
    if (na) LAUNCH(ctx, "k_mo_finish", k_mo_finish, r.row_grid(), r.table->stage, mo, lv, r.s.refs, r.s.perm, sel, r.un, (uint32_t)r.m, gstride, sums, cens, fin);
    r.sel = sel;
    for (r.ncols = 0; r.ncols < mo.n; ++r.ncols) r.col_src[r.ncols] = fin + (size_t)r.ncols * gstride;
    return SDQH_OK;
}

// Sessions (sdqh_table_sessions).  Block 3 = [flags A | flags B | depths | carries A | carries B | first heads | next heads | heads
// per tile and level | level counts | session numbers | row numbers | kept per tile] and, per row, [elements, then running values |
// columns | value carries].  Per session the count of level 2 goes to the host — the call's second wait, as step_groups' — and the
// ways out are taken; block 4 = [sessions: positions | depths | folds | columns] [rows: elements | value carries].
static int step_sessions(StepRun& r) {
    sdqh_ctx* ctx = r.ctx;
    const bool per = r.step.per_session != 0;
    DevSsCols sc = r.step.ss;
    DevWaggs ag = r.step.aggs;
    if (!r.step.out) { sc.n = 0; ag.n = 0; }                          // rows only: no column is computed
    const size_t nc = (size_t)sc.n, nf = (size_t)ag.n;
    bool number = false, rown = false;                                // does a column read the sessions' numbers, the rows' numbers?
    for (int c = 0; c < sc.n; ++c) {
        number |= sc.op[c] == SDQH_SS_NUMBER;
        rown |= !per && (sc.op[c] == SDQH_SS_ROW || sc.op[c] == SDQH_WSLIDE_FIRST || sc.op[c] == SDQH_WEX_AVG);
    }
    const Tiles t(r.n);
    const uint32_t ntiles = t.ntiles; const unsigned tgrid = t.tgrid;
    uint8_t *headsA = nullptr, *headsB = nullptr, *depth = nullptr; WinCarry *carryA = nullptr, *carryB = nullptr; WaggHeads *tfirst = nullptr, *tnext = nullptr;
    uint32_t *tcount = nullptr, *ltot = nullptr, *numb = nullptr, *rowb = nullptr, *tile_kept = nullptr;
    uint64_t *elem = nullptr, *fin = nullptr, *tval = nullptr;
    if (!carve(ctx, r.scratch.p[3], [&](Carver& c) {
            headsA = c.take<uint8_t>((size_t)r.n);
            headsB = c.take<uint8_t>((size_t)r.n);
            depth = c.take<uint8_t>((size_t)r.n);
            carryA = c.take<WinCarry>(ntiles);
            carryB = c.take<WinCarry>(ntiles);
            tfirst = c.take<WaggHeads>(ntiles);
            tnext = c.take<WaggHeads>(ntiles);
            tcount = c.take<uint32_t>((size_t)ntiles * 3);
            ltot = c.take<uint32_t>(3);
            numb = c.take<uint32_t>(number ? (size_t)r.n : 0);
            rowb = c.take<uint32_t>(rown ? (size_t)r.n : 0);
            tile_kept = c.take<uint32_t>(ntiles);
            elem = c.take<uint64_t>(per ? 0 : r.stride * nf);
            fin = c.take<uint64_t>(per ? 0 : r.stride * nc);
            tval = c.take<uint64_t>(per ? 0 : (size_t)ntiles * nf);
        })) return r.nomem();
    if (!number) numb = nullptr;
    if (!rown) rowb = nullptr;
    LAUNCH(ctx, "k_ss_heads", k_ss_heads, tgrid, r.table->stage, r.step.ssr, r.s.keys, r.s.key_stride, r.step.npart, r.s.refs, r.s.perm, r.un, headsA, headsB, depth,
           carryA, carryB, tfirst, tcount, ntiles);
    if (number) {
        LAUNCH(ctx, "k_win_scan", k_win_scan, 1, carryA, ntiles);
        LAUNCH(ctx, "k_win_rank", k_win_rank, tgrid, headsA, carryA, r.un, (int)SDQH_WIN_DENSE_RANK, ~0ull, numb, tile_kept, ntiles);
    }
    if (!per) {
        if (rown) {
            LAUNCH(ctx, "k_win_scan", k_win_scan, 1, carryB, ntiles);
            LAUNCH(ctx, "k_win_rank", k_win_rank, tgrid, headsB, carryB, r.un, (int)SDQH_WIN_ROW_NUMBER, ~0ull, rowb, tile_kept, ntiles);
        }
        if (nf) tile_fold(r, t, ag, headsB, elem, tval, tfirst, true);
        const Tiles mt(r.m);                                          // (the returned rows' tiles)
        LAUNCH(ctx, "k_wagg_next", k_wagg_next, 1, tfirst, r.un, tnext, ntiles);
        LAUNCH(ctx, "k_ss_rows", k_ss_rows, mt.tgrid, r.table->stage, sc, r.s.refs, r.s.perm, headsB, tnext, numb, rowb, r.un, (uint32_t)r.m,
               r.stride, elem, fin, mt.ntiles);
        r.columns(fin, sc.n);
        return SDQH_OK;
    }
    uint32_t tot[3];                                                   // the level pass's counts over k_ss_heads' three levels: level 2 is the sessions
    if (int rc = level_counts(r, tcount, ntiles, ltot, 3, tot)) return rc;
    const int64_t g = (int64_t)tot[2];
    if (g >= 0xFFFFFFFFll) return fail(ctx, SDQH_ERR_UNSUPPORTED, r.me + ": more than 2^32 - 1 sessions");      // (a selection holds fewer rows: never taken)
    const int rc = r.counted(g);
    if (rc || r.ended) return rc;
    const size_t gstride = round_up((size_t)g * 8) / 8;
    uint32_t* sel = nullptr; uint8_t* gdepth = nullptr; uint64_t *sums = nullptr, *val = nullptr;
    if (!carve(ctx, r.scratch.p[4], [&](Carver& c) {
            sel = c.take<uint32_t>((size_t)g);
            gdepth = c.take<uint8_t>((size_t)g);
            sums = c.take<uint64_t>(gstride * nf);
            val = c.take<uint64_t>(gstride * nc);
            elem = c.take<uint64_t>(r.stride * nf);
            tval = c.take<uint64_t>((size_t)ntiles * nf);
        })) return r.nomem();
    if (nf) tile_fold(r, t, ag, headsB, elem, tval, tfirst, false);
    LAUNCH(ctx, "k_gs_run", k_gs_run, tgrid, ag, 2, 1, depth, (const uint32_t*)nullptr, elem, r.stride, r.un, tval, tcount + (size_t)2 * ntiles, ntiles,
           sums, gstride, gdepth, sel, tot[2]);
    if (nc) LAUNCH(ctx, "k_ss_sessions", k_ss_sessions, r.row_grid(), r.table->stage, sc, r.s.refs, r.s.perm, sel, numb, r.un, tot[2], (uint32_t)r.m, gstride, sums, val);
    r.sel = sel;
    for (r.ncols = 0; r.ncols < sc.n; ++r.ncols) r.col_src[r.ncols] = val + (size_t)r.ncols * gstride;
    return SDQH_OK;
}

// Second moments over frames (sdqh_table_window_moments): block 3 = [frame pass | component trees: S and Q per distinct measure, C per
// distinct pair | values].  The frames are found as step_excludes finds them, with nothing excluded; the image is one of COUNT ranges,
// so the frame pass stages the ends and the keys alone (no fold tree of its own: f.tstride is 0, and the component trees are this step's).
static int step_wmoments(StepRun& r) {
    DevWmos mo = r.step.wm;
    DevWranges& rg = mo.rg;
    Frames f(rg, r.n, nullptr);
    const Partitions& p = f.p;
    const uint64_t cap = f.cap;
    const size_t tstride = (size_t)(2 * cap), ntrees = (size_t)(2 * mo.nmeas + mo.npairs);
    uint64_t *tree = nullptr, *fin = nullptr;
    if (!carve(r.ctx, r.scratch.p[3], [&](Carver& c) {
            f.take(c, r.n, rg);
            tree = c.take<uint64_t>(tstride * ntrees);
            fin = c.take<uint64_t>(r.stride * (size_t)rg.n);
        })) return r.nomem();
    frame_pass(r, f, rg, nullptr, nullptr);
    LAUNCH(r.ctx, "k_wmo_stage", k_wmo_stage, p.tgrid, r.table->stage, mo, r.s.refs, r.s.perm, r.un, tstride, cap, tree, p.ntiles);
    LAUNCH(r.ctx, "k_wmo_tiles", k_wmo_tiles, p.tgrid, mo, r.un, tstride, cap, tree, p.ntiles);
    if (cap > (uint64_t)SORT_TILE) {
        LAUNCH(r.ctx, "k_wmo_upper", k_wmo_upper, (unsigned)mo.nmeas, mo, 0, tstride, cap, tree, p.ntiles);
        if (mo.npairs) LAUNCH(r.ctx, "k_wmo_upper", k_wmo_upper, (unsigned)mo.npairs, mo, 1, tstride, cap, tree, p.ntiles);
    }
    LAUNCH(r.ctx, "k_wmo_fold", k_wmo_fold, r.row_grid(), mo, p.rown, f.pend, f.vkey, f.gkey, r.un, (uint32_t)r.m, r.stride, tstride, cap, tree, fin);
    r.columns(fin, rg.n);
    return SDQH_OK;
}

// The table entry points behind their argument checks, the spine of every ordered call: select -> passes -> step -> emit -> fetch.
// who: the entry point's name in messages.
static int ordered_impl(sdqh_ctx* ctx, sdqh_table* table, const char* who, int64_t min_hits, int64_t limit, int nsort, const DevSortTerm* terms, const SortStep& step,
                        int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_n) {
    const std::string me(who);
    Scratch scratch(ctx);
    SortState s;
    if (int rc = sort_select(ctx, table, me, min_hits, nsort, terms, scratch, s)) return rc;      // (a ranks column too short: *out_n untouched)
    const int64_t n = s.n;
    const bool count_only = !out_keys && !out_payload && !out_values && !out_hits && !step.out;
    const bool all_kept = !step.filters || step.per_limit >= n;      // a rank is at most n: nothing to filter, the count is known
    StepRun r{ctx, table, me, step, s, scratch, nsort, n, limit, capacity, count_only, all_kept, out_n, (uint32_t)n, round_up((size_t)n * 8) / 8, std::min<int64_t>(limit, n)};
    // The ways out before anything is ordered.  With every row kept m = min(limit, n) already; a filtering call knows its count
    // only after the ranks, so of these it takes the first alone (and leaves *out_n untouched if a later step fails).
    if (n == 0 && (step.kind == STEP_GROUPS || step.kind == STEP_MOMENTS) && step.level_rows) std::memset(step.level_rows, 0, sizeof(int64_t) * (SDQH_SORT_MAX_KEYS + 1));
    if (n == 0) return r.done(0);                                     // nothing selected (limit >= 1: m = 0 means n = 0)
    if (all_kept && count_only) return r.done(r.m);                   // count-only call
    if (all_kept && r.m > capacity) return r.overflow(r.m);           // the needed count, nothing written
    if (!step.filters) *out_n = r.m;
    if (int rc = sort_passes(ctx, me, nsort, scratch, s)) return rc;
    // the step.  Columns nobody gave an array for are not computed (rows only; quantiles may still filter them); ranks are, as they
    // always were, even where every row is kept and no rank column is asked for
    int step_rc = SDQH_OK;
    switch (step.kind) {
        case STEP_NONE: break;
        case STEP_RANKS: step_rc = step_ranks(r); break;
        case STEP_FRAMES: if (step.out) step_rc = step_frames(r); break;
        case STEP_SLIDES: if (step.out) step_rc = step_slides(r); break;
        case STEP_RANGES: if (step.out) step_rc = step_ranges(r); break;
        case STEP_QUANTILES: if (step.out || !all_kept) step_rc = step_quantiles(r); break;
        case STEP_EXCLUDES: if (step.out) step_rc = step_excludes(r); break;
        case STEP_GROUPS: step_rc = step_groups(r); break;            // (the rows themselves are the step's: always)
        case STEP_DISTINCTS: step_rc = step_distincts(r); break;      // (likewise)
        case STEP_MOMENTS: step_rc = step_moments(r); break;          // (likewise)
        case STEP_SESSIONS: if (step.per_session || (step.out && step.ss.n)) step_rc = step_sessions(r); break;      // (per session likewise; per row its columns alone)
        case STEP_WMOMENTS: if (step.out) step_rc = step_wmoments(r); break;
    }
    if (step_rc || r.ended) return step_rc;
    const int64_t m = r.m;
    int64_t* out_rank = r.rank ? step.out : nullptr;                  // (step.out is the rank column or, with r.ncols, the columns)
    *out_n = m;
    // emit: m rows (>= 1) of the arrays asked for; none if only columns the table does not have were
    SortRows rows;
    if (int rc = sort_rows_alloc(ctx, table, me, m, out_keys != nullptr, out_payload != nullptr, out_values != nullptr, out_hits != nullptr, out_rank != nullptr, scratch, rows)) return rc;
    if (rows.narr) LAUNCH(ctx, "k_sort_emit", k_sort_emit, r.row_grid(), table->stage, s.refs, s.perm, r.sel, r.rank, r.un, (uint32_t)m, rows.o, rows.extra);
    call_end(ctx);                                                    // the call's device time ends here: the fetch is the host's
    if (r.ncols) {                                                    // the columns' first m values
        for (int a = 0; a < r.ncols; ++a)
            HIP_TRY(ctx, hipMemcpyAsync(step.out + (size_t)a * (size_t)capacity, r.col_src[a], (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (!rows.narr) if (int rc = sync_stream(ctx)) return rc;
    }
    if (rows.narr) if (int rc = sort_rows_fetch(ctx, rows, capacity, out_keys, out_payload, out_values, out_hits, out_rank)) return rc;
    if (out_values) for (int v = rows.nval; v < SDQH_TUPLE_MAX_VALUES; ++v) std::memset(out_values + (size_t)v * (size_t)capacity, 0, rows.nb);
    return SDQH_OK;
}

// the checks every entry point makes of a sort column; the term's derivation is left as it is
static bool sort_column_ok(const sdqh_table* table, int kind, int index) {
    const int nv = table->accumulate ? table->nv : 0;
    return (kind == SDQH_SORT_KEY) || (kind == SDQH_SORT_PAYLOAD && index >= 0 && index < table->npay) ||
           (kind == SDQH_SORT_VALUE && index >= 0 && index < nv) || (kind == SDQH_SORT_HITS && table->accumulate);
}
// is a column of `kind` read as doubles?  Values are, keys and hit counts are not, a payload column is what the caller says
static int column_is_f64(int kind, int is_f64) { return kind == SDQH_SORT_VALUE ? 1 : (kind == SDQH_SORT_PAYLOAD ? (is_f64 ? 1 : 0) : 0); }

// the terms of an entry point checked and marshalled; SDQH_OK or the failed call's code.  plain: sdqh_table_sorted's keys (terms
// with no derivation), named "sort key" in its one message
static int sort_terms_set(sdqh_ctx* ctx, const sdqh_table* table, const std::string& me, int nterms, const sdqh_sort_term* in, bool plain, DevSortTerm* terms) {
    std::memset(terms, 0, sizeof(DevSortTerm) * SDQH_SORT_MAX_KEYS);
    for (int i = 0; i < nterms; ++i) {
        const sdqh_sort_term& t = in[i];
        const std::string term = me + ": term " + std::to_string(i);
        if (!sort_column_ok(table, t.kind, t.index)) return fail(ctx, SDQH_ERR_INVALID, (plain ? me + ": sort key" : term) + " names a field the table does not have");
        DevSortKey& k = terms[i].sk;
        k.kind = t.kind; k.index = t.index; k.desc = t.descending ? 1 : 0;
        k.is_f64 = column_is_f64(t.kind, t.is_f64);
        if (t.div < 0 || t.mod < 0) return fail(ctx, SDQH_ERR_INVALID, term + " has a negative divisor or modulus");
        if (t.ranks && (t.ranks->dtype != SDQH_I64 || !t.ranks->data)) return fail(ctx, SDQH_ERR_INVALID, term + ": ranks must be an I64 column");
        terms[i].div = (uint64_t)t.div; terms[i].mod = (uint64_t)t.mod; terms[i].add = t.add;
        terms[i].ranks = t.ranks ? static_cast<const int64_t*>(t.ranks->data) : nullptr;
        terms[i].nranks = t.ranks ? t.ranks->nrows : 0;
        if (term_derived(terms[i]) && k.is_f64) return fail(ctx, SDQH_ERR_INVALID, term + " derives from a double");
    }
    return SDQH_OK;
}

// what every entry point checks before it looks at its terms; ok: the entry point's own conditions on its arguments
static int sort_enter(sdqh_ctx* ctx, const sdqh_table* table, const char* who, bool ok) {
    const std::string me(who);
    if (!ctx || !table || !ok) return fail(ctx, SDQH_ERR_INVALID, me + ": bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, me + ": compile-only context");
    if (table->bitmap_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, me + ": bitmap-only table");
    (void)hipSetDevice(ctx->device);
    return SDQH_OK;
}
static bool sort_args_ok(const void* terms, int nterms, int64_t limit, int64_t capacity, const int64_t* out_n) {
    return out_n && terms && nterms >= 1 && nterms <= SDQH_SORT_MAX_KEYS && limit >= 1 && capacity >= 0;
}
// ... and what every entry point with a step does before it looks at its columns: the arguments they share tested with `own` (the
// entry point's conditions on the rest), sort_enter, the terms marshalled
static int window_enter(sdqh_ctx* ctx, const sdqh_table* table, const char* who, int npartition, int nterms, const sdqh_sort_term* in, int64_t limit, int64_t capacity,
                        const int64_t* out_n, bool own, DevSortTerm* terms) {
    const bool ok = sort_args_ok(in, nterms, limit, capacity, out_n) && npartition >= 0 && npartition <= nterms && own;
    if (int rc = sort_enter(ctx, table, who, ok)) return rc;
    return sort_terms_set(ctx, table, who, nterms, in, false, terms);
}

// the measure of column i of a window entry point (noun: what it calls its columns in messages), checked and stored; desc is unused
static int measure_set(sdqh_ctx* ctx, const sdqh_table* table, const char* who, const char* noun, int i, int kind, int index, int is_f64, DevSortKey& sk) {
    const std::string col = std::string(who) + ": " + noun + " " + std::to_string(i);
    if (!sort_column_ok(table, kind, index)) return fail(ctx, SDQH_ERR_INVALID, col + " names a field the table does not have");
    if (is_f64 && (kind == SDQH_SORT_KEY || kind == SDQH_SORT_HITS)) return fail(ctx, SDQH_ERR_INVALID, col + ": keys and hit counts are integers");
    sk.kind = kind; sk.index = index; sk.is_f64 = column_is_f64(kind, is_f64);
    return SDQH_OK;
}
// how an op's elements fold.  folding_ops_only (frames: SUM / COUNT / MIN / MAX, COUNT a sum of ones); else COUNT, FIRST and LAST fold nothing
static int fold_class(int op, int is_f64, bool folding_ops_only) {
    if (op == SDQH_WAGG_MIN || op == SDQH_WAGG_MAX) return WAGG_UMAX;
    if (op != SDQH_WAGG_SUM) return folding_ops_only ? WAGG_ADD_I : WSL_NONE;
    return is_f64 ? WAGG_ADD_F : WAGG_ADD_I;
}
// The frame of a column of the entry points whose frames depend on the data (ranges, excludes, moments over frames), and what they
// demand of it behind their own tests of op, unit and flags: a VALUE frame (`value`: is there one?) takes exactly one ORDER BY term
// (read here, so: is it there?), one with arithmetic; offsets over a double term are finite; no frame ends before it begins.
struct FrameEnds { int unit, flags; int64_t lo, hi; };
static bool frame_bounds_ok(const FrameEnds* cols, int ncols, const sdqh_sort_term* in, int npartition, int nterms, bool& value) {
    value = false;
    for (int c = 0; c < ncols; ++c) value |= cols[c].unit == SDQH_WRANGE_VALUE;
    bool ok = true, vf64 = false;
    if (value) {
        ok = in && npartition >= 0 && nterms == npartition + 1 && in[npartition].ranks == nullptr;
        if (ok) vf64 = column_is_f64(in[npartition].kind, in[npartition].is_f64) != 0;
    }
    for (int c = 0; ok && c < ncols; ++c) {
        const FrameEnds& g = cols[c];
        const bool both = !(g.flags & (SDQH_WRANGE_LO_UNBOUNDED | SDQH_WRANGE_HI_UNBOUNDED));
        if (g.unit == SDQH_WRANGE_VALUE && vf64) {
            double lo, hi; std::memcpy(&lo, &g.lo, 8); std::memcpy(&hi, &g.hi, 8);
            const bool lo_ok = (g.flags & SDQH_WRANGE_LO_UNBOUNDED) || std::isfinite(lo), hi_ok = (g.flags & SDQH_WRANGE_HI_UNBOUNDED) || std::isfinite(hi);
            ok = lo_ok && hi_ok && !(both && lo > hi);
        } else ok = !(both && g.lo > g.hi);
    }
    return ok;
}
// ... and the head of their DevWranges image: the column count and the VALUE frames' ORDER BY term, its direction and type
static void frame_image(DevWranges& rg, int ncols, bool value, int npartition, const DevSortTerm* terms) {
    rg.n = ncols;
    rg.vcol = value ? npartition : -1; rg.vdesc = value ? terms[npartition].sk.desc : 0; rg.vf64 = value ? terms[npartition].sk.is_f64 : 0;
}
// a measure's place among the n distinct ones of a moments call (columns naming the same measure share it)
static int measure_slot(DevSortKey* sk, int32_t& n, const DevSortKey& m) {
    for (int k = 0; k < n; ++k) if (sk[k].kind == m.kind && sk[k].index == m.index && sk[k].is_f64 == m.is_f64) return k;
    sk[n] = m;
    return n++;
}

int sdqh_table_sorted(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int64_t limit, int nsort, const sdqh_sort_key* sort,
                      int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_n) {
    if (int rc = sort_enter(ctx, table, "table_sorted", sort_args_ok(sort, nsort, limit, capacity, out_n))) return rc;
    sdqh_sort_term in[SDQH_SORT_MAX_KEYS]; std::memset(in, 0, sizeof(in));
    for (int i = 0; i < nsort; ++i) { in[i].kind = sort[i].kind; in[i].index = sort[i].index; in[i].descending = sort[i].descending; in[i].is_f64 = sort[i].is_f64; }
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = sort_terms_set(ctx, table, "table_sorted", nsort, in, true, terms)) return rc;
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), "table_sorted", min_hits, limit, nsort, terms, sort_step(STEP_NONE, 0, nullptr), capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_sorted_by(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int64_t limit, int nterms, const sdqh_sort_term* in,
                         int64_t capacity, int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_n) {
    if (int rc = sort_enter(ctx, table, "table_sorted_by", sort_args_ok(in, nterms, limit, capacity, out_n))) return rc;
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = sort_terms_set(ctx, table, "table_sorted_by", nterms, in, false, terms)) return rc;
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), "table_sorted_by", min_hits, limit, nterms, terms, sort_step(STEP_NONE, 0, nullptr), capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                      int kind, int64_t per_limit, int64_t limit, int64_t capacity,
                      int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_rank, int64_t* out_n) {
    const char* who = "table_window";
    const bool ok = per_limit >= 1 && (kind == SDQH_WIN_ROW_NUMBER || kind == SDQH_WIN_RANK || kind == SDQH_WIN_DENSE_RANK);
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_RANKS, npartition, out_rank);
    st.filters = true; st.rank_kind = kind; st.per_limit = per_limit;
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window_agg(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                          int naggs, const sdqh_window_agg* aggs, int64_t limit, int64_t capacity,
                          int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_aggs, int64_t* out_n) {
    const char* who = "table_window_agg";
    bool ok = aggs && naggs >= 1 && naggs <= SDQH_WAGG_MAX_AGGS;
    for (int a = 0; ok && a < naggs; ++a)
        ok = aggs[a].op >= SDQH_WAGG_SUM && aggs[a].op <= SDQH_WAGG_MAX && aggs[a].frame >= SDQH_FRAME_ROWS && aggs[a].frame <= SDQH_FRAME_PARTITION;
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_FRAMES, npartition, out_aggs);
    st.aggs.n = naggs;
    for (int a = 0; a < naggs; ++a) {
        const sdqh_window_agg& g = aggs[a];
        DevWagg& d = st.aggs.a[a];
        d.op = g.op; d.frame = g.frame;
        if (g.op != SDQH_WAGG_COUNT)                                  // (COUNT ignores its measure)
            if (int rc = measure_set(ctx, table, who, "aggregate", a, g.kind, g.index, g.is_f64, d.sk)) return rc;
        d.cls = fold_class(g.op, d.sk.is_f64, true);
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window_slide(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                            int nslides, const sdqh_window_slide* slides, int64_t limit, int64_t capacity,
                            int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_aggs, int64_t* out_n) {
    const char* who = "table_window_slide";
    bool ok = slides && nslides >= 1 && nslides <= SDQH_WSLIDE_MAX_AGGS;
    for (int a = 0; ok && a < nslides; ++a) ok = slides[a].op >= SDQH_WAGG_SUM && slides[a].op <= SDQH_WSLIDE_LAST && slides[a].lo <= slides[a].hi;
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_SLIDES, npartition, out_aggs);
    st.sl.n = nslides;
    for (int a = 0; a < nslides; ++a) {
        const sdqh_window_slide& g = slides[a];
        DevWslide& d = st.sl.a[a];
        d.g.op = g.op; d.empty = (uint64_t)g.empty; d.w = 1u; d.lo = g.lo; d.hi = g.hi;
        if (g.op != SDQH_WAGG_COUNT)                                  // (COUNT ignores its measure)
            if (int rc = measure_set(ctx, table, who, "slide", a, g.kind, g.index, g.is_f64, d.g.sk)) return rc;
        d.g.cls = fold_class(g.op, d.g.sk.is_f64, false);
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window_range(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                            int nranges, const sdqh_window_range* ranges, int64_t limit, int64_t capacity,
                            int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_aggs, int64_t* out_n) {
    const char* who = "table_window_range";
    bool ok = ranges && nranges >= 1 && nranges <= SDQH_WRANGE_MAX_AGGS, value = false;
    FrameEnds ends[SDQH_WRANGE_MAX_AGGS];
    for (int a = 0; ok && a < nranges; ++a) {
        const sdqh_window_range& g = ranges[a];
        ok = g.op >= SDQH_WAGG_SUM && g.op <= SDQH_WSLIDE_LAST && (g.unit == SDQH_WRANGE_VALUE || g.unit == SDQH_WRANGE_GROUPS) &&
             !(g.flags & ~(SDQH_WRANGE_LO_UNBOUNDED | SDQH_WRANGE_HI_UNBOUNDED));
        ends[a] = FrameEnds{g.unit, g.flags, g.lo, g.hi};
    }
    ok = ok && frame_bounds_ok(ends, nranges, in, npartition, nterms, value);
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_RANGES, npartition, out_aggs);
    frame_image(st.rg, nranges, value, npartition, terms);
    for (int a = 0; a < nranges; ++a) {
        const sdqh_window_range& g = ranges[a];
        DevWrange& d = st.rg.a[a];
        d.g.op = g.op; d.empty = (uint64_t)g.empty; d.unit = g.unit; d.flags = g.flags; d.lo = g.lo; d.hi = g.hi;
        if (g.op != SDQH_WAGG_COUNT)                                  // (COUNT ignores its measure)
            if (int rc = measure_set(ctx, table, who, "range", a, g.kind, g.index, g.is_f64, d.g.sk)) return rc;
        d.g.cls = fold_class(g.op, d.g.sk.is_f64, false);
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window_quantile(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                               int ncols, const sdqh_window_quantile* cols, int64_t per_limit, int64_t limit, int64_t capacity,
                               int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_cols, int64_t* out_n) {
    const char* who = "table_window_quantile";
    bool ok = per_limit >= 1 && cols && ncols >= 1 && ncols <= SDQH_WQUANT_MAX_COLS;
    for (int c = 0; ok && c < ncols; ++c) {
        const sdqh_window_quantile& g = cols[c];
        ok = g.fn >= SDQH_WQ_NTILE && g.fn <= SDQH_WQ_PERCENTILE_CONT;
        if (g.fn == SDQH_WQ_NTILE) ok = ok && g.arg >= 1;
        if (g.fn == SDQH_WQ_NTH) ok = ok && g.arg != 0;
        if (g.fn == SDQH_WQ_PERCENTILE_DISC || g.fn == SDQH_WQ_PERCENTILE_CONT) ok = ok && g.p >= 0.0 && g.p <= 1.0;      // (a NaN fails both)
    }
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_QUANTILES, npartition, out_cols);
    st.filters = true; st.per_limit = per_limit;                      // (on the row number, as sort_step leaves it)
    DevWquants& q = st.q;
    q.n = ncols;
    for (int c = 0; c < ncols; ++c) {
        const sdqh_window_quantile& g = cols[c];
        DevWquant& d = q.a[c];
        d.fn = g.fn; d.arg = g.arg; d.p = g.p; d.empty = (uint64_t)g.empty; d.slot = -1;
        if (g.fn >= SDQH_WQ_NTH) {                                    // (the others have no measure)
            DevSortKey sk; std::memset(&sk, 0, sizeof(sk));
            if (int rc = measure_set(ctx, table, who, "column", c, g.kind, g.index, g.is_f64, sk)) return rc;
            d.is_f64 = sk.is_f64;
            int k = 0;                                                // the measure's element array: shared with an earlier column of the same measure
            while (k < q.nslots && !(q.slot[k].kind == sk.kind && q.slot[k].index == sk.index && q.slot[k].is_f64 == sk.is_f64)) ++k;
            if (k == q.nslots) q.slot[q.nslots++] = sk;
            d.slot = k;
        }
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window_exclude(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                              int ncols, const sdqh_window_exclude* cols, int64_t limit, int64_t capacity,
                              int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_cols, int64_t* out_n) {
    const char* who = "table_window_exclude";
    bool ok = cols && ncols >= 1 && ncols <= SDQH_WEX_MAX_COLS, value = false;
    FrameEnds ends[SDQH_WEX_MAX_COLS];
    for (int c = 0; ok && c < ncols; ++c) {
        const sdqh_window_exclude& g = cols[c];
        ok = g.op >= SDQH_WAGG_SUM && g.op <= SDQH_WEX_AVG && g.unit >= SDQH_WRANGE_VALUE && g.unit <= SDQH_WEX_ROWS &&
             g.exclude >= SDQH_WEX_NO_OTHERS && g.exclude <= SDQH_WEX_TIES && g._pad == 0 && !(g.flags & ~(SDQH_WRANGE_LO_UNBOUNDED | SDQH_WRANGE_HI_UNBOUNDED));
        ends[c] = FrameEnds{g.unit, g.flags, g.lo, g.hi};
    }
    ok = ok && frame_bounds_ok(ends, ncols, in, npartition, nterms, value);
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_EXCLUDES, npartition, out_cols);
    DevWranges& rg = st.ex.rg;
    frame_image(rg, ncols, value, npartition, terms);
    for (int c = 0; c < ncols; ++c) {
        const sdqh_window_exclude& g = cols[c];
        DevWrange& d = rg.a[c];
        const int op = g.op == SDQH_WEX_AVG ? SDQH_WAGG_SUM : g.op;      // an AVG is staged and folded as the SUM it divides
        d.g.op = op; d.empty = (uint64_t)g.empty; d.unit = g.unit; d.flags = g.flags; d.lo = g.lo; d.hi = g.hi;
        st.ex.exclude[c] = g.exclude; st.ex.avg[c] = g.op == SDQH_WEX_AVG ? 1 : 0;
        if (op != SDQH_WAGG_COUNT)                                    // (COUNT ignores its measure)
            if (int rc = measure_set(ctx, table, who, "column", c, g.kind, g.index, g.is_f64, d.g.sk)) return rc;
        d.g.cls = fold_class(op, d.g.sk.is_f64, false);
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_grouping_sets(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int nterms, const sdqh_sort_term* in, uint32_t levels,
                             int naggs, const sdqh_group_agg* aggs, int64_t limit, int64_t capacity,
                             int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_aggs, int64_t* out_level_rows, int64_t* out_n) {
    const char* who = "table_grouping_sets";
    bool ok = naggs >= 0 && naggs <= SDQH_GS_MAX_AGGS && (aggs || naggs == 0) && levels != 0u && nterms >= 1 && nterms <= SDQH_SORT_MAX_KEYS && !(levels >> (nterms + 1));
    for (int a = 0; ok && a < naggs; ++a) ok = (aggs[a].op >= SDQH_WAGG_SUM && aggs[a].op <= SDQH_WAGG_MAX) || aggs[a].op == SDQH_WEX_AVG;
    SortStep st = sort_step(STEP_GROUPS, 0, naggs ? out_aggs : nullptr);
    st.filters = true; st.per_limit = 0;                              // no row is kept for its rank: the count is the groups', known behind the level pass
    st.levels = levels; st.level_rows = out_level_rows;
    st.aggs.n = ok ? naggs : 0;
    // the measures are checked in front of window_enter: a measure the table lacks is SDQH_ERR_INVALID on a bitmap-only table and in a
    // compile-only context too (the header: every argument error comes before SDQH_ERR_UNSUPPORTED)
    for (int a = 0; ctx && table && ok && a < naggs; ++a) {
        const sdqh_group_agg& g = aggs[a];
        DevWagg& d = st.aggs.a[a];
        d.op = g.op == SDQH_WEX_AVG ? SDQH_WAGG_SUM : g.op;             // an AVG is folded as the SUM it divides
        d.frame = SDQH_FRAME_ROWS;
        if (d.op != SDQH_WAGG_COUNT)                                  // (COUNT ignores its measure)
            if (int rc = measure_set(ctx, table, who, "aggregate", a, g.kind, g.index, g.is_f64, d.sk)) return rc;
        d.cls = fold_class(d.op, d.sk.is_f64, true);
        st.avg.avg[a] = g.op == SDQH_WEX_AVG ? 1 : 0; st.avg.is_f64[a] = d.sk.is_f64;
    }
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, 0, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_group_distinct(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int nterms, const sdqh_sort_term* in, int ngroup,
                              int naggs, const sdqh_distinct_agg* aggs, int64_t limit, int64_t capacity,
                              int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_aggs, int64_t* out_n) {
    const char* who = "table_group_distinct";
    bool ok = naggs >= 1 && naggs <= SDQH_GD_MAX_AGGS && aggs && nterms >= 1 && nterms <= SDQH_SORT_MAX_KEYS && ngroup >= 0 && ngroup < nterms;
    for (int a = 0; ok && a < naggs; ++a) ok = aggs[a].op >= SDQH_GD_COUNT_DISTINCT && aggs[a].op <= SDQH_GD_COUNT;
    SortStep st = sort_step(STEP_DISTINCTS, 0, out_aggs);
    st.filters = true; st.per_limit = 0;                              // no row is kept for its rank: the count is the groups', known behind the depth pass
    st.ngroup = ngroup;
    st.aggs.n = st.gd.n = ok ? naggs : 0;
    // the measures in front of window_enter, as sdqh_table_grouping_sets checks them: every argument error comes before SDQH_ERR_UNSUPPORTED
    for (int a = 0; ctx && table && ok && a < naggs; ++a) {
        const sdqh_distinct_agg& g = aggs[a];
        DevWagg& d = st.aggs.a[a];
        st.gd.op[a] = g.op;
        const bool measured = g.op == SDQH_GD_SUM_DISTINCT || g.op == SDQH_GD_AVG_DISTINCT || g.op == SDQH_GD_MODE;      // (the others ignore their measure)
        if (measured)
            if (int rc = measure_set(ctx, table, who, "aggregate", a, g.kind, g.index, g.is_f64, st.gd.sk[a])) return rc;
        // the upper stage's fold: sums of ones, lengths and measures; the MODE word under WAGG_UMAX as a MAX over int64
        const bool mode = g.op == SDQH_GD_MODE || g.op == SDQH_GD_MODE_COUNT;
        const bool sums = g.op == SDQH_GD_SUM_DISTINCT || g.op == SDQH_GD_AVG_DISTINCT;
        d.op = mode ? SDQH_WAGG_MAX : (sums ? SDQH_WAGG_SUM : SDQH_WAGG_COUNT);
        d.frame = SDQH_FRAME_ROWS;
        d.sk = st.gd.sk[a];
        if (!sums) d.sk.is_f64 = 0;
        d.cls = fold_class(d.op, d.sk.is_f64, true);
    }
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, 0, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_group_moments(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int nterms, const sdqh_sort_term* in, uint32_t levels,
                             int naggs, const sdqh_moment_agg* aggs, int64_t limit, int64_t capacity,
                             int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_aggs, int64_t* out_level_rows, int64_t* out_n) {
    const char* who = "table_group_moments";
    bool ok = naggs >= 1 && naggs <= SDQH_GM_MAX_AGGS && aggs && levels != 0u && nterms >= 1 && nterms <= SDQH_SORT_MAX_KEYS && !(levels >> (nterms + 1));
    for (int a = 0; ok && a < naggs; ++a) ok = aggs[a].op >= SDQH_GM_VAR_POP && aggs[a].op <= SDQH_GM_REGR_INTERCEPT;
    SortStep st = sort_step(STEP_MOMENTS, 0, out_aggs);
    st.filters = true; st.per_limit = 0;                              // no row is kept for its rank: the count is the groups', known behind the level pass
    st.levels = levels; st.level_rows = out_level_rows;
    DevMoAggs& mo = st.mo;
    mo.n = ok ? naggs : 0;
    // a product's column among pass 2's (a measure's among the distinct ones: measure_slot)
    auto product = [&](int i, int j) {
        if (i > j) std::swap(i, j);
        for (int c = 0; c < mo.ncen; ++c) if (mo.ci[c] == i && mo.cj[c] == j) return c;
        mo.ci[mo.ncen] = i; mo.cj[mo.ncen] = j;
        return mo.ncen++;
    };
    // the measures in front of window_enter, as sdqh_table_grouping_sets checks them: every argument error comes before SDQH_ERR_UNSUPPORTED
    for (int a = 0; ctx && table && ok && a < naggs; ++a) {
        const sdqh_moment_agg& g = aggs[a];
        const bool two = g.op >= SDQH_GM_COVAR_POP;                   // (VAR_* and STDDEV_* ignore the second measure)
        DevSortKey y, x; std::memset(&y, 0, sizeof(y)); std::memset(&x, 0, sizeof(x));
        if (int rc = measure_set(ctx, table, who, "aggregate", a, g.kind, g.index, g.is_f64, y)) return rc;
        if (two) if (int rc = measure_set(ctx, table, who, "aggregate", a, g.kind2, g.index2, g.is_f64_2, x)) return rc;
        mo.op[a] = g.op;
        mo.my[a] = measure_slot(mo.sk, mo.nmeas, y); mo.mx[a] = two ? measure_slot(mo.sk, mo.nmeas, x) : mo.my[a];
        mo.qy[a] = mo.qx[a] = mo.cc[a] = -1;
        if (!two) mo.qy[a] = product(mo.my[a], mo.my[a]);
        else {
            mo.cc[a] = product(mo.my[a], mo.mx[a]);
            if (g.op >= SDQH_GM_CORR) mo.qx[a] = product(mo.mx[a], mo.mx[a]);
            if (g.op == SDQH_GM_CORR) mo.qy[a] = product(mo.my[a], mo.my[a]);
        }
    }
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, 0, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_window_moments(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                              int ncols, const sdqh_window_moment* cols, int64_t limit, int64_t capacity,
                              int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_cols, int64_t* out_n) {
    const char* who = "table_window_moments";
    bool ok = cols && ncols >= 1 && ncols <= SDQH_WM_MAX_COLS, value = false;
    FrameEnds ends[SDQH_WM_MAX_COLS];
    for (int c = 0; ok && c < ncols; ++c) {
        const sdqh_window_moment& g = cols[c];
        ok = g.op >= SDQH_GM_VAR_POP && g.op <= SDQH_GM_REGR_INTERCEPT && g.unit >= SDQH_WRANGE_VALUE && g.unit <= SDQH_WEX_ROWS && g._pad == 0 &&
             !(g.flags & ~(SDQH_WRANGE_LO_UNBOUNDED | SDQH_WRANGE_HI_UNBOUNDED));
        ends[c] = FrameEnds{g.unit, g.flags, g.lo, g.hi};
    }
    ok = ok && frame_bounds_ok(ends, ncols, in, npartition, nterms, value);
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_WMOMENTS, npartition, out_cols);
    DevWmos& mo = st.wm;
    DevWranges& rg = mo.rg;
    frame_image(rg, ncols, value, npartition, terms);
    // a pair's C tree among the pairs (a measure's trees among the distinct ones: measure_slot — columns naming the same measure share them)
    auto pair_of = [&](int i, int j) {
        if (i == j) return -1;                                        // C of a measure with itself is its Q
        if (i > j) std::swap(i, j);
        for (int c = 0; c < mo.npairs; ++c) if (mo.pi[c] == i && mo.pj[c] == j) return c;
        mo.pi[mo.npairs] = i; mo.pj[mo.npairs] = j;
        return mo.npairs++;
    };
    for (int c = 0; c < ncols; ++c) {
        const sdqh_window_moment& g = cols[c];
        DevWrange& d = rg.a[c];
        d.g.op = SDQH_WAGG_COUNT; d.g.cls = WSL_NONE;                 // the image: k_wrg_stage stages no element for it
        d.unit = g.unit; d.flags = g.flags; d.lo = g.lo; d.hi = g.hi;
        const bool two = g.op >= SDQH_GM_COVAR_POP;                   // (VAR_* and STDDEV_* ignore the second measure)
        DevSortKey y, x; std::memset(&y, 0, sizeof(y)); std::memset(&x, 0, sizeof(x));
        if (int rc = measure_set(ctx, table, who, "column", c, g.kind, g.index, g.is_f64, y)) return rc;
        if (two) if (int rc = measure_set(ctx, table, who, "column", c, g.kind2, g.index2, g.is_f64_2, x)) return rc;
        DevWmoCol& a = mo.a[c];
        a.op = g.op; a.my = measure_slot(mo.sk, mo.nmeas, y); a.mx = two ? measure_slot(mo.sk, mo.nmeas, x) : a.my;
        a.pair = two ? pair_of(a.my, a.mx) : -1;
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

int sdqh_table_sessions(sdqh_ctx* ctx, const sdqh_table* table, int64_t min_hits, int npartition, int nterms, const sdqh_sort_term* in,
                        const sdqh_session_rule* rule, int per_session, int ncols, const sdqh_session_col* cols, int64_t limit, int64_t capacity,
                        int64_t* out_keys, int64_t* out_payload, double* out_values, int64_t* out_hits, int64_t* out_cols, int64_t* out_n) {
    const char* who = "table_sessions";
    bool ok = rule && (rule->rule == SDQH_SS_GAP || rule->rule == SDQH_SS_CHANGE) && (per_session == 0 || per_session == 1) &&
              ncols >= 0 && ncols <= SDQH_SS_MAX_COLS && (cols || ncols == 0);
    for (int c = 0; ok && c < ncols; ++c) ok = cols[c].op >= SDQH_WAGG_SUM && cols[c].op <= SDQH_SS_ROW && !(per_session && cols[c].op == SDQH_SS_ROW);
    const bool gap = ok && rule->rule == SDQH_SS_GAP;
    if (gap) {                                                        // the gap term (read here, so: is it there?), one with arithmetic, and a gap of its type
        ok = in && npartition >= 0 && nterms >= npartition + 1 && nterms <= SDQH_SORT_MAX_KEYS && in[npartition].ranks == nullptr;
        if (ok && column_is_f64(in[npartition].kind, in[npartition].is_f64)) {
            double d; std::memcpy(&d, &rule->gap, 8);
            ok = std::isfinite(d) && d >= 0.0;
        } else if (ok) ok = rule->gap >= 0;
    }
    DevSortTerm terms[SDQH_SORT_MAX_KEYS];
    if (int rc = window_enter(ctx, table, who, npartition, nterms, in, limit, capacity, out_n, ok, terms)) return rc;
    SortStep st = sort_step(STEP_SESSIONS, npartition, out_cols);
    st.per_session = per_session;
    if (per_session) { st.filters = true; st.per_limit = 0; }         // no row is kept for its rank: the count is the sessions', known behind the boundary pass
    st.ssr.rule = rule->rule; st.ssr.gap = rule->gap;
    if (gap) st.ssr.tm = terms[npartition];
    else if (int rc = measure_set(ctx, table, who, "marker", 0, rule->kind, rule->index, rule->is_f64, st.ssr.tm.sk)) return rc;
    st.ss.n = ncols;
    for (int c = 0; c < ncols; ++c) {
        const sdqh_session_col& g = cols[c];
        st.ss.op[c] = g.op; st.ss.slot[c] = -1;
        if (g.op == SDQH_WAGG_COUNT || g.op == SDQH_SS_NUMBER || g.op == SDQH_SS_ROW) continue;      // (they ignore their measure)
        if (int rc = measure_set(ctx, table, who, "column", c, g.kind, g.index, g.is_f64, st.ss.sk[c])) return rc;
    }
    for (int c = 0; c < ncols; ++c) {                                 // the folds among the columns (an AVG as the SUM it divides), as the frames' passes take them
        const int op = st.ss.op[c] == SDQH_WEX_AVG ? SDQH_WAGG_SUM : st.ss.op[c];
        if (op > SDQH_WAGG_MAX) continue;
        DevWagg& d = st.aggs.a[st.aggs.n];
        d.op = op; d.frame = SDQH_FRAME_ROWS; d.sk = st.ss.sk[c];
        d.cls = fold_class(op, d.sk.is_f64, true);
        st.ss.slot[c] = st.aggs.n++;
    }
    return ordered_impl(ctx, const_cast<sdqh_table*>(table), who, min_hits, limit, nterms, terms, st, capacity, out_keys, out_payload, out_values, out_hits, out_n);
}

// what the tests size their cases from: one tile for every family; narrow (the two exports that have it): the largest frame width
// a kernel walks row by row — none does (slides fold two blocks, ranges make two searches and a tree query)
static int window_tile_rows(sdqh_ctx* ctx, const char* who, int64_t* tile_rows, bool has_narrow, int64_t* narrow_max_width) {
    if (!ctx || !tile_rows || (has_narrow && !narrow_max_width)) return fail(ctx, SDQH_ERR_INVALID, std::string(who) + ": bad arguments");
    *tile_rows = SORT_TILE;
    if (has_narrow) *narrow_max_width = 0;
    return SDQH_OK;
}
int sdqh_window_moments_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "window_moments_geometry", tile_rows, false, nullptr); }
int sdqh_sessions_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "sessions_geometry", tile_rows, false, nullptr); }
int sdqh_group_moments_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "group_moments_geometry", tile_rows, false, nullptr); }
int sdqh_group_distinct_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "group_distinct_geometry", tile_rows, false, nullptr); }
int sdqh_grouping_sets_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "grouping_sets_geometry", tile_rows, false, nullptr); }
int sdqh_window_exclude_geometry(sdqh_ctx* ctx, int64_t* tile_rows, int64_t* narrow_max_width) { return window_tile_rows(ctx, "window_exclude_geometry", tile_rows, true, narrow_max_width); }
int sdqh_window_quantile_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "window_quantile_geometry", tile_rows, false, nullptr); }
int sdqh_window_range_geometry(sdqh_ctx* ctx, int64_t* tile_rows, int64_t* narrow_max_width) { return window_tile_rows(ctx, "window_range_geometry", tile_rows, true, narrow_max_width); }
int sdqh_window_slide_geometry(sdqh_ctx* ctx, int64_t* tile_rows, int64_t* narrow_max_width) { return window_tile_rows(ctx, "window_slide_geometry", tile_rows, true, narrow_max_width); }
int sdqh_window_agg_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "window_agg_geometry", tile_rows, false, nullptr); }
int sdqh_window_geometry(sdqh_ctx* ctx, int64_t* tile_rows) { return window_tile_rows(ctx, "window_geometry", tile_rows, false, nullptr); }

int sdqh_text_ranks(sdqh_ctx* ctx, const sdqh_column* text, int64_t nrows, sdqh_column** out_ranks, int64_t* out_distinct) {
    if (!ctx || !text || !out_ranks || !out_distinct || nrows < 0) return fail(ctx, SDQH_ERR_INVALID, "text_ranks: bad arguments");
    if (ctx->compile_only) return fail(ctx, SDQH_ERR_UNSUPPORTED, "text_ranks: compile-only context");
    if (text->dtype != SDQH_STR || text->width < 1 || text->nrows < nrows || (nrows && !text->data)) return fail(ctx, SDQH_ERR_INVALID, "text_ranks: needs a STR column covering nrows");
    if (text->width > TEXT_MAX_WIDTH) return fail(ctx, SDQH_ERR_UNSUPPORTED, "text_ranks: more than " + std::to_string(TEXT_MAX_WIDTH) + " code units per row");
    if (nrows > 0xFFFFFFF0ll) return fail(ctx, SDQH_ERR_UNSUPPORTED, "text_ranks: row references are 32 bits");
    (void)hipSetDevice(ctx->device);
    sdqh_column* rk = nullptr;
    if (int rc = sdqh_column_alloc(ctx, nrows, SDQH_I64, 0, &rk)) return rc;
    *out_distinct = 0;
    if (nrows == 0) { *out_ranks = rk; return SDQH_OK; }
    struct Drop { sdqh_ctx* ctx; sdqh_column* c; ~Drop() { if (c) sdqh_column_free(ctx, c); } } drop{ctx, rk};      // on every way out but the last
    call_begin(ctx);
    Scratch scratch(ctx);
    const int width = text->width;
    const uint32_t* units = static_cast<const uint32_t*>(text->data);
    const uint32_t un = (uint32_t)nrows;
    const Tiles t(nrows);
    const uint32_t ntiles = t.ntiles;
    // one block: [masks | info | tile heads | keys | permutation x 2 | digit counts per tile | digit totals]
    uint32_t *masks = nullptr, *tile_heads = nullptr, *pa = nullptr, *pb = nullptr, *hist = nullptr, *bin_total = nullptr;
    unsigned long long* info = nullptr;
    uint64_t* key = nullptr;
    if (!carve(ctx, scratch.p[0], [&](Carver& c) {
            masks = c.take<uint32_t>(2 * TEXT_MAX_WIDTH);
            info = c.take<unsigned long long>(SORT_INFO);
            tile_heads = c.take<uint32_t>(ntiles);
            key = c.take<uint64_t>((size_t)nrows);
            pa = c.take<uint32_t>((size_t)nrows);
            pb = c.take<uint32_t>((size_t)nrows);
            hist = c.take<uint32_t>((size_t)ntiles * 256);
            bin_total = c.take<uint32_t>(256);
        })) return fail(ctx, SDQH_ERR_NOMEM, "text_ranks: out of device memory");
    // (a) which bytes vary at all
    HIP_TRY(ctx, hipMemsetAsync(masks, 0xFF, TEXT_MAX_WIDTH * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(masks + TEXT_MAX_WIDTH, 0, TEXT_MAX_WIDTH * 4, ctx->stream));
    const int rows_per = TPB / width;
    const unsigned mgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nrows + rows_per - 1) / rows_per, (int64_t)ctx->num_cu * 8));
    LAUNCH(ctx, "k_text_masks", k_text_masks, mgrid, units, (uint64_t)nrows, width, masks);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->result_host, masks, 2 * TEXT_MAX_WIDTH * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
    uint32_t hm[2 * TEXT_MAX_WIDTH];
    std::memcpy(hm, ctx->result_host, sizeof(hm));
    uint16_t vunit[TEXT_MAX_WIDTH * 4]; uint8_t vshift[TEXT_MAX_WIDTH * 4]; int nvb = 0;
    for (int p = 0; p < width; ++p) {
        const uint32_t vary = hm[TEXT_MAX_WIDTH + p] & ~hm[p];
        for (int shift = 24; shift >= 0; shift -= 8) if ((vary >> shift) & 255u) { vunit[nvb] = (uint16_t)p; vshift[nvb] = (uint8_t)shift; ++nvb; }
    }
    // (b) + (c): last word first; within a word the last byte (the lowest digit) first
    const uint32_t* perm = nullptr;
    const unsigned pgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nrows + TPB - 1) / TPB, (int64_t)ctx->num_cu * 8));
    const int nwords = (nvb + TEXT_WORD_BYTES - 1) / TEXT_WORD_BYTES;
    if (nrows > 1) for (int w = nwords - 1; w >= 0; --w) {
        DevTextWord tw; std::memset(&tw, 0, sizeof(tw));
        tw.nbytes = std::min(TEXT_WORD_BYTES, nvb - w * TEXT_WORD_BYTES);
        for (int b = 0; b < tw.nbytes; ++b) { tw.unit[b] = vunit[w * TEXT_WORD_BYTES + b]; tw.shift[b] = vshift[w * TEXT_WORD_BYTES + b]; }
        LAUNCH(ctx, "k_text_pack", k_text_pack, pgrid, units, (uint64_t)nrows, width, tw, key);
        for (int b = tw.nbytes - 1; b >= 0; --b) {
            radix_pass(ctx, key, perm, un, 56 - 8 * b, hist, bin_total, t, pa);
            perm = pa; std::swap(pa, pb);
        }
    }
    // (d) dense ranks
    LAUNCH(ctx, "k_rank_count", k_rank_count, t.tgrid, units, width, perm, un, tile_heads, ntiles);
    LAUNCH(ctx, "k_sort_scan", k_sort_scan, 1, tile_heads, (int)ntiles, info);
    LAUNCH(ctx, "k_rank_place", k_rank_place, t.tgrid, units, width, perm, un, tile_heads, ntiles, static_cast<int64_t*>(rk->data));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->result_host, info, 8, hipMemcpyDeviceToHost, ctx->stream));
    call_end(ctx);
    if (int rc = sync_stream(ctx)) return rc;
    unsigned long long heads;
    std::memcpy(&heads, ctx->result_host, 8);
    *out_distinct = (int64_t)heads + 1;
    *out_ranks = rk; drop.c = nullptr;
    return SDQH_OK;
}

}  // extern "C"
