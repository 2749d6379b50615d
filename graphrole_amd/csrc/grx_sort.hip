// grx_sort.hip -- the library's 64-bit LSD radix sort: batched fp64 columns, raw u64 keys, and one fp64 column with
// the permutation that sorts it.
//
// Eight passes of eight bits, least significant first; each pass is
//   tile_count_kernel : digit histogram of every 4096-key tile                       (HBM bound, wave ballots)
//   scan_rows_kernel  : per digit, exclusive scan of the tile counts + the digit total (tiny)
//   scatter_kernel    : stable placement; a tile's keys are put in digit order in LDS first, so that a digit's
//                       run leaves as one contiguous store
// Pass 0 turns fp64 values into order keys (f64_to_key) and pass 7 turns them back; raw u64 keys skip both.  The
// keys ping-pong between a scratch buffer and the output, which therefore holds the result after the eighth pass.
// Callers: grx_sort_columns (ABI), the quantiser (grx_quant.hip), the 1-D k-means (grx_kmeans.hip: pairs) and
// the graph ingest (grx_ingest.hip: u64).  All integer work: the result is a bit-exact function of the input.
#include "grx_sort.h"

namespace {

// Load the ITEMS keys of this thread.  Wave w of the tile owns the contiguous slice
// [w*64*ITEMS, (w+1)*64*ITEMS); item i of lane l is element i*64 + l of that slice, so
// (wave, item, lane) order == memory order (needed for LSD stability) and loads coalesce.
// The loads are issued back to back from clamped addresses and converted / masked afterwards, behind a scheduling
// barrier: a load inside `if (idx < n)` -- or a conversion next to it -- makes hipcc wait for every load before it
// issues the next one (s_waitcnt vmcnt(0) sixteen times per thread; found in the ISA).
template <bool from_f64>
__device__ __forceinline__ void load_keys(const void *__restrict__ src, int64_t n, int64_t tile_base,
                                          uint64_t (&keys)[SORT_ITEMS], uint32_t &valid_mask)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = tile_base + (int64_t)wave * 64 * SORT_ITEMS + lane;
    const int64_t last = n > 0 ? n - 1 : 0;
    uint64_t raw[SORT_ITEMS];
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        const int64_t idx = base + (int64_t)i * 64;
        raw[i] = reinterpret_cast<const uint64_t *>(src)[idx < n ? idx : last];
    }
    __builtin_amdgcn_sched_barrier(0);
    valid_mask = 0;
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        const bool ok = base + (int64_t)i * 64 < n;
        valid_mask |= ok ? 1u << i : 0u;
        const uint64_t k = from_f64 ? f64_to_key(__longlong_as_double((long long)raw[i])) : raw[i];
        keys[i] = ok ? k : 0xFFFFFFFFFFFFFFFFull;
    }
}

// hist layout per column: [RADIX][ntiles] (digit-major) so one flat exclusive scan yields the
// global output offset of (digit, tile).
template <bool FROM_F64>
__global__ __launch_bounds__(SORT_THREADS) void tile_count_kernel(
    const void *__restrict__ src, int64_t src_ld, int64_t n, int shift, int ntiles,
    uint32_t *__restrict__ hist)
{
    __shared__ uint32_t cnt[RADIX];
    const int col = blockIdx.y, tile = blockIdx.x;
    const char *csrc = reinterpret_cast<const char *>(src) + (size_t)col * src_ld * 8;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    uint64_t keys[SORT_ITEMS];
    uint32_t vm;
    load_keys<FROM_F64>(csrc, n, (int64_t)tile * SORT_TILE, keys, vm);
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        // same-address LDS atomics serialise lane by lane; columns of small integers (degrees, their
        // sums) have whole wavefronts agreeing on most digits: count those with one atomic
        const bool valid = (vm >> i) & 1u;
        const uint32_t d = (uint32_t)(keys[i] >> shift) & 0xFF;
        const uint64_t active = __ballot(valid);
        if (active == 0) continue;                              // uniform over the wave
        const int leader = __ffsll((long long)active) - 1;
        const uint32_t d0 = __shfl(d, leader, 64);
        if (__ballot(valid && d != d0) == 0) {
            if (lane == leader) atomicAdd(&cnt[d0], (uint32_t)__popcll(active));
        } else if (valid) {
            atomicAdd(&cnt[d], 1u);
        }
    }
    __syncthreads();
    hist[((size_t)col * RADIX + threadIdx.x) * ntiles + tile] = cnt[threadIdx.x];
}

// scan_rows_kernel: per (column, digit) exclusive scan of the digit-major counter table
// hist[RADIX][ntiles] across tiles, digit total -> tot.  scatter_kernel scans the 256 digit totals
// itself (digit base) and adds it to the per-tile offset.
__global__ __launch_bounds__(64) void scan_rows_kernel(uint32_t *__restrict__ hist, int ntiles,
                                                       uint32_t *__restrict__ tot)
{
    const int d = blockIdx.x, col = blockIdx.y, lane = threadIdx.x;
    uint32_t *row = hist + ((size_t)col * RADIX + d) * ntiles;
    uint32_t carry = 0;
    for (int t0 = 0; t0 < ntiles; t0 += 64 * 4) {
        uint32_t x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                       // issue the loads together
            const int t = t0 + j * 64 + lane;
            x[j] = (t < ntiles) ? row[t] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + j * 64 + lane;
            uint32_t inc = x[j];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(inc, off, 64);
                if (lane >= off) inc += y;
            }
            if (t < ntiles) row[t] = carry + inc - x[j];
            carry += __shfl(inc, 63, 64);
        }
    }
    if (lane == 0) tot[(size_t)col * RADIX + d] = carry;
}

// PAIRS: a 32-bit payload travels with every key (grx_kmeans.hip: the index of the value, so that the sort also
// yields the permutation).  Single column; pay_src == nullptr: the payload is the position (pass 0).  Stable:
// equal keys keep their index order.
template <bool FROM_F64, bool TO_F64, bool PAIRS>
__global__ __launch_bounds__(SORT_THREADS) void scatter_kernel(
    const void *__restrict__ src, int64_t src_ld, void *__restrict__ dst, int64_t dst_ld,
    const uint32_t *__restrict__ pay_src, uint32_t *__restrict__ pay_dst, int64_t n,
    int shift, int ntiles, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ digit_tot)
{
    __shared__ uint32_t cnt[4][RADIX];
    __shared__ uint32_t gdelta[RADIX];
    __shared__ uint32_t wsum[8];
    __shared__ uint64_t stage[SORT_TILE];
    __shared__ uint32_t stage_pay[PAIRS ? SORT_TILE : 1];       // never touched, and so not allocated, without PAIRS
    const int col = blockIdx.y, tile = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const char *csrc = reinterpret_cast<const char *>(src) + (size_t)col * src_ld * 8;
    char *cdst = reinterpret_cast<char *>(dst) + (size_t)col * dst_ld * 8;
    const uint32_t *off_col = offsets + (size_t)col * RADIX * ntiles;
    const uint32_t *tot_col = digit_tot + (size_t)col * RADIX;
    uint64_t keys[SORT_ITEMS];
    uint32_t pay[SORT_ITEMS];
    uint32_t vm;
    load_keys<FROM_F64>(csrc, n, (int64_t)tile * SORT_TILE, keys, vm);
    if (PAIRS) {
        const int64_t base = (int64_t)tile * SORT_TILE + (int64_t)wave * 64 * SORT_ITEMS + lane;
        const int64_t last = n > 0 ? n - 1 : 0;
#pragma unroll
        for (int i = 0; i < SORT_ITEMS; ++i) {
            const int64_t idx = base + (int64_t)i * 64;
            pay[i] = pay_src ? pay_src[idx < n ? idx : last] : (uint32_t)idx;
        }
    }
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t rank[SORT_ITEMS];
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        const bool valid = (vm >> i) & 1u;
        const uint32_t d = (uint32_t)(keys[i] >> shift) & 0xFF;
        uint64_t peers = __ballot(valid);
        // lanes holding the same digit: eight ballots -- unless the whole wavefront agrees (every
        // constant digit position of an integer-valued column), which one shuffle + ballot detects
        const uint32_t d0 = __shfl(d, peers ? __ffsll((long long)peers) - 1 : 0, 64);
        if (__ballot(valid && d != d0) != 0) {
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool set = (d >> bit) & 1u;
                const uint64_t m = __ballot(set);
                peers &= set ? m : ~m;
            }
        }
        uint32_t r = 0;
        if (valid) {
            const uint32_t before = cnt[wave][d];
            const uint32_t in_group = (uint32_t)__popcll(peers & lt_mask);
            r = before + in_group;
            __builtin_amdgcn_wave_barrier();
            if (in_group == 0) cnt[wave][d] = before + (uint32_t)__popcll(peers);
        }
        __builtin_amdgcn_wave_barrier();
        rank[i] = r;
    }
    __syncthreads();
    // The keys are first placed in digit order in LDS (tile-local position = exclusive digit prefix
    // + wave offset + rank), then written out by consecutive lanes: a digit's run of keys (16 on
    // average) becomes one contiguous global store instead of 8-byte stores to 64 places.
    {
        const int d = threadIdx.x;
        const uint32_t c0 = cnt[0][d], c1 = cnt[1][d], c2 = cnt[2][d], c3 = cnt[3][d];
        const uint32_t total = c0 + c1 + c2 + c3;
        // two exclusive prefixes over the 256 digits: the tile-local one (digit totals of this tile) and
        // the global digit base (digit totals of the whole column, from scan_rows_kernel)
        const uint32_t gtot = tot_col[d];
        uint32_t inc = total, ginc = gtot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(inc, off, 64), gy = __shfl_up(ginc, off, 64);
            if (lane >= off) { inc += y; ginc += gy; }
        }
        if (lane == 63) { wsum[wave] = inc; wsum[4 + wave] = ginc; }
        __syncthreads();
        uint32_t lp = inc - total, gbase = ginc - gtot;
        for (int w = 0; w < wave; ++w) { lp += wsum[w]; gbase += wsum[4 + w]; }
        const uint32_t g = off_col[(size_t)d * ntiles + tile] + gbase;
        gdelta[d] = g - lp;                                     // global position = gdelta[digit] + local position
        cnt[0][d] = lp;
        cnt[1][d] = lp + c0;
        cnt[2][d] = lp + c0 + c1;
        cnt[3][d] = lp + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        if ((vm >> i) & 1u) {
            const uint32_t d = (uint32_t)(keys[i] >> shift) & 0xFF;
            const uint32_t at = cnt[wave][d] + rank[i];
            stage[at] = keys[i];
            if (PAIRS) stage_pay[at] = pay[i];
        }
    }
    __syncthreads();
    const int64_t left = n - (int64_t)tile * SORT_TILE;
    const int nv = (int)(left < SORT_TILE ? left : SORT_TILE);
    for (int j = threadIdx.x; j < nv; j += SORT_THREADS) {
        const uint64_t key = stage[j];
        const uint32_t pos = gdelta[(uint32_t)(key >> shift) & 0xFF] + (uint32_t)j;
        if (TO_F64) reinterpret_cast<double *>(cdst)[pos] = key_to_f64(key);
        else reinterpret_cast<uint64_t *>(cdst)[pos] = key;
        if (PAIRS) pay_dst[pos] = stage_pay[j];
    }
}

template <bool PAIRS>
auto scatter_for(bool from_f64, bool to_f64)
{
    return from_f64 ? scatter_kernel<true, false, PAIRS>
           : to_f64 ? scatter_kernel<false, true, PAIRS>
                    : scatter_kernel<false, false, PAIRS>;
}

// Sorts ncols columns of `in` (column stride ld) into `out` (column stride out_ld), ascending; keysA and hist are
// scratch (make_plan: keys_bytes, hist_bytes).  raw_u64: the columns hold 64-bit keys instead of fp64 values.
// perm != nullptr (one column only): perm[i] = the index sorted position i came from, with payA (n words) as scratch.
int sort_passes(int64_t n, int ncols, const void *in, int64_t ld, void *out, int64_t out_ld, uint64_t *keysA,
                uint32_t *hist, hipStream_t st, bool raw_u64 = false, uint32_t *perm = nullptr, uint32_t *payA = nullptr)
{
    const SortPlan p = make_plan(n, ncols);
    const dim3 grid(p.ntiles, ncols);
    uint32_t *tot = hist + grx_align_up((size_t)ncols * RADIX * (size_t)p.ntiles * 4, 256) / 4;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 8 * pass;
        // ping-pong: pass 0 in->A, odd A->out, even out->A; pass 7 writes fp64 into out.  The payload likewise
        // (pass 0 makes it up: the positions).
        const void *src;
        int64_t sld;
        void *dst;
        int64_t dld;
        if (pass == 0) { src = in; sld = ld; }
        else if (pass & 1) { src = keysA; sld = n; }
        else { src = out; sld = out_ld; }
        if (pass & 1) { dst = out; dld = out_ld; }
        else { dst = keysA; dld = n; }
        const uint32_t *psrc = pass == 0 ? nullptr : ((pass & 1) ? payA : perm);
        uint32_t *pdst = (pass & 1) ? perm : payA;
        const bool from_f64 = pass == 0 && !raw_u64, to_f64 = pass == 7 && !raw_u64;
        {
            GRX_PROF(GRX_K_SORT_COUNT, st);
            if (from_f64) tile_count_kernel<true><<<grid, SORT_THREADS, 0, st>>>(src, sld, n, shift, p.ntiles, hist);
            else tile_count_kernel<false><<<grid, SORT_THREADS, 0, st>>>(src, sld, n, shift, p.ntiles, hist);
        }
        GRX_LAUNCH_CHECK();
        {
            GRX_PROF(GRX_K_SORT_SCAN, st);
            scan_rows_kernel<<<dim3(RADIX, ncols), 64, 0, st>>>(hist, p.ntiles, tot);
        }
        GRX_LAUNCH_CHECK();
        {
            GRX_PROF(GRX_K_SORT_SCATTER, st);
            const auto scatter = perm ? scatter_for<true>(from_f64, to_f64) : scatter_for<false>(from_f64, to_f64);
            scatter<<<grid, SORT_THREADS, 0, st>>>(src, sld, dst, dld, psrc, pdst, n, shift, p.ntiles, hist, tot);
        }
        GRX_LAUNCH_CHECK();
    }
    return GRX_OK;
}

}  // namespace

// internal entry for other translation units (grx_quant.hip): workspace laid out as in
// grx_sort_columns (key buffer, then counters)
int grx_internal_sort_columns(int64_t n, int ncols, const double *cols, int64_t ld, double *out, int64_t out_ld,
                              void *workspace, hipStream_t st)
{
    const SortPlan p = make_plan(n, ncols);
    char *ws = reinterpret_cast<char *>(workspace);
    return sort_passes(n, ncols, cols, ld, out, out_ld, reinterpret_cast<uint64_t *>(ws),
                       reinterpret_cast<uint32_t *>(ws + p.keys_bytes), st);
}

// one fp64 column -> ascending values in `out` and, in `perm`, the index each sorted position came from (stable).
// workspace: grx_internal_sort_pairs_workspace_bytes(n) = key buffer, payload buffer, counters
int grx_internal_sort_pairs(int64_t n, const double *col, double *out, uint32_t *perm, void *workspace, hipStream_t st)
{
    if (n <= 0) return GRX_OK;
    const SortPlan p = make_plan(n, 1);
    char *ws = reinterpret_cast<char *>(workspace);
    uint32_t *payA = reinterpret_cast<uint32_t *>(ws + p.keys_bytes);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + p.keys_bytes + grx_align_up((size_t)n * 4, 256));
    return sort_passes(n, 1, col, n, out, n, reinterpret_cast<uint64_t *>(ws), hist, st, false, perm, payA);
}

size_t grx_internal_sort_pairs_workspace_bytes(int64_t n)
{
    if (n <= 0) return 256;
    const SortPlan p = make_plan(n, 1);
    return p.keys_bytes + grx_align_up((size_t)n * 4, 256) + p.hist_bytes;
}

// raw 64-bit keys (graph ingest: (row, column) / (row, edge sequence) pairs), ascending; same workspace
int grx_internal_sort_u64(int64_t n, const uint64_t *keys, uint64_t *out, void *workspace, hipStream_t st)
{
    if (n <= 0) return GRX_OK;
    const SortPlan p = make_plan(n, 1);
    char *ws = reinterpret_cast<char *>(workspace);
    return sort_passes(n, 1, keys, n, out, n, reinterpret_cast<uint64_t *>(ws),
                       reinterpret_cast<uint32_t *>(ws + p.keys_bytes), st, true);
}

extern "C" {

size_t grx_sort_workspace_bytes(int64_t n, int ncols)
{
    if (n <= 0 || ncols <= 0) return 256;
    const SortPlan p = make_plan(n, ncols);
    return p.keys_bytes + p.hist_bytes;
}

int grx_sort_columns(int64_t n, int ncols, const double *d_cols, int64_t ld, double *d_sorted,
                     int64_t ld_sorted, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && ncols >= 0 && ld >= n && ld_sorted >= n, "grx_sort_columns: bad shape");
    GRX_REQUIRE(n < ((int64_t)1 << 31), "grx_sort_columns: n must be < 2^31");
    if (n == 0 || ncols == 0) return GRX_OK;
    GRX_REQUIRE(d_cols && d_sorted && d_workspace, "grx_sort_columns: NULL pointer");
    if (workspace_bytes < grx_sort_workspace_bytes(n, ncols)) {
        grx_set_error("grx_sort_columns: workspace %zu < %zu", workspace_bytes, grx_sort_workspace_bytes(n, ncols));
        return GRX_ERR_WORKSPACE;
    }
    const SortPlan p = make_plan(n, ncols);
    char *ws = reinterpret_cast<char *>(d_workspace);
    return sort_passes(n, ncols, d_cols, ld, d_sorted, ld_sorted, reinterpret_cast<uint64_t *>(ws),
                       reinterpret_cast<uint32_t *>(ws + p.keys_bytes), grx_stream(stream));
}

}  // extern "C"
