// grx_square_clustering.hip -- the square clustering coefficient of RolX sense making: networkx 3.4.2's
// square_clustering (cluster.py; Lind et al. 2005, Zhang et al. 2008), the probability that two neighbours of a node
// share a common neighbour other than that node.  networkx loops over the pairs {u, w} of G[v] with a set intersection
// per pair; summed over the pairs its integers collapse to (N = G[v] as a set, v itself in it when v has a self-loop,
// d = |N|, k_u = len(G[u]))
//   K1   = sum_{u in N} k_u                         the wedges v -> u -> x that leave v: the work of the row
//   c(x) = |{u in N : x in G[u]}|   for x != v      row v of A^2 with set semantics
//   Q    = sum_{x != v} c(x) (c(x) - 1) / 2         networkx's numerator: the 4-cycles through v
//   S    = sum_{x in N, x != v} c(x)
//   L    = |{x in N, x != v : x has a self-loop}|
//   2T   = S - L + (d - 1) [v has a self-loop]      T = the adjacent unordered pairs inside N
//   potential = (d - 1) (K1 - d) - 2T - Q           C4(v) = potential > 0 ? Q / potential : Q
// Every quantity is an integer until the one division, so below 2^53 the quotient is networkx's own.  networkx divides
// only when potential > 0 and otherwise leaves its numerator: without self-loops Q is 0 then, with them a potential
// <= 0 beside a Q > 0 occurs (a node with a loop whose one other neighbour has a loop too: Q = 1, potential = -1).
//
// Two stages over a symmetric CSR with ascending columns:
//   (1) per row: K1 and the self-loop flag, packed as stat[v] = 2 K1 + flag -- a row body of grx_rowjoin.h's stage (a)
//       (a lane group per row, a workgroup per hub row); it reads the row pointers of the neighbours only;
//   (2) per row: c(x) counted over the wedges, then Q from the counters, S and L from a look-up of the row's own
//       entries, and the division.  One workgroup per row; three launches by K1, which also bounds the distinct x:
//         K1 <= SQ_WAVE_MAX_WEDGES    a workgroup of one wavefront, an open-addressing table of 1 024 slots in LDS
//         K1 <= SQ_LDS_MAX_WEDGES     a workgroup of four, a table of 4 096 slots
//         above                       a workgroup of sixteen and dense int32[n] counters in the workspace, one set per
//                                     workgroup of that launch (SQ_DENSE_WG of them), zeroed once per call and cleaned
//                                     by a second walk over the row's wedges, which also takes Q: atomicExch returns c(x)
//                                     to whichever lane comes first and 0 to the others
//       A table is sized from K1 (the power of two >= 4 K1 / 3, so it is at most three quarters full and never
//       overflows), cleared to that size only, keyed by int32 ids through a multiplicative hash (ids that are congruent
//       modulo every power of two still spread) with linear probing: LDS compare-and-swap claims a slot, an LDS add
//       counts.  Workgroup g takes the rows v = g (mod the grid) of its tier: it reads stat of BLOCK such rows at a
//       time and keeps those of its tier in an LDS list.
//       The wedges of a row: a group of GL lanes per neighbour u, lane k the entries k, k + GL, ... of row u; a
//       neighbour whose row is longer than 32 GL goes to an LDS list and is walked by the whole workgroup afterwards,
//       so a hub among the neighbours does not hold one group for its whole row.
// Bound: 4 sum_v K1(v) = 4 sum_u k_u^2 bytes of gathered column ids (twice for the rows of the dense tier), one LDS
// (global) atomic per wedge.
// Only integer atomics whose combined result does not depend on their order: every output has the same bits in every
// run and for every lanes_per_row (the order of the LDS lists varies; nothing read from them depends on it).
#pragma clang fp contract(off)

#include "grx_rowjoin.h"

namespace {

constexpr int SQ_WAVE_MAX_WEDGES = 768;                      // graphrole_amd/kernels.py carries copies of these two
constexpr int SQ_LDS_MAX_WEDGES = 3072;
constexpr int SQ_WAVE_SLOTS = 1024, SQ_LDS_SLOTS = 4096;     // >= 4 / 3 of the tier's largest K1
constexpr int SQ_DENSE_WG = 128;                             // workgroups (and counter sets) of the dense tier
constexpr int SQ_LIST = 256;                                 // long neighbours a row keeps for the whole workgroup
constexpr int SQ_WAVE_MAX_WG = 8192, SQ_LDS_MAX_WG = 1024;
constexpr int32_t SQ_EMPTY = -1;

static_assert(SQ_WAVE_SLOTS * 3 >= SQ_WAVE_MAX_WEDGES * 4 && SQ_LDS_SLOTS * 3 >= SQ_LDS_MAX_WEDGES * 4, "table size");

// (1)
struct sq_rows {
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col;
    int64_t *__restrict__ stat;
    struct Acc { double k1, loop; };                         // integers below 2^53: exact in every order
    __device__ __forceinline__ void entry(int64_t v, int64_t j, Acc &a) const
    {
        const int32_t u = col[j];
        a.k1 += (double)(row_ptr[u + 1] - row_ptr[u]);
        if (u == (int32_t)v) a.loop += 1.0;
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.k1 = r.sum(a.k1); a.loop = r.sum(a.loop); }
    __device__ __forceinline__ void finish(int64_t v, int64_t, int64_t, const Acc &a) const
    {
        stat[v] = ((int64_t)a.k1 << 1) | (a.loop != 0.0 ? 1 : 0);
    }
};

// the counters of a row: an LDS table ...
struct SqTable {
    int32_t *keys, *cnt;
    uint32_t mask, shift;
    __device__ __forceinline__ uint32_t home(int32_t x) const { return ((uint32_t)x * 2654435769u) >> shift; }
    __device__ __forceinline__ void add(int32_t x) const
    {
        for (uint32_t h = home(x);; h = (h + 1) & mask) {
            const int32_t was = atomicCAS(&keys[h], SQ_EMPTY, x);
            if (was == SQ_EMPTY || was == x) { atomicAdd(&cnt[h], 1); return; }
        }
    }
    __device__ __forceinline__ int64_t get(int32_t x) const          // after the barrier that ends the counting
    {
        for (uint32_t h = home(x);; h = (h + 1) & mask) {
            const int32_t key = keys[h];
            if (key == x) return cnt[h];
            if (key == SQ_EMPTY) return 0;
        }
    }
};
// ... or dense counters in the workspace
struct SqDense {
    int32_t *cnt;
    __device__ __forceinline__ void add(int32_t x) const { atomicAdd(&cnt[x], 1); }
    __device__ __forceinline__ int64_t get(int32_t x) const
    {
        return __hip_atomic_load(&cnt[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ int64_t take(int32_t x) const { return atomicExch(&cnt[x], 0); }
};

template <int BLOCK>
__device__ __forceinline__ int64_t sq_block_sum(int64_t v, int64_t *sm)
{
#pragma unroll
    for (int off = GRX_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, GRX_WAVE);
    if (BLOCK == GRX_WAVE) return v;
    if (threadIdx.x % GRX_WAVE == 0) sm[threadIdx.x / GRX_WAVE] = v;
    __syncthreads();
    int64_t total = 0;
    for (int w = 0; w < BLOCK / GRX_WAVE; ++w) total += sm[w];
    __syncthreads();
    return total;
}

// f(x) for every wedge v -> u -> x with x != v.  Every thread of the workgroup calls it; *s_nlong is 0 on entry and on
// return.
template <int BLOCK, int GL, class F>
__device__ __forceinline__ void sq_walk(int32_t v, int64_t b, int64_t e, const int64_t *__restrict__ row_ptr,
                                        const int32_t *__restrict__ col, int32_t *s_long, int *s_nlong, F f)
{
    constexpr int LONG = 32 * GL;
    const int lane = threadIdx.x % GL, group = threadIdx.x / GL;
    for (int64_t j = b + group; j < e; j += BLOCK / GL) {
        const int32_t u = col[j];
        const int64_t bu = row_ptr[u], eu = row_ptr[u + 1];
        if (eu - bu > LONG) {
            int pos = 0;
            if (lane == 0) pos = atomicAdd(s_nlong, 1);
            pos = __shfl(pos, 0, GL);
            if (pos < SQ_LIST) {
                if (lane == 0) s_long[pos] = u;
                continue;
            }
        }                                                    // (a full list: the group walks the long row itself)
        for (int64_t k = bu + lane; k < eu; k += GL) {
            const int32_t x = col[k];
            if (x != v) f(x);
        }
    }
    __syncthreads();
    const int nlong = *s_nlong < SQ_LIST ? *s_nlong : SQ_LIST;
    for (int i = 0; i < nlong; ++i) {
        const int32_t u = s_long[i];
        const int64_t eu = row_ptr[u + 1];
        for (int64_t k = row_ptr[u] + threadIdx.x; k < eu; k += BLOCK) {
            const int32_t x = col[k];
            if (x != v) f(x);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *s_nlong = 0;
    __syncthreads();
}

// (2) SLOTS > 0: the rows with lo < K1 <= hi through a table of at most SLOTS slots; SLOTS == 0: the rows with
// lo < K1 through dense + blockIdx.x * dense_stride (all zero on entry and on return)
template <int BLOCK, int GL, int SLOTS>
__global__ __launch_bounds__(BLOCK) void sq_count_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ col,
                                                         const int64_t *__restrict__ stat, int64_t lo, int64_t hi,
                                                         int32_t *__restrict__ dense, int64_t dense_stride,
                                                         double *__restrict__ out, int64_t *__restrict__ squares,
                                                         int64_t *__restrict__ potential)
{
    constexpr bool TABLE = SLOTS > 0;
    __shared__ int32_t s_keys[TABLE ? SLOTS : 1], s_cnt[TABLE ? SLOTS : 1];
    __shared__ int32_t s_rows[BLOCK], s_long[SQ_LIST];
    __shared__ int s_nrows, s_nlong;
    __shared__ int64_t s_sum[BLOCK / GRX_WAVE];
    const int t = threadIdx.x;
    if (t == 0) { s_nrows = 0; s_nlong = 0; }
    __syncthreads();
    const SqDense counters{dense + (TABLE ? 0 : blockIdx.x * dense_stride)};
    for (int64_t base = blockIdx.x; base < n; base += (int64_t)BLOCK * gridDim.x) {
        // the rows of this workgroup's residue class that belong to the tier, BLOCK candidates at a time
        const int64_t cand = base + (int64_t)t * gridDim.x;
        if (cand < n) {
            const int64_t k1 = stat[cand] >> 1;
            if (k1 > lo && k1 <= hi) s_rows[atomicAdd(&s_nrows, 1)] = (int32_t)cand;
        }
        __syncthreads();
        const int nrows = s_nrows;
        for (int r = 0; r < nrows; ++r) {
            const int32_t v = s_rows[r];
            const int64_t b = row_ptr[v], e = row_ptr[v + 1], d = e - b;
            const int64_t k1 = stat[v] >> 1, loop = stat[v] & 1;
            int64_t q = 0, s = 0, l = 0;
            if constexpr (TABLE) {
                uint32_t cap = 64, shift = 26;               // cap = 2^(32 - shift) >= 4 K1 / 3 > the distinct x
                while ((int64_t)cap * 3 < k1 * 4) { cap <<= 1; --shift; }
                const SqTable table{s_keys, s_cnt, cap - 1, shift};
                for (uint32_t i = t; i < cap; i += BLOCK) { s_keys[i] = SQ_EMPTY; s_cnt[i] = 0; }
                __syncthreads();
                sq_walk<BLOCK, GL>(v, b, e, row_ptr, col, s_long, &s_nlong, [&](int32_t x) { table.add(x); });
                for (uint32_t i = t; i < cap; i += BLOCK) {
                    const int64_t c = s_cnt[i];
                    q += c * (c - 1) / 2;
                }
                for (int64_t j = b + t; j < e; j += BLOCK) {
                    const int32_t x = col[j];
                    if (x != v) { s += table.get(x); l += stat[x] & 1; }
                }
            } else {
                sq_walk<BLOCK, GL>(v, b, e, row_ptr, col, s_long, &s_nlong, [&](int32_t x) { counters.add(x); });
                __threadfence();
                __syncthreads();
                for (int64_t j = b + t; j < e; j += BLOCK) {
                    const int32_t x = col[j];
                    if (x != v) { s += counters.get(x); l += stat[x] & 1; }
                }
                __syncthreads();
                sq_walk<BLOCK, GL>(v, b, e, row_ptr, col, s_long, &s_nlong, [&](int32_t x) {
                    const int64_t c = counters.take(x);
                    q += c * (c - 1) / 2;
                });
                __threadfence();
            }
            q = sq_block_sum<BLOCK>(q, s_sum);
            s = sq_block_sum<BLOCK>(s, s_sum);
            l = sq_block_sum<BLOCK>(l, s_sum);
            if (t == 0) {
                const int64_t two_t = s - l + (d - 1) * loop;
                const int64_t pot = (d - 1) * (k1 - d) - two_t - q;
                if (squares) squares[v] = q;
                if (potential) potential[v] = pot;
                out[v] = pot > 0 ? (double)q / (double)pot : (double)q;      // networkx divides only then
            }
            __syncthreads();
        }
        if (t == 0) s_nrows = 0;
        __syncthreads();
    }
}

// the workspace: stat int64[n] | SQ_DENSE_WG x int32[n]; each 256-byte aligned
struct SqWs {
    char *base;
    size_t stat_bytes, dense_bytes;
    SqWs(void *b, int64_t n)
        : base(reinterpret_cast<char *>(b)), stat_bytes(grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256)),
          dense_bytes(grx_align_up((size_t)(n > 0 ? n : 1) * 4, 256)) {}
    int64_t *stat() const { return reinterpret_cast<int64_t *>(base); }
    int32_t *dense() const { return reinterpret_cast<int32_t *>(base + stat_bytes); }
    size_t bytes() const { return stat_bytes + SQ_DENSE_WG * dense_bytes; }
};

}  // namespace

extern "C" {

size_t grx_square_clustering_workspace_bytes(int64_t n) { return SqWs(nullptr, n).bytes(); }

int grx_square_clustering(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                          int64_t n_hub_rows, int lanes_per_row, double *d_square_clustering, int64_t *d_squares,
                          int64_t *d_potential, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "grx_square_clustering";
    GRX_REQUIRE(d_square_clustering, "%s: d_square_clustering is NULL", who);
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "%s: n = %lld out of range [0, 2^31)", who, (long long)n);
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_workspace, "%s: null pointer", who);
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "%s: lanes_per_row must be 4, 8, 16 or 32 (got %d)", who, lanes_per_row);
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "%s: hub list", who);
    const SqWs ws(d_workspace, n);
    GRX_REQUIRE(workspace_bytes >= ws.bytes(), "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.bytes());
    hipStream_t st = grx_stream(stream);
    int64_t *stat = ws.stat();
    const int64_t dense_stride = (int64_t)(ws.dense_bytes / 4);
    grx_fill32(ws.dense(), SQ_DENSE_WG * dense_stride, 0, st);

    const sq_rows rows{d_row_ptr, d_col, stat};
    if (n_hub_rows) rj_hub_rows_kernel<<<(unsigned)n_hub_rows, RJ_BLOCK, 0, st>>>(d_row_ptr, d_hub_rows, rows);
    rj_with_lanes(lanes_per_row, [&](auto width) {
        constexpr int L = decltype(width)::value;
        rj_rows_kernel<L><<<grx_grid(n, RJ_BLOCK / L, RJ_ROW_MAX_WG), RJ_BLOCK, 0, st>>>(
            n, d_row_ptr, (int64_t)GRX_HUB_FACTOR * L, rows);
    });

    const int64_t none = INT64_MAX;
    sq_count_kernel<GRX_WAVE, 8, SQ_WAVE_SLOTS><<<grx_grid(n, GRX_WAVE, SQ_WAVE_MAX_WG), GRX_WAVE, 0, st>>>(
        n, d_row_ptr, d_col, stat, -1, SQ_WAVE_MAX_WEDGES, nullptr, 0, d_square_clustering, d_squares, d_potential);
    sq_count_kernel<256, 16, SQ_LDS_SLOTS><<<grx_grid(n, 256, SQ_LDS_MAX_WG), 256, 0, st>>>(
        n, d_row_ptr, d_col, stat, SQ_WAVE_MAX_WEDGES, SQ_LDS_MAX_WEDGES, nullptr, 0, d_square_clustering, d_squares,
        d_potential);
    sq_count_kernel<1024, 32, 0><<<grx_grid(n, 1024, SQ_DENSE_WG), 1024, 0, st>>>(
        n, d_row_ptr, d_col, stat, SQ_LDS_MAX_WEDGES, none, ws.dense(), dense_stride, d_square_clustering, d_squares,
        d_potential);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
