// grx_closeness.hip -- per-target BFS distance sums for RolX sense making: the reach counts and distance sums behind
// networkx 3.4.2's closeness_centrality (closeness.py:107-137) and the reciprocal-distance sums of
// harmonic_centrality (harmonic.py:68-89), all sources at once by a bitset multi-source BFS (MS-BFS: Then et al.,
// "The More the Merrier: Efficient Multi-Source Graph Traversal", VLDB 2014).
//
// A batch holds S = 64 W sources.  Source lane b of the batch is bit b % 64 of word b / 64; every node holds three
// masks of W uint64 words, node-major (word w of node v at v * W + w): visited, and the frontier of this level and of
// the next (two buffers that swap roles every level).  W lanes of a wavefront handle one node, lane w its word w, so
// reading a neighbour's frontier is one contiguous 8 W-byte load.
//
// Level l -> l + 1 pulls over the adjacency it is given: next(v) = (OR over the listed neighbours u of frontier(u)) &
// active & ~visited(v).  A lane stops scanning once its word of visited(v) | next(v) covers every active source bit
// (early exit); a node whose visited words are full reads nothing.  Rows longer than GRX_HUB_FACTOR * lanes_per_row
// are the CSR's hub list and get a workgroup each: its 256 / W lane groups take every (256 / W)-th arc and OR their
// masks in a tree through LDS.  The node's own writer (lane 0 of its group) then adds, with c = popcount(next(v)) and
// d = l + 1:
//   reach(v) += c,  dsum(v) += d c  (int64, exact: dsum <= n^2 < 2^62),
//   harm(v)  += c q(d), q(d) = fl(1 / d) 2^84 as an unsigned 128-bit integer: for d < 2^31 the fp64 value fl(1 / d)
//              is a whole multiple of 2^-84, and the sum stays below n_sources 2^84 < 2^115.
// The levels run as a device-steered round loop (grx_common.h).
// At the end harmonic(v) = harm(v) 2^-84, rounded once to nearest-even: the correctly rounded sum of the fp64
// terms fl(1 / d), the same bits for every W, source order and run.  Integer arithmetic only; no floating-point
// atomics (the source bits are set with integer atomicOr).
// The traversal is written once (ms_level_kernel, ms_level_hub_kernel and the host's ms_bfs: the level core below);
// what the writer adds is a body.  grx_distance_sums runs it with the sums above; grx_eccentricity with two more
// bodies that take a maximum in place of the sums: the eccentricity of every source, the per-target maximum distance
// and the eccentricity bounds of Takes and Kosters.
#pragma clang fp contract(off)

#include "grx_common.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_MAX_WORDS = 16;
constexpr int CL_LEVEL_BATCH = 8;                            // levels enqueued between two read-backs
constexpr int CL_MAX_ROW_BLOCKS = 8192;
constexpr int CL_MAX_BLOCKS = 2048;                           // grid of the per-element launch
constexpr size_t CL_DEFAULT_STATE_BYTES = (size_t)4 << 30;   // state budget of the library's choice of W
constexpr int CL_HARM_SHIFT = 84;                            // harm(v) holds sum c fl(1 / d) scaled by 2^84

bool valid_words(int w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

// W of words = 0: the narrowest power of two that holds the source list, but no wider than the widest power of two
// up to 16 whose state (visited + two frontiers, 24 n bytes per word) fits CL_DEFAULT_STATE_BYTES, and at least 1
int choose_words(int64_t n, int words, int64_t n_sources)
{
    if (words > 0) return words;
    const size_t per_word = (size_t)(n > 0 ? n : 1) * 24;
    int widest = 1;
    while (widest < CL_MAX_WORDS && per_word * (size_t)(widest * 2) <= CL_DEFAULT_STATE_BYTES) widest *= 2;
    const int64_t needed = grx_ceil_div(std::max<int64_t>(n_sources, 1), GRX_WAVE);
    int w = 1;
    while (w < widest && w < needed) w *= 2;
    return w;
}

// the workspace: visited | f0 | f1 (uint64[n W] each) | harm (uint64[2 n]; the distance sums only) | control words
struct MsWs {
    uint64_t *visited, *f0, *f1;
    uint64_t *harm;                                          // (lo, hi) per node; null without with_harm
    int32_t *ctrl;
};

MsWs lay_out(GrxCarve &c, int64_t n, int W, bool with_harm)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    MsWs ws;
    ws.visited = c.take<uint64_t>(nn * (size_t)W);
    ws.f0 = c.take<uint64_t>(nn * (size_t)W);
    ws.f1 = c.take<uint64_t>(nn * (size_t)W);
    ws.harm = with_harm ? c.take<uint64_t>(2 * nn) : nullptr;
    ws.ctrl = c.take<int32_t>(GRX_CTRL_MAX_WORDS);
    return ws;
}

// the source bits of word w that belong to the batch's `count` sources
__device__ __forceinline__ uint64_t active_mask(int count, int w)
{
    const int bits = count - w * GRX_WAVE;
    return bits >= GRX_WAVE ? ~0ull : bits <= 0 ? 0ull : (1ull << bits) - 1;
}

// sum over the W lanes of a group (every lane of the wavefront takes part)
template <int W>
__device__ __forceinline__ int group_sum(int c)
{
#pragma unroll
    for (int off = 1; off < W; off <<= 1) c += __shfl_xor(c, off, W);
    return c;
}

// OR of word w of frontier(u) over the arcs [b, e) with stride `step`, masked to `want`; stops once `want` is covered
template <int W>
__device__ __forceinline__ uint64_t pull_words(int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                               const uint64_t *__restrict__ F, int w, uint64_t want)
{
    if (!want) return 0;
    uint64_t acc = 0;
    int64_t j = b;
    for (; j + 3 * step < e; j += 4 * step) {
        const int64_t u0 = col[j], u1 = col[j + step], u2 = col[j + 2 * step], u3 = col[j + 3 * step];
        acc |= (F[u0 * W + w] | F[u1 * W + w]) | (F[u2 * W + w] | F[u3 * W + w]);
        if ((acc & want) == want) return want;
    }
    for (; j < e; j += step) {
        acc |= F[(int64_t)col[j] * W + w];
        if ((acc & want) == want) return want;
    }
    return acc & want;
}

// lane b < count: bit b of source s_b's visited and frontier words (integer atomics: one node may be the source of
// several lanes of a word); level 0
__global__ __launch_bounds__(CL_BLOCK) void cl_source_init_kernel(int64_t n, int W, int count,
                                                                  const int32_t *__restrict__ src,
                                                                  uint64_t *__restrict__ visited,
                                                                  uint64_t *__restrict__ f0,
                                                                  int32_t *__restrict__ ctrl)
{
    for (int b = blockIdx.x * CL_BLOCK + threadIdx.x; b < count; b += gridDim.x * CL_BLOCK) {
        const int64_t s = src[b];
        if (s < 0 || s >= n) continue;                      // an id outside [0, n) is never written through
        const int64_t cell = s * W + b / GRX_WAVE;
        const unsigned long long bit = 1ull << (b % GRX_WAVE);
        atomicOr(reinterpret_cast<unsigned long long *>(&visited[cell]), bit);
        atomicOr(reinterpret_cast<unsigned long long *>(&f0[cell]), bit);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl[GRX_CT_DONE] = 0; ctrl[GRX_CT_LEVEL] = 0; ctrl[GRX_CT_FOUND] = 0; }
}

// ---- the level core: one BFS level over bodies -----------------------------------------------------------------
// Frontier selection, the pull, the visited / next stores, the hub rows' OR tree and the `found` flag are the two
// kernels below; what a node does with its new source bits is a body: a struct of kernel arguments (a template over W)
// with
//   struct Shared;                                           LDS of the row kernel
//   struct Acc;                                              what a thread carries across its nodes, zero-initialised
//   struct View;                                             what node() reads besides the kernel arguments
//   View row_begin(Shared &sh, int count) const;             row kernel, every thread, before the first node (with a
//                                                            barrier of its own after what it writes)
//   View hub_begin(const uint64_t *part, int d) const;       hub kernel, every thread: part[w] = word w of the hub's
//                                                            new source bits (LDS)
//   bool node(int64_t v, uint64_t nw, bool writer, int d, int w, View view, Acc &a) const;
//                                                            nw = word w of v's new source bits, at distance d (0 in a
//                                                            lane that holds no word of a node of this kernel).  Every
//                                                            lane of the wavefront calls it: the group reductions see
//                                                            them all.  `writer`: the one lane per node that updates
//                                                            v's outputs; true from that lane when it did
//   void row_end(Shared &sh, const Acc &a, int d, int w) const;    row kernel, every thread, after the last node
// The bodies are template arguments, so every call inlines.

// one level, rows up to hub_degree arcs: W lanes per node, CL_BLOCK / W nodes per workgroup and grid step
template <int W, class Body>
__global__ __launch_bounds__(CL_BLOCK) void ms_level_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                            const int32_t *__restrict__ col, int64_t hub_degree,
                                                            int count, uint64_t *__restrict__ visited,
                                                            uint64_t *__restrict__ f0, uint64_t *__restrict__ f1,
                                                            int32_t *__restrict__ ctrl, const Body body)
{
    constexpr int GROUPS = CL_BLOCK / W;
    __shared__ typename Body::Shared sh;
    if (ctrl[GRX_CT_DONE]) return;                          // the same in every lane of the launch
    const int l = ctrl[GRX_CT_LEVEL], d = l + 1;
    const uint64_t *F = (l & 1) ? f1 : f0;
    uint64_t *Fn = (l & 1) ? f0 : f1;
    const int w = threadIdx.x % W;
    const uint64_t active = active_mask(count, w);
    const typename Body::View view = body.row_begin(sh, count);
    int found = 0;                                          // an int: a bool is kept as a lane mask, 2 SGPRs more
    typename Body::Acc acc{};
    // the trip count is the same in every lane of the workgroup: the group reductions of the body see every lane
    for (int64_t first = (int64_t)blockIdx.x * GROUPS; first < n; first += (int64_t)gridDim.x * GROUPS) {
        const int64_t v = first + threadIdx.x / W;
        bool mine = false;
        uint64_t nw = 0;
        if (v < n) {
            const int64_t b = row_ptr[v], e = row_ptr[v + 1];
            if (e - b <= hub_degree) {                      // longer rows: ms_level_hub_kernel
                mine = true;
                const int64_t cell = v * W + w;
                const uint64_t vw = visited[cell];
                nw = pull_words<W>(b, e, 1, col, F, w, active & ~vw);
                Fn[cell] = nw;
                if (nw) visited[cell] = vw | nw;
            }
        }
        if (body.node(v, nw, mine && w == 0, d, w, view, acc)) found = 1;
    }
    if (__ballot(found != 0) && threadIdx.x % GRX_WAVE == 0) ctrl[GRX_CT_FOUND] = 1;
    body.row_end(sh, acc, d, w);
}

// one level, hub rows: one workgroup per hub row; CL_BLOCK / W lane groups take every (CL_BLOCK / W)-th arc
template <int W, class Body>
__global__ __launch_bounds__(CL_BLOCK) void ms_level_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                const int32_t *__restrict__ col,
                                                                const int32_t *__restrict__ hub_rows, int count,
                                                                uint64_t *__restrict__ visited,
                                                                uint64_t *__restrict__ f0, uint64_t *__restrict__ f1,
                                                                int32_t *__restrict__ ctrl, const Body body)
{
    constexpr int GROUPS = CL_BLOCK / W;
    __shared__ uint64_t part[CL_BLOCK];
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL], d = l + 1;
    const uint64_t *F = (l & 1) ? f1 : f0;
    uint64_t *Fn = (l & 1) ? f0 : f1;
    const int t = threadIdx.x, w = t % W;
    const int64_t v = hub_rows[blockIdx.x];
    const int64_t cell = v * W + w;
    const uint64_t vw = visited[cell];
    part[t] = pull_words<W>(row_ptr[v] + t / W, row_ptr[v + 1], GROUPS, col, F, w, active_mask(count, w) & ~vw);
    __syncthreads();
#pragma unroll
    for (int s = CL_BLOCK / 2; s >= W; s >>= 1) {          // part[t] for t < W: the OR over every group
        if (t < s) part[t] |= part[t + s];
        __syncthreads();
    }
    const typename Body::View view = body.hub_begin(part, d);
    if (t >= GRX_WAVE) return;
    const uint64_t nw = t < W ? part[t] : 0;
    if (t < W) {
        Fn[cell] = nw;
        if (nw) visited[cell] = vw | nw;
    }
    typename Body::Acc acc{};
    if (body.node(v, nw, t == 0, d, w, view, acc)) ctrl[GRX_CT_FOUND] = 1;
}

// the graph and the sources of a call
struct MsArgs {
    int64_t n;
    const int64_t *row_ptr;
    const int32_t *col;
    const int32_t *hub_rows;
    int64_t n_hub_rows, hub_degree;
    const int32_t *sources;
    int64_t n_sources;
};

// one BFS from the batch of `count` <= 64 W sources at src: clears the masks, seeds level 0 and runs the levels.
// `what`: the refusal of grx_run_rounds, with the caller's name
template <int W, class Body>
int ms_bfs(const char *what, const MsArgs &a, const MsWs &ws, const int32_t *src, int count, const Body &body,
           hipStream_t st)
{
    const int64_t n = a.n;
    const unsigned row_blocks = grx_grid(n, CL_BLOCK / W, CL_MAX_ROW_BLOCKS);
    grx_fill64(ws.visited, n * W, 0, st);
    grx_fill64(ws.f0, n * W, 0, st);
    cl_source_init_kernel<<<(unsigned)grx_ceil_div(count, CL_BLOCK), CL_BLOCK, 0, st>>>(n, W, count, src, ws.visited,
                                                                                        ws.f0, ws.ctrl);
    GRX_LAUNCH_CHECK();
    int32_t h[2];
    // a BFS has at most n - 1 levels; one more launch finds the empty frontier
    return grx_run_rounds(what, CL_LEVEL_BATCH, n + 1, 2, ws.ctrl, h, st, [&] {
        if (a.n_hub_rows)
            ms_level_hub_kernel<W><<<(unsigned)a.n_hub_rows, CL_BLOCK, 0, st>>>(
                a.row_ptr, a.col, a.hub_rows, count, ws.visited, ws.f0, ws.f1, ws.ctrl, body);
        ms_level_kernel<W><<<row_blocks, CL_BLOCK, 0, st>>>(n, a.row_ptr, a.col, a.hub_degree, count, ws.visited,
                                                            ws.f0, ws.f1, ws.ctrl, body);
        return grx_frontier_advance(ws.ctrl, st);
    });
}

// f(std::integral_constant<int, W>) for the W of a call
template <class F>
int ms_with_words(int W, F f)
{
    switch (W) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
    }
}

// ---- distance sums (grx_distance_sums) ---------------------------------------------------------------------------
// the node's writer: c newly reached sources at distance d
__device__ __forceinline__ void add_level(int64_t v, int c, int d, int64_t *__restrict__ reach,
                                          int64_t *__restrict__ dsum, uint64_t *__restrict__ harm)
{
    reach[v] += c;
    dsum[v] += (int64_t)d * c;
    // fl(1 / d) = m 2^(e - 52) with a 53-bit m and -31 <= e <= 0 (1 <= d < 2^31): times 2^84 is m << (e + 32)
    const double r = 1.0 / (double)d;
    const uint64_t bits = (uint64_t)__double_as_longlong(r);
    const int e = (int)((bits >> 52) & 0x7ff) - 1023;
    const uint64_t m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    const unsigned __int128 q = (unsigned __int128)m << (e + 32);
    unsigned __int128 h = ((unsigned __int128)harm[2 * v + 1] << 64) | harm[2 * v];
    h += (unsigned __int128)(uint64_t)c * q;
    harm[2 * v] = (uint64_t)h;
    harm[2 * v + 1] = (uint64_t)(h >> 64);
}

template <int W>
struct cl_sums {
    int64_t *__restrict__ reach, *__restrict__ dsum;
    uint64_t *__restrict__ harm;
    struct Shared {};
    struct Acc {};
    struct View {};
    __device__ __forceinline__ View row_begin(Shared &, int) const { return {}; }
    __device__ __forceinline__ View hub_begin(const uint64_t *, int) const { return {}; }
    __device__ __forceinline__ bool node(int64_t v, uint64_t nw, bool writer, int d, int, View, Acc &) const
    {
        const int c = group_sum<W>(__popcll(nw));
        if (!(writer && c)) return false;
        add_level(v, c, d, reach, dsum, harm);
        return true;
    }
    __device__ __forceinline__ void row_end(Shared &, const Acc &, int, int) const {}
};

// harmonic(v) = harm(v) 2^-84, rounded once to nearest-even (by hand: the top 53 bits plus the rounding bits below)
__global__ __launch_bounds__(CL_BLOCK) void cl_harmonic_kernel(int64_t n, const uint64_t *__restrict__ harm,
                                                               double *__restrict__ out)
{
    for (int64_t v = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * CL_BLOCK) {
        const unsigned __int128 h = ((unsigned __int128)harm[2 * v + 1] << 64) | harm[2 * v];
        double r = 0.0;
        if (h) {
            const uint64_t hi = (uint64_t)(h >> 64), lo = (uint64_t)h;
            const int top = hi ? 128 - __clzll((long long)hi) : 64 - __clzll((long long)lo);   // bit length
            int shift = top > 53 ? top - 53 : 0;
            uint64_t m = (uint64_t)(h >> shift);
            if (shift) {
                const unsigned __int128 rem = h & (((unsigned __int128)1 << shift) - 1);
                const unsigned __int128 half = (unsigned __int128)1 << (shift - 1);
                if (rem > half || (rem == half && (m & 1))) ++m;
                if (m >> 53) { m >>= 1; ++shift; }
            }
            r = ldexp((double)m, shift - CL_HARM_SHIFT);    // m < 2^53 and the power of two: both exact
        }
        out[v] = r;
    }
}

template <int W>
int sums_run(const MsArgs &a, const MsWs &ws, int64_t *reach, int64_t *dsum, double *harmonic, hipStream_t st)
{
    for (int64_t first = 0; first < a.n_sources; first += 64 * W) {
        const int count = (int)std::min<int64_t>(64 * W, a.n_sources - first);
        const int rc = ms_bfs<W>("grx_distance_sums: the BFS did not end after %lld levels", a, ws, a.sources + first,
                                 count, cl_sums<W>{reach, dsum, ws.harm}, st);
        if (rc != GRX_OK) return rc;
    }
    cl_harmonic_kernel<<<grx_grid(a.n, CL_BLOCK, CL_MAX_BLOCKS), CL_BLOCK, 0, st>>>(a.n, ws.harm, harmonic);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

// ---- eccentricities (grx_eccentricity) ---------------------------------------------------------------------------
// The level core with an extremal reduction in place of the sums, as two bodies.  Pass A of a batch: reach(v) += c,
// lower(v) = max(lower(v), d) for the level d at which new source bits arrive at v, and ecc(b) = the last level at which
// bit b was newly set anywhere (every workgroup ORs its `next` words through LDS and one lane per set bit stores d into
// the batch's int32 slots: many workgroups store the same value in one launch, plain stores).  Pass B, with the upper
// bounds asked for, replays the batch with ecc(b) now known (staged in LDS) and tightens the bounds of Takes and
// Kosters (2013): for the new bits nw of v at level d (level 0: the source itself)
//   upper(v) = min(upper(v), d + min over nw of ecc(b)),  lower(v) = max(lower(v), max over nw of ecc(b) - d),
// valid where d(s, v) = d(v, s): a symmetric CSR.  A source's own level-0 update pins lower = upper = ecc there.

constexpr int EC_WAVES = CL_BLOCK / GRX_WAVE;

// min resp. max over the W lanes of a group (every lane of the wavefront takes part)
template <int W>
__device__ __forceinline__ void group_min_max(int &lo, int &hi)
{
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
        lo = min(lo, __shfl_xor(lo, off, W));
        hi = max(hi, __shfl_xor(hi, off, W));
    }
}

// (min, max) of ecc over the set bits of word w's new bits; (INT32_MAX, -1) for none
__device__ __forceinline__ void ecc_range(uint64_t nw, const int32_t *ecc_w, int &lo, int &hi)
{
    lo = INT32_MAX;
    hi = -1;
    for (uint64_t m = nw; m; m &= m - 1) {
        const int e = ecc_w[__builtin_ctzll(m)];
        lo = min(lo, e);
        hi = max(hi, e);
    }
}

// pass B, level 0: source lane b sits on s_b at distance 0 (integer atomics: one node may carry several lanes)
__global__ __launch_bounds__(CL_BLOCK) void ec_source_bounds_kernel(int64_t n, int count,
                                                                    const int32_t *__restrict__ src,
                                                                    const int32_t *__restrict__ secc,
                                                                    int32_t *__restrict__ lower,
                                                                    int32_t *__restrict__ upper)
{
    for (int b = blockIdx.x * CL_BLOCK + threadIdx.x; b < count; b += gridDim.x * CL_BLOCK) {
        const int64_t s = src[b];
        if (s < 0 || s >= n) continue;
        atomicMin(&upper[s], secc[b]);
        atomicMax(&lower[s], secc[b]);
    }
}

// pass A.  secc: the batch's int32[count] slots of the source eccentricities, written here and read by pass B
template <int W>
struct ec_reach {
    int32_t *__restrict__ secc;
    int64_t *__restrict__ reach;
    int32_t *__restrict__ lower;
    struct Shared { uint64_t seen_of[EC_WAVES][W]; };
    struct Acc { uint64_t seen; };                           // word w of every new bit of the thread's nodes
    struct View {};
    __device__ __forceinline__ View row_begin(Shared &, int) const { return {}; }
    __device__ __forceinline__ View hub_begin(const uint64_t *part, int d) const
    {
        for (int b = threadIdx.x; b < GRX_WAVE * W; b += CL_BLOCK)
            if ((part[b / GRX_WAVE] >> (b % GRX_WAVE)) & 1) secc[b] = d;
        return {};
    }
    __device__ __forceinline__ bool node(int64_t v, uint64_t nw, bool writer, int d, int, View, Acc &a) const
    {
        a.seen |= nw;
        const int c = group_sum<W>(__popcll(nw));
        if (!(writer && c)) return false;
        const int64_t r = reach[v];                         // both loads before the stores: __restrict__ on a member
        const int32_t lw = lower[v];                        // does not let the compiler move the second one up
        reach[v] = r + c;
        lower[v] = max(lw, d);
        return true;
    }
    __device__ __forceinline__ void row_end(Shared &sh, const Acc &a, int d, int w) const
    {
        // OR over the lanes of the wavefront that hold word w, then over the wavefronts through LDS
        uint64_t seen = a.seen;
#pragma unroll
        for (int off = W; off < GRX_WAVE; off <<= 1)
            seen |= __shfl_xor((unsigned long long)seen, off, GRX_WAVE);
        if (threadIdx.x % GRX_WAVE < W) sh.seen_of[threadIdx.x / GRX_WAVE][w] = seen;
        __syncthreads();
        for (int b = threadIdx.x; b < GRX_WAVE * W; b += CL_BLOCK) {
            uint64_t m = 0;
#pragma unroll
            for (int k = 0; k < EC_WAVES; ++k) m |= sh.seen_of[k][b / GRX_WAVE];
            if ((m >> (b % GRX_WAVE)) & 1) secc[b] = d;     // set bits lie below `count`
        }
    }
};

// pass B: ecc(b) staged in LDS for the row kernel, and straight from global memory for the few hub rows
template <int W>
struct ec_bounds {
    const int32_t *__restrict__ secc;
    int32_t *__restrict__ lower, *__restrict__ upper;
    struct Shared { int32_t ecc[GRX_WAVE * W]; };
    struct Acc {};
    typedef const int32_t *View;                             // where node() reads ecc(b)
    __device__ __forceinline__ View row_begin(Shared &sh, int count) const
    {
        for (int b = threadIdx.x; b < GRX_WAVE * W; b += CL_BLOCK) sh.ecc[b] = b < count ? secc[b] : 0;
        __syncthreads();
        return sh.ecc;
    }
    __device__ __forceinline__ View hub_begin(const uint64_t *, int) const { return secc; }
    __device__ __forceinline__ bool node(int64_t v, uint64_t nw, bool writer, int d, int w, View ecc, Acc &) const
    {
        int lo, hi;
        ecc_range(nw, ecc + w * GRX_WAVE, lo, hi);
        group_min_max<W>(lo, hi);
        if (!(writer && hi >= 0)) return false;
        const int32_t up = upper[v], lw = lower[v];         // both loads before the stores, as in ec_reach
        upper[v] = min(up, d + lo);
        lower[v] = max(lw, hi - d);
        return true;
    }
    __device__ __forceinline__ void row_end(Shared &, const Acc &, int, int) const {}
};

// per batch: pass A, then pass B over the same sources when the upper bounds are asked for
template <int W>
int ec_run(const MsArgs &a, const MsWs &ws, int32_t *source_ecc, int64_t *reach, int32_t *lower, int32_t *upper,
           hipStream_t st)
{
    const char *what = "grx_eccentricity: the BFS did not end after %lld levels";
    for (int64_t first = 0; first < a.n_sources; first += 64 * W) {
        const int count = (int)std::min<int64_t>(64 * W, a.n_sources - first);
        const int32_t *src = a.sources + first;
        int32_t *secc = source_ecc + first;
        int rc = ms_bfs<W>(what, a, ws, src, count, ec_reach<W>{secc, reach, lower}, st);
        if (rc == GRX_OK && upper) {
            ec_source_bounds_kernel<<<(unsigned)grx_ceil_div(count, CL_BLOCK), CL_BLOCK, 0, st>>>(a.n, count, src,
                                                                                                  secc, lower, upper);
            rc = ms_bfs<W>(what, a, ws, src, count, ec_bounds<W>{secc, lower, upper}, st);
        }
        if (rc != GRX_OK) return rc;
    }
    return GRX_OK;
}

}  // namespace

extern "C" {

size_t grx_distance_sums_workspace_bytes(int64_t n, int words, int64_t n_sources)
{
    return grx_carve_bytes(lay_out, n, choose_words(n, words, n_sources), true);
}

int grx_distance_sums(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                      int64_t n_hub_rows, int lanes_per_row, const int32_t *d_sources, int64_t n_sources, int words,
                      int64_t *d_reach, int64_t *d_dsum, double *d_harmonic, void *d_workspace,
                      size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "grx_distance_sums: n = %lld out of range", (long long)n);
    GRX_REQUIRE(d_row_ptr && d_col && d_reach && d_dsum && d_harmonic && d_workspace,
                "grx_distance_sums: null pointer");
    GRX_REQUIRE(n_sources >= 0 && n_sources < (int64_t)1 << 31 && (n_sources == 0 || d_sources),
                "grx_distance_sums: source list");
    GRX_REQUIRE(words == 0 || valid_words(words), "grx_distance_sums: words must be 0, 1, 2, 4, 8 or 16 (got %d)",
                words);
    GRX_REQUIRE(lanes_per_row >= 1, "grx_distance_sums: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && (n_hub_rows == 0 || d_hub_rows), "grx_distance_sums: hub list");
    const int W = choose_words(n, words, n_sources);
    GrxCarve c(d_workspace);
    const MsWs ws = lay_out(c, n, W, true);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_distance_sums: workspace %zu bytes, need %zu", workspace_bytes,
                c.used);
    hipStream_t st = grx_stream(stream);
    const MsArgs a{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, (int64_t)GRX_HUB_FACTOR * lanes_per_row,
                   d_sources, n_sources};
    grx_fill64(reinterpret_cast<uint64_t *>(d_reach), n, 0, st);
    grx_fill64(reinterpret_cast<uint64_t *>(d_dsum), n, 0, st);
    grx_fill64(ws.harm, 2 * n, 0, st);
    GRX_LAUNCH_CHECK();
    return ms_with_words(W, [&](auto words) {
        return sums_run<decltype(words)::value>(a, ws, d_reach, d_dsum, d_harmonic, st);
    });
}

size_t grx_eccentricity_workspace_bytes(int64_t n, int words, int64_t n_sources)
{
    return grx_carve_bytes(lay_out, n, choose_words(n, words, n_sources), false);
}

int grx_eccentricity(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                     int64_t n_hub_rows, int lanes_per_row, const int32_t *d_sources, int64_t n_sources, int words,
                     int32_t *d_source_ecc, int64_t *d_reach, int32_t *d_lower, int32_t *d_upper, int accumulate,
                     void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "grx_eccentricity: n = %lld out of range", (long long)n);
    GRX_REQUIRE(d_row_ptr && d_col && d_reach && d_lower && d_workspace, "grx_eccentricity: null pointer");
    GRX_REQUIRE(n_sources >= 0 && n_sources < (int64_t)1 << 31 && (n_sources == 0 || (d_sources && d_source_ecc)),
                "grx_eccentricity: source list");
    GRX_REQUIRE(words == 0 || valid_words(words), "grx_eccentricity: words must be 0, 1, 2, 4, 8 or 16 (got %d)",
                words);
    GRX_REQUIRE(lanes_per_row >= 1, "grx_eccentricity: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && (n_hub_rows == 0 || d_hub_rows), "grx_eccentricity: hub list");
    GRX_REQUIRE(accumulate == 0 || accumulate == 1, "grx_eccentricity: accumulate must be 0 or 1 (got %d)",
                accumulate);
    const int W = choose_words(n, words, n_sources);
    GrxCarve c(d_workspace);
    const MsWs ws = lay_out(c, n, W, false);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_eccentricity: workspace %zu bytes, need %zu", workspace_bytes,
                c.used);
    hipStream_t st = grx_stream(stream);
    const MsArgs a{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, (int64_t)GRX_HUB_FACTOR * lanes_per_row,
                   d_sources, n_sources};
    if (!accumulate) {
        grx_fill64(reinterpret_cast<uint64_t *>(d_reach), n, 0, st);
        grx_fill32(d_lower, n, 0, st);
        if (d_upper) grx_fill32(d_upper, n, INT32_MAX, st);
    }
    if (n_sources) grx_fill32(d_source_ecc, n_sources, 0, st);
    GRX_LAUNCH_CHECK();
    return ms_with_words(W, [&](auto words) {
        return ec_run<decltype(words)::value>(a, ws, d_source_ecc, d_reach, d_lower, d_upper, st);
    });
}

}  // extern "C"
