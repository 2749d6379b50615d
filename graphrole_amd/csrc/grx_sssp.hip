// grx_sssp.hip -- weighted shortest-path distances for RolX sense making: what networkx 3.4.2's
// single_source_dijkstra_path_length(G, s, weight) returns for many sources at once, and from it the per-target sums
// behind closeness_centrality(G, distance=...) and harmonic_centrality(G, distance=...) and the per-source maximum
// behind eccentricity(G, weight=...), by a batched Bellman-Ford relaxation.
//
// Why no priority queue: with weights >= 0 networkx's Dijkstra (dist[v] + cost in fp64) returns for every node the
// minimum over the paths of the left-to-right fp64 sum of the arc weights -- rounding is monotone and fl(d + w) >= d,
// so a longer prefix never sums to less.  That value is also the one fixed point every relaxation from +inf reaches,
// in whatever order the relaxations run: the distances below are networkx's, bit for bit, for every batch width,
// schedule and run.
//
// A batch holds S sources, S = 16, 32 or 64.  dist is fp64, node-major (source lane b of node v at v * S + b): S lanes
// handle one node, lane b its source b, and reading a neighbour's distances is one contiguous 8 S-byte load.  One
// round pulls over the CSR it is given:
//   new(v, b) = min(dist(v, b), min over the listed neighbours u of fl(dist(u, b) + w(u -> v))),
// Jacobi style over TWO buffers that swap roles every round: a round reads only what the rounds before it wrote, so
// the number of rounds -- (the most arcs on any lightest path) + 1 -- is as reproducible as the distances are, and no
// reader ever meets a store of its own launch.  (Relaxing in place would halve the state and be just as exact: values
// only decrease, every visible value is the length of a real path, a row has one writer with aligned 8-byte stores,
// and termination is judged across a kernel boundary.  A stale read would cost a round, never correctness -- but the
// round count would then depend on the schedule; two buffers cost 8 n S bytes more and nothing else.)
// stamp(v) is the last round in which any lane of v decreased (round r = level r - 1 of the loop; the sources carry 0,
// every other node -1 at the start).  v stores new(v, .) into the other buffer only when it decreased in this round or
// in the last one (stamp(v) >= r - 1): the second store brings the buffer that missed the decrease up to date, so
// between two decreases a row costs no store at all, and when a round changes nothing both buffers hold the fixed
// point.  Only v's owner reads and writes stamp(v).  Measured against storing every row in every round (no stamp at
// all would be the simpler form): 723 / 726 ms against 730 / 738 ms for 1 024 sources on BA 1 M / m = 10, and 955 ms
// against 1 072 ms on the 1000 x 1000 grid (12 %), where few rows move per round; profiles/weighted_distances.txt.
// MEASURED AND REMOVED: reading a neighbour u only when stamp(u) >= r - 1 (what it held before was relaxed in an
// earlier round).  It turns 8 S gathered bytes per arc into 4 for the arcs whose tail stands still, but every arc pays
// a second scattered load first, and with 64 random sources per batch most tails move in most rounds: 808.7 ms
// against 726.0 ms without it for 1 024 sources on BA 1 M / m = 10 (11 % slower), 929 ms against 962 ms on the
// 1000 x 1000 grid, one batch of 1 993 rounds (3.5 % faster); profiles/weighted_distances.txt.
// A node that decreases stamps itself r and sets the control word GRX_CT_FOUND; a round without one ends the batch
// (device-steered round loop, grx_common.h).  At most n - 1 rounds decrease something, so the loop refuses after
// n + 1: weights outside the contract end in an error, not a hang.  Rows longer than GRX_HUB_FACTOR * lanes_per_row
// are the CSR's hub list and get a workgroup each: its 256 / S lane groups take every (256 / S)-th arc and reduce
// with fmin through LDS (min is order-free).  The relaxation itself -- pull_min, the source initialisation, the round
// and hub-round kernels and the round loop sp_relax -- lives in grx_relax.h, which grx_weighted_betweenness.hip
// includes as well.
//
// After the batch has converged one thread per node walks its S distances in source order and continues the running
// values the batches before left: reach, dsum, harmonic and far are plain left-to-right sums / maxima in the order of
// d_sources, the same bits for every S, with no floating-point atomics.  The eccentricity of source b is a block
// maximum, then an integer atomicMax on the fp64 bit pattern (non-negative doubles order as uint64).
#pragma clang fp contract(off)

#include "grx_relax.h"

#include <algorithm>

namespace {

constexpr int SP_MAX_BLOCKS = 2048;                           // grid of the per-node launches
constexpr size_t SP_DEFAULT_STATE_BYTES = (size_t)4 << 30;   // state budget of the library's choice of S

size_t state_bytes(int64_t n, int S) { return (size_t)(n > 0 ? n : 1) * ((size_t)S * 16 + 4); }

// batch = 0: the widest S whose state (two dist buffers and the stamps) fits SP_DEFAULT_STATE_BYTES, never below 16
// and no wider than the source list rounded up
int choose_batch(int64_t n, int batch, int64_t n_sources)
{
    if (batch > 0) return batch;
    int widest = 16;
    while (widest < 64 && state_bytes(n, widest * 2) <= SP_DEFAULT_STATE_BYTES) widest *= 2;
    int s = 16;
    while (s < widest && s < n_sources) s *= 2;
    return s;
}

struct SpWs {
    double *d0, *d1;
    int32_t *stamp;
    int32_t *ctrl;
};

// the workspace of batch width S, sized (c.base == NULL) and carved by the same walk
SpWs lay_out(GrxCarve &c, int64_t n, int S)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    SpWs ws;
    ws.d0 = c.take<double>(nn * (size_t)S);
    ws.d1 = c.take<double>(nn * (size_t)S);
    ws.stamp = c.take<int32_t>(nn);
    ws.ctrl = c.take<int32_t>(GRX_CTRL_MAX_WORDS);
    return ws;
}

// the converged batch, one thread per node: its `count` distances in source order continue the running values
template <int S>
__global__ __launch_bounds__(SP_BLOCK) void sp_finish_kernel(int64_t n, int count, const int32_t *__restrict__ src,
                                                             const double *__restrict__ D,
                                                             int64_t *__restrict__ reach, double *__restrict__ dsum,
                                                             double *__restrict__ harmonic, double *__restrict__ far)
{
    __shared__ int32_t source[S];
    if (threadIdx.x < S) source[threadIdx.x] = threadIdx.x < count ? src[threadIdx.x] : -1;
    __syncthreads();
    for (int64_t v = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * SP_BLOCK) {
        int64_t r = reach[v];
        double t = dsum[v], h = harmonic[v], f = far[v];
        const double *row = D + v * S;
        for (int b = 0; b < count; ++b) {
            const double d = row[b];
            if (source[b] == v || !(d < SP_INF)) continue;  // the source itself; no path (or an id outside [0, n))
            r += 1;
            t += d;
            if (d > 0.0) h += 1.0 / d;                      // networkx skips the pairs at distance 0
            f = fmax(f, d);
        }
        reach[v] = r;
        dsum[v] = t;
        harmonic[v] = h;
        far[v] = f;
    }
}

// the converged batch, per source lane: ecc[b] = the largest finite dist(., b)
template <int S>
__global__ __launch_bounds__(SP_BLOCK) void sp_source_kernel(int64_t n, int count, const double *__restrict__ D,
                                                             unsigned long long *__restrict__ ecc_bits)
{
    constexpr int GROUPS = SP_BLOCK / S;
    __shared__ double part[SP_BLOCK];
    const int t = threadIdx.x, lane = t % S;
    double m = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * GROUPS + t / S; v < n; v += (int64_t)gridDim.x * GROUPS) {
        const double d = D[v * S + lane];
        if (d < SP_INF) m = fmax(m, d);
    }
    part[t] = m;
    __syncthreads();
#pragma unroll
    for (int s = SP_BLOCK / 2; s >= S; s >>= 1) {
        if (t < s) part[t] = fmax(part[t], part[t + s]);
        __syncthreads();
    }
    // non-negative doubles order as their bit patterns: an integer maximum, the same whatever the order
    if (t < S && t < count && part[t] > 0.0) atomicMax(&ecc_bits[t], (unsigned long long)__double_as_longlong(part[t]));
}

// the converged batch as rows of the source-major distance matrix: 64 nodes x S lanes are read as they lie (one
// contiguous block), turned in LDS (odd row stride: conflict-free), and written 64 consecutive nodes per source
template <int S>
__global__ __launch_bounds__(SP_BLOCK) void sp_matrix_kernel(int64_t n, int count, const double *__restrict__ D,
                                                             double *__restrict__ dist, int64_t ld)
{
    __shared__ double tile[GRX_WAVE][S + 1];
    const int t = threadIdx.x, vo = t % GRX_WAVE;
    // the trip count is the same in every lane of the workgroup
    for (int64_t v0 = (int64_t)blockIdx.x * GRX_WAVE; v0 < n; v0 += (int64_t)gridDim.x * GRX_WAVE) {
        const int rows = (int)std::min<int64_t>(GRX_WAVE, n - v0);
        for (int i = t; i < rows * S; i += SP_BLOCK) tile[i / S][i % S] = D[v0 * S + i];
        __syncthreads();
        if (vo < rows)
            for (int b = t / GRX_WAVE; b < count; b += SP_BLOCK / GRX_WAVE) dist[b * ld + v0 + vo] = tile[vo][b];
        __syncthreads();
    }
}

struct Args {
    int64_t n;
    const int64_t *row_ptr;
    const int32_t *col;
    const double *w;
    const int32_t *hub_rows;
    int64_t n_hub_rows, hub_degree;
    const int32_t *sources;
    int64_t n_sources;
    int64_t *reach;
    double *dsum, *harmonic, *far, *source_ecc, *dist;
    int64_t ld_dist;
};

template <int S>
int run(const Args &a, const SpWs &ws, int64_t *rounds, hipStream_t st)
{
    const int64_t n = a.n;
    const SpPull g{n, a.row_ptr, a.col, a.w, a.hub_rows, a.n_hub_rows, a.hub_degree};
    for (int64_t first = 0; first < a.n_sources; first += S) {
        const int count = (int)std::min<int64_t>(S, a.n_sources - first);
        const int rc = sp_relax<S>(
            g, a.sources + first, count, ws.d0, ws.d1, ws.stamp, ws.ctrl,
            "grx_weighted_distances: the relaxation did not end after %lld rounds (a negative or NaN weight?)",
            GRX_K_SSSP_ROUND, rounds, st);
        if (rc != GRX_OK) return rc;
        // the last round changed nothing: both buffers hold the fixed point
        GRX_PROF(GRX_K_SSSP_FINISH, st);
        sp_finish_kernel<S><<<grx_grid(n, SP_BLOCK, SP_MAX_BLOCKS), SP_BLOCK, 0, st>>>(
            n, count, a.sources + first, ws.d0, a.reach, a.dsum, a.harmonic, a.far);
        sp_source_kernel<S><<<grx_grid(n, SP_BLOCK / S, SP_MAX_BLOCKS), SP_BLOCK, 0, st>>>(
            n, count, ws.d0, reinterpret_cast<unsigned long long *>(a.source_ecc + first));
        if (a.dist)
            sp_matrix_kernel<S><<<grx_grid(n, GRX_WAVE, SP_MAX_BLOCKS), SP_BLOCK, 0, st>>>(
                n, count, ws.d0, a.dist + first * a.ld_dist, a.ld_dist);
        GRX_LAUNCH_CHECK();
    }
    return GRX_OK;
}

}  // namespace

extern "C" {

size_t grx_weighted_distances_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return grx_carve_bytes(lay_out, n, choose_batch(n, sp_valid_batch(batch) ? batch : 0, n_sources));
}

int grx_weighted_distances(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                           const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                           const int32_t *d_sources, int64_t n_sources, int batch, int64_t *d_reach, double *d_dsum,
                           double *d_harmonic, double *d_far, double *d_source_ecc, double *d_dist, int64_t ld_dist,
                           int64_t *h_rounds, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(batch == 0 || sp_valid_batch(batch), "grx_weighted_distances: batch must be 0, 16, 32 or 64 (got %d)",
                batch);
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "grx_weighted_distances: n = %lld out of range", (long long)n);
    GRX_REQUIRE(n_sources >= 0 && n_sources < (int64_t)1 << 31 && (n_sources == 0 || (d_sources && d_source_ecc)),
                "grx_weighted_distances: source list");
    GRX_REQUIRE(!d_dist || ld_dist >= n, "grx_weighted_distances: ld_dist = %lld below n = %lld", (long long)ld_dist,
                (long long)n);
    const int S = choose_batch(n, batch, n_sources);
    GrxCarve c(d_workspace);
    const SpWs ws = lay_out(c, n, S);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_weighted_distances: workspace %zu bytes, need %zu", workspace_bytes,
                c.used);
    GRX_REQUIRE(d_row_ptr && d_col && d_reach && d_dsum && d_harmonic && d_far && d_workspace,
                "grx_weighted_distances: null pointer");
    GRX_REQUIRE(lanes_per_row >= 1, "grx_weighted_distances: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && (n_hub_rows == 0 || d_hub_rows), "grx_weighted_distances: hub list");
    hipStream_t st = grx_stream(stream);
    const Args a{n, d_row_ptr, d_col, d_w, d_hub_rows, n_hub_rows, (int64_t)GRX_HUB_FACTOR * lanes_per_row,
                 d_sources, n_sources, d_reach, d_dsum, d_harmonic, d_far, d_source_ecc, d_dist, ld_dist};
    grx_fill64(reinterpret_cast<uint64_t *>(d_reach), n, 0, st);
    grx_fill64(reinterpret_cast<uint64_t *>(d_dsum), n, 0, st);
    grx_fill64(reinterpret_cast<uint64_t *>(d_harmonic), n, 0, st);
    grx_fill64(reinterpret_cast<uint64_t *>(d_far), n, 0, st);
    if (n_sources) grx_fill64(reinterpret_cast<uint64_t *>(d_source_ecc), n_sources, 0, st);
    GRX_LAUNCH_CHECK();
    int64_t rounds = 0;
    int rc;
    switch (S) {
    case 16: rc = run<16>(a, ws, &rounds, st); break;
    case 32: rc = run<32>(a, ws, &rounds, st); break;
    default: rc = run<64>(a, ws, &rounds, st); break;
    }
    if (h_rounds) *h_rounds = rounds;
    return rc;
}

}  // extern "C"
