// grx_betweenness.hip -- unweighted betweenness centrality for RolX sense making: a batched multi-source restatement of
// networkx 3.4.2's Brandes loops (betweenness.py: _single_source_shortest_path_basic, _accumulate_basic,
// _accumulate_endpoints, _rescale).
//
// A batch holds B sources (B a multiple of 64).  Per-source state is node-major, cell (v, b) = v * B + b: the BFS
// level (int32, -1 = not reached), sigma (fp64 path counts; overwritten by coeff = (1 + delta) / sigma once the node's
// delta is known) and delta (fp64).  One wavefront handles one (row, 64-lane chunk); lane b of the chunk is one
// source, so reading a neighbour's cells is one contiguous 64-lane load.  Rows longer than GRX_HUB_FACTOR *
// lanes_per_row are the CSR's hub list and get a workgroup each; its four wavefronts' partial sums combine in a
// fixed order.
//
// Forward, level l -> l + 1: pull over the IN-adjacency.  An unreached cell gets sigma = sum of sigma(u) over the
//   in-neighbours u at level l (whole numbers below 2^53: exact in any order).  Rows settled in every lane of the
//   chunk are skipped.  The levels run as a device-steered round loop (grx_common.h); the level word ends as the depth.
// Backward, level l = depth .. 1: pull over the OUT-adjacency.  delta(v) = sum over successors w at level l + 1 of
//   sigma(v) * coeff(w), each term networkx's own product; then coeff(v) = (1 + delta(v)) / sigma(v) replaces sigma(v).
// Accumulation: bc[v] adds the sources' contributions one after another in the caller's order (the sources of a
//   batch in lane order, batches in order), so the result has the same bits for every B.  A final kernel
//   multiplies by the scale of _rescale.  No floating-point atomics (the per-lane reach counts are integer adds).
//
// grx_edge_betweenness (networkx's edge_betweenness_centrality, _accumulate_edges, _rescale_e) runs the same forward and
// backward kernels with coeff written to an array of its own (the backward kernels are templated on that), so that
// sigma survives; after the backward loop of a batch one pass over the arcs adds sigma(v) * coeff(w) -- the term the
// backward pass formed -- of every DAG arc v -> w onto the arc's slot.  One wavefront per row (hub rows: a workgroup,
// its four wavefronts take every fourth arc), the lanes are the batch's sources, so a slot is written by one wavefront
// and every read of level, sigma and coeff is one contiguous load.  The order of the additions is that of
// grx_edge_sum.h: a fixed tree over each aligned group of 16 consecutive sources, the groups one after another in
// source order -- the same bits for every B.  The unused lanes of a partial batch (BW_IDLE) hold +0.0.  Undirected: the
// edge is the sum of its two arc slots, taken by grx_edge_sum.h's final passes together with the scale of _rescale_e.
//
// Compiled with -ffp-contract=off (Makefile; the pragma carries it with the file): every product and sum is its own
// IEEE operation, as in networkx.
#pragma clang fp contract(off)

#include "grx_common.h"
#include "grx_edge_sum.h"

#include <algorithm>

namespace {

constexpr int BW_BLOCK = 256;
constexpr int BW_WAVES = BW_BLOCK / GRX_WAVE;
constexpr int BW_MAX_BATCH = 256;
constexpr int BW_LEVEL_BATCH = 8;                            // forward levels enqueued between two read-backs
constexpr int BW_MAX_ROW_BLOCKS = 1024;
constexpr int BW_MAX_BLOCKS = 2048;                           // grid of the per-element launches
constexpr size_t BW_DEFAULT_STATE_BYTES = (size_t)4 << 30;   // state budget of the library's choice of B

constexpr int32_t BW_IDLE = 0x7fffffff;

// B of batch = 0: the widest multiple of 64 up to 256 whose state fits BW_DEFAULT_STATE_BYTES (at least 64, so above
// ~3.35 M nodes the state is 20 n 64 bytes, more than the budget), and no wider than the source list
// (grx_edge_betweenness: 28 bytes per cell, coeff has an array of its own)
int choose_batch(int64_t n, int batch, int64_t n_sources, bool keep_sigma = false)
{
    if (batch > 0) return batch;
    // level 4 + sigma 8 + delta 8 (+ coeff 8) bytes per (node, source)
    const size_t per_lane = (size_t)(n > 0 ? n : 1) * (keep_sigma ? 28 : 20);
    const int64_t b = (int64_t)(BW_DEFAULT_STATE_BYTES / per_lane) / GRX_WAVE * GRX_WAVE;
    const int64_t widest = std::max<int64_t>(GRX_WAVE, std::min<int64_t>(b, BW_MAX_BATCH));
    const int64_t needed = std::max<int64_t>(GRX_WAVE, grx_ceil_div(n_sources, GRX_WAVE) * GRX_WAVE);
    return (int)std::min<int64_t>(widest, needed);
}

size_t ws_bytes(int64_t n, int B, bool keep_sigma = false)
{
    const size_t cells = (size_t)(n > 0 ? n : 1) * (size_t)B;
    return grx_align_up(cells * 4, 256) + (keep_sigma ? 3 : 2) * grx_align_up(cells * 8, 256) +
           grx_align_up((size_t)B * 4, 256) + 256;
}

struct BwWs {
    int32_t *level;
    double *sigma, *delta;
    double *coeff;                                           // grx_edge_betweenness only; otherwise coeff replaces sigma
    int32_t *reach, *ctrl;
};

BwWs carve(void *base, int64_t n, int B, bool keep_sigma = false)
{
    const size_t cells = (size_t)(n > 0 ? n : 1) * (size_t)B;
    char *p = reinterpret_cast<char *>(base);
    BwWs w;
    w.level = reinterpret_cast<int32_t *>(p); p += grx_align_up(cells * 4, 256);
    w.sigma = reinterpret_cast<double *>(p); p += grx_align_up(cells * 8, 256);
    w.delta = reinterpret_cast<double *>(p); p += grx_align_up(cells * 8, 256);
    w.coeff = nullptr;
    if (keep_sigma) { w.coeff = reinterpret_cast<double *>(p); p += grx_align_up(cells * 8, 256); }
    w.reach = reinterpret_cast<int32_t *>(p); p += grx_align_up((size_t)B * 4, 256);
    w.ctrl = reinterpret_cast<int32_t *>(p);
    return w;
}

// -1 (not reached) in the lanes of the batch's sources, BW_IDLE in the unused lanes of a last, partial batch (settled
// for the row skips, never equal to a level)
__global__ __launch_bounds__(BW_BLOCK) void bw_level_init_kernel(int64_t cells, int B, int count,
                                                                 int32_t *__restrict__ level)
{
    for (int64_t i = (int64_t)blockIdx.x * BW_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * BW_BLOCK)
        level[i] = (int)(i % B) < count ? -1 : BW_IDLE;
}

// lane b < count: source s_b at level 0 with sigma 1 (networkx: sigma[s] = 1.0, D[s] = 0); reach = len(S) so far
__global__ __launch_bounds__(BW_BLOCK) void bw_source_init_kernel(int64_t n, int B, int count,
                                                                  const int32_t *__restrict__ src,
                                                                  int32_t *__restrict__ level,
                                                                  double *__restrict__ sigma,
                                                                  int32_t *__restrict__ reach,
                                                                  int32_t *__restrict__ ctrl)
{
    const int b = threadIdx.x;
    if (b < B) {
        reach[b] = b < count ? 1 : 0;
        if (b < count && src[b] >= 0 && src[b] < n) {       // an id outside [0, n) is never written through
            const int64_t cell = (int64_t)src[b] * B + b;
            level[cell] = 0;
            sigma[cell] = 1.0;
        }
    }
    if (b == 0) { ctrl[GRX_CT_DONE] = 0; ctrl[GRX_CT_LEVEL] = 0; ctrl[GRX_CT_FOUND] = 0; }
}

// sigma(v) of one lane pulled over arcs [b, e) with stride `step` (in-neighbours u at level l); whole numbers
__device__ __forceinline__ double pull_sigma(int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                             const int32_t *__restrict__ level, const double *__restrict__ sigma,
                                             int B, int off, int l)
{
    double acc = 0.0;
    int64_t j = b;
    for (; j + 3 * step < e; j += 4 * step) {
        const int64_t u0 = col[j], u1 = col[j + step], u2 = col[j + 2 * step], u3 = col[j + 3 * step];
        const int l0 = level[u0 * B + off], l1 = level[u1 * B + off];
        const int l2 = level[u2 * B + off], l3 = level[u3 * B + off];
        const double s0 = l0 == l ? sigma[u0 * B + off] : 0.0;
        const double s1 = l1 == l ? sigma[u1 * B + off] : 0.0;
        const double s2 = l2 == l ? sigma[u2 * B + off] : 0.0;
        const double s3 = l3 == l ? sigma[u3 * B + off] : 0.0;
        acc += s0;
        acc += s1;
        acc += s2;
        acc += s3;
    }
    for (; j < e; j += step) {
        const int64_t u = col[j];
        if (level[u * B + off] == l) acc += sigma[u * B + off];
    }
    return acc;
}

// delta(v) of one lane over arcs [b, e) with stride `step`: successors w at level l + 1, terms sigma(v) * coeff(w)
// added in arc order (networkx adds them in the reverse order of S; only that order differs)
__device__ __forceinline__ double pull_delta(int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                             const int32_t *__restrict__ level, const double *__restrict__ coeff,
                                             int B, int off, int l1, double sv)
{
    double acc = 0.0;
    int64_t j = b;
    for (; j + 3 * step < e; j += 4 * step) {
        const int64_t w0 = col[j], w1 = col[j + step], w2 = col[j + 2 * step], w3 = col[j + 3 * step];
        const int a0 = level[w0 * B + off], a1 = level[w1 * B + off];
        const int a2 = level[w2 * B + off], a3 = level[w3 * B + off];
        const double c0 = a0 == l1 ? coeff[w0 * B + off] : 0.0;
        const double c1 = a1 == l1 ? coeff[w1 * B + off] : 0.0;
        const double c2 = a2 == l1 ? coeff[w2 * B + off] : 0.0;
        const double c3 = a3 == l1 ? coeff[w3 * B + off] : 0.0;
        if (a0 == l1) acc += sv * c0;
        if (a1 == l1) acc += sv * c1;
        if (a2 == l1) acc += sv * c2;
        if (a3 == l1) acc += sv * c3;
    }
    for (; j < e; j += step) {
        const int64_t w = col[j];
        if (level[w * B + off] == l1) acc += sv * coeff[w * B + off];
    }
    return acc;
}

// forward, rows up to hub_degree arcs: one wavefront per (row, chunk blockIdx.y)
__global__ __launch_bounds__(BW_BLOCK) void bw_forward_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col, int64_t hub_degree,
                                                              int B, int32_t *__restrict__ level,
                                                              double *__restrict__ sigma,
                                                              int32_t *__restrict__ reach,
                                                              int32_t *__restrict__ ctrl)
{
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    const int lane = threadIdx.x % GRX_WAVE;
    const int off = blockIdx.y * GRX_WAVE + lane;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GRX_WAVE);
    int found = 0;
    for (int64_t v = (int64_t)blockIdx.x * BW_WAVES + wave; v < n; v += (int64_t)gridDim.x * BW_WAVES) {
        const int64_t cell = v * B + off;
        const bool open = level[cell] < 0;
        if (!__ballot(open)) continue;                      // settled in every lane of the chunk
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_degree) continue;                   // bw_forward_hub_kernel
        const double acc = pull_sigma(b, e, 1, col, level, sigma, B, off, l);
        if (open && acc != 0.0) {
            level[cell] = l + 1;
            sigma[cell] = acc;
            ++found;
        }
    }
    if (found) atomicAdd(&reach[off], found);
    if (__ballot(found != 0) && lane == 0) ctrl[GRX_CT_FOUND] = 1;
}

// forward, hub rows: one workgroup per (hub row, chunk); the four wavefronts take every fourth arc
__global__ __launch_bounds__(BW_BLOCK) void bw_forward_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                  const int32_t *__restrict__ col,
                                                                  const int32_t *__restrict__ hub_rows, int B,
                                                                  int32_t *__restrict__ level,
                                                                  double *__restrict__ sigma,
                                                                  int32_t *__restrict__ reach,
                                                                  int32_t *__restrict__ ctrl)
{
    __shared__ double part[BW_WAVES][GRX_WAVE];
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    const int lane = threadIdx.x % GRX_WAVE, wave = threadIdx.x / GRX_WAVE;
    const int off = blockIdx.y * GRX_WAVE + lane;
    const int64_t v = hub_rows[blockIdx.x];
    const int64_t cell = v * B + off;
    const bool open = level[cell] < 0;
    if (!__ballot(open)) return;                            // the same in every wavefront of the workgroup
    const int64_t b = row_ptr[v], e = row_ptr[v + 1];
    part[wave][lane] = pull_sigma(b + wave, e, BW_WAVES, col, level, sigma, B, off, l);
    __syncthreads();
    if (wave != 0) return;
    const double acc = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const bool hit = open && acc != 0.0;
    if (hit) {
        level[cell] = l + 1;
        sigma[cell] = acc;
        atomicAdd(&reach[off], 1);
    }
    if (__ballot(hit) && lane == 0) ctrl[GRX_CT_FOUND] = 1;
}

// networkx _accumulate_*: coeff = (1 + delta[w]) / sigma[w]; delta[v] += sigma[v] * coeff
__device__ __forceinline__ void settle(int64_t cell, double d, double sv, double *__restrict__ coeff,
                                       double *__restrict__ delta)
{
    delta[cell] = d;
    coeff[cell] = (1.0 + d) / sv;                            // coeff(v) for the level above
}

// backward, level l: cells at level l pull delta from their successors at l + 1; one wavefront per (row, chunk).
// KEEP_SIGMA = false: coeff replaces sigma in place (kept_coeff is not read); true: coeff goes to kept_coeff
template <bool KEEP_SIGMA>
__global__ __launch_bounds__(BW_BLOCK) void bw_backward_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ col, int64_t hub_degree,
                                                               int B, int l, const int32_t *__restrict__ level,
                                                               double *__restrict__ sigma,
                                                               double *__restrict__ kept_coeff,
                                                               double *__restrict__ delta)
{
    double *coeff = KEEP_SIGMA ? kept_coeff : sigma;
    const int lane = threadIdx.x % GRX_WAVE;
    const int off = blockIdx.y * GRX_WAVE + lane;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GRX_WAVE);
    for (int64_t v = (int64_t)blockIdx.x * BW_WAVES + wave; v < n; v += (int64_t)gridDim.x * BW_WAVES) {
        const int64_t cell = v * B + off;
        const bool mine = level[cell] == l;
        if (!__ballot(mine)) continue;
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_degree) continue;                   // bw_backward_hub_kernel
        const double sv = mine ? sigma[cell] : 1.0;
        const double d = pull_delta(b, e, 1, col, level, coeff, B, off, l + 1, sv);
        if (mine) settle(cell, d, sv, coeff, delta);
    }
}

template <bool KEEP_SIGMA>
__global__ __launch_bounds__(BW_BLOCK) void bw_backward_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                   const int32_t *__restrict__ col,
                                                                   const int32_t *__restrict__ hub_rows, int B, int l,
                                                                   const int32_t *__restrict__ level,
                                                                   double *__restrict__ sigma,
                                                                   double *__restrict__ kept_coeff,
                                                                   double *__restrict__ delta)
{
    __shared__ double part[BW_WAVES][GRX_WAVE];
    double *coeff = KEEP_SIGMA ? kept_coeff : sigma;
    const int lane = threadIdx.x % GRX_WAVE, wave = threadIdx.x / GRX_WAVE;
    const int off = blockIdx.y * GRX_WAVE + lane;
    const int64_t v = hub_rows[blockIdx.x];
    const int64_t cell = v * B + off;
    const bool mine = level[cell] == l;
    if (!__ballot(mine)) return;
    const int64_t b = row_ptr[v], e = row_ptr[v + 1];
    const double sv = mine ? sigma[cell] : 1.0;
    part[wave][lane] = pull_delta(b + wave, e, BW_WAVES, col, level, coeff, B, off, l + 1, sv);
    __syncthreads();
    if (wave != 0 || !mine) return;
    settle(cell, ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane], sv, coeff, delta);
}

// bc[v] += the contributions of the batch's sources in lane order (networkx: betweenness[w] += delta[w] for w != s;
// with endpoints betweenness[s] += len(S) - 1 and betweenness[w] += delta[w] + 1)
__global__ __launch_bounds__(BW_BLOCK) void bw_accumulate_kernel(int64_t n, int B, int count, int endpoints,
                                                                 const int32_t *__restrict__ level,
                                                                 const double *__restrict__ delta,
                                                                 const int32_t *__restrict__ reach,
                                                                 double *__restrict__ bc)
{
    for (int64_t v = (int64_t)blockIdx.x * BW_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * BW_BLOCK) {
        const int32_t *lv = level + v * B;
        const double *dv = delta + v * B;
        double acc = bc[v];
        for (int b = 0; b < count; ++b) {
            const int l = lv[b];
            if (l > 0 && l != BW_IDLE) acc += endpoints ? dv[b] + 1.0 : dv[b];
            else if (l == 0 && endpoints) acc += (double)(reach[b] - 1);
        }
        bc[v] = acc;
    }
}

__global__ __launch_bounds__(BW_BLOCK) void bw_scale_kernel(int64_t n, double scale, double *__restrict__ bc)
{
    for (int64_t v = (int64_t)blockIdx.x * BW_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * BW_BLOCK)
        bc[v] *= scale;
}


// grx_edge_betweenness, after the backward loop of a batch: the arcs [b, e) with stride `step` of row v, the wavefront's
// lanes being the sources of one 64-lane chunk after another.  Lane `off` holds sigma(v) * coeff(w) when v -> w is an
// arc of its source's BFS DAG (level(w) == level(v) + 1) and +0.0 otherwise; grx_edge_sum.h's order adds them onto the
// slot.  A slot is read and written by lane 0 of the one wavefront that owns it.
__device__ __forceinline__ void edge_row(int64_t v, int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                         const int32_t *__restrict__ level, const double *__restrict__ sigma,
                                         const double *__restrict__ coeff, int B, int lane, double *__restrict__ ebc)
{
    for (int64_t j = b; j < e; j += step) {
        const int64_t w = col[j];
        double acc = 0.0;
        bool any = false;
        for (int off = lane; off < B; off += GRX_WAVE) {
            const int lv = level[v * B + off];
            const bool on = lv >= 0 && lv != BW_IDLE && level[w * B + off] == lv + 1;
            if (!__ballot(on)) continue;                    // 64 times +0.0
            if (!any && lane == 0) acc = ebc[j];
            any = true;
            acc = eb_add_groups<GRX_WAVE>(acc, on ? sigma[v * B + off] * coeff[w * B + off] : 0.0, 0);
        }
        if (any && lane == 0) ebc[j] = acc;
    }
}

// rows up to hub_degree arcs: one wavefront per row
__global__ __launch_bounds__(BW_BLOCK) void bw_edge_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col, int64_t hub_degree, int B,
                                                           const int32_t *__restrict__ level,
                                                           const double *__restrict__ sigma,
                                                           const double *__restrict__ coeff, double *__restrict__ ebc)
{
    const int lane = threadIdx.x % GRX_WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GRX_WAVE);
    for (int64_t v = (int64_t)blockIdx.x * BW_WAVES + wave; v < n; v += (int64_t)gridDim.x * BW_WAVES) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_degree) continue;                   // bw_edge_hub_kernel
        edge_row(v, b, e, 1, col, level, sigma, coeff, B, lane, ebc);
    }
}

// hub rows: one workgroup per hub row; the four wavefronts take every fourth arc (a slot still has one owner)
__global__ __launch_bounds__(BW_BLOCK) void bw_edge_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ col,
                                                               const int32_t *__restrict__ hub_rows, int B,
                                                               const int32_t *__restrict__ level,
                                                               const double *__restrict__ sigma,
                                                               const double *__restrict__ coeff,
                                                               double *__restrict__ ebc)
{
    const int lane = threadIdx.x % GRX_WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GRX_WAVE);
    const int64_t v = hub_rows[blockIdx.x];
    edge_row(v, row_ptr[v] + wave, row_ptr[v + 1], BW_WAVES, col, level, sigma, coeff, B, lane, ebc);
}

// Both entry points: EDGES = false is grx_betweenness (d_out = bc, one value per node), true is grx_edge_betweenness
// (d_out = ebc, one value per arc of the out CSR; `endpoints` is not read)
template <bool EDGES>
int run(const char *name, int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
        int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
        const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row, const int32_t *d_sources,
        int64_t n_sources, int endpoints, double scale, int batch, double *d_out, void *d_workspace,
        size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "%s: n = %lld out of range", name, (long long)n);
    GRX_REQUIRE(d_row_ptr && d_col && d_out && d_workspace, "%s: null pointer", name);
    GRX_REQUIRE(n_sources >= 0 && (n_sources == 0 || d_sources), "%s: source list", name);
    GRX_REQUIRE(batch == 0 || (batch > 0 && batch <= BW_MAX_BATCH && batch % GRX_WAVE == 0),
                "%s: batch must be 0 or a multiple of 64 up to %d (got %d)", name, BW_MAX_BATCH, batch);
    const bool directed = d_in_row_ptr != nullptr;
    GRX_REQUIRE(!directed || d_in_col, "%s: d_in_col is required with d_in_row_ptr", name);
    if (!directed) {                                         // undirected: the CSR is its own in-adjacency
        d_in_col = d_col;
        d_in_hub_rows = d_hub_rows;
        n_in_hub_rows = n_hub_rows;
        in_lanes_per_row = lanes_per_row;
    }
    GRX_REQUIRE(lanes_per_row >= 1 && in_lanes_per_row >= 1, "%s: lanes_per_row must be >= 1", name);
    GRX_REQUIRE(n_hub_rows >= 0 && (n_hub_rows == 0 || d_hub_rows) && n_in_hub_rows >= 0 &&
                    (n_in_hub_rows == 0 || d_in_hub_rows), "%s: hub list", name);
    const int B = choose_batch(n, batch, n_sources, EDGES);
    GRX_REQUIRE(workspace_bytes >= ws_bytes(n, B, EDGES), "%s: workspace %zu bytes, need %zu", name, workspace_bytes,
                ws_bytes(n, B, EDGES));
    hipStream_t st = grx_stream(stream);
    const BwWs ws = carve(d_workspace, n, B, EDGES);
    const int chunks = B / GRX_WAVE;
    const unsigned egrid = grx_grid(n, BW_BLOCK, BW_MAX_BLOCKS);
    const unsigned row_blocks = grx_grid(n, BW_WAVES, BW_MAX_ROW_BLOCKS);
    const dim3 row_grid(row_blocks, (unsigned)chunks);
    const int64_t out_hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    const int64_t in_hub_degree = (int64_t)GRX_HUB_FACTOR * in_lanes_per_row;
    const int64_t cells = n * (int64_t)B;
    const int64_t *in_rp = directed ? d_in_row_ptr : d_row_ptr;

    if (EDGES) eb_rows<EB_ZERO>(n, d_row_ptr, d_col, 0.0, d_out, st);
    else grx_fill64(reinterpret_cast<uint64_t *>(d_out), n, 0, st);
    GRX_LAUNCH_CHECK();
    for (int64_t first = 0; first < n_sources; first += B) {
        const int count = (int)std::min<int64_t>(B, n_sources - first);
        bw_level_init_kernel<<<grx_grid(cells, BW_BLOCK, BW_MAX_BLOCKS), BW_BLOCK, 0, st>>>(cells, B, count, ws.level);
        bw_source_init_kernel<<<1, BW_MAX_BATCH, 0, st>>>(n, B, count, d_sources + first, ws.level, ws.sigma, ws.reach,
                                                          ws.ctrl);
        GRX_LAUNCH_CHECK();
        int32_t h[2];
        // a BFS has at most n levels; one more launch finds the empty frontier
        const int rc = grx_run_rounds(
            EDGES ? "grx_edge_betweenness: the forward pass did not end after %lld levels"
                  : "grx_betweenness: the forward pass did not end after %lld levels",
            BW_LEVEL_BATCH, n + 1, 2, ws.ctrl, h, st, [&] {
                if (n_in_hub_rows)
                    bw_forward_hub_kernel<<<dim3((unsigned)n_in_hub_rows, (unsigned)chunks), BW_BLOCK, 0, st>>>(
                        in_rp, d_in_col, d_in_hub_rows, B, ws.level, ws.sigma, ws.reach, ws.ctrl);
                bw_forward_kernel<<<row_grid, BW_BLOCK, 0, st>>>(n, in_rp, d_in_col, in_hub_degree, B, ws.level,
                                                                 ws.sigma, ws.reach, ws.ctrl);
                return grx_frontier_advance(ws.ctrl, st);
            });
        if (rc != GRX_OK) return rc;
        for (int l = h[GRX_CT_LEVEL]; l >= 1; --l) {        // deepest level first; the sources need no delta
            if (n_hub_rows)
                bw_backward_hub_kernel<EDGES><<<dim3((unsigned)n_hub_rows, (unsigned)chunks), BW_BLOCK, 0, st>>>(
                    d_row_ptr, d_col, d_hub_rows, B, l, ws.level, ws.sigma, ws.coeff, ws.delta);
            bw_backward_kernel<EDGES><<<row_grid, BW_BLOCK, 0, st>>>(n, d_row_ptr, d_col, out_hub_degree, B, l,
                                                                     ws.level, ws.sigma, ws.coeff, ws.delta);
            GRX_LAUNCH_CHECK();
        }
        if (EDGES) {
            if (n_hub_rows)
                bw_edge_hub_kernel<<<(unsigned)n_hub_rows, BW_BLOCK, 0, st>>>(d_row_ptr, d_col, d_hub_rows, B, ws.level,
                                                                              ws.sigma, ws.coeff, d_out);
            bw_edge_kernel<<<row_blocks, BW_BLOCK, 0, st>>>(n, d_row_ptr, d_col, out_hub_degree, B, ws.level, ws.sigma,
                                                            ws.coeff, d_out);
        } else {
            bw_accumulate_kernel<<<egrid, BW_BLOCK, 0, st>>>(n, B, count, endpoints, ws.level, ws.delta, ws.reach,
                                                             d_out);
        }
        GRX_LAUNCH_CHECK();
    }
    if (EDGES) eb_finish(n, d_row_ptr, d_col, directed, scale, d_out, st);
    else bw_scale_kernel<<<egrid, BW_BLOCK, 0, st>>>(n, scale, d_out);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // namespace

extern "C" {

size_t grx_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return ws_bytes(n, choose_batch(n, batch, n_sources));
}

int grx_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                    int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                    const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                    const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, int batch, double *d_bc,
                    void *d_workspace, size_t workspace_bytes, void *stream)
{
    return run<false>("grx_betweenness", n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row, d_in_row_ptr,
                      d_in_col, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources, n_sources, endpoints, scale,
                      batch, d_bc, d_workspace, workspace_bytes, stream);
}

size_t grx_edge_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return ws_bytes(n, choose_batch(n, batch, n_sources, true), true);
}

int grx_edge_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                         int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                         const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                         const int32_t *d_sources, int64_t n_sources, double scale, int batch, double *d_ebc,
                         void *d_workspace, size_t workspace_bytes, void *stream)
{
    return run<true>("grx_edge_betweenness", n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row, d_in_row_ptr,
                     d_in_col, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources, n_sources, 0, scale, batch,
                     d_ebc, d_workspace, workspace_bytes, stream);
}

}  // extern "C"
