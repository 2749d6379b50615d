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
// Accumulation (grx_brandes.h): bc[v] adds the sources' contributions one after another in the caller's order (the
//   sources of a batch in lane order, batches in order), so the result has the same bits for every B.  A final kernel
//   multiplies by the scale of _rescale.  No floating-point atomics (the per-lane reach counts are integer adds).
// The argument checks, the per-batch sequence of these passes and the finish are br_open and br_run of grx_brandes.h,
// shared with grx_weighted_betweenness.hip; BwSide below is what this file hands them.
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

#include "grx_brandes.h"

namespace {

constexpr int BW_BLOCK = 256;
constexpr int BW_WAVES = BW_BLOCK / GRX_WAVE;
static_assert(BW_WAVES == BR_PARTS, "a hub workgroup's wavefronts are the parts br_combine4 adds");
constexpr int BW_MAX_BATCH = 256;
constexpr int BW_MAX_ROW_BLOCKS = 1024;
constexpr int BW_MAX_BLOCKS = 2048;                           // grid of the per-element launches
constexpr size_t BW_DEFAULT_STATE_BYTES = (size_t)4 << 30;   // state budget of the library's choice of B

constexpr int32_t BW_IDLE = 0x7fffffff;

// The workspace, laid out once: level (int32), sigma and delta (fp64) per (node, source) -- 20 bytes a cell; coeff
// (fp64) in an array of its own for grx_edge_betweenness only, 28 bytes a cell (otherwise coeff replaces sigma); the
// per-lane reach counts and the control words
struct BwWs {
    BrLayout lay;
    int32_t *level;
    double *sigma, *delta, *coeff;
    int32_t *reach, *ctrl;
    BwWs(void *base, int64_t n, int B, bool keep_sigma) : lay(base, n, B)
    {
        level = lay.per_cell<int32_t>();
        sigma = lay.per_cell<double>();
        delta = lay.per_cell<double>();
        coeff = keep_sigma ? lay.per_cell<double>() : nullptr;
        reach = lay.take<int32_t>(B);
        ctrl = lay.take<int32_t>(GRX_CTRL_MAX_WORDS);
    }
    size_t bytes() const { return lay.used; }
};

// B of batch = 0: the widest multiple of 64 up to 256 whose state fits BW_DEFAULT_STATE_BYTES (at least 64, so above
// ~3.35 M nodes the state is 20 n 64 bytes, more than the budget), and no wider than the source list
int choose_batch(int64_t n, int batch, int64_t n_sources, bool keep_sigma)
{
    if (batch > 0) return batch;
    const size_t per_lane = (size_t)(n > 0 ? n : 1) * BwWs(nullptr, n, GRX_WAVE, keep_sigma).lay.cell_bytes;
    const int64_t b = (int64_t)(BW_DEFAULT_STATE_BYTES / per_lane) / GRX_WAVE * GRX_WAVE;
    const int64_t widest = std::max<int64_t>(GRX_WAVE, std::min<int64_t>(b, BW_MAX_BATCH));
    const int64_t needed = std::max<int64_t>(GRX_WAVE, grx_ceil_div(n_sources, GRX_WAVE) * GRX_WAVE);
    return (int)std::min<int64_t>(widest, needed);
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
    const double acc = br_combine4(part, lane);
    const bool hit = open && acc != 0.0;
    if (hit) {
        level[cell] = l + 1;
        sigma[cell] = acc;
        atomicAdd(&reach[off], 1);
    }
    if (__ballot(hit) && lane == 0) ctrl[GRX_CT_FOUND] = 1;
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
        if (mine) br_settle(cell, d, sv, coeff, delta);
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
    br_settle(cell, br_combine4(part, lane), sv, coeff, delta);
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

// What br_run drives: the carved state of one call.  EDGES = false is grx_betweenness, true is grx_edge_betweenness
template <bool EDGES>
struct BwSide {
    int64_t n;
    SpPull out, in;                                          // backward and the edge pass pull over `out`, forward over `in`
    bool directed;
    int B;
    BwWs ws;
    hipStream_t st;

    unsigned chunks() const { return (unsigned)(B / GRX_WAVE); }
    unsigned row_blocks() const { return grx_grid(n, BW_WAVES, BW_MAX_ROW_BLOCKS); }
    static const char *forward_refusal()
    {
        return EDGES ? "grx_edge_betweenness: the forward pass did not end after %lld levels"
                     : "grx_betweenness: the forward pass did not end after %lld levels";
    }
    int begin(const int32_t *d_src, int count) const
    {
        const int64_t cells = n * (int64_t)B;
        bw_level_init_kernel<<<grx_grid(cells, BW_BLOCK, BW_MAX_BLOCKS), BW_BLOCK, 0, st>>>(cells, B, count, ws.level);
        bw_source_init_kernel<<<1, BW_MAX_BATCH, 0, st>>>(n, B, count, d_src, ws.level, ws.sigma, ws.reach, ws.ctrl);
        return GRX_OK;
    }
    int forward_round() const
    {
        if (in.n_hub_rows)
            bw_forward_hub_kernel<<<dim3((unsigned)in.n_hub_rows, chunks()), BW_BLOCK, 0, st>>>(
                in.row_ptr, in.col, in.hub_rows, B, ws.level, ws.sigma, ws.reach, ws.ctrl);
        bw_forward_kernel<<<dim3(row_blocks(), chunks()), BW_BLOCK, 0, st>>>(n, in.row_ptr, in.col, in.hub_degree, B,
                                                                             ws.level, ws.sigma, ws.reach, ws.ctrl);
        return grx_frontier_advance(ws.ctrl, st);
    }
    void after_forward(int) const {}                         // the forward kernels counted reach
    void backward(int l) const
    {
        if (out.n_hub_rows)
            bw_backward_hub_kernel<EDGES><<<dim3((unsigned)out.n_hub_rows, chunks()), BW_BLOCK, 0, st>>>(
                out.row_ptr, out.col, out.hub_rows, B, l, ws.level, ws.sigma, ws.coeff, ws.delta);
        bw_backward_kernel<EDGES><<<dim3(row_blocks(), chunks()), BW_BLOCK, 0, st>>>(
            n, out.row_ptr, out.col, out.hub_degree, B, l, ws.level, ws.sigma, ws.coeff, ws.delta);
    }
    void edge_pass(double *d_ebc) const
    {
        if (out.n_hub_rows)
            bw_edge_hub_kernel<<<(unsigned)out.n_hub_rows, BW_BLOCK, 0, st>>>(out.row_ptr, out.col, out.hub_rows, B,
                                                                              ws.level, ws.sigma, ws.coeff, d_ebc);
        bw_edge_kernel<<<row_blocks(), BW_BLOCK, 0, st>>>(n, out.row_ptr, out.col, out.hub_degree, B, ws.level,
                                                          ws.sigma, ws.coeff, d_ebc);
    }
    const int32_t *level() const { return ws.level; }
    int stride() const { return B; }
};

// the argument checks and the batches of both entry points (d_out = bc resp. ebc; `endpoints` is 0 for the edges)
template <bool EDGES>
int entry(const char *name, int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
          int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
          const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row, const int32_t *d_sources,
          int64_t n_sources, int endpoints, double scale, int batch, double *d_out, void *d_workspace,
          size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(batch == 0 || (batch > 0 && batch <= BW_MAX_BATCH && batch % GRX_WAVE == 0),
                "%s: batch must be 0 or a multiple of 64 up to %d (got %d)", name, BW_MAX_BATCH, batch);
    const int B = choose_batch(n, batch, n_sources, EDGES);
    BwSide<EDGES> side{n, {}, {}, false, B, BwWs(d_workspace, n, B, EDGES), grx_stream(stream)};
    const int rc = br_open(name, n, d_row_ptr, d_col, nullptr, d_hub_rows, n_hub_rows, lanes_per_row, d_in_row_ptr,
                           d_in_col, nullptr, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources, n_sources,
                           d_out, d_workspace, workspace_bytes, side.ws.bytes(), side.out, side.in, side.directed);
    if (rc != GRX_OK) return rc;
    return br_run<EDGES>(side, d_sources, n_sources, endpoints, scale, d_out, side.st);
}

}  // namespace

extern "C" {

size_t grx_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return BwWs(nullptr, n, choose_batch(n, batch, n_sources, false), false).bytes();
}

int grx_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                    int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                    const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                    const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, int batch, double *d_bc,
                    void *d_workspace, size_t workspace_bytes, void *stream)
{
    return entry<false>("grx_betweenness", n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row, d_in_row_ptr,
                        d_in_col, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources, n_sources, endpoints,
                        scale, batch, d_bc, d_workspace, workspace_bytes, stream);
}

size_t grx_edge_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return BwWs(nullptr, n, choose_batch(n, batch, n_sources, true), true).bytes();
}

int grx_edge_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                         int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                         const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                         const int32_t *d_sources, int64_t n_sources, double scale, int batch, double *d_ebc,
                         void *d_workspace, size_t workspace_bytes, void *stream)
{
    return entry<true>("grx_edge_betweenness", n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row,
                       d_in_row_ptr, d_in_col, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources, n_sources, 0,
                       scale, batch, d_ebc, d_workspace, workspace_bytes, stream);
}

}  // extern "C"
