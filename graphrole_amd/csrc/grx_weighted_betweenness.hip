// grx_weighted_betweenness.hip -- betweenness centrality over shortest paths by arc weight for RolX sense making: a
// batched multi-source restatement of networkx 3.4.2's weighted Brandes loops (betweenness.py:
// _single_source_dijkstra_path_basic, _accumulate_basic, _accumulate_endpoints, _rescale) without a priority queue.
//
// Why no queue: networkx's Dijkstra settles nodes by the left-to-right fp64 sum of the arc weights and calls two paths
// equally short when those sums are EQUAL as doubles.  The relaxation of grx_relax.h (grx_sssp.hip describes it)
// converges to exactly those sums, so the shortest-path DAG networkx walks follows from the converged distances alone:
//   arc u -> v (weight w) is a DAG arc of source lane b  iff  D(v, b) is finite, fl(D(u, b) + w) == D(v, b) and
//   D(u, b) < D(v, b).
// The strict inequality makes the relation acyclic whatever the weights are; a self-loop is never tight.  An arc whose
// weight is absorbed (fl(d + w) == d) is not a DAG arc -- a stated divergence: what networkx does with it depends on
// the order of its heap.  The rest is the level-synchronous sigma / delta machinery of grx_betweenness.hip with "BFS
// level" replaced by "depth in the DAG" (the most arcs on any lightest path from the source).
//
// A batch holds S sources, S = 16, 32 or 64; state is node-major, cell (v, b) = v * S + b, S lanes per node as in the
// relaxation.  Per cell: D (fp64, the relaxation's first buffer), delta (fp64: the relaxation's SECOND buffer, which
// holds the same fixed point once the relaxation has converged and is free from then on), sigma (fp64 path counts,
// overwritten by coeff = (1 + delta) / sigma once the cell's delta is known) and depth (int32: -2 no path, -1 reached
// and not resolved yet, >= 0 the depth).
//
// Forward (device-steered round loop, grx_common.h): pull over the IN-adjacency with its weights.  In round l a reached,
//   unresolved cell scans its in-arcs; when EVERY DAG predecessor u has 0 <= depth(u) < l it stores sigma = the sum
//   of sigma(u) (whole numbers below 2^53: exact in any order) and depth = l.  A predecessor seen at depth l or -1
//   counts as unresolved, so a round never reads a sigma stored by its own launch and both the values and the number
//   of rounds are reproducible.  A cell must wait for its DEEPEST predecessor: lightest paths of equal weight may have
//   different numbers of arcs, and settling at the first tight predecessor would lose the longer ones.  Sources start
//   at depth 0 with sigma 1 (networkx carries 2 there, hence 2 sigma everywhere: a power of two that cancels exactly in
//   sigma(v) * coeff(w)).  Rows without an open lane are skipped; a round that resolves nothing ends the loop, the
//   level word then holds the deepest depth; more than n + 1 rounds are refused.  A reached cell without any DAG
//   predecessor (possible only through absorbed or zero weights, outside the contract) never resolves and counts as
//   not reached.
// Backward, level l = deepest .. 1, launched from the host: pull over the OUT-adjacency with its weights.  A cell at
//   depth l adds sigma(v) * coeff(x) over its DAG successors x in arc order, each term networkx's own product; every
//   successor is deeper, hence final.  Then coeff(v) = (1 + delta(v)) / sigma(v) replaces sigma(v).
// Accumulation, endpoints and scale are those of grx_betweenness.hip (grx_brandes.h, as are the argument checks and the
//   per-batch sequence of these passes: br_open and br_run, which WbSide below serves): bc[v] adds the sources'
//   contributions one after another in the caller's order (lanes in order, batches in order), the per-lane reach counts are integer adds, there
//   are no floating-point atomics: the same bits for every S and every run.  The reach counts (needed with endpoints
//   only) come from one pass over the depths after the forward loop.  MEASURED AND REMOVED: counting them inside the
//   forward kernels with one atomicAdd per thread that resolved something, as grx_betweenness.hip does -- with S lanes
//   per node every thread of the grid hits one of only S addresses: 1 024 sources on BA 1 M / m = 10 took 1 798.8 ms
//   against 1 789.7 ms without at S = 64, 2 374.7 against 2 090.7 ms at S = 32 and 4 335.4 against 2 711.1 ms at
//   S = 16 (the forward pass alone 2 343 against 717 ms); profiles/weighted_betweenness.txt.
// Hub rows (longer than GRX_HUB_FACTOR * lanes_per_row of the CSR the pass reads) get a workgroup each in both passes:
//   WB_PARTS = 4 lane groups of S lanes take every fourth arc and combine as ((p0 + p1) + p2) + p3 -- four parts for
//   every S, so that the order of the additions does not depend on the batch width.
//
// grx_weighted_edge_betweenness (networkx's edge_betweenness_centrality with a weight, _accumulate_edges, _rescale_e)
// runs the same relaxation, forward and backward kernels with coeff written to an array of its own (the backward
// kernels are templated on that: 36 bytes per cell), so that sigma survives; after the backward loop of a batch one pass
// over the arcs adds sigma(v) * coeff(x) of every DAG arc v -> x (the tight-arc test above, v resolved, x deeper) onto
// the arc's slot.  S lanes per row (hub rows: a workgroup whose WB_PARTS lane groups take every fourth arc), the lanes
// are the batch's sources, so a slot is written by one lane group.  The order of the additions is that of
// grx_edge_sum.h: a fixed tree over each aligned group of 16 consecutive sources, the groups one after another in
// source order -- the same bits for S = 16, 32 and 64.  The unused lanes of a partial batch have no path (depth -2) and
// hold +0.0.  Undirected: the edge is the sum of its two arc slots (grx_edge_sum.h's final passes, with the scale).
#pragma clang fp contract(off)

#include "grx_relax.h"
#include "grx_brandes.h"

namespace {

constexpr int WB_BLOCK = 256;
constexpr int WB_PARTS = BR_PARTS;                           // lane groups of a hub workgroup: the same for every S
constexpr int WB_MAX_ROW_BLOCKS = 8192;
constexpr int WB_MAX_BLOCKS = 2048;                           // grid of the per-element launches
constexpr size_t WB_DEFAULT_STATE_BYTES = (size_t)4 << 30;   // state budget of the library's choice of S

constexpr int32_t WB_OPEN = -1;                              // reached, depth not known yet
constexpr int32_t WB_UNREACHED = -2;

// The workspace, laid out once: D, delta, sigma (fp64) and depth (int32) per (node, source) -- 28 bytes a cell; coeff
// (fp64) in an array of its own for grx_weighted_edge_betweenness only, 36 bytes a cell (otherwise coeff replaces
// sigma); the relaxation's stamp per node; the per-lane reach counts and the control words
struct WbWs {
    BrLayout lay;
    double *D, *delta, *sigma, *coeff;
    int32_t *depth, *stamp, *reach, *ctrl;
    WbWs(void *base, int64_t n, int S, bool keep_sigma) : lay(base, n, S)
    {
        D = lay.per_cell<double>();
        delta = lay.per_cell<double>();
        sigma = lay.per_cell<double>();
        coeff = keep_sigma ? lay.per_cell<double>() : nullptr;
        depth = lay.per_cell<int32_t>();
        stamp = lay.per_node<int32_t>();
        reach = lay.take<int32_t>(S);
        ctrl = lay.take<int32_t>(GRX_CTRL_MAX_WORDS);
    }
    size_t bytes() const { return lay.used; }
};

// batch = 0: the widest S whose state fits WB_DEFAULT_STATE_BYTES, never below 16 and no wider than the source list
// rounded up
int choose_batch(int64_t n, int batch, int64_t n_sources, bool keep_sigma)
{
    if (batch > 0) return batch;
    const BrLayout lay = WbWs(nullptr, n, 1, keep_sigma).lay;
    auto state_bytes = [&](int S) { return lay.nodes * ((size_t)S * lay.cell_bytes + lay.node_bytes); };
    int widest = 16;
    while (widest < 64 && state_bytes(widest * 2) <= WB_DEFAULT_STATE_BYTES) widest *= 2;
    int s = 16;
    while (s < widest && s < n_sources) s *= 2;
    return s;
}

// the converged distances as depth marks: a cell with a path is open, one without (the unused lanes of a last, partial
// batch among them) is never looked at again
__global__ __launch_bounds__(WB_BLOCK) void wb_depth_init_kernel(int64_t cells, const double *__restrict__ D,
                                                                 int32_t *__restrict__ depth)
{
    for (int64_t i = (int64_t)blockIdx.x * WB_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.x * WB_BLOCK)
        depth[i] = D[i] < SP_INF ? WB_OPEN : WB_UNREACHED;
}

// lane b < count: source s_b at depth 0 with sigma 1; reach = 0 (wb_reach_kernel counts once the depths are known)
template <int S>
__global__ __launch_bounds__(GRX_WAVE) void wb_source_init_kernel(int64_t n, int count,
                                                                  const int32_t *__restrict__ src,
                                                                  int32_t *__restrict__ depth,
                                                                  double *__restrict__ sigma,
                                                                  int32_t *__restrict__ reach,
                                                                  int32_t *__restrict__ ctrl)
{
    const int b = threadIdx.x;
    if (b < S) {
        reach[b] = 0;
        if (b < count && src[b] >= 0 && src[b] < n) {       // an id outside [0, n) is never written through
            const int64_t cell = (int64_t)src[b] * S + b;
            depth[cell] = 0;
            sigma[cell] = 1.0;
        }
    }
    if (b == 0) { ctrl[GRX_CT_DONE] = 0; ctrl[GRX_CT_LEVEL] = 0; ctrl[GRX_CT_FOUND] = 0; }
}

// One lane's DAG predecessors among the in-arcs [b, e) with stride `step`: acc += sigma(u) for every tight u resolved
// before round l.  false as soon as a tight predecessor is not (depth -1, or l: stored by this very launch).
template <int S>
__device__ __forceinline__ bool pull_preds(int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                           const double *__restrict__ w, const double *__restrict__ D,
                                           const int32_t *depth, const double *sigma, int lane, double dv, int l,
                                           double &acc)
{
    auto settled = [&](int64_t u) {
        const int p = depth[u * S + lane];
        if (p < 0 || p >= l) return false;
        acc += sigma[u * S + lane];
        return true;
    };
    int64_t j = b;
    for (; j + 3 * step < e; j += 4 * step) {
        const int64_t u0 = col[j], u1 = col[j + step], u2 = col[j + 2 * step], u3 = col[j + 3 * step];
        const double w0 = w ? w[j] : 1.0, w1 = w ? w[j + step] : 1.0;
        const double w2 = w ? w[j + 2 * step] : 1.0, w3 = w ? w[j + 3 * step] : 1.0;
        const double a0 = D[u0 * S + lane], a1 = D[u1 * S + lane], a2 = D[u2 * S + lane], a3 = D[u3 * S + lane];
        const bool t0 = a0 + w0 == dv && a0 < dv, t1 = a1 + w1 == dv && a1 < dv;
        const bool t2 = a2 + w2 == dv && a2 < dv, t3 = a3 + w3 == dv && a3 < dv;
        if (t0 && !settled(u0)) return false;
        if (t1 && !settled(u1)) return false;
        if (t2 && !settled(u2)) return false;
        if (t3 && !settled(u3)) return false;
    }
    for (; j < e; j += step) {
        const int64_t u = col[j];
        const double a = D[u * S + lane];
        if (a + (w ? w[j] : 1.0) == dv && a < dv && !settled(u)) return false;
    }
    return true;
}

// One lane's delta over the out-arcs [b, e) with stride `step`: sigma(v) * coeff(x) over the DAG successors x, added in
// arc order (networkx adds them in the reverse of its settling order; only that order differs).  A successor is deeper
// than l, so its coeff is final; a cell that never resolved (depth < 0) is none.
template <int S>
__device__ __forceinline__ double pull_succ(int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                            const double *__restrict__ w, const double *__restrict__ D,
                                            const int32_t *__restrict__ depth, const double *coeff, int lane,
                                            double dv, int l, double sv)
{
    double acc = 0.0;
    auto add = [&](int64_t j, int64_t x) {
        const double dx = D[x * S + lane];
        if (dv + (w ? w[j] : 1.0) == dx && dv < dx) acc += sv * coeff[x * S + lane];
    };
    int64_t j = b;
    for (; j + 3 * step < e; j += 4 * step) {
        const int64_t x0 = col[j], x1 = col[j + step], x2 = col[j + 2 * step], x3 = col[j + 3 * step];
        const int p0 = depth[x0 * S + lane], p1 = depth[x1 * S + lane];
        const int p2 = depth[x2 * S + lane], p3 = depth[x3 * S + lane];
        if (p0 > l) add(j, x0);
        if (p1 > l) add(j + step, x1);
        if (p2 > l) add(j + 2 * step, x2);
        if (p3 > l) add(j + 3 * step, x3);
    }
    for (; j < e; j += step) {
        const int64_t x = col[j];
        if (depth[x * S + lane] > l) add(j, x);
    }
    return acc;
}

// forward round, rows up to hub_degree arcs: S lanes per node, WB_BLOCK / S nodes per workgroup and grid step
template <int S>
__global__ __launch_bounds__(WB_BLOCK) void wb_forward_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ w, int64_t hub_degree,
                                                              const double *__restrict__ D, int32_t *depth,
                                                              double *sigma, int32_t *__restrict__ ctrl)
{
    constexpr int GROUPS = WB_BLOCK / S;
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL] + 1;
    const int lane = threadIdx.x % S;
    int found = 0;
    for (int64_t v = (int64_t)blockIdx.x * GROUPS + threadIdx.x / S; v < n; v += (int64_t)gridDim.x * GROUPS) {
        const int64_t cell = v * S + lane;
        if (depth[cell] != WB_OPEN) continue;               // a row without an open lane costs this one load
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_degree) continue;                   // wb_forward_hub_kernel
        double acc = 0.0;
        if (pull_preds<S>(b, e, 1, col, w, D, depth, sigma, lane, D[cell], l, acc) && acc > 0.0) {
            sigma[cell] = acc;
            depth[cell] = l;
            ++found;
        }
    }
    if (__ballot(found != 0) && threadIdx.x % GRX_WAVE == 0) ctrl[GRX_CT_FOUND] = 1;
}

// forward round, hub rows: one workgroup of WB_PARTS * S threads per hub row; part p takes every WB_PARTS-th arc
template <int S>
__global__ __launch_bounds__(WB_PARTS * S) void wb_forward_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                      const int32_t *__restrict__ col,
                                                                      const double *__restrict__ w,
                                                                      const int32_t *__restrict__ hub_rows,
                                                                      const double *__restrict__ D, int32_t *depth,
                                                                      double *sigma, int32_t *__restrict__ ctrl)
{
    __shared__ double part[WB_PARTS][S];
    __shared__ int clear[WB_PARTS][S];
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL] + 1;
    const int lane = threadIdx.x % S, p = threadIdx.x / S;
    const int64_t v = hub_rows[blockIdx.x];
    const int64_t cell = v * S + lane;
    const bool open = depth[cell] == WB_OPEN;
    if (!__syncthreads_or(open)) return;                    // the same in every thread of the workgroup
    double acc = 0.0;
    bool ok = false;
    if (open) ok = pull_preds<S>(row_ptr[v] + p, row_ptr[v + 1], WB_PARTS, col, w, D, depth, sigma, lane, D[cell], l, acc);
    part[p][lane] = acc;
    clear[p][lane] = ok;
    __syncthreads();
    if (p != 0 || !open) return;
    if (!(clear[0][lane] && clear[1][lane] && clear[2][lane] && clear[3][lane])) return;
    const double total = br_combine4(part, lane);
    if (total > 0.0) {
        sigma[cell] = total;
        depth[cell] = l;
        ctrl[GRX_CT_FOUND] = 1;
    }
}

// after the forward loop: reach[b] = the resolved cells of lane b, its source among them (networkx's len(S)); block
// sums through LDS, then one integer atomic per lane and workgroup
template <int S>
__global__ __launch_bounds__(WB_BLOCK) void wb_reach_kernel(int64_t n, const int32_t *__restrict__ depth,
                                                            int32_t *__restrict__ reach)
{
    constexpr int GROUPS = WB_BLOCK / S;
    __shared__ int32_t part[WB_BLOCK];
    const int t = threadIdx.x, lane = t % S;
    int32_t count = 0;
    for (int64_t v = (int64_t)blockIdx.x * GROUPS + t / S; v < n; v += (int64_t)gridDim.x * GROUPS)
        count += depth[v * S + lane] >= 0;
    part[t] = count;
    __syncthreads();
#pragma unroll
    for (int s = WB_BLOCK / 2; s >= S; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    if (t < S && part[t]) atomicAdd(&reach[t], part[t]);
}

// backward, level l: the cells at depth l pull delta from their DAG successors.  KEEP_SIGMA = false: coeff replaces
// sigma in place (kept_coeff is not read); true: coeff goes to kept_coeff
template <int S, bool KEEP_SIGMA>
__global__ __launch_bounds__(WB_BLOCK) void wb_backward_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ col,
                                                               const double *__restrict__ w, int64_t hub_degree, int l,
                                                               const double *__restrict__ D,
                                                               const int32_t *__restrict__ depth, double *sigma,
                                                               double *kept_coeff, double *__restrict__ delta)
{
    constexpr int GROUPS = WB_BLOCK / S;
    double *coeff = KEEP_SIGMA ? kept_coeff : sigma;
    const int lane = threadIdx.x % S;
    for (int64_t v = (int64_t)blockIdx.x * GROUPS + threadIdx.x / S; v < n; v += (int64_t)gridDim.x * GROUPS) {
        const int64_t cell = v * S + lane;
        if (depth[cell] != l) continue;
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_degree) continue;                   // wb_backward_hub_kernel
        const double sv = sigma[cell];
        br_settle(cell, pull_succ<S>(b, e, 1, col, w, D, depth, coeff, lane, D[cell], l, sv), sv, coeff, delta);
    }
}

template <int S, bool KEEP_SIGMA>
__global__ __launch_bounds__(WB_PARTS * S) void wb_backward_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                       const int32_t *__restrict__ col,
                                                                       const double *__restrict__ w,
                                                                       const int32_t *__restrict__ hub_rows, int l,
                                                                       const double *__restrict__ D,
                                                                       const int32_t *__restrict__ depth,
                                                                       double *sigma, double *kept_coeff,
                                                                       double *__restrict__ delta)
{
    __shared__ double part[WB_PARTS][S];
    double *coeff = KEEP_SIGMA ? kept_coeff : sigma;
    const int lane = threadIdx.x % S, p = threadIdx.x / S;
    const int64_t v = hub_rows[blockIdx.x];
    const int64_t cell = v * S + lane;
    const bool mine = depth[cell] == l;
    if (!__syncthreads_or(mine)) return;
    const double sv = mine ? sigma[cell] : 1.0;
    part[p][lane] = mine ? pull_succ<S>(row_ptr[v] + p, row_ptr[v + 1], WB_PARTS, col, w, D, depth, coeff, lane,
                                        D[cell], l, sv)
                         : 0.0;
    __syncthreads();
    if (p != 0 || !mine) return;
    br_settle(cell, br_combine4(part, lane), sv, coeff, delta);
}

// grx_weighted_edge_betweenness, after the backward loop of a batch: the arcs [b, e) with stride `step` of row v, the
// S lanes of the group (it starts at wavefront lane `base`) being the batch's sources.  A lane holds sigma(v) *
// coeff(x) when v -> x is an arc of its source's DAG -- v resolved, x deeper, and the tight-arc test of pull_succ --
// and +0.0 otherwise; grx_edge_sum.h's order adds them onto the slot, which the group's first lane reads and writes.
template <int S>
__device__ __forceinline__ void edge_row(int64_t v, int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                         const double *__restrict__ w, const double *__restrict__ D,
                                         const int32_t *__restrict__ depth, const double *__restrict__ sigma,
                                         const double *__restrict__ coeff, int lane, int base,
                                         double *__restrict__ ebc)
{
    const int pv = depth[v * S + lane];
    if (!eb_group_any<S>(pv >= 0, base)) return;            // the same in every lane of the group
    const double dv = D[v * S + lane];
    const double sv = pv >= 0 ? sigma[v * S + lane] : 0.0;
    for (int64_t j = b; j < e; j += step) {
        const int64_t x = col[j];
        bool on = pv >= 0 && depth[x * S + lane] > pv;
        if (on) {
            const double dx = D[x * S + lane];
            on = dv + (w ? w[j] : 1.0) == dx && dv < dx;
        }
        if (!eb_group_any<S>(on, base)) continue;           // S times +0.0
        const double acc = eb_add_groups<S>(lane == 0 ? ebc[j] : 0.0, on ? sv * coeff[x * S + lane] : 0.0, base);
        if (lane == 0) ebc[j] = acc;
    }
}

// rows up to hub_degree arcs: S lanes per row, WB_BLOCK / S rows per workgroup and grid step
template <int S>
__global__ __launch_bounds__(WB_BLOCK) void wb_edge_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ w, int64_t hub_degree,
                                                           const double *__restrict__ D,
                                                           const int32_t *__restrict__ depth,
                                                           const double *__restrict__ sigma,
                                                           const double *__restrict__ coeff, double *__restrict__ ebc)
{
    constexpr int GROUPS = WB_BLOCK / S;
    const int lane = threadIdx.x % S;
    const int base = threadIdx.x % GRX_WAVE - lane;
    for (int64_t v = (int64_t)blockIdx.x * GROUPS + threadIdx.x / S; v < n; v += (int64_t)gridDim.x * GROUPS) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_degree) continue;                   // wb_edge_hub_kernel
        edge_row<S>(v, b, e, 1, col, w, D, depth, sigma, coeff, lane, base, ebc);
    }
}

// hub rows: one workgroup of WB_PARTS * S threads per hub row; part p takes every WB_PARTS-th arc (a slot still has
// one owner)
template <int S>
__global__ __launch_bounds__(WB_PARTS * S) void wb_edge_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                   const int32_t *__restrict__ col,
                                                                   const double *__restrict__ w,
                                                                   const int32_t *__restrict__ hub_rows,
                                                                   const double *__restrict__ D,
                                                                   const int32_t *__restrict__ depth,
                                                                   const double *__restrict__ sigma,
                                                                   const double *__restrict__ coeff,
                                                                   double *__restrict__ ebc)
{
    const int lane = threadIdx.x % S, p = threadIdx.x / S;
    const int base = threadIdx.x % GRX_WAVE - lane;
    const int64_t v = hub_rows[blockIdx.x];
    edge_row<S>(v, row_ptr[v] + p, row_ptr[v + 1], WB_PARTS, col, w, D, depth, sigma, coeff, lane, base, ebc);
}

// What br_run drives: the carved state of one call at batch width S.  EDGES = false is grx_weighted_betweenness, true is
// grx_weighted_edge_betweenness (`endpoints` is 0 there)
template <int S, bool EDGES>
struct WbSide {
    int64_t n;
    SpPull out, in;                                          // backward pulls over `out`; relaxation and forward over `in`
    bool directed;
    int endpoints;
    WbWs ws;
    int64_t *rounds, *levels;                                // relaxation rounds summed, the deepest DAG level
    hipStream_t st;

    unsigned row_blocks() const { return grx_grid(n, WB_BLOCK / S, WB_MAX_ROW_BLOCKS); }
    static const char *forward_refusal()
    {
        return EDGES ? "grx_weighted_edge_betweenness: the forward pass did not end after %lld rounds"
                     : "grx_weighted_betweenness: the forward pass did not end after %lld rounds";
    }
    int begin(const int32_t *d_src, int count) const
    {
        const int64_t cells = n * S;
        const int rc = sp_relax<S>(
            in, d_src, count, ws.D, ws.delta, ws.stamp, ws.ctrl,
            EDGES ? "grx_weighted_edge_betweenness: the relaxation did not end after %lld rounds (a negative or NaN "
                    "weight?)"
                  : "grx_weighted_betweenness: the relaxation did not end after %lld rounds (a negative or NaN weight?)",
            GRX_K_WBC_RELAX, rounds, st);
        if (rc != GRX_OK) return rc;
        // both distance buffers hold the fixed point: ws.delta is free
        wb_depth_init_kernel<<<grx_grid(cells, WB_BLOCK, WB_MAX_BLOCKS), WB_BLOCK, 0, st>>>(cells, ws.D, ws.depth);
        wb_source_init_kernel<S><<<1, GRX_WAVE, 0, st>>>(n, count, d_src, ws.depth, ws.sigma, ws.reach, ws.ctrl);
        return GRX_OK;
    }
    int forward_round() const
    {
        GRX_PROF(GRX_K_WBC_FORWARD, st);
        if (in.n_hub_rows)
            wb_forward_hub_kernel<S><<<(unsigned)in.n_hub_rows, WB_PARTS * S, 0, st>>>(
                in.row_ptr, in.col, in.w, in.hub_rows, ws.D, ws.depth, ws.sigma, ws.ctrl);
        wb_forward_kernel<S><<<row_blocks(), WB_BLOCK, 0, st>>>(n, in.row_ptr, in.col, in.w, in.hub_degree, ws.D,
                                                                ws.depth, ws.sigma, ws.ctrl);
        return grx_frontier_advance(ws.ctrl, st);
    }
    void after_forward(int deepest) const
    {
        *levels = std::max<int64_t>(*levels, deepest);
        if (endpoints)
            wb_reach_kernel<S><<<grx_grid(n, WB_BLOCK / S, WB_MAX_BLOCKS), WB_BLOCK, 0, st>>>(n, ws.depth, ws.reach);
    }
    void backward(int l) const
    {
        GRX_PROF(GRX_K_WBC_BACKWARD, st);
        if (out.n_hub_rows)
            wb_backward_hub_kernel<S, EDGES><<<(unsigned)out.n_hub_rows, WB_PARTS * S, 0, st>>>(
                out.row_ptr, out.col, out.w, out.hub_rows, l, ws.D, ws.depth, ws.sigma, ws.coeff, ws.delta);
        wb_backward_kernel<S, EDGES><<<row_blocks(), WB_BLOCK, 0, st>>>(n, out.row_ptr, out.col, out.w, out.hub_degree,
                                                                        l, ws.D, ws.depth, ws.sigma, ws.coeff,
                                                                        ws.delta);
    }
    void edge_pass(double *d_ebc) const
    {
        if (out.n_hub_rows)
            wb_edge_hub_kernel<S><<<(unsigned)out.n_hub_rows, WB_PARTS * S, 0, st>>>(
                out.row_ptr, out.col, out.w, out.hub_rows, ws.D, ws.depth, ws.sigma, ws.coeff, d_ebc);
        wb_edge_kernel<S><<<row_blocks(), WB_BLOCK, 0, st>>>(n, out.row_ptr, out.col, out.w, out.hub_degree, ws.D,
                                                             ws.depth, ws.sigma, ws.coeff, d_ebc);
    }
    const int32_t *level() const { return ws.depth; }
    int stride() const { return S; }
};

// the argument checks and the batches of both entry points (d_out = bc resp. ebc)
template <bool EDGES>
int entry(const char *name, int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
          const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr,
          const int32_t *d_in_col, const double *d_in_w, const int32_t *d_in_hub_rows, int64_t n_in_hub_rows,
          int in_lanes_per_row, const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, int batch,
          double *d_out, int64_t *h_rounds, int64_t *h_levels, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(batch == 0 || sp_valid_batch(batch), "%s: batch must be 0, 16, 32 or 64 (got %d)", name, batch);
    GRX_REQUIRE(n_sources < (int64_t)1 << 31, "%s: source list", name);
    const int S = choose_batch(n, batch, n_sources, EDGES);
    const WbWs ws(d_workspace, n, S, EDGES);
    SpPull out, in;
    bool directed;
    int rc = br_open(name, n, d_row_ptr, d_col, d_w, d_hub_rows, n_hub_rows, lanes_per_row, d_in_row_ptr, d_in_col,
                     d_in_w, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources, n_sources, d_out, d_workspace,
                     workspace_bytes, ws.bytes(), out, in, directed);
    if (rc != GRX_OK) return rc;
    GRX_REQUIRE((out.w == nullptr) == (in.w == nullptr), "%s: d_w and d_in_w must both be given or both be NULL", name);
    hipStream_t st = grx_stream(stream);
    int64_t rounds = 0, levels = 0;
    auto run = [&](auto side) { return br_run<EDGES>(side, d_sources, n_sources, endpoints, scale, d_out, st); };
    switch (S) {
    case 16: rc = run(WbSide<16, EDGES>{n, out, in, directed, endpoints, ws, &rounds, &levels, st}); break;
    case 32: rc = run(WbSide<32, EDGES>{n, out, in, directed, endpoints, ws, &rounds, &levels, st}); break;
    default: rc = run(WbSide<64, EDGES>{n, out, in, directed, endpoints, ws, &rounds, &levels, st}); break;
    }
    if (h_rounds) *h_rounds = rounds;
    if (h_levels) *h_levels = levels;
    return rc;
}

}  // namespace

extern "C" {

size_t grx_weighted_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return WbWs(nullptr, n, choose_batch(n, sp_valid_batch(batch) ? batch : 0, n_sources, false), false).bytes();
}

int grx_weighted_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                             const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                             const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                             const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                             const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, int batch,
                             double *d_bc, int64_t *h_rounds, int64_t *h_levels, void *d_workspace,
                             size_t workspace_bytes, void *stream)
{
    return entry<false>("grx_weighted_betweenness", n, d_row_ptr, d_col, d_w, d_hub_rows, n_hub_rows, lanes_per_row,
                        d_in_row_ptr, d_in_col, d_in_w, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row, d_sources,
                        n_sources, endpoints, scale, batch, d_bc, h_rounds, h_levels, d_workspace, workspace_bytes,
                        stream);
}

size_t grx_weighted_edge_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources)
{
    return WbWs(nullptr, n, choose_batch(n, sp_valid_batch(batch) ? batch : 0, n_sources, true), true).bytes();
}

int grx_weighted_edge_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                                  const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                                  const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                                  const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                                  const int32_t *d_sources, int64_t n_sources, double scale, int batch, double *d_ebc,
                                  int64_t *h_rounds, int64_t *h_levels, void *d_workspace, size_t workspace_bytes,
                                  void *stream)
{
    return entry<true>("grx_weighted_edge_betweenness", n, d_row_ptr, d_col, d_w, d_hub_rows, n_hub_rows,
                       lanes_per_row, d_in_row_ptr, d_in_col, d_in_w, d_in_hub_rows, n_in_hub_rows, in_lanes_per_row,
                       d_sources, n_sources, 0, scale, batch, d_ebc, h_rounds, h_levels, d_workspace, workspace_bytes,
                       stream);
}

}  // extern "C"
