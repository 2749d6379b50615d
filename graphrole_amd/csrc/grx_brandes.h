// grx_brandes.h -- the Brandes scaffolding that grx_betweenness.hip (shortest paths by hops) and
// grx_weighted_betweenness.hip (by arc weight) share, under all four entry points grx_betweenness,
// grx_edge_betweenness, grx_weighted_betweenness and grx_weighted_edge_betweenness: the argument checks (br_open), the
// walk that lays a workspace out (BrLayout), the per-batch sequence and the finish (br_run), and the device pieces
// that do not depend on how a file lays its cells out (br_settle, br_combine4, br_accumulate_kernel, br_scale_kernel).
// The cell layouts, the pull loops, the forward, backward and edge kernels and the way reach is counted stay with the
// two files, whose headers describe the methods; the order of the per-arc sums is grx_edge_sum.h's.
//
// A file hands br_run its "side": a struct of the carved state with
//   int64_t n; SpPull out, in; bool directed;                the nodes, and what br_open made of the caller's CSRs
//   int begin(const int32_t *d_src, int count) const;        the state of one batch of `count` sources (a GRX_* code)
//   int forward_round() const;                               the hub and the row kernel of one round, then
//                                                            grx_frontier_advance (a GRX_* code)
//   void after_forward(int deepest) const;                   between the forward loop and the backward levels
//   void backward(int l) const;                              the hub and the row kernel of level l
//   void edge_pass(double *d_ebc) const;                     EDGES: the batch's terms onto the arc slots
//   ws                                                       the carved workspace: ws.delta, ws.reach, ws.ctrl
//   const int32_t *level() const;  int stride() const;       the level (depth) array and the cells per node
//   static const char *forward_refusal();                    the message of grx_run_rounds (one %lld)
// Everything has internal linkage; the side is a template argument, so every call inlines.
//
// Compiled with -ffp-contract=off by both including files ((1 + delta) / sigma and the terms of bc are each their own
// IEEE operation, as in networkx); the pragma carries it with the header.
#pragma once
#pragma clang fp contract(off)

#include "grx_common.h"
#include "grx_edge_sum.h"

#include <algorithm>

namespace {

constexpr int BR_BLOCK = 256;                                // threads of the two per-node launches below
constexpr int BR_MAX_BLOCKS = 2048;                          // and their workgroups
constexpr int BR_PARTS = 4;                                  // partial sums of a hub row, whatever the batch width
constexpr int BR_LEVEL_BATCH = 8;                            // forward rounds enqueued between two read-backs

// networkx _accumulate_*: coeff = (1 + delta[w]) / sigma[w]; delta[v] += sigma[v] * coeff
__device__ __forceinline__ void br_settle(int64_t cell, double d, double sv, double *coeff, double *__restrict__ delta)
{
    delta[cell] = d;
    coeff[cell] = (1.0 + d) / sv;                            // coeff(v) for the levels nearer the source
}

// a hub row's BR_PARTS partial sums of one lane, always in this order
template <int W>
__device__ __forceinline__ double br_combine4(const double (&part)[BR_PARTS][W], int lane)
{
    return ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// bc[v] += the contributions of the batch's sources one after another, lanes 0 .. count - 1 of the `stride` cells of
// node v (networkx: betweenness[w] += delta[w] for w != s; with endpoints betweenness[s] += len(S) - 1 and
// betweenness[w] += delta[w] + 1).  level > 0: reached, not the source; level == 0: the source; anything else adds
// nothing.
__global__ __launch_bounds__(BR_BLOCK) void br_accumulate_kernel(int64_t n, int stride, int count, int endpoints,
                                                                 const int32_t *__restrict__ level,
                                                                 const double *__restrict__ delta,
                                                                 const int32_t *__restrict__ reach,
                                                                 double *__restrict__ bc)
{
    for (int64_t v = (int64_t)blockIdx.x * BR_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * BR_BLOCK) {
        const int32_t *lv = level + v * stride;
        const double *dv = delta + v * stride;
        double acc = bc[v];
        for (int b = 0; b < count; ++b) {
            const int l = lv[b];
            if (l > 0) acc += endpoints ? dv[b] + 1.0 : dv[b];
            else if (l == 0 && endpoints) acc += (double)(reach[b] - 1);
        }
        bc[v] = acc;
    }
}

__global__ __launch_bounds__(BR_BLOCK) void br_scale_kernel(int64_t n, double scale, double *__restrict__ bc)
{
    for (int64_t v = (int64_t)blockIdx.x * BR_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * BR_BLOCK)
        bc[v] *= scale;
}

// The walk (GrxCarve) over a workspace of `width` cells per node; cell_bytes and node_bytes are what one (node, source)
// and one node cost, for a file's choice of the batch width.
struct BrLayout : GrxCarve {
    size_t nodes, width, cell_bytes = 0, node_bytes = 0;
    BrLayout(void *b, int64_t n, int w) : GrxCarve(b), nodes(n > 0 ? n : 1), width(w) {}
    template <class T>
    T *per_cell() { cell_bytes += sizeof(T); return take<T>(nodes * width); }
    template <class T>
    T *per_node() { node_bytes += sizeof(T); return take<T>(nodes); }
};

// The checks every entry point makes, in this order, each message after the entry point's name; `out` and `in` are
// the CSRs the passes pull over (undirected, d_in_row_ptr == NULL: the CSR is its own in-adjacency).  `need`: the
// workspace of the batch width the file chose.  The rules on the batch width and on the weights stay with the files.
int br_open(const char *name, int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
            const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr,
            const int32_t *d_in_col, const double *d_in_w, const int32_t *d_in_hub_rows, int64_t n_in_hub_rows,
            int in_lanes_per_row, const int32_t *d_sources, int64_t n_sources, const double *d_out,
            const void *d_workspace, size_t workspace_bytes, size_t need, SpPull &out, SpPull &in, bool &directed)
{
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "%s: n = %lld out of range", name, (long long)n);
    GRX_REQUIRE(d_row_ptr && d_col && d_out && d_workspace, "%s: null pointer", name);
    GRX_REQUIRE(n_sources >= 0 && (n_sources == 0 || d_sources), "%s: source list", name);
    directed = d_in_row_ptr != nullptr;
    GRX_REQUIRE(!directed || d_in_col, "%s: d_in_col is required with d_in_row_ptr", name);
    out = SpPull{n, d_row_ptr, d_col, d_w, d_hub_rows, n_hub_rows, (int64_t)GRX_HUB_FACTOR * lanes_per_row};
    in = directed ? SpPull{n, d_in_row_ptr, d_in_col, d_in_w, d_in_hub_rows, n_in_hub_rows,
                           (int64_t)GRX_HUB_FACTOR * in_lanes_per_row}
                  : out;
    GRX_REQUIRE(lanes_per_row >= 1 && (!directed || in_lanes_per_row >= 1), "%s: lanes_per_row must be >= 1", name);
    GRX_REQUIRE(out.n_hub_rows >= 0 && (out.n_hub_rows == 0 || out.hub_rows) && in.n_hub_rows >= 0 &&
                    (in.n_hub_rows == 0 || in.hub_rows), "%s: hub list", name);
    GRX_REQUIRE(workspace_bytes >= need, "%s: workspace %zu bytes, need %zu", name, workspace_bytes, need);
    return GRX_OK;
}

// Every batch of `side.stride()` sources in the caller's order, then the finish.  EDGES = false: d_out is bc, one value
// per node; true: ebc, one value per arc of `out` (`endpoints` is 0 there).
template <bool EDGES, class Side>
int br_run(Side &side, const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, double *d_out,
           hipStream_t st)
{
    const SpPull &g = side.out;
    const int64_t n = side.n;
    const int B = side.stride();
    const unsigned egrid = grx_grid(n, BR_BLOCK, BR_MAX_BLOCKS);
    if (EDGES) eb_rows<EB_ZERO>(n, g.row_ptr, g.col, 0.0, d_out, st);
    else grx_fill64(reinterpret_cast<uint64_t *>(d_out), n, 0, st);
    GRX_LAUNCH_CHECK();
    for (int64_t first = 0; first < n_sources; first += B) {
        const int count = (int)std::min<int64_t>(B, n_sources - first);
        int rc = side.begin(d_sources + first, count);
        if (rc != GRX_OK) return rc;
        GRX_LAUNCH_CHECK();
        int32_t h[2];
        // a shortest-path DAG over n nodes is at most n - 1 arcs deep; one more round finds that nothing is new
        rc = grx_run_rounds(Side::forward_refusal(), BR_LEVEL_BATCH, n + 1, 2, side.ws.ctrl, h, st,
                            [&] { return side.forward_round(); });
        if (rc != GRX_OK) return rc;
        const int deepest = h[GRX_CT_LEVEL];
        side.after_forward(deepest);
        for (int l = deepest; l >= 1; --l) {                // deepest level first; the sources need no delta
            side.backward(l);
            GRX_LAUNCH_CHECK();
        }
        if (EDGES) side.edge_pass(d_out);
        else br_accumulate_kernel<<<egrid, BR_BLOCK, 0, st>>>(n, B, count, endpoints, side.level(), side.ws.delta,
                                                              side.ws.reach, d_out);
        GRX_LAUNCH_CHECK();
    }
    if (EDGES) eb_finish(n, g.row_ptr, g.col, side.directed, scale, d_out, st);
    else br_scale_kernel<<<egrid, BR_BLOCK, 0, st>>>(n, scale, d_out);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // namespace
