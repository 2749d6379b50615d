// grx_rowjoin.h -- the three stages that grx_structural_holes.hip and grx_clustering.hip share: a masked sparse
// product as one row intersection per arc of a structurally symmetric CSR with ascending columns.  TO BE INCLUDED ONLY
// UNDER `#pragma clang fp contract(off)` (and the Makefile's -ffp-contract=off): the bodies below are inlined into
// these kernels, and every quotient, product and sum of theirs must stay its own IEEE operation.
//   (a) per row: a body accumulates over the entries of the row and writes the row's statistics (and arc_row);
//   (b) per arc (u, v): a group of L lanes walks the shorter of the two rows, lane k entries k, k + L, ..., and looks
//       every entry up in the longer row by binary search; the body adds what a hit contributes and writes the arc's
//       terms;
//   (c) per row: another row body sums the arcs' terms and writes the outputs.
// (a) and (c) are one skeleton in two launch shapes over ONE body: rj_rows_kernel<L> (a group of L lanes per row, lane k
// the entries k, k + L, ... in order, then the fixed butterflies grx_group_sum / grx_group_max) and rj_hub_rows_kernel
// (one workgroup per row longer than GRX_HUB_FACTOR * L, thread t the entries t, t + RJ_BLOCK, ..., then the fixed tree
// grx_block_reduce).  No floating-point atomics, no hand-off between workgroups: the same bits in every run.
//
// A row body is a struct of kernel arguments with
//   struct Acc;                                              zero-initialised accumulators of one lane / thread
//   void entry(int64_t u, int64_t j, Acc &a) const;          entry j of row u
//   template <class R> void reduce(Acc &a, R r) const;       a.x = r.sum(a.x) / r.max(a.x), in a fixed order; every
//                                                            lane of the group (thread of the workgroup) calls it
//   void finish(int64_t u, int64_t b, int64_t e, const Acc &a) const;    lane 0 / thread 0; the row is [b, e)
// and an arc body has the same Acc and reduce, and
//   bool begin(int64_t j, int32_t u, int32_t v, Acc &a) const;    what arc j needs of u and v; false: no intersection
//   void hit(int32_t u, int32_t v, int32_t w, int64_t k, int64_t lo, bool walk_u, Acc &a) const;
//                                                            w = col[k] = col[lo]: k in the walked row (u's if
//                                                            walk_u), lo in the searched one
//   void finish(int64_t j, const Acc &a) const;              lane 0
// Everything has internal linkage; the bodies are template arguments, so every call inlines.
#pragma once
#include "grx_common.h"

#include <type_traits>

namespace {

constexpr int RJ_BLOCK = 256;
constexpr int RJ_ROW_MAX_WG = 2048;      // workgroups of the row kernels (a) and (c)
constexpr int RJ_ARC_MAX_WG = 8192;      // workgroups of the per-arc kernel (b)

template <int L>
struct RjGroup {                         // the reductions of a group of L lanes
    __device__ __forceinline__ double sum(double v) const { return grx_group_sum<L>(v); }
    __device__ __forceinline__ double max(double v) const { return grx_group_max<L>(v); }
};
struct RjBlock {                         // and of a workgroup
    double *sm;
    __device__ __forceinline__ double sum(double v) const { return grx_block_reduce<RJ_BLOCK>(v, sm); }
    __device__ __forceinline__ double max(double v) const { return grx_block_reduce<RJ_BLOCK, true>(v, sm); }
};

template <class Body>
__global__ __launch_bounds__(RJ_BLOCK) void rj_hub_rows_kernel(const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ hub_rows, const Body body)
{
    __shared__ double sm[RJ_BLOCK];
    const int32_t u = hub_rows[blockIdx.x];
    const int64_t b = row_ptr[u], e = row_ptr[u + 1];
    typename Body::Acc a{};
    for (int64_t j = b + threadIdx.x; j < e; j += RJ_BLOCK) body.entry(u, j, a);
    body.reduce(a, RjBlock{sm});
    if (threadIdx.x == 0) body.finish(u, b, e, a);
}

template <int L, class Body>
__global__ __launch_bounds__(RJ_BLOCK) void rj_rows_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           int64_t hub_degree, const Body body)
{
    constexpr int RPG = RJ_BLOCK / L;                       // rows per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t u = g * RPG + slot;
        int64_t b = 0, e = 0;
        if (u < n) { b = row_ptr[u]; e = row_ptr[u + 1]; }
        const bool hub = e - b > hub_degree;                // rj_hub_rows_kernel's
        typename Body::Acc a{};
        if (!hub)
            for (int64_t j = b + lane; j < e; j += L) body.entry(u, j, a);
        body.reduce(a, RjGroup<L>{});
        if (lane == 0 && u < n && !hub) body.finish(u, b, e, a);
    }
}

template <int L, class Body>
__global__ __launch_bounds__(RJ_BLOCK) void rj_arc_kernel(int64_t nnz, const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ arc_row, const Body body)
{
    constexpr int APG = RJ_BLOCK / L;                       // arcs per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (nnz + APG - 1) / APG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t j = g * APG + slot;
        typename Body::Acc a{};
        if (j < nnz) {
            const int32_t u = arc_row[j], v = col[j];
            if (body.begin(j, u, v, a)) {
                const int64_t bu = row_ptr[u], eu = row_ptr[u + 1], bv = row_ptr[v], ev = row_ptr[v + 1];
                const bool walk_u = eu - bu <= ev - bv;     // walk the shorter row, search the longer one
                const int64_t wb = walk_u ? bu : bv, we = walk_u ? eu : ev;
                const int64_t sb = walk_u ? bv : bu, se = walk_u ? ev : eu;
                for (int64_t k = wb + lane; k < we; k += L) {
                    const int32_t w = col[k];
                    int64_t lo = sb, hi = se;
                    while (lo < hi) {
                        const int64_t mid = lo + (hi - lo) / 2;
                        if (col[mid] < w) lo = mid + 1; else hi = mid;
                    }
                    if (lo < se && col[lo] == w) body.hit(u, v, w, k, lo, walk_u, a);
                }
            }
        }
        body.reduce(a, RjGroup<L>{});
        if (lane == 0 && j < nnz) body.finish(j, a);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------
// The workspace: n_vecs vectors of n doubles, n_arcs vectors of nnz doubles, the int32 row of every arc; each 256-byte
// aligned.  Sized (base = NULL) and carved by the same arithmetic.
struct RjWs {
    char *base;
    size_t vec, arc, tail;
    int n_vecs, n_arcs;
    RjWs(void *b, int64_t n, int64_t nnz, int n_vecs_, int n_arcs_)
        : base(reinterpret_cast<char *>(b)), vec(grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256)),
          arc(grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 8, 256)),
          tail(grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 4, 256)), n_vecs(n_vecs_), n_arcs(n_arcs_) {}
    double *row(int i) const { return reinterpret_cast<double *>(base + i * vec); }
    double *per_arc(int i) const { return reinterpret_cast<double *>(base + n_vecs * vec + i * arc); }
    int32_t *arc_row() const { return reinterpret_cast<int32_t *>(base + n_vecs * vec + n_arcs * arc); }
    size_t bytes() const { return n_vecs * vec + n_arcs * arc + tail; }
};

// one call: the graph as the entry point received it, and what rj_prepare adds
struct RjCall {
    int64_t n;
    const int64_t *row_ptr;
    const int32_t *col, *hub_rows;
    int64_t n_hub_rows;
    int lanes;
    hipStream_t st;
    int64_t nnz, hub_degree;
};

// The checks every entry point makes after its own, with its name `who` in every message, and the read-back of the
// number of arcs (the last row pointer: the workspace is carved by it).  n == 0 returns GRX_OK before anything else is
// looked at: the caller returns then too.
int rj_prepare(const char *who, RjCall &c, void *workspace, size_t workspace_bytes, int n_vecs, int n_arcs, void *stream)
{
    GRX_REQUIRE(c.n >= 0 && c.n < (int64_t)1 << 31, "%s: n = %lld out of range [0, 2^31)", who, (long long)c.n);
    if (c.n == 0) return GRX_OK;
    GRX_REQUIRE(c.row_ptr && c.col && workspace, "%s: null pointer", who);
    GRX_REQUIRE(c.lanes == 4 || c.lanes == 8 || c.lanes == 16 || c.lanes == 32,
                "%s: lanes_per_row must be 4, 8, 16 or 32 (got %d)", who, c.lanes);
    GRX_REQUIRE(c.n_hub_rows >= 0 && c.n_hub_rows <= c.n && (c.n_hub_rows == 0 || c.hub_rows), "%s: hub list", who);
    c.st = grx_stream(stream);
    const size_t least = RjWs(nullptr, c.n, 0, n_vecs, n_arcs).bytes();
    GRX_REQUIRE(workspace_bytes >= least, "%s: workspace %zu bytes, need at least %zu", who, workspace_bytes, least);
    c.nnz = 0;
    GRX_CHECK_HIP(hipMemcpyAsync(&c.nnz, c.row_ptr + c.n, sizeof(c.nnz), hipMemcpyDeviceToHost, c.st));
    GRX_CHECK_HIP(hipStreamSynchronize(c.st));
    GRX_REQUIRE(c.nnz >= 0, "%s: row_ptr[n] = %lld", who, (long long)c.nnz);
    const size_t need = RjWs(nullptr, c.n, c.nnz, n_vecs, n_arcs).bytes();
    GRX_REQUIRE(workspace_bytes >= need, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
    c.hub_degree = (int64_t)GRX_HUB_FACTOR * c.lanes;
    return GRX_OK;
}

// f(std::integral_constant<int, L>) for the lane-group width L = lanes_per_row
template <class F>
void rj_with_lanes(int lanes_per_row, F f)
{
    switch (lanes_per_row) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
    }
}

// The launches of one call, hub rows first in (a) and last in (c); no per-arc launch without arcs, no stage (c)
// without `per_row`.
template <class Stats, class Arc, class Reduce>
int rj_run(const RjCall &c, const int32_t *arc_row, const Stats stats, const Arc arc, const Reduce reduce, bool per_row)
{
    if (c.n_hub_rows)
        rj_hub_rows_kernel<<<(unsigned)c.n_hub_rows, RJ_BLOCK, 0, c.st>>>(c.row_ptr, c.hub_rows, stats);
    rj_with_lanes(c.lanes, [&](auto width) {
        constexpr int L = decltype(width)::value;
        const unsigned rgrid = grx_grid(c.n, RJ_BLOCK / L, RJ_ROW_MAX_WG);
        rj_rows_kernel<L><<<rgrid, RJ_BLOCK, 0, c.st>>>(c.n, c.row_ptr, c.hub_degree, stats);
        if (c.nnz > 0)
            rj_arc_kernel<L><<<grx_grid(c.nnz, RJ_BLOCK / L, RJ_ARC_MAX_WG), RJ_BLOCK, 0, c.st>>>(
                c.nnz, c.row_ptr, c.col, arc_row, arc);
        if (per_row) rj_rows_kernel<L><<<rgrid, RJ_BLOCK, 0, c.st>>>(c.n, c.row_ptr, c.hub_degree, reduce);
    });
    if (c.n_hub_rows && per_row)
        rj_hub_rows_kernel<<<(unsigned)c.n_hub_rows, RJ_BLOCK, 0, c.st>>>(c.row_ptr, c.hub_rows, reduce);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // namespace
