// grx_clustering.hip -- the weighted and the directed forms of the clustering coefficient of RolX sense making, as
// networkx 3.4.2's cluster.py defines them: Onnela's geometric mean of the normalised triangle weights, Fagiolo's
// directed coefficient, and the two together.
//
// Over a structurally symmetric CSR (row u lists every neighbour of u in either direction) with a value s per arc
//   undirected  s(u, v) = cbrt(w(u, v) / max_weight)
//   directed    s(u, v) = cbrt(w(u -> v) / max_weight) + cbrt(w(v -> u) / max_weight), an absent direction adds 0
//   no weights  every cube root is 1: s is 1 (undirected) or the number of directions present, 1 or 2
// networkx's numerator is one masked sparse product, a row intersection per arc:
//   t(u) = sum_{v in N(u) \ {u}}  s(u, v) * sum_{w in N(u) & N(v), w not in {u, v}}  s(u, w) * s(v, w)
// (undirected: 2 x its weighted_triangles; directed: its directed_triangles, whose eight cbrt sums per (v, w) are the
// expansion of the three binomials), and clustering(u) = t == 0 ? 0 : t / denominator(u) with
//   undirected  d (d - 1),                d = |N(u) \ {u}|
//   directed    2 (dt (dt - 1) - 2 db),   dt = the directions present at the off-diagonal entries, db = dt - d
// The cube root is taken once per arc and direction, not once per triangle: the intersection loop multiplies only.
// A quotient that equals 1 has the cube root 1 without a call, so constant weights give the unweighted bits, and for
// a graph without weights every quantity is a small integer in fp64: the quotient t / denominator is networkx's own.
//
// Three stages, each a launch for the hub rows (one workgroup per row longer than GRX_HUB_FACTOR * L) and one for the
// rest (a group of L lanes per row), as in grx_structural_holes.hip:
//   (a) per row: s of every arc, the row of every arc, and the denominator from the counted directions;
//   (b) per arc (u, v), u != v: a group of L lanes walks the shorter of the two rows, lane k entries k, k + L, ...,
//       and looks every entry up in the longer row by binary search (columns ascend); a hit w outside {u, v} adds
//       s(u, w) * s(v, w); the lanes' partial sums meet in the fixed butterfly grx_group_sum<L>; lane 0 writes
//       s(u, v) * sum.  Bound: sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers,
//       plus one 8-byte gather per hit (s of the found entry; s of the walked entry streams with its column):
//       latency- and gather-bound like the ego-net join;
//   (c) per row: the sum of its arcs' terms, lane k the arcs k, k + L, ... in order, then the same butterfly (hub rows:
//       thread t the arcs t, t + 256, ..., then a fixed tree in LDS), and the quotient.
// No floating-point atomics, no hand-off between workgroups inside a launch: every output has the same bits in every
// run.
//
// Compiled with -ffp-contract=off (Makefile; the pragma carries it with the file): every quotient, product and sum is
// its own IEEE operation, so tests/clustering_oracle.py can form the same terms.
#pragma clang fp contract(off)

#include "grx_common.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_ROW_MAX_WG = 2048;      // workgroups of the row kernels (a) and (c)
constexpr int CL_ARC_MAX_WG = 8192;      // workgroups of the per-arc kernel (b)

struct ClWs {
    double *s, *term, *den;
    int32_t *arc_row;
};

size_t cl_ws_bytes(int64_t n, int64_t nnz)
{
    const size_t vec = grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256);
    const size_t arc = grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 8, 256);
    return vec + 2 * arc + grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 4, 256);
}

ClWs cl_carve(void *base, int64_t n, int64_t nnz)
{
    char *p = reinterpret_cast<char *>(base);
    const size_t vec = grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256);
    const size_t arc = grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 8, 256);
    ClWs w;
    w.den = reinterpret_cast<double *>(p); p += vec;
    w.s = reinterpret_cast<double *>(p); p += arc;
    w.term = reinterpret_cast<double *>(p); p += arc;
    w.arc_row = reinterpret_cast<int32_t *>(p);
    return w;
}

// fixed-tree workgroup sum (every thread passes its value; the result is valid in thread 0)
__device__ __forceinline__ double block_sum(double v, double *sm)
{
    const int t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = CL_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] = sm[t] + sm[t + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// cbrt(w / max_weight); a quotient of exactly 1 needs no call
__device__ __forceinline__ double cl_root(double w, double max_weight)
{
    const double q = w / max_weight;
    return q == 1.0 ? 1.0 : cbrt(q);
}

// s of arc j; *dirs = the directions present there (a negative value marks an absent one)
__device__ __forceinline__ double cl_arc_value(const double *__restrict__ fwd, const double *__restrict__ bwd,
                                               int64_t j, double max_weight, double *dirs)
{
    const double f = fwd[j];
    if (!bwd) {
        *dirs = 1.0;
        return cl_root(f, max_weight);
    }
    const double b = bwd[j];
    const double sf = f >= 0.0 ? cl_root(f, max_weight) : 0.0;
    const double sb = b >= 0.0 ? cl_root(b, max_weight) : 0.0;
    *dirs = (f >= 0.0 ? 1.0 : 0.0) + (b >= 0.0 ? 1.0 : 0.0);
    return sf + sb;
}

// d (d - 1) resp. 2 (dt (dt - 1) - 2 db) from the exact counts d = off-diagonal entries, dt = their directions
__device__ __forceinline__ double cl_denominator(bool directed, double d, double dt)
{
    const int64_t di = (int64_t)d, dti = (int64_t)dt;
    return directed ? (double)(2 * (dti * (dti - 1) - 2 * (dti - di))) : (double)(di * (di - 1));
}

// ---- (a) per row --------------------------------------------------------------------------------------------------
// fwd == NULL: no value array is read and s is not written (every s is 1)
__global__ __launch_bounds__(CL_BLOCK) void cl_rows_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ col,
                                                               const double *__restrict__ fwd,
                                                               const double *__restrict__ bwd, double max_weight,
                                                               const int32_t *__restrict__ hub_rows,
                                                               double *__restrict__ s, double *__restrict__ den,
                                                               int32_t *__restrict__ arc_row)
{
    __shared__ double sm[CL_BLOCK];
    const int32_t u = hub_rows[blockIdx.x];
    const int64_t b = row_ptr[u], e = row_ptr[u + 1];
    double d = 0.0, dt = 0.0;
    for (int64_t j = b + threadIdx.x; j < e; j += CL_BLOCK) {
        arc_row[j] = u;
        double dirs = 1.0;
        if (fwd) s[j] = cl_arc_value(fwd, bwd, j, max_weight, &dirs);
        if (col[j] != u) { d += 1.0; dt += dirs; }
    }
    d = block_sum(d, sm);
    dt = block_sum(dt, sm);
    if (threadIdx.x == 0) den[u] = cl_denominator(bwd != nullptr, d, dt);
}

template <int L>
__global__ __launch_bounds__(CL_BLOCK) void cl_rows_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ fwd,
                                                           const double *__restrict__ bwd, double max_weight,
                                                           int64_t hub_degree, double *__restrict__ s,
                                                           double *__restrict__ den, int32_t *__restrict__ arc_row)
{
    constexpr int RPG = CL_BLOCK / L;                       // rows per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t u = g * RPG + slot;
        int64_t b = 0, e = 0;
        if (u < n) { b = row_ptr[u]; e = row_ptr[u + 1]; }
        const bool hub = e - b > hub_degree;                // cl_rows_hub_kernel's
        double d = 0.0, dt = 0.0;
        if (!hub) {
            for (int64_t j = b + lane; j < e; j += L) {
                arc_row[j] = (int32_t)u;
                double dirs = 1.0;
                if (fwd) s[j] = cl_arc_value(fwd, bwd, j, max_weight, &dirs);
                if (col[j] != (int32_t)u) { d += 1.0; dt += dirs; }
            }
        }
        d = grx_group_sum<L>(d);
        dt = grx_group_sum<L>(dt);
        if (lane == 0 && u < n && !hub) den[u] = cl_denominator(bwd != nullptr, d, dt);
    }
}

// ---- (b) per arc --------------------------------------------------------------------------------------------------
// s == NULL: every s is 1
template <int L>
__global__ __launch_bounds__(CL_BLOCK) void cl_arc_kernel(int64_t nnz, const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col,
                                                          const double *__restrict__ s,
                                                          const int32_t *__restrict__ arc_row,
                                                          double *__restrict__ term)
{
    constexpr int APG = CL_BLOCK / L;                       // arcs per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (nnz + APG - 1) / APG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t j = g * APG + slot;
        double a = 0.0;
        if (j < nnz) {
            const int32_t u = arc_row[j], v = col[j];
            if (u != v) {
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
                    // u and v are tested at the hit: skipping their two searches up front splits the group before
                    // the search loop and measured 6 % slower (profiles/clustering.txt)
                    if (lo < se && col[lo] == w && w != u && w != v) a += s ? s[k] * s[lo] : 1.0;
                }
            }
        }
        a = grx_group_sum<L>(a);
        if (lane == 0 && j < nnz) term[j] = s ? s[j] * a : a;
    }
}

// ---- (c) per row --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cl_emit(int64_t u, double t, const double *__restrict__ den,
                                        double *__restrict__ clustering, double *__restrict__ triangles)
{
    if (triangles) triangles[u] = t;
    clustering[u] = t == 0.0 ? 0.0 : t / den[u];
}

__global__ __launch_bounds__(CL_BLOCK) void cl_reduce_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                 const int32_t *__restrict__ hub_rows,
                                                                 const double *__restrict__ term,
                                                                 const double *__restrict__ den,
                                                                 double *__restrict__ clustering,
                                                                 double *__restrict__ triangles)
{
    __shared__ double sm[CL_BLOCK];
    const int32_t u = hub_rows[blockIdx.x];
    const int64_t b = row_ptr[u], e = row_ptr[u + 1];
    double t = 0.0;
    for (int64_t j = b + threadIdx.x; j < e; j += CL_BLOCK) t += term[j];
    t = block_sum(t, sm);
    if (threadIdx.x == 0) cl_emit(u, t, den, clustering, triangles);
}

template <int L>
__global__ __launch_bounds__(CL_BLOCK) void cl_reduce_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                             int64_t hub_degree, const double *__restrict__ term,
                                                             const double *__restrict__ den,
                                                             double *__restrict__ clustering,
                                                             double *__restrict__ triangles)
{
    constexpr int RPG = CL_BLOCK / L;
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t u = g * RPG + slot;
        int64_t b = 0, e = 0;
        if (u < n) { b = row_ptr[u]; e = row_ptr[u + 1]; }
        const bool hub = e - b > hub_degree;                // cl_reduce_hub_kernel's
        double t = 0.0;
        if (!hub)
            for (int64_t j = b + lane; j < e; j += L) t += term[j];
        t = grx_group_sum<L>(t);
        if (lane == 0 && u < n && !hub) cl_emit(u, t, den, clustering, triangles);
    }
}

// f(std::integral_constant<int, L>) for the lane-group width L = lanes_per_row
template <class F>
void cl_with_lanes(int lanes_per_row, F f)
{
    switch (lanes_per_row) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
    }
}

}  // namespace

extern "C" {

size_t grx_clustering_workspace_bytes(int64_t n, int64_t nnz) { return cl_ws_bytes(n, nnz); }

int grx_clustering(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_fwd, const double *d_bwd,
                   double max_weight, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                   double *d_clustering, double *d_triangles, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_clustering: n = %lld out of range [0, 2^31)", (long long)n);
    GRX_REQUIRE(d_clustering, "grx_clustering: d_clustering is NULL");
    GRX_REQUIRE(d_fwd || !d_bwd, "grx_clustering: d_bwd without d_fwd (a directed graph without weights passes 1 for "
                                 "a present direction)");
    GRX_REQUIRE(!d_fwd || (max_weight > 0.0 && std::isfinite(max_weight)),
                "grx_clustering: max_weight = %g must be finite and > 0", max_weight);
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_workspace, "grx_clustering: null pointer");
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "grx_clustering: lanes_per_row must be 4, 8, 16 or 32 (got %d)", lanes_per_row);
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "grx_clustering: hub list");
    hipStream_t st = grx_stream(stream);
    // the number of arcs is the last row pointer: the workspace is carved by it
    GRX_REQUIRE(workspace_bytes >= cl_ws_bytes(n, 0), "grx_clustering: workspace %zu bytes, need at least %zu",
                workspace_bytes, cl_ws_bytes(n, 0));
    int64_t nnz = 0;
    GRX_CHECK_HIP(hipMemcpyAsync(&nnz, d_row_ptr + n, sizeof(nnz), hipMemcpyDeviceToHost, st));
    GRX_CHECK_HIP(hipStreamSynchronize(st));
    GRX_REQUIRE(nnz >= 0, "grx_clustering: row_ptr[n] = %lld", (long long)nnz);
    GRX_REQUIRE(workspace_bytes >= cl_ws_bytes(n, nnz), "grx_clustering: workspace %zu bytes, need %zu",
                workspace_bytes, cl_ws_bytes(n, nnz));
    const ClWs ws = cl_carve(d_workspace, n, nnz);
    const int64_t hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    const double *s = d_fwd ? ws.s : nullptr;

    if (n_hub_rows)
        cl_rows_hub_kernel<<<(unsigned)n_hub_rows, CL_BLOCK, 0, st>>>(d_row_ptr, d_col, d_fwd, d_bwd, max_weight,
                                                                      d_hub_rows, ws.s, ws.den, ws.arc_row);
    cl_with_lanes(lanes_per_row, [&](auto width) {
        constexpr int L = decltype(width)::value;
        const unsigned rgrid = grx_grid(n, CL_BLOCK / L, CL_ROW_MAX_WG);
        cl_rows_kernel<L><<<rgrid, CL_BLOCK, 0, st>>>(n, d_row_ptr, d_col, d_fwd, d_bwd, max_weight, hub_degree, ws.s,
                                                      ws.den, ws.arc_row);
        if (nnz > 0)
            cl_arc_kernel<L><<<grx_grid(nnz, CL_BLOCK / L, CL_ARC_MAX_WG), CL_BLOCK, 0, st>>>(
                nnz, d_row_ptr, d_col, s, ws.arc_row, ws.term);
        cl_reduce_kernel<L><<<rgrid, CL_BLOCK, 0, st>>>(n, d_row_ptr, hub_degree, ws.term, ws.den, d_clustering,
                                                        d_triangles);
    });
    if (n_hub_rows)
        cl_reduce_hub_kernel<<<(unsigned)n_hub_rows, CL_BLOCK, 0, st>>>(d_row_ptr, d_hub_rows, ws.term, ws.den,
                                                                        d_clustering, d_triangles);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
