// grx_structural_holes.hip -- Burt's structural-hole measures of RolX sense making: constraint, local constraint and
// the weighted / directed form of effective size, as networkx 3.4.2's structuralholes.py defines them.
//
// Over a structurally symmetric CSR with symmetric mutual weights z (NULL: every z = 1)
//   S(u) = sum_x z(u, x),  X(u) = max_x z(u, x),  P(u, v) = z(u, v) / S(u),  M(v, w) = z(v, w) / X(v)   (0 / 0 = 0)
//   local(u, v)       = (P(u, v) + sum_w P(u, w) P(w, v))^2          constraint(u)     = sum_v local(u, v)
//   effective_size(u) = sum_v (1 - sum_w P(u, w) M(v, w))
// where v runs over row u and w over the common entries of the rows of u and v: both inner sums are one masked sparse
// product, a row intersection per arc.  z(w, v) is read as z(v, w), the entry of row v that the intersection finds.
//
// Three stages, each a launch for the hub rows (one workgroup per row longer than GRX_HUB_FACTOR * L) and one for the
// rest (a group of L lanes per row):
//   (a) row statistics: S and X of every row, and the row of every arc (the per-arc stage is parallel over arcs);
//   (b) per arc (u, v): a group of L lanes walks the shorter of the two rows, lane k entries k, k + L, ..., and looks
//       every entry up in the longer row by binary search (columns ascend); a hit w adds P(u, w) * P(w, v) and
//       P(u, w) * M(v, w), every quotient and product rounded on its own; the lanes' partial sums meet in the fixed
//       butterfly grx_group_sum<L>; lane 0 writes local(u, v) and 1 - redundancy(u, v) of the arc.  The 10^4 arcs of
//       a hub row are 10^4 independent groups spread over the chip.
//       Bound: sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers, plus two 8-byte
//       gathers per hit (z of the found entry, S(w)): latency- and gather-bound like the ego-net join;
//   (c) per row: the sum of its arcs' terms, lane k the arcs k, k + L, ... in order, then the same butterfly (hub rows:
//       thread t the arcs t, t + 256, ..., then a fixed tree in LDS).  NaN for a row that is empty in d_out_row_ptr.
// No floating-point atomics, no hand-off between workgroups inside a launch: every output has the same bits in every
// run.
//
// Compiled with -ffp-contract=off (Makefile; the pragma carries it with the file): every quotient, product and sum is
// its own IEEE operation, so tests/structural_holes_oracle.py can form the same terms.
#pragma clang fp contract(off)

#include "grx_common.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int SH_BLOCK = 256;
constexpr int SH_ROW_MAX_WG = 2048;      // workgroups of the row kernels (a) and (c)
constexpr int SH_ARC_MAX_WG = 8192;      // workgroups of the per-arc kernel (b)

struct ShWs {
    double *S, *X, *loc, *red;
    int32_t *arc_row;
};

size_t sh_ws_bytes(int64_t n, int64_t nnz)
{
    const size_t vec = grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256);
    const size_t arc = grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 8, 256);
    return 2 * vec + 2 * arc + grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 4, 256);
}

ShWs sh_carve(void *base, int64_t n, int64_t nnz)
{
    char *p = reinterpret_cast<char *>(base);
    const size_t vec = grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256);
    const size_t arc = grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 8, 256);
    ShWs w;
    w.S = reinterpret_cast<double *>(p); p += vec;
    w.X = reinterpret_cast<double *>(p); p += vec;
    w.loc = reinterpret_cast<double *>(p); p += arc;
    w.red = reinterpret_cast<double *>(p); p += arc;
    w.arc_row = reinterpret_cast<int32_t *>(p);
    return w;
}

template <int WIDTH>
__device__ __forceinline__ double group_max(double v)
{
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WIDTH));
    return v;
}

// fixed-tree workgroup sum / maximum (every thread passes its value; the result is valid in thread 0)
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double *sm)
{
    const int t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = SH_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] = MAX ? fmax(sm[t], sm[t + s]) : sm[t] + sm[t + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// ---- (a) row statistics -------------------------------------------------------------------------------------------
// z == NULL: S = the row length, X = 1 (0 for an empty row); no value array is read
__global__ __launch_bounds__(SH_BLOCK) void sh_stats_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                const double *__restrict__ z,
                                                                const int32_t *__restrict__ hub_rows,
                                                                double *__restrict__ S, double *__restrict__ X,
                                                                int32_t *__restrict__ arc_row)
{
    __shared__ double sm[SH_BLOCK];
    const int32_t u = hub_rows[blockIdx.x];
    const int64_t b = row_ptr[u], e = row_ptr[u + 1];
    double s = 0.0, x = 0.0;
    for (int64_t j = b + threadIdx.x; j < e; j += SH_BLOCK) {
        arc_row[j] = u;
        if (z) { const double zz = z[j]; s += zz; x = fmax(x, zz); }
    }
    if (z) {
        s = block_reduce<false>(s, sm);
        x = block_reduce<true>(x, sm);
    } else {
        s = (double)(e - b);
        x = e > b ? 1.0 : 0.0;
    }
    if (threadIdx.x == 0) { S[u] = s; X[u] = x; }
}

template <int L>
__global__ __launch_bounds__(SH_BLOCK) void sh_stats_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                            const double *__restrict__ z, int64_t hub_degree,
                                                            double *__restrict__ S, double *__restrict__ X,
                                                            int32_t *__restrict__ arc_row)
{
    constexpr int RPG = SH_BLOCK / L;                       // rows per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t u = g * RPG + slot;
        int64_t b = 0, e = 0;
        if (u < n) { b = row_ptr[u]; e = row_ptr[u + 1]; }
        const bool hub = e - b > hub_degree;                // sh_stats_hub_kernel's
        double s = 0.0, x = 0.0;
        if (!hub) {
            for (int64_t j = b + lane; j < e; j += L) {
                arc_row[j] = (int32_t)u;
                if (z) { const double zz = z[j]; s += zz; x = fmax(x, zz); }
            }
        }
        s = grx_group_sum<L>(s);
        x = group_max<L>(x);
        if (!z) { s = (double)(e - b); x = e > b ? 1.0 : 0.0; }
        if (lane == 0 && u < n && !hub) { S[u] = s; X[u] = x; }
    }
}

// ---- (b) per arc --------------------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(SH_BLOCK) void sh_arc_kernel(int64_t nnz, const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col,
                                                          const double *__restrict__ z,
                                                          const int32_t *__restrict__ arc_row,
                                                          const double *__restrict__ S, const double *__restrict__ X,
                                                          double *__restrict__ loc, double *__restrict__ red)
{
    constexpr int APG = SH_BLOCK / L;                       // arcs per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (nnz + APG - 1) / APG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t j = g * APG + slot;
        double a = 0.0, r = 0.0, su = 0.0;
        if (j < nnz) {
            const int32_t u = arc_row[j], v = col[j];
            const int64_t bu = row_ptr[u], eu = row_ptr[u + 1], bv = row_ptr[v], ev = row_ptr[v + 1];
            su = S[u];
            const double xv = X[v];
            const bool walk_u = eu - bu <= ev - bv;         // walk the shorter row, search the longer one
            const int64_t wb = walk_u ? bu : bv, we = walk_u ? eu : ev;
            const int64_t sb = walk_u ? bv : bu, se = walk_u ? ev : eu;
            for (int64_t k = wb + lane; k < we; k += L) {
                const int32_t w = col[k];
                int64_t lo = sb, hi = se;
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (col[mid] < w) lo = mid + 1; else hi = mid;
                }
                if (lo < se && col[lo] == w) {
                    const int64_t ku = walk_u ? k : lo, kv = walk_u ? lo : k;
                    const double zuw = z ? z[ku] : 1.0, zvw = z ? z[kv] : 1.0;
                    const double puw = su != 0.0 ? zuw / su : 0.0;
                    if (loc) {
                        const double sw = S[w];
                        const double pwv = sw != 0.0 ? zvw / sw : 0.0;
                        a += puw * pwv;
                    }
                    if (red) {
                        const double mvw = xv != 0.0 ? zvw / xv : 0.0;
                        r += puw * mvw;
                    }
                }
            }
        }
        a = grx_group_sum<L>(a);
        r = grx_group_sum<L>(r);
        if (lane == 0 && j < nnz) {
            if (loc) {
                const double zuv = z ? z[j] : 1.0;
                const double puv = su != 0.0 ? zuv / su : 0.0;
                const double t = puv + a;
                loc[j] = t * t;
            }
            if (red) red[j] = 1.0 - r;
        }
    }
}

// ---- (c) per row --------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nan_if_empty(const int64_t *__restrict__ out_row_ptr, int64_t u, double v)
{
    return out_row_ptr[u + 1] == out_row_ptr[u] ? __builtin_nan("") : v;
}

__global__ __launch_bounds__(SH_BLOCK) void sh_reduce_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                 const int64_t *__restrict__ out_row_ptr,
                                                                 const int32_t *__restrict__ hub_rows,
                                                                 const double *__restrict__ loc,
                                                                 const double *__restrict__ red,
                                                                 double *__restrict__ constraint,
                                                                 double *__restrict__ effective_size)
{
    __shared__ double sm[SH_BLOCK];
    const int32_t u = hub_rows[blockIdx.x];
    const int64_t b = row_ptr[u], e = row_ptr[u + 1];
    double c = 0.0, s = 0.0;
    for (int64_t j = b + threadIdx.x; j < e; j += SH_BLOCK) {
        if (constraint) c += loc[j];
        if (effective_size) s += red[j];
    }
    c = block_reduce<false>(c, sm);
    s = block_reduce<false>(s, sm);
    if (threadIdx.x == 0) {
        if (constraint) constraint[u] = nan_if_empty(out_row_ptr, u, c);
        if (effective_size) effective_size[u] = nan_if_empty(out_row_ptr, u, s);
    }
}

template <int L>
__global__ __launch_bounds__(SH_BLOCK) void sh_reduce_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                             const int64_t *__restrict__ out_row_ptr,
                                                             int64_t hub_degree, const double *__restrict__ loc,
                                                             const double *__restrict__ red,
                                                             double *__restrict__ constraint,
                                                             double *__restrict__ effective_size)
{
    constexpr int RPG = SH_BLOCK / L;
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t u = g * RPG + slot;
        int64_t b = 0, e = 0;
        if (u < n) { b = row_ptr[u]; e = row_ptr[u + 1]; }
        const bool hub = e - b > hub_degree;                // sh_reduce_hub_kernel's
        double c = 0.0, s = 0.0;
        if (!hub) {
            for (int64_t j = b + lane; j < e; j += L) {
                if (constraint) c += loc[j];
                if (effective_size) s += red[j];
            }
        }
        c = grx_group_sum<L>(c);
        s = grx_group_sum<L>(s);
        if (lane == 0 && u < n && !hub) {
            if (constraint) constraint[u] = nan_if_empty(out_row_ptr, u, c);
            if (effective_size) effective_size[u] = nan_if_empty(out_row_ptr, u, s);
        }
    }
}

// f(std::integral_constant<int, L>) for the lane-group width L = lanes_per_row
template <class F>
void sh_with_lanes(int lanes_per_row, F f)
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

size_t grx_structural_holes_workspace_bytes(int64_t n, int64_t nnz) { return sh_ws_bytes(n, nnz); }

int grx_structural_holes(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_z,
                         const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                         const int64_t *d_out_row_ptr, double *d_constraint, double *d_effective_size,
                         double *d_local, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_structural_holes: n = %lld out of range [0, 2^31)", (long long)n);
    GRX_REQUIRE(d_constraint || d_effective_size || d_local,
                "grx_structural_holes: d_constraint, d_effective_size and d_local are all NULL");
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_workspace, "grx_structural_holes: null pointer");
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "grx_structural_holes: lanes_per_row must be 4, 8, 16 or 32 (got %d)", lanes_per_row);
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows),
                "grx_structural_holes: hub list");
    hipStream_t st = grx_stream(stream);
    // the number of arcs is the last row pointer: the workspace is carved by it
    GRX_REQUIRE(workspace_bytes >= sh_ws_bytes(n, 0), "grx_structural_holes: workspace %zu bytes, need at least %zu",
                workspace_bytes, sh_ws_bytes(n, 0));
    int64_t nnz = 0;
    GRX_CHECK_HIP(hipMemcpyAsync(&nnz, d_row_ptr + n, sizeof(nnz), hipMemcpyDeviceToHost, st));
    GRX_CHECK_HIP(hipStreamSynchronize(st));
    GRX_REQUIRE(nnz >= 0, "grx_structural_holes: row_ptr[n] = %lld", (long long)nnz);
    GRX_REQUIRE(workspace_bytes >= sh_ws_bytes(n, nnz), "grx_structural_holes: workspace %zu bytes, need %zu",
                workspace_bytes, sh_ws_bytes(n, nnz));
    const ShWs ws = sh_carve(d_workspace, n, nnz);
    const int64_t hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    const int64_t *out_rp = d_out_row_ptr ? d_out_row_ptr : d_row_ptr;
    // the per-arc terms: local constraint straight into the caller's array when it asks for it
    double *loc = d_local ? d_local : d_constraint ? ws.loc : nullptr;
    double *red = d_effective_size ? ws.red : nullptr;

    const bool per_row = d_constraint || d_effective_size;

    if (n_hub_rows)
        sh_stats_hub_kernel<<<(unsigned)n_hub_rows, SH_BLOCK, 0, st>>>(d_row_ptr, d_z, d_hub_rows, ws.S, ws.X,
                                                                       ws.arc_row);
    sh_with_lanes(lanes_per_row, [&](auto width) {
        constexpr int L = decltype(width)::value;
        const unsigned rgrid = grx_grid(n, SH_BLOCK / L, SH_ROW_MAX_WG);
        sh_stats_kernel<L><<<rgrid, SH_BLOCK, 0, st>>>(n, d_row_ptr, d_z, hub_degree, ws.S, ws.X, ws.arc_row);
        if (nnz > 0)
            sh_arc_kernel<L><<<grx_grid(nnz, SH_BLOCK / L, SH_ARC_MAX_WG), SH_BLOCK, 0, st>>>(
                nnz, d_row_ptr, d_col, d_z, ws.arc_row, ws.S, ws.X, loc, red);
        if (per_row)
            sh_reduce_kernel<L><<<rgrid, SH_BLOCK, 0, st>>>(n, d_row_ptr, out_rp, hub_degree, loc, red, d_constraint,
                                                            d_effective_size);
    });
    if (n_hub_rows && per_row)
        sh_reduce_hub_kernel<<<(unsigned)n_hub_rows, SH_BLOCK, 0, st>>>(d_row_ptr, out_rp, d_hub_rows, loc, red,
                                                                        d_constraint, d_effective_size);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
