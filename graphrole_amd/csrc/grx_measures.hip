// grx_measures.hip -- node measures of RolX sense making (Henderson et al., KDD 2012): PageRank and eigenvector
// centrality by power iteration, clustering and effective size from the per-node triangle counts.
//
// Power iteration.  One iteration = a pull SpMV over the in-adjacency (a lane group of L lanes per row, rows longer
// than GRX_HUB_FACTOR * L a workgroup each in a launch before it) with a fused epilogue that writes the new vector and
// per-workgroup partials, then a one-workgroup finalize that reduces the partials in a fixed order and sets the
// device `done` word.  The control words and their read-back are those of the device-steered round loops
// (grx_common.h); the loop itself is power_run's own, bounded by max_iter and ending in GRX_ERR_NOT_CONVERGED.
// No floating-point atomics: results are the same bits run to run.
//
// Compiled with -ffp-contract=off (Makefile): the local measures restate networkx's IEEE operations one by one.
#include "grx_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_MAX_WG = 2048;          // workgroups of the row kernels (partials per quantity)

// scalars of the iteration state (doubles) and control words (int32) in the workspace
enum { SC_ERR = 0, SC_SUMSQ, SC_DSUM, SC_NORM, SC_COUNT };
enum { CT_DONE = 0, CT_ITERS, CT_COUNT };
enum { FIN_INIT = 0, FIN_PAGERANK, FIN_NORM, FIN_ERR };

struct PowerWs {
    double *x[2], *y[2], *z, *sinv, *hacc, *part, *scal;
    int32_t *ctrl;
};

PowerWs lay_out(GrxCarve &c, int64_t n)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    PowerWs w;
    double **vectors[] = {&w.x[0], &w.x[1], &w.y[0], &w.y[1], &w.z, &w.sinv, &w.hacc};
    for (double **v : vectors) *v = c.take<double>(nn);
    w.part = c.take<double>(3 * MS_MAX_WG);
    w.scal = c.take<double>(SC_COUNT);
    w.ctrl = c.take<int32_t>(CT_COUNT);
    return w;
}

// PageRank start (networkx: x = 1/N, dangling = S == 0): x, y = x / S, per-workgroup dangling partials
__global__ __launch_bounds__(MS_BLOCK) void pr_init_kernel(int64_t n, const double *__restrict__ S, double x0,
                                                           double *__restrict__ x, double *__restrict__ y,
                                                           double *__restrict__ sinv, double *__restrict__ part,
                                                           int32_t *__restrict__ ctrl)
{
    __shared__ double sm[MS_BLOCK];
    double dang = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MS_BLOCK) {
        const double s = S[v];
        const double si = s != 0.0 ? 1.0 / s : 0.0;
        sinv[v] = si;
        x[v] = x0;
        y[v] = x0 * si;
        if (s == 0.0) dang += x0;
    }
    const double d = grx_block_reduce<MS_BLOCK>(dang, sm);
    if (threadIdx.x == 0) part[MS_MAX_WG + blockIdx.x] = d;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl[CT_DONE] = 0; ctrl[CT_ITERS] = 0; }
}

__global__ __launch_bounds__(MS_BLOCK) void ev_init_kernel(int64_t n, double x0, double *__restrict__ x,
                                                           int32_t *__restrict__ ctrl)
{
    for (int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MS_BLOCK) x[v] = x0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl[CT_DONE] = 0; ctrl[CT_ITERS] = 0; }
}

// hub rows: one workgroup per row, sum_{u in in(v)} src[u] * w  ->  hacc[v]
__global__ __launch_bounds__(MS_BLOCK) void power_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                             const int32_t *__restrict__ col,
                                                             const double *__restrict__ w,
                                                             const int32_t *__restrict__ hub_rows,
                                                             const double *__restrict__ src,
                                                             double *__restrict__ hacc,
                                                             const int32_t *__restrict__ ctrl)
{
    __shared__ double sm[MS_BLOCK];
    if (ctrl[CT_DONE]) return;
    const int32_t v = hub_rows[blockIdx.x];
    const int64_t b = row_ptr[v], e = row_ptr[v + 1];
    double acc = 0.0;
    if (w) for (int64_t j = b + threadIdx.x; j < e; j += MS_BLOCK) acc += src[col[j]] * w[j];
    else   for (int64_t j = b + threadIdx.x; j < e; j += MS_BLOCK) acc += src[col[j]];
    const double s = grx_block_reduce<MS_BLOCK>(acc, sm);
    if (threadIdx.x == 0) hacc[v] = s;
}

// L lanes per row: lane j of a group sums arcs j, j + L, ... then a fixed butterfly.  hub_degree: rows longer than
// this were summed by power_hub_kernel into hacc.
template <int L>
__device__ __forceinline__ double row_pull(int64_t v, int64_t n, const int64_t *__restrict__ row_ptr,
                                           const int32_t *__restrict__ col, const double *__restrict__ w,
                                           const double *__restrict__ src, const double *__restrict__ hacc,
                                           int64_t hub_degree, int lane)
{
    double acc = 0.0;
    int64_t b = 0, e = 0;
    if (v < n) { b = row_ptr[v]; e = row_ptr[v + 1]; }
    const bool hub = e - b > hub_degree;
    if (!hub) {
        if (w) for (int64_t j = b + lane; j < e; j += L) acc += src[col[j]] * w[j];
        else   for (int64_t j = b + lane; j < e; j += L) acc += src[col[j]];
    }
    acc = grx_group_sum<L>(acc);
    return (v < n && hub) ? hacc[v] : acc;
}

// PageRank iteration (networkx _pagerank_scipy):
//   x' = alpha * (x A + sum(x[dangling]) * p) + (1 - alpha) * p,  A = diag(1/S) W,  p = 1/N
// pulled over the in-adjacency as x'[v] = alpha * (sum_u y[u] w(u, v) + dsum * p) + (1 - alpha) * p, y = x / S
template <int L>
__global__ __launch_bounds__(MS_BLOCK) void pr_iter_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ w, int64_t hub_degree,
                                                           const double *__restrict__ x_in,
                                                           const double *__restrict__ y_in,
                                                           const double *__restrict__ hacc,
                                                           const double *__restrict__ sinv, double alpha, double p,
                                                           double teleport, double *__restrict__ x_out,
                                                           double *__restrict__ y_out, double *__restrict__ part,
                                                           const double *__restrict__ scal,
                                                           const int32_t *__restrict__ ctrl)
{
    __shared__ double sm[MS_BLOCK];
    if (ctrl[CT_DONE]) return;
    constexpr int RPG = MS_BLOCK / L;                       // rows per workgroup pass
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const double dsum = scal[SC_DSUM];
    double err = 0.0, dang = 0.0;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t v = g * RPG + slot;
        const double acc = row_pull<L>(v, n, row_ptr, col, w, y_in, hacc, hub_degree, lane);
        if (lane == 0 && v < n) {
            const double xn = alpha * (acc + dsum * p) + teleport;
            const double si = sinv[v];
            err += fabs(xn - x_in[v]);
            x_out[v] = xn;
            y_out[v] = xn * si;
            if (si == 0.0) dang += xn;
        }
    }
    const double e = grx_block_reduce<MS_BLOCK>(err, sm);
    const double d = grx_block_reduce<MS_BLOCK>(dang, sm);
    if (threadIdx.x == 0) { part[blockIdx.x] = e; part[MS_MAX_WG + blockIdx.x] = d; }
}

// eigenvector iteration (networkx eigenvector_centrality): z[v] = x[v] + sum_{u -> v} x[u] w(u, v), partials of z^2
template <int L>
__global__ __launch_bounds__(MS_BLOCK) void ev_iter_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ w, int64_t hub_degree,
                                                           const double *__restrict__ x_in,
                                                           const double *__restrict__ hacc,
                                                           double *__restrict__ z, double *__restrict__ part,
                                                           const int32_t *__restrict__ ctrl)
{
    __shared__ double sm[MS_BLOCK];
    if (ctrl[CT_DONE]) return;
    constexpr int RPG = MS_BLOCK / L;
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    double sq = 0.0;
    const int64_t groups = (n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t v = g * RPG + slot;
        const double acc = row_pull<L>(v, n, row_ptr, col, w, x_in, hacc, hub_degree, lane);
        if (lane == 0 && v < n) {
            const double zv = x_in[v] + acc;
            z[v] = zv;
            sq += zv * zv;
        }
    }
    const double s = grx_block_reduce<MS_BLOCK>(sq, sm);
    if (threadIdx.x == 0) part[2 * MS_MAX_WG + blockIdx.x] = s;
}

// x' = z / norm, partials of |x' - x|
__global__ __launch_bounds__(MS_BLOCK) void ev_normalize_kernel(int64_t n, const double *__restrict__ z,
                                                                const double *__restrict__ x_in,
                                                                double *__restrict__ x_out, double *__restrict__ part,
                                                                const double *__restrict__ scal,
                                                                const int32_t *__restrict__ ctrl)
{
    __shared__ double sm[MS_BLOCK];
    if (ctrl[CT_DONE]) return;
    const double norm = scal[SC_NORM];
    double err = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * MS_BLOCK) {
        const double xn = z[v] / norm;
        err += fabs(xn - x_in[v]);
        x_out[v] = xn;
    }
    const double e = grx_block_reduce<MS_BLOCK>(err, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = e;
}

// one workgroup: reduce `count` partials of a quantity in a fixed order, then act on the total
__global__ __launch_bounds__(MS_BLOCK) void power_finalize_kernel(int mode, int count, const double *__restrict__ part,
                                                                  double thresh, double *__restrict__ scal,
                                                                  int32_t *__restrict__ ctrl)
{
    __shared__ double sm[MS_BLOCK];
    if (ctrl[CT_DONE]) return;
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    const double *pa = mode == FIN_NORM ? part + 2 * MS_MAX_WG : mode == FIN_INIT ? part + MS_MAX_WG : part;
    for (int i = t; i < count; i += MS_BLOCK) {
        a += pa[i];
        if (mode == FIN_PAGERANK) b += part[MS_MAX_WG + i];
    }
    const double ta = grx_block_reduce<MS_BLOCK>(a, sm);
    const double tb = grx_block_reduce<MS_BLOCK>(b, sm);
    if (t != 0) return;
    if (mode == FIN_INIT) { scal[SC_DSUM] = ta; return; }
    if (mode == FIN_NORM) {
        const double nrm = sqrt(ta);
        scal[SC_SUMSQ] = ta;
        scal[SC_NORM] = nrm != 0.0 ? nrm : 1.0;            // networkx: math.hypot(*x.values()) or 1
        return;
    }
    if (mode == FIN_PAGERANK) scal[SC_DSUM] = tb;
    scal[SC_ERR] = ta;
    ctrl[CT_ITERS] += 1;
    if (ta < thresh) ctrl[CT_DONE] = 1;
}

constexpr int MS_BATCH = 8;              // iterations enqueued between two read-backs

template <int L>
void launch_pr_iter(int grid, hipStream_t st, int64_t n, const int64_t *rp, const int32_t *col, const double *w,
                    int64_t hub_degree, const PowerWs &ws, int cur, double alpha, double p, double teleport)
{
    pr_iter_kernel<L><<<grid, MS_BLOCK, 0, st>>>(n, rp, col, w, hub_degree, ws.x[cur], ws.y[cur], ws.hacc, ws.sinv,
                                                 alpha, p, teleport, ws.x[cur ^ 1], ws.y[cur ^ 1], ws.part, ws.scal,
                                                 ws.ctrl);
}

template <int L>
void launch_ev_iter(int grid, hipStream_t st, int64_t n, const int64_t *rp, const int32_t *col, const double *w,
                    int64_t hub_degree, const PowerWs &ws, int cur)
{
    ev_iter_kernel<L><<<grid, MS_BLOCK, 0, st>>>(n, rp, col, w, hub_degree, ws.x[cur], ws.hacc, ws.z, ws.part,
                                                 ws.ctrl);
}

// shared driver of the two power iterations
int power_run(bool pagerank, int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
              const double *d_out_weight, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
              double alpha, double tol, int max_iter, double *d_x, int *h_iterations, void *d_ws, size_t ws_bytes,
              void *stream)
{
    GRX_REQUIRE(n > 0, "power iteration: n = %lld (networkx returns an empty result for an empty graph)", (long long)n);
    GRX_REQUIRE(n < (int64_t)1 << 31, "power iteration: n must be below 2^31");
    GRX_REQUIRE(d_row_ptr && d_col && d_x && d_ws, "power iteration: null pointer");
    GRX_REQUIRE(!pagerank || d_out_weight, "grx_pagerank: d_out_weight is required");
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "power iteration: lanes_per_row must be 4, 8, 16 or 32 (got %d)", lanes_per_row);
    GRX_REQUIRE(n_hub_rows >= 0 && (n_hub_rows == 0 || d_hub_rows), "power iteration: hub list");
    GRX_REQUIRE(max_iter >= 0, "power iteration: max_iter must be >= 0");
    GRX_REQUIRE(tol >= 0.0, "power iteration: tol must be >= 0");
    GrxCarve c(d_ws);
    const PowerWs ws = lay_out(c, n);
    GRX_REQUIRE(ws_bytes >= c.used, "power iteration: workspace %zu bytes, need %zu", ws_bytes, c.used);
    hipStream_t st = grx_stream(stream);
    const int64_t hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    const int rgrid = (int)grx_grid(n, MS_BLOCK / lanes_per_row, MS_MAX_WG);
    const int egrid = (int)grx_grid(n, MS_BLOCK, MS_MAX_WG);
    const double N = (double)n;
    const double p = 1.0 / N;                               // numpy: np.repeat(1.0 / N, N)
    const double teleport = (1.0 - alpha) * p;
    const double thresh = N * tol;                          // networkx: err < N * tol
    if (pagerank) {
        pr_init_kernel<<<egrid, MS_BLOCK, 0, st>>>(n, d_out_weight, p, ws.x[0], ws.y[0], ws.sinv, ws.part, ws.ctrl);
        GRX_LAUNCH_CHECK();
        power_finalize_kernel<<<1, MS_BLOCK, 0, st>>>(FIN_INIT, egrid, ws.part, thresh, ws.scal, ws.ctrl);
    } else {
        ev_init_kernel<<<egrid, MS_BLOCK, 0, st>>>(n, p, ws.x[0], ws.ctrl);   // networkx: nstart = 1, x = 1 / N
    }
    GRX_LAUNCH_CHECK();
    int32_t h[2] = {0, 0};
    int issued = 0;
    while (issued < max_iter) {
        const int batch = std::min(MS_BATCH, max_iter - issued);
        for (int b = 0; b < batch; ++b, ++issued) {
            const int cur = issued & 1;
            if (n_hub_rows)
                power_hub_kernel<<<(unsigned)n_hub_rows, MS_BLOCK, 0, st>>>(d_row_ptr, d_col, d_w, d_hub_rows,
                                                                            pagerank ? ws.y[cur] : ws.x[cur],
                                                                            ws.hacc, ws.ctrl);
            if (pagerank) {
                switch (lanes_per_row) {
                case 4: launch_pr_iter<4>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur, alpha, p, teleport); break;
                case 8: launch_pr_iter<8>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur, alpha, p, teleport); break;
                case 16: launch_pr_iter<16>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur, alpha, p, teleport); break;
                default: launch_pr_iter<32>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur, alpha, p, teleport); break;
                }
                power_finalize_kernel<<<1, MS_BLOCK, 0, st>>>(FIN_PAGERANK, rgrid, ws.part, thresh, ws.scal, ws.ctrl);
            } else {
                switch (lanes_per_row) {
                case 4: launch_ev_iter<4>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur); break;
                case 8: launch_ev_iter<8>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur); break;
                case 16: launch_ev_iter<16>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur); break;
                default: launch_ev_iter<32>(rgrid, st, n, d_row_ptr, d_col, d_w, hub_degree, ws, cur); break;
                }
                power_finalize_kernel<<<1, MS_BLOCK, 0, st>>>(FIN_NORM, rgrid, ws.part, thresh, ws.scal, ws.ctrl);
                ev_normalize_kernel<<<egrid, MS_BLOCK, 0, st>>>(n, ws.z, ws.x[cur], ws.x[cur ^ 1], ws.part, ws.scal,
                                                                ws.ctrl);
                power_finalize_kernel<<<1, MS_BLOCK, 0, st>>>(FIN_ERR, egrid, ws.part, thresh, ws.scal, ws.ctrl);
            }
            GRX_LAUNCH_CHECK();
        }
        const int rc = grx_read_ctrl(ws.ctrl, CT_COUNT, h, st);
        if (rc != GRX_OK) return rc;
        if (h[0]) break;
    }
    if (h_iterations) *h_iterations = h[1];
    if (!h[0]) {
        grx_set_error("power iteration failed to converge within %d iterations", max_iter);
        return GRX_ERR_NOT_CONVERGED;
    }
    // the result of iteration k lies in x[k & 1]
    GRX_CHECK_HIP(hipMemcpyAsync(d_x, ws.x[h[1] & 1], (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    return GRX_OK;
}

// ---- clustering / effective size -------------------------------------------------------------------------------

// loop[v] = 1 iff v lists itself (columns ascending: a binary search)
__global__ __launch_bounds__(MS_BLOCK) void loop_flags_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col,
                                                              uint8_t *__restrict__ loop)
{
    const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= n) return;
    int64_t lo = row_ptr[v], hi = row_ptr[v + 1];
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (col[mid] < v) lo = mid + 1; else hi = mid;
    }
    loop[v] = (lo < row_ptr[v + 1] && col[lo] == (int32_t)v) ? 1 : 0;
}

// networkx 3.4.2, undirected graphs without parallel edges:
//   clustering(v)     = 0 if T == 0 else 2T / (d' (d' - 1))            (_triangles_and_degree_iter: t = 2T, d = d')
//   effective_size(v) = n - 2t / n, n = d', t = T + #loop-carrying neighbours      (Borgatti, ego graph w/o centre)
//                       NaN for an isolated node (networkx) and for a node whose only neighbour is itself (networkx
//                       raises ZeroDivisionError there)
__device__ __forceinline__ void local_measures(int64_t deg, int64_t own_loop, uint64_t T, int64_t nl, double *cl,
                                               double *es)
{
    const int64_t dp = deg - own_loop;
    *cl = T == 0 ? 0.0 : (double)(2 * (int64_t)T) / (double)(dp * (dp - 1));
    if (deg == 0 || dp == 0) {
        *es = __builtin_nan("");
    } else {
        const int64_t t = (int64_t)T + nl;
        *es = (double)dp - (double)(2 * t) / (double)dp;
    }
}

// graph without self-loops: one thread per row
__global__ __launch_bounds__(MS_BLOCK) void local_plain_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                               const uint64_t *__restrict__ T,
                                                               double *__restrict__ cl, double *__restrict__ es)
{
    const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= n) return;
    double c, e;
    local_measures(row_ptr[v + 1] - row_ptr[v], 0, T[v], 0, &c, &e);
    cl[v] = c;
    es[v] = e;
}

// with self-loops: one wavefront per row counts the loop-carrying neighbours (integers: any order is exact)
__global__ __launch_bounds__(MS_BLOCK) void local_loops_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ col,
                                                               const uint8_t *__restrict__ loop,
                                                               const uint64_t *__restrict__ T,
                                                               double *__restrict__ cl, double *__restrict__ es)
{
    const int64_t v = (int64_t)blockIdx.x * (MS_BLOCK / GRX_WAVE) + threadIdx.x / GRX_WAVE;
    const int lane = threadIdx.x % GRX_WAVE;
    if (v >= n) return;                                     // whole wavefronts leave together
    const int64_t b = row_ptr[v], e = row_ptr[v + 1];
    int nl = 0;
    for (int64_t j = b + lane; j < e; j += GRX_WAVE) {
        const int32_t u = col[j];
        if (u != (int32_t)v) nl += loop[u];
    }
#pragma unroll
    for (int off = GRX_WAVE / 2; off > 0; off >>= 1) nl += __shfl_xor(nl, off, GRX_WAVE);
    if (lane == 0) {
        double c, s;
        local_measures(e - b, loop[v], T[v], nl, &c, &s);
        cl[v] = c;
        es[v] = s;
    }
}

}  // namespace

extern "C" {

size_t grx_pagerank_workspace_bytes(int64_t n) { return grx_carve_bytes(lay_out, n); }
size_t grx_eigenvector_centrality_workspace_bytes(int64_t n) { return grx_carve_bytes(lay_out, n); }

int grx_pagerank(int64_t n, const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                 const double *d_out_weight, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                 double alpha, double tol, int max_iter, double *d_x, int *h_iterations, void *d_workspace,
                 size_t workspace_bytes, void *stream)
{
    return power_run(true, n, d_in_row_ptr, d_in_col, d_in_w, d_out_weight, d_hub_rows, n_hub_rows, lanes_per_row,
                     alpha, tol, max_iter, d_x, h_iterations, d_workspace, workspace_bytes, stream);
}

int grx_eigenvector_centrality(int64_t n, const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                               const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row, double tol,
                               int max_iter, double *d_x, int *h_iterations, void *d_workspace, size_t workspace_bytes,
                               void *stream)
{
    return power_run(false, n, d_in_row_ptr, d_in_col, d_in_w, nullptr, d_hub_rows, n_hub_rows, lanes_per_row, 0.0,
                     tol, max_iter, d_x, h_iterations, d_workspace, workspace_bytes, stream);
}

int grx_local_structure_measures(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const uint64_t *d_T,
                                 uint8_t *d_loop_scratch, double *d_clustering, double *d_effective_size, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_local_structure_measures: n out of range");
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_T && d_clustering && d_effective_size, "grx_local_structure_measures: null pointer");
    GRX_REQUIRE(!d_loop_scratch || d_col, "grx_local_structure_measures: d_col is required with d_loop_scratch");
    hipStream_t st = grx_stream(stream);
    const unsigned thread_grid = (unsigned)grx_ceil_div(n, MS_BLOCK);
    if (!d_loop_scratch) {
        local_plain_kernel<<<thread_grid, MS_BLOCK, 0, st>>>(n, d_row_ptr, d_T, d_clustering, d_effective_size);
        GRX_LAUNCH_CHECK();
        return GRX_OK;
    }
    loop_flags_kernel<<<thread_grid, MS_BLOCK, 0, st>>>(n, d_row_ptr, d_col, d_loop_scratch);
    GRX_LAUNCH_CHECK();
    const unsigned wave_grid = (unsigned)grx_ceil_div(n, MS_BLOCK / GRX_WAVE);
    local_loops_kernel<<<wave_grid, MS_BLOCK, 0, st>>>(n, d_row_ptr, d_col, d_loop_scratch, d_T, d_clustering,
                                                       d_effective_size);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
