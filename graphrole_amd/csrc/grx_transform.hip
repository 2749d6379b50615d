// grx_transform.hip -- role transfer: the node x role memberships of a NEW table under a FIXED role x feature factor.
//
// Reference call site: sklearn NMF(solver='mu').transform(X) = _fit_transform(X, H=components_, update_H=False)
// (sklearn/decomposition/_nmf.py), beta = 2: W0 = sqrt(X.mean() / r) everywhere, then W <- W * (X H^T) / (W H H^T) with
// zero denominators replaced by float32 eps, the error every 10 iterations, stop when (prev - err) / err_init < tol.
//
// With H fixed a row of W only ever needs its own row of Q = X H^T and the r x r matrix B = H H^T: Q is one projection
// pass (grx_project with Z = H^T) and X is never read again.  The loop then runs in blocks of up to ten updates of
//   nmf_transform_block_kernel<R>   one lane per row: its R values of Q and of W in registers (R is a template
//                                   parameter, one instantiation per rank: a vector indexed by a runtime r would live
//                                   in scratch memory), B in LDS, W stored once per block, plus the row's share
//                                   -2 w.q + w B w^T of ||X - W H||^2 - ||X||^2
// against n F 8 bytes per ITERATION of the fit's W pass this moves 3 n r 8 bytes per BLOCK.  The row shares are summed
// per workgroup (fixed tree) and over the workgroups by one wavefront in a fixed order: no floating-point atomics, the
// same bits on every run.
#include "grx_common.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <utility>
#include <vector>

namespace {

constexpr double NMF_EPSILON = 1.1920928955078125e-07;   // np.finfo(np.float32).eps, _nmf.py:39
constexpr int TR_BLOCK = 256;
constexpr int TR_MAX_GRID = GRX_NUM_CU * 8;              // workgroups of the row kernels (grid-stride above that)

// scalars the driver reads back (doubles at the end of the workspace)
enum { TS_SUM = 0, TS_SQ, TS_TERMS, TS_DIRECT, TS_COUNT = 8 };

// sum(X) and ||X||_F^2 in one pass: per-workgroup partials [2][gridDim.x]
__global__ __launch_bounds__(TR_BLOCK) void transform_norms_kernel(int64_t n, int F, const double *__restrict__ X, int64_t ldx,
                                                                   double *__restrict__ partial)
{
    __shared__ double red[TR_BLOCK];
    double s = 0.0, q = 0.0;
    const int64_t stride = (int64_t)gridDim.x * TR_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x; i < n; i += stride) {
#pragma unroll 4
        for (int c = 0; c < F; ++c) {
            const double x = X[(size_t)c * ldx + i];
            s += x;
            q = __fma_rn(x, x, q);
        }
    }
    s = grx_block_reduce<TR_BLOCK>(s, red);
    q = grx_block_reduce<TR_BLOCK>(q, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s;
        partial[gridDim.x + blockIdx.x] = q;
    }
}

// out[blockIdx.x] = sum_b partial[blockIdx.x * nb + b]: one wavefront per output, per-lane sequential sums, one butterfly
__global__ __launch_bounds__(64) void transform_reduce_kernel(const double *__restrict__ partial, int nb, double *__restrict__ out)
{
    const double *src = partial + (size_t)blockIdx.x * nb;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) s += src[b];
    s = grx_group_sum<64>(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// B is constant over the loop, so the compiler would load all R * R entries into registers once (measured: scratch from
// R = 11 on); a compiler-level memory barrier before every row of B makes it read that row from LDS where it is used
#define TR_REREAD_LDS() asm volatile("" ::: "memory")

// `iters` (0 .. 10) multiplicative updates of the rows of W with Q = X H^T and B = H H^T fixed (_nmf.py:_multiplicative_
// update_w, beta = 2, update_H = False: the denominator of every column comes from the W of the previous iteration).
// init != 0: the rows start from sklearn's constant W0 = sqrt(mean(X) / r) (norms[TS_SUM] = sum(X), computed on the
// device so that the first launch needs no read-back) instead of being loaded.  partial[blockIdx.x] = this workgroup's
// sum of -2 w.q + w B w^T over its rows after the updates.
template <int R>
__global__ __launch_bounds__(TR_BLOCK) void nmf_transform_block_kernel(int64_t n, const double *__restrict__ Q, int64_t ldq,
                                                                       double *__restrict__ W, int64_t ldw,
                                                                       const double *__restrict__ B, int iters, int init,
                                                                       const double *__restrict__ norms, double x_size,
                                                                       double *__restrict__ partial)
{
    __shared__ double sB[R * R];
    __shared__ double red[TR_BLOCK];
    for (int idx = threadIdx.x; idx < R * R; idx += TR_BLOCK) sB[idx] = B[idx];
    __syncthreads();
    const double w0 = init ? sqrt((norms[TS_SUM] / x_size) / (double)R) : 0.0;
    double term = 0.0;
    const int64_t stride = (int64_t)gridDim.x * TR_BLOCK;
    for (int64_t row = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x; row < n; row += stride) {
        double q[R], w[R];
#pragma unroll
        for (int k = 0; k < R; ++k) q[k] = Q[(size_t)k * ldq + row];
        if (init) {
#pragma unroll
            for (int k = 0; k < R; ++k) w[k] = w0;
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k) w[k] = W[(size_t)k * ldw + row];
        }
        for (int it = 0; it < iters; ++it) {
            double d[R];
#pragma unroll
            for (int k = 0; k < R; ++k) d[k] = 0.0;
#pragma unroll
            for (int l = 0; l < R; ++l) {
                TR_REREAD_LDS();
#pragma unroll
                for (int k = 0; k < R; ++k) d[k] = __fma_rn(w[l], sB[l * R + k], d[k]);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) w[k] *= q[k] / (d[k] == 0.0 ? NMF_EPSILON : d[k]);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) W[(size_t)k * ldw + row] = w[k];
        double wq = 0.0, wbw = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double bw = 0.0;
            TR_REREAD_LDS();
#pragma unroll
            for (int l = 0; l < R; ++l) bw = __fma_rn(sB[k * R + l], w[l], bw);
            wbw = __fma_rn(w[k], bw, wbw);
            wq = __fma_rn(w[k], q[k], wq);
        }
        term += wbw - 2.0 * wq;
    }
    term = grx_block_reduce<TR_BLOCK>(term, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = term;
}

using BlockKernel = void (*)(int64_t, const double *, int64_t, double *, int64_t, const double *, int, int, const double *,
                             double, double *);
template <int... Rs>
constexpr std::array<BlockKernel, sizeof...(Rs)> block_table(std::integer_sequence<int, Rs...>)
{
    return {nmf_transform_block_kernel<Rs + 1>...};
}
const auto BLOCK_KERNELS = block_table(std::make_integer_sequence<int, GRX_MAX_ROLES>{});

struct TransformLayout {
    char *shared;                                            // the projection, then the direct residual passes
    size_t shared_bytes;
    double *q, *h, *b, *stats, *partial, *scal;
    int64_t ldq;
};

TransformLayout transform_layout(GrxCarve &c, int64_t n, int F, int r)
{
    TransformLayout L;
    L.ldq = (int64_t)grx_align_up((size_t)(n > 0 ? n : 1), 32);
    L.shared_bytes = std::max(grx_project_workspace_bytes(n, r), grx_nmf_workspace_bytes(n, F, r));
    L.shared = c.take<char>(L.shared_bytes);
    L.q = c.take<double>((size_t)r * (size_t)L.ldq);
    L.h = c.take<double>((size_t)r * F);
    L.b = c.take<double>((size_t)r * r);
    L.stats = c.take<double>((size_t)r * 4);
    L.partial = c.take<double>((size_t)2 * TR_MAX_GRID);
    L.scal = c.take<double>(TS_COUNT);
    return L;
}

// pinned block for the few doubles a convergence check reads back; one per host thread
struct Pinned {
    double *ptr = nullptr;
    ~Pinned() { if (ptr) (void)hipHostFree(ptr); }
};
thread_local Pinned g_pinned;

int check_shape(int64_t n, int F, int r)
{
    GRX_REQUIRE(n >= 0, "grx_nmf_transform: n < 0");
    if (F < 1 || r < 1 || F > GRX_MAX_NMF_FEATURES || r > GRX_MAX_ROLES || (r > 16 && r + F > GRX_MAX_NMF_FEATURES)) {
        grx_set_error("grx_nmf_transform: F=%d r=%d outside the compiled limits (F<=%d, r<=%d, and r+F<=%d when r>16)", F, r,
                      GRX_MAX_NMF_FEATURES, GRX_MAX_ROLES, GRX_MAX_NMF_FEATURES);
        return GRX_ERR_UNSUPPORTED;
    }
    return GRX_OK;
}

#define GRX_TRY(expr) do { int rc__ = (expr); if (rc__ != GRX_OK) return rc__; } while (0)

}  // namespace

extern "C" {

size_t grx_nmf_transform_workspace_bytes(int64_t n, int F, int r)
{
    if (F < 1) F = 1;
    if (r < 1) r = 1;
    if (r > GRX_MAX_ROLES) r = GRX_MAX_ROLES;
    return grx_carve_bytes(transform_layout, n, F, r);
}

int grx_nmf_transform(int64_t n, int F, int r, const double *d_X, int64_t ldx, const double *h_H, double tol, int max_iter,
                      double *d_W, int64_t ldw, grx_nmf_info *info, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_TRY(check_shape(n, F, r));
    GRX_REQUIRE(ldx >= n && ldw >= n, "grx_nmf_transform: leading dimension below n");
    GRX_REQUIRE(max_iter >= 0 && tol >= 0.0 && info != nullptr, "grx_nmf_transform: bad tol / max_iter / info");
    info->n_iter = 0;
    info->direct_residuals = 0;
    info->err_init = info->err_last = info->x_sq_norm = 0.0;
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_X && h_H && d_W && d_workspace, "grx_nmf_transform: NULL pointer");
    GrxCarve c(d_workspace);
    const TransformLayout L = transform_layout(c, n, F, r);
    if (workspace_bytes < c.used) {
        grx_set_error("grx_nmf_transform: workspace %zu < %zu", workspace_bytes, c.used);
        return GRX_ERR_WORKSPACE;
    }
    hipStream_t st = grx_stream(stream);
    if (!g_pinned.ptr) GRX_CHECK_HIP(hipHostMalloc(reinterpret_cast<void **>(&g_pinned.ptr), TS_COUNT * 8, hipHostMallocMapped));
    double *host = g_pinned.ptr;

    // Z = H^T (F x r) for the projection, B = H H^T on the host
    std::vector<double> Z((size_t)F * r), Bh((size_t)r * r);
    for (int k = 0; k < r; ++k)
        for (int c = 0; c < F; ++c) Z[(size_t)c * r + k] = h_H[(size_t)k * F + c];
    for (int k = 0; k < r; ++k)
        for (int l = 0; l <= k; ++l) {
            double s = 0.0;
            for (int c = 0; c < F; ++c) s += h_H[(size_t)k * F + c] * h_H[(size_t)l * F + c];
            Bh[(size_t)k * r + l] = Bh[(size_t)l * r + k] = s;
        }
    GRX_CHECK_HIP(hipMemcpyAsync(L.h, h_H, (size_t)r * F * 8, hipMemcpyHostToDevice, st));
    GRX_CHECK_HIP(hipMemcpyAsync(L.b, Bh.data(), (size_t)r * r * 8, hipMemcpyHostToDevice, st));

    const int grid = (int)grx_grid(n, TR_BLOCK, TR_MAX_GRID);
    {
        GRX_PROF(GRX_K_TRANSFORM_NORMS, st);
        transform_norms_kernel<<<grid, TR_BLOCK, 0, st>>>(n, F, d_X, ldx, L.partial);
    }
    GRX_LAUNCH_CHECK();
    transform_reduce_kernel<<<2, 64, 0, st>>>(L.partial, grid, L.scal + TS_SUM);
    GRX_LAUNCH_CHECK();
    GRX_TRY(grx_project(n, F, d_X, ldx, 0, n, Z.data(), r, L.q, L.ldq, L.stats, L.shared, L.shared_bytes, stream));

    const BlockKernel kernel = BLOCK_KERNELS[r - 1];
    const double x_size = (double)n * (double)F;
    auto block = [&](int iters, int init, bool want_terms) -> int {
        {
            GRX_PROF(GRX_K_NMF_TRANSFORM_BLOCK, st);
            kernel<<<grid, TR_BLOCK, 0, st>>>(n, L.q, L.ldq, d_W, ldw, L.b, iters, init, L.scal, x_size, L.partial);
        }
        GRX_LAUNCH_CHECK();
        if (want_terms) {
            transform_reduce_kernel<<<1, 64, 0, st>>>(L.partial, grid, L.scal + TS_TERMS);
            GRX_LAUNCH_CHECK();
        }
        return GRX_OK;
    };
    // ||X - W H||_F: ||X||^2 + sum of the row shares while that does not cancel (the fit's rule: a relative squared
    // residual above 1e-8), the direct pass over X otherwise
    double xx = 0.0;
    auto error_of = [&](double terms, double *err) -> int {
        const double sq = xx + terms;
        if (sq > 1e-8 * xx) { *err = std::sqrt(sq); return GRX_OK; }
        GRX_TRY(grx_nmf_residual(n, F, r, d_X, ldx, d_W, ldw, 0, n, L.h, L.scal + TS_DIRECT, L.shared, L.shared_bytes,
                                 stream));
        GRX_TRY(grx_fetch_begin(host + TS_DIRECT, L.scal + TS_DIRECT, 8, st));
        GRX_TRY(grx_fetch_wait(st));
        *err = std::sqrt(host[TS_DIRECT]);
        info->direct_residuals += 1;
        return GRX_OK;
    };

    // W0 and its error (_nmf.py:826) -- one read-back for sum(X), ||X||^2 and the shares at W0
    GRX_TRY(block(0, 1, true));
    GRX_TRY(grx_fetch_begin(host, L.scal, 3 * 8, st));
    GRX_TRY(grx_fetch_wait(st));
    xx = host[TS_SQ];
    info->x_sq_norm = xx;
    if (!(host[TS_SUM] > 0.0)) {
        // an all-zero table: W0 = 0 stays 0, and sklearn's 0 / 0 comparison never stops the loop
        info->n_iter = max_iter;
        return GRX_OK;
    }
    double err_init = 0.0;
    GRX_TRY(error_of(host[TS_TERMS], &err_init));
    info->err_init = info->err_last = err_init;
    double prev = err_init;
    int n_iter = 0;
    while (n_iter < max_iter) {
        const int step = (max_iter - n_iter) < 10 ? (max_iter - n_iter) : 10;
        const bool check = tol > 0.0 && (n_iter + step) % 10 == 0;
        GRX_TRY(block(step, 0, check));
        n_iter += step;
        if (!check) continue;
        GRX_TRY(grx_fetch_begin(host + TS_TERMS, L.scal + TS_TERMS, 8, st));
        GRX_TRY(grx_fetch_wait(st));
        double err = 0.0;
        GRX_TRY(error_of(host[TS_TERMS], &err));
        info->err_last = err;
        if ((prev - err) / err_init < tol) break;
        prev = err;
    }
    info->n_iter = n_iter;
    GRX_CHECK_HIP(hipStreamSynchronize(st));                  // a last block without a check: W complete on return
    return GRX_OK;
}

}  // extern "C"
