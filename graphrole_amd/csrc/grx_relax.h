// grx_relax.h -- the batched Bellman-Ford relaxation that grx_sssp.hip (distances by weight) and
// grx_weighted_betweenness.hip (the shortest-path DAG behind weighted betweenness) share: the per-arc pull, the source
// initialisation, the round and hub-round kernels and the device-steered round loop.  The header of grx_sssp.hip
// describes the method, what was measured and what was removed; nothing here differs from what that file held.
// Everything has internal linkage: each translation unit instantiates the widths it runs.
#pragma once
#include "grx_common.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_ROUND_BATCH = 8;                            // rounds enqueued between two read-backs
constexpr int SP_MAX_ROW_BLOCKS = 8192;
#define SP_INF __builtin_huge_val()

bool sp_valid_batch(int s) { return s == 16 || s == 32 || s == 64; }

// min of `best` and fl(dist(u, lane) + w(u -> v)) over the arcs [b, e) with stride `step`; w == NULL: every weight
// is 1
template <int S>
__device__ __forceinline__ double pull_min(int64_t b, int64_t e, int step, const int32_t *__restrict__ col,
                                           const double *__restrict__ w, const double *__restrict__ D, int lane,
                                           double best)
{
    int64_t j = b;
    for (; j + 3 * step < e; j += 4 * step) {
        const int64_t u0 = col[j], u1 = col[j + step], u2 = col[j + 2 * step], u3 = col[j + 3 * step];
        const double w0 = w ? w[j] : 1.0, w1 = w ? w[j + step] : 1.0;
        const double w2 = w ? w[j + 2 * step] : 1.0, w3 = w ? w[j + 3 * step] : 1.0;
        const double c0 = D[u0 * S + lane] + w0, c1 = D[u1 * S + lane] + w1;
        const double c2 = D[u2 * S + lane] + w2, c3 = D[u3 * S + lane] + w3;
        best = fmin(best, fmin(fmin(c0, c1), fmin(c2, c3)));
    }
    for (; j < e; j += step) best = fmin(best, D[(int64_t)col[j] * S + lane] + (w ? w[j] : 1.0));
    return best;
}

// lane b < count: dist(s_b, b) = 0 in both buffers, stamp(s_b) = 0 (one node may be the source of several lanes: each
// lane has its own cell, and every stamp store carries the same value)
template <int S>
__global__ __launch_bounds__(SP_BLOCK) void sp_source_init_kernel(int64_t n, int count, const int32_t *__restrict__ src,
                                                                  double *__restrict__ d0, double *__restrict__ d1,
                                                                  int32_t *__restrict__ stamp,
                                                                  int32_t *__restrict__ ctrl)
{
    const int b = threadIdx.x;
    if (b < count) {
        const int64_t s = src[b];
        if (s >= 0 && s < n) {                              // an id outside [0, n) is never written through
            d0[s * S + b] = 0.0;
            d1[s * S + b] = 0.0;
            stamp[s] = 0;
        }
    }
    if (threadIdx.x == 0) { ctrl[GRX_CT_DONE] = 0; ctrl[GRX_CT_LEVEL] = 0; ctrl[GRX_CT_FOUND] = 0; }
}

// one round, rows up to hub_degree arcs: S lanes per node, SP_BLOCK / S nodes per workgroup and grid step
template <int S>
__global__ __launch_bounds__(SP_BLOCK) void sp_round_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                            const int32_t *__restrict__ col,
                                                            const double *__restrict__ w, int64_t hub_degree,
                                                            double *d0, double *d1, int32_t *stamp,
                                                            int32_t *__restrict__ ctrl)
{
    constexpr int GROUPS = SP_BLOCK / S;
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    const double *D = (l & 1) ? d1 : d0;
    double *Dn = (l & 1) ? d0 : d1;
    const int lane = threadIdx.x % S;
    const int group_shift = threadIdx.x % GRX_WAVE / S * S;  // first lane of this node's group in its wavefront
    const unsigned long long group_bits = S == GRX_WAVE ? ~0ull : (1ull << (S % GRX_WAVE)) - 1;
    int found = 0;
    // the trip count is the same in every lane of the workgroup: the ballot below sees every lane
    for (int64_t first = (int64_t)blockIdx.x * GROUPS; first < n; first += (int64_t)gridDim.x * GROUPS) {
        const int64_t v = first + threadIdx.x / S;
        bool lower = false;
        if (v < n) {
            const int64_t b = row_ptr[v], e = row_ptr[v + 1];
            if (e - b <= hub_degree) {                      // longer rows: sp_round_hub_kernel
                const int64_t cell = v * S + lane;
                const double cur = D[cell];
                const int own = stamp[v];
                const double best = pull_min<S>(b, e, 1, col, w, D, lane, cur);
                lower = best < cur;
                if (lower || own >= l) Dn[cell] = best;
            }
        }
        const unsigned long long moved = (__ballot(lower) >> group_shift) & group_bits;
        if (moved && lane == 0) {
            stamp[v] = l + 1;
            found = 1;
        }
    }
    if (__ballot(found != 0) && threadIdx.x % GRX_WAVE == 0) ctrl[GRX_CT_FOUND] = 1;
}

// one round, hub rows: one workgroup per hub row; SP_BLOCK / S lane groups take every (SP_BLOCK / S)-th arc
template <int S>
__global__ __launch_bounds__(SP_BLOCK) void sp_round_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                const int32_t *__restrict__ col,
                                                                const double *__restrict__ w,
                                                                const int32_t *__restrict__ hub_rows, double *d0,
                                                                double *d1, int32_t *stamp,
                                                                int32_t *__restrict__ ctrl)
{
    constexpr int GROUPS = SP_BLOCK / S;
    __shared__ double part[SP_BLOCK];
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    const double *D = (l & 1) ? d1 : d0;
    double *Dn = (l & 1) ? d0 : d1;
    const int t = threadIdx.x, lane = t % S;
    const int64_t v = hub_rows[blockIdx.x];
    part[t] = pull_min<S>(row_ptr[v] + t / S, row_ptr[v + 1], GROUPS, col, w, D, lane, SP_INF);
    __syncthreads();
#pragma unroll
    for (int s = SP_BLOCK / 2; s >= S; s >>= 1) {          // part[t] for t < S: the minimum over every group
        if (t < s) part[t] = fmin(part[t], part[t + s]);
        __syncthreads();
    }
    if (t >= GRX_WAVE) return;
    bool lower = false;
    if (t < S) {
        const int64_t cell = v * S + t;
        const double cur = D[cell];
        const double best = fmin(cur, part[t]);
        lower = best < cur;
        if (lower || stamp[v] >= l) Dn[cell] = best;
    }
    if (__ballot(lower) && t == 0) {                        // behind the stamp reads of its own wavefront
        stamp[v] = l + 1;
        ctrl[GRX_CT_FOUND] = 1;
    }
}

// One batch: `count` <= S sources d_src[0 .. count) relaxed from +inf until a round lowers nothing; d0 and d1 then
// both hold the fixed point.  *rounds += the rounds run.  `what`: the message of the refusal after n + 1 rounds (one
// %lld); prof_id: the GRX_PROF id the rounds are timed under.
template <int S>
int sp_relax(const SpPull &g, const int32_t *d_src, int count, double *d0, double *d1, int32_t *stamp, int32_t *ctrl,
             const char *what, int prof_id, int64_t *rounds, hipStream_t st)
{
    const int64_t n = g.n;
    const unsigned row_blocks = grx_grid(n, SP_BLOCK / S, SP_MAX_ROW_BLOCKS);
    const uint64_t inf_bits = (uint64_t)0x7ff << 52;
    grx_fill64(reinterpret_cast<uint64_t *>(d0), n * S, inf_bits, st);
    grx_fill64(reinterpret_cast<uint64_t *>(d1), n * S, inf_bits, st);
    grx_fill32(stamp, n, -1, st);
    sp_source_init_kernel<S><<<1, SP_BLOCK, 0, st>>>(n, count, d_src, d0, d1, stamp, ctrl);
    GRX_LAUNCH_CHECK();
    int32_t h[2];
    // at most n - 1 rounds lower a distance; one more finds that nothing moves
    const int rc = grx_run_rounds(what, SP_ROUND_BATCH, n + 1, 2, ctrl, h, st, [&] {
        GRX_PROF(prof_id, st);
        if (g.n_hub_rows)
            sp_round_hub_kernel<S><<<(unsigned)g.n_hub_rows, SP_BLOCK, 0, st>>>(g.row_ptr, g.col, g.w, g.hub_rows, d0,
                                                                                d1, stamp, ctrl);
        sp_round_kernel<S><<<row_blocks, SP_BLOCK, 0, st>>>(n, g.row_ptr, g.col, g.w, g.hub_degree, d0, d1, stamp,
                                                            ctrl);
        return grx_frontier_advance(ctrl, st);
    });
    if (rc != GRX_OK) return rc;
    *rounds += (int64_t)h[GRX_CT_LEVEL] + 1;
    return GRX_OK;
}

}  // namespace
