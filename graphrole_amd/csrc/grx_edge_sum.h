// grx_edge_sum.h -- what grx_edge_betweenness (grx_betweenness.hip) and grx_weighted_edge_betweenness
// (grx_weighted_betweenness.hip) share: the order in which an arc slot adds its sources' terms, and the launches that
// zero the slots before the first batch and finish them after the last.
//
// THE ORDER.  The slot of arc v -> w adds, for every source s of the caller's list, the term sigma_s(v) * coeff_s(w)
// when v -> w is an arc of that source's shortest-path DAG and +0.0 otherwise (networkx's _accumulate_edges forms the
// same product).  The caller's list is cut into aligned groups of EB_GROUP = 16 consecutive sources (positions 16 g ..
// 16 g + 15; the positions past the end of the list hold +0.0).  A group's 16 terms t0 .. t15 are summed by the fixed
// tree  (((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7))) + (((t8 + t9) + (t10 + t11)) + ((t12 + t13) + (t14 + t15)))
// and the groups' sums are added one after another, group 0 first, onto the slot, which starts at +0.0.  Every batch
// width of either entry point (64, 128, 192, 256; 16, 32, 64) is a multiple of 16, so a group never straddles two
// batches and the bits depend on a source's position in the list alone: not on the batch width, the launch shape or the
// run.  A group whose terms are all +0.0 may be left out: x + 0.0 == x for every x a slot can hold (none is -0.0).
// One lane group owns a slot, so there are no floating-point atomics.
//
// Compiled with -ffp-contract=off by both including files (the product sigma * coeff must be rounded before the tree
// adds it); the pragma carries it with the header.
#pragma once
#pragma clang fp contract(off)

#include "grx_common.h"

constexpr int EB_GROUP = 16;                                 // sources per fixed-shape tree
constexpr int EB_BLOCK = 256;
constexpr int EB_ROW_LANES = 16;                             // lanes per row of the launches below
constexpr int EB_MAX_ROW_BLOCKS = 2048;                      // their workgroups (EB_BLOCK / EB_ROW_LANES rows each)

// the tree above over each aligned group of 16 lanes; every lane of a group ends with the group's sum (a + b == b + a
// bit for bit, so the butterfly gives all 16 lanes the same bits)
__device__ __forceinline__ double eb_group_sum(double t)
{
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    t += __shfl_xor(t, 4);
    t += __shfl_xor(t, 8);
    return t;
}

// acc plus the sums of the W / 16 groups of the W-lane group that starts at wavefront lane `base`, lowest group first
template <int W>
__device__ __forceinline__ double eb_add_groups(double acc, double term, int base)
{
    const double g = eb_group_sum(term);
#pragma unroll
    for (int k = 0; k < W / EB_GROUP; ++k) acc += __shfl(g, base + EB_GROUP * k);
    return acc;
}

// does any lane of the W-lane group that starts at wavefront lane `base` hold `pred`
template <int W>
__device__ __forceinline__ bool eb_group_any(bool pred, int base)
{
    const uint64_t hit = __ballot(pred);
    if (W == GRX_WAVE) return hit != 0;
    return ((hit >> base) & (((uint64_t)1 << (W % GRX_WAVE)) - 1)) != 0;
}

// Passes over the arc slots by row (the entry points are not told the number of arcs): EB_ROW_LANES lanes per row u,
// each taking every EB_ROW_LANES-th arc j: u -> v.
//   EB_ZERO     ebc[j] = +0.0, before the first batch
//   EB_SCALE    ebc[j] *= scale                                                  (directed: the slot is the arc)
//   EB_COMBINE  u < v: ebc[j] = (ebc[j] + ebc[k]) * scale, k the slot of v -> u  (undirected: for one source only one
//               of the two arcs is a DAG arc, the edge is their sum); k by binary search in the sorted row v; a
//               missing mirror arc counts 0.0.  Slots with u > v are only read here
//   EB_MIRROR   u > v: ebc[j] = ebc[k], so that both slots of an edge hold its value.  Slots with u < v are only read
// A self-loop slot (u == v) keeps its 0.0 in all of them.
enum EbPass { EB_ZERO, EB_SCALE, EB_COMBINE, EB_MIRROR };

__device__ __forceinline__ int64_t eb_find(const int32_t *__restrict__ col, int64_t lo, int64_t hi, int32_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (col[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int PASS>
__global__ __launch_bounds__(EB_BLOCK) void eb_rows_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col, double scale, double *ebc)
{
    constexpr int ROWS = EB_BLOCK / EB_ROW_LANES;
    const int lane = threadIdx.x % EB_ROW_LANES;
    for (int64_t u = (int64_t)blockIdx.x * ROWS + threadIdx.x / EB_ROW_LANES; u < n; u += (int64_t)gridDim.x * ROWS) {
        const int64_t e = row_ptr[u + 1];
        for (int64_t j = row_ptr[u] + lane; j < e; j += EB_ROW_LANES) {
            if (PASS == EB_ZERO) { ebc[j] = 0.0; continue; }
            if (PASS == EB_SCALE) { ebc[j] *= scale; continue; }
            const int64_t v = col[j];
            if (PASS == EB_COMBINE ? !(u < v) : !(u > v)) continue;
            const int64_t vb = row_ptr[v], ve = row_ptr[v + 1];
            const int64_t k = eb_find(col, vb, ve, (int32_t)u);
            const bool found = k < ve && col[k] == (int32_t)u;
            if (PASS == EB_COMBINE) ebc[j] = (ebc[j] + (found ? ebc[k] : 0.0)) * scale;
            else if (found) ebc[j] = ebc[k];
        }
    }
}

template <int PASS>
static inline void eb_rows(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, double scale, double *d_ebc,
                           hipStream_t st)
{
    eb_rows_kernel<PASS><<<grx_grid(n, EB_BLOCK / EB_ROW_LANES, EB_MAX_ROW_BLOCKS), EB_BLOCK, 0, st>>>(
        n, d_row_ptr, d_col, scale, d_ebc);
}

// after the last batch: the per-arc sums become networkx's edge values
static inline void eb_finish(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, bool directed, double scale,
                             double *d_ebc, hipStream_t st)
{
    if (directed) {
        eb_rows<EB_SCALE>(n, d_row_ptr, d_col, scale, d_ebc, st);
    } else {
        eb_rows<EB_COMBINE>(n, d_row_ptr, d_col, scale, d_ebc, st);
        eb_rows<EB_MIRROR>(n, d_row_ptr, d_col, scale, d_ebc, st);
    }
}
