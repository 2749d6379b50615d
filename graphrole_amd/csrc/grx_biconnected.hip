// grx_biconnected.hip -- the number of biconnected components every node belongs to (more than one: an articulation
// point) for RolX sense making: what networkx 3.4.2's biconnected_components and articulation_points
// (networkx/algorithms/components/biconnected.py) find with a depth-first search, found here by the data-parallel
// algorithm of Tarjan and Vishkin ("An efficient parallel biconnectivity algorithm", SIAM J. Comput. 1985) on a BFS
// spanning forest.  Input: the CSR of an undirected graph's distinct arcs (symmetric; rows in any order; self-loop
// entries are skipped everywhere).
//
//  1. Connected components: lock-free union-find over the arcs (hook the larger root under the smaller with atomicCAS,
//     pointer jumping while finding), then every label flattened to its root.  The vertices that are their own label
//     -- the smallest id of each component -- are the forest's roots.
//  2. BFS from every root at once (they never meet), one launch per level: level[v], and parent[v] = the SMALLEST id
//     among the neighbours of v one level up (atomicMin; -1 for a root), so the forest is the same in every run.  The
//     vertices are then bucketed by level (histogram, scan, scatter) and every later per-level launch reads only its
//     own bucket.
//  3. Subtree sizes, deepest level first: size[parent] += size[v].
//  4. Preorder numbers, level 0 first: the trees one after another in root order (a scan of the roots' sizes), the
//     children of p -- the entries c of row p with parent[c] == p -- in row order behind pre[p], so that the subtree of
//     v is exactly [pre[v], pre[v] + size[v]).  A hub row's workgroup places its children with a block scan.
//  5. low / high: min / max of pre[v] and of pre[w] over the non-tree neighbours w of v, then deepest level first
//     atomicMin / atomicMax into the parent.
//  6. The auxiliary graph on the tree edges, each named by its child vertex, through the union-find of step 1: the
//     two ends of every non-tree edge, and (w, parent[w]) when the subtree of w reaches outside the subtree of
//     parent[w] (low[w] < pre[v] or high[w] >= pre[v] + size[v], v = parent[w] not a root).  label[c] = the smallest
//     member of c's set: the biconnected component of the tree edge (parent[c], c).
//  7. Counts: the top of component r is parent[c] of any member c whose parent is a root or lies in another component;
//     count[top] += 1 per component, and every non-root adds 1 for its own parent edge.
//
// Steps 2 to 5 are one launch (two with hub rows) per BFS level; each sweep is O(n + m) work (the BFS reads every
// level[] once per level on top: O(D n)).  The BFS levels run as a device-steered round loop (grx_common.h).  A deep
// graph (a path) is bound by launch latency, D launches per sweep; that case is not optimised.
// int32 ids, integer vector atomics only, no floating point.
#include "grx_common.h"
#include "grx_unionfind.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int BC_BLOCK = 256;
constexpr int BC_WAVES = BC_BLOCK / GRX_WAVE;
constexpr int BC_LEVEL_BATCH = 8;                            // BFS levels enqueued between two read-backs
constexpr int BC_MAX_BLOCKS = 2048;
constexpr int BC_LEVEL_BLOCKS = 1024;                        // grid of a per-level launch (the bucket size is on the device)
constexpr int BC_SCAN_ITEMS = 8;
constexpr int BC_SCAN_TILE = BC_BLOCK * BC_SCAN_ITEMS;
constexpr int BC_BINS = 1024;                                // levels counted in LDS first; deeper ones straight in HBM

enum { CT_NCOMP = GRX_CT_BFS_WORDS, CT_COUNT };   // after the three words of the BFS loop

struct BcWs {
    int32_t *uf;                                             // component labels (1), then tree-edge labels (6)
    int32_t *level, *parent, *size, *pre, *low, *high;
    int32_t *order;                                          // the vertices bucketed by level
    int32_t *offs;                                           // [D + 2]: bucket l is order[offs[l] .. offs[l + 1])
    int32_t *top;                                            // scatter cursors (2), then the components' tops (7)
    int32_t *bsum;                                           // tile sums of the scan
    int32_t *ctrl;
};

// ten arrays of n + 2 words, the tile sums, the control words
BcWs lay_out(GrxCarve &c, int64_t n)
{
    const size_t nn = (size_t)(n > 0 ? n : 1) + 2;
    BcWs ws;
    int32_t **arrays[] = {&ws.uf, &ws.level, &ws.parent, &ws.size, &ws.pre, &ws.low, &ws.high, &ws.order, &ws.offs,
                          &ws.top};
    for (int32_t **f : arrays) *f = c.take<int32_t>(nn);
    ws.bsum = c.take<int32_t>(nn / BC_SCAN_TILE + 2);
    ws.ctrl = c.take<int32_t>(GRX_CTRL_MAX_WORDS);
    return ws;
}

// the union-find of steps 1 and 6 and its loads and stores past the L1: grx_unionfind.h (shared with grx_components.hip)
__device__ __forceinline__ int ld(const int32_t *p) { return grx_ld32(p); }
__device__ __forceinline__ void st(int32_t *p, int v) { grx_st32(p, v); }
__device__ __forceinline__ int uf_find(int32_t *p, int x) { return grx_uf_find(p, x); }
__device__ __forceinline__ void uf_union(int32_t *p, int a, int b) { grx_uf_union(p, a, b); }

// exclusive scan of x over the workgroup; *total = the sum.  lds: BC_WAVES ints
__device__ __forceinline__ int block_excl_scan(int x, int *total, int *lds)
{
    const int lane = threadIdx.x % GRX_WAVE, wave = threadIdx.x / GRX_WAVE;
    int incl = x;
#pragma unroll
    for (int off = 1; off < GRX_WAVE; off <<= 1) {
        const int y = __shfl_up(incl, off, GRX_WAVE);
        if (lane >= off) incl += y;
    }
    if (lane == GRX_WAVE - 1) lds[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BC_WAVES; ++w) {
        const int s = lds[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();                                         // lds is free for the caller's next round
    *total = tot;
    return base + incl - x;
}

#define BC_FOR_EACH(v, n) \
    for (int64_t v = (int64_t)blockIdx.x * BC_BLOCK + threadIdx.x; v < (n); v += (int64_t)gridDim.x * BC_BLOCK)

__global__ __launch_bounds__(BC_BLOCK) void bc_iota_kernel(int64_t n, int32_t *__restrict__ a)
{
    BC_FOR_EACH(v, n) a[v] = (int)v;
}

// ---- in-place exclusive scan of a[0 .. m): tile sums, their scan by one workgroup, tiles again
__global__ __launch_bounds__(BC_BLOCK) void bc_scan_reduce_kernel(int64_t m, const int32_t *__restrict__ a,
                                                                  int32_t *__restrict__ bsum)
{
    __shared__ int lds[BC_WAVES];
    const int64_t first = (int64_t)blockIdx.x * BC_SCAN_TILE + (int64_t)threadIdx.x * BC_SCAN_ITEMS;
    int s = 0;
#pragma unroll
    for (int k = 0; k < BC_SCAN_ITEMS; ++k) s += first + k < m ? a[first + k] : 0;
    int total;
    (void)block_excl_scan(s, &total, lds);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(BC_BLOCK) void bc_scan_spine_kernel(int64_t tiles, int32_t *__restrict__ bsum)
{
    __shared__ int lds[BC_WAVES];
    int carry = 0;
    for (int64_t first = 0; first < tiles; first += BC_BLOCK) {
        const int64_t i = first + threadIdx.x;
        int total;
        const int e = block_excl_scan(i < tiles ? bsum[i] : 0, &total, lds);
        if (i < tiles) bsum[i] = carry + e;
        carry += total;
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_scan_down_kernel(int64_t m, int32_t *__restrict__ a,
                                                                const int32_t *__restrict__ bsum)
{
    __shared__ int lds[BC_WAVES];
    const int64_t first = (int64_t)blockIdx.x * BC_SCAN_TILE + (int64_t)threadIdx.x * BC_SCAN_ITEMS;
    int x[BC_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < BC_SCAN_ITEMS; ++k) { x[k] = first + k < m ? a[first + k] : 0; s += x[k]; }
    int total;
    int run = block_excl_scan(s, &total, lds) + bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < BC_SCAN_ITEMS; ++k) {
        if (first + k < m) a[first + k] = run;
        run += x[k];
    }
}

// ---- 1. connected components (each edge once: from its larger end)
__device__ __forceinline__ void cc_row(int v, int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                       int32_t *uf)
{
    for (; j < e; j += step) {
        const int w = col[j];
        if (w < v) uf_union(uf, v, w);
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_cc_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ col, int64_t hub_degree,
                                                         int32_t *uf)
{
    BC_FOR_EACH(v, n) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b <= hub_degree) cc_row((int)v, b, e, 1, col, uf);
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_cc_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                             const int32_t *__restrict__ col,
                                                             const int32_t *__restrict__ hub_rows, int32_t *uf)
{
    const int v = hub_rows[blockIdx.x];
    cc_row(v, row_ptr[v] + threadIdx.x, row_ptr[v + 1], BC_BLOCK, col, uf);
}

__global__ __launch_bounds__(BC_BLOCK) void bc_flatten_kernel(int64_t n, int32_t *uf)
{
    BC_FOR_EACH(v, n) {
        int r = (int)v, next;
        while ((next = ld(uf + r)) != r) r = next;
        st(uf + v, r);
    }
}

// ---- 2. BFS
__global__ __launch_bounds__(BC_BLOCK) void bc_bfs_init_kernel(int64_t n, const int32_t *__restrict__ cc,
                                                               int32_t *__restrict__ level,
                                                               int32_t *__restrict__ parent,
                                                               int32_t *__restrict__ size, int32_t *__restrict__ ctrl)
{
    BC_FOR_EACH(v, n) {
        const bool root = cc[v] == v;
        level[v] = root ? 0 : -1;
        parent[v] = root ? -1 : INT_MAX;
        size[v] = 1;
    }
    if (blockIdx.x == 0 && threadIdx.x < CT_COUNT) ctrl[threadIdx.x] = 0;
}

// v on level l: every neighbour not yet on a level, or put on level l + 1 by this launch, takes the smallest such v
__device__ __forceinline__ bool bfs_row(int v, int l, int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                        int32_t *level, int32_t *parent)
{
    bool found = false;
    for (; j < e; j += step) {
        const int w = col[j];
        if (w == v) continue;
        const int lw = ld(level + w);
        if (lw < 0 || lw == l + 1) {
            atomicMin(parent + w, v);
            if (lw < 0) st(level + w, l + 1);
            found = true;
        }
    }
    return found;
}

__global__ __launch_bounds__(BC_BLOCK) void bc_bfs_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col, int64_t hub_degree,
                                                          int32_t *level, int32_t *parent, int32_t *ctrl)
{
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    bool found = false;
    BC_FOR_EACH(v, n) {
        if (ld(level + v) != l) continue;
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b <= hub_degree) found |= bfs_row((int)v, l, b, e, 1, col, level, parent);
    }
    if (found) st(ctrl + GRX_CT_FOUND, 1);
}

__global__ __launch_bounds__(BC_BLOCK) void bc_bfs_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ hub_rows, int32_t *level,
                                                              int32_t *parent, int32_t *ctrl)
{
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    const int v = hub_rows[blockIdx.x];
    if (ld(level + v) != l) return;
    if (bfs_row(v, l, row_ptr[v] + threadIdx.x, row_ptr[v + 1], BC_BLOCK, col, level, parent)) st(ctrl + GRX_CT_FOUND, 1);
}

// A symmetric CSR leaves no vertex without a level.  One that is not symmetric can (components follow the arcs both
// ways, the BFS one way): such a vertex becomes a root of its own, so that no later kernel indexes with its level or
// parent; what is computed for that input is not defined.
__global__ __launch_bounds__(BC_BLOCK) void bc_bfs_close_kernel(int64_t n, int32_t *__restrict__ level,
                                                                int32_t *__restrict__ parent)
{
    BC_FOR_EACH(v, n) {
        if (level[v] < 0 || parent[v] == INT_MAX) {
            level[v] = 0;
            parent[v] = -1;
        }
    }
}

// ---- buckets by level.  Each workgroup owns one contiguous chunk of the vertices and counts its levels below BC_BINS
// in LDS, so a level costs one global atomic per workgroup, not one per vertex (a shallow graph has few levels)
__global__ __launch_bounds__(BC_BLOCK) void bc_level_hist_kernel(int64_t n, int64_t chunk,
                                                                 const int32_t *__restrict__ level,
                                                                 int32_t *__restrict__ hist)
{
    __shared__ int bins[BC_BINS];
    for (int b = threadIdx.x; b < BC_BINS; b += BC_BLOCK) bins[b] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * chunk, last = first + chunk < n ? first + chunk : n;
    for (int64_t v = first + threadIdx.x; v < last; v += BC_BLOCK) {
        const int l = level[v];
        if (l < BC_BINS) atomicAdd(&bins[l], 1); else atomicAdd(hist + l, 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < BC_BINS; b += BC_BLOCK)
        if (bins[b]) atomicAdd(hist + b, bins[b]);
}

// the order inside a bucket differs from run to run; nothing that is computed depends on it
__global__ __launch_bounds__(BC_BLOCK) void bc_level_scatter_kernel(int64_t n, int64_t chunk,
                                                                    const int32_t *__restrict__ level,
                                                                    const int32_t *__restrict__ offs,
                                                                    int32_t *__restrict__ cursor,
                                                                    int32_t *__restrict__ order)
{
    __shared__ int bins[BC_BINS];                            // this chunk's count per level, then its running rank
    __shared__ int base[BC_BINS];                            // where this chunk's share of the bucket begins
    for (int b = threadIdx.x; b < BC_BINS; b += BC_BLOCK) bins[b] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * chunk, last = first + chunk < n ? first + chunk : n;
    for (int64_t v = first + threadIdx.x; v < last; v += BC_BLOCK) {
        const int l = level[v];
        if (l < BC_BINS) atomicAdd(&bins[l], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < BC_BINS; b += BC_BLOCK) {
        if (bins[b]) base[b] = offs[b] + atomicAdd(cursor + b, bins[b]);
        bins[b] = 0;
    }
    __syncthreads();
    for (int64_t v = first + threadIdx.x; v < last; v += BC_BLOCK) {
        const int l = level[v];
        const int at = l < BC_BINS ? base[l] + atomicAdd(&bins[l], 1) : offs[l] + atomicAdd(cursor + l, 1);
        order[at] = (int)v;
    }
}

#define BC_FOR_LEVEL(i, offs, l) \
    for (int64_t i = (int64_t)(offs)[l] + (int64_t)blockIdx.x * BC_BLOCK + threadIdx.x, i##_end = (offs)[(l) + 1]; \
         i < i##_end; i += (int64_t)gridDim.x * BC_BLOCK)

// ---- 3. subtree sizes
__global__ __launch_bounds__(BC_BLOCK) void bc_size_level_kernel(const int32_t *__restrict__ order,
                                                                 const int32_t *__restrict__ offs, int l,
                                                                 const int32_t *__restrict__ parent, int32_t *size)
{
    BC_FOR_LEVEL(i, offs, l) {
        const int v = order[i];
        atomicAdd(size + parent[v], size[v]);
    }
}

// ---- 4. preorder numbers
__global__ __launch_bounds__(BC_BLOCK) void bc_root_size_kernel(int64_t n, const int32_t *__restrict__ parent,
                                                                const int32_t *__restrict__ size,
                                                                int32_t *__restrict__ pre)
{
    BC_FOR_EACH(v, n) pre[v] = parent[v] < 0 ? size[v] : 0;
}

__global__ __launch_bounds__(BC_BLOCK) void bc_pre_level_kernel(const int32_t *__restrict__ order,
                                                                const int32_t *__restrict__ offs, int l,
                                                                const int64_t *__restrict__ row_ptr,
                                                                const int32_t *__restrict__ col, int64_t hub_degree,
                                                                const int32_t *__restrict__ parent,
                                                                const int32_t *__restrict__ size, int32_t *pre)
{
    BC_FOR_LEVEL(i, offs, l) {
        const int p = order[i];
        const int64_t b = row_ptr[p], e = row_ptr[p + 1];
        if (e - b > hub_degree) continue;                    // bc_pre_hub_kernel
        int at = pre[p] + 1;
        for (int64_t j = b; j < e; ++j) {
            const int c = col[j];
            if (parent[c] == p) {
                pre[c] = at;
                at += size[c];
            }
        }
    }
}

// one workgroup per hub row on level l: BC_BLOCK row entries per round, the children's sizes scanned over the workgroup
__global__ __launch_bounds__(BC_BLOCK) void bc_pre_hub_kernel(const int32_t *__restrict__ hub_rows,
                                                              const int32_t *__restrict__ level, int l,
                                                              const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ parent,
                                                              const int32_t *__restrict__ size, int32_t *pre)
{
    __shared__ int lds[BC_WAVES];
    const int p = hub_rows[blockIdx.x];
    if (level[p] != l) return;
    const int64_t b = row_ptr[p], e = row_ptr[p + 1];
    int at = pre[p] + 1;
    for (int64_t first = b; first < e; first += BC_BLOCK) {  // the same trip count in every lane: the scan has barriers
        const int64_t j = first + threadIdx.x;
        const int c = j < e ? col[j] : -1;
        const bool child = c >= 0 && parent[c] == p;
        int total;
        const int before = block_excl_scan(child ? size[c] : 0, &total, lds);
        if (child) pre[c] = at + before;
        at += total;
    }
}

// ---- 5. low / high
__device__ __forceinline__ void lowhigh_row(int v, int pv, int64_t j, int64_t e, int step,
                                            const int32_t *__restrict__ col, const int32_t *__restrict__ parent,
                                            const int32_t *__restrict__ pre, int *lo, int *hi)
{
    for (; j < e; j += step) {
        const int w = col[j];
        if (w == v || w == pv || parent[w] == v) continue;   // a self-loop or a tree edge
        const int pw = pre[w];
        *lo = pw < *lo ? pw : *lo;
        *hi = pw > *hi ? pw : *hi;
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_lowhigh_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col, int64_t hub_degree,
                                                              const int32_t *__restrict__ parent,
                                                              const int32_t *__restrict__ pre,
                                                              int32_t *__restrict__ low, int32_t *__restrict__ high)
{
    BC_FOR_EACH(v, n) {
        int lo = pre[v], hi = lo;
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b <= hub_degree) lowhigh_row((int)v, parent[v], b, e, 1, col, parent, pre, &lo, &hi);
        low[v] = lo;                                         // a hub row: pre[v], then bc_lowhigh_hub_kernel
        high[v] = hi;
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_lowhigh_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                                  const int32_t *__restrict__ col,
                                                                  const int32_t *__restrict__ hub_rows,
                                                                  const int32_t *__restrict__ parent,
                                                                  const int32_t *__restrict__ pre, int32_t *low,
                                                                  int32_t *high)
{
    const int v = hub_rows[blockIdx.x];
    const int own = pre[v];
    int lo = own, hi = own;
    lowhigh_row(v, parent[v], row_ptr[v] + threadIdx.x, row_ptr[v + 1], BC_BLOCK, col, parent, pre, &lo, &hi);
    if (lo < own) atomicMin(low + v, lo);
    if (hi > own) atomicMax(high + v, hi);
}

__global__ __launch_bounds__(BC_BLOCK) void bc_lowhigh_level_kernel(const int32_t *__restrict__ order,
                                                                    const int32_t *__restrict__ offs, int l,
                                                                    const int32_t *__restrict__ parent, int32_t *low,
                                                                    int32_t *high)
{
    BC_FOR_LEVEL(i, offs, l) {
        const int v = order[i], p = parent[v];
        atomicMin(low + p, low[v]);
        atomicMax(high + p, high[v]);
    }
}

// ---- 6. the auxiliary graph on the tree edges (named by their child vertex)
// In a BFS forest the two ends of a non-tree edge are at most one level apart and neither is the other's parent, so
// neither is an ancestor of the other: every non-tree edge joins unrelated vertices and needs no ancestor test.  A
// root has tree edges only (all its neighbours are on level 1 with it as their only candidate parent).
__device__ __forceinline__ void aux_row(int v, int pv, int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                        const int32_t *__restrict__ parent, int32_t *uf)
{
    for (; j < e; j += step) {
        const int w = col[j];
        if (w > v && w != pv && parent[w] != v) uf_union(uf, v, w);
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_aux_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col, int64_t hub_degree,
                                                          const int32_t *__restrict__ parent,
                                                          const int32_t *__restrict__ size,
                                                          const int32_t *__restrict__ pre,
                                                          const int32_t *__restrict__ low,
                                                          const int32_t *__restrict__ high, int32_t *uf)
{
    BC_FOR_EACH(w, n) {
        const int v = parent[w];
        const int64_t b = row_ptr[w], e = row_ptr[w + 1];
        if (e - b <= hub_degree) aux_row((int)w, v, b, e, 1, col, parent, uf);
        if (v >= 0 && parent[v] >= 0 && (low[w] < pre[v] || high[w] >= pre[v] + size[v])) uf_union(uf, (int)w, v);
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_aux_hub_kernel(const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ hub_rows,
                                                              const int32_t *__restrict__ parent, int32_t *uf)
{
    const int v = hub_rows[blockIdx.x];
    aux_row(v, parent[v], row_ptr[v] + threadIdx.x, row_ptr[v + 1], BC_BLOCK, col, parent, uf);
}

// ---- 7. counts
__global__ __launch_bounds__(BC_BLOCK) void bc_count_init_kernel(int64_t n, const int32_t *__restrict__ parent,
                                                                 const int32_t *__restrict__ uf,
                                                                 int32_t *__restrict__ top, int64_t *__restrict__ count,
                                                                 int32_t *__restrict__ parent_out,
                                                                 int32_t *__restrict__ label_out)
{
    BC_FOR_EACH(v, n) {
        const int p = parent[v];
        top[v] = -1;
        count[v] = p >= 0;                                   // a non-root lies in the component of its parent edge
        if (parent_out) parent_out[v] = p;
        if (label_out) label_out[v] = p >= 0 ? uf[v] : -1;
    }
}

// every writer of top[r] writes the same vertex: the one member of component r nearest to the root
__global__ __launch_bounds__(BC_BLOCK) void bc_top_kernel(int64_t n, const int32_t *__restrict__ parent,
                                                          const int32_t *__restrict__ uf, int32_t *__restrict__ top)
{
    BC_FOR_EACH(c, n) {
        const int p = parent[c];
        if (p < 0) continue;
        const int r = uf[c];
        if (parent[p] < 0 || uf[p] != r) top[r] = p;
    }
}

__global__ __launch_bounds__(BC_BLOCK) void bc_count_kernel(int64_t n, const int32_t *__restrict__ top,
                                                            int64_t *count, int32_t *ctrl)
{
    __shared__ int lds[BC_WAVES];
    int mine = 0;
    BC_FOR_EACH(r, n) {
        const int t = top[r];
        if (t >= 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(count + t), 1ull);
            ++mine;
        }
    }
    int total;
    (void)block_excl_scan(mine, &total, lds);
    if (threadIdx.x == 0 && total) atomicAdd(ctrl + CT_NCOMP, total);
}

int scan_exclusive(int64_t m, int32_t *a, int32_t *bsum, hipStream_t st)
{
    const int64_t tiles = grx_ceil_div(m, BC_SCAN_TILE);
    bc_scan_reduce_kernel<<<(unsigned)tiles, BC_BLOCK, 0, st>>>(m, a, bsum);
    bc_scan_spine_kernel<<<1, BC_BLOCK, 0, st>>>(tiles, bsum);
    bc_scan_down_kernel<<<(unsigned)tiles, BC_BLOCK, 0, st>>>(m, a, bsum);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // namespace

extern "C" {

size_t grx_biconnected_workspace_bytes(int64_t n) { return grx_carve_bytes(lay_out, n); }

int grx_biconnected(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                    int64_t n_hub_rows, int lanes_per_row, int64_t *d_count, int32_t *d_parent, int32_t *d_label,
                    int64_t *n_components, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "grx_biconnected: n = %lld out of range", (long long)n);
    GRX_REQUIRE(d_row_ptr && d_col && d_count && d_workspace, "grx_biconnected: null pointer");
    GRX_REQUIRE(lanes_per_row >= 1, "grx_biconnected: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "grx_biconnected: hub list");
    GrxCarve c(d_workspace);
    const BcWs ws = lay_out(c, n);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_biconnected: workspace %zu bytes, need %zu", workspace_bytes, c.used);
    hipStream_t st = grx_stream(stream);
    const int64_t hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    const unsigned egrid = grx_grid(n, BC_BLOCK, BC_MAX_BLOCKS), hubs = (unsigned)n_hub_rows;
    const unsigned lgrid = std::min<unsigned>(egrid, BC_LEVEL_BLOCKS);

    // 1. connected components
    bc_iota_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.uf);
    bc_cc_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, d_row_ptr, d_col, hub_degree, ws.uf);
    if (hubs) bc_cc_hub_kernel<<<hubs, BC_BLOCK, 0, st>>>(d_row_ptr, d_col, d_hub_rows, ws.uf);
    bc_flatten_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.uf);
    // 2. BFS from every root
    bc_bfs_init_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.uf, ws.level, ws.parent, ws.size, ws.ctrl);
    GRX_LAUNCH_CHECK();
    int32_t h[CT_COUNT];
    // a BFS has at most n - 1 levels; one more launch finds the empty frontier
    int rc = grx_run_rounds(
        "grx_biconnected: the BFS did not end after %lld levels", BC_LEVEL_BATCH, n + 1, CT_COUNT, ws.ctrl, h, st, [&] {
            if (hubs)
                bc_bfs_hub_kernel<<<hubs, BC_BLOCK, 0, st>>>(d_row_ptr, d_col, d_hub_rows, ws.level, ws.parent,
                                                             ws.ctrl);
            bc_bfs_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, d_row_ptr, d_col, hub_degree, ws.level, ws.parent, ws.ctrl);
            return grx_frontier_advance(ws.ctrl, st);
        });
    if (rc != GRX_OK) return rc;
    const int D = h[GRX_CT_LEVEL];                           // levels 0 .. D (the level word stays the deepest level)
    GRX_REQUIRE(D >= 0 && D < n, "grx_biconnected: BFS depth %d", D);
    //    buckets: offs[l] .. offs[l + 1]
    const int64_t chunk = grx_ceil_div(n, egrid);
    bc_bfs_close_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.level, ws.parent);
    grx_fill32(ws.offs, D + 2, 0, st);
    grx_fill32(ws.top, D + 2, 0, st);
    bc_level_hist_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, chunk, ws.level, ws.offs);
    GRX_LAUNCH_CHECK();
    rc = scan_exclusive(D + 2, ws.offs, ws.bsum, st);
    if (rc != GRX_OK) return rc;
    bc_level_scatter_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, chunk, ws.level, ws.offs, ws.top, ws.order);
    // 3. subtree sizes
    for (int l = D; l >= 1; --l)
        bc_size_level_kernel<<<lgrid, BC_BLOCK, 0, st>>>(ws.order, ws.offs, l, ws.parent, ws.size);
    // 4. preorder numbers
    bc_root_size_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.parent, ws.size, ws.pre);
    GRX_LAUNCH_CHECK();
    rc = scan_exclusive(n, ws.pre, ws.bsum, st);
    if (rc != GRX_OK) return rc;
    for (int l = 0; l < D; ++l) {
        bc_pre_level_kernel<<<lgrid, BC_BLOCK, 0, st>>>(ws.order, ws.offs, l, d_row_ptr, d_col, hub_degree, ws.parent,
                                                        ws.size, ws.pre);
        if (hubs)
            bc_pre_hub_kernel<<<hubs, BC_BLOCK, 0, st>>>(d_hub_rows, ws.level, l, d_row_ptr, d_col, ws.parent,
                                                         ws.size, ws.pre);
    }
    GRX_LAUNCH_CHECK();
    // 5. low / high
    bc_lowhigh_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, d_row_ptr, d_col, hub_degree, ws.parent, ws.pre, ws.low, ws.high);
    if (hubs)
        bc_lowhigh_hub_kernel<<<hubs, BC_BLOCK, 0, st>>>(d_row_ptr, d_col, d_hub_rows, ws.parent, ws.pre, ws.low,
                                                         ws.high);
    for (int l = D; l >= 1; --l)
        bc_lowhigh_level_kernel<<<lgrid, BC_BLOCK, 0, st>>>(ws.order, ws.offs, l, ws.parent, ws.low, ws.high);
    GRX_LAUNCH_CHECK();
    // 6. components of the tree edges
    bc_iota_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.uf);
    bc_aux_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, d_row_ptr, d_col, hub_degree, ws.parent, ws.size, ws.pre, ws.low,
                                              ws.high, ws.uf);
    if (hubs) bc_aux_hub_kernel<<<hubs, BC_BLOCK, 0, st>>>(d_row_ptr, d_col, d_hub_rows, ws.parent, ws.uf);
    bc_flatten_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.uf);
    // 7. counts
    bc_count_init_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.parent, ws.uf, ws.top, d_count, d_parent, d_label);
    bc_top_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.parent, ws.uf, ws.top);
    bc_count_kernel<<<egrid, BC_BLOCK, 0, st>>>(n, ws.top, d_count, ws.ctrl);
    GRX_LAUNCH_CHECK();
    if (n_components) {
        rc = grx_read_ctrl(ws.ctrl, CT_COUNT, h, st);
        if (rc != GRX_OK) return rc;
        *n_components = h[CT_NCOMP];
    }
    return GRX_OK;
}

}  // extern "C"
