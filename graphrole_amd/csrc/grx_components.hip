// grx_components.hip -- connected, weakly connected and strongly connected components of a graph, and multi-seed
// reachability (descendants / ancestors), for RolX sense making: which nodes form the giant component, how large the
// component of every node is, and -- from the largest strongly connected component and four closures -- the bow-tie
// position of every node of a directed graph (Broder et al., "Graph structure in the web", 2000).  What networkx
// 3.4.2's connected_components, weakly_connected_components, strongly_connected_components, descendants and ancestors
// find with sequential searches.  Input: the CSR of the graph's distinct arcs, rows in any order, self-loop entries
// allowed (they change nothing); weights are never read.  label[v] = the smallest row id of v's component.
//
// CONNECTED / WEAK: the union-find of grx_biconnected.hip's step 1 (grx_unionfind.h) run on d_label itself: every
// arc hooks the larger root under the smaller, then every label is flattened to its root.  CONNECTED trusts the
// symmetry of its CSR and takes every edge once, from its larger end; WEAK takes every arc of the out-CSR (union is
// symmetric by itself, so the transpose is not needed).
//
// STRONG: trim and colour (Orzan, "On distributed verification and verified distribution", 2004; Barnat, Bauch, Brim
// and Ceska, "Computing strongly connected components in parallel on CUDA", IPDPS 2011).  One ROUND is a fixed set of
// launches; which phase they run is a control word on the device, advanced by a one-thread kernel at the end:
//
//   TRIM    an alive node with no alive out-neighbour other than itself, or no alive in-neighbour other than itself,
//           is a component of its own: label = own id, and it leaves.  Aliveness is as at the START of the round (a
//           node that leaves in round r is stamped gone = r and still counts as alive for the others in round r), so
//           the round is a Jacobi step and its result does not depend on the order of the threads.  Repeats until a
//           round removes nobody, then COLOUR.
//   COLOUR  colour[v] = min(colour[v], colour[u] over the alive in-neighbours u), from colour[v] = v, double-buffered
//           (read one array, write the other: Jacobi again), until a round changes nothing, then CLOSE.  At the fixed
//           point colour[v] is the smallest alive id that reaches v.
//   CLOSE   the nodes with colour[v] == v are pivots.  Level-synchronous closure backward from them, over in-arcs,
//           inside their own colour: the frontier (reached in the round before; the pivots in the first round) stamps
//           every alive, unreached in-neighbour of its colour with the round's number.  Until a round adds nobody.
//   REMOVE  every node reached gets label = colour and leaves.  TRIM again, or done when nobody is alive.
//
// A pivot p is the smallest id that reaches p's component, hence the smallest id OF that component, and the nodes of
// colour p that reach p are exactly that component: the canonical label falls out with no renaming pass.  Every outer
// iteration removes at least the component of the smallest alive id.  The rounds run as a device-steered round loop
// (grx_common.h), CP_ROUND_BATCH rounds per read-back.  h_rounds is the number of rounds that ran (the launches the
// host enqueues after `done` return at once and are not counted), so it is the same in every run, for every lane width.
//
// Rows: a hub row (the CSR's hub list) gets a workgroup in every kernel.  In the STRONG rounds and in grx_reachable
// every other row gets a group of CP_GROUP lanes; in the union-find of CONNECTED / WEAK it gets ONE thread, as in
// bc_cc_kernel of grx_biconnected.hip (up to GRX_HUB_FACTOR * lanes_per_row entries of a row run serially
// there; a lane group for them is not built).  TRIM reads the out- and the in-row of a node, COLOUR and CLOSE
// the in-row.  NOT BUILT: a compacted list of the alive nodes for the
// later rounds (as grx_kcore.hip keeps its next-round list).  Every round sweeps all n rows; a dead row costs one
// 4-byte read.  Bound: rounds x (4 n bytes + the in-arcs of the alive rows), plus the out-arcs in the TRIM rounds.
// KNOWN WORST CASE, not optimised: a chain of k two-cycles whose ids ascend along the chain peels one component per
// outer iteration (k = 32: 32 outer iterations; the same chain with descending ids: 1); a directed cycle of k nodes
// takes 2 k + 2 rounds, a directed path of k nodes trims from both ends in k / 2 rounds.
//
// Sizes: atomicAdd of 1 into count[label[v]] (one add per run of equal labels in a wavefront), then a gather.
//
// grx_reachable: flag[v] != 0 on entry marks the seeds; a level-synchronous closure along the CSR's arcs (the frontier
// push of CLOSE without the colour test) leaves flag = 1 on every seed and every node reachable from one, 0 elsewhere.
//
// int32 ids, integer vector atomics only, whose results do not depend on their order; no floating point.  Every
// output has the same bits in every run and for every lanes_per_row.
#include "grx_common.h"
#include "grx_unionfind.h"

namespace {

constexpr int CP_BLOCK = 256;
constexpr int CP_GROUP = 8;                                  // lanes per row in the row kernels
constexpr int CP_ROUND_BATCH = 16;                           // rounds enqueued between two read-backs
constexpr int CP_MAX_BLOCKS = 2048;                          // per-node launches (256 nodes a workgroup)
constexpr int CP_MAX_ROW_BLOCKS = 8192;                      // row launches (256 / CP_GROUP rows a workgroup)

// control words of the STRONG loop (word 0 = done, word 1 = the round that runs next, from 1)
enum { ST_DONE = 0, ST_ROUND, ST_PHASE, ST_FLAG, ST_LEFT, ST_ALIVE, ST_FIRST, ST_START, ST_CBUF, ST_OUTER, ST_NCOMP,
       ST_WORDS };
enum { PH_TRIM = 0, PH_COLOUR, PH_CLOSE, PH_REMOVE };
// of grx_reachable, after the three words of a BFS loop
enum { RT_COUNT = GRX_CT_BFS_WORDS, RT_WORDS };
static_assert(ST_WORDS <= GRX_CTRL_MAX_WORDS && RT_WORDS <= GRX_CTRL_MAX_WORDS, "control words");

struct CpWs {
    int32_t *gone;                                           // 0 = alive, else the round the node left in
    int32_t *col[2];                                         // the two colour arrays; col[0] holds the size counts afterwards
    int32_t *stamp;                                          // the CLOSE round that reached the node
    int32_t *ctrl;
};

CpWs lay_out(GrxCarve &c, int64_t n)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    CpWs ws;
    ws.gone = c.take<int32_t>(nn);
    ws.col[0] = c.take<int32_t>(nn);
    ws.col[1] = c.take<int32_t>(nn);
    ws.stamp = c.take<int32_t>(nn);
    ws.ctrl = c.take<int32_t>(GRX_CTRL_MAX_WORDS);
    return ws;
}

// of grx_reachable
struct RcWs {
    int32_t *level, *ctrl;
};

RcWs lay_out_reachable(GrxCarve &c, int64_t n)
{
    RcWs ws;
    ws.level = c.take<int32_t>((size_t)(n > 0 ? n : 1));
    ws.ctrl = c.take<int32_t>(GRX_CTRL_MAX_WORDS);
    return ws;
}

struct Csr {
    const int64_t *row_ptr;
    const int32_t *col;
    int64_t hub_degree;
};

#define CP_FOR_EACH(v, n) \
    for (int64_t v = (int64_t)blockIdx.x * CP_BLOCK + threadIdx.x; v < (n); v += (int64_t)gridDim.x * CP_BLOCK)

template <int WIDTH>
__device__ __forceinline__ int group_min(int v)
{
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, WIDTH));
    return v;
}

// the minimum over the workgroup; lds: one int.  Every thread of the workgroup calls it
__device__ __forceinline__ int block_min(int v, int *lds)
{
    if (threadIdx.x == 0) *lds = INT32_MAX;
    __syncthreads();
    v = group_min<GRX_WAVE>(v);
    if (threadIdx.x % GRX_WAVE == 0) atomicMin(lds, v);
    __syncthreads();
    return *lds;
}

// ---- CONNECTED / WEAK ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CP_BLOCK) void cp_iota_kernel(int64_t n, int32_t *__restrict__ a)
{
    CP_FOR_EACH(v, n) a[v] = (int)v;
}

template <bool SYMMETRIC>
__device__ __forceinline__ void cc_row(int v, int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                       int32_t *uf)
{
    for (; j < e; j += step) {
        const int w = col[j];
        if (SYMMETRIC ? w < v : w != v) grx_uf_union(uf, v, w);
    }
}

template <bool SYMMETRIC>
__global__ __launch_bounds__(CP_BLOCK) void cp_cc_kernel(int64_t n, Csr g, int32_t *uf)
{
    CP_FOR_EACH(v, n) {
        const int64_t b = g.row_ptr[v], e = g.row_ptr[v + 1];
        if (e - b <= g.hub_degree) cc_row<SYMMETRIC>((int)v, b, e, 1, g.col, uf);
    }
}

template <bool SYMMETRIC>
__global__ __launch_bounds__(CP_BLOCK) void cp_cc_hub_kernel(int64_t n, Csr g, const int32_t *__restrict__ hub_rows,
                                                             int32_t *uf)
{
    const int v = hub_rows[blockIdx.x];
    if (v < 0 || v >= n) return;                             // an id outside [0, n) is never read through
    cc_row<SYMMETRIC>(v, g.row_ptr[v] + threadIdx.x, g.row_ptr[v + 1], CP_BLOCK, g.col, uf);
}

__global__ __launch_bounds__(CP_BLOCK) void cp_flatten_kernel(int64_t n, int32_t *uf)
{
    CP_FOR_EACH(v, n) grx_uf_flatten(uf, (int)v);
}

// ---- sizes and the number of components --------------------------------------------------------------------------------
// count[label[v]] += 1: one atomic per run of equal labels among the lanes of a wavefront (a giant component: one per
// wavefront, not one per node).  The trip count is the same in every lane of the workgroup: the ballots see every lane
__global__ __launch_bounds__(CP_BLOCK) void cp_count_kernel(int64_t n, const int32_t *__restrict__ label,
                                                            int32_t *count)
{
    const int lane = threadIdx.x % GRX_WAVE;
    for (int64_t first = (int64_t)blockIdx.x * CP_BLOCK; first < n; first += (int64_t)gridDim.x * CP_BLOCK) {
        const int64_t v = first + threadIdx.x;
        const int mine = v < n ? label[v] : -1;
        const int before = __shfl_up(mine, 1, GRX_WAVE);
        const bool head = mine >= 0 && (lane == 0 || before != mine);
        const unsigned long long heads = __ballot(head), valid = __ballot(mine >= 0);
        if (head) {
            // the run ends before the next head, or at the first lane without a node
            const unsigned long long above = lane == GRX_WAVE - 1 ? 0ull : (~0ull << (lane + 1));
            const unsigned long long stop = (heads | ~valid) & above;
            const int end = stop ? __ffsll((long long)stop) - 1 : GRX_WAVE;
            atomicAdd(count + mine, end - lane);
        }
    }
}

__global__ __launch_bounds__(CP_BLOCK) void cp_finish_kernel(int64_t n, const int32_t *__restrict__ label,
                                                             const int32_t *__restrict__ count,
                                                             int64_t *__restrict__ size, int32_t *ncomp)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int roots = 0;
    CP_FOR_EACH(v, n) {
        const int l = label[v];
        roots += l == (int)v;
        if (size) size[v] = count[l];
    }
#pragma unroll
    for (int off = GRX_WAVE / 2; off > 0; off >>= 1) roots += __shfl_xor(roots, off, GRX_WAVE);
    if (threadIdx.x % GRX_WAVE == 0 && roots) atomicAdd(&total, roots);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(ncomp, total);
}

// ---- STRONG ----------------------------------------------------------------------------------------------------------
struct Strong {
    int64_t n;
    Csr out, in;
    CpWs ws;
    int32_t *label;
};

__global__ __launch_bounds__(CP_BLOCK) void st_init_kernel(Strong s)
{
    CP_FOR_EACH(v, s.n) {
        s.ws.gone[v] = 0;
        s.ws.stamp[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < ST_WORDS) {
        const int k = threadIdx.x;
        s.ws.ctrl[k] = k == ST_ROUND ? 1 : k == ST_ALIVE ? (int32_t)s.n : 0;
    }
}

// what a round's kernels read from the control words
struct Round {
    int r, phase, first, start;
    const int32_t *cur;                                      // the colours this round reads
    int32_t *next;                                           // and the array a COLOUR round writes
};

__device__ __forceinline__ Round round_of(const CpWs &ws)
{
    Round q;
    q.r = ws.ctrl[ST_ROUND];
    q.phase = ws.ctrl[ST_PHASE];
    q.first = ws.ctrl[ST_FIRST];
    q.start = ws.ctrl[ST_START];
    const int b = q.phase == PH_COLOUR ? (q.r & 1) : ws.ctrl[ST_CBUF];
    q.cur = ws.col[b];
    q.next = ws.col[b ^ 1];
    return q;
}

// TRIM: 1 when no entry of the lane's share of the row is another node alive at the start of round r
__device__ __forceinline__ int trim_scan(int v, int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                         const int32_t *gone, int r)
{
    for (; j < e; j += step) {
        const int u = col[j];
        if (u == v) continue;
        const int gu = grx_ld32(gone + u);
        if (gu == 0 || gu == r) return 0;
    }
    return 1;
}

// v leaves in round r as a component of its own; the out-row's and the in-row's scan may both say so: counted once
__device__ __forceinline__ void trim_leave(const Strong &s, int v, int r, int *left)
{
    if (atomicCAS(s.ws.gone + v, 0, r) == 0) {
        s.label[v] = v;
        atomicAdd(left, 1);
    }
}

// COLOUR: the minimum of the colours of the alive entries of the lane's share of the in-row
__device__ __forceinline__ int colour_scan(int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                           const int32_t *__restrict__ gone, const Round &q)
{
    int c = INT32_MAX;
    for (; j < e; j += step) {
        const int u = col[j];
        if (gone[u]) continue;
        c = min(c, q.first ? u : q.cur[u]);
    }
    return c;
}

// CLOSE: is v in the frontier of round r, and has u been reached
__device__ __forceinline__ bool close_frontier(const CpWs &ws, const Round &q, int v)
{
    if (ws.gone[v]) return false;
    return q.r == q.start ? q.cur[v] == v : grx_ld32(ws.stamp + v) == q.r - 1;
}

// the frontier node v of colour c stamps the alive, unreached entries of its colour in the lane's share of its in-row
__device__ __forceinline__ bool close_push(const CpWs &ws, const Round &q, int c, int64_t j, int64_t e, int step,
                                           const int32_t *__restrict__ col)
{
    bool found = false;
    for (; j < e; j += step) {
        const int u = col[j];
        if (ws.gone[u] || q.cur[u] != c || c == u) continue;  // c == u: the pivot itself
        if (grx_ld32(ws.stamp + u) >= q.start) continue;     // reached, in an earlier round or by another thread
        grx_st32(ws.stamp + u, q.r);
        found = true;
    }
    return found;
}

// one workgroup per hub row of one CSR (`inward`: the in CSR, whose rows COLOUR and CLOSE read)
__global__ __launch_bounds__(CP_BLOCK) void st_hub_kernel(Strong s, const int32_t *__restrict__ hub_rows, int inward)
{
    __shared__ int lds, own_gone, own_flag;
    const CpWs &ws = s.ws;
    if (ws.ctrl[ST_DONE]) return;
    const Round q = round_of(ws);
    if (q.phase == PH_REMOVE || (!inward && q.phase != PH_TRIM)) return;
    const int v = hub_rows[blockIdx.x];
    if (v < 0 || v >= s.n) return;                           // an id outside [0, n) is never read through
    const Csr &g = inward ? s.in : s.out;
    const int t = threadIdx.x;
    if (t == 0) {                                            // one read: every wavefront takes the same branch
        own_gone = ws.gone[v];
        own_flag = q.phase == PH_CLOSE && close_frontier(ws, q, v);
    }
    __syncthreads();
    const int64_t b = g.row_ptr[v] + t, e = g.row_ptr[v + 1];
    if (q.phase == PH_TRIM) {
        if (own_gone) return;
        const int none = block_min(trim_scan(v, b, e, CP_BLOCK, g.col, ws.gone, q.r), &lds);
        if (t == 0 && none) trim_leave(s, v, q.r, ws.ctrl + ST_LEFT);
    } else if (q.phase == PH_COLOUR) {
        if (own_gone) return;
        const int c = block_min(colour_scan(b, e, CP_BLOCK, g.col, ws.gone, q), &lds);
        if (t == 0) {
            const int old = q.first ? v : q.cur[v];
            q.next[v] = min(old, c);
            if (c < old) grx_st32(ws.ctrl + ST_FLAG, 1);
        }
    } else {
        if (!own_flag) return;
        if (close_push(ws, q, q.cur[v], b, e, CP_BLOCK, g.col)) grx_st32(ws.ctrl + ST_FLAG, 1);
    }
}

// every row that is not a hub row of the CSR a phase reads: CP_GROUP lanes per row
__global__ __launch_bounds__(CP_BLOCK) void st_rows_kernel(Strong s)
{
    __shared__ int left;
    const CpWs &ws = s.ws;
    if (ws.ctrl[ST_DONE]) return;
    const Round q = round_of(ws);
    if (threadIdx.x == 0) left = 0;
    __syncthreads();
    constexpr int ROWS = CP_BLOCK / CP_GROUP;
    const int g = threadIdx.x % CP_GROUP;
    bool flag = false;
    // the lanes of a group share v: they run the same trips and meet again at the reductions
    for (int64_t v = (int64_t)blockIdx.x * ROWS + threadIdx.x / CP_GROUP; v < s.n; v += (int64_t)gridDim.x * ROWS) {
        if (ws.gone[v]) continue;
        const int64_t ob = s.out.row_ptr[v], oe = s.out.row_ptr[v + 1];
        const int64_t ib = s.in.row_ptr[v], ie = s.in.row_ptr[v + 1];
        const bool out_short = oe - ob <= s.out.hub_degree, in_short = ie - ib <= s.in.hub_degree;
        if (q.phase == PH_TRIM) {
            // nobody in the row = every lane of the group met nobody in its share; a hub row is st_hub_kernel's
            const int none_out = group_min<CP_GROUP>(
                out_short ? trim_scan((int)v, ob + g, oe, CP_GROUP, s.out.col, ws.gone, q.r) : 0);
            const int none_in = group_min<CP_GROUP>(
                in_short ? trim_scan((int)v, ib + g, ie, CP_GROUP, s.in.col, ws.gone, q.r) : 0);
            if (g == 0 && (none_out || none_in)) trim_leave(s, (int)v, q.r, &left);
        } else if (q.phase == PH_COLOUR) {
            if (!in_short) continue;                         // st_hub_kernel writes its colour
            const int c = group_min<CP_GROUP>(colour_scan(ib + g, ie, CP_GROUP, s.in.col, ws.gone, q));
            if (g == 0) {
                const int old = q.first ? (int)v : q.cur[v];
                q.next[v] = min(old, c);
                flag |= c < old;
            }
        } else if (q.phase == PH_CLOSE) {
            if (!in_short || !close_frontier(ws, q, (int)v)) continue;
            flag |= close_push(ws, q, q.cur[v], ib + g, ie, CP_GROUP, s.in.col);
        } else if (g == 0) {                                 // PH_REMOVE
            const int c = q.cur[v];
            if (c == (int)v || ws.stamp[v] >= q.start) {
                s.label[v] = c;
                ws.gone[v] = q.r;
                atomicAdd(&left, 1);
            }
        }
    }
    if (flag) grx_st32(ws.ctrl + ST_FLAG, 1);
    __syncthreads();
    if (threadIdx.x == 0 && left) atomicAdd(ws.ctrl + ST_LEFT, left);
}

// one thread: the end of a round
__global__ void st_advance_kernel(CpWs ws)
{
    int32_t *c = ws.ctrl;
    if (c[ST_DONE]) return;
    const int r = c[ST_ROUND], flag = c[ST_FLAG], left = c[ST_LEFT];
    c[ST_FLAG] = 0;
    c[ST_LEFT] = 0;
    switch (c[ST_PHASE]) {
    case PH_TRIM:
        c[ST_ALIVE] -= left;
        if (c[ST_ALIVE] <= 0) { c[ST_DONE] = 1; return; }    // ST_ROUND stays: the number of rounds run
        if (!left) { c[ST_PHASE] = PH_COLOUR; c[ST_FIRST] = 1; }
        break;
    case PH_COLOUR:
        c[ST_FIRST] = 0;
        if (!flag) { c[ST_PHASE] = PH_CLOSE; c[ST_START] = r + 1; c[ST_CBUF] = (r + 1) & 1; }
        break;
    case PH_CLOSE:
        if (!flag) c[ST_PHASE] = PH_REMOVE;
        break;
    default:
        c[ST_ALIVE] -= left;
        c[ST_OUTER] += 1;
        if (c[ST_ALIVE] <= 0) { c[ST_DONE] = 1; return; }
        c[ST_PHASE] = PH_TRIM;
        break;
    }
    c[ST_ROUND] = r + 1;
}

// ---- grx_reachable ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CP_BLOCK) void rc_init_kernel(int64_t n, int32_t *__restrict__ flag,
                                                           int32_t *__restrict__ level, int32_t *__restrict__ ctrl)
{
    CP_FOR_EACH(v, n) {
        const int seed = flag[v] != 0;
        flag[v] = seed;
        level[v] = seed ? 0 : -1;
    }
    if (blockIdx.x == 0 && threadIdx.x < RT_WORDS) ctrl[threadIdx.x] = 0;
}

// v on level l: every entry of its row that has no level yet gets level l + 1 (the same value from every writer)
__device__ __forceinline__ bool reach_push(int l, int64_t j, int64_t e, int step, const int32_t *__restrict__ col,
                                           int32_t *flag, int32_t *level)
{
    bool found = false;
    for (; j < e; j += step) {
        const int u = col[j];
        if (grx_ld32(level + u) >= 0) continue;
        grx_st32(level + u, l + 1);
        flag[u] = 1;
        found = true;
    }
    return found;
}

__global__ __launch_bounds__(CP_BLOCK) void rc_rows_kernel(int64_t n, Csr g, int32_t *flag, int32_t *level,
                                                           int32_t *ctrl)
{
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    constexpr int ROWS = CP_BLOCK / CP_GROUP;
    const int lane = threadIdx.x % CP_GROUP;
    bool found = false;
    for (int64_t v = (int64_t)blockIdx.x * ROWS + threadIdx.x / CP_GROUP; v < n; v += (int64_t)gridDim.x * ROWS) {
        if (grx_ld32(level + v) != l) continue;
        const int64_t b = g.row_ptr[v], e = g.row_ptr[v + 1];
        if (e - b <= g.hub_degree) found |= reach_push(l, b + lane, e, CP_GROUP, g.col, flag, level);
    }
    if (found) grx_st32(ctrl + GRX_CT_FOUND, 1);
}

__global__ __launch_bounds__(CP_BLOCK) void rc_hub_kernel(int64_t n, Csr g, const int32_t *__restrict__ hub_rows,
                                                          int32_t *flag, int32_t *level, int32_t *ctrl)
{
    if (ctrl[GRX_CT_DONE]) return;
    const int l = ctrl[GRX_CT_LEVEL];
    const int v = hub_rows[blockIdx.x];
    if (v < 0 || v >= n) return;                             // an id outside [0, n) is never read through
    if (grx_ld32(level + v) != l) return;                    // a level, once set, stays
    if (reach_push(l, g.row_ptr[v] + threadIdx.x, g.row_ptr[v + 1], CP_BLOCK, g.col, flag, level))
        grx_st32(ctrl + GRX_CT_FOUND, 1);
}

__global__ __launch_bounds__(CP_BLOCK) void rc_count_kernel(int64_t n, const int32_t *__restrict__ flag, int32_t *ctrl)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int mine = 0;
    CP_FOR_EACH(v, n) mine += flag[v];
#pragma unroll
    for (int off = GRX_WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, GRX_WAVE);
    if (threadIdx.x % GRX_WAVE == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(ctrl + RT_COUNT, total);
}

}  // namespace

extern "C" {

size_t grx_components_workspace_bytes(int64_t n) { return grx_carve_bytes(lay_out, n); }

int grx_components(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                   int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                   const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row, int mode,
                   int32_t *d_label, int64_t *d_size, int64_t *n_components, int64_t *h_rounds, void *d_workspace,
                   size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_components: n = %lld out of range", (long long)n);
    GRX_REQUIRE(mode == GRX_COMPONENTS_CONNECTED || mode == GRX_COMPONENTS_WEAK || mode == GRX_COMPONENTS_STRONG,
                "grx_components: mode %d is none of GRX_COMPONENTS_CONNECTED, _WEAK, _STRONG", mode);
    if (n_components) *n_components = 0;
    if (h_rounds) *h_rounds = 0;
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_label && d_workspace, "grx_components: null pointer");
    GRX_REQUIRE(lanes_per_row >= 1, "grx_components: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "grx_components: hub list");
    if (mode == GRX_COMPONENTS_STRONG) {
        GRX_REQUIRE(d_in_row_ptr && d_in_col,
                    "grx_components: GRX_COMPONENTS_STRONG needs the in CSR (the transpose) as well");
        GRX_REQUIRE(in_lanes_per_row >= 1, "grx_components: in_lanes_per_row must be >= 1");
        GRX_REQUIRE(n_in_hub_rows >= 0 && n_in_hub_rows <= n && (n_in_hub_rows == 0 || d_in_hub_rows),
                    "grx_components: hub list (in CSR)");
    } else if (mode == GRX_COMPONENTS_CONNECTED) {
        GRX_REQUIRE(!d_in_row_ptr && !d_in_col && !d_in_hub_rows && n_in_hub_rows == 0 && in_lanes_per_row == 0,
                    "grx_components: GRX_COMPONENTS_CONNECTED takes one symmetric CSR and no in CSR");
    }
    GrxCarve c(d_workspace);
    const CpWs ws = lay_out(c, n);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_components: workspace %zu bytes, need %zu", workspace_bytes, c.used);
    hipStream_t st = grx_stream(stream);
    const Csr out = {d_row_ptr, d_col, (int64_t)GRX_HUB_FACTOR * lanes_per_row};
    const unsigned ngrid = grx_grid(n, CP_BLOCK, CP_MAX_BLOCKS);
    const unsigned rgrid = grx_grid(n, CP_BLOCK / CP_GROUP, CP_MAX_ROW_BLOCKS);
    const unsigned hubs = (unsigned)n_hub_rows;
    int32_t h[ST_WORDS];
    int64_t rounds = 0;

    if (mode == GRX_COMPONENTS_STRONG) {
        const Csr in = {d_in_row_ptr, d_in_col, (int64_t)GRX_HUB_FACTOR * in_lanes_per_row};
        const unsigned in_hubs = (unsigned)n_in_hub_rows;
        const Strong s = {n, out, in, ws, d_label};
        st_init_kernel<<<ngrid, CP_BLOCK, 0, st>>>(s);
        GRX_LAUNCH_CHECK();
        // every outer iteration removes a component and has at most 3 n + 4 rounds; the round number is an int32
        const int64_t max_rounds = n < 26000 ? (n + 2) * (3 * n + 4) : INT32_MAX - 4 * CP_ROUND_BATCH;
        const int rc = grx_run_rounds(
            "grx_components: the strongly connected components did not end after %lld rounds", CP_ROUND_BATCH,
            max_rounds, ST_WORDS, ws.ctrl, h, st, [&] {
                if (hubs) st_hub_kernel<<<hubs, CP_BLOCK, 0, st>>>(s, d_hub_rows, 0);
                if (in_hubs) st_hub_kernel<<<in_hubs, CP_BLOCK, 0, st>>>(s, d_in_hub_rows, 1);
                st_rows_kernel<<<rgrid, CP_BLOCK, 0, st>>>(s);
                st_advance_kernel<<<1, 1, 0, st>>>(ws);
                return (int)GRX_OK;
            });
        if (rc != GRX_OK) return rc;
        rounds = h[ST_ROUND];
    } else {
        cp_iota_kernel<<<ngrid, CP_BLOCK, 0, st>>>(n, d_label);
        if (mode == GRX_COMPONENTS_CONNECTED) {
            cp_cc_kernel<true><<<ngrid, CP_BLOCK, 0, st>>>(n, out, d_label);
            if (hubs) cp_cc_hub_kernel<true><<<hubs, CP_BLOCK, 0, st>>>(n, out, d_hub_rows, d_label);
        } else {
            cp_cc_kernel<false><<<ngrid, CP_BLOCK, 0, st>>>(n, out, d_label);
            if (hubs) cp_cc_hub_kernel<false><<<hubs, CP_BLOCK, 0, st>>>(n, out, d_hub_rows, d_label);
        }
        cp_flatten_kernel<<<ngrid, CP_BLOCK, 0, st>>>(n, d_label);
        GRX_LAUNCH_CHECK();
    }
    if (!d_size && !n_components) {
        if (h_rounds) *h_rounds = rounds;
        return GRX_OK;
    }
    int32_t *count = ws.col[0];
    if (d_size) {
        grx_fill32(count, n, 0, st);
        cp_count_kernel<<<ngrid, CP_BLOCK, 0, st>>>(n, d_label, count);
    }
    grx_fill32(ws.ctrl + ST_NCOMP, 1, 0, st);
    cp_finish_kernel<<<ngrid, CP_BLOCK, 0, st>>>(n, d_label, count, d_size, ws.ctrl + ST_NCOMP);
    GRX_LAUNCH_CHECK();
    if (n_components) {
        const int rc = grx_read_ctrl(ws.ctrl, ST_WORDS, h, st);
        if (rc != GRX_OK) return rc;
        *n_components = h[ST_NCOMP];
    }
    if (h_rounds) *h_rounds = rounds;
    return GRX_OK;
}

size_t grx_reachable_workspace_bytes(int64_t n) { return grx_carve_bytes(lay_out_reachable, n); }

int grx_reachable(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                  int64_t n_hub_rows, int lanes_per_row, int32_t *d_flag, int64_t *h_count, int64_t *h_levels,
                  void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_reachable: n = %lld out of range", (long long)n);
    if (h_count) *h_count = 0;
    if (h_levels) *h_levels = 0;
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_flag && d_workspace, "grx_reachable: null pointer");
    GRX_REQUIRE(lanes_per_row >= 1, "grx_reachable: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "grx_reachable: hub list");
    GrxCarve c(d_workspace);
    const RcWs ws = lay_out_reachable(c, n);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_reachable: workspace %zu bytes, need %zu", workspace_bytes, c.used);
    hipStream_t st = grx_stream(stream);
    int32_t *level = ws.level, *ctrl = ws.ctrl;
    const Csr g = {d_row_ptr, d_col, (int64_t)GRX_HUB_FACTOR * lanes_per_row};
    const unsigned ngrid = grx_grid(n, CP_BLOCK, CP_MAX_BLOCKS);
    const unsigned rgrid = grx_grid(n, CP_BLOCK / CP_GROUP, CP_MAX_ROW_BLOCKS);
    const unsigned hubs = (unsigned)n_hub_rows;
    rc_init_kernel<<<ngrid, CP_BLOCK, 0, st>>>(n, d_flag, level, ctrl);
    GRX_LAUNCH_CHECK();
    int32_t h[RT_WORDS];
    // a closure has at most n - 1 levels; one more launch finds the empty frontier
    int rc = grx_run_rounds(
        "grx_reachable: the closure did not end after %lld levels", CP_ROUND_BATCH, n + 1, RT_WORDS, ctrl, h, st, [&] {
            if (hubs) rc_hub_kernel<<<hubs, CP_BLOCK, 0, st>>>(n, g, d_hub_rows, d_flag, level, ctrl);
            rc_rows_kernel<<<rgrid, CP_BLOCK, 0, st>>>(n, g, d_flag, level, ctrl);
            return grx_frontier_advance(ctrl, st);
        });
    if (rc != GRX_OK) return rc;
    if (h_levels) *h_levels = h[GRX_CT_LEVEL];
    if (h_count) {
        rc_count_kernel<<<ngrid, CP_BLOCK, 0, st>>>(n, d_flag, ctrl);
        GRX_LAUNCH_CHECK();
        rc = grx_read_ctrl(ctrl, RT_WORDS, h, st);
        if (rc != GRX_OK) return rc;
        *h_count = h[RT_COUNT];
    }
    return GRX_OK;
}

}  // extern "C"
