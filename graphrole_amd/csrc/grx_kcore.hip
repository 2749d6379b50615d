// grx_kcore.hip -- core number and onion layer of every node for RolX sense making: networkx 3.4.2's core_number
// (core.py: Batagelj-Zaversnik bucket peeling, sequential) and onion_layers (Hebert-Dufresne et al., "Multi-scale
// structure and topological anomaly detection via a new network statistic: the onion decomposition", 2016), both from
// one synchronous peeling:
//
//   k = 0, layer = 1, every node alive, deg(v) = degree of v (directed: in + out)
//   while a node is alive:
//       k = max(k, min deg over the alive nodes)
//       F = {alive v : deg(v) <= k}                  decided on the degrees at the start of the round
//       core(v) = k, onion(v) = layer for v in F; F leaves
//       for v in F, for every arc between v and a node u: deg(u) -= 1
//       layer += 1
//
// The peeling itself -- the frontier list, the crossing decrement, the LDS append buffer, the two sweeps of a round
// whose list came out empty (k must jump) and the one-thread finalize -- is grx_peel.h with nodes for items, deg for
// the value, k for the threshold and the onion layer for the round.  The thread that sees old > k >= old - c writes the
// node's core, onion layer and state there and then.
// Bound: 2 (distinct core values) sweeps of 8 n bytes, plus one visit of every arc from each of its ends over the
// whole run (a 4-byte gather of the other end's state; an atomicSub only when that end is still alive: about one per
// edge), plus the hub pulls below.  Never rounds x n.
//
// Hubs (the CSR's hub list: rows longer than GRX_HUB_FACTOR * lanes_per_row) get a workgroup per row and round, on
// both sides of the peel:
//   * a hub in F walks its long row with all 256 threads;
//   * a hub that stays alive PULLS its decrement: its workgroup counts the entries of its row that are in F (state ==
//     layer) and subtracts the count once.  The threads that peel a neighbour of it read the hub flag in its state word
//     and send nothing.  Chosen over collecting pushes in LDS because it needs no per-workgroup table and no key
//     lookup per arc (the pusher reads the target's state word anyway, to skip the ends that have left), and because it
//     puts one atomic on a hub's counter per round whatever the graph: the 1 500 leaves of a star that leave in one
//     round send 0 decrements to the centre instead of 1 500.  Its price is that every alive hub row is read in every
//     round: rounds x (arcs of the alive hub rows) coalesced column reads and 4-byte state gathers.
//   For a directed graph a node's out-row and in-row are pulled separately (by the out CSR's and the in CSR's hub
//   list); the two counts add up, and a reciprocal pair counts twice as in networkx's all_neighbors.
//
// State word of a node: > 0 = the round it left in (its onion layer); <= 0 = alive, minus the hub bits (1 = listed in
// the out CSR's hub list, 2 = in the in CSR's; both for an undirected graph).  A decrement that reaches a node after
// its crossing decrement (or after it left) changes nothing that is read again.
// Integer arithmetic only; core and onion are the same in every run (the order of the lists is not, and is never
// visible).  The CSRs must hold no self-loop (the caller's precondition).
#include "grx_peel.h"

namespace {

constexpr int KC_BLOCK = PL_BLOCK;                           // the appending kernels flush with pl_flush
constexpr int KC_GROUP = 8;                                  // lanes per frontier node in kc_peel_kernel
constexpr int KC_ROUND_BATCH = 16;                           // rounds enqueued between two read-backs
constexpr int KC_MAX_BLOCKS = 2048;                          // workgroups of kc_init and kc_peel
constexpr int KC_OUT_HUB = 1, KC_IN_HUB = 2;

// the workspace, the outputs, and the items of grx_peel.h: a node, alive while its state word is <= 0, valued by deg
struct KcState {
    int32_t *deg, *state;
    PlLists pl;
    int64_t *core, *onion;                                   // onion may be null
    __device__ __forceinline__ bool alive(int64_t v) const { return state[v] <= 0; }
    __device__ __forceinline__ int value(int64_t v) const { return deg[v]; }
    __device__ __forceinline__ void leave(int64_t v, int layer, int k) const
    {
        state[v] = layer;
        core[v] = k;
        if (onion) onion[v] = layer;
    }
};

KcState lay_out(GrxCarve &c, int64_t n, int64_t *core, int64_t *onion)
{
    const size_t nn = (size_t)(n > 0 ? n : 1);
    KcState s;
    s.deg = c.take<int32_t>(nn);
    s.state = c.take<int32_t>(nn);
    s.pl.list0 = c.take<int32_t>(nn);
    s.pl.list1 = c.take<int32_t>(nn);
    s.pl.ctrl = c.take<int32_t>(GRX_CTRL_MAX_WORDS);
    s.core = core;
    s.onion = onion;
    return s;
}

// deg(u) -= c; the one decrement that takes u from above k to k or below puts u into the next round's F
__device__ __forceinline__ void drop(int32_t u, int c, const PlRound &r, const KcState &s, PlAppends &ap)
{
    const int old = atomicSub(&s.deg[u], c);
    if (pl_crosses(old, c, r.thr)) {
        s.leave(u, r.round + 1, r.thr);
        pl_append(u, r, ap);
    }
}

// a node of F tells the other end u of one arc -- unless u left in this or an earlier round, or is an alive hub of
// the CSR that holds the arc on u's side (`skip`: u's workgroup pulls it)
__device__ __forceinline__ void push_arc(int32_t u, int skip, const PlRound &r, const KcState &s, PlAppends &ap)
{
    const int32_t su = s.state[u];
    if (su > 0 ? su <= r.round : ((-su) & skip) != 0) return;
    drop(u, 1, r, s, ap);
}

__global__ __launch_bounds__(KC_BLOCK) void kc_init_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                           const int64_t *__restrict__ in_row_ptr, KcState s)
{
    for (int64_t v = (int64_t)blockIdx.x * KC_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * KC_BLOCK) {
        int64_t d = row_ptr[v + 1] - row_ptr[v];
        if (in_row_ptr) d += in_row_ptr[v + 1] - in_row_ptr[v];
        s.deg[v] = (int32_t)d;
        s.state[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) pl_init_ctrl(s.pl.ctrl, (int32_t)n);
}

// the hub bits of the state words (every listed row once per list: no two threads of a launch share a word)
__global__ __launch_bounds__(KC_BLOCK) void kc_hub_flag_kernel(int64_t n, const int32_t *__restrict__ hub_rows,
                                                               int64_t n_hub_rows, int bits, int32_t *__restrict__ state)
{
    const int64_t i = (int64_t)blockIdx.x * KC_BLOCK + threadIdx.x;
    if (i >= n_hub_rows) return;
    const int64_t h = hub_rows[i];
    if (h < 0 || h >= n) return;                             // an id outside [0, n) is never written through
    state[h] = -((-state[h]) | bits);
}

// the peel of the rows up to hub_degree arcs: KC_GROUP lanes per node of F, over the list
__global__ __launch_bounds__(KC_BLOCK) void kc_peel_kernel(const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col, int64_t hub_degree,
                                                           const int64_t *__restrict__ in_row_ptr,
                                                           const int32_t *__restrict__ in_col, int64_t in_hub_degree,
                                                           KcState s)
{
    __shared__ PlAppends ap;
    if (s.pl.ctrl[PL_DONE]) return;
    const PlRound r = round_of(s.pl);
    if (threadIdx.x == 0) ap.count = 0;
    __syncthreads();
    constexpr int NODES = KC_BLOCK / KC_GROUP;
    const int g = threadIdx.x % KC_GROUP;
    for (int64_t i = (int64_t)blockIdx.x * NODES + threadIdx.x / KC_GROUP; i < r.count;
         i += (int64_t)gridDim.x * NODES) {
        const int64_t v = r.cur[i];
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b <= hub_degree)                              // longer rows: kc_hub_kernel
            for (int64_t j = b + g; j < e; j += KC_GROUP) push_arc(col[j], KC_IN_HUB, r, s, ap);
        if (in_row_ptr) {
            const int64_t ib = in_row_ptr[v], ie = in_row_ptr[v + 1];
            if (ie - ib <= in_hub_degree)
                for (int64_t j = ib + g; j < ie; j += KC_GROUP) push_arc(in_col[j], KC_OUT_HUB, r, s, ap);
        }
    }
    pl_flush(r, ap);
}

// one workgroup per hub row of one CSR: a hub in F pushes along its row; a hub that stays alive pulls -- counts the
// entries of its row that are in F -- and subtracts once.  `skip`: the hub bit of the CSR that holds this CSR's arcs
// on the other end's side (the in CSR for the out CSR's rows and the other way round)
__global__ __launch_bounds__(KC_BLOCK) void kc_hub_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ hub_rows, int skip, KcState s)
{
    __shared__ PlAppends ap;
    __shared__ int total, own;
    if (s.pl.ctrl[PL_DONE]) return;
    const PlRound r = round_of(s.pl);
    const int t = threadIdx.x;
    const int32_t v = hub_rows[blockIdx.x];
    if (v < 0 || v >= n) return;                             // an id outside [0, n) is never read through
    if (t == 0) { ap.count = 0; total = 0; own = s.state[v]; }   // one read: every wavefront takes the same branch
    __syncthreads();
    const int sv = own;
    const int64_t b = row_ptr[v], e = row_ptr[v + 1];
    if (sv == r.round) {
        for (int64_t j = b + t; j < e; j += KC_BLOCK) push_arc(col[j], skip, r, s, ap);
    } else if (sv <= 0) {
        int c = 0;
        for (int64_t j = b + t; j < e; j += KC_BLOCK) c += s.state[col[j]] == r.round;
#pragma unroll
        for (int off = GRX_WAVE / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, GRX_WAVE);
        if (t % GRX_WAVE == 0 && c) atomicAdd(&total, c);
        __syncthreads();
        if (t == 0 && total) drop(v, total, r, s, ap);
    }
    pl_flush(r, ap);
}

}  // namespace

extern "C" {

size_t grx_core_numbers_workspace_bytes(int64_t n) { return grx_carve_bytes(lay_out, n, nullptr, nullptr); }

int grx_core_numbers(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                     int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                     const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row, int64_t *d_core,
                     int64_t *d_onion, int64_t *n_rounds, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n > 0 && n < (int64_t)1 << 31, "grx_core_numbers: n = %lld out of range", (long long)n);
    GRX_REQUIRE(d_row_ptr && d_col && d_core && d_workspace, "grx_core_numbers: null pointer");
    GRX_REQUIRE(lanes_per_row >= 1, "grx_core_numbers: lanes_per_row must be >= 1");
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "grx_core_numbers: hub list");
    const bool directed = d_in_row_ptr != nullptr;
    if (directed) {
        GRX_REQUIRE(d_in_col, "grx_core_numbers: null pointer (in CSR)");
        GRX_REQUIRE(in_lanes_per_row >= 1, "grx_core_numbers: in_lanes_per_row must be >= 1");
        GRX_REQUIRE(n_in_hub_rows >= 0 && n_in_hub_rows <= n && (n_in_hub_rows == 0 || d_in_hub_rows),
                    "grx_core_numbers: hub list (in CSR)");
    } else {
        GRX_REQUIRE(!d_in_col && !d_in_hub_rows && n_in_hub_rows == 0 && in_lanes_per_row == 0,
                    "grx_core_numbers: the in CSR must be given whole or not at all");
    }
    GrxCarve c(d_workspace);
    const KcState s = lay_out(c, n, d_core, d_onion);
    GRX_REQUIRE(workspace_bytes >= c.used, "grx_core_numbers: workspace %zu bytes, need %zu", workspace_bytes, c.used);
    hipStream_t st = grx_stream(stream);
    const int64_t hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    const int64_t in_hub_degree = (int64_t)GRX_HUB_FACTOR * in_lanes_per_row;
    const unsigned init_grid = grx_grid(n, KC_BLOCK, KC_MAX_BLOCKS);
    const unsigned peel_grid = grx_grid(n, KC_BLOCK / KC_GROUP, KC_MAX_BLOCKS);

    kc_init_kernel<<<init_grid, KC_BLOCK, 0, st>>>(n, d_row_ptr, d_in_row_ptr, s);
    if (n_hub_rows)
        kc_hub_flag_kernel<<<(unsigned)grx_ceil_div(n_hub_rows, KC_BLOCK), KC_BLOCK, 0, st>>>(
            n, d_hub_rows, n_hub_rows, directed ? KC_OUT_HUB : KC_OUT_HUB | KC_IN_HUB, s.state);
    if (n_in_hub_rows)
        kc_hub_flag_kernel<<<(unsigned)grx_ceil_div(n_in_hub_rows, KC_BLOCK), KC_BLOCK, 0, st>>>(
            n, d_in_hub_rows, n_in_hub_rows, KC_IN_HUB, s.state);
    GRX_LAUNCH_CHECK();
    int32_t h[2];
    // every round but the last removes a node: at most n rounds
    const int rc = grx_run_rounds(
        "grx_core_numbers: the peeling did not end after %lld rounds", KC_ROUND_BATCH, n + 1, 2, s.pl.ctrl, h, st, [&] {
            pl_sweeps(n, s, st);
            if (n_hub_rows)
                kc_hub_kernel<<<(unsigned)n_hub_rows, KC_BLOCK, 0, st>>>(n, d_row_ptr, d_col, d_hub_rows, KC_IN_HUB,
                                                                         s);
            if (n_in_hub_rows)
                kc_hub_kernel<<<(unsigned)n_in_hub_rows, KC_BLOCK, 0, st>>>(n, d_in_row_ptr, d_in_col, d_in_hub_rows,
                                                                            KC_OUT_HUB, s);
            kc_peel_kernel<<<peel_grid, KC_BLOCK, 0, st>>>(d_row_ptr, d_col, hub_degree, d_in_row_ptr, d_in_col,
                                                           in_hub_degree, s);
            pl_finalize_kernel<<<1, 1, 0, st>>>(s.pl.ctrl);
            return (int)GRX_OK;
        });
    if (rc != GRX_OK) return rc;
    if (n_rounds) *n_rounds = h[PL_ROUND];
    return GRX_OK;
}

}  // extern "C"
