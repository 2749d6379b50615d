// grx_truss.hip -- the truss number of every edge and node for RolX sense making: the largest k such that the edge
// (node) belongs to networkx 3.4.2's k_truss(G, k) (core.py:k_truss; Cohen, "Trusses: cohesive subgraphs for social
// network analysis", 2008) -- the maximal subgraph in which every edge lies in at least k - 2 triangles of that
// subgraph.  networkx peels one k per call, edge by edge in Python; here every k comes from one level-synchronous
// peeling of the EDGES, the scheme of PKT (Kabir and Madduri, "Shared-memory graph truss decomposition", HiPC 2017),
// which is the peeling of grx_peel.h -- the one grx_kcore.hip runs over nodes -- with edges for items and a row
// intersection for a row walk:
//
//   sup(e) = |N(u) & N(v)| for every edge e = (u, v)                          the triangles through e
//   k = 2, round = 1, every edge alive
//   while an edge is alive:
//       F = {alive e : sup(e) <= k - 2}          if empty: k = 2 + min sup over the alive edges, then F
//       t(e) = k for e in F
//       for e = (u, v) in F, for every w in N(u) & N(v) with a = (u, w) and b = (v, w) not gone in an EARLIER round:
//           neither in F:   sup(a) -= 1, sup(b) -= 1
//           only a in F:    sup(b) -= 1  iff  id(e) < id(a)                   the triangle dies once
//           only b in F:    sup(a) -= 1  iff  id(e) < id(b)
//           both in F:      nothing
//       F leaves; round += 1
//   t(v) = max t(e) over the edges at v, 0 for a node without an edge (networkx drops isolated nodes from every truss)
//
// The CSR is symmetric with ascending columns and no self-loop.  An edge is the position of its arc with row < column
// (its id); sup and the state word live there, and rev[j], the position of arc j's reverse (one binary search per arc,
// in the support pass), lets both ends address them.  State word of an edge: 0 = alive, r > 0 = the round it is in F
// (it leaves at the end of that round); -1 at the positions with row > column, which are nobody's id.  State words are
// static within a round but for one transition: the thread that takes an alive edge into the NEXT round's F stores
// round + 1, which every reader of this round takes for alive, as it does 0.  So `state == round` (in F), `0 < state <
// round` (gone) and anything else (alive) are decided without races, and of the two or three frontier edges of one
// triangle exactly the one with the smallest id sends the decrement.
//
// Support pass: rj_arc_kernel of grx_rowjoin.h with a counting body, the intersection for the arcs with row < column
// only (the other arc of the edge would count the same triangles).  The frontier is grx_peel.h's list: of all the
// decrements an edge receives exactly one takes it from above k - 2 to k - 2; that thread writes t(e) at both arcs and
// the state word, and appends e to the next list.  The sweeps of a round whose list came out empty (k must jump) run
// over the arcs, and the levels word counts them.  A lane group per frontier edge walks the shorter row and
// binary-searches the longer one, as rj_arc_kernel does; it is the list-driven variant of that loop, written here
// because its unit of work is a list entry and its hits need no reduction; a frontier edge whose support has reached 0
// (every edge of truss number 2, for one) has no triangle left and is not intersected.  Node column: rj_rows_kernel /
// rj_hub_rows_kernel with a max body.  Measured: profiles/truss.txt (tr_min / tr_collect / tr_finalize there are
// today's pl_* kernels; the peel waits for the longest hub-hub intersection of every round).
// Bound: one row intersection per edge for the supports and one more per edge over the whole peel (each min(d_u, d_v) *
// ceil(log2 max(d_u, d_v)) dependent 4-byte gathers), two 4-byte state gathers per common neighbour, at most three
// atomic decrements per triangle (two when its first edge leaves alone, one when two leave together), one append per
// edge, and two sweeps of 4 to 8 bytes per arc per distinct k.  Hub-hub edges have no path of their own: like
// rj_arc_kernel, one lane group intersects them.
// Integer atomics only, and nothing depends on their order: the same bits in every run, for every lanes_per_row and
// every relabelling (the order of the lists is never visible; which edge of a triangle sends the decrement is, but
// not in the result).  The pragma is the include rule of grx_rowjoin.h; nothing here is floating point but the
// exact small integers its reductions carry.
#pragma clang fp contract(off)

#include "grx_peel.h"
#include "grx_rowjoin.h"

namespace {

constexpr int TR_ROUND_BATCH = 16;                           // rounds enqueued between two read-backs
constexpr int TR_PEEL_MAX_WG = 2048;
static_assert(RJ_BLOCK == PL_BLOCK, "tr_peel_kernel flushes with pl_flush");

// the workspace: arc_row | rev | sup | state | list0 | list1 (int32[nnz] each) | control words.  A list holds nnz / 2
// edges at most; it has room for every position with row < column of a CSR that breaks the symmetry it promised
struct TrWs {
    char *base;
    size_t arc;
    TrWs(void *b, int64_t nnz)
        : base(reinterpret_cast<char *>(b)), arc(grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 4, 256)) {}
    int32_t *at(int i) const { return reinterpret_cast<int32_t *>(base + i * arc); }
    size_t bytes() const { return 6 * arc + 256; }
};

// and the items of grx_peel.h: an edge (the position of its arc with row < column), alive while its state word is 0,
// valued by sup against thr = k - 2
struct TrState {
    int32_t *arc_row, *rev, *sup, *state;
    PlLists pl;
    int32_t *truss;                                          // the caller's [nnz]
    __device__ __forceinline__ bool alive(int64_t j) const { return state[j] == 0; }
    __device__ __forceinline__ int value(int64_t j) const { return sup[j]; }
    __device__ __forceinline__ void leave(int64_t a, int round, int thr) const
    {
        state[a] = round;
        truss[a] = thr + 2;
        truss[rev[a]] = thr + 2;
    }
};

TrState carve(const TrWs &w, int32_t *truss)
{
    return TrState{w.at(0), w.at(1), w.at(2), w.at(3), PlLists{w.at(4), w.at(5), w.at(6)}, truss};
}

// ---- support pass: the bodies of grx_rowjoin.h ------------------------------------------------------------------
struct tr_rows {                                             // (a) the row of every arc
    int32_t *__restrict__ arc_row;
    struct Acc {};
    __device__ __forceinline__ void entry(int64_t u, int64_t j, Acc &) const { arc_row[j] = (int32_t)u; }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &, R) const {}
    __device__ __forceinline__ void finish(int64_t, int64_t, int64_t, const Acc &) const {}
};

struct tr_support {                                          // (b) sup, rev and the state word of every arc
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col, *__restrict__ arc_row;
    int32_t *__restrict__ rev, *__restrict__ sup, *__restrict__ state;
    struct Acc { double c; };                                // a count far below 2^53: exact
    __device__ __forceinline__ bool begin(int64_t, int32_t u, int32_t v, Acc &) const { return u < v; }
    __device__ __forceinline__ void hit(int32_t, int32_t, int32_t, int64_t, int64_t, bool, Acc &a) const { a.c += 1.0; }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.c = r.sum(a.c); }
    __device__ __forceinline__ void finish(int64_t j, const Acc &a) const
    {
        const int32_t u = arc_row[j], v = col[j];
        int64_t lo = row_ptr[v], hi = row_ptr[v + 1];
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (col[mid] < u) lo = mid + 1; else hi = mid;
        }
        // a symmetric CSR holds (v, u); one that does not gets its own position, so nothing is ever indexed outside
        rev[j] = (int32_t)(lo < end && col[lo] == u ? lo : j);
        sup[j] = (int32_t)a.c;
        state[j] = u < v ? 0 : -1;
    }
};

struct tr_node {                                             // the node column: max t over the row's arcs
    const int32_t *__restrict__ truss;
    int64_t *__restrict__ node;
    struct Acc { double m; };                                // 0 for an empty row
    __device__ __forceinline__ void entry(int64_t, int64_t j, Acc &a) const { a.m = fmax(a.m, (double)truss[j]); }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.m = r.max(a.m); }
    __device__ __forceinline__ void finish(int64_t u, int64_t, int64_t, const Acc &a) const { node[u] = (int64_t)a.m; }
};

// ---- peeling ----------------------------------------------------------------------------------------------------
// sup(a) -= 1; the one decrement that takes a from above k - 2 to k - 2 puts a into the next round's F
__device__ __forceinline__ void drop(int32_t a, const PlRound &r, const TrState &s, PlAppends &ap)
{
    const int old = atomicSub(&s.sup[a], 1);
    if (pl_crosses(old, 1, r.thr)) {
        s.leave(a, r.round + 1, r.thr);
        pl_append(a, r, ap);
    }
}

// the peel: a group of L lanes per edge of F walks the shorter of the two rows and searches the longer one
template <int L>
__global__ __launch_bounds__(RJ_BLOCK) void tr_peel_kernel(const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col, TrState s)
{
    __shared__ PlAppends ap;
    if (s.pl.ctrl[PL_DONE]) return;
    const PlRound r = round_of(s.pl);
    if (threadIdx.x == 0) ap.count = 0;
    __syncthreads();
    constexpr int EPG = RJ_BLOCK / L;                       // edges per workgroup pass
    const int lane = threadIdx.x % L;
    for (int64_t i = (int64_t)blockIdx.x * EPG + threadIdx.x / L; i < r.count; i += (int64_t)gridDim.x * EPG) {
        const int32_t e = r.cur[i];
        // sup(e) stands still while e is in F and counts the triangles of e that are still whole: none, no search
        if (s.sup[e] <= 0) continue;
        const int32_t u = s.arc_row[e], v = col[e];
        const int64_t bu = row_ptr[u], eu = row_ptr[u + 1], bv = row_ptr[v], ev = row_ptr[v + 1];
        const bool walk_u = eu - bu <= ev - bv;
        const int32_t p = walk_u ? u : v, q = walk_u ? v : u;   // p's row is walked, q's searched
        const int64_t wb = walk_u ? bu : bv, we = walk_u ? eu : ev;
        const int64_t sb = walk_u ? bv : bu, se = walk_u ? ev : eu;
        for (int64_t k = wb + lane; k < we; k += L) {
            const int32_t w = col[k];
            int64_t lo = sb, hi = se;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (col[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo >= se || col[lo] != w) continue;
            // the ids of (p, w) and (q, w): the arc itself, or its reverse
            const int32_t a = p < w ? (int32_t)k : s.rev[k], b = q < w ? (int32_t)lo : s.rev[lo];
            const int ta = s.state[a], tb = s.state[b];
            if ((ta > 0 && ta < r.round) || (tb > 0 && tb < r.round)) continue;   // the triangle died earlier
            const bool fa = ta == r.round, fb = tb == r.round;
            if (!fa && !fb) {
                drop(a, r, s, ap);
                drop(b, r, s, ap);
            } else if (fa && !fb) {
                if (e < a) drop(b, r, s, ap);
            } else if (fb && !fa) {
                if (e < b) drop(a, r, s, ap);
            }
        }
    }
    pl_flush(r, ap);
}

__global__ void tr_init_kernel(int64_t m, TrState s) { pl_init_ctrl(s.pl.ctrl, (int32_t)m); }

}  // namespace

extern "C" {

size_t grx_truss_numbers_workspace_bytes(int64_t n, int64_t nnz)
{
    (void)n;
    return TrWs(nullptr, nnz).bytes();
}

int grx_truss_numbers(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                      int64_t n_hub_rows, int lanes_per_row, int32_t *d_arc_truss, int64_t *d_node_truss,
                      int64_t *n_rounds, int64_t *n_levels, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "grx_truss_numbers";
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "%s: n = %lld out of range [0, 2^31)", who, (long long)n);
    if (n_rounds) *n_rounds = 0;
    if (n_levels) *n_levels = 0;
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_arc_truss && d_workspace, "%s: null pointer", who);
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "%s: lanes_per_row must be 4, 8, 16 or 32 (got %d)", who, lanes_per_row);
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "%s: hub list", who);
    const size_t least = TrWs(nullptr, 0).bytes();
    GRX_REQUIRE(workspace_bytes >= least, "%s: workspace %zu bytes, need at least %zu", who, workspace_bytes, least);
    RjCall c{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row};
    c.st = grx_stream(stream);
    c.hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    c.nnz = 0;
    GRX_CHECK_HIP(hipMemcpyAsync(&c.nnz, d_row_ptr + n, sizeof(c.nnz), hipMemcpyDeviceToHost, c.st));
    GRX_CHECK_HIP(hipStreamSynchronize(c.st));
    GRX_REQUIRE(c.nnz >= 0 && c.nnz < (int64_t)1 << 31 && c.nnz % 2 == 0,
                "%s: row_ptr[n] = %lld: the arcs of a symmetric CSR without self-loops are even in number and fewer "
                "than 2^31", who, (long long)c.nnz);
    const TrWs ws(d_workspace, c.nnz);
    GRX_REQUIRE(workspace_bytes >= ws.bytes(), "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.bytes());
    if (c.nnz == 0) {
        if (d_node_truss) grx_fill64(reinterpret_cast<uint64_t *>(d_node_truss), n, 0, c.st);
        GRX_LAUNCH_CHECK();
        return GRX_OK;
    }
    const TrState s = carve(ws, d_arc_truss);
    const int64_t m = c.nnz / 2;

    tr_init_kernel<<<1, 1, 0, c.st>>>(m, s);
    int rc = rj_run(c, s.arc_row, tr_rows{s.arc_row},
                    tr_support{d_row_ptr, d_col, s.arc_row, s.rev, s.sup, s.state},
                    tr_rows{nullptr}, false);
    if (rc != GRX_OK) return rc;

    int32_t h[PL_WORDS];
    rj_with_lanes(lanes_per_row, [&](auto width) {
        constexpr int L = decltype(width)::value;
        const unsigned peel_grid = grx_grid(m, RJ_BLOCK / L, TR_PEEL_MAX_WG);
        // every round removes at least one edge: at most m rounds
        rc = grx_run_rounds("grx_truss_numbers: the peeling did not end after %lld rounds", TR_ROUND_BATCH, m + 1,
                            PL_WORDS, s.pl.ctrl, h, c.st, [&] {
                                pl_sweeps(c.nnz, s, c.st);
                                tr_peel_kernel<L><<<peel_grid, RJ_BLOCK, 0, c.st>>>(d_row_ptr, d_col, s);
                                pl_finalize_kernel<<<1, 1, 0, c.st>>>(s.pl.ctrl);
                                return (int)GRX_OK;
                            });
    });
    if (rc != GRX_OK) return rc;
    if (n_rounds) *n_rounds = h[PL_ROUND];
    if (n_levels) *n_levels = h[PL_LEVELS];

    if (d_node_truss) {
        const tr_node node{d_arc_truss, d_node_truss};
        if (n_hub_rows) rj_hub_rows_kernel<<<(unsigned)n_hub_rows, RJ_BLOCK, 0, c.st>>>(d_row_ptr, d_hub_rows, node);
        rj_with_lanes(lanes_per_row, [&](auto width) {
            constexpr int L = decltype(width)::value;
            rj_rows_kernel<L><<<grx_grid(n, RJ_BLOCK / L, RJ_ROW_MAX_WG), RJ_BLOCK, 0, c.st>>>(n, d_row_ptr,
                                                                                                c.hub_degree, node);
        });
        GRX_LAUNCH_CHECK();
    }
    return GRX_OK;
}

}  // extern "C"
