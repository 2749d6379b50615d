// grx_graphlets.hip -- the graphlet degree vector of every node for RolX sense making (Przulj, "Biological network
// comparison using graphlet degree distribution", 2007): for each of the 15 automorphism orbits of the connected graphs
// on 2, 3 and 4 nodes, the number of INDUCED subgraphs that touch the node at that orbit.
//
//   orbit  0        edge                      8         4-cycle
//          1, 2     path on 3: end, middle    9, 10, 11 paw: pendant; triangle node off the tail; triangle node on it
//          3        triangle                  12, 13    diamond: degree-2 node; degree-3 node (on the chord)
//          4, 5     path on 4: end, interior  14        4-clique
//          6, 7     claw: leaf, centre
//
// No induced subgraph is enumerated.  Per node the NON-INDUCED occurrences N0 .. N14 (the copies of the graphlet as a
// subgraph, induced or not, with the node at that orbit) come from a few primitives, and the orbits follow by
// back-substitution through the fixed unit upper-triangular integer matrix GL_A below (N = A o; row k = the coefficients
// of o0 .. o14; every coefficient is the formula of row k applied to the graphlet of the column's orbit).
//   d(v) the degree, t(e) the triangles through edge e, t(v) = 1/2 sum_{u in N(v)} t(vu), S1(v) = sum_{u in N(v)}
//   (d(u) - 1), Q(v) the 4-cycles through v (d_squares of grx_square_clustering), K4(v) the 4-cliques at v
//   N0 = d                N1 = S1                   N2 = C(d, 2)                    N3 = t(v)
//   N4 = sum_u (S1(u) - (d(v) - 1)) - 2 t(v)        N5 = sum_u ((d(v) - 1)(d(u) - 1) - t(vu))
//   N6 = sum_u C(d(u) - 1, 2)                       N7 = C(d, 3)                    N8 = Q(v)
//   N9 = sum_u (t(u) - t(uv))                       N10 = sum_u t(vu)(d(u) - 2)     N11 = t(v)(d(v) - 2)
//   N12 = sum over the triangles {v, u, w} of (t(uw) - 1)          N13 = sum_u C(t(vu), 2)        N14 = K4(v)
//
// Stages over the symmetric CSR with ascending columns and no diagonal entry (grx_truss_numbers' contract):
//   (1) per row (gl_stats, a row body of grx_rowjoin.h): the row of every arc, and S1;
//   (2) per arc with row < column (gl_support, rj_arc_kernel): t(e) by one row intersection, and the position of every
//       arc's reverse by one binary search; gl_mirror copies t(e) to the arc with row > column;
//   (3) per row (gl_pass_a): t(v), N5, N6, N10, N13;
//   (4) per row (gl_pass_b), with t(u) and S1(u) of the neighbours complete: N4, N9;
//   (5) per arc with t(e) > 0 (gl_diamond_kernel: rj_arc_kernel's loop behind that test, which needs the arc's own
//       position; the body is gl_diamond): the sum over the common neighbours w of t(third edge) - 1,
//       added to the row's counter by one 64-bit integer atomic per arc: over the arcs of row v that is 2 N12(v);
//   (6) the 4-cliques (gl_k4_kernel), on the degree-oriented CSR (arc u -> v iff (d(u), u) < (d(v), v); out-rows
//       ascending): a group of L lanes per arc (u, v) of the symmetric CSR with t(uv) >= 2 that is an oriented arc (one
//       binary search in N+(u)).  The group walks the shorter of N+(u) and N+(v) and searches the longer one; its hits
//       w (the oriented triangles u -> v -> w) are taken in turn, and for each the whole group walks the shortest of
//       N+(u), N+(v) and N+(w), lane k the entries k, k + L, ..., and searches the other two: every hit x closes the
//       4-clique u < v < w < x of the orientation, which is therefore listed exactly once.
//       Bound per oriented triangle (u, v, w): min(d+(u), d+(v), d+(w)) * 2 ceil(log2 max d+) dependent 4-byte gathers,
//       and one 64-bit integer atomicAdd per 4-clique found (K4(x) += 1) plus at most one per triangle (K4(w) += its
//       count) and two per arc (K4(u), K4(v)).  Out-rows are bounded by the degeneracy order (d+ <= sqrt(2 m)), not by
//       the hub's degree: a wheel or a book costs its rim / its pages a constant each;
//   (7) per node (gl_finish_kernel): N1, N2, N7, N11 and the rest in int64, and the back-substitution.
// Only integer atomics, and nothing depends on their order: the same bits in every run, for every lanes_per_row and
// every relabelling.  The row-join reductions carry doubles that hold integers: the outputs are exact while every N is
// below 2^53; the final arithmetic is int64.  The pragma is the include rule of grx_rowjoin.h.
#pragma clang fp contract(off)

#include "grx_rowjoin.h"

namespace {

constexpr int GL_ORBITS = 15;
constexpr int GL_K4_MAX_WG = 8192;

// N = A o
constexpr int GL_A[GL_ORBITS][GL_ORBITS] = {
    {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {0, 0, 0, 0, 1, 0, 0, 0, 2, 2, 1, 0, 4, 2, 6},
    {0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 1, 2, 2, 4, 6},
    {0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 2, 1, 3},
    {0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1},
    {0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 3},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 3},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 2, 6},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 2, 3},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 3},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
};

// the per-node vectors of the workspace
enum { GV_T = 0, GV_S1, GV_N4, GV_N5, GV_N6, GV_N9, GV_N10, GV_N12X2, GV_N13, GV_K4, GV_VECS };

// the workspace: GV_VECS x int64[n] | arc_row | rev | sup (int32[nnz] each); every array 256-byte aligned
struct GlWs {
    char *base;
    size_t vec, arc;
    GlWs(void *b, int64_t n, int64_t nnz)
        : base(reinterpret_cast<char *>(b)), vec(grx_align_up((size_t)(n > 0 ? n : 1) * 8, 256)),
          arc(grx_align_up((size_t)(nnz > 0 ? nnz : 1) * 4, 256)) {}
    int64_t *node(int i) const { return reinterpret_cast<int64_t *>(base + i * vec); }
    int32_t *per_arc(int i) const { return reinterpret_cast<int32_t *>(base + GV_VECS * vec + i * arc); }
    size_t bytes() const { return GV_VECS * vec + 3 * arc; }
};

// (1)
struct gl_stats {
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col;
    int32_t *__restrict__ arc_row;
    int64_t *__restrict__ s1;
    struct Acc { double s1; };                               // integers below 2^53: exact in every order
    __device__ __forceinline__ void entry(int64_t v, int64_t j, Acc &a) const
    {
        const int32_t u = col[j];
        arc_row[j] = (int32_t)v;
        a.s1 += (double)(row_ptr[u + 1] - row_ptr[u] - 1);
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.s1 = r.sum(a.s1); }
    __device__ __forceinline__ void finish(int64_t v, int64_t, int64_t, const Acc &a) const { s1[v] = (int64_t)a.s1; }
};

// (2)
struct gl_support {
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col, *__restrict__ arc_row;
    int32_t *__restrict__ rev, *__restrict__ sup;
    struct Acc { double c; };
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
        if (u < v) sup[j] = (int32_t)a.c;
    }
};

__global__ __launch_bounds__(RJ_BLOCK) void gl_mirror_kernel(int64_t nnz, const int32_t *__restrict__ arc_row,
                                                             const int32_t *__restrict__ col,
                                                             const int32_t *__restrict__ rev, int32_t *sup)
{
    for (int64_t j = (int64_t)blockIdx.x * RJ_BLOCK + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * RJ_BLOCK)
        if (arc_row[j] >= col[j]) sup[j] = rev[j] != j ? sup[rev[j]] : 0;
}

// (3)
struct gl_pass_a {
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col, *__restrict__ sup;
    int64_t *__restrict__ t, *__restrict__ n5, *__restrict__ n6, *__restrict__ n10, *__restrict__ n13;
    struct Acc { double t2, n5, n6, n10, n13; };
    __device__ __forceinline__ void entry(int64_t v, int64_t j, Acc &a) const
    {
        const int32_t u = col[j];
        const int64_t dv = row_ptr[v + 1] - row_ptr[v], du = row_ptr[u + 1] - row_ptr[u], s = sup[j];
        a.t2 += (double)s;
        a.n5 += (double)((dv - 1) * (du - 1) - s);
        a.n6 += (double)((du - 1) * (du - 2) / 2);
        a.n10 += (double)(s * (du - 2));
        a.n13 += (double)(s * (s - 1) / 2);
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const
    {
        a.t2 = r.sum(a.t2); a.n5 = r.sum(a.n5); a.n6 = r.sum(a.n6); a.n10 = r.sum(a.n10); a.n13 = r.sum(a.n13);
    }
    __device__ __forceinline__ void finish(int64_t v, int64_t, int64_t, const Acc &a) const
    {
        t[v] = (int64_t)a.t2 / 2; n5[v] = (int64_t)a.n5; n6[v] = (int64_t)a.n6; n10[v] = (int64_t)a.n10;
        n13[v] = (int64_t)a.n13;
    }
};

// (4)
struct gl_pass_b {
    const int32_t *__restrict__ col, *__restrict__ sup;
    const int64_t *__restrict__ t, *__restrict__ s1;
    int64_t *__restrict__ n4, *__restrict__ n9;
    struct Acc { double s, n9; };
    __device__ __forceinline__ void entry(int64_t, int64_t j, Acc &a) const
    {
        const int32_t u = col[j];
        a.s += (double)s1[u];
        a.n9 += (double)(t[u] - sup[j]);
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.s = r.sum(a.s); a.n9 = r.sum(a.n9); }
    __device__ __forceinline__ void finish(int64_t v, int64_t b, int64_t e, const Acc &a) const
    {
        const int64_t d = e - b;
        n4[v] = (int64_t)a.s - d * (d - 1) - 2 * t[v];
        n9[v] = (int64_t)a.n9;
    }
};

// (5) arc (u, v), common neighbour w: the third edge is (v, w), in v's row
struct gl_diamond {
    const int32_t *__restrict__ arc_row, *__restrict__ sup;
    unsigned long long *__restrict__ n12x2;
    struct Acc { double s; };
    __device__ __forceinline__ bool begin(int64_t, int32_t, int32_t, Acc &) const { return true; }
    __device__ __forceinline__ void hit(int32_t, int32_t, int32_t, int64_t k, int64_t lo, bool walk_u, Acc &a) const
    {
        a.s += (double)(sup[walk_u ? lo : k] - 1);
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.s = r.sum(a.s); }
    __device__ __forceinline__ void finish(int64_t j, const Acc &a) const
    {
        if (a.s > 0.0) atomicAdd(&n12x2[arc_row[j]], (unsigned long long)a.s);
    }
};

__device__ __forceinline__ bool gl_contains(const int32_t *__restrict__ col, int64_t lo, int64_t hi, int32_t x)
{
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (col[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < end && col[lo] == x;
}

// (5) as a kernel of its own: rj_arc_kernel's loop behind the test t(e) > 0, which needs the arc's position
template <int L>
__global__ __launch_bounds__(RJ_BLOCK) void gl_diamond_kernel(int64_t nnz, const int64_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ col, const gl_diamond body)
{
    constexpr int APG = RJ_BLOCK / L;
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int64_t groups = (nnz + APG - 1) / APG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t j = g * APG + slot;
        gl_diamond::Acc a{};
        if (j < nnz && body.sup[j] > 0) {
            const int32_t u = body.arc_row[j], v = col[j];
            const int64_t bu = row_ptr[u], eu = row_ptr[u + 1], bv = row_ptr[v], ev = row_ptr[v + 1];
            const bool walk_u = eu - bu <= ev - bv;
            const int64_t wb = walk_u ? bu : bv, we = walk_u ? eu : ev;
            const int64_t sb = walk_u ? bv : bu, se = walk_u ? ev : eu;
            for (int64_t k = wb + lane; k < we; k += L) {
                const int32_t w = col[k];
                int64_t lo = sb, hi = se;
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (col[mid] < w) lo = mid + 1; else hi = mid;
                }
                if (lo < se && col[lo] == w) body.hit(u, v, w, k, lo, walk_u, a);
            }
        }
        body.reduce(a, RjGroup<L>{});
        if (lane == 0 && j < nnz) body.finish(j, a);
    }
}

// (6) every condition that ends a group's work is the same in all of its L lanes, so the lanes of a group are active
// together: the ballot's bits of the group and the shuffles inside it are those of its own lanes
template <int L>
__global__ __launch_bounds__(RJ_BLOCK) void gl_k4_kernel(int64_t nnz, const int32_t *__restrict__ arc_row,
                                                         const int32_t *__restrict__ col,
                                                         const int32_t *__restrict__ sup,
                                                         const int64_t *__restrict__ o_ptr,
                                                         const int32_t *__restrict__ o_col, unsigned long long *k4)
{
    constexpr int APG = RJ_BLOCK / L;
    const int lane = threadIdx.x % L, slot = threadIdx.x / L;
    const int first = threadIdx.x % GRX_WAVE - lane;         // the group's first lane in its wavefront
    const unsigned long long group_bits = (1ull << L) - 1;
    const int64_t groups = (nnz + APG - 1) / APG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t j = g * APG + slot;
        if (j >= nnz || sup[j] < 2) continue;                // a 4-clique gives each of its edges two triangles
        const int32_t u = arc_row[j], v = col[j];
        const int64_t bu = o_ptr[u], eu = o_ptr[u + 1], bv = o_ptr[v], ev = o_ptr[v + 1];
        if (eu - bu < 3 || ev - bv < 2) continue;            // N+(u) holds v, w and x; N+(v) holds w and x
        if (!gl_contains(o_col, bu, eu, v)) continue;        // the other arc of the edge is the oriented one
        const bool walk_u = eu - bu <= ev - bv;
        const int64_t wb = walk_u ? bu : bv, we = walk_u ? eu : ev;
        const int64_t sb = walk_u ? bv : bu, se = walk_u ? ev : eu;
        unsigned long long at_uv = 0;
        for (int64_t k0 = wb; k0 < we; k0 += L) {
            const int64_t k = k0 + lane;
            int32_t w = -1;
            if (k < we) {
                w = o_col[k];
                if (!gl_contains(o_col, sb, se, w)) w = -1;
            }
            unsigned long long hits = (__ballot(w >= 0) >> first) & group_bits;
            while (hits) {
                const int src = __ffsll((long long)hits) - 1;
                hits &= hits - 1;
                const int32_t ww = __shfl(w, src, L);
                const int64_t bw = o_ptr[ww], ew = o_ptr[ww + 1];
                // rows 0, 1, 2 = N+(u), N+(v), N+(w): walk the shortest, search the other two
                const int64_t lu = eu - bu, lv = ev - bv, lw = ew - bw;
                const int pick = lw <= lu && lw <= lv ? 2 : lv <= lu ? 1 : 0;
                const int64_t b0 = pick == 2 ? bw : pick == 1 ? bv : bu, e0 = pick == 2 ? ew : pick == 1 ? ev : eu;
                const int64_t b1 = pick == 0 ? bv : bu, e1 = pick == 0 ? ev : eu;
                const int64_t b2 = pick == 2 ? bv : bw, e2 = pick == 2 ? ev : ew;
                int c = 0;
                for (int64_t i = b0 + lane; i < e0; i += L) {
                    const int32_t x = o_col[i];
                    if (gl_contains(o_col, b1, e1, x) && gl_contains(o_col, b2, e2, x)) {
                        ++c;
                        atomicAdd(&k4[x], 1ull);
                    }
                }
#pragma unroll
                for (int off = L / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, L);
                if (lane == 0 && c) atomicAdd(&k4[ww], (unsigned long long)c);
                at_uv += (unsigned long long)c;
            }
        }
        if (lane == 0 && at_uv) {
            atomicAdd(&k4[u], at_uv);
            atomicAdd(&k4[v], at_uv);
        }
    }
}

// (7)
struct GlNode {
    const int64_t *t, *s1, *n4, *n5, *n6, *n9, *n10, *n12x2, *n13, *k4;
};

__global__ __launch_bounds__(RJ_BLOCK) void gl_finish_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                             const int64_t *__restrict__ squares, GlNode in,
                                                             int64_t *__restrict__ orbits,
                                                             int64_t *__restrict__ noninduced)
{
    for (int64_t v = (int64_t)blockIdx.x * RJ_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * RJ_BLOCK) {
        const int64_t d = row_ptr[v + 1] - row_ptr[v], t = in.t[v];
        int64_t x[GL_ORBITS];
        x[0] = d;
        x[1] = in.s1[v];
        x[2] = d * (d - 1) / 2;
        x[3] = t;
        x[4] = in.n4[v];
        x[5] = in.n5[v];
        x[6] = in.n6[v];
        x[7] = d * (d - 1) / 2 * (d - 2) / 3;
        x[8] = squares[v];
        x[9] = in.n9[v];
        x[10] = in.n10[v];
        x[11] = t * (d - 2);
        x[12] = in.n12x2[v] / 2;
        x[13] = in.n13[v];
        x[14] = in.k4[v];
        if (noninduced)
#pragma unroll
            for (int k = 0; k < GL_ORBITS; ++k) noninduced[k * n + v] = x[k];
        // o_k = N_k - sum_{c > k} A[k][c] o_c, from o14 downward
#pragma unroll
        for (int k = GL_ORBITS - 2; k >= 0; --k)
#pragma unroll
            for (int c = k + 1; c < GL_ORBITS; ++c) x[k] -= GL_A[k][c] * x[c];
#pragma unroll
        for (int k = 0; k < GL_ORBITS; ++k) orbits[k * n + v] = x[k];
    }
}

}  // namespace

extern "C" {

size_t grx_graphlet_orbits_workspace_bytes(int64_t n, int64_t nnz) { return GlWs(nullptr, n, nnz).bytes(); }

int grx_graphlet_orbits(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int64_t *d_o_row_ptr,
                        const int32_t *d_o_col, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                        const int64_t *d_squares, int64_t *d_orbits, int64_t *d_noninduced, int32_t *d_arc_triangles,
                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "grx_graphlet_orbits";
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "%s: n = %lld out of range [0, 2^31)", who, (long long)n);
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_o_row_ptr && d_o_col && d_squares && d_orbits && d_workspace,
                "%s: null pointer", who);
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "%s: lanes_per_row must be 4, 8, 16 or 32 (got %d)", who, lanes_per_row);
    GRX_REQUIRE(n_hub_rows >= 0 && n_hub_rows <= n && (n_hub_rows == 0 || d_hub_rows), "%s: hub list", who);
    const size_t least = GlWs(nullptr, n, 0).bytes();
    GRX_REQUIRE(workspace_bytes >= least, "%s: workspace %zu bytes, need at least %zu", who, workspace_bytes, least);
    RjCall c{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row};
    c.st = grx_stream(stream);
    c.hub_degree = (int64_t)GRX_HUB_FACTOR * lanes_per_row;
    c.nnz = 0;
    int64_t o_nnz = 0;
    GRX_CHECK_HIP(hipMemcpyAsync(&c.nnz, d_row_ptr + n, sizeof(c.nnz), hipMemcpyDeviceToHost, c.st));
    GRX_CHECK_HIP(hipMemcpyAsync(&o_nnz, d_o_row_ptr + n, sizeof(o_nnz), hipMemcpyDeviceToHost, c.st));
    GRX_CHECK_HIP(hipStreamSynchronize(c.st));
    GRX_REQUIRE(c.nnz >= 0 && c.nnz < (int64_t)1 << 31 && c.nnz % 2 == 0,
                "%s: row_ptr[n] = %lld: the arcs of a symmetric CSR without self-loops are even in number and fewer "
                "than 2^31", who, (long long)c.nnz);
    GRX_REQUIRE(o_nnz == c.nnz / 2, "%s: o_row_ptr[n] = %lld: the orientation keeps one arc of every edge (%lld)", who,
                (long long)o_nnz, (long long)(c.nnz / 2));
    const GlWs ws(d_workspace, n, c.nnz);
    GRX_REQUIRE(workspace_bytes >= ws.bytes(), "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.bytes());
    if (c.nnz == 0) {
        grx_fill64(reinterpret_cast<uint64_t *>(d_orbits), GL_ORBITS * n, 0, c.st);
        if (d_noninduced) grx_fill64(reinterpret_cast<uint64_t *>(d_noninduced), GL_ORBITS * n, 0, c.st);
        GRX_LAUNCH_CHECK();
        return GRX_OK;
    }
    int32_t *arc_row = ws.per_arc(0), *rev = ws.per_arc(1);
    int32_t *sup = d_arc_triangles ? d_arc_triangles : ws.per_arc(2);
    unsigned long long *n12x2 = reinterpret_cast<unsigned long long *>(ws.node(GV_N12X2));
    unsigned long long *k4 = reinterpret_cast<unsigned long long *>(ws.node(GV_K4));
    grx_fill64(reinterpret_cast<uint64_t *>(n12x2), n, 0, c.st);
    grx_fill64(reinterpret_cast<uint64_t *>(k4), n, 0, c.st);

    // (1), (2)
    int rc = rj_run(c, arc_row, gl_stats{d_row_ptr, d_col, arc_row, ws.node(GV_S1)},
                    gl_support{d_row_ptr, d_col, arc_row, rev, sup}, gl_stats{}, false);
    if (rc != GRX_OK) return rc;
    gl_mirror_kernel<<<grx_grid(c.nnz, RJ_BLOCK, RJ_ROW_MAX_WG), RJ_BLOCK, 0, c.st>>>(c.nnz, arc_row, d_col, rev, sup);

    // (3), (4): hub rows by a workgroup each, the others by a lane group
    const gl_pass_a pass_a{d_row_ptr, d_col, sup, ws.node(GV_T), ws.node(GV_N5), ws.node(GV_N6), ws.node(GV_N10),
                           ws.node(GV_N13)};
    const gl_pass_b pass_b{d_col, sup, ws.node(GV_T), ws.node(GV_S1), ws.node(GV_N4), ws.node(GV_N9)};
    const gl_diamond diamond{arc_row, sup, n12x2};
    if (n_hub_rows) rj_hub_rows_kernel<<<(unsigned)n_hub_rows, RJ_BLOCK, 0, c.st>>>(d_row_ptr, d_hub_rows, pass_a);
    rj_with_lanes(lanes_per_row, [&](auto width) {
        constexpr int L = decltype(width)::value;
        const unsigned rgrid = grx_grid(n, RJ_BLOCK / L, RJ_ROW_MAX_WG);
        const unsigned agrid = grx_grid(c.nnz, RJ_BLOCK / L, RJ_ARC_MAX_WG);
        rj_rows_kernel<L><<<rgrid, RJ_BLOCK, 0, c.st>>>(n, d_row_ptr, c.hub_degree, pass_a);
        if (n_hub_rows) rj_hub_rows_kernel<<<(unsigned)n_hub_rows, RJ_BLOCK, 0, c.st>>>(d_row_ptr, d_hub_rows, pass_b);
        rj_rows_kernel<L><<<rgrid, RJ_BLOCK, 0, c.st>>>(n, d_row_ptr, c.hub_degree, pass_b);
        // (5), (6)
        gl_diamond_kernel<L><<<agrid, RJ_BLOCK, 0, c.st>>>(c.nnz, d_row_ptr, d_col, diamond);
        gl_k4_kernel<L><<<grx_grid(c.nnz, RJ_BLOCK / L, GL_K4_MAX_WG), RJ_BLOCK, 0, c.st>>>(c.nnz, arc_row, d_col, sup,
                                                                                             d_o_row_ptr, d_o_col, k4);
    });
    // (7)
    const GlNode in{ws.node(GV_T), ws.node(GV_S1), ws.node(GV_N4), ws.node(GV_N5), ws.node(GV_N6), ws.node(GV_N9),
                    ws.node(GV_N10), ws.node(GV_N12X2), ws.node(GV_N13), ws.node(GV_K4)};
    gl_finish_kernel<<<grx_grid(n, RJ_BLOCK, RJ_ROW_MAX_WG), RJ_BLOCK, 0, c.st>>>(n, d_row_ptr, d_squares, in, d_orbits,
                                                                                 d_noninduced);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
