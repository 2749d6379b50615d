// grx_clustering.hip -- the weighted and the directed forms of the clustering coefficient of RolX sense making, as
// networkx 3.4.2's cluster.py defines them: Onnela's geometric mean of the normalised triangle weights, Fagiolo's
// directed coefficient, and the two together.
//
// Over a structurally symmetric CSR (row u lists every neighbour of u in either direction) with a value s per arc
//   undirected  s(u, v) = cbrt(w(u, v) / max_weight)
//   directed    s(u, v) = cbrt(w(u -> v) / max_weight) + cbrt(w(v -> u) / max_weight), an absent direction adds 0
//   no weights  every cube root is 1: s is 1 (undirected) or the number of directions present, 1 or 2
// networkx's numerator is one masked sparse product, a row intersection per arc:
//   t(u) = sum_{v in N(u) \ {u}}  s(u, v) * sum_{w in N(u) & N(v), w not in {u, v}}  s(u, w) * s(v, w)
// (undirected: 2 x its weighted_triangles; directed: its directed_triangles, whose eight cbrt sums per (v, w) are the
// expansion of the three binomials), and clustering(u) = t == 0 ? 0 : t / denominator(u) with
//   undirected  d (d - 1),                d = |N(u) \ {u}|
//   directed    2 (dt (dt - 1) - 2 db),   dt = the directions present at the off-diagonal entries, db = dt - d
// The cube root is taken once per arc and direction, not once per triangle: the intersection loop multiplies only.
// A quotient that equals 1 has the cube root 1 without a call, so constant weights give the unweighted bits, and for
// a graph without weights every quantity is a small integer in fp64: the quotient t / denominator is networkx's own.
//
// Three stages, each a launch for the hub rows (one workgroup per row longer than GRX_HUB_FACTOR * L) and one for the
// rest (a group of L lanes per row); the skeletons are grx_rowjoin.h's, shared with grx_structural_holes.hip, and this
// file holds what a row accumulates, what a hit contributes and what is written:
//   (a) per row: s of every arc, the row of every arc, and the denominator from the counted directions;
//   (b) per arc (u, v), u != v: a group of L lanes walks the shorter of the two rows, lane k entries k, k + L, ...,
//       and looks every entry up in the longer row by binary search (columns ascend); a hit w outside {u, v} adds
//       s(u, w) * s(v, w); the lanes' partial sums meet in the fixed butterfly grx_group_sum<L>; lane 0 writes
//       s(u, v) * sum.  Bound: sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers,
//       plus one 8-byte gather per hit (s of the found entry; s of the walked entry streams with its column):
//       latency- and gather-bound like the ego-net join;
//   (c) per row: the sum of its arcs' terms, lane k the arcs k, k + L, ... in order, then the same butterfly (hub rows:
//       thread t the arcs t, t + 256, ..., then a fixed tree in LDS), and the quotient.
// No floating-point atomics, no hand-off between workgroups inside a launch: every output has the same bits in every
// run.
//
// Compiled with -ffp-contract=off (Makefile; the pragma carries it with the file): every quotient, product and sum is
// its own IEEE operation, so tests/clustering_oracle.py can form the same terms.
#pragma clang fp contract(off)

#include "grx_rowjoin.h"

#include <cmath>

namespace {

// cbrt(w / max_weight); a quotient of exactly 1 needs no call
__device__ __forceinline__ double cl_root(double w, double max_weight)
{
    const double q = w / max_weight;
    return q == 1.0 ? 1.0 : cbrt(q);
}

// s of arc j; *dirs = the directions present there (a negative value marks an absent one)
__device__ __forceinline__ double cl_arc_value(const double *__restrict__ fwd, const double *__restrict__ bwd,
                                               int64_t j, double max_weight, double *dirs)
{
    const double f = fwd[j];
    if (!bwd) {
        *dirs = 1.0;
        return cl_root(f, max_weight);
    }
    const double b = bwd[j];
    const double sf = f >= 0.0 ? cl_root(f, max_weight) : 0.0;
    const double sb = b >= 0.0 ? cl_root(b, max_weight) : 0.0;
    *dirs = (f >= 0.0 ? 1.0 : 0.0) + (b >= 0.0 ? 1.0 : 0.0);
    return sf + sb;
}

// (a) fwd == NULL: no value array is read and s is not written (every s is 1)
struct cl_rows {
    const int32_t *__restrict__ col;
    const double *__restrict__ fwd, *__restrict__ bwd;
    double max_weight;
    double *__restrict__ s, *__restrict__ den;
    int32_t *__restrict__ arc_row;
    struct Acc { double d, dt; };                            // off-diagonal entries, their directions
    __device__ __forceinline__ void entry(int64_t u, int64_t j, Acc &a) const
    {
        arc_row[j] = (int32_t)u;
        double dirs = 1.0;
        if (fwd) s[j] = cl_arc_value(fwd, bwd, j, max_weight, &dirs);
        if (col[j] != (int32_t)u) { a.d += 1.0; a.dt += dirs; }
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.d = r.sum(a.d); a.dt = r.sum(a.dt); }
    // d (d - 1) resp. 2 (dt (dt - 1) - 2 db) from the exact counts
    __device__ __forceinline__ void finish(int64_t u, int64_t, int64_t, const Acc &a) const
    {
        const int64_t di = (int64_t)a.d, dti = (int64_t)a.dt;
        den[u] = bwd ? (double)(2 * (dti * (dti - 1) - 2 * (dti - di))) : (double)(di * (di - 1));
    }
};

// (b) s == NULL: every s is 1
struct cl_arc {
    const double *__restrict__ s;
    double *__restrict__ term;
    struct Acc { double a; };
    __device__ __forceinline__ bool begin(int64_t, int32_t u, int32_t v, Acc &) const { return u != v; }
    // u and v are tested at the hit: skipping their two searches up front splits the group before the search loop and
    // measured 6 % slower (profiles/clustering.txt)
    __device__ __forceinline__ void hit(int32_t u, int32_t v, int32_t w, int64_t k, int64_t lo, bool, Acc &a) const
    {
        if (w != u && w != v) a.a += s ? s[k] * s[lo] : 1.0;
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.a = r.sum(a.a); }
    __device__ __forceinline__ void finish(int64_t j, const Acc &a) const { term[j] = s ? s[j] * a.a : a.a; }
};

// (c)
struct cl_reduce {
    const double *__restrict__ term, *__restrict__ den;
    double *__restrict__ clustering, *__restrict__ triangles;
    struct Acc { double t; };
    __device__ __forceinline__ void entry(int64_t, int64_t j, Acc &a) const { a.t += term[j]; }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.t = r.sum(a.t); }
    __device__ __forceinline__ void finish(int64_t u, int64_t, int64_t, const Acc &a) const
    {
        if (triangles) triangles[u] = a.t;
        clustering[u] = a.t == 0.0 ? 0.0 : a.t / den[u];
    }
};

constexpr int CL_VECS = 1, CL_ARCS = 2;                      // workspace: den | s, term | arc_row

}  // namespace

extern "C" {

size_t grx_clustering_workspace_bytes(int64_t n, int64_t nnz) { return RjWs(nullptr, n, nnz, CL_VECS, CL_ARCS).bytes(); }

int grx_clustering(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_fwd, const double *d_bwd,
                   double max_weight, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                   double *d_clustering, double *d_triangles, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(d_clustering, "grx_clustering: d_clustering is NULL");
    GRX_REQUIRE(d_fwd || !d_bwd, "grx_clustering: d_bwd without d_fwd (a directed graph without weights passes 1 for "
                                 "a present direction)");
    GRX_REQUIRE(!d_fwd || (max_weight > 0.0 && std::isfinite(max_weight)),
                "grx_clustering: max_weight = %g must be finite and > 0", max_weight);
    RjCall c{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row};
    const int rc = rj_prepare("grx_clustering", c, d_workspace, workspace_bytes, CL_VECS, CL_ARCS, stream);
    if (rc != GRX_OK || n == 0) return rc;
    const RjWs ws(d_workspace, n, c.nnz, CL_VECS, CL_ARCS);
    double *den = ws.row(0), *s = ws.per_arc(0), *term = ws.per_arc(1);
    return rj_run(c, ws.arc_row(), cl_rows{d_col, d_fwd, d_bwd, max_weight, s, den, ws.arc_row()},
                  cl_arc{d_fwd ? s : nullptr, term}, cl_reduce{term, den, d_clustering, d_triangles}, true);
}

}  // extern "C"
