// grx_structural_holes.hip -- Burt's structural-hole measures of RolX sense making: constraint, local constraint and
// the weighted / directed form of effective size, as networkx 3.4.2's structuralholes.py defines them.
//
// Over a structurally symmetric CSR with symmetric mutual weights z (NULL: every z = 1)
//   S(u) = sum_x z(u, x),  X(u) = max_x z(u, x),  P(u, v) = z(u, v) / S(u),  M(v, w) = z(v, w) / X(v)   (0 / 0 = 0)
//   local(u, v)       = (P(u, v) + sum_w P(u, w) P(w, v))^2          constraint(u)     = sum_v local(u, v)
//   effective_size(u) = sum_v (1 - sum_w P(u, w) M(v, w))
// where v runs over row u and w over the common entries of the rows of u and v: both inner sums are one masked sparse
// product, a row intersection per arc.  z(w, v) is read as z(v, w), the entry of row v that the intersection finds.
//
// Three stages, each a launch for the hub rows (one workgroup per row longer than GRX_HUB_FACTOR * L) and one for the
// rest (a group of L lanes per row); the skeletons are grx_rowjoin.h's, shared with grx_clustering.hip, and this file
// holds what a row accumulates, what a hit contributes and what is written:
//   (a) row statistics: S and X of every row, and the row of every arc (the per-arc stage is parallel over arcs);
//   (b) per arc (u, v): a group of L lanes walks the shorter of the two rows, lane k entries k, k + L, ..., and looks
//       every entry up in the longer row by binary search (columns ascend); a hit w adds P(u, w) * P(w, v) and
//       P(u, w) * M(v, w), every quotient and product rounded on its own; the lanes' partial sums meet in the fixed
//       butterfly grx_group_sum<L>; lane 0 writes local(u, v) and 1 - redundancy(u, v) of the arc.  The 10^4 arcs of
//       a hub row are 10^4 independent groups spread over the chip.
//       Bound: sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers, plus two 8-byte
//       gathers per hit (z of the found entry, S(w)): latency- and gather-bound like the ego-net join;
//   (c) per row: the sum of its arcs' terms, lane k the arcs k, k + L, ... in order, then the same butterfly (hub rows:
//       thread t the arcs t, t + 256, ..., then a fixed tree in LDS).  NaN for a row that is empty in d_out_row_ptr.
// No floating-point atomics, no hand-off between workgroups inside a launch: every output has the same bits in every
// run.
//
// Compiled with -ffp-contract=off (Makefile; the pragma carries it with the file): every quotient, product and sum is
// its own IEEE operation, so tests/structural_holes_oracle.py can form the same terms.
#pragma clang fp contract(off)

#include "grx_rowjoin.h"

namespace {

// (a) z == NULL: S = the row length, X = 1 (0 for an empty row); no value array is read and nothing is reduced
struct sh_stats {
    const double *__restrict__ z;
    double *__restrict__ S, *__restrict__ X;
    int32_t *__restrict__ arc_row;
    struct Acc { double s, x; };
    __device__ __forceinline__ void entry(int64_t u, int64_t j, Acc &a) const
    {
        arc_row[j] = (int32_t)u;
        if (z) { const double zz = z[j]; a.s += zz; a.x = fmax(a.x, zz); }
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const
    {
        if (z) { a.s = r.sum(a.s); a.x = r.max(a.x); }
    }
    __device__ __forceinline__ void finish(int64_t u, int64_t b, int64_t e, const Acc &a) const
    {
        S[u] = z ? a.s : (double)(e - b);
        X[u] = z ? a.x : e > b ? 1.0 : 0.0;
    }
};

// (b) loc == NULL / red == NULL: that term is not formed
struct sh_arc {
    const double *__restrict__ z, *__restrict__ S, *__restrict__ X;
    double *__restrict__ loc, *__restrict__ red;
    struct Acc { double a, r, su, xv; };
    __device__ __forceinline__ bool begin(int64_t, int32_t u, int32_t v, Acc &a) const
    {
        a.su = S[u];
        a.xv = X[v];
        return true;
    }
    __device__ __forceinline__ void hit(int32_t, int32_t, int32_t w, int64_t k, int64_t lo, bool walk_u, Acc &a) const
    {
        const int64_t ku = walk_u ? k : lo, kv = walk_u ? lo : k;
        const double zuw = z ? z[ku] : 1.0, zvw = z ? z[kv] : 1.0;
        const double puw = a.su != 0.0 ? zuw / a.su : 0.0;
        if (loc) {
            const double sw = S[w];
            const double pwv = sw != 0.0 ? zvw / sw : 0.0;
            a.a += puw * pwv;
        }
        if (red) {
            const double mvw = a.xv != 0.0 ? zvw / a.xv : 0.0;
            a.r += puw * mvw;
        }
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.a = r.sum(a.a); a.r = r.sum(a.r); }
    __device__ __forceinline__ void finish(int64_t j, const Acc &a) const
    {
        if (loc) {
            const double zuv = z ? z[j] : 1.0;
            const double puv = a.su != 0.0 ? zuv / a.su : 0.0;
            const double t = puv + a.a;
            loc[j] = t * t;
        }
        if (red) red[j] = 1.0 - a.r;
    }
};

// (c) NaN for a row that is empty in out_row_ptr
struct sh_reduce {
    const int64_t *__restrict__ out_row_ptr;
    const double *__restrict__ loc, *__restrict__ red;
    double *__restrict__ constraint, *__restrict__ effective_size;
    struct Acc { double c, s; };
    __device__ __forceinline__ void entry(int64_t, int64_t j, Acc &a) const
    {
        if (constraint) a.c += loc[j];
        if (effective_size) a.s += red[j];
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.c = r.sum(a.c); a.s = r.sum(a.s); }
    __device__ __forceinline__ void finish(int64_t u, int64_t, int64_t, const Acc &a) const
    {
        const bool empty = out_row_ptr[u + 1] == out_row_ptr[u];
        if (constraint) constraint[u] = empty ? __builtin_nan("") : a.c;
        if (effective_size) effective_size[u] = empty ? __builtin_nan("") : a.s;
    }
};

constexpr int SH_VECS = 2, SH_ARCS = 2;                      // workspace: S, X | loc, red | arc_row

}  // namespace

extern "C" {

size_t grx_structural_holes_workspace_bytes(int64_t n, int64_t nnz)
{
    return RjWs(nullptr, n, nnz, SH_VECS, SH_ARCS).bytes();
}

int grx_structural_holes(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_z,
                         const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                         const int64_t *d_out_row_ptr, double *d_constraint, double *d_effective_size,
                         double *d_local, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(d_constraint || d_effective_size || d_local,
                "grx_structural_holes: d_constraint, d_effective_size and d_local are all NULL");
    RjCall c{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row};
    const int rc = rj_prepare("grx_structural_holes", c, d_workspace, workspace_bytes, SH_VECS, SH_ARCS, stream);
    if (rc != GRX_OK || n == 0) return rc;
    const RjWs ws(d_workspace, n, c.nnz, SH_VECS, SH_ARCS);
    double *S = ws.row(0), *X = ws.row(1);
    // the per-arc terms: local constraint straight into the caller's array when it asks for it
    double *loc = d_local ? d_local : d_constraint ? ws.per_arc(0) : nullptr;
    double *red = d_effective_size ? ws.per_arc(1) : nullptr;
    return rj_run(c, ws.arc_row(), sh_stats{d_z, S, X, ws.arc_row()}, sh_arc{d_z, S, X, loc, red},
                  sh_reduce{d_out_row_ptr ? d_out_row_ptr : d_row_ptr, loc, red, d_constraint, d_effective_size},
                  d_constraint || d_effective_size);
}

}  // extern "C"
