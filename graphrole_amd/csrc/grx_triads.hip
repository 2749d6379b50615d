// grx_triads.hip -- the triad census of a directed graph, per node and for the graph (Holland and Leinhardt 1970;
// networkx's triadic_census): for each of the 16 isomorphism classes of three nodes with their arcs, the number of
// triads of that class that contain the node.  Columns in networkx's order (TRIAD_NAMES):
//    0 003    1 012    2 102    3 021D   4 021U   5 021C   6 111D   7 111U
//    8 030T   9 030C  10 201   11 120D  12 120U  13 120C  14 210   15 300
//
// Input: the structurally symmetric all-neighbours CSR (ascending distinct columns, no diagonal entry) and one direction
// code per arc slot (u, v): 1 = only u -> v, 2 = only v -> u, 3 = both; the code at (v, u) is the mirror of the one at
// (u, v).  Seen from a node, a neighbour is of class O (out-only, code 1), I (in-only, code 2) or M (mutual, code 3);
// o, i, m are their numbers at the node and d = o + i + m; a pair is asymmetric (code 1 or 2) or mutual (code 3), and
// E_a, E_m are the numbers of such pairs in the graph.
//
// Only the closed triads are enumerated; no open and no dyadic triad is.  Three stages of grx_rowjoin.h (one rj_run):
//   (a) per row (td_stats): the row of every arc, and (o, i, m);
//   (b) per arc (u, v) with u < v (td_arc): one row intersection.  Every hit w counts into common(u, v), written at
//       both slots of the pair (the reverse slot by one binary search).  A hit w > v is a closed triad u < v < w, found
//       exactly once: its 6-bit code is c(u, v) | c(u, w) << 2 | c(v, w) << 4 from the three slots' direction codes,
//       TD_TYPE turns it into the column, and six 64-bit integer atomics follow: one into that column at u, v and w, and
//       one at each of the three into the counter "closed triads here whose opposite pair is asymmetric / mutual";
//   (c) per row y (td_sums), over the entries u of the row with x = the class of y as seen from u: the nine sums
//       S[x][z] of cnt_z(u), and common(y, u) summed over the asymmetric and over the mutual pairs; then, in int64:
//       1. the non-induced wedges that hold y, by type -- as the centre C(o, 2), C(i, 2), o i, m i, m o, C(m, 2) for
//          021D, 021U, 021C, 111D, 111U, 201, and as an end S[x][z] - [z = x] (the neighbours that see y as x) into the
//          type of the class pair: (O,O) 021D, (I,I) 021U, (O,I) 021C, (M,I) 111D, (M,O) 111U, (M,M) 201;
//       2. open triads = those minus TD_OPEN^T applied to the closed columns.  Dropping each of the three pairs of a
//          closed triad in turn leaves three wedges whose types depend on the closed type alone, and every node of the
//          triad is in each of them.  TD_OPEN[closed][wedge], wedges in the order 021D 021U 021C 111D 111U 201:
//              030T  1 1 1 0 0 0      120D  1 0 0 2 0 0      120C  0 0 1 1 1 0      300  0 0 0 0 0 3
//              030C  0 0 3 0 0 0      120U  0 1 0 0 2 0      210   0 0 0 1 1 1
//       3. dyadic triads with y on the pair (012 from the asymmetric pairs, 102 from the mutual ones): the sum over the
//          neighbours u across such a pair of n - d(y) - d(u) + common(y, u);
//       4. dyadic triads with y the isolate: E_K - (sum over u in N(y) of deg_K(u)) + opp_K(y), with deg_a = o + i,
//          deg_m = m and opp_K the counter of (b): the pairs of class K minus those that touch N[y];
//       5. 003 = C(n - 1, 2) minus the other fifteen.
// The totals are the column sums (integer block sums and one atomic per workgroup and column) divided by 3.
// Only integer atomics, and nothing depends on their order: the same bits in every run, for every lanes_per_row and
// every relabelling.  The row-join reductions carry doubles that hold integers: the outputs are exact while every
// intermediate (the largest is C(n - 1, 2) resp. a sum of degrees over a row) is below 2^53; the final arithmetic is
// int64.  The arc kernel has no hub path: one lane group walks a hub-hub intersection alone (a known cost of
// grx_rowjoin.h).  The pragma is the include rule of grx_rowjoin.h.
#pragma clang fp contract(off)

#include "grx_rowjoin.h"

namespace {

constexpr int TD_TYPES = 16;
constexpr int TD_MAX_WG = 2048;          // workgroups of td_pairs_kernel and (per column) of td_totals_kernel

// the column of the triad (a, b, c) with the code c(a, b) | c(a, c) << 2 | c(b, c) << 4 (networkx's TRICODES - 1)
constexpr int TD_TYPE[64] = {
    0, 1, 1, 2, 1, 3, 5, 7, 1, 5, 4, 6, 2, 7, 6, 10,
    1, 5, 3, 7, 4, 8, 8, 12, 5, 9, 8, 13, 6, 13, 11, 14,
    1, 4, 5, 6, 5, 8, 9, 13, 3, 8, 8, 11, 7, 12, 13, 14,
    2, 6, 7, 10, 6, 11, 13, 14, 7, 13, 12, 14, 10, 14, 14, 15,
};
// sixteen entries of it, four bits each: the table travels in four 64-bit constants, not behind a load
constexpr uint64_t td_packed(int quarter)
{
    uint64_t w = 0;
    for (int k = 0; k < 16; ++k) w |= (uint64_t)TD_TYPE[quarter * 16 + k] << (4 * k);
    return w;
}
constexpr uint64_t TD_W0 = td_packed(0), TD_W1 = td_packed(1), TD_W2 = td_packed(2), TD_W3 = td_packed(3);

__device__ __forceinline__ int td_type(int code)
{
    const uint64_t w = code < 32 ? (code < 16 ? TD_W0 : TD_W1) : (code < 48 ? TD_W2 : TD_W3);
    return (int)(w >> ((code & 15) * 4)) & 15;
}

constexpr int TD_WEDGES = 6, TD_CLOSED = 7;
constexpr int TD_WEDGE_COL[TD_WEDGES] = {3, 4, 5, 6, 7, 10};
constexpr int TD_CLOSED_COL[TD_CLOSED] = {8, 9, 11, 12, 13, 14, 15};
constexpr int TD_OPEN[TD_CLOSED][TD_WEDGES] = {
    {1, 1, 1, 0, 0, 0},
    {0, 0, 3, 0, 0, 0},
    {1, 0, 0, 2, 0, 0},
    {0, 1, 0, 0, 2, 0},
    {0, 0, 1, 1, 1, 0},
    {0, 0, 0, 1, 1, 1},
    {0, 0, 0, 0, 0, 3},
};

// workspace: (o, i, m, -) int32 x 4 per node (two vectors) | opp_a | opp_m | pair counters (one vector) | arc_row |
// common (int32[nnz] each); every array 256-byte aligned
constexpr int TD_VECS = 5;
struct TdWs {
    RjWs rj;
    TdWs(void *b, int64_t n, int64_t nnz) : rj(b, n, nnz, TD_VECS, 0) {}
    int4 *oim() const { return reinterpret_cast<int4 *>(rj.row(0)); }
    unsigned long long *opp(int k) const { return reinterpret_cast<unsigned long long *>(rj.row(2 + k)); }
    unsigned long long *pairs() const { return reinterpret_cast<unsigned long long *>(rj.row(4)); }
    int32_t *common() const { return reinterpret_cast<int32_t *>(rj.base + rj.bytes()); }
    size_t bytes() const { return rj.bytes() + rj.tail; }
};

// the sum of v over the workgroup, in thread 0
__device__ __forceinline__ unsigned long long td_block_sum(unsigned long long v, unsigned long long *sm)
{
    const int t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = RJ_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] += sm[t + s];
        __syncthreads();
    }
    const unsigned long long r = sm[0];
    __syncthreads();
    return r;
}

// pairs[0], pairs[1] += the arc slots of asymmetric and of mutual pairs (twice E_a, twice E_m)
__global__ __launch_bounds__(RJ_BLOCK) void td_pairs_kernel(int64_t nnz, const uint8_t *__restrict__ code,
                                                            unsigned long long *pairs)
{
    __shared__ unsigned long long sm[RJ_BLOCK];
    unsigned long long asym = 0, mutual = 0;
    for (int64_t j = (int64_t)blockIdx.x * RJ_BLOCK + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * RJ_BLOCK) {
        const int c = code[j] & 3;
        asym += c == 1 || c == 2;
        mutual += c == 3;
    }
    asym = td_block_sum(asym, sm);
    mutual = td_block_sum(mutual, sm);
    if (threadIdx.x == 0) {
        if (asym) atomicAdd(&pairs[0], asym);
        if (mutual) atomicAdd(&pairs[1], mutual);
    }
}

// (a)
struct td_stats {
    const uint8_t *__restrict__ code;
    int32_t *__restrict__ arc_row;
    int4 *__restrict__ oim;
    struct Acc { double o, i, m; };                          // integers below 2^53: exact in every order
    __device__ __forceinline__ void entry(int64_t u, int64_t j, Acc &a) const
    {
        arc_row[j] = (int32_t)u;
        const int c = code[j] & 3;
        a.o += c == 1 ? 1.0 : 0.0;
        a.i += c == 2 ? 1.0 : 0.0;
        a.m += c == 3 ? 1.0 : 0.0;
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.o = r.sum(a.o); a.i = r.sum(a.i); a.m = r.sum(a.m); }
    __device__ __forceinline__ void finish(int64_t u, int64_t, int64_t, const Acc &a) const
    {
        oim[u] = make_int4((int)a.o, (int)a.i, (int)a.m, 0);
    }
};

// (b)
struct td_arc {
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col, *__restrict__ arc_row;
    const uint8_t *__restrict__ code;
    int64_t n;
    unsigned long long *__restrict__ out, *__restrict__ opp_a, *__restrict__ opp_m;
    int32_t *__restrict__ common;
    struct Acc { double c; int cuv; };
    __device__ __forceinline__ bool begin(int64_t j, int32_t u, int32_t v, Acc &a) const
    {
        if (u >= v) return false;
        a.cuv = code[j] & 3;
        return true;
    }
    __device__ __forceinline__ void hit(int32_t u, int32_t v, int32_t w, int64_t k, int64_t lo, bool walk_u, Acc &a) const
    {
        a.c += 1.0;
        if (w <= v) return;
        const int cuw = code[walk_u ? k : lo] & 3, cvw = code[walk_u ? lo : k] & 3;      // k is in the walked row
        unsigned long long *column = out + td_type(a.cuv | cuw << 2 | cvw << 4) * n;
        atomicAdd(column + u, 1ull);
        atomicAdd(column + v, 1ull);
        atomicAdd(column + w, 1ull);
        atomicAdd((cvw == 3 ? opp_m : opp_a) + u, 1ull);
        atomicAdd((cuw == 3 ? opp_m : opp_a) + v, 1ull);
        atomicAdd((a.cuv == 3 ? opp_m : opp_a) + w, 1ull);
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const { a.c = r.sum(a.c); }
    __device__ __forceinline__ void finish(int64_t j, const Acc &a) const
    {
        const int32_t u = arc_row[j], v = col[j];
        if (u >= v) return;
        int64_t lo = row_ptr[v], hi = row_ptr[v + 1];
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (col[mid] < u) lo = mid + 1; else hi = mid;
        }
        common[j] = (int32_t)a.c;
        if (lo < end && col[lo] == u) common[lo] = (int32_t)a.c;      // a symmetric CSR holds (v, u)
    }
};

// (c) and the finish
struct td_sums {
    const int32_t *__restrict__ col;
    const uint8_t *__restrict__ code;
    const int4 *__restrict__ oim;
    const int32_t *__restrict__ common;
    const unsigned long long *__restrict__ opp_a, *__restrict__ opp_m, *__restrict__ pairs;
    int64_t n;
    int64_t *out;                                            // the closed columns are read, the others written
    struct Acc { double s[3][3], ca, cm; };                  // s[x][z], x and z over O, I, M
    __device__ __forceinline__ void entry(int64_t, int64_t j, Acc &a) const
    {
        const int c = code[j] & 3;
        const int4 q = oim[col[j]];
        const double cm = (double)common[j];
        const int x = c == 3 ? 2 : c == 1 ? 1 : 0;           // y -> u only: u sees y as I; u -> y only: as O
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.s[k][0] += x == k ? (double)q.x : 0.0;
            a.s[k][1] += x == k ? (double)q.y : 0.0;
            a.s[k][2] += x == k ? (double)q.z : 0.0;
        }
        a.ca += c == 3 ? 0.0 : cm;
        a.cm += c == 3 ? cm : 0.0;
    }
    template <class R>
    __device__ __forceinline__ void reduce(Acc &a, R r) const
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int z = 0; z < 3; ++z) a.s[k][z] = r.sum(a.s[k][z]);
        a.ca = r.sum(a.ca);
        a.cm = r.sum(a.cm);
    }
    __device__ __forceinline__ void finish(int64_t y, int64_t, int64_t, const Acc &a) const
    {
        enum { KO = 0, KI = 1, KM = 2 };
        const int4 q = oim[y];
        const int64_t o = q.x, i = q.y, m = q.z, d = o + i + m;
        int64_t s[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int z = 0; z < 3; ++z) s[k][z] = (int64_t)a.s[k][z];
        // 1.: i neighbours see y as O, o see it as I, m as M
        int64_t wedge[TD_WEDGES] = {
            o * (o - 1) / 2 + s[KO][KO] - i, i * (i - 1) / 2 + s[KI][KI] - o, o * i + s[KO][KI] + s[KI][KO],
            m * i + s[KM][KI] + s[KI][KM],     m * o + s[KM][KO] + s[KO][KM],     m * (m - 1) / 2 + s[KM][KM] - m,
        };
        // 2.
        int64_t others = 0;
#pragma unroll
        for (int k = 0; k < TD_CLOSED; ++k) {
            const int64_t t = out[TD_CLOSED_COL[k] * n + y];
            others += t;
#pragma unroll
            for (int w = 0; w < TD_WEDGES; ++w) wedge[w] -= TD_OPEN[k][w] * t;
        }
#pragma unroll
        for (int w = 0; w < TD_WEDGES; ++w) {
            out[TD_WEDGE_COL[w] * n + y] = wedge[w];
            others += wedge[w];
        }
        // 3., 4.
        // the degrees of the neighbours across an asymmetric / a mutual pair, and the deg_K of all neighbours
        const int64_t d_a = s[KO][KO] + s[KO][KI] + s[KO][KM] + s[KI][KO] + s[KI][KI] + s[KI][KM];
        const int64_t d_m = s[KM][KO] + s[KM][KI] + s[KM][KM];
        const int64_t deg_a = s[KO][KO] + s[KI][KO] + s[KM][KO] + s[KO][KI] + s[KI][KI] + s[KM][KI];
        const int64_t deg_m = s[KO][KM] + s[KI][KM] + s[KM][KM];
        const int64_t e_a = (int64_t)(pairs[0] / 2), e_m = (int64_t)(pairs[1] / 2);
        const int64_t t012 = (o + i) * (n - d) - d_a + (int64_t)a.ca + e_a - deg_a + (int64_t)opp_a[y];
        const int64_t t102 = m * (n - d) - d_m + (int64_t)a.cm + e_m - deg_m + (int64_t)opp_m[y];
        out[1 * n + y] = t012;
        out[2 * n + y] = t102;
        // 5.
        out[y] = (n - 1) * (n - 2) / 2 - others - t012 - t102;
    }
};

// totals[t] += the sum of column t (blockIdx.y) over this workgroup's rows
__global__ __launch_bounds__(RJ_BLOCK) void td_totals_kernel(int64_t n, const int64_t *__restrict__ out,
                                                             unsigned long long *totals)
{
    __shared__ unsigned long long sm[RJ_BLOCK];
    const int64_t *column = out + (int64_t)blockIdx.y * n;
    unsigned long long sum = 0;
    for (int64_t v = (int64_t)blockIdx.x * RJ_BLOCK + threadIdx.x; v < n; v += (int64_t)gridDim.x * RJ_BLOCK)
        sum += (unsigned long long)column[v];
    sum = td_block_sum(sum, sm);
    if (threadIdx.x == 0 && sum) atomicAdd(&totals[blockIdx.y], sum);
}

// every triad is counted at its three nodes
__global__ void td_third_kernel(unsigned long long *totals)
{
    if (threadIdx.x < TD_TYPES) totals[threadIdx.x] /= 3;
}

}  // namespace

extern "C" {

size_t grx_triad_census_workspace_bytes(int64_t n, int64_t nnz) { return TdWs(nullptr, n, nnz).bytes(); }

int grx_triad_census(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const uint8_t *d_codes,
                     const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row, int64_t *d_census,
                     int64_t *d_totals, int32_t *d_arc_triads, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "grx_triad_census";
    GRX_REQUIRE(n <= 0 || (d_codes && d_census), "%s: null pointer", who);
    const size_t least = TdWs(nullptr, n, 0).bytes();          // rj_prepare knows of the row-join arrays alone
    GRX_REQUIRE(n <= 0 || workspace_bytes >= least, "%s: workspace %zu bytes, need at least %zu", who, workspace_bytes,
                least);
    RjCall c{n, d_row_ptr, d_col, d_hub_rows, n_hub_rows, lanes_per_row};
    const int rc = rj_prepare(who, c, d_workspace, workspace_bytes, TD_VECS, 0, stream);
    if (rc != GRX_OK || n == 0) return rc;
    const TdWs ws(d_workspace, n, c.nnz);
    GRX_REQUIRE(workspace_bytes >= ws.bytes(), "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.bytes());
    int32_t *arc_row = ws.rj.arc_row(), *common = d_arc_triads ? d_arc_triads : ws.common();
    unsigned long long *out = reinterpret_cast<unsigned long long *>(d_census);
    unsigned long long *totals = reinterpret_cast<unsigned long long *>(d_totals);
    // what the atomics add into: the closed columns 8, 9 and 11 .. 15 (column 10 lies between and is written later),
    // the two counters and the pair counts (three consecutive vectors of the workspace), the totals
    grx_fill64(reinterpret_cast<uint64_t *>(out + 8 * n), 8 * n, 0, c.st);
    grx_fill64(reinterpret_cast<uint64_t *>(ws.opp(0)), (int64_t)(3 * ws.rj.vec / 8), 0, c.st);
    if (totals) grx_fill64(reinterpret_cast<uint64_t *>(totals), TD_TYPES, 0, c.st);
    if (c.nnz > 0)
        td_pairs_kernel<<<grx_grid(c.nnz, RJ_BLOCK, TD_MAX_WG), RJ_BLOCK, 0, c.st>>>(c.nnz, d_codes, ws.pairs());
    const int run = rj_run(c, arc_row, td_stats{d_codes, arc_row, ws.oim()},
                           td_arc{d_row_ptr, d_col, arc_row, d_codes, n, out, ws.opp(0), ws.opp(1), common},
                           td_sums{d_col, d_codes, ws.oim(), common, ws.opp(0), ws.opp(1), ws.pairs(), n, d_census},
                           true);
    if (run != GRX_OK || !totals) return run;
    td_totals_kernel<<<dim3(grx_grid(n, RJ_BLOCK, TD_MAX_WG), TD_TYPES), RJ_BLOCK, 0, c.st>>>(n, d_census, totals);
    td_third_kernel<<<1, GRX_WAVE, 0, c.st>>>(totals);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
