// grx_neighbor_sense.hip -- the neighbour-role pass of RolX NeighborSense (Henderson et al., KDD 2012, section 4): the
// node x role table N = op(A) P of the memberships P of every node's neighbours, a sparse x dense product over a device
// CSR with 1 <= r <= GRX_MAX_ROLES dense columns.  RoleExtractor.neighbor_sense fits Q >= 0 with P Q ~ N from it.
//
//   N[k, i] = sum over the arcs p of row i of w_p * P[col_p, k]            (sum; w == NULL: every w_p = 1)
//   N[k, i] = that sum / sum_p w_p                                         (mean; 0 for a row of zero strength)
// P is node-major (a membership row is 8 r contiguous bytes: what one arc gathers), N feature-major (what grx_gram reads).
//
// Summation order (include/grx.h states it for callers): the arcs of a row are dealt to 8 VIRTUAL slots by their position
// in the row modulo 8 (128 slots for a row with more than NS_LONG_ROW = 1024 arcs), every slot adds its terms in ascending
// order, and the slots meet in the tree h = 4, 2, 1 (64, 32, ...): slot t += slot t + h.  It depends on the positions of
// the row's arcs only, so every launch shape below gives the same bits, and so does every run.  No floating-point
// atomics.  Compiled without contraction (the pragma below): every product is rounded before it is added, so
// tests/neighbor_sense_oracle.py restates the result bit for bit.
//
// Launch shape, the one of grx_aggregate's gather.  A row is walked by G = S x CL lanes (lanes_per_row).  The CL adjacent
// lanes of a slot fetch one membership row together, 16 bytes (two columns) each, so one request covers the row: CL =
// ceil(r / 2) rounded up to a power of two, 1 .. 16, follows from r (the lanes past the row's end idle: one of four at
// r = 6).  S = 1, 2, 4 or 8 PHYSICAL slots carry the 8 virtual ones, A = 8 / S accumulator pairs per lane: per trip of
// 8 arcs a lane loads its A column indices, then its A row fragments -- A independent gathers in flight --, then adds.
// Tree levels between accumulators of one lane are local adds, the others xor-shuffles.  Fewer slots = more gathers in
// flight per lane and more rows per wavefront; the library takes S = 32 / CL, at most 8: 32 lanes per row from r = 5 on,
// the fastest or within 3 % of it at r = 6 and r = 32 (profiles/neighbor_sense.txt).  Rows are 8-byte
// aligned only (any leading dimension): the 16-byte loads are declared so and gfx950 serves them unaligned.
// A long row is skipped there and taken by a whole workgroup of a second launch: min(128, 256 / CL) physical slots carry
// the 128 virtual ones, whose partial rows meet in a tree in LDS (32 KB).  That launch deals the rows to its workgroups
// round-robin (workgroup w looks at the rows w, w + W, ...: 16 bytes of row pointers per node), because a degree-sorted
// graph has its hubs in its first rows: left to the workgroups of the first launch, the 105 long rows of BA 1 M / m = 10
// queued up in a handful of them and made the call up to 2.7 times slower.  Two launches, no workspace, no list of long rows,
// no device -> host read.  No instantiation uses scratch memory.
//
// Bound: per arc one 4-byte column index (streamed), 8 bytes of weight (streamed, when given) and one gathered membership
// row of 8 r bytes; per node 16 bytes of row pointers and 8 r bytes written.  The gather dominates: 20 M arcs x 48 B at
// BA 1 M / m = 10 / r = 6 (profiles/neighbor_sense.txt).
#pragma clang fp contract(off)

#include "grx_common.h"

namespace {

constexpr int NS_BLOCK = 256;
constexpr int NS_SLOTS = 8;              // virtual arc slots of a row
constexpr int NS_LONG_SLOTS = 128;       // virtual arc slots of a long row
constexpr int NS_LONG_ROW = 1024;        // a row with more arcs than this is a long row
constexpr int NS_DEFAULT_LANES = 32;     // lanes per row the library aims at: S = 32 / CL, at most 8
constexpr int NS_GATHERS = 4;            // gathers a lane keeps in flight
constexpr int NS_MAX_WG = 8192;
constexpr int NS_LONG_MAX_WG = 1024;     // workgroups of the long-row launch
constexpr int NS_LDR = GRX_MAX_ROLES;    // stride of a partial row in LDS

struct NsArgs {
    int64_t n;
    const int64_t *__restrict__ row_ptr;
    const int32_t *__restrict__ col;
    const double *__restrict__ w;
    const double *__restrict__ P;
    int64_t ldp;
    int r, mean;
    double *__restrict__ out;
    int64_t ldo;
};

struct NsPair { double x, y; };          // the two columns 2 part, 2 part + 1 of a lane

// this lane's fragment of membership row v; 0.0 past the row's end
__device__ __forceinline__ NsPair ns_load(const NsArgs &A, int64_t v, int part)
{
    typedef double ns_vec2 __attribute__((ext_vector_type(2)));
    typedef ns_vec2 ns_double2 __attribute__((aligned(8)));   // rows are 8-byte aligned: any leading dimension
    const double *__restrict__ row = A.P + v * A.ldp;
    const int k = 2 * part;
    NsPair f{0.0, 0.0};
    if (k + 1 < A.r) {
        const ns_double2 both = *reinterpret_cast<const ns_double2 *>(row + k);
        f.x = both.x;
        f.y = both.y;
    } else if (k < A.r) {
        f.x = row[k];
    }
    return f;
}

// NT trips of one lane: its NA arcs at positions q0 + j period + t stride (j < NT, t < NA) of the row [b, b + d) -- the
// column indices first, then the row fragments (NT x NA independent gathers in flight), then, trip after trip,
// acc[t] += w * fragment and den[t] += w.  A position past the row's end loads nothing and adds +0.0, which changes no
// bit (an accumulator that starts from +0.0 never holds -0.0).
template <int NA, int NT, bool WEIGHTED>
__device__ __forceinline__ void ns_trips(const NsArgs &A, int64_t b, int64_t d, int64_t q0, int stride, int period,
                                         int part, NsPair (&acc)[NA], double (&den)[NA])
{
    int64_t v[NT][NA];
    double wp[NT][NA];
    NsPair f[NT][NA];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            const int64_t q = q0 + (int64_t)j * period + (int64_t)t * stride;
            v[j][t] = 0;
            wp[j][t] = 0.0;
            if (q < d) {
                v[j][t] = A.col[b + q];
                if (WEIGHTED) wp[j][t] = A.w[b + q];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            f[j][t] = NsPair{0.0, 0.0};
            if (q0 + (int64_t)j * period + (int64_t)t * stride < d) f[j][t] = ns_load(A, v[j][t], part);
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            if (WEIGHTED) {
                acc[t].x += wp[j][t] * f[j][t].x;
                acc[t].y += wp[j][t] * f[j][t].y;
                den[t] += wp[j][t];
            } else {
                acc[t].x += f[j][t].x;
                acc[t].y += f[j][t].y;
            }
        }
    }
}

__device__ __forceinline__ double ns_value(double sum, double den, int mean)
{
    return !mean ? sum : den != 0.0 ? sum / den : 0.0;
}

// row u = [b, e), more than NS_LONG_ROW arcs, by the whole workgroup; every thread calls it
template <int CL, bool WEIGHTED>
__device__ __forceinline__ void ns_long_row(const NsArgs &A, int64_t u, int64_t b, int64_t e, double *sm, double *sd)
{
    constexpr int LS = NS_BLOCK / CL < NS_LONG_SLOTS ? NS_BLOCK / CL : NS_LONG_SLOTS;   // physical slots
    constexpr int NA = NS_LONG_SLOTS / LS;                                              // virtual slots of a lane
    const int slot = threadIdx.x / CL, part = threadIdx.x % CL, k = 2 * part;
    const int64_t d = e - b;
    if (slot < LS) {
        NsPair acc[NA] = {};
        double den[NA] = {};
        for (int64_t i = 0; i < d; i += 2 * NS_LONG_SLOTS)
            ns_trips<NA, 2, WEIGHTED>(A, b, d, i + slot, LS, NS_LONG_SLOTS, part, acc, den);
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            const int v = slot + t * LS;                    // the virtual slot
            if (k < A.r) sm[v * NS_LDR + k] = acc[t].x;
            if (k + 1 < A.r) sm[v * NS_LDR + k + 1] = acc[t].y;
            if (WEIGHTED && part == 0) sd[v] = den[t];
        }
    }
    __syncthreads();
    for (int h = NS_LONG_SLOTS / 2; h > 0; h >>= 1) {
        for (int v = slot; v < h; v += NS_BLOCK / CL) {     // 256 / CL lane groups share the h sums of the level
            if (k < A.r) sm[v * NS_LDR + k] += sm[(v + h) * NS_LDR + k];
            if (k + 1 < A.r) sm[v * NS_LDR + k + 1] += sm[(v + h) * NS_LDR + k + 1];
            if (WEIGHTED && part == 0) sd[v] += sd[v + h];
        }
        __syncthreads();
    }
    if (slot == 0) {
        const double den = WEIGHTED ? sd[0] : (double)d;
        if (k < A.r) A.out[(int64_t)k * A.ldo + u] = ns_value(sm[k], den, A.mean);
        if (k + 1 < A.r) A.out[(int64_t)(k + 1) * A.ldo + u] = ns_value(sm[k + 1], den, A.mean);
    }
    __syncthreads();
}

// one level of the tree over the 8 virtual slots v = slot + t S of a row: v += v + H for every v < H
template <int H, int S, int CL, bool WEIGHTED, int NA>
__device__ __forceinline__ void ns_level(NsPair (&acc)[NA], double (&den)[NA])
{
    if constexpr (H >= S) {                                 // partners in one lane: accumulators H / S apart
#pragma unroll
        for (int t = 0; t < H / S; ++t) {
            acc[t].x += acc[t + H / S].x;
            acc[t].y += acc[t + H / S].y;
            if (WEIGHTED) den[t] += den[t + H / S];
        }
    } else {                                                // partners H slots apart: every lane gets the sum
        acc[0].x += __shfl_xor(acc[0].x, H * CL, GRX_WAVE);
        acc[0].y += __shfl_xor(acc[0].y, H * CL, GRX_WAVE);
        if (WEIGHTED) den[0] += __shfl_xor(den[0], H * CL, GRX_WAVE);
    }
}

template <int S, int CL, bool WEIGHTED>
__global__ __launch_bounds__(NS_BLOCK) void ns_rows_kernel(const NsArgs A)
{
    constexpr int G = S * CL, RPG = NS_BLOCK / G;           // lanes per row, rows per workgroup pass
    constexpr int NA = NS_SLOTS / S;                        // virtual slots of a lane: slot, slot + S, ...
    constexpr int NT = NA >= NS_GATHERS ? 1 : NS_GATHERS / NA;   // trips per iteration
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int slot = lane / CL, part = lane % CL, k = 2 * part;
    const int64_t groups = (A.n + RPG - 1) / RPG;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t u = g * RPG + grp;
        int64_t b = 0, e = 0;
        if (u < A.n) { b = A.row_ptr[u]; e = A.row_ptr[u + 1]; }
        const int64_t d = e - b;
        const bool is_long = d > NS_LONG_ROW;
        NsPair acc[NA] = {};
        double den[NA] = {};
        if (!is_long)
            for (int64_t i = 0; i < d; i += NT * NS_SLOTS)
                ns_trips<NA, NT, WEIGHTED>(A, b, d, i + slot, S, NS_SLOTS, part, acc, den);
        // the tree over the virtual slots v = slot + t S: v += v + h for h = 4, 2, 1
        ns_level<4, S, CL, WEIGHTED>(acc, den);
        ns_level<2, S, CL, WEIGHTED>(acc, den);
        ns_level<1, S, CL, WEIGHTED>(acc, den);
        if (slot == 0 && u < A.n && !is_long) {
            const double dn = WEIGHTED ? den[0] : (double)d;
            if (k < A.r) A.out[(int64_t)k * A.ldo + u] = ns_value(acc[0].x, dn, A.mean);
            if (k + 1 < A.r) A.out[(int64_t)(k + 1) * A.ldo + u] = ns_value(acc[0].y, dn, A.mean);
        }
    }
}

// The long rows, a workgroup each.  Thread t of workgroup w looks at the rows w + gridDim.x (t + 256 i): neighbouring
// rows go to different workgroups, so the hubs of a degree-sorted graph -- its first rows -- do not queue up in one.
template <int CL, bool WEIGHTED>
__global__ __launch_bounds__(NS_BLOCK) void ns_long_rows_kernel(const NsArgs A)
{
    __shared__ double sm[NS_LONG_SLOTS * NS_LDR];
    __shared__ double sd[NS_LONG_SLOTS];
    __shared__ unsigned char found[NS_BLOCK];
    for (int64_t base = 0; base < A.n; base += (int64_t)gridDim.x * NS_BLOCK) {
        const int64_t u = base + (int64_t)threadIdx.x * gridDim.x + blockIdx.x;
        const bool is_long = u < A.n && A.row_ptr[u + 1] - A.row_ptr[u] > NS_LONG_ROW;
        found[threadIdx.x] = is_long;
        if (__syncthreads_or(is_long)) {                    // rare; the barrier also publishes found[]
            for (int t = 0; t < NS_BLOCK; ++t) {
                if (found[t]) {                             // uniform over the workgroup
                    const int64_t v = base + (int64_t)t * gridDim.x + blockIdx.x;
                    ns_long_row<CL, WEIGHTED>(A, v, A.row_ptr[v], A.row_ptr[v + 1], sm, sd);
                }
            }
        }
        __syncthreads();                                    // found[] is rewritten by the next pass
    }
}

template <int S, int CL>
void ns_launch(const NsArgs &A, hipStream_t st)
{
    if constexpr (S * CL <= GRX_WAVE) {                     // a row's lanes share a wavefront (the entry point checks)
        const unsigned grid = grx_grid(A.n, NS_BLOCK / (S * CL), NS_MAX_WG);
        const unsigned long_grid = grx_grid(A.n, NS_BLOCK, NS_LONG_MAX_WG);
        if (A.w) {
            ns_rows_kernel<S, CL, true><<<grid, NS_BLOCK, 0, st>>>(A);
            ns_long_rows_kernel<CL, true><<<long_grid, NS_BLOCK, 0, st>>>(A);
        } else {
            ns_rows_kernel<S, CL, false><<<grid, NS_BLOCK, 0, st>>>(A);
            ns_long_rows_kernel<CL, false><<<long_grid, NS_BLOCK, 0, st>>>(A);
        }
    }
}

template <int CL>
void ns_launch_slots(int slots, const NsArgs &A, hipStream_t st)
{
    switch (slots) {
    case 1: ns_launch<1, CL>(A, st); break;
    case 2: ns_launch<2, CL>(A, st); break;
    case 4: ns_launch<4, CL>(A, st); break;
    default: ns_launch<8, CL>(A, st); break;
    }
}

// lanes that share a membership row of r columns, two columns each: a power of two, 1 .. 16
int ns_column_lanes(int r)
{
    int cl = 1;
    while (2 * cl < r) cl *= 2;
    return cl;
}

}  // namespace

extern "C" int grx_neighbor_roles(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                                  const double *d_P, int64_t ldp, int r, int mode, int lanes_per_row, double *d_out,
                                  int64_t ld_out, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_neighbor_roles: n = %lld out of range [0, 2^31)", (long long)n);
    GRX_REQUIRE(r >= 1, "grx_neighbor_roles: r = %d", r);
    if (r > GRX_MAX_ROLES) {
        grx_set_error("grx_neighbor_roles: r = %d above GRX_MAX_ROLES = %d", r, GRX_MAX_ROLES);
        return GRX_ERR_UNSUPPORTED;
    }
    GRX_REQUIRE(mode == GRX_NEIGHBOR_SUM || mode == GRX_NEIGHBOR_MEAN, "grx_neighbor_roles: mode = %d", mode);
    const int cl = ns_column_lanes(r);
    const int slots = lanes_per_row == 0 ? (NS_DEFAULT_LANES / cl < NS_SLOTS ? NS_DEFAULT_LANES / cl : NS_SLOTS) : lanes_per_row > 0 && lanes_per_row % cl == 0 ? lanes_per_row / cl : 0;
    GRX_REQUIRE((slots == 1 || slots == 2 || slots == 4 || slots == 8) && slots * cl <= GRX_WAVE,
                "grx_neighbor_roles: lanes_per_row must be 0 or %d times 1, 2, 4 or 8 and at most %d for r = %d (got %d)",
                cl, GRX_WAVE, r, lanes_per_row);
    GRX_REQUIRE(ldp >= r, "grx_neighbor_roles: ldp = %lld < r = %d", (long long)ldp, r);
    GRX_REQUIRE(ld_out >= n, "grx_neighbor_roles: ld_out = %lld < n = %lld", (long long)ld_out, (long long)n);
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_P && d_out, "grx_neighbor_roles: null pointer");
    const NsArgs A{n, d_row_ptr, d_col, d_w, d_P, ldp, r, mode == GRX_NEIGHBOR_MEAN, d_out, ld_out};
    const hipStream_t st = grx_stream(stream);
    switch (cl) {
    case 1: ns_launch_slots<1>(slots, A, st); break;
    case 2: ns_launch_slots<2>(slots, A, st); break;
    case 4: ns_launch_slots<4>(slots, A, st); break;
    case 8: ns_launch_slots<8>(slots, A, st); break;
    default: ns_launch_slots<16>(slots, A, st); break;
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}
