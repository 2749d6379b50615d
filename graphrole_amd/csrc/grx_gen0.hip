// grx_gen0.hip -- generation-0 features on a CSR graph: weighted degree and the ego-net internal / external weights.
//
// Kernels (all HBM/L2-gather bound; no MFMA -- this is integer-indexed streaming work):
//   row_sums_kernel               weighted degree                                     networkx.py:48-63
//   general ego-net path (weighted or directed graphs)                                networkx.py:71-83,115-123
//     egonet_prepare_kernel       row slots; rows sorted by length into the three kernels below
//     egonet_group_kernel         eight lanes per node (at most 32, second instance: 64 out-neighbours)
//     egonet_big_kernel           a wavefront per node; a workgroup per part of a hub row
//     egonet_combine_kernel       the parts of a hub row, in order
//   triangle path (unweighted undirected graphs)
//     triangle_count_arcs_kernel  triangles per node over the oriented arcs
//     node_info_kernel            info[v] = degree without the self-loop, and whether v has one
//     egonet_from_triangles_kernel  internal / external edge counts from the triangle counts (hub rows: a workgroup each)
//   add_columns_kernel            out = a + b
//
// Determinism: the weighted sums are "per-lane sequential, then a fixed butterfly"; the triangle path counts integers.
#include "grx_common.h"

#include <cstdlib>

namespace {

// ---------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------
// position of key in the ascending slice col[b,e), or -1
__device__ __forceinline__ int64_t find_in_row(const int32_t *__restrict__ col, int64_t b,
                                               int64_t e, int32_t key)
{
    while (b < e) {
        int64_t mid = (b + e) >> 1;
        int32_t c = col[mid];
        if (c < key) b = mid + 1;
        else if (c > key) e = mid;
        else return mid;
    }
    return -1;
}

// first position in col[b,e) with col[pos] >= key
__device__ __forceinline__ int64_t lower_bound_row(const int32_t *__restrict__ col, int64_t b,
                                                   int64_t e, int32_t key)
{
    while (b < e) {
        int64_t mid = (b + e) >> 1;
        if (col[mid] < key) b = mid + 1;
        else e = mid;
    }
    return b;
}

__device__ __forceinline__ int ilog2_i64(int64_t x) { return 63 - __clzll((unsigned long long)(x | 1)); }

// ---------------------------------------------------------------------------------------
// weighted row sums
// ---------------------------------------------------------------------------------------
// G lanes per row, R rows per group in flight (rows v, v + ngroups, ...): the dependent row_ptr -> weights chain
// of one short row leaves the memory system idle, R independent chains keep it busy.  Per row the additions run
// in the same order whatever R is: lane-strided partial sums, then the butterfly.
template <int G, int R>
__global__ __launch_bounds__(256) void row_sums_kernel(const int64_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ col,
                                                       const double *__restrict__ w, int add_loop,
                                                       int64_t row_begin, int64_t row_end,
                                                       double *__restrict__ out)
{
    const int lane = threadIdx.x % G;
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
    for (int64_t v0 = row_begin + group; v0 < row_end; v0 += ngroups * R) {
        int64_t b[R], e[R];
        int64_t longest = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int64_t v = v0 + ngroups * i;
            const bool live = v < row_end;
            b[i] = live ? row_ptr[v] : 0;
            e[i] = live ? row_ptr[v + 1] : 0;
            longest = e[i] - b[i] > longest ? e[i] - b[i] : longest;
        }
        if (w == nullptr) {                                 // implicit weight 1: degree from row_ptr
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int64_t v = v0 + ngroups * i;
                    if (v < row_end)
                        out[v] = (double)((e[i] - b[i]) + ((add_loop && find_in_row(col, b[i], e[i], (int32_t)v) >= 0) ? 1 : 0));
                }
            }
            continue;
        }
        double s[R], loop[R];
#pragma unroll
        for (int i = 0; i < R; ++i) s[i] = loop[i] = 0.0;
        for (int64_t off = lane; off < longest; off += G) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int64_t k = b[i] + off;
                if (k < e[i]) {
                    const double x = w[k];
                    s[i] += x;
                    if (add_loop && col[k] == v0 + ngroups * i) loop[i] = x;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const double si = grx_group_sum<G>(s[i]);
            const double li = grx_group_sum<G>(loop[i]);
            const int64_t v = v0 + ngroups * i;
            if (lane == 0 && v < row_end) out[v] = si + li;
        }
    }
}

// ---------------------------------------------------------------------------------------
// ego-net features
// ---------------------------------------------------------------------------------------
// One node per TPN threads.  Each lane owns ego members m = lane, lane+TPN, ... and for member a
// picks the cheaper of
//   S1: walk row(a), test membership of each entry in ego(v)        cost deg(a) * log deg(v)
//   S2: walk ego(v), look each member up in row(a)                   cost deg(v) * log deg(a)
// S2 obtains the boundary weight of a as rowsum(a) - matched weight; when every entry of row(a)
// matched, the boundary contribution is exactly 0 (no cancellation residue).
// The same features for nodes with at most EGO_GROUP_MAX out-neighbours (almost every node of a
// sparse graph): EIGHT lanes per node instead of a wavefront.  The ego set sits in registers (three
// ids per lane); the members are visited one after the other and their rows are either scanned in
// coalesced chunks of eight arcs, membership by the all-pairs shuffle compare of the triangle
// kernel, or -- long rows, i.e. hub neighbours -- probed by binary search for the (at most 25) ego
// members.  Per lane sequential sums, fixed butterfly: bitwise reproducible.
constexpr int EGO_SLOTS = 4;                                     // ids per lane: nodes with at most 32 out-neighbours
constexpr int EGO_GROUP_MAX = 8 * EGO_SLOTS;
constexpr int EGO_SLOTS_WIDE = 8;                                // a second instance of the kernel: 33 .. 64 out-neighbours
constexpr int EGO_GROUP_MAX_WIDE = 8 * EGO_SLOTS_WIDE;

// Round 5.  What a member a of an ego set contributes needs the ids of row(a), where it begins (weights of matched
// arcs), its length and its weighted row sum.  Read from the CSR that is two row_ptr entries, rowsum[a] and an
// unaligned run of ids: 3 - 4 cache-line requests per (v, a) pair, and the REQUEST rate (~50 G/s beyond the caches,
// profiles/r04_gather_bw.json) is what bounds this kernel.  A streaming pre-pass therefore lays every row out as one
// aligned 128-byte SLOT -- row sum, begin | min(length, SAT) << 40, the first 28 ids (-1 padded) -- so that a pair
// costs ONE aligned request that eight lanes read with one 16-byte load each; rows longer than 28 ids continue in the CSR.
constexpr int EGO_DEG_SHIFT = 40;
constexpr unsigned long long EGO_BEGIN_MASK = (1ull << EGO_DEG_SHIFT) - 1;
constexpr unsigned EGO_DEG_SAT = (1u << 24) - 1;                 // longer rows: length from row_ptr
constexpr int EGO_SLOT_IDS = 28;
struct __align__(16) EgoSlot {
    double rs;
    unsigned long long bd;
    int32_t ids[EGO_SLOT_IDS];
};
static_assert(sizeof(EgoSlot) == 128, "one slot = one 128-byte line");

// slots of all n rows + the rows of [row_begin, row_end) beyond the 8-lane kernel's 32 neighbours, appended to lists by
// out-degree: 33 .. 64 (the wide instance of the group kernel), 65 .. hub - 1 (a wavefront per row), hub and more: a
// workgroup per PART of EGO_PART members (entries {row, part, parts}: a node with 10 000 neighbours is ten work items,
// not one workgroup that finishes long after the others).  The order of the lists does not matter: every row's result
// is computed independently of the others, the parts of a row are summed in part order by egonet_combine_kernel.
constexpr int EGO_PART = 1024;
__global__ __launch_bounds__(256) void egonet_prepare_kernel(
    int64_t n, const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ rowsum,
    int64_t row_begin, int64_t row_end, int64_t hub, EgoSlot *__restrict__ slots, int32_t *__restrict__ wide_rows,
    int32_t *__restrict__ mid_rows, int32_t *__restrict__ hub_parts, unsigned *__restrict__ counts)
{
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < ((n + 63) & ~(int64_t)63); v += (int64_t)gridDim.x * 256) {
        const int64_t d = v < n ? row_ptr[v + 1] - row_ptr[v] : 0;
        const bool owned = v >= row_begin && v < row_end;
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const bool take = owned && (which == 0 ? (d > EGO_GROUP_MAX && d <= EGO_GROUP_MAX_WIDE) : (d > EGO_GROUP_MAX_WIDE && d < hub));
            const unsigned long long bal = __ballot(take);
            if (bal) {
                const int lane = threadIdx.x & 63;
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(&counts[which], (unsigned)__popcll(bal));
                base = __shfl(base, 0, 64);
                if (take) (which == 0 ? wide_rows : mid_rows)[base + __popcll(bal & ((1ull << lane) - 1))] = (int32_t)v;
            }
        }
        if (owned && d >= hub) {
            const unsigned parts = (unsigned)((d + EGO_PART - 1) / EGO_PART);
            const unsigned base = atomicAdd(&counts[2], parts);
            for (unsigned p = 0; p < parts; ++p) {
                hub_parts[3 * (size_t)(base + p)] = (int32_t)v;
                hub_parts[3 * (size_t)(base + p) + 1] = (int32_t)p;
                hub_parts[3 * (size_t)(base + p) + 2] = (int32_t)parts;
            }
        }
    }
    // one thread per 4-byte word of a slot: 32 consecutive threads write one line
    uint32_t *words = reinterpret_cast<uint32_t *>(slots);
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n * 32; idx += (int64_t)gridDim.x * 256) {
        const int64_t r = idx >> 5;
        const int wi = (int)(idx & 31);
        const int64_t b = row_ptr[r];
        const int64_t d = row_ptr[r + 1] - b;
        uint32_t word;
        if (wi < 2) {
            const double rs = rowsum ? rowsum[r] : (double)d;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(rs);
            word = wi == 0 ? (uint32_t)bits : (uint32_t)(bits >> 32);
        } else if (wi < 4) {
            const unsigned long long bd =
                (unsigned long long)b | ((unsigned long long)(d < (int64_t)EGO_DEG_SAT ? d : (int64_t)EGO_DEG_SAT) << EGO_DEG_SHIFT);
            word = wi == 2 ? (uint32_t)bd : (uint32_t)(bd >> 32);
        } else {
            const int k = wi - 4;
            word = k < d ? (uint32_t)col[b + k] : 0xffffffffu;
        }
        words[idx] = word;
    }
}

// The membership filter of ego(v): a Bloom filter of EGO_FILTER_WORDS x 32 bits with TWO bits per member -- bit
// (id mod 4096) and bit ((id >> 12) mod 4096) -- in the group's LDS slice.  With at most 33 members a foreign id passes
// both probes with probability ~1e-4 (one probe: 0.8 %, which sent two thirds of all WAVEFRONT steps down the general
// path: a wavefront takes it when any of its eight groups does).  Graphs below 4096 nodes: the first probe is exact.
constexpr int EGO_FILTER_WORDS = 128;
__device__ __forceinline__ unsigned ego_filter_bit(const unsigned *flt, int32_t b)
{
    const unsigned u = (unsigned)b;
    const unsigned w1 = flt[(u >> 5) & (EGO_FILTER_WORDS - 1)] >> (u & 31u);
    const unsigned w2 = flt[(u >> 17) & (EGO_FILTER_WORDS - 1)] >> ((u >> 12) & 31u);
    return w1 & w2 & 1u;
}
__device__ __forceinline__ void ego_filter_set(unsigned *flt, int32_t b)
{
    const unsigned u = (unsigned)b;
    atomicOr(&flt[(u >> 5) & (EGO_FILTER_WORDS - 1)], 1u << (u & 31u));
    atomicOr(&flt[(u >> 17) & (EGO_FILTER_WORDS - 1)], 1u << ((u >> 12) & 31u));
}

// the byte of a wavefront ballot that belongs to this lane's group of eight (gshift = first lane of the group)
__device__ __forceinline__ unsigned ego_group_bits(unsigned long long ballot, int gshift)
{
    const unsigned half = (gshift & 32) ? (unsigned)(ballot >> 32) : (unsigned)ballot;
    return __builtin_amdgcn_ubfe(half, (unsigned)gshift & 31u, 8u);
}

// membership of the eight ids b (one per lane of the group, -1 = none) in ego(v) = {v} U {uu[0..3] of the group's
// lanes}: the filter decides whether the exact all-pairs shuffle compare has to run at all
template <int SLOTS>
__device__ __forceinline__ bool ego_chunk_inside(int32_t b, int32_t v, const int32_t (&uu)[SLOTS],
                                                 const unsigned *flt, int gshift, int lane)
{
    constexpr int G = 8;
    const bool live = b >= 0;
    const bool maybe = live && ego_filter_bit(flt, b);
    unsigned match = 0;
    if (ego_group_bits(__ballot(maybe), gshift)) {              // uniform over the group
#pragma unroll
        for (int sidx = 0; sidx < G; ++sidx) {
            const int32_t bs = __shfl(b, sidx, G);
            bool hit = false;
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) hit |= bs == uu[i];
            if (ego_group_bits(__ballot(hit), gshift)) match |= 1u << sidx;
        }
    }
    return live && (((match >> lane) & 1u) || b == v);
}

// Nodes with at most EGO_GROUP_MAX out-neighbours: eight lanes per node.  Per member a of ego(v) the group reads the
// slot of a with one 16-byte load per lane (lane 0: row sum, begin | length; lanes 1 - 7: four ids each) and tests
// the ids for membership; WEIGHTS are read for the MATCHED arcs only (the first version scanned ids + 8-byte weights
// of every member row from the CSR: 25-50x the compulsory traffic, profiles/r05_dw5m_pmc.json):
//     internal += w(a -> b)                       for b in ego(v)   (undirected: b >= a, every edge once)
//     external += rowsum(a)                       no arc of row(a) ends in ego(v)       -- no subtraction
//              += 0                               every arc does                         -- exactly 0
//              += rowsum(a) - matched weight      otherwise, unless that difference lost more than six bits to
//                                                 cancellation: then the unmatched weights are added one by one
// The members are taken BATCH at a time: the slots of a whole batch are requested before the first is looked at.
// FAST PATH (the kernel was bound by its VALU instruction stream -- 313 instructions per member, every SIMD 100 % busy,
// the memory system at 17 G requests/s, profiles/r05_egonet.txt): a member whose ids all miss the filter and whose
// row fits its slot contributes rowsum(a) to `external` and nothing else -- four filter probes per lane, one ballot,
// no header broadcast (lane 0 holds the row sum itself).  Everything else -- a filter hit, a row beyond 28 ids, a
// hub row -- takes the general path below.
// The external shares are added by lane 0 in member order, the rest are per-lane sequential sums and a fixed
// butterfly: bitwise reproducible, independent of the launch geometry.
template <int BATCH, int SLOTS, bool DIRECTED>
__global__ __launch_bounds__(256) void egonet_group_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const double *__restrict__ w, const EgoSlot *__restrict__ slots,
    int64_t row_begin, int64_t row_end, const int32_t *__restrict__ rows, const unsigned *__restrict__ n_rows,
    double *__restrict__ internal, double *__restrict__ external)
{
    constexpr bool directed = DIRECTED;      // two instances: the undirected one carries the weights of row(v) in LDS
    // rows == nullptr: the nodes of [row_begin, row_end) with at most 8 SLOTS neighbours; else: the listed nodes
    constexpr int EGO_SLOTS = SLOTS;
    constexpr int EGO_GROUP_MAX = 8 * SLOTS;
    constexpr int G = 8;
    __shared__ unsigned ego_filter[256 / G][EGO_FILTER_WORDS];
    __shared__ int32_t ego_id[256 / G][EGO_GROUP_MAX];
    extern __shared__ double ego_w[];      // undirected graphs only (dynamic: 0 bytes otherwise): the weights of row(v) = w(a -> v)
    const int lane = threadIdx.x % G;
    const int gshift = (threadIdx.x & 63) & ~(G - 1);
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
    unsigned *flt = ego_filter[threadIdx.x / G];
    int32_t *mid = ego_id[threadIdx.x / G];
    double *mw = ego_w + (threadIdx.x / G) * EGO_GROUP_MAX;
    const int4 *slot16 = reinterpret_cast<const int4 *>(slots);
    const int64_t first = rows ? 0 : row_begin, last = rows ? (int64_t)n_rows[0] : row_end;
    for (int64_t it = first + group; it < last; it += ngroups) {
        const int64_t v = rows ? (int64_t)rows[it] : it;
        const int64_t vb = row_ptr[v], ve = row_ptr[v + 1];
        const int dv = (int)(ve - vb);
        if (ve - vb > EGO_GROUP_MAX) continue;                  // uniform over the group
        int32_t uu[EGO_SLOTS];
#pragma unroll
        for (int i = 0; i < EGO_SLOTS; ++i) {
            const int64_t idx = vb + lane + (int64_t)G * i;
            uu[i] = (idx < ve) ? col[idx] : -2;
        }
        bool mine_v = false;
#pragma unroll
        for (int i = 0; i < EGO_SLOTS; ++i) mine_v |= uu[i] == (int32_t)v;
        const bool v_in_row = ego_group_bits(__ballot(mine_v), gshift) != 0u;
        __builtin_amdgcn_wave_barrier();                       // the previous node's readers are done
#pragma unroll
        for (int i = 0; i < EGO_SLOTS; ++i)
            if (uu[i] >= 0) mid[lane + G * i] = uu[i];
#pragma unroll
        for (int i = 0; i < EGO_FILTER_WORDS / (4 * G); ++i)
            reinterpret_cast<uint4 *>(flt)[lane + G * i] = make_uint4(0u, 0u, 0u, 0u);
        __builtin_amdgcn_wave_barrier();
        // UNDIRECTED graphs: every member's row holds the arc back to v (the CSR is symmetric), so v stays OUT of the
        // filter -- a member whose only arc into ego(v) is that one still takes the fast path below, with the arc's
        // weight from row(v) (w(a -> v) = w(v -> a), the same double); the exact test finds b == v without the filter
#pragma unroll
        for (int i = 0; i <= EGO_SLOTS; ++i) {
            const int32_t id = i < EGO_SLOTS ? uu[i < EGO_SLOTS ? i : 0] : ((lane == 0 && directed) ? (int32_t)v : -2);
            if (id >= 0 && (directed || id != (int32_t)v)) ego_filter_set(flt, id);
        }
        double ins = 0.0, ext = 0.0;
        // member v itself: every arc of row(v) ends in ego(v)
#pragma unroll
        for (int i = 0; i < EGO_SLOTS; ++i)
            if (uu[i] >= 0) {
                const double x = w ? w[vb + lane + (int64_t)G * i] : 1.0;
                if (!directed) mw[lane + G * i] = x;
                if (directed || uu[i] >= (int32_t)v) ins += x;
            }
        __builtin_amdgcn_wave_barrier();

        for (int mb = 0; mb < dv; mb += BATCH) {
            int4 q[BATCH];
#pragma unroll
            for (int k = 0; k < BATCH; ++k) {
                q[k] = make_int4(-1, -1, -1, -1);
                if (mb + k < dv) {
                    const int32_t a = mid[mb + k];
                    if (a != (int32_t)v) q[k] = slot16[(int64_t)a * G + lane];
                }
            }
#pragma unroll
            for (int k = 0; k < BATCH; ++k) {
                const int m = mb + k;
                if (m >= dv) break;
                const int32_t a = mid[m];
                if (a == (int32_t)v) continue;                  // a self-loop: row(v) is counted above
                {
                    // fast path: lanes 1 - 7 probe the filter with their four ids (a pad id -1 probes like any other: a hit
                    // only costs the general path); lane 0 contributes "the row does not fit its slot" (length in bits
                    // 8 .. 31 of its fourth word)
                    const unsigned hit = lane ? (ego_filter_bit(flt, q[k].x) | ego_filter_bit(flt, q[k].y) |
                                                 ego_filter_bit(flt, q[k].z) | ego_filter_bit(flt, q[k].w))
                                              : (unsigned)(((unsigned)q[k].w >> 8) > (unsigned)EGO_SLOT_IDS);
                    if (ego_group_bits(__ballot(hit != 0u), gshift) == 0u) {
                        const double rs0 = __longlong_as_double((long long)(((unsigned long long)(unsigned)q[k].y << 32) | (unsigned)q[k].x));
                        if (directed) {
                            if (lane == 0) ext += rs0;
                            continue;
                        }
                        // undirected: exactly one arc of row(a) ends in ego(v), the one back to v
                        const double wva = mw[m];
                        const double e = rs0 - wva;
                        const bool cancelled = lane == 0 && !(e * 64.0 >= rs0);
                        if (ego_group_bits(__ballot(cancelled), gshift) == 0u) {
                            if (lane == 0) {
                                ext += e;
                                if ((int32_t)v >= a) ins += wva;
                            }
                            continue;
                        }
                    }
                }
                // lane 0 of the group holds the header of the slot
                const unsigned rs_lo = (unsigned)__shfl(q[k].x, 0, G), rs_hi = (unsigned)__shfl(q[k].y, 0, G);
                const unsigned bd_lo = (unsigned)__shfl(q[k].z, 0, G), bd_hi = (unsigned)__shfl(q[k].w, 0, G);
                const double rs = __longlong_as_double((long long)(((unsigned long long)rs_hi << 32) | rs_lo));
                const unsigned long long bd = ((unsigned long long)bd_hi << 32) | bd_lo;
                const int64_t ab = (int64_t)(bd & EGO_BEGIN_MASK);
                int64_t da = (int64_t)(bd >> EGO_DEG_SHIFT);
                if (da == (int64_t)EGO_DEG_SAT) da = row_ptr[a + 1] - ab;
                if (da == 0) continue;
                const int64_t ae = ab + da;
                if (da <= (int64_t)EGO_SLOTS * G * (ilog2_i64(da) + 2)) {
                    int cnt = 0;
                    double msum = 0.0;
                    auto chunk = [&](int32_t b, int64_t j) {
                        const bool inside = ego_chunk_inside<SLOTS>(b, (int32_t)v, uu, flt, gshift, lane);
                        cnt += __popc(ego_group_bits(__ballot(inside), gshift));
                        if (inside) {
                            const double x = w ? w[j] : 1.0;
                            msum += x;
                            if (directed || b >= a) ins += x;
                        }
                    };
                    // ids 4 (lane - 1) .. 4 (lane - 1) + 3 of the row sit in this lane's quarter of the slot
                    const int64_t j4 = ab + 4 * (lane - 1);
                    chunk(lane ? q[k].x : -1, j4);
                    if (da > 1) chunk(lane ? q[k].y : -1, j4 + 1);
                    if (da > 2) chunk(lane ? q[k].z : -1, j4 + 2);
                    if (da > 3) chunk(lane ? q[k].w : -1, j4 + 3);
                    for (int64_t j0 = ab + EGO_SLOT_IDS; j0 < ae; j0 += G)
                        chunk(j0 + lane < ae ? col[j0 + lane] : -1, j0 + lane);
                    if (cnt == 0) {
                        if (lane == 0) ext += rs;
                    } else if (cnt != da) {
#pragma unroll
                        for (int off = 1; off < G; off <<= 1) msum += __shfl_xor(msum, off, G);
                        const double e = rs - msum;
                        if (e * 64.0 >= rs) {
                            if (lane == 0) ext += e;
                        } else {
                            // nearly closed row: the difference would carry the rounding of the two sums; add the arcs
                            // that leave the ego set one by one instead
                            for (int64_t j0 = ab; j0 < ae; j0 += G) {
                                const int32_t b = j0 + lane < ae ? col[j0 + lane] : -1;
                                const bool inside = ego_chunk_inside<SLOTS>(b, (int32_t)v, uu, flt, gshift, lane);
                                if (b >= 0 && !inside) ext += w ? w[j0 + lane] : 1.0;
                            }
                        }
                    }
                } else {
                    // long row (a hub): look the ego members up in it
                    int matched = 0;
                    double in_all = 0.0;
#pragma unroll
                    for (int i = 0; i <= EGO_SLOTS; ++i) {
                        int32_t key = -2;
                        if (i < EGO_SLOTS) key = uu[i < EGO_SLOTS ? i : 0];
                        else if (lane == 0 && !v_in_row) key = (int32_t)v;
                        if (key >= 0) {
                            const int64_t pos = lower_bound_row(col, ab, ae, key);
                            if (pos < ae && col[pos] == key) {
                                const double x = w ? w[pos] : 1.0;
                                ++matched;
                                in_all += x;
                                if (directed || key >= a) ins += x;
                            }
                        }
                    }
#pragma unroll
                    for (int off = 1; off < G; off <<= 1) {
                        matched += __shfl_xor(matched, off, G);
                        in_all += __shfl_xor(in_all, off, G);
                    }
                    if (lane == 0 && matched != da) ext += rs - in_all;
                }
            }
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            ins += __shfl_xor(ins, off, G);
            ext += __shfl_xor(ext, off, G);
        }
        if (lane == 0) { internal[v] = ins; external[v] = ext; }
    }
}

// Nodes with more than 64 out-neighbours (round 5; replaces the wavefront / workgroup kernels of rounds 1 - 4, which
// searched ego(v) in global memory for every arc of every member: 38 ms for the hubs of a weighted BA 1 M / 10 M graph).
// WAVES = 1: a wavefront per node (four nodes per workgroup), WAVES = 4: a 256-thread workgroup per node.
//   * ego(v) as a Bloom filter in LDS (two bits per member, 16+ bits of filter per member while it fits); an id that
//     passes both probes is confirmed by a binary search in row(v) itself (ascending ids);
//   * ONE LANE PER MEMBER a: the lane reads the member's slot (row sum, begin | length, first 28 ids) and tests the
//     ids one after the other -- a filter hit costs that lane a search, not the whole group (eight lanes per member
//     made every group wait for the group with a hit);
//   * members whose rows do not fit a slot are taken afterwards by the whole wavefront, 64 ids per step -- or, when the
//     member is the far bigger hub, by looking ego(v) up in row(a), as before;
//   * weights only for the arcs that end in ego(v); external = rowsum(a) - matched with the guards of the group kernel.
// Lane <-> member and lane <-> chunk position are functions of the row alone: bitwise reproducible.
// ... confirmed through a two-level search: every `stride`-th id of row(v) sits in LDS (samp[0 .. ns)), the binary search
// over the samples costs no memory round trip, the remaining `stride` ids are searched in row(v) itself -- fourteen
// dependent global loads per confirmed id (a hub's row) made the hub-to-hub pairs of a power-law graph the whole cost
struct EgoBigSet {
    const unsigned *flt;
    unsigned bit_mask;
    const int32_t *samp;
    int ns, stride;
    const int32_t *col;
    int64_t vb, ve;
    int32_t v;
};
__device__ __forceinline__ bool ego_big_member(const EgoBigSet &S, int32_t b)
{
    const unsigned h1 = (unsigned)b & S.bit_mask, h2 = (((unsigned)b * 0x9E3779B1u) >> 7) & S.bit_mask;
    if (!((S.flt[h1 >> 5] >> (h1 & 31u)) & (S.flt[h2 >> 5] >> (h2 & 31u)) & 1u)) return false;
    if (b == S.v) return true;
    int lo = 0, hi = S.ns;                                      // first sample > b
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (S.samp[mid] <= b) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return false;
    const int64_t begin = S.vb + (int64_t)(lo - 1) * S.stride;
    const int64_t end = begin + S.stride < S.ve ? begin + S.stride : S.ve;
    return find_in_row(S.col, begin, end, b) >= 0;
}

template <int WAVES>
__global__ __launch_bounds__(256) void egonet_big_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ w,
    const EgoSlot *__restrict__ slots, int directed, const int32_t *__restrict__ rows, const unsigned *__restrict__ n_rows,
    int filter_words, double *__restrict__ internal, double *__restrict__ external, double *__restrict__ part_out)
{
    // WAVES == 1: rows = node ids, results to internal / external.  WAVES == 4: rows = {node, part, parts} triples, the
    // members [part EGO_PART, (part + 1) EGO_PART) of the node, results to part_out[2 entry], [2 entry + 1]
    extern __shared__ unsigned ego_big_lds[];
    __shared__ double red[2][4];
    constexpr int T = 64 * WAVES;                               // lanes per node
    constexpr int NODES = 4 / WAVES;                            // nodes per workgroup
    const int wlane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tid = threadIdx.x % T;
    constexpr int SAMPLES = WAVES > 1 ? 1024 : 64;              // ids of row(v) kept in LDS for the two-level search
    unsigned *flt = ego_big_lds + (size_t)(threadIdx.x / T) * (filter_words + SAMPLES);
    int32_t *samp = reinterpret_cast<int32_t *>(flt + filter_words);
    const unsigned bit_mask = (unsigned)filter_words * 32u - 1u;
    const int4 *slot16 = reinterpret_cast<const int4 *>(slots);
    const int64_t count = (int64_t)n_rows[0];
    auto node_sync = [&] { if (WAVES > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier(); };
    for (int64_t it = (int64_t)blockIdx.x * NODES + threadIdx.x / T; it < count; it += (int64_t)gridDim.x * NODES) {
        const int32_t v = WAVES > 1 ? rows[3 * it] : rows[it];
        const int64_t vb = row_ptr[v], ve = row_ptr[v + 1], dv = ve - vb;
        const int64_t m_lo = WAVES > 1 ? (int64_t)rows[3 * it + 1] * EGO_PART : 0;
        const int64_t m_hi = WAVES > 1 ? (m_lo + EGO_PART < dv ? m_lo + EGO_PART : dv) : dv;
        node_sync();                                            // the previous node's readers are done
        for (int i = tid; i < filter_words; i += T) flt[i] = 0u;
        node_sync();
        for (int64_t m = tid; m <= dv; m += T) {
            const int32_t id = m < dv ? col[vb + m] : v;
            const unsigned h1 = (unsigned)id & bit_mask, h2 = (((unsigned)id * 0x9E3779B1u) >> 7) & bit_mask;
            atomicOr(&flt[h1 >> 5], 1u << (h1 & 31u));
            atomicOr(&flt[h2 >> 5], 1u << (h2 & 31u));
        }
        const int stride = (int)((dv + SAMPLES - 1) / SAMPLES) > 0 ? (int)((dv + SAMPLES - 1) / SAMPLES) : 1;
        const int ns = (int)((dv + stride - 1) / stride);
        for (int i = tid; i < ns; i += T) samp[i] = col[vb + (int64_t)i * stride];
        node_sync();
        const EgoBigSet S{flt, bit_mask, samp, ns, stride, col, vb, ve, v};
        double ins = 0.0, ext = 0.0;
        // member v itself: every arc of row(v) ends in ego(v)
        for (int64_t m = m_lo + tid; m < m_hi; m += T)
            if (directed || col[vb + m] >= v) ins += w ? w[vb + m] : 1.0;
        for (int64_t m0 = m_lo; m0 < m_hi; m0 += T) {
            const int64_t m = m0 + tid;
            int32_t a = m < m_hi ? col[vb + m] : -1;
            if (a == v) a = -1;                                 // a self-loop: counted above
            int64_t ab = 0, da = 0;
            double rs = 0.0;
            if (a >= 0) {
                const int4 h = slot16[(int64_t)a * 8];
                rs = __longlong_as_double((long long)(((unsigned long long)(unsigned)h.y << 32) | (unsigned)h.x));
                const unsigned long long bd = ((unsigned long long)(unsigned)h.w << 32) | (unsigned)h.z;
                ab = (int64_t)(bd & EGO_BEGIN_MASK);
                da = (int64_t)(bd >> EGO_DEG_SHIFT);
                if (da == (int64_t)EGO_DEG_SAT) da = row_ptr[a + 1] - ab;
                // the first id sits behind the header in the same quarter of the slot
            }
            const bool is_long = a >= 0 && da > EGO_SLOT_IDS;
            if (a >= 0 && !is_long && da > 0) {
                int cnt = 0;
                double msum = 0.0;
                for (int q = 0; q * 4 < da; ++q) {
                    const int4 ids = slot16[(int64_t)a * 8 + 1 + q];
                    const int32_t b4[4] = {ids.x, ids.y, ids.z, ids.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = q * 4 + j;
                        if (k < da && ego_big_member(S, b4[j])) {
                            const double x = w ? w[ab + k] : 1.0;
                            ++cnt;
                            msum += x;
                            if (directed || b4[j] >= a) ins += x;
                        }
                    }
                }
                if (cnt == 0) ext += rs;
                else if (cnt != da) {
                    const double e = rs - msum;
                    if (e * 64.0 >= rs) ext += e;
                    else {
                        // nearly closed row: add the arcs that leave the ego set one by one
                        for (int64_t k = 0; k < da; ++k) {
                            const int32_t b = col[ab + k];
                            if (!ego_big_member(S, b)) ext += w ? w[ab + k] : 1.0;
                        }
                    }
                }
            }
            // members whose rows do not fit a slot: the whole wavefront takes them one after the other
            unsigned long long todo = __ballot(is_long);
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int32_t a_s = __shfl(a, src, 64);
                const int64_t ab_s = __shfl(ab, src, 64), da_s = __shfl(da, src, 64);
                const double rs_s = __shfl(rs, src, 64);
                const int64_t members = dv + 1;
                if (da_s * (ilog2_i64(members) + 2) <= members * (int64_t)(ilog2_i64(da_s) + 2) * 4) {
                    // scan row(a), 64 ids per step
                    unsigned long long cnt = 0;
                    double msum = 0.0;
                    for (int64_t k0 = 0; k0 < da_s; k0 += 64) {
                        const int64_t k = k0 + wlane;
                        const int32_t b = k < da_s ? col[ab_s + k] : -1;
                        const bool inside = b >= 0 && ego_big_member(S, b);
                        cnt += (unsigned long long)__popcll(__ballot(inside));
                        if (inside) {
                            const double x = w ? w[ab_s + k] : 1.0;
                            msum += x;
                            if (directed || b >= a_s) ins += x;
                        }
                    }
                    if (cnt != 0 && (int64_t)cnt != da_s) {
                        msum = grx_group_sum<64>(msum);
                        const double e = rs_s - msum;
                        if (e * 64.0 >= rs_s) {
                            if (wlane == src) ext += e;
                        } else {
                            for (int64_t k0 = 0; k0 < da_s; k0 += 64) {
                                const int64_t k = k0 + wlane;
                                const int32_t b = k < da_s ? col[ab_s + k] : -1;
                                if (b >= 0 && !ego_big_member(S, b)) ext += w ? w[ab_s + k] : 1.0;
                            }
                        }
                    } else if (cnt == 0 && wlane == src) {
                        ext += rs_s;
                    }
                } else {
                    // a is by far the bigger hub: look the members of ego(v) up in row(a)
                    long long matched = 0;
                    double in_all = 0.0;
                    for (int64_t t0 = 0; t0 <= dv; t0 += 64) {
                        const int64_t t = t0 + wlane;
                        int32_t key = -1;
                        if (t < dv) key = col[vb + t];
                        else if (t == dv && find_in_row(col, vb, ve, v) < 0) key = v;      // v itself, once
                        if (key >= 0) {
                            const int64_t pos = find_in_row(col, ab_s, ab_s + da_s, key);
                            if (pos >= 0) {
                                const double x = w ? w[pos] : 1.0;
                                ++matched;
                                in_all += x;
                                if (directed || key >= a_s) ins += x;
                            }
                        }
                    }
                    matched = (long long)grx_group_sum<64>((double)matched);
                    in_all = grx_group_sum<64>(in_all);
                    if (wlane == src && matched != da_s) ext += rs_s - in_all;
                }
            }
        }
        ins = grx_group_sum<64>(ins);
        ext = grx_group_sum<64>(ext);
        if constexpr (WAVES > 1) {
            if (wlane == 0) { red[0][wave] = ins; red[1][wave] = ext; }
            __syncthreads();
            if (threadIdx.x == 0) {
                double si = 0.0, se = 0.0;
                for (int i = 0; i < WAVES; ++i) { si += red[0][i]; se += red[1][i]; }
                part_out[2 * it] = si;
                part_out[2 * it + 1] = se;
            }
        } else {
            if (wlane == 0) { internal[v] = ins; external[v] = ext; }
        }
    }
}

// the parts of a hub row, added in part order (the entries of a row are consecutive in the list)
__global__ __launch_bounds__(256) void egonet_combine_kernel(const int32_t *__restrict__ parts, const unsigned *__restrict__ n_parts,
                                                             const double *__restrict__ part_out, double *__restrict__ internal,
                                                             double *__restrict__ external)
{
    const int64_t count = (int64_t)n_parts[0];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.x * 256) {
        if (parts[3 * e + 1] != 0) continue;
        double si = 0.0, se = 0.0;
        for (int p = 0; p < parts[3 * e + 2]; ++p) { si += part_out[2 * (e + p)]; se += part_out[2 * (e + p) + 1]; }
        internal[parts[3 * e]] = si;
        external[parts[3 * e]] = se;
    }
}

// ---------------------------------------------------------------------------------------
// ego-net features of UNWEIGHTED UNDIRECTED graphs through per-node triangle counts
// ---------------------------------------------------------------------------------------
// With A' = adjacency without the diagonal, d'(v) its degrees, L(v) the self-loop flags and
// T(v) the number of triangles through v (= edges among the neighbours of v):
//     internal(v) = d'(v) + T(v) + sum_{a in ego(v)} L(a)
//     external(v) = sum_{a in ego(v)} d'(a) - 2 (d'(v) + T(v))
// (networkx.py:71-83 counted edge by edge; all quantities are integers, so this is exact.)
// T comes from the degree-oriented graph (arc u->v iff (d'(u),u) < (d'(v),v)): every triangle
// is found exactly once as a common out-neighbour of the two ends of its lowest arc; oriented
// lists are short even for power-law hubs.
// The ARCS are the work items (round 3).  Rounds 1-2 gave every source u an 8-lane group that walked its arcs: N+(u)
// in registers, a 256-bit membership filter, an all-pairs shuffle compare of 8-id chunks.  Its counters showed the
// instruction stream and the per-source dependency chain as the bound, not the memory system: the exact test (eight
// shuffles, each followed by three compares and a ballot) ran whenever ANY of the eight groups of a wavefront had a
// filter hit, i.e. nearly always (SQ_ACTIVE_INST_ANY 7x the aggregate kernel's for half its memory traffic), a
// wavefront waited for its longest source row, every source cost three dependent round trips, and only ~4 memory
// instructions were in flight per CU.  0.58 ms at BA 1 M / 10 M.  Steps from there (profiles/r03_triangles.txt):
//   N+(u) broadcast into registers, compares instead of shuffles                     0.47 ms
//   arcs as work items, all-pairs compare by DPP lane rotations, 8 lanes per arc      0.43 ms
//   16 lanes per arc, binary search across the lanes (ds_bpermute)                   0.44 ms
//   + a lane-per-arc pass that touches the lists first (64 random lines in flight)   0.52 ms  (rejected)
//   8-byte table entries read by one lane per arc and passed on by ds_bpermute        0.41 ms
//   the four searches of a group interleaved, unconditional loads (no exec juggling)  0.39 ms
// Now: a wavefront takes 64 consecutive arcs u->v; a 16-lane group handles four of them at a time, has the first
// sixteen ids of all eight lists in flight at once -- degree ordering keeps 99.5 % of the oriented lists of the
// BASELINE graphs that short -- and intersects by BINARY SEARCH: the lists are ascending, every lane looks its id of
// N+(v) up among the sixteen ids of N+(u) spread over the group's lanes (five ds_bpermute probes).  Two round trips
// per arc, no per-source loop, every group always has work; VALU 48 % busy, LDS 29 %, 22 G L2 misses/s.
constexpr int TRI_AG = 16;                   // lanes per arc
constexpr int TRI_ARCS = 4;                  // arcs per group and iteration
constexpr int32_t TRI_PAD = 0x7fffffff;      // pads N+(u) to sixteen ascending ids

// is y one of the sixteen ascending ids the group's lanes hold in a?  group_byte = 4 * (first lane of the group)
__device__ __forceinline__ bool tri_search16(int32_t y, int32_t a, int group_byte)
{
    int pos = group_byte;                                       // byte address of lane `lower bound so far`
    int32_t t = __builtin_amdgcn_ds_bpermute(pos + 7 * 4, a);
    pos += (t < y) ? 8 * 4 : 0;
    t = __builtin_amdgcn_ds_bpermute(pos + 3 * 4, a);
    pos += (t < y) ? 4 * 4 : 0;
    t = __builtin_amdgcn_ds_bpermute(pos + 1 * 4, a);
    pos += (t < y) ? 2 * 4 : 0;
    t = __builtin_amdgcn_ds_bpermute(pos, a);
    pos += (t < y) ? 4 : 0;
    t = __builtin_amdgcn_ds_bpermute(pos, a);
    return t == y;
}

__device__ __forceinline__ unsigned long long tri_bperm64(unsigned long long x, int src_byte)
{
    const int lo = __builtin_amdgcn_ds_bpermute(src_byte, (int)(unsigned)x);
    const int hi = __builtin_amdgcn_ds_bpermute(src_byte, (int)(unsigned)(x >> 32));
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// o_arc[k] for the k-th oriented arc u->v (grx.h): begin of N+(v) | |N+(v)| << 32 | |N+(u)| << 42 | (k - begin of
// N+(u)) << 52, the three 10-bit fields saturating at 1023 -- such arcs (hubs of the ORIENTED graph: out-degree is at
// most sqrt(2 m)) are looked up from o_row_ptr instead.
constexpr int TRI_FIELD = 10;
constexpr unsigned TRI_SAT = (1u << TRI_FIELD) - 1;

// A wavefront takes 64 consecutive arcs per iteration: one LANE per arc reads the 8-byte table entry (a coalesced
// 512-byte read), then one 16-lane GROUP per arc, four arcs at a time, receives the entries from the lanes that read
// them, loads the lists and intersects them by the binary search above.
// The counters of the first TRI_HUBS vertices (rows are in degree-descending order: the hubs) are kept per workgroup in
// LDS and added to T once at the end.  Every corner of every triangle is one atomic increment, and on a power-law graph
// a few vertices take most of them (BA 1 M / 10 M: 12 275 of 180 k on vertex 0, 35 k on the first sixteen); atomics to
// ONE address are served one after the other (~9 ns each): 0.15 of the kernel's 0.41 ms was that queue (measured by
// dropping the atomics below an index: 0.41 -> 0.30 without vertex 0, 0.25 without the first sixteen).  With the LDS
// counters 0.27 ms; workgroups of 512 / 1024 threads, which collect more per flush, were slower (0.28 / 0.30).
constexpr int TRI_HUBS = 256;
constexpr int TRI_THREADS = 256;

__device__ __forceinline__ void tri_add(unsigned long long *__restrict__ T, unsigned long long *s_hub, int32_t idx, unsigned c)
{
    if (idx < TRI_HUBS) atomicAdd(&s_hub[idx], (unsigned long long)c);
    else atomicAdd(&T[idx], (unsigned long long)c);
}

__global__ __launch_bounds__(TRI_THREADS) void triangle_count_arcs_kernel(
    const int64_t *__restrict__ o_row_ptr, const int32_t *__restrict__ o_col,
    const unsigned long long *__restrict__ o_arc, int64_t row_begin, int64_t row_end,
    unsigned long long *__restrict__ T)
{
    __shared__ unsigned long long s_hub[TRI_HUBS];
    for (int i = threadIdx.x; i < TRI_HUBS; i += blockDim.x) s_hub[i] = 0;
    __syncthreads();
    constexpr int G = TRI_AG;
    constexpr unsigned long long GMASK = (1ull << G) - 1;
    const int wlane = threadIdx.x & 63;
    const int lane = wlane % G;
    const int gshift = wlane & ~(G - 1);                       // first lane of this group in the wavefront
    const int group_byte = gshift * 4;
    const int g = wlane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t kb = o_row_ptr[row_begin], ke = o_row_ptr[row_end];
    for (int64_t base = kb + wave * 64; base < ke; base += nwaves * 64) {
        const int64_t k_mine = base + wlane;
        unsigned long long d_mine = (k_mine < ke) ? o_arc[k_mine] : 0ull;
        // ---- arcs with a saturated field (rare): the whole wavefront serves them one by one from o_row_ptr
        {
            const unsigned vl = (unsigned)(d_mine >> 32) & TRI_SAT, ul = (unsigned)(d_mine >> 42) & TRI_SAT,
                           ps = (unsigned)(d_mine >> 52) & TRI_SAT;
            unsigned long long todo = __ballot(vl == TRI_SAT || ul == TRI_SAT || ps == TRI_SAT);
            if (vl == TRI_SAT || ul == TRI_SAT || ps == TRI_SAT) d_mine = 0ull;      // not for the group phase
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int64_t k = base + src;
                const int32_t v = o_col[k];
                int64_t lo = row_begin, hi = row_end;           // u: last row with o_row_ptr[row] <= k
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (o_row_ptr[mid] <= k) lo = mid; else hi = mid;
                }
                const int64_t ub = o_row_ptr[lo], ue = o_row_ptr[lo + 1], vb = o_row_ptr[v], ve = o_row_ptr[v + 1];
                unsigned long long c = 0;
                for (int64_t j0 = vb; j0 < ve; j0 += 64) {      // every id of N+(v): binary search in N+(u)
                    const bool have = j0 + wlane < ve;
                    const int32_t y = have ? o_col[j0 + wlane] : -1;
                    int64_t a = ub, e = ue;
                    while (have && a < e) {
                        const int64_t mid = (a + e) >> 1;
                        if (o_col[mid] < y) a = mid + 1; else e = mid;
                    }
                    const bool hit = have && a < ue && o_col[a] == y;
                    if (hit) tri_add(T, s_hub, y, 1u);
                    c += (unsigned long long)__popcll(__ballot(hit));
                }
                if (c && wlane == 0) { tri_add(T, s_hub, v, (unsigned)c); tri_add(T, s_hub, (int32_t)lo, (unsigned)c); }
            }
        }
        // ---- the group phase
#pragma unroll 1
        for (int sub = 0; sub < 64 / ((64 / G) * TRI_ARCS); ++sub) {
            uint32_t vb[TRI_ARCS], ub[TRI_ARCS];
            int vlen[TRI_ARCS], ulen[TRI_ARCS];
#pragma unroll
            for (int j = 0; j < TRI_ARCS; ++j) {
                const int src = sub * 16 + g * TRI_ARCS + j;    // the lane that holds this arc's entry
                const unsigned long long d = tri_bperm64(d_mine, src * 4);
                vb[j] = (uint32_t)d;
                vlen[j] = (int)((unsigned)(d >> 32) & TRI_SAT);
                ulen[j] = (int)((unsigned)(d >> 42) & TRI_SAT);
                ub[j] = (uint32_t)(base + src) - ((unsigned)(d >> 52) & TRI_SAT);
                if (vlen[j] == 0) ulen[j] = 0;                 // nothing to intersect with: do not fetch N+(u) either
                if (ulen[j] == 0) ub[j] = 0;                   // (no arc here: keep the unconditional loads in bounds)
            }
            // eight independent loads per lane (unconditional -- lanes beyond a list read its first id and discard it:
            // a branch around every load cost more than the redundant reads)
            int32_t y0[TRI_ARCS], a0[TRI_ARCS];
#pragma unroll
            for (int j = 0; j < TRI_ARCS; ++j) {
                const bool yv = lane < vlen[j] && ulen[j] > 0, av = lane < ulen[j];
                const int32_t yr = o_col[vb[j] + (yv ? lane : 0)];
                const int32_t ar = o_col[ub[j] + (av ? lane : 0)];
                y0[j] = yv ? yr : -1;
                a0[j] = av ? ar : TRI_PAD;
            }
            // the four binary searches step by step TOGETHER: four independent ds_bpermute in flight per step (one
            // search after the other was twenty serial LDS round trips per group of arcs)
            bool h[TRI_ARCS];
            {
                int pos[TRI_ARCS];
                int32_t t[TRI_ARCS];
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) t[j] = __builtin_amdgcn_ds_bpermute(group_byte + 7 * 4, a0[j]);
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) pos[j] = group_byte + ((t[j] < y0[j]) ? 8 * 4 : 0);
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) t[j] = __builtin_amdgcn_ds_bpermute(pos[j] + 3 * 4, a0[j]);
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) pos[j] += (t[j] < y0[j]) ? 4 * 4 : 0;
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) t[j] = __builtin_amdgcn_ds_bpermute(pos[j] + 1 * 4, a0[j]);
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) pos[j] += (t[j] < y0[j]) ? 2 * 4 : 0;
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) t[j] = __builtin_amdgcn_ds_bpermute(pos[j], a0[j]);
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) pos[j] += (t[j] < y0[j]) ? 4 : 0;
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) t[j] = __builtin_amdgcn_ds_bpermute(pos[j], a0[j]);
#pragma unroll
                for (int j = 0; j < TRI_ARCS; ++j) h[j] = t[j] == y0[j];
            }
            bool longer = false;
#pragma unroll
            for (int j = 0; j < TRI_ARCS; ++j) longer |= (ulen[j] > G || vlen[j] > G) && ulen[j] > 0;
            if (__ballot(h[0] | h[1] | h[2] | h[3] | longer) == 0) continue;     // the usual case: no triangle here
#pragma unroll
            for (int j = 0; j < TRI_ARCS; ++j) {
                unsigned c_arc = 0;
                const unsigned long long b0 = __ballot(h[j]);
                if (b0) {
                    if (h[j]) tri_add(T, s_hub, y0[j], 1u);
                    c_arc = (unsigned)__popcll((b0 >> gshift) & GMASK);
                }
                if (__ballot((ulen[j] > G || vlen[j] > G) && ulen[j] > 0) != 0) {
                    // lists beyond sixteen ids: the remaining chunk pairs, from memory (degree ordering keeps them rare)
                    for (int ja = 0; __ballot(ja < ulen[j]) != 0; ja += G) {
                        const int32_t a = (ja + lane < ulen[j]) ? o_col[ub[j] + ja + lane] : TRI_PAD;
                        for (int jb = (ja == 0) ? G : 0; __ballot(jb < vlen[j] && ja < ulen[j]) != 0; jb += G) {
                            const int32_t y = (jb + lane < vlen[j] && ja < ulen[j]) ? o_col[vb[j] + jb + lane] : -1;
                            const bool hh = tri_search16(y, a, group_byte);
                            const unsigned long long bh = __ballot(hh);
                            if (bh) {
                                if (hh) tri_add(T, s_hub, y, 1u);
                                c_arc += (unsigned)__popcll((bh >> gshift) & GMASK);
                            }
                        }
                    }
                }
                if (__ballot(c_arc != 0) != 0) {
                    if (c_arc && lane == 0) {
                        // the arc's two ends: the target from the column array, the source = the row that owns position k
                        const int64_t k = base + sub * 16 + g * TRI_ARCS + j;
                        const int32_t v = o_col[k];
                        int64_t lo = row_begin, hi = row_end;   // last row with o_row_ptr[row] <= k
                        while (hi - lo > 1) {
                            const int64_t mid = (lo + hi) >> 1;
                            if (o_row_ptr[mid] <= k) lo = mid; else hi = mid;
                        }
                        tri_add(T, s_hub, v, c_arc);
                        tri_add(T, s_hub, (int32_t)lo, c_arc);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TRI_HUBS; i += blockDim.x)
        if (s_hub[i]) atomicAdd(&T[i], s_hub[i]);
}

// info[v] = (d'(v) << 1) | L(v)   (int32: the whole table is 4 B/node and stays L2-resident)
__global__ __launch_bounds__(256) void node_info_kernel(int64_t n, const int64_t *__restrict__ row_ptr,
                                                        const int32_t *__restrict__ col,
                                                        int32_t *__restrict__ info)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        const int64_t loop = find_in_row(col, b, e, (int32_t)v) >= 0 ? 1 : 0;
        info[v] = (int32_t)((((e - b) - loop) << 1) | loop);
    }
}

__device__ __forceinline__ void egonet_finish_row(int64_t v, long long sum_d, long long loops,
                                                  const int32_t *__restrict__ info,
                                                  const unsigned long long *__restrict__ T,
                                                  double *__restrict__ internal, double *__restrict__ external)
{
    const int32_t iv = info[v];
    const long long dv = iv >> 1;
    const long long core = dv + (long long)T[v];
    internal[v] = (double)(core + loops + (iv & 1));
    external[v] = (double)(sum_d + dv - 2 * core);
}

// G = 8 lanes per row; rows with more than hub_deg neighbours are left to the workgroup-per-row
// variant below (integer sums: any order is exact).
__device__ __forceinline__ void egonet_rows_body(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ info, const unsigned long long *__restrict__ T, int64_t row_begin,
    int64_t row_end, int64_t hub_deg, double *__restrict__ internal, double *__restrict__ external, int64_t block,
    int64_t nblocks)
{
    constexpr int G = 8;
    const int lane = threadIdx.x % G;
    const int64_t group = (block * blockDim.x + threadIdx.x) / G;
    const int64_t ngroups = nblocks * blockDim.x / G;
    for (int64_t v = row_begin + group; v < row_end; v += ngroups) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        if (e - b > hub_deg) continue;
        long long sum_d = 0, loops = 0;
        for (int64_t k = b + lane; k < e; k += G) {
            const int32_t a = col[k];
            if (a != (int32_t)v) {
                const int32_t ia = info[a];
                sum_d += ia >> 1;
                loops += ia & 1;
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            sum_d += __shfl_xor(sum_d, off, G);
            loops += __shfl_xor(loops, off, G);
        }
        if (lane == 0) egonet_finish_row(v, sum_d, loops, info, T, internal, external);
    }
}

__device__ __forceinline__ void egonet_hubs_body(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ info, const unsigned long long *__restrict__ T, int64_t row_begin,
    int64_t row_end, const int32_t *__restrict__ hub_rows, int64_t n_hubs,
    double *__restrict__ internal, double *__restrict__ external, int64_t block, int64_t nblocks)
{
    __shared__ long long red[2][4];
    for (int64_t h = block; h < n_hubs; h += nblocks) {
        const int64_t v = hub_rows[h];
        if (v < row_begin || v >= row_end) continue;
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        long long sum_d = 0, loops = 0;
        for (int64_t k = b + threadIdx.x; k < e; k += 256) {
            const int32_t a = col[k];
            if (a != (int32_t)v) {
                const int32_t ia = info[a];
                sum_d += ia >> 1;
                loops += ia & 1;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum_d += __shfl_xor(sum_d, off, 64);
            loops += __shfl_xor(loops, off, 64);
        }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sum_d; red[1][threadIdx.x >> 6] = loops; }
        __syncthreads();
        if (threadIdx.x == 0)
            egonet_finish_row(v, red[0][0] + red[0][1] + red[0][2] + red[0][3],
                              red[1][0] + red[1][1] + red[1][2] + red[1][3], info, T, internal, external);
        __syncthreads();
    }
}

// ONE launch for both: the first hub_blocks workgroups take the hub rows (a workgroup per row: a chain of dependent
// loads 40 deep for a 10 k-neighbour hub), the others the eight-lanes-per-row pass.  As two launches the hub kernel ran
// alone on a few CUs AFTER the row pass (0.04 ms of a 0.155 ms phase at BA 1 M / 10 M); now the chains start first and
// hide behind the row pass.
__global__ __launch_bounds__(256) void egonet_from_triangles_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ info, const unsigned long long *__restrict__ T, int64_t row_begin,
    int64_t row_end, int64_t hub_deg, const int32_t *__restrict__ hub_rows, int64_t n_hubs, int hub_blocks,
    double *__restrict__ internal, double *__restrict__ external)
{
    if ((int)blockIdx.x < hub_blocks)
        egonet_hubs_body(row_ptr, col, info, T, row_begin, row_end, hub_rows, n_hubs, internal, external, blockIdx.x, hub_blocks);
    else
        egonet_rows_body(row_ptr, col, info, T, row_begin, row_end, hub_deg, internal, external,
                         (int64_t)blockIdx.x - hub_blocks, (int64_t)gridDim.x - hub_blocks);
}

__global__ __launch_bounds__(256) void add_columns_kernel(int64_t n, const double *__restrict__ a,
                                                          const double *__restrict__ b,
                                                          double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = a[i] + b[i];
}

}  // namespace

extern "C" {

int grx_row_sums(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                 int add_self_loop, int64_t row_begin, int64_t row_end, double *d_out, void *stream)
{
    GRX_REQUIRE(n >= 0 && row_begin >= 0 && row_begin <= row_end && row_end <= n,
                "grx_row_sums: bad row range [%lld,%lld) for n=%lld", (long long)row_begin,
                (long long)row_end, (long long)n);
    if (row_end == row_begin) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_out, "grx_row_sums: NULL pointer");
    const unsigned grid = grx_grid((row_end - row_begin) * 8, 256, GRX_NUM_CU * 16);
    { GRX_PROF(GRX_K_ROW_SUMS, grx_stream(stream));
    row_sums_kernel<8, 4><<<grid, 256, 0, grx_stream(stream)>>>(d_row_ptr, d_col, d_w, add_self_loop,
                                                            row_begin, row_end, d_out);
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_add_columns(int64_t n, const double *d_a, const double *d_b, double *d_out, void *stream)
{
    GRX_REQUIRE(n >= 0, "grx_add_columns: n < 0");
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_a && d_b && d_out, "grx_add_columns: NULL pointer");
    { GRX_PROF(GRX_K_ADD_COLUMNS, grx_stream(stream));
    add_columns_kernel<<<grx_grid(n, 256 * 4, 2048), 256, 0, grx_stream(stream)>>>(n, d_a, d_b, d_out);
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

static size_t ego_parts_cap(int64_t nnz) { return (size_t)(nnz > 0 ? nnz : 0) / 512 + (size_t)(nnz > 0 ? nnz : 0) / EGO_PART + 64; }

size_t grx_egonet_workspace_bytes(int64_t n, int64_t nnz)
{
    const size_t rows = (size_t)((n > 0 ? n : 0) + 64);
    return rows * sizeof(EgoSlot) + 2 * rows * sizeof(int32_t) + 256 + ego_parts_cap(nnz) * (3 * sizeof(int32_t) + 2 * sizeof(double)) + 64;
}

int grx_egonet_features(int64_t n, int64_t nnz, const int64_t *d_row_ptr, const int32_t *d_col,
                        const double *d_w, const double *d_rowsum, int directed,
                        int64_t row_begin, int64_t row_end, double *d_internal,
                        double *d_external, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && row_begin >= 0 && row_begin <= row_end && row_end <= n,
                "grx_egonet_features: bad row range");
    if (row_end == row_begin) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_internal && d_external, "grx_egonet_features: NULL pointer");
    GRX_REQUIRE(d_w == nullptr || d_rowsum != nullptr,
                "grx_egonet_features: weighted graphs need d_rowsum (grx_row_sums, add_self_loop=0)");
    GRX_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << EGO_DEG_SHIFT), "grx_egonet_features: nnz must be in [0, 2^40) (a slot keeps a row's begin in 40 bits)");
    GRX_REQUIRE(d_workspace != nullptr && workspace_bytes >= grx_egonet_workspace_bytes(n, nnz),
                "grx_egonet_features: workspace too small (grx_egonet_workspace_bytes)");
    GRX_REQUIRE(n < ((int64_t)1 << 31), "grx_egonet_features: more than 2^31 - 1 nodes");
    hipStream_t st = grx_stream(stream);
    const int64_t nrows = row_end - row_begin;
    constexpr int64_t HUB = 512;             // out-degree from which a row goes to the workgroup kernel (egonet_big_kernel, 256 threads, split into parts)
    // workspace: row slots | counters (256 bytes) | rows of the wide group kernel, the wavefront and the workgroup kernel
    const size_t rows_cap = (size_t)(n + 64);
    EgoSlot *slots = reinterpret_cast<EgoSlot *>(d_workspace);
    unsigned *counts = reinterpret_cast<unsigned *>(slots + rows_cap);
    int32_t *wide_rows = reinterpret_cast<int32_t *>(counts + 64);
    int32_t *mid_rows = wide_rows + rows_cap;
    double *part_out = reinterpret_cast<double *>(reinterpret_cast<char *>(mid_rows + rows_cap) + ((16 - (((size_t)(mid_rows + rows_cap)) & 15)) & 15));
    int32_t *hub_parts = reinterpret_cast<int32_t *>(part_out + 2 * ego_parts_cap(nnz));
    GRX_CHECK_HIP(hipMemsetAsync(counts, 0, 256, st));
    {
        GRX_PROF(GRX_K_EGONET_WAVE, st);
        // (one word per thread, no grid-stride cap: the row_ptr -> col chain of a thread is two dependent round trips)
        egonet_prepare_kernel<<<grx_grid(n * 32, 256, (int64_t)1 << 30), 256, 0, st>>>(
            n, d_row_ptr, d_col, d_w ? d_rowsum : nullptr, row_begin, row_end, HUB, slots, wide_rows, mid_rows, hub_parts, counts);
        GRX_LAUNCH_CHECK();
        // nodes with at most EGO_GROUP_MAX neighbours: eight lanes each; the rest: a wavefront each
        const unsigned ggrid = grx_grid(nrows * 8, 256, GRX_NUM_CU * 32);
        const unsigned wgrid = grx_grid(nrows * 8, 256 * 16, GRX_NUM_CU * 8);   // a few per cent of the rows at most
        if (directed) {
            egonet_group_kernel<2, EGO_SLOTS, true><<<ggrid, 256, 0, st>>>(d_row_ptr, d_col, d_w, slots, row_begin, row_end, nullptr,
                                                                           nullptr, d_internal, d_external);
            GRX_LAUNCH_CHECK();
            egonet_group_kernel<2, EGO_SLOTS_WIDE, true><<<wgrid, 256, 0, st>>>(d_row_ptr, d_col, d_w, slots, row_begin, row_end,
                                                                                wide_rows, counts + 0, d_internal, d_external);
        } else {
            egonet_group_kernel<2, EGO_SLOTS, false><<<ggrid, 256, (size_t)(256 / 8) * EGO_GROUP_MAX * sizeof(double), st>>>(
                d_row_ptr, d_col, d_w, slots, row_begin, row_end, nullptr, nullptr, d_internal, d_external);
            GRX_LAUNCH_CHECK();
            egonet_group_kernel<2, EGO_SLOTS_WIDE, false><<<wgrid, 256, (size_t)(256 / 8) * EGO_GROUP_MAX_WIDE * sizeof(double), st>>>(
                d_row_ptr, d_col, d_w, slots, row_begin, row_end, wide_rows, counts + 0, d_internal, d_external);
        }
        GRX_LAUNCH_CHECK();
        // 65 .. HUB - 1 neighbours: a wavefront per node, 32 K filter bits each (>= 64 per member)
        const unsigned grid = grx_grid(nrows, 4 * 16, GRX_NUM_CU * 16);
        egonet_big_kernel<1><<<grid, 256, 4 * (1024 + 64) * sizeof(unsigned), st>>>(d_row_ptr, d_col, d_w, slots, directed, mid_rows,
                                                                             counts + 1, 1024, d_internal, d_external, nullptr);
        GRX_LAUNCH_CHECK();
    }
    {
        // HUB and more: a workgroup per part of 1024 members, 256 K filter bits (16 per member up to 16 K neighbours; beyond
        // that more ids pass the filter and are turned away by the search in row(v)); then the parts of a row in order
        const unsigned grid = grx_grid(nrows, 16, GRX_NUM_CU * 8);
        GRX_PROF(GRX_K_EGONET_BLOCK, st);
        egonet_big_kernel<4><<<grid, 256, (8192 + 1024) * sizeof(unsigned), st>>>(d_row_ptr, d_col, d_w, slots, directed, hub_parts,
                                                                         counts + 2, 8192, d_internal, d_external, part_out);
        GRX_LAUNCH_CHECK();
        egonet_combine_kernel<<<64, 256, 0, st>>>(hub_parts, counts + 2, part_out, d_internal, d_external);
        GRX_LAUNCH_CHECK();
    }
    return GRX_OK;
}

int grx_triangle_counts(int64_t n, const int64_t *d_o_row_ptr, const int32_t *d_o_col, const uint64_t *d_o_arc,
                        int64_t row_begin, int64_t row_end, uint64_t *d_T, void *stream)
{
    GRX_REQUIRE(n >= 0 && row_begin >= 0 && row_begin <= row_end && row_end <= n, "grx_triangle_counts: bad row range");
    if (row_end == row_begin) return GRX_OK;
    GRX_REQUIRE(d_o_row_ptr && d_o_col && d_o_arc && d_T, "grx_triangle_counts: NULL pointer");
    static const int rounds = [] { const char *e = std::getenv("GRX_TRI_ROUNDS"); return e ? atoi(e) : 4; }();
    const int64_t cap = (int64_t)GRX_NUM_CU * (2048 / TRI_THREADS) * rounds;   // workgroups that fill the chip, times rounds
    const unsigned grid = grx_grid((row_end - row_begin) * 8, TRI_THREADS, cap);   // ~64 arcs per wavefront and sweep at 8 arcs per row
    { GRX_PROF(GRX_K_TRIANGLES, grx_stream(stream));
    triangle_count_arcs_kernel<<<grid, TRI_THREADS, 0, grx_stream(stream)>>>(
        d_o_row_ptr, d_o_col, reinterpret_cast<const unsigned long long *>(d_o_arc), row_begin, row_end,
        reinterpret_cast<unsigned long long *>(d_T));
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_egonet_unweighted(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const uint64_t *d_T,
                          int64_t row_begin, int64_t row_end, double *d_internal, double *d_external,
                          int32_t *d_scratch, const int32_t *d_hub_rows, int64_t n_hub_rows, int64_t hub_degree,
                          void *stream)
{
    GRX_REQUIRE(n >= 0 && row_begin >= 0 && row_begin <= row_end && row_end <= n, "grx_egonet_unweighted: bad row range");
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_T && d_internal && d_external && d_scratch, "grx_egonet_unweighted: NULL pointer");
    hipStream_t st = grx_stream(stream);
    {
        GRX_PROF(GRX_K_EGONET_FINISH, st);
        node_info_kernel<<<grx_grid(n, 256, GRX_NUM_CU * 16), 256, 0, st>>>(n, d_row_ptr, d_col, d_scratch);
    }
    GRX_LAUNCH_CHECK();
    if (row_end > row_begin) {
        GRX_PROF(GRX_K_EGONET_FINISH, st);
        const int64_t hub_deg = (d_hub_rows && n_hub_rows > 0) ? hub_degree : ((int64_t)1 << 62);
        const bool hubs = d_hub_rows && n_hub_rows > 0;
        const int hub_blocks = hubs ? (int)grx_grid(n_hub_rows, 1, GRX_NUM_CU * 8) : 0;
        const int row_blocks = (int)grx_grid((row_end - row_begin) * 8, 256, GRX_NUM_CU * 32);
        egonet_from_triangles_kernel<<<hub_blocks + row_blocks, 256, 0, st>>>(
            d_row_ptr, d_col, d_scratch, reinterpret_cast<const unsigned long long *>(d_T), row_begin, row_end,
            hub_deg, d_hub_rows, hubs ? n_hub_rows : 0, hub_blocks, d_internal, d_external);
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

}  // extern "C"
