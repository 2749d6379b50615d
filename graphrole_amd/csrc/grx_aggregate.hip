// grx_aggregate.hip -- the ReFeX neighbour aggregation on a CSR graph               features/extract.py:98-119
//
// Kernels (all HBM/L2-gather bound; no MFMA -- this is integer-indexed streaming work):
//   gather sources
//     pack_rows_kernel / pack_rows8_kernel / pack_rows_tiled_kernel   column-major fp64 -> row-major rows of ldr doubles
//     pack_rows_i32_kernel          integer columns -> int32 rows
//     column_bits_kernel            bits each integer column needs
//     pack_fields_kernel            integer columns + neighbour count -> bit-packed 8- / 16-byte rows
//   sum / mean (var / std) over neighbours, numpy's pairwise tree (pairwise_segment)
//     aggregate_kernel              from fp64 rows
//     aggregate_packed_kernel       from bit-packed rows, summands rebuilt in registers
//     aggregate_combine_kernel      rows with > 128 neighbours: block sums -> row sums along the same tree
//   sum / mean of integer rows, any order
//     aggregate_i32_kernel, aggregate_i32_combine_kernel
//   aggregate_minmax_kernel         min / max over neighbours
//   aggregate_prod_kernel           left-to-right product over neighbours
//
// Determinism: the neighbour sums follow numpy's pairwise-summation tree (a function of the row
// length only), so they are bitwise equal to the reference's Series.sum() for any launch
// geometry; the other reductions are "per-lane sequential, then a fixed butterfly".
#include "grx_common.h"

#include <cstdlib>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------
// pack: column-major columns -> row-major n x ldr (zero padded)
// ---------------------------------------------------------------------------------------
// columns [c_off, c_off + f) of the row-major block; the pad columns [pad_from, ldr) are zeroed
__global__ __launch_bounds__(256) void pack_rows_kernel(int64_t n, int f, int ldr, GrxPtrTable cols_tab,
                                                        double *__restrict__ rows, int c_off, int pad_from)
{
    const double *const *cols = reinterpret_cast<const double *const *>(cols_tab.p);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double *dst = rows + i * ldr;
        for (int c = 0; c < f; ++c) dst[c_off + c] = cols[c][i];
        for (int c = pad_from; c < ldr; ++c) dst[c] = 0.0;
    }
}

// Rows of exactly 64 bytes (ldr = 8: the 5 - 8 retained columns of a generation on the BASELINE graphs).  A wavefront
// turns 64 rows x 8 columns through its LDS slice so that every store instruction writes 1 KiB of consecutive bytes
// (lane l: 16 bytes at l * 16 + k * 1024) -- the thread-per-row form writes 8 bytes per lane at a stride of 64, eight
// times over the same 64 lines.
__global__ __launch_bounds__(256) void pack_rows8_kernel(int64_t n, int f, GrxPtrTable cols_tab, double *__restrict__ rows)
{
    __shared__ double tile[4][64 * 9];                           // [wave][row * 9 + column]: padded against bank conflicts
    const double *const *cols = reinterpret_cast<const double *const *>(cols_tab.p);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *mine = tile[wave];
    const int64_t nblocks = (n + 63) / 64;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk < nblocks; blk += (int64_t)gridDim.x * 4) {
        const int64_t row0 = blk * 64, i = row0 + lane;
        double v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = (c < f && i < n) ? cols[c][i] : 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) mine[lane * 9 + c] = v[c];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int piece = k * 64 + lane;                     // 16-byte piece of the 4 KiB block
            const int r = piece >> 2, c = (piece & 3) * 2;
            if (row0 + r < n) {
                double2 out;
                out.x = mine[r * 9 + c];
                out.y = mine[r * 9 + c + 1];
                *reinterpret_cast<double2 *>(rows + (row0 + r) * 8 + c) = out;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// The same for ldr a multiple of 16 (rows of whole 128-byte lines): a 64-row x 16-column tile goes through LDS so
// that both sides are coalesced -- columns are read 64 rows (512 bytes) at a time, rows written a line at a time.
constexpr int PK_LD = 65;
__global__ __launch_bounds__(256) void pack_rows_tiled_kernel(int64_t n, int f, int ldr, GrxPtrTable cols_tab,
                                                              double *__restrict__ rows, int c_off, int pad_from)
{
    __shared__ double tile[16 * PK_LD];
    const double *const *cols = reinterpret_cast<const double *const *>(cols_tab.p);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int c_end = pad_from < ldr ? ldr : c_off + f;          // the last launch also zeroes the pad columns
    const int64_t ntiles = (n + 63) / 64;
    for (int64_t tile_i = blockIdx.x; tile_i < ntiles; tile_i += gridDim.x) {
        const int64_t row0 = tile_i * 64;
        for (int cb = c_off; cb < c_end; cb += 16) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = cb + wave + 4 * u - c_off;         // column of this launch's table
                const int64_t i = row0 + lane;
                v[u] = (c < f && i < n) ? cols[c][i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) tile[(wave + 4 * u) * PK_LD + lane] = v[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = (t >> 4) + 16 * u, c = t & 15;
                if (row0 + r < n && cb + c < c_end) rows[(row0 + r) * ldr + cb + c] = tile[c * PK_LD + r];
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------
// neighbour aggregation
// ---------------------------------------------------------------------------------------
// The reference sums a node's neighbour rows column by column with Series.sum(), i.e. with
// numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, pairwise_sum_DOUBLE) in
// the order G[node] lists the neighbours (features/extract.py:108-113).  The kernels reproduce
// that association bit for bit:
//     cnt < 8     sequential
//     cnt <= 128  r[j] = x[j] + x[j+8] + ...;  ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7));  then the
//                 cnt % 8 trailing elements one by one
//     cnt > 128   binary tree over blocks: split at cnt/2 rounded down to a multiple of 8
//     cnt > 8192  ndarray.sum() walks the column in chunks of 8192 elements (the ufunc buffer
//                 size); each chunk is summed as above and added to the running total
// which happens to be a good GPU shape: the eight accumulators are eight independent gathers.
//
// S * CL lanes cooperate on one output row.  Lane = (slot, part): the CL ADJACENT lanes of a slot fetch one
// neighbour row together, part = lane % CL owns its fragment of that row; slot = lane / CL owns the accumulators
// r[slot], r[slot+S], ... (A = 8/S accumulators per lane).  The tree levels that pair accumulators of different
// slots are xor-shuffles, the others are local adds.  Fewer slots = more independent gathers per lane and trip (A of
// them) and more rows per wavefront.
// Rows with more than 128 neighbours are cut into the blocks of numpy's recursion by the host
// (grx_aggregate_plan): the aggregate kernels sum each block like a short row and
// aggregate_combine_kernel adds the block sums along the same binary tree.
constexpr int PW_BLOCK = 128;
constexpr int PW_CHUNK = 8192;

// The segment of cnt <= PW_BLOCK neighbours col[b, b + cnt), written once for every row format: res[] = the NV sums
// a lane carries, in every lane of the group.  Src says where the summands come from: src.load(u) = this lane's
// fragment (Src::Raw) of neighbour u's row, src.values(raw, x) = its NV summands.
template <int S, int CL, int NV, class Src>
__device__ __forceinline__ void pairwise_segment(const int32_t *__restrict__ col, const Src &src, int64_t b, int cnt, int slot,
                                                 int part, double (&res)[NV])
{
    // every summand is rounded before it is added, as numpy does: no fma contraction in here
#pragma clang fp contract(off)
    using Raw = typename Src::Raw;
    constexpr int A = 8 / S, G = S * CL;
    static_assert(S >= 1 && S * A == 8, "lane group must hold 1, 2, 4 or 8 neighbour slots");
    const int c8 = cnt & ~7, rem = cnt - c8;
#pragma unroll
    for (int j = 0; j < NV; ++j) res[j] = 0.0;
    // The cnt % 8 trailing neighbours are ADDED last, one by one, but nothing stops their loads from being issued
    // first: indices, then rows, all in flight with the main part's gathers (inside `if (idx < cnt)` each index
    // load was waited for before its gather, and each gather before the next index: up to 2 A round trips in a
    // row).  Clamped indices re-read the last neighbour; the mask is applied where the values are used.
    Raw tail[A];
    if (rem) {                                            // uniform over the lane group
        int64_t ut[A];
#pragma unroll
        for (int t = 0; t < A; ++t) {
            const int idx = c8 + slot + t * S;
            ut[t] = GRX_STREAM_LD(col[b + (idx < cnt ? idx : cnt - 1)]);
        }
#pragma unroll
        for (int t = 0; t < A; ++t) tail[t] = src.load(ut[t]);
    }
    if (c8) {
        // one trip of 8 neighbours: the lane's A indices, then its A rows, then the summands
        double r[A][NV];
        {
            int64_t u[A];
#pragma unroll
            for (int t = 0; t < A; ++t) u[t] = GRX_STREAM_LD(col[b + slot + t * S]);
            Raw raw[A];
#pragma unroll
            for (int t = 0; t < A; ++t) raw[t] = src.load(u[t]);
#pragma unroll
            for (int t = 0; t < A; ++t) src.values(raw[t], r[t]);
        }
        int i = 8;
        if constexpr (A <= 2) {                           // two trips of 8 per iteration: 2 A gathers in flight per lane
            for (; i + 8 < c8; i += 16) {
                int64_t u[2 * A];
#pragma unroll
                for (int t = 0; t < A; ++t) {
                    u[t] = GRX_STREAM_LD(col[b + i + slot + t * S]);
                    u[A + t] = GRX_STREAM_LD(col[b + i + 8 + slot + t * S]);
                }
                Raw raw[2 * A];
#pragma unroll
                for (int t = 0; t < 2 * A; ++t) raw[t] = src.load(u[t]);
#pragma unroll
                for (int t = 0; t < 2 * A; ++t) {            // the earlier trip's summands first
                    double x[NV];
                    src.values(raw[t], x);
#pragma unroll
                    for (int j = 0; j < NV; ++j) r[t % A][j] += x[j];
                }
            }
        }
        for (; i < c8; i += 8) {
            int64_t u[A];
#pragma unroll
            for (int t = 0; t < A; ++t) u[t] = GRX_STREAM_LD(col[b + i + slot + t * S]);
            Raw raw[A];
#pragma unroll
            for (int t = 0; t < A; ++t) raw[t] = src.load(u[t]);
#pragma unroll
            for (int t = 0; t < A; ++t) {
                double x[NV];
                src.values(raw[t], x);
#pragma unroll
                for (int j = 0; j < NV; ++j) r[t][j] += x[j];
            }
        }
        // ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)): level `bit` pairs residue j with j ^ (1 << bit) -- accumulators of
        // different slots by an xor-shuffle, accumulators of one lane by a local add
#pragma unroll
        for (int bit = 0; bit < 3; ++bit) {
            if ((1 << bit) < S) {
#pragma unroll
                for (int t = 0; t < A; ++t)
#pragma unroll
                    for (int j = 0; j < NV; ++j) r[t][j] += __shfl_xor(r[t][j], CL << bit, G);
            } else {
                const int step = (1 << bit) / S;              // distance between partners in r[]
#pragma unroll
                for (int t = 0; t < A; t += 2 * step) {
                    if (t + step < A) {
#pragma unroll
                        for (int j = 0; j < NV; ++j) r[t][j] += r[t + step][j];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) res[j] = r[0][j];
    }
    if (rem) {
        double x[A][NV];
#pragma unroll
        for (int t = 0; t < A; ++t) src.values(tail[t], x[t]);
#pragma unroll
        for (int i = 0; i < 7; ++i) {                     // trailing element i sits in slot i % S, accumulator i / S
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const double v = S > 1 ? __shfl(x[i / S][j], (i % S) * CL + part, G) : x[i / S][j];
                if (i < rem) res[j] += v;
            }
        }
    }
}

// Source of the fp64 kernel.  A neighbour's feature row is padded to LDR doubles (16/32/64/128 bytes, never straddling
// a 128-byte line) and fetched by CL = LDR/2 adjacent lanes, 16 bytes each, so one wave-level load touches 64/CL
// lines; part owns columns 2*part, 2*part+1.  SQDEV: the summands are (m - x)^2 with the per-column values m0, m1
// (pandas' nanvar: avg = sum / count; ((avg - values) ** 2).sum() -- the same pairwise tree over the transformed values).
template <bool SQDEV>
struct RowSource {
    using Raw = double2;
    const double *base;                                   // rows + 2 * part
    int64_t row_stride;
    double m0, m1;
    __device__ __forceinline__ Raw load(int64_t u) const { return *reinterpret_cast<const double2 *>(base + u * row_stride); }
    __device__ __forceinline__ void values(const Raw &x, double (&v)[2]) const
    {
        // the squares must be rounded before they are added, as numpy does
#pragma clang fp contract(off)
        if constexpr (SQDEV) {
            const double t0 = m0 - x.x, t1 = m1 - x.y;
            v[0] = t0 * t0; v[1] = t1 * t1;
        } else {
            v[0] = x.x; v[1] = x.y;
        }
    }
};

// what one lane holds after a segment
template <class T, int N>
struct Totals { T x[N]; };

// Blocks of the rows with more than PW_BLOCK neighbours (grx_aggregate_plan): handled by the same launch
// as the short rows, one lane group per block of 57..128 neighbours -> blk_sums[blk][16]; the
// combine kernel adds them along numpy's recursion afterwards.
struct BlockWork {
    const int32_t *long_rows;
    const int64_t *blk_begin;
    const int32_t *blk_len;
    const int32_t *blk_row;
    int64_t n_blocks;
    double *blk_sums;
};

// The work of one launch for a lane group of G lanes: the plan's blocks inside [row_begin, row_end) first (the longest
// work items of the launch), then the rows of at most PW_BLOCK neighbours.  segment(b, cnt, v) returns the lane's totals
// over the neighbours col[b, b + cnt) of output row v; store_block(k, totals) keeps those of block k for the combine
// kernel, store_row(v, d, totals) writes the outputs of a short row of d neighbours.
template <int G, class Segment, class StoreBlock, class StoreRow>
__device__ __forceinline__ void blocks_then_rows(const int64_t *__restrict__ row_ptr, int64_t row_begin, int64_t row_end,
                                                 const BlockWork &bw, Segment segment, StoreBlock store_block,
                                                 StoreRow store_row)
{
    // The workgroup size comes from the builtin: outside a kernel body blockDim.x is not folded to the scalar load of
    // the launch's size, and ngroups then lives in two vector registers (aggregate_packed_kernel<2, 5, 4>: 95 -> 97,
    // occupancy 5 -> 4).
    const int64_t wg = __builtin_amdgcn_workgroup_size_x();
    const int64_t group = ((int64_t)blockIdx.x * wg + threadIdx.x) / G;
    const int64_t ngroups = (int64_t)gridDim.x * wg / G;
    for (int64_t k = group; k < bw.n_blocks; k += ngroups) {
        const int64_t v = bw.long_rows[bw.blk_row[k]];
        if (v < row_begin || v >= row_end) continue;
        store_block(k, segment(bw.blk_begin[k], bw.blk_len[k], v));
    }
    for (int64_t v = row_begin + group; v < row_end; v += ngroups) {
        const int64_t b = row_ptr[v], d = row_ptr[v + 1] - b;
        if (d > PW_BLOCK) continue;                       // the block loop above + the combine kernel
        store_row(v, d, segment(b, (int)d, v));
    }
}

// VAR: out_sum / out_mean become out_var / out_std -- the sample variance (ddof = 1, pandas' default)
// of the neighbours' values around mean_in (the 'mean' output of a previous launch) and its root.
template <int LDR, int G, bool VAR = false>
__global__ __launch_bounds__(256) void aggregate_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const double *__restrict__ rows, int64_t row_stride, int f, int64_t row_begin, int64_t row_end,
    double *__restrict__ out_sum, double *__restrict__ out_mean, int64_t ld,
    const double *__restrict__ mean_in, BlockWork bw)
{
    constexpr int CL = (LDR >= 16 ? 16 : LDR) / 2;
    const int lane = threadIdx.x % G;
    const int part = lane % CL, slot = lane / CL;
    const int c0 = 2 * part, c1 = 2 * part + 1;
    using Sums = Totals<double, 2>;
    blocks_then_rows<G>(
        row_ptr, row_begin, row_end, bw,
        [&](int64_t b, int cnt, int64_t v) {
            RowSource<VAR> src{rows + 2 * part, row_stride, 0.0, 0.0};
            if constexpr (VAR) {
                src.m0 = c0 < f ? mean_in[(int64_t)c0 * ld + v] : 0.0;
                src.m1 = c1 < f ? mean_in[(int64_t)c1 * ld + v] : 0.0;
            }
            Sums a;
            pairwise_segment<G / CL, CL, 2>(col, src, b, cnt, slot, part, a.x);
            return a;
        },
        [&](int64_t k, const Sums &a) {
            if (slot == 0) {
                bw.blk_sums[k * 16 + c0] = a.x[0];
                bw.blk_sums[k * 16 + c1] = a.x[1];
            }
        },
        [&](int64_t v, int64_t d, const Sums &a) {
            if (slot != 0) return;
            const double cnt = (double)d, a0 = a.x[0], a1 = a.x[1];
            if (VAR) {
                // count - ddof <= 0 -> NaN -> fillna(0) (extract.py:113)
                const double v0 = (d > 1) ? a0 / (cnt - 1.0) : 0.0, v1 = (d > 1) ? a1 / (cnt - 1.0) : 0.0;
                if (c0 < f) {
                    if (out_sum) out_sum[(int64_t)c0 * ld + v] = v0;
                    if (out_mean) out_mean[(int64_t)c0 * ld + v] = sqrt(v0);
                }
                if (c1 < f) {
                    if (out_sum) out_sum[(int64_t)c1 * ld + v] = v1;
                    if (out_mean) out_mean[(int64_t)c1 * ld + v] = sqrt(v1);
                }
            } else {
                if (c0 < f) {
                    if (out_sum) GRX_STREAM_ST(out_sum[(int64_t)c0 * ld + v], a0);
                    if (out_mean) GRX_STREAM_ST(out_mean[(int64_t)c0 * ld + v], (d > 0) ? a0 / cnt : 0.0);
                }
                if (c1 < f) {
                    if (out_sum) GRX_STREAM_ST(out_sum[(int64_t)c1 * ld + v], a1);
                    if (out_mean) GRX_STREAM_ST(out_mean[(int64_t)c1 * ld + v], (d > 0) ? a1 / cnt : 0.0);
                }
            }
        });
}

// Sixteen lanes per long row (lane c = column c): add the block sums along numpy's recursion
//   sum(n) = n <= 128 ? block : sum(n2) + sum(n - n2),  n2 = n/2 - (n/2) % 8
// chunk by chunk (8192 neighbours), running total over the chunks.  The recursion is flattened by the
// host into its post-order program: blk_ops[i] & 0x7F = number of pending additions after pushing
// block i, bit 7 = last block of a chunk.  Every lane runs the stack machine of its column on a
// private LDS stack (no barriers, no staging: the block sums of a row are read once, 128 bytes per
// block and group, sixteen blocks in flight at a time).
// (First version: one 64-lane workgroup per row with the block sums staged in LDS -- 42 us per launch
// for the 6.7 k long rows of BA 1 M, a chain of five dependent round trips per workgroup.)
constexpr int PW_MAX_DEPTH = 12;

__global__ __launch_bounds__(256) void aggregate_combine_kernel(
    const int64_t *__restrict__ row_ptr, int f, int64_t row_begin, int64_t row_end,
    const int32_t *__restrict__ long_rows, const int64_t *__restrict__ blk_ptr, int64_t n_long,
    const uint8_t *__restrict__ blk_ops, const double *__restrict__ blk_sums, double *__restrict__ out_sum,
    double *__restrict__ out_mean, int64_t ld, int var_mode)
{
    __shared__ double stk[16][PW_MAX_DEPTH][16];
    const int c = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int64_t gstride = (int64_t)gridDim.x * 16;
    for (int64_t h = (int64_t)blockIdx.x * 16 + grp; h < n_long; h += gstride) {
        const int64_t v = long_rows[h];
        if (v < row_begin || v >= row_end) continue;               // uniform over the 16 lanes
        const int64_t n = row_ptr[v + 1] - row_ptr[v];
        const int64_t leaf_end = blk_ptr[h + 1];
        int64_t leaf = blk_ptr[h];
        double total = 0.0;
        int sp = 0;
        // batches of 16 blocks: the loads of a batch are independent (hubs have ~100 blocks -- one load
        // at a time would be a 100-deep latency chain), the folding is sequential
        while (leaf < leaf_end) {
            const int m = (int)((leaf_end - leaf) < 16 ? (leaf_end - leaf) : 16);
            double buf[16];
            int ops[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                buf[j] = (j < m) ? blk_sums[(leaf + j) * 16 + c] : 0.0;
                ops[j] = (j < m) ? (int)blk_ops[leaf + j] : 0;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j < m) {
                    double val = buf[j];
                    for (int k = ops[j] & 0x7F; k > 0; --k) val = stk[grp][--sp][c] + val;   // left + right
                    if (ops[j] & 0x80) total += val;             // chunk complete (sp == 0 here)
                    else stk[grp][sp++][c] = val;
                }
            }
            leaf += m;
        }
        if (c < f) {
            if (var_mode) {                                     // long rows have n > 128 >= 2
                const double var = total / ((double)n - 1.0);
                if (out_sum) out_sum[(int64_t)c * ld + v] = var;
                if (out_mean) out_mean[(int64_t)c * ld + v] = sqrt(var);
            } else {
                if (out_sum) out_sum[(int64_t)c * ld + v] = total;
                if (out_mean) out_mean[(int64_t)c * ld + v] = total / (double)n;
            }
        }
    }
}


// ---------------------------------------------------------------------------------------
// neighbour aggregation of INTEGER rows (generation 1 of unweighted graphs)
// ---------------------------------------------------------------------------------------
// When every source column holds exact non-negative integers below 2^31 (degrees, ego-net edge counts: the whole
// generation-0 block of an unweighted graph) the sums are integers below 2^53, so ANY order of additions gives the
// bits numpy's pairwise tree gives -- and the gather source shrinks from 8 to 4 bytes per column: three columns
// are a 16-byte row, four rows per 64-byte request line, a quarter of the table a 4 MiB L2 has to hold (the hit
// rate of the gather follows sqrt(rows that fit / N) on a power-law graph).  Lane = (slot,
// part): CL = LDI / 4 adjacent lanes fetch one neighbour row (int4 each), slot s takes neighbours s, s + S, ...;
// int64 accumulators, xor-butterfly over the slots, mean = double(sum) / count like the fp64 kernel.
// Rows with more than 128 neighbours reuse the block list of the plan: one lane group per block -> int64 partial
// sums (the blk_sums scratch), added per row by aggregate_i32_combine_kernel.
__global__ __launch_bounds__(256) void pack_rows_i32_kernel(int64_t n, int f, int ldi, GrxPtrTable cols_tab,
                                                            int32_t *__restrict__ rows)
{
    const double *const *cols = reinterpret_cast<const double *const *>(cols_tab.p);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int32_t *dst = rows + i * ldi;
        for (int c = 0; c < f; ++c) dst[c] = (int32_t)cols[c][i];
        for (int c = f; c < ldi; ++c) dst[c] = 0;
    }
}

template <int LDI, int G>
__device__ __forceinline__ void i32_segment(const int32_t *__restrict__ col, const int32_t *__restrict__ rows, int64_t b,
                                            int cnt, int part, int slot, long long (&acc)[4])
{
    constexpr int CL = LDI / 4, S = G / CL;
    const int32_t *base = rows + 4 * part;
    acc[0] = acc[1] = acc[2] = acc[3] = 0;
    // four neighbours of this slot per trip: indices first (clamped), then the four row loads, all independent
    for (int k0 = slot; k0 < cnt; k0 += 4 * S) {
        int64_t u[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + t * S;
            u[t] = GRX_STREAM_LD(col[b + (k < cnt ? k : cnt - 1)]);
        }
        int4 x[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = *reinterpret_cast<const int4 *>(base + u[t] * LDI);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (k0 + t * S < cnt) { acc[0] += x[t].x; acc[1] += x[t].y; acc[2] += x[t].z; acc[3] += x[t].w; }
        }
    }
#pragma unroll
    for (int off = CL; off < G; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off, G);
    }
}

template <int LDI, int G>
__global__ __launch_bounds__(256) void aggregate_i32_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const int32_t *__restrict__ rows, int f,
    int64_t row_begin, int64_t row_end, double *__restrict__ out_sum, double *__restrict__ out_mean, int64_t ld,
    BlockWork bw)
{
    constexpr int CL = LDI / 4;
    const int lane = threadIdx.x % G;
    const int part = lane % CL, slot = lane / CL;
    long long *blk = reinterpret_cast<long long *>(bw.blk_sums);
    using Sums = Totals<long long, 4>;
    blocks_then_rows<G>(
        row_ptr, row_begin, row_end, bw,
        [&](int64_t b, int cnt, int64_t) {
            Sums acc;
            i32_segment<LDI, G>(col, rows, b, cnt, part, slot, acc.x);
            return acc;
        },
        [&](int64_t k, const Sums &acc) {
            if (slot == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) blk[k * 16 + 4 * part + j] = acc.x[j];
            }
        },
        [&](int64_t v, int64_t d, const Sums &acc) {
            if (slot != 0) return;
            const double cnt = (double)d;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 4 * part + j;
                if (c < f) {
                    const double sum = (double)acc.x[j];
                    if (out_sum) GRX_STREAM_ST(out_sum[(int64_t)c * ld + v], sum);
                    if (out_mean) GRX_STREAM_ST(out_mean[(int64_t)c * ld + v], (d > 0) ? sum / cnt : 0.0);
                }
            }
        });
}

// sixteen lanes per long row (lane c = column c): integer partial sums of its blocks, any order
__global__ __launch_bounds__(256) void aggregate_i32_combine_kernel(
    const int64_t *__restrict__ row_ptr, int f, int64_t row_begin, int64_t row_end, const int32_t *__restrict__ long_rows,
    const int64_t *__restrict__ blk_ptr, int64_t n_long, const double *__restrict__ blk_sums, double *__restrict__ out_sum,
    double *__restrict__ out_mean, int64_t ld)
{
    const long long *blk = reinterpret_cast<const long long *>(blk_sums);
    const int c = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int64_t gstride = (int64_t)gridDim.x * 16;
    for (int64_t h = (int64_t)blockIdx.x * 16 + grp; h < n_long; h += gstride) {
        const int64_t v = long_rows[h];
        if (v < row_begin || v >= row_end) continue;
        const int64_t n = row_ptr[v + 1] - row_ptr[v];
        long long total = 0;
        // sixteen block sums in flight at a time (hubs have ~100 blocks: one load at a time is a 100-deep latency chain)
        const int64_t kb = blk_ptr[h], ke = blk_ptr[h + 1];
        for (int64_t k0 = kb; k0 < ke; k0 += 16) {
            long long part[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) part[j] = blk[(k0 + j < ke ? k0 + j : ke - 1) * 16 + c];
#pragma unroll
            for (int j = 0; j < 16; ++j) total += k0 + j < ke ? part[j] : 0;
        }
        if (c < f) {
            const double sum = (double)total;
            if (out_sum) out_sum[(int64_t)c * ld + v] = sum;
            if (out_mean) out_mean[(int64_t)c * ld + v] = sum / (double)n;
        }
    }
}

// ---------------------------------------------------------------------------------------
// neighbour aggregation from BIT-PACKED integer rows (generations 1 and 2 of unweighted graphs)
// ---------------------------------------------------------------------------------------
// The gather is bound by the chip's REQUEST rate, and how many requests miss an XCD's 4 MiB L2 is set by the bytes of
// the gather table (profiles/r04_gather_bw.json: 16-, 32- and 64-byte rows gather at the same rows/s; a 64 MB table
// at 62 G rows/s, a 16 MB one at 92, an L2-resident one at 250).  So the table is made as small as exactness allows:
//   * every summand the reference adds in generation g is either an exact integer S (a degree / ego-net count of
//     generation 0, or a neighbour SUM of such a column) or the mean fl(S / d) of one over d neighbours;
//   * the row of node u therefore only has to carry the integers S_k(u) of the distinct base columns and d(u), each in
//     as many bits as the column's maximum needs (grx_column_bits) -- 8 or 16 bytes instead of 16 / 64;
//   * the kernel rebuilds every summand in registers -- double(S), or double(S) / double(d) with the same correctly
//     rounded division that produced the stored mean -- and adds them in numpy's pairwise order exactly like
//     aggregate_kernel does (for integer summands any order gives the same bits; one code path serves both).
// Lane = slot (CL = 1): S = 2, 4 or 8 lanes per output row (packed_slots), lane s owns the strided accumulators r[s],
// r[s+S], ... of EVERY output column (a whole neighbour row is one 8- / 16-byte load of one lane).  Rows longer than 128 neighbours reuse the plan's block list and
// aggregate_combine_kernel unchanged.
struct PackedDesc {
    int n_out;
    uint8_t word[8], shift[8], bits[8], is_mean[8];    // per output: where its source field sits
    uint8_t d_word, d_shift, d_bits;                     // the neighbour-count field (d_bits = 0: none)
};

template <int WORDS>
struct PackedRow { unsigned long long w[WORDS]; };

template <int WORDS>
__device__ __forceinline__ PackedRow<WORDS> packed_load(const unsigned long long *__restrict__ rows, int64_t u)
{
    PackedRow<WORDS> r;
    if constexpr (WORDS == 1) {
        r.w[0] = rows[u];
    } else {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(rows + 2 * u);
        r.w[0] = v.x; r.w[1] = v.y;
    }
    return r;
}

template <int WORDS>
__device__ __forceinline__ unsigned long long packed_field(const PackedRow<WORDS> &r, int word, int shift, int bits)
{
    const unsigned long long w = (WORDS == 2 && word) ? r.w[WORDS - 1] : r.w[0];
    return bits >= 64 ? w : ((w >> shift) & ((1ull << bits) - 1ull));
}

// the F summands of one neighbour row
// Means: fl(S / d) for F columns that share the divisor.  The compiler's fp64 division is, for operands that need no
// scaling (here 0 <= S < 2^53, 1 <= d < 2^31), exactly: y = rcp(d) refined by two Newton steps, q = S * y,
// r = fma(-d, q, S), q' = fma(r, y, q) -- correctly rounded.  The reciprocal and its refinement do not depend on S, so
// they are done ONCE per neighbour row and every column pays three instructions instead of a whole division; the
// result is the same correctly rounded quotient (tests/test_gpu_packed.py compares ~10^8 quotients with the divisions
// aggregate_kernel's sources were produced by).
template <int WORDS, int F>
__device__ __forceinline__ void packed_values(const PackedRow<WORDS> &r, const PackedDesc &d, double (&x)[F])
{
#pragma clang fp contract(off)
    double cnt = 1.0, y = 0.0;
    if (d.d_bits) {
        cnt = (double)(int)packed_field<WORDS>(r, d.d_word, d.d_shift, d.d_bits);       // < 2^31 (place_fields)
        y = __builtin_amdgcn_rcp(cnt);
        double e = __builtin_fma(-cnt, y, 1.0);
        y = __builtin_fma(y, e, y);
        e = __builtin_fma(-cnt, y, 1.0);
        y = __builtin_fma(y, e, y);
    }
#pragma unroll
    for (int j = 0; j < F; ++j) {
        const unsigned long long f = packed_field<WORDS>(r, d.word[j], d.shift[j], d.bits[j]);
        const double s = d.bits[j] <= 31 ? (double)(int)f : (double)(long long)f;
        if (d.is_mean[j]) {
            // the stored mean of a node without neighbours is 0 (NaN -> 0, extract.py:113)
            const double q = s * y;
            const double rem = __builtin_fma(-cnt, q, s);
            x[j] = cnt > 0.0 ? __builtin_fma(rem, y, q) : 0.0;
        } else {
            x[j] = s;
        }
    }
}

// source of the packed kernel: a lane's fragment is the whole 8- / 16-byte row of the neighbour
template <int WORDS, int F>
struct PackedSource {
    using Raw = PackedRow<WORDS>;
    const unsigned long long *rows;
    const PackedDesc &d;
    __device__ __forceinline__ Raw load(int64_t u) const { return packed_load<WORDS>(rows, u); }
    __device__ __forceinline__ void values(const Raw &r, double (&x)[F]) const { packed_values<WORDS, F>(r, d, x); }
};

template <int WORDS, int F, int S>
__global__ __launch_bounds__(256) void aggregate_packed_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const unsigned long long *__restrict__ rows,
    PackedDesc d, int64_t row_begin, int64_t row_end, double *__restrict__ out_sum, double *__restrict__ out_mean,
    int64_t ld, BlockWork bw)
{
    const int slot = threadIdx.x % S;
    const PackedSource<WORDS, F> src{rows, d};
    using Sums = Totals<double, F>;
    blocks_then_rows<S>(
        row_ptr, row_begin, row_end, bw,
        [&](int64_t b, int cnt, int64_t) {
            Sums a;
            pairwise_segment<S, 1, F>(col, src, b, cnt, slot, 0, a.x);
            return a;
        },
        [&](int64_t k, const Sums &a) {
            if (slot == 0) {
#pragma unroll
                for (int j = 0; j < F; ++j) bw.blk_sums[k * 16 + j] = a.x[j];
            }
        },
        [&](int64_t v, int64_t cntl, const Sums &a) {
            // every lane of the group holds the totals: lane s stores columns s, s + S, ...
            const double cnt = (double)cntl;
#pragma unroll
            for (int j = 0; j < F; ++j) {
                if (slot == j % S) {
                    if (out_sum) GRX_STREAM_ST(out_sum[(int64_t)j * ld + v], a.x[j]);
                    if (out_mean) GRX_STREAM_ST(out_mean[(int64_t)j * ld + v], (cntl > 0) ? a.x[j] / cnt : 0.0);
                }
            }
        });
}

// bit-packed gather source: row u = the fields' integers of node u (+ its neighbour count), see PackedDesc
struct PackFieldsArgs {
    const double *src[8];
    uint8_t word[8], shift[8];
    int n_fields;
    uint8_t d_word, d_shift, d_bits;
};

template <int WORDS>
__global__ __launch_bounds__(256) void pack_fields_kernel(int64_t n, PackFieldsArgs a, const int64_t *__restrict__ row_ptr,
                                                          unsigned long long *__restrict__ rows)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        unsigned long long w[2] = {0ull, 0ull};
        for (int k = 0; k < a.n_fields; ++k)
            w[a.word[k]] |= (unsigned long long)(long long)a.src[k][i] << a.shift[k];
        if (a.d_bits) w[a.d_word] |= (unsigned long long)(row_ptr[i + 1] - row_ptr[i]) << a.d_shift;
        if constexpr (WORDS == 1) rows[i] = w[0];
        else *reinterpret_cast<ulonglong2 *>(rows + 2 * i) = make_ulonglong2(w[0], w[1]);
    }
}

// bits[c] = max(bits[c], number of bits of max(column c over the workgroup's slice of rows [rb, re))) for the columns
// flagged in `mask` (exact non-negative integers by construction); bits[] starts at 0.  The width is monotone in the
// value, so the maximum over the slices' widths is the width of the column maximum -- and it can be max-reduced over
// ranks as a 32-bit integer.  grid = (row slices, columns).
__global__ __launch_bounds__(256) void column_bits_kernel(const double *__restrict__ block, int64_t ld, int64_t rb, int64_t re,
                                                          unsigned long long mask, int32_t *__restrict__ bits)
{
    const int c = blockIdx.y;
    if (!((mask >> c) & 1ull)) return;
    const double *x = block + (int64_t)c * ld;
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = rb + (int64_t)blockIdx.x * 256 + threadIdx.x; i < re; i += stride) m = fmax(m, x[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
        // a column whose maximum is not below 2^62 (or not finite) cannot be packed: 64 says so
        const unsigned long long v = (m >= 0.0 && m < 4.6e18) ? (unsigned long long)m : ~0ull;
        atomicMax(bits + c, v ? 64 - __clzll((long long)v) : 1);
    }
}

// product over the neighbours (agg 'prod'): np.multiply.reduce is a plain left-to-right product, so
// one lane per (row, column) multiplies in adjacency order; the empty product is 1.  Not a tuned
// kernel: the lanes of a row read adjacent doubles of each neighbour row, nothing more.
__global__ __launch_bounds__(256) void aggregate_prod_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ rows,
    int64_t row_stride, int f, int64_t row_begin, int64_t row_end, double *__restrict__ out, int64_t ld)
{
    const int64_t total = (row_end - row_begin) * f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t v = row_begin + i / f;
        const int c = (int)(i % f);
        double p = 1.0;
        for (int64_t k = row_ptr[v]; k < row_ptr[v + 1]; ++k) p *= rows[(int64_t)col[k] * row_stride + c];
        out[(int64_t)c * ld + v] = p;
    }
}

// min / max over the neighbours (aggs 'min', 'max' of features/extract.py:36-47); order-free.
template <int LDR, int G>
__global__ __launch_bounds__(256) void aggregate_minmax_kernel(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const double *__restrict__ rows, int64_t row_stride, int f, int64_t row_begin, int64_t row_end,
    double *__restrict__ out_min, double *__restrict__ out_max, int64_t ld)
{
    constexpr int CL = (LDR >= 16 ? 16 : LDR) / 2;
    constexpr int S = G / CL;
    const int lane = threadIdx.x % G;
    const int part = lane % CL, slot = lane / CL;
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
    const double inf = __builtin_huge_val();
    for (int64_t v = row_begin + group; v < row_end; v += ngroups) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        double lo0 = inf, lo1 = inf, hi0 = -inf, hi1 = -inf;
        for (int64_t k = b + slot; k < e; k += S) {
            const int64_t u = col[k];
            const double2 x = *reinterpret_cast<const double2 *>(rows + u * row_stride + 2 * part);
            lo0 = fmin(lo0, x.x); hi0 = fmax(hi0, x.x);
            lo1 = fmin(lo1, x.y); hi1 = fmax(hi1, x.y);
        }
#pragma unroll
        for (int off = CL; off < G; off <<= 1) {
            lo0 = fmin(lo0, __shfl_xor(lo0, off, G)); hi0 = fmax(hi0, __shfl_xor(hi0, off, G));
            lo1 = fmin(lo1, __shfl_xor(lo1, off, G)); hi1 = fmax(hi1, __shfl_xor(hi1, off, G));
        }
        if (slot == 0) {
            const bool any = e > b;                       // no neighbours -> NaN -> fillna(0) (:113)
            const int c0 = 2 * part, c1 = 2 * part + 1;
            if (c0 < f) {
                if (out_min) out_min[(int64_t)c0 * ld + v] = any ? lo0 : 0.0;
                if (out_max) out_max[(int64_t)c0 * ld + v] = any ? hi0 : 0.0;
            }
            if (c1 < f) {
                if (out_min) out_min[(int64_t)c1 * ld + v] = any ? lo1 : 0.0;
                if (out_max) out_max[(int64_t)c1 * ld + v] = any ? hi1 : 0.0;
            }
        }
    }
}

}  // namespace

// Per-graph preprocessing of grx_aggregate: lane-group width and the block list of the long rows.
struct grx_aggregate_plan {
    int64_t n = 0;
    int lanes_per_row = 8;
    int64_t n_long = 0, n_blocks = 0;
    int64_t max_degree = 0;             // longest row (bounds the integer sums of grx_aggregate_i32)
    int32_t *d_long_rows = nullptr;     // [n_long] ascending
    int64_t *d_blk_ptr = nullptr;       // [n_long + 1]
    int64_t *d_blk_begin = nullptr;     // [n_blocks] position in d_col
    int32_t *d_blk_len = nullptr;       // [n_blocks]
    int32_t *d_blk_row = nullptr;       // [n_blocks] index into d_long_rows
    uint8_t *d_blk_ops = nullptr;       // [n_blocks] post-order program of the combine step
    double *d_blk_sums = nullptr;       // [n_blocks * 16] scratch
};

namespace {

// Blocks of numpy's recursion over [begin, begin+n) in order, with the post-order program of the
// additions: ops[i] = how many times "pop left, add" runs after block i has been pushed.
void pairwise_blocks(int64_t begin, int64_t n, std::vector<int64_t> &b, std::vector<int32_t> &len,
                     std::vector<uint8_t> &ops)
{
    if (n <= PW_BLOCK) { b.push_back(begin); len.push_back((int32_t)n); ops.push_back(0); return; }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    pairwise_blocks(begin, n2, b, len, ops);
    pairwise_blocks(begin + n2, n - n2, b, len, ops);
    ++ops.back();
}

BlockWork block_work(const grx_aggregate_plan *p)
{
    return BlockWork{p->d_long_rows, p->d_blk_begin, p->d_blk_len, p->d_blk_row, p->n_long > 0 ? p->n_blocks : 0,
                     p->d_blk_sums};
}

// second launch of an aggregation: the block sums of the long rows -> their outputs (nothing without long rows)
enum class Combine { Sum, Var, I32 };
int launch_combine(Combine kind, const grx_aggregate_plan *p, const int64_t *row_ptr, int f, int64_t rb, int64_t re,
                   double *s, double *m, int64_t ld, hipStream_t st)
{
    if (p->n_long > 0) {
        GRX_PROF(GRX_K_AGGREGATE_HUB, st);
        const unsigned grid = grx_grid(p->n_long, 16, GRX_NUM_CU * 32);
        if (kind == Combine::I32)
            aggregate_i32_combine_kernel<<<grid, 256, 0, st>>>(row_ptr, f, rb, re, p->d_long_rows, p->d_blk_ptr, p->n_long,
                                                               p->d_blk_sums, s, m, ld);
        else
            aggregate_combine_kernel<<<grid, 256, 0, st>>>(row_ptr, f, rb, re, p->d_long_rows, p->d_blk_ptr, p->n_long,
                                                           p->d_blk_ops, p->d_blk_sums, s, m, ld, kind == Combine::Var ? 1 : 0);
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

template <int LDR, int G>
int launch_aggregate_g(const grx_aggregate_plan *p, const int64_t *row_ptr, const int32_t *col, const double *rows,
                       int64_t row_stride, int f, int64_t rb, int64_t re, double *s, double *m, int64_t ld,
                       hipStream_t st, const double *mean_in = nullptr)
{
    const unsigned grid = grx_grid((re - rb) * G, 256, GRX_NUM_CU * 32);
    const BlockWork bw = block_work(p);
    {
        GRX_PROF(GRX_K_AGGREGATE, st);
        if (mean_in) aggregate_kernel<LDR, G, true><<<grid, 256, 0, st>>>(row_ptr, col, rows, row_stride, f, rb, re, s, m, ld, mean_in, bw);
        else aggregate_kernel<LDR, G><<<grid, 256, 0, st>>>(row_ptr, col, rows, row_stride, f, rb, re, s, m, ld, nullptr, bw);
    }
    GRX_LAUNCH_CHECK();
    return launch_combine(mean_in ? Combine::Var : Combine::Sum, p, row_ptr, f, rb, re, s, m, ld, st);
}

template <int LDR, int G>
int launch_minmax_g(const int64_t *row_ptr, const int32_t *col, const double *rows, int64_t row_stride, int f,
                    int64_t rb, int64_t re, double *lo, double *hi, int64_t ld, hipStream_t st)
{
    {
        GRX_PROF(GRX_K_AGGREGATE, st);
        aggregate_minmax_kernel<LDR, G><<<grx_grid((re - rb) * G, 256, GRX_NUM_CU * 32), 256, 0, st>>>(
            row_ptr, col, rows, row_stride, f, rb, re, lo, hi, ld);
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

// lanes per row G for a row stride: S = G / (LDR/2) must be 1, 2, 4 or 8
template <int LDR>
int launch_aggregate(bool minmax, const grx_aggregate_plan *p, const int64_t *row_ptr, const int32_t *col,
                     const double *rows, int64_t row_stride, int f, int64_t rb, int64_t re, double *a, double *b,
                     int64_t ld, hipStream_t st, const double *mean_in = nullptr)
{
    constexpr int CL = (LDR >= 16 ? 16 : LDR) / 2;
    int G = p->lanes_per_row;
    if (G < CL) G = CL;
    if (G > 8 * CL) G = 8 * CL;
    if (G < 4) G = 4;
#define GRX_AGG_CASE(GG)                                                                                              \
    case GG:                                                                                                          \
        if constexpr (GG >= CL && GG <= 8 * CL)                                                                       \
            return minmax ? launch_minmax_g<LDR, GG>(row_ptr, col, rows, row_stride, f, rb, re, a, b, ld, st)         \
                          : launch_aggregate_g<LDR, GG>(p, row_ptr, col, rows, row_stride, f, rb, re, a, b, ld, st,   \
                                                        mean_in);                                                     \
        break;
    switch (G) {
        GRX_AGG_CASE(4)
        GRX_AGG_CASE(8)
        GRX_AGG_CASE(16)
        GRX_AGG_CASE(32)
    default: break;
    }
#undef GRX_AGG_CASE
    grx_set_error("grx_aggregate: no kernel for ldr=%d lanes_per_row=%d", LDR, G);
    return GRX_ERR_UNSUPPORTED;
}

int aggregate_dispatch(bool minmax, const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col,
                       int f, const double *d_rows, int ldr, int64_t row_begin, int64_t row_end, double *d_a,
                       double *d_b, int64_t ld, void *stream, const double *d_mean_in = nullptr)
{
    const char *who = minmax ? "grx_aggregate_minmax" : (d_mean_in ? "grx_aggregate_var" : "grx_aggregate");
    GRX_REQUIRE(plan != nullptr, "%s: NULL plan (grx_aggregate_plan_create)", who);
    const int64_t n = plan->n;
    GRX_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n, "%s: bad row range", who);
    GRX_REQUIRE(f >= 0 && ldr >= f, "%s: ldr=%d < f=%d", who, ldr, f);
    GRX_REQUIRE(ldr == 2 || ldr == 4 || ldr == 8 || (ldr >= 16 && ldr % 16 == 0),
                "%s: ldr=%d must be 2, 4, 8 or a multiple of 16 (use grx_aggregate_ldr)", who, ldr);
    if (row_end == row_begin || f == 0) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_rows, "%s: NULL pointer", who);
    GRX_REQUIRE(ld >= n, "%s: ld < n", who);
    GRX_REQUIRE((reinterpret_cast<uintptr_t>(d_rows) & 127) == 0, "%s: d_rows must be 128-byte aligned", who);
    hipStream_t st = grx_stream(stream);
    if (ldr < 16)
        switch (ldr) {
        case 2:  return launch_aggregate<2>(minmax, plan, d_row_ptr, d_col, d_rows, ldr, f, row_begin, row_end, d_a, d_b, ld, st, d_mean_in);
        case 4:  return launch_aggregate<4>(minmax, plan, d_row_ptr, d_col, d_rows, ldr, f, row_begin, row_end, d_a, d_b, ld, st, d_mean_in);
        default: return launch_aggregate<8>(minmax, plan, d_row_ptr, d_col, d_rows, ldr, f, row_begin, row_end, d_a, d_b, ld, st, d_mean_in);
        }
    // wide rows: 16 columns (one 128-byte segment of every row) per launch
    for (int c0 = 0; c0 < f; c0 += 16) {
        const int fc = (f - c0 < 16) ? (f - c0) : 16;
        double *a = d_a ? d_a + (int64_t)c0 * ld : nullptr;
        double *b = d_b ? d_b + (int64_t)c0 * ld : nullptr;
        int rc = launch_aggregate<16>(minmax, plan, d_row_ptr, d_col, d_rows + c0, ldr, fc, row_begin, row_end, a, b, ld, st,
                                      d_mean_in ? d_mean_in + (int64_t)c0 * ld : nullptr);
        if (rc != GRX_OK) return rc;
    }
    return GRX_OK;
}

struct PackedPlacement { int row_bytes; uint8_t word[8], shift[8]; uint8_t d_word, d_shift; };

// fields in order, first into word 0 while they fit, then word 1; the neighbour count last; no field straddles a word
bool place_fields(const grx_packed_layout *L, PackedPlacement *P)
{
    if (!L || L->n_fields < 1 || L->n_fields > 7 || L->n_out < 1 || L->n_out > 8 || L->degree_bits < 0 || L->degree_bits > 31)
        return false;
    int used[2] = {0, 0}, w = 0;
    auto put = [&](int bits, uint8_t *word, uint8_t *shift) {
        if (bits < 1 || bits > 62) return false;
        if (used[w] + bits > 64) { if (w == 1) return false; w = 1; }
        *word = (uint8_t)w; *shift = (uint8_t)used[w];
        used[w] += bits;
        return true;
    };
    for (int k = 0; k < L->n_fields; ++k)
        if (!put(L->field_bits[k], &P->word[k], &P->shift[k])) return false;
    P->d_word = P->d_shift = 0;
    if (L->degree_bits && !put(L->degree_bits, &P->d_word, &P->d_shift)) return false;
    for (int j = 0; j < L->n_out; ++j)
        if (L->out_field[j] < 0 || L->out_field[j] >= L->n_fields) return false;
    P->row_bytes = used[1] ? 16 : 8;
    return true;
}

// lanes per output row (S): fewer lanes = more gathers in flight per lane (8 / S per trip) and more rows per wavefront
int packed_slots()
{
    static const int s = [] {
        const char *e = std::getenv("GRX_PACKED_SLOTS");
        const int v = e ? std::atoi(e) : 0;
        return (v == 2 || v == 4 || v == 8) ? v : 4;
    }();
    return s;
}

template <int WORDS, int F>
void launch_packed(hipStream_t st, const int64_t *row_ptr, const int32_t *col, const void *rows, const PackedDesc &d,
                   int64_t rb, int64_t re, double *s, double *m, int64_t ld, const BlockWork &bw)
{
    const int S = packed_slots();
    const unsigned grid = grx_grid((re - rb) * S, 256, GRX_NUM_CU * 32);
    const unsigned long long *r = reinterpret_cast<const unsigned long long *>(rows);
    if (S == 2) aggregate_packed_kernel<WORDS, F, 2><<<grid, 256, 0, st>>>(row_ptr, col, r, d, rb, re, s, m, ld, bw);
    else if (S == 4) aggregate_packed_kernel<WORDS, F, 4><<<grid, 256, 0, st>>>(row_ptr, col, r, d, rb, re, s, m, ld, bw);
    else aggregate_packed_kernel<WORDS, F, 8><<<grid, 256, 0, st>>>(row_ptr, col, r, d, rb, re, s, m, ld, bw);
}
}  // namespace

int64_t grx_internal_plan_max_degree(const grx_aggregate_plan *plan) { return plan ? plan->max_degree : 0; }

extern "C" {

int grx_pack_rows(int64_t n, int f, const double *const *h_col_ptrs, double *d_rows, int ldr,
                  void *stream)
{
    GRX_REQUIRE(n >= 0 && f >= 0 && ldr >= f, "grx_pack_rows: bad shape n=%lld f=%d ldr=%d",
                (long long)n, f, ldr);
    if (n == 0 || ldr == 0) return GRX_OK;
    GRX_REQUIRE(h_col_ptrs && d_rows, "grx_pack_rows: NULL pointer");
    // the pointer table travels as a kernel argument, GRX_MAX_PTRS columns per launch
    for (int c0 = 0; c0 < f || c0 == 0; c0 += GRX_MAX_PTRS) {
        const int fc = (f - c0 < GRX_MAX_PTRS) ? f - c0 : GRX_MAX_PTRS;
        const bool last = c0 + fc >= f;
        GrxPtrTable tab;
        for (int c = 0; c < fc; ++c) tab.p[c] = h_col_ptrs[c0 + c];
        {
            GRX_PROF(GRX_K_PACK_ROWS, grx_stream(stream));
            if (ldr % 16 == 0) {
                pack_rows_tiled_kernel<<<grx_grid(n, 64, GRX_NUM_CU * 16), 256, 0, grx_stream(stream)>>>(n, fc, ldr, tab, d_rows, c0, last ? f : ldr);
            } else if (ldr == 8 && c0 == 0 && last && (reinterpret_cast<uintptr_t>(d_rows) & 15) == 0) {
                pack_rows8_kernel<<<grx_grid(grx_ceil_div(n, 64), 4, GRX_NUM_CU * 16), 256, 0, grx_stream(stream)>>>(
                    n, fc, tab, d_rows);
            } else {
                pack_rows_kernel<<<grx_grid(n, 256, GRX_NUM_CU * 16), 256, 0, grx_stream(stream)>>>(n, fc, ldr, tab, d_rows, c0, last ? f : ldr);
            }
        }
        GRX_LAUNCH_CHECK();
        if (last) break;
    }
    return GRX_OK;
}

int grx_aggregate_plan_create(int64_t n, const int64_t *h_row_ptr, grx_aggregate_plan **out)
{
    GRX_REQUIRE(n >= 0 && out != nullptr && (n == 0 || h_row_ptr != nullptr), "grx_aggregate_plan_create: bad arguments");
    auto *p = new grx_aggregate_plan();
    p->n = n;
    const double avg = n ? (double)(h_row_ptr[n] - h_row_ptr[0]) / (double)n : 0.0;
    p->lanes_per_row = avg < 12 ? 4 : avg < 24 ? 8 : avg < 48 ? 16 : 32;
    std::vector<int32_t> long_rows, blk_len, blk_row;
    std::vector<int64_t> blk_ptr, blk_begin;
    std::vector<uint8_t> blk_ops;
    for (int64_t v = 0; v < n; ++v) {
        const int64_t d = h_row_ptr[v + 1] - h_row_ptr[v];
        if (d > p->max_degree) p->max_degree = d;
        if (d <= PW_BLOCK) continue;
        blk_ptr.push_back((int64_t)blk_begin.size());
        const size_t before = blk_begin.size();
        for (int64_t c0 = 0; c0 < d; c0 += PW_CHUNK) {
            pairwise_blocks(h_row_ptr[v] + c0, (d - c0 < PW_CHUNK) ? d - c0 : PW_CHUNK, blk_begin, blk_len, blk_ops);
            blk_ops.back() |= 0x80;                              // end of a chunk
        }
        blk_row.insert(blk_row.end(), blk_begin.size() - before, (int32_t)long_rows.size());
        long_rows.push_back((int32_t)v);
    }
    blk_ptr.push_back((int64_t)blk_begin.size());
    p->n_long = (int64_t)long_rows.size();
    p->n_blocks = (int64_t)blk_begin.size();
    auto upload = [](void **dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(dst, bytes ? bytes : 8);
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = hipSuccess;
    if (p->n_long) {
        e = upload((void **)&p->d_long_rows, long_rows.data(), long_rows.size() * 4);
        if (e == hipSuccess) e = upload((void **)&p->d_blk_ptr, blk_ptr.data(), blk_ptr.size() * 8);
        if (e == hipSuccess) e = upload((void **)&p->d_blk_begin, blk_begin.data(), blk_begin.size() * 8);
        if (e == hipSuccess) e = upload((void **)&p->d_blk_len, blk_len.data(), blk_len.size() * 4);
        if (e == hipSuccess) e = upload((void **)&p->d_blk_row, blk_row.data(), blk_row.size() * 4);
        if (e == hipSuccess) e = upload((void **)&p->d_blk_ops, blk_ops.data(), blk_ops.size());
        if (e == hipSuccess) e = hipMalloc((void **)&p->d_blk_sums, (size_t)p->n_blocks * 16 * 8);
    }
    if (e != hipSuccess) {
        grx_set_error("grx_aggregate_plan_create: %s", hipGetErrorString(e));
        grx_aggregate_plan_destroy(p);
        return GRX_ERR_HIP;
    }
    *out = p;
    return GRX_OK;
}

void grx_aggregate_plan_destroy(grx_aggregate_plan *p)
{
    if (!p) return;
    (void)hipFree(p->d_long_rows); (void)hipFree(p->d_blk_ptr); (void)hipFree(p->d_blk_begin);
    (void)hipFree(p->d_blk_len); (void)hipFree(p->d_blk_row); (void)hipFree(p->d_blk_ops);
    (void)hipFree(p->d_blk_sums);
    delete p;
}

int grx_aggregate_plan_info(const grx_aggregate_plan *p, int64_t *n_long_rows, int64_t *n_blocks, int *lanes_per_row)
{
    GRX_REQUIRE(p != nullptr, "grx_aggregate_plan_info: NULL plan");
    if (n_long_rows) *n_long_rows = p->n_long;
    if (n_blocks) *n_blocks = p->n_blocks;
    if (lanes_per_row) *lanes_per_row = p->lanes_per_row;
    return GRX_OK;
}

int grx_aggregate_plan_set_lanes(grx_aggregate_plan *p, int lanes_per_row)
{
    GRX_REQUIRE(p != nullptr, "grx_aggregate_plan_set_lanes: NULL plan");
    GRX_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16 || lanes_per_row == 32,
                "grx_aggregate_plan_set_lanes: lanes_per_row must be 4, 8, 16 or 32");
    p->lanes_per_row = lanes_per_row;
    return GRX_OK;
}

int grx_aggregate(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                  const double *d_rows, int ldr, int64_t row_begin, int64_t row_end,
                  double *d_sum, double *d_mean, int64_t ld, void *stream)
{
    return aggregate_dispatch(false, plan, d_row_ptr, d_col, f, d_rows, ldr, row_begin, row_end, d_sum, d_mean, ld, stream);
}

int grx_aggregate_var(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                      const double *d_rows, int ldr, int64_t row_begin, int64_t row_end, const double *d_mean,
                      double *d_var, double *d_std, int64_t ld, void *stream)
{
    GRX_REQUIRE(d_mean != nullptr || f == 0 || row_begin == row_end, "grx_aggregate_var: needs the neighbour means (grx_aggregate)");
    return aggregate_dispatch(false, plan, d_row_ptr, d_col, f, d_rows, ldr, row_begin, row_end, d_var, d_std, ld, stream,
                              d_mean);
}

int grx_aggregate_minmax(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                         const double *d_rows, int ldr, int64_t row_begin, int64_t row_end,
                         double *d_min, double *d_max, int64_t ld, void *stream)
{
    return aggregate_dispatch(true, plan, d_row_ptr, d_col, f, d_rows, ldr, row_begin, row_end, d_min, d_max, ld, stream);
}

int grx_aggregate_prod(const int64_t *d_row_ptr, const int32_t *d_col, int f, const double *d_rows, int ldr,
                       int64_t row_begin, int64_t row_end, double *d_prod, int64_t ld, void *stream)
{
    GRX_REQUIRE(f >= 0 && ldr >= f && row_begin >= 0 && row_begin <= row_end && ld >= row_end,
                "grx_aggregate_prod: bad shape");
    if (f == 0 || row_end == row_begin) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_rows && d_prod, "grx_aggregate_prod: NULL pointer");
    aggregate_prod_kernel<<<grx_grid((row_end - row_begin) * f, 256, GRX_NUM_CU * 32), 256, 0, grx_stream(stream)>>>(d_row_ptr, d_col, d_rows, ldr, f, row_begin, row_end,
                                                               d_prod, ld);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

/* row stride in int32 of the integer gather source: 16- or 32-byte rows; 0 = no integer kernel for that many columns */
int grx_aggregate_ldi(int f) { return f <= 0 ? 0 : f <= 4 ? 4 : f <= 8 ? 8 : 0; }

int grx_pack_rows_i32(int64_t n, int f, const double *const *h_col_ptrs, int32_t *d_rows, int ldi, void *stream)
{
    GRX_REQUIRE(n >= 0 && f >= 1 && ldi == grx_aggregate_ldi(f), "grx_pack_rows_i32: ldi must be grx_aggregate_ldi(f)");
    if (n == 0) return GRX_OK;
    GRX_REQUIRE(h_col_ptrs && d_rows, "grx_pack_rows_i32: NULL pointer");
    GrxPtrTable tab;
    for (int c = 0; c < f; ++c) {
        GRX_REQUIRE(h_col_ptrs[c] != nullptr, "grx_pack_rows_i32: column %d is NULL", c);
        tab.p[c] = h_col_ptrs[c];
    }
    { GRX_PROF(GRX_K_PACK_ROWS, grx_stream(stream));
    pack_rows_i32_kernel<<<grx_grid(n, 256, GRX_NUM_CU * 16), 256, 0, grx_stream(stream)>>>(
        n, f, ldi, tab, d_rows);
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_aggregate_i32_ok(const grx_aggregate_plan *plan, int f)
{
    // integer sums stay exact in fp64 while max_degree * 2^31 <= 2^53
    return plan != nullptr && grx_aggregate_ldi(f) != 0 && plan->max_degree < ((int64_t)1 << 22);
}

int grx_aggregate_i32(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                      const int32_t *d_rows, int ldi, int64_t row_begin, int64_t row_end, double *d_sum, double *d_mean,
                      int64_t ld, void *stream)
{
    GRX_REQUIRE(plan != nullptr, "grx_aggregate_i32: NULL plan");
    GRX_REQUIRE(grx_aggregate_i32_ok(plan, f) && ldi == grx_aggregate_ldi(f),
                "grx_aggregate_i32: f=%d / ldi=%d / max degree %lld outside the integer kernel's range", f, ldi,
                (long long)plan->max_degree);
    const int64_t n = plan->n;
    GRX_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n && ld >= n, "grx_aggregate_i32: bad row range");
    if (row_end == row_begin) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_rows, "grx_aggregate_i32: NULL pointer");
    GRX_REQUIRE((reinterpret_cast<uintptr_t>(d_rows) & 63) == 0, "grx_aggregate_i32: d_rows must be 64-byte aligned");
    hipStream_t st = grx_stream(stream);
    const int CL = ldi / 4;
    int G = plan->lanes_per_row;
    if (G < 4) G = 4;
    if (G > 16) G = 16;
    if (G < CL) G = CL;
    const unsigned grid = grx_grid((row_end - row_begin) * G, 256, GRX_NUM_CU * 32);
    const BlockWork bw = block_work(plan);
    {
        GRX_PROF(GRX_K_AGGREGATE, st);
#define GRX_I32_CASE(LL, GG)                                                                                          \
        if (ldi == LL && G == GG)                                                                                     \
            aggregate_i32_kernel<LL, GG><<<grid, 256, 0, st>>>(d_row_ptr, d_col, d_rows, f, row_begin, row_end, d_sum, \
                                                               d_mean, ld, bw);
        GRX_I32_CASE(4, 4) GRX_I32_CASE(4, 8) GRX_I32_CASE(4, 16) GRX_I32_CASE(8, 4) GRX_I32_CASE(8, 8) GRX_I32_CASE(8, 16)
#undef GRX_I32_CASE
    }
    GRX_LAUNCH_CHECK();
    return launch_combine(Combine::I32, plan, d_row_ptr, f, row_begin, row_end, d_sum, d_mean, ld, st);
}

/* ---- bit-packed integer rows (see PackedDesc above) ---------------------------------------------------------- */

int grx_packed_row_bytes(const grx_packed_layout *layout)
{
    PackedPlacement P;
    return place_fields(layout, &P) ? P.row_bytes : 0;
}

int grx_column_bits(int64_t n, int ncols, const double *d_block, int64_t ld, int64_t row_begin, int64_t row_end,
                    uint64_t int_mask, int32_t *d_bits, void *stream)
{
    GRX_REQUIRE(n >= 0 && ncols >= 0 && ncols <= 64 && row_begin >= 0 && row_begin <= row_end && row_end <= n && ld >= n,
                "grx_column_bits: bad shape (at most 64 columns per call)");
    if (ncols == 0) return GRX_OK;
    GRX_REQUIRE(d_block && d_bits, "grx_column_bits: NULL pointer");
    // d_bits accumulates by atomicMax: the CALLER zeroes it (grx_refex_run clears it with its distance matrix)
    const dim3 grid(grx_grid(row_end - row_begin, 256 * 16, 256), (unsigned)ncols);
    column_bits_kernel<<<grid, 256, 0, grx_stream(stream)>>>(d_block, ld, row_begin, row_end, int_mask, d_bits);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_pack_fields(int64_t n, const grx_packed_layout *layout, const double *const *h_field_cols, const int64_t *d_row_ptr,
                    void *d_rows, void *stream)
{
    PackedPlacement P;
    GRX_REQUIRE(place_fields(layout, &P), "grx_pack_fields: the fields do not fit two 64-bit words (grx_packed_row_bytes)");
    GRX_REQUIRE(n >= 0 && h_field_cols && d_rows && (d_row_ptr || !layout->degree_bits), "grx_pack_fields: NULL pointer");
    GRX_REQUIRE((reinterpret_cast<uintptr_t>(d_rows) & 15) == 0, "grx_pack_fields: d_rows must be 16-byte aligned");
    if (n == 0) return GRX_OK;
    PackFieldsArgs a{};
    a.n_fields = layout->n_fields;
    for (int k = 0; k < layout->n_fields; ++k) {
        GRX_REQUIRE(h_field_cols[k] != nullptr, "grx_pack_fields: field column %d is NULL", k);
        a.src[k] = h_field_cols[k];
        a.word[k] = P.word[k];
        a.shift[k] = P.shift[k];
    }
    a.d_word = P.d_word; a.d_shift = P.d_shift; a.d_bits = (uint8_t)layout->degree_bits;
    hipStream_t st = grx_stream(stream);
    const unsigned grid = grx_grid(n, 256, GRX_NUM_CU * 16);
    {
        GRX_PROF(GRX_K_PACK_ROWS, st);
        if (P.row_bytes == 8) pack_fields_kernel<1><<<grid, 256, 0, st>>>(n, a, d_row_ptr, reinterpret_cast<unsigned long long *>(d_rows));
        else pack_fields_kernel<2><<<grid, 256, 0, st>>>(n, a, d_row_ptr, reinterpret_cast<unsigned long long *>(d_rows));
    }
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_aggregate_packed(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col,
                         const grx_packed_layout *layout, const void *d_rows, int64_t row_begin, int64_t row_end,
                         double *d_sum, double *d_mean, int64_t ld, void *stream)
{
    GRX_REQUIRE(plan != nullptr, "grx_aggregate_packed: NULL plan");
    PackedPlacement P;
    GRX_REQUIRE(place_fields(layout, &P), "grx_aggregate_packed: the fields do not fit two 64-bit words");
    const int64_t n = plan->n;
    GRX_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n && ld >= n, "grx_aggregate_packed: bad row range");
    if (row_end == row_begin) return GRX_OK;
    GRX_REQUIRE(d_row_ptr && d_col && d_rows, "grx_aggregate_packed: NULL pointer");
    PackedDesc d{};
    d.n_out = layout->n_out;
    bool any_mean = false;
    for (int j = 0; j < layout->n_out; ++j) {
        const int k = layout->out_field[j];
        d.word[j] = P.word[k]; d.shift[j] = P.shift[k]; d.bits[j] = (uint8_t)layout->field_bits[k];
        d.is_mean[j] = layout->out_is_mean[j] ? 1 : 0;
        any_mean = any_mean || d.is_mean[j];
    }
    GRX_REQUIRE(!any_mean || layout->degree_bits > 0, "grx_aggregate_packed: mean summands need the neighbour-count field");
    d.d_word = P.d_word; d.d_shift = P.d_shift; d.d_bits = (uint8_t)layout->degree_bits;
    hipStream_t st = grx_stream(stream);
    const BlockWork bw = block_work(plan);
    {
        GRX_PROF(GRX_K_AGGREGATE, st);
#define GRX_PACKED_CASE(FF)                                                                                           \
        case FF:                                                                                                      \
            if (P.row_bytes == 8) launch_packed<1, FF>(st, d_row_ptr, d_col, d_rows, d, row_begin, row_end, d_sum, d_mean, ld, bw); \
            else launch_packed<2, FF>(st, d_row_ptr, d_col, d_rows, d, row_begin, row_end, d_sum, d_mean, ld, bw); \
            break;
        switch (layout->n_out) {
            GRX_PACKED_CASE(1) GRX_PACKED_CASE(2) GRX_PACKED_CASE(3) GRX_PACKED_CASE(4)
            GRX_PACKED_CASE(5) GRX_PACKED_CASE(6) GRX_PACKED_CASE(7) GRX_PACKED_CASE(8)
        default: break;
        }
#undef GRX_PACKED_CASE
    }
    GRX_LAUNCH_CHECK();
    return launch_combine(Combine::Sum, plan, d_row_ptr, layout->n_out, row_begin, row_end, d_sum, d_mean, ld, st);
}

/* row stride (in doubles) grx_pack_rows / grx_aggregate use for f columns */
int grx_aggregate_ldr(int f)
{
    if (f <= 2) return 2;
    if (f <= 4) return 4;
    if (f <= 8) return 8;
    return (f + 15) / 16 * 16;
}

}  // extern "C"
