// grx_similarity.hip -- structural similarity, the third application of RolX (Henderson et al., KDD 2012, section 5.2):
// for every query row of a node x column table its k nearest candidate rows, exactly, by cosine similarity or Euclidean
// distance.  Dense all-pairs arithmetic plus selection over 1 <= c <= GRX_MAX_ROLES columns; grx.h states the contract.
//
// Arithmetic (restated bit for bit by tests/similarity_oracle.py).  Every sum over the columns runs j = 0 .. c - 1 in one
// lane, starting from +0.0; every product and every difference is rounded on its own before it is added (compiled
// without contraction: the pragma below and the FILEFLAGS line of the Makefile).
//   cosine:     norm(x) = sqrt(sum_j x_j * x_j);  xn_j = norm > 0 ? x_j / norm : 0;  score = sum_j qn_j * xn_j; key = -score
//   Euclidean:  key = d2 = sum_j (q_j - x_j) * (q_j - x_j);  score = sqrt(d2)
// A pair's key depends on its two rows only -- not on the tile, the segment or the launch shape -- and a product or a
// squared difference does not change when the rows trade places: score(a, b) == score(b, a) bitwise.  The columns are
// padded to CP (the next of 1, 2, 4, 6, 8, 12, 16, 24, 32) with +0.0 on both sides: a padded term is +0.0 and adding it
// to a sum that started from +0.0 changes no bit.
//
// Order: the result of a query is the first k candidates in the strict total order (key ascending, then candidate row
// ascending), the row d_self[q] left out and NaN keys (non-finite input, the caller's to refuse) never taken.  The order
// is strict, so the result is unique whatever the segments and the tiles; there are no floating-point atomics.
//
// Method, three launches (two with one segment).
//   sim_prepare_kernel   the workspace copies Xn [n, CP] and Qn [nq, CP] (one copy when Q aliases X): normalised once
//                        per row for the cosine, copied for the Euclidean distance, padded with zeros.  No pair ever
//                        renormalises a row.
//   sim_scan_kernel      workgroup = ONE wavefront = a tile of SIM_TQ = 128 queries, two per lane, held in registers
//                        (2 CP fp64), against one contiguous range of candidates (blockIdx.y = segment).  Candidates pass
//                        through LDS in tiles of SIM_TC = 64 rows (64 CP doubles, contiguous in Xn): the next tile is in
//                        flight in registers while the current one is scanned.  All lanes read the same candidate at
//                        once -- a broadcast, no bank conflict.  Every query keeps its k best so far as a sorted list
//                        in LDS (slot-major, lane-minor: conflict-free whichever slot a lane touches) and the key of
//                        the last as a threshold in a register; a candidate is inserted only when it beats the
//                        threshold (equal keys do not: within a range the rows ascend), by shifting the tail of the
//                        list.  After warm-up almost nothing passes, so a pair costs CP multiplies, CP adds (Euclidean:
//                        plus CP subtractions) and one compare.  Candidates arriving best-last insert every time
//                        (k shifts per pair: the slow order, still exact).
//   sim_merge_kernel     with more than one segment the scan writes its lists to the workspace ([segment][slot][query])
//                        and one lane per query merges them in segment order with the same insertion, leaving a
//                        segment at its first entry that does not pass (its list is sorted).
// segments = 0: enough segments for 1,024 scan workgroups (one wavefront per SIMD), at most SIM_MAX_SEGMENTS = 256 and
// at least four tiles each; a request above the number of candidate tiles is served with one tile per segment.  The
// scan takes BATCH = 4 candidates (2 above 16 columns) at a time: their keys first, then the tests in row order.
//
// Budget.  LDS per scan workgroup: the tile 512 CP bytes (<= 16 KiB) plus the lists KCAP x 128 x 12 bytes, KCAP = 16 for
// k <= 16 (24 KiB) and 64 above (96 KiB): at c = 6, k = 10 that is 27 KiB, five workgroups = five wavefronts per CU of
// the 160 KiB; at k > 16 one workgroup per CU.  Registers: 2 CP (queries) + CP (tile in flight) fp64.  No instantiation
// uses scratch memory (hipcc -Rpass-analysis=kernel-resource-usage: profiles/similarity.txt).
//
// Bound.  nq n pairs x 2 c fp64 vector operations (3 c for the Euclidean distance), none of them fused: at the chip's
// fp64 vector rate of 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T operations/s (the datasheet's 78.6 TFLOPS counts a
// fused multiply-add as two) that is 3.3 T pairs/s at c = 6 and 0.61 T pairs/s at c = 32 for the cosine: 0.33 ms resp.
// 1.7 ms for 1,024 queries against 1 M rows.  Bytes: X is read once per query tile (8 CP n bytes per 128 queries, from
// L2 after the first tile) and 12 k bytes are written per query: 48 MB + 12 KB against 12 G operations at 1,024 x 1 M x
// c = 6, so the arithmetic is the bound.  The LDS broadcast keeps pace with it only just: a ds_read_b64 takes 2 LDS
// cycles per wavefront and column, the 2 x 2 vector operations it feeds 16 cycles of one SIMD, four SIMDs share the LDS.
// Nobody had measured this instruction mix: profiles/similarity.txt records the achieved fraction of the bound -- 6 % to
// 29 % for 1,024 queries against 1 M rows, 9 % to 12 % for all pairs at 100 k rows: the scan is not yet bound by the
// arithmetic, and one segment per 8 query tiles shows a wavefront alone needs about 600 cycles per candidate row.
//
// Not used: the fp64 MFMA (v_mfma_f64_16x16x4_f64).  Its accumulation order inside the instruction cannot be restated
// operation by operation, so the bits would no longer be those of the oracle and score(a, b) == score(b, a) would not
// follow.  It is the next lever (twice the vector rate), behind a tolerance contract instead of a bitwise one.
#pragma clang fp contract(off)

#include "grx_common.h"

namespace {

constexpr int SIM_WAVE = GRX_WAVE;       // threads of a scan / merge workgroup: one wavefront
constexpr int SIM_QPL = 2;               // queries per lane
constexpr int SIM_TQ = SIM_WAVE * SIM_QPL;   // query tile
constexpr int SIM_TC = 64;               // candidate tile
constexpr int SIM_MAX_SEGMENTS = 256;    // most segments the library chooses
constexpr int SIM_SEGMENT_LIMIT = 1024;  // most segments a call is served with (gridDim.y)
constexpr int SIM_TARGET_WG = 1024;      // scan workgroups the library aims at: one wavefront per SIMD (measured: with
                                         // twice as many the lists' warm-up and the merge cost more than they hide)
constexpr int SIM_MIN_SEG_TILES = 4;     // candidate tiles per segment the library keeps
constexpr int SIM_SMALL_K = 16;          // list capacity of the small instantiation; GRX_MAX_TOPK of the other
constexpr int SIM_BLOCK = 256;           // prepare / fill kernels

struct SimArgs {
    int64_t n, nq;
    const double *__restrict__ Xn;       // [n, CP]
    const double *__restrict__ Qn;       // [nq, CP]
    const int32_t *__restrict__ self;    // [nq] or NULL
    int k;
    int64_t tiles, tiles_per_seg;
    int segments;
    int32_t *__restrict__ out_index;     // [nq, ld_out]
    double *__restrict__ out_score;
    int64_t ld_out;
    double *__restrict__ part_key;       // [segments, k, nq], NULL with one segment
    int32_t *__restrict__ part_idx;
};

__device__ __forceinline__ double sim_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double sim_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// (key, cand) into this lane's sorted list keys[p * STRIDE], ids[p * STRIDE], p < k: behind every entry whose key is not
// greater (the caller offers candidates in ascending row order), the last entry dropped when the list is full
template <int STRIDE>
__device__ __forceinline__ void sim_insert(double *keys, int32_t *ids, int k, int &cnt, double &thr, double key, int32_t cand)
{
    int p = cnt < k ? cnt : k - 1;
    while (p > 0 && keys[(p - 1) * STRIDE] > key) {
        keys[p * STRIDE] = keys[(p - 1) * STRIDE];
        ids[p * STRIDE] = ids[(p - 1) * STRIDE];
        --p;
    }
    keys[p * STRIDE] = key;
    ids[p * STRIDE] = cand;
    if (cnt < k) ++cnt;
    if (cnt == k) thr = keys[(k - 1) * STRIDE];
}

// a candidate is taken when it beats the k-th best so far or the list is not full yet; never a NaN
__device__ __forceinline__ bool sim_passes(double key, double thr, int cnt, int k)
{
    return key < thr || (cnt < k && key == key);
}

__device__ __forceinline__ double sim_score(double key, bool cosine) { return cosine ? -key : sqrt(key); }

// out[r, 0 .. cp) = the row as the scan reads it: x / norm (0 for a row of norm 0) resp. x, zeros from column c on
__global__ __launch_bounds__(SIM_BLOCK) void sim_prepare_kernel(int64_t n, int c, int cp, const double *__restrict__ X,
                                                                 int64_t ldx, int cosine, double *__restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * SIM_BLOCK) {
        const double *row = X + r * ldx;
        double norm = 0.0;
        if (cosine) {
            double s = 0.0;
            for (int j = 0; j < c; ++j) {
                const double p = row[j] * row[j];
                s += p;
            }
            norm = sqrt(s);
        }
        for (int j = 0; j < cp; ++j) {
            double v = j < c ? row[j] : 0.0;
            if (cosine) v = j < c && norm > 0.0 ? v / norm : 0.0;
            out[r * cp + j] = v;
        }
    }
}

// the result of a query without candidates: index -1, score NaN
__global__ __launch_bounds__(SIM_BLOCK) void sim_fill_kernel(int64_t nq, int k, int32_t *__restrict__ index,
                                                              double *__restrict__ score, int64_t ld_out)
{
    for (int64_t t = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x; t < nq * k; t += (int64_t)gridDim.x * SIM_BLOCK) {
        index[t / k * ld_out + t % k] = -1;
        score[t / k * ld_out + t % k] = sim_nan();
    }
}

template <int CP, bool COS, int KCAP>
__global__ __launch_bounds__(SIM_WAVE) void sim_scan_kernel(const SimArgs A)
{
    __shared__ double tile[SIM_TC * CP];
    __shared__ double keys[KCAP * SIM_TQ];
    __shared__ int32_t ids[KCAP * SIM_TQ];
    constexpr int BATCH = CP <= 16 ? 4 : 2;                     // divides SIM_TC
    const int lane = threadIdx.x, k = A.k;
    const int64_t q0 = (int64_t)blockIdx.x * SIM_TQ;
    const int seg = blockIdx.y;

    double q[SIM_QPL][CP], thr[SIM_QPL];
    int32_t self[SIM_QPL];
    int cnt[SIM_QPL];
#pragma unroll
    for (int u = 0; u < SIM_QPL; ++u) {
        const int64_t qi = q0 + u * SIM_WAVE + lane;
        const bool live = qi < A.nq;
#pragma unroll
        for (int j = 0; j < CP; ++j) q[u][j] = live ? A.Qn[qi * CP + j] : 0.0;
        self[u] = live && A.self ? A.self[qi] : -1;
        cnt[u] = live ? 0 : k;                                  // a lane without a query takes nothing
        thr[u] = live ? sim_inf() : -sim_inf();
    }

    const int64_t t_begin = (int64_t)seg * A.tiles_per_seg;
    const int64_t t_end = t_begin + A.tiles_per_seg < A.tiles ? t_begin + A.tiles_per_seg : A.tiles;
    const int64_t total = A.n * CP;                             // doubles of Xn
    double pre[CP];                                             // the tile in flight: doubles j * 64 + lane of it
#pragma unroll
    for (int j = 0; j < CP; ++j) {
        const int64_t at = t_begin * SIM_TC * CP + j * SIM_WAVE + lane;
        pre[j] = t_begin < t_end && at < total ? A.Xn[at] : 0.0;
    }
    for (int64_t t = t_begin; t < t_end; ++t) {
        __syncthreads();                                        // the previous tile has been read
#pragma unroll
        for (int j = 0; j < CP; ++j) tile[j * SIM_WAVE + lane] = pre[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CP; ++j) {
            const int64_t at = (t + 1) * SIM_TC * CP + j * SIM_WAVE + lane;
            pre[j] = t + 1 < t_end && at < total ? A.Xn[at] : 0.0;
        }
        const int64_t base = t * SIM_TC;
        const int rows = A.n - base < SIM_TC ? (int)(A.n - base) : SIM_TC;
        // BATCH candidates at a time: their keys first -- independent chains, the LDS reads in flight together --,
        // then the tests in row order (the whole tile is defined: rows past the end hold zeros and are not offered)
        for (int i0 = 0; i0 < rows; i0 += BATCH) {
            double key[BATCH][SIM_QPL];
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
#pragma unroll
                for (int u = 0; u < SIM_QPL; ++u) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < CP; ++j) {
                        const double x = tile[(i0 + b) * CP + j];
                        if (COS) {
                            const double p = q[u][j] * x;
                            acc += p;
                        } else {
                            const double d = q[u][j] - x;
                            const double p = d * d;
                            acc += p;
                        }
                    }
                    key[b][u] = COS ? -acc : acc;
                }
            }
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                const int32_t cand = (int32_t)(base + i0 + b);
                if (i0 + b >= rows) break;
#pragma unroll
                for (int u = 0; u < SIM_QPL; ++u) {
                    if (sim_passes(key[b][u], thr[u], cnt[u], k) && cand != self[u])
                        sim_insert<SIM_TQ>(keys + u * SIM_WAVE + lane, ids + u * SIM_WAVE + lane, k, cnt[u], thr[u], key[b][u],
                                           cand);
                }
            }
        }
    }

#pragma unroll
    for (int u = 0; u < SIM_QPL; ++u) {
        const int64_t qi = q0 + u * SIM_WAVE + lane;
        if (qi >= A.nq) continue;
        const double *mine = keys + u * SIM_WAVE + lane;
        const int32_t *mine_ids = ids + u * SIM_WAVE + lane;
        for (int p = 0; p < k; ++p) {
            const bool have = p < cnt[u];
            if (A.part_key) {                                   // this segment's list, for the merge
                const int64_t at = ((int64_t)seg * k + p) * A.nq + qi;
                A.part_key[at] = have ? mine[p * SIM_TQ] : sim_nan();
                A.part_idx[at] = have ? mine_ids[p * SIM_TQ] : -1;
            } else {
                A.out_index[qi * A.ld_out + p] = have ? mine_ids[p * SIM_TQ] : -1;
                A.out_score[qi * A.ld_out + p] = have ? sim_score(mine[p * SIM_TQ], COS) : sim_nan();
            }
        }
    }
}

// one lane per query: the segments' sorted lists in segment order (= ascending candidate rows) through the same insertion
__global__ __launch_bounds__(SIM_WAVE) void sim_merge_kernel(const SimArgs A, int cosine)
{
    __shared__ double keys[GRX_MAX_TOPK * SIM_WAVE];
    __shared__ int32_t ids[GRX_MAX_TOPK * SIM_WAVE];
    const int lane = threadIdx.x, k = A.k;
    const int64_t qi = (int64_t)blockIdx.x * SIM_WAVE + lane;
    if (qi >= A.nq) return;                                     // no barrier below
    double *mine = keys + lane;
    int32_t *mine_ids = ids + lane;
    int cnt = 0;
    double thr = sim_inf();
    double head_key = A.part_key[qi];
    int32_t head_idx = A.part_idx[qi];
    for (int s = 0; s < A.segments; ++s) {
        double key = head_key;
        int32_t idx = head_idx;
        if (s + 1 < A.segments) {                               // the next head is in flight while this list is walked
            head_key = A.part_key[(int64_t)(s + 1) * k * A.nq + qi];
            head_idx = A.part_idx[(int64_t)(s + 1) * k * A.nq + qi];
        }
        for (int p = 0; idx >= 0 && sim_passes(key, thr, cnt, k);) {
            sim_insert<SIM_WAVE>(mine, mine_ids, k, cnt, thr, key, idx);
            if (++p == k) break;
            key = A.part_key[((int64_t)s * k + p) * A.nq + qi];
            idx = A.part_idx[((int64_t)s * k + p) * A.nq + qi];
        }
    }
    for (int p = 0; p < k; ++p) {
        const bool have = p < cnt;
        A.out_index[qi * A.ld_out + p] = have ? mine_ids[p * SIM_WAVE] : -1;
        A.out_score[qi * A.ld_out + p] = have ? sim_score(mine[p * SIM_WAVE], cosine != 0) : sim_nan();
    }
}

// columns of the workspace copies: c rounded up to a compiled width
int sim_padded(int c)
{
    const int widths[] = {1, 2, 4, 6, 8, 12, 16, 24, 32};
    for (int w : widths)
        if (c <= w) return w;
    return GRX_MAX_ROLES;
}

// (segments the call is served with, candidate tiles of each): every segment holds at least one tile
void sim_plan(int64_t n, int64_t nq, int segments, int *served, int64_t *tiles_per_seg)
{
    const int64_t tiles = grx_ceil_div(n, SIM_TC);
    int64_t s = segments;
    if (segments == 0) {
        s = grx_ceil_div(SIM_TARGET_WG, grx_ceil_div(nq, SIM_TQ));
        if (s > SIM_MAX_SEGMENTS) s = SIM_MAX_SEGMENTS;
        if (s > tiles / SIM_MIN_SEG_TILES) s = tiles / SIM_MIN_SEG_TILES;
    }
    if (s > SIM_SEGMENT_LIMIT) s = SIM_SEGMENT_LIMIT;
    if (s > tiles) s = tiles;
    if (s < 1) s = 1;
    *tiles_per_seg = grx_ceil_div(tiles, s);
    *served = (int)grx_ceil_div(tiles, *tiles_per_seg);
}

struct SimLayout {
    double *xn, *qn, *part_key;
    int32_t *part_idx;                                       // the two part_ lists are empty when one segment serves
};

SimLayout sim_layout(GrxCarve &cv, int64_t n, int64_t nq, int c, int k, int segments)
{
    int served = 1;
    int64_t tps = 0;
    sim_plan(n, nq, segments, &served, &tps);
    const size_t cp = (size_t)sim_padded(c);
    const size_t lists = served > 1 ? (size_t)served * k * nq : 0;
    SimLayout L;
    L.xn = cv.take<double>((size_t)n * cp);
    L.qn = cv.take<double>((size_t)nq * cp);
    L.part_key = cv.take<double>(lists);
    L.part_idx = cv.take<int32_t>(lists);
    return L;
}

template <int CP, bool COS>
void sim_launch_k(const SimArgs &A, dim3 grid, hipStream_t st)
{
    if (A.k <= SIM_SMALL_K)
        sim_scan_kernel<CP, COS, SIM_SMALL_K><<<grid, SIM_WAVE, 0, st>>>(A);
    else
        sim_scan_kernel<CP, COS, GRX_MAX_TOPK><<<grid, SIM_WAVE, 0, st>>>(A);
}

template <int CP>
void sim_launch(const SimArgs &A, bool cosine, dim3 grid, hipStream_t st)
{
    if (cosine)
        sim_launch_k<CP, true>(A, grid, st);
    else
        sim_launch_k<CP, false>(A, grid, st);
}

bool sim_valid_sizes(int64_t n, int64_t nq, int c, int k, int segments)
{
    return n >= 0 && n < (int64_t)1 << 31 && nq >= 0 && nq < (int64_t)1 << 31 && c >= 1 && c <= GRX_MAX_ROLES && k >= 1 &&
           k <= GRX_MAX_TOPK && segments >= 0;
}

}  // namespace

extern "C" size_t grx_similar_rows_workspace_bytes(int64_t n, int64_t nq, int c, int k, int segments)
{
    if (!sim_valid_sizes(n, nq, c, k, segments) || n == 0 || nq == 0) return 0;
    return grx_carve_bytes(sim_layout, n, nq, c, k, segments);
}

extern "C" int grx_similar_rows(int64_t n, int c, const double *d_X, int64_t ldx, int64_t nq, const double *d_Q,
                                int64_t ldq, const int32_t *d_self, int k, int metric, int segments, int32_t *d_index,
                                double *d_score, int64_t ld_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    GRX_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "grx_similar_rows: n = %lld out of range [0, 2^31)", (long long)n);
    GRX_REQUIRE(nq >= 0 && nq < (int64_t)1 << 31, "grx_similar_rows: nq = %lld out of range [0, 2^31)", (long long)nq);
    GRX_REQUIRE(c >= 1, "grx_similar_rows: c = %d", c);
    if (c > GRX_MAX_ROLES) {
        grx_set_error("grx_similar_rows: c = %d above GRX_MAX_ROLES = %d", c, GRX_MAX_ROLES);
        return GRX_ERR_UNSUPPORTED;
    }
    GRX_REQUIRE(k >= 1 && k <= GRX_MAX_TOPK, "grx_similar_rows: k = %d out of range [1, GRX_MAX_TOPK = %d]", k, GRX_MAX_TOPK);
    GRX_REQUIRE(metric == GRX_SIMILARITY_COSINE || metric == GRX_SIMILARITY_EUCLIDEAN, "grx_similar_rows: metric = %d", metric);
    GRX_REQUIRE(segments >= 0, "grx_similar_rows: segments = %d", segments);
    GRX_REQUIRE(ldx >= c, "grx_similar_rows: ldx = %lld < c = %d", (long long)ldx, c);
    GRX_REQUIRE(ldq >= c, "grx_similar_rows: ldq = %lld < c = %d", (long long)ldq, c);
    GRX_REQUIRE(ld_out >= k, "grx_similar_rows: ld_out = %lld < k = %d", (long long)ld_out, k);
    if (nq == 0) return GRX_OK;
    const hipStream_t st = grx_stream(stream);
    if (n == 0) {                                               // queries without candidates: the slots that exist
        if (d_index && d_score) {
            sim_fill_kernel<<<grx_grid(nq * k, SIM_BLOCK, 2048), SIM_BLOCK, 0, st>>>(nq, k, d_index, d_score, ld_out);
            GRX_LAUNCH_CHECK();
        }
        return GRX_OK;
    }
    GRX_REQUIRE(d_X && d_Q && d_index && d_score && d_workspace, "grx_similar_rows: null pointer");
    GrxCarve cv(d_workspace);
    const SimLayout L = sim_layout(cv, n, nq, c, k, segments);
    GRX_REQUIRE(workspace_bytes >= cv.used, "grx_similar_rows: workspace of %zu bytes, %zu needed "
                "(grx_similar_rows_workspace_bytes)", workspace_bytes, cv.used);

    const bool cosine = metric == GRX_SIMILARITY_COSINE;
    const int cp = sim_padded(c);
    double *Xn = L.xn, *Qn = L.qn;
    sim_prepare_kernel<<<grx_grid(n, SIM_BLOCK, 2048), SIM_BLOCK, 0, st>>>(n, c, cp, d_X, ldx, cosine, Xn);
    if (d_Q == d_X && ldq == ldx && nq == n)
        Qn = Xn;                                                // the rows query themselves: one copy
    else
        sim_prepare_kernel<<<grx_grid(nq, SIM_BLOCK, 2048), SIM_BLOCK, 0, st>>>(nq, c, cp, d_Q, ldq, cosine, Qn);

    SimArgs A{};
    A.n = n;
    A.nq = nq;
    A.Xn = Xn;
    A.Qn = Qn;
    A.self = d_self;
    A.k = k;
    A.tiles = grx_ceil_div(n, SIM_TC);
    sim_plan(n, nq, segments, &A.segments, &A.tiles_per_seg);
    A.out_index = d_index;
    A.out_score = d_score;
    A.ld_out = ld_out;
    if (A.segments > 1) {
        A.part_key = L.part_key;
        A.part_idx = L.part_idx;
    }
    const dim3 grid((unsigned)grx_ceil_div(nq, SIM_TQ), (unsigned)A.segments);
    switch (cp) {
    case 1: sim_launch<1>(A, cosine, grid, st); break;
    case 2: sim_launch<2>(A, cosine, grid, st); break;
    case 4: sim_launch<4>(A, cosine, grid, st); break;
    case 6: sim_launch<6>(A, cosine, grid, st); break;
    case 8: sim_launch<8>(A, cosine, grid, st); break;
    case 12: sim_launch<12>(A, cosine, grid, st); break;
    case 16: sim_launch<16>(A, cosine, grid, st); break;
    case 24: sim_launch<24>(A, cosine, grid, st); break;
    default: sim_launch<32>(A, cosine, grid, st); break;
    }
    if (A.segments > 1)
        sim_merge_kernel<<<(unsigned)grx_ceil_div(nq, SIM_WAVE), SIM_WAVE, 0, st>>>(A, cosine);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}
