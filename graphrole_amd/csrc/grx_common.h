// grx_common.h -- internal helpers shared by the libgrx.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "grx.h"

void grx_set_error(const char *fmt, ...);

#define GRX_CHECK_HIP(expr)                                                                   \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            grx_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            return GRX_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

#define GRX_REQUIRE(cond, ...)                                                                \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            grx_set_error(__VA_ARGS__);                                                       \
            return GRX_ERR_INVALID;                                                           \
        }                                                                                     \
    } while (0)

#define GRX_LAUNCH_CHECK() GRX_CHECK_HIP(hipGetLastError())

static inline hipStream_t grx_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Per-kernel event timing (grx_profile_* in grx.h).  No-ops unless enabled.
enum GrxKernelId {
    GRX_K_ROW_SUMS = 0, GRX_K_EGONET_WAVE, GRX_K_EGONET_BLOCK, GRX_K_PACK_ROWS, GRX_K_AGGREGATE,
    GRX_K_AGGREGATE_HUB, GRX_K_SORT_COUNT, GRX_K_SORT_SCAN, GRX_K_SORT_SCATTER, GRX_K_BIN_THRESHOLD,
    GRX_K_BIN_ASSIGN, GRX_K_CHEBYSHEV, GRX_K_GATHER_COLUMNS, GRX_K_GRAM, GRX_K_PROJECT,
    GRX_K_NNDSVD_APPLY, GRX_K_NMF_W_PASS, GRX_K_REDUCE_PARTIALS, GRX_K_NMF_H_UPDATE,
    GRX_K_NMF_RESIDUAL, GRX_K_ADD_COLUMNS, GRX_K_TRIANGLES, GRX_K_EGONET_FINISH, GRX_K_QUANT, GRX_K_KEY_BITS,
    GRX_K_SEL_MAP, GRX_K_SEL_HIST, GRX_K_SEL_WALK1, GRX_K_SEL_COLLECT, GRX_K_SEL_SEGSORT, GRX_K_SEL_WALK2, GRX_K_ROLE_ROWS,
    GRX_K_SSSP_ROUND, GRX_K_SSSP_FINISH, GRX_K_WBC_RELAX, GRX_K_WBC_FORWARD, GRX_K_WBC_BACKWARD,
    GRX_K_TRANSFORM_NORMS, GRX_K_NMF_TRANSFORM_BLOCK, GRX_K_COUNT
};
bool grx_prof_is_on();
void grx_prof_begin(int id, hipStream_t st);
void grx_prof_end(int id, hipStream_t st);
struct GrxProfScope {
    int id; hipStream_t st;
    GrxProfScope(int i, hipStream_t s) : id(i), st(s) { grx_prof_begin(id, st); }
    ~GrxProfScope() { grx_prof_end(id, st); }
};
#define GRX_PROF(id, st) GrxProfScope grx_prof_scope_##id(id, st)

// Column-pointer tables travel as kernel arguments (no host->device copy per call).
constexpr int GRX_MAX_PTRS = 128;
struct GrxPtrTable { const void *p[GRX_MAX_PTRS]; };

constexpr int GRX_HUB_FACTOR = 32;  // grx_aggregate: rows longer than lanes_per_row * 32 are hubs
constexpr int GRX_WAVE = 64;       // CDNA4 wavefront
constexpr int GRX_NUM_CU = 256;    // MI355X

static inline int64_t grx_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Small device -> host read-backs the host's next launch depends on (distance matrix of the pruner, Gram matrices,
// residuals), without the copy engine and without an interrupt: a one-workgroup kernel stores the bytes into the
// caller's PINNED host buffer (hipHostMalloc: device-visible) and then a sequence number into a pinned flag; the host
// spins on the flag in its own memory.  hipMemcpyAsync + hipStreamSynchronize takes 18 us, this 14
// (tools/microbench/readback_latency.hip, profiles/r05_readback_latency.json); a step has nine such points.
// grx_fetch_begin queues one copy (any number before a wait); grx_fetch_wait returns when all queued copies of the
// calling thread are in host memory -- like hipStreamSynchronize it implies that everything queued on the stream before
// them has finished.  More than 32 KB, sizes that are not multiples of 4, GRX_READBACK=memcpy: the copy engine.
int grx_fetch_begin(void *h_dst_pinned, const void *d_src, size_t bytes, hipStream_t st);
int grx_fetch_wait(hipStream_t st);
static inline size_t grx_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// One walk over a caller-allocated workspace: every array starts on a 256-byte boundary.  base == NULL: only the sizes
// are wanted and take returns NULL.  `used` ends as the bytes of the workspace.  A file states a layout once, as a
// function of the carver and the shape; its *_workspace_bytes runs that on a NULL base, its entry point on d_workspace.
struct GrxCarve {
    char *base;
    size_t used = 0;
    explicit GrxCarve(void *b) : base(reinterpret_cast<char *>(b)) {}
    template <class T>
    T *take(size_t count)
    {
        T *at = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += grx_align_up(count * sizeof(T), 256);
        return at;
    }
};

// the bytes of the workspace that lay_out(carver, shape...) walks
template <class LayOut, class... Shape>
size_t grx_carve_bytes(LayOut lay_out, Shape... shape)
{
    GrxCarve c(nullptr);
    lay_out(c, shape...);
    return c.used;
}

// Workgroups of a grid-stride launch: one per `per_block` items, at least 1 and at most `cap`.
static inline unsigned grx_grid(int64_t items, int64_t per_block, int64_t cap)
{
    const int64_t g = grx_ceil_div(items, per_block);
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

// Grid-stride stores of one constant into `count` 32-bit / 64-bit words (zeroing doubles and int64 is grx_fill64 with
// 0): 256 threads, grx_grid(count, 256, 2048) workgroups.  Launch only: the caller's GRX_LAUNCH_CHECK covers them.
void grx_fill32(int32_t *d_dst, int64_t count, int32_t value, hipStream_t st);
void grx_fill64(uint64_t *d_dst, int64_t count, uint64_t value, hipStream_t st);

// the CSR a pass pulls over (a relaxation pulls over the in-adjacency to walk the out-arcs from each source)
struct SpPull {
    int64_t n;
    const int64_t *row_ptr;
    const int32_t *col;
    const double *w;                                         // NULL: every weight is 1
    const int32_t *hub_rows;
    int64_t n_hub_rows, hub_degree;
};

// ---- round loops the device steers (BFS levels, peeling rounds, power iterations) -------------------------------
// A loop whose trip count only the device knows keeps a few int32 control words at the end of its workspace.  In every
// layout word 0 is `done` and word 1 the counter (BFS level, peeling layer, iteration count); the BFS loops share the
// three words below, and a file with more words continues its own enum after them (grx_peel.h's PL_* and
// grx_measures.hip's CT_ITERS name words 0 and 1 their own way).  Every kernel of a round returns at once when `done`
// is set, and a one-thread kernel at the end of the round advances the counter or sets `done`.  So the host enqueues
// a fixed batch of rounds without waiting, reads the control words back once per batch (grx_read_ctrl: grx_fetch_begin
// + grx_fetch_wait into one pinned block per host thread, allocated on first use and freed when the thread ends) and
// repeats until `done`: the results are those of a loop that checked after every round.
enum { GRX_CT_DONE = 0, GRX_CT_LEVEL, GRX_CT_FOUND, GRX_CT_BFS_WORDS };
constexpr int GRX_CTRL_MAX_WORDS = 16;   // the pinned block; the widest user has 9 (grx_peel.h)

// out[0 .. words) = d_ctrl[0 .. words) once everything queued on st has finished
int grx_read_ctrl(const int32_t *d_ctrl, int words, int32_t *out, hipStream_t st);

// the one-thread end of a BFS level: `found` set -> level += 1, found = 0; else done = 1 (the level word then holds
// the deepest level reached); nothing once `done` is set
int grx_frontier_advance(int32_t *d_ctrl, hipStream_t st);

// Enqueues `batch` rounds (enqueue_one() launches one round, its advancing kernel last, and returns a GRX_* code),
// reads `words` control words into h and repeats until h[0] (`done`).  Refuses with the caller's message `what` -- a
// format with one %lld, the number of rounds issued -- once more than max_rounds have been issued.
template <class Enqueue>
int grx_run_rounds(const char *what, int batch, int64_t max_rounds, int words, const int32_t *d_ctrl, int32_t *h,
                   hipStream_t st, Enqueue enqueue_one)
{
    for (int k = 0; k < words; ++k) h[k] = 0;
    int64_t issued = 0;
    while (!h[0]) {
        GRX_REQUIRE(issued <= max_rounds, what, (long long)issued);
        for (int k = 0; k < batch; ++k, ++issued) {
            const int rc = enqueue_one();
            if (rc != GRX_OK) return rc;
            GRX_LAUNCH_CHECK();
        }
        const int rc = grx_read_ctrl(d_ctrl, words, h, st);
        if (rc != GRX_OK) return rc;
    }
    return GRX_OK;
}

// ---- entry points below the C ABI that one translation unit offers the others -----------------------------------
// grx_sort.hip.  Workspace of the first and the last: grx_sort_workspace_bytes(n, ncols) resp. (n, 1), laid out as in
// grx_sort_columns; of the pairs form: grx_internal_sort_pairs_workspace_bytes(n).
int grx_internal_sort_columns(int64_t n, int ncols, const double *cols, int64_t ld, double *out, int64_t out_ld,
                              void *workspace, hipStream_t st);
int grx_internal_sort_pairs(int64_t n, const double *col, double *out, uint32_t *perm, void *workspace, hipStream_t st);
size_t grx_internal_sort_pairs_workspace_bytes(int64_t n);
int grx_internal_sort_u64(int64_t n, const uint64_t *keys, uint64_t *out, void *workspace, hipStream_t st);
// grx_prune.hip: grx_vertical_log_bin_typed with a place for the outcome flags (d_status, two words; may be NULL)
int grx_internal_vertical_log_bin(int64_t n, int ncols, const double *d_cols, int64_t ld, const uint8_t *h_is_i64, double frac,
                                  uint8_t *d_bins, int64_t ld_bins, int32_t *d_nbins, void *d_workspace,
                                  size_t workspace_bytes, int32_t *d_status, void *stream);
// grx_aggregate.hip
int64_t grx_internal_plan_max_degree(const grx_aggregate_plan *plan);

// Streams that are read exactly once per launch (the neighbour index list, the oriented arc tables, the output
// columns) can carry the non-temporal hint so that they do not evict the hot rows / hub lists the random gathers of
// the same kernel hit in L2.  MEASURED WITHOUT GAIN on MI355X (round 3, -DGRX_NT_STREAMS=1 against 0: aggregation
// 1.011 vs 0.995 ms per step at BA 1 M, 12.95 vs 12.33 ms at config 5, triangle counting 0.588 vs 0.585): the L2 hit
// rate of these kernels is set by how many gather rows fit (sqrt(C / N) on a power-law graph), not by what the
// streams displace.  Off by default; the macro stays for the next experiment.  (grx_gen0.hip, grx_aggregate.hip)
#ifndef GRX_NT_STREAMS
#define GRX_NT_STREAMS 0
#endif
#if GRX_NT_STREAMS
#define GRX_STREAM_LD(p) __builtin_nontemporal_load(&(p))
#define GRX_STREAM_ST(p, v) __builtin_nontemporal_store((v), &(p))
#else
#define GRX_STREAM_LD(p) (p)
#define GRX_STREAM_ST(p, v) ((p) = (v))
#endif

// Fixed-shape butterfly: every lane ends with the same total, the addition tree depends only
// on WIDTH, so results are bitwise reproducible.
template <int WIDTH>
__device__ __forceinline__ double grx_group_sum(double v)
{
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WIDTH);
    return v;
}

template <int WIDTH>
__device__ __forceinline__ double grx_group_max(double v)
{
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WIDTH));
    return v;
}

// Fixed-tree sum (MAX: maximum) over a workgroup of BLOCK threads in sm[BLOCK]: every thread passes its value and
// every thread gets the result; the tree depends only on BLOCK.  All threads of the workgroup must call it.
template <int BLOCK, bool MAX = false>
__device__ __forceinline__ double grx_block_reduce(double v, double *sm)
{
    const int t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] = MAX ? fmax(sm[t], sm[t + s]) : sm[t] + sm[t + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}
