// grx_runtime.hip -- error state, device info, memory / stream / event helpers of the C ABI.
#include <cstdarg>
#include <cstring>
#include <mutex>
#include <vector>

#include "grx_common.h"
#include <cstdlib>

static thread_local char g_err[1024] = "";

void grx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------------------------------
// per-kernel event timing
// ---------------------------------------------------------------------------------------
namespace {
struct ProfRec { int id; hipEvent_t start, stop; };
bool g_prof_on = false;
unsigned long long g_prof_mask = ~0ull;          // bit id set -> kernel id is timed
std::vector<hipEvent_t> g_prof_pool;             // recycled events (hipEventCreate is not free)
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof_pending;
thread_local hipEvent_t g_prof_open[GRX_K_COUNT];
double g_prof_ms[GRX_K_COUNT];
long long g_prof_cnt[GRX_K_COUNT];
const char *const g_prof_names[GRX_K_COUNT] = {
    "row_sums_kernel", "egonet_kernel<64>", "egonet_kernel<512>", "pack_rows_kernel", "aggregate_kernel",
    "aggregate_hub_kernel", "tile_count_kernel", "scan_kernel", "scatter_kernel", "bin_threshold_kernel",
    "bin_assign_kernel", "chebyshev_kernel", "gather_columns_kernel", "gram_kernel", "project_kernel",
    "nndsvd_apply_kernel", "nmf_w_pass_kernel", "reduce_partials_kernel", "nmf_h_update_kernel",
    "nmf_residual_kernel", "add_columns_kernel", "triangle_count_kernel", "egonet_from_triangles_kernel", "lloyd_max (scan+dp+lloyd+assign)",
    "key_bits_kernel", "sel_map_kernel", "sel_hist_kernel", "sel_walk1_kernel", "sel_collect_kernel", "sel_sort_kernel",
    "sel_walk2_kernel", "role_rows_kernel", "sp_round_kernel (+hub)", "sp_finish_kernel (+source)",
    "wbc relaxation: sp_round_kernel (+hub)", "wb_forward_kernel (+hub)", "wb_backward_kernel (+hub)",
    "transform_norms_kernel", "nmf_transform_block_kernel"};
}  // namespace

static hipEvent_t prof_get_event()
{
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_prof_pool.empty()) { hipEvent_t ev = g_prof_pool.back(); g_prof_pool.pop_back(); return ev; }
    }
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}

bool grx_prof_is_on() { return g_prof_on; }

void grx_prof_begin(int id, hipStream_t st)
{
    if (!g_prof_on || !((g_prof_mask >> id) & 1ull)) return;
    hipEvent_t ev = prof_get_event();
    if (!ev) return;
    (void)hipEventRecord(ev, st);
    g_prof_open[id] = ev;
}

void grx_prof_end(int id, hipStream_t st)
{
    if (!g_prof_on || g_prof_open[id] == nullptr) return;
    hipEvent_t ev = prof_get_event();
    if (!ev) return;
    (void)hipEventRecord(ev, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_pending.push_back({id, g_prof_open[id], ev});
    g_prof_open[id] = nullptr;
}

// one-thread kernel whose only purpose is its name in a rocprofv3 kernel trace (grx_trace_marker)
__global__ void grx_marker_kernel(int tag, int *sink)
{
    if (sink && tag == 0x7fffffff) *sink = tag;
}

// ---- read-backs through mapped host memory (grx_common.h) ----------------------------------------------------
namespace {

__global__ __launch_bounds__(256) void publish_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ host_dst, int words,
                                                      volatile uint32_t *flag, uint32_t seq)
{
    for (int i = threadIdx.x; i < words; i += 256) host_dst[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) { *flag = seq; __threadfence_system(); }
}

struct FetchState {
    uint32_t *h_flag = nullptr, *d_flag = nullptr;
    uint32_t seq = 0;
    bool flag_pending = false, sync_pending = false;
    int mode = -1;                                              // 1: mapped flag, 0: copy engine
    ~FetchState() { if (h_flag) (void)hipHostFree(h_flag); }
};
thread_local FetchState g_fetch;

}  // namespace

int grx_fetch_begin(void *h_dst_pinned, const void *d_src, size_t bytes, hipStream_t st)
{
    FetchState &f = g_fetch;
    if (f.mode < 0) {
        const char *e = std::getenv("GRX_READBACK");
        f.mode = (e && e[0] == 'm') ? 0 : 1;                    // GRX_READBACK=memcpy
        if (f.mode == 1) {
            void *h = nullptr, *d = nullptr;
            if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
                f.h_flag = reinterpret_cast<uint32_t *>(h);
                f.d_flag = reinterpret_cast<uint32_t *>(d);
                *f.h_flag = 0;
            } else {
                if (h) (void)hipHostFree(h);
                (void)hipGetLastError();
                f.mode = 0;
            }
        }
    }
    if (bytes == 0) return GRX_OK;
    void *d_dst = nullptr;
    if (f.mode == 1 && bytes <= (32u << 10) && bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(d_src) & 3) == 0 &&
        hipHostGetDevicePointer(&d_dst, h_dst_pinned, 0) == hipSuccess) {
        ++f.seq;
        if (f.seq == 0) f.seq = 1;
        publish_kernel<<<1, 256, 0, st>>>(reinterpret_cast<const uint32_t *>(d_src), reinterpret_cast<uint32_t *>(d_dst),
                                          (int)(bytes / 4), f.d_flag, f.seq);
        GRX_LAUNCH_CHECK();
        f.flag_pending = true;
        return GRX_OK;
    }
    (void)hipGetLastError();                                     // (a buffer that is not device-visible: the copy engine)
    GRX_CHECK_HIP(hipMemcpyAsync(h_dst_pinned, d_src, bytes, hipMemcpyDeviceToHost, st));
    f.sync_pending = true;
    return GRX_OK;
}

int grx_fetch_wait(hipStream_t st)
{
    FetchState &f = g_fetch;
    if (f.sync_pending) {                                       // a copy-engine copy is among them: wait for the stream
        GRX_CHECK_HIP(hipStreamSynchronize(st));
        f.sync_pending = f.flag_pending = false;
        return GRX_OK;
    }
    if (!f.flag_pending) return GRX_OK;
    f.flag_pending = false;
    const uint32_t want = f.seq;
    for (uint64_t spins = 1;; ++spins) {
        if (__atomic_load_n(f.h_flag, __ATOMIC_ACQUIRE) == want) return GRX_OK;
        __builtin_ia32_pause();
        if ((spins & 0xFFFF) == 0) {
            // every ~100 us: has the stream failed, or finished without the flag arriving?
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) {
                if (__atomic_load_n(f.h_flag, __ATOMIC_ACQUIRE) == want) return GRX_OK;
                grx_set_error("grx_fetch_wait: the stream is idle and the read-back flag never arrived");
                return GRX_ERR_HIP;
            }
            if (q != hipErrorNotReady) {
                grx_set_error("grx_fetch_wait: %s", hipGetErrorString(q));
                return GRX_ERR_HIP;
            }
        }
    }
}

// ---- control words of the device-steered round loops, constant fills (grx_common.h) ----------------------------
namespace {

constexpr int FILL_BLOCK = 256;
constexpr int FILL_MAX_BLOCKS = 2048;

template <class T>
__global__ __launch_bounds__(FILL_BLOCK) void grx_fill_kernel(int64_t count, T *__restrict__ a, T value)
{
    for (int64_t i = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * FILL_BLOCK)
        a[i] = value;
}

__global__ void grx_frontier_advance_kernel(int32_t *__restrict__ ctrl)
{
    if (ctrl[GRX_CT_DONE]) return;
    if (ctrl[GRX_CT_FOUND]) {
        ctrl[GRX_CT_LEVEL] += 1;
        ctrl[GRX_CT_FOUND] = 0;
    } else {
        ctrl[GRX_CT_DONE] = 1;
    }
}

struct PinnedCtrl {
    int32_t *h = nullptr;
    ~PinnedCtrl() { if (h) (void)hipHostFree(h); }
};
thread_local PinnedCtrl g_ctrl;

}  // namespace

void grx_fill32(int32_t *d_dst, int64_t count, int32_t value, hipStream_t st)
{
    grx_fill_kernel<<<grx_grid(count, FILL_BLOCK, FILL_MAX_BLOCKS), FILL_BLOCK, 0, st>>>(count, d_dst, value);
}

void grx_fill64(uint64_t *d_dst, int64_t count, uint64_t value, hipStream_t st)
{
    grx_fill_kernel<<<grx_grid(count, FILL_BLOCK, FILL_MAX_BLOCKS), FILL_BLOCK, 0, st>>>(count, d_dst, value);
}

int grx_frontier_advance(int32_t *d_ctrl, hipStream_t st)
{
    grx_frontier_advance_kernel<<<1, 1, 0, st>>>(d_ctrl);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_read_ctrl(const int32_t *d_ctrl, int words, int32_t *out, hipStream_t st)
{
    GRX_REQUIRE(words >= 1 && words <= GRX_CTRL_MAX_WORDS, "grx_read_ctrl: %d control words", words);
    if (!g_ctrl.h) {
        void *h = nullptr;
        GRX_CHECK_HIP(hipHostMalloc(&h, GRX_CTRL_MAX_WORDS * sizeof(int32_t), hipHostMallocMapped));
        g_ctrl.h = reinterpret_cast<int32_t *>(h);
    }
    int rc = grx_fetch_begin(g_ctrl.h, d_ctrl, (size_t)words * sizeof(int32_t), st);
    if (rc == GRX_OK) rc = grx_fetch_wait(st);
    if (rc != GRX_OK) return rc;
    for (int k = 0; k < words; ++k) out[k] = g_ctrl.h[k];
    return GRX_OK;
}

extern "C" {

int grx_trace_marker(int tag, void *stream)
{
    grx_marker_kernel<<<1, 1, 0, grx_stream(stream)>>>(tag, nullptr);
    GRX_LAUNCH_CHECK();
    return GRX_OK;
}

int grx_profile_enable(int on)
{
    g_prof_on = on != 0;
    return GRX_OK;
}

int grx_profile_enabled(void) { return g_prof_on ? 1 : 0; }

int grx_profile_select(uint64_t kernel_mask)
{
    g_prof_mask = kernel_mask ? kernel_mask : ~0ull;
    return GRX_OK;
}

int grx_profile_reset(void)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof_pending) { g_prof_pool.push_back(r.start); g_prof_pool.push_back(r.stop); }
    g_prof_pending.clear();
    for (int i = 0; i < GRX_K_COUNT; ++i) { g_prof_ms[i] = 0.0; g_prof_cnt[i] = 0; }
    return GRX_OK;
}

int grx_profile_kernel_count(void) { return GRX_K_COUNT; }

const char *grx_profile_kernel_name(int id)
{
    return (id >= 0 && id < GRX_K_COUNT) ? g_prof_names[id] : "";
}

int grx_profile_read(int id, double *total_ms, long long *launches)
{
    GRX_REQUIRE(id >= 0 && id < GRX_K_COUNT, "grx_profile_read: bad kernel id %d", id);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof_pending) {
        GRX_CHECK_HIP(hipEventSynchronize(r.stop));
        float ms = 0.f;
        GRX_CHECK_HIP(hipEventElapsedTime(&ms, r.start, r.stop));
        g_prof_ms[r.id] += ms;
        g_prof_cnt[r.id] += 1;
        g_prof_pool.push_back(r.start);
        g_prof_pool.push_back(r.stop);
    }
    g_prof_pending.clear();
    if (total_ms) *total_ms = g_prof_ms[id];
    if (launches) *launches = g_prof_cnt[id];
    return GRX_OK;
}

int grx_version(void) { return GRX_VERSION; }

const char *grx_last_error(void) { return g_err; }

int grx_device_info(int *cu_count, int *wave_size, char *arch_buf, size_t arch_buf_len)
{
    int dev = 0;
    GRX_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    GRX_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (wave_size) *wave_size = prop.warpSize;
    if (arch_buf && arch_buf_len) {
        strncpy(arch_buf, prop.gcnArchName, arch_buf_len - 1);
        arch_buf[arch_buf_len - 1] = 0;
    }
    return GRX_OK;
}

int grx_dev_malloc(void **d_out, size_t bytes)
{
    GRX_REQUIRE(d_out != nullptr, "grx_dev_malloc: d_out is NULL");
    GRX_CHECK_HIP(hipMalloc(d_out, bytes ? bytes : 1));
    return GRX_OK;
}

int grx_dev_free(void *d_ptr)
{
    GRX_CHECK_HIP(hipFree(d_ptr));
    return GRX_OK;
}

int grx_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream)
{
    GRX_CHECK_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, grx_stream(stream)));
    return GRX_OK;
}

int grx_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream)
{
    GRX_CHECK_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, grx_stream(stream)));
    return GRX_OK;
}

int grx_memset(void *d_dst, int value, size_t bytes, void *stream)
{
    GRX_CHECK_HIP(hipMemsetAsync(d_dst, value, bytes, grx_stream(stream)));
    return GRX_OK;
}

int grx_stream_sync(void *stream)
{
    GRX_CHECK_HIP(hipStreamSynchronize(grx_stream(stream)));
    return GRX_OK;
}

int grx_event_create(void **event_out)
{
    GRX_REQUIRE(event_out != nullptr, "grx_event_create: NULL");
    hipEvent_t ev;
    GRX_CHECK_HIP(hipEventCreate(&ev));
    *event_out = ev;
    return GRX_OK;
}

int grx_event_destroy(void *event)
{
    GRX_CHECK_HIP(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)));
    return GRX_OK;
}

int grx_event_record(void *event, void *stream)
{
    GRX_CHECK_HIP(hipEventRecord(reinterpret_cast<hipEvent_t>(event), grx_stream(stream)));
    return GRX_OK;
}

int grx_event_elapsed_ms(void *start, void *stop, float *ms_out)
{
    GRX_REQUIRE(ms_out != nullptr, "grx_event_elapsed_ms: NULL");
    GRX_CHECK_HIP(hipEventSynchronize(reinterpret_cast<hipEvent_t>(stop)));
    GRX_CHECK_HIP(hipEventElapsedTime(ms_out, reinterpret_cast<hipEvent_t>(start),
                                      reinterpret_cast<hipEvent_t>(stop)));
    return GRX_OK;
}

}  // extern "C"
