// kq_api.hip — C-ABI of libggml_mi355x.so: the device probe, the debug knobs, the launch-timing
// log, per-kernel occupancy and LDS opt-in, and the extern "C" functions (argument checking, the
// ggml-surface mirrors vec_dot / from_float / mul_mat). Declared in include/ggml_mi355x.h. The
// decode GEMVs' planners and launches are in kq_gemv_host.hip, the prefill GEMMs' in
// kq_prefill_host.hip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "kq_common.h"
#include "kq_internal.h"

namespace kq {

__global__ void kq_stream_ceiling(const uint8_t *buf, int64_t per_wave, int waves_total, uint32_t *sink);

namespace {

// Per-device probe (the caller's current device): 0 unknown, 1 gfx950, -1 not usable.
// A process may drive several devices (one backend each), so nothing here is cached
// for "the" device.
constexpr int kMaxDevices = 64;
std::mutex g_dev_mu;
std::atomic<int> g_dev_state[kMaxDevices];
int g_dev_cus[kMaxDevices] = {0};

int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return -1;
    return dev;
}

void probe_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || dev >= n) {
        g_dev_state[dev].store(-1);
        return;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        g_dev_state[dev].store(-1);
        return;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "ggml_mi355x: device %d is %s, this library is built for gfx950 only\n", dev,
                prop.gcnArchName);
        g_dev_state[dev].store(-1);
        return;
    }
    g_dev_cus[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    g_dev_state[dev].store(1, std::memory_order_release);
}

// ------------------------------------------------------------------ debug knobs
// Product defaults; mi355x_debug_knob() (tools / A/B runs) overrides them per process.
struct KnobDef {
    const char *name;
    double def;
};
const KnobDef kKnobs[KNOB_COUNT] = {
    {"GEMV_DIAG", 0},  {"GEMV_RING", 0},     {"GEMV_PRE0", 1},
    {"GEMV_SMALL_MB", kRowsSmallBytes / 1e6},      {"GEMV_WPC", 0},
    {"GEMV_SMALL_WG", 0}, {"GEMV_FQMAX", (double)kRowsFusedMaxNb},   {"MMF_WAVES", 0},
    {"MMF_ORDER", 0},  {"ATTN_DIAG", 0},     {"LOOPBACK_NOCOPY", 0}, {"ATTN_OPROJ", 1},
    {"AO_NRB", 0},     {"GEMV_DYN", 8},    {"GEMV_DYN_P", 0},      {"GEMV_DYN_STEPS", 16},
    {"GEMV_SHORT", 1}, {"ATTN_STREAM", -1},  {"ATTN_STREAM_TILE", 0},
    {"ARGMAX_SLICE", 0}, {"MMQ_ID_Q6", 0},
};
std::atomic<double> g_knob[KNOB_COUNT];
std::atomic<bool> g_knob_set[KNOB_COUNT];
std::atomic<uint32_t> g_knob_gen{0};


uint64_t *g_stamps = nullptr;  // diagnostics (mi355x_diag_stamps)
int64_t g_stamps_cap = 0;

// Workgroups of one kernel resident per CU (registers / LDS), cached per
// (device, fn, lds): function attributes are set per device.
struct OccKey {
    int dev;
    const void *fn;
    size_t lds;
};
}  // namespace

int resident_wgs(const void *fn, size_t lds) {
    static std::mutex mu;
    static std::vector<std::pair<OccKey, int>> cache;
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : cache)
        if (e.first.dev == dev && e.first.fn == fn && e.first.lds == lds) return e.second;
    int n = 0;
    if (lds > 64 * 1024) hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, WG_THREADS, lds) != hipSuccess || n <= 0) n = 1;
    if (n > 8) n = 8;
    cache.push_back({{dev, fn, lds}, n});
    return n;
}

double knob(Knob k) { return g_knob_set[k].load(std::memory_order_relaxed) ? g_knob[k].load() : kKnobs[k].def; }
uint32_t knob_generation() { return g_knob_gen.load(); }

// ------------------------------------------------------------ launch timing
struct TimedLaunch {
    std::string kernel;
    double bytes;
    hipEvent_t start, stop;
};
std::mutex g_tmu;
bool g_timing = false;
std::vector<TimedLaunch> g_tlog;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_tpool;
size_t g_tpool_used = 0;

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) return false;
    return st != hipStreamCaptureStatusNone;
}

// Returns true (and the events) when this launch should be timed.
bool timing_slot(hipStream_t s, hipEvent_t &a, hipEvent_t &b) {
    std::lock_guard<std::mutex> lk(g_tmu);
    if (!g_timing || capturing(s)) return false;
    if (g_tpool_used == g_tpool.size()) {
        hipEvent_t e0, e1;
        if (hipEventCreate(&e0) != hipSuccess) return false;
        if (hipEventCreate(&e1) != hipSuccess) {
            hipEventDestroy(e0);
            return false;
        }
        g_tpool.push_back({e0, e1});
    }
    a = g_tpool[g_tpool_used].first;
    b = g_tpool[g_tpool_used].second;
    ++g_tpool_used;
    return true;
}

void timing_log(const std::string &kernel, double bytes, hipEvent_t a, hipEvent_t b) {
    std::lock_guard<std::mutex> lk(g_tmu);
    g_tlog.push_back({kernel, bytes, a, b});
}

int device_ok() {
    const int dev = current_device();
    if (dev < 0) return 0;
    const int st = g_dev_state[dev].load(std::memory_order_acquire);
    if (st) return st > 0;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (g_dev_state[dev].load() == 0) probe_device(dev);
    return g_dev_state[dev].load() > 0;
}

int num_cus() {
    if (!device_ok()) return 256;
    return g_dev_cus[current_device()];
}

// Dynamic LDS above 64 KB must be opted into per kernel.
void allow_lds(const void *fn, size_t lds) {
    if (lds <= 64 * 1024) return;
    static std::mutex mu;
    static std::vector<std::pair<int, const void *>> done;  // (device, fn): set per device
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : done)
        if (e.first == dev && e.second == fn) return;
    hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    done.push_back({dev, fn});
}

uint64_t api_selector_key() {
    return (uint64_t)(uint32_t)(gemv_impl_select(-1) + 1) | ((uint64_t)(uint32_t)rows_waves_select(-1) << 8) |
           ((uint64_t)(uint32_t)(mmq_impl() + 1) << 16) | ((uint64_t)(uint32_t)(prefill_precision() + 1) << 24) |
           ((uint64_t)knob_generation() << 32);
}

}  // namespace kq

using namespace kq;

extern "C" {

size_t mi355x_row_size(int type, int64_t k) {
    if (k < 0 || k % QK) return 0;
    const int64_t nb = k / QK;
    if (type == MI355X_TYPE_Q8_K) return (size_t)(nb * 292);
    if (type == MI355X_TYPE_F32) return (size_t)(k * 4);
    return (size_t)(nb * block_bytes(type));
}

const char *mi355x_version(void) { return "ggml-mi355x 0.1.0 (gfx950, wave64, K-quant GEMV)"; }

int mi355x_device_available(void) { return device_ok(); }

int mi355x_quantize_q8_K(const float *x, size_t x_stride, void *y, int64_t k, int64_t nrows, void *stream) {
    if (k <= 0 || k % QK || nrows < 0) return MI355X_E_INVAL;
    if (nrows == 0) return MI355X_OK;
    if (!x || !y || (x_stride & 3u) || ((uintptr_t)x & 3u) || ((uintptr_t)y & 3u)) return MI355X_E_INVAL;
    if (nrows > 1 && x_stride < (size_t)k * 4) return MI355X_E_INVAL;
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_quantize(x, (int64_t)(x_stride / 4), y, k, nrows, (hipStream_t)stream);
}

static void die(const char *fn, const char *msg) {
    fprintf(stderr, "%s: %s\n", fn, msg);
    abort();
}

// ---- the trait-table surface (ggml_vec_dot_t / ggml_from_float_t): called by
// ggml-cpu's mul_mat from nth threads at once with HOST pointers into its own buffers
// (src0 rows, params->wdata; README.md:121-137, :449), or with device pointers. Each
// calling thread owns a non-blocking stream on its current device plus device staging;
// host operands are copied in, results copied out, and only that stream is synchronized,
// so concurrent callers never serialize on the default stream or share a buffer.
namespace {
struct ThreadCtx {
    int dev = -1;
    hipStream_t st = nullptr;
    void *buf = nullptr;
    size_t cap = 0;
    ~ThreadCtx() {
        if (buf) hipFree(buf);
        if (st) hipStreamDestroy(st);
    }
};
thread_local ThreadCtx t_ctx;

ThreadCtx *thread_ctx(size_t need) {
    ThreadCtx &c = t_ctx;
    const int dev = current_device();
    if (c.dev != dev) {  // the thread moved to another device: new stream and staging there
        if (c.buf) hipFree(c.buf);
        if (c.st) hipStreamDestroy(c.st);
        c.buf = nullptr;
        c.st = nullptr;
        c.cap = 0;
        c.dev = -1;
        if (hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking) != hipSuccess) return nullptr;
        c.dev = dev;
    }
    if (need > c.cap) {
        if (c.buf) hipFree(c.buf);
        c.buf = nullptr;
        c.cap = 0;
        if (hipMalloc(&c.buf, need) != hipSuccess) return nullptr;
        c.cap = need;
    }
    return &c;
}

// True when p is device-accessible memory of the current device (hipMalloc / managed).
// A buffer of another GPU is foreign here: it is staged like host memory (a peer copy),
// never read in place by a kernel of this device.
bool on_device(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // plain pageable host memory: not an error to keep
        return false;
    }
    if (at.type == hipMemoryTypeManaged) return true;
    return at.type == hipMemoryTypeDevice && at.device == current_device();
}
}  // namespace

void mi355x_quantize_row_q8_K(const float *x, void *y, int64_t k) {
    if (k % QK) die(__func__, "k % QK_K != 0");
    if (k == 0) return;
    if (!device_ok()) die(__func__, "no gfx950 device");
    const size_t xb = (size_t)k * 4, yb = (size_t)(k / QK) * 292;
    const bool xd = on_device(x), yd = on_device(y);
    ThreadCtx *c = thread_ctx(((xd ? 0 : xb + 16) + (yd ? 0 : yb) + 255) & ~(size_t)255);
    if (!c) die(__func__, "stream / staging allocation failed");
    const float *dx = x;
    void *dy = y;
    uint8_t *stage = (uint8_t *)c->buf;
    if (!xd) {
        if (hipMemcpyAsync(stage, x, xb, hipMemcpyDefault, c->st) != hipSuccess) die(__func__, "copy in failed");
        dx = (const float *)stage;
        stage += (xb + 15) & ~(size_t)15;
    }
    if (!yd) dy = stage;
    if (mi355x_quantize_q8_K(dx, xb, dy, k, 1, c->st)) die(__func__, "launch failed");
    if (!yd && hipMemcpyAsync(y, dy, yb, hipMemcpyDefault, c->st) != hipSuccess) die(__func__, "copy out failed");
    if (hipStreamSynchronize(c->st) != hipSuccess) die(__func__, "hipStreamSynchronize failed");
}

size_t mi355x_mul_mat_workspace_size(int src0_type, int64_t ne00, int64_t ne01, int64_t ne11) {
    if (!block_bytes(src0_type) || ne00 <= 0 || ne00 % QK || ne11 < 0) return 0;
    if (ne11 == 0 || (ne11 == 1 && ne00 / QK <= kFusedQMaxNb)) return 0;
    size_t bytes = (size_t)ne11 * (size_t)(ne00 / QK) * Q8L_STRIDE;  // >= raw 292-B blocks
    // the f16 prefill path runs instead at ne11 >= 16 once mi355x_prefill_precision selects it
    // (its image and split-K slabs; callers re-query after switching)
    if (ne11 >= kMmqMinCols && ne01 > 0 && prefill_precision() >= MI355X_PREFILL_F16) {
        const size_t f = mmf_workspace(ne01, ne11, ne00 / QK);
        bytes = f > bytes ? f : bytes;
    }
    return (bytes + 255) & ~(size_t)255;
}

size_t mi355x_gemv_fused_workspace_size(int64_t k) {
    if (k <= 0 || k % QK || k / QK <= kFusedQMaxNb) return 0;
    return ((size_t)(k / QK) * Q8L_STRIDE + 255) & ~(size_t)255;
}

int mi355x_mul_mat_q8(int src0_type, const void *src0, int64_t ne00, int64_t ne01, size_t nb01,
                      const void *src1_q8, int64_t ne11, size_t nb11, float *dst, size_t nb1, void *stream) {
    if (ne11 < 0 || ne01 < 0) return MI355X_E_INVAL;
    if (ne11 == 0 || ne01 == 0) return MI355X_OK;
    if (!src1_q8 || ((uintptr_t)src1_q8 & 3u) || (nb11 & 3u) || ((uintptr_t)dst & 3u) || (nb1 & 3u))
        return MI355X_E_INVAL;
    if (ne00 <= 0 || ne00 % QK) return MI355X_E_INVAL;
    if (ne11 > 1 && (nb11 < (size_t)(ne00 / QK) * 292 || nb1 < (size_t)ne01 * 4)) return MI355X_E_INVAL;
    if (ne11 > 0x7fffffff) return MI355X_E_INVAL;
    mi355x_gemv_desc d = {src0_type, src0, ne01, nb01, dst};
    const int ncol = choose_ncol(ne11, (int)(ne00 / QK));
    GemvPlan pl;
    int rc = plan_gemv(&d, 1, ne00, ne11, ncol, false, false, pl);
    if (rc) return rc;
    pl.a.xq = (const uint8_t *)src1_q8;
    pl.a.xq_col_stride = (int64_t)nb11;
    pl.a.y_col_stride[0] = (int64_t)(nb1 / 4);
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_gemv(pl, (hipStream_t)stream);
}

int mi355x_mul_mat(int src0_type, const void *src0, int64_t ne00, int64_t ne01, size_t nb01, const float *src1,
                   int64_t ne11, size_t nb11, float *dst, size_t nb1, void *workspace, size_t workspace_size,
                   void *stream) {
    if (ne11 < 0 || ne01 < 0 || ne00 <= 0 || ne00 % QK) return MI355X_E_INVAL;
    if (!block_bytes(src0_type)) return MI355X_E_UNSUPPORTED;
    if (ne11 == 0 || ne01 == 0) return MI355X_OK;
    if (!src1 || ((uintptr_t)src1 & 3u) || (nb11 & 3u) || !dst || ((uintptr_t)dst & 3u) || (nb1 & 3u))
        return MI355X_E_INVAL;
    if (ne11 > 1 && (nb11 < (size_t)ne00 * 4 || nb1 < (size_t)ne01 * 4)) return MI355X_E_INVAL;
    if (ne11 == 1) {
        mi355x_gemv_desc d = {src0_type, src0, ne01, nb01, dst};
        return gemv_m1(&d, 1, src1, ne00, workspace, workspace_size, (hipStream_t)stream);
    }
    size_t need = mi355x_mul_mat_workspace_size(src0_type, ne00, ne01, ne11);
    if (!workspace || workspace_size < need) return MI355X_E_WORKSPACE;
    if (mmf_applies(src0_type, src0, ne01, nb01, ne11, ne00) && ((uintptr_t)workspace & 15u) == 0) {
        if (!device_ok()) return MI355X_E_NODEVICE;
        int rc = launch_f16img(src1, (int64_t)(nb11 / 4), (uint8_t *)workspace, ne00, ne11, (hipStream_t)stream);
        if (rc) return rc;
        return launch_mmf_gemm(src0_type, src0, ne00, ne01, nb01, (uint8_t *)workspace, ne11, dst, (int64_t)(nb1 / 4),
                               (hipStream_t)stream);
    }
    if (mmq_applies(src0_type, src0, ne01, nb01, ne11) && ((uintptr_t)workspace & 15u) == 0) {
        if (!device_ok()) return MI355X_E_NODEVICE;
        int rc = launch_quantize_q8L(src1, (int64_t)(nb11 / 4), workspace, ne00, ne11, (hipStream_t)stream, true);
        if (rc) return rc;
        return launch_mmq(src0_type, src0, ne00, ne01, nb01, (const uint8_t *)workspace, ne11, dst,
                          (int64_t)(nb1 / 4), (hipStream_t)stream);
    }
    if (!device_ok()) return MI355X_E_NODEVICE;
    int rc = launch_quantize(src1, (int64_t)(nb11 / 4), workspace, ne00, ne11, (hipStream_t)stream);
    if (rc) return rc;
    const size_t q8_row = (size_t)(ne00 / QK) * 292;
    return mi355x_mul_mat_q8(src0_type, src0, ne00, ne01, nb01, workspace, ne11, q8_row, dst, nb1, stream);
}

int mi355x_gemv_fused(const mi355x_gemv_desc *descs, int n_desc, const float *x, int64_t k, void *workspace,
                      size_t workspace_size, void *stream) {
    if (!descs || !x || ((uintptr_t)x & 3u)) return MI355X_E_INVAL;
    if (k <= 0 || k % QK) return MI355X_E_INVAL;
    for (int i = 0; i < n_desc && i < MI355X_MAX_FUSED; ++i)
        if (descs[i].y && ((uintptr_t)descs[i].y & 3u)) return MI355X_E_INVAL;
    return gemv_m1(descs, n_desc, x, k, workspace, workspace_size, (hipStream_t)stream);
}

size_t mi355x_gemv_ext_workspace_size(int64_t k) {
    if (k <= 0 || k % QK) return 0;
    return ext_x_bytes(k) + mi355x_gemv_fused_workspace_size(k);
}

int mi355x_gemv_fused_ext(const mi355x_gemv_desc *descs, int n_desc, const float *x, int64_t k,
                          const mi355x_gemv_ext *ext, void *workspace, size_t workspace_size, void *stream) {
    if (!descs || !x || ((uintptr_t)x & 3u)) return MI355X_E_INVAL;
    if (k <= 0 || k % QK || n_desc < 1 || n_desc > MI355X_MAX_FUSED) return MI355X_E_INVAL;
    if (ext && (ext->prologue < MI355X_PRO_NONE || ext->prologue > MI355X_PRO_SWIGLU)) return MI355X_E_INVAL;
    if (ext && ext->prologue == MI355X_PRO_RMS_NORM && !(ext->eps >= 0.0f)) return MI355X_E_INVAL;
    if (ext && ext->epilogue == MI355X_EPI_SWIGLU && ((uintptr_t)ext->epi_y & 3u)) return MI355X_E_INVAL;
    for (int i = 0; i < n_desc; ++i) {
        if (descs[i].y && ((uintptr_t)descs[i].y & 3u)) return MI355X_E_INVAL;
        if (ext && ext->residual[i] && ((uintptr_t)ext->residual[i] & 3u)) return MI355X_E_INVAL;
    }
    return gemv_m1(descs, n_desc, x, k, workspace, workspace_size, (hipStream_t)stream, ext);
}

int mi355x_debug_stream(const void *buf, size_t bytes, void *sink, void *stream) {
    if (!buf || !sink || ((uintptr_t)buf & 15u)) return MI355X_E_INVAL;
    int dev = current_device();
    if (dev < 0 || !device_ok()) return MI355X_E_NODEVICE;
    const int cus = g_dev_cus[dev] > 0 ? g_dev_cus[dev] : 256;
    const int waves = cus * 12;
    const int64_t per_wave = (int64_t)(bytes / waves) / 2048 * 2048;
    if (per_wave <= 0) return MI355X_E_INVAL;
    const size_t lds = 4 * 4 * 2048;
    allow_lds((const void *)kq_stream_ceiling, lds);
    return timed_launch("kq::kq_stream_ceiling", (double)per_wave * waves, kq_stream_ceiling, dim3((unsigned)(cus * 3)),
                        dim3(256), lds, (hipStream_t)stream, (const uint8_t *)buf, per_wave, waves, (uint32_t *)sink);
}

int mi355x_rows_prologue_plan(int64_t k, int waves, int64_t steps, int *lanes, int *passes) {
    if (k <= 0 || k % QK || waves < 1 || waves > ROWS_WAVES || steps < 0) return MI355X_E_INVAL;
    const int64_t nb = k / QK;
    if (nb > kRowsFusedMaxNb) return MI355X_E_UNSUPPORTED;
    const RowsProForm f = rows_pro_form((int)nb, waves, steps);
    if (f.passes > ROWS_QPASS) return MI355X_E_UNSUPPORTED;  // (plan_rows runs such a row on ROWS_WAVES waves)
    if (lanes) *lanes = 16 << f.lsh;
    if (passes) *passes = f.passes;
    return MI355X_OK;
}

// Descriptors of n contiguous matrices for the plan-only entries (n in range, k checked here).
// The plan reads no weights: a placeholder address with the alignment of a GGUF tensor.
static int placeholder_descs(const int *types, const int64_t *n_rows, int n, int64_t k, mi355x_gemv_desc *d) {
    alignas(16) static const uint8_t dummy_w[16] = {0};
    static float dummy_y;
    if (k <= 0 || k % QK) return MI355X_E_INVAL;
    for (int i = 0; i < n; ++i) {
        const int bb = block_bytes(types[i]);
        if (!bb) return MI355X_E_UNSUPPORTED;
        d[i] = {types[i], dummy_w, n_rows[i], (size_t)(k / QK) * bb, &dummy_y};
    }
    return MI355X_OK;
}

int mi355x_rows_stream_plan(const int *types, const int64_t *n_rows, int n, int64_t k, int batch_rows, int *steps,
                            int *depth, int *form) {
    if (!types || !n_rows || n < 1 || n > MI355X_MAX_FUSED || batch_rows < 0) return MI355X_E_INVAL;
    mi355x_gemv_desc d[MI355X_MAX_FUSED];
    int rc = placeholder_descs(types, n_rows, n, k, d);
    if (rc) return rc;
    if (k / QK > kRowsFusedMaxNb) return MI355X_E_UNSUPPORTED;
    RowsPlan pl;
    rc = plan_rows(d, n, k, true, ROWS_PRO_NONE, pl);
    if (rc) return rc;
    if (batch_rows > 0 && batch_rows < pl.a.bR)  // a smaller chain batch than the plan's
        pl.sh = pl.sh && rows_short_form(pl.steps, pl.depth, batch_rows, pl.a.rpw);
    if (steps) *steps = pl.steps;
    if (depth) *depth = pl.depth;
    if (form) *form = pl.dyn ? MI355X_ROWS_CLAIMED : pl.sh ? MI355X_ROWS_SHORT : MI355X_ROWS_LONG;
    return MI355X_OK;
}

int mi355x_debug_rows_plan(const int *types, const int64_t *n_rows, int n, int64_t k, int fusedq, int prologue,
                           int64_t *out, int cap) {
    if (!types || !n_rows || !out || n < 1 || n > MI355X_MAX_FUSED || cap < MI355X_ROWS_PLAN_FIELDS) return MI355X_E_INVAL;
    if (prologue < MI355X_PRO_NONE || prologue > MI355X_PRO_SWIGLU) return MI355X_E_INVAL;
    if (!fusedq && prologue != MI355X_PRO_NONE) return MI355X_E_INVAL;  // the fused prologue is the fused quantizer's
    mi355x_gemv_desc d[MI355X_MAX_FUSED];
    int rc = placeholder_descs(types, n_rows, n, k, d);
    if (rc) return rc;
    RowsPlan pl;
    rc = plan_rows(d, n, k, fusedq != 0, rows_pro_kind(prologue), pl);
    if (rc) return rc;
    const RowsArgs &a = pl.a;
    int64_t *o = out;
    *o++ = pl.tmask, *o++ = pl.nwv, *o++ = pl.grid.x, *o++ = (int64_t)pl.lds, *o++ = pl.lsh, *o++ = pl.sh, *o++ = pl.dyn;
    *o++ = pl.steps, *o++ = pl.depth, *o++ = a.waves_total;
    for (int i = 0; i <= MI355X_MAX_FUSED; ++i) *o++ = a.wave_prefix[i];
    for (int i = 0; i < MI355X_MAX_FUSED; ++i) *o++ = a.rbase[i];
    for (int i = 0; i < MI355X_MAX_FUSED; ++i) *o++ = a.rrem[i];
    *o++ = a.rpw, *o++ = a.bR, *o++ = a.prio_bytes, *o++ = a.pre0, *o++ = a.dyn_u, *o++ = a.dyn_ush, *o++ = a.dyn_p;
    *o++ = rows_kernel_id(pl.fn);
    return (int)(o - out);
}

int mi355x_debug_rows_prologue(int prologue, const float *x, const float *x2, float eps, int64_t k, int waves, void *out,
                               size_t out_bytes, void *stream) {
    if (!x || !out || ((uintptr_t)x & 15u) || ((uintptr_t)out & 15u)) return MI355X_E_INVAL;
    if (prologue < MI355X_PRO_NONE || prologue > MI355X_PRO_SWIGLU) return MI355X_E_INVAL;
    if (prologue != MI355X_PRO_NONE && (!x2 || ((uintptr_t)x2 & 15u))) return MI355X_E_INVAL;
    if (prologue == MI355X_PRO_RMS_NORM && !(eps >= 0.0f)) return MI355X_E_INVAL;
    const int rc = mi355x_rows_prologue_plan(k, waves, 0, nullptr, nullptr);
    if (rc) return rc;
    const int64_t nb = k / QK;
    if (out_bytes < (size_t)nb * Q8L_STRIDE) return MI355X_E_INVAL;
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_rows_prologue_dbg(rows_pro_kind(prologue), x, x2, eps, (int)nb, waves, (uint8_t *)out, (hipStream_t)stream);
}

int mi355x_debug_block_partials(int src0_type, const void *src0, int64_t ne00, int64_t ne01, size_t nb01,
                                const void *src1_q8, int32_t *out, void *stream) {
    if (!out || !src1_q8 || ((uintptr_t)src1_q8 & 3u)) return MI355X_E_INVAL;
    if (ne01 == 0) return MI355X_OK;
    // the DEBUG kernel stores only the partials; dst is a placeholder
    const int64_t nb = ne00 / QK;
    float *dst = (float *)out;
    mi355x_gemv_desc d = {src0_type, src0, ne01, nb01, dst};
    GemvPlan pl;
    int rc = plan_gemv(&d, 1, ne00, 1, 1, false, true, pl);
    if (rc) return rc;
    pl.a.xq = (const uint8_t *)src1_q8;
    pl.a.xq_col_stride = (int64_t)(nb * 292);
    pl.a.dbg = out;
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_gemv(pl, (hipStream_t)stream);
}

int mi355x_gemv_impl(int impl) {
    if (impl < MI355X_GEMV_AUTO || impl > MI355X_GEMV_DYN) return MI355X_E_INVAL;
    return gemv_impl_select(impl);
}

int mi355x_debug_knob(const char *name, double value, double *previous) {
    if (!name) return MI355X_E_INVAL;
    for (int k = 0; k < KNOB_COUNT; ++k) {
        if (strcmp(name, kKnobs[k].name) != 0) continue;
        if (previous) *previous = knob((Knob)k);
        if (value != value) {  // NaN: back to the product default
            g_knob_set[k].store(false);
        } else {
            g_knob[k].store(value);
            g_knob_set[k].store(true);
        }
        g_knob_gen.fetch_add(1);
        return MI355X_OK;
    }
    return MI355X_E_INVAL;
}

int mi355x_mmq_impl(int impl) {
    if (impl < MI355X_MMQ_AUTO || impl > MI355X_MMQ_TILE192 || impl == 5) return MI355X_E_INVAL;  // 5: retired
    const int prev = mmq_impl();
    mmq_impl_set(impl);
    return prev;
}

int mi355x_prefill_precision(int precision) {
    if (precision < 0) return prefill_precision();  // query
    if (precision > MI355X_PREFILL_F16_ALL) return MI355X_E_INVAL;
    const int prev = prefill_precision();
    prefill_precision_set(precision);
    return prev;
}

int mi355x_gemv_waves(int waves) {
    if (waves < 0 || waves > ROWS_WAVES) return MI355X_E_INVAL;
    return rows_waves_select(waves);
}

}  // extern "C"
namespace kq {
uint64_t *diag_stamps(int64_t *cap) {
    if (cap) *cap = g_stamps_cap;
    return g_stamps;
}
}  // namespace kq
extern "C" {
int mi355x_diag_stamps(void *buf, size_t bytes) {
    g_stamps = (uint64_t *)buf;
    g_stamps_cap = buf ? (int64_t)(bytes / 8) : 0;
    return MI355X_OK;
}

int mi355x_timing_enable(int enable) {
    std::lock_guard<std::mutex> lk(g_tmu);
    g_timing = enable != 0;
    g_tlog.clear();
    g_tpool_used = 0;
    return MI355X_OK;
}

int mi355x_timing_read(mi355x_launch_timing *out, int max) {
    if (hipDeviceSynchronize() != hipSuccess) return MI355X_E_NODEVICE;
    std::lock_guard<std::mutex> lk(g_tmu);
    const int n = (int)g_tlog.size();
    for (int i = 0; i < n && i < max && out; ++i) {
        memset(out[i].kernel, 0, sizeof(out[i].kernel));
        strncpy(out[i].kernel, g_tlog[i].kernel.c_str(), sizeof(out[i].kernel) - 1);
        out[i].bytes = g_tlog[i].bytes;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_tlog[i].start, g_tlog[i].stop) != hipSuccess) ms = -1.f;
        out[i].ms = ms;
    }
    return n;
}

static void vec_dot_dev(int type, const char *fn, int n, float *s, const void *vx, const void *vy, int nrc) {
    if (nrc != 1) die(fn, "nrc != 1 unsupported (reference configuration: nrows == 1)");
    if (n <= 0 || n % QK) die(fn, "n % QK_K != 0");
    if (!device_ok()) die(fn, "no gfx950 device");
    const size_t wb = mi355x_row_size(type, n), qb = mi355x_row_size(MI355X_TYPE_Q8_K, n);
    const bool xd = on_device(vx), yd = on_device(vy), sd = on_device(s);
    const size_t need = (xd ? 0 : (wb + 15) & ~(size_t)15) + (yd ? 0 : (qb + 15) & ~(size_t)15) + 16;
    ThreadCtx *c = thread_ctx(need);
    if (!c) die(fn, "stream / staging allocation failed");
    uint8_t *stage = (uint8_t *)c->buf;
    const void *dx = vx, *dy = vy;
    if (!xd) {
        if (hipMemcpyAsync(stage, vx, wb, hipMemcpyDefault, c->st) != hipSuccess) die(fn, "copy in failed");
        dx = stage;
        stage += (wb + 15) & ~(size_t)15;
    }
    if (!yd) {
        if (hipMemcpyAsync(stage, vy, qb, hipMemcpyDefault, c->st) != hipSuccess) die(fn, "copy in failed");
        dy = stage;
        stage += (qb + 15) & ~(size_t)15;
    }
    float *ds = sd ? s : (float *)stage;
    const int rc = mi355x_mul_mat_q8(type, dx, n, 1, wb, dy, 1, qb, ds, 4, c->st);
    if (rc) die(fn, "launch failed");
    if (!sd && hipMemcpyAsync(s, ds, 4, hipMemcpyDefault, c->st) != hipSuccess) die(fn, "copy out failed");
    if (hipStreamSynchronize(c->st) != hipSuccess) die(fn, "hipStreamSynchronize failed");
}

void mi355x_vec_dot_q4_K_q8_K(int n, float *s, size_t bs, const void *vx, size_t bx, const void *vy, size_t by,
                              int nrc) {
    (void)bs; (void)bx; (void)by;
    vec_dot_dev(MI355X_TYPE_Q4_K, __func__, n, s, vx, vy, nrc);
}
void mi355x_vec_dot_q5_K_q8_K(int n, float *s, size_t bs, const void *vx, size_t bx, const void *vy, size_t by,
                              int nrc) {
    (void)bs; (void)bx; (void)by;
    vec_dot_dev(MI355X_TYPE_Q5_K, __func__, n, s, vx, vy, nrc);
}
void mi355x_vec_dot_q6_K_q8_K(int n, float *s, size_t bs, const void *vx, size_t bx, const void *vy, size_t by,
                              int nrc) {
    (void)bs; (void)bx; (void)by;
    vec_dot_dev(MI355X_TYPE_Q6_K, __func__, n, s, vx, vy, nrc);
}

}  // extern "C"
