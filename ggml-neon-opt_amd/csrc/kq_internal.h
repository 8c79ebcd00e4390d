// kq_internal.h — host-side helpers shared by the C-ABI (kq_api.hip), the host paths of the
// kernels and the backend mirror (kq_backend.hip), one section per source file. Not part of
// the public ABI.
#pragma once

#include <string>
#include <tuple>

#include <hip/hip_ext.h>

#include "kq_common.h"

namespace kq {

// ---------------------------------------------------------------- kq_api.hip
int device_ok();
int num_cus();
constexpr size_t kMaxLds = 160 * 1024;    // LDS per CU (one workgroup may use it all)
constexpr size_t kTargetLds = 80 * 1024;  // aim for >= 2 resident workgroups per CU
void allow_lds(const void *fn, size_t lds);  // dynamic LDS above 64 KB must be opted into per kernel
int resident_wgs(const void *fn, size_t lds);  // workgroups of WG_THREADS resident per CU (cached)
uint64_t *diag_stamps(int64_t *cap);  // mi355x_diag_stamps' buffer (diagnostic builds)
// Experiment / diagnostic knobs of A/B runs. The product reads no environment: a knob
// holds its product default until mi355x_debug_knob() sets it (tools only), and every
// knob that changes a launch plan bumps knob_generation() (part of the graph key).
enum Knob {
    KNOB_GEMV_DIAG,        // timing stops of the KQ_ROWS_DIAG / KQ_GEMV_DIAG builds
    KNOB_GEMV_RING,        // kq_gemv ring depth override (0: by LDS)
    KNOB_GEMV_PRE0,        // recorded in the plan (RowsArgs::pre0); the kernels issue one step whatever it says
    KNOB_GEMV_SMALL_MB,    // launches below this many MB of weights: ROWS_WAVES_SMALL waves
    KNOB_GEMV_WPC,         // cap on active waves per CU (0: none)
    KNOB_GEMV_SMALL_WG,    // cap on workgroups of small launches (0: one per CU)
    KNOB_GEMV_FQMAX,       // most superblocks quantized inside kq_rows
    KNOB_MMF_WAVES,        // kq_mmf waves per workgroup (0: by K)
    KNOB_MMF_ORDER,        // kq_mmf tile order
    KNOB_ATTN_DIAG,        // timing stops of the KQ_ATTN_DIAG build
    KNOB_LOOPBACK_NOCOPY,  // emulated ALL_GATHERs skip their own-slice copy (timing only)
    KNOB_ATTN_OPROJ,       // attention + o-proj fusion: 1 per backend (set_attn_oproj), 0 never, 2 always (A/B)
    KNOB_AO_NRB,           // kq_attn_oproj row blocks (0: by shape)
    KNOB_GEMV_DYN,         // kq_rows_dyn when a wave gets at least this many units (and 16 steps) on average (0: never)
    KNOB_GEMV_DYN_P,       // kq_rows_dyn: static units per wave (0: a ring's worth; A/B only)
    KNOB_GEMV_DYN_STEPS,   // kq_rows_dyn AUTO: 16-superblock steps per wave at least (with GEMV_DYN units)
    KNOB_GEMV_SHORT,       // kq_rows short-stream form where the plan allows it (1); 0: the generic form (A/B)
    KNOB_ATTN_STREAM,      // 0 / 1 / 2: overrides mi355x_attn_stream's mode (-1: the selector's own value)
    KNOB_ATTN_STREAM_TILE, // streamed prompt attention: tokens per tile (0: by the workspace cap)
    KNOB_ARGMAX_SLICE,     // kq_argmax: entries per workgroup (0: kArgmaxSlice; A/B, and the tests of the longer slices)
    KNOB_MMQ_ID_Q6,        // kq_mmq_id on Q6_K experts: 0 by shape, 1 the 128 x 128 tile, 2 64 x 128, 3 128 x 64 (A/B: tools/moe_prefill_bench.py)
    KNOB_COUNT
};
double knob(Knob k);
uint32_t knob_generation();
// Process-wide kernel selectors a captured launch plan depends on (gemv impl / waves,
// mmq impl; attention decode / prompt impl, the MoE prefill form), packed for the backend's graph key.
uint64_t api_selector_key();
uint64_t ops_selector_key();
// Launch timing (mi355x_timing_enable): timing_slot returns true (and the events) when this
// launch should be timed. Called by timed_launch alone.
bool timing_slot(hipStream_t s, hipEvent_t &a, hipEvent_t &b);
void timing_log(const std::string &kernel, double bytes, hipEvent_t a, hipEvent_t b);

// The one launch sequence of the library: with timing on (and no capture) the kernel runs
// between two events and is logged under info()'s name and algorithmic bytes, else it is
// launched plainly; either way the launch's error, or the runtime's last one, is returned.
// info() -> LaunchInfo runs on the timed branch only: an untimed launch builds no name.
struct LaunchInfo {
    std::string name;
    double bytes;
};
template <typename Info>
int timed_launch_args(Info &&info, const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t s, void **args) {
    hipEvent_t e0, e1;
    hipError_t e;
    if (timing_slot(s, e0, e1)) {
        e = hipExtLaunchKernel(fn, grid, block, args, lds, s, e0, e1, 0);
        const LaunchInfo li = info();
        timing_log(li.name, li.bytes, e0, e1);
    } else {
        e = hipLaunchKernel(fn, grid, block, args, lds, s);
    }
    if (e != hipSuccess) return (int)e;
    e = hipGetLastError();
    return e == hipSuccess ? MI355X_OK : (int)e;
}
// Typed kernels: the arguments are converted to the kernel's parameter types (as
// hipLaunchKernelGGL does) and passed by address.
template <typename Info, typename... P, typename... Args>
int timed_launch_lazy(Info &&info, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                      Args &&...args) {
    static_assert(sizeof...(P) == sizeof...(Args), "one argument per kernel parameter");
    std::tuple<P...> params{static_cast<P>(args)...};
    return std::apply(
        [&](P &...p) {
            void *ptrs[] = {(void *)&p...};
            return timed_launch_args(info, (const void *)kern, grid, block, lds, s, ptrs);
        },
        params);
}
template <typename... P, typename... Args>
int timed_launch(const char *name, double bytes, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                 Args &&...args) {
    return timed_launch_lazy([&] { return LaunchInfo{name, bytes}; }, kern, grid, block, lds, s,
                             static_cast<Args &&>(args)...);
}

// ---------------------------------------------------------------- kq_gemv_host.hip
// The decode GEMVs' host path: descriptor checks, both planners, their launches, gemv_m1.
constexpr int64_t kFusedQMaxNb = 32;                              // kq_gemv: in-kernel quantization up to K = 8192
constexpr int64_t kRowsFusedMaxNb = ROWS_QPASS * 4 * ROWS_WAVES;  // kq_rows: up to K = 36864
// launches below this many weight bytes: ROWS_WAVES_SMALL waves. 10 MB -> 5 MB in round 5
// (TinyLlama's 6.5 / 9.5 MB ffn_down and the 8B's 9.4 MB o-proj on 12 waves): both tokens
// +0.3 %, six of six interleaved comparisons; 0 (never) -0.8 % (profiles/r05_gemv_small_mb_ab.txt)
constexpr double kRowsSmallBytes = 5e6;  // (KNOB_GEMV_SMALL_MB's default)
int choose_ncol(int64_t M, int nb);
typedef void (*gemv_fn)(const GemvArgs);
struct GemvPlan {
    GemvArgs a;
    dim3 grid;
    size_t lds;
    gemv_fn fn;
    int ncol, tmask;
    bool fusedq, debug;
};
int plan_gemv(const mi355x_gemv_desc *d, int n_desc, int64_t K, int64_t M, int ncol, bool fusedq, bool debug,
              GemvPlan &pl);
int launch_gemv(const GemvPlan &pl, hipStream_t stream);
typedef void (*rows_fn)(KQ_ROWS_PARAMS);
struct RowsPlan {
    RowsArgs a;
    dim3 grid;
    size_t lds;
    rows_fn fn;
    int tmask;
    bool fusedq;
    int nwv;  // waves per workgroup (one workgroup per CU): ROWS_WAVES, or ROWS_WAVES_SMALL
    int lsh = 0;  // fused prologue: 16 << lsh lanes per superblock (rows_pro_form; the kernel's LSH)
    bool dyn = false;  // kq_rows_dyn: rows claimed from a per-workgroup counter
    // the longest wave's 16-superblock steps and the ring depth of its type, of the matrix
    // with the least room in its ring, and the short-stream form (rows_short_form; the kernel's SH)
    int steps = 0, depth = 0;
    bool sh = false;
};
// Row-stream decode GEMV (kq_rows): returns MI355X_E_UNSUPPORTED when the rows are
// not contiguous or not aligned for it (callers then use kq_gemv). pro: ROWS_PRO_* (the fused
// prologue; ROWS_PRO_NONE unless fusedq). waves_per_cu = 0: ROWS_WAVES_SMALL waves per
// workgroup for launches under kRowsSmallBytes of weights, ROWS_WAVES otherwise. pl.fn is the
// kernel launch_rows launches: nothing picks it again.
int plan_rows(const mi355x_gemv_desc *d, int n_desc, int64_t K, bool fusedq, int pro, RowsPlan &pl,
              int waves_per_cu = 0);
int launch_rows(const RowsPlan &pl, hipStream_t stream);
int rows_kernel_id(rows_fn fn);  // mi355x_debug_rows_plan's `kernel` field
int rows_pro_kind(int prologue);  // MI355X_PRO_* -> ROWS_PRO_*
bool rows_enabled();
int gemv_impl_select(int impl);  // mi355x_gemv_impl / mi355x_gemv_waves: set, return the previous; < 0: query
int rows_waves_select(int waves);
int launch_quantize(const float *x, int64_t x_stride_floats, void *y, int64_t k, int64_t nrows,
                    hipStream_t stream);
int launch_quantize_q8L(const float *x, int64_t x_stride_floats, void *y, int64_t k, int64_t nrows,
                        hipStream_t stream, bool mmq = false);  // mmq: the prefill GEMMs' Q8L/mmq layout
size_t ext_x_bytes(int64_t k);  // the staged prologue's f32 row at the workspace start
int gemv_m1(const mi355x_gemv_desc *d, int n, const float *x, int64_t k, void *ws, size_t ws_size,
            hipStream_t stream, const mi355x_gemv_ext *ext = nullptr);

// ---------------------------------------------------------------- kq_prefill_host.hip
// prefill (ne11 >= kMmqMinCols) pieces, for the backend's shared-activation runs
constexpr int64_t kMmqMinCols = 16;  // below this the NCOL GEMV streams the weights fewer times
int mmq_impl();  // mi355x_mmq_impl / mi355x_prefill_precision: the selectors and their setters
void mmq_impl_set(int impl);
int prefill_precision();
void prefill_precision_set(int precision);
bool mmq_applies(int type, const void *w, int64_t N, size_t row_stride, int64_t M);
int launch_mmq(int type, const void *w, int64_t K, int64_t N, size_t row_stride, const uint8_t *xq, int64_t M,
               float *y, int64_t y_col_stride, hipStream_t stream, const float *res = nullptr,
               int64_t res_col_stride = 0);  // res: ADD epilogue
// f16 prefill path (mi355x_prefill_precision F16, csrc/kq_mmf.hip): the activation image
// (kq_quantize_f16img) at the workspace start, then the GEMM (its split-K slabs after the
// image); res: ADD epilogue
bool mmf_on();
bool mmf_applies(int type, const void *w, int64_t N, size_t row_stride, int64_t M, int64_t K);  // + mmf_prefers
bool mmf_prefers(int type, int64_t N, int64_t K);  // the f16 kernel is the faster one at this shape
int launch_f16img(const float *x, int64_t x_stride_floats, uint8_t *ws, int64_t K, int64_t M, hipStream_t stream);
int launch_mmf_gemm(int type, const void *w, int64_t K, int64_t N, size_t row_stride, uint8_t *ws, int64_t M,
                    float *y, int64_t y_col_stride, hipStream_t stream, const float *res = nullptr,
                    int64_t res_col_stride = 0);
// up to 4 matrices of one type on the image in one launch (split-K slabs only where they
// fit ws_size)
int launch_mmf_multi(int type, int n_mat, const void *const *w, const int64_t *N, const size_t *row_stride,
                     float *const *y, const int64_t *y_col_stride, int64_t K, uint8_t *ws, size_t ws_size, int64_t M,
                     hipStream_t stream, const float *res = nullptr, int64_t res_col_stride = 0);
size_t mmf_workspace(int64_t N, int64_t M, int64_t nb);  // activation image + d*bsum16 (+ the split-K slabs)
// KV-cache store epilogue of launch_mmq_multi (a prompt's k / v projections): kind[d] 1 k,
// 2 v, 0 none; the cells of kq_kv_store (rope(k) -> f16 rows, v -> f16 transposed)
struct MmqKv {
    int kind[4];
    const int32_t *pos;
    const float *rope;
    uint16_t *k_cache, *v_cache;
    int n_ctx, hd;
};
int launch_mmq_multi(const int *types, int n_mat, const void *const *w, const int64_t *N, const size_t *row_stride,
                     float *const *y, const int64_t *y_col_stride, int64_t K, const uint8_t *xq, int64_t M,
                     hipStream_t stream, const MmqKv *kv = nullptr);  // types: Q4_K/Q6_K may mix (kq_mmq_mixed)

// ---------------------------------------------------------------- kq_rows.hip
int launch_rows_prologue_dbg(int pro, const float *x, const float *x2, float eps, int nb, int waves, uint8_t *out,
                             hipStream_t s);
// prefill prologues: rms_norm(x) * w -> Q8L, swiglu(g, u) -> Q8L (nrows rows of n)
int launch_rms_norm_q8L(const float *x, const float *w, void *yq, int64_t n, int64_t nrows, float eps, hipStream_t s);
int launch_swiglu_q8L(const float *g, const float *u, void *yq, int64_t n, int64_t nrows, hipStream_t s);

// ---------------------------------------------------------------- kq_ops.hip
int launch_rms_norm(const float *x, const float *w, float *y, int64_t n, int64_t nrows, float eps, hipStream_t s);
int launch_binary(int op, const float *a, const float *b, float *y, int64_t n, hipStream_t s,
                  int64_t nb = 0);  // 0 add, 1 mul; b of nb elements repeated (0: nb = n)
int launch_attn_prompt(const AttnArgs &a, int n_tok, hipStream_t s);
bool attn_prompt_q8_ok(const AttnArgs &a);  // the group kernel can write a.q8_out
int launch_swiglu(const float *g, const float *u, float *y, int64_t n, hipStream_t s);
int attn_args_from(const mi355x_attn_desc *d, AttnArgs &a);  // + check_attn
// pieces the streamed path shares
size_t attn_prompt_lds(int hd, int n_ctx);
int launch_kv_store(const AttnArgs &a, int n_tok, hipStream_t s);  // kq_kv_store: a prompt's T new cells
bool attn_prompt_f16();  // mi355x_attn_prompt_precision is MI355X_ATTN_PROMPT_F16

// ---------------------------------------------------------------- kq_attn_mfma.hip
// Prompt attention on the f16 matrix cores (after kq_kv_store): every descriptor check_attn passes
int launch_attn_prompt_f16(const AttnArgs &a, int n_tok, hipStream_t s);

// ---------------------------------------------------------------- kq_attn_decode.hip
// The decode attention block: its kernels, their LDS sizing, the dispatch policy, the launch.
int attn_path(const AttnArgs &a);  // MI355X_ATTN_PATH_*: the kernel launch_attn runs (mi355x_attn_path)
int launch_attn(const AttnArgs &a, hipStream_t s);
int attn_impl();              // mi355x_attn_impl's selector
int attn_impl_set(int impl);  // ... set; returns the previous
bool attn_group_ok(const AttnArgs &a, int nwaves);      // the one-workgroup-per-kv-group path applies
size_t attn_group_bytes(const AttnArgs &a, int nwaves);  // its LDS
size_t attn_lds(int hd, int n_ctx);  // the per-head LDS layout (kq_attn_head.h)
// long-cache attention workspace (per stream), before any capture; n_tok > 1: a prompt node
int attn_cells_reserve(const AttnArgs &a, hipStream_t stream, int n_tok = 1);
void *attn_cells_buffer(size_t bytes, hipStream_t stream, bool may_alloc);

// ---------------------------------------------------------------- kq_attn_stream.hip
// Streamed attention for caches of up to kAttnStreamMaxCtx cells (mi355x_attn_stream).
// attn_stream_applies / _prompt_applies: launch_attn / launch_attn_prompt take the streamed kernels
// for these (checked) arguments; attn_stream_workspace: the bytes of attn_cells_buffer they need
// (6 per (token of a tile, head, cell)).
constexpr int kAttnStreamMaxCtx = 131072;
int attn_stream_mode();                         // 0 off, 1 where the other kernels refuse the cache's size, 2 always
bool attn_size_refused(const AttnArgs &a);      // n_ctx > 8192 or attn_lds > 64 KB: refused unless streamed
bool attn_stream_applies(const AttnArgs &a);
bool attn_stream_prompt_applies(const AttnArgs &a);
size_t attn_stream_workspace(const AttnArgs &a, int n_tok);
int launch_attn_stream(const AttnArgs &a, hipStream_t s);
int launch_attn_stream_prompt(const AttnArgs &a, int n_tok, hipStream_t s);
// The batch form (ATTN_BATCH's cells and mask; rows of n_kv entries plus one flag per 32 cells).
// attn_batch_stream_applies: the mode sends these (checked) arguments to it, `refused` saying
// that kq_attn_batch cannot take them; _buffer: its workspace on attn_cells_buffer (null under
// capture without a reservation); launch_attn_batch_stream: the launches after kq_kv_store_batch.
bool attn_batch_stream_applies(const AttnBatchArgs &b, bool refused);
size_t attn_batch_stream_workspace(const AttnBatchArgs &b);
void *attn_batch_stream_buffer(const AttnBatchArgs &b, hipStream_t s);
int launch_attn_batch_stream(const AttnBatchArgs &b, void *ws, hipStream_t s);

// ---------------------------------------------------------------- kq_attn_oproj.hip
// Decode attention + the o-proj GEMV (+ residual ADD) in one launch.
// attn_oproj_buffer: bytes of the device buffer it needs (arrival counters, zeroed once,
// then the records), 0 when the shape is not supported; *nsb: the superblocks of K.
constexpr size_t kAttnOprojCounterBytes = 1024;
constexpr int kAttnOprojMaxCtx = 256;  // kq_attn_oproj fuses caches of at most this many cells
size_t attn_oproj_buffer(int hd, int n_head, int n_head_kv, int n_ctx, int type, int64_t K, int64_t n_rows, int *nsb);
int launch_attn_oproj(const AttnArgs &a, int type, const void *w, int64_t n_rows, size_t row_stride, const float *res,
                      float *y, uint8_t *buf, size_t buf_size, hipStream_t stream);
size_t attn_lds16(int hd, int n_ctx);  // attn_head's LDS per head, 16-B multiple (kq_attn_oproj.hip)

// ---------------------------------------------------------------- kq_argmax.hip
// The argmax of an f32 vector in one launch (greedy sampling). argmax_plan is the one place
// that decides the split (mi355x_argmax_plan); argmax_workspace: the bytes of the arrival
// counter and the workgroups' words (zeroed once by the owner, left ready by every launch).
// step: the step-inputs form (the ARGMAX node's op_params[0] == 1): `out` is the decoder's
// input block [2 + hd] and receives the token, *pos + 1 and the rope row of that position.
constexpr int64_t kArgmaxMaxN = 1 << 24;
struct ArgmaxStep {
    const int32_t *pos;   // may be out + 1
    const float *table;   // [rows][hd]
    int32_t *hist;        // [n_hist]
    int64_t rows, n_hist;
    int hd;
};
int argmax_plan(int64_t n, int *workgroups, int64_t *slice);
size_t argmax_workspace(int64_t n);
int launch_argmax(const float *x, int64_t n, int32_t *out, const ArgmaxStep *step, void *ws, size_t ws_size,
                  hipStream_t stream);
// The argmax of each of `rows` rows of an f32 matrix in one launch (kq_argmax_rows; row_stride in
// floats): a row is split as argmax_plan(n) splits a vector. argmax_rows_workspace: per row a
// counter on a line of its own and the words of the largest split, the same for every n
// (0 outside 1 <= n <= 2^24, 1 <= rows <= 65535).
// step: the step-inputs form (the ARGMAX_BATCH node's op_params[0] == 1): `out` is the batch
// graph's tokens, and row i's pos / cells / mask row / history row are advanced with it.
constexpr int64_t kArgmaxMaxRows = 65535;
struct ArgmaxRowsStep {
    int32_t *pos, *cells;  // [rows]
    float *mask;           // [rows][mask_stride], n_kv entries of a row in use
    int32_t *hist;         // [rows][hist_stride], n_hist entries of a row in use
    int64_t mask_stride, hist_stride, n_kv, n_hist;
    int cell_stride;
};
size_t argmax_rows_workspace(int64_t n, int64_t rows);
int launch_argmax_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int32_t *out,
                       const ArgmaxRowsStep *step, void *ws, size_t ws_size, hipStream_t stream,
                       int64_t out_stride = 1);  // plain form: row i's index goes to out[i * out_stride]
// What the launchers of kq_argmax.hip and kq_sample.hip check first. Their statuses come in this
// order: E_INVAL (input_ok, the launcher's own outputs, step_ok), then workspace_status'
// E_WORKSPACE, then its E_NODEVICE.
// x, the split of n entries and the rows (a vector: one row of n entries rounded up to 16 bytes)
inline bool input_ok(const float *x, int64_t n, int64_t rows, int64_t row_stride, int *wgs, int64_t *slice) {
    if (!x || ((uintptr_t)x & 15u) || argmax_plan(n, wgs, slice) != MI355X_OK) return false;
    return rows >= 1 && rows <= kArgmaxMaxRows && row_stride >= n && !(row_stride & 3);
}
inline int workspace_status(const void *ws, size_t ws_size, size_t need) {
    if (!ws || ((uintptr_t)ws & 7u) || ws_size < need) return MI355X_E_WORKSPACE;
    return device_ok() ? MI355X_OK : MI355X_E_NODEVICE;
}
inline bool step_ok(const ArgmaxStep &s) {
    return s.pos && s.table && s.hist && s.hd > 0 && s.rows >= 0 && s.n_hist >= 0;
}
inline bool step_ok(const ArgmaxRowsStep &s) {
    return s.pos && s.cells && s.mask && s.hist && s.cell_stride >= 1 && s.n_kv >= 0 && s.n_kv <= 0x7fffffff &&
           s.n_hist >= 0 && s.n_hist <= 0x7fffffff && s.mask_stride >= s.n_kv && s.hist_stride >= s.n_hist;
}

// ---------------------------------------------------------------- kq_sample.hip
// The exact top-k of an f32 vector and the sampler chain on it, one launch (kq_topk; kq_topk_rows
// over the rows of a matrix), the slices argmax_plan(n)'s. topk_workspace: per row the counter's
// line and 256 x 64 words, whatever n and top_k are (0 outside argmax_rows_workspace's ranges).
// launch_topk*: sp null: the plain form (idx / val [top_k], per row); else the sampled token,
// `u` the draw(s) and `out` the token(s); step: the step-inputs forms (the SAMPLE / SAMPLE_BATCH
// nodes' op_params[0] == 1), kq_argmax's / kq_argmax_rows' writes, `u` then the draws table: the
// draw of the token that will stand at position p is entry p (0.0f where the table has none).
struct SampleStep {
    ArgmaxStep a;
    int64_t n_draws;
};
struct SampleRowsStep {
    ArgmaxRowsStep a;
    int64_t draws_stride, n_draws;  // entries between two rows of the draws, entries of a row in use
};
size_t topk_workspace(int64_t n, int64_t rows);
bool sampler_ok(const mi355x_sampler *s);
int launch_topk(const float *x, int64_t n, int top_k, int32_t *idx, float *val, const mi355x_sampler *sp, const float *u,
                int32_t *out, const SampleStep *step, void *ws, size_t ws_size, hipStream_t stream);
int launch_topk_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int top_k, int32_t *idx, float *val,
                     const mi355x_sampler *sp, const float *u, int32_t *out, const SampleRowsStep *step, void *ws,
                     size_t ws_size, hipStream_t stream);

// ---------------------------------------------------------------- kq_logprob.hip
// The record of log softmax(x)[target] for each row of an f32 matrix (include/ggml_mi355x.h, the
// rule): launch_argmax_rows, then kq_logsum_rows, both on the one workspace of
// argmax_rows_workspace's layout (logprob_workspace: 0 outside 1 <= n <= 262144, 1 <= rows <= 65535).
constexpr int64_t kLogprobMaxN = MI355X_LOGPROB_MAX_N;
size_t logprob_workspace(int64_t n, int64_t rows);
int launch_logprob_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, const int32_t *targets,
                        mi355x_logprob *out, void *ws, size_t ws_size, hipStream_t stream);

// ---------------------------------------------------------------- kq_penalize.hip
// The sampler's penalties and logit bias, in place on each row of an f32 matrix (include/ggml_mi355x.h,
// the rule): one launch of one workgroup a row, no workspace. penalties_ok: the parameters' ranges.
constexpr int kPenaltyMaxLastN = MI355X_PENALTY_MAX_LAST_N;
constexpr int kLogitBiasMax = MI355X_LOGIT_BIAS_MAX;
bool penalties_ok(const mi355x_penalties *p, int n_bias);
int launch_penalize_rows(float *x, int64_t n, int64_t rows, int64_t row_stride, const mi355x_penalties *p,
                         const int32_t *hist, int64_t hist_stride, int64_t n_hist, const int32_t *end,
                         const int32_t *bias_tok, const float *bias_val, int n_bias, hipStream_t stream);

// ---------------------------------------------------------------- kq_kv_shift.hip
// The context shift (include/ggml_mi355x.h, the rule): every check of mi355x_kv_shift, then one
// launch of kq_kv_shift in the descriptor's form, or none for an empty range. No workspace.
int launch_kv_shift(const mi355x_kv_shift_desc *d, hipStream_t stream);

// ---------------------------------------------------------------- kq_moe.hip
// The mixture-of-experts FFN (include/ggml_mi355x.h, the rule): every check of mi355x_moe_route,
// mi355x_mul_mat_id and mi355x_moe_combine, then one launch each (none for an empty shape):
// kq_gemv_id quantizes its activation row in the prologue and needs no workspace.
// The grouped form of launch_mul_mat_id (mi355x_moe_prefill; moe_grouped(pairs) says whether a
// call of T * n_used pairs takes it): kq_moe_group builds the group table of kq_common.h,
// kq_quantize_q8L the Q8L/mmq rows of the T * ne11 activation rows, kq_mmq_id (kq_mmq.hip) runs
// the tiles. `build` / `quantize` false: an earlier launch on the stream left the table of these
// ids / the rows of this x in the buffers (the backend: one table per MOE_ROUTE node, up and
// gate on one quantization).
constexpr int64_t kMoeGroupedMinPairs = 32;  // AUTO: grouped from this many pairs (profiles/moe_prefill.txt)
static_assert(kMoeGroupedMinPairs >= 16, "decode tokens and the small batches keep kq_gemv_id");
struct MoeGrouped {
    int32_t *table;  // moe_table_bytes(pairs), 4-byte aligned
    size_t table_bytes;
    uint8_t *xq;  // moe_q8_bytes(K, T * ne11), 16-byte aligned
    size_t xq_bytes;
    bool build, quantize;
};
int moe_prefill_mode();
bool moe_grouped(int64_t pairs);
size_t moe_table_bytes(int64_t pairs);
size_t moe_q8_bytes(int64_t K, int64_t rows);
int launch_moe_route(const float *gate_inp, int64_t n_embd, int n_expert, const float *x, int64_t x_stride, int64_t T,
                     int n_used, int32_t *record_out, int64_t record_stride, float *probs_out, hipStream_t stream);
int launch_mul_mat_id(int type, const void *experts, int64_t ne00, int64_t ne01, size_t nb01, size_t nb02, int n_expert,
                      const float *x, int64_t ne11, int64_t x_row_stride, const int32_t *ids, int64_t ids_stride,
                      int n_used, int64_t T, float *y, hipStream_t stream, const MoeGrouped *grouped = nullptr);
int launch_moe_combine(const float *ex, int64_t n, int n_used, int64_t T, const int32_t *records, int64_t record_stride,
                       float *y, hipStream_t stream);

// ---------------------------------------------------------------- kq_attn_batch.hip
// The attention block with cells and mask from the graph. attn_batch_args_from
// checks every argument (n_pos: rows of the rope table, 0 = n_ctx); attn_batch_form: MI355X_ATTN_GROUP /
// MI355X_ATTN_HEAD, MI355X_ATTN_PATH_STREAM (the streamed form, where mi355x_attn_stream's mode
// sends the descriptor), or MI355X_E_UNSUPPORTED where no form takes it.
int attn_batch_args_from(const mi355x_attn_batch_desc *d, int n_pos, AttnBatchArgs &b);
int attn_batch_form(const AttnBatchArgs &b);
int launch_attn_batch(const AttnBatchArgs &b, hipStream_t s);

// ---------------------------------------------------------------- kq_layer.hip
// One decode layer as one persistent launch. The caller fills E, F, nq, nkv,
// type / w, y, x, the norms, eps, att / x1 / h / x2, at (rope_row 1), sync, err; layer_plan
// checks the shape and fills the rest (grid, attention placement, ring depth, LDS layout).
int layer_plan(LayerArgs &a, int hd, int n_head);
int launch_layer(const LayerArgs &a, hipStream_t stream);
int64_t layer_table_stride(const LayerArgs &a);                  // bytes per workgroup's step lists (-1: too long)
void layer_table_fill(const LayerArgs &a, uint8_t *buf, int64_t stride);  // G tables (host memory)

}  // namespace kq
