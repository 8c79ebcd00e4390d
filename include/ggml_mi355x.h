/*
 * ggml_mi355x.h — C-ABI of the MI355X (gfx950) K-quant mat-vec / mat-mat hot path.
 *
 * This is the drop-in boundary for ggml's quantized MUL_MAT path
 * (ggml_compute_forward_mul_mat -> type_traits_cpu[src0].vec_dot, here
 * ggml_vec_dot_q4_K_q8_K). Every entry point is plain C: pointers, sizes,
 * an opaque HIP stream handle (hipStream_t passed as void*, NULL = default
 * stream). No torch or C++ types cross this boundary.
 *
 * Reference interfaces replaced (file:line in /root/reference, which quotes the
 * un-vendored llama.cpp @ a3cb0474):
 *   - ggml_vec_dot_t               README.md:449, :686  (ggml-cpu/arch/arm/quants.c:2059)
 *   - quantize_row_q8_K(_ref)      artifacts/perf/out.folded:184-186
 *   - ggml_compute_forward_mul_mat README.md:137, :157  (ggml-cpu.c:1389, one_chunk :1194)
 *   - ggml_backend_cpu_graph_compute README.md:162      (ggml-cpu.cpp:186) -> mi355x_backend_graph_compute
 *
 * Memory: every data pointer below is DEVICE memory (hipMalloc / torch cuda
 * tensor) unless stated otherwise. Weight blocks are stored exactly as GGUF /
 * ggml stores them (no repack): rows of contiguous superblocks.
 *
 * Errors: functions returning int return 0 on success, a negative
 * MI355X_E* code for argument errors, or a positive hipError_t value. The
 * ggml-surface mirrors that return void (vec_dot, from_float) abort with a
 * message on invalid arguments, as GGML_ASSERT does upstream.
 */
#ifndef GGML_MI355X_H
#define GGML_MI355X_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ formats */
/* Super-block size and block layouts: identical to ggml-common.h. Offsets
 * are proven by the reference disassembly: block_q4_K stride 0x90
 * (README.md:460, :611), d @0 (:529 "[x7,#-144]"), dmin @2 (:507), scales @4
 * (:472 "#-140", :488 "#-132"), qs @16 (:480 "x7-0x80"); block_q8_K stride 0x124
 * (:610), d @0 (:522), qs @4 (:459), bsums @260 (:492 "[x11,#256]"). */
#define MI355X_QK_K 256
#define MI355X_K_SCALE_SIZE 12

typedef uint16_t mi355x_half; /* IEEE binary16 bits (ggml_half) */

typedef struct {
    mi355x_half d;                       /* super-block scale for quantized scales */
    mi355x_half dmin;                    /* super-block scale for quantized mins   */
    uint8_t scales[MI355X_K_SCALE_SIZE]; /* 8 x 6-bit scales + 8 x 6-bit mins      */
    uint8_t qs[MI355X_QK_K / 2];         /* 4-bit quants                           */
} mi355x_block_q4_K;                     /* 144 bytes, 4.5 bpw */

typedef struct {
    mi355x_half d;
    mi355x_half dmin;
    uint8_t scales[MI355X_K_SCALE_SIZE];
    uint8_t qh[MI355X_QK_K / 8];         /* 5th bit of each quant */
    uint8_t qs[MI355X_QK_K / 2];         /* low 4 bits            */
} mi355x_block_q5_K;                     /* 176 bytes, 5.5 bpw */

typedef struct {
    uint8_t ql[MI355X_QK_K / 2];         /* low 4 bits             */
    uint8_t qh[MI355X_QK_K / 4];         /* high 2 bits            */
    int8_t scales[MI355X_QK_K / 16];     /* 8-bit sub-block scales */
    mi355x_half d;                       /* super-block scale      */
} mi355x_block_q6_K;                     /* 210 bytes, 6.5625 bpw */

typedef struct {
    float d;                             /* delta (negative when the block max is positive) */
    int8_t qs[MI355X_QK_K];              /* quants                                          */
    int16_t bsums[MI355X_QK_K / 16];     /* sums of 16 consecutive quants                    */
} mi355x_block_q8_K;                     /* 292 bytes */

/* ggml_type values (ggml.h enum ggml_type) for the types this path handles. */
enum mi355x_type {
    MI355X_TYPE_F32  = 0,
    MI355X_TYPE_F16  = 1,
    MI355X_TYPE_Q4_K = 12,
    MI355X_TYPE_Q5_K = 13,
    MI355X_TYPE_Q6_K = 14,
    MI355X_TYPE_Q8_K = 15,
    MI355X_TYPE_I32  = 26,
    MI355X_TYPE_I64  = 27,   /* cell indices of mi355x_attn_batch / ATTN_BATCH only */
};

enum mi355x_status {
    MI355X_OK           = 0,
    MI355X_E_INVAL      = -1,  /* bad shape / stride / type                    */
    MI355X_E_UNSUPPORTED = -2, /* combination not implemented on this device   */
    MI355X_E_WORKSPACE  = -3,  /* workspace missing or too small               */
    MI355X_E_NODEVICE   = -4,  /* no gfx950 device / HIP runtime unavailable   */
    MI355X_E_COMM       = -6,  /* RCCL missing / communicator error            */
    MI355X_E_LAYER      = -7,  /* a persistent-layer launch lost co-residency:
                                  that step's outputs are invalid (re-armed)   */
};

/* Bytes of one row of `type` with `k` elements (ggml_row_size). k % 256 == 0. */
size_t mi355x_row_size(int type, int64_t k);

/* Library / kernel-object identification (for logs and tests). */
const char *mi355x_version(void);
/* 1 when a gfx950 device is visible and the code object loads, else 0. */
int mi355x_device_available(void);

/* ------------------------------------------------ ggml operator surface */
/* Device mirror of ggml_from_float_t for GGML_TYPE_Q8_K
 * (type_traits_cpu[Q8_K].from_float = quantize_row_q8_K -> quantize_row_q8_K_ref).
 * x: k floats, y: k/256 block_q8_K. Bit-exact with the reference
 * (aarch64 build: iscale*x + 12582912.f contracted to one fma). x and y may be host
 * or device pointers (ggml-cpu passes src1 rows and params->wdata); runs on the
 * calling thread's own stream and returns after it completes (reentrant, see the
 * vec_dot entries below). Aborts if k % 256 != 0, as GGML_ASSERT does. */
void mi355x_quantize_row_q8_K(const float *x, void *y, int64_t k);

/* Device mirror of ggml_vec_dot_t for Q4_K x Q8_K / Q5_K x Q8_K / Q6_K x Q8_K
 * (README.md:449: void (int n, float *s, size_t bs, const void *vx, size_t bx,
 * const void *vy, size_t by, int nrc)). n % 256 == 0, nrc == 1 (the measured
 * reference configuration: no I8MM, README.md:677, so nrows == 1); bs/bx/by are
 * unused exactly as upstream. s, vx, vy may be host pointers (ggml-cpu's src0 rows and
 * params->wdata, as type_traits_cpu[type].vec_dot is called from mul_mat_one_chunk)
 * or device pointers, in any mix. Reentrant: every calling thread uses its own HIP
 * stream and staging buffer on its current device (ggml's nth threads call it at once,
 * README.md:125-131), and the call returns after that stream completes (no default-
 * stream synchronization). The Q4_K result is bit-identical to the reference NEON
 * function's fp32 output (README.md:725-777, fmsub :551, fmadd :614). */
void mi355x_vec_dot_q4_K_q8_K(int n, float *s, size_t bs, const void *vx, size_t bx,
                              const void *vy, size_t by, int nrc);
void mi355x_vec_dot_q5_K_q8_K(int n, float *s, size_t bs, const void *vx, size_t bx,
                              const void *vy, size_t by, int nrc);
void mi355x_vec_dot_q6_K_q8_K(int n, float *s, size_t bs, const void *vx, size_t bx,
                              const void *vy, size_t by, int nrc);

/* ----------------------------------------------------- stream-level API */
/* Quantize `nrows` f32 rows of k elements (row stride x_stride bytes) into
 * contiguous Q8_K rows (k/256 blocks each). Async on `stream`. */
int mi355x_quantize_q8_K(const float *x, size_t x_stride, void *y, int64_t k, int64_t nrows,
                         void *stream);

/* MUL_MAT for src0 in {Q4_K, Q5_K, Q6_K}: dst[N x M] = src0[N x K] . src1[K x M]
 * with ggml conventions: src0 row i at src0 + i*nb01 (ne00 = K, ne01 = N);
 * src1 column j (ggml row j of src1) at src1 + j*nb11, K floats; dst column j at
 * dst + j*nb1, N floats. Semantics = ggml_compute_forward_mul_mat: src1 is first
 * quantized to Q8_K (bit-exact), then every dst element is vec_dot(row, col).
 * M == 1 with K <= 8192 quantizes inside the GEMV kernel (no workspace); other
 * shapes need a workspace of mi355x_mul_mat_workspace_size() bytes (the Q8_K
 * copy of src1). Async on `stream`. */
size_t mi355x_mul_mat_workspace_size(int src0_type, int64_t ne00, int64_t ne01, int64_t ne11);
int mi355x_mul_mat(int src0_type, const void *src0, int64_t ne00, int64_t ne01, size_t nb01,
                   const float *src1, int64_t ne11, size_t nb11,
                   float *dst, size_t nb1,
                   void *workspace, size_t workspace_size, void *stream);

/* Same, with src1 already quantized to Q8_K rows (vec_dot_type), each
 * ne00/256 blocks, column j at src1_q8 + j*nb11. No workspace. */
int mi355x_mul_mat_q8(int src0_type, const void *src0, int64_t ne00, int64_t ne01, size_t nb01,
                      const void *src1_q8, int64_t ne11, size_t nb11,
                      float *dst, size_t nb1, void *stream);

/* Fused decode GEMV over up to MI355X_MAX_FUSED matrices that share one f32
 * input vector x (K floats): e.g. attn_q/attn_k/attn_v, or ffn_gate/ffn_up.
 * Each matrix may have its own K-quant type. Equivalent to n separate
 * mi355x_mul_mat calls with ne11 == 1 (bit-identical results). For K <= 8192
 * x is quantized inside the GEMV (each wave quantizes its own K-range into LDS,
 * one launch, no workspace); above that x is first quantized into `workspace`
 * (mi355x_gemv_fused_workspace_size(k) bytes; 0 means none needed). */
#define MI355X_MAX_FUSED 4
typedef struct {
    int type;            /* MI355X_TYPE_Q4_K / Q5_K / Q6_K */
    const void *w;       /* device: N rows of K/256 blocks  */
    int64_t n_rows;      /* N                                */
    size_t row_stride;   /* nb01 in bytes                    */
    float *y;            /* device: N floats                 */
} mi355x_gemv_desc;
size_t mi355x_gemv_fused_workspace_size(int64_t k);
int mi355x_gemv_fused(const mi355x_gemv_desc *descs, int n_desc, const float *x, int64_t k,
                      void *workspace, size_t workspace_size, void *stream);

/* mi355x_gemv_fused with the decode graph's neighbours of the MUL_MATs fused in
 * (the backend's node fusion uses this): `prologue` transforms x before its Q8_K
 * quantization exactly as the separate node would (MI355X_PRO_RMS_NORM: ggml_rms_norm
 * then ggml_mul by x2 = the norm weight; MI355X_PRO_SWIGLU: x = gate, x2 = up), and
 * descs[i].y receives mul_mat + residual[i] when residual[i] != NULL (ggml_add).
 * Bit-identical to the separate ops. Workspace: mi355x_gemv_ext_workspace_size(k)
 * (used only when the kernel cannot fuse, e.g. rows not contiguous). */
#define MI355X_PRO_NONE 0
#define MI355X_PRO_RMS_NORM 1
#define MI355X_PRO_SWIGLU 2
/* `epilogue` MI355X_EPI_SWIGLU: descs[0] = gate, descs[1] = up (n_desc == 2, equal
 * n_rows, no residual); epi_y[r] = ggml_vec_swiglu_f32(gate, up)[r] is written besides
 * descs[i].y — the GGML_GLU(SWIGLU) node that follows the gate/up MUL_MATs. */
#define MI355X_EPI_NONE 0
#define MI355X_EPI_SWIGLU 1
typedef struct {
    int prologue;
    const float *x2;
    float eps;
    const float *residual[MI355X_MAX_FUSED];
    int epilogue;
    float *epi_y;
} mi355x_gemv_ext;
size_t mi355x_gemv_ext_workspace_size(int64_t k);
int mi355x_gemv_fused_ext(const mi355x_gemv_desc *descs, int n_desc, const float *x, int64_t k,
                          const mi355x_gemv_ext *ext, void *workspace, size_t workspace_size, void *stream);

/* Debug/parity hook: per-superblock integer partials of a Q4_K/Q5_K/Q6_K x Q8_K
 * dot, as the GEMV kernel computes them. For each row r and superblock b:
 * out[2*(r*nb+b)+0] = sumi (sum_j sc_j * dot_j), out[...+1] = summins
 * (sum_g bsums_g * m_{g/2}; for Q6_K: sum_g bsums_g * sc_g). Device pointers. */
/* Diagnostic (no reference counterpart): the streaming ceiling of one launch -- the
 * buffer's first `bytes` (rounded down to whole 2-KB steps of 12 waves per CU) pulled into
 * LDS by non-temporal LDS-DMA, no arithmetic, on `stream`. The time a decode GEMV of that
 * many weight bytes could approach; bench.py's gemv_large "stream_us". buf 16-B aligned,
 * sink >= 4 device bytes. */
int mi355x_debug_stream(const void *buf, size_t bytes, void *sink, void *stream);
int mi355x_debug_block_partials(int src0_type, const void *src0, int64_t ne00, int64_t ne01,
                                size_t nb01, const void *src1_q8, int32_t *out, void *stream);
/* The fused GEMV prologue's mapping of a k-element activation row to a workgroup of `waves`
 * waves whose longest wave streams `steps` steps of 16 superblocks (no launch, no device
 * access): *lanes = lanes that quantize one superblock (16, 32 or 64: the widest with
 * k/256 * lanes <= 64 * waves where steps <= 2, the short launches; 16 for longer streams),
 * *passes = passes over the row (1 for 32 and 64 lanes). MI355X_E_UNSUPPORTED where `waves`
 * waves cannot hold the row (more than 3 passes: the GEMV then runs 12 waves). The debug
 * entry below runs the form of steps = 0. */
int mi355x_rows_prologue_plan(int64_t k, int waves, int64_t steps, int *lanes, int *passes);
/* The decode GEMV's stream plan for one launch of n <= 4 matrices (types[i], n_rows[i] rows of
 * k elements) on the fused-quantization path (no launch, no device access). Per matrix: the
 * most 16-superblock steps one of its waves streams, and the depth of its type's weight ring
 * (3 steps for Q4_K / Q5_K, 2 for Q6_K); *steps and *depth are those of the matrix with the
 * least room (depth - steps). *form = MI355X_ROWS_SHORT where steps <= depth for every matrix
 * and one chain batch covers a wave's rows (the kernel then issues its whole stream before its
 * barrier and runs the steps straight-line), MI355X_ROWS_LONG otherwise (the generic loop), or
 * MI355X_ROWS_CLAIMED (claimed rows, always the generic loop). batch_rows > 0: the form with a
 * chain batch of at most that many rows (0: the plan's own batch). */
enum { MI355X_ROWS_LONG = 0, MI355X_ROWS_SHORT = 1, MI355X_ROWS_CLAIMED = 2 };
int mi355x_rows_stream_plan(const int *types, const int64_t *n_rows, int n, int64_t k, int batch_rows, int *steps,
                            int *depth, int *form);
/* The whole host plan of one kq_rows / kq_rows_dyn launch (no launch, no device access), for the
 * matrices of mi355x_rows_stream_plan; fusedq: the activation is quantized inside the kernel
 * (else a Q8L row is read), prologue: MI355X_PRO_* (MI355X_PRO_NONE unless fusedq). Writes
 * MI355X_ROWS_PLAN_FIELDS integers to out (cap: its length) and returns that count, or a
 * negative error. In order: tmask, nwv, grid_x, lds, lsh, sh, dyn, steps, depth, waves_total,
 * wave_prefix[0..4], rbase[0..3], rrem[0..3], rpw, bR, prio_bytes, pre0, dyn_u, dyn_ush, dyn_p,
 * kernel. kernel names the selected instantiation, not an address:
 * ((((dyn_kernel * 8 + TMASK) * 2 + FUSEDQ) * 4 + PRO) * 4 + LSH) * 2 + SH, dyn_kernel 0 for
 * kq_rows and 1 for kq_rows_dyn, a parameter the instantiation does not have as 0. */
enum { MI355X_ROWS_PLAN_FIELDS = 31 };
int mi355x_debug_rows_plan(const int *types, const int64_t *n_rows, int n, int64_t k, int fusedq, int prologue,
                           int64_t *out, int cap);
/* Debug/parity hook: the fused GEMV prologue alone. One workgroup of `waves` waves loads x
 * (and x2), applies `prologue` (MI355X_PRO_*: x2 = norm weight / up, x = gate) and quantizes
 * to Q8_K exactly as the decode GEMV does before its barrier, then copies the workgroup's
 * image to out: k/256 blocks of 304 B (d f32 @0, 256 int8 @16, 16 int16 bsums @272).
 * Device pointers, 16-B aligned; out_bytes >= k/256 * 304. */
int mi355x_debug_rows_prologue(int prologue, const float *x, const float *x2, float eps, int64_t k, int waves,
                               void *out, size_t out_bytes, void *stream);

/* ------------------------------------------------------------ profiling */
/* Per-launch kernel timing. While enabled, every GEMV/quantize launch made
 * outside a stream capture goes through hipExtLaunchKernelGGL with a start and
 * a stop event (the kernel's own begin/end timestamps, as rocprofv3's kernel
 * trace reports them) and is logged with its kernel name and ALGORITHMIC bytes
 * (weights + f32/Q8_K activations read + f32 outputs written).
 * mi355x_timing_enable(1) clears the log; mi355x_timing_read synchronizes the
 * device and copies up to `max` entries, returning the number logged. */
typedef struct {
    char kernel[96];
    double bytes;
    float ms;
} mi355x_launch_timing;
int mi355x_timing_enable(int enable);
int mi355x_timing_read(mi355x_launch_timing *out, int max);
/* Diagnostics: while `buf` (device memory, `bytes` long) is set, GEMV launches
 * record per-wave s_memrealtime stamps (100 MHz) at kernel entry, after the
 * activation prologue, after the main loop and at exit, then after the first
 * task lookup, after the prologue DMAs are issued and after their wait:
 * 8 x uint64 per wave, [(blockIdx.x * 4 + wave) * 8 + i]. NULL disables. */
int mi355x_diag_stamps(void *buf, size_t bytes);
/* Decode-GEMV implementation selector (A/B runs, parity of every path):
 * MI355X_GEMV_AUTO (row-stream kq_rows when rows are contiguous, else kq_gemv; the
 * claimed-row form kq_rows_dyn for one-type launches with enough rows per wave),
 * MI355X_GEMV_TASKS (always the 8-row-task kq_gemv), MI355X_GEMV_ROWS (kq_rows, one
 * launch per stage; as AUTO) or MI355X_GEMV_DYN (kq_rows_dyn for every one-type
 * launch: rows claimed per workgroup from an LDS counter). Same numerics in all.
 * Returns the previous value, or MI355X_E_INVAL. */
#define MI355X_GEMV_AUTO 0
#define MI355X_GEMV_TASKS 1
#define MI355X_GEMV_ROWS 2
#define MI355X_GEMV_DYN 3
int mi355x_gemv_impl(int impl);
/* Prefill (ne11 >= 16) GEMM selector for the int8-MFMA tile kernel: MI355X_MMQ_TILE64
 * (64 weight rows x 64 activation columns per workgroup), MI355X_MMQ_TILE128 (128 rows x
 * 64 columns, 8 waves: the activation tile fetched once per 128 rows), MI355X_MMQ_TILE128W
 * (128 rows x 128 columns: each wave's weight operands feed two MFMA column tiles),
 * MI355X_MMQ_TILE64W, MI355X_MMQ_TILE192 (both below) or MI355X_MMQ_AUTO (the library's
 * choice by shape, among the first four). Same numerics in all. Returns the previous value, or
 * MI355X_E_INVAL for any other value, the retired 5 included (the selector then stays as it
 * was). */
#define MI355X_MMQ_AUTO 0
#define MI355X_MMQ_TILE64 1
#define MI355X_MMQ_TILE128 2
#define MI355X_MMQ_TILE128W 3
#define MI355X_MMQ_TILE64W 4 /* 64 rows x 128 columns, 4 waves (two column tiles per wave) */
/* 5 is not reused: it was MI355X_MMQ_TILE128X (128 x 128, 4 waves), retired after measuring
 * 20-30 % slower (profiles/r05_mmq_tile128x_ab.txt). */
#define MI355X_MMQ_TILE192 6 /* 192 rows x 64 columns, 12 waves (three per SIMD); Q4_K / Q5_K (Q6_K takes TILE128);
                                a selector only, AUTO never chooses it (profiles/r05_mmq_tile192_ab.txt) */
int mi355x_mmq_impl(int impl);
/* Prefill (ne11 >= 16) precision: MI355X_PREFILL_EXACT (kq_mmq, int8 MFMA, bit-exact
 * against ggml's per-(row, column) vec_dot loop; the default), MI355X_PREFILL_F16 (within
 * a stated tolerance: kq_mmf -- the same Q8_K activation quantization and integer
 * unpacking, the accumulated dot on the f16 matrix core, csrc/kq_mmf.hip -- on the shapes
 * where it is the faster kernel, kq_mmq elsewhere) or MI355X_PREFILL_F16_ALL (kq_mmf on
 * every shape; A/B and tests). The north_star's "within a stated fp32 tolerance on the
 * accumulated dot". The f16 path's input domain: its results are finite and within the
 * tolerance while |d * sc| * max(q) <= 65504 and |dmin * m| <= 65504 on the weight side and
 * 16 * max|x| <= 65504 on the activation side (its f16 operands f16(d * sc) * q,
 * f16(dmin * m), f16(yd * q8) and f16(yd * bsum16) stay finite); beyond that it returns
 * non-finite values, with no fallback. Subnormal, zero and negative block scales, |d| <= 4 and
 * activation rows with 1e3 outliers are inside the domain; d = +-65504 and a 1e5 outlier are
 * outside it. The exact path has no such limit. Replaces no reference interface (ggml-cpu has one precision); a
 * backend option like llama.cpp's GGML_CUDA_FORCE_MMQ / cuBLAS choice. A negative value
 * queries. The library reads no environment: the precision changes only through this
 * call (process-wide; a graph captured before it is re-planned, and a caller sizing its
 * workspace with mi355x_mul_mat_workspace_size must query it again after switching to
 * F16). Returns the previous value, or MI355X_E_INVAL. */
#define MI355X_PREFILL_EXACT 0
#define MI355X_PREFILL_F16 1
#define MI355X_PREFILL_F16_ALL 2
int mi355x_prefill_precision(int precision);
/* Decode GEMV (kq_rows) waves per workgroup (A/B runs, parity of both launch shapes):
 * 0 = by launch size (6 waves under 10 MB of weights, else 12; the debug knob
 * "GEMV_SMALL_MB" moves the threshold), or a fixed count 1..12 where the launch allows it (the in-kernel
 * quantization covers 12 superblocks per wave). Returns the previous value, or
 * MI355X_E_INVAL. */
int mi355x_gemv_waves(int waves);
/* Experiment / diagnostic knobs of A/B runs and timing tools (replaces no reference
 * interface). The library reads no environment variable; every knob holds its product
 * default until set here, process-wide: "GEMV_DIAG", "GEMV_RING", "GEMV_PRE0",
 * "GEMV_SMALL_MB", "GEMV_WPC", "GEMV_SMALL_WG", "GEMV_FQMAX",
 * "MMF_WAVES", "MMF_ORDER", "ATTN_DIAG", "LOOPBACK_NOCOPY", "ATTN_OPROJ", "AO_NRB"
 * (csrc/kq_internal.h). None changes numerics: the DIAG knobs act only in the diagnostic
 * builds (make variant), the others move launch shapes of bit-exact kernels (ATTN_OPROJ: 1
 * each backend's mi355x_backend_set_attn_oproj, 0 never, 2 in every backend), and LOOPBACK_NOCOPY (timing only)
 * leaves emulated all-gathers stale. value NaN restores the default; *previous (may be
 * NULL) receives the value in force before. 0, or MI355X_E_INVAL for an unknown name. */
int mi355x_debug_knob(const char *name, double value, double *previous);

/* --------------------------------------- decode ops of the llama graph (§8f) */
/* The non-matmul nodes of one llama decode token (llm_build_llama, out.folded:249),
 * each bit-compatible with the ggml-cpu function the reference profile shows
 * (artifacts/perf/out.folded; restatement and [U] notes: the CPU checker under the tests).
 * Device pointers, async on `stream`, 0 / MI355X_E* / hipError_t like the GEMVs. */

/* GGML_OP_GET_ROWS (ggml_compute_forward_get_rows_q -> dequantize_row_q4_K,
 * out.folded:103-104): dst[r][0..ne0) = row ids[r] of `table` as f32. type F32 /
 * Q4_K / Q5_K / Q6_K; `n_rows` rows (ne01) of `row_stride` bytes; ids: device int32[n_ids].
 * An id outside [0, n_rows) (ggml: GGML_ASSERT(i01 >= 0 && i01 < ne01)) reads nothing
 * and writes a NaN row. Precondition for the K-quant types: the kernel loads whole 16-byte
 * granules around each 2048-element chunk of a row, so the up to 15 bytes below a row's first
 * byte and above its last (to the enclosing 16-byte boundaries) must be readable device
 * memory: any table inside an allocation with 16 spare bytes on both sides qualifies. */
int mi355x_get_rows(int type, const void *table, int64_t ne0, size_t row_stride, int64_t n_rows,
                    const int32_t *ids, int64_t n_ids, float *dst, void *stream);
/* GGML_OP_RMS_NORM (ggml_compute_forward_rms_norm_f32, out.folded:189-193) over
 * `nrows` rows of n floats, y = x * (1/sqrtf(mean(x^2) + eps)); when w != NULL the
 * following GGML_OP_MUL by the norm weight is fused: y = (x*scale) * w (two roundings,
 * as the two ops). n % 256 == 0. */
int mi355x_rms_norm(const float *x, const float *w, float *y, int64_t n, int64_t nrows, float eps, void *stream);
/* GGML_OP_ADD / GGML_OP_MUL on contiguous f32 (binary_op<op_add/op_mul>, out.folded:91-99, 115-121). */
int mi355x_add(const float *a, const float *b, float *y, int64_t n, void *stream);
int mi355x_mul(const float *a, const float *b, float *y, int64_t n, void *stream);
/* GGML_OP_GLU / GLU_OP_SWIGLU split form (ggml_vec_swiglu_f32, out.folded:107-113):
 * y = silu(gate) * up with ggml_v_silu/ggml_v_expf arithmetic. */
int mi355x_swiglu(const float *gate, const float *up, float *y, int64_t n, void *stream);
/* GGML_OP_ROPE, mode NORMAL, ext_factor 0, attn_factor 1 (ggml_compute_forward_rope_f32,
 * ggml_rope_cache_init, rope_yarn; out.folded:196-208). The per-position cos/sin cache
 * ggml builds on every call is built once for positions [0, n_pos) by the host C
 * library (powf, cosf, sinf: the calls of the CPU path) into a device table of
 * mi355x_rope_table_size() bytes. pos: device int32 (one token). */
size_t mi355x_rope_table_size(int n_pos, int n_dims);
int mi355x_rope_table(float *table, int n_pos, int n_dims, float freq_base, float freq_scale, void *stream);
int mi355x_rope(const float *x, float *y, int head_dim, int n_dims, int n_heads, const int32_t *pos,
                const float *table, int n_pos, void *stream);
/* The non-flash attention block of a decode token, one launch: rope(q), rope(k) at
 * *pos, f16 K/V cache cell write (set_rows, out.folded:209-215; V transposed),
 * KQ = mul_mat(k_cache f16, q->f16) via ggml_vec_dot_f16 (NEON FP16 accumulation,
 * out.folded:140-144), soft_max_ext(scale, causal mask) (out.folded:216-234), KQV =
 * mul_mat(v_cache, kq->f16), permute + cont -> out[n_head*head_dim]. n_kv =
 * min(n_ctx, max(32, pad32(pos+1))). head_dim 64 or 128; n_ctx % 32 == 0, <= 8192 and within
 * the per-head kernel's 64 KB layout (8 n_ctx + 70 head_dim + 16 bytes past 4096 cells: 7616
 * cells at head_dim 64, 7040 at 128); with mi355x_attn_stream on, up to 131072 cells;
 * caches zero-initialised by the caller, 16-B aligned. */
typedef struct {
    const float *q, *k, *v;    /* this token's projections, before rope */
    const int32_t *pos;        /* device int32 */
    const float *rope_table;   /* mi355x_rope_table(n_pos >= n_ctx, n_dims = head_dim) */
    uint16_t *k_cache;         /* f16 [n_ctx][n_head_kv*head_dim] */
    uint16_t *v_cache;         /* f16 [n_head_kv*head_dim][n_ctx] */
    float *out;                /* [n_head*head_dim] */
    int n_ctx, n_head, n_head_kv, head_dim;
    float scale;               /* kq_scale = 1/sqrtf(head_dim) */
    int rope_row;              /* 0: rope_table is the whole table, row *pos read on device;
                                  1: rope_table is already the row of this token's position
                                  (staged by the caller with *pos), read without waiting for pos */
} mi355x_attn_desc;
int mi355x_attn_decode(const mi355x_attn_desc *a, void *stream);
/* Which decode attention kernel mi355x_attn_decode (and the ATTN_DECODE graph node) runs for
 * this descriptor under the current selectors: no launch, no device access (the pointers are
 * only checked and their alignment read). Returns one of the paths below, or a negative
 * MI355X_E_* for a descriptor attn_decode would reject. A captured launch whose workspace was
 * not reserved runs MI355X_ATTN_PATH_HEAD_BATCH in place of MI355X_ATTN_PATH_CELLS. */
#define MI355X_ATTN_PATH_HEAD 0       /* one workgroup per query head, register path (<= 256 cells) */
#define MI355X_ATTN_PATH_HEAD_BATCH 1 /* one workgroup per query head, batched cache loads */
#define MI355X_ATTN_PATH_SPLIT4 2     /* each head split by output over 4 workgroups */
#define MI355X_ATTN_PATH_SPLIT8 3     /* ... over 8 */
#define MI355X_ATTN_PATH_CELLS 4      /* KQ split over cells: kq_attn_cells + kq_attn_cells_kqv */
#define MI355X_ATTN_PATH_GROUP 5      /* one workgroup per KV group (MI355X_ATTN_GROUP) */
/* 6: retired (an experiment build's path); the number stays unused */
#define MI355X_ATTN_PATH_STREAM 7     /* streamed: kq_attn_stream_scores + _softmax + _kqv (mi355x_attn_stream) */
int mi355x_attn_path(const mi355x_attn_desc *a);
/* The same block for a prompt of n_tokens tokens in one graph (llama-bench pp: ggml's
 * batched non-flash path — SET_ROWS of the batch's cells, then KQ / soft_max with the
 * causal mask / KQV per query): q [n_tokens][n_head*head_dim], k, v [n_tokens][kvw],
 * pos device int32 [n_tokens], out [n_tokens][n_head*head_dim]; rope_row must be 0 (the
 * whole table). All cells are written first, then every query attends to the cells at or
 * before its position: each output row equals mi355x_attn_decode's for that token after
 * the tokens before it, bit for bit. A position outside the cache gives a NaN row and no
 * cell. */
int mi355x_attn_prompt(const mi355x_attn_desc *a, int n_tokens, void *stream);
/* Attention kernel selector (A/B runs, parity of all): MI355X_ATTN_SPLIT (default: one
 * workgroup per query head; for caches past 256 cells each head split over 4 or 8 workgroups
 * by output dimension, where the slice's LDS fits), MI355X_ATTN_HEAD (one workgroup per query
 * head at every cache size) or MI355X_ATTN_GROUP (one workgroup per KV group where its cells
 * fit in LDS: cells [0, n_kv) read once and shared by the group's n_head/n_head_kv query
 * heads, 1/gsz of the cache reads). Returns the previous value, or MI355X_E_INVAL. */
#define MI355X_ATTN_GROUP 0
#define MI355X_ATTN_HEAD 1
#define MI355X_ATTN_SPLIT 2
int mi355x_attn_impl(int impl);
/* Streamed attention for long caches (process-wide, like mi355x_attn_impl; default 0). The
 * streamed kernels keep scores and soft_max weights in a global workspace (6 bytes per token,
 * head and cell, on the per-stream attention workspace) and pass the V rows through a fixed LDS
 * ring, so nothing on the chip grows with the cache: 32 <= n_ctx <= 131072, n_ctx % 32 == 0,
 * same bits as the other kernels.
 *   0: off: caches past 8192 cells, or past the per-head kernel's 64 KB layout, are refused;
 *   1: a descriptor refused only for its cache size (mi355x_attn_prompt: also one whose prompt
 *      kernel does not fit the LDS) takes the streamed kernels; every descriptor that runs with
 *      0 keeps its kernel;
 *   2: every valid descriptor takes them, decode, prompt and batch (tests, A/B runs).
 * mi355x_attn_batch (ATTN_BATCH) follows the same modes with its streamed form: rows of n_kv
 * entries, cells and mask from the descriptor (mode 1: a descriptor kq_attn_batch refuses for
 * its size alone). mi355x_attn_prompt and mi355x_attn_batch run their tokens in tiles whose
 * workspace stays under 256 MiB (at least one token). A launch captured into a hipGraph needs
 * its workspace reserved beforehand (the graph backend does it); otherwise it returns
 * MI355X_E_WORKSPACE. The mode is part of the graph backend's plan key. Not covered: the
 * attention + o-proj fusion and the layer engine keep their sizes. Returns the previous mode,
 * or MI355X_E_INVAL. */
int mi355x_attn_stream(int mode);
/* Prompt attention selector (A/B runs, parity of both): MI355X_ATTN_GROUP (default: one
 * workgroup per kv group and token, the group's query heads sharing every K/V load, where
 * n_head/n_head_kv <= 8 and its LDS fits) or MI355X_ATTN_HEAD (one per query head and
 * token). mi355x_attn_batch follows the same selector. Returns the previous value, or
 * MI355X_E_INVAL. */
int mi355x_attn_prompt_impl(int impl);
/* Prompt attention precision (process-wide, like mi355x_attn_prompt_impl; set only by this call:
 * the library reads no environment). MI355X_ATTN_PROMPT_EXACT (0, the default): the kernels above,
 * the decode token's bits. MI355X_ATTN_PROMPT_F16 (1): mi355x_attn_prompt and the graph backend's
 * prompt ATTN_DECODE nodes (T >= 2) run kq_kv_store (the same cache bits) and then
 * kq_attn_prompt_f16 (csrc/kq_attn_mfma.hip), a flash-style kernel on v_mfma_f32_32x32x16_f16
 * that keeps no score matrix, no LDS and no workspace, for every descriptor mi355x_attn_prompt
 * accepts under the current mi355x_attn_stream mode and for those refused only because the exact
 * prompt kernel's LDS does not fit (caches past 8192 cells still need mi355x_attn_stream on).
 * The rule: with q^ = f16(rope(q)) (the exact path's operand) and the cache bits K, V, in exact
 * arithmetic s_c = scale * sum_d q^_d K[c][g][d] for c <= p, m = max s_c, w_c = exp(s_c - m),
 * l = sum w_c, emu_d = sum_c w_c V[g][d][c] / l; the output is within
 *   B_d = eps * sum_c w_c |V_dc| / l + 2^-24 * sum_{c<=p} |V_dc| / l
 *         + 2^-24 * (ceil(n/32) + 32) * sum_c w_c |V_dc| / l,      n = p + 1,
 *   eps = 2^-10 + 4 D,  D = 2^-23 * head_dim * scale * max_c sum_d |q^_d K_cd|
 * of emu_d (f32 accumulation of the dot, one f16 rounding of each soft_max weight in [0, 1], f32
 * accumulation of the output; tests/attn_f16_ref.py restates emulation and bound). Cells after
 * the position contribute nothing; a position outside the cache gives a NaN row and no cell.
 * Decode (mi355x_attn_decode, T = 1 nodes), mi355x_attn_batch, the attention + o-proj fusion and
 * the layer engine stay exact. Under F16 the o-proj's Q8L rows are not written by the attention
 * (a.q8_out is MI355X_E_INVAL; the planner keeps the quantization unfused). The selector is part
 * of the graph backend's plan key. p = -1 queries. Returns the previous value, or MI355X_E_INVAL. */
#define MI355X_ATTN_PROMPT_EXACT 0
#define MI355X_ATTN_PROMPT_F16 1
int mi355x_attn_prompt_precision(int p);
/* The same block for a batch whose KV cells and mask are the graph's own inputs (ggml's
 * SET_ROWS + MUL_MAT + SOFT_MAX(mask) + MUL_MAT): several sequences in one unified cache, or
 * one sequence whose cells are not its positions (a removed cell, a context shift, a reused
 * prefix). `a` as for mi355x_attn_prompt (rows per token, pos int32 [n_tokens], rope_row 0;
 * rope_table has at least n_ctx rows and a position selects only its rope row). Token i's
 * roped K row and V column are written at cell cells[i]; then every query attends over cells
 * [0, n_kv) with the score dot * scale + mask[i][c] (additive, as ggml_compute_forward_soft_max
 * applies it: -INF hides a cell, a finite entry is added; an f16 mask is widened to f32
 * first). Nothing derives visibility from pos. A cell outside [0, n_ctx) or a position outside
 * [0, n_ctx) writes nothing and gives that token a NaN output row. Two tokens of one batch on
 * the same cell is undefined, as in ggml. Cells inside [0, n_kv) must hold finite values
 * (zero-initialised caches do); nothing at or past n_kv is read. The K rows of hidden cells and
 * the V chunks of 32-cell blocks without a visible cell are not loaded (exactly the same bits:
 * csrc/kq_attn_batch.hip). Caches of more than 8192 cells (7616 at head_dim 64, 7040 at 128) run
 * only under mi355x_attn_stream, in the streamed form (kq_kv_store_batch, then per token tile
 * kq_attn_stream_scores / _softmax / _kqv over the descriptor's row, up to 131072 cells, the
 * same bits; there the K rows of 64-cell chunks and the V rows of 512-cell stages without a
 * visible cell are not loaded; a captured launch needs its workspace reserved, else
 * MI355X_E_WORKSPACE). Returns MI355X_E_INVAL for a null pointer, a type outside the list,
 * n_kv % 32 != 0, n_kv < 32, n_kv > n_ctx, mask_row_bytes below n_kv entries, rope_row != 0 or
 * n_tokens <= 0 (before any device access), MI355X_E_UNSUPPORTED for a shape the kernels do
 * not take. */
typedef struct {
    mi355x_attn_desc a;          /* q/k/v/out rows per token, pos int32[n_tokens], rope_row 0 */
    const void *cells; int cells_type;             /* MI355X_TYPE_I32 or I64 (27), [n_tokens] */
    const void *mask;  int mask_type; size_t mask_row_bytes; /* F16 / F32 */
    int n_kv, n_tokens;
} mi355x_attn_batch_desc;
int mi355x_attn_batch(const mi355x_attn_batch_desc *d, void *stream);
/* The form mi355x_attn_batch runs for this descriptor: MI355X_ATTN_GROUP (one workgroup per
 * KV group and token: the group's query heads share every K row, V chunk and mask row; groups
 * of at most 8 heads whose rows fit 160 KB of LDS), MI355X_ATTN_HEAD (one per query head and
 * token) or MI355X_ATTN_PATH_STREAM (7: the streamed form, where mi355x_attn_stream's mode sends
 * the descriptor), or the MI355X_E_* mi355x_attn_batch would return. No launch, no device access. */
int mi355x_attn_batch_path(const mi355x_attn_batch_desc *d);

/* Greedy sampling: *out = the smallest index i whose x[i] equals the maximum of the non-NaN
 * entries of x[0 .. n) under IEEE comparison (llama.cpp's greedy sampler;
 * numpy.argmax(where(isnan(x), -inf, x))). Ties go to the smallest index, -0.0 == +0.0, +-inf
 * are ordinary values, a NaN entry never wins, all NaN gives 0; the result is always in [0, n).
 * Exact, no tolerance. (ggml's own GGML_OP_ARGMAX leaves ties to the backend [U]: the ggml-graph
 * lowering does not map it here.) One launch over several workgroups (csrc/kq_argmax.hip): each
 * reduces a contiguous slice, the workgroup that arrives last combines the slices' results.
 * mi355x_argmax_plan: the split for n entries, no device: slice s is [s * slice, min(n,
 * (s + 1) * slice)), the slices cover [0, n) exactly, slice % 4 == 0; MI355X_E_INVAL outside
 * 1 <= n <= 2^24. mi355x_argmax_workspace_size: the bytes of the workgroups' results and the
 * arrival counter (0 for an n outside the range). The caller owns the workspace (8-B aligned)
 * and zeroes it once before the first call; every call leaves it ready for the next; two calls
 * that can run concurrently must not share one. x: contiguous, 16-B aligned. Returns
 * MI355X_E_INVAL (null or misaligned x, null out, n outside the range), MI355X_E_WORKSPACE
 * (missing or too small) or MI355X_E_NODEVICE, in that order. */
int mi355x_argmax_plan(int64_t n, int *workgroups, int64_t *slice);
size_t mi355x_argmax_workspace_size(int64_t n);
int mi355x_argmax(const float *x, int64_t n, int32_t *out, void *workspace, size_t workspace_size, void *stream);

/* mi355x_argmax of each of `rows` rows of an f32 matrix in one launch: out[i] = the argmax of
 * x[i * row_stride .. + n), by the same rule (smallest index of the maximum of the non-NaN
 * entries, -0.0 == +0.0, all NaN gives 0). Grid (workgroups per row, rows): a row is split as
 * mi355x_argmax_plan(n) splits a vector and handed off on a counter of its own, so a row reduces
 * exactly as mi355x_argmax reduces it alone. row_stride is in floats, >= n; x and row_stride * 4
 * must be 16-B aligned (n itself need not be a multiple of 4). 1 <= n <= 2^24, 1 <= rows <= 65535.
 * mi355x_argmax_rows_workspace_size: per row a counter on a 128-B line of its own and the words
 * of the largest split, 2176 bytes a row whatever n is (0 for an n or rows outside the ranges),
 * so one workspace serves call after call of any n and any rows it is large enough for. The caller owns the workspace (8-B aligned) and
 * zeroes it once before the first call; every call leaves it ready for the next; two calls that
 * can run concurrently must not share one. Returns MI355X_E_INVAL (null or misaligned x, a
 * row_stride below n or not 16-B aligned in bytes, null out, n or rows outside the range),
 * MI355X_E_WORKSPACE (missing or too small) or MI355X_E_NODEVICE, in that order, before any device
 * access. */
size_t mi355x_argmax_rows_workspace_size(int64_t n, int64_t rows);
int mi355x_argmax_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int32_t *out, void *workspace,
                       size_t workspace_size, void *stream);

/* Sampling on the device: the exact top-k of an f32 vector and llama.cpp's default sampler chain
 * (top-k -> top-p -> min-p -> temperature -> one draw [U]) on it, in one launch
 * (csrc/kq_sample.hip): the slices are mi355x_argmax_plan(n)'s, each workgroup selects and sorts
 * its slice's top_k, the workgroup that arrives last merges the slices that can contribute and
 * runs the chain.
 * The rule (exact: the same token as tests/sample_ref.py, no tolerance).
 *   Parameters: top_k in [1, MI355X_SAMPLE_MAX_K], temp finite and >= 0, top_p in (0, 1], min_p in
 *   [0, 1]; anything else is MI355X_E_INVAL. Per sampled token one f32 draw u supplied by the
 *   caller, meant to lie in [0, 1).
 *   Candidates: the m = min(top_k, number of non-NaN entries) largest entries under
 *   mi355x_argmax's order (larger value first, -0.0 == +0.0, among equal values the smaller
 *   index), sorted c_0 .. c_{m-1} with logits l_0 >= l_1 >= ...; a NaN is never a candidate;
 *   m == 0 (all NaN) gives token 0; c_0 is mi355x_argmax's result. If temp == 0, m == 1 or l_0 is
 *   not finite, the token is c_0 and no arithmetic runs.
 *   Arithmetic: every step f32, rounded once per operation, nothing contracted, the division
 *   correctly rounded, the sums sequential in candidate order. v_expf: ggml_v_expf, as the attention's.
 *     1. d_i = l_i - l_0
 *     2. e_i = 0 if d_i == -inf, else v_expf(d_i) (so e_0 == 1.0f)
 *     3. S = e_0 + e_1 + ... + e_{m-1}
 *     4. p_i = e_i / S
 *     5. min-p keeps the prefix of i with e_i >= min_p (it ends before the first i that fails)
 *     6. top-p keeps the shortest prefix whose running sum p_0 + ... + p_j is >= top_p, and all
 *        candidates if top_p >= 1 (or if no running sum reaches top_p)
 *     7. the kept set is the shorter of the two prefixes, never shorter than one candidate: length q
 *     8. t_i = d_i / temp, f_i = 0 if t_i == -inf, else v_expf(t_i), F = f_0 + ... + f_{q-1}
 *     9. r = u * F
 *    10. the token is the first c_i with i < q whose running sum f_0 + ... + f_i is > r; if there
 *        is none (u >= 1, a NaN, or rounding) it is c_{q-1}.
 *   (d_i / temp instead of l_i / temp - max: a tiny temp cannot produce inf - inf.)
 * mi355x_topk: idx[i] / val[i] = c_i / x[c_i] for i < m, -1 / the NaN 0x7fc00000 for m <= i < top_k.
 * mi355x_topk_rows / mi355x_sample_rows: every row of a matrix in one launch, as
 * mi355x_argmax_rows (row_stride in floats, >= n, a multiple of 4): idx / val [rows][top_k],
 * u / out [rows]. mi355x_topk_workspace_size: per row a counter on a 128-B line of its own and
 * 256 x 64 words, 131200 bytes a row whatever n and top_k are (0 for an n or rows outside
 * mi355x_argmax_rows' ranges). The caller owns the workspace (8-B aligned) and zeroes it once;
 * every call leaves it ready for the next, whatever n, rows and top_k that one has; two calls
 * that can run concurrently must not share one. x: 16-B aligned. Returns MI355X_E_INVAL (a null
 * pointer, a misaligned x, n / rows / row_stride / top_k or a sampler parameter outside its
 * range), MI355X_E_WORKSPACE (missing, misaligned or too small) or MI355X_E_NODEVICE, in that
 * order, before any device access. */
#define MI355X_SAMPLE_MAX_K 64
struct mi355x_sampler { int32_t top_k; float temp, top_p, min_p; };
size_t mi355x_topk_workspace_size(int64_t n, int64_t rows);
int mi355x_topk(const float *x, int64_t n, int top_k, int32_t *idx, float *val, void *workspace, size_t workspace_size,
                void *stream);
int mi355x_topk_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int top_k, int32_t *idx, float *val,
                     void *workspace, size_t workspace_size, void *stream);
int mi355x_sample(const float *x, int64_t n, const struct mi355x_sampler *s, const float *u, int32_t *out,
                  void *workspace, size_t workspace_size, void *stream);
int mi355x_sample_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, const struct mi355x_sampler *s,
                       const float *u /* [rows] */, int32_t *out /* [rows] */, void *workspace, size_t workspace_size,
                       void *stream);

/* Log-probabilities on the device: for each of `rows` rows of f32 logits and a target index per
 * row, the exact ingredients of log softmax(x)[target], in two launches in stream order
 * (csrc/kq_logprob.hip): mi355x_argmax_rows, then kq_logsum_rows, in which no workgroup waits for
 * another. llama.cpp's log_softmax (llama-perplexity [U]) sums scalar expf sequentially in f64;
 * this rule differs from it only in the association of that f64 sum and in v_expf for expf.
 * The rule (exact: the same record as tests/logprob_ref.py, bit for bit). For a row x of n
 * entries, 1 <= n <= MI355X_LOGPROB_MAX_N, and its target t:
 *   a   = mi355x_argmax's index, m = x[a]
 *   d_i = x_i - m, one f32 subtraction
 *   e_i = 0 if d_i == -inf, else v_expf(d_i) (ggml_v_expf, as the attention's and the sampler's)
 *   q_j = (e_{4j} + e_{4j+1}) + (e_{4j+2} + e_{4j+3}) in f32, as ggml_vec_soft_max_f32 forms its
 *         group sums; entries past n count as +0.0f
 *   S   = the sum of (double)q_j over a perfect binary tree of adjacent pairs with 65536 leaves,
 *         absent leaves +0.0: level 1 adds leaves (0, 1), (2, 3), ..., level 2 those results
 *         pairwise, and so on, each node one f64 add. Adding +0.0 is exact and no e is negative,
 *         so S depends neither on n's padding nor on how the launch is split.
 *   the record: max = m, x_target = x[t], argmax = a, pad = 0, sum = S. A target outside [0, n)
 *         (unsigned compare) gives x_target = the NaN 0x7fc00000 and reads nothing outside the row.
 * The logarithm is the host's: the device's log is not correctly rounded, so the device stops at
 * the record and mi355x_logprob_value finishes it: (double)x_target - (double)max - log(sum).
 * A row holding a NaN or +inf yields what this arithmetic yields (a NaN sum).
 * row_stride in floats, >= n and a multiple of 4; x 16-B aligned; 1 <= rows <= 65535; targets
 * [rows], 4-B aligned; out [rows], 8-B aligned. mi355x_logprob_workspace_size:
 * mi355x_argmax_rows_workspace_size's bytes and layout (2176 a row whatever n is; 0 for an n or
 * rows outside the ranges): both launches use the one workspace, kq_logsum_rows a row's words for
 * its workgroups' f64 sums and 4 bytes of the row's counter line for a. The caller owns it (8-B
 * aligned), zeroes it once, and may hand it to mi355x_argmax_rows between calls; two calls that
 * can run concurrently must not share one. Returns MI355X_E_INVAL (a null or misaligned pointer,
 * n, rows or row_stride outside its range), MI355X_E_WORKSPACE (missing, misaligned or too small)
 * or MI355X_E_NODEVICE, in that order, before any device access. */
#define MI355X_LOGPROB_MAX_N 262144
struct mi355x_logprob { float max, x_target; int32_t argmax, pad; double sum; };  /* 24 bytes */
size_t mi355x_logprob_workspace_size(int64_t n, int64_t rows);
int mi355x_logprob_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, const int32_t *targets,
                        struct mi355x_logprob *out, void *workspace, size_t workspace_size, void *stream);
/* (defined here, no symbol of the library: the name stands in parentheses) */
static inline double (mi355x_logprob_value)(const struct mi355x_logprob *r) {
    return (double)r->x_target - (double)r->max - log(r->sum);
}

/* Sampler penalties and logit bias on the device: each of `rows` rows of f32 logits is edited in
 * place, before a top-k / sample / argmax call reads it, from the row's window of past tokens and
 * a list of (token, bias) pairs, in one launch of one workgroup a row (csrc/kq_penalize.hip): no
 * atomics, no workgroup waits for another, no workspace.
 * The rule (exact: the same bits as tests/penalize_ref.py).
 *   Parameters: last_n in [0, MI355X_PENALTY_MAX_LAST_N], repeat finite and > 0, freq and present
 *   finite, n_bias in [0, MI355X_LOGIT_BIAS_MAX] pairs (bias_tok[k], bias_val[k]), a bias_val may
 *   be +-inf; anything else is MI355X_E_INVAL.
 *   Window of row i: the history entries hist[i * hist_stride + j] for the j with
 *   end[i] - last_n < j <= end[i] and 0 <= j < n_hist, j computed in 64 bits. end is an int32 on
 *   the device, read at run time; any end, INT32_MIN and INT32_MAX included, reads nothing outside
 *   the row of hist. last_n == 0: no window.
 *   A token id outside [0, n) (unsigned compare), in the window or in the bias list, is ignored
 *   (-1 is the "no token" filler). For a token t, c(t) is the number of window entries equal to
 *   t and B(t) the bias entries with bias_tok[k] == t, in the order of k. If c(t) == 0 and B(t)
 *   is empty, x[t] keeps its bits (a NaN's payload too). For every other t, in f32, every
 *   operation rounded once, nothing contracted, the division correctly rounded:
 *     1. v = x[t]
 *     2. for each k in B(t), in order: v = v + bias_val[k]
 *     3. if c(t) > 0: v = (v <= 0) ? v * repeat : v / repeat, then
 *        v = v - ((float)c(t) * freq + present): one multiply, one add, one subtract
 *     4. x[t] = v
 *   So a NaN logit stays NaN, -inf stays -inf, -0.0 counts as <= 0, and repeat 1 with freq 0 and
 *   present 0 leaves every non-NaN value's bits unchanged.
 *   Against llama.cpp [U]: the bias comes before the penalties, as in its chain (logit-bias,
 *   penalties, top-k); its penalty line is logit -= float(count) * penalty_freq +
 *   float(count > 0) * penalty_present, which is step 3 with the contraction pinned.
 * Every distinct token is written by exactly one thread, which has loaded it before; nothing in
 * global memory is read after another thread's store.
 * 1 <= n <= 2^24, 1 <= rows <= 65535, row_stride >= n in floats, x 4-B aligned. last_n == 0: hist
 * and end may be null; n_bias == 0: the lists may be null; both zero: MI355X_OK, no launch.
 * Returns MI355X_E_INVAL, in this order: a null x or p; n, rows or row_stride outside its range
 * or a misaligned x; last_n, repeat, freq, present or n_bias outside the rule's ranges; last_n > 0
 * with a null hist or end, n_hist < 1, n_hist > 0x7fffffff or hist_stride < n_hist; n_bias > 0
 * with a null list. Then MI355X_E_NODEVICE. All statuses come before any device access. */
#define MI355X_PENALTY_MAX_LAST_N 1024
#define MI355X_LOGIT_BIAS_MAX 256
struct mi355x_penalties { int32_t last_n; float repeat, freq, present; };
int mi355x_penalize_rows(float *x, int64_t n, int64_t rows, int64_t row_stride, const struct mi355x_penalties *p,
                         const int32_t *hist, int64_t hist_stride, int64_t n_hist,
                         const int32_t *end /* [rows], device */, const int32_t *bias_tok, const float *bias_val,
                         int n_bias, void *stream);

/* Context shift on the device: a full KV cache makes room without a new prefill (llama.cpp's
 * llama_memory_seq_rm + llama_memory_seq_add and its K-shift graph, build_rope_shift: a
 * ggml_rope_ext_inplace over the f16 K cache with an I32 delta per cell [U]). One launch of
 * kq_kv_shift (csrc/kq_kv_shift.hip): no atomics, no workgroup waits for another, no workspace.
 * The rule (exact: the same bits as tests/kv_shift_ref.py). A cached K element pair (k0, k1), the
 * f16 bits at channels 2i, 2i + 1 of a KV head, shifted by an integer delta:
 *     x0 = f32(k0); x1 = f32(k1)
 *     (c, s) = rope_table[|delta|][i]      the caller's mi355x_rope_table row, cos then sin
 *     if delta < 0: s = -s
 *     k0' = f16_rne(fmaf(x0, c, -(x1 * s)))
 *     k1' = f16_rne(fmaf(x0, s, x1 * c))
 *   every operation rounded once: what ggml_compute_forward_rope_f16 does with the cos/sin cache
 *   of position delta [U]. delta == 0 leaves the cell untouched: it is not rewritten (ggml
 *   rewrites it with cos 1, sin 0, which differs only for a non-finite cached value: a NaN's
 *   payload, or inf * 0). |delta| >= n_pos (the table's rows) writes NaN bits (0x7e00) to every
 *   element of the cell's K row, as mi355x_rope does: never a silent result (the deltas live on
 *   the device and cannot be checked on the host).
 * MI355X_KV_SHIFT_DELTAS (ggml's K-shift): every K cell c in [0, n_cells) is shifted in place by
 *   delta[c], a device int32 read at run time. V is not touched (v_cache may be NULL). A cell's
 *   delta is loaded together with its K row, so a delta-0 cell is read and never written.
 * MI355X_KV_SHIFT_DISCARD (a cache whose cell is its position, LlamaDecoder): the cells
 *   [keep, keep + discard) are dropped and the cells up to n_past slide down over them: for c in
 *   [keep, n_past - discard), K cell c becomes K cell c + discard shifted by -discard and V cell c
 *   becomes V cell c + discard (a slide along each channel's row of the transposed cache). Cells
 *   below keep and cells at or above n_past - discard keep their bits (the causal attention never
 *   reads past the position). Source and destination overlap; every workgroup owns channels, not
 *   cells, and loads a chunk of cells before it stores it, so none reads what another writes.
 * head_dim 64 or 128 (else MI355X_E_UNSUPPORTED); f16 caches, k_cache and rope_table 16-B aligned.
 * Returns MI355X_E_INVAL for a null descriptor, an unknown form, a null k_cache or rope_table, a
 * null delta (DELTAS) or v_cache (DISCARD), a misaligned pointer, n_ctx, n_head_kv, n_pos or
 * head_dim < 1, n_cells outside [0, n_ctx], keep < 0, discard < 1, keep + discard > n_past,
 * n_past > n_ctx or discard >= n_pos; then MI355X_E_UNSUPPORTED; n_cells == 0 or an empty moved
 * range returns MI355X_OK with no launch; then MI355X_E_NODEVICE. All before any device access. */
#define MI355X_KV_SHIFT_DELTAS 0
#define MI355X_KV_SHIFT_DISCARD 1
typedef struct {
    uint16_t *k_cache;          /* f16 [n_ctx][n_head_kv*head_dim] */
    uint16_t *v_cache;          /* f16 [n_head_kv*head_dim][n_ctx]; may be NULL in the DELTAS form */
    const float *rope_table;    /* mi355x_rope_table(n_pos, head_dim) */
    const int32_t *delta;       /* DELTAS form: device int32 [n_cells]; else NULL */
    int n_ctx, n_head_kv, head_dim, n_pos;
    int form;                   /* MI355X_KV_SHIFT_DELTAS 0 / MI355X_KV_SHIFT_DISCARD 1 */
    int n_cells;                /* DELTAS: cells [0, n_cells) */
    int keep, discard, n_past;  /* DISCARD */
} mi355x_kv_shift_desc;
int mi355x_kv_shift(const mi355x_kv_shift_desc *d, void *stream);

/* Mixture of experts on the device: the MoE arm of llm_build_llama (build_moe_ffn [U], taken when
 * llama.expert_count > 0: Mixtral). Three launches' worth of entry points (csrc/kq_moe.hip): the
 * router, the expert matmul whose weight base is data (ggml's MUL_MAT_ID) and the weighted sum.
 * No atomics, no workgroup waits for another. The rule (exact: the same bits as tests/moe_ref.py)
 * for one row `cur` of n_embd floats, T rows independently:
 *   logits[e] = vec_dot_f32(gate_inp[e], cur) in ggml_vec_dot_f32's NEON order [U]: 4 accumulators
 *     of 4 lanes stepping 16 floats, acc[j][l] = fma(g[16 s + 4 j + l], cur[16 s + 4 j + l],
 *     acc[j][l]); then acc0 += acc2, acc1 += acc3, acc0 += acc1, and (l0 + l1) + (l2 + l3).
 *     n_embd % 16 == 0: there is no scalar tail.
 *   probs = soft_max(logits), no mask, scale 1 (ggml_compute_forward_soft_max_f32 [U]): the max,
 *     e_i = ggml_v_expf(logits_i - max) for i < (n_expert & ~3) with their sums (e0 + e1) + (e2 + e3)
 *     added to a double in order, e_i = expf(logits_i - max) (libm) for the rest, added one by one;
 *     probs_i = e_i * (float)(1.0 / sum).
 *   ids = the first n_used entries of ggml's descending argsort of probs [U], the exchange sort
 *     `for i: for j > i: if p[idx[i]] < p[idx[j]]: swap(idx[i], idx[j])` from idx = 0 .. n - 1.
 *     Exact ties follow that sort, which is not "smallest index first".
 *   w[s] = probs[ids[s]]; w[s] /= (float)(w[0] + w[1] + ... in a double, in slot order) (norm_w; no
 *     scale_w, no clamp).
 *   up = mul_mat_id(up_exps, cur, ids); gate = mul_mat_id(gate_exps, cur, ids);
 *   par = swiglu(gate, up); ex = mul_mat_id(down_exps, par, ids), where for token t and slot s
 *     dst[:, s, t] = W[ids[s, t]] . q8_K(src1[:, s % ne11, t]): every row by mi355x_mul_mat's rule.
 *   out = ex[:, 0] * w[0]; out = out + ex[:, s] * w[s] for s = 1 .., each product and sum rounded
 *     once, in slot order.
 * NaN router logits are unspecified.
 *
 * mi355x_moe_route: gate_inp f32 [n_expert][n_embd] packed; x: T rows of n_embd floats, x_stride
 * floats apart; record_out: per row one record of int32 ids[n_used] followed by float w[n_used]
 * (8 * n_used bytes), record_stride 32-bit words apart (>= 2 * n_used; the words between two
 * records are not written); probs_out: NULL, or f32 [T][n_expert] packed, the probabilities (tests).
 * One launch, one workgroup a row. 2 <= n_expert <= 64, 1 <= n_used <= min(n_expert, 8),
 * n_embd % 16 == 0, else MI355X_E_UNSUPPORTED. MI355X_E_INVAL for a null or misaligned (4 bytes)
 * pointer, n_embd, n_expert or n_used < 1, n_used > n_expert, T < 0, x_stride < n_embd (T > 1) or
 * record_stride < 2 * n_used; T == 0 returns MI355X_OK with no launch; then MI355X_E_NODEVICE.
 *
 * mi355x_mul_mat_id: experts: n_expert matrices of ne01 rows of ne00 K-quant values (Q4_K, Q5_K,
 * Q6_K), nb01 bytes between rows and nb02 between experts; x: f32 [ne00, ne11, T], rows
 * x_row_stride floats apart (row t * ne11 + r), 16-byte aligned rows; ne11 == 1 gives every slot
 * of a token its one row (up, gate), ne11 == n_used one row per slot (down); ids: device int32,
 * ids[t * ids_stride + s] the expert of token t's slot s (a MOE_ROUTE record: ids_stride its
 * record_stride), read on the device by every launch; y: f32 [ne01, n_used, T] packed. One launch
 * of kq_gemv_id, a workgroup per (token, slot) pair and block of rows; only the selected experts'
 * rows are read. An id outside [0, n_expert) writes NaN to that pair's ne01 outputs and reads
 * nothing for it: never a silent result. Q4_K / Q5_K: experts, nb01 and nb02 multiples of 16; a
 * Q6_K tensor may stand at any even address with any even strides (nb02 need not be a multiple of
 * 16): what ggml's 210-byte block_q6_K of 2-byte members can produce. ne00 <= 16384, n_expert <= 64,
 * n_used <= 8, T * n_used <= 65535, else MI355X_E_UNSUPPORTED (as an unknown type).
 * MI355X_E_INVAL for a null pointer, x not 16-byte or ids / y not 4-byte aligned, ne00 < 1 or not
 * a multiple of 256, ne01 < 0, n_expert, n_used < 1, T < 0, ne11 neither 1 nor n_used,
 * x_row_stride not a multiple of 4 or < ne00 (more than one row), ids_stride < n_used, nb01 below
 * a row's bytes, nb02 < ne01 * nb01 (n_expert > 1), a misaligned Q4_K / Q5_K matrix, an odd Q6_K address or stride; then
 * MI355X_E_UNSUPPORTED; then MI355X_E_WORKSPACE (under MI355X_MOE_PREFILL_GROUPED, below: a
 * workspace that is NULL, not 16-byte aligned or below mi355x_mul_mat_id_workspace_size; the
 * kq_gemv_id form needs none: its activation rows are quantized in the launch's prologue, the
 * size is 0 and workspace may be NULL); T == 0 or ne01 == 0 returns MI355X_OK with no launch;
 * then MI355X_E_NODEVICE.
 *
 * mi355x_moe_prefill: which form mi355x_mul_mat_id and the graph backend's MUL_MAT_ID nodes take
 * (process-wide, like mi355x_mmq_impl; reads no environment; part of the backend's plan key).
 * kq_gemv_id streams an expert matrix once per (token, slot) pair; the grouped form streams every
 * expert matrix once per call, whatever T is, and gives the same bits:
 *   kq_moe_group      sorts the T * n_used pairs by expert on the device, at every launch (the ids
 *                     are data, a captured graph is replayed): one workgroup, no global atomics;
 *   kq_quantize_q8L   the T * ne11 activation rows as Q8L blocks in the workspace;
 *   kq_mmq_id         mi355x_mul_mat's int8-MFMA tiles (128 rows x 64 pairs of one expert): the
 *                     weight base, the activation rows and the output rows of a tile come from the
 *                     sorted list. The grid depends on the shapes alone.
 * An id outside [0, n_expert) gives NaN rows in either form. The order of the pairs inside an
 * expert's group is unspecified and enters no result. Same limits as above (T * n_used <= 65535).
 *   MI355X_MOE_PREFILL_AUTO (0, default)  grouped from T * n_used >= 32 pairs, kq_gemv_id below. A
 *                                         call that brings no (or too small a) workspace runs kq_gemv_id:
 *                                         AUTO refuses nothing that form can run;
 *   MI355X_MOE_PREFILL_GEMV (1)           always kq_gemv_id;
 *   MI355X_MOE_PREFILL_GROUPED (2)        grouped for any T >= 1; MI355X_E_WORKSPACE without its workspace.
 * Returns the previous value, or MI355X_E_INVAL. mi355x_mul_mat_id_workspace_size: the bytes a
 * call of that shape needs under the current mode: 0 where it takes kq_gemv_id, else the group
 * table (1152 + 8 bytes a pair) and T * n_used Q8L rows of ne00 / 256 * 304 bytes.
 *
 * mi355x_moe_combine: ex f32 [n, n_used, T] packed, records / record_stride as mi355x_moe_route
 * wrote them (the weights are read at words [n_used, 2 n_used) of a record), y f32 [n, T] packed.
 * One elementwise launch. MI355X_E_INVAL for a null or misaligned (4 bytes) pointer, n < 0,
 * n_used < 1, T < 0 or record_stride < 2 * n_used; MI355X_E_UNSUPPORTED for n_used > 8 or
 * T > 65535; n == 0 or T == 0 returns MI355X_OK with no launch; then MI355X_E_NODEVICE.
 * All statuses come before any device access. */
#define MI355X_MOE_MAX_EXPERTS 64
#define MI355X_MOE_MAX_USED 8
#define MI355X_MUL_MAT_ID_MAX_K 16384
#define MI355X_MOE_PREFILL_AUTO 0
#define MI355X_MOE_PREFILL_GEMV 1
#define MI355X_MOE_PREFILL_GROUPED 2
int mi355x_moe_prefill(int impl);
int mi355x_moe_route(const float *gate_inp, int64_t n_embd, int n_expert, const float *x, int64_t x_stride, int64_t T,
                     int n_used, int32_t *record_out, int64_t record_stride, float *probs_out /* nullable */,
                     void *stream);
size_t mi355x_mul_mat_id_workspace_size(int type, int64_t ne00, int n_used, int64_t T);
int mi355x_mul_mat_id(int type, const void *experts, int64_t ne00, int64_t ne01, size_t nb01, size_t nb02,
                      int n_expert, const float *x, int64_t ne11, int64_t x_row_stride, const int32_t *ids,
                      int64_t ids_stride, int n_used, int64_t T, float *y, void *workspace, size_t workspace_size,
                      void *stream);
int mi355x_moe_combine(const float *ex, int64_t n, int n_used, int64_t T, const int32_t *records, int64_t record_stride,
                       float *y, void *stream);

/* --------------------------------------------- ggml-backend mirror (C++) */
/* A minimal mirror of ggml-backend's device/buffer/graph interface
 * (ggml-backend-impl.h [U]; CPU sibling ggml-cpu.cpp:186, README.md:162),
 * enough for a ggml adapter to forward MUL_MAT nodes. */
/* Node ops: MUL_MAT and the other nodes of a llama decode token (llm_build_llama).
 * Operands (src[i]) and op_params per op:
 *   MUL_MAT      src0 K-quant weights [K, N], src1 f32 [K, M]            -> f32 [N, M]
 *   GET_ROWS     src0 table (F32/Q4_K/Q6_K) [K, rows], src1 I32 ids [n]  -> f32 [K, n]
 *   RMS_NORM     src0 f32 [n, rows]; op_params[0] = eps (float bits)     -> f32
 *   MUL, ADD     src0, src1 f32, same shape (contiguous)                 -> f32
 *   SWIGLU       src0 gate, src1 up (GGML_OP_GLU, GLU_OP_SWIGLU, split)  -> f32
 *   ROPE         src0 f32 [head_dim, n_heads], src1 I32 pos [1], src2 f32 rope table
 *                [n_dims, n_pos] (mi355x_rope_table); op_params[0] = n_dims (mode NORMAL)
 *   ATTN_DECODE  src0 q, src1 k, src2 v (f32, before rope), src3 I32 pos [1],
 *                src4 F16 k_cache [kvw, n_ctx], src5 F16 v_cache [n_ctx, kvw] (transposed),
 *                src6 rope table [head_dim, >= n_ctx], or [head_dim, 1]: the row of this
 *                token's position, staged with pos; op_params = {n_head, n_head_kv, head_dim, scale bits}
 *                -> f32 [head_dim*n_head]: the non-flash attention block
 *                (set_rows, mul_mat f16, soft_max_ext, mul_mat f16, permute, cont).
 *                n_ctx a multiple of 32 within mi355x_attn_decode's sizes: up to 8192 cells
 *                and the per-head kernel's 64 KB layout, or, while mi355x_attn_stream is on,
 *                up to 131072 cells on the streamed kernels (decode and prompt; such a node
 *                joins neither the attention + o-proj fusion nor the layer engine, and a
 *                prompt's o-proj quantization stays unfused).
 *   ATTN_BATCH   src0..src6 as ATTN_DECODE for T tokens (q [n_head*head_dim, T], k, v [kvw, T]
 *                packed rows, pos I32 [T], both caches, the whole rope table [head_dim, n_pos]:
 *                a position >= n_pos has no rope row), src7 cells I32 or I64 [T], src8 mask F16
 *                or F32 [>= n_kv, >= T] (nb[1] the row stride); op_params = {n_head, n_head_kv,
 *                head_dim, scale bits, n_kv} -> f32 [head_dim*n_head, T]: mi355x_attn_batch —
 *                token i stored at cell cells[i], every query over cells [0, n_kv) under its
 *                mask row. One launch unit (store + attention), captured and replayed like any
 *                node: cells, mask and pos are read on the device at run time. It joins none
 *                of the ATTN_DECODE fusions.
 *   ALL_GATHER   src0 f32 [n] (this rank's contiguous row slice of a row-split MUL_MAT
 *                chain stage) -> f32 [n * world]: the slices of every rank in rank order,
 *                one RCCL ncclAllGather over xGMI on the backend stream (captured in the
 *                hipGraph). Needs mi355x_backend_set_comm; the exchange step of the
 *                row split (weight rows of one matrix across the GPUs,
 *                the reference's per-thread row split README.md:125-131 across devices).
 *   ALL_REDUCE   src0 f32 [n] (this rank's PARTIAL output of a K-split MUL_MAT: the
 *                reference's fp32 chain over the rank's superblock range of K) -> f32 [n]
 *                the sum over ranks, one RCCL ncclAllReduce(sum) on the backend stream
 *                (captured in the hipGraph). The exchange step of the K-split ("Megatron")
 *                pairing of SURVEY.md §8e: o-proj and ffn_down split along K at 256-element
 *                superblock boundaries, 2 collectives per layer. The sum re-associates the
 *                row's fp32 chain: within SURVEY.md §8c's fp32 bound, not bit-exact.
 *   ARGMAX       mi355x_argmax of src0, a packed f32 vector of 1 .. 2^24 entries, 16-B aligned;
 *                one launch, never fused or elided; its counter and partials belong to the
 *                backend. op_params[0] = 0: -> I32 [1], the index. op_params[0] = 1, the
 *                step-inputs form (greedy decoding without the host, LlamaDecoder.generate):
 *                src1 I32 pos [1] (may be dst + 1), src2 f32 rope table [head_dim, rows], src3
 *                I32 history [n_hist] -> I32 [2 + head_dim], the decode graph's input block:
 *                dst[0] = the index, dst[1] = pos + 1, dst[2 ..] = the bits of table row
 *                pos + 1 if pos + 1 < rows (else left alone), history[pos + 1] = the index if
 *                pos + 1 < n_hist (unsigned compares). pos + 1 is written even at the end of
 *                the cache: a further replay meets ATTN_DECODE's position outside the cache
 *                (NaN output, caches untouched).
 *   ARGMAX_BATCH mi355x_argmax_rows of src0, f32 [n, T] with packed rows (nb[1] = 4 n, n % 4 == 0,
 *                1 <= n <= 2^24, 1 <= T <= 65535), 16-B aligned; one launch, never fused or
 *                elided; the rows' counters and partials belong to the backend. op_params[0] = 0:
 *                -> I32 [T], the rows' indices. op_params[0] = 1, the step-inputs form (greedy
 *                decoding of several sequences without the host, LlamaDecoder.generate_batch):
 *                src1 I32 pos [T], src2 I32 cells [T], src3 F32 mask [>= n_kv, T] (nb[1] the row
 *                stride), src4 I32 history [n_hist, T] (nb[1] the row stride), op_params[1] =
 *                cell_stride >= 1, op_params[2] = n_kv -> I32 [T], the tokens. For row i, with
 *                tok its index, p = pos[i] + 1 and c = cells[i] + cell_stride: dst[i] = tok,
 *                pos[i] = p, cells[i] = c, mask[i][c] = 0.0f if c < n_kv, history[i][p] = tok if
 *                p < n_hist (unsigned compares: a negative or overrun value writes nothing
 *                outside its array). p and c are written even at the end of the cache: a
 *                further replay meets ATTN_BATCH's cell or position outside the cache (NaN row,
 *                caches untouched). An F16 mask or I64 cells are not taken.
 *   SAMPLE       mi355x_sample of src0 (ARGMAX's vector); one launch, never fused or elided; its
 *                counter and words belong to the backend (a buffer of their own). op_params =
 *                {form, top_k, temp bits, top_p bits, min_p bits}, validated where the node is
 *                enqueued. form 0: src1 F32 u [1] -> I32 [1], the token. form 1, the step-inputs
 *                form (LlamaDecoder.generate(sampler=...)): src1, src2, src3 as ARGMAX's pos, rope
 *                table and history, src4 F32 draws [n_draws] -> I32 [2 + head_dim]: ARGMAX's
 *                writes with the sampled token, its draw u = draws[pos + 1] if pos + 1 < n_draws
 *                (unsigned), else 0.0f (which picks c_0).
 *   SAMPLE_BATCH mi355x_sample_rows of src0 (ARGMAX_BATCH's matrix); one launch, never fused or
 *                elided. op_params = {form, top_k, temp bits, top_p bits, min_p bits, cell_stride,
 *                n_kv}. form 0: src1 F32 u [T] -> I32 [T]. form 1: src1 .. src4 as ARGMAX_BATCH's
 *                pos, cells, mask and history, src5 F32 draws [n_draws, T] (nb[1] the row stride)
 *                -> I32 [T]: ARGMAX_BATCH's writes with row i's sampled token, its draw
 *                draws[i][pos[i] + 1] where that entry exists, else 0.0f.
 *   LOGPROB_BATCH mi355x_logprob_rows of src0, f32 [n, T] with packed rows (nb[1] = 4 n, n % 4 == 0,
 *                1 <= n <= 262144, 1 <= T <= 65535), 16-B aligned, and src1 I32 targets [T]
 *                -> I32 [6, T], 8-B aligned: row i is the struct mi355x_logprob of logits row i
 *                and targets[i] (LlamaDecoder.logprobs). One launch unit of two launches
 *                (kq_argmax_rows, kq_logsum_rows), never fused or elided; its workspace is the
 *                backend's ARGMAX buffer. Captured and replayed like any node: the targets are
 *                read on the device at run time.
 *   PENALIZE     mi355x_penalize_rows in place on src0, the logits, f32 [n, T] with packed rows
 *                (1 <= n <= 2^24, 1 <= T <= 65535), as ARGMAX_BATCH takes them (T 1 in the token
 *                graph): data == src0->data, with src0's type, ne and nb. src1 I32 end [T] (the
 *                graph's positions), src2 I32 history [n_hist, T] (nb[1] the row stride), src3 I32
 *                bias_tok [n_bias], src4 F32 bias_val [n_bias]; src1 / src2 may be null at last_n 0,
 *                src3 / src4 at n_bias 0. op_params = {last_n, the bits of repeat, freq, present,
 *                n_bias}. One launch, never fused or elided, captured and replayed like any node:
 *                end, the history and the lists are read on the device at run time. A SAMPLE /
 *                SAMPLE_BATCH / ARGMAX* node that follows names the PENALIZE node as its src0 (the
 *                same address; the stream gives the order).
 *   KV_SHIFT     mi355x_kv_shift in place on src0, the K cache, F16 [kvw, n_ctx] with packed rows,
 *                16-B aligned: data == src0->data, with src0's type, ne and nb. src1 the V cache,
 *                F16 [n_ctx, kvw] (transposed), or null in the DELTAS form; src2 the rope table
 *                [head_dim, n_pos]; src3 I32 deltas [n_cells], DELTAS form only. op_params =
 *                {n_head_kv, head_dim, form, n_cells} (DELTAS) or {n_head_kv, head_dim, form, keep,
 *                discard, n_past} (DISCARD), with mi355x_kv_shift's ranges; any n_ctx >= 1. Launches
 *                of its own in graph order (none for an empty range), never fused, elided or moved
 *                across an attention node on the same caches; captured and replayed like any node
 *                (every replay shifts again): the deltas are read on the device at run time.
 *   MOE_ROUTE    mi355x_moe_route: src0 gate_inp f32 [n_embd, n_expert] packed, src1 x f32
 *                [n_embd, T] (nb[1] the row stride); op_params = {n_used} -> I32 [2 * n_used, T]
 *                (nb[1] the record stride): row t the record of token t, ids then the weights' bits.
 *   MUL_MAT_ID   mi355x_mul_mat_id: src0 the expert tensor, K-quant [K, N, n_expert] (ne[2] the
 *                experts, nb[1], nb[2]), src1 the activations f32 [K, ne11, T] with ne11 1 or n_used
 *                and packed rows of rows (nb[2] = ne11 * nb[1]), src2 the MOE_ROUTE node (its
 *                ne[0] / 2 is n_used) -> f32 [N, n_used, T] packed. In the grouped form
 *                (mi355x_moe_prefill) the group table, in a buffer of the backend's own, is built
 *                once per MOE_ROUTE node and read by its three consumers, and up and gate, which
 *                share src1, quantize it once: per MoE layer one kq_moe_group, two
 *                kq_quantize_q8L and three kq_mmq_id.
 *   MOE_COMBINE  mi355x_moe_combine: src0 the experts' outputs f32 [n, n_used, T] packed, src1 the
 *                MOE_ROUTE node -> f32 [n, T] packed.
 *                The three MoE nodes get launches of their own in graph order and are never fused or
 *                elided; a graph that holds one of them takes neither the layer engine nor the
 *                attention + o-proj fusion anywhere (whatever the backend's switches say). They are
 *                captured and replayed like any node: the ids and weights are read on the device
 *                at every replay. They count as readers of their sources, so an RMS_NORM -> MUL
 *                pair they read is materialised. */
enum mi355x_op {
    MI355X_OP_NONE = 0, MI355X_OP_MUL_MAT = 1, MI355X_OP_GET_ROWS = 2, MI355X_OP_RMS_NORM = 3,
    MI355X_OP_MUL = 4, MI355X_OP_ADD = 5, MI355X_OP_SWIGLU = 6, MI355X_OP_ROPE = 7,
    MI355X_OP_ATTN_DECODE = 8, MI355X_OP_ALL_GATHER = 9, MI355X_OP_ALL_REDUCE = 10,
    MI355X_OP_ATTN_BATCH = 11, MI355X_OP_ARGMAX = 12, MI355X_OP_ARGMAX_BATCH = 13,
    MI355X_OP_SAMPLE = 14, MI355X_OP_SAMPLE_BATCH = 15, MI355X_OP_LOGPROB_BATCH = 16,
    MI355X_OP_PENALIZE = 17, MI355X_OP_KV_SHIFT = 18,
    MI355X_OP_MOE_ROUTE = 19, MI355X_OP_MUL_MAT_ID = 20, MI355X_OP_MOE_COMBINE = 21,
};
#define MI355X_MAX_SRC 10  /* GGML_MAX_SRC */
#define MI355X_TENSOR_FLAG_OUTPUT 1  /* read by the caller after graph_compute: never elided by fusion */

typedef struct mi355x_tensor {
    int type;                      /* enum mi355x_type (+ F16 = 1, I32 = 26)    */
    int op;                        /* enum mi355x_op                            */
    int64_t ne[4];                 /* elements per dim (ggml order)            */
    size_t nb[4];                  /* bytes per dim                            */
    struct mi355x_tensor *src[MI355X_MAX_SRC];
    void *data;                    /* device pointer                            */
    int32_t op_params[8];
    int32_t flags;                 /* MI355X_TENSOR_FLAG_*                      */
} mi355x_tensor;

typedef struct mi355x_backend *mi355x_backend_t;

/* Devices this library runs on (gfx950 with its code object), for the ggml-backend
 * registration's get_device_count (ggml_backend_reg_i [U], ggml-backend-impl.h; the
 * CPU sibling registers one device, ggml-cpu.cpp). 0 without a GPU. */
int mi355x_device_count(void);
/* The HIP ordinal of the i-th device counted by mi355x_device_count (a host may list a
 * non-gfx950 GPU at a lower ordinal): the `device` argument the calls below take; -1 if
 * there is no such device. */
int mi355x_device_ordinal(int i);
/* Free / total device memory (ggml_backend_device_i.get_memory [U]): 0 or an error. */
int mi355x_device_memory(int device, size_t *free_bytes, size_t *total_bytes);
mi355x_backend_t mi355x_backend_init(int device);        /* NULL on failure */
void mi355x_backend_free(mi355x_backend_t backend);
const char *mi355x_backend_name(mi355x_backend_t backend);
void *mi355x_backend_stream(mi355x_backend_t backend);   /* hipStream_t */
void *mi355x_backend_alloc(mi355x_backend_t backend, size_t size); /* device buffer */
void mi355x_backend_free_buffer(mi355x_backend_t backend, void *ptr);
int mi355x_backend_set_tensor(mi355x_backend_t backend, void *dst, const void *host_src,
                              size_t size);              /* async H2D, bytes unchanged */
int mi355x_backend_get_tensor(mi355x_backend_t backend, void *host_dst, const void *src,
                              size_t size);              /* async D2H */
/* async device memset of `size` bytes to (uint8_t)value (ggml_backend_buffer_i.memset_tensor
 * / clear [U]) */
int mi355x_backend_memset(mi355x_backend_t backend, void *dst, int value, size_t size);
/* Waits for the backend stream. With the persistent layer on (set_layer_engine) it also
 * returns MI355X_E_LAYER when a layer launch since the last check gave up waiting for
 * another workgroup (outputs invalid; the counters are re-armed, as layer_error does). */
int mi355x_backend_synchronize(mi355x_backend_t backend);
int mi355x_backend_supports_op(const mi355x_tensor *op); /* 1 / 0 */
/* Node fusion in graph_compute (default on): RMS_NORM -> MUL(norm weight) ->
 * MUL_MAT(s) and SWIGLU -> MUL_MAT run as ONE GEMV launch whose prologue computes
 * the norm / swiglu before the Q8_K quantization, and MUL_MAT -> ADD(residual)
 * writes mul_mat + residual from the GEMV's epilogue; RMS_NORM -> MUL alone is one
 * kernel. Fused intermediates (not flagged OUTPUT, read by no other node) are not
 * written. Results are bit-identical with fusion off. Returns the previous value. */
int mi355x_backend_set_fusion(mi355x_backend_t backend, int enable);
/* Decode attention fused with the o-proj GEMV (default OFF: bit-identical, but measured 6-10 %
 * slower per token than the two launches; needs fusion on): an ATTN_DECODE
 * of one token whose output only the next node reads, a K-quant MUL_MAT (+ its residual
 * ADD), runs as ONE launch -- workgroup (s, rb) computes the heads of the o-proj's K
 * superblock s, quantizes them to that Q8_K superblock and writes the exact integer records
 * of rows block rb; the last workgroup of each row block replays every row's fp32 chain in
 * superblock order (csrc/kq_attn_oproj.hip). Bit-identical to the two launches. Applies with
 * the per-head attention kernel (mi355x_attn_impl ATTN_HEAD), head_dim 64 / 128, the heads
 * of one K superblock in one KV group, K <= 4096 and a KV cache of <= 256 cells. Returns
 * the previous value. */
int mi355x_backend_set_attn_oproj(mi355x_backend_t backend, int enable);
/* Persistent decode layer (default off; needs fusion on): the 15 nodes of one
 * llm_build_llama decode layer -- RMS_NORM, MUL, MUL_MAT q / k / v, ATTN_DECODE, MUL_MAT o,
 * ADD, RMS_NORM, MUL, MUL_MAT gate / up, SWIGLU, MUL_MAT down, ADD -- run as ONE launch of one
 * workgroup per CU (csrc/kq_layer.hip): each workgroup owns rows of every matrix, streams
 * the next stage's weights into LDS while the current stage's output is handed over
 * between workgroups, and replays each row's fp32 chain in superblock order, so every
 * output is bit-identical to the per-node path (ggml_compute_forward_mul_mat row by row,
 * README.md:125-137). Applies to K-quant weights with contiguous rows, n_embd <= 4096,
 * head_dim 64 / 128, the position's rope row staged with the inputs, and a KV cache whose
 * attention LDS fits beside the weight ring. Returns the previous value. */
int mi355x_backend_set_layer_engine(mi355x_backend_t backend, int enable);
/* Non-zero when a persistent-layer launch since the last call gave up waiting for another
 * workgroup (the device did not keep every workgroup resident): that graph's outputs are
 * invalid. Clears the flag and re-arms the launches' counters. 0 without such launches. */
int mi355x_backend_layer_error(mi355x_backend_t backend);
/* Runs nodes in order on the backend stream. Consecutive MUL_MAT nodes with
 * ne11 == 1 that share src[1] are fused into one launch. When `use_graph` is
 * non-zero the launch sequence is captured once into a hipGraph and replayed
 * on later calls with the same node list (same pointers and shapes).
 * Returns 0 (GGML_STATUS_SUCCESS) or an error code. */
int mi355x_backend_graph_compute(mi355x_backend_t backend, mi355x_tensor *const *nodes,
                                 int n_nodes, int use_graph);

/* ------------------------------------------- ggml graph lowering (host only) */
/* The adapter side of the drop-in: a ggml_tensor-shaped mirror
 * that a ggml backend's graph_compute fills from the ggml_cgraph it is handed
 * (ggml_backend_sched_compute_splits -> iface.graph_compute, README.md:162-163),
 * one mirror per ggml node/leaf with the same fields (type, ne, nb, op, op_params,
 * src, view_src/view_offs, data), and the lowering of llm_build_llama's decode
 * node sequence onto this backend's node list:
 *   GET_ROWS, RMS_NORM, MUL, ADD, MUL_MAT (K-quant x f32), GLU(SWIGLU, split) map 1:1;
 *   RESHAPE / VIEW / PERMUTE / TRANSPOSE are aliases (no node);
 *   the non-flash attention block — ROPE(Q), ROPE(K), SET_ROWS(K cache), SET_ROWS
 *   (V cache), MUL_MAT(K cache, Q), SOFT_MAX(kq, mask, scale), MUL_MAT(V cache, kq),
 *   PERMUTE, CONT — becomes ONE ATTN_DECODE node (rope table from the caller), or ONE
 *   ATTN_BATCH node under mi355x_lower_opts.cells_from_graph;
 *   llama.cpp's K-shift graph (build_rope_shift [U]) — per layer an in-place ROPE over a view
 *   [head_dim, n_head_kv, n_cells] from cell 0 of an F16 K-cache leaf, with an I32 leaf of one
 *   delta per cell, mode NORMAL, n_dims == head_dim, the table's base and scale, no freq
 *   factors — becomes ONE KV_SHIFT node in DELTAS form over ne[2] cells; any other F16 ROPE is
 *   MI355X_E_UNSUPPORTED, never dropped;
 *   [up, gate] MUL_MAT pairs read by SWIGLU(gate, up) are emitted as [gate, up]
 *   (independent nodes; the order the fused gate/up launch takes).
 * The op numbering is this library's (the adapter maps GGML_OP_* by name). */
enum mi355x_gop {
    MI355X_GOP_NONE = 0, MI355X_GOP_GET_ROWS, MI355X_GOP_RMS_NORM, MI355X_GOP_MUL, MI355X_GOP_ADD,
    MI355X_GOP_MUL_MAT, MI355X_GOP_ROPE, MI355X_GOP_SET_ROWS, MI355X_GOP_SOFT_MAX, MI355X_GOP_GLU,
    MI355X_GOP_RESHAPE, MI355X_GOP_VIEW, MI355X_GOP_PERMUTE, MI355X_GOP_TRANSPOSE, MI355X_GOP_CONT,
    MI355X_GOP_CPY,
};
#define MI355X_GLU_SWIGLU 2  /* op_params[0] of a GLU node (ggml_glu_op GGML_GLU_OP_SWIGLU) */
typedef struct mi355x_gtensor {
    int type;                       /* ggml_type numbering (F32 0, F16 1, Q4_K 12, ..., I32 26, I64 27) */
    int op;                         /* enum mi355x_gop                           */
    int64_t ne[4];
    size_t nb[4];
    int32_t op_params[16];          /* as ggml stores them (floats as bits)      */
    int32_t flags;                  /* MI355X_TENSOR_FLAG_OUTPUT for graph outputs */
    struct mi355x_gtensor *src[10];
    struct mi355x_gtensor *view_src;
    size_t view_offs;
    void *data;                     /* device pointer (leaves, and nodes' outputs) */
    char name[64];
} mi355x_gtensor;
typedef struct {
    void *rope_table;               /* f32 [head_dim, n_pos] from mi355x_rope_table  */
    int rope_n_pos;                 /* its rows (>= the KV cache size)           */
    float rope_freq_base, rope_freq_scale; /* the table's parameters (checked against ROPE) */
    int cells_eq_pos;               /* the adapter's promise, checked on the host before the
                                     * call: ONE sequence, every token's K/V cell index
                                     * (SET_ROWS k_idxs / v_idxs) equals its position
                                     * (inp_pos), the mask is the causal mask over cells
                                     * [0, pos] and the KQ / KQV views start at cell 0.
                                     * ATTN_DECODE writes cell == pos and attends over
                                     * [0, pos]; with 0 here attention blocks are not
                                     * lowered (MI355X_E_UNSUPPORTED) unless
                                     * cells_from_graph is set. Takes precedence. */
    int cells_from_graph;           /* (with cells_eq_pos 0) lower an attention block to ONE
                                     * ATTN_BATCH node that reads the cells (the K SET_ROWS
                                     * index leaf) and the mask (the SOFT_MAX mask leaf, F16 or
                                     * F32) on the device; n_kv is the KQ K-view's ne[1]. The
                                     * lowering cannot read device memory, so the adapter
                                     * promises, checked on its host copies (cells_match,
                                     * adapter/mi355x_ggml_mirror.hpp): for every token i and
                                     * channel ch the transposed-V store's index entry
                                     * v_idxs[i*kvw + ch] equals ch*kv_size + k_idxs[i], and
                                     * every k_idxs[i] lies in [0, kv_size). A zero-initialised
                                     * struct keeps the meaning it had before this field. */
} mi355x_lower_opts;
/* Lowers `n` ggml nodes (graph order) into backend nodes. Tensors are written into
 * `arena` (cap entries: nodes and the leaf mirrors they reference); `nodes_out`
 * (cap nodes_cap) receives the node list for mi355x_backend_graph_compute and
 * *n_nodes its length. Returns 0, MI355X_E_UNSUPPORTED (a node or pattern this
 * backend does not take: the caller leaves the graph to another backend) or
 * MI355X_E_INVAL / MI355X_E_WORKSPACE (arena or output too small). */
int mi355x_lower_ggml_graph(mi355x_gtensor *const *gnodes, int n, const mi355x_lower_opts *opts,
                            mi355x_tensor *arena, int arena_cap, mi355x_tensor **nodes_out, int nodes_cap,
                            int *n_nodes);

/* Row split over one process per GPU. RCCL is resolved at run time
 * from the librccl.so.1 already loaded in the process, or /opt/rocm's (dlopen): the
 * library has no link-time RCCL dependency. Rank 0 creates the id, the caller ships
 * its bytes to the other ranks (any control channel: torch.distributed gloo, MPI,
 * a file), then every rank joins. mi355x_comm_id_size() == 128 (ncclUniqueId). */
size_t mi355x_comm_id_size(void);
int mi355x_comm_get_unique_id(void *id_out);                      /* rank 0 */
int mi355x_backend_set_comm(mi355x_backend_t backend, int rank, int world,
                            const void *unique_id);               /* collective: every rank */
int mi355x_backend_comm_world(mi355x_backend_t backend);         /* 0 if no communicator */
/* Test emulation of ONE rank of a world on a single GPU, without a communicator:
 * ALL_GATHER then copies this rank's slice to offset rank*n of its output and leaves
 * the other ranks' parts as the caller put them; ALL_REDUCE leaves its output as the
 * caller put it (the reduced vector the other ranks would deliver; the rank's partial
 * stays readable in its source node). world = 0 turns it off. */
int mi355x_backend_set_comm_loopback(mi355x_backend_t backend, int rank, int world);

/* ------------------------------------------------ GGUF model files (host) */
/* Reader for GGUF v2/v3 files, the loader side of the path: llama-bench reads the
 * model through ggml's gguf_reader (artifacts/perf/out.folded:2-3, 17-22) and
 * llama_model_loader (out.folded:39-46); format restated in kq_gguf.cpp [U].
 * The file is mapped read-only; tensor bytes (GGUF block layout, no repack) go to
 * the device with mi355x_gguf_upload. Host-only except the upload: works without
 * a GPU. */
typedef struct mi355x_gguf *mi355x_gguf_t;

typedef struct {
    const char *name;  /* valid while the file is open */
    int type;          /* ggml type number (enum mi355x_type for the K-quants / F32) */
    int n_dims;
    int64_t ne[4];     /* ne[0] = row length (K), ne[1] = rows (N), unused dims 1 */
    uint64_t offset;   /* absolute byte offset of the data in the file */
    uint64_t size;     /* bytes; 0 when the type's block size is unknown to the reader */
} mi355x_gguf_tensor;

/* GGUF metadata value types (gguf_type [U]) */
enum mi355x_gguf_type {
    MI355X_GGUF_U8 = 0, MI355X_GGUF_I8 = 1, MI355X_GGUF_U16 = 2, MI355X_GGUF_I16 = 3,
    MI355X_GGUF_U32 = 4, MI355X_GGUF_I32 = 5, MI355X_GGUF_F32 = 6, MI355X_GGUF_BOOL = 7,
    MI355X_GGUF_STRING = 8, MI355X_GGUF_ARRAY = 9, MI355X_GGUF_U64 = 10, MI355X_GGUF_I64 = 11,
    MI355X_GGUF_F64 = 12,
};

mi355x_gguf_t mi355x_gguf_open(const char *path);  /* NULL on error (reason on stderr) */
void mi355x_gguf_close(mi355x_gguf_t g);
uint32_t mi355x_gguf_version(mi355x_gguf_t g);
uint64_t mi355x_gguf_alignment(mi355x_gguf_t g);    /* general.alignment, default 32 */
uint64_t mi355x_gguf_data_offset(mi355x_gguf_t g);  /* start of the tensor data section */
int64_t mi355x_gguf_n_tensors(mi355x_gguf_t g);
int64_t mi355x_gguf_find_tensor(mi355x_gguf_t g, const char *name); /* index or -1 */
int mi355x_gguf_get_tensor(mi355x_gguf_t g, int64_t i, mi355x_gguf_tensor *out);
const void *mi355x_gguf_tensor_data(mi355x_gguf_t g, int64_t i);    /* host pointer (mapped) */
/* Async H2D copy of tensor i's bytes to device memory on `stream` (hipStream_t). */
int mi355x_gguf_upload(mi355x_gguf_t g, int64_t i, void *dst_device, size_t dst_size, void *stream);
int64_t mi355x_gguf_n_kv(mi355x_gguf_t g);
int64_t mi355x_gguf_find_key(mi355x_gguf_t g, const char *key);     /* index or -1 */
const char *mi355x_gguf_key(mi355x_gguf_t g, int64_t i);
int mi355x_gguf_kv_type(mi355x_gguf_t g, int64_t i);                /* enum mi355x_gguf_type */
int mi355x_gguf_get_int(mi355x_gguf_t g, int64_t i, int64_t *out);   /* integer / bool values */
int mi355x_gguf_get_float(mi355x_gguf_t g, int64_t i, double *out);  /* any numeric value */
const char *mi355x_gguf_get_str(mi355x_gguf_t g, int64_t i);        /* NULL unless a string */
int64_t mi355x_gguf_arr_n(mi355x_gguf_t g, int64_t i);              /* array length, or -1 */

#ifdef __cplusplus
}
#endif

#endif /* GGML_MI355X_H */
