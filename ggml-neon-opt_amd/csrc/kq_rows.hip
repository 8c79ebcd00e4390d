// kq_rows.hip — decode GEMV (one activation column) over contiguous row streams.
//
// Same numerics as kq_gemv (kq_kernels.hip): integer partials bit-exact, the
// reference's fp32 update in superblock order per row (README.md:551/:614 for
// Q4_K), so outputs are bit-identical to ggml_vec_dot_q4_K_q8_K (and the Q5_K /
// Q6_K siblings) called row by row from ggml_compute_forward_mul_mat
// (ggml-cpu.c:1389, README.md:137).
//
// Decomposition (HBM-bound, so everything serves the weight stream):
//  * a wave owns `rpw` consecutive rows of one matrix; with GGUF's contiguous
//    rows that is ONE contiguous byte stream, fetched in steps of 16 superblocks
//    (2.3-3.4 KB, 3-4 LDS-DMA instructions of 1 KB, non-temporal) into a
//    per-wave ring, completion by counted s_waitcnt vmcnt (a constant in steady
//    state); no workgroup barrier after the prologue;
//  * lane quad q computes superblock 16t+q of the stream (4 lanes x 64 quants,
//    v_dot4_i32_i8, 2 DPP adds) and its leader stores what the reference's fp32
//    update consumes as a 16-B record of floats (RowRec), block-major per row batch;
//  * when a batch of bR rows is complete, lane r replays row r's records in
//    superblock order (the serial fp32 chain, 64 rows per instruction);
//  * the activation is quantized to Q8_K once per workgroup into LDS (aligned
//    304-B "Q8L" blocks: d @0, qs @16, bsums @272): 16, 32 or 64 lanes per superblock
//    by the row and the workgroup's waves (RowsPrologue below), x loaded by inline-asm
//    global loads issued before the weight DMAs; rows past the fused limit are written
//    as Q8L blocks to a workspace by kq_quantize_q8L and copied by DMA.
#include <hip/hip_ext.h>

#include <type_traits>

#include "kq_internal.h"
#include "kq_ops_device.h"
#include "kq_rows_device.h"

// Diagnostics (timing only: MI355X_GEMV_DIAG bits, per-wave s_memrealtime stamps) exist
// only in experiment builds: make variant NAME=rdiag VFLAGS=-DKQ_ROWS_DIAG=1. In the
// product build RDIAG / RSTAMPS are constants and every diagnostic branch compiles out
// (run-time diag branches cost kq_mmq 40 VGPRs).
#ifndef KQ_ROWS_DIAG
#define KQ_ROWS_DIAG 0
#endif
// The diagnostic bits travel in the leading `cfg` parameter and the stamp buffer in the entry
// batch (RowsHot), so a diagnostic build enters as the product does; it takes its stamps
// whether or not a buffer is set (RSTAMP) and writes them only where one is.
#if KQ_ROWS_DIAG
#define RDIAG(ld) ((ld).diag)
#define RSTAMPS(h) ((h).stamps)
#define RSTAMP() __builtin_amdgcn_s_memrealtime()
#else
#define RDIAG(ld) 0
#define RSTAMPS(h) ((uint64_t *)nullptr)
#define RSTAMP() ((uint64_t)0)
#endif
// Stamp slots per wave (tools/stamps.py): entry, ring filled, loop end, exit, transformed,
// quantized, first step, arguments fetched (kq_rows_dyn: units taken), x landed, and the norm
// interval's sums published, barrier passed, scale known, the passes of x the wave holds, and the
// interval after the barrier: first step's wait passed, chain started, stores issued.
constexpr int ROWS_STAMP_SLOTS = 16;
struct NormStamps {
    uint64_t pub = 0, bar = 0, scale = 0;
};

// The kernels' settled steps, each measured as a build switch of its own and then made the only
// form (DESIGN.md §7 "Retired build switches" names the record of each):
//  * the fused prologue issues exactly one weight step before the activation wait, its partial
//    last DMA instruction masked inside the asm so that it is issued on every path; the one
//    constant wait then leaves the residual load and that step in flight (tools/vmem_lint.py
//    checks that every s_waitcnt covering an inline-asm activation load is a constant);
//  * the norm prologue: waves that hold no part of the row go from the norm's barrier straight
//    to their ring fill; the wide forms quantize from the fast total and run the exactness guard
//    afterwards (norm_late); the row's total is a tree where nb is a power of two <= 64;
//  * the short-stream form (template parameter SH, rows_short_form in kq_common.h): at most D
//    steps straight-line, each wait a constant, and lane r keeps row r's result in a register.
#ifndef KQ_ROWS_LINT_BREAK
#define KQ_ROWS_LINT_BREAK 0  // 1: drop the activation wait (a lint self-test build, never run)
#endif

namespace kq {

// The GEMV's outputs (and the SWIGLU epilogue's) are stored write-through (sc1), so the next
// launch's activation is in the memory-side caches before the kernel boundary
// (tools/xfresh.hip: the consumer's fresh-read price 0.15 -> 0.03 us per edge;
// profiles/r04_store_flavour_ab.txt).
__device__ __forceinline__ void store_y(float *p, float v) {
    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

// Q8L quantization of whole rows (K > 8192 path): 16 superblocks per workgroup.
// AM: the prefill GEMMs' layout (quant16_store<true>: the mins operand in place of bsums).
template <bool AM>
__global__ void __launch_bounds__(WG_THREADS) kq_quantize_q8L(const float *__restrict__ x, int64_t x_stride,
                                                              uint8_t *__restrict__ y, int nb, int64_t nblocks) {
    const int lane = threadIdx.x & 63;
    const int64_t bi = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (bi >= nblocks) return;  // whole 16-lane rows drop out together
    const int64_t row = bi / nb;
    const int b = (int)(bi - row * nb);
    const float *xb = x + row * x_stride + (int64_t)b * QK + 16 * (lane & 15);
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *(const u32x4 *)(xb + 4 * k);
    quant16_store<AM>(v, lane & 15, y + bi * Q8L_STRIDE);
}
template __global__ void kq_quantize_q8L<false>(const float *, int64_t, uint8_t *, int, int64_t);
template __global__ void kq_quantize_q8L<true>(const float *, int64_t, uint8_t *, int, int64_t);

// ------------------------------------------------------------ prefill prologues
// The prompt graph's RMS_NORM -> MUL(norm weight) -> MUL_MATs and SWIGLU -> MUL_MAT:
// the op's arithmetic exactly as kq_rms_norm / kq_swiglu compute it (same sum order and
// exactness guard, (x*scale)*w; silu(g)*u on the NEON path), quantized straight into the
// GEMMs' Q8L blocks (row r's superblock b at (r*nb + b)*304); the f32 intermediate is
// never written.
__global__ void __launch_bounds__(256) kq_rms_norm_q8L(const float *__restrict__ x, const float *__restrict__ w,
                                                       uint8_t *__restrict__ yq, int64_t n, float eps) {
    extern __shared__ __attribute__((aligned(16))) double sb_sum[];
    const int64_t row = blockIdx.x;
    const float *xr = x + row * n;
    const int nb = (int)(n / QK);
    const int rid = threadIdx.x >> 4, l = threadIdx.x & 15;
    for (int b0 = 0; b0 < nb; b0 += 16) {
        const int b = b0 + rid;
        double s = 0.0;
        if (b < nb) {
            float v[16];
            const float4 *p = (const float4 *)(xr + (int64_t)b * QK + 16 * l);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 t = p[k];
                v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
            }
            s = sumsq16(v);
        }
        s = row16_sum(s);
        if (b < nb && l == 0) sb_sum[b] = s;
    }
    __syncthreads();
    double total = seq_sum_lds(sb_sum, nb);  // superblocks in order
    if (rms_mean_ambiguous(div_by_count(total, n), n)) {  // ggml's sequential order (block-uniform)
        __syncthreads();
        if (threadIdx.x < 64) {
            const double s = seq_sumsq_wave(xr, n, threadIdx.x);
            if (threadIdx.x == 0) sb_sum[0] = s;
        }
        __syncthreads();
        total = sb_sum[0];
    }
    const float mean = (float)div_by_count(total, n);
    const float scale = 1.0f / sqrtf(mean + eps);
    for (int b0 = 0; b0 < nb; b0 += 16) {
        const int b = b0 + rid;  // uniform over the 16-lane row: quant16_store's DPP row
        if (b >= nb) continue;
        const float4 *p = (const float4 *)(xr + (int64_t)b * QK + 16 * l);
        const float4 *q = (const float4 *)(w + (int64_t)b * QK + 16 * l);
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 t = p[k], m = q[k];
            v[k].x = __float_as_uint((t.x * scale) * m.x);
            v[k].y = __float_as_uint((t.y * scale) * m.y);
            v[k].z = __float_as_uint((t.z * scale) * m.z);
            v[k].w = __float_as_uint((t.w * scale) * m.w);
        }
        quant16_store<true>(v, l, yq + (row * nb + b) * Q8L_STRIDE);  // (prefill only: Q8L/mmq)
    }
}

__global__ void __launch_bounds__(256) kq_swiglu_q8L(const float *__restrict__ g, const float *__restrict__ u,
                                                     uint8_t *__restrict__ yq, int nb, int64_t nblocks) {
    const int64_t bi = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);  // superblock (row * nb + b)
    if (bi >= nblocks) return;  // whole 16-lane rows drop out together
    const int l = threadIdx.x & 15;
    const int64_t e0 = bi * QK + 16 * l;  // rows are contiguous: element index = superblock * 256 + ...
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 gv = *(const float4 *)(g + e0 + 4 * k), uv = *(const float4 *)(u + e0 + 4 * k);
        v[k].x = __float_as_uint(v_silu(gv.x) * uv.x);
        v[k].y = __float_as_uint(v_silu(gv.y) * uv.y);
        v[k].z = __float_as_uint(v_silu(gv.z) * uv.z);
        v[k].w = __float_as_uint(v_silu(gv.w) * uv.w);
    }
    (void)nb;
    quant16_store<true>(v, l, yq + bi * Q8L_STRIDE);  // (prefill only: Q8L/mmq)
}

int launch_rms_norm_q8L(const float *x, const float *w, void *yq, int64_t n, int64_t nrows, float eps, hipStream_t s) {
    if (nrows == 0) return MI355X_OK;
    const size_t lds = (size_t)(n / QK) * 8 + 8;
    return timed_launch("kq::kq_rms_norm_q8L", (double)nrows * (n * 4.0 + (n / QK) * (double)Q8L_STRIDE) + n * 4.0,
                        kq_rms_norm_q8L, dim3((unsigned)nrows), dim3(256), lds, s, x, w, (uint8_t *)yq, n, eps);
}

int launch_swiglu_q8L(const float *g, const float *u, void *yq, int64_t n, int64_t nrows, hipStream_t s) {
    const int64_t nb = n / QK, nblocks = nb * nrows;
    if (nblocks == 0) return MI355X_OK;
    const int64_t wgs = (nblocks + 15) / 16;
    return timed_launch("kq::kq_swiglu_q8L", (double)nblocks * (QK * 8.0 + Q8L_STRIDE), kq_swiglu_q8L, dim3((unsigned)wgs),
                        dim3(256), 0, s, g, u, (uint8_t *)yq, (int)nb, nblocks);
}

// ---------------------------------------------------------------- kernel entry
// The leading parameters (KQ_ROWS_PARAMS, kq_common.h), in SGPRs at wave start with the
// kernarg preload: the activation loads need nothing else.
struct RowsLead {
    const void *x;  // f32 activation; the Q8L row when !FUSEDQ
    const float *x2;
    const uint8_t *w0;
    const float *res0;
    int nb, waves_total, grid, nwv, qiters, n_desc, diag, rbase0, rrem0;
};
__device__ __forceinline__ RowsLead rows_lead(const void *x, const float *x2, const uint8_t *w0, const float *res0,
                                              int nb, int waves_total, int grid, int cfg, int rbase0, int rrem0) {
    RowsLead ld;
    ld.x = x, ld.x2 = x2, ld.w0 = w0, ld.res0 = res0;
    ld.nb = nb, ld.waves_total = waves_total, ld.grid = grid;
    ld.nwv = cfg & 0xff, ld.qiters = (cfg >> 8) & 0xf, ld.n_desc = (cfg >> 12) & 0xf, ld.diag = (cfg >> 16) & 0x1ff;
    ld.rbase0 = rbase0, ld.rrem0 = rrem0;
    return ld;
}

// RowsArgs' entry run (kq_common.h: bR .. stamps_cap), fetched by hand: four wide scalar
// loads behind ONE wait, issued where the call stands (after the activation loads). Left to
// the compiler, kernarg loads are sunk to their first uses, one trip each behind later waits,
// or hoisted above the activation loads with a wait of their own. The product build reads
// 56 dwords; a diagnostic build 64 (the stamp buffer).
typedef uint32_t u32x8s __attribute__((ext_vector_type(8)));
typedef uint32_t u32x16s __attribute__((ext_vector_type(16)));
constexpr int kRowsArgsOff = 14 * 4;  // RowsArgs in the kernarg segment: after the 14 leading dwords
static_assert(alignof(RowsArgs) == 8 && kRowsArgsOff % 8 == 0, "RowsArgs follows the leading parameters unpadded");
#define RA_DW(f) ((int)(offsetof(RowsArgs, f) / 4))
#if KQ_ROWS_DIAG
typedef u32x16s rows_run_tail;
#define KQ_ROWS_RUN_TAIL "s_load_dwordx16"
static_assert(offsetof(RowsArgs, stamps_cap) + 8 <= 64 * 4 && sizeof(RowsArgs) >= 64 * 4, "entry run: 64 dwords");
#else
typedef u32x8s rows_run_tail;
#define KQ_ROWS_RUN_TAIL "s_load_dwordx8"
static_assert(offsetof(RowsArgs, n_rows) + 16 <= 56 * 4 && sizeof(RowsArgs) >= 56 * 4, "entry run: 56 dwords");
#endif
struct RowsRun {
    u32x16s a, b, c;
    rows_run_tail d;
    template <int I>
    __device__ __forceinline__ uint32_t dw() const {
        if constexpr (I < 16) return a[I];
        else if constexpr (I < 32) return b[I - 16];
        else if constexpr (I < 48) return c[I - 32];
        else return d[I - 48];
    }
    template <int I>
    __device__ __forceinline__ int i32() const {
        return (int)dw<I>();
    }
    template <class T, int I>
    __device__ __forceinline__ T *ptr() const {
        return (T *)(uintptr_t)((uint64_t)dw<I>() | ((uint64_t)dw<I + 1>() << 32));
    }
};
__device__ __forceinline__ RowsRun rows_fetch() {
    const auto *ka = __builtin_amdgcn_kernarg_segment_ptr();
    RowsRun r;
    asm volatile("s_load_dwordx16 %0, %4, %5\n\t"
                 "s_load_dwordx16 %1, %4, %6\n\t"
                 "s_load_dwordx16 %2, %4, %7\n\t" KQ_ROWS_RUN_TAIL " %3, %4, %8\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(r.a), "=&s"(r.b), "=&s"(r.c), "=&s"(r.d)
                 : "s"(ka), "i"(kRowsArgsOff), "i"(kRowsArgsOff + 64), "i"(kRowsArgsOff + 128), "i"(kRowsArgsOff + 192));
    return r;
}

// A value of the run in scalar registers of its own from here on: picking among elements of
// one loaded vector by a run-time index would otherwise become an indexed read of the vector
// (through scratch).
template <class T>
__device__ __forceinline__ T sreg(T v) {
    asm volatile("" : "+s"(v));
    return v;
}

// Everything else a wave of kq_rows needs, resolved for its matrix m.
struct RowsHot {
    int m, r0, nrows;  // this wave's matrix and rows [r0, r0 + nrows)
    int type, bR, rpw;
    const uint8_t *w;
    const float *res;
    float *y;
    float eps;
    int epi, epi_n, epi_wave_off;
    float *epi_y;
    uint64_t *stamps;
    int64_t stamps_cap;
};

// The entry run, then this wave's matrix, picked from the loaded arrays with scalar selects:
// with one matrix (o-proj, down, the head) the leading parameters hold its values and nothing
// is searched or picked.
template <int TMASK>
__device__ __forceinline__ RowsHot rows_resolve(const RowsLead &ld, int gw) {
    const RowsRun r = rows_fetch();
    RowsHot h;
    h.bR = r.i32<RA_DW(bR)>(), h.rpw = r.i32<RA_DW(rpw)>();
    h.epi = r.i32<RA_DW(epi)>(), h.epi_n = r.i32<RA_DW(epi_n)>(), h.epi_wave_off = r.i32<RA_DW(epi_wave_off)>();
    h.eps = __uint_as_float(r.dw<RA_DW(eps)>());
    h.epi_y = r.ptr<float, RA_DW(epi_y)>();
#if KQ_ROWS_DIAG
    h.stamps = r.ptr<uint64_t, RA_DW(stamps)>();
    h.stamps_cap = (int64_t)(uintptr_t)r.ptr<uint8_t, RA_DW(stamps_cap)>();
#else
    h.stamps = nullptr, h.stamps_cap = 0;
#endif
    h.m = 0, h.w = ld.w0, h.res = ld.res0;
    h.type = TMASK == 7 ? sreg(r.i32<RA_DW(type)>()) : 0;
    h.y = sreg(r.ptr<float, RA_DW(y)>());
    int j = gw, base = ld.rbase0, rem = ld.rrem0;
    if (ld.n_desc > 1) {  // uniform over the launch
        const int p1 = sreg(r.i32<RA_DW(wave_prefix) + 1>()), p2 = sreg(r.i32<RA_DW(wave_prefix) + 2>()),
                  p3 = sreg(r.i32<RA_DW(wave_prefix) + 3>());
        const int b1 = sreg(r.i32<RA_DW(rbase) + 1>()), b2 = sreg(r.i32<RA_DW(rbase) + 2>()), b3 = sreg(r.i32<RA_DW(rbase) + 3>());
        const int e1 = sreg(r.i32<RA_DW(rrem) + 1>()), e2 = sreg(r.i32<RA_DW(rrem) + 2>()), e3 = sreg(r.i32<RA_DW(rrem) + 3>());
        const uint8_t *w1 = sreg(r.ptr<const uint8_t, RA_DW(w) + 2>()), *w2 = sreg(r.ptr<const uint8_t, RA_DW(w) + 4>()),
                      *w3 = sreg(r.ptr<const uint8_t, RA_DW(w) + 6>());
        const float *s1 = sreg(r.ptr<const float, RA_DW(res) + 2>()), *s2 = sreg(r.ptr<const float, RA_DW(res) + 4>()),
                    *s3 = sreg(r.ptr<const float, RA_DW(res) + 6>());
        float *y1 = sreg(r.ptr<float, RA_DW(y) + 2>()), *y2 = sreg(r.ptr<float, RA_DW(y) + 4>()), *y3 = sreg(r.ptr<float, RA_DW(y) + 6>());
        int m = gw >= p1 ? 1 : 0;
        if (ld.n_desc > 2 && gw >= p2) m = 2;
        if (ld.n_desc > 3 && gw >= p3) m = 3;
        h.m = m;
        j = gw - (m == 0 ? 0 : m == 1 ? p1 : m == 2 ? p2 : p3);
        base = m == 0 ? base : m == 1 ? b1 : m == 2 ? b2 : b3;
        rem = m == 0 ? rem : m == 1 ? e1 : m == 2 ? e2 : e3;
        if (TMASK == 7) {
            const int t1 = sreg(r.i32<RA_DW(type) + 1>()), t2 = sreg(r.i32<RA_DW(type) + 2>()), t3 = sreg(r.i32<RA_DW(type) + 3>());
            h.type = m == 0 ? h.type : m == 1 ? t1 : m == 2 ? t2 : t3;
        }
        h.w = m == 0 ? h.w : m == 1 ? w1 : m == 2 ? w2 : w3;
        h.res = m == 0 ? h.res : m == 1 ? s1 : m == 2 ? s2 : s3;
        h.y = m == 0 ? h.y : m == 1 ? y1 : m == 2 ? y2 : y3;
    }
    h.r0 = j * base + (j < rem ? j : rem);
    h.nrows = gw < ld.waves_total ? base + (j < rem ? 1 : 0) : 0;
    return h;
}

// ---------------------------------------------------------------- the FUSEDQ prologue
// The activation of a fused-quantization launch, shared by kq_rows, kq_rows_dyn and
// kq_rows_prologue_dbg: load() issues the wave's inline-asm loads of x (and of x2: the norm
// weight / up) from the leading parameters alone; the caller issues what it wants in flight
// behind them and waits for them (ONE constant s_waitcnt vmcnt per path, tools/vmem_lint.py);
// finish() pins the registers, applies the transform (PRO) and quantizes into the
// workgroup's Q8L row in LDS. The caller's workgroup barrier completes the row.
//
// Mapping (rows_pro_form, chosen by the host per launch; LSH is a template parameter of the
// kernels: one form's code per kernel, a form picked at run time cost the token 3.5 %,
// profiles/r08_prologue_ab.txt): 16 << LSH lanes hold one superblock, 16 >> LSH consecutive
// values per lane (4 >> LSH 16-B loads of x). LSH = 0: 4 superblocks per wave and pass, up to
// ROWS_QPASS passes of 4 * nwv superblocks; LSH = 1, 2: one pass of 2 or 1 superblocks per
// wave over as many waves as the row has superblocks for.
template <int LSH>
struct RowsPrologue {
    static constexpr int NP = LSH ? 1 : ROWS_QPASS;  // passes held in registers
    static constexpr int NL = 4 >> LSH;              // 16-B loads per pass and vector
    static constexpr int LP = 16 << LSH;             // lanes per superblock
    static constexpr int SPW = 4 >> LSH;             // superblocks per wave and pass
    // The registers of the asm loads: claimed by an empty asm (no instruction, no value: a pass
    // the wave does not load is never read) and loaded in place (gload16_into), so a register
    // is the same one on the path that loads it and on the path that skips the load.
    u32x4 xv[NP][NL];
    u32x4 x2v[NP][NL];  // norm weight / up, same elements as xv
    int qw = 0;  // passes this wave loads (wave-uniform): pass i while its first slot lies in the row
    int nb, pass, wave, lane;

    // slot of pass i held by this lane, its lane index within the superblock, slot -> superblock:
    // slots past the row read superblock nb-1's place and store nothing
    __device__ __forceinline__ int slot(int i) const { return pass * i + SPW * wave + (lane >> (4 + LSH)); }
    __device__ __forceinline__ int sl() const { return lane & (LP - 1); }
    __device__ __forceinline__ int sbk(int j) const { return j < nb ? j : nb - 1; }

    // ASM: the kernels' inline-asm loads, which the caller waits for; false (the debug kernel):
    // ordinary loads that the compiler waits for itself
    template <int PRO, bool ASM = true>
    __device__ __forceinline__ void load(const RowsLead &ld, int wave_, int lane_, int diag) {
        nb = ld.nb, pass = SPW * ld.nwv, wave = wave_, lane = lane_;
        const float *const x = (const float *)ld.x;
        // (diag bit 4: read x again instead of x2, timing only)
        const float *const x2 = (diag & 16) ? x : ld.x2;
#pragma unroll
        for (int i = 0; i < NP; ++i) qw += (i < ld.qiters && pass * i + SPW * wave < nb) ? 1 : 0;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int k = 0; k < NL; ++k) {
                asm volatile("" : "=v"(xv[i][k]));
                if (PRO != ROWS_PRO_NONE) asm volatile("" : "=v"(x2v[i][k]));
            }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (i < qw) {  // waves past the row load nothing
                const int64_t e = (int64_t)sbk(slot(i)) * QK + (16 >> LSH) * sl();
#pragma unroll
                for (int k = 0; k < NL; ++k) {
                    if (ASM) gload16_into(xv[i][k], x + e + 4 * k);
                    else xv[i][k] = *(const u32x4 *)(x + e + 4 * k);
                }
                if (PRO != ROWS_PRO_NONE) {
#pragma unroll
                    for (int k = 0; k < NL; ++k) {
                        if (ASM) gload16_into(x2v[i][k], x2 + e + 4 * k);
                        else x2v[i][k] = *(const u32x4 *)(x2 + e + 4 * k);
                    }
                }
            }
        }
    }

    // the asm loads are invisible to the compiler: pin their registers past each wait
    template <int PRO>
    __device__ __forceinline__ void pin() {
        if constexpr (LSH == 0) {
            asm volatile("" : "+v"(xv[0][0]), "+v"(xv[0][1]), "+v"(xv[0][2]), "+v"(xv[0][3]), "+v"(xv[1][0]),
                         "+v"(xv[1][1]), "+v"(xv[1][2]), "+v"(xv[1][3]), "+v"(xv[2][0]), "+v"(xv[2][1]),
                         "+v"(xv[2][2]), "+v"(xv[2][3]));
        } else {
#pragma unroll
            for (int k = 0; k < NL; ++k) asm volatile("" : "+v"(xv[0][k]));
        }
        if (PRO != ROWS_PRO_NONE) {
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int k = 0; k < NL; ++k) asm volatile("" : "+v"(x2v[i][k]));
        }
    }

    // ggml_vec_swiglu_f32 on pass i: silu(gate) * up
    __device__ __forceinline__ void swiglu_pass(int i) {
#pragma unroll
        for (int k = 0; k < NL; ++k) xv[i][k] = swiglu4(xv[i][k], x2v[i][k]);
    }

    // this lane's 16 >> LSH values of pass i, in order
    __device__ __forceinline__ void values(int i, float v[4 * NL]) const {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            v[4 * k] = __uint_as_float(xv[i][k].x), v[4 * k + 1] = __uint_as_float(xv[i][k].y);
            v[4 * k + 2] = __uint_as_float(xv[i][k].z), v[4 * k + 3] = __uint_as_float(xv[i][k].w);
        }
    }

    // rms_norm then MUL by the norm weight: this wave's superblock sums of squares to `sums`
    // (LDS), a workgroup barrier, the row's total from them on every wave that holds a part of
    // the row (a wave without one goes on to its ring fill; it has joined the
    // barrier, so every wave passes the same barriers). The fast order: the lane's 16 >> LSH
    // squares in order, the xor tree over the superblock's lanes (every aligned group of 16
    // elements is a subtree for every LSH), then the superblocks as a tree where nb is a power
    // of two <= 64 (at most 16 + 6 + 6 adds per value), else in order. The rare rows
    // whose float mean could depend on the order (rms_mean_ambiguous, whose bound holds for any
    // order of at most n + 32 adds per value) are summed again in ggml's order, by each wave:
    // the test is workgroup-uniform, every wave sums the same LDS values by the same instructions.
    __device__ __forceinline__ void norm_publish(double *sums) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (i < qw) {  // wave-uniform: this wave holds x of the pass
                const int j = slot(i);
                double sq = 0.0;
                if (j < nb) {
                    float v[4 * NL];
#pragma unroll
                    for (int k = 0; k < NL; ++k) {
                        v[4 * k] = __uint_as_float(xv[i][k].x), v[4 * k + 1] = __uint_as_float(xv[i][k].y);
                        v[4 * k + 2] = __uint_as_float(xv[i][k].z), v[4 * k + 3] = __uint_as_float(xv[i][k].w);
                    }
                    if constexpr (LSH == 0) {
                        sq = sumsq16(v);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4 * NL; ++k) sq += (double)(v[k] * v[k]);
                    }
                }
                // DPP / lane swaps, every lane of the wave active
                if constexpr (LSH == 0) sq = row16_sum(sq);
                else sq = sblk_sum<LP>(sq);
                if (j < nb && sl() == 0) sums[sbk(j)] = sq;
            }
        }
    }
    __device__ __forceinline__ double norm_total(const double *sums) const {
        if (nb <= 64 && (nb & (nb - 1)) == 0) return tree_sum_lanes(sums, nb, lane);
        return seq_sum_lanes(sums, nb, lane);  // superblocks in order
    }
    static __device__ __forceinline__ float norm_scale(double tot, int64_t n, float eps) {
        const float mean = (float)div_by_count(tot, n);
        return 1.0f / sqrtf(mean + eps);
    }

    // The 16-lane form: total, guard, scale, transform in place.
    __device__ __forceinline__ void norm(double *sums, const float *x, float eps, NormStamps &ns) {
        norm_publish(sums);
        ns.pub = RSTAMP();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        ns.bar = RSTAMP();
        if (qw == 0) return;
        const int64_t n = (int64_t)nb * QK;
        double tot = norm_total(sums);
        if (rms_mean_ambiguous(div_by_count(tot, n), n)) tot = seq_sumsq_wave(x, n, lane);
        float scale = norm_scale(tot, n, eps);
        if (KQ_ROWS_DIAG) asm volatile("" : "+v"(scale));  // (the stamp behind the value)
        ns.scale = RSTAMP();
#pragma unroll
        for (int i = 0; i < NP; ++i)
            if (i < qw)
#pragma unroll
                for (int k = 0; k < NL; ++k) xv[i][k] = normmul4(xv[i][k], x2v[i][k], scale);
    }

    // the wide forms' one pass, transformed into `t`, into the Q8L row at `act`
    __device__ __forceinline__ void quantize_wide(const u32x4 t[NL], uint8_t *act) {
        const int j = slot(0);
        float v[4 * NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            v[4 * k] = __uint_as_float(t[k].x), v[4 * k + 1] = __uint_as_float(t[k].y);
            v[4 * k + 2] = __uint_as_float(t[k].z), v[4 * k + 3] = __uint_as_float(t[k].w);
        }
        quant_wide_store<LP>(v, sl(), act + Q8L_STRIDE * sbk(j), j < nb);
    }

    // The wide forms: the guard after the quantized row is stored. Scale from the
    // fast total, transform into registers of their own (x stays), quantize and store; then the
    // guard, and on an ambiguous row the sum in ggml's order, the transform and the quantization
    // again from x, over this wave's own blocks (same lanes, same addresses, LDS in order). The
    // decision is the same on every wave that holds x, so no barrier is added; the caller's
    // closing barrier publishes whichever blocks were stored last.
    __device__ __forceinline__ void norm_late(uint8_t *act, double *sums, const float *x, float eps, int diag, bool stamp,
                                              uint64_t &sx, NormStamps &ns) {
        static_assert(LSH >= 1 && NP == 1, "one pass in registers");
        norm_publish(sums);
        ns.pub = RSTAMP();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        ns.bar = RSTAMP();
        if (qw == 0) {
            if (stamp) sx = __builtin_amdgcn_s_memrealtime();
            return;
        }
        const int64_t n = (int64_t)nb * QK;
        const double md = div_by_count(norm_total(sums), n);
        float scale = 1.0f / sqrtf((float)md + eps);
        if (KQ_ROWS_DIAG) asm volatile("" : "+v"(scale));
        ns.scale = RSTAMP();
        u32x4 t[NL];
        if (qw) {
#pragma unroll
            for (int k = 0; k < NL; ++k) t[k] = normmul4(xv[0][k], x2v[0][k], scale);
        }
        if (stamp) sx = __builtin_amdgcn_s_memrealtime();
        if (qw && !(diag & 64)) quantize_wide(t, act);
        double mdg = md;
        asm volatile("" : "+v"(mdg));  // the guard's arithmetic stays behind the stores
        if (rms_mean_ambiguous(mdg, n)) {  // about one row in 10^4-10^5
            scale = norm_scale(seq_sumsq_wave(x, n, lane), n, eps);
            if (qw) {
#pragma unroll
                for (int k = 0; k < NL; ++k) t[k] = normmul4(xv[0][k], x2v[0][k], scale);
                if (!(diag & 64)) quantize_wide(t, act);
            }
        }
    }

    // pass i (wave-uniform, i < qw) into the Q8L row at `act`
    __device__ __forceinline__ void quantize_pass(int i, uint8_t *act) {
        const int j = slot(i);
        uint8_t *const qb = act + Q8L_STRIDE * sbk(j);
        if constexpr (LSH == 0) {
            u32x4 cur[4];  // one copy of the quantizer; pick the pass's registers
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // values, not lvalues: a pick among members would become a pick of addresses (scratch)
                const u32x4 p0 = xv[0][k], p1 = xv[1][k], p2 = xv[2][k];
                cur[k] = i == 0 ? p0 : i == 1 ? p1 : p2;
            }
            if (j < nb) quant16_store(cur, lane & 15, qb);
        } else {
            float v[4 * NL];
            values(0, v);
            quant_wide_store<LP>(v, sl(), qb, j < nb);
        }
    }

    // After the caller's wait for the loads: transform and quantize every pass. `sx`
    // (diagnostic builds): the time between the two. diag bits 32 / 64 (timing only): skip
    // the transform / the quantization.
    template <int PRO>
    __device__ __forceinline__ void finish(uint8_t *act, double *sums, const float *x, float eps, int diag, bool stamp,
                                           uint64_t &sx, NormStamps &ns) {
        pin<PRO>();
        if (diag & 32) {
        } else if (PRO == ROWS_PRO_SWIGLU) {
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (i < qw) swiglu_pass(i);
        } else if (PRO == ROWS_PRO_NORM) {
            if constexpr (LSH >= 1) {
                norm_late(act, sums, x, eps, diag, stamp, sx, ns);
                return;
            } else {
                norm(sums, x, eps, ns);
            }
        }
        if (stamp) sx = __builtin_amdgcn_s_memrealtime();
        if (!(diag & 64)) {
#pragma unroll 1
            for (int i = 0; i < qw; ++i) quantize_pass(i, act);
        }
    }
};

// The shared prologue alone (mi355x_debug_rows_prologue): one workgroup of cfg's waves runs
// load (with ordinary loads) / finish and copies its Q8L image (nb * 304 B) to `out`, so that a test sees the
// bytes the GEMV's dot products read (d and every q of a block flip together with a wrong
// tie sign: the GEMV's outputs cannot show it).
template <int PRO, int LSH>
__global__ void __launch_bounds__(ROWS_WAVES * 64) kq_rows_prologue_dbg(const float *x, const float *x2, int nb, int cfg,
                                                                        float eps, uint8_t *out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RowsLead ld = rows_lead(x, x2, nullptr, nullptr, nb, 0, 1, cfg, 0, 0);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    RowsPrologue<LSH> pg;
    pg.template load<PRO, false>(ld, wave, lane, 0);
    uint64_t sx = 0;
    NormStamps ns;
    pg.template finish<PRO>(smem, (double *)(smem + nb * Q8L_STRIDE), x, eps, 0, false, sx, ns);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int ng = nb * (Q8L_STRIDE / 16);
    for (int k = threadIdx.x; k < ng; k += ld.nwv * 64) ((u32x4 *)out)[k] = ((const u32x4 *)smem)[k];
}

template <int PRO>
static auto rows_prologue_dbg_fn(int lsh) {
    return lsh == 2 ? kq_rows_prologue_dbg<PRO, 2> : lsh == 1 ? kq_rows_prologue_dbg<PRO, 1> : kq_rows_prologue_dbg<PRO, 0>;
}

int launch_rows_prologue_dbg(int pro, const float *x, const float *x2, float eps, int nb, int waves, uint8_t *out,
                             hipStream_t s) {
    const RowsProForm f = rows_pro_form(nb, waves);
    const int cfg = rows_cfg(waves, f.passes, 1, 0);
    const size_t lds = (size_t)nb * Q8L_STRIDE + (size_t)nb * 8;
    const auto fn = pro == ROWS_PRO_NORM ? rows_prologue_dbg_fn<ROWS_PRO_NORM>(f.lsh)
                    : pro == ROWS_PRO_SWIGLU ? rows_prologue_dbg_fn<ROWS_PRO_SWIGLU>(f.lsh)
                                             : rows_prologue_dbg_fn<ROWS_PRO_NONE>(f.lsh);
    allow_lds((const void *)fn, lds);
    hipLaunchKernelGGL(fn, dim3(1), dim3(waves * 64), lds, s, x, x2, nb, cfg, eps, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MI355X_OK : (int)e;
}

// The fused prologue of kq_rows and kq_rows_dyn is one sequence. After the activation loads
// (pg.load) and the entry batch, each body issues the residual load and exactly one weight step's
// DMA instructions on every path, the partial last one with its lane mask inside the asm, and
// advances its own stream state; rows_fused_finish is the rest: the one constant wait, which
// leaves that load and that step in flight (tools/vmem_lint.py checks that every s_waitcnt
// covering an inline-asm activation load is a constant), then transform and quantization into
// the Q8L row at `act`. The residual load (this lane's residual of the fused ADD) is issued on
// every path, a dummy read of x without a residual, so that no branch joins a register whose asm
// load is still in flight; the body keeps `rv` live until its flush waits for it. An asm load
// whose register the compiler sees dead is reused while the load is in flight: a build with that
// branch compiled out faulted (profiles/r02_attn_epilogue_rejected.md).
// `ps`: the diagnostic builds' stamps (x landed, transformed, quantized, the norm interval's).
struct ProStamps {
    uint64_t landed = 0, transformed = 0, quantized = 0;
    NormStamps ns;
};
template <int TYPE, int PRO, int LSH>
__device__ __forceinline__ void rows_fused_finish(RowsPrologue<LSH> &pg, const float *x, uint8_t *act, double *sums,
                                                  float eps, int diag, bool stamps, ProStamps &ps) {
    // x landed: the residual load (younger than x) and the step's DMA instructions (all issued
    // on every path) may still be in flight
    if (!KQ_ROWS_LINT_BREAK) vm_wait<rows_ni(TYPE) + 1>();  // (1: tests/test_abi.py, the ISA lint must flag the build)
    ps.landed = RSTAMP();
    pg.template finish<PRO>(act, sums, x, eps, diag, stamps, ps.transformed, ps.ns);
    if (stamps) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ps.quantized = __builtin_amdgcn_s_memrealtime();
    }
}

// The SWIGLU epilogue's value for row r, n4 = n & ~3 rows in the vector body: the arithmetic of
// kq_swiglu (ggml_vec_swiglu_f32: NEON body, libm tail).
__device__ __forceinline__ float rows_swiglu_out(float gv, float uv, int r, int n4) {
    return r < n4 ? v_silu(gv) * uv : (gv / (1.0f + expf(-gv))) * uv;
}

// A wave's stamps (diagnostic builds; the slots' meanings above and in tools/stamps.py). Slot 3,
// the exit, is taken here.
__device__ __forceinline__ void rows_put_stamps(uint64_t *stamps, int64_t cap, int wave, int lane,
                                                const uint64_t (&v)[ROWS_STAMP_SLOTS]) {
    const int64_t o = ((int64_t)blockIdx.x * ROWS_WAVES + wave) * ROWS_STAMP_SLOTS;  // sized for the most waves
    if (lane == 0 && o + ROWS_STAMP_SLOTS - 1 < cap) {
#pragma unroll
        for (int k = 0; k < ROWS_STAMP_SLOTS; ++k) stamps[o + k] = k == 3 ? __builtin_amdgcn_s_memrealtime() : v[k];
    }
}

// `resolve` returns the wave's RowsHot: called after the activation loads are issued (they
// need the leading parameters only), or before the call where the type depends on the matrix.
//
// SH, the short-stream form (the host's choice per launch, rows_short_form): every wave of the
// launch streams at most D steps, so its whole stream is issued before the prologue's barrier
// and nothing is issued after it, and its rows are one chain batch. The steps run without ring
// wrap, batch bookkeeping or issue; integer sums, records and the chain are the generic form's.
template <int TYPE, bool FUSEDQ, int PRO, int TMASK, int LSH, bool SH, class Resolve>
__device__ __forceinline__ void rows_body(const RowsLead &ld, uint8_t *smem, int wave, int lane,
                                          uint64_t st0, Resolve resolve) {
    static_assert(!SH || FUSEDQ, "the short form is built for the fused-quantization launches");
    constexpr int BSZ = block_bytes(TYPE);
    constexpr int NI = rows_ni(TYPE);
    constexpr int PART = rows_gran(TYPE) - 64 * (NI - 1);  // lanes of a step's partial last DMA instruction
    constexpr int SLOT = rows_slot(TYPE);
    constexpr int D = rows_depth(TYPE);
    static_assert(D >= 2 && D <= 4, "vm_wait_k covers 3 steps in flight");
    const int nb = ld.nb;
    const int nwv = ld.nwv;  // waves in this workgroup
    const int q = lane >> 2, s = lane & 3;

    // ---- activation loads first: every wave's requests leave before any argument fetch
    RowsPrologue<LSH> pg;
    if (FUSEDQ) pg.template load<PRO>(ld, wave, lane, RDIAG(ld));
    const RowsHot h = resolve();
    const uint64_t sa = RSTAMP();  // diagnostics: arguments fetched
    const int bR = h.bR;
    const RowsLayout L = rows_layout(nb, TMASK, bR, h.rpw, nwv);
    uint8_t *const ring = smem + L.ring + wave * L.ring_stride;
    uint8_t *const ring_end = ring + D * SLOT;
    RowRec *const recs = (RowRec *)(smem + L.recs + wave * L.recs_stride);
    float *const outs = (float *)(smem + L.outs + wave * L.outs_stride);
    const uint8_t *const actq = smem + L.act;

    // weight stream of this wave
    const int G = h.nrows * nb;               // superblocks
    const int T = (G + ROWS_SB - 1) / ROWS_SB;  // steps
    const uint8_t *src = h.w + (int64_t)h.r0 * nb * BSZ;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);
    const uint8_t *s16 = src - mis;
    const uint8_t *last16 =
        G > 0 ? (const uint8_t *)((uintptr_t)(src + (int64_t)G * BSZ - 1) & ~(uintptr_t)15) : s16;

    // SH: the steps' state, none of which needs the activation: the quad's superblock e_g of the
    // stream (q in step 0), its block and row-in-batch (one division where a step holds whole
    // rows), the LDS offsets of its weight block, activation block and record, and what a step
    // of 16 superblocks advances (row, block) by. They stand in front of the activation wait in
    // the source; pinning them there by an empty asm changed nothing for the token
    // (profiles/r10_short_ab.txt section 2) and was taken out.
    int e_outs = L.outs + wave * L.outs_stride, e_a16 = 0, e_b16 = ROWS_SB;
    int e_g = q, e_io = q, e_rr = 0, e_blk = 0, e_act = 0, e_rec = 0;
    if constexpr (SH) {
        if (nb <= ROWS_SB) {  // uniform
            e_a16 = (int)((unsigned)ROWS_SB / (unsigned)nb);
            e_b16 = ROWS_SB - e_a16 * nb;
            e_rr = (int)((unsigned)q / (unsigned)nb);
            e_io = q - e_rr * nb;
        }
        e_blk = L.ring + wave * L.ring_stride + (int)mis + q * BSZ;
        e_act = L.act + e_io * Q8L_STRIDE;
        // (24-bit multiply: the 64-bit multiply-add the compiler picks for io * bR + rr names a
        // register pair whose unused half can be the residual load's, in flight here)
        e_rec = L.recs + wave * L.recs_stride + (__mul24(e_io, bR) + e_rr) * (int)sizeof(RowRec);
    }

    uint8_t *islot = ring;
    int it_ = 0;  // next step to issue
    auto issue = [&]() {
        rows_issue_step<TYPE>(s16 + (int64_t)it_ * (ROWS_SB * BSZ) + 16 * lane, last16, islot, lane, it_ + 1 < T);
        islot = islot + SLOT == ring_end ? ring : islot + SLOT;
        ++it_;
    };

    const float *const res_p = h.res;
    uint32_t rv = 0;  // residual of the fused ADD for row r0 + lane (first 64 rows)

    // ---- prologue: activation loads, one weight step, quantize, then the rest of the ring
    uint64_t sf = 0;  // diagnostics: first step computed
    ProStamps ps;
    if (FUSEDQ) {
        // residual of the fused ADD: one row per lane, fetched with the activation
        const float *const x = (const float *)ld.x;
        rv = gload4_asm(res_p && h.nrows > 0 ? res_p + h.r0 + (lane < h.nrows ? lane : 0) : x);
        // Exactly one step's DMA instructions on every path: a wave without rows (T == 0) issues
        // them from the activation (valid memory, into a ring slot it never reads)
        if (T == 0) {
            const uint8_t *xb = (const uint8_t *)x + 16 * lane;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (i + 1 == NI) dma16_nt_lanes(xb, (LDS void *)(islot + 1024 * i), lane, PART);
                else dma16_nt(xb, (LDS void *)(islot + 1024 * i));
        }
        if (T > 0) {  // the one step, its partial DMA masked in asm
            const uint8_t *base = s16 + 16 * lane;
            const uint8_t *lim = T > 1 ? base + 1024 * (NI - 1) : base + 1024 * (NI - 1) < last16 ? base + 1024 * (NI - 1) : last16;
#pragma unroll
            for (int i = 0; i + 1 < NI; ++i) {
                const uint8_t *p = base + 1024 * i;
                dma16_nt(T > 1 || p < last16 ? p : last16, (LDS void *)(islot + 1024 * i));
            }
            dma16_nt_lanes(lim, (LDS void *)(islot + 1024 * (NI - 1)), lane, PART);
            islot = islot + SLOT == ring_end ? ring : islot + SLOT;
            ++it_;
        }
        rows_fused_finish<TYPE, PRO>(pg, x, smem + L.act, (double *)(smem + L.sums), h.eps, RDIAG(ld), RSTAMPS(h) != nullptr, ps);
    } else {
        const int ng = nb * (Q8L_STRIDE / 16);
        for (int j = wave; 64 * j < ng; j += nwv) {
            const int k = 64 * j + lane;
            if (k < ng) dma16((const uint8_t *)ld.x + 16 * k, (LDS void *)(smem + L.act + 1024 * j));
        }
        // one weight step in front of the wait for the row: min(T, 1), written so that the
        // compiler sees 0 <= pre0 <= 1 (T >= 0)
        const int pre0 = T >= 1 ? 1 : (T > 0 ? T : 0);
        for (int j = 0; j < pre0; ++j) issue();
        vm_wait_k<NI>(pre0);
    }
    if constexpr (SH) {
        // the rest of the stream (T <= D): step j into slot j, every granule clamped to the last
#pragma unroll
        for (int j = 1; j < D; ++j)
            if (j < T) rows_issue_step<TYPE>(s16 + j * (ROWS_SB * BSZ) + 16 * lane, last16, ring + j * SLOT, lane, false);
    } else {
        while (it_ < D && it_ < T) issue();
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // Q8_K row complete (no vmcnt drain)
    const uint64_t st1 = RSTAMPS(h) ? __builtin_amdgcn_s_memrealtime() : 0;
    uint64_t st2 = 0, sw = 0, sc = 0, ss = 0;  // diagnostics: loop end, first wait passed, chain start, stores issued
    auto put_stamps = [&]() {
        if (RSTAMPS(h)) {
            const uint64_t v[ROWS_STAMP_SLOTS] = {st0, st1, st2, 0, ps.transformed, ps.quantized, sf, sa, ps.landed,
                                                  ps.ns.pub, ps.ns.bar, ps.ns.scale, (uint64_t)pg.qw, sw, sc, ss};
            rows_put_stamps(RSTAMPS(h), h.stamps_cap, wave, lane, v);
        }
    };

    if constexpr (SH) {
        // ---- the short form's steps: copy k runs the step that has k younger steps in flight
        // (step T - 1 - k), so each copy's wait is a constant and a wave with fewer steps enters
        // at a later copy. The state (e_*) advances by one step of 16 superblocks.
        auto step = [&](bool advance) {
            if (!(RDIAG(ld) & 8) && e_g < G) rows_quad_step<TYPE>(smem + e_blk, smem + e_act, s, (RowRec *)(smem + e_rec));
            if (advance) {
                e_g += ROWS_SB, e_blk += SLOT;
                e_io += e_b16, e_rr += e_a16;
                if (e_io >= nb) e_io -= nb, ++e_rr;
                e_act = L.act + e_io * Q8L_STRIDE;
                e_rec = L.recs + wave * L.recs_stride + (__mul24(e_io, bR) + e_rr) * (int)sizeof(RowRec);
            }
        };
        auto copy = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (T > k) {  // uniform
                vm_wait<NI * k>();
                if (RSTAMPS(h) && T == k + 1) sw = __builtin_amdgcn_s_memrealtime();
                step(k > 0);
                if (RSTAMPS(h) && T == k + 1) sf = __builtin_amdgcn_s_memrealtime();
            }
        };
        if constexpr (D > 3) copy(std::integral_constant<int, 3>{});
        if constexpr (D > 2) copy(std::integral_constant<int, 2>{});
        copy(std::integral_constant<int, 1>{});
        copy(std::integral_constant<int, 0>{});
        // ---- the one chain batch: lane r replays row r's records in superblock order and keeps
        // the result; the residual add and the store come from the register
        float v = 0.f;
        float *const outs_s = (float *)(smem + e_outs);
        if (h.nrows > 0) {
            wave_lds_fence();
            sc = RSTAMP();
            if (lane < h.nrows) {
                v = rows_chain<TYPE>((const RowRec *)(smem + L.recs + wave * L.recs_stride) + lane, nb, bR);
            }
            if (KQ_ROWS_DIAG) asm volatile("" : "+v"(v));  // (the stamp behind the value)
            st2 = RSTAMP();
            float *y = h.y + h.r0;
            if (res_p) {  // ggml_add(mul_mat, residual): the same single f32 add per element
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("" : "+v"(rv));
                if (lane < h.nrows) store_y(y + lane, v + __uint_as_float(rv));
            } else {
                if (lane < h.nrows) store_y(y + lane, v);
            }
            ss = RSTAMP();
        }
        // ---- SWIGLU epilogue: the gate wave stages its rows for its up partner, which keeps its own
        if (h.epi && !(RDIAG(ld) & 128)) {  // uniform over the grid
            if (h.m == 0 && lane < h.nrows) outs_s[lane] = v;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (h.m == 1 && lane < h.nrows) {
                const float *gouts = (const float *)(smem + L.outs + (wave - h.epi_wave_off) * L.outs_stride);
                const int n4 = h.epi_n & ~3;
                const int r = h.r0 + lane;
                const float gv = gouts[lane], uv = v;
                store_y(h.epi_y + r, rows_swiglu_out(gv, uv, r, n4));
            }
        }
        put_stamps();
        return;
    }

    // ---- main loop
    int io = q, rr = 0;  // quad's (block, row-in-batch) of superblock 16t+q
    while (io >= nb) {
        io -= nb;
        ++rr;
    }
    int bend = bR * nb < G ? bR * nb : G;  // superblock index ending the current batch
    int brow = 0;
    const uint8_t *cslot = ring;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        if (T - t >= D) vm_wait<NI * (D - 1)>();  // steady state: D-1 younger steps in flight
        else vm_wait_k<NI>(T - t - 1);
        if (RSTAMPS(h) && t == 0) sw = __builtin_amdgcn_s_memrealtime();
        if (!(RDIAG(ld) & 8) && ROWS_SB * t + q < G)
            rows_quad_step<TYPE>(cslot + mis + q * BSZ, actq + io * Q8L_STRIDE, s, recs + io * bR + rr);
        cslot = cslot + SLOT == ring_end ? ring : cslot + SLOT;
        io += ROWS_SB;
        if (nb >= ROWS_SB) {
            if (io >= nb) {
                io -= nb;
                ++rr;
            }
        } else {
            while (io >= nb) {
                io -= nb;
                ++rr;
            }
        }
        if (it_ < T) issue();
        if (RSTAMPS(h) && t == 0) sf = __builtin_amdgcn_s_memrealtime();
        if (ROWS_SB * (t + 1) >= bend) {  // batch complete: replay its rows' chains, lane r <-> row r
            wave_lds_fence();
            if (RSTAMPS(h) && brow == 0) sc = __builtin_amdgcn_s_memrealtime();
            const int nr = bR < h.nrows - brow ? bR : h.nrows - brow;
            if (lane < nr) {
                outs[brow + lane] = rows_chain<TYPE>(recs + lane, nb, bR);
            }
            brow += bR;
            rr -= bR;
            bend = bend + bR * nb < G ? bend + bR * nb : G;
            wave_lds_fence();
        }
    }
    st2 = RSTAMPS(h) ? __builtin_amdgcn_s_memrealtime() : 0;

    // ---- flush staged results (coalesced)
    if (h.nrows > 0) {
        wave_lds_fence();
        float *y = h.y + h.r0;
        if (res_p) {  // ggml_add(mul_mat, residual): the same single f32 add per element
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("" : "+v"(rv));
            for (int k = 0; k < h.nrows; k += 64)
                if (k + lane < h.nrows)
                    store_y(y + k + lane, outs[k + lane] + (k == 0 ? __uint_as_float(rv) : res_p[h.r0 + k + lane]));
        } else {
            for (int k = 0; k < h.nrows; k += 64)
                if (k + lane < h.nrows) store_y(y + k + lane, outs[k + lane]);
        }
        ss = RSTAMP();
    }
    // ---- SWIGLU epilogue (the GLU node after the gate/up MUL_MATs): up wave and its
    // gate partner own the same rows in this workgroup; both results are staged in LDS.
    // Same arithmetic as kq_swiglu (ggml_vec_swiglu_f32: NEON body, libm tail).
    if (h.epi && !(RDIAG(ld) & 128)) {  // uniform over the grid: every wave of the workgroup reaches the barrier (diag 128: timing only)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (h.m == 1 && h.nrows > 0) {
            const float *gouts = (const float *)(smem + L.outs + (wave - h.epi_wave_off) * L.outs_stride);
            const int n4 = h.epi_n & ~3;
            for (int k = 0; k < h.nrows; k += 64)
                if (k + lane < h.nrows) {
                    const int r = h.r0 + k + lane;
                    const float gv = gouts[k + lane], uv = outs[k + lane];
                    store_y(h.epi_y + r, rows_swiglu_out(gv, uv, r, n4));
                }
        }
    }
    put_stamps();
}

// SH: the short-stream form of rows_body (the host picks it per launch, as it picks LSH)
template <int TMASK, bool FUSEDQ, int PRO, int LSH, bool SH>
__global__ void __launch_bounds__(ROWS_WAVES * 64) kq_rows(KQ_ROWS_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RowsLead ld = rows_lead(x, x2, w0, res0, nb, waves_total, grid, cfg, rbase0, rrem0);
    if (RDIAG(ld) & 256) return;  // diagnostics (timing only): empty launch
    const uint64_t st0 = RSTAMP();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = wave * ld.grid + blockIdx.x;  // active waves spread over every CU
    auto resolve = [&]() { return rows_resolve<TMASK>(ld, gw); };

    if (TMASK == 1) {
        rows_body<Q4_K, FUSEDQ, PRO, TMASK, LSH, SH>(ld, smem, wave, lane, st0, resolve);
    } else if (TMASK == 2) {
        rows_body<Q5_K, FUSEDQ, PRO, TMASK, LSH, SH>(ld, smem, wave, lane, st0, resolve);
    } else if (TMASK == 4) {
        rows_body<Q6_K, FUSEDQ, PRO, TMASK, LSH, SH>(ld, smem, wave, lane, st0, resolve);
    } else {  // the type is the matrix's: the entry batch first
        const RowsHot h = resolve();
        auto resolved = [&]() { return h; };
        if (h.type == Q6_K) rows_body<Q6_K, FUSEDQ, PRO, TMASK, LSH, SH>(ld, smem, wave, lane, st0, resolved);
        else if (h.type == Q5_K) rows_body<Q5_K, FUSEDQ, PRO, TMASK, LSH, SH>(ld, smem, wave, lane, st0, resolved);
        else rows_body<Q4_K, FUSEDQ, PRO, TMASK, LSH, SH>(ld, smem, wave, lane, st0, resolved);
    }
}

// (the prologue's form LSH: every fused-quantization kernel in its three forms, each in the
// generic and the short-stream form; the Q8L-row kernels only in the generic one)
#define KQ_ROWS_INST(TM, FQ, PR, LS, SH) template __global__ void kq_rows<TM, FQ, PR, LS, SH>(KQ_ROWS_PARAMS);
#define KQ_ROWS_INST_F(TM, PR, LS) KQ_ROWS_INST(TM, true, PR, LS, false) KQ_ROWS_INST(TM, true, PR, LS, true)
#define KQ_ROWS_INST_P(TM, PR) KQ_ROWS_INST_F(TM, PR, 0) KQ_ROWS_INST_F(TM, PR, 1) KQ_ROWS_INST_F(TM, PR, 2)
#define KQ_ROWS_INST_T(TM) KQ_ROWS_INST_P(TM, 0) KQ_ROWS_INST_P(TM, 1) KQ_ROWS_INST_P(TM, 2) KQ_ROWS_INST(TM, false, 0, 0, false)
KQ_ROWS_INST_T(1)
KQ_ROWS_INST_T(2)
KQ_ROWS_INST_T(4)
KQ_ROWS_INST_T(7)

// ---------------------------------------------------------------- claimed rows (kq_rows_dyn)
// The static split above gives every wave a fixed share of whole rows; in the large GEMVs the
// last wave to finish sets the launch time, and which one that is follows the wave's age on
// its SIMD (issue goes by priority, then age: profiles/r05_rows_agew.txt), not its row count.
// Here workgroup b owns the rows [b*N/G, (b+1)*N/G) of every matrix and its waves CLAIM units
// of U rows from an LDS counter (MI355X_MICROARCH.md **dequeue**, kept inside the CU: one
// ds_add per unit), a ring depth ahead of their compute: the first P units of each wave are
// assigned statically (the ring fill before the prologue's barrier claims nothing), every
// later one is taken when the wave has issued its previous unit's last step. A unit's rows
// stay whole in one wave, so each row's fp32 chain is still replayed in superblock order by
// one lane (bit-identical to the static split and to ggml_vec_dot_q4_K_q8_K row by row,
// README.md:137). Results go to the workgroup's LDS rows and are stored coalesced, with the
// residual ADD and the SWIGLU epilogue, after one workgroup barrier.
namespace {
static_assert(MI355X_MAX_FUSED == 4, "four matrices at most");
struct DynUnit {
    const uint8_t *src;
    int rows, flat, G, T;
};
}  // namespace

// Every matrix of a kq_rows_dyn launch has the same rows and type (plan_rows), so one
// workgroup row range [r0, r0 + nr) serves them all: unit u is matrix u / nu's rows
// [r0 + (u % nu) U, ...), flat output index m * nr + local row. Records of consecutive
// units go into one batch of bR rows, replayed together (lane r <-> batch row r).
// kq_rows_dyn's entry batch: every matrix's pointers stay (a wave takes units of all of them).
struct RowsDynHot {
    int bR, rpw, U, P, ush, N, epi, epi_n;
    const uint8_t *w1, *w2, *w3;
    const float *s1, *s2, *s3;
    float *y0, *y1, *y2, *y3, *epi_y;
    float eps;
    uint64_t *stamps;
    int64_t stamps_cap;
};
__device__ __forceinline__ RowsDynHot rows_dyn_resolve() {
    const RowsRun r = rows_fetch();
    RowsDynHot h;
    h.bR = r.i32<RA_DW(bR)>(), h.rpw = r.i32<RA_DW(rpw)>();
    h.U = r.i32<RA_DW(dyn_u)>(), h.P = r.i32<RA_DW(dyn_p)>(), h.ush = r.i32<RA_DW(dyn_ush)>(), h.N = r.i32<RA_DW(n_rows)>();
    h.epi = r.i32<RA_DW(epi)>(), h.epi_n = r.i32<RA_DW(epi_n)>();
    h.epi_y = r.ptr<float, RA_DW(epi_y)>();
    h.eps = __uint_as_float(r.dw<RA_DW(eps)>());
    h.w1 = sreg(r.ptr<const uint8_t, RA_DW(w) + 2>()), h.w2 = sreg(r.ptr<const uint8_t, RA_DW(w) + 4>());
    h.w3 = sreg(r.ptr<const uint8_t, RA_DW(w) + 6>());
    h.s1 = sreg(r.ptr<const float, RA_DW(res) + 2>()), h.s2 = sreg(r.ptr<const float, RA_DW(res) + 4>());
    h.s3 = sreg(r.ptr<const float, RA_DW(res) + 6>());
    h.y0 = sreg(r.ptr<float, RA_DW(y)>()), h.y1 = sreg(r.ptr<float, RA_DW(y) + 2>());
    h.y2 = sreg(r.ptr<float, RA_DW(y) + 4>()), h.y3 = sreg(r.ptr<float, RA_DW(y) + 6>());
#if KQ_ROWS_DIAG
    h.stamps = r.ptr<uint64_t, RA_DW(stamps)>();
    h.stamps_cap = (int64_t)(uintptr_t)r.ptr<uint8_t, RA_DW(stamps_cap)>();
#else
    h.stamps = nullptr, h.stamps_cap = 0;
#endif
    return h;
}

template <int TYPE, bool FUSEDQ, int PRO, int TMASK, int LSH>
__device__ __forceinline__ void rows_dyn_body(const RowsLead &ld, uint8_t *smem, int wave, int lane,
                                              uint64_t st0) {
    uint64_t sf = 0;  // diagnostics (KQ_ROWS_DIAG builds): first step
    constexpr int BSZ = block_bytes(TYPE);
    constexpr int NI = rows_ni(TYPE);
    constexpr int PART = rows_gran(TYPE) - 64 * (NI - 1);  // lanes of a step's partial last DMA instruction
    constexpr int SLOT = rows_slot(TYPE);
    constexpr int D = rows_depth(TYPE);
    static_assert(D >= 2 && D <= 4, "vm_wait_k covers 3 steps in flight");
    const int nb = ld.nb;
    const int nwv = ld.nwv;
    const int b = (int)blockIdx.x;
    const int q = lane >> 2, s = lane & 3;

    // ---- activation loads first (the leading parameters only), then the entry batch
    const float *const x = (const float *)ld.x;
    RowsPrologue<LSH> pg;
    if (FUSEDQ) pg.template load<PRO>(ld, wave, lane, 0);
    const RowsDynHot h = rows_dyn_resolve();
    // (scalars of their own: a pick among struct members becomes a pick of addresses, in scratch)
    const uint8_t *const w0 = ld.w0, *const w1 = h.w1, *const w2 = h.w2, *const w3 = h.w3;
    const float *const s0 = ld.res0, *const s1 = h.s1, *const s2 = h.s2, *const s3 = h.s3;
    float *const y0 = h.y0, *const y1 = h.y1, *const y2 = h.y2, *const y3 = h.y3;
    const int U = h.U, P = h.P, bR = h.bR;
    const RowsDynLayout L = rows_dyn_layout(nb, TMASK, bR, h.rpw, nwv);
    uint8_t *const ring = smem + L.ring + wave * L.ring_stride;
    uint8_t *const ring_end = ring + D * SLOT;
    RowRec *const recs = (RowRec *)(smem + L.recs + wave * L.recs_stride);
    float *const outs = (float *)(smem + L.outs);
    uint32_t *const cnt = (uint32_t *)(smem + L.cnt);
    const uint8_t *const actq = smem + L.act;

    // ---- the workgroup's rows and units: rows [r0, r0 + nr) of every matrix (the host's
    // N / G split, rbase[0] / rrem[0]); unit u = matrix u / nu, rows r0 + (u % nu) U ..
    const int N = h.N;
    const int ush = h.ush;  // U = 1 << ush
    const int rbase = ld.rbase0, rrem = ld.rrem0;
    const int r0 = b * rbase + (b < rrem ? b : rrem);
    const int nr = rbase + (b < rrem ? 1 : 0);
    const int nu = (nr + U - 1) >> ush;
    const int units = ld.n_desc * nu, nflat = ld.n_desc * nr;
    const int64_t rowb = (int64_t)nb * BSZ;
    auto row_of = [&](int f) { return r0 + f; };
    // unit u's stream (its first byte), rows and flat output index: computed once, when the
    // unit is taken, and kept for its consumption in lane (k & 7) of four registers
    auto unit_of = [&](int u) {
        DynUnit d;
        const int m = (u >= nu ? 1 : 0) + (u >= 2 * nu ? 1 : 0) + (u >= 3 * nu ? 1 : 0);
        const int lr = (u - m * nu) << ush;
        d.rows = nr - lr < U ? nr - lr : U;
        d.flat = m * nr + lr;
        const uint8_t *w = m == 0 ? w0 : m == 1 ? w1 : m == 2 ? w2 : w3;
        d.src = w + (int64_t)(r0 + lr) * rowb;
        d.G = d.rows * nb;
        d.T = (d.G + ROWS_SB - 1) / ROWS_SB;
        return d;
    };
    const int nstat = nwv * P < units ? nwv * P : units;  // statically assigned unit ids [0, nstat)

    // ---- issue side: the unit being issued, its next step, the claimed-unit list
    uint32_t ul = 0, uh = 0, ug = 0, uf = 0;  // lane k & 7: the k-th unit's src (lo, hi), G | rows << 16, flat
    int ki = -1, is = 0, iT = 0, issued = 0;
    bool idone = false, iwait = false;
    const uint8_t *is16 = nullptr, *il16 = nullptr;
    uint8_t *islot = ring;
    auto take = [&](int u) {
        ++ki;
        const DynUnit d = unit_of(u);
        const bool mine = lane == (ki & 7);
        ul = mine ? (uint32_t)(uintptr_t)d.src : ul;
        uh = mine ? (uint32_t)((uintptr_t)d.src >> 32) : uh;
        ug = mine ? (uint32_t)(d.G | (d.rows << 16)) : ug;
        uf = mine ? (uint32_t)d.flat : uf;
        is16 = (const uint8_t *)((uintptr_t)d.src & ~(uintptr_t)15);
        il16 = (const uint8_t *)((uintptr_t)(d.src + (int64_t)d.G * BSZ - 1) & ~(uintptr_t)15);
        iT = d.T;
        is = 0;
    };
    // the next unit: static ones first; a claim only once the counter is set (claim_ok)
    auto next_unit = [&](bool claim_ok) {
        const int k = ki + 1;
        if (k < P) {
            const int u = wave * P + k;
            if (u < nstat) take(u);
            else idone = true;
            return;
        }
        if (!claim_ok) {
            iwait = true;
            return;
        }
        iwait = false;
        uint32_t u = 0;
        if (lane == 0) u = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int uu = __builtin_amdgcn_readfirstlane((int)u);
        if (uu < units) take(uu);
        else idone = true;
    };
    auto issue = [&](bool claim_ok) {  // one step (NI DMA instructions), then the next unit if this one is done
        rows_issue_step<TYPE>(is16 + (int64_t)is * (ROWS_SB * BSZ) + 16 * lane, il16, islot, lane, is + 1 < iT);
        islot = islot + SLOT == ring_end ? ring : islot + SLOT;
        ++is;
        ++issued;
        if (is == iT) next_unit(claim_ok);
    };
    next_unit(false);  // the first static unit (or none)

    // residual of the fused ADD for flat row 64 * wave + lane, fetched with the activation
    // (issued on every path: a dummy read of x without one; kept live until the flush waits)
    const int f0 = 64 * wave + lane;
    const int fm = (f0 >= nr ? 1 : 0) + (f0 >= 2 * nr ? 1 : 0) + (f0 >= 3 * nr ? 1 : 0);
    const float *fres = fm == 0 ? s0 : fm == 1 ? s1 : fm == 2 ? s2 : s3;
    const int frow = row_of(f0 - fm * nr);
    uint32_t rv = 0;

    // ---- prologue: the first unit's first step (a wave without a unit: no step of the stream)
    ProStamps ps;
    if (FUSEDQ) {
        rv = gload4_asm(fres && f0 < nflat && frow < N ? fres + frow : x);
        // exactly one step's NI DMA instructions on every path, as in rows_body
        if (ki < 0) {  // no unit: from the activation, into a slot never read
            const uint8_t *xb = (const uint8_t *)x + 16 * lane;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (i + 1 == NI) dma16_nt_lanes(xb, (LDS void *)(islot + 1024 * i), lane, PART);
                else dma16_nt(xb, (LDS void *)(islot + 1024 * i));
        } else {  // the first unit's first step, its partial DMA masked in asm
            const uint8_t *base = is16 + 16 * lane;
            const uint8_t *lim = iT > 1 ? base + 1024 * (NI - 1) : base + 1024 * (NI - 1) < il16 ? base + 1024 * (NI - 1) : il16;
#pragma unroll
            for (int i = 0; i + 1 < NI; ++i) {
                const uint8_t *p = base + 1024 * i;
                dma16_nt(iT > 1 || p < il16 ? p : il16, (LDS void *)(islot + 1024 * i));
            }
            dma16_nt_lanes(lim, (LDS void *)(islot + 1024 * (NI - 1)), lane, PART);
            islot = islot + SLOT == ring_end ? ring : islot + SLOT;
            ++is;
            ++issued;
            if (is == iT) next_unit(false);
        }
        rows_fused_finish<TYPE, PRO>(pg, x, smem + L.act, (double *)(smem + L.sums), h.eps, 0, RSTAMPS(h) != nullptr, ps);
    } else {
        const int ng = nb * (Q8L_STRIDE / 16);
        for (int j = wave; 64 * j < ng; j += nwv) {
            const int k = 64 * j + lane;
            if (k < ng) dma16((const uint8_t *)ld.x + 16 * k, (LDS void *)(smem + L.act + 1024 * j));
        }
        rv = gload4_asm(fres && f0 < nflat && frow < N ? fres + frow : (const float *)ld.x);
        if (!idone && !iwait && ki >= 0) issue(false);
        vm_wait_k<NI>(issued);
    }
    while (!idone && !iwait && ki >= 0 && issued < D) issue(false);  // the rest of the ring: static units only
    if (wave == 0 && lane == 0) *cnt = (uint32_t)(nwv * P);            // claims start after the static ids
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // Q8_K row complete, counter set
    if (iwait) next_unit(true);
    while (!idone && ki >= 0 && issued < D) issue(true);
    const uint64_t st1 = RSTAMPS(h) ? __builtin_amdgcn_s_memrealtime() : 0;

    // ---- main loop: the oldest step in flight, then one more issued
    int kc = 0, cs = 0, cT = 0, cG = 0, cmis = 0, crows = 0, io = 0, rr = 0;
    int bro = 0;        // batch rows before the current unit
    uint32_t bfl = 0;   // lane r: flat output index of batch row r
    auto consume_unit = [&](int k) {
        const uint32_t gr = (uint32_t)__builtin_amdgcn_readlane((int)ug, k & 7);
        const int flat = __builtin_amdgcn_readlane((int)uf, k & 7);
        cG = (int)(gr & 0xffffu);
        crows = (int)(gr >> 16);
        cT = (cG + ROWS_SB - 1) / ROWS_SB;
        cmis = (int)((uint32_t)__builtin_amdgcn_readlane((int)ul, k & 7) & 15u);
        bfl = lane >= bro && lane < bro + crows ? (uint32_t)(flat + lane - bro) : bfl;
        cs = 0;
        io = q;
        rr = bro;
        while (io >= nb) {
            io -= nb;
            ++rr;
        }
    };
    auto replay = [&]() {  // the batch's rows: lane r <-> batch row r, records in superblock order
        wave_lds_fence();
        if (lane < bro) {
            outs[bfl] = rows_chain<TYPE>(recs + lane, nb, bR);
        }
        wave_lds_fence();
        bro = 0;
    };
    int consumed = 0;
    if (issued > 0) consume_unit(0);
    const uint8_t *cslot = ring;
#pragma unroll 1
    while (consumed < issued) {
        vm_wait_k<NI>(issued - consumed - 1);
        if (ROWS_SB * cs + q < cG) rows_quad_step<TYPE>(cslot + cmis + q * BSZ, actq + io * Q8L_STRIDE, s, recs + io * bR + rr);
        cslot = cslot + SLOT == ring_end ? ring : cslot + SLOT;
        ++consumed;
        ++cs;
        if (!idone) issue(true);
        if (RSTAMPS(h) && consumed == 1) sf = __builtin_amdgcn_s_memrealtime();
        if (cs == cT) {  // the unit's last step: into the batch; replay when the next unit may not fit
            bro += crows;
            if (bro + U > bR || consumed == issued) replay();
            ++kc;
            if (consumed < issued) consume_unit(kc);
        } else {
            io += ROWS_SB;
            while (io >= nb) {
                io -= nb;
                ++rr;
            }
        }
    }

    const uint64_t st2 = RSTAMPS(h) ? __builtin_amdgcn_s_memrealtime() : 0;
    // ---- flush: the workgroup's rows, coalesced, with the residual ADD / SWIGLU epilogue
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(rv));
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int f = f0; f < nflat; f += 64 * nwv) {
        const int m = (f >= nr ? 1 : 0) + (f >= 2 * nr ? 1 : 0) + (f >= 3 * nr ? 1 : 0);
        const int row = f == f0 ? frow : row_of(f - m * nr);
        if (row >= N) continue;  // the short last unit's unused slots
        const float *res = m == 0 ? s0 : m == 1 ? s1 : m == 2 ? s2 : s3;
        float *y = m == 0 ? y0 : m == 1 ? y1 : m == 2 ? y2 : y3;
        float v = outs[f];
        if (res) v = v + (f == f0 ? __uint_as_float(rv) : res[row]);  // ggml_add(mul_mat, residual)
        store_y(y + row, v);
    }
    if (h.epi) {  // y[0] = gate, y[1] = up: the same rows of both in this workgroup
        const int n4 = h.epi_n & ~3;
        for (int f = f0; f < nr; f += 64 * nwv) {
            const int r = row_of(f);
            if (r >= N) continue;
            const float gv = outs[f], uv = outs[nr + f];
            store_y(h.epi_y + r, rows_swiglu_out(gv, uv, r, n4));
        }
    }
    if (RSTAMPS(h)) {  // the kq_rows stamp layout (tools/stamps.py); slot 4: x landed, slot 7: units this wave took
        const uint64_t v[ROWS_STAMP_SLOTS] = {st0, st1, st2, 0, ps.landed, ps.quantized, sf, (uint64_t)(ki + 1)};
        rows_put_stamps(RSTAMPS(h), h.stamps_cap, wave, lane, v);
    }
}
template <int TMASK, bool FUSEDQ, int PRO, int LSH>
__global__ void __launch_bounds__(ROWS_WAVES * 64) kq_rows_dyn(KQ_ROWS_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RowsLead ld = rows_lead(x, x2, w0, res0, nb, waves_total, grid, cfg, rbase0, rrem0);
    const uint64_t st0 = RSTAMP();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int TYPE = TMASK == 1 ? Q4_K : TMASK == 2 ? Q5_K : Q6_K;
    rows_dyn_body<TYPE, FUSEDQ, PRO, TMASK, LSH>(ld, smem, wave, lane, st0);
}

#define KQ_ROWS_DYN_INST(TM, FQ, PR, LS) template __global__ void kq_rows_dyn<TM, FQ, PR, LS>(KQ_ROWS_PARAMS);
#define KQ_ROWS_DYN_INST_P(TM, PR) \
    KQ_ROWS_DYN_INST(TM, true, PR, 0) KQ_ROWS_DYN_INST(TM, true, PR, 1) KQ_ROWS_DYN_INST(TM, true, PR, 2)
#define KQ_ROWS_DYN_INST_T(TM) \
    KQ_ROWS_DYN_INST_P(TM, 0) KQ_ROWS_DYN_INST_P(TM, 1) KQ_ROWS_DYN_INST_P(TM, 2) KQ_ROWS_DYN_INST(TM, false, 0, 0)
KQ_ROWS_DYN_INST_T(1)
KQ_ROWS_DYN_INST_T(2)
KQ_ROWS_DYN_INST_T(4)

}  // namespace kq
