// kq_q3k.hip — Q3_K weights (block_q3_K, 110 B): kq_gemv_q3k, the GEMV for every batch size
// (column groups of up to 8), its planner and the two entries mi355x_mul_mat / mi355x_mul_mat_q8
// hand the type to. The rule is include/ggml_mi355x.h's (mi355x_vec_dot_q3_K_q8_K).
//
// Work split: one workgroup per CU of Q3K_WAVES waves; global wave gw = wave * grid.x + block owns
// a run of whole rows (rbase, one more for gw < rrem), which is one contiguous byte stream since
// rows are packed. A step is 8 consecutive superblocks of that stream: 880 B = 55 granules of
// 16 B, fetched non-temporal by ONE LDS-DMA instruction from the 16-B boundary below the stream
// (110 = 2 mod 4: the stream starts at any even address, so 56 granules cover a step and the
// offset inside the slot is the same for every step). Each wave keeps a ring of Q3K_DEPTH slots
// in flight, counted by hand in vmcnt. grid.y = the groups of NCOL activation columns; a weight
// step is unpacked once and used against every column of the group.
// Lanes: octet o = lane >> 3 takes superblock 8t + o of the stream, lane p = lane & 7 of it the
// share of kq_q3k_device.h; isum is summed over the octet by DPP. The float side runs in row
// order on the whole wave: for o = 0 .. 7 the octet's (isum, y.d * d) are read by v_readlane and
// sumf = fmaf(d_i, (float)isum_i, sumf); a row's last superblock stages sumf in LDS, and the
// staged rows are stored once, from one lane each, after the wave's DMAs have landed.
// Activation: M = 1 and K <= 16384 with an f32 x: the workgroup quantizes x to Q8_K in LDS
// itself (quant_block_wave, kq_quantize_q8K's bits); otherwise the caller's Q8_K rows (292-B
// blocks) are copied into the same Q8L layout (d @0, qs @16, 304 B: 8-byte aligned pieces).
#include <atomic>
#include <string>

#include "kq_common.h"
#include "kq_internal.h"
#include "kq_q3k_device.h"

namespace kq {

constexpr int Q3K_SB = 8;                      // superblocks per step (8 lanes each)
constexpr int Q3K_STEP = Q3K_SB * Q3K_BLOCK;   // 880 B = 55 granules
constexpr int Q3K_SLOT = Q3K_STEP + 16;        // + the granule a misaligned stream spills into
static_assert(Q3K_STEP % 16 == 0 && Q3K_SLOT / 16 <= WAVE, "a step is one LDS-DMA instruction of whole granules");
static_assert(Q3K_DEPTH >= 2 && Q3K_DEPTH <= 8, "q3k_wait covers 7 steps in flight");

//   act:  the column group's Q8L blocks, column-major (ncol * nb * 304 B)
//   ring: per wave Q3K_DEPTH slots (+16 B so that a slot's last dword read has a neighbour)
//   outs: per wave Q3K_OUTS staged results
struct Q3kLayout {
    int act, ring, ring_stride, outs, total;
};
__host__ __device__ inline Q3kLayout q3k_layout(int ncol, int nb, int nwv) {
    Q3kLayout L;
    L.act = 0;
    L.ring = ncol * nb * Q8L_STRIDE;
    L.ring_stride = Q3K_DEPTH * Q3K_SLOT + 16;
    L.outs = L.ring + nwv * L.ring_stride;
    L.total = L.outs + nwv * Q3K_OUTS * 4;
    return L;
}

namespace {

// at most n of the wave's DMA instructions still in flight
__device__ __forceinline__ void q3k_wait(int n) {
    switch (n) {
        case 0: vm_wait<0>(); break;
        case 1: vm_wait<1>(); break;
        case 2: vm_wait<2>(); break;
        case 3: vm_wait<3>(); break;
        case 4: vm_wait<4>(); break;
        case 5: vm_wait<5>(); break;
        case 6: vm_wait<6>(); break;
        default: vm_wait<7>(); break;
    }
}

}  // namespace

template <int NCOL, bool FUSEDQ>
__global__ void __launch_bounds__(Q3K_WAVES * 64) kq_gemv_q3k(const Q3kArgs a) {
    static_assert(!FUSEDQ || NCOL == 1, "the fused quantizer serves the decode token");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nb = a.nb, nwv = a.nwv;
    const int gw = wave * (int)gridDim.x + (int)blockIdx.x;  // active waves spread over every CU
    const int c0 = (int)blockIdx.y * NCOL;
    const int ncg = a.m_total - c0 < NCOL ? a.m_total - c0 : NCOL;
    const Q3kLayout L = q3k_layout(NCOL, nb, nwv);
    uint8_t *const act = smem + L.act;
    uint8_t *const ring = smem + L.ring + wave * L.ring_stride;
    float *const outs = (float *)(smem + L.outs) + wave * Q3K_OUTS;

    // ---- this wave's rows and their stream
    int r0 = 0, nrows = 0;
    if (gw < a.waves_total) {
        r0 = gw * a.rbase + (gw < a.rrem ? gw : a.rrem);
        nrows = a.rbase + (gw < a.rrem ? 1 : 0);
    }
    const int G = nrows * nb;                  // superblocks
    const int T = (G + Q3K_SB - 1) / Q3K_SB;   // steps
    const uint8_t *const src = a.w + (int64_t)r0 * nb * Q3K_BLOCK;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);
    const uint8_t *const s16 = src - mis;
    int it_ = 0, islot = 0;  // next step to issue, its slot
    auto issue = [&]() {
        const int cnt = G - Q3K_SB * it_ < Q3K_SB ? G - Q3K_SB * it_ : Q3K_SB;
        // the granules that hold a byte of the step: none lies wholly outside the tensor
        const int ng = (int)((mis + (uint32_t)(cnt * Q3K_BLOCK) + 15u) >> 4);
        dma16_nt_lanes(s16 + (int64_t)it_ * Q3K_STEP + 16 * lane, (LDS void *)(ring + islot * Q3K_SLOT), lane, ng);
        islot = islot + 1 == Q3K_DEPTH ? 0 : islot + 1;
        ++it_;
    };
    while (it_ < Q3K_DEPTH && it_ < T) issue();

    // ---- the activation blocks of the column group, by every wave of the workgroup
    if (FUSEDQ) {
        for (int b = wave; b < nb; b += nwv) {
            const Q8Lane q = quant_block_wave(a.x + (int64_t)QK * b, lane);
            uint8_t *blk = act + b * Q8L_STRIDE;
            *(uint32_t *)(blk + 16 + 4 * lane) = q.qs4;
            if (lane == 0) *(float *)blk = q.d;
        }
    } else {
        for (int idx = wave; idx < NCOL * nb; idx += nwv) {
            const int c = idx / nb, b = idx - c * nb;
            uint32_t qs4 = 0;
            float d = 0.f;
            if (c < ncg) {  // (a partial group's missing columns read as zero and are never stored)
                const uint8_t *xb = a.xq + (int64_t)(c0 + c) * a.xq_col_stride + (int64_t)b * 292;
                qs4 = *(const uint32_t *)(xb + 4 + 4 * lane);
                d = *(const float *)xb;
            }
            uint8_t *blk = act + idx * Q8L_STRIDE;
            *(uint32_t *)(blk + 16 + 4 * lane) = qs4;
            if (lane == 0) *(float *)blk = d;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (T == 0) return;

    // ---- staged results -> y, once each: after every DMA issued so far has landed, so that the
    // stores leave vmcnt at zero again before the ring's counted waits go on
    float *const yw = a.y + (int64_t)c0 * a.y_col_stride + r0;
    int nst = 0, rdone = 0;  // staged rows, rows already stored
    auto flush = [&]() {
        vm_wait<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wave_lds_fence();
        for (int k = lane; k < nst * NCOL; k += WAVE) {
            const int r = k / NCOL, c = k - r * NCOL;
            if (c < ncg) yw[(int64_t)c * a.y_col_stride + rdone + r] = outs[k];
        }
        vm_wait<0>();
        wave_lds_fence();
        rdone += nst;
        nst = 0;
    };

    // ---- main loop
    const int o = lane >> 3, p = lane & 7;
    float sum[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) sum[c] = 0.f;
    int i0 = 0;    // block-in-row of the step's first superblock
    int iu = 0;    // block-in-row the chain stands at
    int cslot = 0;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        q3k_wait(T - 1 - t < Q3K_DEPTH - 1 ? T - 1 - t : Q3K_DEPTH - 1);
        const int cnt = G - Q3K_SB * t < Q3K_SB ? G - Q3K_SB * t : Q3K_SB;
        int il = i0 + o;  // the octet's block-in-row (an octet past cnt computes on stale bytes, unused)
        if (nb >= Q3K_SB) il -= il >= nb ? nb : 0;
        else il %= nb;
        const Q3Lane wq = q3k_unpack(ring + cslot * Q3K_SLOT, mis + (uint32_t)(o * Q3K_BLOCK), p);
        const float wd = h2f(wq.dh);
        int isum[NCOL];
        float cf[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; ++c) {
            const uint8_t *ab = act + (c * nb + il) * Q8L_STRIDE;
            isum[c] = octet_sum(q3k_dot(wq, ab, p));
            cf[c] = *(const float *)ab * wd;  // d_i = y.d * fp16(x.d)
        }
        // the chain, in row order (uniform over the wave)
#pragma unroll
        for (int k = 0; k < Q3K_SB; ++k) {
            if (k < cnt) {
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    const int ai = __builtin_amdgcn_readlane(isum[c], 8 * k);
                    const float ci = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cf[c]), 8 * k));
                    sum[c] = fmaf(ci, (float)ai, sum[c]);
                }
                if (++iu == nb) {  // the row's last superblock
                    iu = 0;
                    if (lane == 0) {
#pragma unroll
                        for (int c = 0; c < NCOL; ++c) outs[nst * NCOL + c] = sum[c];
                    }
#pragma unroll
                    for (int c = 0; c < NCOL; ++c) sum[c] = 0.f;
                    if (++nst == Q3K_OUTS / NCOL) flush();
                }
            }
        }
        i0 += Q3K_SB;
        while (i0 >= nb) i0 -= nb;
        // the slot is free once its reads have returned: the next step takes it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (it_ < T) issue();
        cslot = cslot + 1 == Q3K_DEPTH ? 0 : cslot + 1;
    }
    if (nst) flush();
}

template __global__ void kq_gemv_q3k<1, true>(const Q3kArgs);
template __global__ void kq_gemv_q3k<1, false>(const Q3kArgs);
template __global__ void kq_gemv_q3k<2, false>(const Q3kArgs);
template __global__ void kq_gemv_q3k<4, false>(const Q3kArgs);
template __global__ void kq_gemv_q3k<8, false>(const Q3kArgs);

// ------------------------------------------------------------ host
// The plan of one kq_gemv_q3k launch: N rows of K / 256 packed blocks against M columns.
// MI355X_E_INVAL: K, N, M out of range, an odd address or stride; MI355X_E_UNSUPPORTED:
// non-contiguous rows (N > 1), K > Q3K_MAX_NB superblocks, or no layout fits.
int plan_q3k(const void *w, int64_t K, int64_t N, size_t row_stride, int64_t M, bool fusedq, Q3kPlan &pl) {
    if (K <= 0 || K % QK || N < 0 || N > 0x7fffffff || M < 0 || M > 0x7fffffff) return MI355X_E_INVAL;
    const int64_t nb = K / QK;
    Q3kArgs &a = pl.a;
    a = Q3kArgs{};
    pl.grid = dim3(1, 1, 1), pl.lds = 0, pl.ncol = 1, pl.fusedq = fusedq;
    a.n_rows = (int)N, a.nb = (int)(nb > 0x7fffffff ? 0x7fffffff : nb), a.m_total = (int)M;
    if (N == 0 || M == 0) return MI355X_OK;  // (waves_total 0: nothing to launch)
    if (!w || ((uintptr_t)w & 1u) || (row_stride & 1u) || row_stride < (size_t)nb * Q3K_BLOCK) return MI355X_E_INVAL;
    if (N > 1 && row_stride != (size_t)nb * Q3K_BLOCK) return MI355X_E_UNSUPPORTED;  // one stream per wave
    if (nb > Q3K_MAX_NB || (fusedq && (nb > Q3K_FUSED_MAX_NB || M != 1))) return MI355X_E_UNSUPPORTED;
    a.w = (const uint8_t *)w;
    a.nwv = Q3K_WAVES;
    // NCOL: the narrowest group that covers min(M, 8), then down while the layout does not fit
    pl.ncol = 0;
    for (int nc = M > 4 ? 8 : M > 2 ? 4 : M > 1 ? 2 : 1; nc >= 1; nc >>= 1) {
        const Q3kLayout L = q3k_layout(nc, (int)nb, a.nwv);
        if ((size_t)L.total > kMaxLds) continue;
        pl.ncol = nc, pl.lds = (size_t)L.total;
        break;
    }
    if (!pl.ncol) return MI355X_E_UNSUPPORTED;
    // whole rows per wave, as even as they come: ceil(N / cap) rows a wave fixes the wave count
    const int64_t cus = num_cus(), cap = cus * a.nwv;
    const int64_t rpw = (N + cap - 1) / cap, waves = (N + rpw - 1) / rpw;
    if (rpw * nb > 0x7fffffff / Q3K_SB) return MI355X_E_UNSUPPORTED;
    a.waves_total = (int)waves;
    a.rbase = (int)(N / waves), a.rrem = (int)(N % waves);
    pl.grid = dim3((unsigned)(waves < cus ? waves : cus), (unsigned)((M + pl.ncol - 1) / pl.ncol), 1);
    const double groups = (double)pl.grid.y;  // the weights are streamed once per column group
    pl.bytes = groups * (double)N * nb * Q3K_BLOCK + (double)M * N * 4.0 + (double)M * nb * (fusedq ? QK * 4.0 : 292.0);
    return MI355X_OK;
}

int launch_q3k(const Q3kPlan &pl, hipStream_t stream) {
    const Q3kArgs &a = pl.a;
    if (a.waves_total == 0) return MI355X_OK;
    typedef void (*fn_t)(const Q3kArgs);
    const fn_t fn = pl.fusedq       ? kq_gemv_q3k<1, true>
                    : pl.ncol == 8 ? kq_gemv_q3k<8, false>
                    : pl.ncol == 4 ? kq_gemv_q3k<4, false>
                    : pl.ncol == 2 ? kq_gemv_q3k<2, false>
                                   : kq_gemv_q3k<1, false>;
    allow_lds((const void *)fn, pl.lds);
    return timed_launch_lazy(
        [&] {
            return LaunchInfo{"kq::kq_gemv_q3k<" + std::to_string(pl.ncol) + ", " + (pl.fusedq ? "true" : "false") + ">",
                              pl.bytes};
        },
        fn, pl.grid, dim3(a.nwv * 64), pl.lds, stream, a);
}

// mi355x_mul_mat_q8's Q3_K arm: the generic operand checks are the caller's
int q3k_mul_mat_q8(const void *w, int64_t K, int64_t N, size_t nb01, const void *q8, int64_t M, size_t nb11, float *dst,
                   size_t nb1, hipStream_t stream) {
    Q3kPlan pl;
    const int rc = plan_q3k(w, K, N, nb01, M, false, pl);
    if (rc) return rc;
    if (!dst) return MI355X_E_INVAL;
    pl.a.xq = (const uint8_t *)q8;
    pl.a.xq_col_stride = (int64_t)nb11;
    pl.a.y = dst;
    pl.a.y_col_stride = (int64_t)(nb1 / 4);
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_q3k(pl, stream);
}

size_t q3k_workspace(int64_t K, int64_t M) {
    if (M == 0 || (M == 1 && K / QK <= Q3K_FUSED_MAX_NB)) return 0;
    return ((size_t)M * (size_t)(K / QK) * Q8L_STRIDE + 255) & ~(size_t)255;  // >= the raw 292-B blocks
}

// mi355x_q3k_prefill: from how many columns on q3k_mul_mat takes kq_mmq's Q3_K body (the int8
// matrix cores, the weights streamed once) instead of kq_gemv_q3k over groups of 8 columns. AUTO's
// 64 is one whole column tile, a condition and no measurement (tools/q3k_bench.py sweeps the
// crossover); MMQ takes it from the prefill GEMMs' floor on.
namespace {
std::atomic<int> g_q3k_prefill{MI355X_Q3K_PREFILL_AUTO};
constexpr int64_t kQ3kMmqAutoCols = 64;
}  // namespace
int q3k_prefill_mode() { return g_q3k_prefill.load(); }
int q3k_prefill_set(int impl) { return g_q3k_prefill.exchange(impl); }
static bool q3k_takes_mmq(int64_t M) {
    const int mode = q3k_prefill_mode();
    return mode == MI355X_Q3K_PREFILL_MMQ ? M >= kMmqMinCols : mode == MI355X_Q3K_PREFILL_AUTO && M >= kQ3kMmqAutoCols;
}

// mi355x_mul_mat's Q3_K arm: the decode token quantizes in the kernel; from q3k_takes_mmq's
// columns on kq_quantize_q8L and kq_mmq<Q3_K> (a workspace that is not 16-byte aligned or holds
// only the raw 292-B blocks keeps the GEMV); every other shape goes through kq_quantize_q8K into
// the workspace first. plan_q3k's refusals come first whichever kernel runs.
int q3k_mul_mat(const void *w, int64_t K, int64_t N, size_t nb01, const float *x, int64_t M, size_t nb11, float *dst,
                size_t nb1, void *ws, size_t ws_size, hipStream_t stream) {
    const int64_t nb = K / QK;
    if (M == 1 && nb <= Q3K_FUSED_MAX_NB) {
        Q3kPlan pl;
        const int rc = plan_q3k(w, K, N, nb01, 1, true, pl);
        if (rc) return rc;
        pl.a.x = x;
        pl.a.y = dst;
        pl.a.y_col_stride = (int64_t)(nb1 / 4);
        if (!device_ok()) return MI355X_E_NODEVICE;
        return launch_q3k(pl, stream);
    }
    Q3kPlan pl;
    int rc = plan_q3k(w, K, N, nb01, M, false, pl);  // the refusals before any launch
    if (rc) return rc;
    const size_t q8_row = (size_t)nb * 292;
    if (!ws || ws_size < q8_row * (size_t)M || ((uintptr_t)ws & 3u)) return MI355X_E_WORKSPACE;
    if (!device_ok()) return MI355X_E_NODEVICE;
    if (q3k_takes_mmq(M) && ((uintptr_t)ws & 15u) == 0 && ws_size >= (size_t)M * (size_t)nb * Q8L_STRIDE) {
        rc = launch_quantize_q8L(x, (int64_t)(nb11 / 4), ws, K, M, stream, true);
        if (rc) return rc;
        return launch_mmq(Q3_K, w, K, N, nb01, (const uint8_t *)ws, M, dst, (int64_t)(nb1 / 4), stream);
    }
    rc = launch_quantize(x, (int64_t)(nb11 / 4), ws, K, M, stream);
    if (rc) return rc;
    return q3k_mul_mat_q8(w, K, N, nb01, ws, M, q8_row, dst, nb1, stream);
}

}  // namespace kq

extern "C" int mi355x_q3k_prefill(int impl) {
    if (impl < MI355X_Q3K_PREFILL_AUTO || impl > MI355X_Q3K_PREFILL_MMQ) return MI355X_E_INVAL;
    return kq::q3k_prefill_set(impl);
}
