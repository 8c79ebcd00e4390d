// kq_attn_head.h — decode attention of one query head on 256 threads (rope + f16 KV-cache
// write + KQ + soft_max + KQV), the body of kq_attn_decode (kq_attn_decode.hip), of the fused
// attention + o-proj kernel (kq_attn_oproj.hip) and of the persistent layer (kq_layer.hip);
// with the steps the cells-split kernels (kq_attn_decode.hip) share with it.
#pragma once

#include "kq_attn_device.h"
#include "kq_device.h"
#include "kq_ops_device.h"

namespace kq {

// ------------------------------------------------------------ decode attention
// One workgroup per query head h (kv head g = h / (n_head/n_head_kv)), 256 threads.
//  0. Every load that does not depend on the position is issued together with the
//     position itself: this token's q/k/v, K-cache row t (the cell thread t scores in
//     the first pass) and the first VPF 8-cell groups of this thread's V-cache row(s).
//     Only the rope-table row waits for the position, so a launch pays two memory
//     latencies instead of four. Prefetched cells at or after pos are never used (the
//     new cell comes from LDS, later cells are masked).
//  1. rope(q_h), rope(k_g) at `pos` -> f16; v_g -> f16. The first query head of each
//     kv group writes the new cell to the caches (K [cell][kvw], V transposed
//     [ch][n_ctx]); every workgroup uses its own LDS copy of that cell, so no
//     workgroup reads a cache cell written in this launch.
//  2. kq[c] = vec_dot_f16(k_cache[c], q16) for c <= pos (NEON FP16 structure), * scale;
//     cells pos < c < n_kv are masked (-INF) and contribute exact zeros below
//     (the cache is zero-initialised, so their dot products are finite).
//  3. soft_max: max; v_expf(w - max) per cell, group sums of 4 in the vaddvq order,
//     the double sum over groups in order (one lane), p = e * (float)(1.0/sum) -> f16.
//  4. kqv[d] = vec_dot_f16(v_cache[g*hd+d][0..n_kv), p16): thread (d, j) runs
//     accumulator j (8 lanes) over cells 32it+8j+l, then the f16 reduce tree.
// A position outside the cache fails loudly: NaN output, caches untouched.
// Caches past ATTN_BATCH_CTX cells (kq_attn_decode<HD, true, DS>, DS = 4 or 8): the head
// is split over DS workgroups by output; q/k/v, the rope row and the first chunk of K rows
// arrive by LDS-DMA with the position, K whole rows per instruction into a two-slot ring
// per wave (KDMA below), soft_max on each thread's own cells (head_dim 64), and the
// workgroup's V rows by LDS-DMA under soft_max ("Split by output").
// Timing diagnostics (MI355X_ATTN_DIAG stops) only in experiment builds
// (make variant-ops NAME=adiag VFLAGS=-DKQ_ATTN_DIAG=1); the product kernel has none.
#ifndef KQ_ATTN_DIAG
#define KQ_ATTN_DIAG 0
#endif
#if KQ_ATTN_DIAG
#define ADIAG(a) ((a).diag)
#else
#define ADIAG(a) 0
#endif
// a diagnostic stop's output: depends on every value it keeps live, always a float in [1, 2)
// (garbage bits would send the next GEMV's rms_norm and soft_max down their slow paths)
__device__ __forceinline__ float adiag_finite(uint32_t bits) { return __uint_as_float((bits & 0x007fffffu) | 0x3f800000u); }

// The settled constants ("Retired build switches of the decode attention").
// Cells whose K row / V chunk is loaded with the position, before it is known (the rest, up to
// the position, after it). All of them -> 64: TinyLlama token +2 %; 64 -> 32: +0.5 % (tg128),
// 8B equal; 128: -1 % (profiles/r05_attn_pfc_ab.txt)
constexpr int ATTN_PFC = 32;
// V-cache iterations (32 cells each) requested together in KQV, past the prefetched ones
constexpr int ATTN_VB = 8;
// K rows per thread per round of the batched KQ. head_dim 128: a K row is 64 VGPRs; two per
// round cost the short-context launch 0.7 us at Llama-3-8B (247 VGPRs)
constexpr int ATTN_KR64 = 2, ATTN_KR128 = 1;
// K-cache ring of the split kernels (KDMA below): per wave ATTN_KD slots of 64 rows (8 KiB)
constexpr int ATTN_KD = 2;
constexpr int ATTN_KSLOT = 64 * 128;

// One LDS-DMA instruction (default cache policy: the V cache is re-read token after token)
// for lanes [0, n) at LDS byte address m0 (wave-uniform), the lane mask set inside the asm.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void attn_dma16_lanes(const void *src, uint32_t m0, int lane, int n) {
    uint64_t save;
    asm volatile(
        "s_mov_b64 %0, exec\n\t"
        "v_cmp_gt_i32_e32 vcc, %2, %3\n\t"
        "s_and_b64 exec, exec, vcc\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, off\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(save)
        : "s"(m0), "s"(n), "v"(lane), "v"(src)
        : "memory", "m0", "vcc");
}
// ... all 64 lanes
__device__ __forceinline__ void attn_dma16(const void *src, uint32_t m0) {
    asm volatile(
        "s_mov_b32 m0, %0\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off"
        :
        : "s"(m0), "v"(src)
        : "memory", "m0");
}
#pragma clang diagnostic pop

// ------------------------------------------------------------ steps shared with the cells split
// What every decode kernel derives from the position it loaded
struct AttnPos {
    bool bad;  // no cache cell for this position: NaN output, caches untouched
    int pos;   // the position (0 when bad)
    int n_kv;  // cells scored: pos + 1 rounded up to 32, at most n_ctx
    int n_it;  // 32-cell iterations holding a cell <= pos; later ones add exact zeros
};
__device__ __forceinline__ AttnPos attn_pos(int pos_in, int n_ctx) {
    AttnPos p;
    p.bad = pos_in < 0 || pos_in >= n_ctx;
    p.pos = p.bad ? 0 : pos_in;
    const int n_kv = (p.pos + 1 + 31) / 32 * 32;
    p.n_kv = n_kv < n_ctx ? n_kv : n_ctx;
    p.n_it = (p.pos + 32) / 32;
    return p;
}

// XCD-aware head order (speed only) of a grid of n_head * DS workgroups: workgroup b runs on
// XCD b % 8, so XCD x takes the consecutive heads [x*n_head/8, (x+1)*n_head/8) (every slice of
// a head on one XCD) and a KV group's cells are fetched into the L2 of 8*gsz/n_head XCDs
// (TinyLlama: 2, Llama-3: 1) instead of all 8. A head count that is no multiple of 8: in order.
template <int DS>
__device__ __forceinline__ void attn_xcd_head(int n_head, unsigned block, int &h, int &ds) {
    h = block / DS, ds = block % DS;
    if ((n_head & 7) == 0) {
        const int x = block & 7, i = block >> 3;
        h = x * (n_head >> 3) + i / DS;
        ds = i % DS;
    }
}

// N 16-B pieces of a K row into kv: a row of the cache, the new cell's LDS copy, the row
// prefetched into registers. One function per source, as the sites name what they read; the
// sources stay separate branches at every site (a select among them takes the register copy's
// address and puts it in scratch).
template <int N>
__device__ __forceinline__ void attn_k_row_global(uint4 (&kv)[N], const uint16_t *row) {
#pragma unroll
    for (int i = 0; i < N; ++i) kv[i] = ((const uint4 *)row)[i];
}
template <int N>
__device__ __forceinline__ void attn_k_row_lds(uint4 (&kv)[N], const uint16_t *k16) {
#pragma unroll
    for (int i = 0; i < N; ++i) kv[i] = ((const uint4 *)k16)[i];
}
template <int N>
__device__ __forceinline__ void attn_k_row_regs(uint4 (&kv)[N], const uint4 (&kpre)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) kv[i] = kpre[i];
}
// ... of a lane's 128 B of a ring slot, piece i at position i ^ sw
template <int N>
__device__ __forceinline__ void attn_k_row_ring(uint4 (&kv)[N], const uint8_t *rowp, int sw) {
#pragma unroll
    for (int i = 0; i < N; ++i) kv[i] = *(const uint4 *)(rowp + 16 * (i ^ sw));
}

// soft_max's max over the block: every wave publishes its own, then (after a barrier) reads all four
__device__ __forceinline__ void wave_fmax_publish(float *scal, int t, float wmx) {
    if ((t & 63) == 0) scal[t >> 6] = wmx;
}
__device__ __forceinline__ float wave4_fmax(const float *scal) {
    return fmaxf(fmaxf(scal[0], scal[1]), fmaxf(scal[2], scal[3]));
}
// the group sum of cells 4g..4g+3 (lanes 4g..4g+3, ec each) in the vaddvq order (e0 + e1) + (e2 + e3): in lane 4g
__device__ __forceinline__ float quad_group_sum(float ec) {
    const float s01 = ec + dpp_mov_f32<0xB1>(ec);  // lane 4g: e0 + e1, lane 4g+2: e2 + e3
    return s01 + dpp_mov_f32<0x4E>(s01);           // lane 4g: (e0 + e1) + (e2 + e3)
}

// The group sums' double sum over a block of four waves: each wave sums its own groups (se) and
// publishes one double with its min last-bit exponent and a non-finite flag in the caller's
// scratch (sum[4], gmin[4], bad[4]); after the barrier the four wave sums are the total, and
// the return value says whether it meets softmax_group_sum's exactness bound (every partial sum
// exact: any order gives ggml's in-order bits). Where it does not, the caller sums gsum in order.
__device__ __forceinline__ bool block_sum_exact4(const SumExact &se, int wv, int ln, double *sum, int *gmin, int *bad,
                                                 double &total) {
    const bool wbad = __any(se.bad);
    const int wgmin = wave_imin(se.gmin);
    double wsum = se.part;  // (meaningful only where exact)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o, 64);
    if (ln == 0) {
        sum[wv] = wsum;
        gmin[wv] = wgmin;
        bad[wv] = wbad;
    }
    __syncthreads();
    const int gm = min(min(gmin[0], gmin[1]), min(gmin[2], gmin[3]));
    total = (sum[0] + sum[1]) + (sum[2] + sum[3]);
    return sum_exact_ok(total, gm, (bad[0] | bad[1] | bad[2] | bad[3]) != 0);
}

// KQV's inner step: the new cell's value (*vnew, the LDS copy) in place of cell pos of the 8
// cells c0 .. c0 + 7 of a V chunk, where it lies among them
__device__ __forceinline__ uint4 attn_patch_new_cell(uint4 v, int pos, int c0, const uint16_t *vnew) {
    uint32_t vw[4] = {v.x, v.y, v.z, v.w};
    if (pos >= c0 && pos < c0 + 8) {
        const int l = pos - c0;
        vw[l >> 1] = (vw[l >> 1] & (0xffff0000u >> (16 * (l & 1)))) | ((uint32_t)*vnew << (16 * (l & 1)));
    }
    return make_uint4(vw[0], vw[1], vw[2], vw[3]);
}
// ... and the four packed FMAs of 8 cells into the accumulator's words
__device__ __forceinline__ void attn_fma4(uint32_t (&acc)[4], uint4 v, uint4 p) {
    acc[0] = pk_fma_w(v.x, p.x, acc[0]);
    acc[1] = pk_fma_w(v.y, p.y, acc[1]);
    acc[2] = pk_fma_w(v.z, p.z, acc[2]);
    acc[3] = pk_fma_w(v.w, p.w, acc[3]);
}

// ------------------------------------------------------------ the per-head body
// attn_lds (kq_attn_decode.hip) on the device: the per-head LDS layout below, before any staged V rows
__device__ __forceinline__ int attn_lds_dev(int hd, int n_ctx) {
    const int gsum = (n_ctx / 4) * 8 <= hd * 64 ? 0 : (n_ctx / 4) * 8;
    return 6 * hd + n_ctx * 6 + hd * 64 + 16 + gsum;
}

// The per-head body, shared by kq_attn_decode (one 256-thread workgroup per head) and the
// fused kernels (kq_attn_oproj.hip, kq_layer.hip: several heads per workgroup, 256
// TPH threads each; every __syncthreads() is reached by all of them in the same order since the
// control flow depends only on the position). t: the thread's index within the head's 256;
// smem: this head's LDS (attn_lds bytes); out: where output d of the head goes
// (out[d], global or LDS); may_write: this workgroup may store the new KV cell.
// TPH: threads per head (256; 128 for head_dim 64 in the fused kernel, where 4 heads share a
// workgroup and 256 threads each would cap it at 128 VGPRs): the register path holds one
// cell per thread (n_kv <= TPH), KQV runs HD * 4 / TPH (d, j) items per thread.
// VPF0: V-cache iterations (32 cells each) prefetched with the position (0: 8 / ITEMS).
// OUT_WT: out is global memory, stored write-through (sc1) for the next launch (kq_rows'
// outputs likewise, store_y).
// SC1_IN: q / k / v were written in this launch by other workgroups (the persistent layer,
// kq_layer.hip): every load of them is an agent-scope (sc1) load, as the hand-off requires.
// DS > 1 (kq_attn_decode past ATTN_BATCH_CTX cells, BATCH): the head is split over DS
// workgroups by output dimension; workgroup ds computes the whole KQ and soft_max (every slice
// needs every weight) and KQV for outputs [ds HD/DS, (ds + 1) HD/DS) only, from its slice of
// the V rows, staged in LDS by LDS-DMA as soon as the position is known. One workgroup's
// cache reads for KQV drop to 1/DS and arrive in one round under KQ and soft_max, where the
// unsplit head waits for them in n_kv / (32 VB) dependent batches after soft_max. The
// accumulation order of every output is unchanged (bit-exact).
template <int HD, int TPH = 256, int VPF0 = 0, bool OUT_WT = false, bool SC1_IN = false, bool BATCH = false,
          int DS = 1>
__device__ __forceinline__ void attn_head(const AttnArgs &a, int h, int t, uint8_t *smem, float *out,
                                          bool may_write, int ds = 0) {
    auto ldin = [](const float *p) {
        if (SC1_IN) return __uint_as_float(__hip_atomic_load((const uint32_t *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        return *p;
    };
    static_assert(HD == 64 || HD == 128, "head_dim");
    constexpr int KV4 = HD / 8;          // 16-B pieces of one K-cache row
    static_assert(TPH == 256 || (TPH == 128 && HD == 64), "threads per head");
    // BATCH (kq_attn_decode): the cache loads past the prefetched cells are batched (KR K rows
    // per round, ATTN_VB V chunks); the fused kernels' register budgets keep one K row and
    // one V chunk per step (PAIR off)
    constexpr bool PAIR = BATCH && TPH == 256 && !SC1_IN;
    static_assert(DS == 1 || (PAIR && (HD / DS) % 4 == 0 && HD / DS * 4 <= TPH), "output slices");
    constexpr int RS = HD / DS;  // V rows (outputs) of this workgroup
    // KDMA (split head_dim-64 kernel, caches past the register path): KQ's K rows arrive by
    // LDS-DMA in chunks of 256 cells, each wave loading the 64 rows its own lanes score, eight
    // whole rows (1 KiB, 8 lanes per row) per instruction. The per-thread row loads of the
    // other paths put 64 different rows under every load instruction, which the texture
    // path serves at about one cache line per cycle (measured: ~0.85 us per 256 cells per
    // workgroup); here an instruction touches 8 rows' lines. Within a row the 16-B chunks are
    // stored at position k ^ ((lane >> 1) & 7) so that each thread's row reads are free of
    // bank conflicts; the dot product itself is unchanged (bit-exact).
    // head_dim 128: a row is 256 B, two lanes per cell (each holding half the row; the odd
    // lane continues the even lane's accumulators: the NEON order), 128 cells per chunk.
    constexpr bool KDMA = PAIR && DS > 1;
    constexpr int CPC = HD == 64 ? 256 : 128;  // (KDMA) cells per chunk, CPC / 4 per wave
    // (KDMA) soft_max on the cells each thread scored (max kept from KQ, group sums across the
    // quad's lanes, every wave summing the groups itself): head_dim 64 (one cell per lane);
    // three barriers instead of five
    constexpr bool KSM = KDMA && HD == 64;
    constexpr int VB = PAIR ? ATTN_VB : 4;
    constexpr int KR = HD == 64 ? ATTN_KR64 : ATTN_KR128;  // K rows per thread per round (register budget)
    constexpr int ITEMS = HD * 4 / TPH;  // KQV (d, j) items per thread
    constexpr int VPF = VPF0 > 0 ? VPF0 : (ATTN_PFC / 32 < 8 / ITEMS ? ATTN_PFC / 32 : 8 / ITEMS);  // prefetched 32-cell iterations per item
    constexpr int KPF = ATTN_PFC < TPH ? ATTN_PFC : TPH;  // K rows prefetched (thread t < KPF)
    static_assert(VPF <= VB, "KQV's first batch holds the prefetched V iterations");
    const int gsz = a.n_head / a.n_head_kv;
    const int g = h / gsz;
    const int kvw = a.n_head_kv * HD;
    if (ADIAG(a) == 4) return;  // diagnostics (MI355X_ATTN_DIAG): empty launch

    // LDS (attn_lds): q16 | k16 | v16 (HD f16 each) | w (n_ctx f32) | p16 (n_ctx f16) |
    // red (HD*32 f16 accumulators) | scal (max, 1/sum, 2 pad) [| gsum]; every piece 16-B aligned
    uint16_t *q16 = (uint16_t *)smem;
    uint16_t *k16 = q16 + HD;
    uint16_t *v16 = k16 + HD;
    float *w = (float *)(smem + 6 * HD);
    uint16_t *p16 = (uint16_t *)(w + a.n_ctx);
    h16 *red = (h16 *)(p16 + a.n_ctx);
    float *scal = (float *)(red + HD * 32);
    // per group of 4 cells: (double)((e0 + e1) + (e2 + e3)); lives in `red` (free until
    // KQV) when it fits, past scal otherwise
    double *gsum = (a.n_ctx / 4) * 8 <= HD * 64 ? (double *)red : (double *)(scal + 4);
    const int VSTR = 2 * a.n_ctx + 16;
    uint8_t *const vlds = smem + (attn_lds_dev(HD, a.n_ctx) + 15) / 16 * 16;
    uint8_t *const kring = vlds + RS * VSTR;  // (KDMA) after the V rows
    // (KDMA) chunk c of K rows, cells [CPC c, CPC c + CPC) clamped to lim - 1, into this
    // wave's ring slot: wave wv's CPC / 4 rows, 1 KiB (8 or 4 whole rows) per instruction.
    // Lane ln of the wave reads the 128 B at slot + 128 ln: a whole row (head_dim 64) or half
    // of one (128: row ln / 2, half ln & 1), its 16-B chunk k at position k ^ ((ln >> 1) & 7)
    auto issue_k = [&](int c, int lim) {
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
        const uint32_t slot = (uint32_t)(uintptr_t)(LDS void *)(kring + (wv * ATTN_KD + c % ATTN_KD) * ATTN_KSLOT);
        const int r = ln >> 3, pp = ln & 7;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int lr = 8 * i + r;  // the lane that reads these 128 B
            int row = CPC * c + (CPC / 4) * wv + (HD == 64 ? lr : lr >> 1);
            row = row < lim ? row : lim - 1;  // (rows past n_kv are never read)
            const int k = (HD == 64 ? 0 : 8 * (lr & 1)) + (pp ^ ((lr >> 1) & 7));
            const uint8_t *src = (const uint8_t *)(a.k_cache + (int64_t)row * kvw + (int64_t)g * HD) + 16 * k;
            attn_dma16(src, __builtin_amdgcn_readfirstlane(slot + 1024 * i));
        }
    };

    // ---- 0. position-independent loads, issued with the position
    const int pos_in = *a.pos;
    float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
    float rc = 0.f, rs = 0.f;  // rope_row: cos/sin of the thread's pair, staged with the position
    if constexpr (KDMA) {
        // q | k | v | the rope row (rope_row) by one LDS-DMA of wave 0 into the first KiB of the
        // V-row area (free until KQ is done), then the first chunk of K rows, all before the
        // position is known. Every memory operation of this path is then an LDS-DMA whose
        // waits are counted here, so rope waits for its inputs only (vmcnt retires in order:
        // a compiler-visible load here would make every later wait cover the K rows too).
        if (t < 64) {  // (head_dim 128: two instructions, q | k then v | rope)
            constexpr int L = HD / 4;  // lanes per vector
#pragma unroll
            for (int i = 0; i < HD / 64; ++i) {
                const int e = 64 * i + t;  // 16-B piece of the 4 HD floats
                const float *src = e < L       ? a.q + (int64_t)h * HD + 4 * e
                                   : e < 2 * L ? a.k + (int64_t)g * HD + 4 * (e - L)
                                   : e < 3 * L ? a.v + (int64_t)g * HD + 4 * (e - 2 * L)
                                   : a.rope_row ? a.rope_table + 4 * (e - 3 * L)
                                                : a.q + (int64_t)h * HD;
                attn_dma16(src, (uint32_t)(uintptr_t)(LDS void *)(vlds + 1024 * i));
            }
        }
        issue_k(0, a.n_ctx);
    } else if (t < HD / 2) {
        if (a.rope_row) {
            rc = a.rope_table[2 * t];
            rs = a.rope_table[2 * t + 1];
        }
        const float *qp = a.q + (int64_t)h * HD + 2 * t;
        const float *kp = a.k + (int64_t)g * HD + 2 * t;
        x0 = ldin(qp);
        x1 = ldin(qp + 1);
        y0 = ldin(kp);
        y1 = ldin(kp + 1);
    } else if (t < HD / 2 + HD) {
        x0 = ldin(a.v + (int64_t)g * HD + (t - HD / 2));
    }
    uint4 kpre[KV4] = {};
    if (!KDMA && t < a.n_ctx && t < KPF && ADIAG(a) != 5) {  // (diag 5: no cache loads, stop after rope; timing only)
        attn_k_row_global(kpre, a.k_cache + (int64_t)t * kvw + (int64_t)g * HD);
    }
    // V rows: staged in LDS on the KDMA path, prefetched into registers on the others (a run-time
    // choice between the two turned KQV's cache loads into flat loads: tg1024 -4 %)
    uint4 vpre[ITEMS][VPF] = {};
#pragma unroll
    for (int ii = 0; ii < ITEMS && !KDMA; ++ii) {
        const int item = t + TPH * ii, d = item >> 2, j = item & 3;
        const uint16_t *vr = a.v_cache + (int64_t)(g * HD + d) * a.n_ctx + 8 * j;
#pragma unroll
        for (int it = 0; it < VPF; ++it)
            if (32 * it < a.n_ctx && ADIAG(a) != 5) vpre[ii][it] = *(const uint4 *)(vr + 32 * it);
    }

    // (attn_pos's lines, kept here: through the helper the compiler knows pos >= 0 earlier, and
    // the fused kernels and kq_attn_decode<HD, false> come out 1 to 5 instructions longer)
    const bool bad = pos_in < 0 || pos_in >= a.n_ctx;  // no cache cell for this position
    const int pos = bad ? 0 : pos_in;
    int n_kv = (pos + 1 + 31) / 32 * 32;
    n_kv = n_kv < a.n_ctx ? n_kv : a.n_ctx;
    // V rows of the head's kv group (DS > 1: the slice's RS rows), cells [0, n_kv), into LDS
    // (KDMA): wave w takes rows [w RS / 4, (w + 1) RS / 4); local row r at vlds + r * VSTR;
    // completion: vmcnt(0) + barrier before KQV. Issued once KQ's cache loads have been used:
    // vmcnt retires in issue order, so a wait for any load issued after the DMAs (rope's inputs,
    // KQ's K rows) would wait for them too; soft_max issues no memory loads and runs under them.
    // A cell past pos holds whatever the cache holds (its weight is an exact 0); the new cell is
    // patched from v16 as on the register path.
    auto issue_v_rows = [&]() {
        if (!KDMA) return;
        // every earlier load has been used; the builtin (unlike an asm wait) tells the compiler,
        // which would otherwise wait vmcnt(0) later for loads it cannot prove consumed (a kpre
        // row on a path that skipped it) — and so for these DMAs behind them. On every path.
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        if (bad) return;
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
        const int gran = n_kv / 8;  // 16-B granules of a row
#pragma unroll 1
        for (int r = wv * (RS / 4); r < (wv + 1) * (RS / 4); ++r) {
            const uint8_t *src = (const uint8_t *)(a.v_cache + (int64_t)(g * HD + ds * RS + r) * a.n_ctx);
#pragma unroll 1
            for (int i = 0; 64 * i < gran; ++i) {
                const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS void *)(vlds + r * VSTR + 1024 * i));
                const int n = __builtin_amdgcn_readfirstlane(gran - 64 * i);
                attn_dma16_lanes(src + 1024 * i + 16 * ln, m0, ln, n < 64 ? n : 64);
            }
        }
    };

    if constexpr (KDMA) {  // the staged q | k | v | rope row landed (wave 0: all but chunk 0's 8 DMAs)
        if (t < 64) __builtin_amdgcn_s_waitcnt(0x0F78);  // vmcnt(8)
        __syncthreads();
        const float *stg = (const float *)vlds;
        if (t < HD / 2) {
            x0 = stg[2 * t], x1 = stg[2 * t + 1];
            y0 = stg[HD + 2 * t], y1 = stg[HD + 2 * t + 1];
            rc = stg[3 * HD + 2 * t], rs = stg[3 * HD + 2 * t + 1];  // (used with rope_row only)
        } else if (t < HD / 2 + HD) {
            x0 = stg[2 * HD + (t - HD / 2)];
        }
        if (!a.rope_row) {  // the position's row of the whole table: loaded now and waited for
                            // here (with chunk 0: the slow path), so no load of the compiler's
                            // is pending where this branch rejoins the rope_row path
            if (t < HD / 2) {
                const float *row = a.rope_table + (int64_t)pos * HD;
                rc = row[2 * t];
                rs = row[2 * t + 1];
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        }
    }
    // ---- 1. rope(q), rope(k), v -> f16 in LDS; the writer stores the new cell
    const float *tc = a.rope_table + (a.rope_row ? 0 : (int64_t)pos * (HD / 2) * 2);
    const bool writer = may_write && !bad && (h % gsz) == 0 && ds == 0;
    if (t < HD / 2) {
        const float c = (KDMA || a.rope_row) ? rc : tc[2 * t], s = (KDMA || a.rope_row) ? rs : tc[2 * t + 1];
        const float2 rq = rope_pair(x0, x1, c, s);
        q16[2 * t] = h2u(f2h_rne(rq.x));
        q16[2 * t + 1] = h2u(f2h_rne(rq.y));
        const float2 rk = rope_pair(y0, y1, c, s);
        const uint16_t k0 = h2u(f2h_rne(rk.x)), k1 = h2u(f2h_rne(rk.y));
        k16[2 * t] = k0;
        k16[2 * t + 1] = k1;
        if (writer) *(uint32_t *)(a.k_cache + (int64_t)pos * kvw + (int64_t)g * HD + 2 * t) = k0 | ((uint32_t)k1 << 16);
    } else if (t < HD / 2 + HD) {
        const int d = t - HD / 2;
        const uint16_t vv = h2u(f2h_rne(x0));
        v16[d] = vv;
        if (writer) a.v_cache[(int64_t)(g * HD + d) * a.n_ctx + pos] = vv;
    }
    __syncthreads();
    if (ADIAG(a) == 1 || ADIAG(a) == 5) {  // diagnostics: stop after the loads and rope
        vm_wait<0>();  // (staged V DMAs, KDMA) land before the wave ends
        if (t < HD) out[t] = adiag_finite(__float_as_uint(x0) ^ kpre[0].x ^ vpre[0][0].x ^ vpre[0][VPF - 1].y);
        return;
    }

    // ---- 2 + 3. KQ and soft_max, in one of four forms: in registers (n_kv <= TPH); the K ring
    // (KDMA) with soft_max on the thread's own cells (KSM); the cache rows KR per round (PAIR) or
    // one by one; and, for all but KSM, soft_max over w in LDS
    if ((!KDMA || HD == 64) && n_kv <= TPH) {  // one cell per thread: score, max, exp and group sum stay in registers
        const int c = t;
        float sc = -INFINITY;
        if (KDMA) __builtin_amdgcn_s_waitcnt(0x0F70);  // (KDMA) chunk 0 of the K rows landed
        if (c < n_kv && c <= pos) {
            uint4 kv[KV4];
            if (c == pos) {
                attn_k_row_lds(kv, k16);
            } else if (KDMA) {  // chunk 0's ring slot of this wave: cell t at lane t & 63
                const int ln = t & 63;
                attn_k_row_ring(kv, kring + (__builtin_amdgcn_readfirstlane(t >> 6) * ATTN_KD) * ATTN_KSLOT + 128 * ln, (ln >> 1) & 7);
            } else if (KPF < TPH && c >= KPF) {  // a cell past the prefetched ones (below the position)
                attn_k_row_global(kv, a.k_cache + (int64_t)c * kvw + (int64_t)g * HD);
            } else {  // prefetched with the position
                attn_k_row_regs(kv, kpre);
            }
            sc = vec_dot_f16_rows<HD>(kv, (const uint4 *)q16) * a.scale;
        }
        issue_v_rows();
        wave_fmax_publish(scal, t, wave_fmax(sc));  // max (order-free): per wave, then over the 4 waves
        __syncthreads();
        if (ADIAG(a) == 2) {  // diagnostics: stop after KQ
            vm_wait<0>();  // (staged V DMAs, KDMA) land before the wave ends
            if (t < HD) out[t] = adiag_finite(__float_as_uint(sc) ^ vpre[0][0].x ^ vpre[0][VPF - 1].y);
            return;
        }
        const float mx = TPH == 256 ? wave4_fmax(scal) : fmaxf(scal[0], scal[1]);
        const float ec = c < n_kv && sc != -INFINITY ? v_expf(sc - mx) : 0.0f;
        const float g4 = quad_group_sum(ec);
        if ((t & 3) == 0 && c < n_kv) gsum[t >> 2] = (double)g4;
        __syncthreads();
        // every wave computes the same sum (no barrier to publish it): ggml's in-order double
        // sum, as a tree where that is exact (softmax_group_sum)
        const double sum = softmax_group_sum(gsum, n_kv / 4, t & 63);
        const float inv = (float)(1.0 / sum);
        if (c < n_kv) p16[c] = h2u(f2h_rne(ec * inv));
        __syncthreads();
        if (ADIAG(a) == 3) {  // diagnostics: stop after soft_max
            vm_wait<0>();  // (staged V DMAs, KDMA) land before the wave ends
            if (t < HD) out[t] = adiag_finite((uint32_t)p16[t] ^ vpre[0][0].x ^ vpre[0][VPF - 1].y);
            return;
        }
    } else {
        if constexpr (KDMA) {
            const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
            const int n_ch = (n_kv + CPC - 1) / CPC;  // chunks; wave wv scores cells CPC c + (CPC / 4) wv + ...
            const int sw = (ln >> 1) & 7;             // this lane's 128 B: chunk k at position k ^ sw
            // head_dim 128: this lane's half of q (chunks 8 (ln & 1) + k)
            uint4 qh[8];
            if (HD == 128) attn_k_row_lds(qh, q16 + 64 * (ln & 1));
            // chunk 0 was issued with the position (prologue); the cache stores of the new cell,
            // issued since, are older than chunk 1 and covered by its waits
            if (n_ch > 1) issue_k(1, n_kv);
            static_assert(ATTN_KD == 2, "the waits below cover two slots per wave");
            float mloc = -INFINITY;  // (KSM) the max over this thread's cells
            for (int c = 0; c < n_ch; ++c) {
                // chunk c landed: the younger chunks in flight (8 DMAs each) may still be
                if (c + 1 < n_ch) __builtin_amdgcn_s_waitcnt(0x0F78);  // vmcnt(8)
                else __builtin_amdgcn_s_waitcnt(0x0F70);
                if constexpr (HD == 64) {
                const int cell = 256 * c + t;
                if (cell < n_kv) {
                    uint4 kv[KV4];
                    if (cell == pos) attn_k_row_lds(kv, k16);
                    else attn_k_row_ring(kv, kring + (wv * ATTN_KD + c % ATTN_KD) * ATTN_KSLOT + 128 * ln, sw);
                    const float sc = cell <= pos ? vec_dot_f16_rows<HD>(kv, (const uint4 *)q16) * a.scale : -INFINITY;
                    w[cell] = sc;
                    mloc = fmaxf(mloc, sc);
                }
                } else {  // head_dim 128: lanes 2m, 2m + 1 score cell 128 c + 32 wv + m
                    const int cell = 128 * c + 32 * wv + (ln >> 1);
                    const bool live = cell < n_kv;  // (uniform per lane pair: both or neither)
                    uint4 kv[8];
                    if (cell == pos) attn_k_row_lds(kv, k16 + 64 * (ln & 1));
                    else attn_k_row_ring(kv, kring + (wv * ATTN_KD + c % ATTN_KD) * ATTN_KSLOT + 128 * ln, sw);
                    // ggml_vec_dot_f16 (NEON FP16), accumulator j over chunks j, 4+j, 8+j, 12+j:
                    // every lane runs its own two chunks per accumulator from 0 (the even lane's
                    // are the first two steps), then again from the even lane's result (the odd
                    // lane's are the last two); the odd lane reduces (acc0 + acc2) + (acc1 + acc3)
                    uint32_t x[4][4], y[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t c0[4] = {kv[j].x, kv[j].y, kv[j].z, kv[j].w};
                        const uint32_t c1[4] = {kv[4 + j].x, kv[4 + j].y, kv[4 + j].z, kv[4 + j].w};
                        const uint32_t q0[4] = {qh[j].x, qh[j].y, qh[j].z, qh[j].w};
                        const uint32_t q1[4] = {qh[4 + j].x, qh[4 + j].y, qh[4 + j].z, qh[4 + j].w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[j][k] = pk_fma_w(c1[k], q1[k], pk_fma_w(c0[k], q0[k], 0u));
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t e = dpp_w<0xA0>(x[j][k]);  // quad_perm [0,0,2,2]: the even lane's
                            y[j][k] = pk_fma_w(c1[k], q1[k], pk_fma_w(c0[k], q0[k], e));
                        }
                    }
                    h16 sv[8];
#pragma unroll
                    for (int l = 0; l < 8; ++l) {
                        const h16 s0 = lane_of(y[0], l) + lane_of(y[2], l);
                        const h16 s1 = lane_of(y[1], l) + lane_of(y[3], l);
                        sv[l] = s0 + s1;
                    }
                    const float dot = f16x8_reduce(sv);
                    if (live && (ln & 1)) w[cell] = cell <= pos ? dot * a.scale : -INFINITY;
                }
                if (c + ATTN_KD < n_ch) issue_k(c + ATTN_KD, n_kv);  // (this slot's reads were used above)
            }
            if constexpr (KSM) {
                // soft_max over the thread's own cells 256 c + t (written by this thread: no
                // barrier before reading them back). max: per wave, then over the 4 waves
                wave_fmax_publish(scal, t, wave_fmax(mloc));
                issue_v_rows();
                __syncthreads();
                if (ADIAG(a) == 2) {  // diagnostics: stop after KQ
                    vm_wait<0>();
                    if (t < HD) out[t] = adiag_finite(__float_as_uint(w[t]));
                    return;
                }
                const float mx = wave4_fmax(scal);
                SumExact se;
                for (int c = 0; c < n_ch; ++c) {  // (uniform trip count: every lane in the quad sums)
                    const int cell = 256 * c + t;
                    const float sv = cell < n_kv ? w[cell] : -INFINITY;
                    const float ec = sv == -INFINITY ? 0.0f : v_expf(sv - mx);
                    const float g4 = quad_group_sum(ec);
                    if (cell < n_kv) {
                        w[cell] = ec;
                        if ((t & 3) == 0) {
                            gsum[cell >> 2] = (double)g4;
                            se.add(g4);
                        }
                    }
                }
                // the block's total through the K ring (free: every chunk consumed), where it is
                // provably the in-order sum; else that sum itself, by every wave
                double sum;
                if (!block_sum_exact4(se, wv, ln, (double *)kring, (int *)(kring + 32), (int *)(kring + 48), sum))
                    sum = seq_group_sum(gsum, n_kv / 4, ln);
                const float inv = (float)(1.0 / sum);
                for (int c = 0; c < n_ch; ++c) {
                    const int cell = 256 * c + t;
                    if (cell < n_kv) p16[cell] = h2u(f2h_rne(w[cell] * inv));
                }
                __syncthreads();
                if (ADIAG(a) == 3) {  // diagnostics: stop after soft_max
                    vm_wait<0>();
                    if (t < HD) out[t] = adiag_finite((uint32_t)p16[t]);
                    return;
                }
            }
        } else if constexpr (PAIR) {
            // KQ + scale + mask; the first pass (c == t) scores the prefetched row. KR cells per
            // thread per round, every row requested before any is used.
            for (int c0 = t; c0 < n_kv; c0 += KR * TPH) {
                uint4 kv[KR][KV4];  // (branches, not selects: a select of the three sources takes
                                    // kpre's address and puts it in scratch)
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const int c = c0 + r * TPH;
                    if (c < n_kv && c <= pos) {
                        if (c == pos) attn_k_row_lds(kv[r], k16);
                        else if (r == 0 && c == t && t < KPF) attn_k_row_regs(kv[r], kpre);
                        else attn_k_row_global(kv[r], a.k_cache + (int64_t)c * kvw + (int64_t)g * HD);
                    }
                }
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const int c = c0 + r * TPH;
                    if (c < n_kv) w[c] = c <= pos ? vec_dot_f16_rows<HD>(kv[r], (const uint4 *)q16) * a.scale : -INFINITY;
                }
            }
        } else {
            // KQ + scale + mask; the first pass (c == t) scores the prefetched row
            for (int c = t; c < n_kv; c += TPH) {
                float s = -INFINITY;
                if (c <= pos) {
                    uint4 kv[KV4];
                    // (this site keeps its own lines: with the attn_k_row_* helpers here the
                    // head_dim-128 fused kernels keep kpre in scratch, 256 VGPRs)
                    if (c == pos) {
#pragma unroll
                        for (int i = 0; i < KV4; ++i) kv[i] = ((const uint4 *)k16)[i];
                    } else if (c == t && t < KPF) {
#pragma unroll
                        for (int i = 0; i < KV4; ++i) kv[i] = kpre[i];
                    } else {
                        const uint4 *kr = (const uint4 *)(a.k_cache + (int64_t)c * kvw + (int64_t)g * HD);
#pragma unroll
                        for (int i = 0; i < KV4; ++i) kv[i] = kr[i];
                    }
                    s = vec_dot_f16_rows<HD>(kv, (const uint4 *)q16) * a.scale;
                }
                w[c] = s;
            }
        }
        if constexpr (!KSM) {
        issue_v_rows();
        __syncthreads();
        if (ADIAG(a) == 2) {  // diagnostics: stop after KQ
            vm_wait<0>();  // (staged V DMAs, KDMA) land before the wave ends
            if (t < HD) out[t] = adiag_finite(__float_as_uint(w[t]) ^ vpre[0][0].x ^ vpre[0][VPF - 1].y);
            return;
        }
        // max (order-free), then exp + group sums
        if (t < 64) {
            float m = -INFINITY;
            for (int c = t; c < n_kv; c += 64) m = fmaxf(m, w[c]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            if (t == 0) scal[0] = m;
        }
        __syncthreads();
        const float mx = scal[0];
        for (int gi = t; gi < n_kv / 4; gi += TPH) {
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wv = w[4 * gi + k];
                e[k] = wv == -INFINITY ? 0.0f : v_expf(wv - mx);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) w[4 * gi + k] = e[k];
            gsum[gi] = (double)((e[0] + e[1]) + (e[2] + e[3]));  // the vaddvq group sum, in parallel
        }
        __syncthreads();
        if (t < 64) {  // ggml's in-order double sum over the groups (a tree where exact)
            double sum = softmax_group_sum(gsum, n_kv / 4, t);
            sum = 1.0 / sum;
            if (t == 0) scal[1] = (float)sum;
        }
        __syncthreads();
        const float inv = scal[1];
        for (int c = t; c < n_kv; c += TPH) p16[c] = h2u(f2h_rne(w[c] * inv));
        __syncthreads();
        if (ADIAG(a) == 3) {  // diagnostics: stop after soft_max
            vm_wait<0>();  // (staged V DMAs, KDMA) land before the wave ends
            if (t < HD) out[t] = adiag_finite((uint32_t)p16[t] ^ vpre[0][0].x ^ vpre[0][VPF - 1].y);
            return;
        }
        }
    }

    // ---- 4. KQV: thread (d, j) -> accumulator j of output d, from the V rows in LDS (KDMA), in
    // batches (PAIR) or one chunk per step (the fused kernels). The V chunks past the prefetched ones
    // are requested ATTN_VB iterations at a time before any of them is used (a loop that
    // loads and then uses each chunk pays one memory latency per 32 cells: tg1024 -18 %).
    if (KDMA) {  // the staged V rows landed (every wave's DMAs); then the new cell patched into
               // them from v16, so the loop below reads LDS only, without per-cell branches
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), seen by the compiler (no stale waits below)
        __syncthreads();
        if (!bad)
            for (int r = t; r < RS; r += TPH) *(uint16_t *)(vlds + r * VSTR + 2 * pos) = v16[ds * RS + r];
        __syncthreads();
    }
    if (ADIAG(a) == 6) {  // diagnostics: stop before KQV's arithmetic (the staged V rows landed)
        if (t < HD) out[t] = adiag_finite((uint32_t)p16[t] ^ *(const uint32_t *)(vlds + 16 * t));
        return;
    }
    const int n_it = (pos + 32) / 32;  // iterations holding a cell <= pos; later ones add exact zeros
#pragma unroll
    for (int ii = 0; ii < (DS > 1 ? 1 : ITEMS); ++ii) {
        const int item = t + TPH * ii;
        const int vr_l = item >> 2, j = item & 3;  // (DS > 1: the local V row; threads past RS * 4 idle)
        if (DS > 1 && vr_l >= RS) break;
        const int d = DS > 1 ? ds * RS + vr_l : vr_l;
        const uint16_t *vr = a.v_cache + (int64_t)(g * HD + d) * a.n_ctx;
        uint32_t acc[4] = {};  // lanes 2k, 2k+1 of accumulator j in word k
        if constexpr (KDMA) {  // V rows in LDS (new cell patched): 8 iterations' reads, then their FMAs
            const uint8_t *vrow = vlds + vr_l * VSTR + 16 * j;
            const uint8_t *prow = (const uint8_t *)p16 + 16 * j;
            int it = 0;
            for (; it + 8 <= n_it; it += 8) {
                uint4 vb[8], pb[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    vb[k] = *(const uint4 *)(vrow + 64 * (it + k));
                    pb[k] = *(const uint4 *)(prow + 64 * (it + k));
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) attn_fma4(acc, vb[k], pb[k]);
            }
            for (; it < n_it; ++it) attn_fma4(acc, *(const uint4 *)(vrow + 64 * it), *(const uint4 *)(prow + 64 * it));
        } else if constexpr (PAIR) {
            for (int it0 = 0; it0 < n_it; it0 += VB) {
                uint4 vb[VB];
#pragma unroll
                for (int k = 0; k < VB; ++k) {
                    const int it = it0 + k;
                    if (it0 == 0 && k < VPF) {
                        vb[k] = vpre[ii][k < VPF ? k : 0];
                    } else if (it < n_it) {
                        vb[k] = *(const uint4 *)(vr + 32 * it + 8 * j);
                    }
                }
#pragma unroll
                for (int k = 0; k < VB; ++k) {
                    const int it = it0 + k;
                    if (it < n_it) {
                        const int c0 = 32 * it + 8 * j;
                        attn_fma4(acc, attn_patch_new_cell(vb[k], pos, c0, v16 + d), *(const uint4 *)(p16 + c0));
                    }
                }
            }
        } else {  // one V chunk per iteration (the fused kernels)
            for (int it = 0; it < n_it; ++it) {  // VPF prefetched iterations, then global loads
                const int c0 = 32 * it + 8 * j;
                uint4 vv;
                if (it < VPF) {
#pragma unroll
                    for (int k = 0; k < VPF; ++k)
                        if (k == it) vv = vpre[ii][k];
                } else {
                    vv = *(const uint4 *)(vr + c0);
                }
                // (this site keeps its own lines: with attn_patch_new_cell + attn_fma4 here
                // kq_attn_decode<128, false> grows by 17 instructions)
                const uint4 pp = *(const uint4 *)(p16 + c0);
                uint32_t vw[4] = {vv.x, vv.y, vv.z, vv.w};
                const uint32_t pw[4] = {pp.x, pp.y, pp.z, pp.w};
                if (pos >= c0 && pos < c0 + 8) {  // the new cell: LDS copy
                    const int l = pos - c0;
                    vw[l >> 1] = (vw[l >> 1] & (0xffff0000u >> (16 * (l & 1)))) | ((uint32_t)v16[d] << (16 * (l & 1)));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = pk_fma_w(vw[k], pw[k], acc[k]);
            }
        }
        const float o = f16x8_reduce_quad(acc);  // accumulators j = 0..3 of output d: one quad of lanes
        if (j == 0) {
            const float ov = bad ? __builtin_nanf("") : o;
            if (OUT_WT) asm volatile("global_store_dword %0, %1, off sc1" ::"v"(out + d), "v"(ov) : "memory");
            else out[d] = ov;
        }
    }
}

}  // namespace kq
