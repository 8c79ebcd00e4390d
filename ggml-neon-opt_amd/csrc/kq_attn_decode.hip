// kq_attn_decode.hip — the decode attention block of a llama token on gfx950 (rope + f16
// KV-cache write + KQ + soft_max + KQV): the per-head kernel in its forms (kq_attn_head.h), the
// split over cells for long caches, the per-kv-group kernel, their LDS sizing, the dispatch
// policy (attn_path) and launch_attn. The reference functions are listed in kq_ops.hip.
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "kq_common.h"
#include "kq_internal.h"
#include "kq_attn_device.h"
#include "kq_attn_head.h"
#include "kq_device.h"
#include "kq_ops_device.h"

namespace kq {

// ------------------------------------------------------------ decode attention
// One workgroup per query head (kq_attn_head.h).
// BATCH: the cache loads past the prefetched cells requested in batches (kq_attn_head.h); the
// launch takes it for caches of more than ATTN_BATCH_CTX cells only: at short context its
// code costs the head_dim-128 launch ~0.3 us (profiles/r05_attn_ab_batch_ctx.txt).
// DS > 1: DS workgroups per head, one slice of the head's outputs each (kq_attn_head.h).
constexpr int ATTN_BATCH_CTX = 256;  // caches above this many cells take kq_attn_decode<HD, true>
// Entry (DESIGN.md §7 "Kernel entry"): the pointers a head needs first are leading plain
// parameters, 14 dwords, in SGPRs at wave start with the kernarg preload (KQ_ATTN_PARAMS; the
// AttnArgs that follows repeats them for the kernels that share it). The rest of AttnArgs
// (out .. n_tok, 14 dwords) is fetched in one batch behind one wait, so no kernarg load is
// left behind a later wait; *pos is the one dependent load.
#define KQ_ATTN_PARAMS                                                                                      \
    const float *q, const float *k, const float *v, const int32_t *pos, const float *rope_table, uint16_t *k_cache, \
        uint16_t *v_cache, const AttnArgs a0
constexpr int kAttnArgsOff = 14 * 4;  // AttnArgs in the kernarg segment: after the 14 leading dwords
static_assert(offsetof(AttnArgs, out) == 56 && offsetof(AttnArgs, rope_row) == 88 && offsetof(AttnArgs, reserved0) == 104 &&
                  sizeof(AttnArgs) == 112 && alignof(AttnArgs) == 8,
              "attn_entry reads out .. n_tok as 8 + 4 + 2 dwords");
typedef uint32_t u32x2s __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
typedef uint32_t u32x8s __attribute__((ext_vector_type(8)));
__device__ __forceinline__ AttnArgs attn_entry(const float *q, const float *k, const float *v, const int32_t *pos,
                                               const float *rope_table, uint16_t *k_cache, uint16_t *v_cache) {
    const auto *ka = __builtin_amdgcn_kernarg_segment_ptr();
    u32x8s r0;
    u32x4s r1;
    u32x2s r2;
    asm volatile("s_load_dwordx8 %0, %3, %4\n\t"
                 "s_load_dwordx4 %1, %3, %5\n\t"
                 "s_load_dwordx2 %2, %3, %6\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&s"(r0), "=&s"(r1), "=&s"(r2)
                 : "s"(ka), "i"(kAttnArgsOff + 56), "i"(kAttnArgsOff + 88), "i"(kAttnArgsOff + 104));
    AttnArgs a;
    a.q = q, a.k = k, a.v = v, a.pos = pos, a.rope_table = rope_table, a.k_cache = k_cache, a.v_cache = v_cache;
    a.out = (float *)(uintptr_t)((uint64_t)r0[0] | ((uint64_t)r0[1] << 32));
    a.n_ctx = (int)r0[2], a.n_head = (int)r0[3], a.n_head_kv = (int)r0[4], a.head_dim = (int)r0[5];
    a.scale = __uint_as_float(r0[6]);
    a.diag = (int)r0[7];
    a.rope_row = (int)r1[0], a.no_store = (int)r1[1];
    a.q8_out = (uint8_t *)(uintptr_t)((uint64_t)r1[2] | ((uint64_t)r1[3] << 32));
    a.reserved0 = (int)r2[0], a.n_tok = (int)r2[1];
    return a;
}

template <int HD, bool BATCH, int DS = 1>
__global__ void __launch_bounds__(256) kq_attn_decode(KQ_ATTN_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const AttnArgs a = attn_entry(q, k, v, pos, rope_table, k_cache, v_cache);
    int h, ds;
    attn_xcd_head<DS>(a.n_head, blockIdx.x, h, ds);
    attn_head<HD, 256, 0, false, false, BATCH, DS>(a, h, threadIdx.x, smem, a.out + (int64_t)h * HD, true, ds);
}

// ------------------------------------------------------------ long caches: KQ split over cells
// The output split (kq_attn_decode<HD, true, DS>) keeps the head's scores and its V slice in
// one workgroup and scores every cell in every slice; past what its LDS holds (~3000 cells at
// head_dim 64) the one-workgroup-per-head kernel streams every K and V row of a head through
// one CU (tg4096: ~21 us per layer). For caches of more than ATTN_CELLS_MIN cells where the
// split would need 8 slices or does not fit (attn_path), the head's KQ splits over cells
// instead, in two launches (DESIGN.md §4 "KQ split over cells", profiles/r06_cells_ab.txt):
//  A kq_attn_cells: workgroup (chunk, g) scores ATTN_CHUNK cells of kv group g for EVERY query
//    head of the group (each K row read once for the gsz heads) into a score workspace
//    [n_head][n_ctx]; the workgroup whose chunk holds the position writes the new cell to both
//    caches (rope'd k, f16 v) and scores that cell from its own copy;
//  B kq_attn_cells_kqv: workgroup (h, ds): soft_max over the head's scores held in registers
//    and KQV for its RS = HD / DS outputs (16 threads per output) from its V rows, LDS-DMA'd
//    under soft_max (the new cell included: A wrote it, a kernel boundary before).
// Every score is the same NEON-FP16 vec_dot as the one-launch kernels', soft_max's max, exps,
// group sums and in-order double sum and the KQV accumulator chains are theirs: bit-exact.
constexpr int ATTN_CHUNK = 64;
constexpr int ATTN_CELLS_SLICES = 8;  // ... also where the output split needs this many slices (tg3072 +5 %, 8B tg2048 +5.5 %; 4: equal)
constexpr int ATTN_CELLS_MIN = 1024;  // only caches of more cells than this take the two launches
constexpr int ATTN_CELLS_RS64 = 8;    // B's outputs per workgroup at head_dim 64 (8: 256 workgroups for 32 heads)
constexpr int ATTN_CELLS_RS128 = 16;  // at head_dim 128 (16: 256 workgroups for 32 heads, one round)
constexpr int ATTN_CELLS_VPAD = 64;   // bytes past 2 n_ctx per V row in B's LDS (a multiple of 16)
constexpr int ATTN_CELLS_GMAX = 8;  // B's soft_max: 4-cell groups per thread in registers (n_ctx <= 8192)

template <int HD>
__global__ void __launch_bounds__(256) kq_attn_cells(const AttnArgs a, float *scores) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int KV4 = HD / 8;                        // 16-B pieces of a K row
    constexpr int KPT = ATTN_CHUNK * KV4 / 256;        // pieces per thread
    const int g = blockIdx.y, c0 = blockIdx.x * ATTN_CHUNK, t = threadIdx.x;
    const int gsz = a.n_head / a.n_head_kv;
    const int kvw = a.n_head_kv * HD;
    // every load that does not depend on the position goes out with it: the chunk's K rows
    // (cells < n_ctx: valid memory whatever the position; cell pos's row is stale and unused)
    uint4 kr[KPT];
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = t + 256 * u, r = i / KV4, k = i % KV4;
        kr[u] = *(const uint4 *)(a.k_cache + (int64_t)(c0 + r) * kvw + (int64_t)g * HD + 8 * k);
    }
    const AttnPos p = attn_pos(*a.pos, a.n_ctx);  // (bad: caches untouched, B outputs NaN)
    const bool bad = p.bad;
    const int pos = p.pos, n_kv = p.n_kv;
    if (c0 >= n_kv) return;  // (uniform)
    // LDS: q16 [gsz][HD] | k16 [HD] | K rows [ATTN_CHUNK][KV4] (piece k of row r at k ^ (r % KV4))
    uint16_t *q16 = (uint16_t *)smem;
    uint16_t *k16 = q16 + gsz * HD;
    uint4 *krow = (uint4 *)(k16 + HD);
    const bool holds = pos >= c0 && pos < c0 + ATTN_CHUNK;
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = t + 256 * u, r = i / KV4, k = i % KV4;
        krow[r * KV4 + (k ^ (r % KV4))] = kr[u];
    }
    // rope(q) of the group's heads at pos (kq_attn_head.h step 1), and the new cell where held
    const float *tc = a.rope_table + (a.rope_row ? 0 : (int64_t)pos * (HD / 2) * 2);
    for (int i = t; i < gsz * (HD / 2); i += 256) {
        const int hh = i / (HD / 2), p2 = i % (HD / 2);
        const float *qp = a.q + (int64_t)(g * gsz + hh) * HD + 2 * p2;
        const float2 rq = rope_pair(qp[0], qp[1], tc[2 * p2], tc[2 * p2 + 1]);
        q16[hh * HD + 2 * p2] = h2u(f2h_rne(rq.x));
        q16[hh * HD + 2 * p2 + 1] = h2u(f2h_rne(rq.y));
    }
    if (holds) {
        for (int p2 = t; p2 < HD / 2; p2 += 256) {
            const float *kp = a.k + (int64_t)g * HD + 2 * p2;
            const float2 rk = rope_pair(kp[0], kp[1], tc[2 * p2], tc[2 * p2 + 1]);
            const uint16_t k0 = h2u(f2h_rne(rk.x)), k1 = h2u(f2h_rne(rk.y));
            k16[2 * p2] = k0;
            k16[2 * p2 + 1] = k1;
            if (!bad) *(uint32_t *)(a.k_cache + (int64_t)pos * kvw + (int64_t)g * HD + 2 * p2) = k0 | ((uint32_t)k1 << 16);
        }
        for (int d = t; d < HD && !bad; d += 256)
            a.v_cache[(int64_t)(g * HD + d) * a.n_ctx + pos] = h2u(f2h_rne(a.v[(int64_t)g * HD + d]));
    }
    __syncthreads();
    for (int i = t; i < ATTN_CHUNK * gsz; i += 256) {  // lane <-> cell, waves <-> heads
        const int r = i % ATTN_CHUNK, hh = i / ATTN_CHUNK, c = c0 + r;
        if (c >= n_kv) continue;
        float sc = -INFINITY;  // cells past pos: masked
        if (c <= pos) {
            uint4 kv[KV4];
            if (c == pos) {
                attn_k_row_lds(kv, k16);
            } else {  // (the chunk's own swizzle, by row: not attn_k_row_ring's)
#pragma unroll
                for (int k = 0; k < KV4; ++k) kv[k] = krow[r * KV4 + (k ^ (r % KV4))];
            }
            sc = vec_dot_f16_rows<HD>(kv, (const uint4 *)(q16 + hh * HD)) * a.scale;
        }
        scores[(int64_t)(g * gsz + hh) * a.n_ctx + c] = sc;
    }
}

// B: every input of the workgroup — the head's n_kv scores and its RS = HD / DS V rows over
// cells [0, n_kv) — arrives by LDS-DMA issued at entry, all in flight at once (a thread's KQV
// chain runs over n_kv / 32 iterations in order: loading them from global memory as it goes
// paid one memory latency per batch). soft_max waits for the scores only (a counted vmcnt: the
// V rows were issued after them), so the V rows land while it runs; KQV reads LDS only.
// LDS: the scores (n_ctx f32; once in registers the region holds the group sums, then p16) |
// red (KQV words, RS x 16 u32) | scal (24 f32: wave maxima, wave ok flags, wave sums as f64) |
// the V rows (RS x VSTR).
template <int VM>
__device__ __forceinline__ void waitcnt_vm_le() {  // s_waitcnt vmcnt(VM) (expcnt, lgkmcnt free)
    static_assert(VM >= 0 && VM < 64, "vmcnt is 6 bits");
    __builtin_amdgcn_s_waitcnt((VM & 15) | ((VM >> 4) << 14) | 0x0F70);
}
__device__ __forceinline__ void waitcnt_vm_floor8(int n) {  // vmcnt(8 floor(min(n, 63) / 8)) <= n
    switch ((n > 63 ? 63 : n) >> 3) {
    case 0: waitcnt_vm_le<0>(); break;
    case 1: waitcnt_vm_le<8>(); break;
    case 2: waitcnt_vm_le<16>(); break;
    case 3: waitcnt_vm_le<24>(); break;
    case 4: waitcnt_vm_le<32>(); break;
    case 5: waitcnt_vm_le<40>(); break;
    case 6: waitcnt_vm_le<48>(); break;
    default: waitcnt_vm_le<56>(); break;
    }
}
template <int HD, int DS>
__global__ void __launch_bounds__(256) kq_attn_cells_kqv(const AttnArgs a, const float *scores) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int RS = HD / DS;  // outputs of this workgroup
    static_assert(RS * 16 <= 256 && (RS & (RS - 1)) == 0 && RS >= 4, "16 threads per output, whole rows per wave");
    int h, ds;
    attn_xcd_head<DS>(a.n_head, blockIdx.x, h, ds);
    const int t = threadIdx.x, ln = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = h / (a.n_head / a.n_head_kv);
    const AttnPos p = attn_pos(*a.pos, a.n_ctx);
    const bool bad = p.bad;
    const int n_kv = p.n_kv, n_it = p.n_it;
    float *w = (float *)smem;
    double *gsum = (double *)smem;
    uint16_t *p16 = (uint16_t *)smem;
    uint32_t *red = (uint32_t *)(w + a.n_ctx);
    float *scal = (float *)(red + RS * 16);
    uint8_t *vlds = (uint8_t *)(scal + 24);
    const int VSTR = 2 * a.n_ctx + ATTN_CELLS_VPAD;  // rows 16 words apart in the banks
    int nv = 0;  // this wave's V-row DMAs (issued after its score DMAs)
    {
        const uint8_t *src = (const uint8_t *)(scores + (int64_t)h * a.n_ctx);
        const int sg = n_kv / 4;
        for (int i = wv; 64 * i < sg; i += 4) {
            const int n = sg - 64 * i < 64 ? sg - 64 * i : 64;
            attn_dma16_lanes(src + 1024 * i + 16 * ln,
                             __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS void *)((uint8_t *)w + 1024 * i)), ln, n);
        }
        const int vg = n_kv / 8;
        for (int r = wv; r < RS; r += 4) {
            const uint8_t *vsrc = (const uint8_t *)(a.v_cache + (int64_t)(g * HD + ds * RS + r) * a.n_ctx);
            for (int i = 0; 64 * i < vg; ++i, ++nv) {
                const int n = vg - 64 * i < 64 ? vg - 64 * i : 64;
                attn_dma16_lanes(vsrc + 1024 * i + 16 * ln,
                                 __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS void *)(vlds + r * VSTR + 1024 * i)),
                                 ln, n);
            }
        }
    }
    waitcnt_vm_floor8(nv);  // this wave's score granules have landed (loads complete in order)
    __syncthreads();
    // soft_max (kq_attn_head.h, the general path): max (order-free), exps and the vaddvq group
    // sums, ggml's in-order double sum, p = e * (float)(1 / sum) -> f16. Thread t holds the
    // 4-cell groups t + 256 k in registers (one LDS read each, all issued together); the double
    // sum is a tree over the block where that is exact (softmax_group_sum's condition: every
    // group sum a float >= 2^(floor(log2(4 ng)) - 29), or zero), else the in-order sum of gsum.
    const int ng = n_kv >> 2;
    float4 ev[ATTN_CELLS_GMAX];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < ATTN_CELLS_GMAX; ++k) {
        const int gi = t + 256 * k;
        ev[k] = gi < ng ? ((const float4 *)w)[gi] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        m = fmaxf(m, fmaxf(fmaxf(ev[k].x, ev[k].y), fmaxf(ev[k].z, ev[k].w)));
    }
    wave_fmax_publish(scal, t, wave_fmax(m));
    __syncthreads();  // (also: every score is in registers, the region is free)
    const float mx = wave4_fmax(scal);
    SumExact se;
#pragma unroll
    for (int k = 0; k < ATTN_CELLS_GMAX; ++k) {
        const int gi = t + 256 * k;
        if (gi < ng) {
            float4 e = ev[k];
            e.x = e.x == -INFINITY ? 0.0f : v_expf(e.x - mx);
            e.y = e.y == -INFINITY ? 0.0f : v_expf(e.y - mx);
            e.z = e.z == -INFINITY ? 0.0f : v_expf(e.z - mx);
            e.w = e.w == -INFINITY ? 0.0f : v_expf(e.w - mx);
            ev[k] = e;
            const float gs = (e.x + e.y) + (e.z + e.w);
            gsum[gi] = (double)gs;
            se.add(gs);  // (exact when the total passes the bound: a subset's sum)
        }
    }
    double *scald = (double *)(scal + 8);
    double sum;
    if (!block_sum_exact4(se, wv, ln, scald, (int *)scal + 4, (int *)scal + 20, sum)) {  // (uniform)
        if (t < 64) {
            const double s = seq_group_sum(gsum, ng, t);
            if (t == 0) scald[4] = s;
        }
        __syncthreads();
        sum = scald[4];
    }
    __syncthreads();  // gsum's readers are done before p16 overwrites it
    const float inv = (float)(1.0 / sum);
#pragma unroll
    for (int k = 0; k < ATTN_CELLS_GMAX; ++k) {
        const int gi = t + 256 * k;
        if (gi < ng) {
            const uint32_t lo = (uint32_t)h2u(f2h_rne(ev[k].x * inv)) | ((uint32_t)h2u(f2h_rne(ev[k].y * inv)) << 16);
            const uint32_t hi = (uint32_t)h2u(f2h_rne(ev[k].z * inv)) | ((uint32_t)h2u(f2h_rne(ev[k].w * inv)) << 16);
            ((uint2 *)p16)[gi] = make_uint2(lo, hi);
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's V rows have landed
    __syncthreads();
    // KQV: word q (f16 lanes 2q, 2q + 1) of accumulator j of output vr over cells 32 it + 8 j +
    // 2 q + {0, 1}, in order: 16 threads per output, each one chain of pk_fmas
    {
        const int vr = t >> 4, jq = t & 15;
        uint32_t acc1 = 0;
        if (vr < RS) {
            const uint32_t *vrow = (const uint32_t *)(vlds + vr * VSTR) + jq;
            const uint32_t *prow = (const uint32_t *)p16 + jq;
            int it = 0;
            for (; it + 16 <= n_it; it += 16) {
                uint32_t vb[16], pb[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    vb[k] = vrow[16 * (it + k)];
                    pb[k] = prow[16 * (it + k)];
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) acc1 = pk_fma_w(vb[k], pb[k], acc1);
            }
            for (; it < n_it; ++it) acc1 = pk_fma_w(vrow[16 * it], prow[16 * it], acc1);
            red[t] = acc1;
        }
        __syncthreads();
    }
    // the GGML_F16_VEC_REDUCE of output vr_l's 4 accumulators: quad (vr_l, j = 0..3)
    const int vr_l = (t >> 2) & (RS - 1), j = t & 3;
    const bool kt = t < 4 * RS;
    uint32_t acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = red[16 * vr_l + 4 * j + k];
    const float o = f16x8_reduce_quad(acc);  // every lane active; quad (4 vr_l .. +3) holds output vr_l
    if (kt && j == 0) a.out[(int64_t)h * HD + ds * RS + vr_l] = bad ? __builtin_nanf("") : o;
}

// One workgroup per kv group (kq_attn_device.h): the group's cells [0, n_kv) are read
// once into LDS and serve its n_head/n_head_kv query heads, one wave each.
template <int HD>
__global__ void __launch_bounds__(1024) kq_attn_group(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    attn_group<HD>(a, blockIdx.x, smem, wave, (int)(blockDim.x >> 6), lane);
}

// ------------------------------------------------------------ LDS sizing, dispatch, launches
size_t attn_lds(int hd, int n_ctx) {
    const size_t gsum = (size_t)(n_ctx / 4) * 8 <= (size_t)hd * 64 ? 0 : (size_t)(n_ctx / 4) * 8;
    return (size_t)6 * hd + (size_t)n_ctx * 6 + (size_t)hd * 64 + 16 + gsum;
}
// ... plus, for the output split, the 1/ds slice of the head's V rows (rows of n_ctx f16, 16 B
// of padding each) and the K ring (KDMA)
size_t attn_lds_v(int hd, int n_ctx, int ds) {
    return (attn_lds(hd, n_ctx) + 15) / 16 * 16 + (size_t)(hd / ds) * ((size_t)n_ctx * 2 + 16) +
           (size_t)4 * ATTN_KD * ATTN_KSLOT;
}
// Output slices per head for a cache of n_ctx cells (1: no split): past the register path's
// ATTN_BATCH_CTX cells, the fewest of 4 / 8 whose V slice fits the LDS beside the rest.
// Every slice scores every cell, so the K reads grow with the slices: 16 slices at 4096 cells
// (head_dim 64) measured slower than one workgroup per head (tg4096 894 against 925 tok/s,
// profiles/r05_attn_split_ab.txt).
// The split path LDS-DMAs whole K-cache rows and V rows (16-B pieces at 16-B offsets from the
// cache bases: both caches must be 16-B aligned, else the per-head kernel runs) and stages q / k
// / v and the rope row with 16-B transfers from 4-B aligned f32 vectors: the global side of an
// LDS-DMA need not be 16-B aligned on this device (the decode graph's staged rope row sits 8 B
// into its input tensor: every decode-graph test past 256 cells runs that way).
int attn_slices(const AttnArgs &a) {
    const uintptr_t mis16 = (uintptr_t)a.v_cache | (uintptr_t)a.k_cache;
    const uintptr_t mis4 = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.rope_table;
    if (attn_impl() != MI355X_ATTN_SPLIT || a.n_ctx <= ATTN_BATCH_CTX || a.n_ctx % 8 || (mis16 & 15u) ||
        (mis4 & 3u))
        return 1;
    for (int ds = 4; ds <= 8; ds *= 2)
        if (attn_lds_v(a.head_dim, a.n_ctx, ds) <= 160 * 1024) return ds;
    return 1;
}

int attn_group_waves(const AttnArgs &a) {
    const int gsz = a.n_head / a.n_head_kv;
    return gsz < 4 ? 4 : gsz > 16 ? 16 : gsz;
}

size_t attn_group_bytes(const AttnArgs &a, int nwaves) {
    const int gsz = a.n_head / a.n_head_kv;
    return (size_t)attn_group_lds(a.head_dim, a.n_ctx, gsz < nwaves ? gsz : nwaves).total;
}

bool attn_group_ok(const AttnArgs &a, int nwaves) {
    const uintptr_t m = (uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v;  // 8-B pair loads
    return (m & 7u) == 0 && a.diag == 0 && attn_group_bytes(a, nwaves) <= 160 * 1024;
}

// MI355X_ATTN_SPLIT (the default: one workgroup per query head, split by output past 256
// cells: profiles/r05_attn_split_ab.txt), MI355X_ATTN_HEAD (one workgroup per query head at
// every size) or MI355X_ATTN_GROUP (one workgroup per kv group: each group's cells read
// once, 1/gsz of the cache traffic, +2.3 us per launch on the TinyLlama token:
// profiles/r02_attention_ab.md). Set only through mi355x_attn_impl().
std::atomic<int> g_attn_impl{MI355X_ATTN_SPLIT};
int attn_impl() { return g_attn_impl.load(); }

size_t attn_cells_lds_a(int hd, int gsz) { return (size_t)gsz * hd * 2 + (size_t)hd * 2 + (size_t)ATTN_CHUNK * hd * 2; }
// B's LDS: the scores region (p16 and the group sums reuse it), red, 96 B of scalars, and RS V
// rows of 2 n_ctx + VPAD bytes
size_t attn_cells_lds_b(int n_ctx, int rs) {
    return (size_t)n_ctx * 4 + (size_t)rs * 64 + 96 + (size_t)rs * (2 * (size_t)n_ctx + ATTN_CELLS_VPAD);
}
// head_dim 128: RS 16 (one round of workgroups) where its V rows fit the LDS, else 8
int attn_cells_rs(int hd, int n_ctx) {
    if (hd == 64) return ATTN_CELLS_RS64;
    return attn_cells_lds_b(n_ctx, ATTN_CELLS_RS128) <= 160 * 1024 ? ATTN_CELLS_RS128 : 8;
}

// The score workspace [n_head][n_ctx] f32: one grow-only buffer per (device, stream), so two
// streams' attentions never share one, allocated outside any stream capture (the backend
// reserves before it captures: attn_cells_reserve). An older, smaller buffer stays allocated:
// a captured graph may still point at it.
struct CellsScratch {
    struct Entry {
        int dev;
        hipStream_t stream;
        void *p;
        size_t bytes;
    };
    std::mutex mu;
    std::vector<Entry> cur;
};
CellsScratch &cells_scratch() {
    static CellsScratch s;
    return s;
}
void *attn_cells_buffer(size_t bytes, hipStream_t stream, bool may_alloc) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    CellsScratch &cs = cells_scratch();
    std::lock_guard<std::mutex> lk(cs.mu);
    for (auto &e : cs.cur)
        if (e.dev == dev && e.stream == stream) {
            if (e.bytes >= bytes) return e.p;
            if (!may_alloc) return nullptr;
            void *p = nullptr;
            if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
            e.p = p, e.bytes = bytes;  // (the old one is kept: graphs may read it)
            return p;
        }
    if (!may_alloc) return nullptr;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    cs.cur.push_back({dev, stream, p, bytes});
    return p;
}

bool attn_cells_applies(const AttnArgs &a) {
    const int gsz = a.n_head_kv > 0 ? a.n_head / a.n_head_kv : 0;
    return attn_impl() == MI355X_ATTN_SPLIT && a.n_ctx > ATTN_CELLS_MIN && a.n_ctx % ATTN_CHUNK == 0 &&
           a.n_ctx <= 1024 * ATTN_CELLS_GMAX &&
           (a.head_dim == 64 || a.head_dim == 128) && gsz >= 1 && gsz <= 16 &&
           (attn_slices(a) == 1 || attn_slices(a) >= ATTN_CELLS_SLICES) &&
           attn_cells_lds_b(a.n_ctx, attn_cells_rs(a.head_dim, a.n_ctx)) <= 160 * 1024 && ((uintptr_t)a.k_cache & 15u) == 0 &&
           ((uintptr_t)a.v_cache & 15u) == 0;
}

// The workspace of a decode attention that will take the two launches, allocated now (callers
// that capture graphs call this first; an eager launch allocates on its own)
int attn_cells_reserve(const AttnArgs &a, hipStream_t stream, int n_tok) {
    if (n_tok > 1 && attn_prompt_f16()) return MI355X_OK;  // kq_attn_prompt_f16 uses no workspace
    if (n_tok > 1 ? attn_stream_prompt_applies(a) : attn_stream_applies(a))
        return attn_cells_buffer(attn_stream_workspace(a, n_tok), stream, true) ? MI355X_OK : MI355X_E_WORKSPACE;
    if (n_tok > 1 || !attn_cells_applies(a)) return MI355X_OK;
    return attn_cells_buffer((size_t)a.n_head * a.n_ctx * 4, stream, true) ? MI355X_OK : MI355X_E_WORKSPACE;
}

template <int HD, int RS>
int launch_attn_cells_t(const AttnArgs &a, float *ws, hipStream_t s, const char *na, const char *nb) {
    const int gsz = a.n_head / a.n_head_kv;
    const size_t la = attn_cells_lds_a(HD, gsz), lb = attn_cells_lds_b(a.n_ctx, RS);
    const dim3 ga((unsigned)(a.n_ctx / ATTN_CHUNK), (unsigned)a.n_head_kv);
    const int rc = timed_launch(na, 0.0, kq_attn_cells<HD>, ga, dim3(256), la, s, a, ws);
    if (rc) return rc;
    allow_lds((const void *)kq_attn_cells_kqv<HD, HD / RS>, lb);
    return timed_launch(nb, 0.0, kq_attn_cells_kqv<HD, HD / RS>, dim3((unsigned)(a.n_head * (HD / RS))), dim3(256), lb, s,
                        a, (const float *)ws);
}
int launch_attn_cells(const AttnArgs &a, float *ws, hipStream_t s) {
    if (a.head_dim == 64)
        return launch_attn_cells_t<64, ATTN_CELLS_RS64>(a, ws, s, "kq::kq_attn_cells<64>", "kq::kq_attn_cells_kqv<64>");
    if (attn_cells_rs(128, a.n_ctx) == ATTN_CELLS_RS128)
        return launch_attn_cells_t<128, ATTN_CELLS_RS128>(a, ws, s, "kq::kq_attn_cells<128>", "kq::kq_attn_cells_kqv<128>");
    return launch_attn_cells_t<128, 8>(a, ws, s, "kq::kq_attn_cells<128>", "kq::kq_attn_cells_kqv<128>");
}

// The kernel launch_attn runs for these arguments (mi355x_attn_path; a captured launch without
// a reserved workspace takes MI355X_ATTN_PATH_HEAD_BATCH instead of the cells split).
int attn_path(const AttnArgs &a) {
    if (attn_stream_applies(a)) return MI355X_ATTN_PATH_STREAM;
    if (attn_impl() == MI355X_ATTN_GROUP && attn_group_ok(a, attn_group_waves(a))) return MI355X_ATTN_PATH_GROUP;
    const int ds = attn_slices(a);
    if (ds > 1 && !attn_cells_applies(a)) return ds == 4 ? MI355X_ATTN_PATH_SPLIT4 : MI355X_ATTN_PATH_SPLIT8;
    if (attn_cells_applies(a)) return MI355X_ATTN_PATH_CELLS;
    return a.n_ctx > ATTN_BATCH_CTX ? MI355X_ATTN_PATH_HEAD_BATCH : MI355X_ATTN_PATH_HEAD;
}

// kq_attn_decode<HD, BATCH, DS> over n_head * DS workgroups, logged under the name the timing
// tools and tests/golden/launch_plans.json know it by ("kq::kq_attn_decode<64, true, 4>",
// "kq::kq_attn_decode<64, false>")
template <int HD, bool BATCH, int DS>
int launch_decode(const AttnArgs &a, hipStream_t s) {
    const size_t lds = DS > 1 ? attn_lds_v(HD, a.n_ctx, DS) : attn_lds(HD, a.n_ctx);
    if (DS > 1) allow_lds((const void *)kq_attn_decode<HD, BATCH, DS>, lds);
    auto info = [] {  // (context-dependent bytes; not a roofline kernel)
        return LaunchInfo{std::string("kq::kq_attn_decode<") + std::to_string(HD) + (BATCH ? ", true" : ", false") +
                              (DS > 1 ? ", " + std::to_string(DS) : std::string()) + ">",
                          0.0};
    };
    return timed_launch_lazy(info, kq_attn_decode<HD, BATCH, DS>, dim3((unsigned)(a.n_head * DS)), dim3(256), lds, s, a.q,
                             a.k, a.v, a.pos, a.rope_table, a.k_cache, a.v_cache, a);
}
template <int HD>
int launch_decode_path(const AttnArgs &a, int path, hipStream_t s) {
    switch (path) {
    case MI355X_ATTN_PATH_SPLIT4: return launch_decode<HD, true, 4>(a, s);
    case MI355X_ATTN_PATH_SPLIT8: return launch_decode<HD, true, 8>(a, s);
    case MI355X_ATTN_PATH_HEAD_BATCH: return launch_decode<HD, true, 1>(a, s);
    default: return launch_decode<HD, false, 1>(a, s);
    }
}
template <int HD>
int launch_group(const AttnArgs &a, hipStream_t s) {
    const int nw = attn_group_waves(a);
    const size_t glds = attn_group_bytes(a, nw);
    allow_lds((const void *)kq_attn_group<HD>, glds);
    return timed_launch(HD == 64 ? "kq::kq_attn_group<64>" : "kq::kq_attn_group<128>", 0.0, kq_attn_group<HD>,
                        dim3(a.n_head_kv), dim3(64 * nw), glds, s, a);
}

int launch_attn(const AttnArgs &a, hipStream_t s) {
    int path = attn_path(a);
    if (path == MI355X_ATTN_PATH_STREAM) return launch_attn_stream(a, s);  // (unreserved under capture: E_WORKSPACE)
    if (path == MI355X_ATTN_PATH_GROUP) return a.head_dim == 64 ? launch_group<64>(a, s) : launch_group<128>(a, s);
    if (path == MI355X_ATTN_PATH_CELLS) {  // long caches past the output split: KQ split over cells, two launches
        hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(s, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone;
        void *ws = attn_cells_buffer((size_t)a.n_head * a.n_ctx * 4, s, !capturing);
        if (ws) return launch_attn_cells(a, (float *)ws, s);
        path = MI355X_ATTN_PATH_HEAD_BATCH;  // captured without a reserved workspace: the one-launch kernel
    }
    // Past the register path's 256 cells the split kernels stage the V rows in LDS by LDS-DMA as
    // soon as the position is known (all of them in flight under KQ and soft_max); shorter caches
    // keep the register prefetch, which issues V with the position itself.
    return a.head_dim == 64 ? launch_decode_path<64>(a, path, s) : launch_decode_path<128>(a, path, s);
}

int attn_impl_set(int impl) { return g_attn_impl.exchange(impl); }

}  // namespace kq
