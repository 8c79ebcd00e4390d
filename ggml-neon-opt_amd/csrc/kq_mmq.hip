// kq_mmq.hip — batched (prefill) K-quant x Q8_K matmul on MFMA, bit-exact.
//
// Replaces, for ne11 = M > 1 activation columns, the per-(row, column) vec_dot
// calls of ggml_compute_forward_mul_mat_one_chunk (ggml-cpu.c:1194,
// README.md:136) with int8 matrix cores while keeping the reference's numerics:
//  * per 32-element sub-block j, v_mfma_i32_32x32x32_i8 gives exact int32 dots of
//    32 weight rows x 32 activation columns (K = 32 = one Q4_K sub-block). Q4_K:
//    the 6-bit scale is split into 3-bit halves folded into the weight operand
//    (nibble*half <= 105 fits int8), so sumi = 8*S8 + S1 accumulates across all
//    sub-blocks inside the matrix core; Q5_K: the same split with the fifth bit as a third
//    MFMA into S8. Exact int32 either way (README.md:754-771);
//  * summins = sum_j mn_j(row) * (bsums[2j] + bsums[2j+1]) on one f16 MFMA 32x32x16
//    (bs = 64*hi + lo split, below): integers below 2^24, so exact (README.md:741-744);
//  * the fp32 chain per output element runs superblock by superblock in order,
//    sumf = fmaf(-(float)summins, dmin, sumf); sumf = fmaf((float)sumi, d, sumf)
//    (fmsub/fmadd, README.md:551/:614) -- the same ops as the GEMV kernels, so
//    the result equals the oracle's mul_mat (and ggml's vec_dot loop) bit for bit.
// Tiles: a workgroup of RT / 16 waves owns 64 * CW activation columns x RT weight rows (2 x
// RT / 32 waves of 32 rows x 32 * CW columns); each superblock's Q8L activation blocks (304 B
// per column) and weight blocks (144 / 176 / 240 B per row) are double-buffered in LDS by
// LDS-DMA, a fixed number of DMA instructions per wave and superblock.
// The steps, one function each: mmq_tile_of (which tile), mmq_issue (a superblock's DMA),
// q45_superblock / q6_superblock (a superblock of one wave's 32 x 32 * CW outputs),
// mmq_store (the outputs, the ADD and the KV-cache epilogue); mmq_tile is the loop.
// kq_mmq_id is the same loop over the pairs of a MoE prompt grouped by expert (mi355x_mul_mat_id's
// grouped form): a tile's weight base, activation rows and output rows come from kq_moe_group's table.
// MFMA operand maps (verified with exact integer data, tools/mfma_layout_check.hip):
//   i8 32x32x32: lane l (r = l&31, h = l>>5) holds A[r][16h+j], B[16h+j][r], j<16;
//   f16 32x32x16: A[r][8h+j], B[8h+j][r], j<8; C/D (every dtype): col = r,
//   row = (reg&3) + 8(reg>>2) + 4h (mmq_acc_col: the activation column, A being the activation).
#include "kq_device.h"
#include "kq_ops_device.h"

// Timing-only ablations of kq_mmq<Q4_K>, compile time so the product kernel carries none of
// them (as run-time branches they cost 40 VGPRs and a wave per SIMD): 1 no chain epilogue,
// 2 no scale split, 4 no integer MFMA, 8 no mins MFMA, 16 launch-order tiles.
// Experiment build: make variant-mmq NAME=d13 VFLAGS=-DKQ_MMQ_DIAG=13 (tools/mmq_diag.sh).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#ifndef KQ_MMQ_DIAG
#define KQ_MMQ_DIAG 0
#endif

namespace kq {

typedef int i32x4m __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) {
    u16x2 r;
    __builtin_memcpy(&r, &v, 4);
    return r;
}
__device__ __forceinline__ uint32_t as_u32(u16x2 v) {
    uint32_t r;
    __builtin_memcpy(&r, &v, 4);
    return r;
}

// Weight rows per workgroup: RT = 64 (4 waves, 2 x 2 of 32 x 32) or 128 (8 waves, 2 x 4):
// the activation tile is fetched once per RT rows, so RT = 128 halves its LDS-DMA traffic.
// Weight bytes per row in the LDS tile: the superblock itself (Q4_K 144, Q5_K 176,
// 16-B aligned rows), or for Q6_K (210 B, any alignment) the 14 granules from the
// 16-B boundary below it.
__host__ __device__ constexpr int mmq_row_bytes(int type) { return type == Q6_K ? MMQ_Q6_STRIDE : block_bytes(type); }
__host__ __device__ constexpr int mmq_b_instr(int type, int rt) { return rt * mmq_row_bytes(type) / 1024; }  // 9 / 11 / 15 per 64 rows
static_assert(64 * MMQ_Q6_STRIDE % 1024 == 0, "whole DMA instructions per 64 rows");

// Accumulator element i (of 16) of a lane in half h of a 32 x 32 MFMA result -> its activation
// column within the 32-column tile (the lane's weight row is lane & 31).
__device__ __forceinline__ int mmq_acc_col(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
// y.d of the activation column that accumulator element i belongs to, in the 32-column tile that
// starts at column c of superblock buffer A (read where it is used).
__device__ __forceinline__ float mmq_yd(const uint8_t *A, int c, int i, int h) {
    return *(const float *)(A + (c + mmq_acc_col(i, h)) * Q8L_STRIDE);
}

// Scale-split multipliers of sub-blocks 2jp (lo nibbles) and 2jp+1 (hi nibbles) as 16-bit
// pairs: sc = 8*sh + sl; sh / sl bytes of all four sub-blocks of a word split with two
// masks, then one byte-broadcast permute per multiplier.
struct SplitScales {
    uint32_t sh03, sl03, sh47, sl47;
};
__device__ __forceinline__ SplitScales split_scales(uint32_t s03, uint32_t s47) {
    return {(s03 >> 3) & 0x07070707u, s03 & 0x07070707u, (s47 >> 3) & 0x07070707u, s47 & 0x07070707u};
}
__device__ __forceinline__ uint32_t bcast16(uint32_t w, int k) {  // byte k of w in both 16-bit lanes
    return __builtin_amdgcn_perm(0u, w, 0x0c000c00u + 0x00010001u * (uint32_t)k);
}
// The four multipliers of sub-block pair jp: lh / ll the 3-bit halves of sub-block 2jp's scale
// (lo nibbles), hh / hl those of sub-block 2jp+1 (hi nibbles).
struct SplitMul {
    u16x2 lh, ll, hh, hl;
};
__device__ __forceinline__ SplitMul split_mul(const SplitScales &ss, int jp) {
    const int kb = 2 * (jp & 1);  // bytes of sub-blocks 2jp, 2jp+1 in their word
    const uint32_t sh = jp < 2 ? ss.sh03 : ss.sh47, sl = jp < 2 ? ss.sl03 : ss.sl47;
    return {as_u16x2(bcast16(sh, kb)), as_u16x2(bcast16(sl, kb)), as_u16x2(bcast16(sh, kb + 1)), as_u16x2(bcast16(sl, kb + 1))};
}
// sumi = 8 * S8 + S1 per accumulator element
__device__ __forceinline__ i32x16 combine_s8_s1(const i32x16 &s8, const i32x16 &s1) {
    i32x16 r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = 8 * s8[i] + s1[i];
    return r;
}
__device__ __forceinline__ i32x16 mfma_i8(const u32x4 &a, const u32x4 &b, const i32x16 &c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const i32x4m *)&a, *(const i32x4m *)&b, c, 0, 0, 0);
}

// B operand of the mins MFMA: [mn_0..7 | 64*mn_0..7] of the lane's row (h selects the half),
// from the 6-bit mins bytes m03 / m47. Each byte pair becomes a 16-bit pair with a magic f16
// exponent (v_perm with a constant byte): 0x64 -> 1024 + mn (ulp 1), 0x54 -> 64 + mn/16
// (ulp 1/16); subtracting the magic and scaling by 1 or 1024 gives mn or 64*mn exactly.
__device__ __forceinline__ f16x8 mins_operand(uint32_t m03, uint32_t m47, int h) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const uint32_t magic = h ? 0x54545454u : 0x64646464u;
    const _Float16 base = h ? (_Float16)64.0f : (_Float16)1024.0f, mul = h ? (_Float16)1024.0f : (_Float16)1.0f;
    const h2 nb2 = {(_Float16)-base, (_Float16)-base}, m2 = {mul, mul};
    const uint32_t w[4] = {__builtin_amdgcn_perm(magic, m03, 0x04010400u), __builtin_amdgcn_perm(magic, m03, 0x04030402u),
                           __builtin_amdgcn_perm(magic, m47, 0x04010400u), __builtin_amdgcn_perm(magic, m47, 0x04030402u)};
    f16x8 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h2 v;
        __builtin_memcpy(&v, &w[k], 4);
        v = (v + nb2) * m2;
        r[2 * k] = v[0];
        r[2 * k + 1] = v[1];
    }
    return r;
}

// Q6_K superblock of one 32x32 tile: 8 chunks of 32 elements; a lane's 16 values of a
// chunk are one 16-element scale group g (int8 scale sc). The scaled weight
// W = sc * (q - 32) (|W| <= 4096) rides in the MFMA operands as two int8 bytes,
// W = 256 * hi + lo with lo in [-128, 127] and hi = (W + 128) >> 8 in [-16, 16]: one
// packed 16-bit multiply-add per two values gives T = W + 128 = q*sc + (128 - 32 sc),
// whose high byte is hi and whose low byte xor 0x80 is lo. Both sums accumulate over
// the whole superblock in the matrix core, sumi = 256 * S_hi + S_lo exactly -- the
// reference's isum - 32*isum_mins with its scales (README.md:369-394 / lane_q6K) --
// instead of two half-empty MFMAs and 32 VALU multiplies per chunk.
// With CW column tiles per wave the weight operands of a chunk are built once and feed
// CW MFMA pairs (the activation operands differ per tile).
// A: the superblock buffer, c0: the wave's first activation column in it, Bbase: the lane's weight
// row there (row n of the matrix, superblock b), r / h: the lane's column and half.
template <int CW>
__device__ __forceinline__ void q6_superblock(const MmqArgs &a, const uint8_t *A, int c0, const uint8_t *Bbase, int n, int b,
                                              int r, int h, f32x16 *sumf) {
    float yd[16 * CW];
#pragma unroll
    for (int ct = 0; ct < CW; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) yd[16 * ct + i] = mmq_yd(A, c0 + 32 * ct, i, h);
    const int nrow = n < a.n_rows ? n : a.n_rows - 1;  // the DMA clamped the same way
    const uint32_t mis = (uint32_t)((uintptr_t)(a.w + (int64_t)nrow * a.row_stride + (int64_t)b * 210) & 15u);
    const uint8_t *region = Bbase + mis;
    const uint32_t s4 = (uint32_t)((uintptr_t)region & 3u);
    const uint8_t *bb = region - s4;
    const u32x4 SC = realign(*(const u32x4a *)(bb + 192), *(const uint32_t *)(bb + 208), s4);
    const uint32_t dh = (*(const uint32_t *)(bb + 208) >> (8u * s4)) & 0xffffu;
    i32x16 shi[CW], slo[CW];
#pragma unroll
    for (int ct = 0; ct < CW; ++ct) shi[ct] = slo[ct] = i32x16{};
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
        const u32x4 L0 = realign(*(const u32x4a *)(bb + 64 * nh + 16 * h), *(const uint32_t *)(bb + 64 * nh + 16 * h + 16), s4);
        const u32x4 L1 = realign(*(const u32x4a *)(bb + 64 * nh + 32 + 16 * h),
                                 *(const uint32_t *)(bb + 64 * nh + 48 + 16 * h), s4);
        const u32x4 H = realign(*(const u32x4a *)(bb + 128 + 32 * nh + 16 * h),
                                *(const uint32_t *)(bb + 144 + 32 * nh + 16 * h), s4);
        // unrolled by 2: fully unrolled, the compiler kept every chunk's MFMA results live (376
        // VGPRs, one wave per SIMD; profiles/r02_prefill_ablation.md)
#pragma unroll 2
        for (int cc = 0; cc < 4; ++cc) {
            const int c = 4 * nh + cc;  // chunk: elements 32c .. 32c+31
            const u32x4 L = (cc & 1) ? L1 : L0;
            const uint32_t sh = (uint32_t)(cc >> 1) * 4u;
            const int sc = h ? sbyte(SC, 2 * c + 1) : sbyte(SC, 2 * c);
            const uint32_t scw = (uint32_t)sc & 0xffffu, cw = (uint32_t)(128 - 32 * sc) & 0xffffu;
            const u16x2 scp = {(uint16_t)scw, (uint16_t)scw}, cp = {(uint16_t)cw, (uint16_t)cw};
            u32x4 blo, bhi;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t x = ((L[k] >> sh) & 0x0f0f0f0fu) | (((H[k] >> (2u * cc)) & 0x03030303u) << 4);  // q, 0..63
                const uint32_t t0 = as_u32(as_u16x2(__builtin_amdgcn_perm(0u, x, 0x0c010c00u)) * scp + cp);  // values 0, 1
                const uint32_t t1 = as_u32(as_u16x2(__builtin_amdgcn_perm(0u, x, 0x0c030c02u)) * scp + cp);  // values 2, 3
                blo[k] = __builtin_amdgcn_perm(t1, t0, 0x06040200u) ^ 0x80808080u;
                bhi[k] = __builtin_amdgcn_perm(t1, t0, 0x07050301u);
            }
#pragma unroll
            for (int ct = 0; ct < CW; ++ct) {
                const u32x4 act = *(const u32x4 *)(A + (c0 + 32 * ct + r) * Q8L_STRIDE + 16 + 32 * c + 16 * h);
                shi[ct] = mfma_i8(act, bhi, shi[ct]);
                slo[ct] = mfma_i8(act, blo, slo[ct]);
            }
        }
    }
    const float xd = h2f(dh);
#pragma unroll
    for (int ct = 0; ct < CW; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i)  // sum += d_all*y.d*(isum - 32*isum_mins)
            sumf[ct][i] = fmaf(xd * yd[16 * ct + i], (float)(256 * shi[ct][i] + slo[ct][i]), sumf[ct][i]);
}

// Q4_K / Q5_K superblock of one wave's 32 rows x 32 * CW columns: sumi = 8 * S8 + S1 over the 8
// sub-blocks in the matrix core (the scale split, below), summins on one f16 MFMA, then the
// reference's fp32 update per element. A: the superblock buffer, c0: the wave's first activation
// column in it, Bt: the lane's weight row there, r / h: the lane's column and half.
template <int TYPE, int CW>
__device__ __forceinline__ void q45_superblock(const uint8_t *A, int c0, const uint8_t *Bt, int r, int h, f32x16 *sumf) {
    const uint8_t *At[CW];  // this lane's activation column of each tile
#pragma unroll
    for (int ct = 0; ct < CW; ++ct) At[ct] = A + (c0 + 32 * ct + r) * Q8L_STRIDE;
    const u32x4 hdr = *(const u32x4 *)Bt;
    // 6-bit scales / mins of the lane's row (get_scale_min_k4, README.md:732-739)
    const uint32_t s03 = hdr.y & 0x3f3f3f3fu;
    const uint32_t m03 = hdr.z & 0x3f3f3f3fu;
    const uint32_t s47 = (hdr.w & 0x0f0f0f0fu) | ((hdr.y >> 2) & 0x30303030u);
    const SplitScales ss = split_scales(s03, s47);
    const uint32_t m47 = ((hdr.w >> 4) & 0x0f0f0f0fu) | ((hdr.z >> 2) & 0x30303030u);
    i32x16 s8[CW], s1[CW];
#pragma unroll
    for (int ct = 0; ct < CW; ++ct) s8[ct] = s1[ct] = i32x16{};
    u32x4 qh = {0u, 0u, 0u, 0u};
    if (TYPE == Q5_K) qh = *(const u32x4 *)(Bt + 16 + 16 * h);
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {  // sub-blocks 2jp (lo nibbles) and 2jp+1 (hi nibbles)
        const u32x4 qv = *(const u32x4 *)(Bt + (TYPE == Q5_K ? 48 : 16) + 32 * jp + 16 * h);
        const u32x4 lo = qv & 0x0f0f0f0fu, hi = (qv >> 4) & 0x0f0f0f0fu;
        u32x4 alo[CW], ahi[CW];
#pragma unroll
        for (int ct = 0; ct < CW; ++ct) {
            alo[ct] = *(const u32x4 *)(At[ct] + 16 + 64 * jp + 16 * h);
            ahi[ct] = *(const u32x4 *)(At[ct] + 48 + 64 * jp + 16 * h);
        }
        const uint32_t sw = jp < 2 ? s03 : s47;
        const int sc_lo = (int)((sw >> (16u * (uint32_t)(jp & 1))) & 0xffu);
        const int sc_hi = (int)((sw >> (16u * (uint32_t)(jp & 1) + 8u)) & 0xffu);
        if (TYPE == Q4_K && (KQ_MMQ_DIAG & 6)) {  // diagnostics (timing only)
#pragma unroll
            for (int ct = 0; ct < CW; ++ct) {
                if (!(KQ_MMQ_DIAG & 4)) {
                    s8[ct] = mfma_i8(alo[ct], lo, s8[ct]);
                    s1[ct] = mfma_i8(ahi[ct], hi, s1[ct]);
                } else {
                    s8[ct][jp] += (int)(lo.x ^ alo[ct].y ^ (uint32_t)sc_lo);
                    s1[ct][jp] += (int)(hi.y ^ ahi[ct].x ^ (uint32_t)sc_hi);
                }
            }
            continue;
        }
        // sc = 8*sh + sl (3-bit halves): nibble*sh and nibble*sl <= 105 stay int8, and a packed
        // 16-bit multiply scales two bytes per half without carries, so the per-sub-block scale
        // rides in the MFMA operand and both sums accumulate across sub-blocks in the matrix core
        // (exact int32).
        const SplitMul m = split_mul(ss, jp);
        if (TYPE == Q4_K) {
            u32x4 b8lo, b1lo, b8hi, b1hi;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b8lo[k] = as_u32(as_u16x2(lo[k]) * m.lh);
                b1lo[k] = as_u32(as_u16x2(lo[k]) * m.ll);
                b8hi[k] = as_u32(as_u16x2(hi[k]) * m.hh);
                b1hi[k] = as_u32(as_u16x2(hi[k]) * m.hl);
            }
#pragma unroll
            for (int ct = 0; ct < CW; ++ct) {
                s8[ct] = mfma_i8(alo[ct], b8lo, s8[ct]);
                s1[ct] = mfma_i8(alo[ct], b1lo, s1[ct]);
                s8[ct] = mfma_i8(ahi[ct], b8hi, s8[ct]);
                s1[ct] = mfma_i8(ahi[ct], b1hi, s1[ct]);
            }
        } else {
            // Q5_K: q = ql + 16 qh (ql the nibble, qh the fifth bit): W = sc q = 8 (sh ql + 2 sc qh)
            // + sl ql with sh ql, sl ql <= 105 and 2 sc qh <= 126 all int8, so three MFMAs per
            // sub-block, two of them into the x8 sum.
            const u16x2 scl = {(uint16_t)(2 * sc_lo), (uint16_t)(2 * sc_lo)};
            const u16x2 sch = {(uint16_t)(2 * sc_hi), (uint16_t)(2 * sc_hi)};
#pragma unroll
            for (int half = 0; half < 2; ++half) {  // sub-block 2jp (lo nibbles), then 2jp+1
                const u32x4 &qn = half ? hi : lo;
                const u16x2 m8 = half ? m.hh : m.lh, m1 = half ? m.hl : m.ll, mq = half ? sch : scl;
                u32x4 b8, b1, bq;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    b8[k] = as_u32(as_u16x2(qn[k]) * m8);
                    b1[k] = as_u32(as_u16x2(qn[k]) * m1);
                    bq[k] = as_u32(as_u16x2((qh[k] >> (uint32_t)(2 * jp + half)) & 0x01010101u) * mq);
                }
#pragma unroll
                for (int ct = 0; ct < CW; ++ct) {
                    const u32x4 &av = half ? ahi[ct] : alo[ct];
                    s8[ct] = mfma_i8(av, b8, s8[ct]);
                    s1[ct] = mfma_i8(av, b1, s1[ct]);
                    s8[ct] = mfma_i8(av, bq, s8[ct]);
                }
            }
        }
    }
    // summins = sum_j mn_j * bs_j exactly on one f16 MFMA 32x32x16 per tile (bs_j =
    // bsums[2j] + bsums[2j+1] = 64*hi + lo, lo in 0..63): A = [lo_0..7 | hi_0..7] of the
    // lane's activation column (stored so by the quantizer: the Q8L/mmq layout), B = [mn_0..7 |
    // 64*mn_0..7] of its weight row; every product and partial sum is an integer below 2^24.
    // (Four dependent f32 MFMAs 32x32x2 cost 256 cycles per superblock against 32 for this one.)
    const f16x8 bm = mins_operand(m03, m47, h);
    // the reference's fp32 update per element, superblock order
    const float xd = h2f(hdr.x & 0xffffu), xdm = h2f(hdr.x >> 16), nxdm = -xdm;
#pragma unroll
    for (int ct = 0; ct < CW; ++ct) {
        const i32x16 sumi = combine_s8_s1(s8[ct], s1[ct]);
        const f16x8 am = *(const f16x8 *)(At[ct] + 272 + 16 * h);  // [lo | hi] of bs_j (Q8L/mmq)
        const f32x16 zero = {};
        const f32x16 mins = (KQ_MMQ_DIAG & 8) ? zero : __builtin_amdgcn_mfma_f32_32x32x16_f16(am, bm, zero, 0, 0, 0);
        if (TYPE == Q4_K && !(KQ_MMQ_DIAG & 1)) {
            // two elements per packed f32 instruction (v_pk_mul_f32 / v_pk_fma_f32, each lane an
            // IEEE mul / fma: the scalar chain's bits; 8B ffn_down 3-8 % faster, the rest equal;
            // Q5_K and Q6_K gain nothing from it, profiles/r04_mmq_pkchain_ab.txt)
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            const f32x2 nxdm2 = {nxdm, nxdm}, xd2 = {xd, xd};
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const f32x2 y2 = {mmq_yd(A, c0 + 32 * ct, i, h), mmq_yd(A, c0 + 32 * ct, i + 1, h)};
                const f32x2 m2 = {mins[i], mins[i + 1]};
                const f32x2 s2 = {(float)sumi[i], (float)sumi[i + 1]};
                f32x2 acc = {sumf[ct][i], sumf[ct][i + 1]};
                acc = __builtin_elementwise_fma(m2, y2 * nxdm2, acc);  // = fma(-mins, yd*xdm, .) exactly
                acc = __builtin_elementwise_fma(s2, y2 * xd2, acc);
                sumf[ct][i] = acc.x;
                sumf[ct][i + 1] = acc.y;
            }
            continue;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float y = mmq_yd(A, c0 + 32 * ct, i, h);
            if (KQ_MMQ_DIAG & 1) {  // diagnostics (timing only)
                sumf[ct][i] += (float)sumi[i] + mins[i] + y;
            } else {  // Q5_K
                const float t = fmaf(y * xd, (float)sumi[i], -((y * xdm) * mins[i]));
                sumf[ct][i] = sumf[ct][i] + t;
            }
        }
    }
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (speed only,
// MI355X_MICROARCH.md), so the column tiles of one row tile go to blocks L, L + 8,
// L + 16, ... (one XCD): the weight tile is fetched into that XCD's L2 once and
// served from it to the others; the activation tiles fit every XCD's L2. With several
// matrices on one activation, a gets this row tile's matrix d (returned).
__device__ __forceinline__ int mmq_tile_of(const MmqArgs &a0, MmqArgs &a, int &tx, int &ty) {
    tx = blockIdx.x;
    ty = blockIdx.y;
    if (!(KQ_MMQ_DIAG & 16)) {
        const int gx = gridDim.x, L = blockIdx.y * gx + blockIdx.x;
        const int span = 8 * gx;                  // blocks per group of 8 row tiles
        const int grp = L / span, in = L - grp * span;
        const int rows_here = gridDim.y - 8 * grp < 8 ? gridDim.y - 8 * grp : 8;
        if (rows_here == 8) {
            ty = 8 * grp + in % 8;
            tx = in / 8;
        }
    }
    int d = 0;
    if (a0.n_mat > 1) {  // several matrices on one activation: this row tile's matrix
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (k < a0.n_mat && ty >= a0.tile0[k]) d = k;
        a.w = a0.mw[d];
        a.row_stride = a0.mrow_stride[d];
        a.n_rows = a0.mn_rows[d];
        a.y = a0.my[d];
        a.y_col_stride = a0.my_col_stride[d];
        a.kv_cur = a0.kv_kind[d];
        ty -= a0.tile0[d];
    }
    return d;
}

// A superblock's DMA plan: superblock b's A_INSTR activation + NB_I weight instructions of
// 1 KB into `buf`, NW per wave (the last one repeated where they do not divide).
__host__ __device__ constexpr int mmq_a_instr(int cw) { return mmq_cols(cw) * Q8L_STRIDE / 1024; }  // 19 per 64 columns (exact)
__host__ __device__ constexpr int mmq_nw(int type, int rt, int cw) {
    return (mmq_a_instr(cw) + mmq_b_instr(type, rt) + mmq_waves(rt, cw) - 1) / mmq_waves(rt, cw);
}
// instruction s of a wave: t < A_INSTR the activation tile's t-th KB, else the weight tile's
template <int TYPE, int RT, int CW>
__device__ __forceinline__ int mmq_instr_of(int wave, int s) {
    constexpr int TOTAL = mmq_a_instr(CW) + mmq_b_instr(TYPE, RT);
    const int t = wave + mmq_waves(RT, CW) * s;
    return t < TOTAL ? t : TOTAL - 1;  // pad: repeat the last one
}
// the activation column (of the launch, clamped to the last one) whose granule this lane fetches in
// activation instruction t, and which of the column's 19 granules
__device__ __forceinline__ int mmq_a_col(const MmqArgs &a, int col0, int t, int lane, int &piece) {
    const int g = 64 * t + lane;
    const int c = g / (Q8L_STRIDE / 16);
    piece = g - c * (Q8L_STRIDE / 16);
    return col0 + c < a.m_cols ? col0 + c : a.m_cols - 1;
}
// ID (kq_mmq_id): column c of the tile is Q8L row xr[s] of the workspace, read from the group
// table once per tile (mmq_id_rows), not column c itself.
template <int TYPE, int RT, int CW, bool ID = false>
__device__ __forceinline__ void mmq_issue(const MmqArgs &a, LDS uint8_t *buf, int b, int col0, int row0, int wave, int lane,
                                          const int *xr = nullptr) {
    constexpr int BSZ = block_bytes(TYPE);
    constexpr int A_BYTES = mmq_cols(CW) * Q8L_STRIDE;
    constexpr int A_INSTR = mmq_a_instr(CW);
    constexpr int NW = mmq_nw(TYPE, RT, CW);
#pragma unroll
    for (int s = 0; s < NW; ++s) {
        const int t = mmq_instr_of<TYPE, RT, CW>(wave, s);
        const uint8_t *src;
        if (t < A_INSTR) {
            int piece;
            int c = mmq_a_col(a, col0, t, lane, piece);
            if (ID) c = xr[s];
            src = a.xq + (int64_t)c * a.xq_col_stride + (int64_t)b * Q8L_STRIDE + 16 * piece;
            dma16(src, buf + 1024 * t);
        } else {
            constexpr int RG = mmq_row_bytes(TYPE) / 16;
            const int g = 64 * (t - A_INSTR) + lane;  // granule in the weight tile
            int rw = g / RG;
            int piece = g - rw * RG;
            if (TYPE == Q6_K && piece > 13) piece = 13;  // padding granules: the row's last one again
            rw = row0 + rw < a.n_rows ? row0 + rw : a.n_rows - 1;
            const uintptr_t blk = (uintptr_t)(a.w + (int64_t)rw * a.row_stride + (int64_t)b * BSZ);
            src = (const uint8_t *)(blk & ~(uintptr_t)15) + 16 * piece;
            dma16(src, buf + A_BYTES + 1024 * (t - A_INSTR));
        }
    }
}
// kq_mmq_id: xr[s], the Q8L row behind the sorted entry this lane fetches in its activation
// instruction s (the same for every superblock: read before the loop, so that no DMA of the
// loop waits for a load of the list).
template <int TYPE, int RT, int CW>
__device__ __forceinline__ void mmq_id_rows(const MmqArgs &a, const int32_t *xrow, int col0, int wave, int lane, int *xr) {
#pragma unroll
    for (int s = 0; s < mmq_nw(TYPE, RT, CW); ++s) {
        const int t = mmq_instr_of<TYPE, RT, CW>(wave, s);
        int piece;
        xr[s] = t < mmq_a_instr(CW) ? xrow[mmq_a_col(a, col0, t, lane, piece)] : 0;
    }
}

// The store of one wave's outputs: the lane's weight row n, 16 activation columns per tile from
// column cb0 on; y = mul_mat (+ res); for a prompt's k / v matrix also the KV-cache cells, as
// kq_kv_store computes them (kq_ops.hip). pair (kq_mmq_id): sorted entry m's outputs go to column
// pair[m] of y; no res, no KV cells there.
template <int CW>
__device__ __forceinline__ void mmq_store(const MmqArgs &a, const f32x16 *sumf, int n, int cb0, int h,
                                          const int32_t *pair = nullptr) {
#pragma unroll
    for (int ct = 0; ct < CW; ++ct) {
        const int cb = cb0 + 32 * ct;
        if (n < a.n_rows) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = cb + mmq_acc_col(i, h);
                if (m >= a.m_cols) continue;
                if (pair)
                    a.y[(int64_t)pair[m] * a.y_col_stride + n] = sumf[ct][i];
                else
                    a.y[(int64_t)m * a.y_col_stride + n] =
                        a.res ? sumf[ct][i] + a.res[(int64_t)m * a.res_col_stride + n] : sumf[ct][i];
            }
        }
        if (a.kv_cur) {
            const int hd = a.kv_hd;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = cb + mmq_acc_col(i, h);
                const float other = __shfl_xor(sumf[ct][i], 1, 64);  // row n ^ 1: the rope partner
                const int pos = m < a.m_cols ? a.kv_pos[m] : -1;
                if (n >= a.n_rows || pos < 0 || pos >= a.kv_n_ctx) continue;  // no cell (its output is NaN)
                if (a.kv_cur == 1) {
                    const int pr = (n % hd) >> 1;
                    const float *tc = a.kv_rope + (int64_t)pos * (hd / 2) * 2;
                    const bool odd = n & 1;
                    const float2 rk = rope_pair(odd ? other : sumf[ct][i], odd ? sumf[ct][i] : other, tc[2 * pr], tc[2 * pr + 1]);
                    a.kv_k_cache[(int64_t)pos * a.n_rows + n] = h2u(f2h_rne(odd ? rk.y : rk.x));
                } else {
                    a.kv_v_cache[(int64_t)n * a.kv_n_ctx + pos] = h2u(f2h_rne(sumf[ct][i]));
                }
            }
        }
    }
}

// One (64 * CW)-column x RT-row output tile over the whole K: RT / 16 waves, each 32 weight
// rows x 32 * CW columns (CW MFMA tiles sharing the wave's weight operands).
// id (kq_mmq_id, else null): the tile's columns are the sorted entries [col0, a.m_cols) of the group
// table: their activation rows and output columns come from its lists.
template <int TYPE, int RT, int CW, bool ID = false>
__device__ __forceinline__ void mmq_tile_at(const MmqArgs &a, int col0, int row0, const MmqIdArgs *id = nullptr) {
    constexpr int COLS = mmq_cols(CW);
    constexpr int A_BYTES = COLS * Q8L_STRIDE;
    constexpr int BUF = A_BYTES + RT * mmq_row_bytes(TYPE);
    static_assert(BUF == mmq_buf_bytes(TYPE, RT, CW), "host and kernel agree on the buffer size");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave & 1, wn = wave >> 1;  // the wave's column half and its 32 rows
    const int r = lane & 31, h = lane >> 5;
    const int nb = a.nb;

    f32x16 sumf[CW];
#pragma unroll
    for (int ct = 0; ct < CW; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) sumf[ct][i] = 0.f;

    int xr[mmq_nw(TYPE, RT, CW)];
    if (ID) mmq_id_rows<TYPE, RT, CW>(a, id->xrow, col0, wave, lane, xr);
    mmq_issue<TYPE, RT, CW, ID>(a, (LDS uint8_t *)smem, 0, col0, row0, wave, lane, xr);
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        // One barrier per superblock (profiles/r03_mmq_onebar_tile128.txt): superblock b (the only
        // DMA in flight) landed; after the barrier every wave's part of b is in LDS and every wave
        // has finished reading b - 1's buffer (lgkmcnt(0) before it), so b + 1 goes into that
        // buffer while b is computed
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (b + 1 < nb)
            mmq_issue<TYPE, RT, CW, ID>(a, (LDS uint8_t *)smem + ((b + 1) & 1) * BUF, b + 1, col0, row0, wave, lane, xr);
        const uint8_t *buf = smem + (b & 1) * BUF;
        const uint8_t *Bt = buf + A_BYTES + (32 * wn + r) * mmq_row_bytes(TYPE);  // this lane's weight row
        if (TYPE == Q6_K) q6_superblock<CW>(a, buf, 32 * CW * wm, Bt, row0 + 32 * wn + r, b, r, h, sumf);
        else q45_superblock<TYPE, CW>(buf, 32 * CW * wm, Bt, r, h, sumf);
    }
    mmq_store<CW>(a, sumf, row0 + 32 * wn + r, col0 + 32 * CW * wm, h, ID ? id->pair : nullptr);
}
template <int TYPE, int RT, int CW>
__device__ __forceinline__ void mmq_tile(const MmqArgs &a, int tx, int ty) {
    mmq_tile_at<TYPE, RT, CW>(a, tx * mmq_cols(CW), ty * RT);
}

// Two waves per SIMD (profiles/r04_mmq_occupancy_ab.txt); 64 x 128: one 4-wave workgroup per CU by
// LDS, so one wave per SIMD and every register; the 12-wave 192 x 64 tile: three
#define KQ_MMQ_WPE_OF(RT, CW) __attribute__((amdgpu_waves_per_eu((RT) == 64 && (CW) == 2 ? 1 : (RT) == 192 ? 3 : 2)))
template <int TYPE, int RT, int CW>
__global__ void __launch_bounds__(mmq_waves(RT, CW) * 64) KQ_MMQ_WPE_OF(RT, CW) kq_mmq(const MmqArgs a0) {
    MmqArgs a = a0;
    int tx, ty;
    mmq_tile_of(a0, a, tx, ty);
    mmq_tile<TYPE, RT, CW>(a, tx, ty);
}

// Q4_K / Q5_K and Q6_K matrices on one activation in one launch (a prompt batch's q/k with a
// Q6_K attn_v): each row tile runs its matrix's kernel body (a0.mtype), LDS sized for Q6_K.
template <int RT, int CW>
__global__ void __launch_bounds__(mmq_waves(RT, CW) * 64) KQ_MMQ_WPE_OF(RT, CW) kq_mmq_mixed(const MmqArgs a0) {
    MmqArgs a = a0;
    int tx, ty;
    const int d = mmq_tile_of(a0, a, tx, ty);
    if (a0.mtype[d] == Q6_K) {
        mmq_tile<Q6_K, RT, CW>(a, tx, ty);
    } else if (a0.mtype[d] == Q5_K) {
        // (the host never launches a Q5_K matrix on the mixed 128 x 128 tiles: beside the
        // Q6_K body its registers would spill; launch_mmq_multi takes 128 x 64 there)
        if constexpr (!(RT == 128 && CW == 2)) mmq_tile<Q5_K, RT, CW>(a, tx, ty);
    } else {
        mmq_tile<Q4_K, RT, CW>(a, tx, ty);
    }
}

// kq_mmq's tile over the pairs of a MoE prompt grouped by expert (kq_moe_group's table): the same
// superblock bodies and chain per (row, column), so the bits of kq_mmq and of kq_gemv_id. The grid
// is a function of the shapes alone (row tiles x an upper bound of the column tiles); a workgroup
// finds its bucket in the table's tile prefix (wave-uniform: at most 65 scalar reads), and with it
// the expert's weight base, its columns' activation rows and output rows. mmq_tile_of keeps the
// column tiles of a row tile, every expert's, on one XCD. Bucket n_expert (ids outside the table)
// reads no weights: NaN to its pairs' rows, as kq_gemv_id stores.
template <int TYPE, int RT, int CW>
__global__ void __launch_bounds__(mmq_waves(RT, CW) * 64) KQ_MMQ_WPE_OF(RT, CW) kq_mmq_id(const MmqArgs a0, const MmqIdArgs g) {
    MmqArgs a = a0;
    a.res = nullptr;
    a.kv_cur = 0;
    int tx, ty;
    mmq_tile_of(a0, a, tx, ty);
    const int32_t *tile0 = g.tab + moe_tab_tile0(CW);  // the prefix of this kernel's column tiles
    const int nbk = g.n_expert + 1;
    if (tx >= tile0[nbk]) return;  // past the last column tile (before any barrier)
    int e = 0;
    for (int k = 1; k < nbk; ++k)
        if (tile0[k] <= tx) e = k;  // the last bucket starting at or before tx: the non-empty one
    const int first = g.tab[MOE_TAB_FIRST + e];
    const int col0 = first + (tx - tile0[e]) * mmq_cols(CW), row0 = ty * RT;
    a.m_cols = first + g.tab[MOE_TAB_COUNT + e];  // the bucket's end: this tile's columns stop there
    if (e == g.n_expert) {
        const int ncol = a.m_cols - col0 < mmq_cols(CW) ? a.m_cols - col0 : mmq_cols(CW);
        for (int i = (int)threadIdx.x; i < ncol * RT; i += mmq_waves(RT, CW) * 64) {
            const int n = row0 + i % RT;
            if (n < a.n_rows) a.y[(int64_t)g.pair[col0 + i / RT] * a.y_col_stride + n] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    a.w = a0.w + (int64_t)e * g.nb02;
    mmq_tile_at<TYPE, RT, CW, true>(a, col0, row0, &g);
}
template __global__ void kq_mmq_id<Q4_K, 128, 1>(const MmqArgs a, const MmqIdArgs g);
template __global__ void kq_mmq_id<Q5_K, 128, 1>(const MmqArgs a, const MmqIdArgs g);
template __global__ void kq_mmq_id<Q6_K, 128, 1>(const MmqArgs a, const MmqIdArgs g);
// Q6_K: 128 x 128 where the buckets fill it (launch_mmq_id); 64 x 128 only under the MMQ_ID_Q6 knob (A/B)
template __global__ void kq_mmq_id<Q6_K, 128, 2>(const MmqArgs a, const MmqIdArgs g);
template __global__ void kq_mmq_id<Q6_K, 64, 2>(const MmqArgs a, const MmqIdArgs g);

#define KQ_MMQ_INST(RT, CW)                                       \
    template __global__ void kq_mmq<Q4_K, RT, CW>(const MmqArgs a); \
    template __global__ void kq_mmq<Q5_K, RT, CW>(const MmqArgs a); \
    template __global__ void kq_mmq<Q6_K, RT, CW>(const MmqArgs a); \
    template __global__ void kq_mmq_mixed<RT, CW>(const MmqArgs a);
KQ_MMQ_INST(64, 1)
KQ_MMQ_INST(128, 1)
KQ_MMQ_INST(128, 2)
KQ_MMQ_INST(64, 2)
// the selector-only 12-wave tile (MI355X_MMQ_TILE192): Q4_K / Q5_K
template __global__ void kq_mmq<Q4_K, 192, 1>(const MmqArgs a);
template __global__ void kq_mmq<Q5_K, 192, 1>(const MmqArgs a);

}  // namespace kq
