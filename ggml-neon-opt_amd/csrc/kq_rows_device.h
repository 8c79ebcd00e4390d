// kq_rows_device.h — device helpers of the row-stream decode kernel (kq_rows.hip):
// fused Q8_K quantization into the aligned Q8L layout, the per-type
// quad partials and the counted-wait helpers.
#pragma once

#include "kq_device.h"
#include "kq_ops_device.h"

namespace kq {

// ---------------------------------------------------------------- fused Q8_K quantization
// Reductions over an aligned row of 16 lanes (DPP only): xor 1, xor 2, 8-mirror, 16-mirror.
template <typename Op>
__device__ __forceinline__ int row16_reduce(int v, Op op) {
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    return v;
}

__device__ __forceinline__ uint32_t qbyte(float iscale, float x) {
    int q = nearest_int_fused(iscale, x);
    q = q < 127 ? q : 127;  // MIN(127, v); the int8 store truncates
    return (uint32_t)q & 0xffu;
}

// One superblock per 16-lane row; lane l of the row owns x[16l .. 16l+15] (v[0..3]).
// quantize_row_q8_K_ref semantics exactly as quant_values_wave (kq_device.h):
// amax ignores NaN, max = first x with |x| == amax, iscale = -127/max (correctly
// rounded), qs = MIN(127, nearest_int(fmaf(iscale, x, 1.5*2^23))) as int8,
// bsums over the stored int8, d = 1/iscale; all-zero block -> zeros.
// Writes the Q8L block (d @0, qs @16, bsums @272) at `qb`. AM (the prefill GEMMs' blocks,
// "Q8L/mmq"): bytes 272..303 hold the f16 operand of kq_mmq's mins MFMA instead of the
// bsums: bs_j = bsums[2j] + bsums[2j+1] = 64*hi + lo (lo in 0..63) as [lo_0..7 | hi_0..7],
// integers exact in f16.
template <bool AM = false>
__device__ __forceinline__ void quant16_store(const u32x4 v[4], int l, uint8_t *qb) {
    float x[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[4 * k + 0] = __uint_as_float(v[k].x);
        x[4 * k + 1] = __uint_as_float(v[k].y);
        x[4 * k + 2] = __uint_as_float(v[k].z);
        x[4 * k + 3] = __uint_as_float(v[k].w);
    }
    // amax and the sign of the first x with |x| == amax: the largest positive and
    // the largest negated value (both >= 0, NaN dropped by fmaxf); only a tie
    // (+amax and -amax both present) needs the first-index scan.
    float mp = 0.f, mn = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mp = fmaxf(mp, x[k]);
        mn = fmaxf(mn, -x[k]);
    }
    const int mpb = row16_reduce(__float_as_int(mp), [](int a, int c) { return a > c ? a : c; });
    const int mnb = row16_reduce(__float_as_int(mn), [](int a, int c) { return a > c ? a : c; });
    const float m = __int_as_float(mpb > mnb ? mpb : mnb);
    bool neg = mnb > mpb;
    if (mpb == mnb && mpb != 0) {  // tie: serial `if (ax > amax)` keeps the first index
        uint32_t key = 0xffffffffu;
#pragma unroll
        for (int k = 15; k >= 0; --k)
            if (fabsf(x[k]) == m) key = 2u * (uint32_t)(16 * l + k) + (x[k] < 0.f ? 1u : 0u);
        key = (uint32_t)row16_reduce((int)key, [](int a, int c) { return (uint32_t)a < (uint32_t)c ? a : c; });
        neg = (key & 1u) != 0;
    }
    const float maxv = neg ? -m : m;
    const float iscale = -127.f / maxv;
    u32x4 q;
    q.x = qbyte(iscale, x[0]) | (qbyte(iscale, x[1]) << 8) | (qbyte(iscale, x[2]) << 16) | (qbyte(iscale, x[3]) << 24);
    q.y = qbyte(iscale, x[4]) | (qbyte(iscale, x[5]) << 8) | (qbyte(iscale, x[6]) << 16) | (qbyte(iscale, x[7]) << 24);
    q.z = qbyte(iscale, x[8]) | (qbyte(iscale, x[9]) << 8) | (qbyte(iscale, x[10]) << 16) |
          (qbyte(iscale, x[11]) << 24);
    q.w = qbyte(iscale, x[12]) | (qbyte(iscale, x[13]) << 8) | (qbyte(iscale, x[14]) << 16) |
          (qbyte(iscale, x[15]) << 24);
    int bsum = sdot4(q.x, 0x01010101u, 0);
    bsum = sdot4(q.y, 0x01010101u, bsum);
    bsum = sdot4(q.z, 0x01010101u, bsum);
    bsum = sdot4(q.w, 0x01010101u, bsum);
    float d = 1.f / iscale;
    if (m == 0.f) {  // `if (!amax)`: d = 0, qs = 0 (bsums then 0)
        q = u32x4{0u, 0u, 0u, 0u};
        bsum = 0;
        d = 0.f;
    }
    *(u32x4 *)(qb + 16 + 16 * l) = q;
    if (AM) {
        const int bs = bsum + __builtin_amdgcn_update_dpp(bsum, bsum, 0xB1, 0xF, 0xF, false);  // lanes 2j, 2j+1
        if (!(l & 1)) {
            *(_Float16 *)(qb + 272 + l) = (_Float16)(bs & 63);
            *(_Float16 *)(qb + 288 + l) = (_Float16)(bs >> 6);
        }
    } else {
        *(int16_t *)(qb + 272 + 2 * l) = (int16_t)bsum;
    }
    if (l == 0) *(float *)qb = d;
}

// ---- one superblock on 32 or 64 lanes (kq_rows' prologue when the row leaves waves idle)
// Rows of 16 lanes exchanged by gfx950's lane swaps: v_permlane16_swap with both operands
// v leaves rows {0, 0, 2, 2} of v in one result and rows {1, 1, 3, 3} in the other, so one
// op of the two combines each row with its neighbour (xor 16) in every lane;
// v_permlane32_swap does the same with the wave's halves (xor 32).
__device__ __forceinline__ void swap_rows16(uint32_t v, uint32_t &a, uint32_t &b) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    a = r[0], b = r[1];
}
__device__ __forceinline__ void swap_rows32(uint32_t v, uint32_t &a, uint32_t &b) {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    a = r[0], b = r[1];
}
// Reduction over the LP (32, 64) lanes of a superblock: every lane ends with the result.
template <int LP, typename Op>
__device__ __forceinline__ int sblk_reduce(int v, Op op) {
    static_assert(LP == 32 || LP == 64, "lanes per superblock");
    v = row16_reduce(v, op);
    uint32_t a, b;
    swap_rows16((uint32_t)v, a, b);
    v = op((int)a, (int)b);
    if (LP == 64) {
        swap_rows32((uint32_t)v, a, b);
        v = op((int)a, (int)b);
    }
    return v;
}
// The same tree in double (xor 1, 2, 4, 8, 16[, 32]; addition is commutative, so every lane
// of the superblock ends with the same bits). Every lane of the wave must be active.
template <int LP>
__device__ __forceinline__ double sblk_sum(double v) {
    static_assert(LP == 32 || LP == 64, "lanes per superblock");
    v = row16_sum(v);
#pragma unroll
    for (int step = 0; step < (LP == 64 ? 2 : 1); ++step) {
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        uint32_t la, lb, ha, hb;
        if (step == 0) swap_rows16((uint32_t)u, la, lb), swap_rows16((uint32_t)(u >> 32), ha, hb);
        else swap_rows32((uint32_t)u, la, lb), swap_rows32((uint32_t)(u >> 32), ha, hb);
        v = __builtin_bit_cast(double, ((uint64_t)ha << 32) | la) + __builtin_bit_cast(double, ((uint64_t)hb << 32) | lb);
    }
    return v;
}

// The total of nb <= 64 doubles in LDS, nb a power of two, as a balanced tree (the norm
// prologue's superblock sums): lane l reads sums[l], then the xor tree over the nb lanes, by
// DPP within a row of 16 and the lane swaps across rows. Lanes from nb on hold +0.0 and add
// it to sums that are >= 0 or NaN, which changes no bit, so for nb < 16 the row's tree is the
// tree over the first nb lanes. Every lane of the wave must be active; returns lane 0's total
// (wave-uniform).
__device__ __forceinline__ double tree_sum_lanes(const double *sums, int nb, int lane) {
    double v = lane < nb ? sums[lane] : 0.0;
    v = row16_sum(v);
    if (nb > 16) {  // (uniform)
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        uint32_t la, lb, ha, hb;
        swap_rows16((uint32_t)u, la, lb), swap_rows16((uint32_t)(u >> 32), ha, hb);
        v = __builtin_bit_cast(double, ((uint64_t)ha << 32) | la) + __builtin_bit_cast(double, ((uint64_t)hb << 32) | lb);
    }
    if (nb > 32) {
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        uint32_t la, lb, ha, hb;
        swap_rows32((uint32_t)u, la, lb), swap_rows32((uint32_t)(u >> 32), ha, hb);
        v = __builtin_bit_cast(double, ((uint64_t)ha << 32) | la) + __builtin_bit_cast(double, ((uint64_t)hb << 32) | lb);
    }
    return readlane_f64(v, 0);
}

// quant16_store's quantizer with one superblock on LP = 32 or 64 lanes: lane l of the
// superblock owns the VP = 256 / LP consecutive values x[VP l .. VP l + VP). The same
// quantize_row_q8_K_ref semantics: the first-index scan of a +-amax tie orders the keys
// 2 (VP l + k) + sign over every lane of the superblock (across its 16-lane rows), bsums are
// the sums of 16 / VP neighbouring lanes. Every lane of the wave runs it (the reductions
// cross 16-lane rows); `st`: this lane's superblock lies in the row and is stored.
template <int LP>
__device__ __forceinline__ void quant_wide_store(const float *x, int l, uint8_t *qb, bool st) {
    constexpr int VP = 256 / LP;
    float mp = 0.f, mn = 0.f;
#pragma unroll
    for (int k = 0; k < VP; ++k) {
        mp = fmaxf(mp, x[k]);
        mn = fmaxf(mn, -x[k]);
    }
    const int mpb = sblk_reduce<LP>(__float_as_int(mp), [](int a, int c) { return a > c ? a : c; });
    const int mnb = sblk_reduce<LP>(__float_as_int(mn), [](int a, int c) { return a > c ? a : c; });
    const float m = __int_as_float(mpb > mnb ? mpb : mnb);
    bool neg = mnb > mpb;
    if (__any(mpb == mnb && mpb != 0)) {  // a tie somewhere in the wave (wave-uniform: the swaps need every lane)
        uint32_t key = 0xffffffffu;
#pragma unroll
        for (int k = VP - 1; k >= 0; --k)
            if (fabsf(x[k]) == m) key = 2u * (uint32_t)(VP * l + k) + (x[k] < 0.f ? 1u : 0u);
        key = (uint32_t)sblk_reduce<LP>((int)key, [](int a, int c) { return (uint32_t)a < (uint32_t)c ? a : c; });
        if (mpb == mnb && mpb != 0) neg = (key & 1u) != 0;
    }
    const float maxv = neg ? -m : m;
    const float iscale = -127.f / maxv;
    uint32_t q[VP / 4];
    int bsum = 0;
#pragma unroll
    for (int k = 0; k < VP / 4; ++k) {
        q[k] = qbyte(iscale, x[4 * k]) | (qbyte(iscale, x[4 * k + 1]) << 8) | (qbyte(iscale, x[4 * k + 2]) << 16) |
               (qbyte(iscale, x[4 * k + 3]) << 24);
        bsum = sdot4(q[k], 0x01010101u, bsum);
    }
    float d = 1.f / iscale;
    if (m == 0.f) {  // `if (!amax)`: d = 0, qs = 0 (bsums then 0)
#pragma unroll
        for (int k = 0; k < VP / 4; ++k) q[k] = 0u;
        bsum = 0;
        d = 0.f;
    }
    // 16 values = 16 / VP neighbouring lanes (exact integer adds)
    bsum += __builtin_amdgcn_update_dpp(bsum, bsum, 0xB1, 0xF, 0xF, false);
    if (VP == 4) bsum += __builtin_amdgcn_update_dpp(bsum, bsum, 0x4E, 0xF, 0xF, false);
    if (st) {
        if (VP == 8) *(uint2 *)(qb + 16 + 8 * l) = make_uint2(q[0], q[VP / 4 - 1]);
        else *(uint32_t *)(qb + 16 + 4 * l) = q[0];
        if (!(l & (16 / VP - 1))) *(int16_t *)(qb + 272 + 2 * (l / (16 / VP))) = (int16_t)bsum;
        if (l == 0) *(float *)qb = d;
    }
}

__device__ __forceinline__ uint32_t gload4_asm(const float *p) {
    uint32_t r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}

// Fused-prologue transforms of 4 activation values held as f32 bits (kq_ops_device.h):
// ggml_vec_swiglu_f32 (silu(g) * u) and rms_norm + MUL ((x * scale) * w).
__device__ __forceinline__ u32x4 swiglu4(u32x4 g, u32x4 u) {
    u32x4 r;
    r.x = __float_as_uint(v_silu(__uint_as_float(g.x)) * __uint_as_float(u.x));
    r.y = __float_as_uint(v_silu(__uint_as_float(g.y)) * __uint_as_float(u.y));
    r.z = __float_as_uint(v_silu(__uint_as_float(g.z)) * __uint_as_float(u.z));
    r.w = __float_as_uint(v_silu(__uint_as_float(g.w)) * __uint_as_float(u.w));
    return r;
}

__device__ __forceinline__ u32x4 normmul4(u32x4 x, u32x4 w, float scale) {
    u32x4 r;
    r.x = __float_as_uint((__uint_as_float(x.x) * scale) * __uint_as_float(w.x));
    r.y = __float_as_uint((__uint_as_float(x.y) * scale) * __uint_as_float(w.y));
    r.z = __float_as_uint((__uint_as_float(x.z) * scale) * __uint_as_float(w.z));
    r.w = __float_as_uint((__uint_as_float(x.w) * scale) * __uint_as_float(w.w));
    return r;
}

__device__ __forceinline__ u32x4 gload16_asm(const float *p) {
    u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}

// The same load into a register that already holds a value (tied in/out): on a path that skips
// the load the register keeps that value, so no copy joins the two paths while the load is in
// flight (with a fresh "=v" destination the compiler placed such copies behind the load).
__device__ __forceinline__ void gload16_into(u32x4 &r, const float *p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(r) : "v"(p) : "memory");
}

// ---------------------------------------------------------------- per-type quad partials
// Lane s (0..3) of a quad covers 64 quants of the superblock at `blk` (LDS) against
// the Q8L activation block `ab`. Every sum is an exact int32; the pairings below
// only re-associate integer additions of lane_q4K/q5K/q6K (kq_device.h).
__device__ __forceinline__ int dotacc(u32x4 q, u32x4 a, int acc) {
    acc = sdot4(q.x, a.x, acc);
    acc = sdot4(q.y, a.y, acc);
    acc = sdot4(q.z, a.z, acc);
    return sdot4(q.w, a.w, acc);
}

struct QuadOut {
    int isum, imin;
    uint32_t dh;  // Q4_K/Q5_K: d | dmin << 16 ; Q6_K: d
};

// Q4_K: s <-> sub-blocks 2s (low nibbles) / 2s+1 (high), qs[32s, 32s+32).
__device__ __forceinline__ QuadOut quad_q4K(const uint8_t *blk, const uint8_t *ab, int s) {
    const u32x4 hdr = *(const u32x4 *)blk;
    const u32x4 q0 = *(const u32x4 *)(blk + 16 + 32 * s);
    const u32x4 q1 = *(const u32x4 *)(blk + 32 + 32 * s);
    const uint8_t *aq = ab + 16 + 64 * s;
    const u32x4 a0 = *(const u32x4 *)(aq), a1 = *(const u32x4 *)(aq + 16);
    const u32x4 a2 = *(const u32x4 *)(aq + 32), a3 = *(const u32x4 *)(aq + 48);
    const ScMn s0 = scales_k4(hdr, 2 * s), s1 = scales_k4(hdr, 2 * s + 1);
    const int dlo = dotacc(q1 & 0x0f0f0f0fu, a1, dotacc(q0 & 0x0f0f0f0fu, a0, 0));
    const int dhi = dotacc((q1 >> 4) & 0x0f0f0f0fu, a3, dotacc((q0 >> 4) & 0x0f0f0f0fu, a2, 0));
    const uint2 bs = *(const uint2 *)(ab + 272 + 8 * s);
    QuadOut r;
    r.isum = __mul24(dlo, s0.sc_lo) + __mul24(dhi, s0.sc_hi);  // |dot| < 2^17: full-rate i24
    r.imin = ((int)(int16_t)(bs.x & 0xffffu) + (int)(int16_t)(bs.x >> 16)) * s0.mn +
             ((int)(int16_t)(bs.y & 0xffffu) + (int)(int16_t)(bs.y >> 16)) * s1.mn;
    r.dh = hdr.x;
    return r;
}

// Q5_K: as Q4_K plus the 5th bit from qh (bit 2s for low nibbles, 2s+1 for high).
__device__ __forceinline__ QuadOut quad_q5K(const uint8_t *blk, const uint8_t *ab, int s) {
    const u32x4 hdr = *(const u32x4 *)blk;
    const u32x4 h0 = *(const u32x4 *)(blk + 16), h1 = *(const u32x4 *)(blk + 32);
    const u32x4 q0 = *(const u32x4 *)(blk + 48 + 32 * s);
    const u32x4 q1 = *(const u32x4 *)(blk + 64 + 32 * s);
    const uint8_t *aq = ab + 16 + 64 * s;
    const u32x4 a0 = *(const u32x4 *)(aq), a1 = *(const u32x4 *)(aq + 16);
    const u32x4 a2 = *(const u32x4 *)(aq + 32), a3 = *(const u32x4 *)(aq + 48);
    const ScMn s0 = scales_k4(hdr, 2 * s), s1 = scales_k4(hdr, 2 * s + 1);
    const uint32_t sl = (uint32_t)(2 * s), shh = (uint32_t)(2 * s + 1);
    const u32x4 lo0 = (q0 & 0x0f0f0f0fu) | (((h0 >> sl) & 0x01010101u) << 4);
    const u32x4 hi0 = ((q0 >> 4) & 0x0f0f0f0fu) | (((h0 >> shh) & 0x01010101u) << 4);
    const u32x4 lo1 = (q1 & 0x0f0f0f0fu) | (((h1 >> sl) & 0x01010101u) << 4);
    const u32x4 hi1 = ((q1 >> 4) & 0x0f0f0f0fu) | (((h1 >> shh) & 0x01010101u) << 4);
    const int dlo = dotacc(lo1, a1, dotacc(lo0, a0, 0));
    const int dhi = dotacc(hi1, a3, dotacc(hi0, a2, 0));
    const uint2 bs = *(const uint2 *)(ab + 272 + 8 * s);
    QuadOut r;
    r.isum = __mul24(dlo, s0.sc_lo) + __mul24(dhi, s0.sc_hi);  // |dot| < 2^17: full-rate i24
    r.imin = ((int)(int16_t)(bs.x & 0xffffu) + (int)(int16_t)(bs.x >> 16)) * s0.mn +
             ((int)(int16_t)(bs.y & 0xffffu) + (int)(int16_t)(bs.y >> 16)) * s1.mn;
    r.dh = hdr.x;
    return r;
}

// Q6_K (210 B, any byte alignment in LDS: 4-aligned dword reads + alignbyte):
// s <-> ql[32s, 32s+32), qh[128 + 32(s>>1), +32), qh bit pair 2(s&1) / +4.
__device__ __forceinline__ QuadOut quad_q6K(const uint8_t *blk, const uint8_t *ab, int s) {
    const uint32_t s4 = (uint32_t)((uintptr_t)blk & 3u);
    const uint8_t *b = blk - s4;
    const int n = s >> 1, part2 = s & 1;
    const u32x4 L0 = realign(*(const u32x4a *)(b + 32 * s), *(const uint32_t *)(b + 32 * s + 16), s4);
    const u32x4 L1 = realign(*(const u32x4a *)(b + 32 * s + 16), *(const uint32_t *)(b + 32 * s + 32), s4);
    const u32x4 H0 = realign(*(const u32x4a *)(b + 128 + 32 * n), *(const uint32_t *)(b + 144 + 32 * n), s4);
    const u32x4 H1 = realign(*(const u32x4a *)(b + 144 + 32 * n), *(const uint32_t *)(b + 160 + 32 * n), s4);
    const uint32_t w208 = *(const uint32_t *)(b + 208);
    const u32x4 SC = realign(*(const u32x4a *)(b + 192), w208, s4);
    const uint32_t shl = (uint32_t)part2 * 2u;
    const u32x4 ql0 = (L0 & 0x0f0f0f0fu) | (((H0 >> shl) & 0x03030303u) << 4);
    const u32x4 qh0 = ((L0 >> 4) & 0x0f0f0f0fu) | (((H0 >> (shl + 4u)) & 0x03030303u) << 4);
    const u32x4 ql1 = (L1 & 0x0f0f0f0fu) | (((H1 >> shl) & 0x03030303u) << 4);
    const u32x4 qh1 = ((L1 >> 4) & 0x0f0f0f0fu) | (((H1 >> (shl + 4u)) & 0x03030303u) << 4);
    const int elo = 128 * n + 32 * part2;  // elements of ql0's low nibbles; ql1: +16
    const uint8_t *aq = ab + 16 + elo;
    const int sb = elo >> 4;
    const int d00 = dotacc(ql0, *(const u32x4 *)(aq), 0);
    const int d01 = dotacc(qh0, *(const u32x4 *)(aq + 64), 0);
    const int d10 = dotacc(ql1, *(const u32x4 *)(aq + 16), 0);
    const int d11 = dotacc(qh1, *(const u32x4 *)(aq + 80), 0);
    QuadOut r;
    r.isum = __mul24(d00, sbyte(SC, sb)) + __mul24(d01, sbyte(SC, sb + 4)) + __mul24(d10, sbyte(SC, sb + 1)) +
             __mul24(d11, sbyte(SC, sb + 5));  // |dot| < 2^17: full-rate i24
    const uint2 bs = *(const uint2 *)(ab + 272 + 8 * s);
    r.imin = (int)(int16_t)(bs.x & 0xffffu) * sbyte(SC, 4 * s) + (int)(int16_t)(bs.x >> 16) * sbyte(SC, 4 * s + 1) +
             (int)(int16_t)(bs.y & 0xffffu) * sbyte(SC, 4 * s + 2) + (int)(int16_t)(bs.y >> 16) * sbyte(SC, 4 * s + 3);
    r.dh = (w208 >> (8u * s4)) & 0xffffu;
    return r;
}

__device__ __forceinline__ int quad_sum(int v) {
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    return v;
}

// ---------------------------------------------------------------- kq_rows' records and chain
// kq_rows keeps its records in LDS, written by the quad leaders and replayed by lane r for row r
// (kq_rows.hip). The leader stores what the chain consumes, as floats (RowRec), so the
// conversions leave the serial chain for the leaders, where 16 of them run at once
// (profiles/r12_chain_ab.txt). The same instruction on the same operand gives the same bits in
// either place.
//
// 16 B as Rec, so the LDS layouts stand. Q4_K: a = (float)sumi, c = y.d * d, b = (float)summins,
// e = y.d * dmin; Q5_K: a = the superblock's whole term (it does not depend on the running sum);
// Q6_K: a = (float)(isum - 32 * isum_mins), c = d_all * y.d. Fields a type does not use are
// neither stored nor read.
struct RowRec {
    float a, c, b, e;
};
static_assert(sizeof(RowRec) == sizeof(Rec), "the record layouts of rows_layout / rows_dyn_layout");

// The leader's record of one superblock, stored at `p` (LDS). dh: QuadOut's.
template <int TYPE>
__device__ __forceinline__ void row_rec_store(RowRec *p, int isum, int imin, uint32_t dh, float yd) {
    if (TYPE == Q6_K) {
        const float a = (float)(isum - 32 * imin), c = h2f(dh) * yd;  // d_all * y.d
        *(float2 *)p = make_float2(a, c);
    } else {
        const float c = yd * h2f(dh & 0xffffu);  // y.d * fp16(x.d)
        const float e = yd * h2f(dh >> 16);      // y.d * fp16(x.dmin)
        if (TYPE == Q5_K) p->a = fmaf(c, (float)isum, -(e * (float)imin));  // d*sumi - dmin*sumi_mins
        else *(float4 *)p = make_float4((float)isum, c, (float)imin, e);
    }
}

// One record into registers: one LDS read instruction.
template <int TYPE>
__device__ __forceinline__ RowRec row_rec_load(const RowRec *p) {
    RowRec r = {0.f, 0.f, 0.f, 0.f};
    if (TYPE == Q5_K) {
        r.a = p->a;
    } else if (TYPE == Q6_K) {
        const float2 v = *(const float2 *)p;
        r.a = v.x, r.c = v.y;
    } else {
        const float4 v = *(const float4 *)p;
        r.a = v.x, r.c = v.y, r.b = v.z, r.e = v.w;
    }
    return r;
}

// The reference's per-superblock fp32 update on such a record: its dependent
// operations and nothing else. The Q4_K negation is of the float (an operand modifier of the
// FMA), never of the integer: INT_MIN and the sign of a zero product would differ.
template <int TYPE>
__device__ __forceinline__ float row_chain_step(const RowRec &r, float s) {
    if (TYPE == Q4_K) {
        s = fmaf(-r.b, r.e, s);  // sumf -= dmin * summins   (fmsub, README.md:551)
        s = fmaf(r.a, r.c, s);   // sumf += d * sumi         (fmadd, README.md:614)
    } else if (TYPE == Q5_K) {
        s = s + r.a;
    } else {  // Q6_K: sum += d_all*y.d*(isum - 32*isum_mins)
        s = fmaf(r.c, r.a, s);
    }
    return s;
}

// Row r's chain, in lane r: records rc[0], rc[stride], .. rc[(nb - 1) * stride] in superblock
// order from s = 0 (the three chain sites of kq_rows.hip). Four records are read at a time.
// Holding a group of 4 or 8 records in registers behind one wait, the next group in flight under
// its FMAs, measured slower on the token than this loop (profiles/r12_chain_ab.txt) and is not
// in the source.
template <int TYPE>
__device__ __forceinline__ float rows_chain(const RowRec *rc, int nb, int stride) {
    float s = 0.f;
#pragma unroll 4
    for (int i = 0; i < nb; ++i) s = row_chain_step<TYPE>(row_rec_load<TYPE>(rc + i * stride), s);
    return s;
}

// One superblock of the stream on its quad: the four lanes' dot products of the weight block at
// `blk` (LDS, the ring) with the activation's Q8L block at `ab`, summed over the quad, and the
// leader's record at `rec`. s: the lane within the quad. The one copy of the step that the short
// form, the generic loop and kq_rows_dyn's loop run.
template <int TYPE>
__device__ __forceinline__ void rows_quad_step(const uint8_t *blk, const uint8_t *ab, int s, RowRec *rec) {
    const QuadOut r = TYPE == Q4_K ? quad_q4K(blk, ab, s) : TYPE == Q5_K ? quad_q5K(blk, ab, s) : quad_q6K(blk, ab, s);
    const int isum = quad_sum(r.isum);
    const int imin = quad_sum(r.imin);
    if (s == 0) {
        const float yd = *(const float *)ab;
        row_rec_store<TYPE>(rec, isum, imin, r.dh, yd);
    }
}

// ---------------------------------------------------------------- the row stream of one wave
struct WaveWork {
    int m, r0, nrows;
};

// s_waitcnt vmcnt(N * k) for runtime k in [0, 3] (tail of the stream).
template <int N>
__device__ __forceinline__ void vm_wait_k(int k) {
    if (k >= 3) vm_wait<3 * N>();
    else if (k == 2) vm_wait<2 * N>();
    else if (k == 1) vm_wait<N>();
    else vm_wait<0>();
}

// One step's DMA instructions (rows_ni of 64 granules, the last one partial) from `base`, this
// lane's first granule of the step, into the ring slot at `slot`. interior: every granule lies
// inside the stream; else each is clamped to the stream's last granule `last16`.
template <int TYPE>
__device__ __forceinline__ void rows_issue_step(const uint8_t *base, const uint8_t *last16, uint8_t *slot, int lane,
                                                bool interior) {
    constexpr int NI = rows_ni(TYPE), PART = rows_gran(TYPE) - 64 * (NI - 1);  // lanes of the partial instruction
    if (interior) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (i + 1 < NI || lane < PART) dma16_nt(base + 1024 * i, (LDS void *)(slot + 1024 * i));
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const uint8_t *p = base + 1024 * i;
            if (i + 1 < NI || lane < PART) dma16_nt(p < last16 ? p : last16, (LDS void *)(slot + 1024 * i));
        }
    }
}

}  // namespace kq
