// kq_q3k_device.h — device helpers of the Q3_K kernels (kq_q3k.hip): a lane's share of one
// block_q3_K read from an LDS slot at any even offset, its 3-bit values assembled four to a
// dword, its four 6-bit scales, and the lane's integer dot against one Q8L activation block.
#pragma once

#include "kq_device.h"

namespace kq {

// block_q3_K: hmask[32] @0, qs[64] @32, scales[12] @96, d (f16) @108.
// Element e = 128n + 32j + l: low two bits (qs[32n + l] >> 2j) & 3, third bit (hmask[l] >> (4n + j)) & 1,
// q = low - (third ? 0 : 4). Lane p of the block's octet owns l in [l0, l0 + 8), l0 = 8 (p & 3), of
// half n = p >> 2: one 8-element piece per j, each inside one 16-element scale group
// is = 8n + 2j + (l0 >> 4).
struct Q3Lane {
    uint32_t q[4][2];  // piece j: eight int8 values q in [-4, 3]
    int sc[4];         // piece j: its group's scale in [-32, 31]
    uint32_t dh;       // the block's d (f16 bits)
};

// Dwords [0, N) of the N * 4 bytes at slot + off (off even; the slot 4-byte aligned): aligned
// LDS reads of N + 1 dwords, shifted into place.
template <int N>
__device__ __forceinline__ void q3k_read(const uint8_t *slot, uint32_t off, uint32_t (&out)[N]) {
    const uint32_t s = off & 3u;
    const uint32_t *b = (const uint32_t *)(slot + (off & ~3u));
    uint32_t w[N + 1];
#pragma unroll
    for (int i = 0; i <= N; ++i) w[i] = b[i];
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], s);
}

// scales[12] as three dwords S -> the scale of group is (ggml's kmask1 / kmask2 shuffle, per index)
__device__ __forceinline__ int q3k_scale(const uint32_t (&S)[3], int is) {
    const uint32_t b = ((is & 4) ? S[1] : S[0]) >> (8u * (uint32_t)(is & 3));
    const uint32_t lo4 = is < 8 ? (b & 15u) : ((b >> 4) & 15u);
    const uint32_t hi2 = (S[2] >> (8u * (uint32_t)(is & 3) + 2u * (uint32_t)(is >> 2))) & 3u;
    return (int)(lo4 | (hi2 << 4)) - 32;
}

// boff: the block's byte offset in the slot (even). Reads stay inside [boff & ~3, boff + 112).
__device__ __forceinline__ Q3Lane q3k_unpack(const uint8_t *slot, uint32_t boff, int p) {
    const int n = p >> 2, l0 = 8 * (p & 3);
    uint32_t hm[2], qs[2], S[3];
    q3k_read<2>(slot, boff + (uint32_t)l0, hm);
    q3k_read<2>(slot, boff + 32u + 32u * (uint32_t)n + (uint32_t)l0, qs);
    q3k_read<3>(slot, boff + 96u, S);
    Q3Lane r;
    const uint32_t doff = boff + 108u;
    r.dh = (*(const uint32_t *)(slot + (doff & ~3u)) >> (8u * (doff & 3u))) & 0xffffu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t hs = (uint32_t)(4 * n + j);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // u = q + 4 in [0, 7] per byte; (u | 0x80) - 4 borrows nothing across bytes
            const uint32_t u = ((qs[h] >> (2u * j)) & 0x03030303u) | (((hm[h] >> hs) & 0x01010101u) << 2);
            r.q[j][h] = ((u | 0x80808080u) - 0x04040404u) ^ 0x80808080u;
        }
        r.sc[j] = q3k_scale(S, 8 * n + 2 * j + (l0 >> 4));
    }
    return r;
}

// The lane's share of isum against the Q8L block ab (d @0, qs @16): two dot4 per piece.
__device__ __forceinline__ int q3k_dot(const Q3Lane &w, const uint8_t *ab, int p) {
    const int n = p >> 2, l0 = 8 * (p & 3);
    const uint8_t *aq = ab + 16 + 128 * n + l0;
    int isum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint2 y = *(const uint2 *)(aq + 32 * j);
        isum += sdot4(w.q[j][1], y.y, sdot4(w.q[j][0], y.x, 0)) * w.sc[j];  // |dot| <= 8 * 4 * 128
    }
    return isum;
}

}  // namespace kq
