// kq_attn_mfma.hip — prompt attention on the gfx950 f16 matrix cores under a stated tolerance
// (mi355x_attn_prompt_precision(MI355X_ATTN_PROMPT_F16); the default, EXACT, runs kq_ops.hip's
// kernels and gives the decode token's bits). The attention counterpart of kq_mmf.
//
// The rule (restated for the tests in tests/attn_f16_ref.py):
//   The operands are the exact path's: kq_kv_store is unchanged, so both caches hold the same
//   bits; the query operand is q^ = f16(rope(q)), the same f32 rope and RNE conversion.
//   For token i at position p (0 <= p < n_ctx), head h, kv head g = h / gsz, in exact arithmetic
//     s_c = scale * sum_d q^_d K[c][g][d]  (c <= p),  m = max s_c,  w_c = exp(s_c - m),
//     l = sum w_c,  emu_d = sum_c w_c V[g][d][c] / l.
//   Cells c > p contribute nothing whatever finite bits they hold; a token outside the cache
//   writes no cell and gets a NaN row. The kernel's output is within, per element,
//     D   = 2^-23 HD scale max_c sum_d |q^_d K_cd|
//     eps = 2^-10 + 4 D
//     B_d = eps sum_c w_c |V_dc| / l + 2^-24 sum_{c<=p} |V_dc| / l
//           + 2^-24 (ceil(n/32) + 32) sum_c w_c |V_dc| / l,   n = p + 1
//   of emu_d (DESIGN.md §4 derives it). What the kernel does to stay inside:
//     the dot accumulates in f32 (v_mfma_f32_32x32x16_f16), scaled after the sum;
//     online soft_max over 32-cell tiles: the running maximum m is updated BEFORE the tile's
//     weights are formed, so every p = exp(s - m) is in [0, 1]; O and l are rescaled by
//     exp(m_old - m_new) at every tile (no deferred rescale); masking is a select to -inf on the
//     score; a row whose cells are all masked so far uses 0 as its maximum (p = 0, no inf - inf);
//     p is rounded to f16 once (RNE) for the second product, l sums the unrounded p in f32;
//     O accumulates in f32 (MFMA), divided by l once at the end.
//
// Structure: a wave owns 32 queries (a tile of the batch, in batch order) of one head; a
// workgroup's 4 waves take 4 consecutive heads (one kv group's where gsz % 4 == 0: their K / V
// reads hit the same lines in L1 / L2). No LDS, no barrier, no workspace: nothing grows with n_ctx.
//   S^T = K Q^^T: A = 16-B pieces of K-cache rows (lane (r, hf): cell c0 + r, elements
//     16 ks + 8 hf ..), B = q^ (lane: query r, the same elements), roped and converted once per
//     tile and kept in registers. Result: the query on the lane (column), the tile's 32 cells in
//     the 16 registers x 2 lane halves: register i of half hf is cell (i & 3) + 8 (i >> 2) + 4 hf.
//     Max and sum per query: 15 register ops and one exchange with lane ^ 32.
//   O^T = V^T P^T: B = the accumulator registers 8 s .. 8 s + 7 as f16 (k-step s), whose k order
//     is 16 s + 8 (j >> 2) + 4 hf + (j & 3); A = the transposed V cache [kvw][n_ctx] read in that
//     same order: two 8-byte runs of 4 consecutive cells per (channel, k-step). Result: channel
//     (i & 3) + 8 (i >> 2) + 4 hf of the 32-channel block in register i, the query on the lane:
//     the rescale and the final divide are per lane, the stores are 16-byte runs of 4 channels.
//   The next tile's K and V fragments are requested before the current tile's products.
// The tile's cell loop runs to the largest valid position of its 32 tokens + 1, rounded up to 32
// (<= n_ctx: n_ctx % 32 == 0); tokens may come in any order. Lanes past n_tokens read no q / pos
// and store nothing.
#include <math.h>

#include "kq_common.h"
#include "kq_internal.h"
#include "kq_device.h"
#include "kq_ops_device.h"

namespace kq {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int F16_QT = 32;     // queries per wave
constexpr int F16_CT = 32;     // cells per tile
constexpr int F16_WAVES = 4;   // heads per workgroup

// exp(x) for x <= 0 (and -inf -> 0): v_exp_f32 of x log2(e); x <= 0 keeps the result <= 1
__device__ __forceinline__ float exp_le0(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

template <int HD>
struct KvFrag {
    u32x4 k[HD / 16];      // A of S^T: cell c0 + r, elements 16 ks + 8 hf .. + 8
    u32x2 v[HD / 32][4];   // A of O^T: channel 32 db + r, cells c0 + 16 s + 8 u + 4 hf .. + 4 at [db][2 s + u]
};

template <int HD>
__device__ __forceinline__ void load_kv(KvFrag<HD> &f, const uint16_t *kp, const uint16_t *vp, int64_t kvw, int64_t nc,
                                        int c0) {
#pragma unroll
    for (int ks = 0; ks < HD / 16; ++ks) f.k[ks] = *(const u32x4 *)(kp + (int64_t)c0 * kvw + 16 * ks);
#pragma unroll
    for (int db = 0; db < HD / 32; ++db)
#pragma unroll
        for (int su = 0; su < 4; ++su) f.v[db][su] = *(const u32x2 *)(vp + (int64_t)db * 32 * nc + c0 + 8 * su);
}

}  // namespace

template <int HD>
__global__ void __launch_bounds__(64 * F16_WAVES) kq_attn_prompt_f16(const AttnArgs a) {
    constexpr int KS = HD / 16;  // k-steps of S^T
    constexpr int DB = HD / 32;  // 32-channel blocks of O^T
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, hf = lane >> 5;
    const int h = (int)blockIdx.x * F16_WAVES + wave;
    if (h >= a.n_head) return;  // (no barrier in this kernel)
    const int g = h / (a.n_head / a.n_head_kv);
    const int i = ((int)gridDim.y - 1 - (int)blockIdx.y) * F16_QT + r;  // latest tiles first: the most cells
    const bool live = i < a.n_tok;
    const int pos_in = live ? a.pos[i] : -1;
    const bool ok = pos_in >= 0 && pos_in < a.n_ctx;
    const int pos = ok ? pos_in : -1;  // -1: every cell masked
    int pmax = pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(pmax, o, 64);
        pmax = other > pmax ? other : pmax;
    }
    const int n_kv = __builtin_amdgcn_readfirstlane((pmax + F16_CT) / F16_CT * F16_CT);  // <= n_ctx; 0: no valid token
    const int64_t kvw = (int64_t)a.n_head_kv * HD, nc = a.n_ctx;

    // q^ = f16(rope(q)) of query r, elements 16 ks + 8 hf .. + 8 (4 rope pairs) per k-step
    f16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (h16)0.0f;
    if (ok) {
        const float *qp = a.q + (int64_t)i * a.n_head * HD + (int64_t)h * HD + 8 * hf;
        const float *tc = a.rope_table + (int64_t)pos * HD + 8 * hf;  // [pos][HD/2][cos, sin]
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4a x0 = *(const f32x4a *)(qp + 16 * ks), x1 = *(const f32x4a *)(qp + 16 * ks + 4);
            const f32x4a c0 = *(const f32x4a *)(tc + 16 * ks), c1 = *(const f32x4a *)(tc + 16 * ks + 4);
            const float2 r0 = rope_pair(x0.x, x0.y, c0.x, c0.y), r1 = rope_pair(x0.z, x0.w, c0.z, c0.w);
            const float2 r2 = rope_pair(x1.x, x1.y, c1.x, c1.y), r3 = rope_pair(x1.z, x1.w, c1.z, c1.w);
            qf[ks][0] = f2h_rne(r0.x), qf[ks][1] = f2h_rne(r0.y), qf[ks][2] = f2h_rne(r1.x), qf[ks][3] = f2h_rne(r1.y);
            qf[ks][4] = f2h_rne(r2.x), qf[ks][5] = f2h_rne(r2.y), qf[ks][6] = f2h_rne(r3.x), qf[ks][7] = f2h_rne(r3.y);
        }
    }

    const uint16_t *kp = a.k_cache + (int64_t)r * kvw + (int64_t)g * HD + 8 * hf;
    const uint16_t *vp = a.v_cache + ((int64_t)g * HD + r) * nc + 4 * hf;
    f32x16 o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] = 0.0f;
    float m = -INFINITY, l = 0.0f;  // the running maximum (both halves agree) and this half's sum
    KvFrag<HD> cur, nxt;
    load_kv<HD>(cur, kp, vp, kvw, nc, 0);  // cells [0, 32): inside every cache
    for (int c0 = 0; c0 < n_kv; c0 += F16_CT) {
        // the next tile's fragments (the last tile requests itself again: always inside [0, n_kv))
        load_kv<HD>(nxt, kp, vp, kvw, nc, c0 + F16_CT < n_kv ? c0 + F16_CT : c0);
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            s = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, cur.k[ks]), qf[ks], s, 0, 0, 0);
        float tm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int c = c0 + (e & 3) + 8 * (e >> 2) + 4 * hf;
            s[e] = c <= pos ? s[e] * a.scale : -INFINITY;  // a select, never an add
            tm = fmaxf(tm, s[e]);
        }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);
        const float mu = mn == -INFINITY ? 0.0f : mn;  // all masked so far: p = exp(-inf - 0) = 0
        const float alpha = exp_le0(m - mu);           // m = -inf: 0 (O and l are 0 then)
        m = mn;
        float ps = 0.0f;
        f16x8 pf[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = exp_le0(s[e] - mu);  // in [0, 1]
            ps += p;
            pf[e >> 3][e & 7] = (h16)p;  // RNE
        }
        l = l * alpha + ps;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const u32x4 vv = {cur.v[db][2 * st].x, cur.v[db][2 * st].y, cur.v[db][2 * st + 1].x, cur.v[db][2 * st + 1].y};
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vv), pf[st], o[db], 0, 0, 0);
            }
        }
        cur = nxt;
    }
    l += __shfl_xor(l, 32, 64);
    if (!live) return;
    const float inv = 1.0f / l;
    float *op = a.out + (int64_t)i * a.n_head * HD + (int64_t)h * HD + 4 * hf;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            f32x4a y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = ok ? o[db][4 * q4 + e] * inv : __builtin_nanf("");
            *(f32x4a *)(op + 32 * db + 8 * q4) = y;
        }
}

// kq_kv_store has run (or the k / v GEMM's epilogue stored the cells): the attention alone
int launch_attn_prompt_f16(const AttnArgs &a0, int n_tok, hipStream_t s) {
    AttnArgs a = a0;
    a.n_tok = n_tok;
    const dim3 grid((unsigned)((a.n_head + F16_WAVES - 1) / F16_WAVES), (unsigned)((n_tok + F16_QT - 1) / F16_QT));
    if (grid.y > 65535u) return MI355X_E_UNSUPPORTED;
    return a.head_dim == 64
               ? timed_launch("kq::kq_attn_prompt_f16<64>", 0.0, kq_attn_prompt_f16<64>, grid, dim3(64 * F16_WAVES), 0, s, a)
               : timed_launch("kq::kq_attn_prompt_f16<128>", 0.0, kq_attn_prompt_f16<128>, grid, dim3(64 * F16_WAVES), 0, s,
                              a);
}

}  // namespace kq
