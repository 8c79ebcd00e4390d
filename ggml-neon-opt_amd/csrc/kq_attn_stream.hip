// kq_attn_stream.hip — streamed attention: caches of up to 131072 cells (mi355x_attn_stream).
//
// Every other attention kernel of the library sizes its LDS (scores, p16, group sums, V rows) or
// a register array by n_ctx, which stops them near 8192 cells. Here nothing on the chip grows
// with the cache: scores, exps and p16 live in a global workspace (6 bytes per (token, head,
// cell): f32 [n_tok][n_head][n_ctx], then f16 of the same shape) and the V rows pass through a
// fixed LDS ring. Three launches per token tile, the token index in the grid (one token: the
// decode step; T tokens: a prompt tile, after kq_kv_store):
//  A kq_attn_stream_scores: workgroup (64-cell chunk, kv group, token): kq_attn_cells' job
//    (kq_attn_decode.hip) — rope(q) of the group's heads, for the decode step rope(k) / f16(v) into both
//    caches by the workgroup whose chunk holds the position, vec_dot_f16 * scale per (head, cell
//    <= pos), -INF past pos — for caches that are a multiple of 32 cells (the last chunk may
//    hold 32) and any token of a tile.
//  B kq_attn_stream_softmax: workgroup (head, token), three passes over the head's row of the
//    workspace: the max; e = v_expf(x - max) (masked cells exact zeros) written back in place
//    with the (e0 + e1) + (e2 + e3) group sums accumulated (SumExact); the double total by the
//    tree where sum_exact_ok proves it equal to ggml's in-order sum, else the in-order sum over
//    all groups, recomputed from the stored exps by one wave; p = f16(e * (float)(1 / sum)).
//  C kq_attn_stream_kqv: workgroup (head, slice of 16 outputs, token), 16 threads per output as
//    kq_attn_cells_kqv. Each wave owns 4 outputs: its 4 V rows and the head's p16 arrive in
//    512-cell chunks through the wave's own LDS ring (STREAM_DEPTH stages, LDS-DMA, counted
//    vmcnt waits: no workgroup barrier inside the loop), and every thread carries its one
//    pk_fma chain across the chunks in 32-cell iteration order; the quad reduce follows.
// The arithmetic is the other kernels', op for op and in their order, so every output bit is
// theirs. Loops run to the n_kv / n_it of the device-read position, never to n_ctx. A position
// outside [0, n_ctx) gives a NaN row and leaves the caches untouched. Every cache and workspace
// offset is 64-bit (a V row of kvw * n_ctx f16 passes 2^31 bytes' neighbourhood at 131072 cells).
//
// The batch form (STREAM_BATCH: mi355x_attn_batch / ATTN_BATCH under mi355x_attn_stream, after
// kq_kv_store_batch of kq_attn_batch.hip) runs the same three bodies per token tile with the
// row taken from the descriptor: cells [0, n_kv), workspace rows of n_kv entries, the score
// dot * scale + mask[token][cell] (kq_attn_batch's), the position selecting the rope row only.
// A 64-cell chunk without a visible cell (mask != -INF) loads no K row; the workgroups of KV
// group 0 leave one flag byte per (token, 32-cell block) behind the p16 rows, from which every
// wave of launch C lists the 512-cell stages that hold a visible cell and runs its ring over
// those alone. A skipped stage adds v * (+0) to every lane, which changes nothing but the sign
// of a zero (the header of kq_attn_batch.hip): a wave with a lane that ends as -0 runs every
// stage again. A token without a cell (kq_kv_store_batch's test) gets a NaN row.
#include <math.h>
#include <stdint.h>

#include <atomic>

#include <hip/hip_ext.h>

#include "kq_common.h"
#include "kq_internal.h"
#include "kq_device.h"
#include "kq_ops_device.h"
#include "kq_attn_head.h"

namespace kq {

constexpr int STREAM_CHUNK = 64;     // A: cells per workgroup
constexpr int STREAM_SM_NT = 1024;   // B: threads per workgroup
constexpr int STREAM_CELLS = 512;    // C: cells per ring stage (one 1-KiB LDS-DMA per V row)
constexpr int STREAM_DEPTH = 3;      // C: ring stages per wave (DEPTH - 1 chunks in flight under the one computed)
constexpr int STREAM_VROW = 2 * STREAM_CELLS + 64;                  // C: a staged V row (rows 16 banks apart)
constexpr int STREAM_STAGE = 4 * STREAM_VROW + 2 * STREAM_CELLS;    // C: 4 V rows + p16 of one chunk
constexpr int STREAM_RS = 16;        // C: outputs per workgroup (4 per wave)
constexpr size_t kStreamKqvLds = (size_t)4 * STREAM_DEPTH * STREAM_STAGE + 256 * 4;
// C, batch form: behind the above, per wave the list of its visible stages (uint16 each)
constexpr int STREAM_LIST = kAttnStreamMaxCtx / STREAM_CELLS;
constexpr size_t kStreamBatchKqvLds = kStreamKqvLds + (size_t)4 * STREAM_LIST * 2;
// a prompt's token tile: the most workspace one tile may take (mi355x_attn_prompt, T > 1)
constexpr size_t kStreamPromptWorkspaceMax = (size_t)256 << 20;

// ------------------------------------------------------------------ A: store and scores
enum { STREAM_DECODE = 0, STREAM_PROMPT = 1, STREAM_BATCH = 2 };

__device__ __forceinline__ int64_t stream_batch_cell(const AttnBatchArgs &b, int i) {
    return b.cells_i64 ? ((const int64_t *)b.cells)[i] : (int64_t)((const int32_t *)b.cells)[i];
}
// the batch form's token has no cell (kq_kv_store_batch stored nothing for it): a NaN row
__device__ __forceinline__ bool stream_batch_bad(const AttnBatchArgs &b, int tok) {
    const int pos = b.a.pos[tok];
    const int64_t cell = stream_batch_cell(b, tok);
    return pos < 0 || pos >= b.n_pos || cell < 0 || cell >= b.a.n_ctx;
}
// bytes of a token's block flags: one per 32 cells, in whole 512-cell stages (C reads 16 B per stage)
__host__ __device__ inline int stream_flags_stride(int n_kv) { return (n_kv / 32 + 15) & ~15; }

// STREAM_PROMPT: token blockIdx.z of the tile at tok0 (q / pos rows per token; the cells were stored by
// kq_kv_store, a kernel boundary before, so cell pos is read from the cache like the others).
// STREAM_BATCH: likewise after kq_kv_store_batch, over the row [0, b->n_kv) under the token's mask
// row (b: the descriptor, null for the other kinds; flags: the tile's block flags).
template <int HD, int KIND>
__device__ __forceinline__ void stream_scores(const AttnArgs &a, const AttnBatchArgs *b, float *scores, uint8_t *flags,
                                              int tok0, uint8_t *smem) {
    constexpr bool PROMPT = KIND != STREAM_DECODE, BATCH = KIND == STREAM_BATCH;
    constexpr int KV4 = HD / 8;                    // 16-B pieces of a K row
    constexpr int KPT = STREAM_CHUNK * KV4 / 256;  // pieces per thread
    static_assert(STREAM_CHUNK == 64, "a thread scores the cell of its lane in every pass; one ballot covers the chunk");
    const int g = blockIdx.y, c0 = blockIdx.x * STREAM_CHUNK, t = threadIdx.x;
    const int ti = PROMPT ? (int)blockIdx.z : 0, tok = PROMPT ? tok0 + ti : 0;
    const int gsz = a.n_head / a.n_head_kv;
    const int kvw = a.n_head_kv * HD;
    // the position first: a chunk past n_kv reads nothing (kq_attn_cells requests its K rows
    // with the position; over a cache of 131072 cells that would read every K row per token)
    const int pos_in = a.pos[tok];
    bool bad;  // no cache cell: caches untouched, C outputs NaN
    int pos, n_kv, rowlen;
    if constexpr (BATCH) {
        if (stream_batch_bad(*b, tok)) return;  // (uniform) C reads nothing of this token's rows
        bad = false, pos = pos_in, n_kv = rowlen = b->n_kv;
    } else {
        bad = pos_in < 0 || pos_in >= a.n_ctx;
        pos = bad ? 0 : pos_in;
        n_kv = (pos + 1 + 31) / 32 * 32;
        n_kv = n_kv < a.n_ctx ? n_kv : a.n_ctx;
        rowlen = a.n_ctx;
    }
    if (c0 >= n_kv) return;  // (uniform)
    float *srow = scores + (int64_t)ti * a.n_head * rowlen;
    // BATCH: the mask entry of this thread's cell c0 + lane (f16 widened first) and the chunk's
    // visible cells, the same 64 bits in every wave
    float m = 0.0f;
    uint64_t vb = ~0ull;
    if constexpr (BATCH) {
        const uint8_t *mp = (const uint8_t *)b->mask + (int64_t)tok * b->mask_row_bytes;
        const int c = c0 + (t & 63);
        m = -INFINITY;
        if (c < n_kv) m = b->mask_f16 ? (float)u2h(((const uint16_t *)mp)[c]) : ((const float *)mp)[c];
        vb = __ballot(m != -INFINITY);
        if (g == 0 && t < 2 && c0 + 32 * t < n_kv)
            flags[(int64_t)ti * stream_flags_stride(n_kv) + (c0 >> 5) + t] = (uint32_t)(vb >> (32 * t)) != 0u;
        if (vb == 0) {  // (uniform) nothing visible: no K row is loaded
            for (int i = t; i < STREAM_CHUNK * gsz; i += 256) {
                const int c1 = c0 + i % STREAM_CHUNK;
                if (c1 < n_kv) srow[(int64_t)(g * gsz + i / STREAM_CHUNK) * rowlen + c1] = -INFINITY;
            }
            return;
        }
    }
    uint4 kr[KPT];
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = t + 256 * u, r = i / KV4, k = i % KV4;
        const bool rd = c0 + r < n_kv && (!BATCH || ((vb >> r) & 1));  // (a hidden cell's row is not read)
        kr[u] = rd ? *(const uint4 *)(a.k_cache + (int64_t)(c0 + r) * kvw + (int64_t)g * HD + 8 * k) : uint4{};
    }
    // LDS: q16 [gsz][HD] | k16 [HD] | K rows [STREAM_CHUNK][KV4] (piece k of row r at k ^ (r % KV4))
    uint16_t *q16 = (uint16_t *)smem;
    uint16_t *k16 = q16 + gsz * HD;
    uint4 *krow = (uint4 *)(k16 + HD);
    const bool holds = !PROMPT && pos >= c0 && pos < c0 + STREAM_CHUNK;
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = t + 256 * u, r = i / KV4, k = i % KV4;
        krow[r * KV4 + (k ^ (r % KV4))] = kr[u];
    }
    const float *tc = a.rope_table + (a.rope_row ? 0 : (int64_t)pos * (HD / 2) * 2);
    const float *qrow = a.q + (int64_t)tok * a.n_head * HD;
    for (int i = t; i < gsz * (HD / 2); i += 256) {
        const int hh = i / (HD / 2), p2 = i % (HD / 2);
        const float *qp = qrow + (int64_t)(g * gsz + hh) * HD + 2 * p2;
        const float2 rq = rope_pair(qp[0], qp[1], tc[2 * p2], tc[2 * p2 + 1]);
        q16[hh * HD + 2 * p2] = h2u(f2h_rne(rq.x));
        q16[hh * HD + 2 * p2 + 1] = h2u(f2h_rne(rq.y));
    }
    if (holds) {  // the decode step's new cell: both caches, and the chunk's own copy of the K row
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
    for (int i = t; i < STREAM_CHUNK * gsz; i += 256) {  // lane <-> cell, waves <-> heads
        const int r = i % STREAM_CHUNK, hh = i / STREAM_CHUNK, c = c0 + r;
        if (c >= n_kv) continue;
        float sc = -INFINITY;  // cells past pos (BATCH: hidden by the mask): masked
        if (BATCH ? m != -INFINITY : c <= pos) {
            uint4 kv[KV4];
            if (holds && c == pos) {
#pragma unroll
                for (int k = 0; k < KV4; ++k) kv[k] = ((const uint4 *)k16)[k];
            } else {
#pragma unroll
                for (int k = 0; k < KV4; ++k) kv[k] = krow[r * KV4 + (k ^ (r % KV4))];
            }
            sc = vec_dot_f16_rows<HD>(kv, (const uint4 *)(q16 + hh * HD)) * a.scale;
            if constexpr (BATCH) sc = sc + m;  // (r is the lane in every pass: this thread's mask entry)
        }
        srow[(int64_t)(g * gsz + hh) * rowlen + c] = sc;
    }
}

template <int HD, bool PROMPT>
__global__ void __launch_bounds__(256) kq_attn_stream_scores(const AttnArgs a, float *scores, int tok0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stream_scores<HD, PROMPT ? STREAM_PROMPT : STREAM_DECODE>(a, nullptr, scores, nullptr, tok0, smem);
}

template <int HD>
__global__ void __launch_bounds__(256) kq_attn_stream_scores_batch(const AttnBatchArgs b, float *scores, uint8_t *flags,
                                                                   int tok0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stream_scores<HD, STREAM_BATCH>(b.a, &b, scores, flags, tok0, smem);
}

// ------------------------------------------------------------------ B: soft_max over the workspace
// ggml's in-order `sum += (ggml_float)g` over the ng group sums of the exps e (global memory,
// written by this workgroup before the barrier the caller passed): lane l forms group c0 + l's
// sum as pass 2 did, the dependent adds read the lanes in order. One whole wave.
__device__ __forceinline__ double stream_seq_sum(const float4 *e4, int ng, int lane) {
    double tot = 0.0;
    for (int c0 = 0; c0 < ng; c0 += 64) {
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (c0 + lane < ng) e = e4[c0 + lane];
        const double v = (double)((e.x + e.y) + (e.z + e.w));
        const int m = ng - c0 < 64 ? ng - c0 : 64;
        for (int i = 0; i < m; ++i) tot += readlane_f64(v, i);
    }
    return tot;
}

// The three passes over one head's row: ng groups of four scores at w4, their p16 at p2
__device__ __forceinline__ void stream_softmax_row(float4 *w4, uint2 *p2, int ng) {
    constexpr int NW = STREAM_SM_NT / 64;
    __shared__ float s_max[NW];
    __shared__ double s_part[NW + 1];
    __shared__ int s_gmin[NW], s_bad[NW];
    const int t = threadIdx.x, ln = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    // 1: the max (order-free)
    float m = -INFINITY;
    for (int gi = t; gi < ng; gi += STREAM_SM_NT) {
        const float4 x = w4[gi];
        m = fmaxf(m, fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)));
    }
    const float wmx = wave_fmax(m);
    if (ln == 0) s_max[wv] = wmx;
    __syncthreads();
    float mx = s_max[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) mx = fmaxf(mx, s_max[k]);
    // 2: the exps in place, the vaddvq group sums into the exact-sum tree
    SumExact se;
    for (int gi = t; gi < ng; gi += STREAM_SM_NT) {
        float4 e = w4[gi];
        e.x = e.x == -INFINITY ? 0.0f : v_expf(e.x - mx);
        e.y = e.y == -INFINITY ? 0.0f : v_expf(e.y - mx);
        e.z = e.z == -INFINITY ? 0.0f : v_expf(e.z - mx);
        e.w = e.w == -INFINITY ? 0.0f : v_expf(e.w - mx);
        w4[gi] = e;
        se.add((e.x + e.y) + (e.z + e.w));  // (exact when the total passes the bound: a subset's sum)
    }
    const bool wbad = __any(se.bad);
    const int wgmin = wave_imin(se.gmin);
    double part = se.part;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (ln == 0) {
        s_part[wv] = part;
        s_gmin[wv] = wgmin;
        s_bad[wv] = wbad;
    }
    __syncthreads();  // (also: every thread's exps are visible to the workgroup)
    int gmin = s_gmin[0], anybad = s_bad[0];
    double st = s_part[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) {
        gmin = min(gmin, s_gmin[k]);
        anybad |= s_bad[k];
        st += s_part[k];
    }
    double sum = st;
    if (!sum_exact_ok(st, gmin, anybad != 0)) {  // (uniform)
        if (t < 64) {
            const double s = stream_seq_sum((const float4 *)w4, ng, t);
            if (t == 0) s_part[NW] = s;
        }
        __syncthreads();
        sum = s_part[NW];
    }
    // 3: p = e * (float)(1 / sum) -> f16 (each thread re-reads the groups it wrote)
    const float inv = (float)(1.0 / sum);
    for (int gi = t; gi < ng; gi += STREAM_SM_NT) {
        const float4 e = w4[gi];
        const uint32_t lo = (uint32_t)h2u(f2h_rne(e.x * inv)) | ((uint32_t)h2u(f2h_rne(e.y * inv)) << 16);
        const uint32_t hi = (uint32_t)h2u(f2h_rne(e.z * inv)) | ((uint32_t)h2u(f2h_rne(e.w * inv)) << 16);
        p2[gi] = make_uint2(lo, hi);
    }
}

__global__ void __launch_bounds__(STREAM_SM_NT) kq_attn_stream_softmax(const AttnArgs a, float *scores, uint16_t *p16,
                                                                       int tok0) {
    const int h = blockIdx.x, ti = blockIdx.y;
    const int pos_in = a.pos[tok0 + ti];
    const bool bad = pos_in < 0 || pos_in >= a.n_ctx;
    const int pos = bad ? 0 : pos_in;
    int n_kv = (pos + 1 + 31) / 32 * 32;
    n_kv = n_kv < a.n_ctx ? n_kv : a.n_ctx;
    const int64_t row = ((int64_t)ti * a.n_head + h) * a.n_ctx;
    stream_softmax_row((float4 *)(scores + row), (uint2 *)(p16 + row), n_kv >> 2);
}

// ... of the batch form: the descriptor's row, the rows n_kv apart
__global__ void __launch_bounds__(STREAM_SM_NT) kq_attn_stream_softmax_batch(const AttnBatchArgs b, float *scores,
                                                                             uint16_t *p16, int tok0) {
    const int h = blockIdx.x, ti = blockIdx.y;
    if (stream_batch_bad(b, tok0 + ti)) return;  // (uniform) launch A wrote no scores for this token
    const int64_t row = ((int64_t)ti * b.a.n_head + h) * b.n_kv;
    stream_softmax_row((float4 *)(scores + row), (uint2 *)(p16 + row), b.n_kv >> 2);
}

// ------------------------------------------------------------------ C: KQV through the LDS ring
template <int VM>
__device__ __forceinline__ void stream_wait_vm() {  // s_waitcnt vmcnt(VM), a compiler barrier for memory
    static_assert(VM >= 0 && VM < 64, "vmcnt is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
}

// BATCH (b: the descriptor, null otherwise; flags: launch A's block flags of the tile): the row
// is the descriptor's, and the ring runs over the stages that hold a visible cell.
template <int HD, bool BATCH>
__device__ __forceinline__ void stream_kqv(const AttnArgs &a, const AttnBatchArgs *b, const uint16_t *p16,
                                           const uint8_t *flags, int tok0, uint8_t *smem) {
    constexpr int DS = HD / STREAM_RS;
    constexpr int NDMA = 5;  // LDS-DMA instructions of one stage: 4 V rows + p16
    static_assert((STREAM_DEPTH - 1) * NDMA < 64, "the counted waits fit vmcnt");
    const int h = blockIdx.x / DS, ds = blockIdx.x % DS, ti = blockIdx.y;
    const int t = threadIdx.x, ln = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = h / (a.n_head / a.n_head_kv);
    bool bad;
    int n_kv, rowlen;  // the cells accumulated (32-cell iterations), the workspace's row stride
    if constexpr (BATCH) {
        bad = stream_batch_bad(*b, tok0 + ti);
        n_kv = bad ? 0 : b->n_kv;  // (no cell: nothing is read, a NaN row)
        rowlen = b->n_kv;
    } else {
        const int pos_in = a.pos[tok0 + ti];
        bad = pos_in < 0 || pos_in >= a.n_ctx;
        const int pos = bad ? 0 : pos_in;
        const int n_it = (pos + 32) / 32;  // 32-cell iterations holding a cell <= pos (32 n_it <= n_ctx)
        n_kv = 32 * n_it;
        rowlen = a.n_ctx;
    }
    const int nch = (n_kv + STREAM_CELLS - 1) / STREAM_CELLS;
    uint8_t *ring = smem + (size_t)wv * STREAM_DEPTH * STREAM_STAGE;  // this wave's stages
    uint32_t *red = (uint32_t *)(smem + (size_t)4 * STREAM_DEPTH * STREAM_STAGE);
    const uint32_t ring_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS void *)ring);
    // the wave's 4 V rows (outputs ds * 16 + 4 wv + r) and the head's p16 row
    const int64_t vrow0 = (int64_t)(g * HD + ds * STREAM_RS + 4 * wv) * a.n_ctx;
    const uint8_t *vsrc = (const uint8_t *)(a.v_cache + vrow0) + 16 * ln;
    const uint8_t *psrc = (const uint8_t *)(p16 + ((int64_t)ti * a.n_head + h) * rowlen) + 16 * ln;
    const int64_t vstep = (int64_t)a.n_ctx * 2;
    // chunk c -> stage j % DEPTH (j: its place among the chunks the ring runs over): NDMA
    // instructions on every path (a partial chunk masks lanes), bytes [1024 c, 1024 c + 2 cells)
    // of each row: inside the row's first 2 n_kv <= 2 n_ctx bytes
    auto issue = [&](int j, int c) {
        const int cells = n_kv - c * STREAM_CELLS < STREAM_CELLS ? n_kv - c * STREAM_CELLS : STREAM_CELLS;
        const int nl = cells >> 3;  // 16-B lanes
        const uint32_t st = ring_lds + (uint32_t)((j % STREAM_DEPTH) * STREAM_STAGE);
        const int64_t off = (int64_t)c * (2 * STREAM_CELLS);
#pragma unroll
        for (int r = 0; r < 4; ++r) attn_dma16_lanes(vsrc + r * vstep + off, st + (uint32_t)(r * STREAM_VROW), ln, nl);
        attn_dma16_lanes(psrc + off, st + (uint32_t)(4 * STREAM_VROW), ln, nl);
    };
    // BATCH: the wave's list of the chunks with a visible cell, in order, built before the ring
    // starts (uniform control flow; the flag loads are the kernel's only loads the compiler
    // counts, and all of them are consumed here): lane l looks at chunk s0 + l's 16 flag bytes
    // (those past the row's n_kv / 32 blocks are not flags)
    uint16_t *list = BATCH ? (uint16_t *)(smem + kStreamKqvLds) + wv * STREAM_LIST : nullptr;
    int n_vis = nch;
    if constexpr (BATCH) {
        const int nblk = n_kv >> 5;
        const uint8_t *frow = flags + (int64_t)ti * stream_flags_stride(rowlen);
        n_vis = 0;
        for (int s0 = 0; s0 < nch; s0 += 64) {
            const int s = s0 + ln;
            bool on = false;
            if (s < nch) {
                const uint4 f = *(const uint4 *)(frow + 16 * s);
                const uint32_t fw[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int rem = nblk - 16 * s - 4 * k;  // flags in word k
                    const uint32_t keep = rem >= 4 ? 0xffffffffu : rem <= 0 ? 0u : (1u << (8 * rem)) - 1u;
                    on = on || (fw[k] & keep) != 0u;
                }
            }
            const uint64_t bl = __ballot(on);
            if (on) list[n_vis + __popcll(bl & ((1ull << ln) - 1ull))] = (uint16_t)s;
            n_vis += __builtin_amdgcn_readfirstlane((int)__popcll(bl));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the list is written (read back by other lanes)
        __builtin_amdgcn_wave_barrier();
    }
    // the j-th chunk of a run: of the list, or (every) of all chunks
    auto chunk_of = [&](int j, bool every) {
        if constexpr (BATCH) {
            if (!every) return __builtin_amdgcn_readfirstlane((int)list[j]);
        }
        return j;
    };
    const int r = ln >> 4, jq = ln & 15;
    uint32_t acc1 = 0;
    auto run = [&](const bool every) {
        const int nj = every ? nch : n_vis;
        acc1 = 0;
#pragma unroll
        for (int j = 0; j < STREAM_DEPTH - 1; ++j)
            if (j < nj) issue(j, chunk_of(j, every));  // (uniform)
        for (int j = 0; j < nj; ++j) {
            // stage (j + DEPTH - 1) % DEPTH was read in the last round: those reads have returned
            // (lgkmcnt(0)) before the DMA that overwrites it is issued
            if (j + STREAM_DEPTH - 1 < nj) {
                const int cn = chunk_of(j + STREAM_DEPTH - 1, every);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                issue(j + STREAM_DEPTH - 1, cn);
                stream_wait_vm<(STREAM_DEPTH - 1) * NDMA>();
            } else if (STREAM_DEPTH > 2 && j + 1 < nj) {
                stream_wait_vm<NDMA>();  // (DEPTH 3: one later chunk in flight)
            } else {
                stream_wait_vm<0>();
            }
            static_assert(STREAM_DEPTH == 2 || STREAM_DEPTH == 3, "the tail waits above are written for 2 or 3 stages");
            const int c = chunk_of(j, every);
            const uint8_t *st = ring + (j % STREAM_DEPTH) * STREAM_STAGE;
            const uint32_t *vrow = (const uint32_t *)(st + r * STREAM_VROW) + jq;
            const uint32_t *prow = (const uint32_t *)(st + 4 * STREAM_VROW) + jq;
            const int its = (n_kv - c * STREAM_CELLS < STREAM_CELLS ? n_kv - c * STREAM_CELLS : STREAM_CELLS) >> 5;
            if (its == STREAM_CELLS / 32) {
                uint32_t vb[16], pb[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    vb[k] = vrow[16 * k];
                    pb[k] = prow[16 * k];
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) acc1 = pk_fma_w(vb[k], pb[k], acc1);
            } else {
                for (int k = 0; k < its; ++k) acc1 = pk_fma_w(vrow[16 * k], prow[16 * k], acc1);
            }
        }
    };
    static_assert(STREAM_CELLS / 32 == 16, "a full stage is 16 iterations");
    if constexpr (BATCH) {
        run(false);
        // a skipped stage's products are v * (+0): they can only have turned a lane that ends as
        // -0 into +0 (kq_attn_batch.hip's header). A wave with such a lane runs every stage.
        const bool negz = (acc1 & 0xffffu) == 0x8000u || (acc1 >> 16) == 0x8000u;
        if (n_vis < nch && __any(negz)) {  // (uniform)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the last stage's reads returned
            run(true);
        }
    } else {
        run(true);
    }
    red[t] = acc1;
    __syncthreads();
    // the GGML_F16_VEC_REDUCE of output vr_l's 4 accumulators: quad (vr_l, j = 0..3)
    const int vr_l = (t >> 2) & (STREAM_RS - 1), j = t & 3;
    const bool kt = t < 4 * STREAM_RS;
    uint32_t acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = red[16 * vr_l + 4 * j + k];
    const float o = f16x8_reduce_quad(acc);  // every lane active; the quad's lane 0 holds output vr_l
    if (kt && j == 0)
        a.out[((int64_t)(tok0 + ti) * a.n_head + h) * HD + ds * STREAM_RS + vr_l] = bad ? __builtin_nanf("") : o;
}

template <int HD>
__global__ void __launch_bounds__(256) kq_attn_stream_kqv(const AttnArgs a, const uint16_t *p16, int tok0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stream_kqv<HD, false>(a, nullptr, p16, nullptr, tok0, smem);
}

template <int HD>
__global__ void __launch_bounds__(256) kq_attn_stream_kqv_batch(const AttnBatchArgs b, const uint16_t *p16,
                                                                const uint8_t *flags, int tok0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stream_kqv<HD, true>(b.a, &b, p16, flags, tok0, smem);
}

// ------------------------------------------------------------------ host side
namespace {

std::atomic<int> g_attn_stream{0};

size_t stream_scores_lds(int hd, int gsz) {
    return (size_t)gsz * hd * 2 + (size_t)hd * 2 + (size_t)STREAM_CHUNK * hd * 2;
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone;
}

// the three launches for tokens [tok0, tok0 + nt) of a prompt (prompt) or the decode step
template <int HD>
int launch_stream_tile(const AttnArgs &a, bool prompt, int tok0, int nt, uint8_t *ws, hipStream_t s) {
    const int gsz = a.n_head / a.n_head_kv;
    float *scores = (float *)ws;
    uint16_t *p16 = (uint16_t *)(ws + (size_t)nt * a.n_head * a.n_ctx * 4);
    const dim3 ga((unsigned)((a.n_ctx + STREAM_CHUNK - 1) / STREAM_CHUNK), (unsigned)a.n_head_kv, (unsigned)nt);
    const size_t la = stream_scores_lds(HD, gsz);
    int rc = prompt ? timed_launch(HD == 64 ? "kq::kq_attn_stream_scores<64, prompt>" : "kq::kq_attn_stream_scores<128, prompt>",
                                   0.0, kq_attn_stream_scores<HD, true>, ga, dim3(256), la, s, a, scores, tok0)
                    : timed_launch(HD == 64 ? "kq::kq_attn_stream_scores<64>" : "kq::kq_attn_stream_scores<128>",
                                   0.0, kq_attn_stream_scores<HD, false>, ga, dim3(256), la, s, a, scores, tok0);
    if (rc) return rc;
    rc = timed_launch("kq::kq_attn_stream_softmax", 0.0, kq_attn_stream_softmax, dim3((unsigned)a.n_head, (unsigned)nt),
                      dim3(STREAM_SM_NT), 0, s, a, scores, p16, tok0);
    if (rc) return rc;
    allow_lds((const void *)kq_attn_stream_kqv<HD>, kStreamKqvLds);
    return timed_launch(HD == 64 ? "kq::kq_attn_stream_kqv<64>" : "kq::kq_attn_stream_kqv<128>", 0.0, kq_attn_stream_kqv<HD>,
                        dim3((unsigned)(a.n_head * (HD / STREAM_RS)), (unsigned)nt), dim3(256), kStreamKqvLds, s, a,
                        (const uint16_t *)p16, tok0);
}

// ... of the batch form for tokens [tok0, tok0 + nt): rows of n_kv entries, then the block flags
template <int HD>
int launch_stream_batch_tile(const AttnBatchArgs &b, int tok0, int nt, uint8_t *ws, hipStream_t s) {
    const AttnArgs &a = b.a;
    const int gsz = a.n_head / a.n_head_kv;
    float *scores = (float *)ws;
    uint16_t *p16 = (uint16_t *)(ws + (size_t)nt * a.n_head * b.n_kv * 4);
    uint8_t *flags = ws + (size_t)nt * a.n_head * b.n_kv * 6;
    const dim3 ga((unsigned)((b.n_kv + STREAM_CHUNK - 1) / STREAM_CHUNK), (unsigned)a.n_head_kv, (unsigned)nt);
    int rc = timed_launch(HD == 64 ? "kq::kq_attn_stream_scores<64, batch>" : "kq::kq_attn_stream_scores<128, batch>", 0.0,
                          kq_attn_stream_scores_batch<HD>, ga, dim3(256), stream_scores_lds(HD, gsz), s, b, scores, flags, tok0);
    if (rc) return rc;
    rc = timed_launch("kq::kq_attn_stream_softmax<batch>", 0.0, kq_attn_stream_softmax_batch,
                      dim3((unsigned)a.n_head, (unsigned)nt), dim3(STREAM_SM_NT), 0, s, b, scores, p16, tok0);
    if (rc) return rc;
    allow_lds((const void *)kq_attn_stream_kqv_batch<HD>, kStreamBatchKqvLds);
    return timed_launch(HD == 64 ? "kq::kq_attn_stream_kqv<64, batch>" : "kq::kq_attn_stream_kqv<128, batch>", 0.0,
                        kq_attn_stream_kqv_batch<HD>, dim3((unsigned)(a.n_head * (HD / STREAM_RS)), (unsigned)nt), dim3(256),
                        kStreamBatchKqvLds, s, b, (const uint16_t *)p16, (const uint8_t *)flags, tok0);
}

// tokens per tile: by the workspace cap (ATTN_STREAM_TILE: fewer), at least one
int stream_tile(size_t per_tok, int n_tok) {
    int64_t tile = (int64_t)(kStreamPromptWorkspaceMax / per_tok);
    const int64_t kt = (int64_t)knob(KNOB_ATTN_STREAM_TILE);
    if (kt > 0 && kt < tile) tile = kt;
    if (tile > 65535) tile = 65535;  // one grid row per token
    if (tile > n_tok) tile = n_tok;
    return tile < 1 ? 1 : (int)tile;
}

// the batch form's workspace per token of a tile: 6 bytes per (head, cell of the row), the block flags
size_t stream_batch_per_tok(const AttnBatchArgs &b) {
    return (size_t)b.a.n_head * b.n_kv * 6 + (size_t)stream_flags_stride(b.n_kv);
}

}  // namespace

// mi355x_attn_stream's mode, or the ATTN_STREAM debug knob's where that holds one (bench runs
// reach the selector through --knob only; a knob change renews the graph key by itself)
int attn_stream_mode() {
    const double k = knob(KNOB_ATTN_STREAM);
    return k == 0.0 || k == 1.0 || k == 2.0 ? (int)k : g_attn_stream.load();
}

// what the other kernels refuse for the cache's size alone (check_attn)
bool attn_size_refused(const AttnArgs &a) { return a.n_ctx > 8192 || attn_lds(a.head_dim, a.n_ctx) > 64 * 1024; }

// the shapes the streamed kernels take (check_attn has passed the rest)
static bool stream_shape_ok(const AttnArgs &a) {
    const int gsz = a.n_head_kv > 0 ? a.n_head / a.n_head_kv : 0;
    return (a.head_dim == 64 || a.head_dim == 128) && a.n_ctx >= 32 && a.n_ctx <= kAttnStreamMaxCtx && a.n_ctx % 32 == 0 &&
           gsz >= 1 && stream_scores_lds(a.head_dim, gsz) <= 64 * 1024 && a.n_head <= 65535;
}

bool attn_stream_applies(const AttnArgs &a) {
    const int mode = attn_stream_mode();
    return mode != 0 && stream_shape_ok(a) && (mode == 2 || attn_size_refused(a));
}

bool attn_stream_prompt_applies(const AttnArgs &a) {
    const int mode = attn_stream_mode();
    return mode != 0 && stream_shape_ok(a) &&
           (mode == 2 || attn_size_refused(a) || attn_prompt_lds(a.head_dim, a.n_ctx) > 160 * 1024);
}

// tokens per tile of a prompt of n_tok tokens
int attn_stream_tile(const AttnArgs &a, int n_tok) { return stream_tile((size_t)a.n_head * a.n_ctx * 6, n_tok); }

size_t attn_stream_workspace(const AttnArgs &a, int n_tok) {
    return (size_t)attn_stream_tile(a, n_tok < 1 ? 1 : n_tok) * a.n_head * a.n_ctx * 6;
}

int launch_attn_stream(const AttnArgs &a, hipStream_t s) {
    uint8_t *ws = (uint8_t *)attn_cells_buffer(attn_stream_workspace(a, 1), s, !capturing(s));
    if (!ws) return MI355X_E_WORKSPACE;  // captured without a reservation: no other kernel takes the shape
    return a.head_dim == 64 ? launch_stream_tile<64>(a, false, 0, 1, ws, s) : launch_stream_tile<128>(a, false, 0, 1, ws, s);
}

int launch_attn_stream_prompt(const AttnArgs &a0, int n_tok, hipStream_t s) {
    if (n_tok <= 0) return MI355X_OK;
    if (a0.q8_out) return MI355X_E_INVAL;  // the Q8L-output fusion is the group kernel's (attn_prompt_q8_ok)
    AttnArgs a = a0;
    a.n_tok = n_tok;
    uint8_t *ws = (uint8_t *)attn_cells_buffer(attn_stream_workspace(a, n_tok), s, !capturing(s));
    if (!ws) return MI355X_E_WORKSPACE;
    int rc = MI355X_OK;
    if (!a.no_store) rc = launch_kv_store(a, n_tok, s);
    const int tile = attn_stream_tile(a, n_tok);
    for (int tok0 = 0; tok0 < n_tok && !rc; tok0 += tile) {
        const int nt = n_tok - tok0 < tile ? n_tok - tok0 : tile;
        rc = a.head_dim == 64 ? launch_stream_tile<64>(a, true, tok0, nt, ws, s) : launch_stream_tile<128>(a, true, tok0, nt, ws, s);
    }
    return rc;
}

// ---- the batch form (kq_attn_batch.hip selects it: attn_batch_form)
bool attn_batch_stream_applies(const AttnBatchArgs &b, bool refused) {
    const int mode = attn_stream_mode();
    return mode != 0 && stream_shape_ok(b.a) && (mode == 2 || refused);
}

size_t attn_batch_stream_workspace(const AttnBatchArgs &b) {
    const size_t per_tok = stream_batch_per_tok(b);
    return (size_t)stream_tile(per_tok, b.n_tok) * per_tok;
}

void *attn_batch_stream_buffer(const AttnBatchArgs &b, hipStream_t s) {
    return attn_cells_buffer(attn_batch_stream_workspace(b), s, !capturing(s));
}

int launch_attn_batch_stream(const AttnBatchArgs &b, void *ws, hipStream_t s) {
    const int tile = stream_tile(stream_batch_per_tok(b), b.n_tok);
    int rc = MI355X_OK;
    for (int tok0 = 0; tok0 < b.n_tok && !rc; tok0 += tile) {
        const int nt = b.n_tok - tok0 < tile ? b.n_tok - tok0 : tile;
        rc = b.a.head_dim == 64 ? launch_stream_batch_tile<64>(b, tok0, nt, (uint8_t *)ws, s)
                                : launch_stream_batch_tile<128>(b, tok0, nt, (uint8_t *)ws, s);
    }
    return rc;
}

}  // namespace kq

using namespace kq;

extern "C" {

int mi355x_attn_stream(int mode) {
    if (mode < 0 || mode > 2) return MI355X_E_INVAL;
    return g_attn_stream.exchange(mode);
}

}  // extern "C"
