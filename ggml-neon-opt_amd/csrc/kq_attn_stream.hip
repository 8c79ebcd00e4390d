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
// a prompt's token tile: the most workspace one tile may take (mi355x_attn_prompt, T > 1)
constexpr size_t kStreamPromptWorkspaceMax = (size_t)256 << 20;

// ------------------------------------------------------------------ A: store and scores
// PROMPT: token blockIdx.z of the tile at tok0 (q / pos rows per token; the cells were stored by
// kq_kv_store, a kernel boundary before, so cell pos is read from the cache like the others).
template <int HD, bool PROMPT>
__global__ void __launch_bounds__(256) kq_attn_stream_scores(const AttnArgs a, float *scores, int tok0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int KV4 = HD / 8;                    // 16-B pieces of a K row
    constexpr int KPT = STREAM_CHUNK * KV4 / 256;  // pieces per thread
    const int g = blockIdx.y, c0 = blockIdx.x * STREAM_CHUNK, t = threadIdx.x;
    const int ti = PROMPT ? (int)blockIdx.z : 0, tok = PROMPT ? tok0 + ti : 0;
    const int gsz = a.n_head / a.n_head_kv;
    const int kvw = a.n_head_kv * HD;
    // the position first: a chunk past n_kv reads nothing (kq_attn_cells requests its K rows
    // with the position; over a cache of 131072 cells that would read every K row per token)
    const int pos_in = a.pos[tok];
    const bool bad = pos_in < 0 || pos_in >= a.n_ctx;  // no cache cell: caches untouched, C outputs NaN
    const int pos = bad ? 0 : pos_in;
    int n_kv = (pos + 1 + 31) / 32 * 32;
    n_kv = n_kv < a.n_ctx ? n_kv : a.n_ctx;
    if (c0 >= n_kv) return;  // (uniform)
    uint4 kr[KPT];
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = t + 256 * u, r = i / KV4, k = i % KV4;
        kr[u] = c0 + r < n_kv ? *(const uint4 *)(a.k_cache + (int64_t)(c0 + r) * kvw + (int64_t)g * HD + 8 * k) : uint4{};
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
    float *srow = scores + (int64_t)ti * a.n_head * a.n_ctx;
    for (int i = t; i < STREAM_CHUNK * gsz; i += 256) {  // lane <-> cell, waves <-> heads
        const int r = i % STREAM_CHUNK, hh = i / STREAM_CHUNK, c = c0 + r;
        if (c >= n_kv) continue;
        float sc = -INFINITY;  // cells past pos: masked
        if (c <= pos) {
            uint4 kv[KV4];
            if (holds && c == pos) {
#pragma unroll
                for (int k = 0; k < KV4; ++k) kv[k] = ((const uint4 *)k16)[k];
            } else {
#pragma unroll
                for (int k = 0; k < KV4; ++k) kv[k] = krow[r * KV4 + (k ^ (r % KV4))];
            }
            sc = vec_dot_f16_rows<HD>(kv, (const uint4 *)(q16 + hh * HD)) * a.scale;
        }
        srow[(int64_t)(g * gsz + hh) * a.n_ctx + c] = sc;
    }
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

__global__ void __launch_bounds__(STREAM_SM_NT) kq_attn_stream_softmax(const AttnArgs a, float *scores, uint16_t *p16,
                                                                       int tok0) {
    constexpr int NW = STREAM_SM_NT / 64;
    __shared__ float s_max[NW];
    __shared__ double s_part[NW + 1];
    __shared__ int s_gmin[NW], s_bad[NW];
    const int h = blockIdx.x, ti = blockIdx.y, t = threadIdx.x, ln = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int pos_in = a.pos[tok0 + ti];
    const bool bad = pos_in < 0 || pos_in >= a.n_ctx;
    const int pos = bad ? 0 : pos_in;
    int n_kv = (pos + 1 + 31) / 32 * 32;
    n_kv = n_kv < a.n_ctx ? n_kv : a.n_ctx;
    const int ng = n_kv >> 2;
    const int64_t row = ((int64_t)ti * a.n_head + h) * a.n_ctx;
    float4 *w4 = (float4 *)(scores + row);
    uint2 *p2 = (uint2 *)(p16 + row);
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

// ------------------------------------------------------------------ C: KQV through the LDS ring
template <int VM>
__device__ __forceinline__ void stream_wait_vm() {  // s_waitcnt vmcnt(VM), a compiler barrier for memory
    static_assert(VM >= 0 && VM < 64, "vmcnt is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
}

template <int HD>
__global__ void __launch_bounds__(256) kq_attn_stream_kqv(const AttnArgs a, const uint16_t *p16, int tok0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int DS = HD / STREAM_RS;
    constexpr int NDMA = 5;  // LDS-DMA instructions of one stage: 4 V rows + p16
    static_assert((STREAM_DEPTH - 1) * NDMA < 64, "the counted waits fit vmcnt");
    const int h = blockIdx.x / DS, ds = blockIdx.x % DS, ti = blockIdx.y;
    const int t = threadIdx.x, ln = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = h / (a.n_head / a.n_head_kv);
    const int pos_in = a.pos[tok0 + ti];
    const bool bad = pos_in < 0 || pos_in >= a.n_ctx;
    const int pos = bad ? 0 : pos_in;
    const int n_it = (pos + 32) / 32;  // 32-cell iterations holding a cell <= pos (32 n_it <= n_ctx)
    const int n_kv = 32 * n_it;
    const int nch = (n_kv + STREAM_CELLS - 1) / STREAM_CELLS;
    uint8_t *ring = smem + (size_t)wv * STREAM_DEPTH * STREAM_STAGE;  // this wave's stages
    uint32_t *red = (uint32_t *)(smem + (size_t)4 * STREAM_DEPTH * STREAM_STAGE);
    const uint32_t ring_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(LDS void *)ring);
    // the wave's 4 V rows (outputs ds * 16 + 4 wv + r) and the head's p16 row
    const int64_t vrow0 = (int64_t)(g * HD + ds * STREAM_RS + 4 * wv) * a.n_ctx;
    const uint8_t *vsrc = (const uint8_t *)(a.v_cache + vrow0) + 16 * ln;
    const uint8_t *psrc = (const uint8_t *)(p16 + ((int64_t)ti * a.n_head + h) * a.n_ctx) + 16 * ln;
    const int64_t vstep = (int64_t)a.n_ctx * 2;
    // chunk c -> stage c % DEPTH: NDMA instructions on every path (a partial chunk masks lanes),
    // bytes [1024 c, 1024 c + 2 cells) of each row: inside the row's first 2 n_kv <= 2 n_ctx bytes
    auto issue = [&](int c) {
        const int cells = n_kv - c * STREAM_CELLS < STREAM_CELLS ? n_kv - c * STREAM_CELLS : STREAM_CELLS;
        const int nl = cells >> 3;  // 16-B lanes
        const uint32_t st = ring_lds + (uint32_t)((c % STREAM_DEPTH) * STREAM_STAGE);
        const int64_t off = (int64_t)c * (2 * STREAM_CELLS);
#pragma unroll
        for (int r = 0; r < 4; ++r) attn_dma16_lanes(vsrc + r * vstep + off, st + (uint32_t)(r * STREAM_VROW), ln, nl);
        attn_dma16_lanes(psrc + off, st + (uint32_t)(4 * STREAM_VROW), ln, nl);
    };
#pragma unroll
    for (int c = 0; c < STREAM_DEPTH - 1; ++c)
        if (c < nch) issue(c);  // (uniform)
    const int r = ln >> 4, jq = ln & 15;
    uint32_t acc1 = 0;
    for (int c = 0; c < nch; ++c) {
        // stage (c + DEPTH - 1) % DEPTH was read in the last round: those reads have returned
        // (lgkmcnt(0)) before the DMA that overwrites it is issued
        if (c + STREAM_DEPTH - 1 < nch) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(c + STREAM_DEPTH - 1);
            stream_wait_vm<(STREAM_DEPTH - 1) * NDMA>();
        } else if (STREAM_DEPTH > 2 && c + 1 < nch) {
            stream_wait_vm<NDMA>();  // (DEPTH 3: one later chunk in flight)
        } else {
            stream_wait_vm<0>();
        }
        static_assert(STREAM_DEPTH == 2 || STREAM_DEPTH == 3, "the tail waits above are written for 2 or 3 stages");
        const uint8_t *st = ring + (c % STREAM_DEPTH) * STREAM_STAGE;
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
    static_assert(STREAM_CELLS / 32 == 16, "a full stage is 16 iterations");
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

// tokens per tile of a prompt of n_tok tokens: by the workspace cap (ATTN_STREAM_TILE: fewer), at least one
int attn_stream_tile(const AttnArgs &a, int n_tok) {
    const size_t per_tok = (size_t)a.n_head * a.n_ctx * 6;
    int64_t tile = (int64_t)(kStreamPromptWorkspaceMax / per_tok);
    const int64_t kt = (int64_t)knob(KNOB_ATTN_STREAM_TILE);
    if (kt > 0 && kt < tile) tile = kt;
    if (tile > 65535) tile = 65535;  // one grid row per token
    if (tile > n_tok) tile = n_tok;
    return tile < 1 ? 1 : (int)tile;
}

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

}  // namespace kq

using namespace kq;

extern "C" {

int mi355x_attn_stream(int mode) {
    if (mode < 0 || mode > 2) return MI355X_E_INVAL;
    return g_attn_stream.exchange(mode);
}

}  // extern "C"
