// kq_attn_batch.hip — the non-flash attention block of a batch of tokens whose KV cells and
// mask come from the graph's own inputs (ggml: SET_ROWS(k_idxs / v_idxs) + MUL_MAT(K cache, Q)
// + SOFT_MAX(kq, mask, scale) + MUL_MAT(V cache, kq)): several sequences in one unified
// cache, or one sequence whose cells have moved (a removed cell, a context shift, a prefix
// reused at another offset). kq_attn_decode (kq_attn_decode.hip) / kq_attn_prompt (kq_ops.hip) store a token at
// cell == pos and attend causally over [0, pos]; here nothing derives a cell or visibility
// from the position, which only selects the rope row.
//
// Two launches on one stream:
//  kq_kv_store_batch: token i's rope(k) at pos[i] -> the f16 K row of cell cells[i], v -> the
//    transposed f16 V column of that cell (kq_kv_store's arithmetic). A cell outside
//    [0, n_ctx) or a position outside [0, n_pos) writes nothing. Every store is complete
//    before the second launch starts, so a query sees every cell of its own batch.
//  kq_attn_batch: one workgroup per (KV group, token) — the group's n_head / n_head_kv query
//    heads share every K row, V chunk and the token's mask row, as kq_attn_prompt_group does
//    — or per (query head, token) where the group's rows do not fit the LDS or the group has
//    more than 8 heads. Per query the arithmetic is kq_attn_prompt's, op for op:
//    vec_dot_f16_rows, the order-free max, v_expf, the (e0 + e1) + (e2 + e3) group sums,
//    softmax_group_sum, p16 = f16(w * inv), the four-accumulator f16 KQV, f16x8_reduce_quad;
//    the row runs over cells [0, n_kv) and the score is dot * scale + mask[c]
//    (ggml_compute_forward_soft_max_f32: wp = sp * scale, wp += slope * mask with slope 1; an
//    f16 mask widened to f32 first), so a finite non-zero mask entry is added as it is and
//    -INF gives the weight exact +0.
//
// Load skipping. The token's mask row is staged in LDS once (f32) with one "any visible" flag
// per 32-cell block (visible: mask != -INF). Global loads that cannot change a bit are left out:
//  * KQ of a masked cell: its score is dot * scale + (-INF) = -INF whatever finite (or -inf)
//    value the dot has, so the K row is not read and -INF is written. (A dot that overflowed
//    to +inf or a NaN in the cell would give NaN in ggml: cells inside [0, n_kv) hold finite
//    values whose dot stays finite, as every cell this library wrote does.)
//  * soft_max runs over the whole row from LDS, nothing is skipped there: a masked cell's
//    e is exact +0 and a group of four masked cells adds 0.0 to the double sum, as in ggml.
//  * KQV of a block without a visible cell: every weight of the block is +0 (w = +0, inv > 0,
//    f16(+0) = +0) and for a finite v, fma(v, +0, acc) = acc + (+-0) leaves acc unchanged —
//    except for the sign of a zero: acc = -0 becomes +0 when v * (+0) is +0. acc starts at +0
//    and turns -0 only when a visible product underflows to -0 (or v = -0 meets acc = -0).
//    By induction over the cells in order, the accumulator with the skips (s) and ggml's (f)
//    are equal or (s, f) = (-0, +0): a visible cell with v * p != 0 gives both the same
//    rounded value (the sign of an underflow is the product's), one with v * p == 0 keeps the
//    pair inside {(-0, +0), equal}. So only a FINAL accumulator lane that is -0 can differ;
//    a thread that ends with such a lane runs its cells again without skipping, which is ggml's
//    order exactly. Every other thread's lanes are ggml's bit for bit.
//  Visible cells are never compacted: the groups of four and the accumulator lane cell % 32
//  are positional, so a skipped block keeps its place. Nothing at or past cell n_kv is read.
//
// Caches past this kernel's sizes (attn_size_refused, or neither LDS form fits) run, under
// mi355x_attn_stream, kq_kv_store_batch and then the batch form of the streamed kernels
// (kq_attn_stream.hip; attn_batch_form returns MI355X_ATTN_PATH_STREAM), with the same bits.
#include <math.h>
#include <stdint.h>

#include <atomic>

#include <hip/hip_ext.h>

#include "kq_common.h"
#include "kq_internal.h"
#include "kq_device.h"
#include "kq_ops_device.h"

namespace kq {

constexpr int BATCH_GMAX = 8;  // query heads per kv group handled by the group form
extern std::atomic<int> g_prompt_impl;  // mi355x_attn_prompt_impl (kq_ops.hip): ATTN_HEAD forces the per-head form

__device__ __forceinline__ int64_t batch_cell(const AttnBatchArgs &b, int i) {
    return b.cells_i64 ? ((const int64_t *)b.cells)[i] : (int64_t)((const int32_t *)b.cells)[i];
}

template <int HD>
__global__ void __launch_bounds__(256) kq_kv_store_batch(const AttnBatchArgs b) {
    const AttnArgs &a = b.a;
    const int i = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const int pos = a.pos[i];
    const int64_t cell = batch_cell(b, i);
    // no cell for this token (its output row is NaN)
    if (pos < 0 || pos >= b.n_pos || cell < 0 || cell >= a.n_ctx) return;
    const int kvw = a.n_head_kv * HD;
    const float *tc = a.rope_table + (int64_t)pos * (HD / 2) * 2;
    if (t < HD / 2) {
        const float *kp = a.k + (int64_t)i * kvw + (int64_t)g * HD + 2 * t;
        const float2 rk = rope_pair(kp[0], kp[1], tc[2 * t], tc[2 * t + 1]);
        const uint16_t k0 = h2u(f2h_rne(rk.x)), k1 = h2u(f2h_rne(rk.y));
        *(uint32_t *)(a.k_cache + cell * kvw + (int64_t)g * HD + 2 * t) = k0 | ((uint32_t)k1 << 16);
    } else if (t < HD / 2 + HD) {
        const int d = t - HD / 2;
        a.v_cache[(int64_t)(g * HD + d) * a.n_ctx + cell] = h2u(f2h_rne(a.v[(int64_t)i * kvw + (int64_t)g * HD + d]));
    }
}

// LDS (R = the workgroup's query heads): q16 [R][HD] | w [R][n_kv] f32 | p16 [R][n_kv], with
// gsum [R][n_kv/4] f64 over the same bytes (read before p16 is written) | scal [R][4] f32 |
// the token's mask row [n_kv] f32 | the block flags [n_kv/32]
size_t attn_batch_lds(int hd, int n_kv, int rows) {
    return (size_t)rows * ((size_t)2 * hd + (size_t)n_kv * 6 + 16) + (size_t)n_kv * 4 + (size_t)(n_kv / 32) * 4;
}

// GSZ: the workgroup's heads fixed at compile time (1: the per-head form and MHA; 4, 8: the
// common groups), or 0 for any group of at most BATCH_GMAX heads.
template <int HD, int GSZ>
__global__ void __launch_bounds__(256) kq_attn_batch(const AttnBatchArgs b) {
    constexpr int KV4 = HD / 8;
    constexpr int ITEMS = HD * 4 / 256;
    constexpr int GM = GSZ > 0 ? GSZ : BATCH_GMAX;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const AttnArgs &a = b.a;
    const int t = threadIdx.x, lane = t & 63, i = blockIdx.y;
    const int gq = a.n_head / a.n_head_kv;
    const int R = GSZ > 0 ? GSZ : gq;  // <= BATCH_GMAX (host check)
    const int h0 = b.per_head ? (int)blockIdx.x : (int)blockIdx.x * gq;  // heads [h0, h0 + R) of kv group g
    const int g = h0 / gq;
    const int nkv = b.n_kv, nblk = nkv >> 5, ng = nkv >> 2;
    const int kvw = a.n_head_kv * HD, nc = a.n_ctx;
    const int pos = a.pos[i];
    const int64_t cell = batch_cell(b, i);
    const int64_t orow = (int64_t)i * a.n_head * HD + (int64_t)h0 * HD;
    if (pos < 0 || pos >= b.n_pos || cell < 0 || cell >= nc) {  // no cell was stored: a NaN row
        for (int u = t; u < R * HD; u += 256) a.out[orow + u] = __builtin_nanf("");
        return;
    }
    uint16_t *q16 = (uint16_t *)smem;              // [R][HD]
    float *w = (float *)(q16 + R * HD);            // [R][nkv]
    uint16_t *p16 = (uint16_t *)(w + R * nkv);     // [R][nkv]
    double *gsum = (double *)p16;                  // [R][nkv/4], before p16
    float *scal = (float *)(p16 + R * nkv);        // [R][4]: max, 1 / sum
    float *mrow = scal + 4 * R;                    // [nkv]
    int *vis = (int *)(mrow + nkv);                // [nblk]: the block has a visible cell

    // the token's mask row -> f32, and the per-block flags (a wave covers two blocks a pass)
    const uint8_t *mp = (const uint8_t *)b.mask + (int64_t)i * b.mask_row_bytes;
    for (int c = t; c < nkv; c += 256) {
        const float m = b.mask_f16 ? (float)u2h(((const uint16_t *)mp)[c]) : ((const float *)mp)[c];
        mrow[c] = m;
        const uint64_t bl = __ballot(m != -INFINITY);
        if ((lane & 31) == 0) vis[c >> 5] = (uint32_t)(bl >> (lane & 32)) != 0u;
    }
    {  // rope(q) of the workgroup's heads at the token's position -> f16
        const float *tc = a.rope_table + (int64_t)pos * (HD / 2) * 2;
        for (int u = t; u < R * (HD / 2); u += 256) {
            const int hh = u / (HD / 2), pr = u - hh * (HD / 2);
            const float *qp = a.q + (int64_t)i * a.n_head * HD + (int64_t)(h0 + hh) * HD + 2 * pr;
            const float2 rq = rope_pair(qp[0], qp[1], tc[2 * pr], tc[2 * pr + 1]);
            q16[hh * HD + 2 * pr] = h2u(f2h_rne(rq.x));
            q16[hh * HD + 2 * pr + 1] = h2u(f2h_rne(rq.y));
        }
    }
    __syncthreads();
    // KQ: thread t owns cells t, t + 256, ...; one K row load serves every head; a masked
    // cell's row is not read
    for (int c = t; c < nkv; c += 256) {
        const float m = mrow[c];
        if (m != -INFINITY) {
            uint4 kv[KV4];
            const uint4 *kr = (const uint4 *)(a.k_cache + (int64_t)c * kvw + (int64_t)g * HD);
#pragma unroll
            for (int k = 0; k < KV4; ++k) kv[k] = kr[k];
#pragma unroll
            for (int hh = 0; hh < GM; ++hh)
                if (GSZ > 0 || hh < R)
                    w[hh * nkv + c] = vec_dot_f16_rows<HD>(kv, (const uint4 *)(q16 + hh * HD)) * a.scale + m;
        } else {
            for (int r = 0; r < R; ++r) w[r * nkv + c] = -INFINITY;
        }
    }
    __syncthreads();
    // soft_max per row: max (one wave per row, order-free)
    for (int hh = t >> 6; hh < R; hh += 4) {
        float m = -INFINITY;
        for (int c = lane; c < nkv; c += 64) m = fmaxf(m, w[hh * nkv + c]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) scal[4 * hh] = m;
    }
    __syncthreads();
    // v_expf and the vaddvq group sums
    for (int u = t; u < R * ng; u += 256) {
        const int hh = u / ng, gi = u - hh * ng;
        const float mx = scal[4 * hh];
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float wv = w[hh * nkv + 4 * gi + k];
            e[k] = wv == -INFINITY ? 0.0f : v_expf(wv - mx);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) w[hh * nkv + 4 * gi + k] = e[k];
        gsum[hh * ng + gi] = (double)((e[0] + e[1]) + (e[2] + e[3]));
    }
    __syncthreads();
    // ggml's in-order double sum (a tree where exact: softmax_group_sum), one wave per row
    for (int hh = t >> 6; hh < R; hh += 4) {
        const float inv = (float)(1.0 / softmax_group_sum(gsum + hh * ng, ng, lane));
        if (lane == 0) scal[4 * hh + 1] = inv;
    }
    __syncthreads();
    for (int u = t; u < R * nkv; u += 256) {
        const int hh = u / nkv;
        p16[u] = h2u(f2h_rne(w[u] * scal[4 * hh + 1]));
    }
    __syncthreads();
    // KQV: thread (d, j) -> accumulator j of output d of every head (cells 32 it + 8 j + l); one
    // V chunk per (d, j, it) serves them all, 4 chunks in flight; a block without a visible
    // cell is neither loaded nor accumulated (the header comment: exact, but for the sign of a
    // zero lane, which the second pass settles)
#pragma unroll
    for (int ii = 0; ii < ITEMS; ++ii) {
        const int item = t + 256 * ii;
        const int d = item >> 2, j = item & 3;
        const uint16_t *vr = a.v_cache + (int64_t)(g * HD + d) * nc;
        uint32_t acc[GM][4];  // lanes 2k, 2k+1 of head hh's accumulator j in word k
        auto run = [&](const bool every) {
#pragma unroll
            for (int hh = 0; hh < GM; ++hh)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[hh][k] = 0u;
            for (int it0 = 0; it0 < nblk; it0 += 4) {
                bool on[4];
                uint4 vq[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int it = it0 + k < nblk ? it0 + k : nblk - 1;
                    on[k] = it0 + k < nblk && (every || __builtin_amdgcn_readfirstlane(vis[it]) != 0);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) vq[k] = on[k] ? *(const uint4 *)(vr + 32 * (it0 + k) + 8 * j) : uint4{};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!on[k]) continue;
                    const int c0 = 32 * (it0 + k) + 8 * j;
#pragma unroll
                    for (int hh = 0; hh < GM; ++hh) {
                        if (GSZ == 0 && hh >= R) break;
                        const uint4 pp = *(const uint4 *)(p16 + hh * nkv + c0);
                        acc[hh][0] = pk_fma_w(vq[k].x, pp.x, acc[hh][0]);
                        acc[hh][1] = pk_fma_w(vq[k].y, pp.y, acc[hh][1]);
                        acc[hh][2] = pk_fma_w(vq[k].z, pp.z, acc[hh][2]);
                        acc[hh][3] = pk_fma_w(vq[k].w, pp.w, acc[hh][3]);
                    }
                }
            }
        };
        run(false);
        bool negz = false;  // a lane that ended as -0: a skipped +0 product could have made it +0
#pragma unroll
        for (int hh = 0; hh < GM; ++hh)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                negz = negz || (acc[hh][k] & 0xffffu) == 0x8000u || (acc[hh][k] >> 16) == 0x8000u;
        if (negz) run(true);
        // the 4 accumulators of output d sit in the 4 lanes of a quad (j = t & 3)
#pragma unroll
        for (int hh = 0; hh < GM; ++hh) {
            if (GSZ == 0 && hh >= R) break;
            const float o = f16x8_reduce_quad(acc[hh]);
            if (j == 0) a.out[orow + (int64_t)hh * HD + d] = o;
        }
    }
}

namespace {

constexpr size_t kBatchLdsMax = 160 * 1024;

}  // namespace

// MI355X_ATTN_GROUP (one workgroup per kv group and token), MI355X_ATTN_HEAD (one per query
// head and token: where the group's rows do not fit, the group has more than BATCH_GMAX heads,
// or mi355x_attn_prompt_impl asks for it), or MI355X_E_UNSUPPORTED where neither form's LDS fits.
static int attn_batch_lds_form(const AttnBatchArgs &b) {
    const int gsz = b.a.n_head / b.a.n_head_kv;
    if (gsz <= BATCH_GMAX && attn_batch_lds(b.a.head_dim, b.n_kv, gsz) <= kBatchLdsMax &&
        g_prompt_impl.load() == MI355X_ATTN_GROUP)
        return MI355X_ATTN_GROUP;
    if (attn_batch_lds(b.a.head_dim, b.n_kv, 1) <= kBatchLdsMax) return MI355X_ATTN_HEAD;
    return MI355X_E_UNSUPPORTED;
}

// ... or MI355X_ATTN_PATH_STREAM, the streamed form (kq_attn_stream.hip), under mi355x_attn_stream:
// mode 1 where kq_attn_batch refuses the descriptor for its size alone (the cache's, as the
// per-head kernels do, or neither LDS form fits), mode 2 for every shape the streamed kernels take.
int attn_batch_form(const AttnBatchArgs &b) {
    const int form = attn_batch_lds_form(b);
    const bool refused = attn_size_refused(b.a) || form < 0;
    if (attn_batch_stream_applies(b, refused)) return MI355X_ATTN_PATH_STREAM;
    return refused ? MI355X_E_UNSUPPORTED : form;
}

int check_attn_batch(const AttnBatchArgs &b) {
    if (!b.cells || !b.mask || b.n_tok <= 0) return MI355X_E_INVAL;
    if (b.n_kv < 32 || b.n_kv % 32 || b.n_kv > b.a.n_ctx || b.n_pos <= 0) return MI355X_E_INVAL;
    if (b.mask_row_bytes < (int64_t)b.n_kv * (b.mask_f16 ? 2 : 4)) return MI355X_E_INVAL;
    if (b.a.rope_row) return MI355X_E_INVAL;  // per-token positions: the whole rope table
    if (b.n_tok > 65535) return MI355X_E_UNSUPPORTED;  // one grid row per token
    const int form = attn_batch_form(b);  // (past the cache sizes of kq_attn_batch: the streamed form, or refused)
    return form < 0 ? form : MI355X_OK;
}

int launch_attn_batch(const AttnBatchArgs &b0, hipStream_t s) {
    int rc = check_attn_batch(b0);
    if (rc) return rc;
    AttnBatchArgs b = b0;
    const AttnArgs &a = b.a;
    const int gsz = a.n_head / a.n_head_kv;
    const int form = attn_batch_form(b);
    if (form == MI355X_ATTN_PATH_STREAM) {  // the store, then three launches per token tile
        void *ws = attn_batch_stream_buffer(b, s);
        if (!ws) return MI355X_E_WORKSPACE;  // captured without a reservation: nothing was stored
        const dim3 gs((unsigned)b.n_tok, (unsigned)a.n_head_kv);
        rc = a.head_dim == 64 ? timed_launch("kq::kq_kv_store_batch<64>", 0.0, kq_kv_store_batch<64>, gs, dim3(256), 0, s, b)
                              : timed_launch("kq::kq_kv_store_batch<128>", 0.0, kq_kv_store_batch<128>, gs, dim3(256), 0, s, b);
        return rc ? rc : launch_attn_batch_stream(b, ws, s);
    }
    b.per_head = form == MI355X_ATTN_HEAD ? 1 : 0;
    const int rows = b.per_head ? 1 : gsz;
    const size_t lds = attn_batch_lds(a.head_dim, b.n_kv, rows);
    const dim3 gs((unsigned)b.n_tok, (unsigned)a.n_head_kv);
    const dim3 ga((unsigned)(b.per_head ? a.n_head : a.n_head_kv), (unsigned)b.n_tok);
#define KQ_BATCH_LAUNCH(HD, G)                                                                                  \
    {                                                                                                         \
        allow_lds((const void *)kq_attn_batch<HD, G>, lds);                                                   \
        return timed_launch("kq::kq_attn_batch<" #HD ">", 0.0, kq_attn_batch<HD, G>, ga, dim3(256), lds, s, b);   \
    }
    if (a.head_dim == 64) {
        rc = timed_launch("kq::kq_kv_store_batch<64>", 0.0, kq_kv_store_batch<64>, gs, dim3(256), 0, s, b);
        if (rc) return rc;
        if (rows == 1) KQ_BATCH_LAUNCH(64, 1)
        if (rows == 4) KQ_BATCH_LAUNCH(64, 4)
        if (rows == 8) KQ_BATCH_LAUNCH(64, 8)
        KQ_BATCH_LAUNCH(64, 0)
    }
    rc = timed_launch("kq::kq_kv_store_batch<128>", 0.0, kq_kv_store_batch<128>, gs, dim3(256), 0, s, b);
    if (rc) return rc;
    if (rows == 1) KQ_BATCH_LAUNCH(128, 1)
    if (rows == 4) KQ_BATCH_LAUNCH(128, 4)
    if (rows == 8) KQ_BATCH_LAUNCH(128, 8)
    KQ_BATCH_LAUNCH(128, 0)
#undef KQ_BATCH_LAUNCH
}

// The descriptor -> kernel arguments, every argument check included (no device access).
// n_pos: rows of the rope table (0: n_ctx, what mi355x_attn_desc documents).
int attn_batch_args_from(const mi355x_attn_batch_desc *d, int n_pos, AttnBatchArgs &b) {
    if (!d || !d->cells || !d->mask) return MI355X_E_INVAL;
    if (d->cells_type != MI355X_TYPE_I32 && d->cells_type != MI355X_TYPE_I64) return MI355X_E_INVAL;
    if (d->mask_type != MI355X_TYPE_F16 && d->mask_type != MI355X_TYPE_F32) return MI355X_E_INVAL;
    if (d->n_tokens <= 0 || d->a.rope_row) return MI355X_E_INVAL;
    if (d->n_kv < 32 || d->n_kv % 32 || d->n_kv > d->a.n_ctx) return MI355X_E_INVAL;
    if (d->mask_row_bytes < (size_t)d->n_kv * (d->mask_type == MI355X_TYPE_F16 ? 2 : 4)) return MI355X_E_INVAL;
    const int rc = attn_args_from(&d->a, b.a);
    if (rc) return rc;
    b.cells = d->cells;
    b.mask = d->mask;
    b.mask_row_bytes = (int64_t)d->mask_row_bytes;
    b.cells_i64 = d->cells_type == MI355X_TYPE_I64;
    b.mask_f16 = d->mask_type == MI355X_TYPE_F16;
    b.n_kv = d->n_kv;
    b.n_tok = d->n_tokens;
    b.n_pos = n_pos > 0 ? n_pos : d->a.n_ctx;
    b.per_head = 0;
    return check_attn_batch(b);
}

}  // namespace kq

using namespace kq;

extern "C" {

int mi355x_attn_batch(const mi355x_attn_batch_desc *d, void *stream) {
    AttnBatchArgs b;
    const int rc = attn_batch_args_from(d, 0, b);
    if (rc) return rc;
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_attn_batch(b, (hipStream_t)stream);
}

int mi355x_attn_batch_path(const mi355x_attn_batch_desc *d) {
    AttnBatchArgs b;
    const int rc = attn_batch_args_from(d, 0, b);
    return rc ? rc : attn_batch_form(b);
}

}  // extern "C"
