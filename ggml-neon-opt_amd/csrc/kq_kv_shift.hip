// kq_kv_shift.hip — the context shift on the device: cached K rows are re-roped in place by an
// integer position delta, and (DISCARD form) the cells after a discarded stretch slide down over
// it, so a full KV cache makes room without a new prefill (llama.cpp's llama_memory_seq_rm /
// llama_memory_seq_add and its K-shift graph, build_rope_shift [U]; LlamaDecoder.shift and
// generate(keep=)).
//
// The rule is stated in include/ggml_mi355x.h (mi355x_kv_shift) and restated in
// tests/kv_shift_ref.py; the caches hold the same bits. The arithmetic is rope_pair followed by
// f2h_rne (kq_ops_device.h), what ggml_compute_forward_rope_f16 does with the cos/sin cache of
// position `delta` [U].
//
// kq_kv_shift<HD, FORM>, 256 threads a workgroup, one 16-byte vector (8 f16: 4 rope pairs) a
// thread and load. No atomics, no hand-off, no wait on another workgroup.
//   DELTAS: the vectors of cells [0, n_cells) are dealt to the threads in order (a workgroup: 256
//     consecutive vectors of the K rows). A thread issues the load of its cell's delta and of its
//     K vector together (one round trip, not the delta first), then for delta != 0 loads the 8
//     floats of table row |delta|, rotates and stores; delta == 0 stores nothing. Every thread
//     reads and writes its own 16 bytes only. V is not touched.
//   DISCARD: ownership by channel, not by cell, so that no workgroup reads what another writes
//     although source and destination cells overlap. Workgroups [0, kvw / 32) own a column of 32
//     channels (64 bytes of every K row), workgroups [kvw / 32, kvw / 32 + kvw) one channel row
//     of the transposed V cache. Each walks its destination cells [keep, n_past - discard) in
//     ascending chunks of kShiftChunk = 256 cells: it loads the chunk's sources (cells
//     c + discard), waits for them, meets at the barrier, and only then stores the chunk. A later
//     chunk reads cells above everything stored so far (discard >= 1). The table row is the same
//     for every cell: a thread loads its 8 floats once.
//     The V side moves 2 bytes a thread and chunk (a slide by an odd number of cells has no
//     common alignment), and the K side of a model with few KV heads runs few workgroups: the
//     launch is latency-bound there, far from the HBM roofline (context shift).
#include <string.h>

#include "kq_device.h"
#include "kq_internal.h"
#include "kq_ops_device.h"

namespace kq {

namespace {

constexpr int kShiftThreads = 256;
constexpr int kShiftChunk = 256;    // DISCARD: destination cells a workgroup loads before it stores them
constexpr int kShiftSliceVecs = 4;  // DISCARD, K side: 16-byte vectors (of 8 channels) a workgroup owns in every row
static_assert(kShiftChunk % (kShiftThreads / kShiftSliceVecs) == 0, "whole passes a chunk");

struct KvShiftArgs {
    uint16_t *k;         // [n_ctx][kvw]
    uint16_t *v;         // [kvw][n_ctx] (DISCARD)
    const float *table;  // [n_pos][HD / 2][cos, sin]
    const int32_t *delta;
    int kvw, n_ctx, n_pos;
    int n_cells;               // DELTAS
    int keep, discard, n_end;  // DISCARD: destination cells [keep, n_end), n_end = n_past - discard
};

// the 4 pairs of K vector `w` rotated with (cos, sin) pairs cs[0 .. 3]; neg: the sines negated
__device__ __forceinline__ uint4 shift_vec(uint4 w, const float4 &cs01, const float4 &cs23, bool neg) {
    const uint32_t in[4] = {w.x, w.y, w.z, w.w};
    const float c[4] = {cs01.x, cs01.z, cs23.x, cs23.z};
    const float s[4] = {cs01.y, cs01.w, cs23.y, cs23.w};
    uint32_t out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x0 = (float)u2h((uint16_t)in[j]), x1 = (float)u2h((uint16_t)(in[j] >> 16));
        const float2 r = rope_pair(x0, x1, c[j], neg ? -s[j] : s[j]);
        out[j] = (uint32_t)h2u(f2h_rne(r.x)) | ((uint32_t)h2u(f2h_rne(r.y)) << 16);
    }
    return make_uint4(out[0], out[1], out[2], out[3]);
}

template <int HD, int FORM>
__global__ void __launch_bounds__(kShiftThreads) kq_kv_shift(const KvShiftArgs a) {
    const int t = (int)threadIdx.x;
    if (FORM == MI355X_KV_SHIFT_DELTAS) {
        const uint32_t vpr = (uint32_t)a.kvw / 8;  // vectors a row
        const uint32_t vi = blockIdx.x * kShiftThreads + t;  // (n_cells * vpr < 2^31: the launcher's check)
        if (vi >= (uint32_t)a.n_cells * vpr) return;
        const uint32_t cell = vi / vpr, col = vi % vpr;
        uint4 *p = (uint4 *)(a.k + (int64_t)cell * a.kvw) + col;
        // the delta with the row, not ahead of it: the fence (no instruction) keeps the compiler from
        // sinking the row's load behind the test of the delta, a dependent round trip later (so a
        // delta-0 cell's row is read, never written)
        const int32_t d = a.delta[cell];
        const uint4 w = *p;
        wave_lds_fence();
        if (d == 0) return;
        const uint32_t ad = d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
        if (ad >= (uint32_t)a.n_pos) {  // outside the table: NaN, never a silent result
            *p = make_uint4(0x7e007e00u, 0x7e007e00u, 0x7e007e00u, 0x7e007e00u);
            return;
        }
        const float4 *cs = (const float4 *)(a.table + ((int64_t)ad * (HD / 2) + (col * 8 % HD) / 2) * 2);
        *p = shift_vec(w, cs[0], cs[1], d < 0);
        return;
    }
    const int nk = a.kvw / (8 * kShiftSliceVecs);
    if ((int)blockIdx.x < nk) {  // a column of 32 channels of K
        constexpr int kCellsPass = kShiftThreads / kShiftSliceVecs, kPasses = kShiftChunk / kCellsPass;
        const int col = (int)blockIdx.x * kShiftSliceVecs + (t % kShiftSliceVecs);
        const float4 *cs = (const float4 *)(a.table + ((int64_t)a.discard * (HD / 2) + (col * 8 % HD) / 2) * 2);
        const float4 cs01 = cs[0], cs23 = cs[1];
        for (int c0 = a.keep; c0 < a.n_end; c0 += kShiftChunk) {
            uint4 w[kPasses];
#pragma unroll
            for (int j = 0; j < kPasses; ++j) {
                const int cell = c0 + j * kCellsPass + t / kShiftSliceVecs;
                w[j] = make_uint4(0, 0, 0, 0);
                if (cell < a.n_end) w[j] = *((const uint4 *)(a.k + (int64_t)(cell + a.discard) * a.kvw) + col);
            }
#pragma unroll
            for (int j = 0; j < kPasses; ++j) w[j] = shift_vec(w[j], cs01, cs23, true);
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's sources have landed
            __syncthreads();                     // ... and every wave's: the chunk may be overwritten
#pragma unroll
            for (int j = 0; j < kPasses; ++j) {
                const int cell = c0 + j * kCellsPass + t / kShiftSliceVecs;
                if (cell < a.n_end) *((uint4 *)(a.k + (int64_t)cell * a.kvw) + col) = w[j];
            }
        }
        return;
    }
    // a channel row of V: cell c takes cell c + discard
    uint16_t *row = a.v + (int64_t)((int)blockIdx.x - nk) * a.n_ctx;
    for (int c0 = a.keep; c0 < a.n_end; c0 += kShiftChunk) {
        const int cell = c0 + t;
        uint16_t x = 0;
        if (cell < a.n_end) x = row[cell + a.discard];
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        __syncthreads();
        if (cell < a.n_end) row[cell] = x;
    }
}

}  // namespace

int launch_kv_shift(const mi355x_kv_shift_desc *d, hipStream_t stream) {
    if (!d || (d->form != MI355X_KV_SHIFT_DELTAS && d->form != MI355X_KV_SHIFT_DISCARD)) return MI355X_E_INVAL;
    const bool deltas = d->form == MI355X_KV_SHIFT_DELTAS;
    if (!d->k_cache || !d->rope_table || (deltas ? !d->delta : !d->v_cache)) return MI355X_E_INVAL;
    if (((uintptr_t)d->k_cache & 15u) || ((uintptr_t)d->rope_table & 15u) || ((uintptr_t)d->delta & 3u) ||
        ((uintptr_t)d->v_cache & 1u))
        return MI355X_E_INVAL;
    if (d->n_ctx < 1 || d->n_head_kv < 1 || d->n_pos < 1 || d->head_dim < 1) return MI355X_E_INVAL;
    if (deltas) {
        if (d->n_cells < 0 || d->n_cells > d->n_ctx) return MI355X_E_INVAL;
    } else if (d->keep < 0 || d->discard < 1 || (int64_t)d->keep + d->discard > d->n_past || d->n_past > d->n_ctx ||
               d->discard >= d->n_pos) {
        return MI355X_E_INVAL;
    }
    if (d->head_dim != 64 && d->head_dim != 128) return MI355X_E_UNSUPPORTED;
    if ((int64_t)d->n_head_kv * d->head_dim > 0x7fffffff) return MI355X_E_UNSUPPORTED;
    KvShiftArgs a;
    memset(&a, 0, sizeof(a));
    a.k = d->k_cache;
    a.v = d->v_cache;
    a.table = d->rope_table;
    a.delta = d->delta;
    a.kvw = d->n_head_kv * d->head_dim;
    a.n_ctx = d->n_ctx;
    a.n_pos = d->n_pos;
    const double row_bytes = 2.0 * a.kvw;
    if (deltas) {
        if (d->n_cells == 0) return MI355X_OK;  // nothing to shift: no launch
        if (!device_ok()) return MI355X_E_NODEVICE;
        a.n_cells = d->n_cells;
        const int64_t vecs = (int64_t)a.n_cells * (a.kvw / 8);
        if (vecs > 0x7fffffff) return MI355X_E_UNSUPPORTED;  // (the kernel's 32-bit vector index)
        const dim3 grid((unsigned)((vecs + kShiftThreads - 1) / kShiftThreads));
        const double bytes = (double)a.n_cells * (4.0 + 2.0 * row_bytes);  // every row read and written
        return d->head_dim == 64
                   ? timed_launch("kq::kq_kv_shift<64, deltas>", bytes, kq_kv_shift<64, MI355X_KV_SHIFT_DELTAS>, grid,
                                  dim3(kShiftThreads), 0, stream, a)
                   : timed_launch("kq::kq_kv_shift<128, deltas>", bytes, kq_kv_shift<128, MI355X_KV_SHIFT_DELTAS>, grid,
                                  dim3(kShiftThreads), 0, stream, a);
    }
    a.keep = d->keep;
    a.discard = d->discard;
    a.n_end = d->n_past - d->discard;
    if (a.n_end <= a.keep) return MI355X_OK;  // no cell moves: no launch
    if (!device_ok()) return MI355X_E_NODEVICE;
    const dim3 grid((unsigned)(a.kvw / (8 * kShiftSliceVecs) + a.kvw));
    const double bytes = (double)(a.n_end - a.keep) * 4.0 * row_bytes;  // K and V cells, each read and written
    return d->head_dim == 64
               ? timed_launch("kq::kq_kv_shift<64, discard>", bytes, kq_kv_shift<64, MI355X_KV_SHIFT_DISCARD>, grid,
                              dim3(kShiftThreads), 0, stream, a)
               : timed_launch("kq::kq_kv_shift<128, discard>", bytes, kq_kv_shift<128, MI355X_KV_SHIFT_DISCARD>, grid,
                              dim3(kShiftThreads), 0, stream, a);
}

}  // namespace kq

extern "C" {

int mi355x_kv_shift(const mi355x_kv_shift_desc *d, void *stream) { return kq::launch_kv_shift(d, (hipStream_t)stream); }

}  // extern "C"
