// kq_argmax.hip — greedy sampling on the device: the argmax of an f32 vector (the logits)
// in ONE launch over several workgroups, and, in its step-inputs form, the next decode
// token's inputs (token id, position, the position's rope row) written where the decode
// graph reads them, so the same captured graph is replayed token after token with no host
// copy and no synchronization in between (LlamaDecoder.generate).
//
// Semantics (llama.cpp's greedy sampler; numpy.argmax(where(isnan(x), -inf, x))): the
// smallest index whose value equals the maximum of the non-NaN entries under IEEE
// comparison. -0.0 == +0.0, +-inf are ordinary values, a NaN never wins, all NaN -> 0; the
// result is always in [0, n). Exact: the order is carried by an integer key, no arithmetic.
//
// Key. A value's bits become an ordered 32-bit key (NaN -> 0, below every number; -0.0 ->
// +0.0 first; negative: all bits flipped, else the sign bit set), and (key << 32) | ~index is
// a 64-bit word whose unsigned maximum is the answer: the larger value, then the smaller index.
//
// Decomposition. Workgroup s reduces slice [s * slice, min(n, (s + 1) * slice)) (16-B loads;
// the vector's last, partial 16 bytes by scalar loads): each lane over its vectors in index
// order, DPP within a row of 16 lanes, the lane swaps across rows, LDS across the waves.
// Hand-off (kq_attn_oproj's; MI355X_MICROARCH.md, valid forms, row 1): the workgroup's word
// is stored write-through (sc1) by one lane, that wave drains it (vmcnt(0)), workgroup
// barrier, ONE agent-scope add on the counter; the workgroup whose add returns wgs - 1 reads
// every word with sc1 loads behind a workgroup barrier, reduces them the same way and writes
// the result. It stores 0 back to the counter, so every launch and every graph replay
// starts at 0. No workgroup waits for another: nothing can deadlock, placement only changes speed.
//
// Rows. kq_argmax_rows is the same reduction over each of T rows of a matrix in one launch, grid
// (workgroups per row, T): a row is split as argmax_plan splits a vector of its length and handed
// off on a counter of its own, so the rows never meet. Its step-inputs form ends one step of
// several sequences (LlamaDecoder.generate_batch): the last arriver of row i writes the
// sequence's next token, position and cell where the batch graph reads them, makes that cell
// visible in the row's own mask and files the token in the row's history.
#include <string.h>

#include "kq_argmax_device.h"
#include "kq_internal.h"
#include "kq_rows_device.h"

namespace kq {

namespace {

constexpr int kArgmaxSlice = 1024;  // entries per workgroup up to 256 workgroups (ARGMAX_SLICE: A/B)

struct ArgmaxArgs {
    const float *x;
    int n, slice, wgs;
    unsigned long long *part;  // workspace: one word per workgroup ...
    uint32_t *cnt;             // ... behind the arrival counter
    int32_t *out;              // plain form: [1]; step form: the decoder's input block [2 + hd]
    TokenStepArgs step;
};

__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const uint32_t hi =
        (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(v >> 32), (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)hi << 32) | lo;
}

// The maximum over the wave, in every lane (every lane active): row16_reduce's DPP steps,
// then the rows by the lane swaps (sblk_reduce's, kq_rows_device.h)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = max_u64(v, dpp_u64<0xB1>(v));
    v = max_u64(v, dpp_u64<0x4E>(v));
    v = max_u64(v, dpp_u64<0x141>(v));
    v = max_u64(v, dpp_u64<0x140>(v));
    uint32_t la, lb, ha, hb;
    swap_rows16((uint32_t)v, la, lb), swap_rows16((uint32_t)(v >> 32), ha, hb);
    v = max_u64(((unsigned long long)ha << 32) | la, ((unsigned long long)hb << 32) | lb);
    swap_rows32((uint32_t)v, la, lb), swap_rows32((uint32_t)(v >> 32), ha, hb);
    return max_u64(((unsigned long long)ha << 32) | la, ((unsigned long long)hb << 32) | lb);
}

// ... over the workgroup's 4 waves, in every thread; `lds`: 4 words no other reduction uses
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long *lds) {
    v = wave_max_u64(v);
    if (((int)threadIdx.x & 63) == 0) lds[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    return max_u64(max_u64(lds[0], lds[1]), max_u64(lds[2], lds[3]));
}

// The word of slice [lo, hi) of x (lo % 4 == 0, x 16-B aligned; hi % 4 != 0 only at x's end), in
// every thread of the workgroup
__device__ __forceinline__ unsigned long long slice_word(const float *x, int lo, int hi) {
    __shared__ unsigned long long red[4];
    const int t = (int)threadIdx.x;
    // ---- this lane's vectors lo/4 + t, + 256, ... in index order: a strict > keeps the first
    uint32_t bestk = 0u, besti = 0xffffffffu;  // (no entry: the word 0, below every entry's)
    const int vfull = hi >> 2;  // vectors [lo/4, vfull) are whole
    for (int v0 = (lo >> 2) + t; v0 < vfull; v0 += 4 * kArgmaxThreads) {
        u32x4 r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v0 + j * kArgmaxThreads < vfull) r[j] = *(const u32x4 *)(x + 4 * (int64_t)(v0 + j * kArgmaxThreads));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (v0 + j * kArgmaxThreads >= vfull) break;
            const uint32_t i0 = 4u * (uint32_t)(v0 + j * kArgmaxThreads);
            const uint32_t k0 = ord_key(r[j].x), k1 = ord_key(r[j].y), k2 = ord_key(r[j].z), k3 = ord_key(r[j].w);
            if (k0 > bestk) bestk = k0, besti = i0;
            if (k1 > bestk) bestk = k1, besti = i0 + 1;
            if (k2 > bestk) bestk = k2, besti = i0 + 2;
            if (k3 > bestk) bestk = k3, besti = i0 + 3;
        }
    }
    // the vector's last n % 4 entries (the last slice only), after every whole vector of the slice
    if (t == kArgmaxThreads - 1)
        for (int i = 4 * vfull; i < hi; ++i) {
            const uint32_t k = ord_key(__float_as_uint(x[i]));
            if (k > bestk) bestk = k, besti = (uint32_t)i;
        }
    return block_max_u64(((unsigned long long)bestk << 32) | (uint32_t)~besti, red);
}

// Hand-off of this workgroup's word `w` (word `wg` of `part`) on the counter `cnt` that `wgs`
// workgroups count in on. False in every thread of a workgroup that is not the last arriver; in
// the last arriver's threads true, and *token = the index of the maximum over all the words.
__device__ __forceinline__ bool hand_off(unsigned long long w, unsigned long long *part, uint32_t *cnt, int wg, int wgs,
                                         int n, int32_t *token) {
    __shared__ unsigned long long red[4];
    __shared__ int flag;
    const int t = (int)threadIdx.x;
    // ---- the word write-through, then the arrival; the last arriver goes on
    if (t == 0) __hip_atomic_store(part + wg, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!arrive_last(cnt, wgs, &flag)) return false;

    // ---- the last arriver: every workgroup's word (wgs <= 256: one per thread), sc1 loads
    w = t < wgs ? __hip_atomic_load(part + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    w = block_max_u64(w, red);
    const uint32_t idx = ~(uint32_t)w;
    *token = idx < (uint32_t)n ? (int32_t)idx : 0;  // (all NaN: the word 0)
    return true;
}

__global__ void __launch_bounds__(kArgmaxThreads) kq_argmax(const ArgmaxArgs p) {
    const int t = (int)threadIdx.x;
    const int lo = (int)blockIdx.x * p.slice;  // (lo < n: wgs = ceil(n / slice))
    const int hi = p.n - lo < p.slice ? p.n : lo + p.slice;
    int32_t token;
    if (!hand_off(slice_word(p.x, lo, hi), p.part, p.cnt, (int)blockIdx.x, p.wgs, p.n, &token)) return;
    if (!p.step.pos) {
        if (t == 0) p.out[0] = token;
        return;
    }
    const uint32_t next = p.step.next();
    __syncthreads();  // pos may be out + 1: every thread has read it before one of them writes it
    p.step.write(p.out, next, token);
}

struct ArgmaxRowsArgs {
    const float *x;
    int64_t row_stride;  // floats between two rows
    int n, slice, wgs;
    uint8_t *ws;         // workspace, per row (kArgmaxRowBytes): the counter's line, then the row's words
    int32_t *out;        // [T]: the rows' indices (step form: the sequences' next tokens)
    RowsStepArgs step;
    int64_t out_stride;  // plain form: entries of out between two rows' indices
};

__global__ void __launch_bounds__(kArgmaxThreads) kq_argmax_rows(const ArgmaxRowsArgs p) {
    const int64_t row = (int64_t)blockIdx.y;
    const int lo = (int)blockIdx.x * p.slice;  // (lo < n: wgs = ceil(n / slice))
    const int hi = p.n - lo < p.slice ? p.n : lo + p.slice;
    uint32_t *cnt = (uint32_t *)(p.ws + (size_t)row * kArgmaxRowBytes);
    unsigned long long *part = (unsigned long long *)((uint8_t *)cnt + kArgmaxCounterBytes);
    int32_t token;
    if (!hand_off(slice_word(p.x + row * p.row_stride, lo, hi), part, cnt, (int)blockIdx.x, p.wgs, p.n, &token)) return;
    if (threadIdx.x != 0) return;
    if (!p.step.pos) {
        p.out[row * p.out_stride] = token;
        return;
    }
    uint32_t np, nc;
    p.step.next(row, np, nc);
    p.step.write(p.out, row, np, nc, token);
}

}  // namespace

int argmax_plan(int64_t n, int *workgroups, int64_t *slice) {
    if (n < 1 || n > kArgmaxMaxN) return MI355X_E_INVAL;
    int64_t s = (int64_t)knob(KNOB_ARGMAX_SLICE);
    s = s > 0 ? (s + 3) & ~(int64_t)3 : kArgmaxSlice;
    if ((n + s - 1) / s > kArgmaxMaxWgs) s = ((n + kArgmaxMaxWgs - 1) / kArgmaxMaxWgs + 3) & ~(int64_t)3;
    if (workgroups) *workgroups = (int)((n + s - 1) / s);
    if (slice) *slice = s;
    return MI355X_OK;
}

size_t argmax_workspace(int64_t n) {
    int wgs = 0;
    if (argmax_plan(n, &wgs, nullptr) != MI355X_OK) return 0;
    // (the words of every split a knob can select: the size depends on n alone)
    return kArgmaxCounterBytes + 8 * (size_t)(n < kArgmaxMaxWgs ? n : kArgmaxMaxWgs);
}

int launch_argmax(const float *x, int64_t n, int32_t *out, const ArgmaxStep *step, void *ws, size_t ws_size,
                  hipStream_t stream) {
    int wgs = 0;
    int64_t slice = 0;
    if (!out || !input_ok(x, n, 1, (n + 3) & ~(int64_t)3, &wgs, &slice) || (step && !step_ok(*step))) return MI355X_E_INVAL;
    if (const int rc = workspace_status(ws, ws_size, argmax_workspace(n))) return rc;
    ArgmaxArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x;
    p.n = (int)n;
    p.slice = (int)slice;
    p.wgs = wgs;
    p.cnt = (uint32_t *)ws;
    p.part = (unsigned long long *)((uint8_t *)ws + kArgmaxCounterBytes);
    p.out = out;
    if (step) p.step = step_args(*step);
    return timed_launch("kq::kq_argmax", (double)n * 4.0, kq_argmax, dim3((unsigned)wgs), dim3(kArgmaxThreads), 0, stream,
                        p);
}

size_t argmax_rows_workspace(int64_t n, int64_t rows) {
    if (argmax_plan(n, nullptr, nullptr) != MI355X_OK || rows < 1 || rows > kArgmaxMaxRows) return 0;
    return (size_t)rows * kArgmaxRowBytes;
}

int launch_argmax_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int32_t *out,
                       const ArgmaxRowsStep *step, void *ws, size_t ws_size, hipStream_t stream, int64_t out_stride) {
    int wgs = 0;
    int64_t slice = 0;
    if (!out || out_stride < 1 || !input_ok(x, n, rows, row_stride, &wgs, &slice) || (step && !step_ok(*step)))
        return MI355X_E_INVAL;
    if (const int rc = workspace_status(ws, ws_size, argmax_rows_workspace(n, rows))) return rc;
    ArgmaxRowsArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x;
    p.row_stride = row_stride;
    p.n = (int)n;
    p.slice = (int)slice;
    p.wgs = wgs;
    p.ws = (uint8_t *)ws;
    p.out = out;
    p.out_stride = out_stride;
    if (step) p.step = step_args(*step);
    return timed_launch("kq::kq_argmax_rows", (double)rows * (double)n * 4.0, kq_argmax_rows,
                        dim3((unsigned)wgs, (unsigned)rows), dim3(kArgmaxThreads), 0, stream, p);
}

}  // namespace kq

extern "C" {

int mi355x_argmax_plan(int64_t n, int *workgroups, int64_t *slice) { return kq::argmax_plan(n, workgroups, slice); }

size_t mi355x_argmax_workspace_size(int64_t n) { return kq::argmax_workspace(n); }

int mi355x_argmax(const float *x, int64_t n, int32_t *out, void *workspace, size_t workspace_size, void *stream) {
    return kq::launch_argmax(x, n, out, nullptr, workspace, workspace_size, (hipStream_t)stream);
}

size_t mi355x_argmax_rows_workspace_size(int64_t n, int64_t rows) { return kq::argmax_rows_workspace(n, rows); }

int mi355x_argmax_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int32_t *out, void *workspace,
                       size_t workspace_size, void *stream) {
    return kq::launch_argmax_rows(x, n, rows, row_stride, out, nullptr, workspace, workspace_size, (hipStream_t)stream);
}

}  // extern "C"
