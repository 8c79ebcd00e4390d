// kq_logprob.hip — log-probabilities on the device: for every row of an f32 matrix of logits and
// a target index per row, the exact ingredients of log softmax(x)[target] (the record of
// include/ggml_mi355x.h, struct mi355x_logprob), so that scoring a text copies 24 bytes a token to
// the host instead of a row of the vocabulary (LlamaDecoder.logprobs, .perplexity).
//
// The rule is stated in include/ggml_mi355x.h (mi355x_logprob_rows) and restated in
// tests/logprob_ref.py; the record is the same bit for bit. The logarithm stays on the host
// (mi355x_logprob_value): the device's log is not correctly rounded.
//
// Two launches in stream order, and no workgroup ever waits for another.
//   1. kq_argmax_rows, plain form: row i's index a goes to 4 bytes of the row's own counter line
//      in the workspace (kLogprobArgmaxAt), where no other row's workgroup reads or writes.
//   2. kq_logsum_rows, grid (ceil(n / 1024), rows): workgroup b of a row owns entries
//      [1024 b, 1024 b + 1024), one subtree of the rule's tree of 65536 quads. Lane t loads the
//      block's 16-byte vector t (the row's last, partial vector by scalar loads, its missing
//      entries +0.0f), reads m = x[a], forms its quad sum in f32 and converts it to f64; the 8
//      tree levels inside the block are steps between adjacent lanes: DPP within a row of 16 on
//      the two halves of the double, the lane swaps across rows (sblk_sum, kq_rows_device.h),
//      then LDS across the 4 waves in the tree's order. Every node is one f64 add.
//      Hand-off: kq_argmax's, on the same arrive_last (kq_argmax_device.h; MI355X_MICROARCH.md,
//      valid forms, row 1): the block's sum stored write-through (sc1) by one lane, drained,
//      barrier, one agent-scope add on the row's counter; the last arriver reads all block sums
//      (sc1 loads behind the barrier; absent blocks +0.0), finishes the tree over 256 slots the
//      same way, writes the record and has stored 0 back to the counter.
// Both launches use the one workspace of argmax_rows_workspace's layout: they are ordered on the
// stream, and launch 2 overwrites the words launch 1 is done with.
#include <string.h>

#include "kq_argmax_device.h"
#include "kq_device.h"
#include "kq_internal.h"
#include "kq_ops_device.h"
#include "kq_rows_device.h"

namespace kq {

namespace {

constexpr int kLogsumBlock = 4 * kArgmaxThreads;  // entries per workgroup: one 16-byte vector a lane
static_assert((kLogprobMaxN + kLogsumBlock - 1) / kLogsumBlock <= kArgmaxMaxWgs,
              "one block sum per thread of the last arriver");
static_assert(kLogprobMaxN / 4 == 256 * kArgmaxMaxWgs, "the rule's tree: 65536 quads, 256 a block");
// a row's argmax in its counter line: the counter is the line's first word, the rest is unused
constexpr size_t kLogprobArgmaxAt = 64;
static_assert(kLogprobArgmaxAt + 4 <= kArgmaxCounterBytes && kArgmaxRowBytes % 4 == 0, "inside the row's counter line");

struct LogsumArgs {
    const float *x;
    int64_t row_stride;  // floats between two rows
    int n;
    const int32_t *targets;  // [rows]
    uint8_t *ws;             // per row kArgmaxRowBytes: the counter's line (the argmax in it), then the block sums
    mi355x_logprob *out;     // [rows]
};

// The sum of v over the workgroup as the rule's tree over its 256 threads (thread t leaf t), in
// every thread: the wave's 6 levels, then (w0 + w1) + (w2 + w3); `lds`: 4 doubles, free on entry
__device__ __forceinline__ double block_tree_sum(double v, double *lds) {
    v = sblk_sum<64>(v);
    if (((int)threadIdx.x & 63) == 0) lds[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__device__ __forceinline__ float exp_term(float x, float m) {
    const float d = x - m;
    return d == -INFINITY ? 0.0f : v_expf(d);
}

__global__ void __launch_bounds__(kArgmaxThreads) kq_logsum_rows(const LogsumArgs p) {
    __shared__ double red[4];
    __shared__ int flag;
    const int t = (int)threadIdx.x, blk = (int)blockIdx.x, nblk = (int)gridDim.x;
    const int64_t row = (int64_t)blockIdx.y;
    const float *x = p.x + row * p.row_stride;
    uint8_t *rw = p.ws + (size_t)row * kArgmaxRowBytes;
    uint32_t *cnt = (uint32_t *)rw;
    unsigned long long *part = (unsigned long long *)(rw + kArgmaxCounterBytes);
    const uint32_t a0 = *(const uint32_t *)(rw + kLogprobArgmaxAt);
    const int a = a0 < (uint32_t)p.n ? (int)a0 : 0;  // (kq_argmax_rows' index is inside the row)
    const float m = x[a];

    // ---- this lane's quad: entries [i0, i0 + 4) of the row, those from n on +0.0f
    const int i0 = blk * kLogsumBlock + 4 * t;
    float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, e3 = 0.0f;
    if (i0 + 4 <= p.n) {
        const f32x4 v = *(const f32x4 *)(x + i0);
        e0 = exp_term(v.x, m), e1 = exp_term(v.y, m), e2 = exp_term(v.z, m), e3 = exp_term(v.w, m);
    } else {  // the row's last, partial vector (or past the row)
        if (i0 < p.n) e0 = exp_term(x[i0], m);
        if (i0 + 1 < p.n) e1 = exp_term(x[i0 + 1], m);
        if (i0 + 2 < p.n) e2 = exp_term(x[i0 + 2], m);
    }
    const float q = (e0 + e1) + (e2 + e3);
    const double bsum = block_tree_sum((double)q, red);

    // ---- the block's sum write-through, then the arrival; the last arriver goes on
    if (t == 0)
        __hip_atomic_store(part + blk, __builtin_bit_cast(unsigned long long, bsum), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (!arrive_last(cnt, nblk, &flag)) return;

    // ---- the last arriver: every block's sum (nblk <= 256: one per thread), sc1 loads; the
    // tree's upper 8 levels (every thread is past its read of red: arrive_last's barriers)
    const unsigned long long w = t < nblk ? __hip_atomic_load(part + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    const double S = block_tree_sum(__builtin_bit_cast(double, w), red);
    if (t != 0) return;
    const uint32_t tg = (uint32_t)p.targets[row];
    mi355x_logprob r;
    r.max = m;
    r.x_target = tg < (uint32_t)p.n ? x[tg] : __uint_as_float(0x7fc00000u);
    r.argmax = a;
    r.pad = 0;
    r.sum = S;
    p.out[row] = r;
}

}  // namespace

size_t logprob_workspace(int64_t n, int64_t rows) {
    return n > kLogprobMaxN ? 0 : argmax_rows_workspace(n, rows);
}

int launch_logprob_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, const int32_t *targets,
                        mi355x_logprob *out, void *ws, size_t ws_size, hipStream_t stream) {
    if (!targets || ((uintptr_t)targets & 3u) || !out || ((uintptr_t)out & 7u) || n > kLogprobMaxN ||
        !input_ok(x, n, rows, row_stride, nullptr, nullptr))
        return MI355X_E_INVAL;
    if (const int rc = workspace_status(ws, ws_size, logprob_workspace(n, rows))) return rc;
    if (const int rc = launch_argmax_rows(x, n, rows, row_stride, (int32_t *)((uint8_t *)ws + kLogprobArgmaxAt), nullptr, ws,
                                          ws_size, stream, (int64_t)(kArgmaxRowBytes / 4)))
        return rc;
    LogsumArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x;
    p.row_stride = row_stride;
    p.n = (int)n;
    p.targets = targets;
    p.ws = (uint8_t *)ws;
    p.out = out;
    const unsigned nblk = (unsigned)((n + kLogsumBlock - 1) / kLogsumBlock);
    return timed_launch("kq::kq_logsum_rows", (double)rows * (double)n * 4.0, kq_logsum_rows, dim3(nblk, (unsigned)rows),
                        dim3(kArgmaxThreads), 0, stream, p);
}

}  // namespace kq

extern "C" {

size_t mi355x_logprob_workspace_size(int64_t n, int64_t rows) { return kq::logprob_workspace(n, rows); }

int mi355x_logprob_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, const int32_t *targets,
                        struct mi355x_logprob *out, void *workspace, size_t workspace_size, void *stream) {
    return kq::launch_logprob_rows(x, n, rows, row_stride, targets, out, workspace, workspace_size, (hipStream_t)stream);
}

}  // extern "C"
