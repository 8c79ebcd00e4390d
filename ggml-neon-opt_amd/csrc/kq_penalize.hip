// kq_penalize.hip — the sampler's penalties and logit bias on the device: every row of an f32
// matrix of logits is edited in place before the top-k (kq_sample.hip) reads it, from the row's
// window of the tokens generated so far (the history the step-inputs nodes write) and a list of
// (token, bias) pairs, so a penalised token costs one short launch and no host copy
// (LlamaDecoder.generate with an editing Sampler).
//
// The rule is stated in include/ggml_mi355x.h (mi355x_penalize_rows) and restated in
// tests/penalize_ref.py; the edited row is the same bit for bit. The arithmetic is plain C++:
// the build's -ffp-contract=off keeps the multiply, the add and the subtract apart and its f32
// division is correctly rounded.
//
// kq_penalize_rows, grid (rows), one workgroup of 256 threads a row. No atomics, no hand-off, no
// wait on another workgroup; every loop is bounded by last_n and n_bias.
//   1. The workgroup loads the row's window (<= 1024 ids) and the bias list (<= 256 ids and
//      values) into LDS, an id outside [0, n) as -1, both padded with -1 to whole 16-byte
//      vectors; one barrier.
//   2. Window owner: the thread that holds window entry j (j = t, t + 256, ...) owns its token
//      when no entry i < j holds the same token. One scan of the window counts the token's
//      occurrences before j and in all (a wave holds 64 consecutive entries: only in their
//      stretch of the window the scan compares places); the owner then loads x[t], adds the
//      token's biases in list order, applies the penalties and stores.
//   3. Bias owner: the thread that holds bias entry k owns its token when no k' < k holds the
//      same token and the token is not in the window. It adds the biases alone.
// Every distinct token therefore has exactly one owner, which is the only thread that reads or
// writes x[token]: nothing in global memory is read after another thread's store.
// The scans read 16 bytes of LDS at an address that is the same in every lane (a broadcast): no
// bank conflicts (MI355X_MICROARCH.md, LDS).
#include <cmath>
#include <string.h>

#include "kq_device.h"
#include "kq_internal.h"

namespace kq {

namespace {

constexpr int kPenalizeThreads = 256;
static_assert(kPenaltyMaxLastN % kPenalizeThreads == 0 && kLogitBiasMax == kPenalizeThreads,
              "whole window entries a thread, one bias entry a thread");

struct PenalizeArgs {
    float *x;
    int64_t row_stride;   // floats between two rows
    const int32_t *hist;  // [rows][hist_stride], n_hist entries of a row in use
    int64_t hist_stride;
    const int32_t *end;  // [rows]
    const int32_t *bias_tok;
    const float *bias_val;
    uint32_t n;
    int n_hist, last_n, n_bias;
    float repeat, freq, present;
};

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// how many of the padded list's entries [lo, hi) equal tok (lo, hi: multiples of 4, the same in
// every lane; every lane reads the same 16 bytes)
__device__ __forceinline__ int matches(const int32_t *lds, int lo, int hi, int32_t tok) {
    int c = 0;
#pragma unroll 4
    for (int i = lo; i < hi; i += 4) {
        const i32x4 w = *(const i32x4 *)(lds + i);
        c += ((w.x == tok) + (w.y == tok)) + ((w.z == tok) + (w.w == tok));
    }
    return c;
}

// how many of the padded list's entries [0, len4) equal tok, and how many of those stand before
// entry j. The wave's lanes hold the 64 consecutive entries from `base` (a multiple of 64, the
// same in every lane): only in that stretch the entry's place is compared, lane by lane.
__device__ __forceinline__ void count_in(const int32_t *lds, int len4, int32_t tok, int j, int base, int &before, int &all) {
    base = __builtin_amdgcn_readfirstlane(base);
    const int m0 = base < len4 ? base : len4, m1 = base + 64 < len4 ? base + 64 : len4;
    const int head = matches(lds, 0, m0, tok);
    int b = head, c = head;
    for (int i = m0; i < m1; i += 4) {
        const i32x4 w = *(const i32x4 *)(lds + i);
        const int e0 = w.x == tok, e1 = w.y == tok, e2 = w.z == tok, e3 = w.w == tok;
        c += (e0 + e1) + (e2 + e3);
        b += ((e0 & (i < j)) + (e1 & (i + 1 < j))) + ((e2 & (i + 2 < j)) + (e3 & (i + 3 < j)));
    }
    before = b;
    all = c + matches(lds, m1, len4, tok);
}

// v plus the biases of tok among the padded list's entries [0, nb4), in list order (a padding
// entry's token is -1: never tok)
__device__ __forceinline__ float add_biases(float v, const int32_t *btok, const float *bval, int nb4, int32_t tok) {
#pragma unroll 2
    for (int k = 0; k < nb4; k += 4) {
        const i32x4 t = *(const i32x4 *)(btok + k);
        const f32x4 b = *(const f32x4 *)(bval + k);
        if (t.x == tok) v = v + b.x;
        if (t.y == tok) v = v + b.y;
        if (t.z == tok) v = v + b.z;
        if (t.w == tok) v = v + b.w;
    }
    return v;
}

__global__ void __launch_bounds__(kPenalizeThreads) kq_penalize_rows(const PenalizeArgs p) {
    __shared__ __attribute__((aligned(16))) int32_t win[kPenaltyMaxLastN];
    __shared__ __attribute__((aligned(16))) int32_t btok[kLogitBiasMax];
    __shared__ __attribute__((aligned(16))) float bval[kLogitBiasMax];
    const int t = (int)threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x;
    float *x = p.x + row * p.row_stride;

    // ---- the window: history entries [lo, hi] of the row, inside [0, n_hist) whatever end is
    int len = 0;
    int64_t lo = 0;
    if (p.last_n > 0) {
        const int64_t e = (int64_t)p.end[row];
        const int64_t hi = e < (int64_t)p.n_hist - 1 ? e : (int64_t)p.n_hist - 1;
        lo = e - p.last_n + 1 > 0 ? e - p.last_n + 1 : 0;
        if (hi >= lo) len = (int)(hi - lo + 1);  // <= last_n
    }
    const int len4 = (len + 3) & ~3, nb4 = (p.n_bias + 3) & ~3;
    const int32_t *hist = p.hist + row * p.hist_stride + lo;
    for (int j = t; j < len4; j += kPenalizeThreads) {
        const int32_t v = j < len ? hist[j] : -1;
        win[j] = (uint32_t)v < p.n ? v : -1;
    }
    if (t < nb4) {
        const int32_t v = t < p.n_bias ? p.bias_tok[t] : -1;
        btok[t] = (uint32_t)v < p.n ? v : -1;
        bval[t] = t < p.n_bias ? p.bias_val[t] : 0.0f;
    }
    __syncthreads();

    // ---- window owners: biases, then the penalties
    for (int j = t; j < len; j += kPenalizeThreads) {
        const int32_t tok = win[j];
        int before, c;
        count_in(win, len4, tok, j, j - (t & 63), before, c);
        if (tok < 0 || before) continue;
        float v = add_biases(x[tok], btok, bval, nb4, tok);
        v = v <= 0.0f ? v * p.repeat : v / p.repeat;
        const float cost = (float)c * p.freq + p.present;
        x[tok] = v - cost;
    }
    // ---- bias owners: the tokens no window entry holds
    if (t < p.n_bias) {
        const int32_t tok = btok[t];
        int before, c;
        count_in(btok, nb4, tok, t, t & ~63, before, c);
        // (no entry before t holds tok: the whole list's biases of tok are those from t on)
        if (tok >= 0 && !before && !matches(win, 0, len4, tok)) x[tok] = add_biases(x[tok], btok, bval, nb4, tok);
    }
}

}  // namespace

bool penalties_ok(const mi355x_penalties *p, int n_bias) {
    return p && p->last_n >= 0 && p->last_n <= kPenaltyMaxLastN && std::isfinite(p->repeat) && p->repeat > 0.0f &&
           std::isfinite(p->freq) && std::isfinite(p->present) && n_bias >= 0 && n_bias <= kLogitBiasMax;
}

int launch_penalize_rows(float *x, int64_t n, int64_t rows, int64_t row_stride, const mi355x_penalties *pen,
                         const int32_t *hist, int64_t hist_stride, int64_t n_hist, const int32_t *end,
                         const int32_t *bias_tok, const float *bias_val, int n_bias, hipStream_t stream) {
    if (!x || ((uintptr_t)x & 3u) || !pen || n < 1 || n > kArgmaxMaxN || rows < 1 || rows > kArgmaxMaxRows || row_stride < n)
        return MI355X_E_INVAL;
    if (!penalties_ok(pen, n_bias)) return MI355X_E_INVAL;
    if (pen->last_n > 0 && (!hist || !end || n_hist < 1 || n_hist > 0x7fffffff || hist_stride < n_hist)) return MI355X_E_INVAL;
    if (n_bias > 0 && (!bias_tok || !bias_val)) return MI355X_E_INVAL;
    if (pen->last_n == 0 && n_bias == 0) return MI355X_OK;  // nothing to edit: no launch
    if (!device_ok()) return MI355X_E_NODEVICE;
    PenalizeArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x;
    p.row_stride = row_stride;
    if (pen->last_n > 0) p.hist = hist, p.hist_stride = hist_stride, p.end = end, p.n_hist = (int)n_hist;
    p.bias_tok = bias_tok;
    p.bias_val = bias_val;
    p.n = (uint32_t)n;
    p.last_n = pen->last_n;
    p.n_bias = n_bias;
    p.repeat = pen->repeat;
    p.freq = pen->freq;
    p.present = pen->present;
    return timed_launch("kq::kq_penalize_rows", (double)rows * (12.0 * pen->last_n + 16.0 * n_bias),
                        kq_penalize_rows, dim3((unsigned)rows), dim3(kPenalizeThreads), 0, stream, p);
}

}  // namespace kq

extern "C" {

int mi355x_penalize_rows(float *x, int64_t n, int64_t rows, int64_t row_stride, const struct mi355x_penalties *p,
                         const int32_t *hist, int64_t hist_stride, int64_t n_hist, const int32_t *end,
                         const int32_t *bias_tok, const float *bias_val, int n_bias, void *stream) {
    return kq::launch_penalize_rows(x, n, rows, row_stride, p, hist, hist_stride, n_hist, end, bias_tok, bias_val, n_bias,
                                    (hipStream_t)stream);
}

}  // extern "C"
