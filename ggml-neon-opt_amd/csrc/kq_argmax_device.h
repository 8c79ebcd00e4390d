// kq_argmax_device.h — what kq_argmax.hip (greedy) and kq_sample.hip (top-k and the sampler)
// share on the device: the launch shape, the workspace's counter line, the ordered key of a value,
// the arrival count of the hand-off, and the step-inputs forms' kernel arguments with their writes
// (step_args fills them from the host's structs of kq_internal.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kq_internal.h"

namespace kq {

constexpr int kArgmaxThreads = 256;
constexpr int kArgmaxMaxWgs = 256;  // the last arriver reads one word per thread
constexpr size_t kArgmaxCounterBytes = 128;  // the counter on a line of its own, then the words
// kq_argmax_rows, kq_logsum_rows: a row's part of the workspace, the counter's line and the words
// of the largest split. The same for every n, so every counter keeps its place whatever a
// workspace served before (a place that depended on n would land on another call's leftover
// words), and a whole number of lines, so no row's words share a line with a counter. Row 0's
// counter is kq_argmax's and the next is past kq_argmax's words: the backend's one buffer serves
// these kernels.
constexpr size_t kArgmaxRowBytes = kArgmaxCounterBytes + 8 * (size_t)kArgmaxMaxWgs;
static_assert(kArgmaxRowBytes % kArgmaxCounterBytes == 0, "a row's part is a whole number of lines");

__device__ __forceinline__ uint32_t ord_key(uint32_t b) {
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;  // NaN: below -inf's key (0x007fffff)
    if (b == 0x80000000u) b = 0u;                     // -0.0 == +0.0
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}

// The arrival of a workgroup whose words are stored write-through (sc1): every wave drains its
// stores, workgroup barrier, ONE agent-scope add on `cnt` that `wgs` workgroups count in on.
// True in every thread of the workgroup whose add came last (it has stored 0 back, so the next
// launch starts at 0), false in every other; nobody waits. `flag`: an LDS word of the caller's.
__device__ __forceinline__ bool arrive_last(uint32_t *cnt, int wgs, int *flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = old == (uint32_t)(wgs - 1);
        if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// The token step (kq_argmax, kq_topk; pos != null): out is the decoder's input block [2 + hd],
// out[0] = token, out[1] = *pos + 1, out[2 ..] = the bits of table row *pos + 1 where it exists,
// hist[*pos + 1] = token where it exists. Run by every thread of the last arriver.
struct TokenStepArgs {
    const int32_t *pos;
    const uint32_t *table;
    int32_t *hist;
    uint32_t rows, n_hist;
    int hd;
    // *pos + 1. pos may be out + 1, so every thread's load of it has returned here (a barrier
    // alone waits for no counter), and the caller puts a workgroup barrier between this and write
    __device__ __forceinline__ uint32_t next() const {
        uint32_t next = (uint32_t)*pos + 1u;
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(next)::"memory");
        return next;
    }
    __device__ __forceinline__ void write(int32_t *out, uint32_t next, int32_t token) const {
        const int t = (int)threadIdx.x;
        if (t == 0) {
            out[0] = token;
            out[1] = (int32_t)next;
            if (next < n_hist) hist[next] = token;
        }
        if (next < rows)
            for (int k = t; k < hd; k += kArgmaxThreads) out[2 + k] = (int32_t)table[(size_t)next * hd + k];
    }
};

// The rows step (kq_argmax_rows, kq_topk_rows; pos != null): row i's last arriver writes the
// token to out[i], advances pos[i] and cells[i], shows the new cell in mask row i and files the
// token in history row i, where those entries exist. Row i's entries are touched by that
// workgroup alone and written by its thread 0 alone.
struct RowsStepArgs {
    int32_t *pos, *cells, *hist;
    float *mask;
    int64_t mask_stride, hist_stride;  // entries between two rows
    uint32_t n_kv, n_hist;
    int cell_stride;
    // the row's new position and cell: the loads of pos[i] and cells[i] have returned before write
    __device__ __forceinline__ void next(int64_t row, uint32_t &np, uint32_t &nc) const {
        np = (uint32_t)pos[row] + 1u, nc = (uint32_t)cells[row] + (uint32_t)cell_stride;
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(np), "+v"(nc)::"memory");
    }
    __device__ __forceinline__ void write(int32_t *out, int64_t row, uint32_t np, uint32_t nc, int32_t token) const {
        if (threadIdx.x != 0) return;
        out[row] = token;
        pos[row] = (int32_t)np;
        cells[row] = (int32_t)nc;
        if (nc < n_kv) mask[row * mask_stride + nc] = 0.0f;  // the cell the next step writes: visible to its own row
        if (np < n_hist) hist[row * hist_stride + np] = token;
    }
};

inline TokenStepArgs step_args(const ArgmaxStep &s) {
    return {s.pos, (const uint32_t *)s.table, s.hist, (uint32_t)s.rows, (uint32_t)s.n_hist, s.hd};
}

inline RowsStepArgs step_args(const ArgmaxRowsStep &s) {
    return {s.pos, s.cells, s.hist, s.mask, s.mask_stride, s.hist_stride, (uint32_t)s.n_kv, (uint32_t)s.n_hist,
            s.cell_stride};
}

}  // namespace kq
