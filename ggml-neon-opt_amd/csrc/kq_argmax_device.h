// kq_argmax_device.h — what kq_argmax.hip (greedy) and kq_sample.hip (top-k and the sampler)
// share on the device: the launch shape, the workspace's counter line and the ordered key of a
// value; and kq_sample.hip's arrival count, a restatement of the one inside kq_argmax.hip's hand_off.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kq {

constexpr int kArgmaxThreads = 256;
constexpr int kArgmaxMaxWgs = 256;  // the last arriver reads one word per thread
constexpr size_t kArgmaxCounterBytes = 128;  // the counter on a line of its own, then the words

__device__ __forceinline__ uint32_t ord_key(uint32_t b) {
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;  // NaN: below -inf's key (0x007fffff)
    if (b == 0x80000000u) b = 0u;                     // -0.0 == +0.0
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}

// NOT shared with kq_argmax.hip: hand_off there carries the same sequence inline (its code stays
// as it was), and only kq_sample.hip calls this one. A fix to either copy belongs in both.
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

}  // namespace kq
