// kq_sample.hip — sampling on the device: the exact top-k of an f32 vector (the logits) in ONE
// launch over several workgroups, and on its last arriver llama.cpp's default sampler chain
// (top-k -> top-p -> min-p -> temperature -> one draw), so a sampled token is staged for the
// next decode step exactly as kq_argmax stages a greedy one (LlamaDecoder.generate(sampler=...)).
//
// The rule (include/ggml_mi355x.h, mi355x_sample; restated in tests/sample_ref.py; the same
// token, no tolerance). Parameters top_k in [1, 64], temp finite >= 0, top_p in (0, 1], min_p in
// [0, 1]; one f32 draw u per token, meant to lie in [0, 1).
//   Candidates: the m = min(top_k, number of non-NaN entries) largest entries under kq_argmax's
//   order (larger value first, -0.0 == +0.0, among equal values the smaller index), sorted
//   c_0 .. c_{m-1} with logits l_0 >= l_1 >= ... A NaN is never a candidate; m == 0 gives token 0;
//   c_0 is mi355x_argmax's result. If temp == 0, m == 1 or l_0 is not finite the token is c_0 and
//   no arithmetic runs. Else, every step f32, one rounding per operation, nothing contracted, the
//   division correctly rounded, the sums sequential in candidate order:
//     1. d_i = l_i - l_0            2. e_i = d_i == -inf ? 0 : v_expf(d_i)   (e_0 == 1)
//     3. S = e_0 + e_1 + ...        4. p_i = e_i / S
//     5. min-p keeps the candidates before the first i with !(e_i >= min_p)
//     6. top-p keeps the shortest prefix whose running sum p_0 + .. + p_j is >= top_p (all m if
//        top_p >= 1 or no running sum reaches it)
//     7. q = the shorter of the two prefixes, at least 1
//     8. t_i = d_i / temp, f_i = t_i == -inf ? 0 : v_expf(t_i), F = f_0 + .. + f_{q-1}
//     9. r = u * F
//    10. the token is the first c_i, i < q, whose running sum f_0 + .. + f_i is > r; if there is
//        none (u >= 1, a NaN, rounding) it is c_{q-1}.
//   d_i / temp, not l_i / temp - max: a tiny temp cannot give inf - inf.
//
// Words. An entry's word is kq_argmax's, (ord_key << 32) | ~index, except that a NaN's word is 0,
// the word of "no entry": words of entries are unique, so no tie logic exists anywhere, and a
// word that is 0 is never a candidate.
//
// Decomposition. The slices are argmax_plan(n)'s. Workgroup s builds the words of its slice (16-B
// loads; the vector's last n % 4 entries by scalar loads), selects the slice's min(top_k,
// entries) largest and stores them SORTED, largest first, in its 64 places of the workspace;
// places it does not fill up to top_k hold 0. Hand-off: kq_argmax's, on the same arrive_last
// (kq_argmax_device.h): the words write-through, drained, barrier, one agent-scope add; the last
// arriver stores 0 back to the counter; nobody waits. The last arriver reads each slice's FIRST
// word (one per thread), keeps the min(top_k, wgs) slices with the largest first words (a slice
// whose maximum is not among the top_k largest maxima cannot contribute), loads only those
// slices' words (<= 64 x 64 words, 32 KB of LDS), selects and sorts the final m with the same
// routine, and one of its waves runs the rule above: the e and f values in parallel, the sums in
// order.
//
// Selection (select_sorted, one routine at both levels): a radix select on the whole 64-bit word,
// 8 bits a pass from the top, histograms in LDS; bin 255 - t is thread t's, a scan over the
// threads finds the bin that holds the top_k-th word, and the select leaves as soon as that bin
// completes top_k exactly. The words >= the threshold are compacted and ordered by rank counting
// (a word's rank is the number of larger words).
#include <string.h>

#include "kq_argmax_device.h"
#include "kq_device.h"
#include "kq_internal.h"
#include "kq_ops_device.h"

// Timing stops of the diagnostic builds (make variant-sample NAME=sd1 VFLAGS=-DKQ_SAMPLE_DIAG=1; results
// invalid): 1: the last arriver leaves right after the arrival (no merge, no tail), 2: after the
// merge (no sampling tail). tools/generate_bench.py --sampler --launch-only times the launch under each.
#ifndef KQ_SAMPLE_DIAG
#define KQ_SAMPLE_DIAG 0
#endif

namespace kq {

namespace {

constexpr int kTopkMaxK = MI355X_SAMPLE_MAX_K;
// a row's part of the workspace: the counter's line, then 64 places for each of 256 slices,
// whatever n and top_k are (kArgmaxRowBytes' argument: a counter's place never depends on the call)
constexpr size_t kTopkRowBytes = kArgmaxCounterBytes + 8 * (size_t)kArgmaxMaxWgs * kTopkMaxK;
static_assert(kTopkRowBytes % kArgmaxCounterBytes == 0, "a row's part is a whole number of lines");

typedef unsigned long long u64;

struct TopkShared {
    u64 buf[kTopkMaxK * kTopkMaxK];  // the last arriver: the kept slices' words
    u64 first[kArgmaxMaxWgs];        // ... every slice's first word
    u64 cand[kTopkMaxK], sorted[kTopkMaxK];
    uint32_t hist[256];
    uint32_t wsum[4], sel[3], ncand;
    int keep[kTopkMaxK];
    int flag, token;
};

__device__ __forceinline__ u64 entry_word(uint32_t bits, uint32_t i) {
    const uint32_t k = ord_key(bits);
    return k ? ((u64)k << 32) | (uint32_t)~i : 0ull;
}

// The words of slice [lo, hi) of x (lo % 4 == 0, x 16-B aligned; hi % 4 != 0 only at x's end),
// each handed to exactly one thread: lane t's first vector is kept in registers (the whole slice
// at the default split), the further ones are loaded again pass after pass.
struct SliceWords {
    const float *x;
    int vnext, vfull, hi;
    u64 c[4];
    __device__ __forceinline__ SliceWords(const float *x_, int lo, int hi_) : x(x_), hi(hi_) {
        const int t = (int)threadIdx.x, v0 = (lo >> 2) + t;
        vfull = hi >> 2;
        vnext = v0 + kArgmaxThreads;
        c[0] = c[1] = c[2] = c[3] = 0ull;
        if (v0 < vfull) {
            const u32x4 r = *(const u32x4 *)(x + 4 * (int64_t)v0);
            const uint32_t i0 = 4u * (uint32_t)v0;
            c[0] = entry_word(r.x, i0), c[1] = entry_word(r.y, i0 + 1), c[2] = entry_word(r.z, i0 + 2),
            c[3] = entry_word(r.w, i0 + 3);
        }
    }
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        f(c[0]), f(c[1]), f(c[2]), f(c[3]);
        for (int v = vnext; v < vfull; v += kArgmaxThreads) {
            const u32x4 r = *(const u32x4 *)(x + 4 * (int64_t)v);
            const uint32_t i0 = 4u * (uint32_t)v;
            f(entry_word(r.x, i0)), f(entry_word(r.y, i0 + 1)), f(entry_word(r.z, i0 + 2)), f(entry_word(r.w, i0 + 3));
        }
        if ((int)threadIdx.x == kArgmaxThreads - 1)
            for (int i = 4 * vfull; i < hi; ++i) f(entry_word(__float_as_uint(x[i]), (uint32_t)i));
    }
};

// `count` words in LDS
struct LdsWords {
    const u64 *w;
    int count;
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        for (int i = (int)threadIdx.x; i < count; i += kArgmaxThreads) f(w[i]);
    }
};

// The m = min(top_k, nonzero words) largest of the words `ws` hands out, in s.sorted[0 .. m),
// largest first; m in every thread. On entry s.hist and s.ncand are 0 (and every thread is past
// its last use of s.cand / s.sorted); on exit they are 0 again, behind a barrier.
template <typename Words>
__device__ __forceinline__ int select_sorted(const Words &ws, int top_k, TopkShared &s) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    u64 prefix = 0ull;  // the bytes chosen so far, the lower ones 0: at the end the threshold
    uint32_t need = (uint32_t)top_k, m = 0u;
    for (int shift = 56;; shift -= 8) {
        const u64 himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        ws.each([&](u64 w) {
            if (w != 0ull && (w & himask) == prefix) atomicAdd(&s.hist[(uint32_t)(w >> shift) & 255u], 1u);
        });
        __syncthreads();
        // thread t owns bin 255 - t: an inclusive scan over the threads counts from the top bin down
        const uint32_t own = s.hist[255 - t];
        s.hist[255 - t] = 0u;
        uint32_t incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) s.wsum[wave] = incl;
        __syncthreads();
        const uint32_t w0 = s.wsum[0], w1 = s.wsum[1], w2 = s.wsum[2], w3 = s.wsum[3];
        incl += (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
        if (shift == 56) {  // every nonzero word is in the first histogram
            const uint32_t total = w0 + w1 + w2 + w3;
            need = m = need < total ? need : total;
            if (m == 0u) return 0;  // (every thread: total is the same sum of s.wsum in all of them)
        }
        if (incl - own < need && need <= incl) s.sel[0] = (uint32_t)(255 - t), s.sel[1] = incl - own, s.sel[2] = own;
        __syncthreads();
        prefix |= (u64)s.sel[0] << shift;
        need -= s.sel[1];
        if (s.sel[2] == need || shift == 0) break;  // the bin completes top_k exactly (shift 0: one word a bin)
    }
    ws.each([&](u64 w) {
        if (w != 0ull && w >= prefix) {
            const uint32_t slot = atomicAdd(&s.ncand, 1u);
            if (slot < (uint32_t)kTopkMaxK) s.cand[slot] = w;
        }
    });
    __syncthreads();
    if (t == 0) s.ncand = 0u;
    if (t < (int)m) {
        const u64 w = s.cand[t];
        int rank = 0;
        for (int j = 0; j < (int)m; ++j) rank += s.cand[j] > w ? 1 : 0;
        s.sorted[rank] = w;
    }
    __syncthreads();
    return (int)m;
}

// One row's top-k: false in every thread of a workgroup that is not the row's last arriver; in
// the last arriver's threads true, *m_out the number of candidates and s.sorted[0 .. m) their
// words, largest first. part: the row's 256 x 64 places behind its counter cnt.
__device__ __forceinline__ bool topk_row(const float *x, int n, int slice, int wgs, int top_k, uint32_t *cnt, u64 *part,
                                         TopkShared &s, int *m_out) {
    const int t = (int)threadIdx.x, wg = (int)blockIdx.x;
    const int lo = wg * slice;  // (lo < n: wgs = ceil(n / slice))
    const int hi = n - lo < slice ? n : lo + slice;
    s.hist[t] = 0u;
    if (t == 0) s.ncand = 0u;
    __syncthreads();
    const SliceWords sw(x, lo, hi);
    int m = select_sorted(sw, top_k, s);
    // ---- the slice's words write-through, every wave drained, barrier, one add
    if (t < top_k) __hip_atomic_store(part + (size_t)wg * kTopkMaxK + t, t < m ? s.sorted[t] : 0ull, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
    if (!arrive_last(cnt, wgs, &s.flag)) return false;
    if (KQ_SAMPLE_DIAG == 1) {
        *m_out = 0;
        return true;
    }

    // ---- the last arriver: every slice's first word (wgs <= 256: one per thread), sc1 loads
    const u64 f = t < wgs ? __hip_atomic_load(part + (size_t)t * kTopkMaxK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    s.first[t] = f;
    const int nz = __syncthreads_count(f != 0ull);
    const int nkeep = nz < top_k ? nz : top_k;
    if (f != 0ull) {  // (nonzero words are unique: the rank has no ties)
        int rank = 0;
        for (int j = 0; j < wgs; ++j) rank += s.first[j] > f ? 1 : 0;
        if (rank < top_k) s.keep[rank] = t;
    }
    __syncthreads();
    const int total = nkeep * top_k;
    for (int i = t; i < total; i += kArgmaxThreads) {
        const int sl = s.keep[i / top_k] & (kArgmaxMaxWgs - 1), j = i % top_k;  // (masked: never outside the row's places)
        s.buf[i] = __hip_atomic_load(part + (size_t)sl * kTopkMaxK + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const LdsWords lw = {s.buf, total};
    *m_out = select_sorted(lw, top_k, s);
    return true;
}

struct SamplerArgs {
    float temp, top_p, min_p;
};

// The rule's steps on the m sorted candidates, by the first wave alone (every lane of it active):
// the token, in every lane.
__device__ __forceinline__ int32_t sample_tail(const float *x, const u64 *sorted, int m, const SamplerArgs &sp, float u) {
    const int i = (int)threadIdx.x;
    if (m == 0) return 0;
    const bool on = i < m;
    const uint32_t c = on ? ~(uint32_t)sorted[i] : 0u;
    const float l = on ? x[c] : -INFINITY;
    const int32_t c0 = __shfl((int)c, 0, 64);
    const float l0 = __shfl(l, 0, 64);
    if (sp.temp == 0.0f || m == 1 || !(__builtin_fabsf(l0) < INFINITY)) return c0;
    const float d = l - l0;
    const float e = d == -INFINITY ? 0.0f : v_expf(d);
    float S = __shfl(e, 0, 64);
    for (int j = 1; j < m; ++j) S = S + __shfl(e, j, 64);
    const float p = e / S;
    const uint64_t below = __ballot(on && !(e >= sp.min_p));
    int q = below ? (int)__builtin_ctzll(below) : m;
    if (sp.top_p < 1.0f) {
        float acc = 0.0f, run = 0.0f;
        for (int j = 0; j < m; ++j) {
            const float pj = __shfl(p, j, 64);
            acc = j ? acc + pj : pj;
            if (i == j) run = acc;
        }
        const uint64_t reached = __ballot(on && run >= sp.top_p);
        const int qp = reached ? (int)__builtin_ctzll(reached) + 1 : m;
        q = qp < q ? qp : q;
    }
    q = q < 1 ? 1 : q;
    const float tt = d / sp.temp;
    const float f = tt == -INFINITY ? 0.0f : v_expf(tt);
    float acc = 0.0f, run = 0.0f;
    for (int j = 0; j < q; ++j) {
        const float fj = __shfl(f, j, 64);
        acc = j ? acc + fj : fj;
        if (i == j) run = acc;
    }
    const float F = __shfl(run, q - 1, 64);
    const float r = u * F;
    const uint64_t over = __ballot(i < q && run > r);
    const int k = over ? (int)__builtin_ctzll(over) : q - 1;
    return __shfl((int)c, k, 64);
}

// ... and its result in every thread of the workgroup
__device__ __forceinline__ int32_t sample_token(const float *x, TopkShared &s, int m, const SamplerArgs &sp, float u) {
    if ((int)threadIdx.x < 64) {
        const int32_t tok = sample_tail(x, s.sorted, KQ_SAMPLE_DIAG == 2 ? 0 : m, sp, u);
        if (threadIdx.x == 0) s.token = tok;
    }
    __syncthreads();
    return s.token;
}

// The plain form's outputs: idx / val [top_k], places >= m: -1 / the quiet NaN
__device__ __forceinline__ void write_topk(const float *x, const TopkShared &s, int m, int top_k, int32_t *idx, float *val) {
    const int t = (int)threadIdx.x;
    if (t >= top_k) return;
    const uint32_t c = t < m ? ~(uint32_t)s.sorted[t] : 0u;
    idx[t] = t < m ? (int32_t)c : -1;
    val[t] = t < m ? x[c] : __uint_as_float(0x7fc00000u);
}

enum { TOPK_PLAIN = 0, TOPK_SAMPLE = 1, TOPK_STEP = 2 };

struct TopkArgs {
    const float *x;
    int n, slice, wgs, top_k, mode;
    uint8_t *ws;
    int32_t *idx;  // TOPK_PLAIN: [top_k] ...
    float *val;    // ... and their values
    SamplerArgs sp;
    const float *u;  // TOPK_SAMPLE: the draw [1]; TOPK_STEP: the draws table [n_draws]
    int32_t *out;    // TOPK_SAMPLE: [1]; TOPK_STEP: the decoder's input block [2 + hd], as kq_argmax's
    // TOPK_STEP: TokenStepArgs' members with n_draws among them, not the struct embedded: with
    // n_draws behind it the kernarg loads move, and the plain form at 128256 entries measured
    // 0.2 us slower (profiles/token_selection_refactor.txt)
    const int32_t *pos;
    const uint32_t *table;
    int32_t *hist;
    uint32_t rows, n_hist, n_draws;
    int hd;
    __device__ __forceinline__ TokenStepArgs step() const { return {pos, table, hist, rows, n_hist, hd}; }
};

__global__ void __launch_bounds__(kArgmaxThreads) kq_topk(const TopkArgs p) {
    __shared__ TopkShared s;
    const int t = (int)threadIdx.x;
    int m;
    if (!topk_row(p.x, p.n, p.slice, p.wgs, p.top_k, (uint32_t *)p.ws, (u64 *)(p.ws + kArgmaxCounterBytes), s, &m)) return;
    if (p.mode == TOPK_PLAIN) {
        write_topk(p.x, s, m, p.top_k, p.idx, p.val);
        return;
    }
    if (p.mode == TOPK_SAMPLE) {
        const int32_t token = sample_token(p.x, s, m, p.sp, p.u[0]);
        if (t == 0) p.out[0] = token;
        return;
    }
    const TokenStepArgs step = p.step();
    const uint32_t next = step.next();
    const float u = next < p.n_draws ? p.u[next] : 0.0f;
    // (its barrier: pos may be out + 1, and every thread has read it before one of them writes it)
    const int32_t token = sample_token(p.x, s, m, p.sp, u);
    step.write(p.out, next, token);
}

struct TopkRowsArgs {
    const float *x;
    int64_t row_stride;  // floats between two rows
    int n, slice, wgs, top_k, mode;
    uint8_t *ws;         // per row kTopkRowBytes
    int32_t *idx;        // TOPK_PLAIN: [rows][top_k] ...
    float *val;
    SamplerArgs sp;
    const float *u;      // TOPK_SAMPLE: [rows]; TOPK_STEP: the draws [rows][draws_stride]
    int32_t *out;        // [rows]
    RowsStepArgs step;   // TOPK_STEP, kq_argmax_rows'
    int64_t draws_stride;
    uint32_t n_draws;
};

__global__ void __launch_bounds__(kArgmaxThreads) kq_topk_rows(const TopkRowsArgs p) {
    __shared__ TopkShared s;
    const int64_t row = (int64_t)blockIdx.y;
    const float *x = p.x + row * p.row_stride;
    uint8_t *ws = p.ws + (size_t)row * kTopkRowBytes;
    int m;
    if (!topk_row(x, p.n, p.slice, p.wgs, p.top_k, (uint32_t *)ws, (u64 *)(ws + kArgmaxCounterBytes), s, &m)) return;
    if (p.mode == TOPK_PLAIN) {
        write_topk(x, s, m, p.top_k, p.idx + row * p.top_k, p.val + row * p.top_k);
        return;
    }
    if (p.mode == TOPK_SAMPLE) {
        const int32_t token = sample_token(x, s, m, p.sp, p.u[row]);
        if (threadIdx.x == 0) p.out[row] = token;
        return;
    }
    uint32_t np, nc;
    p.step.next(row, np, nc);
    const float u = np < p.n_draws ? p.u[row * p.draws_stride + np] : 0.0f;
    p.step.write(p.out, row, np, nc, sample_token(x, s, m, p.sp, u));
}

bool top_k_ok(int top_k) { return top_k >= 1 && top_k <= kTopkMaxK; }

// where the result goes: the plain form's (sp null) idx / val, or the sampled token(s) with the draw(s)
bool dest_ok(const mi355x_sampler *sp, int top_k, const int32_t *idx, const float *val, const float *u,
             const int32_t *out) {
    return sp ? sampler_ok(sp) && u && out : top_k_ok(top_k) && idx && val;
}

// a step's draws table: only a sampler has one
bool draws_ok(const mi355x_sampler *sp, int64_t n_draws, int64_t draws_stride) {
    return sp && n_draws >= 0 && n_draws <= 0x7fffffff && draws_stride >= n_draws;
}

}  // namespace

size_t topk_workspace(int64_t n, int64_t rows) {
    if (argmax_plan(n, nullptr, nullptr) != MI355X_OK || rows < 1 || rows > kArgmaxMaxRows) return 0;
    return (size_t)rows * kTopkRowBytes;
}

bool sampler_ok(const mi355x_sampler *s) {
    // (written so that a NaN fails every test)
    return s && top_k_ok(s->top_k) && s->temp >= 0.0f && s->temp < INFINITY && s->top_p > 0.0f && s->top_p <= 1.0f &&
           s->min_p >= 0.0f && s->min_p <= 1.0f;
}

int launch_topk(const float *x, int64_t n, int top_k, int32_t *idx, float *val, const mi355x_sampler *sp, const float *u,
                int32_t *out, const SampleStep *step, void *ws, size_t ws_size, hipStream_t stream) {
    int wgs = 0;
    int64_t slice = 0;
    if (!input_ok(x, n, 1, (n + 3) & ~(int64_t)3, &wgs, &slice) || !dest_ok(sp, top_k, idx, val, u, out))
        return MI355X_E_INVAL;
    if (step && !(step_ok(step->a) && draws_ok(sp, step->n_draws, step->n_draws))) return MI355X_E_INVAL;
    if (const int rc = workspace_status(ws, ws_size, topk_workspace(n, 1))) return rc;
    TopkArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x;
    p.n = (int)n;
    p.slice = (int)slice;
    p.wgs = wgs;
    p.top_k = sp ? sp->top_k : top_k;
    p.mode = !sp ? TOPK_PLAIN : step ? TOPK_STEP : TOPK_SAMPLE;
    p.ws = (uint8_t *)ws;
    p.idx = idx;
    p.val = val;
    if (sp) p.sp = {sp->temp, sp->top_p, sp->min_p};
    p.u = u;
    p.out = out;
    if (step) {
        const TokenStepArgs a = step_args(step->a);
        p.pos = a.pos, p.table = a.table, p.hist = a.hist, p.rows = a.rows, p.n_hist = a.n_hist, p.hd = a.hd;
        p.n_draws = (uint32_t)step->n_draws;
    }
    return timed_launch("kq::kq_topk", (double)n * 4.0, kq_topk, dim3((unsigned)wgs), dim3(kArgmaxThreads), 0, stream, p);
}

int launch_topk_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int top_k, int32_t *idx, float *val,
                     const mi355x_sampler *sp, const float *u, int32_t *out, const SampleRowsStep *step, void *ws,
                     size_t ws_size, hipStream_t stream) {
    int wgs = 0;
    int64_t slice = 0;
    if (!input_ok(x, n, rows, row_stride, &wgs, &slice) || !dest_ok(sp, top_k, idx, val, u, out)) return MI355X_E_INVAL;
    if (step && !(step_ok(step->a) && draws_ok(sp, step->n_draws, step->draws_stride))) return MI355X_E_INVAL;
    if (const int rc = workspace_status(ws, ws_size, topk_workspace(n, rows))) return rc;
    TopkRowsArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x;
    p.row_stride = row_stride;
    p.n = (int)n;
    p.slice = (int)slice;
    p.wgs = wgs;
    p.top_k = sp ? sp->top_k : top_k;
    p.mode = !sp ? TOPK_PLAIN : step ? TOPK_STEP : TOPK_SAMPLE;
    p.ws = (uint8_t *)ws;
    p.idx = idx;
    p.val = val;
    if (sp) p.sp = {sp->temp, sp->top_p, sp->min_p};
    p.u = u;
    p.out = out;
    if (step) p.step = step_args(step->a), p.draws_stride = step->draws_stride, p.n_draws = (uint32_t)step->n_draws;
    return timed_launch("kq::kq_topk_rows", (double)rows * (double)n * 4.0, kq_topk_rows,
                        dim3((unsigned)wgs, (unsigned)rows), dim3(kArgmaxThreads), 0, stream, p);
}

}  // namespace kq

extern "C" {

size_t mi355x_topk_workspace_size(int64_t n, int64_t rows) { return kq::topk_workspace(n, rows); }

int mi355x_topk(const float *x, int64_t n, int top_k, int32_t *idx, float *val, void *workspace, size_t workspace_size,
                void *stream) {
    return kq::launch_topk(x, n, top_k, idx, val, nullptr, nullptr, nullptr, nullptr, workspace, workspace_size,
                           (hipStream_t)stream);
}

int mi355x_topk_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, int top_k, int32_t *idx, float *val,
                     void *workspace, size_t workspace_size, void *stream) {
    return kq::launch_topk_rows(x, n, rows, row_stride, top_k, idx, val, nullptr, nullptr, nullptr, nullptr, workspace,
                                workspace_size, (hipStream_t)stream);
}

int mi355x_sample(const float *x, int64_t n, const struct mi355x_sampler *s, const float *u, int32_t *out, void *workspace,
                  size_t workspace_size, void *stream) {
    if (!s) return MI355X_E_INVAL;
    return kq::launch_topk(x, n, 0, nullptr, nullptr, s, u, out, nullptr, workspace, workspace_size, (hipStream_t)stream);
}

int mi355x_sample_rows(const float *x, int64_t n, int64_t rows, int64_t row_stride, const struct mi355x_sampler *s,
                       const float *u, int32_t *out, void *workspace, size_t workspace_size, void *stream) {
    if (!s) return MI355X_E_INVAL;
    return kq::launch_topk_rows(x, n, rows, row_stride, 0, nullptr, nullptr, s, u, out, nullptr, workspace, workspace_size,
                                (hipStream_t)stream);
}

}  // extern "C"
