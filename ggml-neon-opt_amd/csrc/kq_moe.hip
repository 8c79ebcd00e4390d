// kq_moe.hip — the mixture-of-experts FFN of llm_build_llama on the device (build_moe_ffn [U],
// taken when llama.expert_count > 0: Mixtral): the router (kq_moe_route), the expert GEMV whose
// weight base is data (kq_gemv_id, ggml's MUL_MAT_ID) and the weighted sum of the experts' outputs
// (kq_moe_combine). The rule is stated in include/ggml_mi355x.h (mi355x_moe_route,
// mi355x_mul_mat_id, mi355x_moe_combine) and restated in tests/moe_ref.py; the device gives the
// same bits. No global atomics, no workgroup waits for another; no workspace but the grouped form's.
//
// kq_moe_route, one workgroup of 4 waves per row of x:
//   dots     16 lanes per expert, lane c the accumulator lane c of ggml_vec_dot_f32's NEON form
//            (4 accumulators of 4 lanes, 16 floats a step: acc[c] = fma(g[16 s + c], x[16 s + c],
//            acc[c]) over the steps in order), 16 experts a round over the workgroup; then
//            acc0 += acc2, acc1 += acc3, acc0 += acc1 and (l0 + l1) + (l2 + l3) by lane exchanges
//            (float addition is commutative, so the pairs' operand order is free).
//   the rest wave 0, lane e holding expert e: soft_max (the order-free max, ggml_v_expf for the
//            first n & ~3 entries and libm's expf for the tail, the (e0 + e1) + (e2 + e3) group sums
//            added to a double in order, p = e * (float)(1 / sum)), then n_used passes of ggml's
//            argsort (the exchange sort `for i: for j > i: if p[idx[i]] < p[idx[j]]: swap`): in
//            pass i the value at position i is replaced by each strictly larger value met in
//            position order, the displaced value taking that position; only those positions
//            change, so a pass is one ballot and one exchange per such value, not n compares.
//            Positions below n_used are final after n_used passes. w = p[ids] / (float)(the sum
//            of w in a double, in slot order).
//
// kq_gemv_id<TYPE, RPW>, a workgroup of 4 waves per (token, slot) pair and 4 * RPW rows:
//   The expert id is read from device memory by every launch (and so by every replay of a
//   captured graph): a plain wave-uniform load. An id outside [0, n_expert) stores NaN to the
//   workgroup's rows and reads neither weights nor activations.
//   prologue the pair's f32 activation row, quantized to Q8_K in the aligned Q8L layout in LDS by
//            quant16_store (a superblock per 16 lanes, 16 superblocks a pass over the workgroup):
//            kq_quantize_q8L's arithmetic. Each workgroup quantizes the row it needs, so the
//            launch needs no workspace and no second launch.
//   stream   a wave owns RPW rows. A quad of lanes owns one superblock of a row and reads its bytes
//            from global memory straight into registers (16-byte loads; a Q6_K block, 210 bytes at
//            any even address, through 4-byte aligned loads from the dword below it, realigned by
//            v_alignbyte: no byte outside the dwords the block touches is read); 4 rows are
//            in flight per pass. rows_quad_step (kq_rows_device.h) forms the quad's exact integer
//            sums and the leader's record in LDS: the one copy of the dot.
//   chain    lane r replays row r's records in superblock order with rows_chain: the reference's
//            fp32 chain, the bits of kq_rows / kq_gemv and of the CPU oracle.
//   Only the selected expert's rows are read. T * n_used pairs are independent workgroups: a
//   prompt is correct but not weight-amortised.
//
// The grouped form of mi355x_mul_mat_id (mi355x_moe_prefill: GROUPED, or AUTO from
// kMoeGroupedMinPairs pairs), the same bits with every expert matrix read once per call:
//   kq_moe_group     one workgroup sorts the pairs by expert into the group table (kq_common.h),
//                    at every launch: the ids are data and a captured graph is replayed
//   kq_quantize_q8L  the T * ne11 activation rows, the Q8L/mmq layout, into the workspace
//   kq_mmq_id        kq_mmq's tiles with the weight base, the activation rows and the output rows
//                    of a tile taken from the table (kq_mmq.hip)
//
// kq_moe_combine: y[i, t] = ex[i, 0, t] * w[0, t], then + ex[i, s, t] * w[s, t] for s = 1 .. in
// slot order, each product and sum rounded once (no fused multiply-add), one thread an element.
#include <string.h>

#include <algorithm>
#include <atomic>

#include "kq_device.h"
#include "kq_internal.h"
#include "kq_ops_device.h"
#include "kq_rows_device.h"

namespace kq {

namespace {

constexpr int kMoeThreads = 256;
constexpr int kMoeMaxExperts = MI355X_MOE_MAX_EXPERTS;
constexpr int kMoeMaxUsed = MI355X_MOE_MAX_USED;
constexpr int kIdMaxNb = MI355X_MUL_MAT_ID_MAX_K / QK;  // superblocks of a row: LDS for the Q8L row and the records
constexpr int kIdBatch = 4;                            // rows of a wave in flight per pass

// ---------------------------------------------------------------- libm's expf
// glibc's expf (the soft_max tail of ggml_vec_soft_max_f32 beyond n & ~3 entries is scalar expf
// [U]): exp2f_data's table of 2^(i/32) and its degree-3 polynomial in double, with the fused
// multiply-adds of the build that CPUs with FMA dispatch to; x <= 0 here. The rule's restatement
// takes this tail from the host's libm, so rows with a tail (n_expert % 4 != 0) are bit-exact
// where the host's expf is that build: tests/test_moe_expf.py restates this function on the host
// (it reads the table and the constants from this file) and compares it with the host's expf.
__device__ const uint64_t kExp2fTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull,
    0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull,
    0x3feedea64c123422ull, 0x3feece086061892dull, 0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull,
    0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, 0x3feee89f995ad3adull,
    0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
    0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

__device__ __forceinline__ float libm_expf(float x) {
    constexpr double N = 32.0;
    constexpr double kInvLn2N = 0x1.71547652b82fep+0 * N, kShift = 0x1.8p+52;
    constexpr double C0 = 0x1.c6af84b912394p-5 / N / N / N, C1 = 0x1.ebfce50fac4f3p-3 / N / N, C2 = 0x1.62e42ff0c52d6p-1 / N;
    if (x != x) return x;
    if (x < -0x1.9fe368p6f) return 0.0f;     // underflow (and -inf)
    if (x > 0x1.62e42ep6f) return INFINITY;  // overflow
    double z = kInvLn2N * (double)x;
    double kd = z + kShift;
    const uint64_t ki = __builtin_bit_cast(uint64_t, kd);
    kd -= kShift;
    const double r = z - kd;
    const double s = __builtin_bit_cast(double, kExp2fTab[ki % 32] + (ki << 47));
    z = __builtin_fma(C0, r, C1);
    double y = __builtin_fma(C2, r, 1.0);
    y = __builtin_fma(z, r * r, y);
    return (float)(y * s);
}

__device__ __forceinline__ float lane_f32(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// ---------------------------------------------------------------- kq_moe_route
struct RouteArgs {
    const float *gate;  // [n_expert][n_embd]
    const float *x;     // rows of n_embd
    int64_t x_stride;   // floats
    int32_t *rec;       // per row: int32 ids[n_used], float w[n_used]
    int64_t rec_stride;  // words
    float *probs;        // [T][n_expert] or null
    int n_embd, n_expert, n_used;
};

__global__ void __launch_bounds__(kMoeThreads) kq_moe_route(const RouteArgs a) {
    __shared__ float logit[kMoeMaxExperts];
    __shared__ float part[kMoeMaxExperts / 4 + 4];  // the soft_max group sums, then the tail's terms
    const int tid = (int)threadIdx.x, lane = tid & 63, c = tid & 15;
    const int64_t row = blockIdx.x;
    const float *xr = a.x + row * a.x_stride;
    const int steps = a.n_embd / 16;
    for (int e = tid >> 4; e < a.n_expert; e += kMoeThreads / 16) {
        const float *g = a.gate + (int64_t)e * a.n_embd;
        float acc = 0.f;
#pragma unroll 4
        for (int s = 0; s < steps; ++s) acc = __builtin_fmaf(g[16 * s + c], xr[16 * s + c], acc);
        // c = 4 j + l: accumulator j, lane l
        acc = acc + __shfl_xor(acc, 8, 16);  // acc0 += acc2 (c < 4), acc1 += acc3 (4 <= c < 8)
        acc = acc + __shfl_xor(acc, 4, 16);  // acc0 += acc1
        acc = acc + __shfl_xor(acc, 1, 16);  // l0 + l1, l2 + l3
        acc = acc + __shfl_xor(acc, 2, 16);  // (l0 + l1) + (l2 + l3)
        if (c == 0) logit[e] = acc;
    }
    __syncthreads();
    if (tid >= 64) return;  // (no barrier below)
    const int n = a.n_expert, n4 = n & ~3;
    const bool in = lane < n;
    const float w = in ? logit[lane] : -INFINITY;
    const float mx = wave_fmax(w);
    float e = 0.f;
    if (in) e = lane < n4 ? v_expf(w - mx) : libm_expf(w - mx);
    float gs = e + __shfl_xor(e, 1, 64);
    gs = gs + __shfl_xor(gs, 2, 64);  // lane 4 k: (e0 + e1) + (e2 + e3)
    if (lane < n4 && !(lane & 3)) part[lane >> 2] = gs;
    if (lane >= n4 && in) part[n4 / 4 + (lane - n4)] = e;
    wave_lds_fence();
    double sum = 0.0;
    const int terms = n4 / 4 + (n - n4);
    for (int k = 0; k < terms; ++k) sum += (double)part[k];
    const float inv = (float)(1.0 / sum);
    const float p = e * inv;
    if (a.probs && in) a.probs[row * n + lane] = p;

    // ggml's argsort, the passes that settle positions [0, n_used): lane j holds position j
    float pv = p;
    int id = lane;
    for (int i = 0; i < a.n_used; ++i) {
        float cur = lane_f32(pv, i);
        int cid = __builtin_amdgcn_readlane(id, i);
        int last = i;
        for (;;) {
            const uint64_t m = __ballot(lane > last && in && pv > cur);
            if (!m) break;
            const int r = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
            const float nv = lane_f32(pv, r);
            const int nid = __builtin_amdgcn_readlane(id, r);
            if (lane == r) pv = cur, id = cid;
            cur = nv, cid = nid, last = r;
        }
        if (lane == i) pv = cur, id = cid;
    }
    double ws = 0.0;
    for (int s = 0; s < a.n_used; ++s) ws += (double)lane_f32(pv, s);
    const float wn = pv / (float)ws;
    if (lane < a.n_used) {
        int32_t *rec = a.rec + row * a.rec_stride;
        rec[lane] = id;
        rec[a.n_used + lane] = __float_as_int(wn);
    }
}

// ---------------------------------------------------------------- kq_gemv_id
struct GemvIdArgs {
    const uint8_t *w;    // [n_expert] matrices of N rows
    int64_t nb01, nb02;  // bytes between rows, between experts
    const float *x;      // [T][ne11] rows of K floats
    int64_t x_stride;    // floats between rows
    const int32_t *ids;  // ids[t * ids_stride + s]
    int64_t ids_stride;  // words
    float *y;            // [T][n_used][N]
    int n_expert, n_used, ne11, nb, N;
};

template <int TYPE, int RPW>
__global__ void __launch_bounds__(kMoeThreads) kq_gemv_id(const GemvIdArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    static_assert(RPW % kIdBatch == 0 && RPW <= 64, "whole batches; a chain lane per row");
    constexpr int BB = TYPE == Q4_K ? 144 : TYPE == Q5_K ? 176 : 210;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = (int)blockIdx.y;
    const int t = pair / a.n_used, slot = pair - t * a.n_used;
    const int nb = a.nb;
    const int row0 = (int)blockIdx.x * (WAVES_PER_WG * RPW);
    float *y = a.y + (int64_t)pair * a.N;
    const int id = __builtin_amdgcn_readfirstlane(a.ids[(int64_t)t * a.ids_stride + slot]);
    if ((uint32_t)id >= (uint32_t)a.n_expert) {  // never a silent result: the ids cannot be checked on the host
        for (int r = row0 + tid; r < row0 + WAVES_PER_WG * RPW && r < a.N; r += kMoeThreads)
            y[r] = __uint_as_float(0x7fc00000u);
        return;
    }
    uint8_t *act = smem;                                                       // [nb] Q8L blocks
    RowRec *recs = (RowRec *)(smem + (size_t)nb * Q8L_STRIDE) + (size_t)wave * RPW * nb;  // [RPW][nb]

    // ---- prologue: the pair's activation row -> Q8L in LDS
    const float *xr = a.x + ((int64_t)t * a.ne11 + (slot % a.ne11)) * a.x_stride;
    for (int b = tid >> 4; b < nb; b += kMoeThreads / 16) {  // whole 16-lane rows drop out together
        const float *xb = xr + (int64_t)b * QK + 16 * (lane & 15);
        u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *(const u32x4 *)(xb + 4 * k);
        quant16_store<false>(v, lane & 15, act + b * Q8L_STRIDE);
    }
    __syncthreads();

    // ---- stream: quad q of the wave <-> superblock b0 + q of each of the batch's rows
    const int wrow0 = row0 + wave * RPW;
    if (wrow0 >= a.N) return;  // (no barrier below)
    const uint8_t *wbase = a.w + (int64_t)id * a.nb02;
    const int q = lane >> 2, s = lane & 3;
    for (int rb = 0; rb < RPW; rb += kIdBatch) {
        if (wrow0 + rb >= a.N) break;
        for (int b0 = 0; b0 < nb; b0 += 16) {
            const int sb = b0 + q;
            if (sb < nb) {  // whole quads
#pragma unroll
                for (int r = 0; r < kIdBatch; ++r) {
                    int row = wrow0 + rb + r;
                    row = row < a.N ? row : a.N - 1;  // past the end: the last row again, never stored
                    rows_quad_step<TYPE>(wbase + (int64_t)row * a.nb01 + (int64_t)sb * BB, act + sb * Q8L_STRIDE, s,
                                         recs + (rb + r) * nb + sb);
                }
            }
        }
    }
    wave_lds_fence();  // this wave's records before its own reads
    // ---- chain: lane r <-> row r
    if (lane < RPW && wrow0 + lane < a.N) y[wrow0 + lane] = rows_chain<TYPE>(recs + lane * nb, nb, 1);
}

constexpr size_t gemv_id_lds(int nb, int rpw) {
    return (size_t)nb * Q8L_STRIDE + (size_t)WAVES_PER_WG * rpw * nb * sizeof(RowRec);
}
static_assert(gemv_id_lds(kIdMaxNb, 8) <= 64 * 1024, "the largest launch within the default LDS limit");

// ---------------------------------------------------------------- kq_moe_combine
__global__ void __launch_bounds__(kMoeThreads) kq_moe_combine(const float *__restrict__ ex, const int32_t *rec,
                                                              int64_t rec_stride, float *__restrict__ y, int n,
                                                              int n_used) {
    const int i = (int)(blockIdx.x * kMoeThreads + threadIdx.x);
    const int64_t t = blockIdx.y;
    if (i >= n) return;
    const float *e = ex + t * n_used * (int64_t)n + i;
    const float *w = (const float *)(rec + t * rec_stride + n_used);
    float out = e[0] * w[0];
    for (int s = 1; s < n_used; ++s) out = out + e[(int64_t)s * n] * w[s];
    y[t * n + i] = out;
}

bool moe_type_ok(int type) { return type == Q4_K || type == Q5_K || type == Q6_K; }

// ---------------------------------------------------------------- kq_moe_group
// The group table of kq_common.h from a MOE_ROUTE node's ids, one workgroup, one launch, LDS
// atomics only: count the pairs per bucket, one thread forms the three prefixes (at most 65
// buckets), then every pair takes the next free entry of its bucket. Which entry a pair gets
// within its bucket depends on the order the atomics retire in, so the sort is not stable and
// not the same from run to run; no result depends on it, every output element of kq_mmq_id
// being the chain of its own (row, pair). A stable sort would cost a scan per bucket for nothing.
constexpr int kGroupThreads = 1024;
struct GroupArgs {
    const int32_t *ids;
    int64_t ids_stride;
    int32_t *tab;
    int n_expert, n_used, pairs;
};

__global__ void __launch_bounds__(kGroupThreads) kq_moe_group(const GroupArgs a) {
    __shared__ int cnt[MOE_BUCKETS], next[MOE_BUCKETS];
    const int tid = (int)threadIdx.x, nbk = a.n_expert + 1;
    if (tid < nbk) cnt[tid] = 0;
    __syncthreads();
    for (int p = tid; p < a.pairs; p += kGroupThreads) {
        const int t = p / a.n_used;
        const int id = a.ids[(int64_t)t * a.ids_stride + (p - t * a.n_used)];
        atomicAdd(&cnt[(uint32_t)id < (uint32_t)a.n_expert ? id : a.n_expert], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int first = 0, tile = 0, tilew = 0;
        for (int k = 0; k < nbk; ++k) {
            const int c = cnt[k];
            a.tab[MOE_TAB_COUNT + k] = c;
            a.tab[MOE_TAB_FIRST + k] = first;
            a.tab[MOE_TAB_TILE0 + k] = tile;
            a.tab[MOE_TAB_TILE0W + k] = tilew;
            next[k] = first;
            first += c;
            tile += (c + 63) / 64;
            tilew += (c + 127) / 128;
        }
        a.tab[MOE_TAB_TILE0 + nbk] = tile;
        a.tab[MOE_TAB_TILE0W + nbk] = tilew;
    }
    __syncthreads();
    int32_t *list_pair = a.tab + MOE_TAB_LIST, *list_tok = list_pair + a.pairs;
    for (int p = tid; p < a.pairs; p += kGroupThreads) {
        const int t = p / a.n_used;
        const int id = a.ids[(int64_t)t * a.ids_stride + (p - t * a.n_used)];
        const int at = atomicAdd(&next[(uint32_t)id < (uint32_t)a.n_expert ? id : a.n_expert], 1);
        list_pair[at] = p;
        list_tok[at] = t;
    }
}

std::atomic<int> g_moe_prefill{MI355X_MOE_PREFILL_AUTO};  // mi355x_moe_prefill()

}  // namespace

template <int TYPE, int RT, int CW>
__global__ void kq_mmq_id(const MmqArgs a, const MmqIdArgs g);

int moe_prefill_mode() { return g_moe_prefill.load(); }

bool moe_grouped(int64_t pairs) {
    const int mode = moe_prefill_mode();
    return mode == MI355X_MOE_PREFILL_GROUPED ? pairs >= 1 : mode == MI355X_MOE_PREFILL_AUTO && pairs >= kMoeGroupedMinPairs;
}

size_t moe_table_bytes(int64_t pairs) { return ((size_t)moe_table_words(pairs) * 4 + 255) & ~(size_t)255; }
size_t moe_q8_bytes(int64_t K, int64_t rows) { return (size_t)rows * (size_t)(K / QK) * Q8L_STRIDE; }

namespace {

int launch_moe_group(const int32_t *ids, int64_t ids_stride, int n_expert, int n_used, int pairs, int32_t *table,
                     hipStream_t stream) {
    GroupArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = ids;
    a.ids_stride = ids_stride;
    a.tab = table;
    a.n_expert = n_expert;
    a.n_used = n_used;
    a.pairs = pairs;
    return timed_launch("kq::kq_moe_group", 4.0 * (2.0 * pairs + (double)moe_table_words(pairs)), kq_moe_group, dim3(1),
                        dim3(kGroupThreads), 0, stream, a);
}

// kq_mmq_id on the table and the Q8L rows of `gr`: 128 x 64 tiles (narrow column tiles waste least
// on ragged experts), row tiles x
// the most column tiles any routing of `pairs` pairs can need (every non-empty bucket ends with
// one partial tile, and no tile is empty), so the grid depends on the shapes alone
int launch_mmq_id(int type, const GemvIdArgs &g, const MoeGrouped &gr, int pairs, hipStream_t stream) {
    // Q6_K: 128 x 128 once an expert's average bucket fills a 128-column tile (Mixtral's down at 1024 pairs:
    // 426 against 501 us, 224 against 344 on two experts; at 256 pairs and below 128 x 64 wins, 176 against
    // 219; 64 x 128 wins nowhere: profiles/moe_prefill.txt). The MMQ_ID_Q6 knob forces a shape (A/B).
    int q6 = type == Q6_K ? (int)knob(KNOB_MMQ_ID_Q6) : 3;
    if (q6 < 1 || q6 > 3) q6 = pairs >= 128 * g.n_expert ? 1 : 3;
    const int RT = q6 == 2 ? 64 : 128, CW = q6 == 3 ? 1 : 2;
    MmqArgs a;
    memset(&a, 0, sizeof(a));
    a.w = g.w;
    a.row_stride = g.nb01;
    a.n_rows = g.N;
    a.xq = gr.xq;
    a.nb = g.nb;
    a.xq_col_stride = (int64_t)g.nb * Q8L_STRIDE;
    a.y = g.y;
    a.y_col_stride = g.N;
    a.n_mat = 1;
    MmqIdArgs id;
    memset(&id, 0, sizeof(id));
    id.tab = gr.table;
    id.pair = gr.table + MOE_TAB_LIST;
    id.xrow = g.ne11 == 1 ? id.pair + pairs : id.pair;  // the token list, or (row t * n_used + s) the pair list
    id.nb02 = g.nb02;
    id.n_expert = g.n_expert;
    const int col_tiles = std::min(pairs / mmq_cols(CW) + g.n_expert + 1, pairs);
    const dim3 grid((unsigned)col_tiles, (unsigned)((g.N + RT - 1) / RT));
    const size_t lds = 2 * (size_t)mmq_buf_bytes(type, RT, CW) + 16;  // (+16: the Q6_K realign reads past the last row)
    const void *fn = type == Q4_K   ? (const void *)kq_mmq_id<Q4_K, 128, 1>
                     : type == Q5_K ? (const void *)kq_mmq_id<Q5_K, 128, 1>
                     : q6 == 1      ? (const void *)kq_mmq_id<Q6_K, 128, 2>
                     : q6 == 2      ? (const void *)kq_mmq_id<Q6_K, 64, 2>
                                    : (const void *)kq_mmq_id<Q6_K, 128, 1>;
    allow_lds(fn, lds);
    void *args[] = {&a, &id};
    return timed_launch_args(
        [&] {
            return LaunchInfo{type == Q4_K   ? "kq::kq_mmq_id<q4_K>"
                              : type == Q5_K ? "kq::kq_mmq_id<q5_K>"
                                             : "kq::kq_mmq_id<q6_K>",
                              (double)g.n_expert * g.N * g.nb * block_bytes(type) +
                                  (double)pairs * ((double)g.nb * Q8L_STRIDE + 4.0 * g.N)};
        },
        fn, grid, dim3((unsigned)(64 * mmq_waves(RT, CW))), lds, stream, args);
}

}  // namespace

int launch_moe_route(const float *gate_inp, int64_t n_embd, int n_expert, const float *x, int64_t x_stride, int64_t T,
                     int n_used, int32_t *record_out, int64_t record_stride, float *probs_out, hipStream_t stream) {
    if (!gate_inp || !x || !record_out || ((uintptr_t)gate_inp & 3u) || ((uintptr_t)x & 3u) ||
        ((uintptr_t)record_out & 3u) || ((uintptr_t)probs_out & 3u))
        return MI355X_E_INVAL;
    if (n_embd < 1 || n_expert < 1 || n_used < 1 || n_used > n_expert || T < 0) return MI355X_E_INVAL;
    if (T > 1 && x_stride < n_embd) return MI355X_E_INVAL;
    if (record_stride < 2 * (int64_t)n_used) return MI355X_E_INVAL;
    if (n_expert < 2 || n_expert > kMoeMaxExperts || n_used > kMoeMaxUsed || n_embd % 16 || n_embd > 0x7fffffff ||
        T > 0x7fffffff)
        return MI355X_E_UNSUPPORTED;
    if (T == 0) return MI355X_OK;
    if (!device_ok()) return MI355X_E_NODEVICE;
    RouteArgs a;
    memset(&a, 0, sizeof(a));
    a.gate = gate_inp;
    a.x = x;
    a.x_stride = x_stride;
    a.rec = record_out;
    a.rec_stride = record_stride;
    a.probs = probs_out;
    a.n_embd = (int)n_embd;
    a.n_expert = n_expert;
    a.n_used = n_used;
    const double bytes = 4.0 * (double)n_embd * ((double)n_expert + (double)T) + 8.0 * n_used * (double)T;
    return timed_launch("kq::kq_moe_route", bytes, kq_moe_route, dim3((unsigned)T), dim3(kMoeThreads), 0, stream, a);
}

int launch_mul_mat_id(int type, const void *experts, int64_t ne00, int64_t ne01, size_t nb01, size_t nb02, int n_expert,
                      const float *x, int64_t ne11, int64_t x_row_stride, const int32_t *ids, int64_t ids_stride,
                      int n_used, int64_t T, float *y, hipStream_t stream, const MoeGrouped *grouped) {
    if (!experts || !x || !ids || !y || ((uintptr_t)x & 15u) || ((uintptr_t)ids & 3u) || ((uintptr_t)y & 3u))
        return MI355X_E_INVAL;
    if (ne00 < 1 || ne00 % QK || ne01 < 0 || n_expert < 1 || n_used < 1 || T < 0) return MI355X_E_INVAL;
    if (ne11 != 1 && ne11 != n_used) return MI355X_E_INVAL;
    if ((x_row_stride & 3) || (T * ne11 > 1 && x_row_stride < ne00) || ids_stride < n_used) return MI355X_E_INVAL;
    if (!moe_type_ok(type)) return MI355X_E_UNSUPPORTED;
    const size_t row_bytes = (size_t)(ne00 / QK) * block_bytes(type);
    if (nb01 < row_bytes || (n_expert > 1 && ne01 > 0 && nb02 < (size_t)ne01 * nb01)) return MI355X_E_INVAL;
    // Q4_K / Q5_K blocks are read with 16-byte loads; a Q6_K block may stand at any even address (what
    // ggml's block_q6_K, 210 bytes with 2-byte members, can produce: quad_q6K reads d from one dword, which
    // holds it whole at an address 0 or 2 mod 4 only)
    if (type != Q6_K && (((uintptr_t)experts & 15u) || (nb01 & 15u) || (nb02 & 15u))) return MI355X_E_INVAL;
    if (type == Q6_K && (((uintptr_t)experts & 1u) || (nb01 & 1u) || (nb02 & 1u))) return MI355X_E_INVAL;
    if (n_expert > kMoeMaxExperts || n_used > kMoeMaxUsed || ne00 > MI355X_MUL_MAT_ID_MAX_K || ne01 > 0x7fffffff ||
        T * n_used > 65535)
        return MI355X_E_UNSUPPORTED;
    const int pairs = (int)(T * n_used);
    // the grouped form's table and Q8L rows: the caller's, 4- and 16-byte aligned and large enough
    bool take_grouped = moe_grouped(pairs);
    if (take_grouped &&
        (!grouped || !grouped->table || !grouped->xq || ((uintptr_t)grouped->table & 3u) || ((uintptr_t)grouped->xq & 15u) ||
         grouped->table_bytes < moe_table_bytes(pairs) || grouped->xq_bytes < moe_q8_bytes(ne00, T * ne11))) {
        // GROUPED asked for the form: an error. AUTO promises the faster form to a caller who brought its
        // workspace and refuses no call that kq_gemv_id can run
        if (moe_prefill_mode() == MI355X_MOE_PREFILL_GROUPED) return MI355X_E_WORKSPACE;
        take_grouped = false;
    }
    if (T == 0 || ne01 == 0) return MI355X_OK;
    if (!device_ok()) return MI355X_E_NODEVICE;
    GemvIdArgs a;
    memset(&a, 0, sizeof(a));
    a.w = (const uint8_t *)experts;
    a.nb01 = (int64_t)nb01;
    a.nb02 = (int64_t)nb02;
    a.x = x;
    a.x_stride = x_row_stride;
    a.ids = ids;
    a.ids_stride = ids_stride;
    a.y = y;
    a.n_expert = n_expert;
    a.n_used = n_used;
    a.ne11 = (int)ne11;
    a.nb = (int)(ne00 / QK);
    a.N = (int)ne01;
    if (take_grouped) {  // kq_moe_group and kq_quantize_q8L (unless an earlier launch left their outputs), kq_mmq_id
        int rc = grouped->build ? launch_moe_group(ids, ids_stride, n_expert, n_used, pairs, grouped->table, stream) : 0;
        if (!rc && grouped->quantize) rc = launch_quantize_q8L(x, x_row_stride, grouped->xq, ne00, T * ne11, stream, true);
        return rc ? rc : launch_mmq_id(type, a, *grouped, pairs, stream);
    }
    // 8 rows a wave where that still leaves every CU a few workgroups; else 4
    const int rpw = ((ne01 + 31) / 32) * pairs >= 512 ? 8 : 4;
    const int per_wg = WAVES_PER_WG * rpw;
    const dim3 grid((unsigned)((ne01 + per_wg - 1) / per_wg), (unsigned)pairs);
    const size_t lds = gemv_id_lds(a.nb, rpw);
    const double bytes = (double)pairs * ((double)ne01 * row_bytes + 4.0 * ne00 + 4.0 * ne01);
    void (*fn)(const GemvIdArgs) = nullptr;
    const char *name = "";
#define KQ_ID_CASE(TY, NAME)                                                                   \
    if (type == TY) {                                                                          \
        fn = rpw == 8 ? kq_gemv_id<TY, 8> : kq_gemv_id<TY, 4>;                                 \
        name = rpw == 8 ? "kq::kq_gemv_id<" NAME ", 8>" : "kq::kq_gemv_id<" NAME ", 4>";       \
    }
    KQ_ID_CASE(Q4_K, "q4_K")
    KQ_ID_CASE(Q5_K, "q5_K")
    KQ_ID_CASE(Q6_K, "q6_K")
#undef KQ_ID_CASE
    return timed_launch(name, bytes, fn, grid, dim3(kMoeThreads), lds, stream, a);
}

int launch_moe_combine(const float *ex, int64_t n, int n_used, int64_t T, const int32_t *records, int64_t record_stride,
                       float *y, hipStream_t stream) {
    if (!ex || !records || !y || ((uintptr_t)ex & 3u) || ((uintptr_t)records & 3u) || ((uintptr_t)y & 3u))
        return MI355X_E_INVAL;
    if (n < 0 || n_used < 1 || T < 0 || record_stride < 2 * (int64_t)n_used) return MI355X_E_INVAL;
    if (n_used > kMoeMaxUsed || n > 0x7fffffff - kMoeThreads || T > 65535) return MI355X_E_UNSUPPORTED;
    if (n == 0 || T == 0) return MI355X_OK;
    if (!device_ok()) return MI355X_E_NODEVICE;
    const dim3 grid((unsigned)((n + kMoeThreads - 1) / kMoeThreads), (unsigned)T);
    const double bytes = 4.0 * (double)n * (double)T * (n_used + 1.0);
    return timed_launch("kq::kq_moe_combine", bytes, kq_moe_combine, grid, dim3(kMoeThreads), 0, stream, ex, records,
                        record_stride, y, (int)n, n_used);
}

}  // namespace kq

extern "C" {

int mi355x_moe_route(const float *gate_inp, int64_t n_embd, int n_expert, const float *x, int64_t x_stride, int64_t T,
                     int n_used, int32_t *record_out, int64_t record_stride, float *probs_out, void *stream) {
    return kq::launch_moe_route(gate_inp, n_embd, n_expert, x, x_stride, T, n_used, record_out, record_stride, probs_out,
                                (hipStream_t)stream);
}

size_t mi355x_mul_mat_id_workspace_size(int type, int64_t ne00, int n_used, int64_t T) {
    (void)type;
    if (ne00 < 1 || ne00 % kq::QK || n_used < 1 || T < 1 || T * n_used > 65535) return 0;
    // kq_gemv_id quantizes the activation rows in its own prologue; the grouped form keeps the
    // group table and the Q8L rows (one per slot at most) there
    if (!kq::moe_grouped(T * n_used)) return 0;
    return kq::moe_table_bytes(T * n_used) + kq::moe_q8_bytes(ne00, T * n_used);
}

int mi355x_moe_prefill(int impl) {
    if (impl < MI355X_MOE_PREFILL_AUTO || impl > MI355X_MOE_PREFILL_GROUPED) return MI355X_E_INVAL;
    return kq::g_moe_prefill.exchange(impl);
}

int mi355x_mul_mat_id(int type, const void *experts, int64_t ne00, int64_t ne01, size_t nb01, size_t nb02, int n_expert,
                      const float *x, int64_t ne11, int64_t x_row_stride, const int32_t *ids, int64_t ids_stride,
                      int n_used, int64_t T, float *y, void *workspace, size_t workspace_size, void *stream) {
    // the grouped form's buffers in the workspace: the table, then the Q8L rows. launch_mul_mat_id returns
    // MI355X_E_WORKSPACE between the shape checks and the device check where the form needs more than it got
    kq::MoeGrouped gr;
    memset(&gr, 0, sizeof(gr));
    const size_t need = mi355x_mul_mat_id_workspace_size(type, ne00, n_used, T);
    if (workspace && need && workspace_size >= need) {
        const size_t tb = kq::moe_table_bytes(T * n_used);
        gr.table = (int32_t *)workspace;
        gr.table_bytes = tb;
        gr.xq = (uint8_t *)workspace + tb;
        gr.xq_bytes = workspace_size - tb;
    }
    gr.build = gr.quantize = true;
    return kq::launch_mul_mat_id(type, experts, ne00, ne01, nb01, nb02, n_expert, x, ne11, x_row_stride, ids, ids_stride,
                                 n_used, T, y, (hipStream_t)stream, &gr);
}

int mi355x_moe_combine(const float *ex, int64_t n, int n_used, int64_t T, const int32_t *records, int64_t record_stride,
                       float *y, void *stream) {
    return kq::launch_moe_combine(ex, n, n_used, T, records, record_stride, y, (hipStream_t)stream);
}

}  // extern "C"
