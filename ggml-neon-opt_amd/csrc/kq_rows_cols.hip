// kq_rows_cols.hip — small-batch GEMV: kq_rows' row streams against 2 to 15 activation columns.
//
// Same numerics as kq_rows (kq_rows.hip): integer partials bit-exact, the reference's fp32
// update in superblock order per (row, column), so y[c][row] has the bits of
// ggml_vec_dot_q4_K_q8_K (and the Q5_K / Q6_K siblings) called per (row, column).
//
// Decomposition (bound by the weight stream, which is read once for the whole column group;
// the matrix cores are not used: at 2 to 8 columns an MFMA tile would be mostly padding):
//  * weights as in kq_rows: a wave owns consecutive rows of one matrix as ONE contiguous byte
//    stream, fetched in steps of 16 superblocks by LDS-DMA (non-temporal, from the 16-byte
//    boundary below the stream, so Q6_K rows may start at any even address) into a per-wave
//    ring, completion by counted s_waitcnt vmcnt; no workgroup barrier after the prologue;
//  * activations: the column group's Q8L blocks come from the workspace by LDS-DMA once per
//    workgroup, ahead of the first weight step. The kernel reads the PLAIN Q8L layout
//    (kq_quantize_q8L<false>: d @0, qs @16, the 16 int16 bsums @272; Q6_K needs every bsum, which
//    the prefill GEMMs' "AM" layout folds in pairs), and every producer on this path writes it:
//    kq_quantize_q8L<false>, kq_rms_norm_q8L<false>, kq_swiglu_q8L<false>. Nothing is quantized here;
//  * dot: lane quad q computes superblock 16t + q of the stream. It unpacks its weight quants once
//    into registers (quad_unpack: nibbles, the Q5_K high bits, the Q6_K 4 + 2 bits, scales and
//    mins) and runs over the group's columns with v_dot4_i32_i8 (quad_dot), two DPP adds per sum;
//    the quad's leader stores the RowRec of each (row, column, superblock);
//  * chain: when a batch of bR rows is complete, lane p replays the records of (row p / NCOL,
//    column p % NCOL) in superblock order: bR * NCOL <= 64 pairs per instruction, the chain's
//    latency once per batch. Batches need not end on a step boundary: a wave with more than one
//    batch has two record buffers, and a step's superblocks fall into the oldest unreplayed batch
//    or the one after it (bR * nb >= 16);
//  * NCOL = 2 / 4 / 8 columns per workgroup, a partial group masked, grid.y groups (M = 9 .. 15:
//    two groups of 8). The host (plan_rows_cols, kq_gemv_host.hip) takes the widest NCOL whose
//    rows_cols_layout leaves two workgroups resident on a CU (80 KB each): 8 up to K = 3840,
//    4 up to K = 7936, 2 up to K = 15872 (one-type launches; a few hundred bytes per wave less
//    with mixed types); beyond that the call keeps the kq_quantize + kq_gemv path.
//  * up to MI355X_MAX_FUSED matrices of any K-quant types on one activation (q/k/v, gate + up),
//    and the residual epilogue y[c] = mul_mat + res[c] (the one f32 add of ggml_add).
#include <hip/hip_ext.h>

#include "kq_internal.h"
#include "kq_rows_device.h"

namespace kq {

namespace {

// write-through (sc1), as kq_rows stores: the next launch reads it from the memory-side caches
__device__ __forceinline__ void cols_store_y(float *p, float v) {
    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

struct ColsWave {
    int type, r0, nrows;
    const uint8_t *w;
    const float *res;
    float *y;
    int64_t res_cs, y_cs;
};

// This wave's matrix and rows, picked with selects (no indexed read of the argument block).
__device__ __forceinline__ ColsWave cols_resolve(const RowsColsArgs &a, int gw) {
    int m = 0;
    if (a.n_desc > 1 && gw >= a.wave_prefix[1]) m = 1;
    if (a.n_desc > 2 && gw >= a.wave_prefix[2]) m = 2;
    if (a.n_desc > 3 && gw >= a.wave_prefix[3]) m = 3;
#define COLS_PICK(f) (m == 0 ? a.f[0] : m == 1 ? a.f[1] : m == 2 ? a.f[2] : a.f[3])
    ColsWave h;
    const int j = gw - COLS_PICK(wave_prefix), base = COLS_PICK(rbase), rem = COLS_PICK(rrem);
    h.type = COLS_PICK(type);
    h.w = COLS_PICK(w), h.res = COLS_PICK(res), h.y = COLS_PICK(y);
    h.res_cs = COLS_PICK(res_col_stride), h.y_cs = COLS_PICK(y_col_stride);
#undef COLS_PICK
    h.r0 = j * base + (j < rem ? j : rem);
    h.nrows = gw < a.waves_total ? base + (j < rem ? 1 : 0) : 0;
    return h;
}

// ncg: the columns of this group (1 .. NCOL); c0: its first column
template <int TYPE, int NCOL>
__device__ __forceinline__ void rows_cols_body(const RowsColsArgs &a, const ColsWave &h, uint8_t *smem, int wave, int lane,
                                               int c0, int ncg) {
    constexpr int BSZ = block_bytes(TYPE);
    constexpr int NI = rows_ni(TYPE);
    constexpr int SLOT = rows_slot(TYPE);
    constexpr int D = rows_depth(TYPE);
    static_assert(D >= 2 && D <= 3, "vm_wait_k covers 3 steps in flight");
    const int nb = a.nb, bR = a.bR;
    const int q = lane >> 2, s = lane & 3;
    const RowsColsLayout L = rows_cols_layout(NCOL, nb, a.tmask, bR, a.nbuf, a.rpw);
    uint8_t *const ring = smem + L.ring + wave * L.ring_stride;
    uint8_t *const ring_end = ring + D * SLOT;
    RowRec *const recs = (RowRec *)(smem + L.recs + wave * L.recs_stride);
    float *const outs = (float *)(smem + L.outs + wave * L.outs_stride);
    const uint8_t *const actq = smem + L.act;

    // weight stream of this wave
    const int G = h.nrows * nb;                 // superblocks
    const int T = (G + ROWS_SB - 1) / ROWS_SB;  // steps
    const uint8_t *src = h.w + (int64_t)h.r0 * nb * BSZ;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 15u);
    const uint8_t *s16 = src - mis;
    const uint8_t *last16 = G > 0 ? (const uint8_t *)((uintptr_t)(src + (int64_t)G * BSZ - 1) & ~(uintptr_t)15) : s16;
    uint8_t *islot = ring;
    int it_ = 0;  // next step to issue
    auto issue = [&]() {
        rows_issue_step<TYPE>(s16 + (int64_t)it_ * (ROWS_SB * BSZ) + 16 * lane, last16, islot, lane, it_ + 1 < T);
        islot = islot + SLOT == ring_end ? ring : islot + SLOT;
        ++it_;
    };

    // ---- prologue: the ring behind the activation's DMAs (issued by the caller), one wait
    // that leaves the ring in flight, the workgroup's only barrier
    while (it_ < D && it_ < T) issue();
    vm_wait_k<NI>(it_);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (T == 0) return;

    // ---- main loop
    int io = q, rr = 0;  // quad's (block, row of the wave) of superblock 16t + q
    while (io >= nb) {
        io -= nb;
        ++rr;
    }
    int b0 = 0, par = 0;  // the oldest unreplayed batch: its first row, its record buffer
    const uint8_t *cslot = ring;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        if (T - t >= D) vm_wait<NI * (D - 1)>();  // steady state: D-1 younger steps in flight
        else vm_wait_k<NI>(T - t - 1);
        if (ROWS_SB * t + q < G) {
            int lr = rr - b0;  // row of batch b0, or of the batch after it
            const int sel = lr >= bR ? 1 : 0;
            lr -= sel * bR;
            RowRec *const rec = recs + (((par ^ sel) * bR + lr) * nb + io) * NCOL;
            const QuadW wq = quad_unpack<TYPE>(cslot + mis + q * BSZ, s);
#pragma unroll 1
            for (int c = 0; c < ncg; ++c) {  // (uniform)
                const uint8_t *ab = actq + (c * nb + io) * Q8L_STRIDE;
                const QuadOut r = quad_dot<TYPE>(wq, ab, s);
                const int isum = quad_sum(r.isum);
                const int imin = quad_sum(r.imin);
                if (s == 0) row_rec_store<TYPE>(rec + c, isum, imin, r.dh, *(const float *)ab);
            }
        }
        cslot = cslot + SLOT == ring_end ? ring : cslot + SLOT;
        io += ROWS_SB;
        while (io >= nb) {
            io -= nb;
            ++rr;
        }
        if (it_ < T) issue();
        // batches complete with this step: lane p <-> (row p / NCOL, column p % NCOL)
        const int done = ROWS_SB * (t + 1);
        while (b0 < h.nrows) {  // (uniform)
            const int be = b0 + bR < h.nrows ? b0 + bR : h.nrows;
            if (be * nb > done) break;
            wave_lds_fence();
            const int np = (be - b0) * NCOL;
            for (int p = lane; p < np; p += WAVE) {
                const int r = p / NCOL, c = p % NCOL;
                if (c < ncg) outs[(b0 + r) * NCOL + c] = rows_chain<TYPE>(recs + ((par * bR + r) * nb) * NCOL + c, nb, NCOL);
            }
            b0 = be;
            par ^= 1;
            wave_lds_fence();
        }
    }

    // ---- flush staged results, with the residual ADD (ggml_add: the one f32 add per element)
    wave_lds_fence();
    float *const y = h.y + (int64_t)c0 * h.y_cs + h.r0;
    const float *const res = h.res ? h.res + (int64_t)c0 * h.res_cs + h.r0 : nullptr;
    for (int k = lane; k < h.nrows * NCOL; k += WAVE) {
        const int r = k / NCOL, c = k % NCOL;
        if (c >= ncg) continue;
        float v = outs[k];
        if (res) v = v + res[(int64_t)c * h.res_cs + r];
        cols_store_y(y + (int64_t)c * h.y_cs + r, v);
    }
}

}  // namespace

template <int NCOL>
__global__ void __launch_bounds__(ROWS_COLS_WAVES * 64) kq_rows_cols(const RowsColsArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = wave * (int)gridDim.x + (int)blockIdx.x;  // active waves spread over every CU
    const int c0 = (int)blockIdx.y * NCOL;
    const int ncg = a.m_total - c0 < NCOL ? a.m_total - c0 : NCOL;

    // the group's activation blocks: ncg columns of nb blocks are one contiguous run
    const uint8_t *xg = a.xq + (int64_t)c0 * a.nb * Q8L_STRIDE;
    const int ng = ncg * a.nb * (Q8L_STRIDE / 16);
    for (int j = wave; 64 * j < ng; j += ROWS_COLS_WAVES) {
        const int k = 64 * j + lane;
        if (k < ng) dma16(xg + 16 * k, (LDS void *)(smem + 1024 * j));
    }
    const ColsWave h = cols_resolve(a, gw);
    if (h.type == Q6_K) rows_cols_body<Q6_K, NCOL>(a, h, smem, wave, lane, c0, ncg);
    else if (h.type == Q5_K) rows_cols_body<Q5_K, NCOL>(a, h, smem, wave, lane, c0, ncg);
    else rows_cols_body<Q4_K, NCOL>(a, h, smem, wave, lane, c0, ncg);
}

template __global__ void kq_rows_cols<2>(const RowsColsArgs);
template __global__ void kq_rows_cols<4>(const RowsColsArgs);
template __global__ void kq_rows_cols<8>(const RowsColsArgs);

}  // namespace kq
