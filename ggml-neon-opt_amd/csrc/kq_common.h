// kq_common.h — shared device/host definitions for the gfx950 K-quant kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ggml_mi355x.h"

namespace kq {

constexpr int QK = 256;
constexpr int WAVE = 64;
constexpr int WG_THREADS = 256;     // 4 waves per workgroup
constexpr int WAVES_PER_WG = WG_THREADS / WAVE;
constexpr int LANES_PER_BLOCK = 8;  // 8 lanes cooperate on one superblock
constexpr int BLOCKS_PER_STEP = WAVE / LANES_PER_BLOCK;  // 8 superblocks per wave-step
constexpr int ACT_QS_STRIDE = 272;  // LDS bytes per activation superblock (256 + 16 pad)
constexpr int MAX_NCOL = 8;

constexpr int Q4_K = MI355X_TYPE_Q4_K;
constexpr int Q5_K = MI355X_TYPE_Q5_K;
constexpr int Q6_K = MI355X_TYPE_Q6_K;

__host__ __device__ constexpr int block_bytes(int type) {
    return type == Q4_K ? 144 : type == Q5_K ? 176 : type == Q6_K ? 210 : 0;
}

// Argument block of the GEMV / small-M kernel (passed by value).
struct GemvArgs {
    int n_desc;
    int nb;           // K / 256
    int R;            // rows per task (8: one per lane octet)
    int m_total;      // activation columns in total (grid.y covers ceil(m_total/NCOL))
    int tasks_total;
    int out_per_wg;   // LDS floats for staged outputs (tasks_per_wg * 8 * NCOL)
    int diag;         // diagnostics: bit0 prologue only, bit1 empty
    int ring;         // LDS ring depth D (weight steps in flight per wave)
    int ring_override; // host-side experiment knob (MI355X_GEMV_RING), 0 = auto
    int task_prefix[MI355X_MAX_FUSED + 1];
    int type[MI355X_MAX_FUSED];
    int n_rows[MI355X_MAX_FUSED];
    const uint8_t *w[MI355X_MAX_FUSED];
    int64_t row_stride[MI355X_MAX_FUSED];  // bytes
    float *y[MI355X_MAX_FUSED];
    int64_t y_col_stride[MI355X_MAX_FUSED];  // floats between dst columns
    const float *x;       // f32 input (FUSEDQ): column j at x + j*x_col_stride
    int64_t x_col_stride; // floats
    const uint8_t *xq;    // Q8_K input (!FUSEDQ): column j at xq + j*xq_col_stride
    int64_t xq_col_stride; // bytes
    int32_t *dbg;         // debug partials (DEBUG builds of the kernel only)
    uint64_t *stamps;     // diagnostics: per-wave s_memrealtime stamps (or null)
    int64_t stamps_cap;   // entries available in stamps
};

// LDS layout of one workgroup (dynamic shared memory).
//   ring: per wave D slots of `slot` bytes (8 rows x one superblock)
//   act:  per wave, its K-range of activations (f32 staging / raw Q8_K per column)
//   recs: 2 task slots x 3 waves x ncol x 8 rows x spw exact chain records
//   outs: staged results of wave 0 (tasks_per_wg x ncol x 8 floats)
struct LdsLayout {
    int ring, act, act_per_wave, act_col, recs, outs, spw, total;
};

__host__ __device__ inline LdsLayout lds_layout(int ncol, int nb, int out_per_wg, bool fusedq, int slot, int D) {
    LdsLayout L;
    L.spw = (nb + WAVES_PER_WG - 1) / WAVES_PER_WG;  // max superblocks per wave per task
    L.ring = 0;
    L.act = WAVES_PER_WG * D * slot;
    L.act_col = (L.spw * 292 + 16 + 15) & ~15;
    L.act_per_wave = fusedq ? L.spw * 1024 : ncol * L.act_col;
    L.recs = L.act + WAVES_PER_WG * L.act_per_wave;
    L.outs = L.recs + 2 * (WAVES_PER_WG - 1) * ncol * 8 * L.spw * 16;
    L.total = L.outs + out_per_wg * 4;
    return L;
}

// ---------------------------------------------------------------- row-stream decode GEMV
// kq_rows (M = 1): one workgroup of ROWS_WAVES waves per CU. Global wave index
// gw = wave * gridDim.x + blockIdx.x (active waves spread over every CU). Matrix d
// owns global waves [wave_prefix[d], wave_prefix[d+1]); its j-th wave owns rows
// [j*rbase[d] + min(j, rrem[d]), ...) — rbase[d] rows, one more for j < rrem[d].
#ifndef KQ_ROWS_WAVES
#define KQ_ROWS_WAVES 12
#endif
constexpr int ROWS_WAVES = KQ_ROWS_WAVES;  // the most waves per workgroup (LDS layout, launch bounds)
// Small launches run ROWS_WAVES_SMALL waves per workgroup (the wave count is a launch
// parameter, passed in `cfg`): fewer waves to dispatch for a stream that is short anyway.
#ifndef KQ_ROWS_WAVES_SMALL
#define KQ_ROWS_WAVES_SMALL 6
#endif
constexpr int ROWS_WAVES_SMALL = KQ_ROWS_WAVES_SMALL;
constexpr int ROWS_QPASS = 3;  // fused-quantization passes of 4*ROWS_WAVES superblocks

// Kernel entry (kq_rows, kq_rows_dyn): what a wave needs before its first memory request comes
// as leading plain parameters, 14 dwords, which the kernarg preload puts in SGPRs at wave start
// (the activation loads then issue with no scalar-memory trip): x (the Q8L row when !FUSEDQ),
// x2, the first matrix's w / res, nb, waves_total, the grid size, `cfg` (rows_cfg: waves per
// workgroup, the prologue's pass count, n_desc, the diagnostic bits), the first matrix's
// rbase / rrem. RowsArgs follows; the kernels read its first run (up to `stamps_cap`) in ONE
// batch of scalar loads behind one wait (rows_resolve, kq_rows.hip) and pick per-matrix values
// from the loaded arrays. The kernels read neither gridDim nor blockDim, and nothing of the
// host's plan below that run.
#define KQ_ROWS_PARAMS                                                                                        \
    const void *x, const float *x2, const uint8_t *w0, const float *res0, int nb, int waves_total, int grid, \
        int cfg, int rbase0, int rrem0, const RowsArgs a
__host__ __device__ constexpr int rows_cfg(int nwv, int qiters, int n_desc, int diag) {
    return nwv | (qiters << 8) | (n_desc << 12) | (diag << 16);
}
// The fused prologue's mapping of the activation row to the workgroup: 16 << lsh lanes
// quantize one superblock (16, 8 or 4 consecutive values per lane), the widest form with
// nb * lanes <= 64 * nwv, so that one pass covers the row with as many of the workgroup's
// waves as it has; rows that fill the workgroup anyway keep 16 lanes per superblock and as
// many passes of 4 * nwv superblocks as they need (up to ROWS_QPASS). `steps`: the most
// 16-superblock steps any wave of the launch streams. The wide forms pay in the short,
// latency-bound launches (K = 2048 at 6 waves -0.13 to -0.2 us, K = 5632 at 12 waves -0.27 us);
// a launch whose waves stream many steps loses with them (Llama-3-8B gate + up, 10 steps per
// wave: 9.88 -> 10.94 us, profiles/r08_prologue_ab.txt) and keeps 16 lanes.
constexpr int ROWS_PRO_WIDE_STEPS = 2;  // wide forms up to this many steps per wave
struct RowsProForm {
    int lsh, passes;
};
__host__ __device__ constexpr RowsProForm rows_pro_form(int nb, int nwv, int64_t steps = 0) {
    const bool wide = steps <= ROWS_PRO_WIDE_STEPS;
    return wide && nb * 64 <= 64 * nwv   ? RowsProForm{2, 1}
           : wide && nb * 32 <= 64 * nwv ? RowsProForm{1, 1}
                                         : RowsProForm{0, (nb + 4 * nwv - 1) / (4 * nwv)};
}

// The short-stream form of kq_rows (its template parameter SH), chosen by the host per launch:
// every matrix's longest wave streams no more steps than the ring of its type holds (steps <=
// depth, for the matrix with the least room: the whole stream is issued before the prologue's
// barrier and nothing after it), and one chain batch covers a wave's rows (bR >= rpw). Only the fused-quantization kernels have the form.
__host__ __device__ constexpr bool rows_short_form(int64_t steps, int depth, int bR, int rpw) {
    return steps <= depth && bR >= rpw;
}

struct RowsArgs {
    // ---- the run the kernels read at entry (one batch)
    int bR;           // rows per chain batch (bR*nb % 16 == 0 unless bR >= rpw)
    int rpw;          // max rows per wave (LDS sizing)
    int wave_prefix[MI355X_MAX_FUSED + 1];
    // SWIGLU epilogue (epi != 0): y[0] = gate, y[1] = up with equal rows and wave counts,
    // up wave `wave` pairs with gate wave `wave - epi_wave_off` of the same workgroup
    // (identical row ranges); epi_y[r] = swiglu(gate[r], up[r]) for r < epi_n
    int epi;
    int rbase[MI355X_MAX_FUSED];
    int rrem[MI355X_MAX_FUSED];
    int type[MI355X_MAX_FUSED];
    const uint8_t *w[MI355X_MAX_FUSED];
    // fused neighbours of the MUL_MAT in the decode graph (FUSEDQ only):
    const float *res[MI355X_MAX_FUSED];  // y[m] = mul_mat + res[m] (the ADD after the MUL_MAT), or null
    float *y[MI355X_MAX_FUSED];
    float *epi_y;
    float eps;            // ROWS_PRO_NORM: rms_norm epsilon
    int epi_n, epi_wave_off;
    // kq_rows_dyn (claimed rows): workgroup b owns rows [b*N/G, (b+1)*N/G) of every matrix
    // (rpw = the most such rows over the matrices, summed); its waves claim units of dyn_u
    // rows from an LDS counter, the first dyn_p units of each wave assigned statically
    int dyn_u, dyn_p, dyn_ush;  // (dyn_u = 1 << dyn_ush; rbase[0] / rrem[0]: the rows N / G split)
    int n_rows[MI355X_MAX_FUSED];
    uint64_t *stamps;     // diagnostic builds
    int64_t stamps_cap;
    // ---- the host's plan; what the kernels need of it travels as leading parameters
    int n_desc;
    int nb;           // K / 256
    int waves_total;
    const float *x;       // f32 activation (FUSEDQ)
    const uint8_t *xq;    // Q8L activation row (!FUSEDQ), written by kq_quantize_q8L
    const float *x2;      // ROWS_PRO_NORM: norm weight (the MUL after RMS_NORM); ROWS_PRO_SWIGLU: up (x = gate)
    int pro;              // ROWS_PRO_*: transform of x before its Q8_K quantization
    int diag;         // diagnostics (timing only): bit3 stream weights only, 16/32 prologue, 64 no quantization, 128 no SWIGLU epilogue, 256 empty launch
    // ---- recorded plan fields (mi355x_debug_rows_plan, tests/golden/rows_plans.json): no kernel
    // reads them any more; the kernels issue one weight step before the activation wait and
    // set no wave priority
    int pre0;         // the GEMV_PRE0 knob: weight steps once issued before the activation was quantized
    int64_t prio_bytes;  // the most weight bytes any wave streams
};
constexpr int ROWS_PRO_NONE = 0, ROWS_PRO_NORM = 1, ROWS_PRO_SWIGLU = 2;

// One step = 16 consecutive superblocks of a wave's row stream (2304 / 2816 / 3360
// B), fetched as 16-B granules from the 16-B boundary below them (+1 granule of
// slack for a misaligned Q6_K stream): 145 / 177 / 211 granules = 3 / 3 / 4
// LDS-DMA instructions. Ring depth per type keeps 6.8-8.5 KB in flight per wave,
// ~80-100 KB per CU (measured ceiling: 2-3 KB steps, ~96 KB per CU, nt -> 7.1 TB/s).
constexpr int ROWS_SB = 16;     // superblocks per step (4 lanes each)
constexpr int Q8L_STRIDE = 304; // LDS/workspace Q8_K block: d @0, qs @16, bsums @272 (16-B aligned)
// kq_mmq tiles (RT weight rows x 64*CW columns), two superblock buffers in LDS each.
// The waves form two column groups: a wave takes 32 rows x 32 * CW of the tile's 64 * CW columns.
__host__ __device__ constexpr int mmq_cols(int cw) { return 64 * cw; }
__host__ __device__ constexpr int mmq_waves(int rt, int cw) { return rt / 16; }
// Q6_K rows staged at MMQ_Q6_STRIDE bytes: the 14 granules of a 210-B block (fetched from
// the 16-B boundary below it, 224 B) plus one padding granule at 240, so consecutive rows start
// 60 dwords apart (16 bank offsets) instead of 56 (8): the tile's realigned row reads
// conflicted for 71 % of the LDS's active cycles at 224 (profiles/r06_prefill_stall.md).
constexpr int MMQ_Q6_STRIDE = 240;
static_assert(MMQ_Q6_STRIDE % 16 == 0 && MMQ_Q6_STRIDE >= 224, "whole granules");
__host__ __device__ constexpr int mmq_buf_bytes(int type, int rt, int cw) {
    return mmq_cols(cw) * Q8L_STRIDE + rt * (type == Q6_K ? MMQ_Q6_STRIDE : block_bytes(type));
}
constexpr int ROWS_RECS = 64;   // chain records per wave per batch (soft cap)
__host__ __device__ constexpr int rows_gran(int type) { return block_bytes(type) + 1; }
__host__ __device__ constexpr int rows_slot(int type) { return 16 * rows_gran(type); }
__host__ __device__ constexpr int rows_ni(int type) { return (rows_gran(type) + 63) / 64; }
#ifndef KQ_ROWS_DQ4
#define KQ_ROWS_DQ4 3
#endif
#ifndef KQ_ROWS_DQ6
#define KQ_ROWS_DQ6 2
#endif
__host__ __device__ constexpr int rows_depth(int type) {
    return type == Q4_K ? KQ_ROWS_DQ4 : type == Q5_K ? 3 : KQ_ROWS_DQ6;
}
__host__ __device__ constexpr int rows_ring_bytes(int type) { return rows_depth(type) * rows_slot(type); }
__host__ __device__ constexpr int cmax(int a, int b) { return a > b ? a : b; }
__host__ __device__ constexpr int rows_ring(int tmask) {
    return 16 + cmax((tmask & 1) ? rows_ring_bytes(Q4_K) : 0,
                     cmax((tmask & 2) ? rows_ring_bytes(Q5_K) : 0, (tmask & 4) ? rows_ring_bytes(Q6_K) : 0));
}

//   act:  Q8_K activation row in the aligned Q8L layout (nb * 304 B)
//   ring: per wave, the ring of its type (+16 B tail slack for Q6_K realign reads)
//   recs: per wave bR*nb chain records (16 B), block-major [blk][row]
//   outs: per wave rpw staged results
struct RowsLayout {
    int act, ring, ring_stride, recs, recs_stride, outs, outs_stride, sums, total;
};
// nwv = the launch's waves per workgroup (blockDim.x / 64)
__host__ __device__ inline RowsLayout rows_layout(int nb, int tmask, int bR, int rpw, int nwv) {
    RowsLayout L;
    L.act = 0;
    L.ring = nb * Q8L_STRIDE;
    L.ring_stride = rows_ring(tmask);
    L.recs = L.ring + nwv * L.ring_stride;
    L.recs_stride = bR * nb * 16;
    L.outs = L.recs + nwv * L.recs_stride;
    L.outs_stride = (rpw * 4 + 15) & ~15;
    L.sums = L.outs + nwv * L.outs_stride;  // ROWS_PRO_NORM: per-superblock sums of squares (double)
    L.total = L.sums + nb * 8;
    return L;
}

// kq_rows_dyn: act | ring (per wave) | recs (per wave: a batch of bR rows, bR x nb records) |
// outs (the workgroup's rows of every matrix, flat) | sums | claim counter
struct RowsDynLayout {
    int act, ring, ring_stride, recs, recs_stride, outs, sums, cnt, total;
};
__host__ __device__ inline RowsDynLayout rows_dyn_layout(int nb, int tmask, int bR, int flat_rows, int nwv) {
    RowsDynLayout L;
    L.act = 0;
    L.ring = nb * Q8L_STRIDE;
    L.ring_stride = rows_ring(tmask);
    L.recs = L.ring + nwv * L.ring_stride;
    L.recs_stride = bR * nb * 16;
    L.outs = L.recs + nwv * L.recs_stride;
    L.sums = L.outs + ((flat_rows * 4 + 15) & ~15);
    L.cnt = L.sums + nb * 8;
    L.total = L.cnt + 16;
    return L;
}

// Decode attention block (kq_attn_decode.hip): one workgroup per query head.
struct AttnArgs {
    const float *q, *k, *v;       // projections of this token (before rope)
    const int32_t *pos;           // device: the token's position (cache cell)
    const float *rope_table;      // [n_ctx][head_dim/2][cos, sin]
    uint16_t *k_cache;            // f16 [n_ctx][n_head_kv*head_dim]
    uint16_t *v_cache;            // f16 [n_head_kv*head_dim][n_ctx] (transposed, non-FA layout)
    float *out;                   // [n_head*head_dim]
    int n_ctx, n_head, n_head_kv, head_dim;
    float scale;
    int diag;  // diagnostics only (MI355X_ATTN_DIAG): 1/2/3 stop after loads/KQ/soft_max, 4 empty
    int rope_row;  // rope_table holds only the row of *pos (no position-dependent load)
    int no_store;     // prompt batch: the KV cells are already stored (the k/v GEMM's epilogue)
    uint8_t *q8_out;  // prompt batch (kq_attn_prompt_group): also the output rows as Q8L blocks
                      // for the next GEMM (row i's superblock b at (i*nb + b)*304), or null
    int reserved0;    // unused, written as 0 (keeps the offsets attn_entry reads the struct at)
    int n_tok;        // prompt batch (kq_attn_prompt_group), set by launch_attn_prompt: its tokens
};

// Batched attention with the KV cells and the mask read from the graph's inputs
// (kq_attn_batch.hip): `a` as for a prompt batch (rows per token, rope_row 0).
struct AttnBatchArgs {
    AttnArgs a;
    const void *cells;        // device int32 / int64 [n_tok]: token i's cache cell
    const void *mask;         // device f16 / f32: token i's row at mask + i * mask_row_bytes, >= n_kv entries
    int64_t mask_row_bytes;
    int cells_i64, mask_f16;
    int n_kv;                 // the row: cells [0, n_kv), n_kv % 32 == 0, <= a.n_ctx
    int n_tok;
    int n_pos;                // rows of the rope table: a position outside [0, n_pos) has no cell
    int per_head;             // set by launch_attn_batch: one workgroup per query head, not per kv group
};

// Decode attention fused with the o-proj GEMV (kq_attn_oproj.hip): workgroup (s, rb) runs the
// attention of the heads of superblock s of the o-proj's K, quantizes them (one Q8_K
// superblock) and writes the exact per-superblock records of rows [rb*R, rb*R + R); the
// last of the nsb workgroups of row block rb replays each row's chain in superblock order.
struct AttnOprojArgs {
    AttnArgs at;              // the attention (this node's heads; at.out unused)
    const uint8_t *w;         // o-proj weights: n_rows rows of nsb superblocks, row_stride bytes
    int64_t row_stride;
    int n_rows, nsb, R, n_rb;
    int head_lds;             // LDS bytes per head (attn_lds, 16-B multiple)
    const float *res;         // residual (ggml_add after the mul_mat), or null
    float *y;                 // n_rows outputs
    uint8_t *recs;            // [n_rb][R][nsb] 16-B records (written sc1, read sc1)
    uint32_t *cnt;            // [n_rb] arrival counters (monotonic: last = old % nsb == nsb - 1)
};

// ---------------------------------------------------------------- persistent decode layer
// kq_layer (kq_layer.hip): one llm_build_llama decode layer as ONE launch of one workgroup
// per CU. Stages: 0 q/k/v (attn_norm prologue), attention, 1 o-proj (+ x -> x1),
// 2 gate/up (ffn_norm prologue, SWIGLU -> h), 3 down (+ x1 -> x2). Matrices m: 0 q, 1 k,
// 2 v, 3 o, 4 gate, 5 up, 6 down. Edges e (counter sets in `sync`): 0 q/k/v -> attention,
// 1 attention -> o-proj, 2 x1 -> gate/up, 3 h -> down.
constexpr int LAYER_WAVES = 8;       // 7 weight-stream waves + 1 control wave
constexpr int LAYER_SYNC_U32 = 32 * 33;  // epoch + 4 edges x 8 shards, each on its own 128-B line
struct LayerArgs {
    int G;                           // workgroups (one per CU, all co-resident)
    int E, F, nb_e, nb_f, nq, nkv;   // embd, ffn, K / 256 of each; rows of attn_q, attn_k (= attn_v)
    int type[7];
    const uint8_t *w[7];             // contiguous rows of K / 256 blocks
    float *y[3];                     // q / k / v (written sc1: the attention's inputs)
    const float *x;                  // layer input (written by the previous launch)
    const float *attn_norm, *ffn_norm;
    float eps;
    float *att, *x1, *h, *x2;        // attention output, ffn_inp = o + x, swiglu(gate, up), layer output
    AttnArgs at;                     // q / k / v = y[0..2], rope_row staged with the position
    int n_attn, hpw, attn_stride, head_lds;  // attention workgroups, heads per workgroup, placement
    uint32_t *sync;                  // this launch's counter block (LAYER_SYNC_U32 words, zeroed once)
    int *err;                        // set when a wait timed out (co-residency lost): results invalid
    uint32_t expect[4][8];           // producers per edge and shard
    int D, slot;                     // ring slots per stream wave, bytes per slot
    int o_aux, act_bytes, o_sums, o_res, lds;  // LDS layout (ring at 0)
    const uint8_t *tab;              // every workgroup's step table (layer_table_fill), tab_stride bytes apart
    int64_t tab_stride;
    uint64_t *stamps;                // KQ_LAYER_STAMPS builds: 32 s_memrealtime stamps per workgroup
    int64_t stamps_cap;
};

// ---------------------------------------------------------------- batched (prefill) MFMA GEMM
// kq_mmq (M > 1): RT x 64 * CW output tiles (RT 64 / 128 rows, CW 1 / 2), Q8L activations in a workspace.
struct MmqArgs {
    const uint8_t *w;        // weight rows (16-B aligned, row_stride % 16 == 0)
    int64_t row_stride;      // bytes
    int n_rows;
    const uint8_t *xq;       // Q8L activation columns
    int64_t xq_col_stride;   // bytes (nb * 304)
    int m_cols;
    float *y;                // dst column j at y + j * y_col_stride
    int64_t y_col_stride;    // floats
    int nb;
    const float *res;        // ADD epilogue (null: none): y = mul_mat + res, res column j at
    int64_t res_col_stride;  //   res + j * res_col_stride (the one f32 add of ggml_add)
    // kq_mmq over up to 4 matrices of one type sharing the activation
    // (q/k/v of a prompt batch): row tiles [tile0[d], tile0[d+1]) are matrix d's; n_mat 1:
    // the fields above only
    int n_mat;
    int tile0[5];
    int mtype[4];  // kq_mmq_mixed: each matrix's type (Q4_K / Q5_K / Q6_K)
    // KV-cache store epilogue of a prompt's k / v projections (kv_kind[d]: 1 k -> rope ->
    // f16 cache rows, 2 v -> f16 transposed cache; 0 none); kv_cur: this tile's matrix
    int kv_kind[4], kv_cur;
    const int32_t *kv_pos;   // cell of each column (token)
    const float *kv_rope;    // [n_ctx][head_dim/2][cos, sin]
    uint16_t *kv_k_cache, *kv_v_cache;
    int kv_n_ctx, kv_hd;
    const uint8_t *mw[4];
    int64_t mrow_stride[4];
    int mn_rows[4];
    float *my[4];
    int64_t my_col_stride[4];
};

// ---------------------------------------------------------------- expert-grouped MoE prefill
// The group table kq_moe_group (kq_moe.hip) builds from a MOE_ROUTE node's ids at every launch and
// kq_mmq_id (kq_mmq.hip) reads: int32 words. Bucket e < n_expert holds the (token, slot) pairs
// routed to expert e, bucket n_expert those whose id lies outside the table. Per bucket the pair
// count, the bucket's first entry in the sorted lists and its first column tile, for tiles of 64
// and of 128 columns (prefixes of ceil(count / 64) and ceil(count / 128); entry n_expert + 1 is
// the total). Then the two sorted lists of
// `pairs` entries each: the pair index p = t * n_used + s (the output row, and the activation
// row of an ne11 == n_used source) and the token t (the activation row of an ne11 == 1 source),
// so the GEMM divides nothing. The order of the pairs inside a bucket is unspecified.
constexpr int MOE_BUCKETS = MI355X_MOE_MAX_EXPERTS + 1;
constexpr int MOE_TAB_COUNT = 0, MOE_TAB_FIRST = 72, MOE_TAB_TILE0 = 144, MOE_TAB_TILE0W = 216, MOE_TAB_LIST = 288;
__host__ __device__ constexpr int moe_tab_tile0(int cw) { return cw == 2 ? MOE_TAB_TILE0W : MOE_TAB_TILE0; }  // kq_mmq_id's CW
static_assert(MOE_TAB_FIRST >= MOE_BUCKETS && MOE_TAB_TILE0 >= MOE_TAB_FIRST + MOE_BUCKETS &&
                  MOE_TAB_TILE0W >= MOE_TAB_TILE0 + MOE_BUCKETS + 1 && MOE_TAB_LIST >= MOE_TAB_TILE0W + MOE_BUCKETS + 1,
              "the four per-bucket arrays before the lists");
__host__ __device__ constexpr int64_t moe_table_words(int64_t pairs) { return MOE_TAB_LIST + 2 * pairs; }
// kq_mmq_id: what differs from kq_mmq. Of MmqArgs: w the expert tensor's base, m_cols unused
// (a tile's columns end with its bucket), y_col_stride the rows of an expert (y packed).
struct MmqIdArgs {
    const int32_t *tab;   // the group table
    const int32_t *xrow;  // sorted entry -> Q8L row of the workspace (the token or the pair list)
    const int32_t *pair;  // sorted entry -> pair index: its outputs at y + pair * y_col_stride
    int64_t nb02;         // bytes between experts
    int n_expert;
};

// ------------------------------------------- batched (prefill) f16 MFMA GEMM, stated tolerance
// kq_mmf (MI355X_PREFILL_F16): 128 weight rows x 128 activation columns per 4-wave
// workgroup, K in half-superblock steps. The activation goes through kq_quantize_f16img
// (the reference's Q8_K quantization, then f16(d*q) in the kernel's k order, 512 B per
// superblock, plus f16(d*bsum16) x 16 = 32 B), the weights are dequantized in registers.
constexpr int MMF_RT = 128;                      // weight rows per workgroup (4 waves x 32)
constexpr int MMF_COLS = 128;                    // activation columns per workgroup (4 MFMA tiles)
constexpr int MMF_IMG = 512;                     // f16 image bytes per superblock and column
constexpr int MMF_BSB = 32;                      // f16 d*bsum16 bytes per superblock and column
constexpr int MMF_BUF = MMF_COLS * (MMF_IMG / 2 + MMF_BSB);  // one half-superblock LDS buffer (36 KB)
struct MmfArgs {
    const uint8_t *w;          // weight rows
    int64_t row_stride;        // bytes
    int n_rows;
    const uint8_t *img;        // activation image, column j at img + j * nb * 512
    const uint8_t *bs;         // d*bsum16, column j at bs + j * nb * 32
    int m_cols;
    float *y;                  // dst column j at y + j * y_col_stride (n_split == 1)
    int64_t y_col_stride;      // floats
    float *slab;               // n_split > 1: partial sums [n_split][m_cols][n_rows]
    int nb;                    // superblocks of K
    int nbs;                   // superblocks per K split
    int n_split;
    int n_ct;                  // column tiles
    int n_rt;                  // row tiles
    int order;                 // tile order (speed only): 0 row tiles, 1 column tiles consecutive per XCD
    const float *res;          // ADD epilogue (null: none): y = mul_mat + res, column j at
    int64_t res_col_stride;    //   res + j * res_col_stride
    // up to 4 matrices of one type on one activation image in one launch (a prompt batch's
    // q/k/v or gate/up): row tiles [tile0[d], tile0[d+1]) are matrix d's, its rows are slab
    // columns [roff[d], roff[d] + mn_rows[d]) of n_rows (the sum); n_mat 1: the fields above
    int n_mat;
    int tile0[5];
    int roff[4];
    const uint8_t *mw[4];
    int64_t mrow_stride[4];
    int mn_rows[4];
    float *my[4];
    int64_t my_col_stride[4];
};

}  // namespace kq
