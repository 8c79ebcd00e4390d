// kq_prefill_host.hip — host path of the prefill GEMMs (ne11 >= kMmqMinCols): the bit-exact
// int8 tiles (kq_mmq: tile shape, LDS, launches) and the f16 matrix-core path (kq_mmf: the
// activation image, split-K plan, workspace, launches), with their selectors.
#include <algorithm>
#include <string.h>

#include <atomic>
#include <string>

#include "kq_common.h"
#include "kq_internal.h"

namespace kq {

template <int TYPE, int RT, int CW>
__global__ void kq_mmq(const MmqArgs a);
template <int RT, int CW>
__global__ void kq_mmq_mixed(const MmqArgs a);
__global__ void kq_quantize_f16img(const float *x, int64_t x_stride, uint8_t *img, uint8_t *bs, int nb, int64_t nblocks);
template <int TYPE, int NW>
__global__ void kq_mmf(const MmfArgs a);
__global__ void kq_mmf_reduce(const float *slab, int n_split, int m_cols, int n_rows, int slab_rows, float *y,
                              int64_t y_col_stride, const float *res, int64_t res_col_stride);

namespace {
std::atomic<int> g_mmq_impl{MI355X_MMQ_AUTO};  // mi355x_mmq_impl()
std::atomic<int> g_prefill{MI355X_PREFILL_EXACT};
}  // namespace

// ------------------------------------------------------------ batched MFMA path
// Prefill tile selector, set only through mi355x_mmq_impl (the library reads no environment):
// AUTO (mmq_shape's choice by grid) or one tile shape forced (the four AUTO chooses among, or
// the selector-only 192 x 64).
int mmq_impl() { return g_mmq_impl.load(); }
void mmq_impl_set(int impl) { g_mmq_impl.store(impl); }

// Prefill tile shape (kq_mmq's RT x CW): weight rows per workgroup RT = 64 (4 waves) or 128
// (8 waves: the activation tile fetched once per 128 rows), activation columns 64 * CW (CW = 2:
// each wave's weight operands feed two MFMA column tiles, half the operand-building vector
// work per MFMA). AUTO, by the grid each shape would launch (profiles/r03_mmq_tiles.txt):
//  * a grid of >= 160 workgroups at 128 x 128: 128 x 128 (TinyLlama Q6_K head 256 -> 167 us,
//    gate/up 28.3 -> 26.0, 8B ffn_up 98 -> 95, 8B Q5_K ffn_up 147 -> 125); on 128-workgroup
//    grids it loses 30-40 % (half the CUs idle);
//  * else Q6_K whose 64 x 128 grid has >= 192 workgroups: 64 x 128 (one 4-wave workgroup
//    per CU, every register: 8B Q6_K ffn_down 219-226 -> 192-194 us; Q4_K / Q5_K are slower
//    on it);
//  * else Q4_K / Q5_K whose 128 x 64 grid has >= 256 workgroups: 128 x 64 (8B q/o 33 -> 31,
//    ffn_down 108-116 -> 101-106; Q5_K q/o 42.4 -> 40.5, ffn_down 132 -> 128 with the
//    three-MFMA Q5_K split, profiles/r03_mmq_q5_tiles.txt);
//  * else 64 x 64 (small grids).
struct MmqShape {
    int rt, cw;
};
MmqShape mmq_shape(int type, int64_t rows, int64_t M) {
    const int impl = mmq_impl();
    if (impl == MI355X_MMQ_TILE128) return {128, 1};
    if (impl == MI355X_MMQ_TILE128W) return {128, 2};
    if (impl == MI355X_MMQ_TILE64W) return {64, 2};
    if (impl == MI355X_MMQ_TILE64) return {64, 1};
    if (impl == MI355X_MMQ_TILE192) return type == Q6_K ? MmqShape{128, 1} : MmqShape{192, 1};
    const int64_t rt128 = (rows + 127) / 128;
    const int64_t g128x128 = rt128 * ((M + 127) / 128), g128x64 = rt128 * ((M + 63) / 64);
    // a 128 x 128 grid that fills under ~3/4 of two workgroups per CU, where the 128 x 64 one
    // has two per CU: 128 x 64 (TinyLlama's 11264-row gate+up at M = 512: 352 against 704
    // workgroups, 49.8 -> 41.6 us; Llama-3-8B ffn_up's 448 keep 128 x 128, 95 against 97 us;
    // profiles/r05_mmq_tl_tiles.txt)
    if (type != Q6_K && g128x128 >= 160 && g128x128 < 384 && g128x64 >= 512) return {128, 1};
    if (g128x128 >= 160) return {128, 2};
    if (type == Q6_K && ((rows + 63) / 64) * ((M + 127) / 128) >= 192) return {64, 2};
    if (type != Q6_K && rt128 * ((M + 63) / 64) >= 256) return {128, 1};
    return {64, 1};
}
const void *mmq_fn(int type, bool mixed, MmqShape sh) {
#define KQ_MMQ_PICK(RT, CW)                                                      \
    return mixed          ? (const void *)kq_mmq_mixed<RT, CW>                 \
         : type == Q5_K ? (const void *)kq_mmq<Q5_K, RT, CW>                   \
         : type == Q6_K ? (const void *)kq_mmq<Q6_K, RT, CW>                   \
                        : (const void *)kq_mmq<Q4_K, RT, CW>;
    if (sh.rt == 192 && !mixed && type != Q6_K)
        return type == Q5_K ? (const void *)kq_mmq<Q5_K, 192, 1> : (const void *)kq_mmq<Q4_K, 192, 1>;
    if (sh.rt == 128 && sh.cw == 2) KQ_MMQ_PICK(128, 2)
    if (sh.rt == 64 && sh.cw == 2) KQ_MMQ_PICK(64, 2)
    if (sh.rt == 128) KQ_MMQ_PICK(128, 1)
    KQ_MMQ_PICK(64, 1)
#undef KQ_MMQ_PICK
}
// two superblock buffers: mmq_cols(cw) Q8L columns + rt weight rows (Q6_K: MMQ_Q6_STRIDE, the 224-B
// granule span + padding), +16 B for the Q6_K realign reads past the last row
size_t mmq_lds(int type, MmqShape sh) { return 2 * (size_t)mmq_buf_bytes(type, sh.rt, sh.cw) + 16; }

// ------------------------------------------- prefill on the f16 matrix core (stated tolerance)
// mi355x_prefill_precision: MI355X_PREFILL_EXACT (kq_mmq, bit-exact, the default) or
// MI355X_PREFILL_F16 (kq_mmf: the reference's Q8_K activation and integer unpacking, the
// accumulated dot on v_mfma_f32_32x32x16_f16 within the tolerance of kq_mmf.hip's header).
// Set only through mi355x_prefill_precision(): the numerics never change from the environment.
int prefill_precision() { return g_prefill.load(); }
void prefill_precision_set(int precision) { g_prefill.store(precision); }

// Waves per kq_mmf workgroup (MI355X_MMF_WAVES, A/B only): 4 (128-row workgroups, two per
// CU) or 8 (256-row workgroups, one per CU); 0 by shape: 8 from K >= 8192, where the
// activation tile's refill is the longer wait (8B ffn_down Q4_K 99-106 -> 88-96 us, Q6_K
// 134 -> 117-122, Q5_K 104 -> 93), 4 below it (8B ffn_up 82.5 vs 99.7 us on 8 waves:
// its 224-workgroup grid leaves CUs idle) -- profiles/r03_mmf_waves_ab.txt.
int mmf_nw(int64_t K) {
    const int v = (int)knob(KNOB_MMF_WAVES);
    return v == 4 || v == 8 ? v : K >= 8192 ? 8 : 4;
}
// K split of kq_mmf: double it while the grid has fewer workgroups than CUs and every
// split keeps >= 4 superblocks (8 half-superblock steps); splits combine in order (NW = 4:
// filling both resident slots per CU with a 4-way split measured slower on 8B q/o, 34 ->
// 37 us).
struct MmfPlan {
    int nw, n_ct, n_rt, n_split, nbs;
};
MmfPlan mmf_plan_nw(int64_t N, int64_t M, int64_t nb, int nw) {
    MmfPlan p;
    p.nw = nw;
    p.n_ct = (int)((M + MMF_COLS - 1) / MMF_COLS);
    p.n_rt = (int)((N + 32 * nw - 1) / (32 * nw));
    int s = 1;
    while ((int64_t)p.n_ct * p.n_rt * s < 256 && nb >= 8 * s) s *= 2;
    p.nbs = (int)((nb + s - 1) / s);
    p.n_split = (int)((nb + p.nbs - 1) / p.nbs);
    return p;
}
size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
// workspace: activation image + d*bsum16 (+ the split-K slabs of either tile shape)
size_t mmf_workspace(int64_t N, int64_t M, int64_t nb) {
    size_t w = al256((size_t)M * nb * MMF_IMG) + al256((size_t)M * nb * MMF_BSB), slab = 0;
    for (int nw = 4; nw <= 8; nw += 4) {
        const MmfPlan p = mmf_plan_nw(N, M, nb, nw);
        const size_t sb = p.n_split > 1 ? al256((size_t)p.n_split * M * N * 4) : 0;
        slab = sb > slab ? sb : slab;
    }
    return w + slab;
}
// Where the f16 path is the faster one (M = 512, profiles/r03_mmf_*): Q5_K and Q6_K
// everywhere; Q4_K from N*K >= 32 M elements (8B ffn_up / ffn_down), while the int8 tiles
// stay ahead on the smaller Q4_K GEMMs (8B q/o 36 vs 38 us, TinyLlama gate 31 vs 36 us).
// The precision switch promises the stated tolerance, which the bit-exact kernel meets
// trivially; MI355X_PREFILL_F16_ALL forces the f16 kernel on every shape (A/B, tests).
bool mmf_prefers(int type, int64_t N, int64_t K) {
    return prefill_precision() == MI355X_PREFILL_F16_ALL || type != Q4_K || N * K >= ((int64_t)32 << 20);
}
bool mmf_applies(int type, const void *w, int64_t N, size_t row_stride, int64_t M, int64_t K) {
    if (prefill_precision() < MI355X_PREFILL_F16) return false;
    if (!rows_enabled() || M < kMmqMinCols || N <= 0) return false;
    if (type != Q4_K && type != Q5_K && type != Q6_K) return false;
    if (N >= (1ll << 31) || M >= (1ll << 31)) return false;
    if (!mmf_prefers(type, N, K)) return false;
    if (type == Q6_K) return true;  // 210-B blocks: unaligned vector loads
    return ((uintptr_t)w & 15u) == 0 && (row_stride & 15u) == 0;
}

bool mmf_on() { return prefill_precision() >= MI355X_PREFILL_F16; }

int launch_f16img(const float *x, int64_t x_stride, uint8_t *ws, int64_t K, int64_t M, hipStream_t stream) {
    const int64_t nb = K / QK;
    uint8_t *img = ws, *bs = ws + al256((size_t)M * nb * MMF_IMG);
    const int64_t nblocks = nb * M;
    if (nblocks == 0) return MI355X_OK;
    const int64_t qwgs = (nblocks + WAVES_PER_WG - 1) / WAVES_PER_WG;
    return timed_launch("kq::kq_quantize_f16img", (double)nblocks * (QK * 4.0 + MMF_IMG + MMF_BSB), kq_quantize_f16img,
                        dim3((unsigned)qwgs), dim3(WG_THREADS), 0, stream, x, x_stride, img, bs, (int)nb, nblocks);
}

int launch_mmf_multi(int type, int n_mat, const void *const *w, const int64_t *N, const size_t *row_stride,
                     float *const *y, const int64_t *y_col_stride, int64_t K, uint8_t *ws, size_t ws_size, int64_t M,
                     hipStream_t stream, const float *res, int64_t res_col_stride) {
    if (n_mat < 1 || n_mat > 4 || (res && n_mat > 1)) return MI355X_E_INVAL;
    const int64_t nb = K / QK;
    const int nw = mmf_nw(K);
    int64_t n_total = 0, tiles = 0;
    for (int d = 0; d < n_mat; ++d) {
        n_total += N[d];
        tiles += (N[d] + 32 * nw - 1) / (32 * nw);
    }
    MmfPlan p = mmf_plan_nw(tiles * 32 * nw, M, nb, nw);  // the split by the grid's row tiles
    uint8_t *img = ws, *bs = ws + al256((size_t)M * nb * MMF_IMG);
    uint8_t *slab_at = bs + al256((size_t)M * nb * MMF_BSB);
    if (p.n_split > 1 && (size_t)(slab_at - ws) + (size_t)p.n_split * M * n_total * 4 > ws_size) {
        p.n_split = 1;  // the slabs do not fit this workspace: no K split
        p.nbs = (int)nb;
    }
    MmfArgs a;
    memset(&a, 0, sizeof(a));
    a.w = (const uint8_t *)w[0];
    a.row_stride = (int64_t)row_stride[0];
    a.n_rows = (int)n_total;
    a.img = img;
    a.bs = bs;
    a.m_cols = (int)M;
    a.y = y[0];
    a.y_col_stride = y_col_stride[0];
    a.slab = (float *)slab_at;
    a.nb = (int)nb;
    a.nbs = p.nbs;
    a.n_split = p.n_split;
    a.n_ct = p.n_ct;
    a.n_rt = (int)tiles;
    a.res = res;
    a.res_col_stride = res_col_stride;
    a.n_mat = n_mat;
    int64_t t0 = 0, r0 = 0;
    for (int d = 0; d < n_mat; ++d) {
        a.tile0[d] = (int)t0;
        a.roff[d] = (int)r0;
        a.mw[d] = (const uint8_t *)w[d];
        a.mrow_stride[d] = (int64_t)row_stride[d];
        a.mn_rows[d] = (int)N[d];
        a.my[d] = y[d];
        a.my_col_stride[d] = y_col_stride[d];
        t0 += (N[d] + 32 * nw - 1) / (32 * nw);
        r0 += N[d];
    }
    a.tile0[n_mat] = (int)t0;
    if (n_mat == 1) a.n_rows = (int)N[0];
    a.order = (int)knob(KNOB_MMF_ORDER);  // A/B only
    const void *fn = nw == 8 ? (type == Q5_K ? (const void *)kq_mmf<Q5_K, 8> : type == Q6_K ? (const void *)kq_mmf<Q6_K, 8>
                                                                                        : (const void *)kq_mmf<Q4_K, 8>)
                             : (type == Q5_K ? (const void *)kq_mmf<Q5_K, 4> : type == Q6_K ? (const void *)kq_mmf<Q6_K, 4>
                                                                                        : (const void *)kq_mmf<Q4_K, 4>);
    const size_t lds = 2 * (size_t)MMF_BUF;
    allow_lds(fn, lds);
    const dim3 grid((unsigned)((int64_t)p.n_ct * tiles * p.n_split)), block(64 * nw);
    void *args[] = {&a};
    int rc = timed_launch_args(
        [&] {
            return LaunchInfo{std::string("kq::kq_mmf<") + std::to_string(type) + ", " + std::to_string(nw) + ">",
                              (double)n_total * nb * block_bytes(type) + (double)M * nb * (MMF_IMG + MMF_BSB) +
                                  (double)M * n_total * 4.0};
        },
        fn, grid, block, lds, stream, args);
    if (rc) return rc;
    if (p.n_split > 1) {
        for (int d = 0; d < n_mat; ++d) {
            const int64_t total = M * N[d];
            const dim3 rg((unsigned)((total + 255) / 256));
            const float *sl = (const float *)slab_at + a.roff[d];
            const float *rs = n_mat == 1 ? res : nullptr;
            rc = timed_launch("kq::kq_mmf_reduce", (double)total * 4.0 * (p.n_split + 1), kq_mmf_reduce, rg, dim3(256), 0,
                              stream, sl, p.n_split, (int)M, (int)N[d], (int)n_total, y[d], y_col_stride[d], rs,
                              res_col_stride);
            if (rc) return rc;
        }
    }
    return MI355X_OK;
}

int launch_mmf_gemm(int type, const void *w, int64_t K, int64_t N, size_t row_stride, uint8_t *ws, int64_t M,
                    float *y, int64_t y_col_stride, hipStream_t stream, const float *res, int64_t res_col_stride) {
    return launch_mmf_multi(type, 1, &w, &N, &row_stride, &y, &y_col_stride, K, ws, mmf_workspace(N, M, K / QK), M,
                            stream, res, res_col_stride);
}

// Up to 4 matrices on one Q8L activation in ONE launch (a prompt batch's q/k/v: the small k/v
// GEMMs do not run as half-empty launches of their own), on the tile mmq_shape picks for their
// rows together. Matrices of different K-quant types run on kq_mmq_mixed (each row tile its
// matrix's body). res: the ADD epilogue of a single matrix; kv: the KV-cache epilogue.
namespace {
int launch_mmq_tiles(const int *types, int n_mat, const void *const *w, const int64_t *N, const size_t *row_stride,
                     float *const *y, const int64_t *y_col_stride, int64_t K, const uint8_t *xq, int64_t M,
                     hipStream_t stream, const MmqKv *kv, const float *res, int64_t res_col_stride) {
    if (n_mat < 1 || n_mat > 4 || (res && n_mat > 1)) return MI355X_E_INVAL;
    const int type = types[0];
    bool mixed = false;
    for (int d = 1; d < n_mat; ++d) mixed |= types[d] != type;
    if (mixed)
        for (int d = 0; d < n_mat; ++d)
            if (types[d] != Q4_K && types[d] != Q5_K && types[d] != Q6_K) return MI355X_E_INVAL;
    int64_t all_rows = 0;
    for (int d = 0; d < n_mat; ++d) all_rows += N[d];
    MmqShape sh = mmq_shape(types[0], all_rows, M);  // (several types: on the first one's choice)
    bool has_q5 = false;
    for (int d = 0; d < n_mat; ++d) has_q5 |= types[d] == Q5_K;
    if (mixed && has_q5 && sh.rt == 128 && sh.cw == 2) sh = {128, 1};  // kq_mmq_mixed<128, 2> has no Q5_K body
    if (sh.rt == 192 && (mixed || type == Q6_K)) sh = {128, 1};  // the 12-wave 192-row tile: Q4_K / Q5_K only
    const int rt = sh.rt;
    MmqArgs a;
    memset(&a, 0, sizeof(a));
    a.n_mat = n_mat;
    a.res = res;
    a.res_col_stride = res_col_stride;
    a.xq = xq;
    a.nb = (int)(K / QK);
    a.xq_col_stride = (int64_t)a.nb * Q8L_STRIDE;
    a.m_cols = (int)M;
    int tiles = 0;
    double wbytes = 0, ybytes = 0;
    for (int d = 0; d < n_mat; ++d) {
        a.tile0[d] = tiles;
        a.mw[d] = (const uint8_t *)w[d];
        a.mrow_stride[d] = (int64_t)row_stride[d];
        a.mn_rows[d] = (int)N[d];
        a.my[d] = y[d];
        a.my_col_stride[d] = y_col_stride[d];
        a.mtype[d] = types[d];
        tiles += (int)((N[d] + rt - 1) / rt);
        wbytes += (double)N[d] * a.nb * block_bytes(types[d]);
        ybytes += (double)M * N[d] * 4.0;
    }
    a.tile0[n_mat] = tiles;
    if (kv) {
        for (int d = 0; d < n_mat; ++d) a.kv_kind[d] = kv->kind[d];
        a.kv_pos = kv->pos;
        a.kv_rope = kv->rope;
        a.kv_k_cache = kv->k_cache;
        a.kv_v_cache = kv->v_cache;
        a.kv_n_ctx = kv->n_ctx;
        a.kv_hd = kv->hd;
    }
    a.w = a.mw[0];
    a.row_stride = a.mrow_stride[0];
    a.n_rows = a.mn_rows[0];
    a.y = a.my[0];
    a.y_col_stride = a.my_col_stride[0];
    const void *fn = mmq_fn(type, mixed, sh);
    size_t lds = mmq_lds(mixed ? Q6_K : type, sh);  // mixed: the largest tile of its bodies
    if (mixed) lds = std::max(lds, std::max(mmq_lds(Q4_K, sh), mmq_lds(Q5_K, sh)));
    const dim3 grid((unsigned)((M + mmq_cols(sh.cw) - 1) / mmq_cols(sh.cw)), (unsigned)tiles, 1);
    allow_lds(fn, lds);
    void *args[] = {&a};
    return timed_launch_args(
        [&] {
            return LaunchInfo{mixed ? std::string("kq::kq_mmq_mixed") : std::string("kq::kq_mmq<") + std::to_string(type) + ">",
                              wbytes + (double)M * a.nb * Q8L_STRIDE + ybytes};
        },
        fn, grid, dim3((unsigned)(64 * mmq_waves(rt, sh.cw))), lds, stream, args);
}
}  // namespace

int launch_mmq(int type, const void *w, int64_t K, int64_t N, size_t row_stride, const uint8_t *xq, int64_t M,
               float *y, int64_t y_col_stride, hipStream_t stream, const float *res, int64_t res_col_stride) {
    return launch_mmq_tiles(&type, 1, &w, &N, &row_stride, &y, &y_col_stride, K, xq, M, stream, nullptr, res,
                            res_col_stride);
}

int launch_mmq_multi(const int *types, int n_mat, const void *const *w, const int64_t *N, const size_t *row_stride,
                     float *const *y, const int64_t *y_col_stride, int64_t K, const uint8_t *xq, int64_t M,
                     hipStream_t stream, const MmqKv *kv) {
    return launch_mmq_tiles(types, n_mat, w, N, row_stride, y, y_col_stride, K, xq, M, stream, kv, nullptr, 0);
}

bool mmq_applies(int type, const void *w, int64_t N, size_t row_stride, int64_t M) {
    if (!rows_enabled() || M < kMmqMinCols || N <= 0) return false;
    if (type != Q4_K && type != Q5_K && type != Q6_K) return false;
    if (N >= (1ll << 31) || M >= (1ll << 31)) return false;
    if (type == Q6_K) return true;  // any alignment: fetched from the 16-B boundary below each block
    return ((uintptr_t)w & 15u) == 0 && (row_stride & 15u) == 0;
}

}  // namespace kq
