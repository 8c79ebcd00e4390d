// kq_gemv_host.hip — host path of the decode GEMVs: the descriptor checks, the planners of
// kq_gemv (plan_gemv) and of kq_rows / kq_rows_dyn (plan_rows, a sequence of named steps pinned
// by tests/golden/rows_plans.json), their launches, and gemv_m1, which picks between them.
#include <string.h>

#include <atomic>
#include <string>

#include "kq_common.h"
#include "kq_internal.h"

namespace kq {

template <int NCOL, bool FUSEDQ, bool DEBUG, int TMASK>
__global__ void kq_gemv(const GemvArgs a);
__global__ void kq_quantize_q8K(const float *x, int64_t x_stride, uint8_t *y, int nb, int64_t nblocks);
template <int TMASK, bool FUSEDQ, int PRO, int LSH, bool SH>
__global__ void kq_rows(KQ_ROWS_PARAMS);
template <int TMASK, bool FUSEDQ, int PRO, int LSH>
__global__ void kq_rows_dyn(KQ_ROWS_PARAMS);
template <bool AM>
__global__ void kq_quantize_q8L(const float *x, int64_t x_stride, uint8_t *y, int nb, int64_t nblocks);

namespace {

std::atomic<int> g_impl{MI355X_GEMV_AUTO};  // mi355x_gemv_impl()
std::atomic<int> g_rows_waves{0};           // mi355x_gemv_waves: 0 = by size, else fixed

int type_bit(int type) { return type == Q4_K ? 1 : type == Q5_K ? 2 : type == Q6_K ? 4 : 0; }

// What both planners check alike, in the order the error codes are promised: n_desc, K, the
// planner's limit on nb (nb_err where it is passed), then per descriptor the type, the row count,
// non-null w / y and w's 4-byte alignment for a matrix with rows, and the planner's own
// conditions on that descriptor: own(d[i], nb, block bytes) -> error code. Returns the OR of the
// types' bits in tmask and the summed bytes of one superblock column (rows x block bytes).
template <typename Own>
int check_descs(const mi355x_gemv_desc *d, int n_desc, int64_t K, int64_t nb_max, int nb_err, Own own, int &tmask,
                double &bytes_total) {
    if (n_desc < 1 || n_desc > MI355X_MAX_FUSED) return MI355X_E_INVAL;
    if (K <= 0 || K % QK != 0) return MI355X_E_INVAL;
    const int64_t nb = K / QK;
    if (nb > nb_max) return nb_err;
    tmask = 0;
    bytes_total = 0;
    for (int i = 0; i < n_desc; ++i) {
        const int bb = block_bytes(d[i].type);
        if (!bb) return MI355X_E_UNSUPPORTED;
        if (d[i].n_rows < 0 || d[i].n_rows > 0x7fffffff) return MI355X_E_INVAL;
        if (d[i].n_rows > 0) {
            if (!d[i].w || !d[i].y) return MI355X_E_INVAL;
            if (((uintptr_t)d[i].w & 3u) != 0) return MI355X_E_INVAL;
            const int rc = own(d[i], nb, bb);
            if (rc) return rc;
        }
        bytes_total += (double)d[i].n_rows * bb;
        tmask |= type_bit(d[i].type);
    }
    return MI355X_OK;
}

template <int NCOL, bool FUSEDQ, bool DEBUG>
gemv_fn pick_tm(int tmask) {
    switch (tmask) {
        case 1: return kq_gemv<NCOL, FUSEDQ, DEBUG, 1>;
        case 4: return kq_gemv<NCOL, FUSEDQ, DEBUG, 4>;
        default: return kq_gemv<NCOL, FUSEDQ, DEBUG, 7>;
    }
}

gemv_fn pick_gemv(int ncol, bool fusedq, bool debug, int tmask) {
    if (debug) return pick_tm<1, false, true>(tmask);
    if (fusedq) return pick_tm<1, true, false>(tmask);
    switch (ncol) {
        case 1: return pick_tm<1, false, false>(tmask);
        case 2: return pick_tm<2, false, false>(tmask);
        case 4: return pick_tm<4, false, false>(tmask);
        default: return pick_tm<8, false, false>(tmask);
    }
}

// Same spelling as rocprofv3's kernel names (kernel-trace "Kernel_Name").
std::string gemv_name(const GemvPlan &pl) {
    return std::string("kq::kq_gemv<") + std::to_string(pl.ncol) + ", " + (pl.fusedq ? "true" : "false") + ", " +
           (pl.debug ? "true" : "false") + ", " + std::to_string(pl.tmask) + ">";
}

// Algorithmic bytes of one launch: weights + activations read + f32 outputs.
double gemv_bytes(const GemvArgs &a, bool fusedq) {
    double w = 0, y = 0;
    for (int i = 0; i < a.n_desc; ++i) {
        w += (double)a.n_rows[i] * a.nb * block_bytes(a.type[i]);
        y += (double)a.n_rows[i] * 4.0 * a.m_total;
    }
    const double x = fusedq ? (double)a.nb * QK * 4.0 * a.m_total : (double)a.nb * 292.0 * a.m_total;
    return w + x + y;
}

}  // namespace

int choose_ncol(int64_t M, int nb) {
    if (M <= 1) return 1;
    const int cands[4] = {8, 4, 2, 1};
    for (int i = 0; i < 4; ++i) {
        const int nc = cands[i];
        if (nc > M && nc > 1) continue;
        if ((size_t)lds_layout(nc, nb, 8 * nc, false, 8 * 16 * 14, 4).total <= kTargetLds) return nc;
    }
    return 1;
}

// Validates descriptors and fills the launch plan. Returns MI355X_OK or an error.
int plan_gemv(const mi355x_gemv_desc *d, int n_desc, int64_t K, int64_t M, int ncol, bool fusedq, bool debug,
              GemvPlan &pl) {
    GemvArgs &a = pl.a;
    if (M < 0) return MI355X_E_INVAL;
    int tmask = 0;
    double bytes_total = 0;
    const int rc = check_descs(
        d, n_desc, K, 0x7fffffff / 8, MI355X_E_INVAL,
        [](const mi355x_gemv_desc &m, int64_t nb, int bb) {
            if (m.row_stride < (size_t)(nb * bb) || (m.row_stride & 1u)) return MI355X_E_INVAL;
            if (m.type != Q6_K && (m.row_stride & 3u)) return MI355X_E_INVAL;
            return MI355X_OK;
        },
        tmask, bytes_total);
    if (rc) return rc;
    const int64_t nb = K / QK;
    memset(&a, 0, sizeof(a));
    if (tmask != 1 && tmask != 4) tmask = 7;
    a.n_desc = n_desc;
    a.nb = (int)nb;
    a.R = BLOCKS_PER_STEP;
    a.m_total = (int)M;
    int64_t tasks = 0;
    for (int i = 0; i < n_desc; ++i) {
        a.type[i] = d[i].type;
        a.n_rows[i] = (int)d[i].n_rows;
        a.w[i] = (const uint8_t *)d[i].w;
        a.row_stride[i] = (int64_t)d[i].row_stride;
        a.y[i] = d[i].y;
        a.task_prefix[i] = (int)tasks;
        tasks += (d[i].n_rows + a.R - 1) / a.R;
    }
    if (tasks > 0x7fffffff) return MI355X_E_INVAL;
    for (int i = n_desc; i <= MI355X_MAX_FUSED; ++i) a.task_prefix[i] = (int)tasks;
    a.tasks_total = (int)tasks;
    pl.ncol = ncol;
    pl.fusedq = fusedq;
    pl.debug = debug;
    pl.tmask = tmask;
    pl.fn = pick_gemv(ncol, fusedq, debug, tmask);
    a.diag = (int)knob(KNOB_GEMV_DIAG);
    a.ring_override = (int)knob(KNOB_GEMV_RING);
    a.stamps = diag_stamps(&a.stamps_cap);
    // One workgroup per 8-row task, at most one round of resident workgroups; each
    // workgroup strides over tasks. Ring depth: as deep as LDS allows 2+ resident
    // workgroups per CU. Staged outputs bound the tasks per workgroup.
    const int slot = tmask == 1 ? 8 * 16 * 9 : 8 * 16 * 14;
    const int dcands[3] = {tmask == 1 ? 8 : 6, tmask == 1 ? 6 : 5, 4};
    int D = 4;
    for (int i = 0; i < 3; ++i) {
        D = dcands[i];
        if ((size_t)lds_layout(ncol, (int)nb, 8 * ncol, fusedq, slot, D).total <= kTargetLds) break;
    }
    if (a.ring_override > 0) D = a.ring_override < 13 ? a.ring_override : 13;
    a.ring = D;
    const int64_t base_lds = lds_layout(ncol, (int)nb, 0, fusedq, slot, D).total;
    if ((size_t)base_lds > kMaxLds) return MI355X_E_UNSUPPORTED;
    int64_t wgs = (int64_t)num_cus() * resident_wgs((const void *)pl.fn, (size_t)base_lds + 1024);
    if (wgs > tasks) wgs = tasks > 0 ? tasks : 1;
    int64_t tpw = (tasks + wgs - 1) / wgs;
    while (tpw * 8 * ncol * 4 > 4096 && tpw > 1) {
        wgs *= 2;
        tpw = (tasks + wgs - 1) / wgs;
    }
    a.out_per_wg = (int)(tpw * 8 * ncol);
    const LdsLayout L = lds_layout(ncol, (int)nb, a.out_per_wg, fusedq, slot, D);
    if ((size_t)L.total > kMaxLds) return MI355X_E_UNSUPPORTED;
    pl.lds = (size_t)L.total;
    pl.grid = dim3((unsigned)wgs, (unsigned)((M + ncol - 1) / ncol), 1);
    return MI355X_OK;
}

int launch_gemv(const GemvPlan &pl, hipStream_t stream) {
    const GemvArgs &a = pl.a;
    if (a.tasks_total == 0 || a.m_total == 0) return MI355X_OK;
    allow_lds((const void *)pl.fn, pl.lds);
    return timed_launch_lazy([&] { return LaunchInfo{gemv_name(pl), gemv_bytes(a, pl.fusedq)}; }, pl.fn, pl.grid,
                             dim3(WG_THREADS), pl.lds, stream, a);
}

// ------------------------------------------------------------ row-stream decode GEMV
bool rows_enabled() { return g_impl.load() != MI355X_GEMV_TASKS; }
int gemv_impl_select(int impl) { return impl < 0 ? g_impl.load() : g_impl.exchange(impl); }
int rows_waves_select(int waves) { return waves < 0 ? g_rows_waves.load() : g_rows_waves.exchange(waves); }

int rows_pro_kind(int prologue) {
    return prologue == MI355X_PRO_RMS_NORM ? ROWS_PRO_NORM : prologue == MI355X_PRO_SWIGLU ? ROWS_PRO_SWIGLU : ROWS_PRO_NONE;
}

namespace {

// (sh: the short-stream form, of the statically split fused-quantization kernels only)
template <int TM, bool FQ, int PR, int LS>
rows_fn rows_inst(bool dyn, bool sh) {
    if constexpr (TM == 7) {
        if constexpr (FQ) return sh ? kq_rows<TM, FQ, PR, LS, true> : kq_rows<TM, FQ, PR, LS, false>;
        else return kq_rows<TM, FQ, PR, LS, false>;
    } else {
        if (dyn) return kq_rows_dyn<TM, FQ, PR, LS>;
        if constexpr (FQ) return sh ? kq_rows<TM, FQ, PR, LS, true> : kq_rows<TM, FQ, PR, LS, false>;
        else return kq_rows<TM, FQ, PR, LS, false>;
    }
}

template <int TM, int PR>
rows_fn rows_pick_form(int lsh, bool dyn, bool sh) {
    return lsh == 2   ? rows_inst<TM, true, PR, 2>(dyn, sh)
           : lsh == 1 ? rows_inst<TM, true, PR, 1>(dyn, sh)
                      : rows_inst<TM, true, PR, 0>(dyn, sh);
}

template <int TM>
rows_fn rows_pick_pro(bool fusedq, int pro, bool dyn, int lsh, bool sh) {
    if (!fusedq) return rows_inst<TM, false, 0, 0>(dyn, false);
    return pro == ROWS_PRO_NORM     ? rows_pick_form<TM, 1>(lsh, dyn, sh)
           : pro == ROWS_PRO_SWIGLU ? rows_pick_form<TM, 2>(lsh, dyn, sh)
                                    : rows_pick_form<TM, 0>(lsh, dyn, sh);
}

// lsh: the fused prologue's form (RowsPlan::lsh), sh: the short-stream form (RowsPlan::sh),
// template parameters of the kernels
rows_fn pick_rows(int tmask, bool fusedq, int pro, bool dyn, int lsh, bool sh) {
    switch (tmask) {
        case 1: return rows_pick_pro<1>(fusedq, pro, dyn, lsh, sh);
        case 2: return rows_pick_pro<2>(fusedq, pro, dyn, lsh, sh);
        case 4: return rows_pick_pro<4>(fusedq, pro, dyn, lsh, sh);
        default: return rows_pick_pro<7>(fusedq, pro, false, lsh, sh);
    }
}

// ---- plan_rows' steps, in the order it runs them

// The descriptors, and the knobs and diagnostics that travel in RowsArgs.
void rows_fill_args(const mi355x_gemv_desc *d, int n_desc, int64_t nb, RowsArgs &a) {
    memset(&a, 0, sizeof(a));
    a.n_desc = n_desc;
    a.nb = (int)nb;
    for (int i = 0; i < n_desc; ++i) {
        a.type[i] = d[i].type;
        a.w[i] = (const uint8_t *)d[i].w;
        a.y[i] = d[i].y;
        a.n_rows[i] = (int)d[i].n_rows;
    }
    a.diag = (int)knob(KNOB_GEMV_DIAG);
    // A recorded plan field that no kernel reads (RowsArgs): the kernels issue one weight step
    // before the activation is quantized. A deeper early burst delays the activation loads
    // queued behind it: alone, K = 2048 GEMVs ran 5-9 % faster with the whole ring, but with
    // the fused norm prologue (two vectors to fetch) the decode token was 1.6 % slower
    // (profiles/r01_wave_priority_and_pre0.txt).
    const int pre = (int)knob(KNOB_GEMV_PRE0);
    a.pre0 = pre < 0 ? 0 : pre > 3 ? 3 : pre;
    a.stamps = diag_stamps(&a.stamps_cap);
}

// Waves: one workgroup per CU of ROWS_WAVES waves, or of ROWS_WAVES_SMALL for a launch
// under kRowsSmallBytes of weights (measured on the graph-replayed token: fewer waves
// to dispatch, the short stream does not need them; profiles/r02_rows_waves.md).
// waves_per_cu > 0: the caller's count.
int rows_waves_per_cu(bool fusedq, int64_t nb, bool small, int waves_per_cu) {
    if (waves_per_cu > 0) return waves_per_cu;
    const int fixed = g_rows_waves.load();
    const int want = fixed > 0 ? fixed : small ? ROWS_WAVES_SMALL : ROWS_WAVES;
    // the fused quantization covers ROWS_QPASS passes of 4 superblocks per wave
    return !fusedq || nb <= ROWS_QPASS * 4 * want ? want : ROWS_WAVES;
}

// The most waves of the launch: one workgroup per CU (an A/B knob caps the workgroups of small
// launches, GEMV_SMALL_WG) of nwv waves (an experiment knob caps the active ones, GEMV_WPC).
int64_t rows_wave_cap(int nwv, bool small, int64_t &n_wg) {
    const int wpc_env = (int)knob(KNOB_GEMV_WPC);
    const int active = wpc_env > 0 && wpc_env < nwv ? wpc_env : nwv;
    const int small_wg_env = (int)knob(KNOB_GEMV_SMALL_WG);
    n_wg = num_cus();
    if (small_wg_env > 0 && small && small_wg_env < n_wg) n_wg = small_wg_env;
    return n_wg * active;
}

// Each matrix gets waves in proportion to its bytes (never more waves than rows): wv[].
void rows_split_waves(const mi355x_gemv_desc *d, int n_desc, int64_t nb, double bytes_total, int64_t cap,
                      int64_t wv[MI355X_MAX_FUSED]) {
    int64_t waves = 0;
    for (int i = 0; i < MI355X_MAX_FUSED; ++i) wv[i] = 0;
    for (int i = 0; i < n_desc; ++i) {
        if (d[i].n_rows == 0) continue;
        const double share = (double)d[i].n_rows * block_bytes(d[i].type) / bytes_total;
        int64_t w = (int64_t)(share * (double)cap);
        // at least one full 16-superblock step per wave (short rows: several rows per wave)
        const int64_t min_rows = (ROWS_SB + nb - 1) / nb;
        const int64_t wmax = (d[i].n_rows + min_rows - 1) / min_rows;
        if (w > wmax) w = wmax;
        if (w < 1) w = 1;
        wv[i] = w;
        waves += w;
    }
    while (waves > cap) {  // the max(1, .) floors may overshoot by < n_desc: trim the largest
        int big = 0;
        for (int i = 1; i < n_desc; ++i)
            if (wv[i] > wv[big]) big = i;
        --wv[big];
        --waves;
    }
}

// Rows split evenly over a matrix's waves (wave_prefix / rbase / rrem). longest[i]: the rows of
// matrix i's longest wave, 0 for a matrix without waves; rpw, prio_bytes, the stream's steps and
// the prologue's form all derive from it. Returns the most rows of any wave.
int64_t rows_split_rows(const mi355x_gemv_desc *d, int n_desc, int64_t nb, const int64_t wv[MI355X_MAX_FUSED],
                        RowsArgs &a, int64_t longest[MI355X_MAX_FUSED]) {
    int64_t waves = 0, rpw = 0;
    a.prio_bytes = 0;
    for (int i = 0; i < n_desc; ++i) {
        a.wave_prefix[i] = (int)waves;
        longest[i] = 0;
        if (wv[i] > 0) {
            a.rbase[i] = (int)(d[i].n_rows / wv[i]);
            a.rrem[i] = (int)(d[i].n_rows % wv[i]);
            longest[i] = a.rbase[i] + (a.rrem[i] ? 1 : 0);
            const int64_t b = longest[i] * nb * block_bytes(d[i].type);
            rpw = longest[i] > rpw ? longest[i] : rpw;
            a.prio_bytes = b > a.prio_bytes ? b : a.prio_bytes;
        }
        waves += wv[i];
    }
    for (int i = n_desc; i <= MI355X_MAX_FUSED; ++i) a.wave_prefix[i] = (int)waves;
    a.waves_total = (int)waves;
    return rpw;
}

// rows per chain batch: ~ROWS_RECS records, batch ends on a step boundary (bR*nb % 16 == 0)
int rows_chain_batch(int64_t nb, int rpw) {
    int g16 = ROWS_SB;
    while (nb % g16) g16 >>= 1;
    const int u = ROWS_SB / g16;
    int bR_full = (int)(ROWS_RECS / nb) / u * u;
    if (bR_full < u) bR_full = u;
    return rpw <= bR_full ? rpw : bR_full;
}

// the short-stream form: every matrix's longest stream fits the ring of its type, and one
// chain batch covers a wave's rows (GEMV_SHORT 0: the generic form, A/B runs). The plan
// keeps the steps and depth of the matrix with the least room (depth - steps).
void rows_stream_form(const mi355x_gemv_desc *d, int n_desc, int64_t nb, const int64_t longest[MI355X_MAX_FUSED],
                      RowsPlan &pl) {
    pl.steps = 0, pl.depth = 0;
    for (int i = 0; i < n_desc; ++i) {
        if (longest[i] == 0) continue;
        const int st = (int)((longest[i] * nb + ROWS_SB - 1) / ROWS_SB);
        const int dp = rows_depth(d[i].type);
        if (!pl.depth || dp - st < pl.depth - pl.steps || (dp - st == pl.depth - pl.steps && st > pl.steps))
            pl.steps = st, pl.depth = dp;
    }
    pl.sh = pl.fusedq && knob(KNOB_GEMV_SHORT) != 0 && rows_short_form(pl.steps, pl.depth, pl.a.bR, pl.a.rpw);
}

// Claimed rows (kq_rows_dyn) for one-type launches whose waves get enough units to balance
// (GEMV_DYN units per wave on average; MI355X_GEMV_DYN: every one-type launch). A unit is
// U whole rows of at least one 16-superblock step; each wave's first P units (a ring's
// worth) are static. Rewrites the static split's rows, batch, LDS and grid where it applies.
void rows_try_claimed(const mi355x_gemv_desc *d, int n_desc, int64_t nb, int64_t n_wg, RowsPlan &pl) {
    RowsArgs &a = pl.a;
    const int tmask = pl.tmask;
    pl.dyn = false;
    const double dyn_min = knob(KNOB_GEMV_DYN);
    const bool force = g_impl.load() == MI355X_GEMV_DYN;
    bool same_rows = true;  // kq_rows_dyn: one workgroup row range for every matrix
    for (int i = 1; i < n_desc; ++i) same_rows = same_rows && d[i].n_rows == d[0].n_rows;
    if (tmask == 7 || !same_rows || !(force || dyn_min > 0)) return;
    // U: whole rows, a power of two, at least one 16-superblock step; two steps where every
    // wave streams many (a claim and a unit's bookkeeping per two steps)
    int ush = 0;
    while ((int64_t)(1 << ush) * nb < ROWS_SB) ++ush;
    const double steps_per_wave = (double)n_desc * d[0].n_rows * nb / ROWS_SB / n_wg / pl.nwv;
    if ((int64_t)(1 << ush) * nb == ROWS_SB && steps_per_wave >= 16) ++ush;
    const int U = 1 << ush;
    const int Tu = (int)((U * nb + ROWS_SB - 1) / ROWS_SB);
    const int D = rows_depth(tmask == 1 ? Q4_K : tmask == 2 ? Q5_K : Q6_K);
    // flat output slots per workgroup: its row units (strided placement) or rows, per matrix
    const int64_t flat = (int64_t)n_desc * ((d[0].n_rows + n_wg - 1) / n_wg);
    const int64_t rows = (int64_t)n_desc * d[0].n_rows;
    // replay batch: ~ROWS_RECS records, whole units
    int bRd = (int)(ROWS_RECS / nb) / U * U;
    if (bRd < U) bRd = U;
    // AUTO (profiles/r06_dyn_ab.txt): claimed rows paid where every wave streams many steps
    // in many units (the Q6_K heads, 70B gate + up: -1 to -3 %); with few units per wave
    // (8B ffn_up, 70B ffn_down: +5 to +10 %) the units' bookkeeping costs more than the
    // balance gains
    const double per_wave = (double)rows / (double)n_wg / U / pl.nwv;
    const bool auto_ok = per_wave >= dyn_min && steps_per_wave >= knob(KNOB_GEMV_DYN_STEPS);
    const RowsDynLayout DL = rows_dyn_layout((int)nb, tmask, bRd, (int)flat, pl.nwv);
    if (!(force || auto_ok) || rows <= 0 || (size_t)DL.total > kMaxLds || flat >= 0x7fffffff / 64) return;
    pl.dyn = true;
    a.dyn_u = U;
    a.dyn_ush = ush;
    a.rbase[0] = (int)(d[0].n_rows / n_wg);
    a.rrem[0] = (int)(d[0].n_rows % n_wg);
    a.dyn_p = (D + Tu - 1) / Tu;
    const int p_knob = (int)knob(KNOB_GEMV_DYN_P);
    if (p_knob > 0) a.dyn_p = p_knob;
    a.bR = bRd;
    a.rpw = (int)flat;
    pl.lds = (size_t)DL.total;
    pl.grid = dim3((unsigned)n_wg, 1, 1);
    pl.sh = false;
}

std::string rows_name(const RowsPlan &pl) {
    return std::string(pl.dyn ? "kq::kq_rows_dyn<" : "kq::kq_rows<") + std::to_string(pl.tmask) + ", " + (pl.fusedq ? "true" : "false") + ", " +
           std::to_string(pl.a.pro) + ">";
}

double rows_bytes(const RowsArgs &a, bool fusedq) {
    double w = 0, y = 0;
    for (int i = 0; i < a.n_desc; ++i) {
        const double rows = (double)a.n_rows[i];
        w += rows * a.nb * block_bytes(a.type[i]);
        y += rows * 4.0;
    }
    return w + y + (fusedq ? (double)a.nb * QK * 4.0 : (double)a.nb * Q8L_STRIDE);
}

}  // namespace

// The instantiation `fn` as an integer (mi355x_debug_rows_plan's `kernel` field): the first
// (kernel, TMASK, FUSEDQ, PRO, LSH, SH) in ascending order that pick_rows() maps to it, so a
// parameter the instantiation does not have reads 0. -1: not a kernel of pick_rows().
int rows_kernel_id(rows_fn fn) {
    const int tmasks[4] = {1, 2, 4, 7};
    for (int dyn = 0; dyn < 2; ++dyn)
        for (int tm : tmasks)
            for (int fq = 0; fq < 2; ++fq)
                for (int pro = 0; pro < 3; ++pro)
                    for (int lsh = 0; lsh < 3; ++lsh)
                        for (int sh = 0; sh < 2; ++sh)
                            if (pick_rows(tm, fq != 0, pro, dyn != 0, lsh, sh != 0) == fn)
                                return ((((dyn * 8 + tm) * 2 + fq) * 4 + pro) * 4 + lsh) * 2 + sh;
    return -1;
}

int plan_rows(const mi355x_gemv_desc *d, int n_desc, int64_t K, bool fusedq, int pro, RowsPlan &pl, int waves_per_cu) {
    RowsArgs &a = pl.a;
    if (pro < ROWS_PRO_NONE || pro > ROWS_PRO_SWIGLU || (!fusedq && pro != ROWS_PRO_NONE)) return MI355X_E_INVAL;
    double bytes_total = 0;
    const int rc = check_descs(
        d, n_desc, K, fusedq && kRowsFusedMaxNb < 4096 ? kRowsFusedMaxNb : 4096, MI355X_E_UNSUPPORTED,
        [](const mi355x_gemv_desc &m, int64_t nb, int bb) {
            // one contiguous stream per wave; Q4_K/Q5_K superblocks 16-B aligned in LDS
            if (m.row_stride != (size_t)(nb * bb)) return MI355X_E_UNSUPPORTED;
            if (m.type != Q6_K && ((uintptr_t)m.w & 15u)) return MI355X_E_UNSUPPORTED;
            return MI355X_OK;
        },
        pl.tmask, bytes_total);
    if (rc) return rc;
    if (pl.tmask != 1 && pl.tmask != 2 && pl.tmask != 4) pl.tmask = 7;
    pl.fusedq = fusedq;
    const int64_t nb = K / QK;
    rows_fill_args(d, n_desc, nb, a);
    a.pro = pro;
    const bool small = bytes_total * nb < knob(KNOB_GEMV_SMALL_MB) * 1e6;  // (0: never)
    pl.nwv = rows_waves_per_cu(fusedq, nb, small, waves_per_cu);
    if (pl.nwv > ROWS_WAVES) return MI355X_E_INVAL;
    int64_t n_wg = 0, wv[MI355X_MAX_FUSED], longest[MI355X_MAX_FUSED];
    rows_split_waves(d, n_desc, nb, bytes_total, rows_wave_cap(pl.nwv, small, n_wg), wv);
    const int64_t rpw = rows_split_rows(d, n_desc, nb, wv, a, longest);
    if (rpw > 0x7fffffff / 64) return MI355X_E_UNSUPPORTED;
    a.rpw = (int)(rpw > 0 ? rpw : 1);
    // the prologue's form, by the row, the waves and the longest stream of the launch
    pl.lsh = fusedq ? rows_pro_form((int)nb, pl.nwv, (rpw * nb + ROWS_SB - 1) / ROWS_SB).lsh : 0;
    a.bR = rows_chain_batch(nb, a.rpw);
    rows_stream_form(d, n_desc, nb, longest, pl);
    const RowsLayout L = rows_layout((int)nb, pl.tmask, a.bR, a.rpw, pl.nwv);
    if ((size_t)L.total > kMaxLds) return MI355X_E_UNSUPPORTED;
    pl.lds = (size_t)L.total;
    const int64_t grid = a.waves_total < n_wg ? a.waves_total : n_wg;
    pl.grid = dim3((unsigned)(grid > 0 ? grid : 1), 1, 1);
    rows_try_claimed(d, n_desc, nb, n_wg, pl);
    pl.fn = pick_rows(pl.tmask, fusedq, pro, pl.dyn, pl.lsh, pl.sh);  // once: the kernel launch_rows launches
    return MI355X_OK;
}

int launch_rows(const RowsPlan &pl, hipStream_t stream) {
    const RowsArgs &a = pl.a;
    if (a.waves_total == 0) return MI355X_OK;
    allow_lds((const void *)pl.fn, pl.lds);
    // the leading parameters (KQ_ROWS_PARAMS): what a wave needs before its first memory
    // request; the kernels read neither gridDim nor blockDim, and the prologue's pass count
    // (passes of 4 superblocks per wave over the activation) is divided here
    const void *x = pl.fusedq ? (const void *)a.x : (const void *)a.xq;
    // (the prologue's form, rows_pro_form at plan time: its lanes per superblock are the kernel's LSH)
    const int qiters = !pl.fusedq ? 0 : pl.lsh ? 1 : (a.nb + 4 * pl.nwv - 1) / (4 * pl.nwv);
    if (pl.lsh < 0 || pl.lsh > 2 || (pl.lsh && (!pl.fusedq || a.nb * (16 << pl.lsh) > 64 * pl.nwv))) return MI355X_E_INVAL;
    // cfg's fields are a few bits each: a plan outside them would run another launch silently
    // (the short form's kernel issues nothing after its barrier and replays one batch)
    if (pl.sh && (!pl.fusedq || pl.dyn || !rows_short_form(pl.steps, pl.depth, a.bR, a.rpw))) return MI355X_E_INVAL;
    if (pl.nwv < 1 || pl.nwv > ROWS_WAVES || qiters > ROWS_QPASS || a.n_desc < 1 || a.n_desc > MI355X_MAX_FUSED)
        return MI355X_E_INVAL;
    const int cfg = rows_cfg(pl.nwv, qiters, a.n_desc, a.diag & 0x1ff);
    const int grid = (int)pl.grid.x;
    return timed_launch_lazy([&] { return LaunchInfo{rows_name(pl), rows_bytes(a, pl.fusedq)}; }, pl.fn, pl.grid,
                             dim3(pl.nwv * 64), pl.lds, stream, x, a.x2, a.w[0], a.res[0], a.nb, a.waves_total, grid,
                             cfg, a.rbase[0], a.rrem[0], a);
}

int launch_quantize_q8L(const float *x, int64_t x_stride_floats, void *y, int64_t k, int64_t nrows,
                        hipStream_t stream, bool mmq) {
    const auto kern = mmq ? kq_quantize_q8L<true> : kq_quantize_q8L<false>;
    const int64_t nb = k / QK;
    const int64_t nblocks = nb * nrows;
    if (nblocks == 0) return MI355X_OK;
    const int64_t wgs = (nblocks + 15) / 16;
    return timed_launch("kq::kq_quantize_q8L", (double)nblocks * (QK * 4.0 + Q8L_STRIDE), kern, dim3((unsigned)wgs),
                        dim3(WG_THREADS), 0, stream, x, x_stride_floats, (uint8_t *)y, (int)nb, nblocks);
}

int launch_quantize(const float *x, int64_t x_stride_floats, void *y, int64_t k, int64_t nrows,
                    hipStream_t stream) {
    const int64_t nb = k / QK;
    const int64_t nblocks = nb * nrows;
    if (nblocks == 0) return MI355X_OK;
    const int64_t wgs = (nblocks + WAVES_PER_WG - 1) / WAVES_PER_WG;
    return timed_launch("kq::kq_quantize_q8K", (double)nblocks * (QK * 4.0 + 292.0), kq_quantize_q8K,
                        dim3((unsigned)wgs), dim3(WG_THREADS), 0, stream, x, x_stride_floats, (uint8_t *)y, (int)nb,
                        nblocks);
}

size_t ext_x_bytes(int64_t k) { return ((size_t)k * 4 + 255) & ~(size_t)255; }

namespace {

int launch_rows_checked(const RowsPlan &rp, hipStream_t stream) {
    if (!device_ok()) return MI355X_E_NODEVICE;
    return launch_rows(rp, stream);
}

// gemv_m1 with a fused prologue / residual / SWIGLU epilogue on kq_rows' fused quantizer:
// the launch's code, or MI355X_E_UNSUPPORTED where the launch has to be staged instead.
int rows_ext_launch(const mi355x_gemv_desc *d, int n, const float *x, int64_t k, const mi355x_gemv_ext *ext,
                    hipStream_t stream) {
    RowsPlan rp;
    const int rc = plan_rows(d, n, k, true, rows_pro_kind(ext->prologue), rp);
    if (rc) return rc;
    rp.a.x = x;
    rp.a.x2 = ext->x2;
    rp.a.eps = ext->eps;
    for (int i = 0; i < n; ++i) rp.a.res[i] = ext->residual[i];
    if (ext->epilogue == MI355X_EPI_SWIGLU) {
        // SWIGLU epilogue in-kernel when gate wave j and up wave j land in the same
        // workgroup with the same rows: equal wave counts, up's first wave on a
        // workgroup boundary (gw = wave * grid + block)
        const int g = (int)rp.grid.x;
        // (kq_rows_dyn: a workgroup owns the same rows of both by construction)
        const bool paired = rp.dyn || (rp.a.wave_prefix[2] == 2 * rp.a.wave_prefix[1] && rp.a.wave_prefix[1] % g == 0 &&
                                       rp.a.rbase[0] == rp.a.rbase[1] && rp.a.rrem[0] == rp.a.rrem[1]);
        if (!paired) return MI355X_E_UNSUPPORTED;
        rp.a.epi = 1;
        rp.a.epi_n = (int)d[0].n_rows;
        rp.a.epi_wave_off = rp.a.wave_prefix[1] / g;
        rp.a.epi_y = ext->epi_y;
    }
    return launch_rows_checked(rp, stream);
}

// gemv_m1 with `ext` (a fused prologue, residuals or the SWIGLU epilogue): kq_rows applies them
// in-kernel when it takes the shape with the fused quantizer; otherwise staged: the prologue runs
// as its own kernel into the front of the workspace and the residual adds follow the GEMV (the
// same kernels as the separate nodes, so the bits do not depend on the path).
int gemv_m1_ext(const mi355x_gemv_desc *d, int n, const float *x, int64_t k, void *ws, size_t ws_size,
                hipStream_t stream, const mi355x_gemv_ext *ext) {
    if (ext->prologue != MI355X_PRO_NONE && !ext->x2) return MI355X_E_INVAL;
    const bool epi = ext->epilogue == MI355X_EPI_SWIGLU;
    if (ext->epilogue != MI355X_EPI_NONE && !epi) return MI355X_E_INVAL;
    if (epi && (n != 2 || !ext->epi_y || d[0].n_rows != d[1].n_rows || ext->residual[0] || ext->residual[1]))
        return MI355X_E_INVAL;
    const bool x2_ok = ext->prologue == MI355X_PRO_NONE || ((uintptr_t)ext->x2 & 15u) == 0;
    if (rows_enabled() && k / QK <= kRowsFusedMaxNb && ((uintptr_t)x & 15u) == 0 && x2_ok) {
        const int rc = rows_ext_launch(d, n, x, k, ext, stream);
        if (rc != MI355X_E_UNSUPPORTED) return rc;
    }
    const float *xs = x;
    uint8_t *w8 = (uint8_t *)ws;
    size_t wsz = ws_size;
    if (ext->prologue != MI355X_PRO_NONE) {
        if (!ws || ws_size < ext_x_bytes(k) || ((uintptr_t)ws & 15u)) return MI355X_E_WORKSPACE;
        if (!device_ok()) return MI355X_E_NODEVICE;
        float *xt = (float *)ws;
        const int rc = ext->prologue == MI355X_PRO_RMS_NORM ? launch_rms_norm(x, ext->x2, xt, k, 1, ext->eps, stream)
                                                            : launch_swiglu(x, ext->x2, xt, k, stream);
        if (rc) return rc;
        xs = xt;
        w8 += ext_x_bytes(k);
        wsz -= ext_x_bytes(k);
    }
    int rc = gemv_m1(d, n, xs, k, w8, wsz, stream, nullptr);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (ext->residual[i] && d[i].n_rows > 0) {
            rc = launch_binary(0, d[i].y, ext->residual[i], d[i].y, d[i].n_rows, stream);
            if (rc) return rc;
        }
    if (epi && d[0].n_rows > 0) return launch_swiglu(d[0].y, d[1].y, ext->epi_y, d[0].n_rows, stream);
    return MI355X_OK;
}

}  // namespace

// One activation column (decode): kq_rows when the rows are contiguous (always for
// GGUF tensors), kq_gemv otherwise. x is quantized inside the GEMV for K <= 8192
// (x 16-B aligned), else into `ws` first.
int gemv_m1(const mi355x_gemv_desc *d, int n, const float *x, int64_t k, void *ws, size_t ws_size,
            hipStream_t stream, const mi355x_gemv_ext *ext) {
    const bool has_ext = ext && (ext->prologue != MI355X_PRO_NONE || ext->epilogue != MI355X_EPI_NONE || [&] {
        for (int i = 0; i < n && i < MI355X_MAX_FUSED; ++i)
            if (ext->residual[i]) return true;
        return false;
    }());
    if (has_ext) return gemv_m1_ext(d, n, x, k, ws, ws_size, stream, ext);
    const bool fusedq = k / QK <= kFusedQMaxNb && ((uintptr_t)x & 15u) == 0;
    const size_t need = (size_t)(k / QK) * 292;
    if (rows_enabled()) {
        RowsPlan rp;
        // GEMV_FQMAX (A/B only): the most superblocks quantized inside kq_rows; above it one
        // kq_quantize_q8L launch first and the GEMV DMAs the Q8L row
        const int64_t fq_max = (int64_t)knob(KNOB_GEMV_FQMAX);
        const bool rows_fq = k / QK <= fq_max && k / QK <= kRowsFusedMaxNb && ((uintptr_t)x & 15u) == 0;
        int rc = plan_rows(d, n, k, rows_fq, ROWS_PRO_NONE, rp);
        if (rc == MI355X_OK) {
            if (rows_fq) {
                rp.a.x = x;
                return launch_rows_checked(rp, stream);
            }
            const size_t need_l = (size_t)(k / QK) * Q8L_STRIDE;
            if (!ws || ws_size < need_l || ((uintptr_t)ws & 15u)) return MI355X_E_WORKSPACE;
            if (!device_ok()) return MI355X_E_NODEVICE;
            rc = launch_quantize_q8L(x, k, ws, k, 1, stream);
            if (rc) return rc;
            rp.a.xq = (const uint8_t *)ws;
            return launch_rows(rp, stream);
        }
        if (rc != MI355X_E_UNSUPPORTED) return rc;
    }
    GemvPlan pl;
    int rc = plan_gemv(d, n, k, 1, 1, fusedq, false, pl);
    if (rc) return rc;
    if (fusedq) {
        pl.a.x = x;
        pl.a.x_col_stride = k;
        if (!device_ok()) return MI355X_E_NODEVICE;
        return launch_gemv(pl, stream);
    }
    if (!ws || ws_size < need || ((uintptr_t)ws & 3u)) return MI355X_E_WORKSPACE;
    if (!device_ok()) return MI355X_E_NODEVICE;
    rc = launch_quantize(x, k, ws, k, 1, stream);
    if (rc) return rc;
    pl.a.xq = (const uint8_t *)ws;
    pl.a.xq_col_stride = (int64_t)need;
    return launch_gemv(pl, stream);
}

}  // namespace kq
