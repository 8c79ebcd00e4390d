// kq_plan.hip — the fusion planner of the ggml-backend mirror: reads a node list and
// decides which nodes run as one launch (plan_launches), what the executor may hand from
// one launch to the next (attn_feeds_batched_mm, kv_epilogue), the key a captured
// hipGraph is cached under, and which nodes the device takes at all (supports_op).
// Host code only: no launch is issued here (kq_backend.hip enqueues the plan).
#include "kq_plan.h"

namespace kq {
namespace {

bool is_kquant(int t) { return t == MI355X_TYPE_Q4_K || t == MI355X_TYPE_Q5_K || t == MI355X_TYPE_Q6_K; }

// Byte range [lo, hi) a tensor's data spans (ggml_nbytes: the last element of every
// dim; K-quant rows are whole blocks).
struct Span {
    uintptr_t lo = 0, hi = 0;
};
Span span_of(const mi355x_tensor *t) {
    Span s;
    if (!t || !t->data) return s;
    const int64_t blck = is_kquant(t->type) ? MI355X_QK_K : 1;
    uint64_t bytes = (uint64_t)(t->ne[0] / blck) * t->nb[0];
    for (int d = 1; d < 4; ++d)
        if (t->ne[d] > 1) bytes += (uint64_t)(t->ne[d] - 1) * t->nb[d];
    s.lo = (uintptr_t)t->data;
    s.hi = s.lo + (uintptr_t)bytes;
    return s;
}

// readers[i]: number of node operands (over all nodes) that read node i's output.
// A read is credited to the LATEST earlier node whose output overlaps the operand's
// bytes (ggml-alloc reuses a dead node's buffer for a later node, so the latest
// writer is the producer); reads through views at an offset count too. When the
// latest overlapping writer does not cover the whole operand, older overlapping
// writers are credited as well: over-counting only disables a fusion, it never
// elides a live output.
std::vector<int> count_readers(mi355x_tensor *const *nodes, int n) {
    std::vector<int> r(n, 0);
    std::vector<Span> out(n);
    for (int i = 0; i < n; ++i)
        if (nodes[i]->op != MI355X_OP_NONE) out[i] = span_of(nodes[i]);
    for (int j = 0; j < n; ++j)
        for (int s = 0; s < MI355X_MAX_SRC; ++s) {
            const mi355x_tensor *u = nodes[j]->src[s];
            if (!u) continue;
            const Span us = span_of(u);
            for (int i = j - 1; i >= 0; --i) {
                if (nodes[i] == u) {  // the operand IS node i (whatever its buffer)
                    ++r[i];
                    break;
                }
                const Span &o = out[i];
                if (o.hi <= o.lo || us.hi <= us.lo || !(o.lo < us.hi && us.lo < o.hi)) continue;
                ++r[i];
                if (o.lo <= us.lo && us.hi <= o.hi) break;  // fully produced by node i
            }
        }
    return r;
}

bool elidable(const mi355x_tensor *t, int readers) {
    return readers == 1 && !(t->flags & MI355X_TENSOR_FLAG_OUTPUT);
}

bool is_gemv_node(const mi355x_tensor *t) { return t->op == MI355X_OP_MUL_MAT && t->src[1]->ne[1] == 1; }

// nodes[i] is an RMS_NORM and nodes[i + 1] the MUL of it (src[0]) by a weight: that MUL,
// else null. Shapes and readers are the caller's conditions.
const mi355x_tensor *norm_mul(mi355x_tensor *const *nodes, int n, int i) {
    if (nodes[i]->op != MI355X_OP_RMS_NORM || i + 1 >= n) return nullptr;
    const mi355x_tensor *m = nodes[i + 1];
    return m->op == MI355X_OP_MUL && m->src[0] == nodes[i] ? m : nullptr;
}

// A batched MUL_MAT that runs on the int8 GEMM (kq_mmq, Q8L activation blocks): always in
// the exact precision, and in the f16 one where kq_mmf is not the faster kernel
bool mm_exact(const mi355x_tensor *t) {
    const mi355x_tensor *w = t->src[0], *x = t->src[1];
    return !mmf_applies(w->type, w->data, w->ne[1], w->nb[1], x->ne[1], w->ne[0]);
}

// MUL_MATs that can share one tile-GEMM launch: one type, or K-quants of different types
// (kq_mmq_mixed: a prompt batch's Q4_K / Q5_K q/k with the Q6_K attn_v of use_more_bits layers)
bool multi_types_ok(int a, int b) { return a == b || (is_kquant(a) && is_kquant(b)); }

// A decode attention whose output only the next node, a GEMV (the o-proj), reads: both
// run as one kq_attn_oproj launch when its shape allows (bit-identical: kq_attn_oproj.hip).
bool attn_oproj_fusable(const PlanOpts &o, const mi355x_tensor *t, const mi355x_tensor *mm, int readers) {
    const int ko = (int)knob(KNOB_ATTN_OPROJ);  // A/B: 0 never, 2 every backend
    if (ko == 0 || (ko == 1 && !o.attn_oproj) || t->op != MI355X_OP_ATTN_DECODE || t->src[0]->ne[1] != 1) return false;
    if (attn_impl() == MI355X_ATTN_GROUP || !elidable(t, readers)) return false;  // (per-head kernels)
    if (!is_gemv_node(mm) || mm->src[1] != t || !is_kquant(mm->src[0]->type)) return false;
    const mi355x_tensor *w = mm->src[0];
    if (w->ne[0] != t->ne[0] || w->ne[2] != 1 || w->ne[3] != 1 || mm->nb[0] != 4) return false;
    const int nh = t->op_params[0], nkv = t->op_params[1], hd = t->op_params[2];
    return attn_oproj_buffer(hd, nh, nkv, (int)t->src[4]->ne[1], w->type, w->ne[0], w->ne[1], nullptr) > 0;
}

// ---- LaunchKind::Layer: the 15 nodes of one llm_build_llama decode layer as one kq_layer launch
bool contiguous_kq(const mi355x_tensor *w) {
    return is_kquant(w->type) && w->ne[0] % MI355X_QK_K == 0 && w->ne[2] == 1 && w->ne[3] == 1 &&
           w->nb[1] == (size_t)(w->ne[0] / MI355X_QK_K) * mi355x_row_size(w->type, MI355X_QK_K) &&
           (w->type == MI355X_TYPE_Q6_K || ((uintptr_t)w->data & 15u) == 0);
}
bool f32_vec(const mi355x_tensor *t, int64_t n, bool aligned16) {
    return t && t->type == MI355X_TYPE_F32 && nelem(t) == n && t->ne[0] == n && t->nb[0] == 4 && t->data &&
           (!aligned16 || ((uintptr_t)t->data & 15u) == 0);
}
// ADD(a, b) where one operand is node `mm` and the other is `res`'s bytes: true
bool add_of(const mi355x_tensor *ad, const mi355x_tensor *mm, const mi355x_tensor *res) {
    if (!ad || ad->op != MI355X_OP_ADD) return false;
    const mi355x_tensor *o = other_operand(ad, mm);
    return o && o->data == res->data && o->type == MI355X_TYPE_F32 && nelem(o) == nelem(res);
}
bool spans_overlap(const mi355x_tensor *p, const mi355x_tensor *q) {
    const Span a = span_of(p), c = span_of(q);
    return a.lo < c.hi && c.lo < a.hi;
}

bool layer_match(const PlanOpts &po, mi355x_tensor *const *nodes, int n, int i, const std::vector<int> &readers,
                 LayerArgs &la) {
    if (!po.layer_engine || i + 15 > n) return false;
    mi355x_tensor *const *t = nodes + i;
    const mi355x_tensor *n1 = t[0], *q = t[2], *k = t[3], *v = t[4], *at = t[5], *o = t[6], *x1 = t[7];
    const mi355x_tensor *n2 = t[8], *g = t[10], *u = t[11], *sw = t[12], *dn = t[13], *x2 = t[14];
    const mi355x_tensor *m1 = norm_mul(nodes, n, i), *m2 = norm_mul(nodes, n, i + 8);
    if (!m1 || !m2) return false;
    const mi355x_tensor *x = n1->src[0];
    const int64_t E = n1->ne[0];
    if (!f32_vec(x, E, true) || !f32_vec(n1, E, false) || !f32_vec(m1->src[1], E, true) || !f32_vec(m1, E, false))
        return false;
    if (!elidable(n1, readers[i]) || readers[i + 1] != 3 || (m1->flags & MI355X_TENSOR_FLAG_OUTPUT)) return false;
    for (const mi355x_tensor *mm : {q, k, v})
        if (!is_gemv_node(mm) || mm->src[1] != m1 || !contiguous_kq(mm->src[0]) || mm->src[0]->ne[0] != E ||
            !f32_vec(mm, mm->src[0]->ne[1], true))
            return false;
    if (at->op != MI355X_OP_ATTN_DECODE || at->src[0] != q || at->src[1] != k || at->src[2] != v) return false;
    if (at->src[6]->ne[1] != 1) return false;  // the position's rope row staged with the inputs
    const int nh = at->op_params[0], nkv = at->op_params[1], hd = at->op_params[2];
    if (k->src[0]->ne[1] != v->src[0]->ne[1] || (int64_t)nh * hd != q->src[0]->ne[1] || q->src[0]->ne[1] != E ||
        (int64_t)nkv * hd != k->src[0]->ne[1] || !f32_vec(at, E, true))
        return false;
    if (!is_gemv_node(o) || o->src[1] != at || !contiguous_kq(o->src[0]) || o->src[0]->ne[0] != E ||
        o->src[0]->ne[1] != E || !elidable(o, readers[i + 6]))
        return false;
    if (!add_of(x1, o, x) || !f32_vec(x1, E, true)) return false;
    if (n2->src[0] != x1 || !elidable(n2, readers[i + 8]) || !f32_vec(m2->src[1], E, true) || readers[i + 9] != 2 ||
        (m2->flags & MI355X_TENSOR_FLAG_OUTPUT))
        return false;
    if (f_of(n1->op_params[0]) != f_of(n2->op_params[0])) return false;  // one eps per layer (llama)
    for (const mi355x_tensor *mm : {g, u})
        if (!is_gemv_node(mm) || mm->src[1] != m2 || !contiguous_kq(mm->src[0]) || mm->src[0]->ne[0] != E)
            return false;
    const int64_t F = g->src[0]->ne[1];
    if (u->src[0]->ne[1] != F || !elidable(g, readers[i + 10]) || !elidable(u, readers[i + 11])) return false;
    if (sw->op != MI355X_OP_SWIGLU || sw->src[0] != g || sw->src[1] != u || !f32_vec(sw, F, true)) return false;
    if (!is_gemv_node(dn) || dn->src[1] != sw || !contiguous_kq(dn->src[0]) || dn->src[0]->ne[0] != F ||
        dn->src[0]->ne[1] != E || !elidable(dn, readers[i + 13]))
        return false;
    if (!add_of(x2, dn, x1) || !f32_vec(x2, E, false)) return false;
    // written in the launch: q, k, v, att, x1, h, x2 -- none of them over an input or another
    const mi355x_tensor *wr[6] = {q, k, v, at, x1, sw};
    for (int a0 = 0; a0 < 6; ++a0) {
        if (spans_overlap(wr[a0], x) || spans_overlap(wr[a0], x2)) return false;
        for (int a1 = a0 + 1; a1 < 6; ++a1)
            if (spans_overlap(wr[a0], wr[a1])) return false;
    }
    memset(&la, 0, sizeof(la));
    la.E = (int)E;
    la.F = (int)F;
    la.nq = (int)q->src[0]->ne[1];
    la.nkv = (int)k->src[0]->ne[1];
    const mi355x_tensor *ws[7] = {q->src[0], k->src[0], v->src[0], o->src[0], g->src[0], u->src[0], dn->src[0]};
    for (int m = 0; m < 7; ++m) {
        la.type[m] = ws[m]->type;
        la.w[m] = (const uint8_t *)ws[m]->data;
    }
    la.y[0] = (float *)q->data;
    la.y[1] = (float *)k->data;
    la.y[2] = (float *)v->data;
    la.x = (const float *)x->data;
    la.attn_norm = (const float *)m1->src[1]->data;
    la.ffn_norm = (const float *)m2->src[1]->data;
    la.eps = f_of(n1->op_params[0]);
    la.att = (float *)at->data;
    la.x1 = (float *)x1->data;
    la.h = (float *)sw->data;
    la.x2 = (float *)x2->data;
    mi355x_attn_desc d;
    attn_desc_of(at, d);
    d.rope_row = 1;
    if (attn_args_from(&d, la.at) != 0 || attn_size_refused(la.at)) return false;  // (streamed caches: ATTN_DECODE alone)
    return layer_plan(la, hd, nh) == MI355X_OK;
}

// supports_op: contiguous f32 with data
bool contig_f32(const mi355x_tensor *t) { return t && t->type == MI355X_TYPE_F32 && t->nb[0] == 4 && t->data; }

// A MOE_ROUTE node's output: T records of I32 [2 * n_used], 4-byte aligned, nb[1] the record stride
bool moe_records_ok(const mi355x_tensor *t, int n_used, int64_t T) {
    return t->type == MI355X_TYPE_I32 && t->data && !((uintptr_t)t->data & 3u) && t->nb[0] == 4 && n_used >= 1 &&
           t->ne[0] == 2 * (int64_t)n_used && t->ne[1] == T && T >= 1 && nelem(t) == t->ne[0] * T && t->nb[1] % 4 == 0 &&
           t->nb[1] >= (size_t)t->ne[0] * 4;
}

// ATTN_DECODE / ATTN_BATCH: the caches (src4, src5) exactly [n_ctx][kvw] and [kvw][n_ctx] f16,
// 16-B aligned (the kernels' addressing), n_ctx a multiple of 32 up to max_ctx (8192; up to
// kAttnStreamMaxCtx while mi355x_attn_stream is on); pos (src3) i32
bool kv_caches_ok(const mi355x_tensor *op, int nkv, int hd, int64_t max_ctx = 8192) {
    const mi355x_tensor *kc = op->src[4], *vc = op->src[5];
    if (kc->type != MI355X_TYPE_F16 || vc->type != MI355X_TYPE_F16) return false;
    if (kc->ne[0] != (int64_t)nkv * hd || op->src[3]->type != MI355X_TYPE_I32) return false;
    if (vc->ne[0] != kc->ne[1] || vc->ne[1] != kc->ne[0]) return false;
    if (kc->nb[0] != 2 || kc->nb[1] != (size_t)kc->ne[0] * 2) return false;
    if (vc->nb[0] != 2 || vc->nb[1] != (size_t)vc->ne[0] * 2) return false;
    if (((uintptr_t)kc->data & 15u) || ((uintptr_t)vc->data & 15u)) return false;
    const int64_t n_ctx = kc->ne[1];
    return n_ctx >= 32 && n_ctx % 32 == 0 && n_ctx <= max_ctx;
}

// T tokens (T > 1: rows packed): q [nh*hd, T], k, v [kvw, T] contiguous f32, pos [T]
bool qkv_rows_ok(const mi355x_tensor *op, int nh, int nkv, int hd, int64_t T) {
    for (int s = 0; s < 3; ++s)
        if (!contig_f32(op->src[s])) return false;
    if (op->src[0]->ne[0] != (int64_t)nh * hd) return false;
    if (nelem(op->src[0]) != (int64_t)nh * hd * T || nelem(op->src[1]) != (int64_t)nkv * hd * T ||
        nelem(op->src[2]) != (int64_t)nkv * hd * T || op->src[3]->ne[0] != T)
        return false;
    return T == 1 || (op->src[0]->nb[1] == (size_t)nh * hd * 4 && op->src[1]->nb[1] == (size_t)nkv * hd * 4 &&
                      op->src[2]->nb[1] == (size_t)nkv * hd * 4);
}

}  // namespace

void attn_desc_of(const mi355x_tensor *t, mi355x_attn_desc &a) {
    a.q = (const float *)t->src[0]->data;
    a.k = (const float *)t->src[1]->data;
    a.v = (const float *)t->src[2]->data;
    a.pos = (const int32_t *)t->src[3]->data;
    a.k_cache = (uint16_t *)t->src[4]->data;
    a.v_cache = (uint16_t *)t->src[5]->data;
    a.rope_table = (const float *)t->src[6]->data;
    a.out = (float *)t->data;
    a.n_head = t->op_params[0];
    a.n_head_kv = t->op_params[1];
    a.head_dim = t->op_params[2];
    a.scale = f_of(t->op_params[3]);
    a.n_ctx = (int)t->src[4]->ne[1];
}

// SAMPLE / SAMPLE_BATCH: op_params[1 .. 4] = top_k and the bits of temp, top_p, min_p
void sampler_of(const mi355x_tensor *t, mi355x_sampler &s) {
    s.top_k = t->op_params[1];
    s.temp = f_of(t->op_params[2]);
    s.top_p = f_of(t->op_params[3]);
    s.min_p = f_of(t->op_params[4]);
}

// PENALIZE: op_params = {last_n, the bits of repeat, freq, present, n_bias}; returns n_bias
int penalties_of(const mi355x_tensor *t, mi355x_penalties &p) {
    p.last_n = t->op_params[0];
    p.repeat = f_of(t->op_params[1]);
    p.freq = f_of(t->op_params[2]);
    p.present = f_of(t->op_params[3]);
    return t->op_params[4];
}

// KV_SHIFT: src0 .. src3 = K cache, V cache, rope table, deltas; op_params = {n_head_kv, head_dim,
// form, n_cells} (DELTAS) or {n_head_kv, head_dim, form, keep, discard, n_past} (DISCARD)
void kv_shift_desc_of(const mi355x_tensor *t, mi355x_kv_shift_desc &d) {
    memset(&d, 0, sizeof(d));
    d.k_cache = (uint16_t *)t->src[0]->data;
    d.v_cache = t->src[1] ? (uint16_t *)t->src[1]->data : nullptr;
    d.rope_table = (const float *)t->src[2]->data;
    d.delta = t->src[3] ? (const int32_t *)t->src[3]->data : nullptr;
    d.n_ctx = (int)t->src[0]->ne[1];
    d.n_head_kv = t->op_params[0];
    d.head_dim = t->op_params[1];
    d.n_pos = (int)t->src[2]->ne[1];
    d.form = t->op_params[2];
    if (d.form == MI355X_KV_SHIFT_DELTAS) {
        d.n_cells = t->op_params[3];
    } else {
        d.keep = t->op_params[3];
        d.discard = t->op_params[4];
        d.n_past = t->op_params[5];
    }
}

ArgmaxStep token_step_of(const mi355x_tensor *t) {
    const mi355x_tensor *tab = t->src[2], *hist = t->src[3];
    return {(const int32_t *)t->src[1]->data, (const float *)tab->data, (int32_t *)hist->data, tab->ne[1], hist->ne[0],
            (int)tab->ne[0]};
}

ArgmaxRowsStep rows_step_of(const mi355x_tensor *t, int first_param) {
    const mi355x_tensor *mask = t->src[3], *hist = t->src[4];
    return {(int32_t *)t->src[1]->data, (int32_t *)t->src[2]->data, (float *)mask->data, (int32_t *)hist->data,
            (int64_t)(mask->nb[1] / 4), (int64_t)(hist->nb[1] / 4), t->op_params[first_param + 1], hist->ne[0],
            t->op_params[first_param]};
}

// ATTN_BATCH: the ATTN_DECODE operands, the cells (src7), the mask (src8) and n_kv
void attn_batch_desc_of(const mi355x_tensor *t, mi355x_attn_batch_desc &d) {
    attn_desc_of(t, d.a);
    d.a.rope_row = 0;
    d.cells = t->src[7]->data;
    d.cells_type = t->src[7]->type;
    d.mask = t->src[8]->data;
    d.mask_type = t->src[8]->type;
    d.mask_row_bytes = t->src[8]->nb[1];
    d.n_kv = t->op_params[4];
    d.n_tokens = (int)t->src[0]->ne[1];
}

bool batched_mm_shares(const PlanOpts &o, const mi355x_tensor *t) {
    if (t->op != MI355X_OP_MUL_MAT) return false;
    const mi355x_tensor *w = t->src[0], *x = t->src[1];
    if (x->ne[1] < 16 || (x->nb[1] & 3u) || (t->nb[1] & 3u) || ((uintptr_t)o.workspace & 15u)) return false;
    if (!mmf_applies(w->type, w->data, w->ne[1], w->nb[1], x->ne[1], w->ne[0]) &&
        !mmq_applies(w->type, w->data, w->ne[1], w->nb[1], x->ne[1]))
        return false;
    return o.workspace_size >= mi355x_mul_mat_workspace_size(w->type, w->ne[0], w->ne[1], x->ne[1]);
}

std::vector<Launch> plan_launches(const PlanOpts &po, mi355x_tensor *const *nodes, int n) {
    const bool fuse = po.fuse;
    std::vector<Launch> out;
    const std::vector<int> readers = fuse ? count_readers(nodes, n) : std::vector<int>(n, 0);
    auto index_of = [&](const mi355x_tensor *u, int lo, int hi) {
        for (int i = lo; i < hi; ++i)
            if (nodes[i] == u) return i;
        return -1;
    };
    // a graph with MoE nodes joins neither the layer engine nor the attention + o-proj fusion
    bool moe = false;
    for (int k = 0; k < n; ++k)
        moe |= nodes[k]->op == MI355X_OP_MOE_ROUTE || nodes[k]->op == MI355X_OP_MUL_MAT_ID ||
               nodes[k]->op == MI355X_OP_MOE_COMBINE;
    int i = 0, ly_blocks = 0;
    while (i < n) {
        const mi355x_tensor *t = nodes[i];
        Launch l;
        l.first = i;
        l.count = 1;
        int head = i;  // first MUL_MAT of a run
        if (fuse && !moe && layer_match(po, nodes, n, i, readers, l.la)) {
            l.kind = LaunchKind::Layer;
            l.count = 15;
            l.ly_block = ly_blocks++;
            out.push_back(l);
            i += 15;
            continue;
        }
        if (fuse && !moe && i + 1 < n && attn_oproj_fusable(po, t, nodes[i + 1], readers[i])) {
            const mi355x_tensor *mm = nodes[i + 1];
            l.kind = LaunchKind::AttnOproj;
            l.count = 2;
            l.y[0] = (float *)mm->data;
            int end = i + 2;
            if (end < n && nodes[end]->op == MI355X_OP_ADD && elidable(mm, readers[i + 1])) {
                const mi355x_tensor *ad = nodes[end], *other = other_operand(ad, mm);
                if (other && index_of(other, i, end) < 0 && ad->ne[0] == mm->ne[0] && ad->ne[1] == 1 &&
                    ad->type == MI355X_TYPE_F32 && other->type == MI355X_TYPE_F32 && nelem(other) == ad->ne[0] &&
                    other->nb[0] == 4 && ad->nb[0] == 4) {
                    l.res[0] = (const float *)other->data;
                    l.y[0] = (float *)ad->data;
                    l.count = 3;
                    ++end;
                }
            }
            out.push_back(l);
            i = end;
            continue;
        }
        // RMS_NORM -> MUL(weight) starting here, whose norm output only the MUL reads
        const mi355x_tensor *nm = fuse ? norm_mul(nodes, n, i) : nullptr;
        if (nm && !elidable(t, readers[i])) nm = nullptr;
        // prologue fusion: RMS_NORM -> MUL -> MUL_MAT run, SWIGLU -> MUL_MAT run
        if (nm && i + 2 < n && is_gemv_node(nodes[i + 2]) && nodes[i + 2]->src[1] == nm && nm->ne[0] == t->ne[0] &&
            t->ne[1] == 1) {
            int cnt = 0;
            while (i + 2 + cnt < n && cnt < MI355X_MAX_FUSED && is_gemv_node(nodes[i + 2 + cnt]) &&
                   nodes[i + 2 + cnt]->src[1] == nm)
                ++cnt;
            if (readers[i + 1] == cnt && !(nm->flags & MI355X_TENSOR_FLAG_OUTPUT)) {
                l.pro = MI355X_PRO_RMS_NORM;
                l.x = (const float *)t->src[0]->data;
                l.x2 = (const float *)nm->src[1]->data;
                l.eps = f_of(t->op_params[0]);
                head = i + 2;
            }
        } else if (fuse && t->op == MI355X_OP_SWIGLU && i + 1 < n && is_gemv_node(nodes[i + 1]) &&
                   nodes[i + 1]->src[1] == t && elidable(t, readers[i]) && t->ne[1] == 1) {
            l.pro = MI355X_PRO_SWIGLU;
            l.x = (const float *)t->src[0]->data;
            l.x2 = (const float *)t->src[1]->data;
            head = i + 1;
        }
        const mi355x_tensor *h = nodes[head];
        if (h->op == MI355X_OP_MUL_MAT && h->src[1]->ne[1] == 1 && (l.pro != MI355X_PRO_NONE || head == i)) {
            int cnt = 1;
            while (head + cnt < n && cnt < MI355X_MAX_FUSED) {
                const mi355x_tensor *u = nodes[head + cnt];
                if (!is_gemv_node(u)) break;
                if (u->src[1]->data != h->src[1]->data || u->src[0]->ne[0] != h->src[0]->ne[0]) break;
                ++cnt;
            }
            l.kind = LaunchKind::GemvRun;
            l.first = head;
            l.count = cnt;
            if (l.pro == MI355X_PRO_NONE) l.x = (const float *)h->src[1]->data;
            for (int k = 0; k < cnt; ++k) l.y[k] = (float *)nodes[head + k]->data;
            int end = head + cnt;
            // epilogue fusion: ADD(mul_mat, residual) right after the run (the last
            // MUL_MAT's output, or any of the run's outputs, one ADD each)
            while (fuse && end < n && nodes[end]->op == MI355X_OP_ADD) {
                const mi355x_tensor *ad = nodes[end];
                int j = index_of(ad->src[0], head, head + cnt);
                if (j < 0) j = index_of(ad->src[1], head, head + cnt);
                if (j < 0) break;
                const int k = j - head;
                const mi355x_tensor *other = other_operand(ad, nodes[j]);
                if (l.res[k] || !elidable(nodes[j], readers[j])) break;
                if (index_of(other, i, end) >= 0) break;  // residual produced inside the fused range
                if (ad->ne[0] != nodes[j]->ne[0] || ad->ne[1] != 1 || ad->type != MI355X_TYPE_F32) break;
                l.res[k] = (const float *)other->data;
                l.y[k] = (float *)ad->data;
                ++end;
            }
            // epilogue fusion: SWIGLU(gate, up) of a two-MUL_MAT run whose outputs only it reads
            if (fuse && end < n && cnt == 2 && nodes[end]->op == MI355X_OP_SWIGLU && !l.res[0] && !l.res[1]) {
                const mi355x_tensor *sg = nodes[end];
                if (sg->src[0] == nodes[head] && sg->src[1] == nodes[head + 1] && elidable(nodes[head], readers[head]) &&
                    elidable(nodes[head + 1], readers[head + 1]) && nodes[head]->ne[0] == nodes[head + 1]->ne[0] &&
                    sg->ne[0] == nodes[head]->ne[0] && sg->ne[1] == 1 && sg->type == MI355X_TYPE_F32) {
                    l.epi_y = (float *)sg->data;
                    ++end;
                }
            }
            out.push_back(l);
            i = end;
            continue;
        }
        // prefill (batched, ne11 >= 16) fusions: the normed / swiglu'd activation goes straight
        // into the GEMMs' Q8L blocks (never written as f32), and MUL_MAT -> ADD as the GEMM's
        // epilogue; only where every consumer takes the shared-activation GEMM. On the f16
        // path (kq_mmf) only where every consumer stays on the int8 GEMM: kq_mmf reads an f16
        // image of the f32 activation.
        if (fuse) {
            auto shares_run = [&](int first, const mi355x_tensor *src, int &cnt) {
                cnt = 0;
                while (first + cnt < n && nodes[first + cnt]->op == MI355X_OP_MUL_MAT &&
                       nodes[first + cnt]->src[1] == src && batched_mm_shares(po, nodes[first + cnt]) &&
                       mm_exact(nodes[first + cnt]))
                    ++cnt;
                return cnt > 0;
            };
            int cnt = 0;
            if (nm && t->ne[1] >= 16 && i + 2 < n && nm->ne[0] == t->ne[0] && nm->ne[1] == t->ne[1] &&
                nm->src[1]->ne[0] == t->ne[0] && nelem(nm->src[1]) == t->ne[0] && t->nb[1] == (size_t)t->ne[0] * 4 &&
                t->src[0]->nb[1] == (size_t)t->ne[0] * 4 && ((uintptr_t)t->src[0]->data & 15u) == 0 &&
                !(nm->flags & MI355X_TENSOR_FLAG_OUTPUT) && shares_run(i + 2, nm, cnt) && readers[i + 1] == cnt) {
                l.kind = LaunchKind::PrefillPrologue;
                l.pro = MI355X_PRO_RMS_NORM;
                l.x = (const float *)t->src[0]->data;
                l.x2 = (const float *)nm->src[1]->data;
                l.eps = f_of(t->op_params[0]);
                l.q8_of = nm;
                l.count = 2;
                out.push_back(l);
                i += 2;
                continue;
            }
            if (t->op == MI355X_OP_SWIGLU && t->ne[1] >= 16 && t->ne[0] % MI355X_QK_K == 0 &&
                t->nb[1] == (size_t)t->ne[0] * 4 && t->src[0]->nb[1] == t->nb[1] && t->src[1]->nb[1] == t->nb[1] &&
                nelem(t->src[0]) == nelem(t) && nelem(t->src[1]) == nelem(t) && !(t->flags & MI355X_TENSOR_FLAG_OUTPUT) &&
                shares_run(i + 1, t, cnt) && readers[i] == cnt) {
                l.kind = LaunchKind::PrefillPrologue;
                l.pro = MI355X_PRO_SWIGLU;
                l.x = (const float *)t->src[0]->data;
                l.x2 = (const float *)t->src[1]->data;
                l.q8_of = t;
                out.push_back(l);
                i += 1;
                continue;
            }
            if (t->op == MI355X_OP_MUL_MAT && t->src[1]->ne[1] >= 16 && batched_mm_shares(po, t)) {
                // (the f16 GEMM: one weight type per launch)
                int run = 1;
                while (i + run < n && run < 4) {
                    const mi355x_tensor *u = nodes[i + run];
                    if (u->op != MI355X_OP_MUL_MAT || u->src[1] != t->src[1] ||
                        !(mm_exact(t) ? multi_types_ok(t->src[0]->type, u->src[0]->type)
                                      : t->src[0]->type == u->src[0]->type) ||
                        u->src[0]->ne[0] != t->src[0]->ne[0] || !batched_mm_shares(po, u))
                        break;
                    ++run;
                }
                if (run >= 2) {
                    l.kind = LaunchKind::MmMulti;
                    l.count = run;
                    out.push_back(l);
                    i += run;
                    continue;
                }
            }
            if (t->op == MI355X_OP_MUL_MAT && t->src[1]->ne[1] >= 16 && i + 1 < n && nodes[i + 1]->op == MI355X_OP_ADD &&
                elidable(t, readers[i]) && batched_mm_shares(po, t)) {
                const mi355x_tensor *ad = nodes[i + 1], *other = other_operand(ad, t);
                if (other && ad->ne[0] == t->ne[0] && ad->ne[1] == t->ne[1] && other->ne[0] == t->ne[0] &&
                    other->ne[1] == t->ne[1] && other->nb[0] == 4 && ad->nb[0] == 4 && ad->type == MI355X_TYPE_F32 &&
                    other->type == MI355X_TYPE_F32) {
                    l.kind = LaunchKind::MmAdd;
                    l.res[0] = (const float *)other->data;
                    l.y[0] = (float *)ad->data;
                    l.count = 2;
                    out.push_back(l);
                    i += 2;
                    continue;
                }
            }
        }
        // single node (with RMS_NORM -> MUL fused when the norm output is only read by the MUL)
        if (nm && nm->ne[0] == t->ne[0] && nm->src[1]->ne[0] == t->ne[0] && nm->src[1]->ne[1] == 1) {
            l.norm_w = (const float *)nm->src[1]->data;
            l.norm_y = (float *)nm->data;
            l.count = 2;
        }
        out.push_back(l);
        i += l.count;
    }
    return out;
}

// A prompt ATTN_DECODE (>= 16 tokens, contiguous rows) whose output is the activation of the
// batched MUL_MAT the next launch starts with, on the group kernel that can write its Q8L rows.
bool attn_feeds_batched_mm(const PlanOpts &o, const mi355x_tensor *t, const Launch &next,
                           mi355x_tensor *const *nodes) {
    if (t->src[0]->ne[1] < 16 || t->nb[1] != (size_t)t->ne[0] * 4) return false;
    if (next.kind != LaunchKind::Node && next.kind != LaunchKind::MmAdd && next.kind != LaunchKind::MmMulti) return false;
    const mi355x_tensor *m = nodes[next.first];
    if (m->op == MI355X_OP_MUL_MAT && !mm_exact(m)) return false;  // kq_mmf reads an f16 image, not Q8L
    if (m->op != MI355X_OP_MUL_MAT || m->src[1] != t || m->src[0]->ne[0] != t->ne[0]) return false;
    if (next.kind == LaunchKind::Node && next.count != 1) return false;
    if (!batched_mm_shares(o, m)) return false;
    mi355x_attn_desc d;
    attn_desc_of(t, d);
    d.rope_row = 0;
    AttnArgs a;
    return attn_args_from(&d, a) == 0 && attn_prompt_q8_ok(a);
}

// The MmMulti launch `l` holds the k and v MUL_MATs that the prompt ATTN_DECODE of `next`
// reads (src[1], src[2]): its KV-cache cells can be stored by the GEMM's epilogue.
bool kv_epilogue(mi355x_tensor *const *nodes, const Launch &l, const Launch &next, MmqKv &kv) {
    const mi355x_tensor *t = nodes[next.first];
    if (next.kind != LaunchKind::Node || t->op != MI355X_OP_ATTN_DECODE || t->src[0]->ne[1] < 2) return false;
    const int hd = t->op_params[2], n_head_kv = t->op_params[1];
    if ((hd != 64 && hd != 128) || n_head_kv <= 0) return false;
    const mi355x_tensor *kc = t->src[4], *vc = t->src[5];
    if (((uintptr_t)kc->data & 15u) || ((uintptr_t)vc->data & 15u)) return false;
    memset(&kv, 0, sizeof(kv));
    int found = 0;
    for (int k = 0; k < l.count; ++k) {
        const mi355x_tensor *u = nodes[l.first + k];
        const int role = u == t->src[1] ? 1 : u == t->src[2] ? 2 : 0;
        if (!role) continue;
        if (u->ne[0] != (int64_t)n_head_kv * hd || u->ne[1] != t->src[0]->ne[1]) return false;
        kv.kind[k] = role;
        found |= role;
    }
    if (found != 3) return false;
    kv.pos = (const int32_t *)t->src[3]->data;
    kv.rope = (const float *)t->src[6]->data;
    kv.k_cache = (uint16_t *)kc->data;
    kv.v_cache = (uint16_t *)vc->data;
    kv.n_ctx = (int)kc->ne[1];
    kv.hd = hd;
    return true;
}

std::vector<uint64_t> graph_key_of(mi355x_tensor *const *nodes, int n_nodes) {
    std::vector<uint64_t> key;
    key.reserve((size_t)n_nodes * 16 + 2);
    // the plan captured under this key also depends on the process-wide kernel selectors
    // (mmq_impl decides MmMulti batching and the KV-store epilogue, attn_prompt_impl the
    // attention's Q8L output, ...): a changed selector must not replay the old graph
    key.push_back(api_selector_key());
    key.push_back(ops_selector_key());
    for (int i = 0; i < n_nodes; ++i) {
        const mi355x_tensor *t = nodes[i];
        key.push_back((uint64_t)(uintptr_t)t->data);
        key.push_back((uint64_t)t->op);
        key.push_back((uint64_t)t->flags);
        for (int d = 0; d < 4; ++d) key.push_back((uint64_t)t->ne[d]);
        for (int d = 0; d < 8; ++d) key.push_back((uint64_t)(uint32_t)t->op_params[d]);
        for (int s = 0; s < MI355X_MAX_SRC; ++s) {
            const mi355x_tensor *u = t->src[s];
            if (!u) { key.push_back(0); continue; }
            key.push_back((uint64_t)(uintptr_t)u->data);
            key.push_back((uint64_t)u->type);
            for (int d = 0; d < 4; ++d) key.push_back((uint64_t)u->ne[d]);
            for (int d = 0; d < 4; ++d) key.push_back((uint64_t)u->nb[d]);
        }
        for (int d = 0; d < 4; ++d) key.push_back((uint64_t)t->nb[d]);
    }
    return key;
}

// ggml_backend_device_i::supports_op for this device: MUL_MAT of a contiguous-row
// K-quant src0 with an f32 src1, 2-D (no broadcast over ne2/ne3), and the other
// nodes of a llama decode token on contiguous f32 (the op table in the header).
bool supports_op(const mi355x_tensor *op) {
    if (!op) return false;
    switch (op->op) {
        case MI355X_OP_NONE:
            return true;
        case MI355X_OP_MUL_MAT: {
            const mi355x_tensor *w = op->src[0], *x = op->src[1];
            if (!w || !x) return false;
            if (!is_kquant(w->type) || x->type != MI355X_TYPE_F32 || op->type != MI355X_TYPE_F32) return false;
            if (w->ne[0] % MI355X_QK_K || w->ne[0] != x->ne[0]) return false;
            if (w->ne[2] != 1 || w->ne[3] != 1 || x->ne[2] != 1 || x->ne[3] != 1) return false;
            if (op->ne[0] != w->ne[1] || op->ne[1] != x->ne[1]) return false;
            if (x->nb[0] != 4 || op->nb[0] != 4) return false;  // contiguous rows
            return w->nb[0] == mi355x_row_size(w->type, MI355X_QK_K);
        }
        case MI355X_OP_GET_ROWS: {
            const mi355x_tensor *w = op->src[0], *ids = op->src[1];
            if (!w || !ids || ids->type != MI355X_TYPE_I32 || !ids->data || ids->nb[0] != 4 || !contig_f32(op))
                return false;
            if (w->type != MI355X_TYPE_F32 && !is_kquant(w->type)) return false;
            if (op->ne[1] > 1 && op->nb[1] != (size_t)op->ne[0] * 4) return false;  // dst rows packed (kernel: out + r*k)
            return op->ne[0] == w->ne[0] && op->ne[1] == ids->ne[0] && w->ne[0] % MI355X_QK_K == 0;
        }
        case MI355X_OP_RMS_NORM:
            // the kernel reads x + row*n with 16-B loads: src0 and dst packed rows, 16-B aligned
            return contig_f32(op) && contig_f32(op->src[0]) && op->ne[0] % MI355X_QK_K == 0 &&
                   op->nb[1] == (size_t)op->ne[0] * 4 && op->src[0]->nb[1] == (size_t)op->ne[0] * 4 &&
                   nelem(op->src[0]) == nelem(op) && ((uintptr_t)op->src[0]->data & 15u) == 0;
        case MI355X_OP_MUL:
        case MI355X_OP_ADD:
            // src1 the same shape, or one row repeated over the rows (ggml_mul by the norm weight)
            return contig_f32(op) && contig_f32(op->src[0]) && contig_f32(op->src[1]) && nelem(op->src[0]) == nelem(op) &&
                   (nelem(op->src[1]) == nelem(op) || (nelem(op->src[1]) == op->ne[0] && op->nb[1] == (size_t)op->ne[0] * 4));
        case MI355X_OP_SWIGLU:
            return contig_f32(op) && contig_f32(op->src[0]) && contig_f32(op->src[1]) &&
                   nelem(op->src[0]) == nelem(op) && nelem(op->src[1]) == nelem(op);
        case MI355X_OP_ROPE:
            return contig_f32(op) && contig_f32(op->src[0]) && op->src[1] && op->src[1]->type == MI355X_TYPE_I32 &&
                   contig_f32(op->src[2]) && op->op_params[0] > 0 && op->op_params[0] <= op->ne[0] &&
                   op->src[2]->ne[0] == op->op_params[0];
        case MI355X_OP_ALL_GATHER:
            // a packed f32 slice gathered into a packed f32 vector (world known at compute time)
            return contig_f32(op) && contig_f32(op->src[0]) && op->ne[1] == 1 && op->src[0]->ne[1] == 1 &&
                   op->src[0]->ne[0] > 0 && op->ne[0] % op->src[0]->ne[0] == 0;
        case MI355X_OP_ALL_REDUCE:
            // a packed f32 partial summed over the ranks into a packed f32 vector of the same length
            return contig_f32(op) && contig_f32(op->src[0]) && nelem(op) == nelem(op->src[0]) && nelem(op) > 0;
        case MI355X_OP_ATTN_DECODE: {
            for (int s = 0; s < 7; ++s)
                if (!op->src[s] || !op->src[s]->data) return false;
            const int nh = op->op_params[0], nkv = op->op_params[1], hd = op->op_params[2];
            if ((hd != 64 && hd != 128) || nkv <= 0 || nh % nkv) return false;
            // T tokens (T > 1: a prompt batch): one rope row per position of the whole table
            const int64_t T = op->src[0]->ne[1], n_ctx = op->src[4]->ne[1];
            if (T < 1 || T > 0x7fffffff) return false;
            if (!kv_caches_ok(op, nkv, hd, attn_stream_mode() != 0 ? kAttnStreamMaxCtx : 8192) ||
                !qkv_rows_ok(op, nh, nkv, hd, T))
                return false;
            if (T > 1 && op->src[6]->ne[1] < n_ctx) return false;
            if (op->src[6]->ne[1] != 1 && op->src[6]->ne[1] < n_ctx) return false;  // row or table
            if (op->src[6]->ne[0] != hd) return false;
            return contig_f32(op) && op->ne[0] == (int64_t)nh * hd && op->ne[1] == T &&
                   (T == 1 || op->nb[1] == (size_t)nh * hd * 4);
        }
        case MI355X_OP_ATTN_BATCH: {
            for (int s = 0; s < 9; ++s)
                if (!op->src[s] || !op->src[s]->data) return false;
            const int nh = op->op_params[0], nkv = op->op_params[1], hd = op->op_params[2], n_kv = op->op_params[4];
            if ((hd != 64 && hd != 128) || nkv <= 0 || nh <= 0 || nh % nkv) return false;
            const mi355x_tensor *tab = op->src[6], *cells = op->src[7], *mask = op->src[8];
            // T tokens: q, k, v, pos as ATTN_DECODE's, cells [T]
            const int64_t T = op->src[0]->ne[1];
            if (T < 1 || T > 65535) return false;
            if (!kv_caches_ok(op, nkv, hd, attn_stream_mode() != 0 ? kAttnStreamMaxCtx : 8192) ||
                !qkv_rows_ok(op, nh, nkv, hd, T))
                return false;
            if (n_kv < 32 || n_kv % 32 || n_kv > op->src[4]->ne[1]) return false;
            if (!contig_f32(tab) || tab->ne[0] != hd || tab->ne[1] < 1 || tab->ne[1] > 0x7fffffff) return false;
            if ((cells->type != MI355X_TYPE_I32 && cells->type != MI355X_TYPE_I64) || nelem(cells) != T) return false;
            if (cells->nb[0] != (cells->type == MI355X_TYPE_I64 ? 8u : 4u)) return false;
            if (mask->type != MI355X_TYPE_F16 && mask->type != MI355X_TYPE_F32) return false;
            const size_t me = mask->type == MI355X_TYPE_F16 ? 2 : 4;
            if (mask->nb[0] != me || mask->ne[0] < n_kv || mask->ne[1] < T || mask->nb[1] < (size_t)n_kv * me) return false;
            mi355x_attn_batch_desc d;
            attn_batch_desc_of(op, d);
            AttnBatchArgs ba;
            // the LDS of either form, or the streamed form under mi355x_attn_stream
            if (attn_batch_args_from(&d, (int)tab->ne[1], ba) != MI355X_OK) return false;
            return contig_f32(op) && op->ne[0] == (int64_t)nh * hd && op->ne[1] == T &&
                   (T == 1 || op->nb[1] == (size_t)nh * hd * 4);
        }
        case MI355X_OP_ARGMAX: {
            // a packed, 16-B aligned f32 vector of mi355x_argmax's sizes -> I32 [1]; the
            // step-inputs form: pos [1], the rope table [hd, rows], the history -> I32 [2 + hd]
            const mi355x_tensor *x = op->src[0];
            if (!x || x->ne[0] < 1 || x->ne[0] > kArgmaxMaxN || !f32_vec(x, x->ne[0], true)) return false;
            if (op->type != MI355X_TYPE_I32 || !op->data || op->nb[0] != 4 || nelem(op) != op->ne[0]) return false;
            if (op->op_params[0] == 0) return op->ne[0] == 1;
            if (op->op_params[0] != 1) return false;
            const mi355x_tensor *pos = op->src[1], *tab = op->src[2], *hist = op->src[3];
            auto i32_vec = [](const mi355x_tensor *t) {
                return t && t->type == MI355X_TYPE_I32 && t->data && t->nb[0] == 4 && t->ne[0] >= 1 && nelem(t) == t->ne[0];
            };
            if (!i32_vec(pos) || pos->ne[0] != 1 || !i32_vec(hist) || hist->ne[0] > 0x7fffffff) return false;
            if (!contig_f32(tab) || tab->ne[0] < 1 || tab->ne[1] < 1 || tab->ne[1] > 0x7fffffff || tab->ne[2] != 1 ||
                tab->ne[3] != 1 || tab->nb[1] != (size_t)tab->ne[0] * 4)
                return false;
            return op->ne[0] == 2 + tab->ne[0];
        }
        case MI355X_OP_ARGMAX_BATCH: {
            // f32 [n, T] of mi355x_argmax_rows' sizes, rows packed and 16-B aligned -> I32 [T]; the
            // step-inputs form: pos [T], cells [T], the f32 mask [>= n_kv, T], the history [n_hist, T]
            const mi355x_tensor *x = op->src[0];
            if (!x || x->type != MI355X_TYPE_F32 || !x->data || ((uintptr_t)x->data & 15u) || x->nb[0] != 4) return false;
            const int64_t n = x->ne[0], T = x->ne[1];
            if (n < 1 || n > kArgmaxMaxN || n % 4 || T < 1 || T > kArgmaxMaxRows || nelem(x) != n * T) return false;
            if (x->nb[1] != (size_t)n * 4) return false;
            auto i32_vec = [T](const mi355x_tensor *t) {
                return t && t->type == MI355X_TYPE_I32 && t->data && t->nb[0] == 4 && t->ne[0] == T && nelem(t) == T;
            };
            if (!i32_vec(op)) return false;
            if (op->op_params[0] == 0) return true;
            if (op->op_params[0] != 1) return false;
            const mi355x_tensor *mask = op->src[3], *hist = op->src[4];
            const int64_t n_kv = op->op_params[2];
            if (!i32_vec(op->src[1]) || !i32_vec(op->src[2]) || op->op_params[1] < 1 || n_kv < 1) return false;
            if (!mask || mask->type != MI355X_TYPE_F32 || !mask->data || mask->nb[0] != 4 || mask->ne[0] < n_kv ||
                mask->ne[1] != T || nelem(mask) != mask->ne[0] * T || mask->nb[1] % 4 || mask->nb[1] < (size_t)n_kv * 4)
                return false;
            return hist && hist->type == MI355X_TYPE_I32 && hist->data && hist->nb[0] == 4 && hist->ne[0] >= 1 &&
                   hist->ne[0] <= 0x7fffffff && hist->ne[1] == T && nelem(hist) == hist->ne[0] * T && hist->nb[1] % 4 == 0 &&
                   hist->nb[1] >= (size_t)hist->ne[0] * 4;
        }
        case MI355X_OP_SAMPLE:
        case MI355X_OP_SAMPLE_BATCH: {
            // the ARGMAX / ARGMAX_BATCH node of the same form on the same operands, the sampler's
            // parameters in their ranges, and one more source: the draw(s) of the plain form (F32
            // [1] / [T]) or the draws table of the step-inputs form (F32 [n_draws] / [n_draws, T])
            const bool batch = op->op == MI355X_OP_SAMPLE_BATCH;
            const int form = op->op_params[0];
            if (form != 0 && form != 1) return false;
            mi355x_sampler sp;
            sampler_of(op, sp);
            if (!sampler_ok(&sp)) return false;
            mi355x_tensor am = *op;
            am.op = batch ? MI355X_OP_ARGMAX_BATCH : MI355X_OP_ARGMAX;
            am.op_params[1] = op->op_params[5], am.op_params[2] = op->op_params[6];
            if (!supports_op(&am)) return false;
            const mi355x_tensor *u = op->src[form == 0 ? 1 : batch ? 5 : 4];
            const int64_t T = batch ? op->src[0]->ne[1] : 1;
            if (!u || u->type != MI355X_TYPE_F32 || !u->data || ((uintptr_t)u->data & 3u) || u->nb[0] != 4) return false;
            if (form == 0) return u->ne[0] == T && nelem(u) == T;
            return u->ne[0] >= 1 && u->ne[0] <= 0x7fffffff && u->ne[1] == T && nelem(u) == u->ne[0] * T &&
                   (T == 1 || (u->nb[1] % 4 == 0 && u->nb[1] >= (size_t)u->ne[0] * 4));
        }
        case MI355X_OP_LOGPROB_BATCH: {
            // f32 [n, T] of mi355x_logprob_rows' sizes, rows packed and 16-B aligned, and I32 targets
            // [T] -> I32 [6, T], 8-B aligned: the rows' records
            const mi355x_tensor *x = op->src[0], *tg = op->src[1];
            if (!x || x->type != MI355X_TYPE_F32 || !x->data || ((uintptr_t)x->data & 15u) || x->nb[0] != 4) return false;
            const int64_t n = x->ne[0], T = x->ne[1];
            if (n < 1 || n > kLogprobMaxN || n % 4 || T < 1 || T > kArgmaxMaxRows || nelem(x) != n * T) return false;
            if (x->nb[1] != (size_t)n * 4) return false;
            if (!tg || tg->type != MI355X_TYPE_I32 || !tg->data || ((uintptr_t)tg->data & 3u) || tg->nb[0] != 4 ||
                tg->ne[0] != T || nelem(tg) != T)
                return false;
            return op->type == MI355X_TYPE_I32 && op->data && !((uintptr_t)op->data & 7u) && op->nb[0] == 4 &&
                   op->ne[0] == 6 && op->ne[1] == T && nelem(op) == 6 * T && op->nb[1] == sizeof(mi355x_logprob);
        }
        case MI355X_OP_PENALIZE: {
            // in place on src0, f32 [n, T] of mi355x_penalize_rows' sizes with packed rows; end I32 [T]
            // and the history I32 [n_hist, T] (null at last_n 0); the bias lists I32 / F32 [n_bias]
            // (null at n_bias 0)
            const mi355x_tensor *x = op->src[0], *end = op->src[1], *hist = op->src[2], *bt = op->src[3], *bv = op->src[4];
            if (!x || x->type != MI355X_TYPE_F32 || !x->data || ((uintptr_t)x->data & 3u) || x->nb[0] != 4) return false;
            const int64_t n = x->ne[0], T = x->ne[1];
            if (n < 1 || n > kArgmaxMaxN || T < 1 || T > kArgmaxMaxRows || nelem(x) != n * T || x->nb[1] != (size_t)n * 4)
                return false;
            if (op->data != x->data || op->type != x->type || memcmp(op->ne, x->ne, sizeof(op->ne)) ||
                memcmp(op->nb, x->nb, sizeof(op->nb)))
                return false;
            mi355x_penalties pen;
            const int n_bias = penalties_of(op, pen);
            if (!penalties_ok(&pen, n_bias)) return false;
            if (pen.last_n > 0) {
                if (!end || end->type != MI355X_TYPE_I32 || !end->data || end->nb[0] != 4 || end->ne[0] != T || nelem(end) != T)
                    return false;
                if (!hist || hist->type != MI355X_TYPE_I32 || !hist->data || hist->nb[0] != 4 || hist->ne[0] < 1 ||
                    hist->ne[0] > 0x7fffffff || hist->ne[1] != T || nelem(hist) != hist->ne[0] * T || hist->nb[1] % 4 ||
                    hist->nb[1] < (size_t)hist->ne[0] * 4)
                    return false;
            }
            if (n_bias > 0) {
                auto list = [n_bias](const mi355x_tensor *t, int type) {
                    return t && t->type == type && t->data && t->nb[0] == 4 && t->ne[0] == n_bias && nelem(t) == n_bias;
                };
                if (!list(bt, MI355X_TYPE_I32) || !list(bv, MI355X_TYPE_F32)) return false;
            }
            return true;
        }
        case MI355X_OP_KV_SHIFT: {
            // in place on src0, the K cache F16 [kvw, n_ctx], packed rows, 16-B aligned; the V cache F16
            // [n_ctx, kvw] (DISCARD; optional in DELTAS); the table f32 [hd, n_pos]; I32 deltas [n_cells]
            // (DELTAS); the parameters in mi355x_kv_shift's ranges
            const mi355x_tensor *kc = op->src[0], *vc = op->src[1], *tab = op->src[2], *dl = op->src[3];
            const int nkv = op->op_params[0], hd = op->op_params[1], form = op->op_params[2];
            if ((hd != 64 && hd != 128) || nkv < 1 || (int64_t)nkv * hd > 0x7fffffff) return false;
            if (!kc || kc->type != MI355X_TYPE_F16 || !kc->data || ((uintptr_t)kc->data & 15u)) return false;
            const int64_t kvw = (int64_t)nkv * hd, n_ctx = kc->ne[1];
            if (kc->ne[0] != kvw || n_ctx < 1 || n_ctx > 0x7fffffff || nelem(kc) != kvw * n_ctx || kc->nb[0] != 2 ||
                kc->nb[1] != (size_t)kvw * 2)
                return false;
            if (op->data != kc->data || op->type != kc->type || memcmp(op->ne, kc->ne, sizeof(op->ne)) ||
                memcmp(op->nb, kc->nb, sizeof(op->nb)))
                return false;
            if (!contig_f32(tab) || ((uintptr_t)tab->data & 15u) || tab->ne[0] != hd || tab->ne[1] < 1 ||
                tab->ne[1] > 0x7fffffff || nelem(tab) != tab->ne[0] * tab->ne[1] || tab->nb[1] != (size_t)hd * 4)
                return false;
            if (vc && (vc->type != MI355X_TYPE_F16 || !vc->data || vc->ne[0] != n_ctx || vc->ne[1] != kvw ||
                       nelem(vc) != kvw * n_ctx || vc->nb[0] != 2 || vc->nb[1] != (size_t)n_ctx * 2))
                return false;
            if (form == MI355X_KV_SHIFT_DELTAS) {
                const int n_cells = op->op_params[3];
                return n_cells >= 0 && n_cells <= n_ctx && dl && dl->type == MI355X_TYPE_I32 && dl->data &&
                       !((uintptr_t)dl->data & 3u) && dl->nb[0] == 4 && dl->ne[0] == n_cells && nelem(dl) == n_cells;
            }
            if (form != MI355X_KV_SHIFT_DISCARD || !vc || dl) return false;
            const int64_t keep = op->op_params[3], discard = op->op_params[4], n_past = op->op_params[5];
            return keep >= 0 && discard >= 1 && keep + discard <= n_past && n_past <= n_ctx && discard < tab->ne[1];
        }
        case MI355X_OP_MOE_ROUTE: {
            // gate_inp f32 [n_embd, n_expert] packed, x f32 [n_embd, T] -> the records I32 [2 * n_used, T]
            const mi355x_tensor *gi = op->src[0], *x = op->src[1];
            const int n_used = op->op_params[0];
            if (!contig_f32(gi) || !contig_f32(x)) return false;
            const int64_t E = gi->ne[0], ne = gi->ne[1], T = x->ne[1];
            if (E < 16 || E % 16 || E > 0x7fffffff || ne < 2 || ne > MI355X_MOE_MAX_EXPERTS || nelem(gi) != E * ne ||
                gi->nb[1] != (size_t)E * 4)
                return false;
            if (n_used < 1 || n_used > ne || n_used > MI355X_MOE_MAX_USED) return false;
            if (x->ne[0] != E || T < 1 || T > 65535 / n_used || nelem(x) != E * T || x->nb[1] % 4 ||
                x->nb[1] < (size_t)E * 4)
                return false;
            return moe_records_ok(op, n_used, T);
        }
        case MI355X_OP_MUL_MAT_ID: {
            // the expert tensor [K, N, n_expert], the activations f32 [K, ne11, T], the MOE_ROUTE node
            // -> f32 [N, n_used, T] packed
            const mi355x_tensor *w = op->src[0], *x = op->src[1], *rt = op->src[2];
            if (!w || !x || !rt || !w->data || !is_kquant(w->type) || !contig_f32(x) || !contig_f32(op)) return false;
            if (rt->op != MI355X_OP_MOE_ROUTE || rt->ne[0] < 2 || rt->ne[0] % 2) return false;
            const int64_t K = w->ne[0], N = w->ne[1], ne = w->ne[2], n_used = rt->ne[0] / 2, T = rt->ne[1];
            if (!moe_records_ok(rt, (int)n_used, T) || n_used > MI355X_MOE_MAX_USED) return false;
            if (K < MI355X_QK_K || K % MI355X_QK_K || K > MI355X_MUL_MAT_ID_MAX_K || N < 1 || N > 0x7fffffff || ne < 1 ||
                ne > MI355X_MOE_MAX_EXPERTS || w->ne[3] != 1 || T * n_used > 65535)
                return false;
            if (w->nb[0] != mi355x_row_size(w->type, MI355X_QK_K) || w->nb[1] < (size_t)(K / MI355X_QK_K) * w->nb[0] ||
                w->nb[2] < (size_t)N * w->nb[1])
                return false;
            if (w->type != MI355X_TYPE_Q6_K && (((uintptr_t)w->data & 15u) || (w->nb[1] & 15u) || (w->nb[2] & 15u)))
                return false;
            if (w->type == MI355X_TYPE_Q6_K && (((uintptr_t)w->data & 1u) || (w->nb[1] & 1u) || (w->nb[2] & 1u)))
                return false;  // (a Q6_K block at an even address)
            const int64_t ne11 = x->ne[1];
            if (x->ne[0] != K || (ne11 != 1 && ne11 != n_used) || x->ne[2] != T || x->ne[3] != 1 ||
                ((uintptr_t)x->data & 15u) || x->nb[1] % 16 || x->nb[1] < (size_t)K * 4 ||
                x->nb[2] != (size_t)ne11 * x->nb[1])
                return false;
            return op->ne[0] == N && op->ne[1] == n_used && op->ne[2] == T && op->ne[3] == 1 &&
                   op->nb[1] == (size_t)N * 4 && op->nb[2] == (size_t)N * 4 * n_used;
        }
        case MI355X_OP_MOE_COMBINE: {
            // the experts' outputs f32 [n, n_used, T] packed, the MOE_ROUTE node -> f32 [n, T] packed
            const mi355x_tensor *ex = op->src[0], *rt = op->src[1];
            if (!contig_f32(ex) || !rt || rt->op != MI355X_OP_MOE_ROUTE || rt->ne[0] < 2 || rt->ne[0] % 2 ||
                !contig_f32(op))
                return false;
            const int64_t n = ex->ne[0], n_used = rt->ne[0] / 2, T = rt->ne[1];
            if (!moe_records_ok(rt, (int)n_used, T) || n_used > MI355X_MOE_MAX_USED || T > 65535) return false;
            if (n < 1 || n > 0x7fffff00 || ex->ne[1] != n_used || ex->ne[2] != T || ex->ne[3] != 1 ||
                ex->nb[1] != (size_t)n * 4 || ex->nb[2] != (size_t)n * 4 * n_used)
                return false;
            return op->ne[0] == n && op->ne[1] == T && nelem(op) == n * T && op->nb[1] == (size_t)n * 4;
        }
        default:
            return false;
    }
}

}  // namespace kq
