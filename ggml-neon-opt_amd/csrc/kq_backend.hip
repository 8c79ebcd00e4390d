// kq_backend.hip — the ggml-backend mirror: a HIP "device" that owns a stream,
// device buffers and a hipGraph cache, and executes MUL_MAT nodes.
//
// Sibling of the reference's CPU backend entry ggml_backend_cpu_graph_compute
// (ggml-cpu.cpp:186, README.md:162), called by the scheduler at
// ggml_backend_sched_compute_splits (ggml-backend.cpp:1553, README.md:163).
// Where the CPU backend fans the graph out to OpenMP threads and each thread
// walks every node (ggml_graph_compute_thread, ggml-cpu.c:2883), this backend
// enqueues one kernel per (fused) node on its HIP stream; repeated graphs
// (decode steps) are replayed from a captured hipGraph. Which nodes fuse into one
// launch is the planner's decision (kq_plan.h); this file executes the plan.
#include <algorithm>
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <rccl/rccl.h>

#include <string>
#include <vector>

#include "kq_common.h"
#include "kq_internal.h"
#include "kq_plan.h"

using kq::attn_batch_desc_of;
using kq::attn_desc_of;
using kq::rows_step_of;
using kq::kv_shift_desc_of;
using kq::penalties_of;
using kq::sampler_of;
using kq::token_step_of;
using kq::f_of;
using kq::Launch;
using kq::LaunchKind;
using kq::nelem;

struct mi355x_backend {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string name;
    void *workspace = nullptr;
    size_t workspace_size = 0;
    // captured hipGraphs by node-list key, most recently used last (the decode token and
    // a prompt batch alternate without recapturing)
    struct Captured {
        std::vector<uint64_t> key;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
    };
    std::vector<Captured> graphs;
    bool fuse = true;
    bool attn_oproj = false;  // decode attention + o-proj GEMV in one launch (kq_attn_oproj.hip): measured
                              // slower than the two launches, so opt-in
    void *fx = nullptr;      // its arrival counters (zeroed at allocation) and records
    size_t fx_size = 0;
    int fx_nsb = 0;          // the superblock count the counters' rounds are aligned to
    void *am = nullptr;      // the ARGMAX / ARGMAX_BATCH / LOGPROB_BATCH nodes' arrival counters and partials, zeroed at
    size_t am_size = 0;      // allocation; every launch leaves them ready for the next
    void *sm = nullptr;      // the SAMPLE / SAMPLE_BATCH nodes' counters and words (kq_sample.hip), as am
    size_t sm_size = 0;
    void *mg = nullptr;      // the grouped MUL_MAT_ID nodes' group table (kq_moe_group): one, rebuilt per MOE_ROUTE
    size_t mg_size = 0;      // node; the Q8L rows share the workspace with the other GEMMs
    bool layer_engine = false;  // each decode layer as one persistent launch (kq_layer.hip)
    uint32_t *ly_sync = nullptr;  // the persistent layers' counter blocks (zeroed at allocation), then err
    int ly_blocks = 0;
    std::vector<std::vector<uint32_t>> ly_keys;  // block i's (layer index, producers per edge and shard)
    struct LyTab {                 // step tables (kq::layer_table_fill) built for one full geometry `key`
        void *dev = nullptr;
        int64_t stride = 0;
        std::vector<uint64_t> key;
    };
    std::vector<LyTab> ly_tabs;    // one entry per distinct key (several models / cache sizes coexist)
    ncclComm_t comm = nullptr;  // row split: one RCCL communicator per backend (rank of a world)
    bool loop_nocopy = false;   // emulated rank, timing only (MI355X_LOOPBACK_NOCOPY)
    int rank = 0, world = 0;
    int loop_rank = -1, loop_world = 0;  // single-GPU emulation of one rank (tests)
};

namespace {

// Every backend entry point runs on the backend's own device and restores the
// caller's current device afterwards (ggml-cuda's ggml_cuda_set_device discipline):
// one process may hold several backends (llama.cpp's layer split).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) hipSetDevice(prev);
    }
};

// The persistent layers' step tables depend on every field layer_table_fill reads: the
// weights and their types, the stage shapes, the ring geometry (D, slot: byte positions
// and issue gates) and the attention placement and LDS layout (which move with n_ctx).
constexpr size_t kMaxLyTabs = 256;

std::vector<uint64_t> ly_tab_key(const kq::LayerArgs &la) {
    std::vector<uint64_t> key = {(uint64_t)la.G,      (uint64_t)la.E,           (uint64_t)la.F,
                                 (uint64_t)la.nb_e,   (uint64_t)la.nb_f,        (uint64_t)la.nq,
                                 (uint64_t)la.nkv,    (uint64_t)la.n_attn,      (uint64_t)la.hpw,
                                 (uint64_t)la.attn_stride, (uint64_t)la.head_lds, (uint64_t)la.D,
                                 (uint64_t)la.slot,   (uint64_t)la.o_aux,       (uint64_t)la.act_bytes,
                                 (uint64_t)la.o_sums, (uint64_t)la.o_res,       (uint64_t)la.lds};
    for (int m = 0; m < 7; ++m) {
        key.push_back((uint64_t)(uintptr_t)la.w[m]);
        key.push_back((uint64_t)la.type[m]);
    }
    return key;
}

// ---- RCCL, resolved at run time: the copy already loaded in the process (torch
// bundles one) or /opt/rocm's. Only the entry points the row split uses.
struct Rccl {
    bool tried = false, ok = false;
    ncclResult_t (*get_unique_id)(ncclUniqueId *) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*all_gather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*all_reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                               hipStream_t) = nullptr;
    const char *(*error_string)(ncclResult_t) = nullptr;
};

Rccl &rccl() {
    static Rccl r;
    if (r.tried) return r;
    r.tried = true;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        fprintf(stderr, "ggml_mi355x: librccl.so.1 not found (%s)\n", dlerror());
        return r;
    }
    r.get_unique_id = (decltype(r.get_unique_id))dlsym(h, "ncclGetUniqueId");
    r.comm_init_rank = (decltype(r.comm_init_rank))dlsym(h, "ncclCommInitRank");
    r.comm_destroy = (decltype(r.comm_destroy))dlsym(h, "ncclCommDestroy");
    r.all_gather = (decltype(r.all_gather))dlsym(h, "ncclAllGather");
    r.all_reduce = (decltype(r.all_reduce))dlsym(h, "ncclAllReduce");
    r.error_string = (decltype(r.error_string))dlsym(h, "ncclGetErrorString");
    r.ok = r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.all_gather && r.all_reduce && r.error_string;
    return r;
}

constexpr size_t kMaxGraphs = 4;

void destroy_captured(mi355x_backend::Captured &c) {
    if (c.exec) hipGraphExecDestroy(c.exec);
    if (c.graph) hipGraphDestroy(c.graph);
    c.exec = nullptr;
    c.graph = nullptr;
}

void drop_graph(mi355x_backend *b) {
    for (auto &c : b->graphs) destroy_captured(c);
    b->graphs.clear();
}

// the captured graph of this node list (moved to the back: most recently used), or null
mi355x_backend::Captured *find_graph(mi355x_backend *b, const std::vector<uint64_t> &key) {
    for (size_t i = 0; i < b->graphs.size(); ++i)
        if (b->graphs[i].key == key) {
            if (i + 1 != b->graphs.size()) {
                mi355x_backend::Captured c = b->graphs[i];
                b->graphs.erase(b->graphs.begin() + (long)i);
                b->graphs.push_back(c);
            }
            return &b->graphs.back();
        }
    return nullptr;
}

const mi355x_backend::LyTab *find_ly_tab(const mi355x_backend *b, const std::vector<uint64_t> &key) {
    for (const auto &t : b->ly_tabs)
        if (t.dev && t.key == key) return &t;
    return nullptr;
}

// a persistent layer launch's counter block key (see ensure_layer_blocks)
std::vector<uint32_t> ly_block_key(const Launch &l) {
    std::vector<uint32_t> k = {(uint32_t)l.ly_block};
    for (int e = 0; e < 4; ++e)
        for (int q = 0; q < 8; ++q) k.push_back(l.la.expect[e][q]);
    return k;
}

int find_ly_block(const mi355x_backend *b, const std::vector<uint32_t> &k) {
    for (size_t i = 0; i < b->ly_keys.size(); ++i)
        if (b->ly_keys[i] == k) return (int)i;
    return -1;
}

kq::PlanOpts plan_opts(const mi355x_backend *b) {
    return {b->fuse, b->attn_oproj, b->layer_engine, b->workspace, b->workspace_size};
}

// What the workspace holds of an activation: the Q8L blocks (int8-MFMA GEMMs, kq_mmq) or
// the f16 image (kq_mmf) of tensor `src`'s M rows of K. q/k/v and gate/up of a prompt batch
// read one normed activation: the launches after the first run the GEMM alone.
struct Q8State {
    const void *src = nullptr;
    int64_t k = 0, m = 0;
    size_t nb = 0;
    bool f16 = false;  // the workspace holds kq_mmf's f16 activation image, not Q8L blocks

    bool holds(const mi355x_tensor *x, int64_t K, int64_t M, bool f) const {
        return src == x->data && k == K && m == M && nb == x->nb[1] && f16 == f;
    }
    void set(const mi355x_tensor *x, int64_t K, int64_t M, bool f) { src = x->data, k = K, m = M, nb = x->nb[1], f16 = f; }
    // an output (ncols columns, col_stride floats apart) overlapping the activation's bytes invalidates it
    void drop_if_overlaps(const float *y, int64_t col_stride, int64_t ncols) {
        const uintptr_t o0 = (uintptr_t)y, o1 = o0 + (size_t)col_stride * 4 * (size_t)ncols;
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + nb * (size_t)m;
        if (o0 < s1 && s0 < o1) *this = Q8State();
    }
};

// the workspace holds x's Q8L blocks (f16: its f16 image) after this: quantized / imaged unless it already does
int ensure_activation(mi355x_backend *b, const mi355x_tensor *x, int64_t K, int64_t M, bool f16, Q8State &q8) {
    if (q8.holds(x, K, M, f16)) return 0;
    q8 = Q8State();
    const float *xd = (const float *)x->data;
    const int64_t xs = (int64_t)(x->nb[1] / 4);
    const int rc = f16 ? kq::launch_f16img(xd, xs, (uint8_t *)b->workspace, K, M, b->stream)
                       : kq::launch_quantize_q8L(xd, xs, b->workspace, K, M, b->stream, true);
    if (!rc) q8.set(x, K, M, f16);
    return rc;
}

// A MUL_MAT of ne11 >= 16 columns on the shared-activation GEMMs: the exact int8 one, or the
// stated-tolerance f16 one where it applies (res: the ADD epilogue)
int enqueue_batched_mm(mi355x_backend *b, const mi355x_tensor *t, Q8State &q8, float *y = nullptr,
                       int64_t y_stride = 0, const float *res = nullptr, int64_t res_stride = 0) {
    const mi355x_tensor *w = t->src[0], *x = t->src[1];
    if (!y) {
        y = (float *)t->data;
        y_stride = (int64_t)(t->nb[1] / 4);
    }
    const int64_t K = w->ne[0], M = x->ne[1];
    const bool f16 = kq::mmf_applies(w->type, w->data, w->ne[1], w->nb[1], M, K);
    int rc = ensure_activation(b, x, K, M, f16, q8);
    if (rc) return rc;
    rc = f16 ? kq::launch_mmf_gemm(w->type, w->data, K, w->ne[1], w->nb[1], (uint8_t *)b->workspace, M, y, y_stride,
                                   b->stream, res, res_stride)
             : kq::launch_mmq(w->type, w->data, K, w->ne[1], w->nb[1], (const uint8_t *)b->workspace, M, y, y_stride,
                              b->stream, res, res_stride);
    if (rc)
        q8 = Q8State();
    else
        q8.drop_if_overlaps(y, y_stride, t->ne[1]);
    return rc;
}

// the (token, slot) pairs of a MUL_MAT_ID node: T * n_used of its MOE_ROUTE records
int64_t id_pairs(const mi355x_tensor *t) { return t->src[2]->ne[1] * (t->src[2]->ne[0] / 2); }

// A MUL_MAT_ID node, the expert ids read on the device at every replay. In the grouped form
// (kq::moe_grouped) the group table in b->mg is built by the first consumer of a MOE_ROUTE node
// (`table_of`: the node whose table b->mg holds) and read by the others, and up and gate, which
// share src1, quantize it once (q8).
int enqueue_mul_mat_id(mi355x_backend *b, const mi355x_tensor *t, Q8State &q8, const mi355x_tensor *&table_of) {
    const mi355x_tensor *w = t->src[0], *x = t->src[1], *rt = t->src[2];
    const int64_t K = w->ne[0], rows = x->ne[1] * x->ne[2];
    kq::MoeGrouped gr = {(int32_t *)b->mg, b->mg_size, (uint8_t *)b->workspace, b->workspace_size, true, true};
    const bool grouped = kq::moe_grouped(id_pairs(t));
    if (grouped) {
        // (ensure_workspace sized both for this node under the mode of this plan key)
        if (b->mg_size < kq::moe_table_bytes(id_pairs(t)) || b->workspace_size < kq::moe_q8_bytes(K, rows))
            return MI355X_E_WORKSPACE;
        gr.build = table_of != rt;
        gr.quantize = !q8.holds(x, K, rows, false);
    }
    if (!grouped || gr.quantize) q8 = Q8State();
    const int rc = kq::launch_mul_mat_id(w->type, w->data, K, w->ne[1], w->nb[1], w->nb[2], (int)w->ne[2],
                                         (const float *)x->data, x->ne[1], (int64_t)(x->nb[1] / 4),
                                         (const int32_t *)rt->data, (int64_t)(rt->nb[1] / 4), (int)(rt->ne[0] / 2),
                                         rt->ne[1], (float *)t->data, b->stream, &gr);
    if (rc || !grouped) {
        q8 = Q8State();
        return rc;
    }
    table_of = rt;
    q8.set(x, K, rows, false);
    q8.drop_if_overlaps((const float *)t->data, w->ne[1], id_pairs(t));
    return 0;
}

// The matrices of one multi-matrix tile-GEMM launch, in launch order
struct MatSet {
    const void *w[4];
    int types[4];
    int64_t N[4], y_col_stride[4];
    size_t row_stride[4];
    float *y[4];
    int n = 0;
    void add(const mi355x_tensor *mm) {
        w[n] = mm->src[0]->data;
        types[n] = mm->src[0]->type;
        N[n] = mm->src[0]->ne[1];
        row_stride[n] = mm->src[0]->nb[1];
        y[n] = (float *)mm->data;
        y_col_stride[n++] = (int64_t)(mm->nb[1] / 4);
    }
};

int rccl_failed(const char *what, ncclResult_t r) {
    fprintf(stderr, "ggml_mi355x: %s: %s\n", what, rccl().error_string(r));
    return MI355X_E_COMM;
}

int enqueue_node(mi355x_backend *b, const Launch &l, const mi355x_tensor *t) {
    hipStream_t st = b->stream;
    switch (t->op) {
        case MI355X_OP_NONE:
            return 0;
        case MI355X_OP_MUL_MAT: {
            const mi355x_tensor *w = t->src[0], *x = t->src[1];
            return mi355x_mul_mat(w->type, w->data, w->ne[0], w->ne[1], w->nb[1], (const float *)x->data, x->ne[1],
                                  x->nb[1], (float *)t->data, t->nb[1], b->workspace, b->workspace_size, st);
        }
        case MI355X_OP_GET_ROWS:
            return mi355x_get_rows(t->src[0]->type, t->src[0]->data, t->src[0]->ne[0], t->src[0]->nb[1],
                                   t->src[0]->ne[1], (const int32_t *)t->src[1]->data, t->src[1]->ne[0],
                                   (float *)t->data, st);
        case MI355X_OP_RMS_NORM:
            if (l.norm_w)
                return mi355x_rms_norm((const float *)t->src[0]->data, l.norm_w, l.norm_y, t->ne[0], nelem(t) / t->ne[0],
                                       f_of(t->op_params[0]), st);
            return mi355x_rms_norm((const float *)t->src[0]->data, nullptr, (float *)t->data, t->ne[0],
                                   nelem(t) / t->ne[0], f_of(t->op_params[0]), st);
        case MI355X_OP_MUL:
        case MI355X_OP_ADD:  // src1 of one row is repeated over src0's rows (ggml broadcast)
            if (!kq::device_ok()) return MI355X_E_NODEVICE;
            return kq::launch_binary(t->op == MI355X_OP_ADD ? 0 : 1, (const float *)t->src[0]->data,
                                 (const float *)t->src[1]->data, (float *)t->data, nelem(t), st, nelem(t->src[1]));
        case MI355X_OP_SWIGLU:
            return mi355x_swiglu((const float *)t->src[0]->data, (const float *)t->src[1]->data, (float *)t->data,
                                 nelem(t), st);
        case MI355X_OP_ROPE:
            return mi355x_rope((const float *)t->src[0]->data, (float *)t->data, (int)t->ne[0], t->op_params[0],
                               (int)(nelem(t) / t->ne[0]), (const int32_t *)t->src[1]->data,
                               (const float *)t->src[2]->data, (int)t->src[2]->ne[1], st);
        case MI355X_OP_ALL_GATHER: {
            if (!b->comm && b->loop_world > 0) {  // emulated rank: own slice into place, the rest untouched
                if (nelem(t) != nelem(t->src[0]) * b->loop_world) return MI355X_E_COMM;
                if (b->loop_nocopy) return 0;  // (timing of a rank's compute alone: tools/split_budget.py)
                const size_t n = (size_t)nelem(t->src[0]) * 4;
                const hipError_t e = hipMemcpyAsync((char *)t->data + (size_t)b->loop_rank * n, t->src[0]->data, n,
                                                    hipMemcpyDeviceToDevice, st);
                return e == hipSuccess ? 0 : (int)e;
            }
            if (!b->comm || nelem(t) != nelem(t->src[0]) * b->world) return MI355X_E_COMM;
            const ncclResult_t r = rccl().all_gather(t->src[0]->data, t->data, (size_t)nelem(t->src[0]), ncclFloat32,
                                                     b->comm, st);
            return r == ncclSuccess ? 0 : rccl_failed("ncclAllGather", r);
        }
        case MI355X_OP_ALL_REDUCE: {
            if (!b->comm && b->loop_world > 0) return 0;  // emulated rank: the caller's reduced vector stays
            if (!b->comm || nelem(t) != nelem(t->src[0])) return MI355X_E_COMM;
            const ncclResult_t r = rccl().all_reduce(t->src[0]->data, t->data, (size_t)nelem(t), ncclFloat32, ncclSum,
                                                     b->comm, st);
            return r == ncclSuccess ? 0 : rccl_failed("ncclAllReduce", r);
        }
        case MI355X_OP_ATTN_DECODE: {
            mi355x_attn_desc a;
            attn_desc_of(t, a);
            const int64_t n_tok = t->src[0]->ne[1];
            if (n_tok > 1) {  // a prompt batch: all cells first, then every query (causal)
                a.rope_row = 0;
                return mi355x_attn_prompt(&a, (int)n_tok, st);
            }
            a.rope_row = t->src[6]->ne[1] == 1 ? 1 : 0;  // the position's row, staged with pos
            return mi355x_attn_decode(&a, st);
        }
        case MI355X_OP_ARGMAX: {
            const int64_t n = t->src[0]->ne[0];
            if (t->op_params[0] == 0)
                return kq::launch_argmax((const float *)t->src[0]->data, n, (int32_t *)t->data, nullptr, b->am,
                                         b->am_size, st);
            const kq::ArgmaxStep step = token_step_of(t);
            return kq::launch_argmax((const float *)t->src[0]->data, n, (int32_t *)t->data, &step, b->am, b->am_size, st);
        }
        case MI355X_OP_ARGMAX_BATCH: {
            const mi355x_tensor *x = t->src[0];
            if (t->op_params[0] == 0)
                return kq::launch_argmax_rows((const float *)x->data, x->ne[0], x->ne[1], x->ne[0], (int32_t *)t->data,
                                              nullptr, b->am, b->am_size, st);
            const kq::ArgmaxRowsStep step = rows_step_of(t, 1);
            return kq::launch_argmax_rows((const float *)x->data, x->ne[0], x->ne[1], x->ne[0], (int32_t *)t->data, &step,
                                          b->am, b->am_size, st);
        }
        case MI355X_OP_SAMPLE: {
            mi355x_sampler sp;
            sampler_of(t, sp);
            const int64_t n = t->src[0]->ne[0];
            if (t->op_params[0] == 0)
                return kq::launch_topk((const float *)t->src[0]->data, n, 0, nullptr, nullptr, &sp,
                                       (const float *)t->src[1]->data, (int32_t *)t->data, nullptr, b->sm, b->sm_size, st);
            const kq::SampleStep step = {token_step_of(t), t->src[4]->ne[0]};
            return kq::launch_topk((const float *)t->src[0]->data, n, 0, nullptr, nullptr, &sp,
                                   (const float *)t->src[4]->data, (int32_t *)t->data, &step, b->sm, b->sm_size, st);
        }
        case MI355X_OP_SAMPLE_BATCH: {
            mi355x_sampler sp;
            sampler_of(t, sp);
            const mi355x_tensor *x = t->src[0];
            if (t->op_params[0] == 0)
                return kq::launch_topk_rows((const float *)x->data, x->ne[0], x->ne[1], x->ne[0], 0, nullptr, nullptr, &sp,
                                            (const float *)t->src[1]->data, (int32_t *)t->data, nullptr, b->sm, b->sm_size,
                                            st);
            const mi355x_tensor *draws = t->src[5];
            const kq::SampleRowsStep step = {rows_step_of(t, 5), (int64_t)(draws->nb[1] / 4), draws->ne[0]};
            return kq::launch_topk_rows((const float *)x->data, x->ne[0], x->ne[1], x->ne[0], 0, nullptr, nullptr, &sp,
                                        (const float *)draws->data, (int32_t *)t->data, &step, b->sm, b->sm_size, st);
        }
        case MI355X_OP_LOGPROB_BATCH: {  // two launches: kq_argmax_rows, kq_logsum_rows
            const mi355x_tensor *x = t->src[0];
            return kq::launch_logprob_rows((const float *)x->data, x->ne[0], x->ne[1], x->ne[0],
                                           (const int32_t *)t->src[1]->data, (mi355x_logprob *)t->data, b->am, b->am_size,
                                           st);
        }
        case MI355X_OP_PENALIZE: {  // in place on the logits; end, the history and the lists read on the device
            const mi355x_tensor *x = t->src[0], *hist = t->src[2];
            mi355x_penalties pen;
            const int n_bias = penalties_of(t, pen);
            const bool win = pen.last_n > 0;
            return kq::launch_penalize_rows((float *)x->data, x->ne[0], x->ne[1], x->ne[0], &pen,
                                            win ? (const int32_t *)hist->data : nullptr, win ? (int64_t)(hist->nb[1] / 4) : 0,
                                            win ? hist->ne[0] : 0, win ? (const int32_t *)t->src[1]->data : nullptr,
                                            n_bias ? (const int32_t *)t->src[3]->data : nullptr,
                                            n_bias ? (const float *)t->src[4]->data : nullptr, n_bias, st);
        }
        case MI355X_OP_KV_SHIFT: {  // in place on the caches; the deltas read on the device
            mi355x_kv_shift_desc d;
            kv_shift_desc_of(t, d);
            return kq::launch_kv_shift(&d, st);
        }
        case MI355X_OP_MOE_ROUTE: {  // the records the MUL_MAT_ID / MOE_COMBINE nodes read on the device
            const mi355x_tensor *gi = t->src[0], *x = t->src[1];
            return kq::launch_moe_route((const float *)gi->data, gi->ne[0], (int)gi->ne[1], (const float *)x->data,
                                        (int64_t)(x->nb[1] / 4), x->ne[1], t->op_params[0], (int32_t *)t->data,
                                        (int64_t)(t->nb[1] / 4), nullptr, st);
        }
        case MI355X_OP_MOE_COMBINE: {  // (MUL_MAT_ID: enqueue_mul_mat_id)
            const mi355x_tensor *ex = t->src[0], *rt = t->src[1];
            return kq::launch_moe_combine((const float *)ex->data, ex->ne[0], (int)(rt->ne[0] / 2), rt->ne[1],
                                          (const int32_t *)rt->data, (int64_t)(rt->nb[1] / 4), (float *)t->data, st);
        }
        case MI355X_OP_ATTN_BATCH: {  // store + attention, cells / mask / pos read on the device
            mi355x_attn_batch_desc d;
            attn_batch_desc_of(t, d);
            kq::AttnBatchArgs ba;
            const int rc = kq::attn_batch_args_from(&d, (int)t->src[6]->ne[1], ba);
            if (rc) return rc;
            if (!kq::device_ok()) return MI355X_E_NODEVICE;
            return kq::launch_attn_batch(ba, st);
        }
        default:
            return MI355X_E_UNSUPPORTED;
    }
}

int enqueue(mi355x_backend *b, mi355x_tensor *const *nodes, const std::vector<Launch> &launches) {
    Q8State q8;
    const mi355x_tensor *kv_done = nullptr;  // prompt ATTN whose KV cells a GEMM epilogue stored
    const mi355x_tensor *table_of = nullptr;  // the MOE_ROUTE node whose group table b->mg holds
    if (!kq::device_ok()) return MI355X_E_NODEVICE;
    const kq::PlanOpts po = plan_opts(b);
    for (size_t li = 0; li < launches.size(); ++li) {
        const Launch &l = launches[li];
        const mi355x_tensor *t = nodes[l.first];
        int rc;
        const bool q8_fuse = l.kind == LaunchKind::Node && t->op == MI355X_OP_ATTN_DECODE && li + 1 < launches.size() &&
                             kq::attn_feeds_batched_mm(po, t, launches[li + 1], nodes);
        if (q8_fuse || (l.kind == LaunchKind::Node && t == kv_done)) {
            // prompt attention: its KV cells already stored by the k/v GEMM's epilogue
            // (kv_done), and/or its output only read by the next launch's GEMM (the o-proj),
            // for which the group kernel also writes the Q8L blocks (no kq_quantize_q8L)
            mi355x_attn_desc d;
            attn_desc_of(t, d);
            d.rope_row = 0;
            kq::AttnArgs a;
            rc = kq::attn_args_from(&d, a);
            if (rc) return rc;
            a.no_store = t == kv_done;
            kv_done = nullptr;
            if (q8_fuse) a.q8_out = (uint8_t *)b->workspace;
            rc = kq::launch_attn_prompt(a, (int)t->src[0]->ne[1], b->stream);
            if (rc) return rc;
            q8 = Q8State();
            if (q8_fuse) q8.set(t, t->ne[0], t->ne[1], false);
            continue;
        }
        if (l.kind == LaunchKind::PrefillPrologue) {  // the activation's Q8L blocks for the MUL_MATs after it
            const mi355x_tensor *m = l.q8_of;
            const int64_t K = m->ne[0], M = m->ne[1];
            rc = l.pro == MI355X_PRO_RMS_NORM
                     ? kq::launch_rms_norm_q8L(l.x, l.x2, b->workspace, K, M, l.eps, b->stream)
                     : kq::launch_swiglu_q8L(l.x, l.x2, b->workspace, K, M, b->stream);
            if (rc) return rc;
            q8.set(m, K, M, false);  // int8 Q8L blocks now, whatever a preceding f16 GEMM left
            continue;
        }
        if (l.kind == LaunchKind::Layer) {  // a decode layer: one persistent launch
            kq::LayerArgs la = l.la;
            const int blk = find_ly_block(b, ly_block_key(l));
            if (!b->ly_sync || blk < 0 || blk >= b->ly_blocks) return MI355X_E_WORKSPACE;
            const mi355x_backend::LyTab *tb = find_ly_tab(b, ly_tab_key(la));
            if (!tb) return MI355X_E_WORKSPACE;
            la.tab = (const uint8_t *)tb->dev;
            la.tab_stride = tb->stride;
            la.sync = b->ly_sync + (size_t)blk * kq::LAYER_SYNC_U32;
            la.err = (int *)(b->ly_sync + (size_t)b->ly_blocks * kq::LAYER_SYNC_U32);
            rc = kq::launch_layer(la, b->stream);
            if (rc) return rc;
            q8 = Q8State();
            continue;
        }
        if (l.kind == LaunchKind::AttnOproj) {  // decode attention + o-proj (+ residual): one launch
            const mi355x_tensor *mm = nodes[l.first + 1];
            mi355x_attn_desc d;
            attn_desc_of(t, d);
            d.rope_row = t->src[6]->ne[1] == 1 ? 1 : 0;  // the position's row, staged with pos
            kq::AttnArgs a;
            rc = kq::attn_args_from(&d, a);
            if (rc) return rc;
            const mi355x_tensor *w = mm->src[0];
            rc = kq::launch_attn_oproj(a, w->type, w->data, w->ne[1], w->nb[1], l.res[0], l.y[0], (uint8_t *)b->fx,
                                       b->fx_size, b->stream);
            if (rc) return rc;
            q8 = Q8State();
            continue;
        }
        if (l.kind == LaunchKind::MmMulti) {  // several batched MUL_MATs on one activation: one tile-GEMM launch
            bool f16 = kq::mmf_on();  // the f16 GEMM where it is the faster kernel for every matrix
            for (int k = 0; f16 && k < l.count; ++k) {
                const mi355x_tensor *u = nodes[l.first + k]->src[0];
                f16 = kq::mmf_applies(u->type, u->data, u->ne[1], u->nb[1], nodes[l.first + k]->src[1]->ne[1], u->ne[0]);
            }
            const mi355x_tensor *x = t->src[1];
            const int64_t K = t->src[0]->ne[0], M = x->ne[1];
            rc = ensure_activation(b, x, K, M, f16, q8);
            if (rc) return rc;
            // the prompt attention right after, reading k and v of this group: its KV cells
            // stored by the int8 launch's epilogue (kq_kv_store's arithmetic), one launch fewer.
            // Then k and v go first: their row tiles (and the cache stores) start first.
            kq::MmqKv kv;
            const bool kv_fuse = !f16 && li + 1 < launches.size() && kq::kv_epilogue(nodes, l, launches[li + 1], kv);
            MatSet ms;
            int kinds[4] = {};
            for (const bool kv_pass : {true, false})  // k and v, then the rest (all of them without the epilogue)
                for (int k = 0; k < l.count; ++k)
                    if ((kv_fuse && kv.kind[k] != 0) == kv_pass) {
                        kinds[ms.n] = kv_pass ? kv.kind[k] : 0;
                        ms.add(nodes[l.first + k]);
                    }
            if (kv_fuse) memcpy(kv.kind, kinds, sizeof(kinds));
            rc = f16 ? kq::launch_mmf_multi(t->src[0]->type, ms.n, ms.w, ms.N, ms.row_stride, ms.y, ms.y_col_stride, K,
                                            (uint8_t *)b->workspace, b->workspace_size, M, b->stream)
                     : kq::launch_mmq_multi(ms.types, ms.n, ms.w, ms.N, ms.row_stride, ms.y, ms.y_col_stride, K,
                                            (const uint8_t *)b->workspace, M, b->stream, kv_fuse ? &kv : nullptr);
            if (rc) return rc;
            if (kv_fuse) kv_done = nodes[launches[li + 1].first];
            for (int k = 0; k < ms.n; ++k) q8.drop_if_overlaps(ms.y[k], ms.y_col_stride[k], M);
            continue;
        }
        if (l.kind == LaunchKind::MmAdd) {  // batched MUL_MAT with the residual ADD as its epilogue
            const mi355x_tensor *ad = nodes[l.first + 1], *other = kq::other_operand(ad, t);
            rc = enqueue_batched_mm(b, t, q8, l.y[0], (int64_t)(ad->nb[1] / 4), l.res[0], (int64_t)(other->nb[1] / 4));
            if (rc) return rc;
            continue;
        }
        if (l.kind != LaunchKind::GemvRun && l.count == 1 && kq::batched_mm_shares(po, t)) {
            rc = enqueue_batched_mm(b, t, q8);
            if (rc) return rc;
            continue;
        }
        if (l.kind == LaunchKind::Node && t->op == MI355X_OP_MUL_MAT_ID) {
            rc = enqueue_mul_mat_id(b, t, q8, table_of);
            if (rc) return rc;
            continue;
        }
        q8 = Q8State();  // any other launch may overwrite the workspace or the activation
        if (l.kind == LaunchKind::GemvRun) {
            const mi355x_tensor *w = t->src[0];
            mi355x_gemv_desc d[MI355X_MAX_FUSED];
            mi355x_gemv_ext ext;
            memset(&ext, 0, sizeof(ext));
            ext.prologue = l.pro;
            ext.x2 = l.x2;
            ext.eps = l.eps;
            for (int k = 0; k < l.count; ++k) {
                const mi355x_tensor *n = nodes[l.first + k];
                d[k].type = n->src[0]->type;
                d[k].w = n->src[0]->data;
                d[k].n_rows = n->src[0]->ne[1];
                d[k].row_stride = n->src[0]->nb[1];
                d[k].y = l.y[k];
                ext.residual[k] = l.res[k];
            }
            ext.epilogue = l.epi_y ? MI355X_EPI_SWIGLU : MI355X_EPI_NONE;
            ext.epi_y = l.epi_y;
            rc = mi355x_gemv_fused_ext(d, l.count, l.x, w->ne[0], &ext, b->workspace, b->workspace_size, b->stream);
        } else {
            rc = enqueue_node(b, l, t);
        }
        if (rc) return rc;
    }
    return 0;
}

// ---- graph_compute's steps, in its order. Each returns a status; what a step (re)allocates
// it allocates outside any capture, after waiting for the stream and dropping the captured
// graphs that may reference the old allocation.

// The device buffer *buf grown to `need` bytes (never shrunk), zeroed where `zero`: on the backend
// stream (non-blocking: a legacy-stream memset is not ordered before its next launch), then waited for.
int grow_buffer(mi355x_backend *b, void **buf, size_t *size, size_t need, bool zero) {
    if (need <= *size) return MI355X_OK;
    hipStreamSynchronize(b->stream);
    drop_graph(b);
    if (*buf) hipFree(*buf);
    *buf = nullptr;
    *size = 0;
    if (hipMalloc(buf, need) != hipSuccess) return MI355X_E_WORKSPACE;
    *size = need;
    if (zero && (hipMemsetAsync(*buf, 0, need, b->stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess))
        return MI355X_E_WORKSPACE;
    return MI355X_OK;
}

// every node supported; the workspace grown to the largest MUL_MAT's need, or the Q8L rows of the
// largest MUL_MAT_ID that takes the grouped form, whose group table gets a buffer of its own
int ensure_workspace(mi355x_backend *b, mi355x_tensor *const *nodes, int n_nodes) {
    size_t ws = 0, mg = 0;
    for (int i = 0; i < n_nodes; ++i) {
        if (!mi355x_backend_supports_op(nodes[i])) return MI355X_E_UNSUPPORTED;
        if (nodes[i]->op == MI355X_OP_MUL_MAT_ID && kq::moe_grouped(id_pairs(nodes[i]))) {
            const mi355x_tensor *x = nodes[i]->src[1];
            ws = std::max(ws, kq::moe_q8_bytes(x->ne[0], x->ne[1] * x->ne[2]));
            mg = std::max(mg, kq::moe_table_bytes(id_pairs(nodes[i])));
        }
        if (nodes[i]->op == MI355X_OP_MUL_MAT) {
            const mi355x_tensor *w = nodes[i]->src[0];
            size_t need = mi355x_mul_mat_workspace_size(w->type, w->ne[0], w->ne[1], nodes[i]->src[1]->ne[1]);
            const size_t nf = mi355x_gemv_ext_workspace_size(w->ne[0]);
            need = need > nf ? need : nf;
            if (nodes[i]->src[1]->ne[1] == 1 && ((uintptr_t)nodes[i]->src[1]->data & 15u))
                need = need > (size_t)(w->ne[0] / 256) * kq::Q8L_STRIDE ? need : (size_t)(w->ne[0] / 256) * kq::Q8L_STRIDE;
            ws = need > ws ? need : ws;
        }
    }
    const int rc = grow_buffer(b, &b->mg, &b->mg_size, mg, false);
    return rc ? rc : grow_buffer(b, &b->workspace, &b->workspace_size, ws, false);
}

// the fused attention + o-proj launches' buffer: sized, and its counters zeroed
int ensure_attn_oproj_buffer(mi355x_backend *b, mi355x_tensor *const *nodes, const std::vector<Launch> &launches) {
    size_t need = 0;
    int nsb = 0;
    bool mixed = false;
    for (const Launch &l : launches) {
        if (l.kind != LaunchKind::AttnOproj) continue;
        const mi355x_tensor *t = nodes[l.first], *w = nodes[l.first + 1]->src[0];
        int k = 0;
        const size_t sz = kq::attn_oproj_buffer(t->op_params[2], t->op_params[0], t->op_params[1],
                                                (int)t->src[4]->ne[1], w->type, w->ne[0], w->ne[1], &k);
        need = sz > need ? sz : need;
        mixed |= nsb && k != nsb;
        nsb = k;
    }
    if (mixed) return MI355X_E_UNSUPPORTED;  // (never built by plan_launches' callers: one o-proj shape per graph)
    if (!need || (need <= b->fx_size && nsb == b->fx_nsb)) return MI355X_OK;
    hipStreamSynchronize(b->stream);
    drop_graph(b);
    if (need > b->fx_size) {
        if (b->fx) hipFree(b->fx);
        b->fx = nullptr;
        b->fx_size = 0;
        if (hipMalloc(&b->fx, need) != hipSuccess) return MI355X_E_WORKSPACE;
        b->fx_size = need;
    }
    // on the backend stream (non-blocking: a legacy-stream memset is not ordered
    // before its next launch), then waited for
    if (hipMemsetAsync(b->fx, 0, kq::kAttnOprojCounterBytes, b->stream) != hipSuccess ||
        hipStreamSynchronize(b->stream) != hipSuccess)
        return MI355X_E_WORKSPACE;
    b->fx_nsb = nsb;
    return MI355X_OK;
}

// the ARGMAX, ARGMAX_BATCH and LOGPROB_BATCH nodes' counters and partials: sized for the largest, zeroed when
// (re)allocated.
// The nodes of a graph run one after the other on the backend stream, so they share it.
int ensure_argmax_buffer(mi355x_backend *b, mi355x_tensor *const *nodes, int n_nodes) {
    size_t need = 0;
    for (int i = 0; i < n_nodes; ++i)
        if (nodes[i]->op == MI355X_OP_ARGMAX) need = std::max(need, kq::argmax_workspace(nodes[i]->src[0]->ne[0]));
        else if (nodes[i]->op == MI355X_OP_ARGMAX_BATCH)
            need = std::max(need, kq::argmax_rows_workspace(nodes[i]->src[0]->ne[0], nodes[i]->src[0]->ne[1]));
        else if (nodes[i]->op == MI355X_OP_LOGPROB_BATCH)
            need = std::max(need, kq::logprob_workspace(nodes[i]->src[0]->ne[0], nodes[i]->src[0]->ne[1]));
    return grow_buffer(b, &b->am, &b->am_size, need, true);
}

// ... and the SAMPLE and SAMPLE_BATCH nodes', in a buffer of their own (b->am keeps its layout)
int ensure_sample_buffer(mi355x_backend *b, mi355x_tensor *const *nodes, int n_nodes) {
    size_t need = 0;
    for (int i = 0; i < n_nodes; ++i)
        if (nodes[i]->op == MI355X_OP_SAMPLE) need = std::max(need, kq::topk_workspace(nodes[i]->src[0]->ne[0], 1));
        else if (nodes[i]->op == MI355X_OP_SAMPLE_BATCH)
            need = std::max(need, kq::topk_workspace(nodes[i]->src[0]->ne[0], nodes[i]->src[0]->ne[1]));
    return grow_buffer(b, &b->sm, &b->sm_size, need, true);
}

// The persistent layers' counter blocks: one per Layer launch, zeroed whenever they are
// (re)allocated. A launch's counters are monotonic over its launches with ITS producer
// counts, so a block is keyed by (layer index in the graph, producers per edge and shard):
// graphs with other counts (another cache size or model on this backend) get blocks of
// their own instead of inheriting counters stepped by other counts.
int ensure_layer_blocks(mi355x_backend *b, const std::vector<Launch> &launches) {
    std::vector<std::vector<uint32_t>> fresh;
    for (const Launch &l : launches) {
        if (l.kind != LaunchKind::Layer) continue;
        const std::vector<uint32_t> k = ly_block_key(l);
        if (find_ly_block(b, k) < 0 && std::find(fresh.begin(), fresh.end(), k) == fresh.end()) fresh.push_back(k);
    }
    if (fresh.empty()) return MI355X_OK;
    const size_t need = b->ly_keys.size() + fresh.size();
    hipStreamSynchronize(b->stream);
    if ((int)need > b->ly_blocks) {  // grow (capacity doubles): every counter restarts at 0
        drop_graph(b);
        int cap = b->ly_blocks ? b->ly_blocks : 8;
        while (cap < (int)need) cap *= 2;
        if (b->ly_sync) hipFree(b->ly_sync);
        b->ly_sync = nullptr;
        b->ly_blocks = 0;
        const size_t bytes = ((size_t)cap * kq::LAYER_SYNC_U32 + 64) * 4;
        if (hipMalloc(&b->ly_sync, bytes) != hipSuccess) {
            b->ly_keys.clear();
            return MI355X_E_WORKSPACE;
        }
        b->ly_blocks = cap;
        if (hipMemsetAsync(b->ly_sync, 0, bytes, b->stream) != hipSuccess ||
            hipStreamSynchronize(b->stream) != hipSuccess)
            return MI355X_E_WORKSPACE;
    }
    // new blocks are still zero: blocks past ly_keys.size() were zeroed when allocated
    // and never launched on
    for (auto &k : fresh) b->ly_keys.push_back(std::move(k));
    return MI355X_OK;
}

// The persistent layers' step tables: built on the host once per full geometry (weights,
// shape, ring depth, attention placement, LDS layout) and kept; a table is never rebuilt in
// place, so a captured graph never reads a table that changed under it.
// The cache bound clears every table from inside the loop, also those this graph's earlier
// launches just found or built (enqueue then fails with E_WORKSPACE). Evicting without
// that is a change to this function alone, with a test of its own.
int ensure_layer_tables(mi355x_backend *b, const std::vector<Launch> &launches) {
    for (const Launch &l : launches) {
        if (l.kind != LaunchKind::Layer) continue;
        std::vector<uint64_t> key = ly_tab_key(l.la);
        if (find_ly_tab(b, key)) continue;
        if (b->ly_tabs.size() >= kMaxLyTabs) {  // bound the cache: start over (graphs may read them)
            hipStreamSynchronize(b->stream);
            drop_graph(b);
            for (auto &t : b->ly_tabs)
                if (t.dev) hipFree(t.dev);
            b->ly_tabs.clear();
        }
        const int64_t stride = kq::layer_table_stride(l.la);
        if (stride <= 0) return MI355X_E_UNSUPPORTED;
        std::vector<uint8_t> host((size_t)(stride * l.la.G));
        kq::layer_table_fill(l.la, host.data(), stride);
        mi355x_backend::LyTab tb;
        if (hipMalloc(&tb.dev, host.size()) != hipSuccess) return MI355X_E_WORKSPACE;
        if (hipMemcpy(tb.dev, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(tb.dev);
            return MI355X_E_WORKSPACE;
        }
        tb.stride = stride;
        tb.key.swap(key);
        b->ly_tabs.push_back(std::move(tb));
    }
    return MI355X_OK;
}

// long-cache attention: the score workspace of a decode node (the split over cells, the
// streamed kernels), of a prompt node and of an ATTN_BATCH node that take the streamed kernels
int reserve_attn_cells(mi355x_backend *b, mi355x_tensor *const *nodes, const std::vector<Launch> &launches) {
    for (const Launch &l : launches) {
        const mi355x_tensor *t = nodes[l.first];
        if (l.kind == LaunchKind::Node && t->op == MI355X_OP_ATTN_BATCH) {
            mi355x_attn_batch_desc d;
            attn_batch_desc_of(t, d);
            kq::AttnBatchArgs ba;
            if (kq::attn_batch_args_from(&d, (int)t->src[6]->ne[1], ba) == MI355X_OK &&
                kq::attn_batch_form(ba) == MI355X_ATTN_PATH_STREAM && !kq::attn_batch_stream_buffer(ba, b->stream))
                return MI355X_E_WORKSPACE;
            continue;
        }
        if (l.kind != LaunchKind::Node || t->op != MI355X_OP_ATTN_DECODE) continue;
        const int64_t T = t->src[0]->ne[1];
        mi355x_attn_desc d = {};
        attn_desc_of(t, d);
        if (T > 1) d.rope_row = 0;
        kq::AttnArgs a = {};
        if (kq::attn_args_from(&d, a) == MI355X_OK && kq::attn_cells_reserve(a, b->stream, (int)T) != MI355X_OK)
            return MI355X_E_WORKSPACE;
    }
    return MI355X_OK;
}

// the plan captured into a hipGraph under the node list's key (unless cached), then launched
int capture_and_launch(mi355x_backend *b, mi355x_tensor *const *nodes, int n_nodes, const std::vector<Launch> &launches) {
    std::vector<uint64_t> key = kq::graph_key_of(nodes, n_nodes);
    mi355x_backend::Captured *c = find_graph(b, key);
    if (!c) {
        if (hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return MI355X_E_UNSUPPORTED;
        const int rc = enqueue(b, nodes, launches);
        hipGraph_t g = nullptr;
        const hipError_t ec = hipStreamEndCapture(b->stream, &g);
        if (rc || ec != hipSuccess) {
            if (g) hipGraphDestroy(g);
            return rc ? rc : (int)ec;
        }
        hipGraphExec_t ge = nullptr;
        if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) {
            hipGraphDestroy(g);
            return MI355X_E_UNSUPPORTED;
        }
        if (b->graphs.size() == kMaxGraphs) {  // the least recently used goes
            hipStreamSynchronize(b->stream);
            destroy_captured(b->graphs.front());
            b->graphs.erase(b->graphs.begin());
        }
        mi355x_backend::Captured nc;
        nc.key.swap(key);
        nc.graph = g;
        nc.exec = ge;
        b->graphs.push_back(nc);
        c = &b->graphs.back();
    }
    const hipError_t e = hipGraphLaunch(c->exec, b->stream);
    return e == hipSuccess ? 0 : (int)e;
}

// the setters of a planning option: a captured graph holds the old plan. Returns the previous value.
int toggle(mi355x_backend *b, bool &field, int enable) {
    DeviceGuard dg(b->device);
    const int prev = field ? 1 : 0;
    if ((enable != 0) != field) {
        hipStreamSynchronize(b->stream);
        drop_graph(b);
        field = enable != 0;
    }
    return prev;
}

}  // namespace

extern "C" {

int mi355x_device_count(void) {
    int ndev = 0, n = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    for (int d = 0; d < ndev; ++d) {
        DeviceGuard dg(d);
        n += kq::device_ok() ? 1 : 0;  // gfx950 with the library's code object
    }
    return n;
}

int mi355x_device_ordinal(int i) {
    int ndev = 0;
    if (i < 0 || hipGetDeviceCount(&ndev) != hipSuccess) return -1;
    for (int d = 0; d < ndev; ++d) {
        bool ok;
        {
            DeviceGuard dg(d);
            ok = kq::device_ok() != 0;
        }
        if (ok && i-- == 0) return d;
    }
    return -1;
}

int mi355x_device_memory(int device, size_t *free_bytes, size_t *total_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return MI355X_E_NODEVICE;
    DeviceGuard dg(device);
    size_t f = 0, t = 0;
    const hipError_t e = hipMemGetInfo(&f, &t);
    if (e != hipSuccess) return (int)e;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return MI355X_OK;
}

mi355x_backend_t mi355x_backend_init(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    DeviceGuard dg(device);
    if (!kq::device_ok()) return nullptr;
    mi355x_backend *b = new mi355x_backend();
    b->device = device;
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
        delete b;
        return nullptr;
    }
    b->name = "MI355X" + std::to_string(device);
    return b;
}

void mi355x_backend_free(mi355x_backend_t b) {
    if (!b) return;
    {
    DeviceGuard dg(b->device);
    hipStreamSynchronize(b->stream);
    drop_graph(b);
    if (b->workspace) hipFree(b->workspace);
    if (b->fx) hipFree(b->fx);
    if (b->am) hipFree(b->am);
    if (b->sm) hipFree(b->sm);
    if (b->mg) hipFree(b->mg);
    if (b->ly_sync) hipFree(b->ly_sync);
    for (auto &t : b->ly_tabs)
        if (t.dev) hipFree(t.dev);
    if (b->comm) rccl().comm_destroy(b->comm);
    hipStreamDestroy(b->stream);
    }
    delete b;
}

const char *mi355x_backend_name(mi355x_backend_t b) { return b ? b->name.c_str() : "MI355X"; }

void *mi355x_backend_stream(mi355x_backend_t b) { return b ? (void *)b->stream : nullptr; }

void *mi355x_backend_alloc(mi355x_backend_t b, size_t size) {
    if (!b) return nullptr;
    DeviceGuard dg(b->device);
    void *p = nullptr;
    if (hipMalloc(&p, size ? size : 1) != hipSuccess) return nullptr;
    return p;
}

void mi355x_backend_free_buffer(mi355x_backend_t b, void *ptr) {
    if (!b || !ptr) return;
    DeviceGuard dg(b->device);
    hipStreamSynchronize(b->stream);
    drop_graph(b);  // a captured graph may reference the buffer
    hipFree(ptr);
}

int mi355x_backend_memset(mi355x_backend_t b, void *dst, int value, size_t size) {
    if (!b || (!dst && size)) return MI355X_E_INVAL;
    if (!size) return MI355X_OK;
    DeviceGuard dg(b->device);
    const hipError_t e = hipMemsetAsync(dst, value & 0xff, size, b->stream);
    return e == hipSuccess ? MI355X_OK : (int)e;
}

int mi355x_backend_set_tensor(mi355x_backend_t b, void *dst, const void *host_src, size_t size) {
    if (!b || (!dst && size)) return MI355X_E_INVAL;
    DeviceGuard dg(b->device);
    // (hipStreamWriteValue32 per word for tiny inputs was measured 10 us/token slower
    // than this one copy of inp_tokens + inp_pos)
    const hipError_t e = hipMemcpyAsync(dst, host_src, size, hipMemcpyHostToDevice, b->stream);
    return e == hipSuccess ? 0 : (int)e;
}

int mi355x_backend_get_tensor(mi355x_backend_t b, void *host_dst, const void *src, size_t size) {
    if (!b || (!src && size)) return MI355X_E_INVAL;
    DeviceGuard dg(b->device);
    const hipError_t e = hipMemcpyAsync(host_dst, src, size, hipMemcpyDeviceToHost, b->stream);
    return e == hipSuccess ? 0 : (int)e;
}

int mi355x_backend_synchronize(mi355x_backend_t b) {
    if (!b) return MI355X_E_INVAL;
    DeviceGuard dg(b->device);
    const hipError_t e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return (int)e;
    // a persistent-layer launch that gave up waiting left invalid outputs: report it here,
    // where every caller that reads results already stops (and re-arm the counters)
    if (b->layer_engine && b->ly_sync) {
        const int le = mi355x_backend_layer_error(b);
        if (le) return le > 0 ? MI355X_E_LAYER : le;
    }
    return 0;
}

int mi355x_backend_supports_op(const mi355x_tensor *op) { return kq::supports_op(op) ? 1 : 0; }

size_t mi355x_comm_id_size(void) { return sizeof(ncclUniqueId); }

int mi355x_comm_get_unique_id(void *id_out) {
    if (!id_out) return MI355X_E_INVAL;
    Rccl &r = rccl();
    if (!r.ok) return MI355X_E_COMM;
    ncclUniqueId id;
    const ncclResult_t e = r.get_unique_id(&id);
    if (e != ncclSuccess) return rccl_failed("ncclGetUniqueId", e);
    memcpy(id_out, &id, sizeof(id));
    return MI355X_OK;
}

int mi355x_backend_set_comm(mi355x_backend_t b, int rank, int world, const void *unique_id) {
    if (!b || world < 1 || rank < 0 || rank >= world || !unique_id) return MI355X_E_INVAL;
    Rccl &r = rccl();
    if (!r.ok) return MI355X_E_COMM;
    DeviceGuard dg(b->device);
    hipStreamSynchronize(b->stream);
    drop_graph(b);  // a captured graph holds the old communicator's collectives
    if (b->comm) {
        r.comm_destroy(b->comm);
        b->comm = nullptr;
        b->world = 0;
    }
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    ncclComm_t c = nullptr;
    const ncclResult_t e = r.comm_init_rank(&c, world, id, rank);
    if (e != ncclSuccess)
        return rccl_failed(("ncclCommInitRank(rank " + std::to_string(rank) + " of " + std::to_string(world) + ")").c_str(), e);
    b->comm = c;
    b->rank = rank;
    b->world = world;
    return MI355X_OK;
}

int mi355x_backend_comm_world(mi355x_backend_t b) {
    return b && b->comm ? b->world : (b && b->loop_world ? b->loop_world : 0);
}

int mi355x_backend_set_comm_loopback(mi355x_backend_t b, int rank, int world) {
    if (!b || world < 0 || (world > 0 && (rank < 0 || rank >= world))) return MI355X_E_INVAL;
    DeviceGuard dg(b->device);
    hipStreamSynchronize(b->stream);
    drop_graph(b);
    b->loop_rank = world > 0 ? rank : -1;
    b->loop_world = world;
    // timing only: emulated ALL_GATHERs skip their own-slice copy, so a token's time is the
    // rank's compute alone (the gathered vectors are then stale: never for parity runs)
    b->loop_nocopy = kq::knob(kq::KNOB_LOOPBACK_NOCOPY) != 0;  // mi355x_debug_knob("LOOPBACK_NOCOPY")
    return MI355X_OK;
}

int mi355x_backend_set_attn_oproj(mi355x_backend_t b, int enable) {
    return b ? toggle(b, b->attn_oproj, enable) : MI355X_E_INVAL;
}

int mi355x_backend_set_layer_engine(mi355x_backend_t b, int enable) {
    return b ? toggle(b, b->layer_engine, enable) : MI355X_E_INVAL;
}

int mi355x_backend_layer_error(mi355x_backend_t b) {
    if (!b) return MI355X_E_INVAL;
    if (!b->ly_sync) return 0;
    DeviceGuard dg(b->device);
    if (hipStreamSynchronize(b->stream) != hipSuccess) return MI355X_E_NODEVICE;
    int err = 0;
    const size_t words = (size_t)b->ly_blocks * kq::LAYER_SYNC_U32 + 64;
    if (hipMemcpy(&err, b->ly_sync + (size_t)b->ly_blocks * kq::LAYER_SYNC_U32, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return MI355X_E_NODEVICE;
    if (err) {  // the counters of an abandoned launch are out of step: start every block again
        if (hipMemsetAsync(b->ly_sync, 0, words * 4, b->stream) != hipSuccess ||
            hipStreamSynchronize(b->stream) != hipSuccess)
            return MI355X_E_NODEVICE;
    }
    return err ? 1 : 0;
}

int mi355x_backend_set_fusion(mi355x_backend_t b, int enable) {
    return b ? toggle(b, b->fuse, enable) : MI355X_E_INVAL;
}

int mi355x_backend_graph_compute(mi355x_backend_t b, mi355x_tensor *const *nodes, int n_nodes, int use_graph) {
    if (!b || (n_nodes > 0 && !nodes) || n_nodes < 0) return MI355X_E_INVAL;
    DeviceGuard dg(b->device);
    // replay fast path: the node list of the captured graph (every decode step after
    // the first) was validated, planned and captured under this key already
    if (use_graph && !b->graphs.empty()) {
        const std::vector<uint64_t> key = kq::graph_key_of(nodes, n_nodes);
        if (mi355x_backend::Captured *c = find_graph(b, key)) {
            const hipError_t e = hipGraphLaunch(c->exec, b->stream);
            return e == hipSuccess ? 0 : (int)e;
        }
    }
    int rc = ensure_workspace(b, nodes, n_nodes);
    if (rc) return rc;
    const std::vector<Launch> launches = kq::plan_launches(plan_opts(b), nodes, n_nodes);
    if ((rc = ensure_attn_oproj_buffer(b, nodes, launches))) return rc;
    if ((rc = ensure_argmax_buffer(b, nodes, n_nodes))) return rc;
    if ((rc = ensure_sample_buffer(b, nodes, n_nodes))) return rc;
    if ((rc = ensure_layer_blocks(b, launches))) return rc;
    if ((rc = ensure_layer_tables(b, launches))) return rc;
    if ((rc = reserve_attn_cells(b, nodes, launches))) return rc;
    return use_graph ? capture_and_launch(b, nodes, n_nodes, launches) : enqueue(b, nodes, launches);
}

}  // extern "C"
