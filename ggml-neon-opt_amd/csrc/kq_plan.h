// kq_plan.h — the backend's fusion planner (kq_plan.hip): which nodes of a graph run as
// one launch. The only interface between the planner and the executor (kq_backend.hip);
// the planner sees the graph and a PlanOpts, never the backend. Not part of the public ABI.
#pragma once

#include <string.h>

#include <vector>

#include "kq_common.h"
#include "kq_internal.h"

namespace kq {

enum class LaunchKind {
    Node,             // any single node (RMS_NORM with its MUL fused: norm_w)
    GemvRun,          // a run of ne11 == 1 MUL_MATs sharing src1, with its fused neighbours
    PrefillPrologue,  // norm / swiglu of a prompt batch -> the Q8L blocks of the MUL_MATs after it
    MmAdd,            // batched MUL_MAT + ADD
    MmMulti,          // batched MUL_MATs on one activation in one tile-GEMM launch
    AttnOproj,        // decode ATTN_DECODE -> MUL_MAT (-> ADD) in one launch (kq_attn_oproj)
    Layer,            // a whole decode layer (15 nodes) in one persistent launch (kq_layer)
};

struct Launch {
    int first, count;  // nodes[first .. first+count): the MUL_MAT run, or the single node
    LaunchKind kind = LaunchKind::Node;
    const mi355x_tensor *q8_of = nullptr;  // PrefillPrologue: the node whose (never written) output the Q8L blocks stand for
    int pro = MI355X_PRO_NONE;
    const float *x = nullptr, *x2 = nullptr;  // GEMV input (prologue source) and its second operand
    float eps = 0.f;
    float *y[MI355X_MAX_FUSED] = {};
    const float *res[MI355X_MAX_FUSED] = {};
    const float *norm_w = nullptr;  // single RMS_NORM with its MUL fused
    float *norm_y = nullptr;
    float *epi_y = nullptr;  // GEMV run [gate, up] with the SWIGLU node fused as its epilogue
    int ly_block = -1;       // Layer: its counter block
    LayerArgs la;            // Layer: the launch's arguments (sync / err set at enqueue)
};

struct PlanOpts {
    bool fuse, attn_oproj, layer_engine;  // mi355x_backend_set_fusion / _attn_oproj / _layer_engine
    const void *workspace;                // the shared-activation GEMMs need it aligned and large enough
    size_t workspace_size;
};

inline int64_t nelem(const mi355x_tensor *t) { return t->ne[0] * t->ne[1] * t->ne[2] * t->ne[3]; }
inline float f_of(int32_t bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
// the ADD's other source when one of them is node `mm`, else null
inline const mi355x_tensor *other_operand(const mi355x_tensor *add, const mi355x_tensor *mm) {
    return add->src[0] == mm ? add->src[1] : add->src[1] == mm ? add->src[0] : nullptr;
}

std::vector<Launch> plan_launches(const PlanOpts &o, mi355x_tensor *const *nodes, int n);
// A batched MUL_MAT (ne11 >= 16) on the tile GEMMs, its activation shared through the workspace
bool batched_mm_shares(const PlanOpts &o, const mi355x_tensor *t);
bool attn_feeds_batched_mm(const PlanOpts &o, const mi355x_tensor *t, const Launch &next, mi355x_tensor *const *nodes);
bool kv_epilogue(mi355x_tensor *const *nodes, const Launch &l, const Launch &next, MmqKv &kv);
void attn_desc_of(const mi355x_tensor *t, mi355x_attn_desc &a);  // rope_row left to the caller
void attn_batch_desc_of(const mi355x_tensor *t, mi355x_attn_batch_desc &d);
void sampler_of(const mi355x_tensor *t, mi355x_sampler &s);  // SAMPLE / SAMPLE_BATCH: op_params[1 .. 4]
int penalties_of(const mi355x_tensor *t, mi355x_penalties &p);  // PENALIZE: op_params[0 .. 3]; returns n_bias ([4])
void kv_shift_desc_of(const mi355x_tensor *t, mi355x_kv_shift_desc &d);  // KV_SHIFT: its sources and op_params
// the step-inputs forms' operands: ARGMAX / SAMPLE (pos, rope table, history: src1 .. 3), and
// ARGMAX_BATCH / SAMPLE_BATCH (pos, cells, mask, history: src1 .. 4; cell_stride and n_kv at
// op_params[first_param], [first_param + 1])
ArgmaxStep token_step_of(const mi355x_tensor *t);
ArgmaxRowsStep rows_step_of(const mi355x_tensor *t, int first_param);
std::vector<uint64_t> graph_key_of(mi355x_tensor *const *nodes, int n_nodes);
bool supports_op(const mi355x_tensor *op);  // mi355x_backend_supports_op

}  // namespace kq
