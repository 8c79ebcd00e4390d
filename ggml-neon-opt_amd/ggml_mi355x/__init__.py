"""ggml_mi355x — Python host mirror of the ggml K-quant MUL_MAT operator surface,
bound to libggml_mi355x.so (HIP, gfx950) through its C-ABI (include/ggml_mi355x.h).

The names follow ggml: ``vec_dot_q4_K_q8_K`` (ggml_vec_dot_t, README.md:449),
``quantize_row_q8_K`` (from_float of Q8_K), ``mul_mat`` (ggml_compute_forward_mul_mat,
ggml-cpu.c:1389) and a ``Backend`` mirroring ggml-backend's device interface
(graph_compute, ggml-cpu.cpp:186). PyTorch is only plumbing here: device
buffers and the current HIP stream handle. There is no CPU fallback: if the
shared library or a gfx950 device is missing, every compute call raises.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("MI355X_LIB") or os.path.join(PKG_ROOT, "lib", "libggml_mi355x.so")

TYPE_F32, TYPE_F16, TYPE_Q4_K, TYPE_Q5_K, TYPE_Q6_K, TYPE_Q8_K, TYPE_I32 = 0, 1, 12, 13, 14, 15, 26
TYPE_I64 = 27  # cell indices of attn_batch / OP_ATTN_BATCH
QK_K = 256
BLOCK_BYTES = {TYPE_Q4_K: 144, TYPE_Q5_K: 176, TYPE_Q6_K: 210, TYPE_Q8_K: 292}
TYPE_NAMES = {TYPE_Q4_K: "q4_K", TYPE_Q5_K: "q5_K", TYPE_Q6_K: "q6_K", TYPE_Q8_K: "q8_K", TYPE_F32: "f32"}
MAX_FUSED = 4
OP_NONE, OP_MUL_MAT, OP_GET_ROWS, OP_RMS_NORM, OP_MUL, OP_ADD, OP_SWIGLU, OP_ROPE, OP_ATTN_DECODE, OP_ALL_GATHER, \
    OP_ALL_REDUCE = range(11)
OP_ATTN_BATCH = 11
OP_ARGMAX = 12  # op_params[0]: ARGMAX_PLAIN / ARGMAX_STEP_INPUTS
ARGMAX_PLAIN, ARGMAX_STEP_INPUTS = 0, 1
OP_ARGMAX_BATCH = 13  # the argmax of every row; op_params[0]: ARGMAX_PLAIN / ARGMAX_STEP_INPUTS
# op_params = [SAMPLE_PLAIN / SAMPLE_STEP_INPUTS, top_k, f32_bits(temp), f32_bits(top_p), f32_bits(min_p)]
# (sampler_params); the batch op appends cell_stride, n_kv
OP_SAMPLE, OP_SAMPLE_BATCH = 14, 15
SAMPLE_PLAIN, SAMPLE_STEP_INPUTS = 0, 1
SAMPLE_MAX_K = 64
OP_LOGPROB_BATCH = 16  # src0 the logits [n, T], src1 I32 targets [T] -> I32 [6, T]: the rows' records (LOGPROB_DTYPE)
LOGPROB_MAX_N = 262144
# in place on src0, the logits [n, T]; src1 I32 end [T], src2 I32 history [n_hist, T], src3 / src4 the bias lists
# [n_bias]; op_params: penalize_params(...)
OP_PENALIZE = 17
PENALTY_MAX_LAST_N, LOGIT_BIAS_MAX = 1024, 256
# in place on src0, the K cache F16 [kvw, n_ctx]; src1 the V cache F16 [n_ctx, kvw] (DISCARD), src2 the rope table
# [head_dim, n_pos], src3 I32 deltas [n_cells] (DELTAS); op_params: kv_shift_params(...)
OP_KV_SHIFT = 18
KV_SHIFT_DELTAS, KV_SHIFT_DISCARD = 0, 1
# the MoE FFN: MOE_ROUTE src0 gate_inp f32 [n_embd, n_expert], src1 x [n_embd, T], op_params [n_used] -> the records
# I32 [2 * n_used, T] (ids, then the weights' bits); MUL_MAT_ID src0 the experts [K, N, n_expert], src1 f32
# [K, 1 or n_used, T], src2 the MOE_ROUTE node -> f32 [N, n_used, T]; MOE_COMBINE src0 f32 [n, n_used, T], src1 the
# MOE_ROUTE node -> f32 [n, T]
OP_MOE_ROUTE, OP_MUL_MAT_ID, OP_MOE_COMBINE = 19, 20, 21
MOE_MAX_EXPERTS, MOE_MAX_USED, MUL_MAT_ID_MAX_K = 64, 8, 16384
MAX_SRC = 10
FLAG_OUTPUT = 1
E_OK, E_INVAL, E_UNSUPPORTED, E_WORKSPACE, E_NODEVICE, E_COMM, E_LAYER = 0, -1, -2, -3, -4, -6, -7
PRO_NONE, PRO_RMS_NORM, PRO_SWIGLU = 0, 1, 2
EPI_NONE, EPI_SWIGLU = 0, 1
ATTN_GROUP, ATTN_HEAD, ATTN_SPLIT = 0, 1, 2
# mi355x_attn_path: the decode attention kernel a descriptor takes
ATTN_PATH_HEAD, ATTN_PATH_HEAD_BATCH, ATTN_PATH_SPLIT4, ATTN_PATH_SPLIT8, ATTN_PATH_CELLS, ATTN_PATH_GROUP, _ = range(7)  # (6: retired)
ATTN_PATH_STREAM = 7  # the streamed kernels (attn_stream)
MMQ_AUTO, MMQ_TILE64, MMQ_TILE128, MMQ_TILE128W, MMQ_TILE64W, MMQ_TILE192 = 0, 1, 2, 3, 4, 6
PREFILL_EXACT, PREFILL_F16, PREFILL_F16_ALL = 0, 1, 2
ATTN_PROMPT_EXACT, ATTN_PROMPT_F16 = 0, 1  # attn_prompt_precision
MOE_PREFILL_AUTO, MOE_PREFILL_GEMV, MOE_PREFILL_GROUPED = 0, 1, 2  # moe_prefill

# Every symbol include/ggml_mi355x.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "mi355x_row_size", "mi355x_version", "mi355x_device_available",
    "mi355x_quantize_row_q8_K", "mi355x_vec_dot_q4_K_q8_K", "mi355x_vec_dot_q5_K_q8_K",
    "mi355x_vec_dot_q6_K_q8_K", "mi355x_quantize_q8_K", "mi355x_mul_mat_workspace_size",
    "mi355x_mul_mat", "mi355x_mul_mat_q8", "mi355x_gemv_fused", "mi355x_debug_block_partials", "mi355x_debug_stream",
    "mi355x_backend_init", "mi355x_backend_free", "mi355x_backend_name", "mi355x_backend_stream",
    "mi355x_backend_alloc", "mi355x_backend_free_buffer", "mi355x_backend_set_tensor",
    "mi355x_backend_get_tensor", "mi355x_backend_synchronize", "mi355x_backend_supports_op",
    "mi355x_backend_graph_compute", "mi355x_timing_enable", "mi355x_timing_read", "mi355x_diag_stamps",
    "mi355x_gemv_fused_workspace_size", "mi355x_gemv_impl",
    "mi355x_gguf_open", "mi355x_gguf_close", "mi355x_gguf_version", "mi355x_gguf_alignment",
    "mi355x_gguf_data_offset", "mi355x_gguf_n_tensors", "mi355x_gguf_find_tensor", "mi355x_gguf_get_tensor",
    "mi355x_gguf_tensor_data", "mi355x_gguf_upload", "mi355x_gguf_n_kv", "mi355x_gguf_find_key",
    "mi355x_gguf_key", "mi355x_gguf_kv_type", "mi355x_gguf_get_int", "mi355x_gguf_get_float",
    "mi355x_gguf_get_str", "mi355x_gguf_arr_n",
    "mi355x_gemv_ext_workspace_size", "mi355x_gemv_fused_ext", "mi355x_backend_set_fusion",
    "mi355x_get_rows", "mi355x_rms_norm", "mi355x_add", "mi355x_mul", "mi355x_swiglu",
    "mi355x_rope_table_size", "mi355x_rope_table", "mi355x_rope", "mi355x_attn_decode", "mi355x_attn_path",
    "mi355x_comm_id_size", "mi355x_comm_get_unique_id", "mi355x_backend_set_comm", "mi355x_backend_comm_world",
    "mi355x_backend_set_comm_loopback", "mi355x_lower_ggml_graph", "mi355x_attn_impl",
    "mi355x_mmq_impl",
    "mi355x_prefill_precision",
    "mi355x_gemv_waves",
    "mi355x_debug_knob",
    "mi355x_device_count", "mi355x_device_ordinal", "mi355x_device_memory", "mi355x_backend_memset", "mi355x_backend_set_attn_oproj",
    "mi355x_backend_set_layer_engine", "mi355x_backend_layer_error",
    "mi355x_attn_prompt",
    "mi355x_attn_prompt_impl", "mi355x_attn_stream", "mi355x_attn_prompt_precision",
    "mi355x_attn_batch", "mi355x_attn_batch_path",
    "mi355x_rows_prologue_plan", "mi355x_rows_stream_plan", "mi355x_debug_rows_prologue",
    "mi355x_debug_rows_plan",
    "mi355x_argmax_plan", "mi355x_argmax_workspace_size", "mi355x_argmax",
    "mi355x_argmax_rows_workspace_size", "mi355x_argmax_rows",
    "mi355x_topk_workspace_size", "mi355x_topk", "mi355x_topk_rows", "mi355x_sample", "mi355x_sample_rows",
    "mi355x_logprob_workspace_size", "mi355x_logprob_rows",
    "mi355x_penalize_rows",
    "mi355x_kv_shift",
    "mi355x_moe_route", "mi355x_mul_mat_id_workspace_size", "mi355x_mul_mat_id", "mi355x_moe_combine",
    "mi355x_moe_prefill",
)


class Mi355xError(RuntimeError):
    pass


class SamplerDesc(ctypes.Structure):
    """struct mi355x_sampler"""
    _fields_ = [("top_k", ctypes.c_int32), ("temp", ctypes.c_float), ("top_p", ctypes.c_float),
                ("min_p", ctypes.c_float)]


class PenaltiesDesc(ctypes.Structure):
    """struct mi355x_penalties"""
    _fields_ = [("last_n", ctypes.c_int32), ("repeat", ctypes.c_float), ("freq", ctypes.c_float),
                ("present", ctypes.c_float)]


class KvShiftDesc(ctypes.Structure):
    """mi355x_kv_shift_desc"""
    _fields_ = [("k_cache", ctypes.c_void_p), ("v_cache", ctypes.c_void_p), ("rope_table", ctypes.c_void_p),
                ("delta", ctypes.c_void_p), ("n_ctx", ctypes.c_int), ("n_head_kv", ctypes.c_int),
                ("head_dim", ctypes.c_int), ("n_pos", ctypes.c_int), ("form", ctypes.c_int), ("n_cells", ctypes.c_int),
                ("keep", ctypes.c_int), ("discard", ctypes.c_int), ("n_past", ctypes.c_int)]


class GemvDesc(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("w", ctypes.c_void_p), ("n_rows", ctypes.c_int64),
                ("row_stride", ctypes.c_size_t), ("y", ctypes.c_void_p)]


class LaunchTiming(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_char * 96), ("bytes", ctypes.c_double), ("ms", ctypes.c_float)]


class Tensor(ctypes.Structure):
    pass


Tensor._fields_ = [("type", ctypes.c_int), ("op", ctypes.c_int), ("ne", ctypes.c_int64 * 4),
                   ("nb", ctypes.c_size_t * 4), ("src", ctypes.POINTER(Tensor) * MAX_SRC), ("data", ctypes.c_void_p),
                   ("op_params", ctypes.c_int32 * 8), ("flags", ctypes.c_int32)]


class GTensor(ctypes.Structure):
    """mi355x_gtensor: the ggml_tensor-shaped mirror the lowering reads."""
    pass


GTensor._fields_ = [("type", ctypes.c_int), ("op", ctypes.c_int), ("ne", ctypes.c_int64 * 4),
                    ("nb", ctypes.c_size_t * 4), ("op_params", ctypes.c_int32 * 16), ("flags", ctypes.c_int32),
                    ("src", ctypes.POINTER(GTensor) * 10), ("view_src", ctypes.POINTER(GTensor)),
                    ("view_offs", ctypes.c_size_t), ("data", ctypes.c_void_p), ("name", ctypes.c_char * 64)]


class LowerOpts(ctypes.Structure):
    _fields_ = [("rope_table", ctypes.c_void_p), ("rope_n_pos", ctypes.c_int), ("rope_freq_base", ctypes.c_float),
                ("rope_freq_scale", ctypes.c_float), ("cells_eq_pos", ctypes.c_int),
                ("cells_from_graph", ctypes.c_int)]


(GOP_NONE, GOP_GET_ROWS, GOP_RMS_NORM, GOP_MUL, GOP_ADD, GOP_MUL_MAT, GOP_ROPE, GOP_SET_ROWS, GOP_SOFT_MAX, GOP_GLU,
 GOP_RESHAPE, GOP_VIEW, GOP_PERMUTE, GOP_TRANSPOSE, GOP_CONT, GOP_CPY) = range(16)
GLU_SWIGLU = 2


class AttnDesc(ctypes.Structure):
    _fields_ = [("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("pos", ctypes.c_void_p),
                ("rope_table", ctypes.c_void_p), ("k_cache", ctypes.c_void_p), ("v_cache", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("n_ctx", ctypes.c_int), ("n_head", ctypes.c_int),
                ("n_head_kv", ctypes.c_int), ("head_dim", ctypes.c_int), ("scale", ctypes.c_float),
                ("rope_row", ctypes.c_int)]


class AttnBatchDesc(ctypes.Structure):
    """mi355x_attn_batch_desc"""
    _fields_ = [("a", AttnDesc), ("cells", ctypes.c_void_p), ("cells_type", ctypes.c_int), ("mask", ctypes.c_void_p),
                ("mask_type", ctypes.c_int), ("mask_row_bytes", ctypes.c_size_t), ("n_kv", ctypes.c_int),
                ("n_tokens", ctypes.c_int)]


class GemvExt(ctypes.Structure):
    _fields_ = [("prologue", ctypes.c_int), ("x2", ctypes.c_void_p), ("eps", ctypes.c_float),
                ("residual", ctypes.c_void_p * MAX_FUSED), ("epilogue", ctypes.c_int), ("epi_y", ctypes.c_void_p)]

_lib = None


def lib():
    """Load libggml_mi355x.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Mi355xError(f"{LIB_PATH} missing: run __graft_entry__.build() (make -C ggml-neon-opt_amd)")
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, i64, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int
    L.mi355x_row_size.argtypes = [i32, i64]
    L.mi355x_row_size.restype = sz
    L.mi355x_version.restype = ctypes.c_char_p
    L.mi355x_device_available.restype = i32
    L.mi355x_device_count.restype = i32
    L.mi355x_device_ordinal.restype = i32
    L.mi355x_device_ordinal.argtypes = [i32]
    L.mi355x_device_memory.argtypes = [i32, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.mi355x_device_memory.restype = i32
    L.mi355x_backend_memset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, i32, ctypes.c_size_t]
    L.mi355x_backend_memset.restype = i32
    L.mi355x_backend_set_attn_oproj.argtypes = [ctypes.c_void_p, i32]
    L.mi355x_backend_set_attn_oproj.restype = i32
    L.mi355x_backend_set_layer_engine.argtypes = [ctypes.c_void_p, i32]
    L.mi355x_backend_set_layer_engine.restype = i32
    L.mi355x_backend_layer_error.argtypes = [ctypes.c_void_p]
    L.mi355x_backend_layer_error.restype = i32
    L.mi355x_quantize_row_q8_K.argtypes = [vp, vp, i64]
    for n in ("q4_K", "q5_K", "q6_K"):
        getattr(L, f"mi355x_vec_dot_{n}_q8_K").argtypes = [i32, vp, sz, vp, sz, vp, sz, i32]
    L.mi355x_quantize_q8_K.argtypes = [vp, sz, vp, i64, i64, vp]
    L.mi355x_quantize_q8_K.restype = i32
    L.mi355x_mul_mat_workspace_size.argtypes = [i32, i64, i64, i64]
    L.mi355x_mul_mat_workspace_size.restype = sz
    L.mi355x_mul_mat.argtypes = [i32, vp, i64, i64, sz, vp, i64, sz, vp, sz, vp, sz, vp]
    L.mi355x_mul_mat.restype = i32
    L.mi355x_mul_mat_q8.argtypes = [i32, vp, i64, i64, sz, vp, i64, sz, vp, sz, vp]
    L.mi355x_mul_mat_q8.restype = i32
    L.mi355x_gemv_fused.argtypes = [ctypes.POINTER(GemvDesc), i32, vp, i64, vp, sz, vp]
    L.mi355x_gemv_fused_workspace_size.argtypes = [i64]
    L.mi355x_gemv_fused_workspace_size.restype = sz
    L.mi355x_gemv_fused.restype = i32
    L.mi355x_debug_block_partials.argtypes = [i32, vp, i64, i64, sz, vp, vp, vp]
    L.mi355x_debug_block_partials.restype = i32
    L.mi355x_debug_stream.argtypes = [vp, sz, vp, vp]
    L.mi355x_debug_stream.restype = i32
    L.mi355x_rows_prologue_plan.argtypes = [i64, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.mi355x_rows_prologue_plan.restype = i32
    if hasattr(L, "mi355x_rows_stream_plan"):  # (an older library under MI355X_LIB, A/B runs: without it)
        L.mi355x_rows_stream_plan.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i64), i32, i64, i32,
                                              ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.mi355x_rows_stream_plan.restype = i32
    if hasattr(L, "mi355x_debug_rows_plan"):
        L.mi355x_debug_rows_plan.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i64), i32, i64, i32, i32,
                                             ctypes.POINTER(i64), i32]
        L.mi355x_debug_rows_plan.restype = i32
    L.mi355x_debug_rows_prologue.argtypes = [i32, vp, vp, ctypes.c_float, i64, i32, vp, sz, vp]
    L.mi355x_debug_rows_prologue.restype = i32
    L.mi355x_backend_init.argtypes = [i32]
    L.mi355x_backend_init.restype = vp
    L.mi355x_backend_free.argtypes = [vp]
    L.mi355x_backend_name.argtypes = [vp]
    L.mi355x_backend_name.restype = ctypes.c_char_p
    L.mi355x_backend_stream.argtypes = [vp]
    L.mi355x_backend_stream.restype = vp
    L.mi355x_backend_alloc.argtypes = [vp, sz]
    L.mi355x_backend_alloc.restype = vp
    L.mi355x_backend_free_buffer.argtypes = [vp, vp]
    L.mi355x_backend_set_tensor.argtypes = [vp, vp, vp, sz]
    L.mi355x_backend_set_tensor.restype = i32
    L.mi355x_backend_get_tensor.argtypes = [vp, vp, vp, sz]
    L.mi355x_backend_get_tensor.restype = i32
    L.mi355x_backend_synchronize.argtypes = [vp]
    L.mi355x_backend_synchronize.restype = i32
    L.mi355x_backend_supports_op.argtypes = [ctypes.POINTER(Tensor)]
    L.mi355x_backend_supports_op.restype = i32
    L.mi355x_backend_graph_compute.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Tensor)), i32, i32]
    L.mi355x_backend_graph_compute.restype = i32
    L.mi355x_timing_enable.argtypes = [i32]
    L.mi355x_timing_enable.restype = i32
    L.mi355x_timing_read.argtypes = [ctypes.POINTER(LaunchTiming), i32]
    L.mi355x_timing_read.restype = i32
    L.mi355x_gemv_impl.argtypes = [i32]
    L.mi355x_gemv_impl.restype = i32
    L.mi355x_diag_stamps.argtypes = [vp, sz]
    L.mi355x_diag_stamps.restype = i32
    f32 = ctypes.c_float
    L.mi355x_gemv_ext_workspace_size.argtypes = [i64]
    L.mi355x_gemv_ext_workspace_size.restype = sz
    L.mi355x_gemv_fused_ext.argtypes = [ctypes.POINTER(GemvDesc), i32, vp, i64, ctypes.POINTER(GemvExt), vp, sz, vp]
    L.mi355x_gemv_fused_ext.restype = i32
    L.mi355x_backend_set_fusion.argtypes = [vp, i32]
    L.mi355x_backend_set_fusion.restype = i32
    L.mi355x_get_rows.argtypes = [i32, vp, i64, sz, i64, vp, i64, vp, vp]
    L.mi355x_rms_norm.argtypes = [vp, vp, vp, i64, i64, f32, vp]
    L.mi355x_add.argtypes = [vp, vp, vp, i64, vp]
    L.mi355x_mul.argtypes = [vp, vp, vp, i64, vp]
    L.mi355x_swiglu.argtypes = [vp, vp, vp, i64, vp]
    L.mi355x_rope_table_size.argtypes = [i32, i32]
    L.mi355x_rope_table_size.restype = sz
    L.mi355x_rope_table.argtypes = [vp, i32, i32, f32, f32, vp]
    L.mi355x_rope.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, vp]
    L.mi355x_attn_decode.argtypes = [ctypes.POINTER(AttnDesc), vp]
    L.mi355x_attn_path.argtypes = [ctypes.POINTER(AttnDesc)]
    L.mi355x_attn_path.restype = i32
    L.mi355x_attn_prompt.argtypes = [ctypes.POINTER(AttnDesc), i32, vp]
    L.mi355x_attn_batch.argtypes = [ctypes.POINTER(AttnBatchDesc), vp]
    L.mi355x_attn_batch.restype = i32
    L.mi355x_attn_batch_path.argtypes = [ctypes.POINTER(AttnBatchDesc)]
    L.mi355x_attn_batch_path.restype = i32
    if hasattr(L, "mi355x_argmax"):  # (an older library under MI355X_LIB, A/B runs: without it)
        L.mi355x_argmax_plan.argtypes = [i64, ctypes.POINTER(i32), ctypes.POINTER(i64)]
        L.mi355x_argmax_plan.restype = i32
        L.mi355x_argmax_workspace_size.argtypes = [i64]
        L.mi355x_argmax_workspace_size.restype = sz
        L.mi355x_argmax.argtypes = [vp, i64, vp, vp, sz, vp]
        L.mi355x_argmax.restype = i32
    if hasattr(L, "mi355x_argmax_rows"):
        L.mi355x_argmax_rows_workspace_size.argtypes = [i64, i64]
        L.mi355x_argmax_rows_workspace_size.restype = sz
        L.mi355x_argmax_rows.argtypes = [vp, i64, i64, i64, vp, vp, sz, vp]
        L.mi355x_argmax_rows.restype = i32
    if hasattr(L, "mi355x_topk"):
        L.mi355x_topk_workspace_size.argtypes = [i64, i64]
        L.mi355x_topk_workspace_size.restype = sz
        L.mi355x_topk.argtypes = [vp, i64, i32, vp, vp, vp, sz, vp]
        L.mi355x_topk.restype = i32
        L.mi355x_topk_rows.argtypes = [vp, i64, i64, i64, i32, vp, vp, vp, sz, vp]
        L.mi355x_topk_rows.restype = i32
        L.mi355x_sample.argtypes = [vp, i64, ctypes.POINTER(SamplerDesc), vp, vp, vp, sz, vp]
        L.mi355x_sample.restype = i32
        L.mi355x_sample_rows.argtypes = [vp, i64, i64, i64, ctypes.POINTER(SamplerDesc), vp, vp, vp, sz, vp]
        L.mi355x_sample_rows.restype = i32
    if hasattr(L, "mi355x_logprob_rows"):
        L.mi355x_logprob_workspace_size.argtypes = [i64, i64]
        L.mi355x_logprob_workspace_size.restype = sz
        L.mi355x_logprob_rows.argtypes = [vp, i64, i64, i64, vp, vp, vp, sz, vp]
        L.mi355x_logprob_rows.restype = i32
    if hasattr(L, "mi355x_penalize_rows"):
        L.mi355x_penalize_rows.argtypes = [vp, i64, i64, i64, ctypes.POINTER(PenaltiesDesc), vp, i64, i64, vp, vp, vp, i32,
                                           vp]
        L.mi355x_penalize_rows.restype = i32
    if hasattr(L, "mi355x_kv_shift"):
        L.mi355x_kv_shift.argtypes = [ctypes.POINTER(KvShiftDesc), vp]
        L.mi355x_kv_shift.restype = i32
    if hasattr(L, "mi355x_mul_mat_id"):
        L.mi355x_moe_route.argtypes = [vp, i64, i32, vp, i64, i64, i32, vp, i64, vp, vp]
        L.mi355x_moe_route.restype = i32
        L.mi355x_mul_mat_id_workspace_size.argtypes = [i32, i64, i32, i64]
        L.mi355x_mul_mat_id_workspace_size.restype = sz
        L.mi355x_mul_mat_id.argtypes = [i32, vp, i64, i64, sz, sz, i32, vp, i64, i64, vp, i64, i32, i64, vp, vp, sz, vp]
        L.mi355x_mul_mat_id.restype = i32
        L.mi355x_moe_combine.argtypes = [vp, i64, i32, i64, vp, i64, vp, vp]
        L.mi355x_moe_combine.restype = i32
    if hasattr(L, "mi355x_moe_prefill"):
        L.mi355x_moe_prefill.argtypes = [i32]
        L.mi355x_moe_prefill.restype = i32
    L.mi355x_attn_prompt_impl.argtypes = [i32]
    L.mi355x_attn_prompt_impl.restype = i32
    if hasattr(L, "mi355x_attn_prompt_precision"):  # (an older library under MI355X_LIB, A/B runs: without it)
        L.mi355x_attn_prompt_precision.argtypes = [i32]
        L.mi355x_attn_prompt_precision.restype = i32
    L.mi355x_attn_impl.argtypes = [i32]
    L.mi355x_attn_impl.restype = i32
    L.mi355x_attn_stream.argtypes = [i32]
    L.mi355x_attn_stream.restype = i32
    L.mi355x_mmq_impl.argtypes = [i32]
    L.mi355x_mmq_impl.restype = i32
    L.mi355x_prefill_precision.argtypes = [i32]
    L.mi355x_prefill_precision.restype = i32
    L.mi355x_gemv_waves.argtypes = [i32]
    L.mi355x_gemv_waves.restype = i32
    L.mi355x_debug_knob.argtypes = [ctypes.c_char_p, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
    L.mi355x_debug_knob.restype = i32
    for n in ("mi355x_get_rows", "mi355x_rms_norm", "mi355x_add", "mi355x_mul", "mi355x_swiglu",
              "mi355x_rope_table", "mi355x_rope", "mi355x_attn_decode", "mi355x_attn_prompt"):
        getattr(L, n).restype = i32
    L.mi355x_lower_ggml_graph.argtypes = [ctypes.POINTER(ctypes.POINTER(GTensor)), i32, ctypes.POINTER(LowerOpts),
                                          ctypes.POINTER(Tensor), i32, ctypes.POINTER(ctypes.POINTER(Tensor)), i32,
                                          ctypes.POINTER(i32)]
    L.mi355x_lower_ggml_graph.restype = i32
    L.mi355x_comm_id_size.argtypes = []
    L.mi355x_comm_id_size.restype = sz
    L.mi355x_comm_get_unique_id.argtypes = [vp]
    L.mi355x_comm_get_unique_id.restype = i32
    L.mi355x_backend_set_comm.argtypes = [vp, i32, i32, vp]
    L.mi355x_backend_set_comm.restype = i32
    L.mi355x_backend_comm_world.argtypes = [vp]
    L.mi355x_backend_comm_world.restype = i32
    L.mi355x_backend_set_comm_loopback.argtypes = [vp, i32, i32]
    L.mi355x_backend_set_comm_loopback.restype = i32
    from . import gguf as _gguf
    _gguf.bind(L)
    _lib = L
    return L


GEMV_AUTO, GEMV_TASKS, GEMV_ROWS, GEMV_DYN = 0, 1, 2, 3


def gemv_impl(impl):
    """Select the decode GEMV kernel (GEMV_AUTO / GEMV_ROWS: row-stream kq_rows, one
    launch per stage, the claimed-row kq_rows_dyn where enough rows per wave; GEMV_TASKS:
    kq_gemv; GEMV_DYN: kq_rows_dyn for every one-type launch). Returns the previous selection."""
    prev = lib().mi355x_gemv_impl(impl)
    if prev < 0:
        raise Mi355xError(f"mi355x_gemv_impl failed with status {prev}")
    return prev


def timing_enable(enable=True):
    """Start (and clear) or stop per-launch kernel timing (hipExtLaunchKernelGGL events)."""
    lib().mi355x_timing_enable(1 if enable else 0)


def timing_read():
    """Synchronize the device; return [(kernel_name, algorithmic_bytes, ms), ...]."""
    n = lib().mi355x_timing_read(None, 0)
    if n < 0:
        raise Mi355xError(f"mi355x_timing_read failed ({n})")
    buf = (LaunchTiming * max(n, 1))()
    n = lib().mi355x_timing_read(buf, n)
    return [(buf[i].kernel.decode(), buf[i].bytes, buf[i].ms) for i in range(n)]


def version() -> str:
    return lib().mi355x_version().decode()


def device_available() -> bool:
    return bool(lib().mi355x_device_available())


def row_size(type_: int, k: int) -> int:
    return int(lib().mi355x_row_size(type_, k))


def _check(rc: int, what: str):
    if rc == E_LAYER:
        raise Mi355xError(f"{what}: a persistent-layer launch lost co-residency; that step's outputs "
                          "are invalid (counters re-armed)")
    if rc != 0:
        raise Mi355xError(f"{what} failed with status {rc}")


def _require_device():
    if not device_available():
        raise Mi355xError("no gfx950 device visible: the HIP path cannot run (there is no CPU fallback)")


def _stream(stream):
    if stream is not None:
        return ctypes.c_void_p(stream)
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------- tensor helpers
def _torch():
    import torch
    return torch


def quantize_q8_K(x, out=None, stream=None):
    """x: (M, K) float32 cuda tensor -> (M, K/256*292) uint8 cuda tensor (Q8_K rows)."""
    torch = _torch()
    _require_device()
    if x.dim() == 1:
        x = x[None]
    assert x.dtype == torch.float32 and x.is_cuda and x.stride(1) == 1
    M, K = x.shape
    if out is None:
        out = torch.empty((M, K // QK_K * 292), dtype=torch.uint8, device=x.device)
    _check(lib().mi355x_quantize_q8_K(x.data_ptr(), x.stride(0) * 4, out.data_ptr(), K, M, _stream(stream)),
           "mi355x_quantize_q8_K")
    return out


def mul_mat(type_, w, K, x, out=None, workspace=None, stream=None):
    """dst (M, N) = mul_mat(w (N rows of `type_`), x (M, K) f32), ggml semantics."""
    torch = _torch()
    _require_device()
    if x.dim() == 1:
        x = x[None]
    M = x.shape[0]
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws = int(lib().mi355x_mul_mat_workspace_size(type_, K, N, M))
    if M == 1 and x.data_ptr() % 16:
        ws = max(ws, K // QK_K * 304)  # Q8L activation blocks (kq_rows)
    if ws and (workspace is None or workspace.numel() < ws):
        workspace = _workspace(ws, x.device, stream)
    _check(lib().mi355x_mul_mat(type_, w.data_ptr(), K, N, w.stride(0), x.data_ptr(), M, x.stride(0) * 4,
                                out.data_ptr(), out.stride(0) * 4,
                                workspace.data_ptr() if ws else None, ws, _stream(stream)), "mi355x_mul_mat")
    return out


def mul_mat_q8(type_, w, K, q8, out=None, stream=None):
    torch = _torch()
    _require_device()
    if q8.dim() == 1:
        q8 = q8[None]
    M = q8.shape[0]
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=q8.device)
    _check(lib().mi355x_mul_mat_q8(type_, w.data_ptr(), K, N, w.stride(0), q8.data_ptr(), M, q8.stride(0),
                                   out.data_ptr(), out.stride(0) * 4, _stream(stream)), "mi355x_mul_mat_q8")
    return out


_ws_cache = {}


def _workspace(nbytes, device, stream=None):
    """Scratch for the quantized activation, one per (device, stream): launches on one
    stream are ordered, those on different streams (other threads) may overlap."""
    torch = _torch()
    key = (str(device), _stream(stream).value or 0)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def gemv_fused(mats, x, stream=None, workspace=None):
    """mats: list of (type, w tensor (N, rowbytes), y tensor (N,) f32); x: (K,) f32. One launch
    (two when K > 8192: Q8_K quantization into a workspace first)."""
    _require_device()
    n = len(mats)
    descs = (GemvDesc * n)()
    for i, (t, w, y) in enumerate(mats):
        descs[i] = GemvDesc(t, w.data_ptr(), w.shape[0], w.stride(0), y.data_ptr())
    K = x.shape[-1]
    need = int(lib().mi355x_gemv_fused_workspace_size(K))
    if need and (workspace is None or workspace.numel() < need):
        workspace = _workspace(need, x.device, stream)
    _check(lib().mi355x_gemv_fused(descs, n, x.data_ptr(), K, workspace.data_ptr() if need else None, need,
                                   _stream(stream)), "mi355x_gemv_fused")


def mmq_impl(impl):
    """Prefill GEMM variant (MMQ_*); returns the previous."""
    return int(lib().mi355x_mmq_impl(impl))


def prefill_precision(p=-1):
    """Prefill (M >= 16) precision: PREFILL_EXACT (bit-exact kq_mmq), PREFILL_F16 (stated
    tolerance: kq_mmf where it is faster) or PREFILL_F16_ALL (kq_mmf on every shape); -1
    queries. Returns the previous value."""
    return int(lib().mi355x_prefill_precision(p))


def gemv_waves(waves):
    """kq_rows waves per workgroup: 0 = by launch size, else fixed (1..12); returns the previous."""
    return int(lib().mi355x_gemv_waves(waves))


def rows_prologue_plan(k, waves, steps=0):
    """(lanes per superblock, passes) of the fused GEMV prologue for a k-element row on a
    workgroup of `waves` waves whose longest wave streams `steps` 16-superblock steps
    (mi355x_rows_prologue_plan: the host's choice, no device), or the error code
    (E_UNSUPPORTED: the row does not fit that many waves)."""
    lanes, passes = ctypes.c_int(0), ctypes.c_int(0)
    rc = int(lib().mi355x_rows_prologue_plan(k, waves, steps, ctypes.byref(lanes), ctypes.byref(passes)))
    return (lanes.value, passes.value) if rc == 0 else rc


ROWS_LONG, ROWS_SHORT, ROWS_CLAIMED = 0, 1, 2


def rows_stream_plan(mats, k, batch_rows=0):
    """(steps, depth, form) of one decode GEMV launch of `mats` = [(type, n_rows), ...] over
    k-element rows (mi355x_rows_stream_plan: the host's choice, no device): the most
    16-superblock steps a wave streams and the ring depth of its type, for the matrix with the
    least room in its ring, and ROWS_SHORT / ROWS_LONG / ROWS_CLAIMED; or the error code."""
    n = len(mats)
    types = (ctypes.c_int32 * n)(*[int(t) for t, _ in mats])
    rows = (ctypes.c_int64 * n)(*[int(r) for _, r in mats])
    steps, depth, form = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = int(lib().mi355x_rows_stream_plan(types, rows, n, k, batch_rows, ctypes.byref(steps), ctypes.byref(depth),
                                           ctypes.byref(form)))
    return (steps.value, depth.value, form.value) if rc == 0 else rc


ROWS_PLAN_FIELDS = ("tmask", "nwv", "grid_x", "lds", "lsh", "sh", "dyn", "steps", "depth", "waves_total",
                    *(f"wave_prefix{i}" for i in range(MAX_FUSED + 1)), *(f"rbase{i}" for i in range(MAX_FUSED)),
                    *(f"rrem{i}" for i in range(MAX_FUSED)), "rpw", "bR", "prio_bytes", "pre0", "dyn_u", "dyn_ush",
                    "dyn_p", "kernel")


def rows_plan(mats, k, fusedq=True, prologue=0):
    """The whole host plan of one decode GEMV launch of `mats` = [(type, n_rows), ...] over
    k-element rows (mi355x_debug_rows_plan: no launch, no device): a dict keyed by
    ROWS_PLAN_FIELDS (`kernel`: the selected instantiation, see the header); or the error code."""
    n = len(mats)
    types = (ctypes.c_int32 * n)(*[int(t) for t, _ in mats])
    rows = (ctypes.c_int64 * n)(*[int(r) for _, r in mats])
    out = (ctypes.c_int64 * len(ROWS_PLAN_FIELDS))()
    rc = int(lib().mi355x_debug_rows_plan(types, rows, n, k, int(bool(fusedq)), prologue, out, len(out)))
    if rc < 0:
        return rc
    assert rc == len(ROWS_PLAN_FIELDS), rc
    return dict(zip(ROWS_PLAN_FIELDS, (int(v) for v in out)))


def debug_rows_prologue(x, waves, prologue=PRO_NONE, x2=None, eps=0.0, stream=None):
    """The fused GEMV prologue alone on one workgroup of `waves` waves
    (mi355x_debug_rows_prologue): the Q8L image of x after `prologue`, a uint8 tensor
    [K / 256, 304] (d f32 @0, 256 int8 @16, 16 int16 bsums @272)."""
    _require_device()
    torch = _torch()
    K = x.shape[-1]
    out = torch.empty((K // QK_K, 304), dtype=torch.uint8, device=x.device)
    _check(lib().mi355x_debug_rows_prologue(prologue, x.data_ptr(), x2.data_ptr() if x2 is not None else None, eps, K,
                                            waves, out.data_ptr(), out.numel(), _stream(stream)),
           "mi355x_debug_rows_prologue")
    return out


DEBUG_KNOBS = ("GEMV_DIAG", "GEMV_RING", "GEMV_PRE0", "GEMV_SMALL_MB", "GEMV_WPC",
               "GEMV_SMALL_WG", "GEMV_FQMAX", "MMF_WAVES", "MMF_ORDER", "ATTN_DIAG", "LOOPBACK_NOCOPY",
               "ATTN_OPROJ", "AO_NRB", "GEMV_DYN", "GEMV_DYN_P", "GEMV_DYN_STEPS", "GEMV_SHORT", "ATTN_STREAM",
               "ATTN_STREAM_TILE", "ARGMAX_SLICE", "MMQ_ID_Q6")


def debug_knob(name, value=float("nan")):
    """Experiment knob of A/B runs (mi355x_debug_knob; the library reads no environment):
    set `name` to `value` (NaN: back to the product default). Returns the previous value."""
    prev = ctypes.c_double(0.0)
    rc = lib().mi355x_debug_knob(name.encode(), float(value), ctypes.byref(prev))
    if rc != 0:
        raise Mi355xError(f"debug_knob: unknown knob {name!r}")
    return prev.value


def attn_prompt_impl(impl):
    """Prompt attention, and attn_batch / OP_ATTN_BATCH: ATTN_GROUP (per kv group and token where it
    fits, default) / ATTN_HEAD (per query head and token); returns the previous."""
    return int(lib().mi355x_attn_prompt_impl(impl))


def attn_prompt_precision(p=-1):
    """Prompt attention precision (mi355x_attn_prompt_precision): ATTN_PROMPT_EXACT (default: the
    decode token's bits) / ATTN_PROMPT_F16 (kq_attn_prompt_f16 on the f16 matrix cores, within the
    bound include/ggml_mi355x.h states; attn_prompt and the graph backend's prompt nodes follow it,
    decode and attn_batch stay exact). -1 queries. Returns the previous value, E_INVAL otherwise."""
    return int(lib().mi355x_attn_prompt_precision(p))


def attn_impl(impl):
    """ATTN_SPLIT (default: per query head, split by output past 256 cache cells) / ATTN_HEAD
    (per query head) / ATTN_GROUP (per kv group); returns the previous."""
    return int(lib().mi355x_attn_impl(impl))


def attn_stream(mode):
    """Streamed attention for caches of up to 131072 cells (mi355x_attn_stream): 0 off (default),
    1 for the descriptors refused for their cache size alone, 2 for every valid descriptor (tests,
    A/B). attn_path / attn_decode / attn_prompt, attn_batch / attn_batch_path and the graph backend
    (OP_ATTN_BATCH included) follow it. Returns the previous mode, E_INVAL for any other value."""
    return int(lib().mi355x_attn_stream(mode))


def moe_prefill(impl):
    """Which form mul_mat_id and the backend's MUL_MAT_ID nodes take (mi355x_moe_prefill): MOE_PREFILL_AUTO
    (default: the expert-grouped int8-MFMA tiles, kq_moe_group + kq_mmq_id, from 32 (token, slot) pairs,
    kq_gemv_id below), MOE_PREFILL_GEMV (always kq_gemv_id) or MOE_PREFILL_GROUPED (grouped for any T >= 1);
    the same bits either way. Part of the backend's plan key. Returns the previous value, E_INVAL for any other."""
    return int(_lib_with("mi355x_moe_prefill").mi355x_moe_prefill(impl))


def gemv_fused_ext(mats, x, prologue=PRO_NONE, x2=None, eps=0.0, residual=None, epi_y=None, stream=None):
    """gemv_fused with the decode graph's neighbours fused (mi355x_gemv_fused_ext):
    prologue PRO_RMS_NORM (x2 = norm weight) / PRO_SWIGLU (x = gate, x2 = up),
    y_i = mul_mat_i + residual[i], and with epi_y (mats = [gate, up]) the SWIGLU
    epilogue epi_y = swiglu(y_0, y_1)."""
    _require_device()
    n = len(mats)
    descs = (GemvDesc * n)()
    for i, (t, w, y) in enumerate(mats):
        descs[i] = GemvDesc(t, w.data_ptr(), w.shape[0], w.stride(0), y.data_ptr())
    ext = GemvExt()
    ext.prologue = prologue
    ext.x2 = x2.data_ptr() if x2 is not None else None
    ext.eps = eps
    for i in range(MAX_FUSED):
        r = residual[i] if residual is not None and i < len(residual) else None
        ext.residual[i] = r.data_ptr() if r is not None else None
    ext.epilogue = EPI_SWIGLU if epi_y is not None else EPI_NONE
    ext.epi_y = epi_y.data_ptr() if epi_y is not None else None
    K = x.shape[-1]
    need = int(lib().mi355x_gemv_ext_workspace_size(K))
    ws = _workspace(need, x.device, stream)
    _check(lib().mi355x_gemv_fused_ext(descs, n, x.data_ptr(), K, ctypes.byref(ext), ws.data_ptr(), need,
                                       _stream(stream)), "mi355x_gemv_fused_ext")


# ------------------------------------------- decode ops (mi355x_get_rows ... attn)
def get_rows(type_, table, K, ids, out=None, stream=None):
    """table: (rows, rowbytes) uint8 (or (rows, K) f32); ids: int32 cuda -> (n, K) f32."""
    torch = _torch()
    _require_device()
    n = ids.numel()
    if out is None:
        out = torch.empty((n, K), dtype=torch.float32, device=ids.device)
    _check(lib().mi355x_get_rows(type_, table.data_ptr(), K, table.stride(0) * table.element_size(), table.shape[0],
                                 ids.data_ptr(), n, out.data_ptr(), _stream(stream)), "mi355x_get_rows")
    return out


def rms_norm(x, eps, w=None, out=None, stream=None):
    torch = _torch()
    _require_device()
    x2 = x if x.dim() == 2 else x[None]
    if out is None:
        out = torch.empty_like(x)
    _check(lib().mi355x_rms_norm(x.data_ptr(), w.data_ptr() if w is not None else None, out.data_ptr(),
                                 x2.shape[1], x2.shape[0], eps, _stream(stream)), "mi355x_rms_norm")
    return out


def add(a, b, out=None, stream=None):
    out = _torch().empty_like(a) if out is None else out
    _check(lib().mi355x_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream(stream)), "mi355x_add")
    return out


def mul(a, b, out=None, stream=None):
    out = _torch().empty_like(a) if out is None else out
    _check(lib().mi355x_mul(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream(stream)), "mi355x_mul")
    return out


def swiglu(g, u, out=None, stream=None):
    out = _torch().empty_like(g) if out is None else out
    _check(lib().mi355x_swiglu(g.data_ptr(), u.data_ptr(), out.data_ptr(), g.numel(), _stream(stream)),
           "mi355x_swiglu")
    return out


def rope_table(n_pos, n_dims, freq_base=10000.0, freq_scale=1.0, device="cuda", stream=None):
    torch = _torch()
    _require_device()
    t = torch.empty((n_pos, n_dims // 2, 2), dtype=torch.float32, device=device)
    _check(lib().mi355x_rope_table(t.data_ptr(), n_pos, n_dims, freq_base, freq_scale, _stream(stream)),
           "mi355x_rope_table")
    return t


def rope(x, head_dim, n_dims, pos, table, out=None, stream=None):
    """x: (n_heads*head_dim,) f32; pos: int32 cuda tensor (1,)."""
    out = _torch().empty_like(x) if out is None else out
    _check(lib().mi355x_rope(x.data_ptr(), out.data_ptr(), head_dim, n_dims, x.numel() // head_dim, pos.data_ptr(),
                             table.data_ptr(), table.shape[0], _stream(stream)), "mi355x_rope")
    return out


def attn_decode(q, k, v, pos, table, k_cache, v_cache, n_head, n_head_kv, head_dim, scale, out=None, stream=None,
                rope_row=False):
    """k_cache: (n_ctx, n_head_kv*hd) int16/uint16 view of f16; v_cache: (n_head_kv*hd, n_ctx).
    rope_row: `table` is only the rope row of *pos (staged by the caller with the position)."""
    out = _torch().empty(n_head * head_dim, dtype=_torch().float32, device=q.device) if out is None else out
    a = AttnDesc(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(), table.data_ptr(), k_cache.data_ptr(),
                 v_cache.data_ptr(), out.data_ptr(), k_cache.shape[0], n_head, n_head_kv, head_dim, scale,
                 1 if rope_row else 0)
    _check(lib().mi355x_attn_decode(ctypes.byref(a), _stream(stream)), "mi355x_attn_decode")
    return out


def attn_path(n_ctx, n_head, n_head_kv, head_dim, cache_offset=0, f32_offset=0, rope_row=True):
    """The decode attention kernel (ATTN_PATH_*) mi355x_attn_decode would run for this shape under
    the current selectors: no launch, no device access (the descriptor's addresses are synthetic,
    16-B aligned plus `cache_offset` for the caches and `f32_offset` for q / k / v / rope)."""
    base = 1 << 20
    f = base + f32_offset
    a = AttnDesc(f, f + 4096, f + 8192, base, f + 12288, base + (1 << 12) + cache_offset,
                 base + (1 << 13) + cache_offset, base + (1 << 14), n_ctx, n_head, n_head_kv, head_dim,
                 1.0 / float(head_dim) ** 0.5, 1 if rope_row else 0)
    return int(lib().mi355x_attn_path(ctypes.byref(a)))


def attn_prompt(q, k, v, pos, table, k_cache, v_cache, n_head, n_head_kv, head_dim, scale, out=None, stream=None):
    """A prompt batch of T tokens: q (T, n_head*hd), k, v (T, n_head_kv*hd) f32, pos int32 cuda (T,),
    table the whole rope table; writes the T cells, returns out (T, n_head*hd)."""
    T = pos.numel()
    out = _torch().empty((T, n_head * head_dim), dtype=_torch().float32, device=q.device) if out is None else out
    a = AttnDesc(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(), table.data_ptr(), k_cache.data_ptr(),
                 v_cache.data_ptr(), out.data_ptr(), k_cache.shape[0], n_head, n_head_kv, head_dim, scale, 0)
    _check(lib().mi355x_attn_prompt(ctypes.byref(a), T, _stream(stream)), "mi355x_attn_prompt")
    return out


def _attn_batch_desc(q, k, v, pos, cells, mask, table, k_cache, v_cache, out, n_head, n_head_kv, head_dim, scale,
                     n_kv):
    torch = _torch()
    T = pos.numel()
    a = AttnDesc(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(), table.data_ptr(), k_cache.data_ptr(),
                 v_cache.data_ptr(), out.data_ptr(), k_cache.shape[0], n_head, n_head_kv, head_dim, scale, 0)
    if cells.dtype not in (torch.int32, torch.int64) or cells.numel() != T or not cells.is_contiguous():
        raise Mi355xError("attn_batch: cells must be a contiguous int32 / int64 tensor of one entry per token")
    if mask.dtype not in (torch.float16, torch.float32) or mask.dim() != 2 or mask.stride(1) != 1 or \
            mask.shape[0] < T:
        raise Mi355xError("attn_batch: mask must be float16 / float32 (rows >= T, >= n_kv) with unit column stride")
    return AttnBatchDesc(a, cells.data_ptr(), TYPE_I64 if cells.dtype == torch.int64 else TYPE_I32, mask.data_ptr(),
                         TYPE_F16 if mask.dtype == torch.float16 else TYPE_F32,
                         mask.stride(0) * mask.element_size(), n_kv, T)


def attn_batch(q, k, v, pos, cells, mask, table, k_cache, v_cache, n_head, n_head_kv, head_dim, scale, n_kv,
               out=None, stream=None):
    """The attention block of T tokens with the KV cells and the mask given (mi355x_attn_batch):
    q (T, n_head*hd), k, v (T, n_head_kv*hd) f32 before rope; pos int32 cuda (T,), only the rope
    row; cells int32 / int64 cuda (T,): token i is stored at cell cells[i]; mask (>= T, >= n_kv)
    float16 / float32, additive (0 visible, -inf hidden), row stride free; table the whole rope
    table. Every query attends over cells [0, n_kv). Returns out (T, n_head*hd)."""
    _require_device()
    T = pos.numel()
    out = _torch().empty((T, n_head * head_dim), dtype=_torch().float32, device=q.device) if out is None else out
    d = _attn_batch_desc(q, k, v, pos, cells, mask, table, k_cache, v_cache, out, n_head, n_head_kv, head_dim, scale,
                         n_kv)
    _check(lib().mi355x_attn_batch(ctypes.byref(d), _stream(stream)), "mi355x_attn_batch")
    return out


def attn_batch_path(n_ctx, n_head, n_head_kv, head_dim, n_kv):
    """ATTN_GROUP / ATTN_HEAD, or ATTN_PATH_STREAM (7) where attn_stream's mode sends the shape to
    the streamed form: the form mi355x_attn_batch takes for this shape (negative: the status it
    would return). No launch, no device access (synthetic, aligned addresses)."""
    base = 1 << 20
    a = AttnDesc(base, base + 4096, base + 8192, base + 64, base + 12288, base + (1 << 12), base + (1 << 13),
                 base + (1 << 14), n_ctx, n_head, n_head_kv, head_dim, 1.0 / float(head_dim) ** 0.5, 0)
    d = AttnBatchDesc(a, base + 128, TYPE_I32, base + 256, TYPE_F32, 4 * n_kv, n_kv, 1)
    return int(lib().mi355x_attn_batch_path(ctypes.byref(d)))


def _lib_with(symbol):
    L = lib()
    if not hasattr(L, symbol):
        raise Mi355xError(f"{LIB_PATH} has no {symbol} (a library built before it)")
    return L


def _vector_of(name, x):
    torch = _torch()
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
        raise Mi355xError(f"{name}: x must be a contiguous float32 cuda vector")
    return x.numel()


def _rows_of(name, x):
    torch = _torch()
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1 and
            x.stride(1) == 1):
        raise Mi355xError(f"{name}: x must be a 2-D float32 cuda tensor with unit column stride")
    rows, n = x.shape
    return rows, n, (x.stride(0) if rows > 1 else (n + 3) & ~3)  # (one row: torch's stride of it means nothing)


def _int32_out(name, out, device, rows=None):
    """out, or a new one: [1] (rows None) or one entry per row."""
    torch = _torch()
    out = torch.empty(rows or 1, dtype=torch.int32, device=device) if out is None else out
    if rows is None and not (out.is_cuda and out.dtype == torch.int32 and out.numel() >= 1):
        raise Mi355xError(f"{name}: out must be an int32 cuda tensor")
    if rows is not None and not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= rows):
        raise Mi355xError(f"{name}: out must be a contiguous int32 cuda tensor of one entry per row")
    return out


def _zeroed_workspace(workspace, nbytes, device, stream):
    """workspace, or a fresh zeroed one of nbytes."""
    torch = _torch()
    if workspace is None:
        workspace = torch.zeros(nbytes or 1, dtype=torch.uint8, device=device)
        if stream is not None:
            torch.cuda.current_stream().synchronize()  # zeroed on torch's stream, used on `stream`
    return workspace


def argmax_plan(n):
    """(workgroups, slice) of mi355x_argmax over n entries (mi355x_argmax_plan: the host's choice,
    no device): slice s is [s * slice, min(n, (s + 1) * slice)); or the error code."""
    wgs, slice_ = ctypes.c_int(0), ctypes.c_int64(0)
    rc = int(_lib_with("mi355x_argmax").mi355x_argmax_plan(n, ctypes.byref(wgs), ctypes.byref(slice_)))
    return (wgs.value, slice_.value) if rc == 0 else rc


def argmax_workspace_size(n):
    """Bytes of mi355x_argmax's workspace for n entries (0: n outside 1 .. 2^24)."""
    return int(_lib_with("mi355x_argmax").mi355x_argmax_workspace_size(n))


def argmax(x, out=None, workspace=None, stream=None):
    """Greedy sampling (mi355x_argmax): the smallest index of the maximum of the non-NaN entries
    of x, a contiguous f32 cuda vector, as an int32 cuda tensor [1] (no synchronization).
    workspace: a uint8 cuda tensor of argmax_workspace_size(n) bytes, zeroed once by its owner and
    reusable call after call on one stream; None: a fresh zeroed one."""
    _require_device()
    n = _vector_of("argmax", x)
    out = _int32_out("argmax", out, x.device)
    workspace = _zeroed_workspace(workspace, argmax_workspace_size(n), x.device, stream)
    _check(_lib_with("mi355x_argmax").mi355x_argmax(x.data_ptr(), n, out.data_ptr(), workspace.data_ptr(),
                                                    workspace.numel(), _stream(stream)), "mi355x_argmax")
    return out


def argmax_rows_workspace_size(n, rows):
    """Bytes of mi355x_argmax_rows' workspace for `rows` rows of n entries (0: n outside 1 .. 2^24
    or rows outside 1 .. 65535)."""
    return int(_lib_with("mi355x_argmax_rows").mi355x_argmax_rows_workspace_size(n, rows))


def argmax_rows(x, out=None, workspace=None, stream=None):
    """mi355x_argmax_rows: argmax's rule on every row of x, a 2-D f32 cuda tensor [T, n] with unit
    column stride (the row stride is free: >= n and a multiple of 4 floats), as an int32 cuda
    tensor [T] (no synchronization). workspace: a uint8 cuda tensor of
    argmax_rows_workspace_size(n, T) bytes, zeroed once by its owner and reusable call after call
    on one stream; None: a fresh zeroed one."""
    _require_device()
    rows, n, stride = _rows_of("argmax_rows", x)
    out = _int32_out("argmax_rows", out, x.device, rows)
    workspace = _zeroed_workspace(workspace, argmax_rows_workspace_size(n, rows), x.device, stream)
    _check(_lib_with("mi355x_argmax_rows").mi355x_argmax_rows(x.data_ptr(), n, rows, stride, out.data_ptr(),
                                                              workspace.data_ptr(), workspace.numel(), _stream(stream)),
           "mi355x_argmax_rows")
    return out


def topk_workspace_size(n, rows=1):
    """Bytes of the workspace of topk / sample (rows = 1) and topk_rows / sample_rows: 131200 a row
    whatever n and top_k are (0: n outside 1 .. 2^24 or rows outside 1 .. 65535)."""
    return int(_lib_with("mi355x_topk").mi355x_topk_workspace_size(n, rows))


def sampler_params(form, top_k, temp, top_p, min_p):
    """The SAMPLE nodes' leading op_params."""
    return [form, top_k, f32_bits(temp), f32_bits(top_p), f32_bits(min_p)]


def topk(x, top_k, workspace=None, stream=None):
    """mi355x_topk: the top_k (1 .. 64) largest non-NaN entries of x, a contiguous f32 cuda vector,
    under argmax's order, sorted: (idx int32 [top_k], val f32 [top_k]) cuda tensors, places past
    the number of non-NaN entries -1 / NaN (no synchronization). workspace: a uint8 cuda tensor of
    topk_workspace_size(n) bytes, zeroed once by its owner and reusable call after call on one
    stream, whatever n and top_k are; None: a fresh zeroed one."""
    torch = _torch()
    _require_device()
    n, k = _vector_of("topk", x), max(int(top_k), 1)
    idx = torch.empty(k, dtype=torch.int32, device=x.device)
    val = torch.empty(k, dtype=torch.float32, device=x.device)
    workspace = _zeroed_workspace(workspace, topk_workspace_size(n), x.device, stream)
    _check(_lib_with("mi355x_topk").mi355x_topk(x.data_ptr(), n, int(top_k), idx.data_ptr(), val.data_ptr(),
                                                workspace.data_ptr(), workspace.numel(), _stream(stream)), "mi355x_topk")
    return idx, val


def topk_rows(x, top_k, workspace=None, stream=None):
    """mi355x_topk_rows: topk's rule on every row of x, a 2-D f32 cuda tensor [T, n] with unit
    column stride (the row stride >= n and a multiple of 4 floats): (idx int32 [T, top_k], val f32
    [T, top_k]). workspace: topk_workspace_size(n, T) bytes, as topk's."""
    torch = _torch()
    _require_device()
    rows, n, stride = _rows_of("topk_rows", x)
    k = max(int(top_k), 1)
    idx = torch.empty((rows, k), dtype=torch.int32, device=x.device)
    val = torch.empty((rows, k), dtype=torch.float32, device=x.device)
    workspace = _zeroed_workspace(workspace, topk_workspace_size(n, rows), x.device, stream)
    _check(_lib_with("mi355x_topk").mi355x_topk_rows(x.data_ptr(), n, rows, stride, int(top_k), idx.data_ptr(),
                                                     val.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                                     _stream(stream)), "mi355x_topk_rows")
    return idx, val


def sample(x, u, top_k=40, top_p=0.95, min_p=0.05, temp=0.8, out=None, workspace=None, stream=None):
    """mi355x_sample: one token from x, a contiguous f32 cuda vector of logits, by llama.cpp's
    default chain (top-k -> top-p -> min-p -> temperature -> the draw u; the exact rule is in
    include/ggml_mi355x.h), as an int32 cuda tensor [1] (no synchronization). u: an f32 cuda
    tensor whose first entry is the draw, meant to lie in [0, 1). workspace: as topk's."""
    torch = _torch()
    _require_device()
    n = _vector_of("sample", x)
    if not (u.is_cuda and u.dtype == torch.float32 and u.numel() >= 1):
        raise Mi355xError("sample: u must be a float32 cuda tensor")
    out = _int32_out("sample", out, x.device)
    workspace = _zeroed_workspace(workspace, topk_workspace_size(n), x.device, stream)
    sp = SamplerDesc(int(top_k), float(temp), float(top_p), float(min_p))
    _check(_lib_with("mi355x_topk").mi355x_sample(x.data_ptr(), n, ctypes.byref(sp), u.data_ptr(), out.data_ptr(),
                                                  workspace.data_ptr(), workspace.numel(), _stream(stream)),
           "mi355x_sample")
    return out


def sample_rows(x, u, top_k=40, top_p=0.95, min_p=0.05, temp=0.8, out=None, workspace=None, stream=None):
    """mi355x_sample_rows: sample's rule on every row of x [T, n] (as topk_rows'), row i with the
    draw u[i] (a contiguous f32 cuda tensor [T]), as an int32 cuda tensor [T]."""
    torch = _torch()
    _require_device()
    rows, n, stride = _rows_of("sample_rows", x)
    if not (u.is_cuda and u.dtype == torch.float32 and u.is_contiguous() and u.numel() >= rows):
        raise Mi355xError("sample_rows: u must be a contiguous float32 cuda tensor of one entry per row")
    out = _int32_out("sample_rows", out, x.device, rows)
    workspace = _zeroed_workspace(workspace, topk_workspace_size(n, rows), x.device, stream)
    sp = SamplerDesc(int(top_k), float(temp), float(top_p), float(min_p))
    _check(_lib_with("mi355x_topk").mi355x_sample_rows(x.data_ptr(), n, rows, stride, ctypes.byref(sp), u.data_ptr(),
                                                       out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                                       _stream(stream)), "mi355x_sample_rows")
    return out


def logprob_dtype():
    """struct mi355x_logprob as a numpy structured dtype (24 bytes)."""
    import numpy as np
    return np.dtype([("max", "<f4"), ("x_target", "<f4"), ("argmax", "<i4"), ("pad", "<i4"), ("sum", "<f8")])


def logprob_workspace_size(n, rows):
    """Bytes of mi355x_logprob_rows' workspace for `rows` rows of n entries: argmax_rows' 2176 a row
    (0: n outside 1 .. 262144 or rows outside 1 .. 65535)."""
    return int(_lib_with("mi355x_logprob_rows").mi355x_logprob_workspace_size(n, rows))


def logprob_rows(x, targets, workspace=None, stream=None):
    """mi355x_logprob_rows: for every row of x, a 2-D f32 cuda tensor [T, n] of logits with unit
    column stride (the row stride >= n and a multiple of 4 floats), and its target index (targets:
    T ints, or an int32 cuda tensor [T]) the record of log softmax(x)[target]: a structured numpy
    array [T] of logprob_dtype() (max, x_target, argmax, pad, sum; the exact rule is in
    include/ggml_mi355x.h), after one synchronization; logprob_value(records) finishes it.
    workspace: a uint8 cuda tensor of logprob_workspace_size(n, T) bytes, zeroed once by its owner
    and reusable call after call on one stream, argmax_rows calls included; None: a fresh zeroed one."""
    import numpy as np
    torch = _torch()
    _require_device()
    rows, n, stride = _rows_of("logprob_rows", x)
    if not torch.is_tensor(targets):
        targets = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32)).to(x.device)
        if stream is not None:
            torch.cuda.current_stream().synchronize()  # copied on torch's stream, read on `stream`
    if not (targets.is_cuda and targets.dtype == torch.int32 and targets.is_contiguous() and targets.numel() == rows):
        raise Mi355xError("logprob_rows: targets must be one int32 per row")
    out = torch.empty(rows * 24, dtype=torch.uint8, device=x.device)
    workspace = _zeroed_workspace(workspace, logprob_workspace_size(n, rows), x.device, stream)
    _check(_lib_with("mi355x_logprob_rows").mi355x_logprob_rows(x.data_ptr(), n, rows, stride, targets.data_ptr(),
                                                                out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                                                _stream(stream)), "mi355x_logprob_rows")
    if stream is not None:
        torch.cuda.synchronize()
    return out.cpu().numpy().view(logprob_dtype()).copy()


def logprob_value(records):
    """mi355x_logprob_value over records of logprob_dtype(): float64 log-probabilities,
    x_target - max - log(sum), the logarithm taken on the host (a target outside its row: NaN)."""
    import math
    import numpy as np
    r = np.asarray(records)
    # libm's log, one value at a time, as the header's inline function takes it
    logs = np.array([math.log(s) if s > 0 else (-math.inf if s == 0 else math.nan) for s in r["sum"].ravel().tolist()],
                    dtype=np.float64).reshape(r.shape)
    with np.errstate(all="ignore"):
        return r["x_target"].astype(np.float64) - r["max"].astype(np.float64) - logs


def penalize_params(last_n, repeat, freq, present, n_bias):
    """The PENALIZE node's op_params."""
    return [last_n, f32_bits(repeat), f32_bits(freq), f32_bits(present), n_bias]


def bias_pairs(bias):
    """A logit bias, None, a dict {token: bias} or a list of (token, bias) pairs, as the list of
    (int, float) pairs in its order."""
    if bias is None:
        return []
    pairs = [(int(t), float(v)) for t, v in (bias.items() if isinstance(bias, dict) else bias)]
    if len(pairs) > LOGIT_BIAS_MAX or any(not -2 ** 31 <= t < 2 ** 31 for t, _ in pairs):
        raise Mi355xError(f"logit bias: at most {LOGIT_BIAS_MAX} (int32 token, bias) pairs")
    return pairs


def penalize_rows(x, hist=None, end=None, last_n=0, repeat=1.0, freq=0.0, present=0.0, bias=None, stream=None):
    """mi355x_penalize_rows: the sampler's repetition / frequency / presence penalties and logit bias
    (the exact rule is in include/ggml_mi355x.h), in place on x, a contiguous f32 cuda vector [n]
    or a 2-D one [rows, n] with unit column stride (any row stride >= n); returns x (no
    synchronization). hist: an int32 cuda tensor [n_hist] or [rows, n_hist] with unit column
    stride, the rows' past tokens; end: one int per row (or an int32 cuda tensor [rows]): row i's
    window is hist[i][end[i] - last_n + 1 .. end[i]], clipped to the row. bias: None, a dict
    {token: bias}, a list of (token, bias) pairs (added in list order; float("-inf") bans a
    token), or a pair of cuda tensors (int32 [n_bias], float32 [n_bias]). last_n 0: hist and end
    are not needed. With a `stream` and an end or bias given on the host, the call synchronizes."""
    import numpy as np
    torch = _torch()
    _require_device()
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (1, 2) and x.numel() >= 1 and
            x.stride(-1) == 1):
        raise Mi355xError("penalize_rows: x must be a float32 cuda vector or matrix with unit column stride")
    rows, n = (1, x.shape[0]) if x.dim() == 1 else x.shape
    stride = x.stride(0) if x.dim() == 2 and rows > 1 else n
    copied = False
    hist_ptr, hist_stride, n_hist, end_ptr = None, 0, 0, None
    if last_n > 0:
        if not (torch.is_tensor(hist) and hist.is_cuda and hist.dtype == torch.int32 and hist.dim() in (1, 2) and
                hist.numel() >= 1 and hist.stride(-1) == 1 and (hist.shape[0] if hist.dim() == 2 else 1) == rows):
            raise Mi355xError("penalize_rows: hist must be an int32 cuda tensor [n_hist] or [rows, n_hist] with unit "
                              "column stride")
        n_hist = hist.shape[-1]
        hist_stride = hist.stride(0) if hist.dim() == 2 and rows > 1 else n_hist
        if end is None:
            raise Mi355xError("penalize_rows: end is needed with last_n > 0")
        if not torch.is_tensor(end):
            end = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(end), dtype=np.int32)).to(x.device)
            copied = True
        if not (end.is_cuda and end.dtype == torch.int32 and end.is_contiguous() and end.numel() == rows):
            raise Mi355xError("penalize_rows: end must be one int32 per row")
        hist_ptr, end_ptr = hist.data_ptr(), end.data_ptr()
    if isinstance(bias, tuple) and len(bias) == 2 and torch.is_tensor(bias[0]):
        bt, bv = bias
        if not (bt.is_cuda and bt.dtype == torch.int32 and bt.is_contiguous() and bv.is_cuda and bv.dtype == torch.float32 and
                bv.is_contiguous() and bt.numel() == bv.numel()):
            raise Mi355xError("penalize_rows: bias tensors must be int32 / float32 cuda vectors of one length")
        n_bias = bt.numel()
    else:
        pairs = bias_pairs(bias)
        n_bias = len(pairs)
        if n_bias:
            bt = torch.tensor([t for t, _ in pairs], dtype=torch.int32).to(x.device)
            bv = torch.tensor([v for _, v in pairs], dtype=torch.float32).to(x.device)
            copied = True
    if copied and stream is not None:
        torch.cuda.current_stream().synchronize()  # copied on torch's stream, read on `stream`
    pen = PenaltiesDesc(int(last_n), float(repeat), float(freq), float(present))
    _check(_lib_with("mi355x_penalize_rows").mi355x_penalize_rows(
        x.data_ptr(), n, rows, stride, ctypes.byref(pen), hist_ptr, hist_stride, n_hist, end_ptr,
        bt.data_ptr() if n_bias else None, bv.data_ptr() if n_bias else None, n_bias, _stream(stream)),
        "mi355x_penalize_rows")
    if copied and stream is not None:
        torch.cuda.synchronize()  # the copies made here are read on `stream`: they stay until it is done
    return x


def kv_shift_params(n_head_kv, head_dim, n_cells=None, keep=None, discard=None, n_past=None):
    """The KV_SHIFT node's op_params: the DELTAS form over n_cells cells, or the DISCARD form."""
    if n_cells is not None:
        return [n_head_kv, head_dim, KV_SHIFT_DELTAS, n_cells]
    return [n_head_kv, head_dim, KV_SHIFT_DISCARD, keep, discard, n_past]


def kv_shift(k_cache, table, n_head_kv, head_dim, v_cache=None, delta=None, n_cells=None, keep=None, discard=None,
             n_past=None, stream=None):
    """mi355x_kv_shift: the context shift in place on the caches (the exact rule is in
    include/ggml_mi355x.h); no synchronization. k_cache: a contiguous 2-byte cuda tensor
    [n_ctx, n_head_kv * head_dim] (f16 bits); table: rope_table(n_pos, head_dim). With `delta`, an
    int32 cuda tensor, the DELTAS form: K cell c in [0, n_cells) (default: every delta) is re-roped
    by delta[c]; V is not touched. Otherwise the DISCARD form: cells [keep, keep + discard) are
    dropped and the cells up to n_past slide down over them, K re-roped by -discard, V (v_cache, a
    contiguous 2-byte cuda tensor [n_head_kv * head_dim, n_ctx]) moved."""
    torch = _torch()
    _require_device()
    kvw = n_head_kv * head_dim

    def cache(name, x, shape1):
        if not (torch.is_tensor(x) and x.is_cuda and x.element_size() == 2 and x.dim() == 2 and x.is_contiguous() and
                x.shape[1] == shape1):
            raise Mi355xError(f"kv_shift: {name} must be a contiguous 2-byte cuda tensor [*, {shape1}]")
        return x.shape[0]

    n_ctx = cache("k_cache", k_cache, kvw)
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and
            table.numel() >= head_dim and table.numel() % head_dim == 0):
        raise Mi355xError("kv_shift: table must be a contiguous float32 cuda tensor of whole rope rows")
    d = KvShiftDesc(k_cache.data_ptr(), None, table.data_ptr(), None, n_ctx, n_head_kv, head_dim,
                    table.numel() // head_dim, KV_SHIFT_DELTAS, 0, 0, 0, 0)
    if v_cache is not None:
        if cache("v_cache", v_cache, n_ctx) != kvw:
            raise Mi355xError(f"kv_shift: v_cache must have {kvw} rows")
        d.v_cache = v_cache.data_ptr()
    if delta is not None:
        if not (torch.is_tensor(delta) and delta.is_cuda and delta.dtype == torch.int32 and delta.dim() == 1 and
                delta.is_contiguous()):
            raise Mi355xError("kv_shift: delta must be a contiguous int32 cuda vector")
        d.delta = delta.data_ptr()
        d.n_cells = delta.numel() if n_cells is None else n_cells
        if d.n_cells > delta.numel():
            raise Mi355xError("kv_shift: n_cells exceeds the deltas")
    else:
        if v_cache is None or keep is None or discard is None or n_past is None:
            raise Mi355xError("kv_shift: the DISCARD form needs v_cache, keep, discard and n_past")
        d.form, d.keep, d.discard, d.n_past = KV_SHIFT_DISCARD, keep, discard, n_past
    _check(_lib_with("mi355x_kv_shift").mi355x_kv_shift(ctypes.byref(d), _stream(stream)), "mi355x_kv_shift")


def moe_route(gate_inp, x, n_used, records=None, probs=False, stream=None):
    """mi355x_moe_route: the router of a MoE layer (the exact rule is in include/ggml_mi355x.h). gate_inp: f32
    cuda [n_expert, n_embd]; x: f32 cuda [T, n_embd] (rows may be strided) or [n_embd]. Returns the records, an
    int32 cuda tensor [T, >= 2 * n_used] (row t: the ids, then the bits of the weights; `records` to write
    into, its row stride the record stride), and with probs=True also the probabilities f32 [T, n_expert]."""
    torch = _torch()
    _require_device()
    if x.dim() == 1:
        x = x[None]
    if not (gate_inp.is_cuda and gate_inp.dtype == torch.float32 and gate_inp.dim() == 2 and gate_inp.is_contiguous()):
        raise Mi355xError("moe_route: gate_inp must be a contiguous float32 cuda tensor [n_expert, n_embd]")
    n_expert, n_embd = gate_inp.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == n_embd and x.stride(1) == 1):
        raise Mi355xError(f"moe_route: x must be a float32 cuda tensor [T, {n_embd}] with contiguous rows")
    T = x.shape[0]
    if records is None:
        records = torch.zeros((T, 2 * n_used), dtype=torch.int32, device=x.device)
    if not (records.is_cuda and records.dtype == torch.int32 and records.dim() == 2 and records.shape[0] == T and
            records.stride(1) == 1):
        raise Mi355xError("moe_route: records must be an int32 cuda tensor [T, >= 2 * n_used] with contiguous rows")
    pr = torch.zeros((T, n_expert), dtype=torch.float32, device=x.device) if probs else None
    _check(_lib_with("mi355x_mul_mat_id").mi355x_moe_route(
        gate_inp.data_ptr(), n_embd, n_expert, x.data_ptr(), x.stride(0), T, n_used, records.data_ptr(),
        records.stride(0), pr.data_ptr() if probs else None, _stream(stream)), "mi355x_moe_route")
    return (records, pr) if probs else records


def mul_mat_id(type_, experts, K, x, records, n_used, out=None, stream=None):
    """mi355x_mul_mat_id: experts: uint8 cuda [n_expert, N, >= row bytes] (the last dim contiguous; the strides are
    nb02, nb01); x: f32 cuda [T, ne11, K] with ne11 1 or n_used, packed over the tokens; records: moe_route's (the
    ids are its first n_used words a row). Returns f32 cuda [T, n_used, N]."""
    torch = _torch()
    _require_device()
    if not (experts.is_cuda and experts.dtype == torch.uint8 and experts.dim() == 3 and experts.stride(2) == 1):
        raise Mi355xError("mul_mat_id: experts must be a uint8 cuda tensor [n_expert, N, row bytes]")
    n_expert, N = experts.shape[0], experts.shape[1]
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == K and x.stride(2) == 1 and
            x.stride(0) == x.shape[1] * x.stride(1)):
        raise Mi355xError(f"mul_mat_id: x must be a float32 cuda tensor [T, ne11, {K}], its rows evenly strided")
    T, ne11 = x.shape[0], x.shape[1]
    if not (records.is_cuda and records.dtype == torch.int32 and records.dim() == 2 and records.shape[0] == T and
            records.stride(1) == 1):
        raise Mi355xError("mul_mat_id: records must be an int32 cuda tensor [T, >= n_used]")
    if out is None:
        out = torch.empty((T, n_used, N), dtype=torch.float32, device=x.device)
    L = _lib_with("mi355x_mul_mat_id")
    ws = int(L.mi355x_mul_mat_id_workspace_size(type_, K, n_used, T))
    workspace = _workspace(ws, x.device, stream) if ws else None
    _check(L.mi355x_mul_mat_id(type_, experts.data_ptr(), K, N, experts.stride(1), experts.stride(0), n_expert,
                               x.data_ptr(), ne11, x.stride(1), records.data_ptr(), records.stride(0), n_used, T,
                               out.data_ptr(), workspace.data_ptr() if ws else None, ws, _stream(stream)),
           "mi355x_mul_mat_id")
    return out


def moe_combine(ex, records, n_used, out=None, stream=None):
    """mi355x_moe_combine: ex f32 cuda [T, n_used, n] packed, records moe_route's -> f32 cuda [T, n]."""
    torch = _torch()
    _require_device()
    if not (ex.is_cuda and ex.dtype == torch.float32 and ex.dim() == 3 and ex.shape[1] == n_used and ex.is_contiguous()):
        raise Mi355xError("moe_combine: ex must be a contiguous float32 cuda tensor [T, n_used, n]")
    T, _, n = ex.shape
    if not (records.is_cuda and records.dtype == torch.int32 and records.dim() == 2 and records.shape[0] == T and
            records.stride(1) == 1):
        raise Mi355xError("moe_combine: records must be an int32 cuda tensor [T, >= 2 * n_used]")
    if out is None:
        out = torch.empty((T, n), dtype=torch.float32, device=ex.device)
    _check(_lib_with("mi355x_mul_mat_id").mi355x_moe_combine(ex.data_ptr(), n, n_used, T, records.data_ptr(),
                                                             records.stride(0), out.data_ptr(), _stream(stream)),
           "mi355x_moe_combine")
    return out


def block_partials(type_, w, K, q8_row, stream=None):
    """Per-superblock integer partials -> (N, nb, 2) int32 cuda tensor."""
    torch = _torch()
    _require_device()
    N = w.shape[0]
    out = torch.zeros((N, K // QK_K, 2), dtype=torch.int32, device=w.device)
    _check(lib().mi355x_debug_block_partials(type_, w.data_ptr(), K, N, w.stride(0), q8_row.data_ptr(),
                                             out.data_ptr(), _stream(stream)), "mi355x_debug_block_partials")
    return out


# ------------------------------------------- raw ggml surface (device pointers)
def vec_dot_q4_K_q8_K(n, s, bs, vx, bx, vy, by, nrc):
    lib().mi355x_vec_dot_q4_K_q8_K(n, s, bs, vx, bx, vy, by, nrc)


def vec_dot_q5_K_q8_K(n, s, bs, vx, bx, vy, by, nrc):
    lib().mi355x_vec_dot_q5_K_q8_K(n, s, bs, vx, bx, vy, by, nrc)


def vec_dot_q6_K_q8_K(n, s, bs, vx, bx, vy, by, nrc):
    lib().mi355x_vec_dot_q6_K_q8_K(n, s, bs, vx, bx, vy, by, nrc)


def quantize_row_q8_K(x, y, k):
    lib().mi355x_quantize_row_q8_K(x, y, k)


# ------------------------------------------------------------ backend mirror
class Backend:
    """ggml-backend device mirror: own stream, device buffers, graph_compute."""

    def __init__(self, device=0):
        _require_device()
        self.h = lib().mi355x_backend_init(device)
        if not self.h:
            raise Mi355xError("mi355x_backend_init failed")
        self._keep = []

    @property
    def name(self):
        return lib().mi355x_backend_name(self.h).decode()

    @property
    def stream(self):
        return lib().mi355x_backend_stream(self.h)

    def alloc(self, size):
        p = lib().mi355x_backend_alloc(self.h, size)
        if not p:
            raise Mi355xError("alloc failed")
        return p

    def free_buffer(self, p):
        lib().mi355x_backend_free_buffer(self.h, p)

    def set_tensor(self, dst, host_array):
        import numpy as np
        a = np.ascontiguousarray(host_array)
        self._keep.append(a)  # keep alive until synchronize
        _check(lib().mi355x_backend_set_tensor(self.h, dst, a.ctypes.data, a.nbytes), "set_tensor")

    def get_tensor(self, host_array, src):
        _check(lib().mi355x_backend_get_tensor(self.h, host_array.ctypes.data, src, host_array.nbytes),
               "get_tensor")

    def synchronize(self):
        _check(lib().mi355x_backend_synchronize(self.h), "synchronize")
        self._keep.clear()

    def set_fusion(self, enable):
        return int(lib().mi355x_backend_set_fusion(self.h, 1 if enable else 0))

    def set_attn_oproj(self, enable):
        """Decode attention + o-proj GEMV in one launch (default off); returns the previous."""
        return int(lib().mi355x_backend_set_attn_oproj(self.h, 1 if enable else 0))

    def set_layer_engine(self, enable):
        """Each decode layer as one persistent launch (csrc/kq_layer.hip); returns the previous."""
        return int(lib().mi355x_backend_set_layer_engine(self.h, 1 if enable else 0))

    def layer_error(self):
        """Non-zero if a persistent-layer launch gave up waiting (results invalid); clears it."""
        return int(lib().mi355x_backend_layer_error(self.h))

    def set_comm(self, rank, world, unique_id: bytes):
        """Join the RCCL communicator of a row split (every rank, same id bytes)."""
        buf = ctypes.create_string_buffer(bytes(unique_id), len(unique_id))
        _check(lib().mi355x_backend_set_comm(self.h, rank, world, buf), "set_comm")

    def set_comm_loopback(self, rank, world):
        """Test emulation of one rank of a row split on this GPU (no communicator)."""
        _check(lib().mi355x_backend_set_comm_loopback(self.h, rank, world), "set_comm_loopback")

    @property
    def comm_world(self):
        return int(lib().mi355x_backend_comm_world(self.h))

    def graph_compute(self, nodes, use_graph=True):
        arr = (ctypes.POINTER(Tensor) * len(nodes))(*[ctypes.pointer(n) for n in nodes])
        return int(lib().mi355x_backend_graph_compute(self.h, arr, len(nodes), 1 if use_graph else 0))

    def close(self):
        if self.h:
            lib().mi355x_backend_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lower_ggml_graph(gnodes, rope_table_ptr, rope_n_pos, freq_base, freq_scale=1.0, arena_cap=None,
                     cells_eq_pos=True, cells_from_graph=False):
    """mi355x_lower_ggml_graph over a list of GTensor nodes (graph order). Returns
    (status, [Tensor node list], arena) — the arena keeps the nodes alive.
    cells_eq_pos: the adapter's promise (mi355x_lower_opts) that the batch is one
    sequence whose KV cells equal its positions under a causal mask. cells_from_graph (with
    cells_eq_pos False): attention blocks become ATTN_BATCH nodes that read the K store's cell
    indices and the soft_max mask on the device; the promise is that the V store's indices
    match the K store's (v_idxs[i*kvw + ch] == ch*kv_size + k_idxs[i], cells inside the cache)."""
    n = len(gnodes)
    arr = (ctypes.POINTER(GTensor) * max(1, n))(*[ctypes.pointer(t) for t in gnodes])
    cap = arena_cap or (4 * n + 64)
    arena = (Tensor * cap)()
    out = (ctypes.POINTER(Tensor) * cap)()
    nn = ctypes.c_int(0)
    opts = LowerOpts(rope_table_ptr, rope_n_pos, freq_base, freq_scale, 1 if cells_eq_pos else 0,
                     1 if cells_from_graph else 0)
    rc = int(lib().mi355x_lower_ggml_graph(arr, n, ctypes.byref(opts), arena, cap, out, cap, ctypes.byref(nn)))
    return rc, [out[i].contents for i in range(nn.value)], (arena, out)


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (rank 0 of a row split creates it, the others receive it)."""
    n = int(lib().mi355x_comm_id_size())
    buf = ctypes.create_string_buffer(n)
    _check(lib().mi355x_comm_get_unique_id(buf), "comm_get_unique_id")
    return buf.raw


def supports_op(t: Tensor) -> bool:
    return bool(lib().mi355x_backend_supports_op(ctypes.byref(t)))


def make_tensor(type_, ne0, ne1, data, row_stride=None, op=OP_NONE, src0=None, src1=None, srcs=None,
                op_params=None, flags=0) -> Tensor:
    """2-D ggml-style tensor descriptor: ne0 elements per row, ne1 rows, row stride nb1 bytes.
    `srcs` (list) overrides src0/src1; op_params: up to 8 int32 (use f32_bits for floats)."""
    t = Tensor()
    t.type = type_
    t.op = op
    nb0 = BLOCK_BYTES.get(type_, 2 if type_ == TYPE_F16 else 8 if type_ == TYPE_I64 else 4)
    nb1 = row_stride if row_stride is not None else (ne0 // QK_K * nb0 if type_ in BLOCK_BYTES else ne0 * nb0)
    t.ne[0], t.ne[1], t.ne[2], t.ne[3] = ne0, ne1, 1, 1
    t.nb[0], t.nb[1], t.nb[2], t.nb[3] = nb0, nb1, nb1 * ne1, nb1 * ne1
    srcs = list(srcs) if srcs is not None else [src0, src1]
    for i in range(MAX_SRC):
        s = srcs[i] if i < len(srcs) else None
        t.src[i] = ctypes.pointer(s) if s is not None else ctypes.POINTER(Tensor)()
    t.data = data
    for i, v in enumerate(op_params or []):
        t.op_params[i] = v
    t.flags = flags
    return t


def f32_bits(v: float) -> int:
    import struct
    return struct.unpack("<i", struct.pack("<f", v))[0]
