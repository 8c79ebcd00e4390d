// ggml-mi355x.h — public header of the MI355X K-quant ggml backend, the sibling of
// ggml/include/ggml-cpu.h / ggml-cuda.h [U] in llama.cpp's tree.
//
// The backend is registered like every ggml backend: ggml_backend_mi355x_reg() is added
// to ggml-backend-reg.cpp's registry (or the library is loaded dynamically through
// GGML_BACKEND_DL_IMPL's ggml_backend_init), and llama.cpp's scheduler then hands it the
// graph splits whose nodes its device's supports_op accepts (ggml-backend.cpp:1553 ->
// iface.graph_compute, README.md:162-163).
#pragma once

#include "ggml-backend.h"

#ifdef __cplusplus
extern "C" {
#endif

// the registry entry: one device per gfx950 GPU the library runs on
GGML_BACKEND_API ggml_backend_reg_t ggml_backend_mi355x_reg(void);
// a backend (one HIP stream) on device `device`; NULL when it does not exist
GGML_BACKEND_API ggml_backend_t ggml_backend_mi355x_init(int device);
GGML_BACKEND_API bool ggml_backend_is_mi355x(ggml_backend_t backend);
// device buffer type (weights and compute buffers live in device memory, GGUF bytes
// unchanged: no repack)
GGML_BACKEND_API ggml_backend_buffer_type_t ggml_backend_mi355x_buffer_type(int device);
GGML_BACKEND_API int ggml_backend_mi355x_get_device_count(void);
// Several sequences in the unified KV cache, or one whose cells are not its positions (a
// removed cell, a context shift, a reused prefix). Off (the default): such a graph is refused
// (GGML_STATUS_FAILED), as a graph the backend cannot compute always is. On: its attention
// blocks run as ATTN_BATCH nodes that take each token's cell from the K store's indices and
// the mask from the graph's KQ mask, when the V store's indices name the same cells
// (mi355x_adapter::cells_match). Graphs whose cells equal their positions under a causal mask
// keep the single-sequence path either way. Also returned by the registry's get_proc_address
// under this name.
GGML_BACKEND_API void ggml_backend_mi355x_set_multi_seq(ggml_backend_t backend, bool enable);
// KV caches of more than 7040-7616 cells (the per-head attention kernels' limit), up to 131072:
// off (the default), a graph over such a cache is refused (GGML_STATUS_FAILED); on, its
// attention runs on the library's streamed kernels (mi355x_attn_stream mode 1, same bits).
// Process-wide, like the library's selector; caches that run today keep their kernels either
// way. With ggml_backend_mi355x_set_multi_seq on as well, multi-sequence graphs (ATTN_BATCH)
// over such caches run on the streamed kernels too. Also returned by the registry's
// get_proc_address under this name.
GGML_BACKEND_API void ggml_backend_mi355x_set_long_context(bool enable);
// Prompt (batched, single-sequence) attention on the f16 matrix cores within the library's stated
// bound (mi355x_attn_prompt_precision F16) instead of the decode token's bits: off (the default),
// nothing changes; on, the attention of graphs of two or more tokens runs kq_attn_prompt_f16.
// Decode graphs, multi-sequence graphs (ATTN_BATCH) and both KV caches keep their bits.
// Process-wide, like the library's selector. Also returned by the registry's get_proc_address
// under this name.
GGML_BACKEND_API void ggml_backend_mi355x_set_prompt_attn_f16(bool enable);

#ifdef __cplusplus
}
#endif
