"""llm_build_llama's graph over a ubatch of T tokens whose logits are ALL wanted (one token
per sequence of a multi-sequence decode step: inp_out_ids selects every row, so there is no
GET_ROWS after the last attention and the output norm and head run on [n_embd, T]) — test
infrastructure beside tests/ggml_graph.py, whose builder keeps only the last token's row.
Same ggml_build_forward_expand order; the KQ / KQV views span n_kv cells of the cache from
cell 0 and the mask is [n_kv, T]."""
from __future__ import annotations

import numpy as np

import ggml_mi355x as g
from tests.ggml_graph import F16, F32, I32, I64, Graph, f32_bits, rope_params


def llama_batch_graph(hp, L, n_ctx, n_tokens, alloc=None, n_kv=None, mask_type=F16):
    """L as for tests.ggml_graph.llama_decode_graph ("inp_tokens", "inp_pos", "kq_mask", "k_idxs",
    "v_idxs": device pointers of [T] I32, [T] I32, [n_kv, T] mask_type, [T] I64, [kvw*T] I64).
    The last node is result_output [n_vocab, T], flagged OUTPUT. Returns Graph."""
    G = Graph(alloc)
    E, V, hd, nh, nkv = hp["n_embd"], hp["n_vocab"], hp["head_dim"], hp["n_head"], hp["n_head_kv"]
    kvw = nkv * hd
    eps = f32_bits(hp["eps"])
    T = n_tokens
    n_kv = n_ctx if n_kv is None else n_kv

    def mat(name):
        t, ne0, ne1, data, rb = L[name]
        return G.leaf(t, [ne0, ne1], data, nb=[g.BLOCK_BYTES[t], rb, rb * ne1, rb * ne1], name=name)

    def vec(name, n):
        return G.leaf(F32, [n], L[name], name=name)

    tok = G.leaf(I32, [T], L["inp_tokens"], name="inp_tokens")
    pos = G.leaf(I32, [T], L["inp_pos"], name="inp_pos")
    mask = G.leaf(mask_type, [n_kv, T], L["kq_mask"], name="kq_mask")
    inpL = G.node(g.GOP_GET_ROWS, F32, [E, T], [mat("token_embd"), tok], name="inp_embd")
    scale = f32_bits(np.float32(1.0) / np.sqrt(np.float32(hd)))
    for il in range(hp["n_layer"]):
        p = f"blk.{il}."
        inpSA = inpL
        cur = G.node(g.GOP_RMS_NORM, F32, [E, T], [inpL], [eps], name="norm")
        cur = G.node(g.GOP_MUL, F32, [E, T], [cur, vec(p + "attn_norm", E)], name="attn_norm")
        q = G.node(g.GOP_MUL_MAT, F32, [nh * hd, T], [mat(p + "attn_q"), cur], name="Qcur")
        q = G.alias(g.GOP_RESHAPE, q, [hd, nh, T])
        q = G.node(g.GOP_ROPE, F32, [hd, nh, T], [q, pos], rope_params(hd, hp["freq_base"]), name="Qcur_rope")
        k = G.node(g.GOP_MUL_MAT, F32, [kvw, T], [mat(p + "attn_k"), cur], name="Kcur")
        k = G.alias(g.GOP_RESHAPE, k, [hd, nkv, T])
        k = G.node(g.GOP_ROPE, F32, [hd, nkv, T], [k, pos], rope_params(hd, hp["freq_base"]), name="Kcur_rope")
        v = G.node(g.GOP_MUL_MAT, F32, [kvw, T], [mat(p + "attn_v"), cur], name="Vcur")
        v = G.alias(g.GOP_RESHAPE, v, [hd, nkv, T])
        kc = G.leaf(F16, [kvw, n_ctx], L[f"k_cache.{il}"], name=f"cache_k_l{il}")
        vc = G.leaf(F16, [n_ctx, kvw], L[f"v_cache.{il}"], name=f"cache_v_l{il}")
        k_idxs = G.leaf(I64, [T], L["k_idxs"], name="k_idxs")
        v_idxs = G.leaf(I64, [kvw * T], L["v_idxs"], name="v_idxs")
        kview = G.alias(g.GOP_VIEW, kc, [kvw, n_ctx])
        G.node(g.GOP_SET_ROWS, F16, [kvw, n_ctx], [G.alias(g.GOP_RESHAPE, k, [kvw, T]), k_idxs], view_src=kview,
               data=kc.data, name="k_store")
        vview = G.alias(g.GOP_RESHAPE, vc, [1, kvw * n_ctx])
        G.node(g.GOP_SET_ROWS, F16, [1, kvw * n_ctx], [G.alias(g.GOP_RESHAPE, v, [1, kvw * T]), v_idxs],
               view_src=vview, data=vc.data, name="v_store")
        qp = G.alias(g.GOP_PERMUTE, q, [hd, T, nh])
        kv = G.alias(g.GOP_VIEW, kc, [hd, n_kv, nkv])
        kq = G.node(g.GOP_MUL_MAT, F32, [n_kv, T, nh], [kv, qp], name="kq")
        kq = G.node(g.GOP_SOFT_MAX, F32, [n_kv, T, nh], [kq, mask], [scale, f32_bits(0.0)], name="kq_soft_max")
        vv = G.alias(g.GOP_VIEW, vc, [n_kv, hd, nkv])
        kqv = G.node(g.GOP_MUL_MAT, F32, [hd, T, nh], [vv, kq], name="kqv")
        cur = G.alias(g.GOP_PERMUTE, kqv, [hd, nh, T])
        cur = G.node(g.GOP_CONT, F32, [hd * nh, T], [cur], name="kqv_out")
        cur = G.node(g.GOP_MUL_MAT, F32, [E, T], [mat(p + "attn_output"), cur], name="attn_out")
        ffn_inp = G.node(g.GOP_ADD, F32, [E, T], [cur, inpSA], name="ffn_inp")
        cur = G.node(g.GOP_RMS_NORM, F32, [E, T], [ffn_inp], [eps], name="norm")
        cur = G.node(g.GOP_MUL, F32, [E, T], [cur, vec(p + "ffn_norm", E)], name="ffn_norm")
        F = hp["n_ff"]
        tmp = G.node(g.GOP_MUL_MAT, F32, [F, T], [mat(p + "ffn_up"), cur], name="ffn_up")
        gt = G.node(g.GOP_MUL_MAT, F32, [F, T], [mat(p + "ffn_gate"), cur], name="ffn_gate")
        cur = G.node(g.GOP_GLU, F32, [F, T], [gt, tmp], [g.GLU_SWIGLU, 0], name="ffn_swiglu")
        cur = G.node(g.GOP_MUL_MAT, F32, [E, T], [mat(p + "ffn_down"), cur], name="ffn_out")
        inpL = G.node(g.GOP_ADD, F32, [E, T], [cur, ffn_inp], name="l_out")
    cur = G.node(g.GOP_RMS_NORM, F32, [E, T], [inpL], [eps], name="norm")
    cur = G.node(g.GOP_MUL, F32, [E, T], [cur, vec("output_norm", E)], name="result_norm")
    G.node(g.GOP_MUL_MAT, F32, [V, T], [mat("output"), cur], flags=g.FLAG_OUTPUT, name="result_output")
    return G
