"""Synthetic MoE llama models (Mixtral's layout) for the MoE tests: tests/llama_model.py's weights with the
dense FFN of every layer replaced by a router and expert tensors, for the CPU rule (tests/moe_ref.py) and,
the same bytes, for ggml_mi355x.llama.LlamaDecoder.

Q4_K_M mix [U]: ffn_down_exps Q6_K in the use_more_bits layers, every other expert tensor Q4_K; the router
ffn_gate_inp stays f32 (llama-quant.cpp never quantizes it [U])."""
import numpy as np

from tests import llama_model as LM


def build(hp, seed=0):
    """Host weights: llama_model.build's dict without ffn_gate / ffn_up / ffn_down, plus per layer
    ffn_gate_inp f32 [n_expert, n_embd] and ffn_gate_exps / ffn_up_exps / ffn_down_exps
    (type, uint8 [n_expert, rows, row bytes])."""
    w = LM.build(hp, seed)
    rng = np.random.default_rng([seed, 0x40E])
    E, F, L, ne = hp["n_embd"], hp["n_ff"], hp["n_layer"], hp["n_expert"]
    for i in range(L):
        p = f"blk.{i}."
        for m in ("ffn_gate", "ffn_up", "ffn_down"):
            del w[p + m]
        # logits of a few units apart: the selection varies from token to token, the weights are uneven
        w[p + "ffn_gate_inp"] = (rng.standard_normal((ne, E)) * 2.0 / np.sqrt(E)).astype(np.float32)
        dt = LM.Q6_K if LM.use_more_bits(i, L) else LM.Q4_K
        w[p + "ffn_gate_exps"] = (LM.Q4_K, np.stack([LM.kquant(rng, LM.Q4_K, F, E) for _ in range(ne)]))
        w[p + "ffn_up_exps"] = (LM.Q4_K, np.stack([LM.kquant(rng, LM.Q4_K, F, E) for _ in range(ne)]))
        w[p + "ffn_down_exps"] = (dt, np.stack([LM.kquant(rng, dt, E, F) for _ in range(ne)]))
    return w


def oracle_model(hp, w, n_ctx):
    """The dict tests/moe_ref.decode_token_moe expects (+ a fresh zero KV cache)."""
    from oracle import kq_ops_oracle as O
    layers = []
    for i in range(hp["n_layer"]):
        p = f"blk.{i}."
        layers.append({"attn_norm": w[p + "attn_norm"], "ffn_norm": w[p + "ffn_norm"], "wq": w[p + "attn_q"],
                       "wk": w[p + "attn_k"], "wv": w[p + "attn_v"], "wo": w[p + "attn_output"],
                       "gate_inp": w[p + "ffn_gate_inp"], "gate_exps": w[p + "ffn_gate_exps"],
                       "up_exps": w[p + "ffn_up_exps"], "down_exps": w[p + "ffn_down_exps"]})
    model = {"hp": hp, "tok_embd": w["token_embd"], "output": w["output"], "output_norm": w["output_norm"],
             "layers": layers, "rope_table": O.rope_table(n_ctx, hp["head_dim"], hp["freq_base"])}
    kvw = hp["n_head_kv"] * hp["head_dim"]
    cache = [(np.zeros((n_ctx, kvw), np.uint16), np.zeros((kvw, n_ctx), np.uint16)) for _ in range(hp["n_layer"])]
    return model, cache
