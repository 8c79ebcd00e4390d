"""A tiny MoE llama GGUF file (Mixtral's tensor names, 3-D expert tensors) through the native reader:
the expert tensors keep their bytes and their [n_expert, rows, row bytes] shape, and the model loader's
hparams carry llama.expert_count / llama.expert_used_count. No device."""
import numpy as np

from oracle import kq_oracle_np as N
from tests import gguf_writer as G

E, FF, KV, V, NE, NU = 256, 512, 128, 512, 4, 2


def _write(path, rng, moe=True):
    kv = [("general.architecture", G.STRING, "llama"), ("llama.block_count", G.U32, 1), ("llama.embedding_length", G.U32, E),
          ("llama.feed_forward_length", G.U32, FF), ("llama.attention.head_count", G.U32, E // 64),
          ("llama.attention.head_count_kv", G.U32, KV // 64), ("llama.attention.layer_norm_rms_epsilon", G.F32, 1e-5),
          ("llama.rope.freq_base", G.F32, 1e6)]
    if moe:
        kv += [("llama.expert_count", G.U32, NE), ("llama.expert_used_count", G.U32, NU)]
    spec = [("token_embd.weight", 12, (E, V)), ("blk.0.attn_norm.weight", 0, (E,)), ("blk.0.attn_q.weight", 12, (E, E)),
            ("blk.0.attn_k.weight", 12, (E, KV)), ("blk.0.attn_v.weight", 14, (E, KV)), ("blk.0.attn_output.weight", 12, (E, E)),
            ("blk.0.ffn_norm.weight", 0, (E,)), ("blk.0.ffn_gate_inp.weight", 0, (E, NE)),
            ("blk.0.ffn_gate_exps.weight", 12, (E, FF, NE)), ("blk.0.ffn_up_exps.weight", 12, (E, FF, NE)),
            ("blk.0.ffn_down_exps.weight", 14, (FF, E, NE)), ("output_norm.weight", 0, (E,)), ("output.weight", 14, (E, V))]
    tensors, out = [], {}
    for name, gt, ne in spec:
        rows = int(np.prod(ne[1:])) if len(ne) > 1 else 1
        if gt == 0:
            data = np.frombuffer(rng.standard_normal(ne[0] * rows).astype(np.float32).tobytes(), np.uint8)
        else:
            data = N.random_blocks(rng, gt, rows, ne[0]).reshape(-1)
        tensors.append((name, gt, ne, data))
        out[name] = (gt, ne, data)
    G.write_gguf(path, kv, tensors)
    return out


def test_moe_gguf_round_trip(tmp_path):
    from ggml_mi355x.gguf import GGUFFile
    from ggml_mi355x.llama import LAYER_MATS, MOE_LAYER_MATS, MOE_ROUTER, gguf_hparams, layer_mats
    rng = np.random.default_rng(7)
    path = tmp_path / "moe.gguf"
    want = _write(path, rng)
    with GGUFFile(path) as f:
        hp = gguf_hparams(f)
        assert hp["n_expert"] == NE and hp["n_expert_used"] == NU
        assert (hp["n_embd"], hp["n_layer"], hp["n_head"], hp["n_head_kv"], hp["n_ff"], hp["n_vocab"]) == (E, 1, 4, 2, FF, V)
        assert hp["freq_base"] == 1e6
        assert layer_mats(hp) == MOE_LAYER_MATS and MOE_LAYER_MATS[:4] == LAYER_MATS[:4]
        for name in layer_mats(hp) + (MOE_ROUTER,):
            assert f"blk.0.{name}.weight" in f.tensors, name
        for name, (gt, ne, data) in want.items():
            info = f.tensors[name]
            assert info["type"] == gt and info["ne"] == tuple(ne) and info["n_dims"] == len(ne), name
            assert (f.bytes(name) == data).all(), name
        # the experts keep three dimensions: [n_expert, rows, row bytes], expert e's matrix a contiguous slab
        assert f.shape_bytes("blk.0.ffn_up_exps.weight") == (NE, FF, E // 256 * 144)
        assert f.shape_bytes("blk.0.ffn_down_exps.weight") == (NE, E, FF // 256 * 210)
        assert f.shape_bytes("blk.0.attn_q.weight") == (E, E // 256 * 144)
        assert f.shape_bytes("blk.0.ffn_gate_inp.weight") == (NE, E * 4)
        up = f.bytes("blk.0.ffn_up_exps.weight").reshape(f.shape_bytes("blk.0.ffn_up_exps.weight"))
        src = want["blk.0.ffn_up_exps.weight"][2].reshape(NE * FF, -1)
        for e in range(NE):
            assert (up[e] == src[e * FF:(e + 1) * FF]).all()


def test_dense_gguf_has_no_moe_keys(tmp_path):
    from ggml_mi355x.gguf import GGUFFile
    from ggml_mi355x.llama import LAYER_MATS, gguf_hparams, hparams, layer_mats
    path = tmp_path / "dense.gguf"
    _write(path, np.random.default_rng(8), moe=False)
    with GGUFFile(path) as f:
        hp = gguf_hparams(f)
    assert "n_expert" not in hp and layer_mats(hp) == LAYER_MATS
    assert hp == hparams(E, 1, 4, 2, FF, V, eps=hp["eps"], freq_base=1e6)
    assert hparams(E, 1, 4, 2, FF, V, n_expert=0, n_expert_used=0) == hparams(E, 1, 4, 2, FF, V)
