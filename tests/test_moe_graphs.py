"""The node lists LlamaDecoder builds for a MoE model on a describe-only decoder (backend None): the MoE
arm of the one layer body in every graph, in upstream's order; and a dense hp still gives the recorded
node lists (tests/golden/llama_graphs.json through tests/llama_graph_sig.py), with or without the new
hparams arguments. Host only."""
import json
import os

import pytest
import torch

import ggml_mi355x as g
from ggml_mi355x.llama import LlamaDecoder, hparams
from ggml_mi355x.rowsplit import TokenSplit
from tests import llama_graph_sig as S
from tests import moe_model as MM

HP = hparams(256, 2, 4, 2, 256, 512, n_expert=4, n_expert_used=2)
N_CTX = 32
ATTN = [g.OP_RMS_NORM, g.OP_MUL, g.OP_MUL_MAT, g.OP_MUL_MAT, g.OP_MUL_MAT]
MOE = [g.OP_RMS_NORM, g.OP_MUL, g.OP_MOE_ROUTE, g.OP_MUL_MAT_ID, g.OP_MUL_MAT_ID, g.OP_SWIGLU, g.OP_MUL_MAT_ID,
       g.OP_MOE_COMBINE, g.OP_ADD]
HEAD = [g.OP_RMS_NORM, g.OP_MUL, g.OP_MUL_MAT]


@pytest.fixture(scope="module")
def weights():
    w = MM.build(HP, 0)
    return {k: ((v[0], torch.from_numpy(v[1])) if isinstance(v, tuple) else torch.from_numpy(v)) for k, v in w.items()}


def _src(n, i):
    return n.src[i].contents


def _check_moe(nodes, first, T, weights, layer):
    """nodes[first:] start with ffn_norm's RMS_NORM of `layer`."""
    E, F, ne, nu = HP["n_embd"], HP["n_ff"], HP["n_expert"], HP["n_expert_used"]
    norm, m2, route, up, gate, glu, down, comb, add = nodes[first:first + 9]
    assert [n.op for n in nodes[first:first + 9]] == MOE
    p = f"blk.{layer}."
    assert list(route.ne) == [2 * nu, T, 1, 1] and route.type == g.TYPE_I32 and list(route.op_params)[:1] == [nu]
    gi = _src(route, 0)
    assert gi.data == weights[p + "ffn_gate_inp"].data_ptr() and list(gi.ne)[:2] == [E, ne] and gi.type == g.TYPE_F32
    assert _src(route, 1).data == m2.data
    for n, name, K, N, ne11 in ((up, "ffn_up_exps", E, F, 1), (gate, "ffn_gate_exps", E, F, 1),
                                (down, "ffn_down_exps", F, E, nu)):
        t, w = weights[p + name]
        wt, x, rt = _src(n, 0), _src(n, 1), _src(n, 2)
        assert wt.type == t and wt.data == w.data_ptr() and list(wt.ne) == [K, N, ne, 1]
        assert (wt.nb[1], wt.nb[2]) == (w.stride(1), w.stride(0))
        assert rt.data == route.data and rt.op == g.OP_MOE_ROUTE
        assert list(n.ne) == [N, nu, T, 1] and (n.nb[1], n.nb[2]) == (4 * N, 4 * N * nu)
        assert list(x.ne) == [K, ne11, T, 1] and (x.nb[1], x.nb[2]) == (4 * K, 4 * K * ne11)
    assert _src(up, 1).data == m2.data and _src(down, 1).data == glu.data
    assert _src(glu, 0).data == gate.data and _src(glu, 1).data == up.data and list(glu.ne) == [F, nu, T, 1]
    assert _src(comb, 0).data == down.data and _src(comb, 1).data == route.data and list(comb.ne) == [E, T, 1, 1]
    assert _src(add, 0).data == comb.data and list(add.ne) == [E, T, 1, 1]
    for n in (route, up, gate, glu, down, comb, add):
        assert g.supports_op(n), n.op


def test_token_graph_has_the_moe_arm(weights):
    dec = LlamaDecoder(None, HP, weights, N_CTX)
    ops = [n.op for n in dec.nodes]
    layer = ATTN + [g.OP_ATTN_DECODE, g.OP_MUL_MAT, g.OP_ADD] + MOE
    assert ops == [g.OP_GET_ROWS] + layer * 2 + HEAD
    for li in range(2):
        _check_moe(dec.nodes, 1 + li * len(layer) + 8, 1, weights, li)
    assert all(g.supports_op(n) for n in dec.nodes if n.op in (g.OP_MOE_ROUTE, g.OP_MUL_MAT_ID, g.OP_MOE_COMBINE, g.OP_SWIGLU))


def test_prompt_and_batch_graphs_have_the_moe_arm(weights):
    dec = LlamaDecoder(None, HP, weights, N_CTX)
    pg = dec._prompt_graph(5)
    ops = [n.op for n in pg["nodes"]]
    layer = ATTN + [g.OP_ATTN_DECODE, g.OP_MUL_MAT, g.OP_ADD] + MOE
    last = ATTN + [g.OP_ATTN_DECODE, g.OP_MUL_MAT, g.OP_GET_ROWS, g.OP_GET_ROWS, g.OP_ADD] + MOE
    assert ops == [g.OP_GET_ROWS] + layer + last + HEAD
    _check_moe(pg["nodes"], 1 + 8, 5, weights, 0)
    _check_moe(pg["nodes"], 1 + len(layer) + 10, 1, weights, 1)  # inp_out_ids: the last layer's FFN over one row
    bg = dec._batch_graph(3, 32)
    layer_b = ATTN + [g.OP_ATTN_BATCH, g.OP_MUL_MAT, g.OP_ADD] + MOE
    assert [n.op for n in bg["nodes"]] == [g.OP_GET_ROWS] + layer_b * 2 + HEAD
    _check_moe(bg["nodes"], 1 + 8, 3, weights, 0)
    lg = dec._prompt_graph(4, all_rows=True)
    assert [n.op for n in lg["nodes"]] == [g.OP_GET_ROWS] + layer * 2 + HEAD + [g.OP_LOGPROB_BATCH]


def test_moe_refuses_a_row_split(weights):
    dense = hparams(512, 2, 8, 2, 768, 1024)
    split = TokenSplit(dense, 2, 0, "gather")
    with pytest.raises(g.Mi355xError):
        LlamaDecoder(None, dict(dense, n_expert=4, n_expert_used=2), weights, N_CTX, split=split)
    with pytest.raises(g.Mi355xError):
        hparams(256, 2, 4, 2, 256, 512, n_expert=4, n_expert_used=5)


def test_dense_node_lists_are_the_recorded_ones():
    """n_expert == 0, given or not: the dict and every node list of before."""
    assert hparams(512, 2, 8, 2, 768, 1024, n_expert=0, n_expert_used=0) == S.HP
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llama_graphs.json")) as f:
        golden = json.load(f)
    built = S.graphs()
    assert sorted(built) == sorted(golden)
    for name in ("token.row", "token.table", "prompt.1", "prompt.5", "batch.3.32"):
        assert built[name]["nodes"] == golden[name]["nodes"], name
    # an hp dict with the MoE keys present but zero takes the dense arm too
    wt = S._weights()
    a = LlamaDecoder(None, S.HP, wt, S.N_CTX)
    b = LlamaDecoder(None, dict(S.HP, n_expert=0, n_expert_used=0), wt, S.N_CTX)
    sa = S.signature(a.nodes, S.owners(a, a.inp, a.nodes))
    sb = S.signature(b.nodes, S.owners(b, b.inp, b.nodes))
    assert sa == sb == golden["token.row"]["nodes"]
