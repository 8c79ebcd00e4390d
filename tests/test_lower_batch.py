"""CPU tests of the lowering's cells_from_graph option (mi355x_lower_opts, csrc/kq_lower.cpp):
llm_build_llama's graph (tests/ggml_graph.py) of 1 and 3 tokens lowers to one ATTN_BATCH node per
layer that takes the K store's cell indices and the soft_max mask from the graph; cells_eq_pos
keeps precedence, neither flag refuses as before, and what ATTN_BATCH cannot express is refused.
Host only: no device is touched."""
import ctypes

import pytest

import ggml_mi355x as g
from ggml_mi355x.llama import hparams
from tests import ggml_graph as GG
from tests.test_lower import _describe, _leaves

HP = hparams(512, 2, 8, 2, 768, 1024)
N_CTX = 64


def build(n_tokens, n_ctx=N_CTX):
    wt, dec = _describe(HP, n_ctx)
    L = _leaves(HP, wt, dec)
    L["k_idxs"], L["v_idxs"], L["kq_mask"], L["inp_out_ids"] = 0x1000, 0x2000, 0x3000, 0x4000
    G = GG.llama_decode_graph(HP, L, n_ctx, n_tokens=n_tokens)
    return G, dec, (wt, L)


def lower(G, dec, **kw):
    return g.lower_ggml_graph(G.nodes, dec.table.data_ptr(), N_CTX, HP["freq_base"], **kw)


def nodes_of(G, op):
    return [t for t in G.nodes if t.op == op]


@pytest.mark.parametrize("n_tokens", [1, 3])
def test_cells_from_graph_lowers_to_attn_batch(n_tokens):
    G, dec, keep = build(n_tokens)
    rc, nodes, arena = lower(G, dec, cells_eq_pos=False, cells_from_graph=True)
    assert rc == 0
    ops = [n.op for n in nodes]
    assert ops.count(g.OP_ATTN_BATCH) == HP["n_layer"] and g.OP_ATTN_DECODE not in ops
    k_idxs = next(t for t in G.keep if t.name == b"k_idxs")
    mask = next(t for t in G.keep if t.name == b"kq_mask")
    hd, nh, nkv = HP["head_dim"], HP["n_head"], HP["n_head_kv"]
    for n in nodes:
        if n.op != g.OP_ATTN_BATCH:
            continue
        cells, m = n.src[7].contents, n.src[8].contents
        assert cells.data == k_idxs.data == 0x1000 and cells.type == GG.I64 and cells.ne[0] == n_tokens
        assert m.data == mask.data == 0x3000 and m.type == GG.F16 and m.nb[1] == mask.nb[1]
        assert tuple(n.op_params[:5]) == (nh, nkv, hd, GG.f32_bits(1.0 / 8.0), N_CTX)
        assert n.ne[0] == nh * hd and n.ne[1] == n_tokens
        assert n.src[3].contents.data == dec.pos.data_ptr()
        assert n.src[6].contents.data == dec.table.data_ptr() and not n.src[9]
        assert g.supports_op(n)
    assert all(g.supports_op(n) for n in nodes)
    # the rest of the graph is the node list the cells_eq_pos lowering gives
    rc2, nodes2, arena2 = lower(G, dec)
    assert rc2 == 0 and [n.op for n in nodes2] == [g.OP_ATTN_DECODE if o == g.OP_ATTN_BATCH else o for o in ops]


@pytest.mark.parametrize("n_tokens", [1, 3])
def test_cells_eq_pos_takes_precedence_and_no_flag_refuses(n_tokens):
    G, dec, keep = build(n_tokens)
    rc, nodes, arena = lower(G, dec, cells_eq_pos=True, cells_from_graph=True)
    ops = [n.op for n in nodes]
    assert rc == 0 and ops.count(g.OP_ATTN_DECODE) == HP["n_layer"] and g.OP_ATTN_BATCH not in ops
    assert lower(G, dec, cells_eq_pos=False, cells_from_graph=False)[0] == g.E_UNSUPPORTED
    assert lower(G, dec, cells_eq_pos=False)[0] == g.E_UNSUPPORTED


@pytest.mark.parametrize("n_tokens", [1, 3])
def test_cells_from_graph_refuses_what_attn_batch_cannot_express(n_tokens):
    def rc_of(mutate):
        G, dec, keep = build(n_tokens)
        extra = mutate(G)
        return lower(G, dec, cells_eq_pos=False, cells_from_graph=True)[0], extra

    assert rc_of(lambda G: None)[0] == 0
    kvw = HP["n_head_kv"] * HP["head_dim"]

    # a mask leaf of type I32
    def i32_mask(G):
        m = GG.Graph().leaf(GG.I32, [N_CTX, n_tokens], 0x3000, name="kq_mask")
        for sm in nodes_of(G, g.GOP_SOFT_MAX):
            sm.src[1] = ctypes.pointer(m)
        return m

    assert rc_of(i32_mask)[0] == g.E_UNSUPPORTED

    # a v_idxs of the wrong length
    def short_v(G):
        v = GG.Graph().leaf(GG.I64, [kvw * n_tokens - 1], 0x2000, name="v_idxs")
        for st in nodes_of(G, g.GOP_SET_ROWS)[1::2]:
            st.src[1] = ctypes.pointer(v)
        return v

    assert rc_of(short_v)[0] == g.E_UNSUPPORTED

    # a shifted K view
    def shift_view(G):
        kq = next(t for t in G.nodes if t.op == g.GOP_MUL_MAT and t.name == b"kq")
        kq.src[0].contents.view_offs = 64

    assert rc_of(shift_view)[0] == g.E_UNSUPPORTED

    # a K view of 40 cells (alone, and with the V view following it): not whole 32-cell blocks
    def k40(G):
        kq = next(t for t in G.nodes if t.op == g.GOP_MUL_MAT and t.name == b"kq")
        kq.src[0].contents.ne[1] = 40

    def kv40(G):
        k40(G)
        kqv = next(t for t in G.nodes if t.op == g.GOP_MUL_MAT and t.name == b"kqv")
        kqv.src[0].contents.ne[0] = 40

    assert rc_of(k40)[0] == g.E_UNSUPPORTED
    assert rc_of(kv40)[0] == g.E_UNSUPPORTED

    # views of 32 cells (a prefix of the cache) are taken: n_kv = 32
    def kv32(G):
        for name, d in ((b"kq", 1), (b"kqv", 0)):
            for t in G.nodes:
                if t.op == g.GOP_MUL_MAT and t.name == name:
                    t.src[0].contents.ne[d] = 32

    G, dec, keep = build(n_tokens)
    kv32(G)
    rc, nodes, arena = lower(G, dec, cells_eq_pos=False, cells_from_graph=True)
    assert rc == 0 and all(n.op_params[4] == 32 for n in nodes if n.op == g.OP_ATTN_BATCH)
