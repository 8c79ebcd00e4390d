"""CPU tests of the K-shift graph's lowering (mi355x_lower_ggml_graph, csrc/kq_lower.cpp kshift()):
llama.cpp's context-shift graph (llama-kv-cache build_graph_shift / build_rope_shift [U]: per layer
a VIEW [head_dim, n_head_kv, kv_size] of the f16 K cache and a ggml_rope_ext_inplace over it with
the I32 k_shift leaf) becomes one KV_SHIFT node a layer, any other f16 ROPE is refused, and the
decode graph lowers as before. Host only: no device is touched."""
import ctypes

import pytest

import ggml_mi355x as g
from ggml_mi355x.llama import hparams
from tests import ggml_graph as GG
from tests import test_lower as TL

HP = hparams(512, 2, 8, 2, 768, 1024)
N_CTX = 64
SHIFT = 0x5000  # the k_shift leaf's (fake) address


def kshift_graph(hp, dec, n_ctx, n_cells=None, delta_len=None, in_place=True, base=None, factors=False):
    """build_graph_shift for every layer of the decoder's caches."""
    G = GG.Graph()
    hd, nkv = hp["head_dim"], hp["n_head_kv"]
    n_cells = n_ctx if n_cells is None else n_cells
    shift = G.leaf(GG.I32, [n_cells if delta_len is None else delta_len], SHIFT, name="k_shift")
    ff = G.leaf(GG.F32, [hd // 2], 0x6000, name="rope_freqs") if factors else None
    for il in range(hp["n_layer"]):
        kc = G.leaf(GG.F16, [nkv * hd, n_ctx], dec.k_cache[il].data_ptr(), name=f"cache_k_l{il}")
        view = G.alias(g.GOP_VIEW, kc, [hd, nkv, n_cells])
        G.node(g.GOP_ROPE, GG.F16, [hd, nkv, n_cells], [view, shift] + ([ff] if factors else []),
               GG.rope_params(hd, hp["freq_base"] if base is None else base), view_src=kc,
               data=kc.data if in_place else None, name=f"k_shifted_l{il}")
    return G


def lower(G, dec, hp, n_ctx=N_CTX, **kw):
    return g.lower_ggml_graph(G.nodes, dec.table.data_ptr(), n_ctx, hp["freq_base"], **kw)


@pytest.mark.parametrize("n_cells", [N_CTX, 40])
def test_kshift_graph_lowers_to_one_node_a_layer(n_cells):
    wt, dec = TL._describe(HP, N_CTX)
    hd, nkv = HP["head_dim"], HP["n_head_kv"]
    for kw in (dict(), dict(cells_eq_pos=False), dict(cells_eq_pos=False, cells_from_graph=True)):
        rc, nodes, keep = lower(kshift_graph(HP, dec, N_CTX, n_cells), dec, HP, **kw)
        assert rc == 0 and len(nodes) == HP["n_layer"]
        for il, n in enumerate(nodes):
            assert n.op == g.OP_KV_SHIFT and n.type == g.TYPE_F16
            assert list(n.op_params)[:4] == [nkv, hd, g.KV_SHIFT_DELTAS, n_cells] == g.kv_shift_params(nkv, hd, n_cells=n_cells)
            kc, tab, dl = n.src[0].contents, n.src[2].contents, n.src[3].contents
            assert not n.src[1] and not n.src[4]  # no V cache: the K-shift leaves V alone
            assert n.data == kc.data == dec.k_cache[il].data_ptr()
            assert (tuple(n.ne), tuple(n.nb)) == (tuple(kc.ne), tuple(kc.nb)) == ((nkv * hd, N_CTX, 1, 1), (2, nkv * hd * 2) + (nkv * hd * 2 * N_CTX,) * 2)
            assert (tab.type, tab.ne[0], tab.ne[1], tab.nb[1], tab.data) == (g.TYPE_F32, hd, N_CTX, hd * 4, dec.table.data_ptr())
            assert (dl.type, dl.ne[0], dl.ne[1], dl.data) == (g.TYPE_I32, n_cells, 1, SHIFT)
            assert g.supports_op(n)
        assert ctypes.addressof(nodes[0].src[3].contents) == ctypes.addressof(nodes[1].src[3].contents)  # one delta leaf


def test_other_f16_ropes_are_refused_not_dropped():
    wt, dec = TL._describe(HP, N_CTX)
    ok = kshift_graph(HP, dec, N_CTX)
    assert lower(ok, dec, HP)[0] == 0
    for kw in (dict(factors=True), dict(base=500000.0), dict(in_place=False), dict(delta_len=N_CTX - 1),
               dict(delta_len=N_CTX + 1), dict(n_cells=N_CTX + 32)):
        rc, nodes, _ = lower(kshift_graph(HP, dec, N_CTX, **kw), dec, HP)
        assert rc == g.E_UNSUPPORTED and nodes == [], kw

    def mutated(mutate):
        G = kshift_graph(HP, dec, N_CTX)
        mutate([t for t in G.nodes if t.op == g.GOP_ROPE][1])
        return lower(G, dec, HP)[0]

    assert mutated(lambda r: None) == 0
    assert mutated(lambda r: r.op_params.__setitem__(2, 2)) == g.E_UNSUPPORTED                          # NEOX
    assert mutated(lambda r: r.op_params.__setitem__(1, HP["head_dim"] // 2)) == g.E_UNSUPPORTED       # n_dims
    assert mutated(lambda r: r.op_params.__setitem__(6, GG.f32_bits(0.5))) == g.E_UNSUPPORTED          # freq_scale
    assert mutated(lambda r: r.src[0].contents.nb.__setitem__(2, r.src[0].contents.nb[2] * 2)) == g.E_UNSUPPORTED
    assert mutated(lambda r: setattr(r.src[0].contents, "data", r.data + 1024)) == g.E_UNSUPPORTED     # not from cell 0
    f32_delta = GG.Graph().leaf(GG.F32, [N_CTX], SHIFT, name="k_shift")
    assert mutated(lambda r: r.src.__setitem__(1, ctypes.pointer(f32_delta))) == g.E_UNSUPPORTED
    # an f16 ROPE of the cache leaf itself (no [head_dim, n_head_kv, n_cells] view)
    G = GG.Graph()
    kc = G.leaf(GG.F16, [HP["n_head_kv"] * HP["head_dim"], N_CTX], dec.k_cache[0].data_ptr())
    G.node(g.GOP_ROPE, GG.F16, [HP["n_head_kv"] * HP["head_dim"], N_CTX], [kc, G.leaf(GG.I32, [N_CTX], SHIFT)],
           GG.rope_params(HP["head_dim"], HP["freq_base"]), view_src=kc, data=kc.data)
    assert lower(G, dec, HP)[0] == g.E_UNSUPPORTED
    # a table shorter than the cache, or none
    assert g.lower_ggml_graph(ok.nodes, dec.table.data_ptr(), N_CTX - 1, HP["freq_base"])[0] == g.E_UNSUPPORTED
    assert g.lower_ggml_graph(ok.nodes, None, N_CTX, HP["freq_base"])[0] == g.E_UNSUPPORTED
    assert g.lower_ggml_graph(ok.nodes, dec.table.data_ptr(), N_CTX, HP["freq_base"], arena_cap=3)[0] == g.E_WORKSPACE


def test_head_dim_128():
    hp = hparams(1024, 2, 8, 2, 1536, 512)
    wt, dec = TL._describe(hp, N_CTX)
    rc, nodes, _ = lower(kshift_graph(hp, dec, N_CTX), dec, hp)
    assert rc == 0 and [n.op for n in nodes] == [g.OP_KV_SHIFT] * 2 and nodes[0].op_params[1] == 128
    assert all(g.supports_op(n) for n in nodes)


@pytest.mark.parametrize("hp", [HP, hparams(1024, 2, 8, 2, 1536, 512)], ids=["small-gqa4", "hd128"])
def test_the_decode_graph_lowers_as_before(hp):
    """The f32 ROPE nodes of the attention blocks are untouched by the f16 case: the op sequence,
    shapes, parameters and operands of LlamaDecoder(backend=None), as tests/test_lower.py compares."""
    wt, dec = TL._describe(hp, N_CTX)
    G = GG.llama_decode_graph(hp, TL._leaves(hp, wt, dec), N_CTX)
    rc, nodes, keep = g.lower_ggml_graph(G.nodes, dec.table.data_ptr(), N_CTX, hp["freq_base"])
    assert rc == 0 and len(nodes) == len(dec.nodes) == 2 + 15 * hp["n_layer"] + 2
    assert g.OP_KV_SHIFT not in [n.op for n in nodes]
    for i, (a, b) in enumerate(zip(TL.canon(nodes), TL.canon(dec.nodes))):
        assert a == b, (i, a, b)
