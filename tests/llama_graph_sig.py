"""Pointer-free signatures of the node lists LlamaDecoder builds (tests/test_llama_graphs.py).

tests/test_lower.py's canon() with the raw address of a leaf replaced by the storage it
points into: per node (op, ne, op_params, flags, operands), an operand being the index of
the node that produces it or, for a leaf, (type, ne0, ne1, nb1, owner, byte offset). owner
is a weight's key, k_cache.i / v_cache.i, table, inp (the graph's input block) or buf.j
(node j's output buffer, which a row split's residual views read). Host only: the decoders
are describe-only (backend None, CPU tensors)."""
import ctypes
import json

import torch

import ggml_mi355x as g
from ggml_mi355x.llama import LlamaDecoder, hparams
from ggml_mi355x.rowsplit import TokenSplit
from tests import llama_model as LM

HP = hparams(512, 2, 8, 2, 768, 1024)
N_CTX = 64


def _span(t):
    return t.data_ptr(), t.numel() * t.element_size()


def owners(dec, inp, nodes):
    """(name, first byte, bytes) of every storage a leaf of `nodes` may point into."""
    out = []
    for k, v in dec.w.items():
        out.append((k,) + _span(v[1] if isinstance(v, tuple) else v))
    for i, (kc, vc) in enumerate(zip(dec.k_cache, dec.v_cache)):
        out.append((f"k_cache.{i}",) + _span(kc))
        out.append((f"v_cache.{i}",) + _span(vc))
    out.append(("table",) + _span(dec.table))
    out.append(("inp",) + _span(inp))
    for j, n in enumerate(nodes):  # every node's output is f32 [ne1, ne0]
        out.append((f"buf.{j}", n.data, 4 * n.ne[0] * n.ne[1]))
    return out


def _owner(own, addr):
    hits = [(name, addr - lo) for name, lo, size in own if lo <= addr < lo + size]
    assert len(hits) == 1, (addr, hits)
    return hits[0]


def signature(nodes, own):
    """One canonical line (a JSON list) per node."""
    idx = {ctypes.addressof(n): i for i, n in enumerate(nodes)}
    out = []
    for n in nodes:
        srcs = []
        for s in range(g.MAX_SRC):
            if not n.src[s]:
                break
            t = n.src[s].contents
            a = ctypes.addressof(t)
            srcs.append(idx[a] if a in idx else [t.type, t.ne[0], t.ne[1], t.nb[1], *_owner(own, t.data)])
        out.append(json.dumps([n.op, list(n.ne), list(n.op_params), n.flags, srcs], separators=(",", ":")))
    return out


def _weights():
    w = LM.build(HP, 0)
    return {k: ((v[0], torch.from_numpy(v[1])) if isinstance(v, tuple) else torch.from_numpy(v)) for k, v in w.items()}


def _node_of(nodes, buf):
    """Index of the node whose output buffer `buf` is."""
    hits = [j for j, n in enumerate(nodes) if n.data == buf.data_ptr()]
    assert len(hits) == 1, hits
    return hits[0]


def graphs():
    """name -> {"nodes": signature} of every graph a describe-only decoder builds; a split decoder's
    entry also has the node index behind every entry of dec.gathers and dec.reduces."""
    wt = _weights()
    out = {}
    for rope_src in ("row", "table"):
        dec = LlamaDecoder(None, HP, wt, N_CTX, rope_src=rope_src)
        out[f"token.{rope_src}"] = dict(nodes=signature(dec.nodes, owners(dec, dec.inp, dec.nodes)))
    for mode in ("gather", "reduce"):
        for r in (0, 1):
            split = TokenSplit(HP, 2, r, mode)
            dec = LlamaDecoder(None, HP, split.slice_weights(wt), N_CTX, split=split)
            out[f"split.{mode}.{r}"] = dict(
                nodes=signature(dec.nodes, owners(dec, dec.inp, dec.nodes)),
                gathers=[_node_of(dec.nodes, b) for b in dec.gathers],
                reduces=[[_node_of(dec.nodes, a), _node_of(dec.nodes, b)] for a, b in dec.reduces])
    dec = LlamaDecoder(None, HP, wt, N_CTX)
    for n_tok in (1, 5):
        pg = dec._prompt_graph(n_tok)
        out[f"prompt.{n_tok}"] = dict(nodes=signature(pg["nodes"], owners(dec, pg["inp"], pg["nodes"])))
    bg = dec._batch_graph(3, 32)
    out["batch.3.32"] = dict(nodes=signature(bg["nodes"], owners(dec, bg["inp"], bg["nodes"])))
    return out
