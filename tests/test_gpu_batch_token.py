"""GPU: three sequences decoded together, one token each per step, through the ATTN_BATCH node —
(a) llm_build_llama's ubatch graph with T outputs (tests/ggml_graph_batch.py) lowered with
cells_from_graph and run by graph_compute(use_graph=True), so the steps after the first are
hipGraph replays with new input contents on the same pointers, and (b) LlamaDecoder.step_batch —
against the oracle decoding each sequence alone.

Why the bits must be equal. Sequence s owns the cells [32 s, 32 s + 32) in order: the token at
position p sits at cell 32 s + p and its mask row shows the cells 32 s .. 32 s + p. The oracle's
token of that sequence alone (O.decode_token on the sequence's own cache) runs its row over the
cells [0, 32) of that cache; the batch runs it over [0, n_kv = 128) of the shared cache, where the
other sequences' cells are whole 32-aligned blocks of masked cells: their scores are -INF, their
weights exact +0, so they add 0.0 to the soft_max's double sum and leave every f16 KQV
accumulator as it is. The sequence's own cells keep their place inside the groups of four and
their accumulator lane (cell % 32), since the shift 32 s is a whole number of blocks. Hence each
row of the batch equals O.decode_token of its sequence bit for bit, and so do the GEMMs' rows
(each column of a batched MUL_MAT is its own GEMV chain). Interleaved layouts, where that
argument does not hold, are covered at op level (tests/test_gpu_attn_batch.py)."""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, N_SEQ, STEPS = 128, 3, 4
TOKENS = [[7, 1000, 7, 123], [511, 3, 900, 64], [2, 2, 777, 1023]]  # [sequence][step]


def step_inputs(step):
    """Tokens, positions, cells and the [T, n_ctx] mask of one step (every sequence at position `step`)."""
    tok = [TOKENS[s][step] for s in range(N_SEQ)]
    pos = [step] * N_SEQ
    cells = [32 * s + step for s in range(N_SEQ)]
    mask = np.full((N_SEQ, N_CTX), -np.inf, np.float32)
    for s in range(N_SEQ):
        mask[s, 32 * s:32 * s + step + 1] = 0.0
    return tok, pos, cells, mask


@pytest.fixture(scope="module")
def model():
    """The 2-layer model (width 512: head_dim 64, 4 query heads per KV head) and the oracle's
    logits [step][sequence], each sequence decoded alone on its own cache."""
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    from ggml_mi355x.llama import hparams
    O.lib()
    hp = hparams(512, 2, 8, 2, 768, 1024)
    w = LM.build(hp, 77)
    ref = [[None] * N_SEQ for _ in range(STEPS)]
    for s in range(N_SEQ):
        om, cache = LM.oracle_model(hp, w, 32)
        for p in range(STEPS):
            ref[p][s], _ = O.decode_token(om, TOKENS[s][p], p, cache)
    return hp, w, ref


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_step_batch_equals_each_sequence_alone(dev, model, fuse):
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    hp, w, ref = model
    b = g.Backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), N_CTX, fuse=fuse)
    for step in range(STEPS):
        tok, pos, cells, mask = step_inputs(step)
        lg = dec.step_batch(tok, pos, cells, mask, N_CTX)
        b.synchronize()
        got = lg.cpu().numpy()
        assert got.shape == (N_SEQ, hp["n_vocab"])
        for s in range(N_SEQ):
            assert bits_equal(got[s], ref[step][s]), (step, s, first_mismatch(got[s], ref[step][s]))
    assert len(dec._batches) == 1  # one graph per (T, n_kv), replayed
    b.close()


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_lowered_batch_graph_replays_bit_exact(dev, model, fuse):
    import torch
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder
    from tests import ggml_graph as GG
    from tests import llama_model as LM
    from tests.ggml_graph_batch import llama_batch_graph
    from tests.test_lower import _leaves
    hp, w, ref = model
    T, kvw = N_SEQ, hp["n_head_kv"] * hp["head_dim"]
    b = g.Backend()
    wd = LM.to_device(w, dev)
    dec = LlamaDecoder(b, hp, wd, N_CTX, fuse=fuse, rope_src="table")  # device leaves: weights, caches, table
    bufs = []

    def alloc(nbytes):
        x = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        bufs.append(x)
        return x.data_ptr()

    # the graph's inputs, each a device buffer of its own written before every step
    inp = {"inp_tokens": torch.zeros(T, dtype=torch.int32, device=dev),
           "inp_pos": torch.zeros(T, dtype=torch.int32, device=dev),
           "k_idxs": torch.zeros(T, dtype=torch.int64, device=dev),
           "v_idxs": torch.zeros(kvw * T, dtype=torch.int64, device=dev),
           "kq_mask": torch.zeros((T, N_CTX), dtype=torch.float16, device=dev)}
    L = _leaves(hp, wd, dec)
    L.update({k: v.data_ptr() for k, v in inp.items()})
    G = llama_batch_graph(hp, L, N_CTX, T, alloc=alloc, mask_type=GG.F16)
    assert g.lower_ggml_graph(G.nodes, dec.table.data_ptr(), N_CTX, hp["freq_base"], cells_eq_pos=False)[0] == \
        g.E_UNSUPPORTED
    rc, nodes, keep = g.lower_ggml_graph(G.nodes, dec.table.data_ptr(), N_CTX, hp["freq_base"], cells_eq_pos=False,
                                         cells_from_graph=True)
    assert rc == 0 and [n.op for n in nodes].count(g.OP_ATTN_BATCH) == hp["n_layer"]
    out = next(x for x in bufs if x.data_ptr() == G.nodes[-1].data)
    torch.cuda.synchronize()
    for step in range(STEPS):
        tok, pos, cells, mask = step_inputs(step)
        v_idxs = (np.arange(kvw, dtype=np.int64)[None, :] * N_CTX + np.asarray(cells, np.int64)[:, None]).ravel()
        b.set_tensor(inp["inp_tokens"].data_ptr(), np.asarray(tok, np.int32))
        b.set_tensor(inp["inp_pos"].data_ptr(), np.asarray(pos, np.int32))
        b.set_tensor(inp["k_idxs"].data_ptr(), np.asarray(cells, np.int64))
        b.set_tensor(inp["v_idxs"].data_ptr(), v_idxs)
        b.set_tensor(inp["kq_mask"].data_ptr(), mask.astype(np.float16))
        assert b.graph_compute(nodes, use_graph=True) == 0
        b.synchronize()
        got = out[:T * hp["n_vocab"]].cpu().numpy().reshape(T, hp["n_vocab"])
        for s in range(N_SEQ):
            assert bits_equal(got[s], ref[step][s]), (step, s, first_mismatch(got[s], ref[step][s]))
    b.close()
