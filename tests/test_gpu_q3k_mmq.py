"""Q3_K prompts on the int8 matrix cores (kq_mmq's Q3_K body) against tests/q3k_ref.py, by bits: every
instantiated tile shape, the selector q3k_prefill, and a 65-token LlamaDecoder prompt under the default."""
import numpy as np
import pytest

from tests import q3k_ref as R
from tests.test_gpu_parity import bits_equal, first_mismatch, t
from tests.test_gpu_q3k import Q3, Q4, _at, _case
from tests.test_gpu_rows_cols import _timed

pytestmark = pytest.mark.gpu
MMQ = ["kq::kq_quantize_q8L", "kq::kq_mmq<11>"]


def _run(dev, K, N, M, offset=0):
    import ggml_mi355x as g
    w, x, _, ref = _case(K, N, 130)
    got, names = _timed(lambda: g.mul_mat(Q3, _at(dev, w, offset), K, t(x[:M], dev)).cpu().numpy())
    assert bits_equal(got, ref[:M]), first_mismatch(got, ref[:M])
    return names


# K: one superblock (no second buffer) / an odd block count (rows at every even offset in their granules, both
# buffers reused). N: every lane's row clamped / a wave with one live row / past a 64-row / a 128-row tile.
# M: the floor / a partial column tile / a second tile of one column / past a 128-column tile.
@pytest.mark.parametrize("K,N,M,offset", [(256, 1, 16, 0), (256, 33, 33, 2), (768, 67, 65, 0), (768, 130, 130, 2)])
@pytest.mark.parametrize("tile", ["MMQ_TILE64", "MMQ_TILE128", "MMQ_TILE128W"])
def test_mmq_tiles(dev, tile, K, N, M, offset):
    import ggml_mi355x as g
    prev, prev_tile = g.q3k_prefill(g.Q3K_PREFILL_MMQ), g.mmq_impl(getattr(g, tile))
    try:
        assert _run(dev, K, N, M, offset) == MMQ
    finally:
        g.mmq_impl(prev_tile)
        g.q3k_prefill(prev)


def test_selector(dev):
    import ggml_mi355x as g
    assert "kq_gemv_q3k" in _run(dev, 768, 67, 63)[-1] and _run(dev, 768, 67, 64) == MMQ  # AUTO: from 64 columns
    prev = g.q3k_prefill(g.Q3K_PREFILL_GEMV)
    try:
        assert prev == g.Q3K_PREFILL_AUTO and "kq_gemv_q3k" in _run(dev, 768, 67, 64)[-1]
    finally:
        g.q3k_prefill(prev)


def test_llama_decoder_prompt_65(dev):
    """test_llama_decoder_q3_k_m_mix's model: a 65-token prompt from position 0 under the default selector."""
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    hp, n_ctx = hparams(256, 2, 4, 2, 512, 512), 96
    w, rng = LM.build(hp, 7), np.random.default_rng(11)
    mix = {"token_embd": Q3, "output": 14, "attn_q": Q3, "attn_k": Q3, "ffn_gate": Q3, "ffn_up": Q3, "attn_v": 13,
           "attn_output": Q4, "ffn_down": Q4}
    for name, (_, old) in [(k, v) for k, v in w.items() if isinstance(v, tuple)]:
        ty, K = mix[name.split(".")[-1]], hp["n_ff"] if name.endswith("ffn_down") else hp["n_embd"]
        w[name] = (ty, R.weights(rng, old.shape[0], K) if ty == Q3 else LM.kquant(rng, ty, old.shape[0], K, edges=True))
    b = g.Backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), n_ctx)
    tokens = np.random.default_rng(2).integers(0, 512, size=65).tolist()
    got, names = _timed(lambda: (dec.prompt(tokens, 0, use_graph=False), b.synchronize())[0].cpu().numpy().reshape(-1))
    model, cache = LM.oracle_model(hp, w, n_ctx)
    for pos, tok in enumerate(tokens):
        ref = R.decode_token(model, tok, pos, cache)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert "kq::kq_mmq<11>" in names, names
    b.close()
