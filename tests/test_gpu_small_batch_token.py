"""mi355x_small_batch FUSED on a decoder: a step of three sequences on kq_rows_cols gives the
logits and the tokens of the per-node path, in fewer launches, and leaves the default as it was."""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch
from tests.test_gpu_plan import _llama, _timed

pytestmark = pytest.mark.gpu


def _args(stride=1):
    """Three sequences, each seeing its own first cell (cells 0, stride, 2 * stride) of 32."""
    mask = np.full((3, 32), -np.inf, np.float32)
    for s in range(3):
        mask[s, stride * s] = 0.0
    return ([1, 2, 3], [0, 0, 0], [0, stride, 2 * stride], mask, 32)


def _step(dev, mode):
    """One eager step_batch under `mode`: (logits, launch names); the selector restored."""
    import ggml_mi355x as g
    prev = g.small_batch(mode)
    try:
        b, dec = _llama(dev)
        dec.step_batch(*_args())
        b.synchronize()
        out = {}
        rows = _timed(lambda: out.setdefault("l", dec.step_batch(*_args(), use_graph=False)))
        logits = out["l"].cpu().numpy()
        b.close()
        return logits, [r[0] for r in rows]
    finally:
        g.small_batch(prev)


def test_step_batch_bits_and_launches(dev):
    import ggml_mi355x as g
    nodes, names_n = _step(dev, g.SMALL_BATCH_NODES)
    fused, names_f = _step(dev, g.SMALL_BATCH_FUSED)
    assert bits_equal(fused, nodes), first_mismatch(fused, nodes)
    assert any("kq_rows_cols" in n for n in names_f)
    assert not any("kq_gemv<" in n or n in ("kq::kq_quantize_q8K", "kq::kq_quantize") for n in names_f), names_f
    assert len(names_f) < len(names_n), (len(names_f), len(names_n))
    assert g.small_batch() == g.SMALL_BATCH_NODES
    assert _step(dev, g.SMALL_BATCH_NODES)[1] == names_n  # and the default plans what it planned


def test_generate_batch_graph_replays(dev):
    import ggml_mi355x as g
    toks = {}
    for mode in (g.SMALL_BATCH_NODES, g.SMALL_BATCH_FUSED):
        prev = g.small_batch(mode)
        try:
            b, dec = _llama(dev)
            # three steps in chunks of one: the captured graph is replayed twice after its first run
            tokens, pos, cells, mask, n_kv = _args(stride=8)
            toks[mode] = dec.generate_batch(tokens, pos, cells, mask, 3, n_kv, chunk=1, use_graph=True)
            b.close()
        finally:
            g.small_batch(prev)
    assert toks[g.SMALL_BATCH_FUSED] == toks[g.SMALL_BATCH_NODES] and all(len(s) == 3 for s in toks[g.SMALL_BATCH_FUSED])

