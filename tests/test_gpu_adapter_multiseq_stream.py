"""GPU: the multi-sequence and the long-context option of the ggml-backend registration together
(ggml_backend_mi355x_set_multi_seq + ggml_backend_mi355x_set_long_context,
adapter/ggml-mi355x.cpp) through the harness tests/adapter/multiseq_longctx_test.cpp (prebuilt by
__graft_entry__.build()): a graph whose KQ mask hides a cell inside [0, pos], over a cache of
8224 cells, is refused with long-context off and computes with both options on — its ATTN_BATCH
nodes on the streamed kernels — the logits LlamaDecoder.step_batch gives for the same inputs under
mi355x_attn_stream mode 1."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "adapter", "bin", "multiseq_longctx_test")
N_CTX = 8224
TOKENS = [7, 1000, 123, 1]
POSITIONS = [2, 3, 8191, 8223]  # each >= 2: cell 1 is the hidden one


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from tests.test_adapter import glue_inputs
    from ggml_mi355x.llama import hparams
    hp = hparams(512, 2, 8, 2, 768, 1024)
    argv, w = glue_inputs(tmp_path_factory.mktemp("multiseq_longctx"), hp, N_CTX, 43, TOKENS)
    return hp, argv, w


@pytest.fixture
def stream_mode():
    """Sets mi355x_attn_stream for one test and puts the previous mode back."""
    import ggml_mi355x as g
    prev = []

    def set_mode(mode):
        p = g.attn_stream(mode)
        assert p >= 0
        if not prev:
            prev.append(p)
    yield set_mode
    if prev:
        g.attn_stream(prev[0])


def test_hidden_cell_graph_over_a_long_cache_is_refused_with_long_context_off(dev, files):
    hp, argv, w = files
    assert os.path.exists(HARNESS), "tests/adapter/bin/multiseq_longctx_test missing: run __graft_entry__.build()"
    r = subprocess.run([HARNESS] + argv + ["off", ",".join(map(str, POSITIONS))], capture_output=True, text=True,
                       timeout=200)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "refused -1" in r.stdout and "hidden" not in r.stdout


def test_hidden_cell_graph_over_a_long_cache_computes_with_both_options_on(dev, files, stream_mode):
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    hp, argv, w = files
    assert os.path.exists(HARNESS), "tests/adapter/bin/multiseq_longctx_test missing: run __graft_entry__.build()"
    r = subprocess.run([HARNESS] + argv + ["on", ",".join(map(str, POSITIONS))], capture_output=True, text=True,
                       timeout=200)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("hidden") == len(TOKENS) and "refused" not in r.stdout
    got = np.fromfile(argv[3], np.float32).reshape(len(TOKENS), hp["n_vocab"])
    # the Python path on the same inputs: each token at cell == position with cell 1 hidden
    stream_mode(1)
    assert g.attn_batch_path(N_CTX, hp["n_head"], hp["n_head_kv"], hp["head_dim"], N_CTX) == g.ATTN_PATH_STREAM
    b = g.Backend()
    try:
        dec = LlamaDecoder(b, hp, LM.to_device(w, dev), N_CTX)
        for i, (tok, p) in enumerate(zip(TOKENS, POSITIONS)):
            mask = np.full((1, N_CTX), -np.inf, np.float32)
            mask[0, 0:p + 1] = 0.0
            mask[0, 1] = -np.inf
            lg = dec.step_batch([tok], [p], [p], mask, N_CTX)
            b.synchronize()
            want = lg.cpu().numpy()[0]
            assert np.isfinite(want).all()
            assert bits_equal(got[i], want), (p, first_mismatch(got[i], want))
    finally:
        b.close()
