"""GPU: the multi-sequence option of the ggml-backend registration
(ggml_backend_mi355x_set_multi_seq, adapter/ggml-mi355x.cpp) through the harness
tests/adapter/multiseq_test.cpp (prebuilt by __graft_entry__.build()): a graph whose KQ mask
hides a cell inside [0, pos] — which tests/test_gpu_adapter.py sees refused — succeeds with the
option on, with the logits LlamaDecoder.step_batch gives for the same inputs, and is still
refused with the option off."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "adapter", "bin", "multiseq_test")
N_CTX = 64
TOKENS = [7, 1000, 7, 123, 1]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from tests.test_adapter import glue_inputs
    from ggml_mi355x.llama import hparams
    hp = hparams(512, 2, 8, 2, 768, 1024)
    argv, w = glue_inputs(tmp_path_factory.mktemp("multiseq"), hp, N_CTX, 43, TOKENS)
    return hp, argv, w


def test_hidden_cell_graph_runs_with_multi_seq_on(dev, files):
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    hp, argv, w = files
    assert os.path.exists(HARNESS), "tests/adapter/bin/multiseq_test missing: run __graft_entry__.build()"
    r = subprocess.run([HARNESS] + argv + ["on"], capture_output=True, text=True, timeout=200)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "hidden 0" in r.stdout and "refused" not in r.stdout
    got = np.fromfile(argv[3], np.float32).reshape(len(TOKENS) + 1, hp["n_vocab"])
    # the Python path on the same inputs: the tokens at cell == position, then the last token
    # again at the next position with cell 0 hidden
    b = g.Backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), N_CTX)
    for p, tok in enumerate(TOKENS):
        dec.step(tok, p)
        b.synchronize()
        want = dec.logits.cpu().numpy()
        assert bits_equal(got[p], want), (p, first_mismatch(got[p], want))
    p = len(TOKENS)
    mask = np.full((1, N_CTX), -np.inf, np.float32)
    mask[0, 1:p + 1] = 0.0
    lg = dec.step_batch([TOKENS[-1]], [p], [p], mask, N_CTX)
    b.synchronize()
    want = lg.cpu().numpy()[0]
    assert np.isfinite(want).all()
    assert bits_equal(got[p], want), first_mismatch(got[p], want)
    b.close()


def test_hidden_cell_graph_is_refused_with_multi_seq_off(dev, files):
    hp, argv, w = files
    assert os.path.exists(HARNESS), "tests/adapter/bin/multiseq_test missing: run __graft_entry__.build()"
    r = subprocess.run([HARNESS] + argv + ["off"], capture_output=True, text=True, timeout=200)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "refused -1" in r.stdout and "hidden" not in r.stdout
