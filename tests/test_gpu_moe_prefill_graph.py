"""The 2-layer MoE llama of tests/test_gpu_moe_graph.py (tests/moe_model.py; n_ctx 64) through LlamaDecoder with
the MUL_MAT_ID nodes in the expert-grouped form (MOE_PREFILL_GROUPED): prompt over 24 tokens (48 pairs a layer)
against the step loop by logits and K-cache bits, a second prompt on the same decoder (the plan, and the captured
graph, reused: the ids are read at every replay), the launches of a layer by name, logprobs against the same call
under MOE_PREFILL_GEMV. The step loops run under MOE_PREFILL_GEMV: kq_gemv_id, the kernel the rule is checked on in
tests/test_gpu_moe_graph.py."""
import contextlib

import numpy as np
import pytest
import torch

import ggml_mi355x as g
from ggml_mi355x.llama import LlamaDecoder, hparams
from tests import llama_model as LM
from tests import moe_model as MM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HP = hparams(256, 2, 4, 2, 256, 512, n_expert=4, n_expert_used=2)
N_CTX = 64
SEED = 3
TOKENS_A = [(17 + 37 * i) % 512 for i in range(24)]
TOKENS_B = [(401 + 101 * i) % 512 for i in range(24)]


@contextlib.contextmanager
def _mode(impl):
    prev = g.moe_prefill(impl)
    try:
        yield
    finally:
        g.moe_prefill(prev)


def _bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _k_bits(dec):
    return [_bits(c.view(torch.int16).to(torch.int32)) for c in dec.k_cache]


@pytest.fixture(scope="module")
def moe():
    wd = LM.to_device(MM.build(HP, SEED), DEV)
    b = g.Backend()
    dec = LlamaDecoder(b, HP, wd, N_CTX)
    steps = {}
    with _mode(g.MOE_PREFILL_GEMV):  # the references, once
        for name, toks in (("a", TOKENS_A), ("b", TOKENS_B)):
            dec.reset()
            for p, tok in enumerate(toks):
                lg = _bits(dec.step(tok, p))
            steps[name] = (lg, _k_bits(dec))
    yield dict(dec=dec, b=b, steps=steps)
    b.close()


def test_prompt_equals_steps_and_a_second_prompt_reuses_the_graph(moe):
    dec = moe["dec"]
    with _mode(g.MOE_PREFILL_GROUPED):
        for name, toks in (("a", TOKENS_A), ("b", TOKENS_B), ("a", TOKENS_A)):
            want, kc = moe["steps"][name]
            dec.reset()
            got = _bits(dec.prompt(toks))
            assert (got == want).all(), (name, int((got != want).sum()))
            for a, c in zip(kc, _k_bits(dec)):
                assert (a == c).all(), name


def test_launches_of_a_layer(moe):
    dec = moe["dec"]
    with _mode(g.MOE_PREFILL_GROUPED):
        dec.reset()
        g.timing_enable(True)
        lg = dec.prompt(TOKENS_A, use_graph=False)
        got = _bits(lg)
        names = [r[0].split("<")[0].replace("kq::", "") for r in g.timing_read()]
        g.timing_enable(False)
    assert (got == moe["steps"]["a"][0]).all()
    starts = [i for i, n in enumerate(names) if n == "kq_moe_route"]
    ends = [i for i, n in enumerate(names) if n == "kq_moe_combine"]
    assert len(starts) == len(ends) == HP["n_layer"], names
    for s, e in zip(starts, ends):
        assert names[s + 1:e] == ["kq_moe_group", "kq_quantize_q8L", "kq_mmq_id", "kq_mmq_id", "kq_swiglu",
                                  "kq_quantize_q8L", "kq_mmq_id"], names[s:e + 1]
    assert not any("kq_gemv_id" in n for n in names), names


def test_logprobs_equal_the_gemv_form(moe):
    dec = moe["dec"]
    with _mode(g.MOE_PREFILL_GEMV):
        dec.reset()
        want = dec.logprobs(TOKENS_A, records=True)
    with _mode(g.MOE_PREFILL_GROUPED):
        dec.reset()
        got = dec.logprobs(TOKENS_A, records=True)
    assert got.tobytes() == want.tobytes()
