"""A 2-layer MoE llama (n_embd 256, 4 heads / 2 KV heads of 64, n_ff 256, 4 experts of which 2 are used,
vocabulary 512, n_ctx 32, the q4_k_m mix) through LlamaDecoder, logits by bits: step against
tests/moe_ref.decode_token_moe, prompt against steps, step_batch against per-sequence steps, generate
against the step + argmax loop, a replayed captured graph whose second token selects other experts than
the token it was captured with, and fusion on against off."""
import numpy as np
import pytest
import torch

import ggml_mi355x as g
from ggml_mi355x.llama import LlamaDecoder, hparams
from tests import llama_model as LM
from tests import moe_model as MM
from tests import moe_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HP = hparams(256, 2, 4, 2, 256, 512, n_expert=4, n_expert_used=2)
N_CTX = 32
SEED = 3
TOKENS = [17, 401, 5, 260, 99]


def _bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().view(np.uint32).copy()


@pytest.fixture(scope="module")
def moe():
    w = MM.build(HP, SEED)
    model, cache = MM.oracle_model(HP, w, N_CTX)
    trace, ref = [], []
    for p, tok in enumerate(TOKENS[:4]):  # the reference, once: 4 positions
        tr = []
        ref.append(M.decode_token_moe(model, tok, p, cache, trace=tr).view(np.uint32).copy())
        trace.append(tr)
    wd = LM.to_device(w, DEV)
    b = g.Backend()
    dec = LlamaDecoder(b, HP, wd, N_CTX)
    yield dict(w=w, wd=wd, b=b, dec=dec, ref=ref, trace=trace)
    b.close()


def test_step_matches_the_rule_over_four_positions(moe):
    dec = moe["dec"]
    dec.reset()
    for p, tok in enumerate(TOKENS[:4]):
        got = _bits(dec.step(tok, p, use_graph=False))
        assert (got == moe["ref"][p]).all(), (p, int((got != moe["ref"][p]).sum()))


def test_replayed_graph_reads_the_ids_of_every_token(moe):
    """The captured graph is replayed for a token whose layer-0 experts differ from those of the token it was
    captured with: a launch that baked the ids at capture gives the second token the first one's experts."""
    ids0 = [sorted(moe["trace"][p][0]["ids"].tolist()) for p in range(4)]
    assert ids0[0] != ids0[1], ids0  # (the seed is chosen so that this holds)
    dec = moe["dec"]
    dec.reset()
    for p, tok in enumerate(TOKENS[:4]):
        got = _bits(dec.step(tok, p, use_graph=True))
        assert (got == moe["ref"][p]).all(), (p, int((got != moe["ref"][p]).sum()))


def test_prompt_equals_steps(moe):
    dec = moe["dec"]
    dec.reset()
    for p, tok in enumerate(TOKENS):
        want = _bits(dec.step(tok, p))
    kc = [_bits(c.view(torch.int16).to(torch.int32)) for c in dec.k_cache]
    dec.reset()
    got = _bits(dec.prompt(TOKENS))
    assert (got == want).all()
    for a, c in zip(kc, dec.k_cache):
        assert (a == _bits(c.view(torch.int16).to(torch.int32))).all()


def test_step_batch_equals_per_sequence_steps(moe):
    """Two sequences, each on its own block of 32 cells (cell = 32 s + position), two steps."""
    dec = moe["dec"]
    seqs = [[17, 401], [260, 99]]
    want = []
    for s in seqs:
        dec.reset()
        want.append([_bits(dec.step(tok, p)) for p, tok in enumerate(s)])
    b2 = g.Backend()
    try:
        d2 = LlamaDecoder(b2, HP, moe["wd"], 64)
        for p in range(2):
            mask = np.full((2, 64), -np.inf, np.float32)
            for s in range(2):
                mask[s, 32 * s:32 * s + p + 1] = 0.0
            lg = _bits(d2.step_batch([seqs[0][p], seqs[1][p]], [p, p], [p, 32 + p], mask, 64))
            for s in range(2):
                assert (lg[s] == want[s][p]).all(), (p, s)
    finally:
        b2.close()


def test_generate_equals_the_step_argmax_loop(moe):
    dec = moe["dec"]
    dec.reset()
    tok, want = TOKENS[0], []
    for p in range(8):
        lg = dec.step(tok, p)
        torch.cuda.synchronize()
        tok = int(np.argmax(lg.cpu().numpy()))
        want.append(tok)
    dec.reset()
    assert dec.generate(TOKENS[0], 0, 8) == want
    dec.reset()
    assert dec.generate(TOKENS[0], 0, 8, chunk=3, use_graph=False) == want


def test_fusion_on_and_off_give_the_same_bits(moe):
    b2 = g.Backend()
    try:
        d2 = LlamaDecoder(b2, HP, moe["wd"], N_CTX, fuse=False)
        for p, tok in enumerate(TOKENS[:4]):
            got = _bits(d2.step(tok, p))
            assert (got == moe["ref"][p]).all(), p
        d2.reset()
        want = _bits(d2.prompt(TOKENS))
        dec = moe["dec"]
        dec.reset()
        assert (_bits(dec.prompt(TOKENS)) == want).all()
    finally:
        b2.close()


def test_attn_oproj_switch_leaves_a_moe_graph_unfused(moe):
    """A graph with MoE nodes takes the attention + o-proj fusion nowhere, whatever the backend's switch says:
    the same launches (read by name, uncaptured) and the same bits."""
    b2 = g.Backend()
    try:
        b2.set_attn_oproj(True)
        d2 = LlamaDecoder(b2, HP, moe["wd"], N_CTX)
        for p, tok in enumerate(TOKENS[:2]):
            g.timing_enable(True)
            lg = d2.step(tok, p, use_graph=False)
            got = _bits(lg)
            names = [r[0] for r in g.timing_read()]
            g.timing_enable(False)
            assert (got == moe["ref"][p]).all(), p
            assert not any("attn_oproj" in n for n in names), names
            assert sum("kq_gemv_id" in n for n in names) == 3 * HP["n_layer"], names
            assert sum("kq_moe_route" in n for n in names) == HP["n_layer"], names
    finally:
        b2.close()
