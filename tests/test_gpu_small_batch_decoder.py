"""mi355x_small_batch FUSED through LlamaDecoder against the CPU oracle, by bits: step_batch of 2, 8, 9
and 15 sequences over four positions, a group-of-4 layout behind the SwiGLU prologue, prompts of 2, 9
and 15 tokens, generate_batch's replayed graph, a Q3_K mix and a MoE model.

The construction and the argument why the bits must be equal are those of tests/test_gpu_batch_token.py:
sequence s owns the cells [32 s, 32 s + 32) of a cache of n_ctx = 32 * n_seq cells, the token at
position p sits in cell 32 s + p and sees the cells 32 s .. 32 s + p; the oracle decodes each sequence
alone on a 32-cell cache of its own. The other sequences' cells are whole masked blocks that add exact
zeros, and every column of a batched MUL_MAT is its own GEMV chain."""
import functools

import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch
from tests.test_gpu_rows_cols import _timed

pytestmark = pytest.mark.gpu

STEPS, MAX_SEQ = 4, 15
Q3, Q4 = 11, 12


@pytest.fixture(autouse=True)
def fused():
    import ggml_mi355x as g
    prev = g.small_batch(g.SMALL_BATCH_FUSED)
    yield
    g.small_batch(prev)
    assert g.small_batch() == g.SMALL_BATCH_NODES


@pytest.fixture
def new_backend():
    """g.Backend() that is closed after the test, passed or failed."""
    import ggml_mi355x as g
    made = []

    def make():
        made.append(g.Backend())
        return made[-1]
    yield make
    for b in made:
        b.close()


def _host(b, out):
    """The device tensor `out` on the host, after the backend's stream has finished."""
    b.synchronize()
    return out.cpu().numpy()


def _tokens(n_vocab):
    """[sequence][step], the same for every test of a vocabulary: sequence s's tokens do not depend on n_seq."""
    return np.random.default_rng(n_vocab).integers(0, n_vocab, size=(MAX_SEQ, STEPS)).tolist()


def _inputs(n_seq, step, toks):
    mask = np.full((n_seq, 32 * n_seq), -np.inf, np.float32)
    for s in range(n_seq):
        mask[s, 32 * s:32 * s + step + 1] = 0.0
    return [toks[s][step] for s in range(n_seq)], [step] * n_seq, [32 * s + step for s in range(n_seq)], mask


def _alone(decode, make, n_seq, toks):
    """ref[step][sequence]: each sequence decoded alone by `decode` on a fresh 32-cell cache from make()."""
    ref = [[None] * n_seq for _ in range(STEPS)]
    for s in range(n_seq):
        model, cache = make()
        for p in range(STEPS):
            out = decode(model, toks[s][p], p, cache)
            ref[p][s] = out[0] if isinstance(out, tuple) else out
    return ref


@functools.lru_cache(maxsize=None)
def _tiny(mix):
    """Two layers, E = 512 (head_dim 64, 4 query heads per KV head), FF = 768, V = 1024, and the oracle's
    logits of MAX_SEQ sequences over STEPS positions (computed once per mix, read by every test)."""
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    from ggml_mi355x.llama import hparams
    O.lib()
    hp = hparams(512, 2, 8, 2, 768, 1024)
    w = LM.build(hp, 77, mix=mix)
    return hp, w, _alone(O.decode_token, lambda: LM.oracle_model(hp, w, 32), MAX_SEQ, _tokens(1024))


def _run_steps(new_backend, dev, hp, w, ref, n_seq, fuse=True, eager_from=STEPS - 1):
    """Four step_batch calls (captured and replayed up to `eager_from`, eager and timed from there),
    every row of every step against ref; the names of the eager steps' launches."""
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    toks, n_ctx, names = _tokens(hp["n_vocab"]), 32 * n_seq, []
    b = new_backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), n_ctx, fuse=fuse)

    def step(p, use_graph):
        return _host(b, dec.step_batch(*_inputs(n_seq, p, toks), n_ctx, use_graph=use_graph))

    for p in range(STEPS):
        if p < eager_from:
            got = step(p, True)
        else:
            got, nm = _timed(lambda: step(p, False))
            names += nm
        assert got.shape == (n_seq, hp["n_vocab"])
        for s in range(n_seq):
            assert bits_equal(got[s], ref[p][s]), (p, s, first_mismatch(got[s], ref[p][s]))
    return names


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("mix", ["q4_k_m", "q5_k_m"])
@pytest.mark.parametrize("n_seq", [2, 8, 9, 15])
def test_step_batch_equals_each_sequence_alone(dev, new_backend, n_seq, mix, fuse):
    """2: the minimum; 8: exactly one group; 9: a group of 8 and a group of 1; 15: the last count before
    kq_mmq. Positions 0 to 3: the attention between the fused GEMVs runs over up to four live cells."""
    hp, w, ref = _tiny(mix)
    names = _run_steps(new_backend, dev, hp, w, ref, n_seq, fuse=fuse)
    assert any("kq_rows_cols" in n for n in names), names
    assert not any("kq_gemv<" in n or "kq_quantize_q8K" in n for n in names), names
    if fuse:  # the plain-layout prologues: attn_norm and ffn_norm of both layers, output_norm; SwiGLU of both layers
        assert sum("kq_rms_norm_q8L" in n for n in names) == 5 and sum("kq_swiglu_q8L" in n for n in names) == 2, names


def test_sixteen_sequences_leave_kq_rows_cols(dev, new_backend):
    """The 15 / 16 boundary through the decoder: at 16 columns kq_mmq takes every matrix."""
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    hp, w, _ = _tiny("q4_k_m")
    toks = _tokens(1024) + [[5, 1000, 77, 300]]
    ref = _alone(O.decode_token, lambda: LM.oracle_model(hp, w, 32), 16, toks)[:2]
    from ggml_mi355x.llama import LlamaDecoder
    b = new_backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), 512)
    for p in range(2):
        got, names = _timed(lambda: _host(b, dec.step_batch(*_inputs(16, p, toks), 512, use_graph=False)))
        assert not any("kq_rows_cols" in n for n in names) and any("kq_mmq" in n for n in names), names
        for s in range(16):
            assert bits_equal(got[s], ref[p][s]), (p, s, first_mismatch(got[s], ref[p][s]))


def test_group_of_four_behind_the_swiglu_prologue(dev, new_backend):
    """One layer, E = 256, FF the first K at which ffn_down's layout (its type, its 256 rows) has no room
    for a group of 8, read from the planner: at 8 sequences ffn_down runs as two groups of four on the
    blocks kq_swiglu_q8L wrote, the E-wide matrices as one group of eight."""
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    from ggml_mi355x.llama import hparams
    O.lib()
    E, down = 256, 14  # (use_more_bits(0, 1): the only layer's ffn_down is Q6_K)
    FF = next(k for k in range(256, 1 << 16, 256) if g.rows_cols_plan(k, 8, type=down, n_rows=E)["ncol"] < 8)
    hp = hparams(E, 1, 4, 2, FF, 512)
    w = LM.build(hp, 78)
    assert w["blk.0.ffn_down"][0] == down
    p = g.rows_cols_plan(FF, 8, type=down, n_rows=E)
    assert (p["ncol"], p["groups"]) == (4, 2) and g.rows_cols_plan(E, 8, n_rows=FF)["ncol"] == 8
    ref = _alone(O.decode_token, lambda: LM.oracle_model(hp, w, 32), 8, _tokens(512))
    names = _run_steps(new_backend, dev, hp, w, ref, 8)
    assert "kq::kq_rows_cols<4>" in names and "kq::kq_rows_cols<8>" in names and "kq::kq_swiglu_q8L" in names, names


@functools.lru_cache(maxsize=None)
def _prompt_case():
    """One sequence of 3 + 15 tokens on the tiny q4_k_m model: the oracle's logits after each token."""
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    hp, w, _ = _tiny("q4_k_m")
    toks = np.random.default_rng(3).integers(0, 1024, size=18).tolist()
    model, cache = LM.oracle_model(hp, w, 32)
    return toks, [O.decode_token(model, t, p, cache)[0] for p, t in enumerate(toks)]


@pytest.mark.parametrize("n_tok", [2, 9, 15])
def test_short_prompt_after_a_history(dev, new_backend, n_tok):
    """prompt() of 2, 9 and 15 tokens at position 3, after three decoded tokens: its last logits."""
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    hp, w, _ = _tiny("q4_k_m")
    toks, ref = _prompt_case()
    b = new_backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), 32)
    for p in range(3):
        assert bits_equal(_host(b, dec.step(toks[p], p)).reshape(-1), ref[p]), p
    got, names = _timed(lambda: _host(b, dec.prompt(toks[3:3 + n_tok], 3, use_graph=False)).reshape(-1))
    assert bits_equal(got, ref[2 + n_tok]), first_mismatch(got, ref[2 + n_tok])
    assert any("kq_rows_cols" in n for n in names), names
    assert not any("kq_gemv<" in n or "kq_quantize_q8K" in n or "kq_mmq" in n for n in names), names


def test_generate_batch_replays_equal_the_oracles_greedy_tokens(dev, new_backend):
    """Nine sequences, four steps in chunks of one: the graph captured at the first step is replayed three
    times, every step's ARGMAX_BATCH staging the next. Each sequence's tokens are those of the oracle
    decoding it alone and taking the first largest logit."""
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    hp, w, _ = _tiny("q4_k_m")
    n_seq, n_ctx = 9, 288
    first = [t[0] for t in _tokens(1024)[:n_seq]]
    want = []
    for s in range(n_seq):
        model, cache = LM.oracle_model(hp, w, 32)
        tok, seq = first[s], []
        for p in range(STEPS):
            tok = int(np.argmax(O.decode_token(model, tok, p, cache)[0]))
            seq.append(tok)
        want.append(seq)
    b = new_backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), n_ctx)
    _, pos, cells, mask = _inputs(n_seq, 0, _tokens(1024))
    got = dec.generate_batch(first, pos, cells, mask, STEPS, n_ctx, chunk=1, use_graph=True)
    assert got == want


def _q3k_model():
    """The Q3_K_M-like mix of test_gpu_q3k.test_llama_decoder_q3_k_m_mix (two layers, E = 256, FF = V = 512)."""
    from ggml_mi355x.llama import hparams
    from tests import llama_model as LM
    from tests import q3k_ref as R
    hp = hparams(256, 2, 4, 2, 512, 512)
    w, rng = LM.build(hp, 7), np.random.default_rng(11)
    mix = {"token_embd": Q3, "output": 14, "attn_q": Q3, "attn_k": Q3, "ffn_gate": Q3, "ffn_up": Q3, "attn_v": 13,
           "attn_output": Q4, "ffn_down": Q4}
    for name, (_, old) in [(k, v) for k, v in w.items() if isinstance(v, tuple)]:
        ty, k = mix[name.split(".")[-1]], hp["n_ff"] if name.endswith("ffn_down") else hp["n_embd"]
        w[name] = (ty, R.weights(rng, old.shape[0], k) if ty == Q3 else LM.kquant(rng, ty, old.shape[0], k, edges=True))
    return hp, w


def test_q3k_mix_keeps_its_single_nodes(dev, new_backend):
    """Four sequences: the Q3_K matrices stay single nodes on kq_gemv_q3k while attn_v, attn_output, ffn_down
    and the output run on kq_rows_cols, against tests/q3k_ref.py's composed token."""
    from tests import llama_model as LM
    from tests import q3k_ref as R
    hp, w = _q3k_model()
    ref = _alone(R.decode_token, lambda: LM.oracle_model(hp, w, 32), 4, _tokens(512))
    names = _run_steps(new_backend, dev, hp, w, ref, 4)
    assert any("kq_gemv_q3k" in n for n in names) and any("kq_rows_cols" in n for n in names), names


@functools.lru_cache(maxsize=None)
def _moe_case():
    from ggml_mi355x.llama import hparams
    from tests import moe_model as MM
    from tests import moe_ref as M
    hp = hparams(256, 2, 4, 2, 256, 512, n_expert=4, n_expert_used=2)  # tests/test_gpu_moe_graph.py's model
    w = MM.build(hp, 3)
    return hp, w, _alone(M.decode_token_moe, lambda: MM.oracle_model(hp, w, 32), 9, _tokens(512))


@pytest.mark.parametrize("n_seq", [3, 9])
def test_moe_attention_matrices_on_kq_rows_cols(dev, new_backend, n_seq):
    """The planner's moe flag keeps the layer engine and the attention + o-proj fusion out: q/k/v and the
    o-proj are left to the patterns above (kq_rows_cols), the experts stay on their own kernels."""
    hp, w, ref = _moe_case()
    names = _run_steps(new_backend, dev, hp, w, ref, n_seq)
    assert sum("kq_rows_cols" in n for n in names) == 2 * hp["n_layer"] + 1, names  # q/k/v, o-proj + ADD; the head
    assert sum("kq_gemv_id<" in n or "kq_mmq_id<" in n for n in names) == 3 * hp["n_layer"] and sum("kq_moe_route" in n for n in names) == hp["n_layer"], names
    assert not any("kq_gemv<" in n or "attn_oproj" in n or "kq_layer" in n for n in names), names
