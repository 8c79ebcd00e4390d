"""LlamaDecoder.generate: greedy decoding with the token picked on the device (a step-inputs
ARGMAX node ends each token and stages the next), against the loop a user had to write before
(step, synchronize, logits to the host, numpy argmax) on a second decoder of the same weights,
and against the CPU oracle's llm_build_llama restatement. Two layers, n_ctx 64, the smallest
vocabulary whose argmax runs on at least 3 workgroups."""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, N_GEN, N_ORACLE = 64, 12, 6
WIDTHS = {"hd64": (2048, 2, 32, 4, 5632), "hd128": (1024, 2, 8, 2, 2816)}
_cache = {}


def ref_argmax(x):
    return int(np.argmax(np.where(np.isnan(x), -np.inf, x)))


def vocab():
    import ggml_mi355x as g
    v = 256
    while g.argmax_plan(v)[0] < 3:
        v += 256
    return v


def host_loop(dec, b, token, pos, n):
    """What a user writes without generate: one synchronization and one logits copy per token."""
    out = []
    for p in range(pos, pos + n):
        dec.step(token, p)
        b.synchronize()
        token = ref_argmax(dec.logits.cpu().numpy())
        out.append(token)
    return out


def state(dec):
    import torch
    torch.cuda.synchronize()
    return dict(logits=dec.logits.cpu().numpy().copy(), inp=dec.inp.cpu().numpy().copy(),
                k=[c.cpu().numpy().copy() for c in dec.k_cache], v=[c.cpu().numpy().copy() for c in dec.v_cache])


def setup(dev, name):
    """One run per width, shared by the tests: decoder A generates, decoder B runs the host loop,
    the oracle decodes the first tokens. The results are kept as host copies."""
    if name in _cache:
        return _cache[name]
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    O.lib()
    hp = hparams(*WIDTHS[name], vocab())
    w = LM.build(hp, seed=21)
    wd = LM.to_device(w, dev)
    ba, bb = g.Backend(), g.Backend()
    da, db = LlamaDecoder(ba, hp, wd, N_CTX), LlamaDecoder(bb, hp, wd, N_CTX)
    toks = da.generate(1, 0, N_GEN)
    ba.synchronize()
    sa = state(da)
    hist = da.history.cpu().numpy().copy()
    ref = host_loop(db, bb, 1, 0, N_GEN)
    sb = state(db)
    model, cache = LM.oracle_model(hp, w, N_CTX)
    otoks, tok = [], 1
    for p in range(N_ORACLE):
        lg, _ = O.decode_token(model, tok, p, cache)
        tok = ref_argmax(lg)
        otoks.append(tok)
    next_ref, _ = O.decode_token(model, otoks[-1], N_ORACLE, cache)  # the token after them, for step()
    r = dict(hp=hp, da=da, db=db, ba=ba, bb=bb, toks=toks, ref=ref, sa=sa, sb=sb, otoks=otoks, next_ref=next_ref,
             hist=hist)
    _cache[name] = r
    return r


@pytest.fixture(scope="module", autouse=True)
def close_backends():
    yield
    for r in _cache.values():
        r["ba"].close()
        r["bb"].close()
    _cache.clear()


@pytest.fixture(scope="module")
def tiny(dev):
    return setup(dev, "hd64")


@pytest.mark.parametrize("name", list(WIDTHS))
def test_generate_equals_host_loop_and_oracle(dev, name):
    r = setup(dev, name)
    assert len(r["toks"]) == N_GEN and all(isinstance(t, int) for t in r["toks"])
    assert r["toks"] == r["ref"]
    sa, sb = r["sa"], r["sb"]
    assert bits_equal(sa["logits"], sb["logits"]), first_mismatch(sa["logits"], sb["logits"])
    for i in range(r["hp"]["n_layer"]):
        assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
    assert sa["inp"][1] == N_GEN and sa["inp"][0] == r["toks"][-1]  # staged for a 13th step
    assert r["toks"][:N_ORACLE] == r["otoks"]
    hist = r["hist"]
    assert hist[1:N_GEN + 1].tolist() == r["toks"] and (hist[N_GEN + 1:] == 0).all() and hist[0] == 0


@pytest.mark.parametrize("kw", [dict(chunk=5), dict(chunk=1), dict(use_graph=False), dict(chunk=5, use_graph=False)],
                         ids=["chunk5", "chunk1", "eager", "eager-chunk5"])
def test_chunks_and_eager_give_the_same_tokens(tiny, kw):
    assert tiny["da"].generate(1, 0, N_GEN, **kw) == tiny["toks"]


def test_eos_stops_the_run(tiny):
    toks = tiny["toks"]
    eos = toks[3]
    assert eos not in toks[:3], "the run repeats a token before its 4th: pick another seed"
    for chunk in (32, 3):  # eos inside the first chunk, and in the second
        assert tiny["da"].generate(1, 0, N_GEN, eos=eos, chunk=chunk) == toks[:4]
    assert tiny["da"].generate(1, 0, 0) == []


def test_end_of_the_cache(tiny):
    import ggml_mi355x as g
    da, db = tiny["da"], tiny["db"]
    start = N_CTX - 3
    got = da.generate(7, start, 3)
    assert got == host_loop(db, tiny["bb"], 7, start, 3)
    tiny["ba"].synchronize()
    assert int(da.inp.cpu()[1]) == N_CTX  # pos + 1 is written even there
    before, hist = state(da), da.history.cpu().numpy().copy()
    for n, pos in ((4, start), (1, N_CTX), (N_CTX + 1, 0), (1, -1)):
        with pytest.raises(g.Mi355xError):
            da.generate(7, pos, n)
    tiny["ba"].synchronize()
    after = state(da)
    for i in range(tiny["hp"]["n_layer"]):
        assert (after["k"][i] == before["k"][i]).all() and (after["v"][i] == before["v"][i]).all(), i
    assert (after["inp"] == before["inp"]).all() and (da.history.cpu().numpy() == hist).all()


def test_step_after_generate(tiny):
    """step restages the whole input block: the token after the oracle's 6 is bit-exact."""
    da = tiny["da"]
    assert da.generate(1, 0, N_ORACLE) == tiny["otoks"]
    da.step(tiny["otoks"][-1], N_ORACLE)
    tiny["ba"].synchronize()
    got = da.logits.cpu().numpy()
    assert bits_equal(got, tiny["next_ref"]), first_mismatch(got, tiny["next_ref"])


def test_generate_refuses_a_row_split(tiny):
    import ggml_mi355x as g
    da = tiny["da"]
    da.split = object()
    try:
        with pytest.raises(g.Mi355xError):
            da.generate(1, 0, 1)
    finally:
        da.split = None


def test_launch_count(tiny):
    """One generated token is the decode token's launches plus the argmax; a plain step on the
    same decoder keeps its count (test_llama_fused_launch_count's 5 per layer + 2)."""
    import ggml_mi355x as g
    da, L = tiny["da"], tiny["hp"]["n_layer"]
    da.generate(1, 0, 1, use_graph=False)
    g.timing_enable(True)
    da.generate(1, 0, 1, use_graph=False)
    rows = g.timing_read()
    g.timing_enable(False)
    names = [r[0] for r in rows]
    assert len(rows) == 5 * L + 3, names
    assert names[-1] == "kq::kq_argmax" and names.count("kq::kq_argmax") == 1
    g.timing_enable(True)
    da.step(5, 1, use_graph=False)
    rows = g.timing_read()
    g.timing_enable(False)
    assert len(rows) == 5 * L + 2, [r[0] for r in rows]
    assert not any("argmax" in r[0] for r in rows)
