"""LlamaDecoder.generate / generate_batch with a Sampler: every token sampled on the device (a
step-inputs SAMPLE / SAMPLE_BATCH node ends each step and stages the next), against the loop a
user had to write before on a second decoder of the same weights: step, synchronize, the logits
to the host, tests/sample_ref's rule with the same draws. Two layers, n_ctx 64 (the batch: 128),
the widths and the vocabulary of tests/test_gpu_generate.py and tests/test_gpu_generate_batch.py."""
import numpy as np
import pytest

from tests import sample_ref as R
from tests import test_gpu_generate as G
from tests import test_gpu_generate_batch as GB
from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, N_GEN = G.N_CTX, G.N_GEN
# high temperature, nothing cut: the reference alone makes the run leave the greedy one
HOT = dict(top_k=40, top_p=1.0, min_p=0.0, temp=4.0)
SEED = 5
_cache = {}


def kw_of(s):
    return dict(top_k=s.top_k, top_p=s.top_p, min_p=s.min_p, temp=s.temp)


def host_loop(dec, b, token, pos, n, sampler):
    """One synchronization, one logits copy and one host-side sample per token; the token that
    will stand at position p + 1 is picked with entry p + 1 of the seed's draws."""
    draws = R.draws(sampler.seed, dec.n_ctx + 1)
    out = []
    for p in range(pos, pos + n):
        dec.step(token, p)
        b.synchronize()
        token = R.ref_sample(dec.logits.cpu().numpy(), draws[p + 1], **kw_of(sampler))
        out.append(token)
    return out


def setup(dev, name):
    if name in _cache:
        return _cache[name]
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder, Sampler, hparams
    from tests import llama_model as LM
    O.lib()
    hp = hparams(*G.WIDTHS[name], G.vocab())
    wd = LM.to_device(LM.build(hp, seed=21), dev)
    ba, bb = g.Backend(), g.Backend()
    da, db = LlamaDecoder(ba, hp, wd, N_CTX), LlamaDecoder(bb, hp, wd, N_CTX)
    S = Sampler(seed=SEED, **HOT)
    toks = da.generate(1, 0, N_GEN, sampler=S)
    ba.synchronize()
    sa = G.state(da)
    hist = da.history.cpu().numpy().copy()
    ref = host_loop(db, bb, 1, 0, N_GEN, S)
    sb = G.state(db)
    greedy_ref = G.host_loop(db, bb, 1, 0, N_GEN)
    r = dict(hp=hp, da=da, db=db, ba=ba, bb=bb, S=S, toks=toks, ref=ref, sa=sa, sb=sb, hist=hist, greedy_ref=greedy_ref)
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


def fresh(ba, bb, da, db):
    """Both decoders' caches zeroed: what earlier runs left in cells a test shows cannot differ."""
    import torch
    ba.synchronize()
    bb.synchronize()
    da.reset()
    db.reset()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(G.WIDTHS))
def test_generate_equals_the_host_sampling_loop(dev, name):
    r = setup(dev, name)
    # first the reference alone: a bad choice of inputs names itself
    assert r["ref"] != r["greedy_ref"], "the host loop's sampled run equals the greedy one: pick another seed"
    assert len(r["toks"]) == N_GEN and all(isinstance(t, int) for t in r["toks"])
    assert r["toks"] == r["ref"]
    sa, sb = r["sa"], r["sb"]
    assert bits_equal(sa["logits"], sb["logits"]), first_mismatch(sa["logits"], sb["logits"])
    for i in range(r["hp"]["n_layer"]):
        assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
    assert sa["inp"][1] == N_GEN and sa["inp"][0] == r["toks"][-1]  # staged for a 13th step
    hist = r["hist"]
    assert hist[1:N_GEN + 1].tolist() == r["toks"] and (hist[N_GEN + 1:] == 0).all() and hist[0] == 0


@pytest.mark.parametrize("kw", [dict(chunk=5), dict(chunk=1), dict(use_graph=False), dict()],
                         ids=["chunk5", "chunk1", "eager", "again"])
def test_chunks_eager_and_a_second_call_give_the_same_tokens(tiny, kw):
    assert tiny["da"].generate(1, 0, N_GEN, sampler=tiny["S"], **kw) == tiny["toks"]


def test_the_draw_belongs_to_the_position(tiny):
    """Entry p picks the token that will stand at position p: a run that starts later, from the
    tokens the first run produced, goes on as the first did; another seed gives another run, and
    the first seed again (the table rewritten twice) the first run."""
    from ggml_mi355x.llama import Sampler
    da, toks = tiny["da"], tiny["toks"]
    da.generate(1, 0, 4, sampler=tiny["S"])
    assert da.generate(toks[3], 4, N_GEN - 4, sampler=tiny["S"]) == toks[4:]
    other = da.generate(1, 0, N_GEN, sampler=Sampler(seed=SEED + 1, **HOT))
    assert other != toks and other == host_loop(tiny["db"], tiny["bb"], 1, 0, N_GEN, Sampler(seed=SEED + 1, **HOT))
    assert da.generate(1, 0, N_GEN, sampler=Sampler(seed=SEED, **HOT)) == toks


def test_top_k_one_temp_zero_and_none_are_greedy(tiny):
    from ggml_mi355x.llama import Sampler
    da, greedy = tiny["da"], tiny["greedy_ref"]
    assert da.generate(1, 0, N_GEN, sampler=Sampler(top_k=1, seed=SEED)) == greedy
    assert da.generate(1, 0, N_GEN, sampler=Sampler(temp=0.0, seed=SEED)) == greedy
    assert da.generate(1, 0, N_GEN) == greedy
    assert da.generate(1, 0, N_GEN, sampler=None) == greedy


def test_end_of_the_cache_and_refusals(tiny):
    import ggml_mi355x as g
    da, db, S = tiny["da"], tiny["db"], tiny["S"]
    start = N_CTX - 3
    fresh(tiny["ba"], tiny["bb"], da, db)
    assert da.generate(7, start, 3, sampler=S) == host_loop(db, tiny["bb"], 7, start, 3, S)  # draws[n_ctx] exists
    tiny["ba"].synchronize()
    assert int(da.inp.cpu()[1]) == N_CTX
    with pytest.raises(g.Mi355xError):
        da.generate(7, start, 4, sampler=S)
    da.split = object()
    try:
        with pytest.raises(g.Mi355xError):
            da.generate(1, 0, 1, sampler=S)
    finally:
        da.split = None


def test_launch_counts(tiny):
    """A sampled token is the decode token's launches plus one kq_topk; sampler=None still runs
    today's launches, ending in kq_argmax."""
    import ggml_mi355x as g
    da, L = tiny["da"], tiny["hp"]["n_layer"]
    for sampler, last in ((tiny["S"], "kq::kq_topk"), (None, "kq::kq_argmax")):
        da.generate(1, 0, 1, use_graph=False, sampler=sampler)
        g.timing_enable(True)
        da.generate(1, 0, 1, use_graph=False, sampler=sampler)
        rows = g.timing_read()
        g.timing_enable(False)
        names = [r[0] for r in rows]
        assert len(rows) == 5 * L + 3, names
        assert names[-1] == last and names.count(last) == 1
        assert sum("argmax" in n or "topk" in n for n in names) == 1


# ---------------------------------------------------------------- several sequences
def batch_host_loop(dec, b, tokens, pos, cells, mask, n, sampler, n_kv=GB.N_CTX, cell_stride=1):
    tokens, pos, cells, mask = list(tokens), list(pos), list(cells), np.array(mask, np.float32)
    draws = [R.draws([sampler.seed, i], dec.n_ctx + 1) for i in range(len(tokens))]
    out = [[] for _ in tokens]
    for _ in range(n):
        lg = dec.step_batch(tokens, pos, cells, mask, n_kv)
        b.synchronize()
        lg = lg.cpu().numpy()
        for i in range(len(tokens)):
            tokens[i] = R.ref_sample(lg[i], draws[i][pos[i] + 1], **kw_of(sampler))
            out[i].append(tokens[i])
            pos[i] += 1
            cells[i] += cell_stride
            if cells[i] < n_kv:
                mask[i, cells[i]] = 0.0
    return out


def test_generate_batch_equals_the_host_sampling_loop(dev):
    """T = 3 sequences at different positions of their blocks: tokens, histories, mask rows and
    cells; sequence i uses its own row of draws (at its own positions)."""
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder, Sampler, hparams
    from tests import llama_model as LM
    O.lib()
    T, NC = GB.N_SEQ, GB.N_CTX
    hp = hparams(*GB.WIDTHS["hd64"], GB.vocab())
    wd = LM.to_device(LM.build(hp, seed=77), dev)
    ba, bb = g.Backend(), g.Backend()
    try:
        da, db = LlamaDecoder(ba, hp, wd, NC), LlamaDecoder(bb, hp, wd, NC)
        S = Sampler(seed=SEED, **HOT)
        pos, cells, mask = GB.block_start()
        ref = batch_host_loop(db, bb, GB.START, pos, cells, mask, N_GEN, S)
        greedy, _ = GB.host_loop(db, bb, GB.START, pos, cells, mask, N_GEN)
        assert all(ref[i] != greedy[i] for i in range(T)), "a sequence's sampled run equals its greedy one"
        ref = batch_host_loop(db, bb, GB.START, pos, cells, mask, N_GEN, S)  # (again: B's state is the sampled run's)
        toks = da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S)
        ba.synchronize()
        assert toks == ref
        sa, sb = GB.state(da), GB.state(db)
        assert bits_equal(sa["logits"], sb["logits"]), first_mismatch(sa["logits"], sb["logits"])
        for i in range(hp["n_layer"]):
            assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
        hist, inp = sa["hist"], sa["inp"]
        for s in range(T):
            assert hist[s, 1:N_GEN + 1].tolist() == toks[s] and hist[s, 0] == 0 and (hist[s, N_GEN + 1:] == 0).all()
        assert inp[:T].tolist() == [t[-1] for t in toks]
        assert inp[T:2 * T].tolist() == [N_GEN] * T
        assert inp[2 * T:3 * T].tolist() == [32 * s + N_GEN for s in range(T)]
        want = np.full((T, NC), -np.inf, np.float32)
        for s in range(T):
            want[s, 32 * s:32 * s + N_GEN + 1] = 0.0
        assert (inp[3 * T:].view(np.float32).reshape(T, NC) == want).all()
        # the same seed again, in chunks and eager; greedy is untouched
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S, chunk=5) == toks
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S, use_graph=False) == toks
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC) == greedy
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=Sampler(top_k=1)) == greedy
        # the draw belongs to the sequence and its position: sequences started at other positions
        p2, c2, m2 = [3, 0, 5], [32 * 0 + 3, 32 * 1 + 0, 32 * 2 + 5], np.full((T, NC), -np.inf, np.float32)
        for s in range(T):
            m2[s, 32 * s:32 * s + p2[s] + 1] = 0.0
        fresh(ba, bb, da, db)
        ref2 = batch_host_loop(db, bb, GB.START, p2, c2, m2, 6, S)
        assert da.generate_batch(GB.START, p2, c2, m2, 6, NC, sampler=S) == ref2
    finally:
        ba.close()
        bb.close()
