"""LlamaDecoder.generate / generate_batch with a Sampler that edits the logits (penalties, logit
bias): a PENALIZE node between the logits and the SAMPLE node, the window read from the history
the steps write, against the loop a user had to write before on a second decoder of the same
weights: step, synchronize, the logits to the host, tests/penalize_ref's rule on the tokens so far,
tests/sample_ref's rule with the same draws. The shapes and helpers are those of
tests/test_gpu_generate.py and tests/test_gpu_generate_batch.py; every run starts at position 8 on
zeroed caches."""
import numpy as np
import pytest

from tests import penalize_ref as P
from tests import sample_ref as R
from tests import test_gpu_generate as G
from tests import test_gpu_generate_batch as GB
from tests import test_gpu_generate_sample as GS
from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, N_GEN, POS = G.N_CTX, G.N_GEN, 8
HOT, SEED = GS.HOT, GS.SEED
PRESENCE = 1e4  # no token of the window can be picked again
_cache = {}


def edit(lg, S, win):
    """The sampler's edit of one row of logits on the host."""
    return P.penalize_row(lg, win if S.penalizes() else [], S.repeat_penalty, S.freq_penalty, S.presence_penalty,
                          S.logit_bias)[0]


def window_of(hist, p, last_n):
    return [hist[j] for j in range(max(0, p - last_n + 1), p + 1) if j in hist]


def start_hist(token, pos, context):
    hist = {pos - len(context) + i: t for i, t in enumerate(context)}
    hist[pos] = token
    return hist


def host_loop(dec, b, token, pos, n, S, context=()):
    """One synchronization, one logits copy, the edit and the sample on the host per token. Returns
    the tokens and the last step's edited logits."""
    draws = R.draws(S.seed, dec.n_ctx + 1)
    hist, out, lg = start_hist(token, pos, list(context)), [], None
    for p in range(pos, pos + n):
        dec.step(token, p)
        b.synchronize()
        lg = edit(dec.logits.cpu().numpy(), S, window_of(hist, p, S.repeat_last_n))
        token = R.ref_sample(lg, draws[p + 1], **GS.kw_of(S))
        out.append(token)
        hist[p + 1] = token
    return out, lg


def fresh(r):
    GS.fresh(r["ba"], r["bb"], r["da"], r["db"])


def setup(dev):
    if "tiny" in _cache:
        return _cache["tiny"]
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder, Sampler, hparams
    from tests import llama_model as LM
    O.lib()
    hp = hparams(*G.WIDTHS["hd64"], G.vocab())
    wd = LM.to_device(LM.build(hp, seed=21), dev)
    ba, bb = g.Backend(), g.Backend()
    da, db = LlamaDecoder(ba, hp, wd, N_CTX), LlamaDecoder(bb, hp, wd, N_CTX)
    r = dict(hp=hp, da=da, db=db, ba=ba, bb=bb)
    _cache["tiny"] = r
    # a sampler without edits, first: the decoder's history is still as allocated
    S0 = Sampler(seed=SEED, **HOT)
    r["S0"], r["plain0"] = S0, da.generate(1, 0, N_GEN, sampler=S0)
    ba.synchronize()
    r["hist0"] = da.history.cpu().numpy().copy()
    r["plain0_ref"] = GS.host_loop(db, bb, 1, 0, N_GEN, S0)
    # the plain run from position 8 on zeroed caches, then the penalised reference and the device
    fresh(r)
    r["plain"] = GS.host_loop(db, bb, 1, POS, N_GEN, S0)
    ctx = [t for t in (3, 5, 7, 5, 3, 11, 2, 13, 17) if t != r["plain"][0]][:POS - 1]
    ctx.insert(2, r["plain"][0])  # eight tokens that include the plain run's first
    S = Sampler(seed=SEED, presence_penalty=PRESENCE, repeat_penalty=1.1, freq_penalty=0.25, **HOT)
    r["S"], r["ctx"] = S, ctx
    fresh(r)
    r["ref"], r["ref_logits"] = host_loop(db, bb, 1, POS, N_GEN, S, ctx)
    r["sb"] = G.state(db)
    r["toks"] = da.generate(1, POS, N_GEN, sampler=S, context=ctx)
    ba.synchronize()
    r["sa"] = G.state(da)
    r["hist"] = da.history.cpu().numpy().copy()
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
    return setup(dev)


def test_generate_equals_the_host_loop_with_the_rule(tiny):
    r = tiny
    # first the reference alone: the penalised run leaves the plain one at step 0
    assert r["ctx"].count(r["plain"][0]) == 1 and len(r["ctx"]) == POS
    assert r["ref"][0] != r["plain"][0], "the penalty did not change the first token: pick other inputs"
    assert len(set(r["ref"])) == N_GEN and not set(r["ref"]) & set(r["ctx"])  # presence 1e4: no token twice
    assert len(r["toks"]) == N_GEN and all(isinstance(t, int) for t in r["toks"])
    assert r["toks"] == r["ref"]
    sa, sb = r["sa"], r["sb"]
    # the logits buffer holds the edited logits of the last step; decoder B's are the unedited ones
    assert bits_equal(sa["logits"], r["ref_logits"]), first_mismatch(sa["logits"], r["ref_logits"])
    assert not bits_equal(sa["logits"], sb["logits"])
    for i in range(r["hp"]["n_layer"]):
        assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
    assert sa["inp"][1] == POS + N_GEN and sa["inp"][0] == r["toks"][-1]
    hist = r["hist"]
    assert hist[:POS].tolist() == r["ctx"] and hist[POS] == 1                # the context and the start token
    assert hist[POS + 1:POS + N_GEN + 1].tolist() == r["toks"] and (hist[POS + N_GEN + 1:] == 0).all()


@pytest.mark.parametrize("kw", [dict(chunk=5), dict(chunk=1), dict(use_graph=False), dict()],
                         ids=["chunk5", "chunk1", "eager", "again"])
def test_chunks_eager_and_a_second_call_give_the_same_tokens(tiny, kw):
    assert tiny["da"].generate(1, POS, N_GEN, sampler=tiny["S"], context=tiny["ctx"], **kw) == tiny["toks"]


def test_a_short_context_and_a_short_window(tiny):
    """Three tokens of context: the history below them holds -1. repeat_last_n 4: the window leaves
    the context behind after three steps."""
    from ggml_mi355x.llama import Sampler
    r = tiny
    da, db = r["da"], r["db"]
    ctx = [9, r["plain"][0], 4]
    want, _ = host_loop(db, r["bb"], 1, POS, N_GEN, r["S"], ctx)
    assert want[0] != r["plain"][0]
    assert da.generate(1, POS, N_GEN, sampler=r["S"], context=ctx) == want
    r["ba"].synchronize()
    hist = da.history.cpu().numpy()
    assert (hist[:POS - 3] == -1).all() and hist[POS - 3:POS].tolist() == ctx and hist[POS] == 1
    S4 = Sampler(seed=SEED, presence_penalty=PRESENCE, repeat_last_n=4, **HOT)
    want4, _ = host_loop(db, r["bb"], 1, POS, N_GEN, S4, ctx)
    import torch
    da.history.fill_(77)  # stale entries below the window are never read; those in it are rewritten
    torch.cuda.synchronize()
    assert da.generate(1, POS, N_GEN, sampler=S4, context=ctx) == want4
    r["ba"].synchronize()
    hist = da.history.cpu().numpy()
    assert (hist[:POS - 3] == 77).all() and hist[POS - 3:POS].tolist() == ctx  # entries [pos - 3, pos] alone were written
    # greedy decoding with penalties: temp 0
    Sg = Sampler(temp=0.0, presence_penalty=PRESENCE)
    wantg, _ = host_loop(db, r["bb"], 1, POS, N_GEN, Sg, ctx)
    assert len(set(wantg)) == N_GEN and da.generate(1, POS, N_GEN, sampler=Sg, context=ctx) == wantg


def test_a_ban_of_every_plain_token(tiny):
    from ggml_mi355x.llama import Sampler
    r = tiny
    ban = {t: float("-inf") for t in sorted(set(r["plain"]))}
    S = Sampler(seed=SEED, logit_bias=ban, **HOT)
    assert S.edits() and not S.penalizes()
    want, _ = host_loop(r["db"], r["bb"], 1, POS, N_GEN, S)
    assert not set(want) & set(r["plain"])
    assert r["da"].generate(1, POS, N_GEN, sampler=S) == want
    # another list of the same length in the same graph: the lists are refilled
    ban2 = {t: float("-inf") for t in list(dict.fromkeys(want))[:len(ban)]}
    ban2.update({-1 - i: 1.0 for i in range(len(ban) - len(ban2))})
    S2 = Sampler(seed=SEED, logit_bias=ban2, **HOT)
    want2, _ = host_loop(r["db"], r["bb"], 1, POS, N_GEN, S2)
    assert want2 != want
    n_graphs = len(r["da"]._gen_sampled)
    assert r["da"].generate(1, POS, N_GEN, sampler=S2) == want2
    assert len(r["da"]._gen_sampled) == n_graphs
    assert r["da"].generate(1, POS, N_GEN, sampler=S) == want
    # the bias and the penalties together
    S3 = Sampler(seed=SEED, logit_bias=ban, presence_penalty=PRESENCE, **HOT)
    want3, _ = host_loop(r["db"], r["bb"], 1, POS, N_GEN, S3, r["ctx"])
    assert r["da"].generate(1, POS, N_GEN, sampler=S3, context=r["ctx"]) == want3


def test_a_sampler_without_edits_is_as_before(tiny):
    """No PENALIZE node, no history write below pos + 1, and the tokens of
    tests/test_gpu_generate_sample.py's setup (the same weights, sampler and seed)."""
    import ggml_mi355x as g
    from ggml_mi355x.llama import Sampler
    r, da = tiny, tiny["da"]
    assert r["plain0"] == r["plain0_ref"]
    hist = r["hist0"]
    assert hist[0] == 0 and hist[1:N_GEN + 1].tolist() == r["plain0"] and (hist[N_GEN + 1:] == 0).all()
    assert not r["S0"].edits()
    ops = [n.op for n in da._generate_graph(r["S0"])["nodes"]]
    assert g.OP_PENALIZE not in ops and ops == [n.op for n in da.nodes] + [g.OP_SAMPLE]
    assert [n.op for n in da._generate_graph(r["S"])["nodes"]] == [n.op for n in da.nodes] + [g.OP_PENALIZE, g.OP_SAMPLE]
    da.history.fill_(55)
    fresh(r)  # (synchronizes torch's stream too)
    assert da.generate(1, 0, N_GEN, sampler=Sampler(seed=SEED, repeat_last_n=0, repeat_penalty=1.5, **HOT),
                       context=[1, 2, 3]) == r["plain0"]  # (no window: no edit; the context is ignored)
    r["ba"].synchronize()
    assert int(da.history[0]) == 55
    fresh(r)


def test_launch_counts(tiny):
    """A penalised token is the sampled token's launches plus one kq_penalize_rows before kq_topk."""
    import ggml_mi355x as g
    da, L = tiny["da"], tiny["hp"]["n_layer"]
    da.generate(1, POS, 1, use_graph=False, sampler=tiny["S"], context=tiny["ctx"])
    g.timing_enable(True)
    da.generate(1, POS, 1, use_graph=False, sampler=tiny["S"], context=tiny["ctx"])
    rows = g.timing_read()
    g.timing_enable(False)
    names = [r[0] for r in rows]
    assert len(rows) == 5 * L + 4, names
    assert names[-2:] == ["kq::kq_penalize_rows", "kq::kq_topk"] and names.count("kq::kq_penalize_rows") == 1


# ---------------------------------------------------------------- several sequences
def batch_host_loop(dec, b, tokens, pos, cells, mask, n, S, contexts, n_kv=GB.N_CTX):
    tokens, pos, cells, mask = list(tokens), list(pos), list(cells), np.array(mask, np.float32)
    T = len(tokens)
    draws = [R.draws([S.seed, i], dec.n_ctx + 1) for i in range(T)]
    hists = [start_hist(tokens[i], pos[i], list(contexts[i] or [])) for i in range(T)]
    out, edited = [[] for _ in tokens], None
    for _ in range(n):
        lg = dec.step_batch(tokens, pos, cells, mask, n_kv)
        b.synchronize()
        lg = lg.cpu().numpy()
        edited = np.stack([edit(lg[i], S, window_of(hists[i], pos[i], S.repeat_last_n)) for i in range(T)])
        for i in range(T):
            tokens[i] = R.ref_sample(edited[i], draws[i][pos[i] + 1], **GS.kw_of(S))
            out[i].append(tokens[i])
            pos[i] += 1
            hists[i][pos[i]] = tokens[i]
            cells[i] += 1
            if cells[i] < n_kv:
                mask[i, cells[i]] = 0.0
    return out, edited


def test_generate_batch_equals_the_host_loop_with_the_rule(dev):
    """Three sequences, each with its own context (one empty) and its own position."""
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
        S0 = Sampler(seed=SEED, **HOT)
        pos, cells = [8, 3, 5], [32 * 0 + 8, 32 * 1 + 3, 32 * 2 + 5]
        mask = np.full((T, NC), -np.inf, np.float32)
        for s in range(T):
            mask[s, 32 * s:32 * s + pos[s] + 1] = 0.0
        plain = GS.batch_host_loop(db, bb, GB.START, pos, cells, mask, N_GEN, S0)
        contexts = [[4, plain[0][0], 6, 4, 9, 1, 0, 8], None, [plain[2][0], 12]]
        S = Sampler(seed=SEED, presence_penalty=PRESENCE, freq_penalty=0.5, logit_bias={plain[1][0]: float("-inf")}, **HOT)
        GS.fresh(ba, bb, da, db)
        ref, ref_logits = batch_host_loop(db, bb, GB.START, pos, cells, mask, N_GEN, S, contexts)
        # first the reference alone: every sequence leaves its plain run at step 0 (1: by the ban)
        assert all(ref[i][0] != plain[i][0] for i in range(T)), "an edit did not change a first token"
        toks = da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S, contexts=contexts)
        ba.synchronize()
        assert toks == ref
        sa, sb = GB.state(da), GB.state(db)
        assert bits_equal(sa["logits"], ref_logits), first_mismatch(sa["logits"], ref_logits)
        for i in range(hp["n_layer"]):
            assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
        hist = sa["hist"]
        for s in range(T):
            ctx = contexts[s] or []
            lo = pos[s] - len(ctx)
            assert (hist[s, :lo] == -1).all() and hist[s, lo:pos[s]].tolist() == ctx and hist[s, pos[s]] == GB.START[s]
            assert hist[s, pos[s] + 1:pos[s] + N_GEN + 1].tolist() == toks[s] and (hist[s, pos[s] + N_GEN + 1:] == 0).all()
        # the same again, in chunks and eager; without edits the plain run, whatever the contexts are
        kw = dict(sampler=S, contexts=contexts)
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, chunk=5, **kw) == toks
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, use_graph=False, **kw) == toks
        assert da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S0, contexts=contexts) == plain
        nodes = da._generate_batch_graph(T, NC, 1, S)["nodes"]
        assert [n.op for n in nodes[-2:]] == [g.OP_PENALIZE, g.OP_SAMPLE_BATCH]
        assert g.OP_PENALIZE not in [n.op for n in da._generate_batch_graph(T, NC, 1, S0)["nodes"]]
        with pytest.raises(g.Mi355xError):
            da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S, contexts=contexts[:2])
        with pytest.raises(g.Mi355xError):
            da.generate_batch(GB.START, pos, cells, mask, N_GEN, NC, sampler=S, contexts=[[1] * 9, None, None])
    finally:
        ba.close()
        bb.close()
