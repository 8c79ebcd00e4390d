"""LlamaDecoder.logprobs and .perplexity on the device (the all-rows prompt graph with its
LOGPROB_BATCH node) against tests/logprob_ref.py applied to the logits a second decoder of the
same weights produces with step(), token by token: the records bit for bit, because the prompt
graph's rows already equal step's. The model is tests/test_gpu_generate_batch.py's two-layer hd64
model (n_ctx 128, the smallest vocabulary with three workgroups per row)."""
import math

import numpy as np
import pytest

from tests import logprob_ref as R
from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, N_LONG, N_SHORT = 128, 33, 9
_cache = {}


def step_logits(r, tokens):
    """The logits of every token of `tokens` decoded one by one from position 0 on decoder B: [n, V]."""
    db, bb = r["db"], r["bb"]
    out = np.empty((len(tokens), r["hp"]["n_vocab"]), np.float32)
    for p, t in enumerate(tokens):
        lg = db.step(int(t), p)
        bb.synchronize()
        out[p] = lg.cpu().numpy()
    return out


def caches(dec):
    import torch
    torch.cuda.synchronize()
    return [c.cpu().numpy().copy() for c in dec.k_cache + dec.v_cache]


def setup(dev):
    if _cache:
        return _cache
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    from tests.test_gpu_generate_batch import WIDTHS, vocab
    hp = hparams(*WIDTHS["hd64"], vocab())
    assert hp["n_vocab"] % 4 == 0 and hp["n_vocab"] > 2048  # three blocks of kq_logsum_rows a row
    wd = LM.to_device(LM.build(hp, seed=77), dev)
    ba, bb = g.Backend(), g.Backend()
    r = dict(hp=hp, ba=ba, bb=bb, da=LlamaDecoder(ba, hp, wd, N_CTX), db=LlamaDecoder(bb, hp, wd, N_CTX))
    r["tokens"] = [int(t) for t in np.random.default_rng(5).integers(0, hp["n_vocab"], N_LONG)]
    r["logits"] = step_logits(r, r["tokens"])  # computed once, left unchanged
    r["kv_steps"] = caches(r["db"])
    _cache.update(r)
    return _cache


@pytest.fixture(scope="module")
def tiny(dev):
    return setup(dev)


@pytest.fixture(scope="module", autouse=True)
def close_backends():
    yield
    if _cache:
        _cache["ba"].close()
        _cache["bb"].close()
    _cache.clear()


def fresh(dec, backend):
    import torch
    backend.synchronize()
    dec.reset()
    torch.cuda.synchronize()


def want_records(r, n_tok, lo=0):
    """The rule on rows lo .. n_tok - 2 of the step logits, each row's target the next token."""
    return R.ref_records(r["logits"][lo:n_tok - 1], r["tokens"][lo + 1:n_tok])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("n_tok", [N_SHORT, N_LONG])
def test_logprobs_equal_the_rule_on_step_logits(tiny, n_tok, use_graph):
    import ggml_mi355x as g
    da = tiny["da"]
    fresh(da, tiny["ba"])
    toks = tiny["tokens"][:n_tok]
    got = da.logprobs(toks, use_graph=use_graph, records=True)
    want = want_records(tiny, n_tok)
    assert got.shape == (n_tok - 1,) and R.same_records(got, want), R.first_mismatch(got, want)
    # the graph's own logits are step's rows, and the values are logprob_value of the records
    pg = da._prompt_graph(n_tok, all_rows=True)
    lg = pg["logits"].cpu().numpy()
    assert bits_equal(lg, tiny["logits"][:n_tok]), first_mismatch(lg, tiny["logits"][:n_tok])
    lp = da.logprobs(toks, use_graph=use_graph)
    assert lp.dtype == np.float64 and lp.shape == (n_tok - 1,)
    assert (lp.view(np.uint64) == R.value(want).view(np.uint64)).all() and (lp < 0).all()
    # given targets: one value per row, the last row's too
    tg = [0, tiny["hp"]["n_vocab"] - 1, int(want["argmax"][2])] + toks[4:] + [5]
    rec = da.logprobs(toks, targets=tg, use_graph=use_graph, records=True)
    want_t = R.ref_records(tiny["logits"][:n_tok], tg)
    assert rec.shape == (n_tok,) and R.same_records(rec, want_t), R.first_mismatch(rec, want_t)
    assert rec["x_target"][2] == rec["max"][2]
    assert math.isnan(da.logprobs(toks, targets=[-1] * n_tok)[0])  # outside the vocabulary


def test_kv_caches_and_prompt_after_logprobs(tiny):
    da, db = tiny["da"], tiny["db"]
    toks = tiny["tokens"]
    fresh(da, tiny["ba"])
    da.logprobs(toks)
    kv_lp = caches(da)
    # prompt() after logprobs(): the same bits as on a fresh decoder, and its graph is its own
    la = da.prompt(toks)
    tiny["ba"].synchronize()
    la = la.cpu().numpy()
    fresh(db, tiny["bb"])
    lb = db.prompt(toks)
    tiny["bb"].synchronize()
    lb = lb.cpu().numpy()
    kv_prompt = caches(db)
    assert bits_equal(la, lb), first_mismatch(la, lb)
    assert bits_equal(la, tiny["logits"][N_LONG - 1])
    for i, (a, b, c) in enumerate(zip(kv_lp, kv_prompt, tiny["kv_steps"])):
        assert (a == b).all() and (a == c).all(), i
    assert (da._prompts[N_LONG]["nodes"] is not da._prompts[("all_rows", N_LONG)]["nodes"])
    assert ("all_rows", N_LONG) not in db._prompts


def test_start_pos_continues_a_context(tiny):
    da = tiny["da"]
    toks = tiny["tokens"]
    fresh(da, tiny["ba"])
    cut = 20
    first = da.logprobs(toks[:cut], records=True)
    rest = da.logprobs(toks[cut:], start_pos=cut, records=True)
    assert R.same_records(first, want_records(tiny, cut))
    want = want_records(tiny, N_LONG, lo=cut)
    assert rest.shape == (N_LONG - cut - 1,) and R.same_records(rest, want), R.first_mismatch(rest, want)


def host_perplexity(r, text, n_ctx, bos=None):
    """llama-perplexity's procedure with the rule on step logits: (ppl, nll, count, top1)."""
    nll, count, hits = 0.0, 0, 0
    for c in range(len(text) // n_ctx):
        chunk = text[c * n_ctx:(c + 1) * n_ctx]
        run = ([bos] + chunk[1:]) if bos is not None else chunk
        lg = step_logits(r, run)
        rows = range(n_ctx // 2, n_ctx - 1)
        rec = R.ref_records(lg[rows.start:rows.stop], [chunk[i + 1] for i in rows])
        for v in R.value(rec).tolist():
            nll += -v
        count += len(rec)
        hits += int((rec["argmax"] == [chunk[i + 1] for i in rows]).sum())
    return math.exp(nll / count), nll, count, hits / count


def test_perplexity_equals_the_host_rule(tiny):
    da = tiny["da"]
    V = tiny["hp"]["n_vocab"]
    text = [int(t) for t in np.random.default_rng(6).integers(0, V, 96 + 7)]  # three chunks of 32 and a rest
    seen = []
    got = da.perplexity(text, n_ctx=32, n_batch=16, progress=lambda *a: seen.append(a))
    ppl, nll, count, top1 = host_perplexity(tiny, text, 32)
    assert count == 3 * 15 and got["count"] == count
    assert got["nll"] == nll and got["ppl"] == ppl and got["top1"] == top1, (got, ppl, nll, top1)
    assert [s[:2] for s in seen] == [(1, 3), (2, 3), (3, 3)] and seen[-1][2:] == (nll, count)
    # one batch a chunk and a batch that is no divisor of the chunk give the same records, so the same sums
    for n_batch in (32, 20, 512):
        assert da.perplexity(text, n_ctx=32, n_batch=n_batch) == got, n_batch
    # bos replaces each chunk's first token (one chunk)
    gb = da.perplexity(text[:40], n_ctx=32, n_batch=32, bos=7)
    ppl, nll, count, top1 = host_perplexity(tiny, text[:32], 32, bos=7)
    assert (gb["ppl"], gb["nll"], gb["count"], gb["top1"]) == (ppl, nll, count, top1)
    assert gb["nll"] != da.perplexity(text[:40], n_ctx=32, n_batch=32)["nll"] or text[0] == 7


def test_launch_count(tiny):
    """The all-rows graph is the launches of its own nodes without the LOGPROB_BATCH node (the
    prompt graph without the row selection) plus two, kq_argmax_rows and kq_logsum_rows; prompt()
    on the same decoder has neither."""
    import ggml_mi355x as g
    da, ba = tiny["da"], tiny["ba"]
    toks = tiny["tokens"][:N_SHORT]
    da.logprobs(toks, use_graph=False)
    g.timing_enable(True)
    da.logprobs(toks, use_graph=False)
    lp = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    pg = da._prompt_graph(N_SHORT, all_rows=True)
    g.timing_enable(True)
    assert ba.graph_compute(pg["nodes"][:-1], use_graph=False) == 0
    plain = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    g.timing_enable(True)
    da.prompt(toks, use_graph=False)
    prompt = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    assert len(plain) >= 5 and not any("argmax" in n or "logsum" in n for n in plain + prompt), (plain, prompt)
    assert lp == plain + ["kq::kq_argmax_rows", "kq::kq_logsum_rows"], (lp, plain)
