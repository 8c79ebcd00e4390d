"""LlamaDecoder.shift and generate(keep=): the context shift on the decoder's own caches against
tests/kv_shift_ref.py and the CPU oracle, and generation past the end of the cache against the loop
a user writes with step, a host-side pick, an explicit shift and restaging at the same points, on a
second decoder of the same weights. The model, width and vocabulary are those of
tests/test_gpu_generate.py (two layers, n_ctx 64)."""
import numpy as np
import pytest

from tests import kv_shift_ref as K
from tests import penalize_ref as P
from tests import sample_ref as R
from tests import test_gpu_generate as G
from tests import test_gpu_generate_sample as GS
from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, KEEP, N_LONG = G.N_CTX, 4, 150
_cache = {}


def setup(dev):
    if _cache:
        return _cache["r"]
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    O.lib()
    hp = hparams(*G.WIDTHS["hd64"], G.vocab())
    w = LM.build(hp, seed=21)
    wd = LM.to_device(w, dev)
    ba, bb = g.Backend(), g.Backend()
    da, db = LlamaDecoder(ba, hp, wd, N_CTX), LlamaDecoder(bb, hp, wd, N_CTX)
    r = _cache["r"] = dict(hp=hp, w=w, da=da, db=db, ba=ba, bb=bb)
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


def fresh(r):
    GS.fresh(r["ba"], r["bb"], r["da"], r["db"])


def host_loop(r, token, n, pick, keep=KEEP, discard=None, on_shift=None):
    """Decoder B: step, synchronize, the logits to the host, pick(logits, pos, epoch) -> token, and
    at a full cache an explicit shift; the next step restages the inputs at the new position."""
    db, bb = r["db"], r["bb"]
    out, pos, epoch = [], 0, 0
    while len(out) < n:
        db.step(token, pos)
        bb.synchronize()
        token = pick(db.logits.cpu().numpy(), pos, epoch)
        out.append(token)
        pos += 1
        if pos == N_CTX and len(out) < n:
            d = discard or (N_CTX - keep) // 2
            db.shift(N_CTX, keep, d)
            epoch += 1
            pos = N_CTX - d
            if on_shift:
                on_shift(token, d)
    return out


def greedy(lg, pos, epoch):
    return G.ref_argmax(lg)


def test_shift_equals_the_reference_and_the_oracle(tiny):
    """Both caches of every layer after shift(64, 4, 30) are the reference applied to a copy read
    back before it, and the token after it is the oracle's on those caches, bit for bit."""
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    r, da = tiny, tiny["da"]
    hp, hd = r["hp"], r["hp"]["head_dim"]
    fresh(r)
    toks = da.generate(1, 0, N_CTX)  # every cell written
    before = G.state(da)
    hist, inp = da.history.cpu().numpy().copy(), before["inp"]
    model, cache = LM.oracle_model(hp, r["w"], N_CTX)
    tab = model["rope_table"]
    assert (tab.view(np.int32).reshape(N_CTX, hd) == da._table_host.numpy()).all()  # the decoder's own table
    da.shift(N_CTX, KEEP, 30)
    after = G.state(da)
    for i in range(hp["n_layer"]):
        k, v = before["k"][i].view(np.uint16), before["v"][i].view(np.uint16)
        assert k.any(axis=1).all()
        wk, wv = K.shift_discard(k, v, tab, hd, KEEP, 30, N_CTX)
        gk, gv = after["k"][i].view(np.uint16), after["v"][i].view(np.uint16)
        assert (gk == wk).all() and (gv == wv).all(), (i, np.argwhere(gk != wk)[:4], np.argwhere(gv != wv)[:4])
        assert not (gk[KEEP:34] == k[KEEP:34]).all(axis=1).any() and (gk[34:] == k[34:]).all() and (gk[:KEEP] == k[:KEEP]).all()
        cache[i] = (wk.copy(), wv.copy())
    # shift leaves the history, the draws and the input block alone
    assert (after["inp"] == inp).all() and (da.history.cpu().numpy() == hist).all()
    da.step(toks[-1], 34)
    r["ba"].synchronize()
    got = da.logits.cpu().numpy()
    want, _ = O.decode_token(model, toks[-1], 34, cache)
    assert bits_equal(got, want), first_mismatch(got, want)


def test_generate_past_the_end_equals_the_host_loop(tiny):
    r, da = tiny, tiny["da"]
    fresh(r)
    want = host_loop(r, 1, N_LONG, greedy)
    assert len(set(want)) > 8  # (a run that left its first tokens behind)
    r["want"] = want
    sb = G.state(r["db"])
    fresh(r)
    got = da.generate(1, 0, N_LONG, keep=KEEP)
    assert len(got) == N_LONG and all(isinstance(t, int) for t in got)
    assert got == want
    # three shifts: positions 64 -> 34 three times, 150 = 64 + 30 + 30 + 26
    r["ba"].synchronize()
    assert int(da.inp.cpu()[1]) == 34 + 26 and int(da.inp.cpu()[0]) == got[-1]
    hist = da.history.cpu().numpy()
    assert hist[35:35 + 26].tolist() == got[-26:] and hist[34] == got[-27]
    # the tokens that moved down with their cells at the third shift: those of positions [34, 64), which are
    # the second run's last token and the third run's first 29
    assert hist[KEEP:34].tolist() == got[93:123]
    sa = G.state(da)
    for i in range(r["hp"]["n_layer"]):
        assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i


@pytest.mark.parametrize("kw", [dict(chunk=1), dict(chunk=7), dict(chunk=32), dict(chunk=1, use_graph=False),
                                dict(chunk=7, use_graph=False), dict(chunk=32, use_graph=False)],
                         ids=["chunk1", "chunk7", "chunk32", "eager-chunk1", "eager-chunk7", "eager-chunk32"])
def test_chunks_and_eager_give_the_same_tokens(tiny, kw):
    r = tiny
    if "want" not in r:
        fresh(r)
        r["want"] = host_loop(r, 1, N_LONG, greedy)
    fresh(r)
    assert r["da"].generate(1, 0, N_LONG, keep=KEEP, **kw) == r["want"]


def test_another_discard_and_eos(tiny):
    r, da = tiny, tiny["da"]
    for keep, discard, n in ((0, 1, 70), (10, 54, 130), (62, 2, 70), (0, 64, 70)):
        fresh(r)
        want = host_loop(r, 1, n, greedy, keep=keep, discard=discard)
        fresh(r)
        assert da.generate(1, 0, n, keep=keep, discard=discard, chunk=9) == want, (keep, discard)
    want = r.get("want") or host_loop(r, 1, N_LONG, greedy)
    eos = want[100]
    first = want.index(eos)
    fresh(r)
    assert da.generate(1, 0, N_LONG, keep=KEEP, eos=eos) == want[:first + 1]


def test_sampled_generation_takes_fresh_draws_after_a_shift(tiny):
    from ggml_mi355x.llama import Sampler
    r, da = tiny, tiny["da"]
    S = Sampler(seed=3, **GS.HOT)
    draws = [R.draws(3, N_CTX + 1)] + [R.draws([3, 0, e], N_CTX + 1) for e in (1, 2, 3)]
    assert (S.draws(N_CTX + 1, epoch=2) == draws[2]).all()

    def pick(lg, pos, epoch):
        return R.ref_sample(lg, draws[epoch][pos + 1], **GS.kw_of(S))

    fresh(r)
    want = host_loop(r, 1, N_LONG, pick)
    stale = host_loop(r, 1, N_LONG, lambda lg, pos, epoch: R.ref_sample(lg, draws[0][pos + 1], **GS.kw_of(S)))
    assert want[:N_CTX] == stale[:N_CTX] and want != stale, "the epochs' draws changed nothing: pick another seed"
    for kw in (dict(), dict(chunk=7), dict(chunk=1, use_graph=False)):
        fresh(r)
        assert da.generate(1, 0, N_LONG, keep=KEEP, sampler=S, **kw) == want, kw
    # a following call without a shift starts from epoch 0 again
    fresh(r)
    assert da.generate(1, 0, 20, sampler=S) == want[:20]


def test_penalised_generation_moves_the_history(tiny):
    """repeat_last_n 16: after a shift the window holds the 16 tokens that stand before the new
    position, the last one picked on the last cell."""
    from ggml_mi355x.llama import Sampler
    r, da = tiny, tiny["da"]
    S = Sampler(repeat_penalty=1.3, repeat_last_n=16)
    draws = [R.draws(S.seed, N_CTX + 1)] + [R.draws([S.seed, 0, e], N_CTX + 1) for e in (1, 2, 3)]
    hist = {0: 1}

    def pick(lg, pos, epoch):
        win = [hist[j] for j in range(max(0, pos - 15), pos + 1)]
        lg = P.penalize_row(lg, win, S.repeat_penalty, S.freq_penalty, S.presence_penalty, S.logit_bias)[0]
        hist[pos + 1] = R.ref_sample(lg, draws[epoch][pos + 1], **GS.kw_of(S))
        return hist[pos + 1]

    def on_shift(last, d):
        moved = {p - d: hist[p] for p in range(KEEP + d, N_CTX)}
        hist.update(moved)
        hist[N_CTX - d] = last

    def unpenalised(lg, pos, epoch):
        return R.ref_sample(lg, draws[epoch][pos + 1], **GS.kw_of(S))

    fresh(r)
    want = host_loop(r, 1, N_LONG, pick, on_shift=on_shift)
    fresh(r)
    assert want != host_loop(r, 1, N_LONG, unpenalised), "the penalty changed nothing: pick other parameters"
    for kw in (dict(), dict(chunk=5), dict(use_graph=False)):
        fresh(r)
        assert da.generate(1, 0, N_LONG, keep=KEEP, sampler=S, **kw) == want, kw
    r["ba"].synchronize()
    h = da.history.cpu().numpy()
    assert h[KEEP:34 + 26 + 1].tolist() == [hist[p] for p in range(KEEP, 34 + 26 + 1)]


def test_without_keep_and_short_of_the_end_nothing_changes(tiny):
    import ggml_mi355x as g
    r, da = tiny, tiny["da"]
    fresh(r)
    want = G.host_loop(r["db"], r["bb"], 1, 0, 20)
    fresh(r)
    assert da.generate(1, 0, 20) == want
    fresh(r)
    n_shifts = len(da._shifts)
    assert da.generate(1, 0, 20, keep=KEEP) == want
    fresh(r)
    assert da.generate(1, 44, 20, keep=KEEP, discard=7) == G.host_loop(r["db"], r["bb"], 1, 44, 20)  # ends on the last cell
    assert len(da._shifts) == n_shifts  # never reached the end: no shift was built or run
    assert [n.op for n in da._generate_graph(None)["nodes"]] == [n.op for n in da.nodes] + [g.OP_ARGMAX]
    assert da._generate_graph(None) is da._gen
    with pytest.raises(g.Mi355xError):
        da.generate(1, 44, 21)  # the refusal without keep
