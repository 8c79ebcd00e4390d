"""LlamaDecoder.generate_batch: greedy decoding of three sequences together with the tokens
picked on the device (a step-inputs ARGMAX_BATCH node ends each step and stages the next: tokens,
positions, cells and the new cell in its own mask row), against the loop a user had to write
before on a second decoder of the same weights (step_batch, synchronize, logits to the host,
numpy argmax per row, the mask rebuilt on the host), and against the CPU oracle decoding each
sequence alone. The model and the layout are those of tests/test_gpu_batch_token.py (sequence s
owns the cells [32 s, 32 s + 32): cell = 32 s + position, for which that file's docstring proves
each row equal to the sequence decoded alone), with the smallest vocabulary whose argmax runs on
at least 3 workgroups per row. Two layers, n_ctx 128."""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch

pytestmark = pytest.mark.gpu

N_CTX, N_SEQ, N_GEN, N_ORACLE = 128, 3, 12, 6
WIDTHS = {"hd64": (512, 2, 8, 2, 768), "hd128": (1024, 2, 8, 2, 2816)}
START = [7, 511, 2]  # the sequences' first tokens
_cache = {}


def ref_argmax(x):
    return int(np.argmax(np.where(np.isnan(x), -np.inf, x)))


def vocab():
    import ggml_mi355x as g
    v = 256
    while g.argmax_plan(v)[0] < 3:
        v += 256
    return v


def block_start(p=0):
    """Every sequence at position p of its own 32-cell block: (pos, cells, mask)."""
    mask = np.full((N_SEQ, N_CTX), -np.inf, np.float32)
    for s in range(N_SEQ):
        mask[s, 32 * s:32 * s + p + 1] = 0.0
    return [p] * N_SEQ, [32 * s + p for s in range(N_SEQ)], mask


def interleaved_start():
    """cell_stride 3: sequence s on the cells s, s + 3, ..."""
    mask = np.full((N_SEQ, N_CTX), -np.inf, np.float32)
    for s in range(N_SEQ):
        mask[s, s] = 0.0
    return [0] * N_SEQ, list(range(N_SEQ)), mask


def host_loop(dec, b, tokens, pos, cells, mask, n, n_kv=N_CTX, cell_stride=1):
    """What a user writes without generate_batch: per step one synchronization, the logits to the
    host, numpy's argmax per row and the mask rebuilt and copied again."""
    tokens, pos, cells, mask = list(tokens), list(pos), list(cells), np.array(mask, np.float32)
    out = [[] for _ in tokens]
    for _ in range(n):
        lg = dec.step_batch(tokens, pos, cells, mask, n_kv)
        b.synchronize()
        lg = lg.cpu().numpy()
        for i in range(len(tokens)):
            tokens[i] = ref_argmax(lg[i])
            out[i].append(tokens[i])
            pos[i] += 1
            cells[i] += cell_stride
            if cells[i] < n_kv:
                mask[i, cells[i]] = 0.0
    return out, (tokens, pos, cells, mask)


def state(dec, n_kv=N_CTX):
    import torch
    torch.cuda.synchronize()
    g = dec._batches[(N_SEQ, n_kv)]
    hist = dec.batch_history.cpu().numpy().copy() if hasattr(dec, "batch_history") else None
    return dict(logits=g["logits"].cpu().numpy().copy(), inp=g["inp"].cpu().numpy().copy(), hist=hist,
                k=[c.cpu().numpy().copy() for c in dec.k_cache], v=[c.cpu().numpy().copy() for c in dec.v_cache])


def same_state(a, b, n_layer):
    for i in range(n_layer):
        assert (a["k"][i] == b["k"][i]).all() and (a["v"][i] == b["v"][i]).all(), i
    assert (a["inp"] == b["inp"]).all()
    assert (a["hist"] == b["hist"]).all()
    assert bits_equal(a["logits"], b["logits"])


def setup(dev, name):
    """One run per width, shared by the tests: decoder A generates, decoder B runs the host loop,
    the oracle decodes each sequence's first tokens alone. The results are kept as host copies."""
    if name in _cache:
        return _cache[name]
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    O.lib()
    hp = hparams(*WIDTHS[name], vocab())
    w = LM.build(hp, seed=77)
    wd = LM.to_device(w, dev)
    ba, bb = g.Backend(), g.Backend()
    da, db = LlamaDecoder(ba, hp, wd, N_CTX), LlamaDecoder(bb, hp, wd, N_CTX)
    pos, cells, mask = block_start()
    toks = da.generate_batch(START, pos, cells, mask, N_GEN, N_CTX)
    ba.synchronize()
    sa = state(da)
    ref, _ = host_loop(db, bb, START, pos, cells, mask, N_GEN)
    sb = state(db)
    otoks = []
    for s in range(N_SEQ):
        model, cache = LM.oracle_model(hp, w, 32)
        tok, seq = START[s], []
        for p in range(N_ORACLE):
            lg, _ = O.decode_token(model, tok, p, cache)
            tok = ref_argmax(lg)
            seq.append(tok)
        otoks.append(seq)
    r = dict(hp=hp, da=da, db=db, ba=ba, bb=bb, toks=toks, ref=ref, sa=sa, sb=sb, otoks=otoks)
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


def fresh(r):
    """Both decoders' caches zeroed: what a test leaves in cells that a later one shows cannot differ."""
    import torch
    r["ba"].synchronize()
    r["bb"].synchronize()
    r["da"].reset()
    r["db"].reset()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(WIDTHS))
def test_generate_batch_equals_host_loop_and_oracle(dev, name):
    r = setup(dev, name)
    toks = r["toks"]
    assert len(toks) == N_SEQ and all(len(t) == N_GEN and all(isinstance(x, int) for x in t) for t in toks)
    assert toks == r["ref"]
    sa, sb = r["sa"], r["sb"]
    assert bits_equal(sa["logits"], sb["logits"]), first_mismatch(sa["logits"], sb["logits"])
    for i in range(r["hp"]["n_layer"]):
        assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
    assert [t[:N_ORACLE] for t in toks] == r["otoks"]
    assert len({tuple(t) for t in toks}) == N_SEQ  # the sequences differ: a row mix-up would show
    # the history: the token picked at position p in entry p + 1, zeros elsewhere
    hist = sa["hist"]
    assert hist.shape == (N_SEQ, N_CTX + 1)
    for s in range(N_SEQ):
        assert hist[s, 1:N_GEN + 1].tolist() == toks[s] and hist[s, 0] == 0 and (hist[s, N_GEN + 1:] == 0).all()
    # the input block is left staged for a 13th step; the mask rows show exactly cells 32 s .. 32 s + 12
    T, inp = N_SEQ, sa["inp"]
    assert inp[:T].tolist() == [t[-1] for t in toks]
    assert inp[T:2 * T].tolist() == [N_GEN] * T
    assert inp[2 * T:3 * T].tolist() == [32 * s + N_GEN for s in range(T)]
    want = np.full((T, N_CTX), -np.inf, np.float32)
    for s in range(T):
        want[s, 32 * s:32 * s + N_GEN + 1] = 0.0
    assert (inp[3 * T:].view(np.uint32) == want.view(np.uint32).ravel()).all()


@pytest.mark.parametrize("kw", [dict(chunk=5), dict(chunk=1), dict(use_graph=False), dict(chunk=5, use_graph=False)],
                         ids=["chunk5", "chunk1", "eager", "eager-chunk5"])
def test_chunks_and_eager_give_the_same_tokens(tiny, kw):
    pos, cells, mask = block_start()
    assert tiny["da"].generate_batch(START, pos, cells, mask, N_GEN, N_CTX, **kw) == tiny["toks"]


def test_interleaved_cells(tiny):
    """cell_stride 3: the sequences' cells alternate, so only the host loop is the reference."""
    fresh(tiny)
    pos, cells, mask = interleaved_start()
    got = tiny["da"].generate_batch(START, pos, cells, mask, N_GEN, N_CTX, cell_stride=3)
    ref, (_, rpos, rcells, rmask) = host_loop(tiny["db"], tiny["bb"], START, pos, cells, mask, N_GEN, cell_stride=3)
    assert got == ref
    sa, sb = state(tiny["da"]), state(tiny["db"])
    assert bits_equal(sa["logits"], sb["logits"]), first_mismatch(sa["logits"], sb["logits"])
    for i in range(tiny["hp"]["n_layer"]):
        assert (sa["k"][i] == sb["k"][i]).all() and (sa["v"][i] == sb["v"][i]).all(), i
    T, inp = N_SEQ, sa["inp"]
    assert inp[T:2 * T].tolist() == rpos and inp[2 * T:3 * T].tolist() == rcells == [s + 3 * N_GEN for s in range(T)]
    assert (inp[3 * T:].view(np.uint32) == rmask.view(np.uint32).ravel()).all()


def test_eos_ends_one_sequence(tiny):
    toks = tiny["toks"]
    s = next((s for s in range(N_SEQ) if toks[s][3] not in toks[s][:3] and
              any(toks[s][3] not in toks[o] for o in range(N_SEQ) if o != s)), None)
    assert s is not None, "every sequence repeats its 4th token earlier, or every other one meets it: pick another seed"
    eos = toks[s][3]
    want = [t[:t.index(eos) + 1] if eos in t else t for t in toks]
    assert want[s] == toks[s][:4] and any(len(w) == N_GEN for w in want)
    pos, cells, mask = block_start()
    for chunk in (32, 3):  # eos inside the first chunk, and in the second
        assert tiny["da"].generate_batch(START, pos, cells, mask, N_GEN, N_CTX, eos=eos, chunk=chunk) == want
    assert tiny["da"].generate_batch(START, pos, cells, mask, 0, N_CTX) == [[], [], []]


def test_end_of_the_cache_and_refusals(tiny):
    import ggml_mi355x as g
    da, db = tiny["da"], tiny["db"]
    fresh(tiny)
    pos, cells, mask = block_start(29)  # 3 cells before the end of every sequence's block
    got = da.generate_batch([5, 6, 7], pos, cells, mask, 3, N_CTX)
    ref, (rtok, rpos, rcells, _) = host_loop(db, tiny["bb"], [5, 6, 7], pos, cells, mask, 3)
    assert got == ref
    before = state(da)
    T = N_SEQ
    assert before["inp"][T:2 * T].tolist() == [32] * T  # pos + 1 and the next cell are written even there
    assert before["inp"][2 * T:3 * T].tolist() == [32 * s + 32 for s in range(T)]
    assert bits_equal(before["logits"], state(db)["logits"])

    p0, c0, m0 = block_start()
    seen = m0.copy()
    seen[1, 5] = 0.0  # a cell sequence 0 will write, visible to sequence 1
    own = m0.copy()
    own[0, 1] = 0.0  # ... and one visible to its own sequence before its turn
    refused = [
        dict(pos=pos, cells=cells, mask=mask, n=4),                     # the 4th step enters the next block, seen there
        dict(pos=p0, cells=c0, mask=seen, n=N_GEN),
        dict(pos=p0, cells=c0, mask=own, n=N_GEN),
        dict(pos=p0, cells=[0, 6, 64], mask=np.full((T, N_CTX), -np.inf, np.float32), n=N_GEN),  # cells 6 .. 11 twice
        dict(pos=p0, cells=c0, mask=m0, n=N_GEN, n_kv=100),             # n_kv no multiple of 32
        dict(pos=p0, cells=c0, mask=m0, n=-1),
        dict(pos=p0, cells=c0, mask=m0, n=2, chunk=0),
        dict(pos=p0, cells=c0, mask=m0, n=2, cell_stride=0),
        dict(pos=[N_CTX - 1] * T, cells=c0, mask=m0, n=2),              # the positions leave the rope table
        dict(pos=p0, cells=[0, 32, N_CTX - 2], mask=m0, n=2, cell_stride=3),
    ]
    for kw in refused:
        kw = dict(kw)
        args = (kw.pop("pos"), kw.pop("cells"), kw.pop("mask"), kw.pop("n"), kw.pop("n_kv", N_CTX))
        with pytest.raises(g.Mi355xError):
            da.generate_batch([5, 6, 7], *args, **kw)
    da.split = object()  # a row split
    try:
        with pytest.raises(g.Mi355xError):
            da.generate_batch([5, 6, 7], p0, c0, m0, 2, N_CTX)
    finally:
        da.split = None
    assert (N_SEQ, 100) not in da._batches  # refused before a graph was built
    same_state(state(da), before, tiny["hp"]["n_layer"])


def test_step_batch_after_generate_batch(tiny):
    """step_batch restages the whole block: the 7th step equals the host-loop decoder's, bit for bit."""
    da, db = tiny["da"], tiny["db"]
    fresh(tiny)
    pos, cells, mask = block_start()
    got = da.generate_batch(START, pos, cells, mask, N_ORACLE, N_CTX)
    ref, (tok, rpos, rcells, rmask) = host_loop(db, tiny["bb"], START, pos, cells, mask, N_ORACLE)
    assert got == ref == tiny["otoks"]
    la = da.step_batch(tok, rpos, rcells, rmask, N_CTX)
    tiny["ba"].synchronize()
    la = la.cpu().numpy()
    lb = db.step_batch(tok, rpos, rcells, rmask, N_CTX)
    tiny["bb"].synchronize()
    lb = lb.cpu().numpy()
    assert bits_equal(la, lb), first_mismatch(la, lb)
    assert [ref_argmax(la[s]) for s in range(N_SEQ)] == [t[N_ORACLE] for t in tiny["toks"]]


def test_launch_count(tiny):
    """One generate_batch step is the launches of one step_batch step plus one, the argmax; a plain
    step_batch on the same decoder keeps its count and has no argmax launch."""
    import ggml_mi355x as g
    da = tiny["da"]
    pos, cells, mask = block_start()
    da.generate_batch(START, pos, cells, mask, 1, N_CTX, use_graph=False)
    g.timing_enable(True)
    da.generate_batch(START, pos, cells, mask, 1, N_CTX, use_graph=False)
    gen = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    g.timing_enable(True)
    da.step_batch(START, pos, cells, mask, N_CTX, use_graph=False)
    step = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    assert len(step) >= 5 and not any("argmax" in n for n in step), step
    assert gen == step + ["kq::kq_argmax_rows"], (gen, step)
