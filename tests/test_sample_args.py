"""mi355x_topk / mi355x_sample and their rows forms without a device: the error order (E_INVAL,
then E_WORKSPACE, then E_NODEVICE, all before any device access), every parameter bound, the
workspace sizes, and the node list LlamaDecoder builds for generate with and without a sampler
(describe-only decoders: host tensors, no device work)."""
import ctypes

import numpy as np
import pytest

X, IDX, VAL, U, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
ROW = 131200  # the counter's 128-B line + 256 slices x 64 words


@pytest.fixture(scope="module")
def L():
    import ggml_mi355x as g
    return g.lib()


def sampler(top_k=40, temp=0.8, top_p=0.95, min_p=0.05):
    import ggml_mi355x as g
    return ctypes.byref(g.SamplerDesc(top_k, temp, top_p, min_p))


def no_device_rc():
    import ggml_mi355x as g
    return g.E_NODEVICE if not g.device_available() else None


def test_workspace_sizes(L):
    import ggml_mi355x as g
    for n in (1, 3, 1024, 32000, 128256, 1 << 24):
        assert g.topk_workspace_size(n) == ROW  # whatever n is, and there is no top_k to depend on
        assert g.topk_workspace_size(n, 3) == 3 * ROW
    assert g.topk_workspace_size(32000, 65535) == 65535 * ROW
    for n, rows in ((0, 1), (-1, 1), ((1 << 24) + 1, 1), (5, 0), (5, -2), (5, 65536)):
        assert g.topk_workspace_size(n, rows) == 0
    assert ROW % 128 == 0 and g.SAMPLE_MAX_K == 64


def test_topk_error_order(L):
    import ggml_mi355x as g
    n = 3000
    ok = (X, n, 40, IDX, VAL, WS, ROW, None)

    def call(**kw):
        a = dict(x=X, n=n, k=40, idx=IDX, val=VAL, ws=WS, size=ROW)
        a.update(kw)
        return L.mi355x_topk(a["x"], a["n"], a["k"], a["idx"], a["val"], a["ws"], a["size"], None)

    for bad in (dict(x=None), dict(x=X + 4), dict(n=0), dict(n=(1 << 24) + 1), dict(k=0), dict(k=65), dict(k=-1),
                dict(idx=None), dict(val=None)):
        assert call(**bad) == g.E_INVAL, bad
        assert call(ws=None, **bad) == g.E_INVAL, bad  # E_INVAL comes first
    for bad in (dict(ws=None), dict(ws=WS + 4), dict(size=ROW - 1), dict(size=0)):
        assert call(**bad) == g.E_WORKSPACE, bad
    if no_device_rc() is not None:
        assert L.mi355x_topk(*ok) == g.E_NODEVICE
        assert call(k=1) == g.E_NODEVICE and call(k=64) == g.E_NODEVICE and call(n=1) == g.E_NODEVICE


def test_topk_rows_error_order(L):
    import ggml_mi355x as g
    n, rows = 3000, 3

    def call(**kw):
        a = dict(x=X, n=n, rows=rows, stride=n, k=8, idx=IDX, val=VAL, ws=WS, size=rows * ROW)
        a.update(kw)
        return L.mi355x_topk_rows(a["x"], a["n"], a["rows"], a["stride"], a["k"], a["idx"], a["val"], a["ws"], a["size"],
                                  None)

    for bad in (dict(x=None), dict(x=X + 8), dict(n=0), dict(rows=0), dict(rows=65536), dict(stride=n - 4),
                dict(stride=n + 2), dict(k=0), dict(k=65), dict(idx=None), dict(val=None)):
        assert call(**bad) == g.E_INVAL, bad
        assert call(size=0, **bad) == g.E_INVAL, bad
    for bad in (dict(ws=None), dict(size=rows * ROW - 1), dict(size=ROW)):
        assert call(**bad) == g.E_WORKSPACE, bad
    if no_device_rc() is not None:
        assert call() == g.E_NODEVICE and call(stride=n + 4) == g.E_NODEVICE


BAD_SAMPLERS = [dict(top_k=0), dict(top_k=65), dict(top_k=-3), dict(temp=-0.5), dict(temp=float("inf")),
                dict(temp=float("nan")), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan")),
                dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan"))]
GOOD_SAMPLERS = [dict(), dict(top_k=1), dict(top_k=64), dict(temp=0.0), dict(temp=1e30), dict(top_p=1.0),
                 dict(top_p=1e-30), dict(min_p=0.0), dict(min_p=1.0)]


def test_sample_error_order_and_bounds(L):
    import ggml_mi355x as g
    n = 3000

    def call(sp=None, **kw):
        a = dict(x=X, n=n, u=U, out=OUT, ws=WS, size=ROW)
        a.update(kw)
        return L.mi355x_sample(a["x"], a["n"], sampler(**(sp or {})), a["u"], a["out"], a["ws"], a["size"], None)

    for bad in (dict(x=None), dict(x=X + 4), dict(n=0), dict(u=None), dict(out=None)):
        assert call(**bad) == g.E_INVAL, bad
        assert call(ws=None, **bad) == g.E_INVAL, bad
    assert L.mi355x_sample(X, n, None, U, OUT, WS, ROW, None) == g.E_INVAL
    for sp in BAD_SAMPLERS:
        assert call(sp) == g.E_INVAL, sp
        assert call(sp, ws=None) == g.E_INVAL, sp
    for sp in GOOD_SAMPLERS:
        assert call(sp, ws=None) == g.E_WORKSPACE, sp
        assert call(sp, size=ROW - 1) == g.E_WORKSPACE, sp
        if no_device_rc() is not None:
            assert call(sp) == g.E_NODEVICE, sp


def test_sample_rows_error_order(L):
    import ggml_mi355x as g
    n, rows = 3000, 2

    def call(sp=None, **kw):
        a = dict(x=X, n=n, rows=rows, stride=n, u=U, out=OUT, ws=WS, size=rows * ROW)
        a.update(kw)
        return L.mi355x_sample_rows(a["x"], a["n"], a["rows"], a["stride"], sampler(**(sp or {})), a["u"], a["out"], a["ws"],
                                    a["size"], None)

    for bad in (dict(x=None), dict(rows=0), dict(stride=n - 4), dict(stride=n + 1), dict(u=None), dict(out=None)):
        assert call(**bad) == g.E_INVAL, bad
    for sp in BAD_SAMPLERS:
        assert call(sp, ws=None) == g.E_INVAL, sp
    assert L.mi355x_sample_rows(X, n, rows, n, None, U, OUT, WS, rows * ROW, None) == g.E_INVAL
    assert call(size=ROW) == g.E_WORKSPACE and call(ws=None) == g.E_WORKSPACE
    if no_device_rc() is not None:
        assert call() == g.E_NODEVICE


def test_sampler_object_bounds():
    import ggml_mi355x as g
    from ggml_mi355x.llama import Sampler
    s = Sampler()
    assert (s.top_k, s.top_p, s.min_p, s.temp, s.seed) == (40, 0.95, 0.05, 0.8, 0)  # llama.cpp's defaults
    assert s.params() == [g.SAMPLE_STEP_INPUTS, 40, g.f32_bits(0.8), g.f32_bits(0.95), g.f32_bits(0.05)]
    for sp in BAD_SAMPLERS:
        with pytest.raises(g.Mi355xError):
            Sampler(**sp)
    for sp in GOOD_SAMPLERS:
        Sampler(**sp)
    # the draws: numpy's PCG64 float32 stream of the seed, a batch's row i seeded [seed, i]
    d = Sampler(seed=7).draws(65)
    assert d.dtype == np.float32 and (d == np.random.Generator(np.random.PCG64(7)).random(65, dtype=np.float32)).all()
    assert (Sampler(seed=7).draws(9, 2) == np.random.Generator(np.random.PCG64([7, 2])).random(9, dtype=np.float32)).all()
    assert (0 <= d).all() and (d < 1).all()


def test_supports_op_checks_the_sampler_where_the_node_is_enqueued():
    import ggml_mi355x as g
    g.lib()
    n = 3000
    x = g.make_tensor(g.TYPE_F32, n, 1, X)
    u = g.make_tensor(g.TYPE_F32, 1, 1, U)

    def node(params, srcs=None):
        return g.make_tensor(g.TYPE_I32, 1, 1, OUT, op=g.OP_SAMPLE, srcs=srcs or [x, u], op_params=params,
                             flags=g.FLAG_OUTPUT)

    assert g.supports_op(node(g.sampler_params(g.SAMPLE_PLAIN, 40, 0.8, 0.95, 0.05)))
    assert not g.supports_op(node(g.sampler_params(g.SAMPLE_PLAIN, 65, 0.8, 0.95, 0.05)))
    assert not g.supports_op(node(g.sampler_params(g.SAMPLE_PLAIN, 40, -1.0, 0.95, 0.05)))
    assert not g.supports_op(node(g.sampler_params(g.SAMPLE_PLAIN, 40, 0.8, 0.0, 0.05)))
    assert not g.supports_op(node(g.sampler_params(g.SAMPLE_PLAIN, 40, 0.8, 0.95, 1.5)))
    assert not g.supports_op(node(g.sampler_params(2, 40, 0.8, 0.95, 0.05)))
    assert not g.supports_op(node(g.sampler_params(g.SAMPLE_PLAIN, 40, 0.8, 0.95, 0.05), srcs=[x]))  # no draw
    # the batch op: rows of a multiple of 4 entries, one draw a row
    T, nb = 3, 3000
    xb = g.make_tensor(g.TYPE_F32, nb, T, X)
    ub = g.make_tensor(g.TYPE_F32, T, 1, U)
    nodeb = g.make_tensor(g.TYPE_I32, T, 1, OUT, op=g.OP_SAMPLE_BATCH, srcs=[xb, ub],
                          op_params=g.sampler_params(g.SAMPLE_PLAIN, 8, 1.0, 1.0, 0.0), flags=g.FLAG_OUTPUT)
    assert g.supports_op(nodeb)
    nodeb.src[1] = ctypes.pointer(u)
    assert not g.supports_op(nodeb)


def ops(nodes):
    return [n.op for n in nodes]


def test_generate_node_lists():
    """With a sampler the generate node list ends in OP_SAMPLE with the stated op_params and the
    draws as its last source; with sampler=None it is today's list, op for op."""
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder, Sampler
    from tests import llama_graph_sig as S
    dec = LlamaDecoder(None, S.HP, S._weights(), S.N_CTX)
    hd = S.HP["head_dim"]
    greedy = dec._generate_graph()["nodes"]
    assert ops(greedy) == ops(dec.nodes) + [g.OP_ARGMAX]
    assert list(greedy[-1].op_params)[:2] == [g.ARGMAX_STEP_INPUTS, 0] and not greedy[-1].src[4]
    sp = Sampler(top_k=12, top_p=0.9, min_p=0.1, temp=1.5, seed=3)
    sampled = dec._generate_graph(sp)["nodes"]
    assert ops(sampled) == ops(dec.nodes) + [g.OP_SAMPLE]
    last = sampled[-1]
    assert list(last.op_params) == [g.SAMPLE_STEP_INPUTS, 12, g.f32_bits(1.5), g.f32_bits(0.9), g.f32_bits(0.1), 0, 0, 0]
    assert last.flags == g.FLAG_OUTPUT and last.type == g.TYPE_I32 and last.ne[0] == 2 + hd
    assert last.data == greedy[-1].data == dec.inp.data_ptr()
    for s in range(4):  # ARGMAX's sources, then the draws
        a, b = last.src[s].contents, greedy[-1].src[s].contents
        assert (a.type, a.ne[0], a.ne[1], a.data) == (b.type, b.ne[0], b.ne[1], b.data), s
    draws = last.src[4].contents
    assert (draws.type, draws.ne[0], draws.ne[1]) == (g.TYPE_F32, S.N_CTX + 1, 1) and not last.src[5]
    # cached per sampler parameters, whatever the seed; the greedy graph is untouched
    assert dec._generate_graph(Sampler(top_k=12, top_p=0.9, min_p=0.1, temp=1.5, seed=99))["nodes"] is sampled
    assert dec._generate_graph(Sampler(top_k=13, top_p=0.9, min_p=0.1, temp=1.5))["nodes"] is not sampled
    assert dec._generate_graph()["nodes"] is greedy
