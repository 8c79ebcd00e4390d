"""CPU checks of the penalties' host side: the order of mi355x_penalize_rows' argument errors (on
fake pointers: all are returned before any device access), what mi355x_backend_supports_op takes
of a PENALIZE node, Sampler's new arguments and edits(), and the node lists of generate's graphs on
a describe-only decoder. No device, no launch."""
import ctypes
import math

import pytest

X, HIST, END, BT, BV = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
V = 32000
INF, NAN = float("inf"), float("nan")


def test_argument_errors_in_order_without_device():
    import ggml_mi355x as g
    L = g.lib()

    def call(**kw):
        a = dict(x=X, n=V, rows=3, stride=V, p="ok", last_n=64, repeat=1.1, freq=0.0, present=0.0, hist=HIST,
                 hist_stride=512, n_hist=512, end=END, bt=BT, bv=BV, n_bias=2)
        a.update(kw)
        pen = g.PenaltiesDesc(a["last_n"], a["repeat"], a["freq"], a["present"])
        return L.mi355x_penalize_rows(a["x"], a["n"], a["rows"], a["stride"], ctypes.byref(pen) if a["p"] == "ok" else None,
                                      a["hist"], a["hist_stride"], a["n_hist"], a["end"], a["bt"], a["bv"], a["n_bias"], None)

    bad_args = (
        dict(x=None), dict(p=None),                                                              # null x or p
        dict(n=0), dict(n=(1 << 24) + 1, stride=(1 << 24) + 1), dict(rows=0), dict(rows=65536),  # the ranges
        dict(stride=V - 1), dict(x=X + 2),
        dict(last_n=-1), dict(last_n=1025), dict(repeat=0.0), dict(repeat=-1.0), dict(repeat=INF),  # the rule's ranges
        dict(repeat=NAN), dict(freq=INF), dict(freq=NAN), dict(present=-INF), dict(present=NAN),
        dict(n_bias=-1), dict(n_bias=257),
        dict(hist=None), dict(end=None), dict(n_hist=0), dict(n_hist=1 << 31, hist_stride=1 << 31),  # the window's sources
        dict(hist_stride=511),
        dict(bt=None), dict(bv=None),                                                            # the lists
    )
    for bad in bad_args:
        assert call(**bad) == g.E_INVAL, bad
    # optional arguments: no window, no list
    assert call(last_n=0, n_bias=0, hist=None, end=None, bt=None, bv=None, n_hist=0, hist_stride=0) == g.E_OK  # no launch
    assert call(last_n=0, n_bias=0) == g.E_OK
    # ... but the ranges are still checked
    assert call(last_n=0, n_bias=0, x=None) == g.E_INVAL
    assert call(last_n=0, n_bias=0, repeat=0.0) == g.E_INVAL
    if not g.device_available():
        assert call() == g.E_NODEVICE
        assert call(last_n=0, hist=None, end=None, n_hist=0, hist_stride=0) == g.E_NODEVICE  # bias alone
        assert call(n_bias=0, bt=None, bv=None) == g.E_NODEVICE                              # the window alone
        assert call(x=X + 4, n=7, stride=12, last_n=1024, n_bias=256) == g.E_NODEVICE        # 4-B aligned x, a padded row
        assert call(n=1 << 24, stride=1 << 24, rows=65535, n_hist=(1 << 31) - 1, hist_stride=1 << 31) == g.E_NODEVICE


# ---------------------------------------------------------------- supports_op on hand-made nodes
def _node(T=1, n=V, x="ok", end="ok", hist="ok", bt="ok", bv="ok", last_n=64, repeat=1.1, freq=0.0, present=0.0, n_bias=3,
          data="x", **dst):
    import ggml_mi355x as g
    x = g.make_tensor(g.TYPE_F32, n, T, 0x100000) if x == "ok" else x
    end = g.make_tensor(g.TYPE_I32, T, 1, 0x8000) if end == "ok" else end
    hist = g.make_tensor(g.TYPE_I32, 513, T, 0x200000) if hist == "ok" else hist
    bt = g.make_tensor(g.TYPE_I32, n_bias, 1, 0x9000) if bt == "ok" else bt
    bv = g.make_tensor(g.TYPE_F32, n_bias, 1, 0xa000) if bv == "ok" else bv
    t = g.make_tensor(dst.get("type", g.TYPE_F32), dst.get("ne0", n), dst.get("ne1", T), 0x100000 if data == "x" else data,
                      row_stride=dst.get("row_stride"), op=g.OP_PENALIZE, srcs=[x, end, hist, bt, bv],
                      op_params=g.penalize_params(last_n, repeat, freq, present, n_bias), flags=g.FLAG_OUTPUT)
    return t


@pytest.mark.parametrize("T", [1, 3])
def test_supports_op_accepts(T):
    import ggml_mi355x as g
    assert g.OP_PENALIZE == 17 and g.PENALTY_MAX_LAST_N == 1024 and g.LOGIT_BIAS_MAX == 256
    assert g.supports_op(_node(T))
    for n in (1, 7, 2304, 128256, 1 << 24):
        assert g.supports_op(_node(T, n=n)), n
    assert g.supports_op(_node(T, last_n=1024, n_bias=256))
    assert g.supports_op(_node(T, last_n=0, end=None, hist=None))            # bias alone: no window sources
    assert g.supports_op(_node(T, n_bias=0, bt=None, bv=None))               # the window alone
    assert g.supports_op(_node(T, last_n=0, n_bias=0, end=None, hist=None, bt=None, bv=None))
    assert g.supports_op(_node(T, freq=-2.0, present=1e4, repeat=1e-3))
    assert g.supports_op(_node(T, hist=g.make_tensor(g.TYPE_I32, 65, T, 0x200000, row_stride=4 * 80)))  # strided history
    assert g.supports_op(_node(65535, n=4))


@pytest.mark.parametrize("T", [1, 3])
def test_supports_op_refuses(T):
    import ggml_mi355x as g
    # in place only: another address, type, shape or stride than src0's
    assert not g.supports_op(_node(T, data=0x100010))
    assert not g.supports_op(_node(T, data=None))
    assert not g.supports_op(_node(T, type=g.TYPE_I32))
    assert not g.supports_op(_node(T, ne0=V - 1))
    assert not g.supports_op(_node(T, ne1=T + 1))
    assert not g.supports_op(_node(3, row_stride=4 * V + 16))
    # the logits
    assert not g.supports_op(_node(T, x=None))
    assert not g.supports_op(_node(T, x=g.make_tensor(g.TYPE_F16, V, T, 0x100000)))
    assert not g.supports_op(_node(T, x=g.make_tensor(g.TYPE_F32, V, T, 0x100002), data=0x100002))
    assert not g.supports_op(_node(T, n=(1 << 24) + 1))
    assert not g.supports_op(_node(65536, n=4))
    strided = g.make_tensor(g.TYPE_F32, V, 3, 0x100000, row_stride=4 * V + 16)
    assert not g.supports_op(_node(3, x=strided, row_stride=4 * V + 16))                       # packed rows only
    # a parameter out of range
    for kw in (dict(last_n=-1), dict(last_n=1025), dict(repeat=0.0), dict(repeat=-1.1), dict(repeat=INF), dict(repeat=NAN),
               dict(freq=INF), dict(freq=NAN), dict(present=-INF), dict(present=NAN), dict(n_bias=257), dict(n_bias=-1)):
        assert not g.supports_op(_node(T, **kw)), kw
    # the window's sources, needed at last_n > 0
    assert not g.supports_op(_node(T, end=None))
    assert not g.supports_op(_node(T, hist=None))
    assert not g.supports_op(_node(T, end=g.make_tensor(g.TYPE_I32, T + 1, 1, 0x8000)))
    assert not g.supports_op(_node(T, end=g.make_tensor(g.TYPE_F32, T, 1, 0x8000)))
    assert not g.supports_op(_node(T, end=g.make_tensor(g.TYPE_I32, T, 1, None)))
    assert not g.supports_op(_node(T, hist=g.make_tensor(g.TYPE_I32, 513, T + 1, 0x200000)))
    assert not g.supports_op(_node(T, hist=g.make_tensor(g.TYPE_F32, 513, T, 0x200000)))
    assert not g.supports_op(_node(T, hist=g.make_tensor(g.TYPE_I32, 513, T, None)))
    assert not g.supports_op(_node(3, hist=g.make_tensor(g.TYPE_I32, 513, 3, 0x200000, row_stride=4 * 512)))
    # the lists, needed at n_bias > 0
    assert not g.supports_op(_node(T, bt=None))
    assert not g.supports_op(_node(T, bv=None))
    assert not g.supports_op(_node(T, bt=g.make_tensor(g.TYPE_I32, 2, 1, 0x9000)))
    assert not g.supports_op(_node(T, bv=g.make_tensor(g.TYPE_F32, 4, 1, 0xa000)))
    assert not g.supports_op(_node(T, bt=g.make_tensor(g.TYPE_F32, 3, 1, 0x9000)))
    assert not g.supports_op(_node(T, bv=g.make_tensor(g.TYPE_I32, 3, 1, 0xa000)))
    assert not g.supports_op(_node(T, bv=g.make_tensor(g.TYPE_F32, 3, 1, None)))


# ---------------------------------------------------------------- Sampler
def test_sampler_defaults_and_edits():
    from ggml_mi355x.llama import Sampler
    S = Sampler()
    assert (S.repeat_last_n, S.repeat_penalty, S.freq_penalty, S.presence_penalty, S.logit_bias) == (64, 1.0, 0.0, 0.0, [])
    assert not S.edits()
    assert not Sampler(repeat_last_n=0, repeat_penalty=1.5, freq_penalty=1.0, presence_penalty=1.0).edits()  # no window
    assert not Sampler(logit_bias={}).edits() and not Sampler(logit_bias=[]).edits()
    assert Sampler(repeat_penalty=1.1).edits() and Sampler(freq_penalty=0.5).edits() and Sampler(presence_penalty=-1).edits()
    assert Sampler(logit_bias={5: -INF}).edits() and Sampler(repeat_last_n=0, logit_bias=[(5, 0.0)]).edits()
    assert Sampler(temp=0, repeat_penalty=1.3).edits()  # greedy with penalties
    # the PENALIZE node's parameters; the window is left out where the penalty is the identity
    import ggml_mi355x as g
    assert Sampler(repeat_penalty=1.5, repeat_last_n=7, logit_bias=[(1, 2.0), (1, 3.0)]).penalize_params() == \
        g.penalize_params(7, 1.5, 0.0, 0.0, 2)
    assert Sampler(logit_bias={3: 1.0}).penalize_params() == g.penalize_params(0, 1.0, 0.0, 0.0, 1)
    S = Sampler(logit_bias={3: 1.0, 9: -INF})
    assert S.logit_bias == [(3, 1.0), (9, -INF)]
    assert Sampler(logit_bias=[(9, 0.1), (3, 1), (9, 2)]).logit_bias == [(9, float.fromhex("0x1.99999ap-4")), (3, 1.0), (9, 2.0)]
    assert Sampler(repeat_penalty=1.1).repeat_penalty == float.fromhex("0x1.19999ap+0")  # the float32 the device takes
    assert Sampler().params() == Sampler(repeat_penalty=1.3, logit_bias={1: 1.0}).params()  # the SAMPLE node's are as before


def test_sampler_argument_checks():
    import ggml_mi355x as g
    from ggml_mi355x.llama import Sampler
    bad = (dict(repeat_last_n=-1), dict(repeat_last_n=1025), dict(repeat_last_n=3.5),
           dict(repeat_penalty=0.0), dict(repeat_penalty=-1.0), dict(repeat_penalty=INF), dict(repeat_penalty=NAN),
           dict(repeat_penalty=1e-50), dict(repeat_penalty=1e39),  # 0 and inf as float32
           dict(freq_penalty=INF), dict(freq_penalty=NAN), dict(freq_penalty=1e39),
           dict(presence_penalty=-INF), dict(presence_penalty=NAN),
           dict(logit_bias={i: 1.0 for i in range(257)}), dict(logit_bias=[(1, NAN)]), dict(logit_bias=[(2 ** 31, 1.0)]),
           dict(logit_bias=[1, 2]), dict(logit_bias=[("a", 1.0)]), dict(logit_bias=5))
    for kw in bad:
        with pytest.raises(g.Mi355xError):
            Sampler(**kw)
    Sampler(repeat_last_n=1024, logit_bias={i: -INF for i in range(256)}, repeat_penalty=1e-30, freq_penalty=-3.0)
    assert math.isinf(Sampler(logit_bias=[(0, 1e39)]).logit_bias[0][1])  # a bias may be +-inf


# ---------------------------------------------------------------- the decoder, describe only
@pytest.fixture(scope="module")
def dec():
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_graph_sig as S
    return LlamaDecoder(None, S.HP, S._weights(), S.N_CTX)


def addr(t):
    return ctypes.addressof(t)


def test_generate_graph_node_lists(dec):
    import ggml_mi355x as g
    from ggml_mi355x.llama import Sampler
    from tests import llama_graph_sig as S
    V_, n_ctx = S.HP["n_vocab"], S.N_CTX
    plain = dec._generate_graph(Sampler())
    # a sampler without edits: the node list and the cache entry of a sampler before penalties existed
    assert [n.op for n in plain["nodes"]] == [n.op for n in dec.nodes] + [g.OP_SAMPLE]
    assert dec._generate_graph(Sampler(repeat_last_n=0, repeat_penalty=2.0)) is plain
    assert dec._generate_graph(Sampler(seed=9, logit_bias={})) is plain
    assert list(dec._gen_sampled) == [tuple(Sampler().params())]
    assert addr(plain["nodes"][-1].src[0].contents) == addr(dec.nodes[-1])
    # an editing sampler: ... logits, PENALIZE, SAMPLE(src0 = PENALIZE)
    E = Sampler(repeat_penalty=1.1, repeat_last_n=16, logit_bias={3: -INF, 5: 1.0})
    ge = dec._generate_graph(E)
    assert ge is not plain and dec._generate_graph(Sampler(repeat_penalty=1.1, repeat_last_n=16, logit_bias={7: 1.0, 8: 2.0})) is ge
    assert dec._generate_graph(Sampler(repeat_penalty=1.1, repeat_last_n=16, logit_bias={7: 1.0})) is not ge  # n_bias
    assert dec._generate_graph(Sampler(repeat_penalty=1.2, repeat_last_n=16, logit_bias={3: -INF, 5: 1.0})) is not ge
    assert [n.op for n in ge["nodes"]] == [n.op for n in dec.nodes] + [g.OP_PENALIZE, g.OP_SAMPLE]
    assert all(addr(a) == addr(b) for a, b in zip(ge["nodes"], dec.nodes))
    pen, sm, logits = ge["nodes"][-2], ge["nodes"][-1], dec.nodes[-1]
    assert addr(sm.src[0].contents) == addr(pen) and addr(pen.src[0].contents) == addr(logits)
    assert (pen.data, pen.type, tuple(pen.ne), tuple(pen.nb)) == (logits.data, logits.type, tuple(logits.ne), tuple(logits.nb))
    assert pen.ne[0] == V_ and pen.ne[1] == 1
    assert list(pen.op_params)[:5] == g.penalize_params(16, 1.1, 0.0, 0.0, 2)
    end, hist, bt, bv = (pen.src[i].contents for i in range(1, 5))
    assert (end.data, end.ne[0]) == (dec.pos.data_ptr(), 1)
    assert (hist.data, hist.ne[0], hist.ne[1]) == (dec.history.data_ptr(), n_ctx, 1)
    assert (bt.data, bt.ne[0], bt.type) == (dec._bias["tok"].data_ptr(), 2, g.TYPE_I32)
    assert (bv.data, bv.ne[0], bv.type) == (dec._bias["val"].data_ptr(), 2, g.TYPE_F32)
    assert dec._bias["tok"].numel() == dec._bias["val"].numel() == 256
    assert g.supports_op(pen) and g.supports_op(sm)
    # bias alone: no window sources
    gb = dec._generate_graph(Sampler(logit_bias={1: 1.0}))
    pen = gb["nodes"][-2]
    assert pen.op == g.OP_PENALIZE and not pen.src[1] and not pen.src[2] and pen.op_params[0] == 0 and g.supports_op(pen)
    # greedy is untouched
    assert [n.op for n in dec._generate_graph(None)["nodes"]] == [n.op for n in dec.nodes] + [g.OP_ARGMAX]


def test_generate_refusals(dec):
    import ggml_mi355x as g
    from ggml_mi355x.llama import Sampler
    E = Sampler(repeat_penalty=1.1)
    for ctx in ([1, 2, 3, 4], [2 ** 31], [1, -2 ** 31 - 1]):  # longer than pos, not int32
        with pytest.raises(g.Mi355xError):
            dec.generate(1, 3, 2, sampler=E, context=ctx)
    dec.split = object()
    try:
        with pytest.raises(g.Mi355xError):
            dec.generate(1, 3, 2, sampler=E, context=[1])
        with pytest.raises(g.Mi355xError):
            dec.generate_batch([1], [3], [3], [[0.0] * 32], 2, 32, sampler=E, contexts=[[1]])
    finally:
        dec.split = None
