"""CPU checks of the context shift's host side: every argument error of mi355x_kv_shift (on fake
pointers: all are returned before any device access), what mi355x_backend_supports_op takes of a
KV_SHIFT node, Sampler.draws' epochs, LlamaDecoder.shift's node list on a describe-only decoder and
generate(keep=)'s argument errors. No device, no launch."""
import ctypes

import numpy as np
import pytest

K, V, TAB, DELTA = 0x100000, 0x200000, 0x300000, 0x400000
N_CTX, NKV, HD = 96, 2, 64


def test_argument_errors_without_device():
    import ggml_mi355x as g
    L = g.lib()

    def call(**kw):
        a = dict(k=K, v=V, tab=TAB, delta=DELTA, n_ctx=N_CTX, nkv=NKV, hd=HD, n_pos=N_CTX, form=g.KV_SHIFT_DELTAS,
                 n_cells=N_CTX, keep=4, discard=30, n_past=N_CTX, desc=True)
        a.update(kw)
        d = g.KvShiftDesc(a["k"], a["v"], a["tab"], a["delta"], a["n_ctx"], a["nkv"], a["hd"], a["n_pos"], a["form"],
                          a["n_cells"], a["keep"], a["discard"], a["n_past"])
        return L.mi355x_kv_shift(ctypes.byref(d) if a["desc"] else None, None)

    D = dict(form=g.KV_SHIFT_DISCARD, delta=None)
    bad_args = (
        dict(desc=False), dict(form=2), dict(form=-1),                       # no descriptor, an unknown form
        dict(k=None), dict(tab=None), dict(delta=None), dict(v=None, **D),   # a null required pointer
        dict(k=K + 8), dict(tab=TAB + 4), dict(delta=DELTA + 2),             # misaligned
        dict(n_ctx=0), dict(nkv=0), dict(n_pos=0), dict(hd=0),
        dict(n_cells=-1), dict(n_cells=N_CTX + 1),                           # n_cells outside [0, n_ctx]
        dict(keep=-1, **D), dict(discard=0, **D), dict(discard=-3, **D),     # keep < 0, discard < 1
        dict(keep=67, **D), dict(keep=4, discard=93, **D),                   # keep + discard > n_past
        dict(n_past=N_CTX + 1, **D),                                         # n_past > n_ctx
        dict(discard=40, n_pos=40, **D), dict(discard=40, n_pos=12, **D),    # discard >= n_pos
    )
    for bad in bad_args:
        assert call(**bad) == g.E_INVAL, bad
    for hd in (32, 96, 256):  # as the attention
        assert call(hd=hd) == g.E_UNSUPPORTED and call(hd=hd, **D) == g.E_UNSUPPORTED
    assert call(hd=32, n_cells=-1) == g.E_INVAL  # the ranges first
    # nothing to do: OK with no launch, with and without a device
    assert call(n_cells=0) == g.E_OK
    assert call(n_cells=0, v=None) == g.E_OK           # V is optional in the DELTAS form
    assert call(keep=66, discard=30, **D) == g.E_OK    # keep + discard == n_past: no cell moves
    assert call(keep=0, discard=50, n_past=50, **D) == g.E_OK
    assert call(n_cells=0, k=None) == g.E_INVAL        # ... but the arguments are still checked
    if not g.device_available():
        assert call() == g.E_NODEVICE
        assert call(v=None, n_cells=1, hd=128) == g.E_NODEVICE
        assert call(**D) == g.E_NODEVICE
        assert call(keep=0, discard=1, n_ctx=1000, n_past=1000, n_pos=2, **D) == g.E_NODEVICE
        assert call(keep=17, discard=N_CTX - 18, **D) == g.E_NODEVICE  # one moved cell


# ---------------------------------------------------------------- supports_op on hand-made nodes
def _node(form, params, k="ok", v="ok", tab="ok", delta="ok", data=K, n_ctx=N_CTX, n_pos=N_CTX, **dst):
    import ggml_mi355x as g
    kvw = NKV * HD
    k = g.make_tensor(g.TYPE_F16, kvw, n_ctx, K) if k == "ok" else k
    v = g.make_tensor(g.TYPE_F16, n_ctx, kvw, V) if v == "ok" else v
    tab = g.make_tensor(g.TYPE_F32, HD, n_pos, TAB) if tab == "ok" else tab
    delta = g.make_tensor(g.TYPE_I32, params[-1], 1, DELTA) if delta == "ok" else delta
    srcs = [k, v, tab] + ([delta] if form == 0 else [])
    return g.make_tensor(dst.get("type", g.TYPE_F16), dst.get("ne0", kvw), dst.get("ne1", n_ctx), data, op=g.OP_KV_SHIFT,
                         srcs=srcs, op_params=[NKV, HD, form] + list(params))


def test_supports_op():
    import ggml_mi355x as g
    assert g.OP_KV_SHIFT == 18 and (g.KV_SHIFT_DELTAS, g.KV_SHIFT_DISCARD) == (0, 1)
    assert g.kv_shift_params(2, 64, n_cells=7) == [2, 64, 0, 7]
    assert g.kv_shift_params(2, 64, keep=4, discard=30, n_past=64) == [2, 64, 1, 4, 30, 64]
    ok = [_node(0, [N_CTX]), _node(0, [N_CTX], v=None), _node(0, [0]), _node(0, [5]),
          _node(1, [4, 30, N_CTX]), _node(1, [0, 1, 1000], n_ctx=1000, n_pos=1000), _node(1, [66, 30, N_CTX]),
          _node(1, [0, 1, 7], n_pos=2)]
    for t in ok:
        assert g.supports_op(t), list(t.op_params)
    f32k = g.make_tensor(g.TYPE_F32, NKV * HD, N_CTX, K)
    short_delta = g.make_tensor(g.TYPE_I32, 5, 1, DELTA)
    bad = [_node(0, [N_CTX], k=None), _node(0, [N_CTX], tab=None), _node(0, [N_CTX], delta=None),
           _node(0, [N_CTX], k=f32k), _node(0, [N_CTX], data=K + 256), _node(0, [N_CTX], type=g.TYPE_F32),
           _node(0, [N_CTX], ne1=N_CTX - 1), _node(0, [N_CTX + 1]), _node(0, [-1]), _node(0, [N_CTX], delta=short_delta),
           _node(0, [N_CTX], delta=g.make_tensor(g.TYPE_F32, N_CTX, 1, DELTA)),
           _node(0, [N_CTX], tab=g.make_tensor(g.TYPE_F32, 128, N_CTX, TAB)),
           _node(0, [N_CTX], v=g.make_tensor(g.TYPE_F16, N_CTX, HD, V)),
           _node(1, [4, 30, N_CTX], v=None), _node(1, [-1, 30, N_CTX]), _node(1, [4, 0, N_CTX]), _node(1, [67, 30, N_CTX]),
           _node(1, [4, 30, N_CTX + 1]), _node(1, [4, 30, N_CTX], n_pos=30), _node(2, [N_CTX])]
    for t in bad:
        assert not g.supports_op(t), list(t.op_params)
    t = _node(0, [N_CTX])
    t.op_params[1] = 96  # head_dim
    assert not g.supports_op(t)


# ---------------------------------------------------------------- the sampler's epochs
def test_draws_epoch_zero_is_as_before():
    from ggml_mi355x.llama import Sampler
    from tests import sample_ref as R
    S = Sampler(seed=3)
    for n in (1, 65):
        assert (S.draws(n) == R.draws(3, n)).all() and (S.draws(n, epoch=0) == R.draws(3, n)).all()
        assert (S.draws(n, 2) == R.draws([3, 2], n)).all() and (S.draws(n, 2, 0) == R.draws([3, 2], n)).all()
        assert (S.draws(n, epoch=1) == R.draws([3, 0, 1], n)).all()
        assert (S.draws(n, epoch=4) == R.draws([3, 0, 4], n)).all()
        assert (S.draws(n, 2, epoch=1) == R.draws([3, 2, 1], n)).all()
    assert not (S.draws(65, epoch=1) == S.draws(65)).all() and not (S.draws(65, epoch=1) == S.draws(65, epoch=2)).all()
    assert S.draws(5, epoch=1).dtype == np.float32


# ---------------------------------------------------------------- the decoder, describe only
@pytest.fixture(scope="module")
def dec():
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_graph_sig as S
    return LlamaDecoder(None, S.HP, S._weights(), S.N_CTX)


def test_shift_node_list(dec):
    import ggml_mi355x as g
    from tests import llama_graph_sig as S
    hd, nkv, n_ctx = S.HP["head_dim"], S.HP["n_head_kv"], S.N_CTX
    dec.shift(n_ctx, 4, 30)
    assert list(dec._shifts) == [(n_ctx, 4, 30)]
    sh = dec._shifts[(n_ctx, 4, 30)]
    assert len(sh["nodes"]) == S.HP["n_layer"]
    for i, n in enumerate(sh["nodes"]):
        assert n.op == g.OP_KV_SHIFT and list(n.op_params)[:6] == [nkv, hd, g.KV_SHIFT_DISCARD, 4, 30, n_ctx]
        kc, vc, tab = (n.src[j].contents for j in range(3))
        assert not n.src[3]
        assert n.data == kc.data == dec.k_cache[i].data_ptr() and vc.data == dec.v_cache[i].data_ptr()
        assert (n.type, tuple(n.ne), tuple(n.nb)) == (kc.type, tuple(kc.ne), tuple(kc.nb)) and kc.type == g.TYPE_F16
        assert (kc.ne[0], kc.ne[1], vc.ne[0], vc.ne[1]) == (nkv * hd, n_ctx, n_ctx, nkv * hd)
        assert (tab.data, tab.ne[0], tab.ne[1]) == (dec.table.data_ptr(), hd, n_ctx)
        assert g.supports_op(n)
    dec.shift(n_ctx, 4, 30)
    assert dec._shifts[(n_ctx, 4, 30)] is sh and len(dec._shifts) == 1  # cached by (n_past, keep, discard)
    dec.shift(n_ctx - 1, 4, 30)
    assert len(dec._shifts) == 2
    dec.shift(n_ctx, 34, 30)  # nothing moves: no node list
    assert len(dec._shifts) == 2
    for n_past, keep, discard in ((n_ctx + 1, 4, 30), (n_ctx, -1, 30), (n_ctx, 4, 0), (n_ctx, 40, 30)):
        with pytest.raises(g.Mi355xError):
            dec.shift(n_past, keep, discard)
    dec.split = object()
    try:
        with pytest.raises(g.Mi355xError):
            dec.shift(n_ctx, 4, 30)
    finally:
        dec.split = None


def test_generate_keep_argument_errors(dec):
    import ggml_mi355x as g
    from tests import llama_graph_sig as S
    n_ctx = S.N_CTX
    # without keep: the refusal as before
    for n, pos in ((4, n_ctx - 3), (1, n_ctx), (n_ctx + 1, 0), (1, -1)):
        with pytest.raises(g.Mi355xError, match="outside the KV cache"):
            dec.generate(7, pos, n)
    with pytest.raises(g.Mi355xError):
        dec.generate(7, 0, 4, discard=8)  # discard needs keep
    for kw in (dict(keep=-1), dict(keep=n_ctx - 1), dict(keep=n_ctx), dict(keep=2.5), dict(keep=4, discard=0),
               dict(keep=4, discard=n_ctx - 3), dict(keep=4, discard=-1), dict(keep=4, discard=1.5)):
        with pytest.raises(g.Mi355xError):
            dec.generate(7, 0, 200, **kw)
    for pos in (-1, n_ctx):
        with pytest.raises(g.Mi355xError):
            dec.generate(7, pos, 200, keep=4)
    with pytest.raises(g.Mi355xError):
        dec.generate(7, 0, -1, keep=4)
    assert dec.generate(7, 0, 0, keep=4) == [] and dec.generate(7, 0, 0) == []
    dec.split = object()
    try:
        with pytest.raises(g.Mi355xError):
            dec.generate(7, 0, 200, keep=4)
    finally:
        dec.split = None
