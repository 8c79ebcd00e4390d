"""CPU checks of the MoE entry points' host side: every argument error of mi355x_moe_route,
mi355x_mul_mat_id and mi355x_moe_combine (on fake pointers: all are returned before any device access) and
what mi355x_backend_supports_op takes of the three nodes. No device, no launch."""
import ctypes

GI, X, REC, PROBS, W, Y, EX = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
E, NE, NU, T = 256, 8, 2, 3


def _route(L, **kw):
    a = dict(gi=GI, n_embd=E, n_expert=NE, x=X, x_stride=E, T=T, n_used=NU, rec=REC, rec_stride=2 * NU, probs=None)
    a.update(kw)
    return L.mi355x_moe_route(a["gi"], a["n_embd"], a["n_expert"], a["x"], a["x_stride"], a["T"], a["n_used"], a["rec"],
                              a["rec_stride"], a["probs"], None)


def test_moe_route_argument_errors_without_device():
    import ggml_mi355x as g
    L = g.lib()
    bad = (dict(gi=None), dict(x=None), dict(rec=None), dict(gi=GI + 2), dict(x=X + 1), dict(rec=REC + 2), dict(probs=PROBS + 2),
           dict(n_embd=0), dict(n_expert=0), dict(n_used=0), dict(n_used=NE + 1), dict(T=-1), dict(x_stride=E - 1),
           dict(rec_stride=2 * NU - 1), dict(n_expert=65, n_used=66))
    for b in bad:
        assert _route(L, **b) == g.E_INVAL, b
    for b in (dict(n_expert=1, n_used=1), dict(n_expert=65), dict(n_expert=16, n_used=9, rec_stride=18), dict(n_embd=264, x_stride=264),
              dict(n_embd=8, x_stride=8)):
        assert _route(L, **b) == g.E_UNSUPPORTED, b
    assert _route(L, n_embd=264, x_stride=264, T=-1) == g.E_INVAL  # the ranges first
    assert _route(L, T=0) == g.E_OK and _route(L, T=0, x=None) == g.E_INVAL
    assert _route(L, T=1, x_stride=0) in (g.E_OK, g.E_NODEVICE)  # one row: the stride is not read
    if not g.device_available():
        for ok in (dict(), dict(probs=PROBS), dict(n_expert=64, n_used=8, rec_stride=20), dict(n_expert=2, n_used=1),
                   dict(x_stride=E + 4)):
            assert _route(L, **ok) == g.E_NODEVICE, ok


def _mmid(L, **kw):
    import ggml_mi355x as g
    a = dict(type=g.TYPE_Q4_K, w=W, ne00=512, ne01=20, nb01=288, nb02=20 * 288, n_expert=4, x=X, ne11=1, xs=512, ids=REC,
             ids_stride=2 * NU, n_used=NU, T=T, y=Y, ws=None, ws_size=0)
    a.update(kw)
    return L.mi355x_mul_mat_id(a["type"], a["w"], a["ne00"], a["ne01"], a["nb01"], a["nb02"], a["n_expert"], a["x"], a["ne11"],
                               a["xs"], a["ids"], a["ids_stride"], a["n_used"], a["T"], a["y"], a["ws"], a["ws_size"], None)


def test_mul_mat_id_argument_errors_without_device():
    import ggml_mi355x as g
    L = g.lib()
    q6 = dict(type=g.TYPE_Q6_K, nb01=420, nb02=20 * 420)
    bad = (dict(w=None), dict(x=None), dict(ids=None), dict(y=None), dict(x=X + 4), dict(ids=REC + 2), dict(y=Y + 1),
           dict(ne00=0), dict(ne00=500), dict(ne01=-1), dict(n_expert=0), dict(n_used=0), dict(T=-1),
           dict(ne11=3), dict(ne11=0), dict(xs=510), dict(xs=508), dict(ids_stride=1),
           dict(nb01=287), dict(nb01=272), dict(nb02=19 * 288),
           dict(w=W + 8), dict(nb01=296, nb02=20 * 296), dict(nb02=20 * 288 + 8),  # Q4_K: 16-byte loads
           dict(type=g.TYPE_Q5_K, nb01=352, nb02=20 * 352, w=W + 4),
           dict(w=W + 1, **q6), dict(type=g.TYPE_Q6_K, nb01=421, nb02=20 * 421),  # Q6_K: even addresses and strides
           dict(type=g.TYPE_Q6_K, nb01=420, nb02=20 * 420 + 1))
    for b in bad:
        assert _mmid(L, **b) == g.E_INVAL, b
    for b in (dict(type=g.TYPE_Q8_K), dict(type=g.TYPE_F32), dict(n_expert=65), dict(n_used=9, ids_stride=18, ne11=9),
              dict(ne00=16384 + 256, nb01=65 * 144, nb02=20 * 65 * 144, xs=16640), dict(T=32768)):
        assert _mmid(L, **b) == g.E_UNSUPPORTED, b
    assert _mmid(L, type=g.TYPE_Q8_K, T=-1) == g.E_INVAL  # the ranges first
    assert _mmid(L, T=0) == g.E_OK and _mmid(L, ne01=0) == g.E_OK and _mmid(L, T=0, y=None) == g.E_INVAL
    assert L.mi355x_mul_mat_id_workspace_size(g.TYPE_Q4_K, 4096, 2, 1) == 0  # quantized in the launch's prologue
    if not g.device_available():
        oks = (dict(), dict(ne11=NU), dict(xs=516), dict(**q6), dict(w=W + 2, **q6),
               dict(type=g.TYPE_Q6_K, nb01=420, nb02=20 * 420 + 2, w=W + 6),  # a Q6_K tensor at any even address and stride
               dict(type=g.TYPE_Q5_K, nb01=352, nb02=20 * 352), dict(ws=W, ws_size=64), dict(n_expert=1, nb02=0),
               dict(ne00=16384, nb01=64 * 144, nb02=20 * 64 * 144, xs=16384), dict(T=32767))
        for ok in oks:
            assert _mmid(L, **ok) == g.E_NODEVICE, ok


def _combine(L, **kw):
    a = dict(ex=EX, n=E, n_used=NU, T=T, rec=REC, rec_stride=2 * NU, y=Y)
    a.update(kw)
    return L.mi355x_moe_combine(a["ex"], a["n"], a["n_used"], a["T"], a["rec"], a["rec_stride"], a["y"], None)


def test_moe_combine_argument_errors_without_device():
    import ggml_mi355x as g
    L = g.lib()
    for b in (dict(ex=None), dict(rec=None), dict(y=None), dict(ex=EX + 2), dict(rec=REC + 1), dict(y=Y + 2), dict(n=-1),
              dict(n_used=0), dict(T=-1), dict(rec_stride=3)):
        assert _combine(L, **b) == g.E_INVAL, b
    for b in (dict(n_used=9, rec_stride=18), dict(T=65536), dict(n=2 ** 31)):
        assert _combine(L, **b) == g.E_UNSUPPORTED, b
    assert _combine(L, n=0) == g.E_OK and _combine(L, T=0) == g.E_OK and _combine(L, T=0, y=None) == g.E_INVAL
    if not g.device_available():
        for ok in (dict(), dict(n=7), dict(n_used=1), dict(n_used=8, rec_stride=16), dict(rec_stride=10), dict(T=65535)):
            assert _combine(L, **ok) == g.E_NODEVICE, ok


# ---------------------------------------------------------------- supports_op on hand-made nodes
def _set3(t, ne1, ne2):
    t.ne[1], t.ne[2], t.nb[2], t.nb[3] = ne1, ne2, t.nb[1] * ne1, t.nb[1] * ne1 * ne2
    return t


def _nodes(typ=None, K=512, N=20, ne=4, nu=NU, T=T, ne11=1, w_data=W, nb1=None, nb2=None, rec_stride=None):
    import ggml_mi355x as g
    typ = g.TYPE_Q4_K if typ is None else typ
    gi = g.make_tensor(g.TYPE_F32, E, NE, GI)
    x = g.make_tensor(g.TYPE_F32, E, T, X)
    route = g.make_tensor(g.TYPE_I32, 2 * nu, T, REC, op=g.OP_MOE_ROUTE, srcs=[gi, x], op_params=[nu],
                          row_stride=rec_stride)
    w = g.make_tensor(typ, K, N, w_data, row_stride=nb1)
    w.ne[2] = ne
    w.nb[2] = nb2 if nb2 is not None else w.nb[1] * N
    w.nb[3] = w.nb[2] * ne
    act = _set3(g.make_tensor(g.TYPE_F32, K, ne11 * T, X), ne11, T)
    mm = _set3(g.make_tensor(g.TYPE_F32, N, nu * T, Y, op=g.OP_MUL_MAT_ID, srcs=[w, act, route]), nu, T)
    cb = g.make_tensor(g.TYPE_F32, N, T, EX, op=g.OP_MOE_COMBINE, srcs=[mm, route])
    return dict(gi=gi, x=x, route=route, w=w, act=act, mm=mm, cb=cb)  # (keeps every descriptor alive)


def test_supports_op():
    import ggml_mi355x as g
    assert (g.OP_MOE_ROUTE, g.OP_MUL_MAT_ID, g.OP_MOE_COMBINE) == (19, 20, 21)
    for kw in (dict(), dict(ne11=NU), dict(typ=g.TYPE_Q5_K), dict(typ=g.TYPE_Q6_K), dict(typ=g.TYPE_Q6_K, w_data=W + 2),
               dict(typ=g.TYPE_Q6_K, nb2=20 * 420 + 2), dict(rec_stride=32), dict(T=1), dict(nu=1), dict(K=16384)):
        n = _nodes(**kw)
        assert g.supports_op(n["route"]) and g.supports_op(n["mm"]) and g.supports_op(n["cb"]), kw
    for kw in (dict(typ=g.TYPE_Q6_K, w_data=W + 1), dict(typ=g.TYPE_Q6_K, nb2=20 * 420 + 1), dict(typ=g.TYPE_Q6_K, nb1=421),
               dict(w_data=W + 8), dict(nb1=296), dict(nb2=20 * 288 + 8), dict(ne=65), dict(K=16384 + 256), dict(ne=0)):
        n = _nodes(**kw)
        assert not g.supports_op(n["mm"]), kw
    n = _nodes()
    n["route"].op_params[0] = 3  # n_used does not match the record
    assert not g.supports_op(n["route"])
    n = _nodes()
    n["route"].op_params[0] = NU
    n["route"].type = g.TYPE_F32
    assert not g.supports_op(n["route"]) and not g.supports_op(n["mm"]) and not g.supports_op(n["cb"])
    n = _nodes(ne11=NU)
    n["act"].ne[1] = 3  # neither 1 nor n_used
    assert not g.supports_op(n["mm"])
    n = _nodes()
    n["mm"].src[2] = ctypes.pointer(n["x"])  # not a MOE_ROUTE node
    assert not g.supports_op(n["mm"])
    n = _nodes()
    n["mm"].ne[0] = 24
    assert not g.supports_op(n["mm"])
    n = _nodes()
    n["cb"].ne[1] = T + 1
    assert not g.supports_op(n["cb"])
    n = _nodes()
    n["gi"].ne[1] = 1  # one expert
    assert not g.supports_op(n["route"])
    n = _nodes()
    n["gi"].ne[0] = n["x"].ne[0] = 264  # n_embd % 16
    assert not g.supports_op(n["route"])
    # a 3-D src0 still is no MUL_MAT
    n = _nodes()
    n["mm"].op = g.OP_MUL_MAT
    assert not g.supports_op(n["mm"])
