"""mi355x_kv_shift on the device against tests/kv_shift_ref.py, by bits: the DELTAS form (ggml's
K-shift) and the DISCARD form (a cache whose cell is its position), through the C entry and as a
KV_SHIFT node through mi355x_backend_graph_compute, captured and not. Caches are random finite f16,
one rope table, n_head_kv 2, head_dim 64 and 128.
The DISCARD kernel's chunk is 256 cells (kShiftChunk, csrc/kq_kv_shift.hip): a workgroup loads 256
destination cells' sources before it stores them. N_DISCARD = 1000 cells makes every workgroup
walk three whole chunks and a remainder of 232."""
import numpy as np
import pytest

from tests import kv_shift_ref as K

pytestmark = pytest.mark.gpu

NKV = 2
N_DELTAS, N_DISCARD, CHUNK = 96, 1000, 256
_tables = {}


def table(dev, hd, n_pos):
    """(the device table, its host copy [n_pos, hd / 2, 2]): built once per shape."""
    import torch
    import ggml_mi355x as g
    if (hd, n_pos) not in _tables:
        t = g.rope_table(n_pos, hd, 10000.0, 1.0, device=dev)
        torch.cuda.synchronize()
        _tables[(hd, n_pos)] = (t, t.cpu().numpy().reshape(n_pos, hd // 2, 2).copy())
    return _tables[(hd, n_pos)]


def caches(dev, seed, n_ctx, hd):
    import torch
    rng = np.random.default_rng(seed)
    k, v = K.random_cache(rng, (n_ctx, NKV * hd)), K.random_cache(rng, (NKV * hd, n_ctx))
    kd, vd = torch.from_numpy(k.view(np.int16)).to(dev), torch.from_numpy(v.view(np.int16)).to(dev)
    return k, v, kd, vd


def host(x):
    return x.cpu().numpy().view(np.uint16)


def mixed_deltas(n_pos):
    """Zeros, both signs, the largest in-table value on both sides."""
    d = np.zeros(N_DELTAS, np.int32)
    d[1::3] = np.arange(1, 1 + len(d[1::3]))
    d[2::3] = -np.arange(3, 3 + len(d[2::3]))
    d[7], d[8], d[10], d[11] = n_pos - 1, -(n_pos - 1), 1, -1
    d[90:] = 0
    return d


@pytest.mark.parametrize("hd", [64, 128])
def test_deltas(dev, hd):
    import torch
    import ggml_mi355x as g
    n_pos = N_DELTAS
    tab, tab_h = table(dev, hd, n_pos)
    k, v, kd, vd = caches(dev, 10 + hd, N_DELTAS, hd)
    delta = mixed_deltas(n_pos)
    assert (delta == 0).sum() > 30 and (delta > 0).any() and (delta < 0).any() and abs(delta).max() == n_pos - 1
    dd = torch.from_numpy(delta).to(dev)
    g.kv_shift(kd, tab, NKV, hd, v_cache=vd, delta=dd)
    torch.cuda.synchronize()
    want = K.shift_deltas(k, delta, tab_h, hd)
    got = host(kd)
    assert (got == want).all(), np.argwhere(got != want)[:4]
    assert (got[delta == 0] == k[delta == 0]).all() and not (got[delta != 0] == k[delta != 0]).all(axis=1).any()
    assert (host(vd) == v).all()
    # one out-of-table entry (and INT32_MIN): NaN bits in those cells only; fewer cells than deltas
    delta2 = delta.copy()
    delta2[5], delta2[6], delta2[9] = n_pos, -n_pos, -2 ** 31
    dd.copy_(torch.from_numpy(delta2))
    kd.copy_(torch.from_numpy(k.view(np.int16)))
    torch.cuda.synchronize()
    g.kv_shift(kd, tab, NKV, hd, delta=dd, n_cells=50)  # no V cache at all
    torch.cuda.synchronize()
    delta2[50:] = 0
    want = K.shift_deltas(k, delta2, tab_h, hd)
    got = host(kd)
    assert (got == want).all(), np.argwhere(got != want)[:4]
    nan_cells = np.isnan(got.view(np.float16)).any(axis=1)
    assert np.flatnonzero(nan_cells).tolist() == [5, 6, 9] and (got[[5, 6, 9]] == K.NAN_BITS).all()
    assert (got[50:] == k[50:]).all()


_discard = {}


def discard_inputs(dev, hd):
    if hd not in _discard:
        _discard[hd] = caches(dev, 20 + hd, N_DISCARD, hd)
    return _discard[hd]


DISCARD_CASES = [(0, 1, N_DISCARD), (5, 3, N_DISCARD - 7), (0, N_DISCARD // 2, N_DISCARD), (17, N_DISCARD - 18, N_DISCARD),
                 (40, N_DISCARD - 40, N_DISCARD), (0, CHUNK, N_DISCARD)]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("keep,discard,n_past", DISCARD_CASES,
                         ids=["overlap-in-every-chunk", "odd", "disjoint", "one-cell", "nothing-moves", "one-chunk-apart"])
def test_discard(dev, hd, keep, discard, n_past):
    import torch
    import ggml_mi355x as g
    assert N_DISCARD >= 3 * CHUNK + 1 and N_DISCARD % CHUNK
    tab, tab_h = table(dev, hd, N_DISCARD)
    k, v, kd, vd = discard_inputs(dev, hd)
    kd.copy_(torch.from_numpy(k.view(np.int16)))
    vd.copy_(torch.from_numpy(v.view(np.int16)))
    torch.cuda.synchronize()
    g.kv_shift(kd, tab, NKV, hd, v_cache=vd, keep=keep, discard=discard, n_past=n_past)
    torch.cuda.synchronize()
    wk, wv = K.shift_discard(k, v, tab_h, hd, keep, discard, n_past)
    gk, gv = host(kd), host(vd)
    # the whole caches: the untouched cells too
    assert (gk == wk).all(), np.argwhere(gk != wk)[:4]
    assert (gv == wv).all(), np.argwhere(gv != wv)[:4]
    moved = n_past - discard - keep
    assert ((gk != k).any(axis=1).sum() > 0) == (moved > 0)


@pytest.mark.parametrize("hd", [64, 128])
def test_node_captured_and_not(dev, hd):
    """The KV_SHIFT node through graph_compute: eager, then captured and replayed: every replay
    shifts again, so two replays equal the reference applied twice."""
    import torch
    import ggml_mi355x as g
    n_ctx, kvw = N_DISCARD, NKV * hd
    tab, tab_h = table(dev, hd, n_ctx)
    k, v, kd, vd = discard_inputs(dev, hd)
    keep, discard, n_past = 5, 3, n_ctx - 7
    kt, vt = g.make_tensor(g.TYPE_F16, kvw, n_ctx, kd.data_ptr()), g.make_tensor(g.TYPE_F16, n_ctx, kvw, vd.data_ptr())
    tt = g.make_tensor(g.TYPE_F32, hd, n_ctx, tab.data_ptr())
    node = g.make_tensor(g.TYPE_F16, kvw, n_ctx, kd.data_ptr(), op=g.OP_KV_SHIFT, srcs=[kt, vt, tt],
                         op_params=g.kv_shift_params(NKV, hd, keep=keep, discard=discard, n_past=n_past))
    delta = np.zeros(n_ctx, np.int32)
    delta[3:n_ctx - 2] = -4
    delta[100:140] = 9
    dd = torch.from_numpy(delta).to(dev)
    dnode = g.make_tensor(g.TYPE_F16, kvw, n_ctx, kd.data_ptr(), op=g.OP_KV_SHIFT,
                          srcs=[kt, None, tt, g.make_tensor(g.TYPE_I32, n_ctx, 1, dd.data_ptr())],
                          op_params=g.kv_shift_params(NKV, hd, n_cells=n_ctx))
    assert g.supports_op(node) and g.supports_op(dnode)
    once = K.shift_discard(k, v, tab_h, hd, keep, discard, n_past)
    twice = K.shift_discard(once[0], once[1], tab_h, hd, keep, discard, n_past)
    d_once = K.shift_deltas(k, delta, tab_h, hd)
    d_twice = K.shift_deltas(d_once, delta, tab_h, hd)
    b = g.Backend()
    try:
        for nd, use_graph, times, (wk, wv) in ((node, False, 1, once), (node, True, 1, once), (node, True, 2, twice),
                                               (dnode, False, 1, (d_once, v)), (dnode, True, 2, (d_twice, v))):
            kd.copy_(torch.from_numpy(k.view(np.int16)))
            vd.copy_(torch.from_numpy(v.view(np.int16)))
            torch.cuda.synchronize()
            for _ in range(times):
                assert b.graph_compute([nd], use_graph=use_graph) == 0
            b.synchronize()
            gk, gv = host(kd), host(vd)
            assert (gk == wk).all() and (gv == wv).all(), (use_graph, times, np.argwhere(gk != wk)[:4])
        # the deltas are read at run time: the captured graph with other deltas
        delta[:] = 0
        delta[500] = -1
        dd.copy_(torch.from_numpy(delta))
        kd.copy_(torch.from_numpy(k.view(np.int16)))
        torch.cuda.synchronize()
        assert b.graph_compute([dnode], use_graph=True) == 0
        b.synchronize()
        assert (host(kd) == K.shift_deltas(k, delta, tab_h, hd)).all()
        # the launch shows in mi355x_timing
        g.timing_enable(True)
        assert b.graph_compute([node], use_graph=False) == 0
        b.synchronize()
        rows = g.timing_read()
        g.timing_enable(False)
        assert [r[0] for r in rows] == [f"kq::kq_kv_shift<{hd}, discard>"], rows
    finally:
        b.close()
