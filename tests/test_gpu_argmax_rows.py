"""kq_argmax_rows on the device: every row exact against numpy.argmax(where(isnan(x), -inf, x),
axis=1), through the C-ABI call and through both forms of the backend's ARGMAX_BATCH node. The
sizes follow the kernel's own split (argmax_plan): the smallest multiple of 256 that takes three
workgroups per row, that + 4, and a length that is no multiple of 4 on rows padded to the next
16 bytes (the padding holds +inf: a kernel that read it would answer wrongly). T is 1, 3 and 5,
so the grid has one row and several, and the rows' counters and words lie apart."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -7


def ref_rows(x):
    return np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1).astype(np.int32)


def vocab():
    import ggml_mi355x as g
    v = 256
    while g.argmax_plan(v)[0] < 3:
        v += 256
    return v


def shapes():
    """(n, row_stride) of the three sizes; the slice S of all of them."""
    import ggml_mi355x as g
    v = vocab()
    wgs, s = g.argmax_plan(v)
    assert wgs == 3 and g.argmax_plan(v + 4) == (3, s) and g.argmax_plan(v + 3) == (3, s)
    return [(v, v), (v + 4, v + 4), (v + 3, v + 4)], s


def run(x, stride, dev, workspace=None):
    """x [T, n] on rows of `stride` floats whose padding is +inf."""
    import torch
    import ggml_mi355x as g
    T, n = x.shape
    buf = np.full((T, stride), np.inf, np.float32)
    buf[:, :n] = x
    xd = torch.from_numpy(buf).to(dev)[:, :n]
    out = g.argmax_rows(xd, workspace=workspace)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (T,) and got.dtype == np.int32
    return got


def built_rows(n, S, T):
    """name -> [T, n]: rows built to go wrong. Every row of a case differs from its neighbours."""
    rng = np.random.default_rng(100 * T + n % 7)
    base = rng.standard_normal((T, n)).astype(np.float32)
    neg = (-np.abs(rng.standard_normal((T, n))) - 1.0).astype(np.float32)
    wgs = (n + S - 1) // S
    out = {"random": base.copy(), "all negative": neg.copy()}
    for b in range(1, wgs):  # the maximum on both sides of each slice boundary: the smaller index wins
        x = base.copy()
        x[:, b * S - 1] = x[:, b * S] = 9.5
        out[f"tie across boundary {b}"] = x
        x = base.copy()
        for i in range(T):  # ... and a few entries away from it, another distance in every row
            x[i, b * S - 1 - i] = x[i, b * S + 2 * i] = 9.5
        out[f"tie around boundary {b}"] = x
    x = base.copy()
    for i in range(T):
        x[i, 0 if i % 2 == 0 else n - 1] = 9.5
    out["maximum at 0 / n - 1"] = x
    x = base.copy()
    for i in range(T):
        x[i, n - 1 if i % 2 == 0 else 0] = 9.5
    out["maximum at n - 1 / 0"] = x
    x = base.copy()
    x[:, 0] = x[:, n - 1] = 9.5
    out["tie of first and last"] = x
    for par in (0, 1):  # an all-NaN row next to a normal row
        x = base.copy()
        x[par::2] = np.nan
        out[f"all-NaN rows {par}"] = x
    x = base.copy()
    x[:, ::3] = np.nan
    x[:, :S] = np.nan  # the whole first slice of every row: its workgroup has no entry to offer
    out["NaN never wins"] = x
    x = np.full((T, n), np.nan, np.float32)
    for i in range(T):
        # one number among NaNs, in the tail where n % 4 != 0. (Finite: for -inf among NaNs the
        # kernel's rule, the maximum of the non-NaN entries, and numpy's formula part ways;
        # tests/test_gpu_argmax.py holds kq_argmax to the rule there.)
        x[i, n - 1 - i] = -np.finfo(np.float32).max
    out["one number among NaNs"] = x
    x = neg.copy()
    for i in range(T):  # -0.0 == +0.0: the smaller index wins whichever holds which
        a, b = (-0.0, 0.0) if i % 2 == 0 else (0.0, -0.0)
        x[i, S - 1 - i], x[i, S + 5 + i] = a, b
    out["zero ties"] = x
    x = np.full((T, n), -np.inf, np.float32)
    out["all -inf"] = x.copy()
    for i in range(T):
        x[i, (i * 997 + 3) % n] = np.inf
        x[i, n - 1] = np.inf
    out["+inf twice"] = x
    x = base.copy()
    for i in range(T):
        x[i, (S + 1 + 5 * i) % n] = -np.inf if i % 2 else np.inf
    out["+-inf among numbers"] = x
    x = base.copy()
    for i in range(T):  # every row's maximum in another slice
        sl = i % wgs
        lo, hi = sl * S, min(n, (sl + 1) * S)
        x[i, lo + (i * 131 + 7) % (hi - lo)] = 9.5
    out["a slice per row"] = x
    return out


@pytest.mark.parametrize("T", [1, 3, 5])
@pytest.mark.parametrize("k", range(3), ids=["v3", "v3+4", "odd-padded"])
def test_rows(dev, T, k):
    sh, S = shapes()
    n, stride = sh[k]
    assert (n % 4 != 0) == (k == 2) and stride % 4 == 0
    cases = built_rows(n, S, T)
    assert len(cases) >= 17
    for name, x in cases.items():
        ref = ref_rows(x)
        got = run(x, stride, dev)
        assert (got == ref).all(), (name, n, T, got, ref)
    # the cases mean what their names say
    assert (ref_rows(cases["tie across boundary 1"]) == S - 1).all()
    assert (ref_rows(cases["tie of first and last"]) == 0).all()
    assert (ref_rows(cases["all-NaN rows 0"])[0::2] == 0).all()
    assert (ref_rows(cases["all -inf"]) == 0).all()
    assert (ref_rows(cases["zero ties"]) == S - 1 - np.arange(T)).all()
    if T >= 3:
        assert len(set(ref_rows(cases["a slice per row"])[:3] // S)) == 3


def test_workspace_reuse(dev):
    """Zeroed once by its owner: every call leaves every row's counter at 0 for the next, and the
    counters keep their place whatever n the workspace served before. The first calls run 32
    workgroups a row, so every row's words 0 .. 31 are left non-zero; the short rows after them
    (n = 8, 5, 200: fewer words than that) would never finish if a counter's place depended on n."""
    import torch
    import ggml_mi355x as g
    (n, stride), T, big = shapes()[0][2], 5, 32000
    row = g.argmax_rows_workspace_size(n, 1)
    assert g.argmax_plan(big)[0] >= 17
    assert g.argmax_rows_workspace_size(big, T) == T * row == g.argmax_rows_workspace_size(8, T)
    ws = torch.zeros(T * row, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(11)

    def check(t, m):
        x = rng.standard_normal((t, m)).astype(np.float32)
        got = run(x, (m + 3) & ~3, dev, workspace=ws)
        assert (got == ref_rows(x)).all(), (t, m, got)
        lines = ws.cpu().numpy().reshape(T, row)[:, :128]
        assert (lines == 0).all(), (t, m)  # the counter's whole line: no word lies on it

    for t, m in ((T, big), (T, big), (2, 8), (T, 8), (T, 5), (3, 200), (T, n), (2, n), (T, big), (T, 8)):
        check(t, m)
    words = ws.cpu().numpy().reshape(T, row)[:, 128:].view(np.uint64)
    assert (words[:, :32] != 0).all()  # what the 32-workgroup calls left behind
    xd = torch.zeros((T, stride), dtype=torch.float32, device=dev)
    out = torch.zeros(T, dtype=torch.int32, device=dev)
    rc = g.lib().mi355x_argmax_rows(xd.data_ptr(), n, T, stride, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, None)
    assert rc == g.E_WORKSPACE


def test_backend_buffer_serves_vectors_and_short_rows(dev):
    """One backend: an ARGMAX node over a long vector (126 words behind the counter), then an
    ARGMAX_BATCH node of short rows, then both again: the rows' counters lie clear of the words."""
    import torch
    import ggml_mi355x as g
    nv, n, T = 128256, 8, 3
    b = g.Backend()
    rng = np.random.default_rng(29)
    v = torch.zeros(nv, dtype=torch.float32, device=dev)
    vout = torch.full((1,), -1, dtype=torch.int32, device=dev)
    vt = g.make_tensor(g.TYPE_F32, nv, 1, v.data_ptr())
    vec = g.make_tensor(g.TYPE_I32, 1, 1, vout.data_ptr(), op=g.OP_ARGMAX, srcs=[vt], op_params=[g.ARGMAX_PLAIN],
                        flags=g.FLAG_OUTPUT)
    x = torch.zeros((T, n), dtype=torch.float32, device=dev)
    out = torch.full((T,), -1, dtype=torch.int32, device=dev)
    xt = g.make_tensor(g.TYPE_F32, n, T, x.data_ptr())
    rows = g.make_tensor(g.TYPE_I32, T, 1, out.data_ptr(), op=g.OP_ARGMAX_BATCH, srcs=[xt], op_params=[g.ARGMAX_PLAIN],
                         flags=g.FLAG_OUTPUT)
    big = torch.zeros((T, 32000), dtype=torch.float32, device=dev)
    bout = torch.full((T,), -1, dtype=torch.int32, device=dev)
    bt = g.make_tensor(g.TYPE_F32, 32000, T, big.data_ptr())
    big_rows = g.make_tensor(g.TYPE_I32, T, 1, bout.data_ptr(), op=g.OP_ARGMAX_BATCH, srcs=[bt],
                             op_params=[g.ARGMAX_PLAIN], flags=g.FLAG_OUTPUT)
    # the largest node first, so the buffer is allocated (and zeroed) once and then only reused
    for node, dst, ten in ((big_rows, bout, big), (vec, vout, v), (rows, out, x), (vec, vout, v), (big_rows, bout, big),
                           (rows, out, x)):
        h = rng.standard_normal(tuple(ten.shape)).astype(np.float32)
        ten.copy_(torch.from_numpy(h))
        dst.fill_(-1)
        torch.cuda.synchronize()
        assert b.graph_compute([node], use_graph=False) == 0
        b.synchronize()
        assert (dst.cpu().numpy() == ref_rows(h.reshape(-1, h.shape[-1]))).all(), tuple(ten.shape)
    b.close()


def test_longer_slice_gives_the_same_answers(dev):
    import ggml_mi355x as g
    sh, S = shapes()
    T = 3
    g.debug_knob("ARGMAX_SLICE", 2 * S)
    try:
        for n, stride in sh:
            assert g.argmax_plan(n) == (2, 2 * S)
            for name, x in built_rows(n, S, T).items():
                assert (run(x, stride, dev) == ref_rows(x)).all(), (name, n)
    finally:
        g.debug_knob("ARGMAX_SLICE")  # (NaN: back to the default)


def test_plain_node_replays(dev):
    import torch
    import ggml_mi355x as g
    n, T = vocab(), 3
    b = g.Backend()
    x = torch.zeros((T, n), dtype=torch.float32, device=dev)
    out = torch.full((T,), -1, dtype=torch.int32, device=dev)
    xt = g.make_tensor(g.TYPE_F32, n, T, x.data_ptr())
    node = g.make_tensor(g.TYPE_I32, T, 1, out.data_ptr(), op=g.OP_ARGMAX_BATCH, srcs=[xt], op_params=[g.ARGMAX_PLAIN],
                         flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    rng = np.random.default_rng(13)
    for _ in range(3):  # the same node list, new data: replays of the captured graph
        h = rng.standard_normal((T, n)).astype(np.float32)
        x.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        assert b.graph_compute([node], use_graph=True) == 0
        b.synchronize()
        assert (out.cpu().numpy() == ref_rows(h)).all()
    b.close()


def ref_step(x, tok, pos, cells, mask, hist, cell_stride, n_kv, n_hist, tokens=None):
    """The step-inputs form restated (in place); mask and hist as [T, row] arrays, mask as uint32 bits.
    tokens: the rows' tokens where they are not the argmax (tests/test_gpu_sample.py: the sampled ones)."""
    for i in range(x.shape[0]):
        t = ref_rows(x[i:i + 1])[0] if tokens is None else tokens[i]
        p = np.int32((int(pos[i]) + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31)
        c = np.int32((int(cells[i]) + cell_stride + 2 ** 31) % 2 ** 32 - 2 ** 31)
        tok[i], pos[i], cells[i] = t, p, c
        if 0 <= c < n_kv:  # (the device compares unsigned)
            mask[i, c] = 0  # the bits of 0.0f
        if 0 <= p < n_hist:
            hist[i, p] = t


@pytest.mark.parametrize("cell_stride", [1, 3])
def test_step_inputs_node(dev, cell_stride):
    """The step form on a hand-made input block (tokens | pos | cells | mask, the decoder's layout)
    and a history with padded rows: two runs, the second a replay from the state the first left.
    Rows 0 and 1 advance inside their arrays; row 2's new cell is n_kv (the first run) and row 3's
    new position n_hist: neither is written; row 4 starts from negative values."""
    import torch
    import ggml_mi355x as g
    n, T, n_kv, n_hist, hrow = vocab(), 5, 64, 40, 44
    b = g.Backend()
    rng = np.random.default_rng(17 + cell_stride)
    h = rng.standard_normal((T, n)).astype(np.float32)
    h[1, 5] = h[1, 2000] = 9.5
    x = torch.from_numpy(h).to(dev)
    inp_h = np.full(3 * T + T * n_kv, SENT, np.int32)
    inp_h[T:2 * T] = [5, 0, 7, n_hist - 1, -5]
    inp_h[2 * T:3 * T] = [9, 0, n_kv - cell_stride, 20, -1 - 2 * cell_stride]
    m = inp_h[3 * T:].view(np.float32).reshape(T, n_kv)
    m[:] = -np.inf
    m[:, ::5] = rng.standard_normal((T, len(range(0, n_kv, 5)))).astype(np.float32)
    hist_h = np.full((T, hrow), SENT, np.int32)
    inp = torch.from_numpy(inp_h.copy()).to(dev)
    hist = torch.from_numpy(hist_h.copy()).to(dev)
    srcs = [g.make_tensor(g.TYPE_F32, n, T, x.data_ptr()),
            g.make_tensor(g.TYPE_I32, T, 1, inp[T:2 * T].data_ptr()),
            g.make_tensor(g.TYPE_I32, T, 1, inp[2 * T:3 * T].data_ptr()),
            g.make_tensor(g.TYPE_F32, n_kv, T, inp[3 * T:].data_ptr()),
            g.make_tensor(g.TYPE_I32, n_hist, T, hist.data_ptr(), row_stride=4 * hrow)]
    node = g.make_tensor(g.TYPE_I32, T, 1, inp.data_ptr(), op=g.OP_ARGMAX_BATCH, srcs=srcs,
                         op_params=[g.ARGMAX_STEP_INPUTS, cell_stride, n_kv], flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    torch.cuda.synchronize()
    ref_inp, ref_hist = inp_h.copy(), hist_h.copy()
    for run_no in range(2):
        assert b.graph_compute([node], use_graph=True) == 0
        b.synchronize()
        before = ref_inp.copy()
        ref_step(h, ref_inp[:T], ref_inp[T:2 * T], ref_inp[2 * T:3 * T], ref_inp[3 * T:].view(np.uint32).reshape(T, n_kv),
                 ref_hist, cell_stride, n_kv, n_hist)
        got, hs = inp.cpu().numpy(), hist.cpu().numpy()
        # every word: tokens, pos, cells, the mask bit for bit, the history with its padding
        assert (got.view(np.uint32) == ref_inp.view(np.uint32)).all(), (run_no, np.nonzero(got != ref_inp)[0][:8])
        assert (hs == ref_hist).all(), run_no
        changed = np.nonzero(before[3 * T:] != ref_inp[3 * T:])[0]
        assert len(changed) <= T and (ref_inp[3 * T:][changed] == 0).all()  # at most one mask word per row, +0.0
    assert (ref_hist[:, n_hist:] == SENT).all()
    # what the restatement did with the rows built for it
    assert ref_inp[0] == ref_rows(h)[0] and ref_inp[1] == 5
    assert ref_inp[T + 3] == n_hist + 1 and (ref_hist[3] == SENT).all()        # positions n_hist, n_hist + 1: no entry
    assert ref_inp[2 * T + 2] == n_kv + cell_stride                            # cells n_kv, n_kv + stride: no mask word
    assert (ref_inp[3 * T:].reshape(T, n_kv)[2] == inp_h[3 * T:].reshape(T, n_kv)[2]).all()
    assert ref_inp[T + 4] == -3 and (ref_hist[4] == SENT).all()                # negative positions: no entry
    assert ref_inp[2 * T + 4] == -1                                            # negative cells: no mask word
    assert (ref_inp[3 * T:].reshape(T, n_kv)[4] == inp_h[3 * T:].reshape(T, n_kv)[4]).all()
    b.close()
