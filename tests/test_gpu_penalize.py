"""mi355x_penalize_rows and the PENALIZE node on the device against tests/penalize_ref.py: whole
matrices as uint32, the rows' padding included. The padding of x is poisoned; the history rows
stand in a larger buffer whose other entries hold a valid token that no window and no list names
(GUARD: an entry read from outside a row's [0, n_hist) would edit x[GUARD]), and so do the entries
around end."""
import numpy as np
import pytest

from tests import penalize_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x7fa5a5a5  # the padding of x
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
PEN = dict(repeat=1.1, freq=0.25, present=0.5)


def f_of(bits):
    return np.array([bits], np.uint32).view(F)[0]


class Case:
    """x [rows, stride] with n entries a row in use, a history [rows, n_hist] inside a guarded buffer
    of rows of hrow entries, and end [rows] inside a guarded buffer."""

    def __init__(self, seed, n, rows, ends, n_hist=64, stride=None, hrow=None, tokens=None, special=True):
        rng = np.random.default_rng(seed)
        self.n, self.rows, self.stride, self.n_hist = n, rows, n if stride is None else stride, n_hist
        self.hrow = n_hist + 5 if hrow is None else hrow
        self.guard = n - 1  # a token of the vocabulary that no window and no list holds
        x = np.full((rows, self.stride), f_of(POISON), F)
        x[:, :n] = (4 * rng.standard_normal((rows, n))).astype(F)
        if special and n >= 7:
            x[:, 0] = f_of(0x7fc12345)  # a NaN with a payload
            x[:, 1], x[:, 2], x[:, 3], x[:, 4] = np.inf, -np.inf, 0.0, -0.0
            if n > 16:
                x[:, n - 2] = f_of(0xffc00001)  # ... and one no window names: it keeps its bits
        self.x = x
        top = max(1, min(n - 2, 48))  # ids [0, top): repeats are common
        h = rng.integers(0, top, (rows, n_hist)).astype(np.int32) if tokens is None else np.array(tokens, np.int32)
        assert h.shape == (rows, n_hist)
        self.hist = h
        self.buf = np.full(8 + rows * self.hrow + 8, self.guard, np.int32)
        self.buf[8:8 + rows * self.hrow].reshape(rows, self.hrow)[:, :n_hist] = h
        self.ends = np.array(ends, np.int64)
        assert self.ends.shape == (rows,)
        self.end_buf = np.full(4 + rows + 4, 3, np.int32)  # (3: another window than any row's)
        self.end_buf[4:4 + rows] = self.ends.astype(np.int32)

    def to(self, dev):
        import torch
        self.xd = torch.from_numpy(self.x.copy()).to(dev)
        self.bufd = torch.from_numpy(self.buf).to(dev)
        self.endd = torch.from_numpy(self.end_buf).to(dev)
        self.histd = self.bufd[8:8 + self.rows * self.hrow].view(self.rows, self.hrow)[:, :self.n_hist]
        return self

    def ref(self, x=None, ends=None, **kw):
        return R.penalize_rows(self.x if x is None else x, self.hist, self.ends if ends is None else ends, n=self.n, **kw)

    def run(self, **kw):
        import ggml_mi355x as g
        import torch
        g.penalize_rows(self.xd[:, :self.n], self.histd, self.endd[4:4 + self.rows], **kw)
        torch.cuda.synchronize()
        return self.xd.cpu().numpy()

    def untouched_buffers(self):
        return (self.bufd.cpu().numpy() == self.buf).all() and (self.endd.cpu().numpy() == self.end_buf).all()


def check(case, got, want, touched, what=""):
    assert R.same(got, want, touched), (what, R.first_mismatch(got, want, touched))
    pad = got[:, case.n:].view(np.uint32)
    assert (pad == POISON).all(), what
    assert case.untouched_buffers(), what


def mixed_bias(n):
    """Duplicates, a token that is in every window's range and one that is only biased, a ban,
    ids outside the vocabulary."""
    only = n - 3 if n > 60 else n - 1
    return [(2, 0.5), (only, 1.25), (2, -0.125), (5 % n, -np.inf), (-1, 9.0), (n, 9.0), (I32_MIN, 9.0), (only, -3.0),
            (0, 1.0), (1, -np.inf), (4 % n, 2.0)]


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("n,stride,rows", [(7, 12, 1), (7, 12, 3), (1024, 1024, 1), (1024, 1028, 3), (32000, 32000, 3)],
                         ids=["n7", "n7x3", "n1024", "n1024x3", "n32000x3"])
def test_shapes(dev, n, stride, rows):
    ends = [63, 40, 9][:rows]  # each row its own window
    c = Case(1, n, rows, ends, stride=stride).to(dev)
    bias = [(t, v) for t, v in mixed_bias(n) if t != c.guard]
    want, touched = c.ref(last_n=20, bias=bias, **PEN)
    check(c, c.run(last_n=20, bias=bias, **PEN), want, touched)
    assert touched.any(axis=1).all() and not touched[:, c.guard].any()


# ---------------------------------------------------------------- window lengths
@pytest.mark.parametrize("last_n", [1, 2, 64, 255, 256, 257, 1024])
def test_window_lengths(dev, last_n):
    c = Case(2 + last_n, 1024, 3, [1499, 700, 100], n_hist=1500).to(dev)  # row 2: clipped at 0 from last_n 102 on
    want, touched = c.ref(last_n=last_n, bias=mixed_bias(1024), **PEN)
    check(c, c.run(last_n=last_n, bias=mixed_bias(1024), **PEN), want, touched)
    assert not touched[:, c.guard].any()
    # the window alone
    c.to(dev)
    want, touched = c.ref(last_n=last_n, **PEN)
    check(c, c.run(last_n=last_n, **PEN), want, touched, "no bias")
    assert touched.sum(axis=1).tolist() == [len(set(R.window(c.hist[i], c.ends[i], last_n))) for i in range(3)]


# ---------------------------------------------------------------- window position
@pytest.mark.parametrize("last_n", [5, 64, 1024])
def test_window_position(dev, last_n):
    n_hist = 40
    ends = [0, 3, -1, n_hist - 1, n_hist, n_hist + 3, n_hist + 63, n_hist + 5000, I32_MIN, I32_MAX, -64, I32_MAX - 1023]
    c = Case(5, 1024, len(ends), ends, n_hist=n_hist).to(dev)
    want, touched = c.ref(last_n=last_n, **PEN)
    check(c, c.run(last_n=last_n, **PEN), want, touched)
    rows = touched.any(axis=1).tolist()
    assert rows[0] and rows[1] and not rows[2] and rows[3] and not rows[8] and not rows[9] and not rows[10] and not rows[11]
    assert rows[4] == (last_n > 1) and rows[5] == (last_n > 4) and rows[6] == (last_n > 64) and not rows[7]
    assert not touched[:, c.guard].any()  # nothing outside a row of the history was read


# ---------------------------------------------------------------- repeats and ids
def test_one_repeated_token(dev):
    n_hist = 1100
    tokens = np.full((2, n_hist), 9, np.int32)
    tokens[1, ::2] = 11
    c = Case(7, 1024, 2, [1099, 1050], n_hist=n_hist, tokens=tokens).to(dev)
    kw = dict(last_n=1024, repeat=1.0, freq=0.001, present=0.0)
    want, touched = c.ref(**kw)
    check(c, c.run(**kw), want, touched)
    assert touched.sum(axis=1).tolist() == [1, 2]
    assert want[0, 9] == F(c.x[0, 9] - F(F(1024.0) * F(0.001)))  # (float)1024 * freq


def test_token_ids_outside_the_vocabulary(dev):
    n, n_hist = 1024, 64
    tokens = np.random.default_rng(8).integers(0, 40, (3, n_hist)).astype(np.int32)
    tokens[:, ::3] = -1
    tokens[:, 1::7] = n
    tokens[:, 2::11] = I32_MIN
    tokens[2, :] = [-1, n, I32_MIN, I32_MAX] * 16  # a window without one token of the vocabulary
    c = Case(8, n, 3, [63, 50, 63], n_hist=n_hist, tokens=tokens).to(dev)
    bias = [(-1, 1.0), (n, 1.0), (I32_MIN, -np.inf), (I32_MAX, 1.0), (n + 5, 2.0)]
    want, touched = c.ref(last_n=64, bias=bias, **PEN)
    check(c, c.run(last_n=64, bias=bias, **PEN), want, touched)
    assert touched[0].any() and touched[1].any() and not touched[2].any()


# ---------------------------------------------------------------- logit values
def test_special_logit_values(dev):
    """NaN with a payload, +-inf, +-0: in the window, biased, both, and untouched."""
    n, n_hist = 64, 16
    tokens = np.array([[0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 20, 21, 22, 23, 24, 25]], np.int32)
    c = Case(9, n, 1, [15], n_hist=n_hist, tokens=tokens)
    vals = [f_of(0x7fc12345), np.inf, -np.inf, 0.0, -0.0]
    for base in (0, 8, 30):  # [0, 5): window; [8, 13): biased only; [30, 35): untouched
        c.x[0, base:base + 5] = vals
    c.x[0, 20:25] = vals     # window and biased
    c.to(dev)
    bias = [(8 + i, 1.5) for i in range(5)] + [(20 + i, -2.5) for i in range(5)] + [(9, -np.inf), (10, np.inf), (12, -0.0)]
    want, touched = c.ref(last_n=16, bias=bias, **PEN)
    got = c.run(last_n=16, bias=bias, **PEN)
    check(c, got, want, touched)
    assert (got[0, 30:35].view(np.uint32) == c.x[0, 30:35].view(np.uint32)).all()  # the payload too
    assert np.isnan(got[0, [0, 8, 20]]).all() and np.isnan(got[0, 9]) and np.isnan(got[0, 10])  # NaN stays; inf - inf
    assert got[0, 2] == -np.inf and got[0, 1] == np.inf
    assert got[0, 3] == got[0, 4] == F(-1.0)  # -0.0 counts as <= 0; twice in the window: 2 * 0.25 + 0.5
    # identity parameters leave every finite and infinite value's bits
    c.x[0, [0, 8, 20]] = 1.0
    c.to(dev)
    got = c.run(last_n=16, repeat=1.0, freq=0.0, present=0.0)
    assert (got.view(np.uint32) == c.x.view(np.uint32)).all()


# ---------------------------------------------------------------- bias lists
@pytest.mark.parametrize("n_bias", [0, 1, 255, 256])
@pytest.mark.parametrize("last_n", [0, 64])
def test_bias_lists(dev, n_bias, last_n):
    n = 1024
    rng = np.random.default_rng(10 + n_bias)
    # tokens of the windows' range and others, many twice or more; the order matters
    toks = rng.integers(0, 120, n_bias)
    vals = (8 * rng.standard_normal(n_bias)).astype(F)
    bias = [(int(t), float(v)) for t, v in zip(toks, vals)]
    if n_bias >= 255:
        bias[3], bias[100], bias[200], bias[254] = (7, -np.inf), (7, 1.0), (1000, 1e8), (1000, -1e8)
        bias[17], bias[18] = (900, -1e8), (900, 1e-3)
    elif n_bias == 1:
        bias = [(7, -np.inf)]
    c = Case(11, n, 3, [63, 30, 5]).to(dev)
    c.x[:, 900] = 1e8
    c.to(dev)
    want, touched = c.ref(last_n=last_n, bias=bias, **PEN)
    check(c, c.run(last_n=last_n, bias=bias, **PEN), want, touched)
    if n_bias >= 255:
        assert (want[:, 7] == -np.inf).all() and (want[:, 900] == F(1e-3)).all()  # a ban; the order of the biases
    if n_bias == 0 and last_n == 0:
        assert not touched.any()


def test_bias_order_on_the_device(dev):
    c = Case(12, 64, 1, [0], special=False)
    c.x[0, 10] = c.x[0, 11] = 1e8
    c.to(dev)
    got = c.run(bias=[(10, -1e8), (10, 1e-3), (11, 1e-3), (11, -1e8)])
    assert got[0, 10] == F(1e-3) and got[0, 11] == F(0.0)


# ---------------------------------------------------------------- repeated calls
def test_two_calls_equal_the_reference_applied_twice(dev):
    c = Case(13, 1024, 3, [63, 20, 2]).to(dev)
    kw = dict(last_n=64, bias=mixed_bias(1024), **PEN)
    once, t1 = c.ref(**kw)
    twice, t2 = c.ref(x=once, **kw)
    c.run(**kw)
    check(c, c.run(**kw), twice, t1 | t2)
    assert not R.same(once, twice, np.zeros_like(t1))


def test_a_vector_and_the_refusals(dev):
    import torch
    import ggml_mi355x as g
    c = Case(14, 1024, 1, [63]).to(dev)
    want, touched = c.ref(last_n=64, bias={3: 1.0}, **PEN)
    v = c.xd[0]
    assert g.penalize_rows(v, c.histd[0], 63, last_n=64, bias={3: 1.0}, **PEN) is v
    torch.cuda.synchronize()
    check(c, c.xd.cpu().numpy(), want, touched)
    with pytest.raises(g.Mi355xError):
        g.penalize_rows(v, c.histd[0], None, last_n=64)
    with pytest.raises(g.Mi355xError):
        g.penalize_rows(v, None, 63, last_n=64)
    with pytest.raises(g.Mi355xError):
        g.penalize_rows(v, c.histd[0], 63, last_n=1025)
    with pytest.raises(g.Mi355xError):
        g.penalize_rows(v, c.histd[0], 63, last_n=64, repeat=0.0)
    with pytest.raises(g.Mi355xError):
        g.penalize_rows(v, bias=[(i, 1.0) for i in range(257)])
    with pytest.raises(g.Mi355xError):
        g.penalize_rows(v.to(torch.float64))
    check(c, c.xd.cpu().numpy(), want, touched, "a refused call wrote nothing")


# ---------------------------------------------------------------- the node
@pytest.mark.parametrize("T", [1, 3])
def test_node_eager_and_replayed(dev, T):
    """The PENALIZE node in place on its src0: eager, then replayed from the hipGraph twice with end
    changed on the device in between (the same node list: end is read at run time)."""
    import torch
    import ggml_mi355x as g
    n, n_hist = 1024, 200
    c = Case(15 + T, n, T, [150, 63, 7][:T], n_hist=n_hist).to(dev)
    bias = mixed_bias(n)
    bt = torch.tensor([t for t, _ in bias], dtype=torch.int32).to(dev)
    bv = torch.tensor([v for _, v in bias], dtype=torch.float32).to(dev)
    end = c.endd[4:4 + T]
    xt = g.make_tensor(g.TYPE_F32, n, T, c.xd.data_ptr())
    srcs = [xt, g.make_tensor(g.TYPE_I32, T, 1, end.data_ptr()),
            g.make_tensor(g.TYPE_I32, n_hist, T, c.histd.data_ptr(), row_stride=4 * c.hrow),
            g.make_tensor(g.TYPE_I32, len(bias), 1, bt.data_ptr()), g.make_tensor(g.TYPE_F32, len(bias), 1, bv.data_ptr())]
    node = g.make_tensor(g.TYPE_F32, n, T, c.xd.data_ptr(), op=g.OP_PENALIZE, srcs=srcs,
                         op_params=g.penalize_params(64, PEN["repeat"], PEN["freq"], PEN["present"], len(bias)),
                         flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    b = g.Backend()
    try:
        runs = [(False, c.ends), (True, c.ends), (True, np.array([199, 5, 120][:T])), (True, np.array([-1, 250, I32_MAX][:T]))]
        seen = []
        for use_graph, ends in runs:
            c.xd.copy_(torch.from_numpy(c.x))
            end.copy_(torch.from_numpy(ends.astype(np.int32)))
            torch.cuda.synchronize()
            assert b.graph_compute([node], use_graph=use_graph) == 0
            b.synchronize()
            want, touched = c.ref(ends=ends, last_n=64, bias=bias, **PEN)
            got = c.xd.cpu().numpy()
            assert R.same(got, want, touched), (use_graph, ends, R.first_mismatch(got, want, touched))
            assert (c.bufd.cpu().numpy() == c.buf).all()
            seen.append(want)
        assert not R.same(seen[1], seen[2], np.zeros(seen[1].shape, bool))  # the changed end changed the result
    finally:
        b.close()
