"""kq_topk's sampling tail on the device: the token equals tests/sample_ref.ref_sample (the
rule of include/ggml_mi355x.h restated in numpy float32 plus the oracle's v_expf), no tolerance.
The boundary and special cases of tests/test_sample_rule.py, random logits over many draws, the
rows form, and both forms of the backend's SAMPLE node, eager and captured."""
import numpy as np
import pytest

from tests import sample_ref as R
from tests.test_sample_rule import equal_logits

pytestmark = pytest.mark.gpu

F = np.float32
N = 3075  # four slices of the default split, the last of 3 entries


@pytest.fixture(scope="module", autouse=True)
def oracle_lib(oracle):
    from oracle import kq_ops_oracle as O
    O.lib()


class Runner:
    """One workspace, one draw cell and one output for every call of a test."""

    def __init__(self, dev):
        import torch
        import ggml_mi355x as g
        self.dev = dev
        self.ws = torch.zeros(g.topk_workspace_size(N), dtype=torch.uint8, device=dev)
        self.u = torch.zeros(1, dtype=torch.float32, device=dev)
        self.out = torch.zeros(1, dtype=torch.int32, device=dev)
        self.x, self.xd = None, None

    def __call__(self, x, u, **kw):
        import torch
        import ggml_mi355x as g
        if x is not self.x:
            self.x, self.xd = x, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.dev)
        self.u.copy_(torch.from_numpy(np.array([u], np.float32)))
        torch.cuda.synchronize()
        g.sample(self.xd, self.u, out=self.out, workspace=self.ws, **kw)
        torch.cuda.synchronize()
        return int(self.out.cpu()[0])


@pytest.fixture(scope="module")
def run(dev):
    return Runner(dev)


def pad(x, at):
    """x's entries scattered over N entries (the rest far below), so the candidates meet across slices."""
    full = np.full(N, -80.0, np.float32)
    full[at] = x
    return full


def test_eight_equal_logits_draw_boundaries(run):
    x, at = equal_logits(N, 8)
    kw = dict(top_k=8, top_p=1.0, min_p=0.0, temp=1.0)
    for j in range(8):
        assert run(x, j / 8, **kw) == at[j] == R.ref_sample(x, j / 8, **kw)
        below = np.nextafter(F(j / 8), F(-1))
        assert run(x, below, **kw) == R.ref_sample(x, below, **kw) == at[max(j - 1, 0)]


def test_top_p_and_min_p_boundaries(run):
    x, at = equal_logits(N, 4)
    assert run(x, 0.99, top_k=4, top_p=0.5, min_p=0.0, temp=1.0) == at[1]
    assert run(x, 0.49, top_k=4, top_p=0.5, min_p=0.0, temp=1.0) == at[0]
    up = float(np.nextafter(F(0.5), F(1)))
    assert run(x, 0.99, top_k=4, top_p=up, min_p=0.0, temp=1.0) == at[2] == R.ref_sample(x, 0.99, 4, up, 0.0, 1.0)
    x = pad(np.array([2.0, 1.0, 0.0], np.float32), [3, 1500, 3074])
    e = R.ref_trace(x, 0.0, top_k=3, top_p=1.0, min_p=0.0, temp=1.0)["e"]
    for i in (1, 2):
        for mp in (e[i], np.nextafter(e[i], F(0)), np.nextafter(e[i], F(1))):
            for u in (0.0, 0.7, 0.95, 0.9999):
                kw = dict(top_k=3, top_p=1.0, min_p=float(mp), temp=1.0)
                assert run(x, u, **kw) == R.ref_sample(x, u, **kw), (i, mp, u)
    assert run(x, 0.9999, top_k=3, top_p=1.0, min_p=float(np.nextafter(e[2], F(1))), temp=1.0) == 1500
    assert run(x, 0.9999, top_k=3, top_p=1.0, min_p=1.0, temp=1.0) == 3


def test_special_values(run):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(N).astype(np.float32)
    x[rng.integers(0, N, 200)] = np.nan
    for u in (0.0, 0.5, 0.999):
        assert run(x, u, top_k=40, top_p=0.95, min_p=0.05, temp=0.0) == R.ref_argmax(x)
        assert run(x, u, top_k=1, top_p=0.95, min_p=0.05, temp=0.8) == R.ref_argmax(x)
    assert run(np.full(N, np.nan, np.float32), 0.3) == 0
    # a -inf candidate is never drawn by a u in [0, 1); u >= 1 and NaN give c_{q-1}
    x = np.full(N, -np.inf, np.float32)
    x[1030], x[3074] = 0.0, 0.0
    kw = dict(top_k=8, top_p=1.0, min_p=0.0, temp=1.0)
    for u in (0.0, 0.25, float(np.nextafter(F(0.5), F(0))), 0.5, 0.75, float(np.nextafter(F(1), F(0)))):
        assert run(x, u, **kw) == (1030 if u < 0.5 else 3074) == R.ref_sample(x, u, **kw), u
    for u in (1.0, 2.0, np.nan):
        assert run(x, u, **kw) == R.ref_sample(x, u, **kw) == 5
    # a non-finite l_0 gives c_0
    x = rng.standard_normal(N).astype(np.float32)
    x[2000], x[77] = np.inf, np.inf
    assert run(x, 0.9, top_k=4, top_p=1.0, min_p=0.0, temp=1.0) == 77
    assert run(np.full(N, -np.inf, np.float32), 0.9, top_k=4, top_p=1.0, min_p=0.0, temp=1.0) == 0
    # u = 1 and NaN: the last kept candidate
    x, at = equal_logits(N, 5)
    for u in (1.0, 2.0, np.nan):
        assert run(x, u, top_k=5, top_p=1.0, min_p=0.0, temp=1.0) == at[4]
        assert run(x, u, top_k=5, top_p=0.6, min_p=0.0, temp=1.0) == at[2]
    # a tiny temperature: d / temp is -inf or 0, never inf - inf
    x = pad(np.array([3.0, 1.0, 3.0, -2.0], np.float32), [10, 1100, 2100, 3074])
    assert run(x, 0.75, top_k=4, top_p=1.0, min_p=0.0, temp=1e-30) == 2100
    assert run(x, 0.25, top_k=4, top_p=1.0, min_p=0.0, temp=1e-30) == 10


PARAMS = [dict(top_k=40, top_p=0.95, min_p=0.05, temp=0.8), dict(top_k=64, top_p=1.0, min_p=0.0, temp=4.0),
          dict(top_k=7, top_p=0.7, min_p=0.2, temp=0.3)]


@pytest.mark.parametrize("kw", PARAMS, ids=["default", "flat", "sharp"])
def test_random_logits(run, kw):
    """Standard normal x 4 over 64 draws: the same token as the reference for every draw, and the
    draws reach more than one candidate."""
    seed = PARAMS.index(kw)
    x = (np.random.default_rng(100 + seed).standard_normal(N) * 4).astype(np.float32)
    us = R.draws(200 + seed, 64)
    want = [R.ref_sample(x, u, **kw) for u in us]
    got = [run(x, float(u), **kw) for u in us]
    assert got == want
    assert len(set(want)) > 1


def test_rows(dev):
    import torch
    import ggml_mi355x as g
    T = 3
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((T, N + 1)) * 4).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)[:, :N]
    us = R.draws(13, T)
    kw = dict(top_k=40, top_p=0.95, min_p=0.05, temp=2.0)
    out = g.sample_rows(xd, torch.from_numpy(us).to(dev), **kw)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [R.ref_sample(x[i, :N], us[i], **kw) for i in range(T)]


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
def test_plain_batch_node(dev, use_graph):
    """The plain SAMPLE_BATCH node, T = 3 rows with a draw each, replayed on new data and draws."""
    import torch
    import ggml_mi355x as g
    T, n = 3, 3076  # (the batch node's rows: a multiple of 4 entries, packed)
    b = g.Backend()
    x = torch.zeros((T, n), dtype=torch.float32, device=dev)
    u = torch.zeros(T, dtype=torch.float32, device=dev)
    out = torch.full((T,), -1, dtype=torch.int32, device=dev)
    kw = dict(top_k=40, top_p=0.95, min_p=0.05, temp=2.0)
    xt = g.make_tensor(g.TYPE_F32, n, T, x.data_ptr())
    ut = g.make_tensor(g.TYPE_F32, T, 1, u.data_ptr())
    node = g.make_tensor(g.TYPE_I32, T, 1, out.data_ptr(), op=g.OP_SAMPLE_BATCH, srcs=[xt, ut],
                         op_params=g.sampler_params(g.SAMPLE_PLAIN, 40, 2.0, 0.95, 0.05), flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    rng = np.random.default_rng(14)
    tokens = set()
    for i in range(3):
        h = (rng.standard_normal((T, n)) * 4).astype(np.float32)
        us = R.draws(15 + i, T)
        x.copy_(torch.from_numpy(h))
        u.copy_(torch.from_numpy(us))
        torch.cuda.synchronize()
        assert b.graph_compute([node], use_graph=use_graph) == 0
        b.synchronize()
        want = [R.ref_sample(h[r], us[r], **kw) for r in range(T)]
        assert out.cpu().tolist() == want
        assert all(want[r] != R.ref_argmax(h[r]) for r in range(2))  # (a draw decides, not the maximum)
        tokens.update(want)
    assert len(tokens) > T
    b.close()


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
def test_plain_node_and_the_backend_buffer(dev, use_graph):
    """The plain SAMPLE node, replayed on new data and a new draw; then, on the same backend (one
    buffer), 126 slices at top_k 64 followed by 8 entries at top_k 2."""
    import torch
    import ggml_mi355x as g
    b = g.Backend()
    u = torch.zeros(1, dtype=torch.float32, device=dev)
    out = torch.full((1,), -1, dtype=torch.int32, device=dev)

    def node_of(x, kw):
        xt = g.make_tensor(g.TYPE_F32, x.numel(), 1, x.data_ptr())
        ut = g.make_tensor(g.TYPE_F32, 1, 1, u.data_ptr())
        nd = g.make_tensor(g.TYPE_I32, 1, 1, out.data_ptr(), op=g.OP_SAMPLE, srcs=[xt, ut],
                           op_params=g.sampler_params(g.SAMPLE_PLAIN, kw["top_k"], kw["temp"], kw["top_p"], kw["min_p"]),
                           flags=g.FLAG_OUTPUT)
        assert g.supports_op(nd)
        return nd, (xt, ut)

    rng = np.random.default_rng(13)
    kw = dict(top_k=40, top_p=0.95, min_p=0.05, temp=1.5)
    x = torch.zeros(N, dtype=torch.float32, device=dev)
    node, keep = node_of(x, kw)
    for i in range(3):  # the same node list, new data: a replay of the captured graph
        h = (rng.standard_normal(N) * 4).astype(np.float32)
        x.copy_(torch.from_numpy(h))
        u.fill_(0.3 * i + 0.1)
        torch.cuda.synchronize()
        assert b.graph_compute([node], use_graph=use_graph) == 0
        b.synchronize()
        assert int(out.cpu()[0]) == R.ref_sample(h, F(0.3 * i + 0.1), **kw)
    big_h = (rng.standard_normal(128256) * 4).astype(np.float32)
    small_h = (rng.standard_normal(8) - 30.0).astype(np.float32)
    big, small = torch.from_numpy(big_h).to(dev), torch.from_numpy(small_h).to(dev)
    kb, ks = dict(top_k=64, top_p=1.0, min_p=0.0, temp=3.0), dict(top_k=2, top_p=1.0, min_p=0.0, temp=3.0)
    nb, keep_b = node_of(big, kb)
    ns, keep_s = node_of(small, ks)
    u.fill_(0.8)
    torch.cuda.synchronize()
    for nd, h, k in ((nb, big_h, kb), (ns, small_h, ks), (nb, big_h, kb)):
        assert b.graph_compute([nd], use_graph=use_graph) == 0
        b.synchronize()
        assert int(out.cpu()[0]) == R.ref_sample(h, F(0.8), **k)
    b.close()


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
def test_step_inputs_node(dev, use_graph):
    """The step-inputs form, driven directly, as tests/test_gpu_argmax.py::test_step_inputs_node
    checks ARGMAX's: the token, pos + 1, the rope row of pos + 1 and the history entry; the draw
    is draws[pos + 1], and pos + 1 outside the table gives c_0."""
    import torch
    import ggml_mi355x as g
    hd, rows, n_draws = 64, 32, 20
    b = g.Backend()
    rng = np.random.default_rng(17)
    h = (rng.standard_normal(N) * 4).astype(np.float32)
    x = torch.from_numpy(h).to(dev)
    table_h = rng.standard_normal((rows, hd)).astype(np.float32)
    table = torch.from_numpy(table_h).to(dev)
    draws_h = R.draws(18, n_draws)
    draws = torch.from_numpy(draws_h).to(dev)
    kw = dict(top_k=40, top_p=1.0, min_p=0.0, temp=4.0)
    want = [R.ref_sample(h, u, **kw) for u in draws_h]
    c0 = R.ref_argmax(h)
    assert len(set(want)) > 3 and any(w != c0 for w in want[6:8])
    SENT = -7
    inp = torch.full((2 + hd,), SENT, dtype=torch.int32, device=dev)
    hist = torch.full((rows,), SENT, dtype=torch.int32, device=dev)
    srcs = [g.make_tensor(g.TYPE_F32, N, 1, x.data_ptr()),
            g.make_tensor(g.TYPE_I32, 1, 1, inp[1:2].data_ptr()),  # pos = dst + 1, as in the decoder
            g.make_tensor(g.TYPE_F32, hd, rows, table.data_ptr()),
            g.make_tensor(g.TYPE_I32, rows, 1, hist.data_ptr()),
            g.make_tensor(g.TYPE_F32, n_draws, 1, draws.data_ptr())]
    node = g.make_tensor(g.TYPE_I32, 2 + hd, 1, inp.data_ptr(), op=g.OP_SAMPLE, srcs=srcs,
                         op_params=g.sampler_params(g.SAMPLE_STEP_INPUTS, 40, 4.0, 1.0, 0.0), flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)

    def step(pos):
        if pos is not None:
            inp.fill_(SENT)
            hist.fill_(SENT)
            inp[1] = pos
            torch.cuda.synchronize()
        assert b.graph_compute([node], use_graph=use_graph) == 0
        b.synchronize()
        return inp.cpu().numpy(), hist.cpu().numpy()

    got, hs = step(5)
    assert got[0] == want[6] and got[1] == 6 and (got[2:] == table_h[6].view(np.int32)).all()
    assert hs[6] == want[6] and (np.delete(hs, 6) == SENT).all()
    got, hs = step(None)  # a second run from the state the first left: pos 6 -> 7, the next draw
    assert got[0] == want[7] and got[1] == 7 and (got[2:] == table_h[7].view(np.int32)).all()
    assert hs[7] == want[7] and hs[6] == want[6] and (np.delete(hs, [6, 7]) == SENT).all()
    got, hs = step(n_draws - 2)  # the table's last entry
    assert got[0] == want[n_draws - 1] and got[1] == n_draws - 1
    got, hs = step(n_draws - 1)  # pos + 1 outside the draws: u = 0, c_0; the rope row and history exist
    assert got[0] == c0 and got[1] == n_draws and (got[2:] == table_h[n_draws].view(np.int32)).all()
    assert hs[n_draws] == c0
    got, hs = step(rows - 1)  # the last row: the token and pos + 1 are written, the row and history are not
    assert got[0] == c0 and got[1] == rows and (got[2:] == SENT).all() and (hs == SENT).all()
    got, hs = step(-2)  # a negative position (unsigned compares): -2 + 1 is outside every table
    assert got[0] == c0 and got[1] == -1 and (got[2:] == SENT).all() and (hs == SENT).all()
    got, hs = step(-1)  # -1 + 1 = 0: entry 0 of each
    assert got[0] == want[0] and got[1] == 0 and (got[2:] == table_h[0].view(np.int32)).all() and hs[0] == want[0]
    b.close()


B_T, B_N, B_NKV, B_NHIST, B_HROW, B_NDRAWS, B_DROW = 5, 3076, 64, 40, 44, 20, 24
B_KW = dict(top_k=40, top_p=1.0, min_p=0.0, temp=4.0)
B_POS = [5, 0, B_NDRAWS - 1, B_NHIST - 1, -5]
PAD_DRAW = F(0.999)  # the draws' padding: a kernel that read it would not answer c_0


def batch_step_case():
    """The inputs of test_step_inputs_batch_node and, per run, the tokens of the reference: row i's
    is ref_sample with the draw draws[i][pos[i] + 1], 0.0 where the table has no such entry."""
    if not hasattr(batch_step_case, "made"):
        h = (np.random.default_rng(23).standard_normal((B_T, B_N)) * 4).astype(np.float32)
        draws = np.full((B_T, B_DROW), PAD_DRAW, np.float32)
        for i in range(B_T):
            draws[i, :B_NDRAWS] = R.draws([24, i], B_NDRAWS)
        tokens = []
        for run_no in range(2):
            new = [p + 1 + run_no for p in B_POS]
            tokens.append([R.ref_sample(h[i], draws[i, p] if 0 <= p < B_NDRAWS else F(0.0), **B_KW)
                           for i, p in enumerate(new)])
        batch_step_case.made = h, draws, tokens
    return batch_step_case.made


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
@pytest.mark.parametrize("cell_stride", [1, 3])
def test_step_inputs_batch_node(dev, cell_stride, use_graph):
    """The step-inputs SAMPLE_BATCH node on a hand-made input block (tokens | pos | cells | mask, the
    decoder's layout) with sentinels, a history with padded rows and a draws table with padded rows,
    as tests/test_gpu_argmax_rows.py::test_step_inputs_node drives ARGMAX_BATCH's: two runs, the
    second from the state the first left. Every word of the block and of the history equals
    ref_step's rule on the tokens of ref_sample. Rows 0 and 1 advance inside all their arrays; row
    2's new cell is n_kv (no mask word) and its new position n_draws (the draw is 0.0, the token c_0,
    the history and the cell are written); row 3's new position is n_hist (no history entry); row 4
    starts from a negative position and cell."""
    import torch
    import ggml_mi355x as g
    from tests.test_gpu_argmax_rows import SENT, ref_step
    T, n, n_kv, n_hist = B_T, B_N, B_NKV, B_NHIST
    h, draws_h, tokens = batch_step_case()
    c0 = [R.ref_argmax(h[i]) for i in range(T)]
    # of the reference itself: draws decide (else the greedy tail would pass), and row 2 shows a read of the padding
    for run_no in range(2):
        assert sum(tokens[run_no][i] != c0[i] for i in range(T)) >= 2 and tokens[run_no][2] == c0[2]
    assert R.ref_sample(h[2], PAD_DRAW, **B_KW) != c0[2]
    b = g.Backend()
    x = torch.from_numpy(h).to(dev)
    draws = torch.from_numpy(draws_h).to(dev)
    inp_h = np.full(3 * T + T * n_kv, SENT, np.int32)
    inp_h[T:2 * T] = B_POS
    inp_h[2 * T:3 * T] = [9, 0, n_kv - cell_stride, 20, -1 - 2 * cell_stride]
    m = inp_h[3 * T:].view(np.float32).reshape(T, n_kv)
    m[:] = -np.inf
    m[:, ::5] = np.random.default_rng(25).standard_normal((T, len(range(0, n_kv, 5)))).astype(np.float32)
    hist_h = np.full((T, B_HROW), SENT, np.int32)
    inp = torch.from_numpy(inp_h.copy()).to(dev)
    hist = torch.from_numpy(hist_h.copy()).to(dev)
    srcs = [g.make_tensor(g.TYPE_F32, n, T, x.data_ptr()),
            g.make_tensor(g.TYPE_I32, T, 1, inp[T:2 * T].data_ptr()),
            g.make_tensor(g.TYPE_I32, T, 1, inp[2 * T:3 * T].data_ptr()),
            g.make_tensor(g.TYPE_F32, n_kv, T, inp[3 * T:].data_ptr()),
            g.make_tensor(g.TYPE_I32, n_hist, T, hist.data_ptr(), row_stride=4 * B_HROW),
            g.make_tensor(g.TYPE_F32, B_NDRAWS, T, draws.data_ptr(), row_stride=4 * B_DROW)]
    node = g.make_tensor(g.TYPE_I32, T, 1, inp.data_ptr(), op=g.OP_SAMPLE_BATCH, srcs=srcs,
                         op_params=g.sampler_params(g.SAMPLE_STEP_INPUTS, 40, 4.0, 1.0, 0.0) + [cell_stride, n_kv],
                         flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    torch.cuda.synchronize()
    ref_inp, ref_hist = inp_h.copy(), hist_h.copy()
    for run_no in range(2):
        assert b.graph_compute([node], use_graph=use_graph) == 0
        b.synchronize()
        ref_step(h, ref_inp[:T], ref_inp[T:2 * T], ref_inp[2 * T:3 * T], ref_inp[3 * T:].view(np.uint32).reshape(T, n_kv),
                 ref_hist, cell_stride, n_kv, n_hist, tokens=tokens[run_no])
        got, hs = inp.cpu().numpy(), hist.cpu().numpy()
        # every word: tokens, pos, cells, the mask bit for bit, the history with its padding
        assert (got.view(np.uint32) == ref_inp.view(np.uint32)).all(), (run_no, np.nonzero(got != ref_inp)[0][:8])
        assert (hs == ref_hist).all(), run_no
    # what the restatement did with the rows built for them
    mask0, mask1 = inp_h[3 * T:].reshape(T, n_kv), ref_inp[3 * T:].reshape(T, n_kv)
    assert [int((mask0[i] != mask1[i]).sum()) for i in range(T)] == [2, 2, 0, 2, 0]
    assert ref_inp[2 * T + 2] == n_kv + cell_stride and ref_inp[2 * T + 4] == -1   # cells n_kv ..: no mask word; negative: none
    assert (ref_hist[2, B_NDRAWS:B_NDRAWS + 2] == c0[2]).all()                     # positions n_draws ..: c_0, filed
    assert ref_inp[T + 3] == n_hist + 1 and (ref_hist[3] == SENT).all()            # positions n_hist ..: no entry
    assert ref_inp[T + 4] == -3 and (ref_hist[4] == SENT).all()                    # negative positions: no entry
    assert (ref_hist[:, n_hist:] == SENT).all()
    b.close()
