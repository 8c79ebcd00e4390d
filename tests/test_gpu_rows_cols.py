"""kq_rows_cols (mi355x_small_batch FUSED): 2 to 15 activation columns through mul_mat and the
graph backend against the CPU oracle's mul_mat, by bits, one kq_rows_cols launch per call."""
import numpy as np
import pytest

from tests.llama_model import kquant
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fused():
    import ggml_mi355x as g
    prev = g.small_batch(g.SMALL_BATCH_FUSED)
    yield
    g.small_batch(prev)


def _timed(run):
    import ggml_mi355x as g
    g.timing_enable(True)
    try:
        out = run()
        return out, [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)


def _one_cols_launch(names):
    assert sum("kq_rows_cols" in n for n in names) == 1 and not any("kq_gemv<" in n for n in names), names


def _x(rng, M, K):
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[M // 2, 256:512] = 0.0  # one column with an all-zero middle superblock (d = 0)
    return x


def _check_mul_mat(dev, oracle, type_, K, N, M, seed, offset=0):
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(seed)
    w = kquant(rng, type_, N, K, edges=True)
    x = _x(rng, M, K)
    buf = torch.zeros(w.size + 16, dtype=torch.uint8, device=dev)
    wd = buf[offset:offset + w.size].view(N, w.shape[1])
    wd.copy_(t(w, dev))
    got, names = _timed(lambda: g.mul_mat(type_, wd, K, t(x, dev)).cpu().numpy())
    _one_cols_launch(names)
    ref = oracle.mul_mat(type_, w, x)
    assert bits_equal(got, ref), first_mismatch(got, ref)


@pytest.mark.parametrize("type_", [12, 13, 14])
@pytest.mark.parametrize("M", [2, 3, 8, 9, 15])
def test_single_matrix(dev, oracle, type_, M):
    """K = 768: three superblocks, a step that is not full; N = 70: partial last batch and wave."""
    _check_mul_mat(dev, oracle, type_, 768, 70, M, 1000 * type_ + M)


def test_long_stream_unaligned_q6(dev, oracle):
    """17 superblocks a row, past one step; no row of the Q6_K matrix 16-byte aligned."""
    _check_mul_mat(dev, oracle, 14, 4352, 9, 5, 7, offset=2)


def _smallest_n_with_two_batches(K, M, type_):
    import ggml_mi355x as g
    lo, hi = 1, 1 << 20  # rows_per_wave grows with N: bisect the first N past one chain batch
    while lo < hi:
        mid = (lo + hi) // 2
        p = g.rows_cols_plan(K, M, type=type_, n_rows=mid)
        lo, hi = (lo, mid) if p["rows_per_wave"] > p["batch_rows"] else (mid + 1, hi)
    return lo


def test_narrower_group_and_two_row_batches(dev, oracle):
    """The first K whose layout has no room for a group of 8 (from rows_cols_layout, not a
    number written here), at the smallest N whose waves replay two chain batches."""
    import ggml_mi355x as g
    K = next(k for k in range(256, 1 << 16, 256) if g.rows_cols_plan(k, 8)["ncol"] < 8)
    N = _smallest_n_with_two_batches(K, 8, 12)
    p = g.rows_cols_plan(K, 8, n_rows=N)
    assert p["ncol"] in (2, 4) and p["groups"] == 8 // p["ncol"] and p["rows_per_wave"] > p["batch_rows"]
    _check_mul_mat(dev, oracle, 12, K, N, 8, 11)


def test_two_row_batches_short_rows(dev, oracle):
    """Three superblocks a row: a step's superblocks fall into two chain batches (both record buffers)."""
    _check_mul_mat(dev, oracle, 13, 768, _smallest_n_with_two_batches(768, 3, 13) + 70, 3, 13)


@pytest.mark.parametrize("types", [(12, 12, 12), (12, 12, 14)])
def test_backend_three_matrices_one_launch(dev, oracle, types):
    _backend_case(oracle, list(zip(types, (512, 128, 128))), 512, 5, add=False)


def test_backend_mul_mat_add(dev, oracle):
    _backend_case(oracle, [(12, 512)], 512, 3, add=True)


def _backend_case(oracle, specs, K, M, add):
    import ggml_mi355x as g
    rng = np.random.default_rng(len(specs) * 10 + M)
    be = g.Backend(0)
    ws = [kquant(rng, ty, n, K, edges=True) for ty, n in specs]
    x = _x(rng, M, K)

    def up(a):
        p = be.alloc(a.nbytes)
        be.set_tensor(p, a)
        return p

    xt = g.make_tensor(g.TYPE_F32, K, M, up(x))
    nodes = [g.make_tensor(g.TYPE_F32, n, M, be.alloc(n * M * 4), op=g.OP_MUL_MAT,
                           src0=g.make_tensor(ty, K, n, up(w)), src1=xt) for (ty, n), w in zip(specs, ws)]
    refs = [oracle.mul_mat(ty, w, x) for (ty, n), w in zip(specs, ws)]
    if add:
        r = rng.standard_normal((M, specs[0][1])).astype(np.float32)
        rt = g.make_tensor(g.TYPE_F32, specs[0][1], M, up(r))
        nodes.append(g.make_tensor(g.TYPE_F32, specs[0][1], M, be.alloc(r.nbytes), op=g.OP_ADD, src0=nodes[0], src1=rt))
        outs, refs = [nodes[1]], [refs[0] + r]
    else:
        outs = nodes
    rc, names = _timed(lambda: be.graph_compute(nodes, use_graph=0))
    assert rc == 0
    _one_cols_launch(names)
    for o, ref in zip(outs, refs):
        h = np.zeros(ref.shape, np.float32)
        be.get_tensor(h, o.data)
        be.synchronize()
        assert bits_equal(h, ref), first_mismatch(h, ref)
    be.close()
