"""mi355x_mul_mat_id and mi355x_moe_combine on the device against tests/moe_ref.py, by bits: every type,
K of 1, 2 and 9 superblocks (uneven over a pass), N of a partial wave, a partial workgroup and several
workgroups, broadcast and per-slot activations, the id patterns a launch can bake wrongly, a Q6_K expert
tensor whose experts are not 16-byte aligned, an id outside the table (NaN rows, exact neighbours), the
output guard. Weights and activations are the scale edges of tests/test_gpu_block_edges.py."""
import numpy as np
import pytest
import torch

import ggml_mi355x as g
from oracle import kq_oracle_np as N
from tests import moe_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NE, NU = 4, 2
TYPES = [g.TYPE_Q4_K, g.TYPE_Q5_K, g.TYPE_Q6_K]
F32 = np.float32
GUARD = F32(-12345.0)
_cache = {}


def _experts(typ, K, Nr):
    key = (typ, K, Nr)
    if key not in _cache:
        rng = np.random.default_rng([typ, K, Nr])
        _cache[key] = np.stack([N.edge_blocks(rng, typ, Nr, K) for _ in range(NE)])
    return _cache[key]


def _ids(pattern, T):
    if pattern == "first_last":   # the first and the last expert
        return np.array([[0, NE - 1], [NE - 1, 0], [0, NE - 1]][:T], np.int32)
    if pattern == "same_every_token":
        return np.array([[2, 1]] * T, np.int32)
    return np.array([[1, 1], [3, 3], [0, 0]][:T], np.int32)  # the same expert twice in one token


def _run(typ, ex_host, ex_dev, K, x, ids, ne11):
    T = ids.shape[0]
    Nr = ex_host.shape[1]
    rec = torch.zeros((T, 2 * NU), dtype=torch.int32, device=DEV)
    rec[:, :NU] = torch.from_numpy(ids).to(DEV)
    out = torch.full((T * NU * Nr + 64,), float(GUARD), dtype=torch.float32, device=DEV)
    y = g.mul_mat_id(typ, ex_dev, K, torch.from_numpy(x).to(DEV), rec, NU, out=out[:T * NU * Nr].view(T, NU, Nr))
    torch.cuda.synchronize()
    assert (out[T * NU * Nr:].cpu().numpy() == GUARD).all()
    return y.cpu().numpy()


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("K", [256, 512, 2304])
@pytest.mark.parametrize("Nr", [8, 20, 264])
def test_mul_mat_id_matches_the_rule(typ, K, Nr):
    ex = _experts(typ, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    rng = np.random.default_rng([K, Nr])
    for T, ne11, pattern in ((1, 1, "first_last"), (3, 1, "same_every_token"), (3, NU, "first_last"),
                             (1, NU, "twice"), (3, NU, "twice"), (3, 1, "twice")):
        x = N.edge_activations(rng, T * ne11, K, first=T + ne11).reshape(T, ne11, K)
        ids = _ids(pattern, T)
        got = _run(typ, ex, exd, K, x, ids, ne11)
        want = M.mul_mat_id(typ, ex, x, ids)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (T, ne11, pattern, np.argwhere(~same)[:4])


def _rolled_experts(typ, K, Nr):
    """NE experts of Nr rows from one edge_blocks matrix, expert e its rows rolled by 13 e (every expert other
    bytes at a given row, every scale category in each)."""
    key = ("rolled", typ, K, Nr)
    if key not in _cache:
        base = N.edge_blocks(np.random.default_rng([typ, K, Nr, 1]), typ, Nr, K)
        _cache[key] = np.stack([np.roll(base, 13 * e, axis=0) for e in range(NE)])
    return _cache[key]


def _kernels(fn):
    g.timing_enable(True)
    fn()
    names = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    return names


@pytest.mark.parametrize("typ", TYPES)
def test_eight_rows_a_wave(typ):
    """ceil(N / 32) * pairs >= 512: the launch takes kq_gemv_id<TYPE, 8> (the form of a decode token's up /
    gate at Mixtral's shapes); N 2750 leaves the last workgroup 2 rows short of a wave's batch of 4."""
    K, Nr, T = 512, 2750, 3
    assert (Nr + 31) // 32 * T * NU >= 512
    ex = _rolled_experts(typ, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    rng = np.random.default_rng(8)
    for ne11 in (1, NU):
        x = N.edge_activations(rng, T * ne11, K, first=ne11).reshape(T, ne11, K)
        ids = np.array([[0, NE - 1], [2, 2], [1, 0]], np.int32)
        got = _run(typ, ex, exd, K, x, ids, ne11)
        want = M.mul_mat_id(typ, ex, x, ids)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (ne11, np.argwhere(~same)[:4])
    rec = torch.zeros((T, 2 * NU), dtype=torch.int32, device=DEV)
    xd = torch.zeros((T, 1, K), dtype=torch.float32, device=DEV)
    names = _kernels(lambda: g.mul_mat_id(typ, exd, K, xd, rec, NU))
    assert len(names) == 1 and names[0].endswith(", 8>"), names
    small = torch.from_numpy(_experts(typ, K, 264)).to(DEV)
    names = _kernels(lambda: g.mul_mat_id(typ, small, K, xd, rec, NU))
    assert len(names) == 1 and names[0].endswith(", 4>"), names


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("K", [4352, 14336])
def test_rows_of_more_than_sixteen_superblocks(typ, K):
    """K 4352 (17 superblocks) and 14336 (56, Mixtral's down): the prologue quantizes in more than one pass
    of 16 superblocks and a quad walks more than one superblock of a row."""
    Nr, T = 20, 3
    ex = _experts(typ, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    rng = np.random.default_rng([K, 9])
    for ne11 in (1, NU):
        x = N.edge_activations(rng, T * ne11, K, first=1).reshape(T, ne11, K)
        ids = np.array([[3, 0], [1, 1], [0, 2]], np.int32)
        got = _run(typ, ex, exd, K, x, ids, ne11)
        want = M.mul_mat_id(typ, ex, x, ids)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (ne11, np.argwhere(~same)[:4])


def test_q6k_experts_off_the_16_byte_grid():
    """nb02 not a multiple of 16 (two pad bytes behind every expert) and a base 2 bytes off: no expert
    starts on a 16-byte boundary, and the 210-byte blocks fall on every even offset within 16 bytes."""
    K, Nr = 512, 20
    ex = _experts(g.TYPE_Q6_K, K, Nr)
    rb = ex.shape[2]
    nb02 = Nr * rb + 2
    assert nb02 % 16 and rb % 16
    buf = torch.zeros(2 + NE * nb02 + 64, dtype=torch.uint8, device=DEV)
    exd = torch.as_strided(buf, (NE, Nr, rb), (nb02, rb, 1), 2)
    exd.copy_(torch.from_numpy(ex).to(DEV))
    assert exd.data_ptr() % 16 == 2 and all((exd.data_ptr() + e * nb02) % 16 for e in range(NE))
    rng = np.random.default_rng(5)
    for ne11 in (1, NU):
        x = N.edge_activations(rng, 3 * ne11, K).reshape(3, ne11, K)
        ids = np.array([[0, 3], [1, 2], [3, 1]], np.int32)
        got = _run(g.TYPE_Q6_K, ex, exd, K, x, ids, ne11)
        want = M.mul_mat_id(g.TYPE_Q6_K, ex, x, ids)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), np.argwhere(~same)[:4]


@pytest.mark.parametrize("typ", TYPES)
def test_id_outside_the_table_gives_nan_rows(typ):
    K, Nr = 512, 20
    ex = _experts(typ, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    x = N.edge_activations(np.random.default_rng(6), 3, K).reshape(3, 1, K)
    ids = np.array([[0, NE], [-1, 2], [3, 1 << 30]], np.int32)
    got = _run(typ, ex, exd, K, x, ids, 1)
    want = M.mul_mat_id(typ, ex, x, ids)
    for t, s in ((0, 1), (1, 0), (2, 1)):
        assert np.isnan(got[t, s]).all() and np.isnan(want[t, s]).all()
    for t, s in ((0, 0), (1, 1), (2, 0)):  # the neighbouring rows are exact
        same = (got[t, s].view(np.uint32) == want[t, s].view(np.uint32)) | (np.isnan(got[t, s]) & np.isnan(want[t, s]))
        assert same.all()


@pytest.mark.parametrize("n,n_used,T", [(256, 2, 1), (100, 1, 3), (1000, 8, 3), (257, 3, 2)])
def test_combine_matches_the_rule(n, n_used, T):
    rng = np.random.default_rng([n, n_used, T])
    ex = rng.standard_normal((T, n_used, n)).astype(F32)
    ex[0, 0, :3] = [1.0, 1.0 + 2.0 ** -12, 3.0]
    w = rng.uniform(0.05, 1.0, (T, n_used)).astype(F32)
    if n_used >= 3:  # (a + b) + c != a + (b + c)
        ex[0, :3, 0] = [1.0, 2.0 ** -24, 2.0 ** -24]
        w[0, :3] = 1.0
    stride = 2 * n_used + 2
    rec = torch.full((T, stride), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rec[:, n_used:2 * n_used] = torch.from_numpy(w.view(np.int32)).to(DEV)
    out = torch.full((T * n + 32,), float(GUARD), dtype=torch.float32, device=DEV)
    y = g.moe_combine(torch.from_numpy(ex).to(DEV), rec, n_used, out=out[:T * n].view(T, n))
    torch.cuda.synchronize()
    assert (out[T * n:].cpu().numpy() == GUARD).all()
    got = y.cpu().numpy()
    for t in range(T):
        want = M.combine(ex[t], w[t])
        assert (got[t].view(np.uint32) == want.view(np.uint32)).all(), t
