"""The expert-grouped form of mi355x_mul_mat_id (MOE_PREFILL_GROUPED: kq_moe_group, kq_quantize_q8L, kq_mmq_id)
against tests/moe_ref.mul_mat_id, by bits, and against the same call under MOE_PREFILL_GEMV (kq_gemv_id, a second
yardstick). Weights and activations are the scale edges of tests/test_gpu_block_edges.py. The shapes: every type;
K of one superblock and of three (both LDS buffers used again); N of 40 rows (a partial 64-row half of the tile)
and 136 (a second 128-row tile of 8 rows); 4 experts of which 2 are used; ne11 1 and n_used; 80 tokens (160 pairs)
routed so that the buckets hold 0 / 1 / 64 / 95 pairs (an empty expert, a one-column tile, an exactly full tile, a
full tile and a partial one), all on one expert, the same expert in both slots of a token, and one token. Then an
id outside the table, a Q6_K tensor off the 16-byte grid, the launches by name. The numpy rule runs on every
shape here (a fraction of a second each)."""
import contextlib

import numpy as np
import pytest
import torch

import ggml_mi355x as g
from oracle import kq_oracle_np as N
from tests import moe_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NE, NU, T = 4, 2, 80
TYPES = [g.TYPE_Q4_K, g.TYPE_Q5_K, g.TYPE_Q6_K]
F32 = np.float32
GUARD = F32(-12345.0)
_cache = {}


@contextlib.contextmanager
def _mode(impl):
    prev = g.moe_prefill(impl)
    try:
        yield
    finally:
        g.moe_prefill(prev)


def _experts(typ, K, Nr):
    key = (typ, K, Nr)
    if key not in _cache:
        rng = np.random.default_rng([typ, K, Nr, 7])
        _cache[key] = np.stack([N.edge_blocks(rng, typ, Nr, K) for _ in range(NE)])
    return _cache[key]


def _ids(pattern):
    if pattern == "0_1_64_95":  # pairs per expert; which pair goes where is shuffled
        flat = np.repeat(np.arange(NE, dtype=np.int32), [0, 1, 64, 95])
        assert flat.size == T * NU
        return np.random.default_rng(11).permutation(flat).reshape(T, NU)
    if pattern == "one_expert":
        return np.full((T, NU), 2, np.int32)
    if pattern == "twice":  # the same expert in both slots of a token
        return np.repeat((np.arange(T, dtype=np.int32) * 3 % NE)[:, None], NU, axis=1)
    assert pattern == "one_token"
    return np.array([[3, 0]], np.int32)


def _run(typ, ex_dev, Nr, K, x, ids):
    n_tok = ids.shape[0]
    rec = torch.full((n_tok, 2 * NU), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rec[:, :NU] = torch.from_numpy(ids).to(DEV)
    n = n_tok * NU * Nr
    out = torch.full((n + 64,), float(GUARD), dtype=torch.float32, device=DEV)
    y = g.mul_mat_id(typ, ex_dev, K, torch.from_numpy(x).to(DEV), rec, NU, out=out[:n].view(n_tok, NU, Nr))
    torch.cuda.synchronize()
    assert (out[n:].cpu().numpy() == GUARD).all()
    return y.cpu().numpy()


def _same(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _check(typ, ex, exd, K, x, ids, tag):
    Nr = ex.shape[1]
    with _mode(g.MOE_PREFILL_GROUPED):
        got = _run(typ, exd, Nr, K, x, ids)
    with _mode(g.MOE_PREFILL_GEMV):
        gemv = _run(typ, exd, Nr, K, x, ids)
    want = M.mul_mat_id(typ, ex, x, ids)
    same = _same(got, want)
    assert same.all(), (tag, "rule", int((~same).sum()), np.argwhere(~same)[:4])
    same = _same(got, gemv)
    assert same.all(), (tag, "gemv", int((~same).sum()), np.argwhere(~same)[:4])
    return got, want


@pytest.mark.parametrize("typ", TYPES)
@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("Nr", [40, 136])
def test_grouped_matches_the_rule_and_the_gemv_form(typ, K, Nr):
    ex = _experts(typ, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    rng = np.random.default_rng([K, Nr, 3])
    for pattern in ("0_1_64_95", "one_expert", "twice", "one_token"):
        ids = _ids(pattern)
        for ne11 in (1, NU):
            x = N.edge_activations(rng, ids.shape[0] * ne11, K, first=ne11).reshape(ids.shape[0], ne11, K)
            _check(typ, ex, exd, K, x, ids, (pattern, ne11))


@pytest.mark.parametrize("typ", TYPES)
def test_id_outside_the_table_gives_that_pair_a_nan_row(typ):
    K, Nr = 256, 40
    ex = _experts(typ, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    ids = _ids("0_1_64_95").copy()
    ids[37, 1] = NE
    x = N.edge_activations(np.random.default_rng(6), T, K).reshape(T, 1, K)
    got, want = _check(typ, ex, exd, K, x, ids, "outside")
    assert np.isnan(got[37, 1]).all() and np.isnan(want[37, 1]).all()
    assert np.isnan(got).sum() == np.isnan(want).sum()  # (the edge blocks make NaN of their own: the same ones)
    for bad in (-1, 1 << 30):  # negative and huge ids take the same bucket
        ids[37, 1] = bad
        with _mode(g.MOE_PREFILL_GROUPED):
            again = _run(typ, exd, Nr, K, x, ids)
        assert _same(again, got).all()


def test_q6k_experts_off_the_16_byte_grid():
    """A base 2 bytes off the grid and nb02 no multiple of 16: the tiles' 16-byte granules and the realignment in
    q6_superblock come from each expert's own address."""
    K, Nr = 768, 40
    ex = _experts(g.TYPE_Q6_K, K, Nr)
    rb = ex.shape[2]
    nb02 = Nr * rb + 2
    assert nb02 % 16
    buf = torch.zeros(2 + NE * nb02 + 64, dtype=torch.uint8, device=DEV)
    exd = torch.as_strided(buf, (NE, Nr, rb), (nb02, rb, 1), 2)
    exd.copy_(torch.from_numpy(ex).to(DEV))
    assert exd.data_ptr() % 16 == 2 and len({(exd.data_ptr() + e * nb02) % 16 for e in range(NE)}) == NE
    rng = np.random.default_rng(5)
    ids = _ids("0_1_64_95")
    ids[0] = [0, 1]  # every expert in use: 1 / 1 / 64 / 94
    for ne11 in (1, NU):
        x = N.edge_activations(rng, T * ne11, K).reshape(T, ne11, K)
        _check(g.TYPE_Q6_K, ex, exd, K, x, ids, ne11)


def test_q6k_takes_the_wide_tile_from_128_pairs_an_expert():
    """512 pairs on 4 Q6_K experts: the launch takes the 128 x 128 tile by itself (buckets of 3 / 130 / 128 / 251
    pairs: a partial tile, a full one and 2 columns, an exactly full one, a full and a partial one)."""
    K, Nr, n_tok = 256, 136, 256
    ex = _experts(g.TYPE_Q6_K, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    flat = np.repeat(np.arange(NE, dtype=np.int32), [3, 130, 128, 251])
    ids = np.random.default_rng(12).permutation(flat).reshape(n_tok, NU)
    for ne11 in (1, NU):
        x = N.edge_activations(np.random.default_rng(13), n_tok * ne11, K).reshape(n_tok, ne11, K)
        _check(g.TYPE_Q6_K, ex, exd, K, x, ids, ("wide", ne11))


@pytest.mark.parametrize("shape", [1, 2, 3])
def test_q6k_tile_shapes_of_the_knob(shape):
    """The shapes of kq_mmq_id on Q6_K experts forced by the MMQ_ID_Q6 knob (1 the 128 x 128 tile, 2 the 64 x 128
    one, both on the table's prefix of 128-column tiles; 3 the 128 x 64 one): the bits of the default launch."""
    K, Nr = 768, 136
    ex = _experts(g.TYPE_Q6_K, K, Nr)
    exd = torch.from_numpy(ex).to(DEV)
    ids = _ids("0_1_64_95").copy()
    ids[5, 0] = -1
    x = N.edge_activations(np.random.default_rng(9), T * NU, K).reshape(T, NU, K)
    with _mode(g.MOE_PREFILL_GROUPED):
        want = _run(g.TYPE_Q6_K, exd, Nr, K, x, ids)
        g.debug_knob("MMQ_ID_Q6", shape)
        try:
            got = _run(g.TYPE_Q6_K, exd, Nr, K, x, ids)
        finally:
            g.debug_knob("MMQ_ID_Q6")  # (NaN: back to the default)
    assert _same(got, want).all() and np.isnan(got[5, 0]).all()


def _kernels(fn):
    g.timing_enable(True)
    fn()
    names = [r[0] for r in g.timing_read()]
    g.timing_enable(False)
    return names


@pytest.mark.parametrize("typ", TYPES)
def test_launches_by_name(typ):
    K, Nr = 256, 40
    exd = torch.from_numpy(_experts(typ, K, Nr)).to(DEV)
    rec = torch.zeros((T, 2 * NU), dtype=torch.int32, device=DEV)
    xd = torch.zeros((T, 1, K), dtype=torch.float32, device=DEV)
    with _mode(g.MOE_PREFILL_GROUPED):
        names = _kernels(lambda: g.mul_mat_id(typ, exd, K, xd, rec, NU))
        assert len(names) == 3 and "kq_moe_group" in names[0] and "kq_quantize_q8L" in names[1] and \
            "kq_mmq_id" in names[2], names
        names = _kernels(lambda: g.mul_mat_id(typ, exd, K, xd[:1], rec[:1], NU))  # any T >= 1
        assert [n.split("<")[0] for n in names] == ["kq::kq_moe_group", "kq::kq_quantize_q8L", "kq::kq_mmq_id"], names
    with _mode(g.MOE_PREFILL_GEMV):
        names = _kernels(lambda: g.mul_mat_id(typ, exd, K, xd, rec, NU))
        assert len(names) == 1 and "kq_gemv_id" in names[0], names
    with _mode(g.MOE_PREFILL_AUTO):
        names = _kernels(lambda: g.mul_mat_id(typ, exd, K, xd[:3], rec[:3], NU))
        assert len(names) == 1 and "kq_gemv_id" in names[0], names
