"""Decode attention, the forms of the per-head body (kq_attn_head.h) that the other attention
tests leave out: a head count that is no multiple of 8 on the output split (the plain head
order with more than one slice per head), the per-head kernel where soft_max's group sums move
behind the scalars (past 2048 cells at head_dim 64, past 4096 at 128), and a position outside
the cache on every one of these kernels. Same oracle and bar as tests/test_gpu_ops.py:
bit-exact output at every position, both caches equal afterwards.

Each case first asserts mi355x_attn_path under its selector, so it says which kernel it ran.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


# (hd, nh, nkv, n_ctx, selector, expected path, rope_row)
CASES = [
    # the output split with 4 heads: the plain head order with DS > 1
    (64, 4, 2, 288, "SPLIT", "SPLIT4", True),    # 2 chunks of 256 cells
    (64, 4, 2, 288, "SPLIT", "SPLIT4", False),
    (128, 4, 2, 288, "SPLIT", "SPLIT4", True),   # 3 chunks of 128 cells: a ring slot is reused
    (128, 4, 2, 288, "SPLIT", "SPLIT4", False),
    (64, 4, 2, 2400, "SPLIT", "SPLIT8", True),   # no multiple of 64 (not the cells split); 10 chunks
    (128, 4, 2, 1312, "SPLIT", "SPLIT8", True),
    # one workgroup per head past 256 cells: K rows 2 / 1 per round, batched KQV
    (64, 4, 2, 288, "HEAD", "HEAD_BATCH", True),
    (128, 4, 2, 288, "HEAD", "HEAD_BATCH", True),
    (64, 4, 2, 2080, "HEAD", "HEAD_BATCH", True),   # gsum behind scal (n_ctx > 2048 at head_dim 64)
    (128, 4, 2, 4128, "HEAD", "HEAD_BATCH", True),  # ... (n_ctx > 4096 at head_dim 128)
    # the register path as kq_attn_decode<HD, false>
    (64, 4, 2, 256, "SPLIT", "HEAD", True),
    (128, 4, 2, 96, "SPLIT", "HEAD", True),
]


@pytest.mark.parametrize("hd,nh,nkv,n_ctx,sel,path,rope_row", CASES,
                         ids=[f"hd{c[0]}-ctx{c[3]}-{c[4].lower()}-{c[5].lower()}-{'row' if c[6] else 'table'}"
                              for c in CASES])
def test_attn_decode_forms(dev, O, hd, nh, nkv, n_ctx, sel, path, rope_row):
    """Every cell of both caches random; positions across the whole cache bit-exact with the
    oracle, both caches equal afterwards; then positions n_ctx and -1: all-NaN output, caches
    untouched."""
    import torch
    import ggml_mi355x as g
    prev = g.attn_impl(getattr(g, "ATTN_" + sel))
    try:
        assert g.attn_path(n_ctx, nh, nkv, hd) == getattr(g, "ATTN_PATH_" + path)
        rng = np.random.default_rng(7 * n_ctx + hd + int(rope_row))
        kvw = nkv * hd
        tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
        tref = O.rope_table(n_ctx, hd, 10000.0)
        kc_ref = rng.standard_normal((n_ctx, kvw)).astype(np.float16).view(np.uint16)
        vc_ref = rng.standard_normal((kvw, n_ctx)).astype(np.float16).view(np.uint16)
        kc = torch.from_numpy(kc_ref.view(np.int16).copy()).to(dev)
        vc = torch.from_numpy(vc_ref.view(np.int16).copy()).to(dev)
        scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
        for p in sorted(x for x in {0, 31, 32, 255, 256, 257, n_ctx // 2 + 7, n_ctx - 9, n_ctx - 1} if x < n_ctx):
            q = (rng.standard_normal(nh * hd) * 2).astype(np.float32)
            k = (rng.standard_normal(kvw) * 2).astype(np.float32)
            v = rng.standard_normal(kvw).astype(np.float32)
            pos = torch.tensor([p], dtype=torch.int32, device=dev)
            got = g.attn_decode(t(q, dev), t(k, dev), t(v, dev), pos, tab[p].contiguous() if rope_row else tab, kc, vc,
                                nh, nkv, hd, scale, rope_row=rope_row).cpu().numpy()
            ref = O.attn_decode(O.rope(q, hd, hd, p, tref), O.rope(k, hd, hd, p, tref), v, kc_ref, vc_ref, p, nh, nkv,
                                hd, scale)
            assert bits_equal(got, ref), (p, first_mismatch(got, ref))
        assert (kc.cpu().numpy().view(np.uint16) == kc_ref).all()
        assert (vc.cpu().numpy().view(np.uint16) == vc_ref).all()
        # a position outside the cache: NaN, caches untouched
        x = torch.ones(nh * hd, device=dev)
        for p in (n_ctx, -1):
            out = g.attn_decode(x, x[:kvw], x[:kvw], torch.tensor([p], dtype=torch.int32, device=dev),
                                tab[0].contiguous() if rope_row else tab, kc, vc, nh, nkv, hd, scale, rope_row=rope_row)
            assert torch.isnan(out).all(), p
            assert (kc.cpu().numpy().view(np.uint16) == kc_ref).all(), p
            assert (vc.cpu().numpy().view(np.uint16) == vc_ref).all(), p
    finally:
        g.attn_impl(prev)
