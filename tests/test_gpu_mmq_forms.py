"""Prefill GEMM (kq_mmq / kq_mmq_mixed, ggml-neon-opt_amd/csrc/kq_mmq.hip), what the other prefill tests
leave out on the forced tiles (mi355x_mmq_impl 1-4: 64 x 64, 128 x 64, 128 x 128, 64 x 128): the tile
order over more than one group of eight row tiles, several matrices of one and of two types in one
launch on every tile with the KV-cache epilogue, and the ADD epilogue. Same oracle and bar as
tests/test_gpu_parity.py: every output on bits.

Each reference is computed once per module and shared by the selectors that check against it.
"""
import functools

import numpy as np
import pytest

from tests.attn_prompt_ref import rand_caches, ref_attn_prompt, scale_of
from tests.test_gpu_attn_prompt import cache_mismatch, check_rows
from tests.test_gpu_attn_stream import to_dev
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

Q4_K, Q5_K, Q6_K = 12, 13, 14
TILES = {0: "auto", 1: "tile64", 2: "tile128", 3: "tile128w", 4: "tile64w"}  # mi355x_mmq_impl
ROWS = {1: 64, 2: 128, 3: 128, 4: 64}   # weight rows per workgroup of the forced tiles
COLS = {1: 64, 2: 64, 3: 128, 4: 128}   # activation columns per workgroup


@pytest.fixture
def forced():
    """Sets mi355x_mmq_impl for the test and puts the previous selector back."""
    import ggml_mi355x as g
    prev = []

    def force(impl):
        prev.append(g.mmq_impl(impl))
    yield force
    if prev:
        g.mmq_impl(prev[0])


def launches(run):
    """The launch names of `run` (the timing hook)."""
    import ggml_mi355x as g
    g.timing_enable(True)
    try:
        run()
        return [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)


# ---------------------------------------------------------------- 1: tile order
ORDER_K, ORDER_N, ORDER_M = 768, 1030, 70


@functools.lru_cache(maxsize=None)
def order_case(type_):
    from oracle import kq_oracle, kq_oracle_np
    rng = np.random.default_rng(ORDER_K + 7 * ORDER_N + 13 * ORDER_M + type_)
    w = kq_oracle_np.random_blocks(rng, type_, ORDER_N, ORDER_K)
    x = rng.standard_normal((ORDER_M, ORDER_K)).astype(np.float32)
    x[1, 256:512] = 0.0  # an all-zero activation block (d = 0), the middle superblock
    return w, x, kq_oracle.mul_mat(type_, w, x)


@pytest.mark.parametrize("type_", [Q4_K, Q5_K, Q6_K], ids=["q4k", "q5k", "q6k"])
@pytest.mark.parametrize("impl", [1, 2, 3, 4], ids=[TILES[i] for i in (1, 2, 3, 4)])
def test_tile_order_and_buffer_parity(dev, forced, type_, impl):
    """K = 768: three superblocks, so the two LDS buffers alternate with an odd count. N = 1030: 9 row
    tiles of 128 rows (one full group of 8 that mmq_tile_of deals over the XCDs and an unremapped tail
    group of 1) or 17 of 64 rows (two groups and 1), the last row tile clamped to 6 rows. M = 70: a
    partial column tile at both widths."""
    import ggml_mi355x as g
    forced(impl)
    n_rt = -(-ORDER_N // ROWS[impl])
    assert n_rt % 8 == 1 and n_rt > 8 and ORDER_N % ROWS[impl] and ORDER_M % COLS[impl] and ORDER_K // 256 == 3
    w, x, ref = order_case(type_)
    wd, xd = t(w, dev), t(x, dev)
    out = []
    names = launches(lambda: out.append(g.mul_mat(type_, wd, ORDER_K, xd).cpu().numpy()))
    assert sum("kq_mmq<%d>" % type_ in n for n in names) == 1, names
    assert bits_equal(out[0], ref), first_mismatch(out[0], ref)


# ---------------------------------------------------------------- 2: several matrices in one launch
QKV_T, QKV_E, QKV_HD, QKV_NH, QKV_NKV, QKV_CTX = 37, 512, 64, 8, 2, 64
MIXES = [(Q4_K, Q4_K, Q4_K), (Q4_K, Q4_K, Q6_K), (Q5_K, Q5_K, Q6_K)]


@functools.lru_cache(maxsize=None)
def qkv_case(mix, edges=False):
    """q / k / v = MUL_MAT(w, x) on one activation, then the prompt attention: the oracle's mul_mat per
    matrix and tests/attn_prompt_ref.py (equal to decoding the tokens one by one, outputs and caches:
    tests/test_ops_oracle.py::test_prompt_reference_equals_sequential_decode). edges: the weights with the
    scale edges of tests/llama_model.py (tests/test_gpu_block_edges.py); off, those of every earlier run."""
    from oracle import kq_oracle, kq_ops_oracle
    from tests import llama_model as LM
    hd, nh, nkv, n_ctx, T, E = QKV_HD, QKV_NH, QKV_NKV, QKV_CTX, QKV_T, QKV_E
    rng = np.random.default_rng([QKV_T, QKV_E, *mix])
    ws = [LM.kquant(rng, mix[0], nh * hd, E, edges=edges), LM.kquant(rng, mix[1], nkv * hd, E, edges=edges),
          LM.kquant(rng, mix[2], nkv * hd, E, edges=edges)]
    x = rng.standard_normal((T, E)).astype(np.float32)
    pos = np.arange(20, 20 + T, dtype=np.int32)
    kc0, vc0 = rand_caches(rng, n_ctx, nkv * hd)
    refs = [kq_oracle.mul_mat(ty, w, x) for ty, w in zip(mix, ws)]
    kc_ref, vc_ref = kc0.copy(), vc0.copy()
    att_ref = ref_attn_prompt(kq_ops_oracle, refs[0], refs[1], refs[2], pos.tolist(), kc_ref, vc_ref,
                              kq_ops_oracle.rope_table(n_ctx, hd, 10000.0), nh, nkv, hd)
    return ws, x, pos, kc0, vc0, refs, att_ref, kc_ref, vc_ref


@pytest.mark.parametrize("mix", MIXES, ids=["q4k-q4k-q4k", "q4k-q4k-q6k", "q5k-q5k-q6k"])
@pytest.mark.parametrize("impl", [0, 1, 2, 3, 4], ids=[TILES[i] for i in range(5)])
def test_qkv_in_one_launch_on_every_tile(dev, forced, mix, impl):
    """q (512 rows), k and v (128 rows each) of 37 tokens at K = 512 as one launch: kq_mmq with three
    matrices, or kq_mmq_mixed where the types differ (each row tile its matrix's body; with a Q5_K matrix
    the 128 x 128 selector runs the 128 x 64 tile: kq_mmq_mixed<128, 2> has no Q5_K body, so on it the Q5_K
    row tiles would keep the 7.0 the outputs are filled with; the launch log carries no tile shape, the
    bits of q and k are what shows the fallback was taken). The launch stores the KV cells
    (no kq_kv_store). Eager and replayed, from junk caches each time: q, k, v, the attention rows and both
    caches on bits."""
    forced(impl)
    check_qkv_launch(dev, mix, qkv_case(mix))


def check_qkv_launch(dev, mix, case):
    """The body of test_qkv_in_one_launch_on_every_tile on one qkv_case, under the selector in force."""
    import torch
    import ggml_mi355x as g
    hd, nh, nkv, n_ctx, T, E = QKV_HD, QKV_NH, QKV_NKV, QKV_CTX, QKV_T, QKV_E
    ws, x, pos, kc0, vc0, refs, att_ref, kc_ref, vc_ref = case
    rows = [nh * hd, nkv * hd, nkv * hd]
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    wd = [t(w, dev) for w in ws]
    xd, posd = t(x, dev), t(pos, dev)
    kc, vc, kcj, vcj = to_dev(kc0, dev), to_dev(vc0, dev), to_dev(kc0, dev), to_dev(vc0, dev)
    outs = [torch.empty((T, n), dtype=torch.float32, device=dev) for n in rows]
    att = torch.empty((T, rows[0]), dtype=torch.float32, device=dev)
    F32 = g.TYPE_F32
    xt = g.make_tensor(F32, E, T, xd.data_ptr())
    wt = [g.make_tensor(ty, E, n, w.data_ptr()) for ty, n, w in zip(mix, rows, wd)]
    mm = [g.make_tensor(F32, n, T, o.data_ptr(), op=g.OP_MUL_MAT, src0=w_, src1=xt) for n, o, w_ in zip(rows, outs, wt)]
    post = g.make_tensor(g.TYPE_I32, T, 1, posd.data_ptr())
    kct = g.make_tensor(g.TYPE_F16, rows[1], n_ctx, kc.data_ptr())
    vct = g.make_tensor(g.TYPE_F16, n_ctx, rows[1], vc.data_ptr())
    tabt = g.make_tensor(F32, hd, n_ctx, tab.data_ptr())
    at = g.make_tensor(F32, rows[0], T, att.data_ptr(), op=g.OP_ATTN_DECODE, srcs=[mm[0], mm[1], mm[2], post, kct, vct, tabt],
                       op_params=[nh, nkv, hd, g.f32_bits(scale_of(hd))])
    nodes = mm + [at]
    be = g.Backend()
    try:
        be.set_fusion(True)
        for pi, use_graph in enumerate((0, 1)):
            kc.copy_(kcj)
            vc.copy_(vcj)
            for o in outs + [att]:
                o.fill_(7.0)
            torch.cuda.synchronize()

            def run():
                assert be.graph_compute(nodes, use_graph=use_graph) == 0
                be.synchronize()
            if pi == 0:
                names = launches(run)
                mixed = len(set(mix)) > 1
                assert sum("kq_mmq_mixed" in n for n in names) == (1 if mixed else 0), names
                assert sum("kq_mmq<" in n for n in names) == (0 if mixed else 1), names
                assert not any("kq_kv_store" in n for n in names), names
            else:
                run()
            for name, o, ref in zip("qkv", outs, refs):
                got = o.cpu().numpy()
                assert bits_equal(got, ref), (pi, name, first_mismatch(got, ref))
            check_rows(att.cpu().numpy(), att_ref, pos.tolist(), n_ctx, ("pass", pi, "att"))
            assert cache_mismatch(kc, kc_ref) is None, ("k cache, pass", pi, cache_mismatch(kc, kc_ref))
            assert cache_mismatch(vc, vc_ref) is None, ("v cache, pass", pi, cache_mismatch(vc, vc_ref))
    finally:
        be.close()


# ---------------------------------------------------------------- 3: the ADD epilogue
RES_K, RES_N, RES_M = 512, 130, 33


@functools.lru_cache(maxsize=None)
def res_case(type_):
    from oracle import kq_oracle, kq_oracle_np, kq_ops_oracle
    rng = np.random.default_rng(RES_K + 7 * RES_N + 13 * RES_M + type_)
    w = kq_oracle_np.random_blocks(rng, type_, RES_N, RES_K)
    x = rng.standard_normal((RES_M, RES_K)).astype(np.float32)
    res = rng.standard_normal((RES_M, RES_N)).astype(np.float32)
    ref = kq_ops_oracle.add(kq_oracle.mul_mat(type_, w, x), res).reshape(RES_M, RES_N)
    return w, x, res, ref


@pytest.mark.parametrize("type_", [Q4_K, Q5_K, Q6_K], ids=["q4k", "q5k", "q6k"])
@pytest.mark.parametrize("impl", [1, 2, 3, 4], ids=[TILES[i] for i in (1, 2, 3, 4)])
def test_res_epilogue(dev, forced, type_, impl):
    """MUL_MAT followed by ADD (the residual) as one kq_mmq launch, no kq_binary: K = 512, N = 130 (a
    clamped last row tile at both heights), M = 33 (a partial column tile); the sum is the one f32 add of
    ggml_add on the oracle's mul_mat."""
    import torch
    import ggml_mi355x as g
    forced(impl)
    w, x, res, ref = res_case(type_)
    wd, xd, resd = t(w, dev), t(x, dev), t(res, dev)
    y = torch.full((RES_M, RES_N), 7.0, dtype=torch.float32, device=dev)
    s = torch.full((RES_M, RES_N), 7.0, dtype=torch.float32, device=dev)
    F32 = g.TYPE_F32
    xt = g.make_tensor(F32, RES_K, RES_M, xd.data_ptr())
    wt = g.make_tensor(type_, RES_K, RES_N, wd.data_ptr())
    rt = g.make_tensor(F32, RES_N, RES_M, resd.data_ptr())
    mm = g.make_tensor(F32, RES_N, RES_M, y.data_ptr(), op=g.OP_MUL_MAT, src0=wt, src1=xt)
    ad = g.make_tensor(F32, RES_N, RES_M, s.data_ptr(), op=g.OP_ADD, src0=mm, src1=rt)
    be = g.Backend()
    try:
        be.set_fusion(True)
        for pi, use_graph in enumerate((0, 1)):
            s.fill_(7.0)
            torch.cuda.synchronize()

            def run():
                assert be.graph_compute([mm, ad], use_graph=use_graph) == 0
                be.synchronize()
            if pi == 0:
                names = launches(run)
                assert sum("kq_mmq<%d>" % type_ in n for n in names) == 1, names
                assert not any("kq_binary" in n for n in names), names
            else:
                run()
            got = s.cpu().numpy()
            assert bits_equal(got, ref), (pi, first_mismatch(got, ref))
    finally:
        be.close()
