"""Kernel entry of the decode kernels: what a wave does between its first instruction and its
first memory request. kq_rows / kq_rows_dyn take their first-needed arguments
as leading plain parameters (preloaded into SGPRs), read the rest of their argument block in
one batch and pick per-matrix values by scalar selects; the host passes the grid size, the
waves per workgroup and the prologue's pass count. kq_attn_decode takes q / k / v / pos / the
rope table / the caches the same way and the rest of AttnArgs in one batch; kq_get_rows reads
its chunk's blocks as one 16-B load per thread into LDS.

Every case is bit-exact against the CPU oracle, run eagerly and through a captured graph
replayed twice (the replayed graph is the product path, and the one where the kernarg
preload has to hold from replay to replay). Shapes: K of 1, 2, 8 and 22 superblocks (one
prologue pass that not every wave joins, up to two passes at 6 waves per workgroup), row
counts below / at / above one row per lane (1, 3, 64, 65, 200: most waves own no rows, the
rows-per-wave split has a remainder), each type alone, two and three matrices of mixed types
(the matrix search and the picks), residual / rms_norm prologue / SWIGLU epilogue, a Q6_K
stream that starts off a 16-B boundary, and the claimed-row kernel.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

Q4, Q5, Q6 = 12, 13, 14
NS = (1, 3, 64, 65, 200)


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


def eager_and_replays(fn, outs, check):
    """fn() eagerly, then captured once and replayed twice; `outs` are poisoned before each
    run, so a launch that did not write shows; check(tag) asserts on the outputs."""
    import torch
    for o in outs:
        o.fill_(float("nan")) if o.is_floating_point() else o.zero_()
    fn()
    torch.cuda.synchronize()
    check("eager")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fn()
    for rep in (1, 2):
        for o in outs:
            o.fill_(float("nan")) if o.is_floating_point() else o.zero_()
        gr.replay()
        torch.cuda.synchronize()
        check(f"replay {rep}")


# ---------------------------------------------------------------- GEMV: one matrix
@pytest.mark.parametrize("K", [256, 512, 2048, 5632])
@pytest.mark.parametrize("type_", [Q4, Q5, Q6])
def test_mul_mat_one_matrix(dev, oracle, npo, type_, K):
    """mi355x_mul_mat, M = 1: the leading parameters alone describe the launch."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(K + type_)
    x = rng.standard_normal((1, K)).astype(np.float32)
    xd = t(x, dev)
    for N in NS:
        w = npo.random_blocks(rng, type_, N, K)
        ref = oracle.mul_mat(type_, w, x)
        wd, y = t(w, dev), torch.empty((1, N), device=dev)

        def check(tag):
            got = y.cpu().numpy()
            assert bits_equal(got, ref), (N, tag, first_mismatch(got, ref))
        eager_and_replays(lambda: g.mul_mat(type_, wd, K, xd, out=y), [y], check)


def test_mul_mat_unaligned_q6_stream(dev, oracle, npo):
    """A weight slice that starts at an odd Q6_K row: the stream base is 4-B but not 16-B
    aligned (K = 512: rows of 420 B; K = 5632: 4620 B), with and without a residual."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(6)
    for K, first in ((512, 1), (512, 3), (5632, 1)):
        N = 65
        w = npo.random_blocks(rng, Q6, N + first, K)
        x = rng.standard_normal((1, K)).astype(np.float32)
        res = rng.standard_normal(N).astype(np.float32)
        wd = t(w, dev)[first:]
        assert wd.data_ptr() % 16 != 0 and wd.data_ptr() % 4 == 0
        mm = oracle.mul_mat(Q6, w[first:], x)
        xd, rd = t(x, dev), t(res, dev)
        y, y2 = torch.empty((1, N), device=dev), torch.empty(N, device=dev)

        def run():
            g.mul_mat(Q6, wd, K, xd, out=y)
            g.gemv_fused_ext([(Q6, wd, y2)], xd[0], residual=[rd])

        def check(tag):
            assert bits_equal(y.cpu().numpy(), mm), (K, first, tag)
            assert bits_equal(y2.cpu().numpy(), (mm[0] + res).astype(np.float32)), (K, first, tag, "residual")
        eager_and_replays(run, [y, y2], check)


# ---------------------------------------------------------------- GEMV: fused matrices
FUSED = [((Q4, 65), (Q6, 200)), ((Q6, 3), (Q4, 64)), ((Q4, 200), (Q4, 64), (Q6, 65)), ((Q5, 1), (Q6, 3), (Q4, 200)),
         ((Q4, 64), (Q4, 64), (Q4, 64))]


@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("mats", FUSED, ids=lambda m: "+".join(f"{ty}x{n}" for ty, n in m))
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_gemv_fused_matrices(dev, oracle, npo, mats, K, residual):
    """Two and three matrices in one launch, mixed types (the type is the wave's matrix's)
    and one type (the type is the kernel's): every wave finds its matrix, its rows, its
    weights, its residual and its output among the loaded tables."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(K + len(mats) + sum(n for _, n in mats))
    x = rng.standard_normal(K).astype(np.float32)
    ws = [npo.random_blocks(rng, ty, n, K) for ty, n in mats]
    res = [rng.standard_normal(n).astype(np.float32) for _, n in mats]
    refs = [oracle.mul_mat(ty, w, x[None])[0] for (ty, _), w in zip(mats, ws)]
    if residual:  # the middle matrix without one: the pick of a null pointer
        res[1] = None
        refs = [r if s is None else (r + s).astype(np.float32) for r, s in zip(refs, res)]
    xd, wds = t(x, dev), [t(w, dev) for w in ws]
    rds = [None if s is None else t(s, dev) for s in res]
    ys = [torch.empty(n, device=dev) for _, n in mats]
    descs = [(ty, wd, y) for (ty, _), wd, y in zip(mats, wds, ys)]

    def run():
        if residual:
            g.gemv_fused_ext(descs, xd, residual=rds)
        else:
            g.gemv_fused(descs, xd)

    def check(tag):
        for i, (y, ref) in enumerate(zip(ys, refs)):
            got = y.cpu().numpy()
            assert bits_equal(got, ref), (i, tag, first_mismatch(got, ref))
    eager_and_replays(run, ys, check)


@pytest.mark.parametrize("mats,K", [(((Q4, 200), (Q4, 64), (Q6, 64)), 2048), (((Q4, 65),), 512), (((Q6, 200), (Q6, 200)), 256)],
                         ids=["qkv", "one", "pair"])
def test_gemv_norm_prologue(dev, O, oracle, npo, mats, K):
    """RMS_NORM -> MUL -> MUL_MATs (+ residual) in one launch: x and the norm weight are the
    leading parameters, eps comes with the batch."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(K)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    xin = O.mul(O.rms_norm(x, 1e-5), nw)
    ws = [npo.random_blocks(rng, ty, n, K) for ty, n in mats]
    res = [rng.standard_normal(n).astype(np.float32) for _, n in mats]
    refs = [O.add(oracle.mul_mat(ty, w, xin[None])[0], r) for (ty, _), w, r in zip(mats, ws, res)]
    xd, nwd = t(x, dev), t(nw, dev)
    ys = [torch.empty(n, device=dev) for _, n in mats]
    descs = [(ty, t(w, dev), y) for (ty, _), w, y in zip(mats, ws, ys)]
    rds = [t(r, dev) for r in res]

    def check(tag):
        for i, (y, ref) in enumerate(zip(ys, refs)):
            got = y.cpu().numpy()
            assert bits_equal(got, ref), (i, tag, first_mismatch(got, ref))
    eager_and_replays(lambda: g.gemv_fused_ext(descs, xd, prologue=g.PRO_RMS_NORM, x2=nwd, eps=1e-5, residual=rds),
                      ys, check)


@pytest.mark.parametrize("n", [5632, 200])
def test_gemv_swiglu_epilogue_and_prologue(dev, O, oracle, npo, n):
    """gate / up with the SWIGLU epilogue (paired waves at the real shape, staged at 200 rows),
    then down with the SWIGLU prologue and the residual (K = n where it is whole superblocks)."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(n)
    K = 2048
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    ws = [npo.random_blocks(rng, Q4, n, K) for _ in range(2)]
    xin = O.mul(O.rms_norm(x, 1e-5), nw)
    refs = [oracle.mul_mat(Q4, w, xin[None])[0] for w in ws]
    href = O.swiglu(refs[0], refs[1])
    ys = [torch.empty(n, device=dev) for _ in range(2)]
    h = torch.empty(n, device=dev)
    xd, nwd = t(x, dev), t(nw, dev)
    descs = [(Q4, t(w, dev), y) for w, y in zip(ws, ys)]
    outs, down = ys + [h], None
    if n % 256 == 0:  # down: SWIGLU prologue over gate / up, Q6_K, residual
        wdn = npo.random_blocks(rng, Q6, 65, n)
        r = rng.standard_normal(65).astype(np.float32)
        dref = O.add(oracle.mul_mat(Q6, wdn, href[None])[0], r)
        yd = torch.empty(65, device=dev)
        down = ([(Q6, t(wdn, dev), yd)], t(r, dev), dref, yd)
        outs = outs + [yd]

    def run():
        g.gemv_fused_ext(descs, xd, prologue=g.PRO_RMS_NORM, x2=nwd, eps=1e-5, epi_y=h)
        if down:
            g.gemv_fused_ext(down[0], ys[0], prologue=g.PRO_SWIGLU, x2=ys[1], residual=[down[1]])

    def check(tag):
        for y, ref in zip(ys, refs):
            assert bits_equal(y.cpu().numpy(), ref), tag
        assert bits_equal(h.cpu().numpy(), href), (tag, first_mismatch(h.cpu().numpy(), href))
        if down:
            assert bits_equal(down[3].cpu().numpy(), down[2]), (tag, first_mismatch(down[3].cpu().numpy(), down[2]))
    eager_and_replays(run, outs, check)


@pytest.mark.parametrize("type_,n_mat", [(Q6, 1), (Q4, 2), (Q5, 3)])
def test_claimed_rows_kernel(dev, O, oracle, npo, type_, n_mat):
    """kq_rows_dyn (forced on a small shape; the product takes it for the Q6_K heads): the same
    entry, every matrix's pointers kept for the whole launch."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(n_mat)
    K, N = 2048, 1000
    x = rng.standard_normal(K).astype(np.float32)
    ws = [npo.random_blocks(rng, type_, N, K) for _ in range(n_mat)]
    res = [rng.standard_normal(N).astype(np.float32) for _ in range(n_mat)]
    refs = [O.add(oracle.mul_mat(type_, w, x[None])[0], r) for w, r in zip(ws, res)]
    ys = [torch.empty(N, device=dev) for _ in range(n_mat)]
    descs = [(type_, t(w, dev), y) for w, y in zip(ws, ys)]
    xd, rds = t(x, dev), [t(r, dev) for r in res]
    prev = g.gemv_impl(g.GEMV_DYN)
    try:
        g.timing_enable(True)
        g.gemv_fused_ext(descs, xd, residual=rds)
        names = [r[0] for r in g.timing_read()]
        g.timing_enable(False)
        assert any("kq_rows_dyn" in n for n in names), names

        def check(tag):
            for i, (y, ref) in enumerate(zip(ys, refs)):
                got = y.cpu().numpy()
                assert bits_equal(got, ref), (i, tag, first_mismatch(got, ref))
        eager_and_replays(lambda: g.gemv_fused_ext(descs, xd, residual=rds), ys, check)
    finally:
        g.timing_enable(False)
        g.gemv_impl(prev)


def test_graph_compute_fusions(dev, O):
    """The backend's decode graph with its fusions (q/k/v with the norm prologue, o-proj with
    the residual, gate / up with the SWIGLU epilogue, down with the residual, the Q6_K head):
    one token computed eagerly, then the captured graph over three more tokens."""
    import torch
    import ggml_mi355x as g
    from tests import llama_model as LM
    from ggml_mi355x.llama import LlamaDecoder, hparams
    hp = hparams(2048, 1, 32, 4, 5632, 1024)
    n_ctx = 64
    w = LM.build(hp, 5, mix="q4_k_m")
    b = g.Backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), n_ctx, fuse=True)
    model, cache = LM.oracle_model(hp, w, n_ctx)
    for p, tok in enumerate([0, 1023, 17, 500]):
        dec.step(tok, p, use_graph=p > 0)
        b.synchronize()
        ref, trace = O.decode_token(model, tok, p, cache)
        hid, got = dec.last_hidden.cpu().numpy(), dec.logits.cpu().numpy()
        assert bits_equal(hid, trace[-1]), (p, "hidden", first_mismatch(hid, trace[-1]))
        assert bits_equal(got, ref), (p, first_mismatch(got, ref))
    torch.cuda.synchronize()
    b.close()


# ---------------------------------------------------------------- attention
@pytest.mark.parametrize("hd,nh,nkv", [(64, 8, 2), (128, 8, 4)])
def test_attn_decode_positions(dev, O, hd, nh, nkv):
    """Decode attention at the first cell, around the 32-cell boundary and at the last cell of
    the cache, the position read on the device; then a position outside the cache: NaN
    outputs, both caches untouched."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(hd)
    n_ctx, kvw = 64, nkv * hd
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    tref = O.rope_table(n_ctx, hd, 10000.0)
    kc_ref = O.fp32_to_fp16(rng.standard_normal((n_ctx, kvw)).astype(np.float32)).reshape(n_ctx, kvw).astype(np.uint16)
    vc_ref = O.fp32_to_fp16(rng.standard_normal((kvw, n_ctx)).astype(np.float32)).reshape(kvw, n_ctx).astype(np.uint16)
    kc, vc = t(kc_ref.view(np.int16), dev), t(vc_ref.view(np.int16), dev)
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    q, k, v = (torch.empty(n, device=dev) for n in (nh * hd, kvw, kvw))
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(nh * hd, device=dev)

    def run():
        g.attn_decode(q, k, v, pos, tab, kc, vc, nh, nkv, hd, scale, out=out)
    for p in (0, 31, 32, 33, n_ctx - 1):
        qh = (rng.standard_normal(nh * hd) * 2).astype(np.float32)
        kh = (rng.standard_normal(kvw) * 2).astype(np.float32)
        vh = rng.standard_normal(kvw).astype(np.float32)
        q.copy_(t(qh, dev)), k.copy_(t(kh, dev)), v.copy_(t(vh, dev)), pos.fill_(p)
        ref = O.attn_decode(O.rope(qh, hd, hd, p, tref), O.rope(kh, hd, hd, p, tref), vh, kc_ref, vc_ref, p, nh, nkv,
                            hd, scale)

        def check(tag):
            got = out.cpu().numpy()
            assert bits_equal(got, ref), (p, tag, first_mismatch(got, ref))
            assert (kc.cpu().numpy().view(np.uint16) == kc_ref).all(), (p, tag, "k cache")
            assert (vc.cpu().numpy().view(np.uint16) == vc_ref).all(), (p, tag, "v cache")
        eager_and_replays(run, [out], check)
    pos.fill_(n_ctx)

    def check_bad(tag):
        assert torch.isnan(out).all(), tag
        assert (kc.cpu().numpy().view(np.uint16) == kc_ref).all(), (tag, "k cache")
        assert (vc.cpu().numpy().view(np.uint16) == vc_ref).all(), (tag, "v cache")
    eager_and_replays(run, [], check_bad)


# ---------------------------------------------------------------- get_rows
@pytest.mark.parametrize("K", [2048, 2304])
@pytest.mark.parametrize("type_", [Q4, Q6])
def test_get_rows_first_and_last(dev, O, npo, type_, K):
    """The embedding row of the first and of the last token id (V - 1). K = 2048: one whole
    chunk of 8 superblocks per workgroup; 2304: a second chunk of one block, and Q6_K rows
    (1890 B) that start off a 16-B boundary (the last id is odd)."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(type_)
    V = 300
    table = npo.random_blocks(rng, type_, V, K)
    td = t(table, dev)
    ids = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty((1, K), device=dev)
    for tok in (0, V - 1):
        ids.fill_(tok)
        ref = O.get_rows(type_, table, K, np.array([tok], np.int32))

        def check(tag):
            got = out.cpu().numpy()
            assert bits_equal(got, ref), (tok, tag, first_mismatch(got, ref))
        eager_and_replays(lambda: g.get_rows(type_, td, K, ids, out=out), [out], check)
