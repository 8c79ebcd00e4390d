"""The decode GEMV's fused prologue (kq_rows.hip RowsPrologue, shared by kq_rows and
kq_rows_dyn): the bytes of the workgroup's Q8_K row, seen through mi355x_debug_rows_prologue.

The GEMV's outputs cannot show a wrong sign of a +-amax tie (d and every q of the block flip
together), so the quantizer's forms (16, 32 and 64 lanes per superblock, picked by the row and
the workgroup's waves: rows_pro_form) are checked on their bytes, bit-exact against the CPU
oracle's quantize_row_q8_K: every (K, waves) the entry accepts, the golden edge blocks, ties
placed inside one lane / across lanes of a 16-lane row / across 16-lane rows / at the ends of a
superblock, NaNs, and the rms_norm and SWIGLU transforms. Then GEMVs on both kernels at forced
6 and 12 waves, eager and replayed.

(K, waves) pairs a workgroup of that many waves cannot hold (more than 3 passes of 4
superblocks per wave: K > 3072 * waves) must be refused with E_UNSUPPORTED; plan_rows never
launches them (it takes 12 waves for such rows).
"""
import os

import numpy as np
import pytest

from tests.adversarial import _seq_sumsq, order_split_rows
from tests.test_gpu_entry import eager_and_replays
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

Q4, Q6 = 12, 14
KS = (256, 512, 1024, 2048, 5632, 8192, 14336)
WAVES = (1, 4, 6, 12)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "q8K_edges.npz")


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


def q8l_to_q8k(img):
    """[nb, 304] Q8L blocks (d @0, qs @16, bsums @272) -> [nb * 292] Q8_K bytes."""
    img = np.ascontiguousarray(img, np.uint8)
    out = np.empty((img.shape[0], 292), np.uint8)
    out[:, 0:4] = img[:, 0:4]
    out[:, 4:260] = img[:, 16:272]
    out[:, 260:292] = img[:, 272:304]
    return out.reshape(-1)


def supported(K, waves):
    return K // 256 <= 12 * waves


def run_prologue(g, dev, x, waves, **kw):
    kw = {k: (t(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return q8l_to_q8k(g.debug_rows_prologue(t(x, dev), waves, **kw).cpu().numpy())


def check_blocks(got, ref, what):
    ref = np.asarray(ref, np.uint8).reshape(-1)
    if not (got == ref).all():
        i = int(np.flatnonzero(got != ref)[0])
        b, o = divmod(i, 292)
        raise AssertionError((what, "block", b, "byte", o, "d" if o < 4 else "qs" if o < 260 else "bsums",
                              int(got[i]), int(ref[i])))


def tie_positions():
    """Pairs of positions in a superblock: inside one lane of every form (4, 8 and 16 values per
    lane), in two lanes of one 16-lane row (per form), in two 16-lane rows of a superblock on 32
    and on 64 lanes (neighbouring rows and the two halves of the wave), first and last element."""
    pairs = [(20, 21), (20, 23), (0, 255)]
    for vp in (16, 8, 4):
        pairs.append((vp * 1 + 1, vp * 9 + 2))
    pairs += [(8 * 3, 8 * 18 + 1), (4 * 5 + 1, 4 * 17 + 2), (4 * 17, 4 * 33 + 3), (4 * 2 + 3, 4 * 49)]
    return pairs


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("K", KS)
def test_prologue_bytes(dev, oracle, K, waves):
    import ggml_mi355x as g
    nb = K // 256
    rng = np.random.default_rng(K + waves)
    x0 = rng.standard_normal(K).astype(np.float32)
    if not supported(K, waves):
        assert g.rows_prologue_plan(K, waves) == g.E_UNSUPPORTED
        with pytest.raises(g.Mi355xError):
            g.debug_rows_prologue(t(x0, dev), waves)
        return
    lanes, passes = g.rows_prologue_plan(K, waves)
    assert nb * lanes <= 64 * waves * passes and (passes == 1 or lanes == 16)
    check_blocks(run_prologue(g, dev, x0, waves), oracle.quantize_q8_K(x0), "random")
    places = sorted({0, nb // 2, nb - 1})
    # the golden edge blocks, each in the first, a middle and the last superblock
    edges = np.load(GOLDEN)["x"]
    for r in range(len(edges)):
        x = x0.copy()
        for n, b in enumerate(places):
            x[256 * b: 256 * b + 256] = edges[(r + n) % len(edges)]
        check_blocks(run_prologue(g, dev, x, waves), oracle.quantize_q8_K(x), ("edge", r))
    # +-amax ties, both sign orders
    for p, q in tie_positions():
        for sgn in (1.0, -1.0):
            x = (x0 * 0.25).clip(-2.5, 2.5).astype(np.float32)
            for b in places:
                x[256 * b + p], x[256 * b + q] = 3.0 * sgn, -3.0 * sgn
            check_blocks(run_prologue(g, dev, x, waves), oracle.quantize_q8_K(x), ("tie", p, q, sgn))
    # NaNs beside finite values (amax ignores them), and an all-zero superblock
    x = x0.copy()
    for b in places:
        x[256 * b + np.array([0, 17, 100, 255])] = np.nan
    x[256 * (nb // 2): 256 * (nb // 2) + 256][5:9] = 0.0
    check_blocks(run_prologue(g, dev, x, waves), oracle.quantize_q8_K(x), "nan")
    x = x0.copy()
    x[256 * (nb - 1):] = 0.0
    check_blocks(run_prologue(g, dev, x, waves), oracle.quantize_q8_K(x), "zero block")


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("K", KS)
def test_prologue_norm_random(dev, oracle, O, K, waves):
    import ggml_mi355x as g
    if not supported(K, waves):
        return
    rng = np.random.default_rng(7 * K + waves)
    for rep in range(3):
        x = (rng.standard_normal(K) * 3).astype(np.float32)
        w = rng.uniform(0.5, 1.5, K).astype(np.float32)
        ref = oracle.quantize_q8_K(O.mul(O.rms_norm(x, 1e-5), w))
        check_blocks(run_prologue(g, dev, x, waves, prologue=g.PRO_RMS_NORM, x2=w, eps=1e-5), ref, ("norm", rep))


def fast_sumsq(x, vp):
    """Mirror of the prologue's fast order with vp values per lane: the lane's vp squares in
    order, a xor tree over the 256 / vp lanes of the superblock, superblocks in order."""
    x = np.asarray(x, np.float32)
    tot = 0.0
    for b in range(x.size // 256):
        n = 256 // vp
        s = []
        for l in range(n):
            a = 0.0
            for v in x[256 * b + vp * l: 256 * b + vp * l + vp]:
                a += float(np.float32(v) * np.float32(v))
            s.append(a)
        step = 1
        while step < n:
            s = [s[i] + s[i ^ step] for i in range(n)]
            step *= 2
        tot += s[0]
    return tot


@pytest.mark.parametrize("n", [1024, 2048, 8192])
def test_prologue_norm_order_split(dev, oracle, O, n):
    """Rows whose float mean differs between the sequential order and the prologue's fast order
    of every form: the match with the oracle shows that the sequential re-sum ran."""
    import ggml_mi355x as g
    rows, ms, _ = order_split_rows(n)
    w = np.random.default_rng(n).uniform(0.5, 1.5, n).astype(np.float32)
    for waves in WAVES:
        if not supported(n, waves):
            continue
        lanes, _ = g.rows_prologue_plan(n, waves)
        for r, row in enumerate(rows):
            fast = np.float32(fast_sumsq(row, 256 // lanes) / n)
            assert fast != ms[r] and ms[r] == np.float32(_seq_sumsq(row) / n), (waves, r, fast, ms[r])
            ref = oracle.quantize_q8_K(O.mul(O.rms_norm(row, 0.0), w))
            check_blocks(run_prologue(g, dev, row, waves, prologue=g.PRO_RMS_NORM, x2=w, eps=0.0), ref, (waves, r))


def test_prologue_swiglu(dev, oracle, O):
    import ggml_mi355x as g
    K = 5632
    rng = np.random.default_rng(K)
    gate = (rng.standard_normal(K) * 2).astype(np.float32)
    up = rng.standard_normal(K).astype(np.float32)
    ref = oracle.quantize_q8_K(O.swiglu(gate, up))
    for waves in (4, 6, 12):
        check_blocks(run_prologue(g, dev, gate, waves, prologue=g.PRO_SWIGLU, x2=up), ref, waves)


# ---------------------------------------------------------------- GEMVs on the new prologue
@pytest.fixture(params=[(0, 6), (0, 12), (3, 6), (3, 12)], ids=["rows6", "rows12", "dyn6", "dyn12"])
def kernel(request):
    import ggml_mi355x as g
    which, waves = request.param
    prev, prev_w = g.gemv_impl(which), g.gemv_waves(waves)
    yield request.param
    g.gemv_impl(prev)
    g.gemv_waves(prev_w)


def gemv_check(ys, refs):
    def check(tag):
        for i, (y, ref) in enumerate(zip(ys, refs)):
            got = y.cpu().numpy()
            assert bits_equal(got, ref), (i, tag, first_mismatch(got, ref))
    return check


@pytest.mark.parametrize("K", [512, 2048, 5632])
@pytest.mark.parametrize("mode", ["plain", "norm_residual"])
def test_gemv_forms(dev, oracle, npo, O, kernel, K, mode):
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(K + len(mode))
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    xin = O.mul(O.rms_norm(x, 1e-5), nw) if mode == "norm_residual" else x
    xd, nwd = t(x, dev), t(nw, dev)
    launches = [((ty, N),) for ty in (Q4, Q6) for N in (3, 65, 200)] + [((Q4, 200), (Q6, 65), (Q4, 3))]
    for mats in launches:
        ws = [npo.random_blocks(rng, ty, n, K) for ty, n in mats]
        res = [rng.standard_normal(n).astype(np.float32) for _, n in mats]
        refs = [oracle.mul_mat(ty, w, xin[None])[0] for (ty, _), w in zip(mats, ws)]
        ys = [torch.empty(n, device=dev) for _, n in mats]
        descs = [(ty, t(w, dev), y) for (ty, _), w, y in zip(mats, ws, ys)]
        if mode == "plain":
            run = lambda: g.gemv_fused(descs, xd)
        else:
            refs = [O.add(r, s) for r, s in zip(refs, res)]
            rds = [t(s, dev) for s in res]
            run = lambda: g.gemv_fused_ext(descs, xd, prologue=g.PRO_RMS_NORM, x2=nwd, eps=1e-5, residual=rds)
        eager_and_replays(run, ys, gemv_check(ys, refs))


@pytest.mark.parametrize("K", [512, 2048, 5632])
def test_gemv_swiglu_then_down(dev, oracle, npo, O, kernel, K):
    """gate / up (K rows each, from 512 inputs) with the SWIGLU epilogue, then down over the K
    gate / up values with the SWIGLU prologue: N rows of Q4_K and of Q6_K."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(K)
    Kin = 512
    x = (rng.standard_normal(Kin) * 3).astype(np.float32)
    wg, wu = (npo.random_blocks(rng, Q4, K, Kin) for _ in range(2))
    gr, ur = (oracle.mul_mat(Q4, w, x[None])[0] for w in (wg, wu))
    href = O.swiglu(gr, ur)
    xd = t(x, dev)
    yg, yu, h = (torch.empty(K, device=dev) for _ in range(3))
    gu = [(Q4, t(wg, dev), yg), (Q4, t(wu, dev), yu)]
    for ty in (Q4, Q6):
        for N in (3, 65, 200):
            wd = npo.random_blocks(rng, ty, N, K)
            dref = oracle.mul_mat(ty, wd, href[None])[0]
            yd = torch.empty(N, device=dev)
            down = [(ty, t(wd, dev), yd)]

            def run():
                g.gemv_fused_ext(gu, xd, epi_y=h)
                g.gemv_fused_ext(down, yg, prologue=g.PRO_SWIGLU, x2=yu)
            eager_and_replays(run, [yg, yu, h, yd], gemv_check([yg, yu, h, yd], [gr, ur, href, dref]))
