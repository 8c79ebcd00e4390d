"""The Q8L-row decode GEMV kernels (FUSEDQ = false: kq_quantize_q8L writes the activation's Q8L
row to the workspace, kq_rows<TM, false, 0> / kq_rows_dyn<TM, false, 0> copy it to LDS by DMA) on
small shapes. The product reaches them at K > 36864 only (tests/test_gpu_large.py); here the knob
GEMV_FQMAX = 0 forces them, and g.mul_mat's outputs are compared with the oracle's mul_mat on bits.

The activation starts one float off a 16-byte boundary: g.mul_mat sizes the workspace that the
Q8L row needs from mi355x_mul_mat_workspace_size, which is 0 for K <= 8192 unless the activation
is off that boundary, so with an aligned one no case below would get past MI355X_E_WORKSPACE. The
off-boundary activation takes the same two launches (asserted from the timing names).

K: 256 (nb = 1: several rows per step), 768 (nb = 3: rows straddle steps, the `while (io >= nb)`
advance runs), 4352 (nb = 17 > 16: the single-subtract advance). N: 1, 37, 300 (most waves without
rows, a short stream, several steps). Q4_K, Q5_K, Q6_K (210-byte blocks: streams off a 16-byte
boundary). Each on kq_rows and, with gemv_impl forced to GEMV_DYN, on kq_rows_dyn. For K > 256
one superblock of x is all zero.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

ROWS, DYN = 0, 3  # gemv_impl: by launch / kq_rows_dyn for every one-type launch
TMASK = {12: 1, 13: 2, 14: 4}
_cases = {}  # (ty, K, N) -> (w, x, ref): built once, shared by both kernels, never written


def case(oracle, npo, ty, K, N):
    key = (ty, K, N)
    if key not in _cases:
        rng = np.random.default_rng(100000 * ty + 10 * K + N)
        w = npo.random_blocks(rng, ty, N, K)
        x = rng.standard_normal(K).astype(np.float32)
        if K > 256:
            x[256:512] = 0.0  # an all-zero superblock
        _cases[key] = (w, x, oracle.mul_mat(ty, w, x[None])[0])
    return _cases[key]


@pytest.mark.parametrize("impl", [ROWS, DYN], ids=["rows", "dyn"])
@pytest.mark.parametrize("ty", [12, 13, 14], ids=["q4k", "q5k", "q6k"])
@pytest.mark.parametrize("N", [1, 37, 300])
@pytest.mark.parametrize("K", [256, 768, 4352])
def test_q8l_rows_small(dev, oracle, npo, K, N, ty, impl):
    import torch
    import ggml_mi355x as g
    w, x, ref = case(oracle, npo, ty, K, N)
    xd = torch.zeros(K + 1, dtype=torch.float32, device=dev)
    xd[1:] = torch.from_numpy(x)
    xin = xd[1:]
    assert xin.data_ptr() % 16 == 4
    wd = t(w, dev)
    prev = g.gemv_impl(impl)
    try:
        g.debug_knob("GEMV_FQMAX", 0)
        pl = g.rows_plan([(ty, N)], K, fusedq=False)
        assert pl["dyn"] == (impl == DYN) and pl["sh"] == 0, pl
        g.timing_enable(True)
        got = g.mul_mat(ty, wd, K, xin).cpu().numpy()[0]
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
        g.debug_knob("GEMV_FQMAX")  # back to the default
        g.gemv_impl(prev)
    kernel = ("kq::kq_rows_dyn<" if impl == DYN else "kq::kq_rows<") + f"{TMASK[ty]}, false, 0>"
    assert names == ["kq::kq_quantize_q8L", kernel], names
    assert bits_equal(got, ref), (K, N, ty, impl, first_mismatch(got, ref))
