"""CPU: the rule of the f16 matrix-core prompt attention (tests/attn_f16_ref.py restates it from
include/ggml_mi355x.h): the float64 emulation on a hand-computed case, the float32 restatement of
kq_attn_prompt_f16's own operation order against the emulation within the recorded fraction of the
bound, and the bound's power to reject three wrong kernels. Neither side of these comparisons is the
code under test (tests/test_gpu_attn_prompt_f16.py holds the kernel to the same bound)."""
import math

import numpy as np
import pytest

from tests import attn_f16_ref as R

# max |restate_f32 - emulate| / bound over the grid below measured 0.186 (head_dim 64, 64 cells, N(0, 2)
# scores); the restatement is held to a quarter of the bound ("Prompt attention on the
# matrix cores")
FRACTION = 0.25
HEAD_DIMS = [64, 128]
CELLS = [1, 33, 64, 320, 4096]
QSCALES = [0.05, 2.0, 40.0]
NH, NKV = 2, 1


def inputs(hd, n_cells, qscale, seed):
    """One token at the last of n_cells cells of junk-free random caches (n_ctx: the next multiple of 32,
    so the cells after the position are there to be masked)."""
    rng = np.random.default_rng([hd, n_cells, int(qscale * 100), seed])
    n_ctx = (n_cells + 31) // 32 * 32
    kc = rng.standard_normal((n_ctx, NKV * hd), dtype=np.float32).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((NKV * hd, n_ctx), dtype=np.float32).astype(np.float16).view(np.uint16)
    q = R.qhat((rng.standard_normal(NH * hd) * qscale).astype(np.float32))
    return q, kc, vc, n_cells - 1


def ratio(got, q, kc, vc, pos, hd):
    sc = 1.0 / math.sqrt(hd)
    e, b = R.emulate(q, kc, vc, pos, NH, NKV, hd, sc), R.bound(q, kc, vc, pos, NH, NKV, hd, sc)
    assert (b > 0).all()
    return float(np.max(np.abs(got.astype(np.float64) - e) / b))


def test_emulate_hand_computed_two_cells():
    """q^ = (2, 0), K = (0, 1), (1, 7), scale 0.5: scores 0 and 1, weights e^-1 and 1; V rows (1, 3) and
    (-2, 4). Position 0 sees cell 0 alone; the third cell (junk) is never seen."""
    q = np.array([2.0, 0.0], np.float16)
    kc = np.array([[0, 1], [1, 7], [100, 100]], np.float16)
    vc = np.array([[1, 3, 1000], [-2, 4, -1000]], np.float16)
    w0 = math.exp(-1.0)
    want = np.array([(w0 * 1 + 3) / (w0 + 1), (w0 * -2 + 4) / (w0 + 1)])
    assert np.allclose(R.emulate(q, kc, vc, 1, 1, 1, 2, 0.5), want, rtol=1e-15, atol=0)
    assert np.array_equal(R.emulate(q, kc, vc, 0, 1, 1, 2, 0.5), np.array([1.0, -2.0]))
    assert np.array_equal(R.emulate(q, kc.view(np.uint16), vc.view(np.uint16), 1, 1, 1, 2, 0.5),
                          R.emulate(q, kc, vc, 1, 1, 1, 2, 0.5))  # bits or values


def test_bound_hand_computed_two_cells():
    q = np.array([2.0, 0.0], np.float16)
    kc = np.array([[0, 1], [1, 7]], np.float16)
    vc = np.array([[1, 3], [-2, 4]], np.float16)
    w0 = math.exp(-1.0)
    l = 1 + w0
    delta = 2.0 ** -23 * 2 * 0.5 * 2.0  # max_c sum |q K| = 2 (cell 1)
    eps = 2.0 ** -10 + 4 * delta
    wv = np.array([(w0 * 1 + 3) / l, (w0 * 2 + 4) / l])
    av = np.array([4 / l, 6 / l])
    want = eps * wv + 2.0 ** -24 * av + 2.0 ** -24 * 33 * wv
    assert np.allclose(R.bound(q, kc, vc, 1, 1, 1, 2, 0.5), want, rtol=1e-14, atol=0)


def test_perm_is_the_accumulator_fragment_order():
    """Element j of lane half hf at k-step s is accumulator register 8 s + j, whose row is
    (i & 3) + 8 (i >> 2) + 4 hf."""
    for s in range(2):
        for hf in range(2):
            for j in range(8):
                i = 8 * s + j
                assert R.PERM[16 * s + 8 * hf + j] == (i & 3) + 8 * (i >> 2) + 4 * hf
    assert sorted(R.PERM.tolist()) == list(range(32))
    assert all(R.HALF[(i & 3) + 8 * (i >> 2) + 4 * hf] == hf for i in range(16) for hf in range(2))


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("n_cells", CELLS)
@pytest.mark.parametrize("qscale", QSCALES)
def test_restatement_within_the_recorded_fraction(hd, n_cells, qscale):
    worst = 0.0
    for seed in range(8):
        q, kc, vc, pos = inputs(hd, n_cells, qscale, seed)
        got = R.restate_f32(q, kc, vc, pos, NH, NKV, hd, 1.0 / math.sqrt(hd))
        worst = max(worst, ratio(got, q, kc, vc, pos, hd))
    print("max |restate - emu| / B", worst)
    assert worst <= FRACTION


def test_restatement_ignores_the_cells_after_the_position():
    q, kc, vc, _ = inputs(64, 64, 2.0, 0)
    a = R.restate_f32(q, kc, vc, 40, NH, NKV, 64, 0.125)
    kc2, vc2 = kc.copy(), vc.copy()
    kc2[41:] = np.float16(60000.0).view(np.uint16)
    vc2[:, 41:] = np.float16(-60000.0).view(np.uint16)
    assert np.array_equal(a, R.restate_f32(q, kc2, vc2, 40, NH, NKV, 64, 0.125))
    assert np.array_equal(R.emulate(q, kc, vc, 40, NH, NKV, 64, 0.125), R.emulate(q, kc2, vc2, 40, NH, NKV, 64, 0.125))


# Positions of the discrimination runs: early ones (a peaked query's own cell is its largest score
# often enough that the off-by-one mask shows), the second and later tiles (the maximum can move)
MUT_POSITIONS = [1, 2, 3, 5, 33, 40, 63, 64, 95, 200, 319]


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("qscale", [2.0, 40.0], ids=["normal", "peaked"])
@pytest.mark.parametrize("mutate", ["mask", "rescale", "vorder"])
def test_bound_rejects_wrong_kernels(hd, qscale, mutate):
    """The mask off by one, no rescale when the maximum moves, V's cells in natural k order: each leaves
    the bound on the normal and on the peaked inputs (the correct restatement stays inside on the same
    inputs)."""
    worst_ok, worst_mut = 0.0, 0.0
    sc = 1.0 / math.sqrt(hd)
    for pos in MUT_POSITIONS:
        q, kc, vc, _ = inputs(hd, 320, qscale, pos)
        worst_ok = max(worst_ok, ratio(R.restate_f32(q, kc, vc, pos, NH, NKV, hd, sc), q, kc, vc, pos, hd))
        with np.errstate(all="ignore"):
            r = ratio(np.nan_to_num(R.restate_f32(q, kc, vc, pos, NH, NKV, hd, sc, mutate=mutate), nan=1e30), q, kc, vc,
                      pos, hd)
        worst_mut = max(worst_mut, r)
    print(mutate, "correct", worst_ok, "mutant", worst_mut)
    assert worst_ok <= FRACTION
    assert worst_mut > 1.0
