"""The sampler's rule as tests/sample_ref.py restates it (include/ggml_mi355x.h, mi355x_sample),
on the CPU: boundaries that are exact by construction (equal logits: every e and f is 1.0f, the
sums are small integers), the special values, and that the rule samples the distribution it
states. The kernel is checked against this reference in tests/test_gpu_sample.py."""
import numpy as np
import pytest

from tests import sample_ref as R

F = np.float32


@pytest.fixture(scope="module", autouse=True)
def oracle_lib(oracle):
    from oracle import kq_ops_oracle as O
    O.lib()


def equal_logits(n, k, value=1.5, seed=3):
    """n entries, k of them (at random places) equal to `value`, the rest far below."""
    rng = np.random.default_rng(seed)
    x = (-50.0 - np.abs(rng.standard_normal(n))).astype(np.float32)
    at = np.sort(rng.choice(n, k, replace=False))
    x[at] = value
    return x, at


def test_ref_topk_order():
    x = np.array([1.0, np.nan, 3.0, -0.0, 3.0, 0.0, -np.inf, np.inf], np.float32)
    assert R.ref_topk(x, 64).tolist() == [7, 2, 4, 0, 3, 5, 6]
    assert R.ref_topk(x, 3).tolist() == [7, 2, 4]
    assert R.ref_topk(np.full(5, np.nan, np.float32), 4).tolist() == []
    idx, val = R.ref_topk_out(x[:2], 3)
    assert idx.tolist() == [0, -1, -1] and val[0] == 1.0 and val.view(np.uint32)[1:].tolist() == [0x7fc00000] * 2
    rng = np.random.default_rng(0)
    y = rng.standard_normal(500).astype(np.float32)
    y[::3] = y[0]
    want = sorted(range(500), key=lambda i: (-float(y[i]), i))[:40]
    assert R.ref_topk(y, 40).tolist() == want
    assert R.ref_topk(y, 1)[0] == R.ref_argmax(y)


def test_eight_equal_logits_draw_boundaries():
    """F == 8 and the running sums are 1 .. 8: u = j / 8 gives r = j exactly, and the strict > picks c_j."""
    x, at = equal_logits(100, 8)
    tr = R.ref_trace(x, 0.0, top_k=8, top_p=1.0, min_p=0.0, temp=1.0)
    assert tr["c"].tolist() == at.tolist() and tr["F"] == 8 and tr["q"] == 8
    for j in range(8):
        assert R.ref_sample(x, j / 8, top_k=8, top_p=1.0, min_p=0.0, temp=1.0) == at[j]
        below = np.nextafter(F(j / 8), F(-1))
        if j:
            assert R.ref_sample(x, below, top_k=8, top_p=1.0, min_p=0.0, temp=1.0) == at[j - 1]


def test_four_equal_logits_top_p_half_keeps_two():
    x, at = equal_logits(64, 4)
    tr = R.ref_trace(x, 0.99, top_k=4, top_p=0.5, min_p=0.0, temp=1.0)
    assert tr["p"].tolist() == [0.25] * 4 and tr["qb"] == 2 and tr["q"] == 2 and tr["F"] == 2
    assert tr["token"] == at[1]
    assert R.ref_sample(x, 0.49, top_k=4, top_p=0.5, min_p=0.0, temp=1.0) == at[0]
    assert R.ref_trace(x, 0.0, top_k=4, top_p=np.nextafter(F(0.5), F(1)), min_p=0.0, temp=1.0)["q"] == 3


def test_min_p_just_above_and_below_an_e():
    x = np.full(16, -40.0, np.float32)
    x[3], x[9], x[12] = 2.0, 1.0, 0.0
    kw = dict(top_k=3, top_p=1.0, temp=1.0)
    e = R.ref_trace(x, 0.0, min_p=0.0, **kw)["e"]
    assert e[0] == 1 and e[1] > e[2] > 0
    # (kept with min_p == e_i, kept just below it, dropped just above it; e_2 < e_1 ends the prefix anyway)
    assert R.ref_trace(x, 0.0, min_p=e[1], **kw)["qa"] == 2
    assert R.ref_trace(x, 0.0, min_p=np.nextafter(e[1], F(0)), **kw)["qa"] == 2
    assert R.ref_trace(x, 0.0, min_p=np.nextafter(e[1], F(1)), **kw)["qa"] == 1
    assert R.ref_trace(x, 0.0, min_p=e[2], **kw)["qa"] == 3
    assert R.ref_trace(x, 0.0, min_p=np.nextafter(e[2], F(0)), **kw)["qa"] == 3
    assert R.ref_trace(x, 0.0, min_p=np.nextafter(e[2], F(1)), **kw)["qa"] == 2
    tr = R.ref_trace(x, 0.999, min_p=np.nextafter(e[2], F(1)), **kw)
    assert tr["q"] == 2 and tr["token"] == 9
    assert R.ref_trace(x, 0.999, min_p=1.0, **kw)["token"] == 3  # e_0 == 1 >= 1: never fewer than one


def test_temp_zero_and_top_k_one_are_argmax():
    rng = np.random.default_rng(5)
    for _ in range(8):
        x = rng.standard_normal(300).astype(np.float32)
        x[rng.integers(0, 300, 20)] = np.nan
        for u in (0.0, 0.5, 0.999):
            assert R.ref_sample(x, u, temp=0.0) == R.ref_argmax(x)
            assert R.ref_sample(x, u, top_k=1) == R.ref_argmax(x)
    assert R.ref_sample(np.full(7, np.nan, np.float32), 0.3) == 0


def test_neg_inf_candidate_is_never_drawn():
    """Two zeros among -inf entries, all eight kept: f is 1, 1, 0, ..., so every draw in [0, 1)
    lands on one of the two (r = 2 u exactly). Only the fallback of step 10 (u >= 1 or NaN)
    names c_{q-1}, whatever its f is."""
    x = np.full(8, -np.inf, np.float32)
    x[2], x[5] = 0.0, 0.0
    kw = dict(top_k=8, top_p=1.0, min_p=0.0, temp=1.0)
    for u in (0.0, 0.25, np.nextafter(F(0.5), F(0)), 0.5, 0.75, np.nextafter(F(1), F(0))):
        tr = R.ref_trace(x, u, **kw)
        assert tr["m"] == 8 and tr["q"] == 8 and tr["F"] == 2 and tr["f"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
        assert tr["token"] == (2 if u < 0.5 else 5), u
    assert R.ref_trace(x, 1.0, **kw)["token"] == 7


def test_non_finite_l0_gives_c0():
    x = np.array([1.0, np.inf, 2.0, np.inf], np.float32)
    assert R.ref_sample(x, 0.9, top_k=4, top_p=1.0, min_p=0.0, temp=1.0) == 1
    x = np.full(6, -np.inf, np.float32)
    assert R.ref_sample(x, 0.9, top_k=4, top_p=1.0, min_p=0.0, temp=1.0) == 0
    x[4] = np.nan
    x[0] = np.nan
    assert R.ref_sample(x, 0.9, top_k=4, top_p=1.0, min_p=0.0, temp=1.0) == 1


def test_u_one_and_nan_give_the_last_kept():
    x, at = equal_logits(50, 5)
    for u in (1.0, 2.0, np.nan):
        assert R.ref_sample(x, u, top_k=5, top_p=1.0, min_p=0.0, temp=1.0) == at[4]
        assert R.ref_sample(x, u, top_k=5, top_p=0.6, min_p=0.0, temp=1.0) == at[2]


def test_tiny_temp_has_no_inf_minus_inf():
    x = np.array([3.0, 1.0, 3.0, -2.0], np.float32)
    tr = R.ref_trace(x, 0.75, top_k=4, top_p=1.0, min_p=0.0, temp=1e-30)
    assert tr["f"].tolist() == [1.0, 1.0, 0.0, 0.0] and tr["token"] == 2


def test_the_rule_samples_the_distribution_it_states():
    """20000 PCG64 draws on one fixed 40-candidate vector: every kept candidate's frequency is
    within 4 sigma of its f_i / F (sigma of a binomial count; the rule is tested, not the kernel)."""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(400) * 2.0).astype(np.float32)
    kw = dict(top_k=40, top_p=0.95, min_p=0.05, temp=0.8)
    tr = R.ref_trace(x, 0.0, **kw)
    q, f = tr["q"], tr["f"].astype(np.float64)
    assert tr["m"] == 40 and 3 <= q <= 40
    prob = f[:q] / f[:q].sum()
    # the draw, vectorized: the rule's own running sums and r = u * F in float32
    run = R.seq_sums(tr["f"][:q])
    N = 20000
    u = R.draws(2024, N)
    r = (u * tr["F"]).astype(np.float32)
    k = np.minimum((run[None, :] > r[:, None]).argmax(axis=1), q - 1)
    k = np.where((run[None, :] > r[:, None]).any(axis=1), k, q - 1)
    for i in (0, 1, N // 2, N - 1):  # ... which is what ref_sample does draw by draw
        assert R.ref_sample(x, u[i], **kw) == tr["c"][k[i]]
    counts = np.bincount(k, minlength=q)
    sigma = np.sqrt(N * prob * (1 - prob))
    assert (np.abs(counts - N * prob) <= 4 * sigma).all(), (counts, N * prob)
    assert counts.sum() == N and (counts[prob * N > 50] > 0).all()
