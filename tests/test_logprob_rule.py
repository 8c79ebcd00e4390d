"""CPU checks of the log-probability rule's restatement (tests/logprob_ref.py): its sum against a
float64 log-sum-exp, the tree's independence of padding, -inf entries, ties, targets. No device."""
import math

import numpy as np
import pytest

from tests import logprob_ref as R

SIZES = [1, 3, 5, 1025, 32000, 128256, 262144]
SCALES = [0.01, 1.0, 3.0, 10.0, 50.0]
_base = {}


def base(n):
    if n not in _base:
        _base[n] = np.random.default_rng(0x10F + n).standard_normal(n).astype(np.float32)
    return _base[n]


@pytest.mark.parametrize("n", SIZES)
def test_sum_against_float64_logsumexp(n):
    """|log S - ref| <= 1e-6. The bound: ggml states about 2 ulp for v_expf and the f32 quad sum
    adds two roundings, so S is within about 4e-7 relative of the exact sum; 2.5 x that. (The f64
    tree's own error, 16 levels of 2^-53, is far below.) Measured with these inputs: 1.1e-7 at worst."""
    worst = 0.0
    for scale in SCALES:
        x = (base(n) * np.float32(scale)).astype(np.float32)
        a, m, S = R.ref_sum(x)
        assert a == int(np.argmax(x)) and m == x.max()
        ref = math.log(math.fsum(np.exp(x.astype(np.float64) - float(m)).tolist()))
        err = abs(math.log(S) - ref)
        worst = max(worst, err)
        assert err <= 1e-6, (n, scale, err)
    print(f"n {n}: worst |log S - ref| {worst:.3g}")


@pytest.mark.parametrize("n", [1, 3, 5, 1025, 4099])
def test_tree_is_independent_of_padding(n):
    x = (base(n) * np.float32(3.0)).astype(np.float32)
    a, m, S = R.ref_sum(x)
    # the row at the front of a longer row whose further entries have e == 0
    for extra in (1, 3, 1024, 70000):
        long = np.concatenate([x, np.full(extra, -np.inf, np.float32)])
        assert R.ref_sum(long) == (a, m, S), extra
    # ... and the tree over fewer leaves (absent leaves are +0.0 and adding +0.0 is exact)
    e = R.exp_terms(x, m)
    leaves = 1
    while 4 * leaves < n:
        leaves *= 2
    while leaves <= R.LEAVES:
        assert R.tree_sum(R.quad_sums(e, leaves)) == S, leaves
        leaves *= 2


def test_neg_inf_entries_contribute_exactly_zero():
    n = 5003
    x = (base(n) * np.float32(2.0)).astype(np.float32)
    a = int(np.argmax(x))
    gone = np.array([i for i in (0, 1, 2, 3, 7, 1024, 4096, 5000, 5002) if i != a])
    y = x.copy()
    y[gone] = -np.inf
    e = R.exp_terms(x, x[a])
    e[gone] = 0.0
    assert R.ref_sum(y) == (a, x[a], R.tree_sum(R.quad_sums(e)))
    assert (R.exp_terms(y, x[a])[gone].view(np.uint32) == 0).all()  # +0.0f, not v_expf(-inf)
    # one finite entry among -inf: S == 1 exactly, the log-probability of that entry 0
    z = np.full(77, -np.inf, np.float32)
    z[41] = -3.5
    r = R.ref_record(z, 41)
    assert (int(r["argmax"]), float(r["max"]), float(r["sum"]), float(R.value(r))) == (41, -3.5, 1.0, 0.0)
    assert R.value(R.ref_record(z, 40)) == -np.inf


def test_a_tie_for_the_maximum_picks_the_smaller_index():
    x = (base(1025) * np.float32(0.5)).astype(np.float32)
    x[[700, 90, 1024]] = 9.0
    r = R.ref_record(x, 700)
    assert int(r["argmax"]) == 90 and r["max"] == np.float32(9.0) and r["x_target"] == np.float32(9.0)
    assert r["sum"] >= 3.0  # the three maxima count 1.0 each
    z = np.array([-1.0, -0.0, 0.0, -2.0], np.float32)  # -0.0 == +0.0: the first of them, its own bits
    r = R.ref_record(z, 2)
    assert int(r["argmax"]) == 1 and np.signbit(r["max"]) and not np.signbit(r["x_target"])


def test_targets_and_the_record():
    x = base(1025)
    assert R.DTYPE.itemsize == 24 and R.DTYPE.fields["sum"][1] == 16
    a, m, S = R.ref_sum(x)
    for t in (0, 1024, a):
        r = R.ref_record(x, t)
        assert r["x_target"] == x[t] and r["pad"] == 0 and float(r["sum"]) == S
        assert float(R.value(r)) == float(x[t]) - float(m) - math.log(S)
    assert float(R.value(R.ref_record(x, a))) <= 0.0
    for t in (-1, 1025, 2 ** 31 - 1, -2 ** 31):
        r = R.ref_record(x, t)
        assert r["x_target"].view(np.uint32) == 0x7fc00000 and math.isnan(float(R.value(r)))
    # the values over a row are a distribution
    lp = R.value(R.ref_records(np.tile(base(5), (5, 1)), range(5)))
    assert abs(np.exp(lp).sum() - 1.0) < 1e-6


def test_header_states_the_rule_and_python_mirrors_it():
    import os
    import ggml_mi355x as g
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ggml_mi355x.h")).read()
    for piece in ("struct mi355x_logprob { float max, x_target; int32_t argmax, pad; double sum; }",
                  "#define MI355X_LOGPROB_MAX_N 262144", "MI355X_OP_LOGPROB_BATCH = 16", "mi355x_logprob_value"):
        assert piece in hdr, piece
    assert g.OP_LOGPROB_BATCH == 16 and g.LOGPROB_MAX_N == R.MAX_N and g.logprob_dtype() == R.DTYPE
    recs = R.ref_records(np.tile(base(1025), (3, 1)), [0, 5, -1])
    got, want = g.logprob_value(recs), R.value(recs)
    assert got.dtype == np.float64 and (got.view(np.uint64) == want.view(np.uint64)).all()
