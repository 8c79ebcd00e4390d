"""CPU checks of tests/penalize_ref.py, the numpy restatement of mi355x_penalize_rows' rule
(include/ggml_mi355x.h): the header's worked case by bits, the order of the biases, the identity
parameters, the window as a multiset, the largest count and the ids outside the vocabulary."""
import numpy as np

from tests import penalize_ref as R

F = np.float32


def bits(v):
    return int(np.asarray(v, dtype=F).view(np.uint32))


def test_worked_case_by_bits():
    x = np.array([1.5, -2.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 3.0], dtype=F)
    win = [0, 1, 1, 2, 3, 4, 5, 6, 9, -1]
    bias = [(7, -np.inf), (0, 1.0), (0, 0.5)]
    y, touched = R.penalize_row(x, win, repeat=1.1, freq=0.25, present=0.5, bias=bias)
    assert bits(y[0]) == 0x3ffd1746   # ((1.5 + 1.0 + 0.5) / 1.1f) - 0.75
    assert bits(y[1]) == 0xc04ccccd   # (-2 * 1.1f) - 1.0
    assert bits(y[2]) == 0xbf400000   # -0.75
    assert bits(y[3]) == 0xbf400000   # -0.0 counts as <= 0: -0.0 * 1.1f - 0.75
    assert np.isnan(y[4]) and y[5] == np.inf and y[6] == -np.inf and y[7] == -np.inf
    assert touched.all()
    # the same through the rows form, the window cut out of a history by end and last_n
    hist = np.array([[5, 5] + win + [0, 0]], dtype=np.int32)
    y2, t2 = R.penalize_rows(x[None, :], hist, [11], last_n=10, repeat=1.1, freq=0.25, present=0.5, bias=bias)
    assert R.same(y2[0], y, touched) and t2.all()


def test_bias_order_matters():
    x = np.array([0.0, 1e8], dtype=F)
    a, _ = R.penalize_row(x, bias=[(1, -1e8), (1, 1e-3)])
    b, _ = R.penalize_row(x, bias=[(1, 1e-3), (1, -1e8)])
    assert bits(a[1]) == bits(F(1e-3)) and bits(b[1]) == bits(F(0.0))
    assert bits(a[0]) == bits(b[0]) == 0


def test_identity_parameters_keep_the_bits():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64).astype(F)
    x[:6] = [0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42]  # (finite and infinite values: a NaN may lose its payload)
    win = list(rng.integers(0, 64, 200))
    y, touched = R.penalize_row(x, win, repeat=1.0, freq=0.0, present=0.0)
    assert (y.view(np.uint32) == x.view(np.uint32)).all() and touched.sum() == len(set(win))
    y, touched = R.penalize_row(x)  # no window, no bias: nothing is written
    assert (y.view(np.uint32) == x.view(np.uint32)).all() and not touched.any()
    payload = np.array([0x7fc12345, 0xffc00001], np.uint32).view(F)
    y, touched = R.penalize_row(payload, [0], repeat=1.5, bias=[(5, 1.0)])
    assert bits(y[1]) == 0xffc00001 and not touched[1] and np.isnan(y[0]) and touched[0]  # the untouched NaN keeps its payload


def test_a_permuted_window_gives_the_same_result():
    rng = np.random.default_rng(4)
    x = rng.standard_normal(50).astype(F)
    win = list(rng.integers(-2, 52, 300))
    kw = dict(repeat=1.3, freq=0.125, present=-0.5, bias=[(3, 0.25), (60, 1.0), (3, -2.0)])
    y, touched = R.penalize_row(x, win, **kw)
    for seed in range(3):
        p = list(np.random.default_rng(seed).permutation(win))
        y2, t2 = R.penalize_row(x, p, **kw)
        assert (y2.view(np.uint32) == y.view(np.uint32)).all() and (t2 == touched).all()


def test_1024_copies_of_one_token():
    x = np.array([2.0, -3.0, 5.0], dtype=F)
    freq = F(0.001)
    y, touched = R.penalize_row(x, [1] * 1024, repeat=1.0, freq=freq, present=0.0)
    assert bits(y[1]) == bits(F(F(-3.0) - F(F(1024.0) * freq))) and touched.tolist() == [False, True, False]
    hist = np.full((1, 2000), 1, np.int32)
    y2, _ = R.penalize_rows(x[None, :], hist, [1500], last_n=1024, repeat=1.0, freq=freq, present=0.0)
    assert bits(y2[0, 1]) == bits(y[1])


def test_ids_outside_the_vocabulary_are_ignored():
    x = np.arange(8, dtype=F)
    win = [-1, 8, 9, -2 ** 31, 2 ** 31 - 1, 1 << 20]
    y, touched = R.penalize_row(x, win, repeat=2.0, freq=1.0, present=1.0, bias=[(-1, 5.0), (8, -np.inf), (-2 ** 31, 1.0)])
    assert (y.view(np.uint32) == x.view(np.uint32)).all() and not touched.any()
    y, touched = R.penalize_row(x, win + [7], repeat=2.0, freq=1.0, present=1.0)
    assert y[7] == F(7.0 / 2.0 - 2.0) and touched.sum() == 1


def test_window_position():
    hist = np.arange(10, dtype=np.int32)
    assert R.window(hist, 4, 3) == [2, 3, 4]
    assert R.window(hist, 1, 5) == [0, 1]                    # clipped at 0
    assert R.window(hist, -1, 5) == [] and R.window(hist, 3, 0) == []
    assert R.window(hist, 12, 5) == [8, 9]                   # end past the row
    assert R.window(hist, 2 ** 31 - 1, 1024) == [] and R.window(hist, -2 ** 31, 1024) == []
    assert R.window(hist, 9, 1024) == list(range(10))
