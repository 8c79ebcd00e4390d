"""kq_topk on the device: idx / val equal tests/sample_ref.ref_topk exactly (the top_k largest
non-NaN entries under kq_argmax's order, sorted), through mi355x_topk and mi355x_topk_rows. The
sizes follow the kernel's split (argmax_plan): one slice, a tail of n % 4 entries, a last slice
shorter than top_k (3075), 256 slices, more than top_k, so the last arriver prunes (262144 + 4),
a slice the plan grows itself (300003), and slices of 4096 entries (ARGMAX_SLICE), where a lane
reads further vectors of its slice pass after pass."""
import numpy as np
import pytest

from tests import sample_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 2, 40, 64)
SIZES = (1, 3, 7, 1024, 1025, 3075, 262144 + 4, 300003)


def run(x, k, dev, workspace=None):
    import torch
    import ggml_mi355x as g
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    idx, val = g.topk(xd, k, workspace=workspace)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def check(x, k, dev, workspace=None, what=None):
    idx, val = run(x, k, dev, workspace)
    ridx, rval = R.ref_topk_out(x, k)
    assert idx.tolist() == ridx.tolist(), (what, len(x), k)
    assert (val.view(np.uint32) == rval.view(np.uint32)).all(), (what, len(x), k)


@pytest.fixture(params=["default", "slice4096"])
def S(request):
    """The slice of the value cases' split: three workgroups and a tail, n = 2 S + 3."""
    import ggml_mi355x as g
    if request.param == "default":
        s = g.argmax_plan(32000)[1]
        assert g.argmax_plan(2 * s + 3) == (3, s)
        yield s
    else:
        g.debug_knob("ARGMAX_SLICE", 4096)
        try:
            assert g.argmax_plan(2 * 4096 + 3) == (3, 4096)
            yield 4096
        finally:
            g.debug_knob("ARGMAX_SLICE")


def test_plans_of_the_sizes(dev):
    import ggml_mi355x as g
    assert g.argmax_plan(3075) == (4, 1024)  # a last slice of 3 entries, shorter than top_k
    wgs, s = g.argmax_plan(262144 + 4)
    assert wgs == 256 and s > 1024  # more slices than top_k
    wgs, s = g.argmax_plan(300003)
    assert s > 1024 and 64 < wgs <= 256


@pytest.mark.parametrize("n", SIZES)
def test_random_values(dev, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    y = np.round(rng.standard_normal(n) * 3).astype(np.float32)  # many equal values: the index decides
    for k in KS:
        check(x, k, dev, what="normal")
        check(y, k, dev, what="ties")


@pytest.mark.parametrize("n", [1025, 2 * 4096 + 3, 5 * 4096])
def test_longer_slices(dev, n):
    import ggml_mi355x as g
    g.debug_knob("ARGMAX_SLICE", 4096)
    try:
        rng = np.random.default_rng(n)
        x = rng.standard_normal(n).astype(np.float32)
        y = np.round(rng.standard_normal(n) * 3).astype(np.float32)
        for k in KS:
            check(x, k, dev, what="normal")
            check(y, k, dev, what="ties")
    finally:
        g.debug_knob("ARGMAX_SLICE")


def test_all_equal(dev, S):
    n = 2 * S + 3
    for k in KS:
        idx, val = run(np.full(n, 1.25, np.float32), k, dev)
        assert idx.tolist() == list(range(k)) and (val == 1.25).all()


def test_ties_across_a_slice_boundary(dev, S):
    """Seven equal maxima around the first boundary, top_k 5: the k-th place is tied across slices
    and goes to the smaller index; then the same below a larger maximum in the last slice."""
    n = 2 * S + 3
    base = (-np.abs(np.random.default_rng(3).standard_normal(n)) - 1.0).astype(np.float32)
    x = base.copy()
    x[S - 3:S + 4] = 9.5
    idx, _ = run(x, 5, dev)
    assert idx.tolist() == list(range(S - 3, S + 2))
    x[n - 1] = 10.0
    idx, _ = run(x, 5, dev)
    assert idx.tolist() == [n - 1] + list(range(S - 3, S + 1))
    for k in KS:
        check(x, k, dev)


def test_the_whole_top_k_in_the_last_slice(dev, S):
    n = 2 * S + 100
    x = (-np.abs(np.random.default_rng(4).standard_normal(n)) - 1.0).astype(np.float32)
    x[2 * S:] = np.random.default_rng(5).permutation(100).astype(np.float32)
    for k in KS:
        check(x, k, dev)
    idx, _ = run(x, 64, dev)
    assert idx.min() >= 2 * S


def test_one_candidate_per_slice(dev):
    import ggml_mi355x as g
    n = 262144 + 4
    wgs, s = g.argmax_plan(n)
    rng = np.random.default_rng(6)
    x = (-np.abs(rng.standard_normal(n)) - 1.0).astype(np.float32)
    slices = rng.permutation(wgs)[:64]
    at = slices * s + rng.integers(0, 4, 64)  # (inside its slice: the last slice has >= 4 entries)
    assert (at < n).all()
    x[at] = 1.0 + rng.permutation(64).astype(np.float32)
    for k in KS:
        check(x, k, dev)
    idx, _ = run(x, 64, dev)
    assert sorted(idx.tolist()) == sorted(at.tolist())


def test_special_values(dev, S):
    n = 2 * S + 3
    neg = (-np.abs(np.random.default_rng(2).standard_normal(n)) - 1.0).astype(np.float32)
    x = neg.copy()  # -0.0 == +0.0: the smaller index first, whichever holds which; val keeps the sign
    x[5], x[S - 1], x[S + 5], x[n - 1] = -0.0, 0.0, -0.0, 0.0
    idx, val = run(x, 4, dev)
    assert idx.tolist() == [5, S - 1, S + 5, n - 1]
    assert np.signbit(val).tolist() == [True, False, True, False]
    check(x, 40, dev, what="zeros")
    x = neg.copy()
    x[3], x[S], x[n - 2] = np.inf, np.inf, -np.inf
    check(x, 3, dev, what="inf")
    check(x, 64, dev, what="inf")
    x = np.full(n, -np.inf, np.float32)
    x[n - 1] = np.inf
    for k in KS:
        check(x, k, dev, what="-inf")
    x = np.zeros(n, np.float32)  # denormals and the largest finite values keep their order
    x[3], x[S + 1], x[7] = np.float32(1e-45), np.float32(-1e-45), np.finfo(np.float32).max
    check(x, 40, dev, what="denormal")
    idx, _ = run(x, 2, dev)
    assert idx.tolist() == [7, 3]


def test_nan_is_never_a_candidate(dev, S):
    n = 2 * S + 3
    base = np.random.default_rng(7).standard_normal(n).astype(np.float32)
    x = base.copy()
    x[::7] = np.nan
    x[3] = np.array([0xffc00001], np.uint32).view(np.float32)[0]
    x[4] = np.array([0x7f800001], np.uint32).view(np.float32)[0]
    for k in KS:
        check(x, k, dev, what="nan")
    x = base.copy()
    x[:S] = np.nan  # the whole first slice has no candidate
    check(x, 40, dev, what="nan slice")
    # fewer than top_k non-NaN entries: -1 / NaN places
    x = np.full(n, np.nan, np.float32)
    x[1], x[S + 2], x[n - 1] = 2.0, -np.inf, 3.0
    idx, val = run(x, 40, dev)
    assert idx.tolist() == [n - 1, 1, S + 2] + [-1] * 37
    assert val[:3].tolist() == [3.0, 2.0, -np.inf] and (val[3:].view(np.uint32) == 0x7fc00000).all()
    for k in KS:
        check(x, k, dev, what="few")
    # all NaN
    for m in (1, 3, n):
        idx, val = run(np.full(m, np.nan, np.float32), 2, dev)
        assert idx.tolist() == [-1, -1] and (val.view(np.uint32) == 0x7fc00000).all()


def test_one_workspace_across_shrinking_calls(dev):
    """126 slices at top_k 64, then 8 entries at top_k 2 on the same workspace (zeroed once): the
    second call sees none of the first's words; then the long one again."""
    import torch
    import ggml_mi355x as g
    n = 128256
    assert g.argmax_plan(n)[0] == 126
    ws = torch.zeros(g.topk_workspace_size(n), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(9)
    big = rng.standard_normal(n).astype(np.float32) + 5.0
    small = (rng.standard_normal(8) - 20.0).astype(np.float32)
    check(big, 64, dev, workspace=ws)
    check(small, 2, dev, workspace=ws)
    check(small, 64, dev, workspace=ws)
    check(big[:1025], 40, dev, workspace=ws)
    check(big, 64, dev, workspace=ws)
    xd = torch.zeros(n, dtype=torch.float32, device=dev)
    idx = torch.zeros(64, dtype=torch.int32, device=dev)
    val = torch.zeros(64, dtype=torch.float32, device=dev)
    rc = g.lib().mi355x_topk(xd.data_ptr(), n, 64, idx.data_ptr(), val.data_ptr(), ws.data_ptr(), ws.numel() - 1, None)
    assert rc == g.E_WORKSPACE


def test_rows_equal_single_calls(dev):
    import torch
    import ggml_mi355x as g
    T, n = 3, 3075
    rng = np.random.default_rng(10)
    x = rng.standard_normal((T, n + 1)).astype(np.float32)  # row stride n + 1: a multiple of 4
    x[1] = np.round(x[1] * 2)
    x[2, ::2] = np.nan
    xd = torch.from_numpy(x).to(dev)[:, :n]
    ws = torch.zeros(g.topk_workspace_size(n, T), dtype=torch.uint8, device=dev)
    for k in (40, 2, 64):  # one workspace, top_k shrinking and growing
        idx, val = g.topk_rows(xd, k, workspace=ws)
        torch.cuda.synchronize()
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        for i in range(T):
            ridx, rval = R.ref_topk_out(x[i, :n], k)
            assert idx[i].tolist() == ridx.tolist(), (i, k)
            assert (val[i].view(np.uint32) == rval.view(np.uint32)).all(), (i, k)
            sidx, sval = run(x[i, :n], k, dev)
            assert sidx.tolist() == idx[i].tolist() and (sval.view(np.uint32) == val[i].view(np.uint32)).all()
