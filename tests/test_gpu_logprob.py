"""mi355x_logprob_rows on the device (kq_argmax_rows, then kq_logsum_rows): every record equal to
tests/logprob_ref.py's bit for bit, max, x_target, argmax, pad and the 8 bytes of sum. The sizes
follow kq_logsum_rows' split, one workgroup per 1024 entries: one block and less, the block's
edge, three blocks with a partial last vector, the vocabularies of the models and the largest n.
Rows that are no multiple of 4 entries lie on rows padded with +inf to the next 16 bytes: a
kernel that read the padding would answer NaN. The reference sums are computed once per size."""
import numpy as np
import pytest

from tests import logprob_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2052, 32000, 128256, 262144]
ROWS = [1, 3, 8]
SCALES = [1.0, 3.0, 0.25, 10.0, 1.0, 30.0, 2.0, 5.0]  # row i's logits: standard normal times SCALES[i]
_rows, _sums = {}, {}


def matrix(n):
    """The 8 rows of size n (every test of that n takes the first `rows` of them)."""
    if n not in _rows:
        rng = np.random.default_rng(0x5EED + n)
        _rows[n] = (rng.standard_normal((8, n)) * np.array(SCALES)[:, None]).astype(np.float32)
    return _rows[n]


def records(key, x, targets):
    """ref_records(x, targets) with the rows' (argmax, max, S) computed once per key."""
    if key not in _sums:
        _sums[key] = [R.ref_sum(row) for row in x]
    out = np.zeros(len(targets), R.DTYPE)
    for i, t in enumerate(targets):
        a, m, S = _sums[key][i]
        out[i] = (m, x[i, t] if 0 <= t < x.shape[1] else R.NAN, a, 0, S)
    return out


def on_device(x, dev, stride=None):
    """x [T, n] as a cuda view on rows of `stride` floats (n rounded up to 4) whose padding is +inf."""
    import torch
    T, n = x.shape
    stride = (n + 3) & ~3 if stride is None else stride
    buf = np.full((T, stride), np.inf, np.float32)
    buf[:, :n] = x
    return torch.from_numpy(buf).to(dev)[:, :n]


def targets_for(x):
    """Row by row: 0, n - 1, the argmax, -1, n, and entries inside the row."""
    T, n = x.shape
    kinds = [0, n - 1, R.ref_argmax(x[2 % T]), -1, n, (7 * n) // 13, 2 ** 31 - 1, n // 2]
    return kinds[:T]


def check(got, want):
    assert got.dtype == R.DTYPE and got.shape == want.shape
    assert R.same_records(got, want), R.first_mismatch(got, want)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", SIZES)
def test_records_equal_the_rule(dev, n, rows):
    import ggml_mi355x as g
    x = matrix(n)[:rows]
    tg = targets_for(x)
    want = records(n, matrix(n), tg)
    check(g.logprob_rows(on_device(x, dev), tg), want)
    assert (want["pad"] == 0).all()
    if rows == 8:  # a record carries what the host needs: the values are those of a float64 log-softmax
        lp = g.logprob_value(want)
        ref = np.array([x[i, t].astype(np.float64) - x[i].max().astype(np.float64) -
                        np.log(np.exp(x[i].astype(np.float64) - x[i].max().astype(np.float64)).sum())
                        if 0 <= t < n else np.nan for i, t in enumerate(tg)])
        ok = ~np.isnan(ref)
        assert np.isnan(lp[~ok]).all() and np.abs(lp[ok] - ref[ok]).max() <= 1e-6


@pytest.mark.parametrize("n", [5, 1025, 32000])
def test_strided_matrix(dev, n):
    import ggml_mi355x as g
    x = matrix(n)[:3]
    xd = on_device(x, dev, stride=(n + 4 + 3) & ~3)
    assert xd.stride(0) == (n + 7) & ~3 and xd.stride(0) >= n + 4
    tg = [n - 1, 0, n // 3]
    check(g.logprob_rows(xd, tg), records(n, matrix(n), tg))


def test_targets(dev):
    """One row under every kind of target: x_target alone changes; outside the row the NaN 0x7fc00000."""
    import ggml_mi355x as g
    n = 2052
    row = matrix(n)[1]
    a = R.ref_argmax(row)
    tg = [0, n - 1, a, -1, n, n + 1, 2 ** 31 - 1, -2 ** 31, 1024, 2051 - 3]
    x = np.tile(row, (len(tg), 1))
    want = records(("targets", n), x, tg)
    got = g.logprob_rows(on_device(x, dev), tg)
    check(got, want)
    outside = [i for i, t in enumerate(tg) if not 0 <= t < n]
    assert (got["x_target"][outside].view(np.uint32) == 0x7fc00000).all() and len(outside) == 5
    assert got["x_target"][2] == got["max"][2] and (got["argmax"] == a).all()
    assert len(set(got["sum"].view(np.uint64).tolist())) == 1 and len(set(got["max"].view(np.uint32).tolist())) == 1


def built_rows(n):
    """name -> row: rows built to go wrong (n = 2052: three blocks, the last of one whole vector)."""
    rng = np.random.default_rng(99)
    base = rng.standard_normal(n).astype(np.float32)
    out = {}
    x = base.copy()
    x[[1023, 1024]] = 9.5  # the maximum twice, on both sides of a block boundary: the smaller index
    out["maximum twice"] = x
    x = base.copy()
    x[[2051, 7]] = 9.5
    out["maximum at 7 and n - 1"] = x
    x = base.copy()
    x[::3] = -np.inf
    x[1024:2048] = -np.inf  # a whole block of e == 0
    out["-inf entries"] = x
    out["spread"] = (base * np.float32(400.0)).astype(np.float32)  # most e underflow to 0
    x = (base * np.float32(30.0)).astype(np.float32)
    x[5] = 1.0e30
    out["one huge entry"] = x  # every other d is about -1e30: e == 0, S == 1
    x = np.full(n, -np.inf, np.float32)
    x[2049] = -17.25
    out["one finite entry among -inf"] = x
    x = (-np.abs(base) - 1.0).astype(np.float32)
    x[300], x[1500] = -0.0, 0.0  # -0.0 == +0.0: the first, with its own sign in max
    out["zero tie"] = x
    out["all equal"] = np.full(n, 1.5, np.float32)  # S == n exactly
    out["denormal e"] = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-100.0)).astype(np.float32)
    return out


def test_built_rows(dev):
    import ggml_mi355x as g
    n = 2052
    rows = built_rows(n)
    x = np.stack(list(rows.values()))
    tg = [1024, 7, 4, 100, 5, 2049, 1500, 2051, 1]
    want = records(("built", n), x, tg)
    got = g.logprob_rows(on_device(x, dev), tg)
    for i, name in enumerate(rows):
        assert got[i].tobytes() == want[i].tobytes(), (name, got[i], want[i])
    names = list(rows)
    assert got["argmax"][names.index("maximum twice")] == 1023 and got["argmax"][names.index("maximum at 7 and n - 1")] == 7
    assert got["sum"][names.index("one huge entry")] == 1.0 and got["sum"][names.index("one finite entry among -inf")] == 1.0
    assert got["sum"][names.index("all equal")] == float(n)
    z = got[names.index("zero tie")]
    assert z["argmax"] == 300 and np.signbit(z["max"]) and not np.signbit(z["x_target"])
    assert g.logprob_value(got)[names.index("one finite entry among -inf")] == 0.0


def test_one_workspace_call_after_call(dev):
    """Two calls back to back on one workspace with different n and rows, enqueued through the
    C-ABI with no synchronization in between: both exact, whichever comes first."""
    import torch
    import ggml_mi355x as g
    L = g.lib()
    big, small = (32000, 8), (1025, 3)
    ws = torch.zeros(g.logprob_workspace_size(big[0], big[1]), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for order in ((big, small), (small, big), (small, small)):
        runs = []
        for n, rows in order:
            x = matrix(n)[:rows]
            tg = targets_for(x)
            xd = on_device(x, dev)
            tgd = torch.tensor(tg, dtype=torch.int32, device=dev)
            out = torch.zeros(24 * rows, dtype=torch.uint8, device=dev)
            runs.append((n, tg, out, xd, tgd))
        for n, tg, out, xd, tgd in runs:
            assert L.mi355x_logprob_rows(xd.data_ptr(), n, len(tg), xd.stride(0), tgd.data_ptr(), out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), stream) == 0
        torch.cuda.synchronize()
        for n, tg, out, _, _ in runs:
            check(out.cpu().numpy().view(R.DTYPE), records(n, matrix(n), tg))


def test_workspace_shared_with_argmax_rows(dev):
    """argmax_rows before and after a logprob_rows call on the same workspace: the counters come
    back to 0 and the words one kernel leaves are nothing the other reads."""
    import torch
    import ggml_mi355x as g
    n, rows = 128256, 3
    x = matrix(n)[:rows]
    xd = on_device(x, dev)
    ws = torch.zeros(g.logprob_workspace_size(n, rows), dtype=torch.uint8, device=dev)
    assert ws.numel() == g.argmax_rows_workspace_size(n, rows)
    ref = np.array([R.ref_argmax(r) for r in x], np.int32)
    tg = targets_for(x)
    a1 = g.argmax_rows(xd, workspace=ws)
    got = g.logprob_rows(xd, tg, workspace=ws)
    a2 = g.argmax_rows(xd, workspace=ws)
    torch.cuda.synchronize()
    assert (a1.cpu().numpy() == ref).all() and (a2.cpu().numpy() == ref).all()
    check(got, records(n, matrix(n), tg))
    # every counter is 0 again; the argmax the first launch left in the counter's line is row i's
    w = ws.cpu().numpy().reshape(rows, 2176)
    assert (w[:, :4].view(np.uint32) == 0).all()
    assert (w[:, 64:68].view(np.int32).ravel() == ref).all()
