"""kq_argmax on the device: exact against numpy.argmax(where(isnan(x), -inf, x)) (the
smallest index of the maximum of the non-NaN entries; llama.cpp's greedy sampler), through the
C-ABI call and through both forms of the backend's ARGMAX node. Every size comes from
argmax_plan, so the cases follow the kernel's own split: S entries per workgroup, lane t of a
workgroup reads the 16-B vectors t, t + 256, ... of its slice, four in flight, then steps on by
1024 vectors. The value, tie and NaN cases run on four splits: the default one (S = 1024, one
vector per lane), slices of 4096 and 8192 entries (ARGMAX_SLICE: four vectors per lane in one
block of loads, and a second block), and a vector long enough (300003 entries) that the plan
itself grows the slice past 256 workgroups' worth."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def ref_argmax(x):
    return int(np.argmax(np.where(np.isnan(x), -np.inf, x)))


@pytest.fixture(scope="module")
def S():
    """The default split's slice (the workspace and node tests)."""
    import ggml_mi355x as g
    wgs, s = g.argmax_plan(32000)
    assert wgs >= 3 and g.argmax_plan(2 * s + 3) == (3, s)  # one slice size over the tests' range
    return s


@pytest.fixture(params=["default", "slice4096", "slice8192", "n300003"])
def split(request, S):
    """(n, S) of one split: three workgroups and a tail (n = 2 S + 3) of the default slice and of
    two longer ones, or the plan's own grown slice of a long vector."""
    import ggml_mi355x as g
    if request.param.startswith("slice"):
        s = int(request.param[5:])
        g.debug_knob("ARGMAX_SLICE", s)
        try:
            assert g.argmax_plan(2 * s + 3) == (3, s)
            yield 2 * s + 3, s
        finally:
            g.debug_knob("ARGMAX_SLICE")  # (NaN: back to the default)
    elif request.param == "n300003":
        wgs, s = g.argmax_plan(300003)
        assert s > S and s % 4 == 0 and 3 <= wgs <= 256 and s // 4 > 256 + 7  # some lanes hold two vectors
        yield 300003, s
    else:
        yield 2 * S + 3, S


def run(x, dev, workspace=None):
    import torch
    import ggml_mi355x as g
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    out = g.argmax(xd, workspace=workspace)
    torch.cuda.synchronize()
    return int(out.cpu()[0])


def sizes(S, n):
    return [1, 2, 3, 5, 63, 64, 65, 257, S - 1, S, S + 1, 2 * S + 3, 32000, 128256, 128257, n]


@pytest.mark.parametrize("k", range(16))
def test_values(dev, split, k):
    n = sizes(split[1], split[0])[k]
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    assert run(x, dev) == ref_argmax(x), n
    y = (-np.abs(rng.standard_normal(n)) - 3.0).astype(np.float32)  # every entry negative
    assert (y < 0).all()
    assert run(y, dev) == ref_argmax(y), n


def tie_pairs(n, S):
    pairs = {
        "one vector of a lane": (4 * 7 + 1, 4 * 7 + 3),
        "two lanes of a row": (4 * 3 + 2, 4 * 9),
        "two rows of a wave": (4 * 3, 4 * 40 + 1),
        "two halves of a wave": (4 * 5 + 3, 4 * 37),
        "two waves": (4 * 10, 4 * (64 * 2 + 10)),
        "two slices": (S - 1, S),
        "second and third slice": (2 * S - 1, 2 * S),
        "a whole vector and the tail": (4 * (n // 4) - 4, n - 1),
        "first and last": (0, n - 1),
    }
    if S // 4 > 256 + 7:  # lane 7 holds a second vector of its slice (the same block of loads)
        pairs["two vectors of a lane"] = (4 * 7, 4 * (7 + 256))
        pairs["two vectors of a lane, second entry first"] = (4 * 7 + 2, 4 * (7 + 256) + 1)
    if S // 4 > 3 * 256 + 7:  # ... the block's first and last
        pairs["first and fourth vector of a lane"] = (4 * 7 + 3, 4 * (7 + 3 * 256))
    if S // 4 > 1024 + 7:  # ... and one of the next block, 1024 vectors on
        pairs["two blocks of a lane"] = (4 * 7 + 1, 4 * (7 + 1024) + 2)
        pairs["fourth vector and the next block"] = (4 * (7 + 3 * 256), 4 * (7 + 1024))
    return pairs


def test_tie_cases_cover_every_level(split):
    """No case is dropped by the split it runs on: every split but the default one has the tie
    in one lane's two vectors, and the longest slice the tie across the lane's blocks."""
    n, S = split
    names = set(tie_pairs(n, S))
    assert ("two vectors of a lane" in names) == (S > 1024)
    assert ("two blocks of a lane" in names) == (S >= 8192)
    assert all(0 <= i < j < n for i, j in tie_pairs(n, S).values())


@pytest.mark.parametrize("offset", [0, 1], ids=["slice0", "slice1"])
def test_ties_go_to_the_smallest_index(dev, split, offset):
    n, S = split
    pairs = tie_pairs(n, S)
    base = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    for name, (i, j) in pairs.items():
        if offset and max(i, j) < S:  # the same lanes of the second workgroup
            i, j = i + S, j + S
        x = base.copy()
        x[i] = x[j] = 9.5
        assert ref_argmax(x) == min(i, j)
        assert run(x, dev) == min(i, j), (name, i, j)
        x[i] = x[j] = np.float32(-9.5)  # a tie that is not the maximum changes nothing
        assert run(x, dev) == ref_argmax(x), name


def test_special_values(dev, split):
    n, S = split
    assert run(np.full(n, 1.25, np.float32), dev) == 0
    assert run(np.full(n, -np.inf, np.float32), dev) == 0
    x = np.full(n, -np.inf, np.float32)
    x[n - 1] = np.inf
    assert run(x, dev) == n - 1
    x = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    x[n - 1] = np.inf
    assert run(x, dev) == n - 1
    x[S] = np.inf
    assert run(x, dev) == S
    # -0.0 == +0.0: the smaller index wins whichever holds which
    neg = (-np.abs(np.random.default_rng(2).standard_normal(n)) - 1.0).astype(np.float32)
    for a, b in ((-0.0, 0.0), (0.0, -0.0)):
        x = neg.copy()
        x[0], x[5] = a, b
        assert run(x, dev) == 0, (a, b)
        x = neg.copy()
        x[S - 1], x[S + 5] = a, b
        assert run(x, dev) == S - 1, (a, b)
    # denormals and the largest finite values keep their order
    x = np.zeros(n, np.float32)
    x[3], x[S + 1] = np.float32(1e-45), np.float32(-1e-45)
    assert run(x, dev) == 3
    x = np.full(n, -np.finfo(np.float32).max, np.float32)
    x[2 * S + 1] = -np.finfo(np.float32).max / 2
    assert run(x, dev) == 2 * S + 1


def test_nan_never_wins(dev, split):
    n, S = split
    base = np.random.default_rng(7).standard_normal(n).astype(np.float32)
    x = base.copy()
    x[0] = np.nan
    assert run(x, dev) == ref_argmax(x)
    x = base.copy()
    x[:S] = np.nan  # the whole first slice: its workgroup has no entry to offer
    assert run(x, dev) == ref_argmax(x) >= S
    x = base.copy()
    x[::7] = np.nan
    x[3] = np.array([0xffc00001], np.uint32).view(np.float32)[0]  # a negative NaN with a payload
    x[4] = np.array([0x7f800001], np.uint32).view(np.float32)[0]  # the smallest NaN above +inf's bits
    assert np.isnan(x[3]) and np.isnan(x[4])
    assert run(x, dev) == ref_argmax(x)
    x = np.full(n, np.nan, np.float32)
    assert run(x, dev) == 0
    x[n - 1] = -np.inf  # one number among NaNs, in the tail
    assert run(x, dev) == n - 1
    if S // 4 > 256 + 7:  # a lane whose first vector is all NaN takes its second
        x = base.copy()
        x[:4 * 256] = np.nan
        x[4 * (7 + 256) + 1] = 9.5
        assert run(x, dev) == 4 * (7 + 256) + 1
    for m in (1, 3, 5):
        assert run(np.full(m, np.nan, np.float32), dev) == 0


def test_workspace_reuse_and_size(dev, S):
    import torch
    import ggml_mi355x as g
    n = 2 * S + 3
    ws = torch.zeros(g.argmax_workspace_size(n), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(11)
    for _ in range(3):  # zeroed once: every call leaves it ready for the next
        x = rng.standard_normal(n).astype(np.float32)
        assert run(x, dev, workspace=ws) == ref_argmax(x)
    # a shorter vector on the same workspace (fewer workgroups count in), then the long one again
    for m in (5, S + 1, n):
        x = rng.standard_normal(m).astype(np.float32)
        assert run(x, dev, workspace=ws) == ref_argmax(x), m
    xd = torch.zeros(n, dtype=torch.float32, device=dev)
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = g.lib().mi355x_argmax(xd.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, None)
    assert rc == g.E_WORKSPACE


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
def test_plain_node(dev, S, use_graph):
    import torch
    import ggml_mi355x as g
    n = 2 * S + 3
    b = g.Backend()
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    out = torch.full((1,), -1, dtype=torch.int32, device=dev)
    xt = g.make_tensor(g.TYPE_F32, n, 1, x.data_ptr())
    node = g.make_tensor(g.TYPE_I32, 1, 1, out.data_ptr(), op=g.OP_ARGMAX, srcs=[xt], op_params=[g.ARGMAX_PLAIN],
                         flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    rng = np.random.default_rng(13)
    for _ in range(3):  # the same node list, new data: a replay of the captured graph
        h = rng.standard_normal(n).astype(np.float32)
        x.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        assert b.graph_compute([node], use_graph=use_graph) == 0
        b.synchronize()
        assert int(out.cpu()[0]) == ref_argmax(h)
    b.close()


@pytest.mark.parametrize("use_graph", [True, False], ids=["hipgraph", "eager"])
def test_step_inputs_node(dev, S, use_graph):
    """The step-inputs form, driven directly: the token, pos + 1, the rope row of pos + 1 and
    the history entry; at the last row only the token and pos + 1."""
    import torch
    import ggml_mi355x as g
    n, hd, rows = 2 * S + 3, 64, 32
    b = g.Backend()
    rng = np.random.default_rng(17)
    h = rng.standard_normal(n).astype(np.float32)
    x = torch.from_numpy(h).to(dev)
    table_h = rng.standard_normal((rows, hd)).astype(np.float32)
    table = torch.from_numpy(table_h).to(dev)
    SENT = -7
    inp = torch.full((2 + hd,), SENT, dtype=torch.int32, device=dev)
    hist = torch.full((rows,), SENT, dtype=torch.int32, device=dev)
    srcs = [g.make_tensor(g.TYPE_F32, n, 1, x.data_ptr()),
            g.make_tensor(g.TYPE_I32, 1, 1, inp[1:2].data_ptr()),  # pos = dst + 1, as in the decoder
            g.make_tensor(g.TYPE_F32, hd, rows, table.data_ptr()),
            g.make_tensor(g.TYPE_I32, rows, 1, hist.data_ptr())]
    node = g.make_tensor(g.TYPE_I32, 2 + hd, 1, inp.data_ptr(), op=g.OP_ARGMAX, srcs=srcs,
                         op_params=[g.ARGMAX_STEP_INPUTS], flags=g.FLAG_OUTPUT)
    assert g.supports_op(node)
    tok = ref_argmax(h)

    inp[1] = 5
    torch.cuda.synchronize()
    assert b.graph_compute([node], use_graph=use_graph) == 0
    b.synchronize()
    got, hs = inp.cpu().numpy(), hist.cpu().numpy()
    assert got[0] == tok and got[1] == 6
    assert (got[2:] == table_h[6].view(np.int32)).all()
    assert hs[6] == tok and (np.delete(hs, 6) == SENT).all()

    # a second run from the state the first left: pos 6 -> 7
    assert b.graph_compute([node], use_graph=use_graph) == 0
    b.synchronize()
    got, hs = inp.cpu().numpy(), hist.cpu().numpy()
    assert got[0] == tok and got[1] == 7 and (got[2:] == table_h[7].view(np.int32)).all()
    assert hs[7] == tok and hs[6] == tok and (np.delete(hs, [6, 7]) == SENT).all()

    # the last row: the token and pos + 1 = rows are written, the row and the history are not
    inp.fill_(SENT)
    hist.fill_(SENT)
    inp[1] = rows - 1
    torch.cuda.synchronize()
    assert b.graph_compute([node], use_graph=use_graph) == 0
    b.synchronize()
    got, hs = inp.cpu().numpy(), hist.cpu().numpy()
    assert got[0] == tok and got[1] == rows
    assert (got[2:] == SENT).all() and (hs == SENT).all()

    # a negative position (unsigned compares): -1 + 1 = 0 is row 0; -2 + 1 is outside
    inp.fill_(SENT)
    inp[1] = -2
    torch.cuda.synchronize()
    assert b.graph_compute([node], use_graph=use_graph) == 0
    b.synchronize()
    got, hs = inp.cpu().numpy(), hist.cpu().numpy()
    assert got[0] == tok and got[1] == -1 and (got[2:] == SENT).all() and (hs == SENT).all()
    b.close()
