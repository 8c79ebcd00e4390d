"""CPU checks of the row-wise argmax's host side: the workspace size, the order of
mi355x_argmax_rows' argument errors (on fake pointers: all are returned before any device
access), and what mi355x_backend_supports_op takes of an ARGMAX_BATCH node. The ARGMAX node is
still judged as tests/test_argmax_plan.py says. No device, no launch."""
import ctypes

import pytest

from tests import test_argmax_plan as AP

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 32000, 128256, 128257, 1 << 24]
ROWS = [1, 2, 3, 8, 64, 65535]


def test_workspace_size():
    import ggml_mi355x as g
    for rows in ROWS:
        sizes = [g.argmax_rows_workspace_size(n, rows) for n in SIZES]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (rows, sizes)  # monotone in n
        for n, s in zip(SIZES, sizes):
            # one 8-B word per workgroup of the plan and a counter fit, for every row
            assert s >= rows * (8 * g.argmax_plan(n)[0] + 4), (n, rows)
    for n in SIZES:
        sizes = [g.argmax_rows_workspace_size(n, rows) for rows in ROWS]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (n, sizes)  # every row has a part of its own
        # a row's part is a whole number of 128-B lines: no row's words share a line with a counter
        assert g.argmax_rows_workspace_size(n, 2) == 2 * g.argmax_rows_workspace_size(n, 1)
        assert g.argmax_rows_workspace_size(n, 1) % 128 == 0 and g.argmax_rows_workspace_size(n, 1) >= 256
    # a row's part does not depend on n: every counter keeps its place when a workspace goes from
    # one n to another (a place that moved would land on the words the other n left behind)
    for rows in ROWS:
        assert len({g.argmax_rows_workspace_size(n, rows) for n in SIZES}) == 1, rows


@pytest.mark.parametrize("n,rows", [(0, 1), (-1, 1), ((1 << 24) + 1, 1), (32000, 0), (32000, -1), (32000, 65536)])
def test_workspace_size_is_zero_outside_the_ranges(n, rows):
    import ggml_mi355x as g
    assert g.argmax_rows_workspace_size(n, rows) == 0
    # mi355x_argmax_rows itself: before any device access
    assert g.lib().mi355x_argmax_rows(0x1000, n, rows, max(n, 4) + 4 & ~3, 0x2000, 0x3000, 1 << 30, None) == g.E_INVAL


def test_argument_errors_in_order_without_device():
    import ggml_mi355x as g
    L = g.lib()
    n, rows = 32000, 8
    ws = g.argmax_rows_workspace_size(n, rows)
    X, OUT, WS = 0x1000, 0x2000, 0x3000
    assert L.mi355x_argmax_rows(None, n, rows, n, OUT, WS, ws, None) == g.E_INVAL
    assert L.mi355x_argmax_rows(0x1004, n, rows, n, OUT, WS, ws, None) == g.E_INVAL       # x not 16-B aligned
    assert L.mi355x_argmax_rows(X, n, rows, n - 4, OUT, WS, ws, None) == g.E_INVAL        # row_stride < n
    assert L.mi355x_argmax_rows(X, n, rows, n + 2, OUT, WS, ws, None) == g.E_INVAL        # row_stride * 4 not 16-B aligned
    assert L.mi355x_argmax_rows(X, n - 1, rows, n - 1, OUT, WS, ws, None) == g.E_INVAL    # ... for an odd n too
    assert L.mi355x_argmax_rows(X, n, 0, n, OUT, WS, ws, None) == g.E_INVAL
    assert L.mi355x_argmax_rows(X, n, 65536, n, OUT, WS, 1 << 40, None) == g.E_INVAL
    assert L.mi355x_argmax_rows(X, n, rows, n, None, WS, ws, None) == g.E_INVAL
    # E_INVAL comes before E_WORKSPACE: a bad argument with a bad workspace
    assert L.mi355x_argmax_rows(X, n, rows, n - 4, OUT, None, 0, None) == g.E_INVAL
    assert L.mi355x_argmax_rows(X, n, rows, n, None, WS, ws - 1, None) == g.E_INVAL
    assert L.mi355x_argmax_rows(X, n, rows, n, OUT, None, ws, None) == g.E_WORKSPACE
    assert L.mi355x_argmax_rows(X, n, rows, n, OUT, WS, ws - 1, None) == g.E_WORKSPACE
    assert L.mi355x_argmax_rows(X, n, rows, n, OUT, WS, g.argmax_rows_workspace_size(n, rows - 1), None) == g.E_WORKSPACE
    if not g.device_available():
        assert L.mi355x_argmax_rows(X, n, rows, n, OUT, WS, ws, None) == g.E_NODEVICE
        assert L.mi355x_argmax_rows(X, n - 1, rows, n + 4, OUT, WS, ws, None) == g.E_NODEVICE  # a padded odd row


# ---------------------------------------------------------------- supports_op on hand-made nodes
V, N_KV, NH = 32000, 64, 48


def _plain(T, x=None, dst_type=None, dst_n=None, dst_data=0x9000, form=None):
    import ggml_mi355x as g
    x = g.make_tensor(g.TYPE_F32, V, T, 0x100000) if x is None else x
    return g.make_tensor(g.TYPE_I32 if dst_type is None else dst_type, T if dst_n is None else dst_n, 1, dst_data,
                         op=g.OP_ARGMAX_BATCH, srcs=[x], op_params=[g.ARGMAX_PLAIN if form is None else form])


def _step(T, pos="ok", cells="ok", mask="ok", hist="ok", dst_n=None, x=None, cell_stride=1, n_kv=N_KV):
    import ggml_mi355x as g
    x = g.make_tensor(g.TYPE_F32, V, T, 0x100000) if x is None else x
    pos = g.make_tensor(g.TYPE_I32, T, 1, 0x9000 + 4 * T) if pos == "ok" else pos  # (the decoder's block:
    cells = g.make_tensor(g.TYPE_I32, T, 1, 0x9000 + 8 * T) if cells == "ok" else cells  # tokens | pos | cells | mask)
    mask = g.make_tensor(g.TYPE_F32, N_KV, T, 0x9000 + 12 * T) if mask == "ok" else mask
    hist = g.make_tensor(g.TYPE_I32, NH, T, 0x30000) if hist == "ok" else hist
    return g.make_tensor(g.TYPE_I32, T if dst_n is None else dst_n, 1, 0x9000, op=g.OP_ARGMAX_BATCH,
                         srcs=[x, pos, cells, mask, hist], op_params=[g.ARGMAX_STEP_INPUTS, cell_stride, n_kv])


@pytest.mark.parametrize("T", [1, 3])
def test_supports_op_accepts_both_forms(T):
    import ggml_mi355x as g
    assert g.OP_ARGMAX_BATCH == 13
    assert g.supports_op(_plain(T))
    assert g.supports_op(_step(T))
    assert g.supports_op(_step(T, cell_stride=3))
    # a mask and a history with padded rows
    assert g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F32, N_KV + 32, T, 0xa000)))
    assert g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F32, N_KV, T, 0xa000, row_stride=4 * N_KV + 64)))
    assert g.supports_op(_step(T, hist=g.make_tensor(g.TYPE_I32, NH, T, 0x30000, row_stride=4 * NH + 16)))
    for n in (4, 2304, 1 << 24):
        assert g.supports_op(_plain(T, x=g.make_tensor(g.TYPE_F32, n, T, 0x100000))), n


@pytest.mark.parametrize("T", [1, 3])
def test_supports_op_refuses_bad_sources_and_dst(T):
    import ggml_mi355x as g
    assert not g.supports_op(_plain(T, x=g.make_tensor(g.TYPE_F16, V, T, 0x100000)))            # f16 source
    strided = g.make_tensor(g.TYPE_F32, V, T, 0x100000)
    strided.nb[0] = 8
    assert not g.supports_op(_plain(T, x=strided))                                               # strided entries
    assert not g.supports_op(_plain(3, x=g.make_tensor(g.TYPE_F32, V, 3, 0x100000, row_stride=4 * V + 16)))  # strided rows
    assert not g.supports_op(_plain(T, x=g.make_tensor(g.TYPE_F32, V, T, 0x100004)))            # misaligned source
    assert not g.supports_op(_plain(T, x=g.make_tensor(g.TYPE_F32, V, T, None)))
    for n in (V + 1, V + 2, 5):
        assert not g.supports_op(_plain(T, x=g.make_tensor(g.TYPE_F32, n, T, 0x100000))), n     # n % 4 != 0
    assert not g.supports_op(_plain(T, x=g.make_tensor(g.TYPE_F32, (1 << 24) + 4, T, 0x100000)))  # n outside the range
    assert not g.supports_op(_plain(T, dst_type=g.TYPE_F32))                                     # dst of the wrong type
    assert not g.supports_op(_plain(T, dst_n=T + 1))                                             # dst of the wrong length
    assert not g.supports_op(_plain(3, dst_n=1))
    assert not g.supports_op(_plain(T, dst_data=None))
    assert not g.supports_op(_plain(T, form=2))                                                  # a form of 2
    assert not g.supports_op(_plain(T, form=-1))
    no_src = _plain(T)
    no_src.src[0] = ctypes.POINTER(g.Tensor)()
    assert not g.supports_op(no_src)


@pytest.mark.parametrize("T", [1, 3])
def test_supports_op_refuses_bad_step_operands(T):
    import ggml_mi355x as g
    assert not g.supports_op(_step(T, dst_n=T + 1))
    assert not g.supports_op(_step(T, x=g.make_tensor(g.TYPE_F16, V, T, 0x100000)))
    for name in ("pos", "cells"):  # missing, f32, I64, of another length, no data
        assert not g.supports_op(_step(T, **{name: None})), name
        assert not g.supports_op(_step(T, **{name: g.make_tensor(g.TYPE_F32, T, 1, 0x9100)})), name
        assert not g.supports_op(_step(T, **{name: g.make_tensor(g.TYPE_I64, T, 1, 0x9100)})), name
        assert not g.supports_op(_step(T, **{name: g.make_tensor(g.TYPE_I32, T + 1, 1, 0x9100)})), name
        assert not g.supports_op(_step(T, **{name: g.make_tensor(g.TYPE_I32, T, 1, None)})), name
    # mask: missing, F16, I32, narrower than n_kv, rows of another count, row stride below n_kv, no data
    assert not g.supports_op(_step(T, mask=None))
    assert not g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F16, N_KV, T, 0xa000)))
    assert not g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_I32, N_KV, T, 0xa000)))
    assert not g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F32, N_KV - 1, T, 0xa000)))
    assert not g.supports_op(_step(T, n_kv=N_KV + 32))
    assert not g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F32, N_KV, T + 1, 0xa000)))
    assert not g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F32, N_KV, T, 0xa000, row_stride=4 * N_KV - 4)))
    assert not g.supports_op(_step(T, mask=g.make_tensor(g.TYPE_F32, N_KV, T, None)))
    # history: missing, f32, rows of another count, no data
    assert not g.supports_op(_step(T, hist=None))
    assert not g.supports_op(_step(T, hist=g.make_tensor(g.TYPE_F32, NH, T, 0x30000)))
    assert not g.supports_op(_step(T, hist=g.make_tensor(g.TYPE_I32, NH, T + 1, 0x30000)))
    assert not g.supports_op(_step(T, hist=g.make_tensor(g.TYPE_I32, NH, T, None)))
    # cell_stride and n_kv
    assert not g.supports_op(_step(T, cell_stride=0))
    assert not g.supports_op(_step(T, cell_stride=-1))
    assert not g.supports_op(_step(T, n_kv=0))


def test_argmax_node_is_judged_as_before():
    """The ARGMAX node takes no matrix and no third form: test_argmax_plan.py's cases, unchanged."""
    import ggml_mi355x as g
    AP.test_supports_op_accepts_both_forms()
    AP.test_supports_op_refuses_bad_sources_and_dst()
    AP.test_supports_op_refuses_bad_step_operands()
    # an ARGMAX_BATCH's operands on an ARGMAX node, and the reverse, are refused
    batch_as_vec = _step(3)
    batch_as_vec.op = g.OP_ARGMAX
    assert not g.supports_op(batch_as_vec)
    vec_as_batch = AP._step()
    vec_as_batch.op = g.OP_ARGMAX_BATCH
    assert not g.supports_op(vec_as_batch)
