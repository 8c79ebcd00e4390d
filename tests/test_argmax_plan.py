"""CPU checks of the argmax's host side: the split mi355x_argmax_plan decides, the workspace
size, and what mi355x_backend_supports_op takes of an ARGMAX node. No device, no launch."""
import ctypes

import pytest

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 32000, 128256, 128257, 1 << 24]


@pytest.mark.parametrize("n", SIZES)
def test_plan_covers_the_vector(n):
    import ggml_mi355x as g
    wgs, s = g.argmax_plan(n)
    assert wgs >= 1
    assert s % 4 == 0
    assert (wgs - 1) * s < n <= wgs * s  # the slices cover [0, n), none is empty
    assert g.argmax_workspace_size(n) > 0


def test_workspace_size_grows_with_n():
    import ggml_mi355x as g
    sizes = [g.argmax_workspace_size(n) for n in sorted(SIZES)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    # one 8-B word per workgroup of the plan and a counter fit
    for n in SIZES:
        assert g.argmax_workspace_size(n) >= 8 * g.argmax_plan(n)[0] + 4


@pytest.mark.parametrize("n", [0, -1, (1 << 24) + 1])
def test_plan_refuses_sizes_outside_the_range(n):
    import ggml_mi355x as g
    assert g.argmax_plan(n) == g.E_INVAL
    assert g.argmax_workspace_size(n) == 0
    # mi355x_argmax itself: before any device access
    assert g.lib().mi355x_argmax(0x1000, n, 0x2000, 0x3000, 1 << 20, None) == g.E_INVAL


def test_argmax_argument_checks_without_device():
    import ggml_mi355x as g
    L = g.lib()
    ws = g.argmax_workspace_size(32000)
    assert L.mi355x_argmax(None, 32000, 0x2000, 0x3000, ws, None) == g.E_INVAL
    assert L.mi355x_argmax(0x1004, 32000, 0x2000, 0x3000, ws, None) == g.E_INVAL  # x not 16-B aligned
    assert L.mi355x_argmax(0x1000, 32000, None, 0x3000, ws, None) == g.E_INVAL
    assert L.mi355x_argmax(0x1000, 32000, 0x2000, None, ws, None) == g.E_WORKSPACE
    assert L.mi355x_argmax(0x1000, 32000, 0x2000, 0x3000, ws - 1, None) == g.E_WORKSPACE
    if not g.device_available():
        assert L.mi355x_argmax(0x1000, 32000, 0x2000, 0x3000, ws, None) == g.E_NODEVICE


# ---------------------------------------------------------------- supports_op on hand-made nodes
HD, ROWS, NH, V = 64, 32, 48, 32000


def _plain(x=None, dst_type=None, dst_n=1, dst_data=0x9000):
    import ggml_mi355x as g
    x = g.make_tensor(g.TYPE_F32, V, 1, 0x1000) if x is None else x
    return g.make_tensor(g.TYPE_I32 if dst_type is None else dst_type, dst_n, 1, dst_data, op=g.OP_ARGMAX, srcs=[x],
                         op_params=[g.ARGMAX_PLAIN])


def _step(pos="ok", tab="ok", hist="ok", dst_n=2 + HD, x=None):
    import ggml_mi355x as g
    x = g.make_tensor(g.TYPE_F32, V, 1, 0x1000) if x is None else x
    pos = g.make_tensor(g.TYPE_I32, 1, 1, 0x9004) if pos == "ok" else pos  # (dst + 1: the decoder's layout)
    tab = g.make_tensor(g.TYPE_F32, HD, ROWS, 0x20000) if tab == "ok" else tab
    hist = g.make_tensor(g.TYPE_I32, NH, 1, 0x30000) if hist == "ok" else hist
    return g.make_tensor(g.TYPE_I32, dst_n, 1, 0x9000, op=g.OP_ARGMAX, srcs=[x, pos, tab, hist],
                         op_params=[g.ARGMAX_STEP_INPUTS])


def test_supports_op_accepts_both_forms():
    import ggml_mi355x as g
    assert g.OP_ARGMAX == 12
    assert g.supports_op(_plain())
    assert g.supports_op(_step())
    for n in (1, 5, 1 << 24):
        assert g.supports_op(_plain(x=g.make_tensor(g.TYPE_F32, n, 1, 0x1000))), n


def test_supports_op_refuses_bad_sources_and_dst():
    import ggml_mi355x as g
    assert not g.supports_op(_plain(x=g.make_tensor(g.TYPE_F16, V, 1, 0x1000)))   # f16 source
    strided = g.make_tensor(g.TYPE_F32, V, 1, 0x1000)
    strided.nb[0] = 8
    assert not g.supports_op(_plain(x=strided))                                     # strided source
    assert not g.supports_op(_plain(x=g.make_tensor(g.TYPE_F32, V, 1, 0x1004)))    # misaligned source
    assert not g.supports_op(_plain(x=g.make_tensor(g.TYPE_F32, V, 2, 0x1000)))    # not a vector
    assert not g.supports_op(_plain(x=g.make_tensor(g.TYPE_F32, (1 << 24) + 4, 1, 0x1000)))  # n outside the range
    assert not g.supports_op(_plain(dst_type=g.TYPE_F32))                           # dst of the wrong type
    assert not g.supports_op(_plain(dst_n=2))                                       # dst of the wrong length
    assert not g.supports_op(_plain(dst_data=None))
    bad_form = _plain()
    bad_form.op_params[0] = 2
    assert not g.supports_op(bad_form)
    no_src = _plain()
    no_src.src[0] = ctypes.POINTER(g.Tensor)()
    assert not g.supports_op(no_src)


def test_supports_op_refuses_bad_step_operands():
    import ggml_mi355x as g
    assert not g.supports_op(_step(dst_n=1))            # the plain dst on the step form
    assert not g.supports_op(_step(dst_n=2 + HD + 1))   # dst is exactly [2 + head_dim]
    assert not g.supports_op(_step(x=g.make_tensor(g.TYPE_F16, V, 1, 0x1000)))
    # pos: missing, f32, two entries
    assert not g.supports_op(_step(pos=None))
    assert not g.supports_op(_step(pos=g.make_tensor(g.TYPE_F32, 1, 1, 0x9004)))
    assert not g.supports_op(_step(pos=g.make_tensor(g.TYPE_I32, 2, 1, 0x9004)))
    # table: missing, f16, strided rows, no data
    assert not g.supports_op(_step(tab=None))
    assert not g.supports_op(_step(tab=g.make_tensor(g.TYPE_F16, HD, ROWS, 0x20000)))
    assert not g.supports_op(_step(tab=g.make_tensor(g.TYPE_F32, HD, ROWS, 0x20000, row_stride=4 * HD + 16)))
    assert not g.supports_op(_step(tab=g.make_tensor(g.TYPE_F32, HD, ROWS, None)))
    # a table of another head_dim than the dst's row
    assert not g.supports_op(_step(tab=g.make_tensor(g.TYPE_F32, 2 * HD, ROWS, 0x20000)))
    # history: missing, f32, two rows
    assert not g.supports_op(_step(hist=None))
    assert not g.supports_op(_step(hist=g.make_tensor(g.TYPE_F32, NH, 1, 0x30000)))
    assert not g.supports_op(_step(hist=g.make_tensor(g.TYPE_I32, NH, 2, 0x30000)))
