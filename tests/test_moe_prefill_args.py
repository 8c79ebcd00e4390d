"""CPU checks of the expert-grouped MoE prefill's host side: the selector mi355x_moe_prefill, what
mi355x_mul_mat_id_workspace_size returns under each mode, and where MI355X_E_WORKSPACE stands among the statuses
of mi355x_mul_mat_id (on fake pointers: every status here is returned before any device access). No device, no
launch. Every test leaves the selector as it found it."""
import contextlib

W, X, REC, Y, WS = 0x500000, 0x200000, 0x300000, 0x600000, 0x700000
NU = 2
Q8L = 304  # bytes of a Q8L block (a superblock of an activation row in the workspace)


@contextlib.contextmanager
def _mode(g, impl):
    prev = g.moe_prefill(impl)
    assert prev in (g.MOE_PREFILL_AUTO, g.MOE_PREFILL_GEMV, g.MOE_PREFILL_GROUPED)
    try:
        yield prev
    finally:
        g.moe_prefill(prev)


def _size(g, T, K=4096, typ=None):
    return int(g.lib().mi355x_mul_mat_id_workspace_size(g.TYPE_Q4_K if typ is None else typ, K, NU, T))


def _mmid(g, **kw):
    a = dict(type=g.TYPE_Q4_K, w=W, ne00=512, ne01=20, nb01=288, nb02=20 * 288, n_expert=4, x=X, ne11=1, xs=512, ids=REC,
             ids_stride=2 * NU, n_used=NU, T=3, y=Y, ws=None, ws_size=0)
    a.update(kw)
    return g.lib().mi355x_mul_mat_id(a["type"], a["w"], a["ne00"], a["ne01"], a["nb01"], a["nb02"], a["n_expert"], a["x"],
                                     a["ne11"], a["xs"], a["ids"], a["ids_stride"], a["n_used"], a["T"], a["y"], a["ws"],
                                     a["ws_size"], None)


def test_selector_values():
    import ggml_mi355x as g
    assert (g.MOE_PREFILL_AUTO, g.MOE_PREFILL_GEMV, g.MOE_PREFILL_GROUPED) == (0, 1, 2)
    first = g.moe_prefill(g.MOE_PREFILL_GEMV)
    try:
        assert first == g.MOE_PREFILL_AUTO  # the default
        assert g.moe_prefill(g.MOE_PREFILL_GROUPED) == g.MOE_PREFILL_GEMV
        assert g.moe_prefill(g.MOE_PREFILL_AUTO) == g.MOE_PREFILL_GROUPED
        for bad in (-1, 3, 7, 1 << 20):
            assert g.moe_prefill(bad) == g.E_INVAL
            assert g.moe_prefill(g.MOE_PREFILL_AUTO) == g.MOE_PREFILL_AUTO  # a refused value changes nothing
    finally:
        g.moe_prefill(first)


def test_workspace_size_by_mode():
    import ggml_mi355x as g
    with _mode(g, g.MOE_PREFILL_GEMV):
        for T in (1, 3, 16, 512, 32767):
            assert _size(g, T) == 0, T
    with _mode(g, g.MOE_PREFILL_AUTO):
        assert _size(g, 1) == 0  # (tests/test_moe_args.py asserts the same shape)
        assert _size(g, 7) == 0  # 14 pairs: below any threshold the mode may have (never under 16)
        assert _size(g, 32767) > 0
    with _mode(g, g.MOE_PREFILL_GROUPED):
        sizes = [_size(g, T) for T in (1, 2, 3, 16, 80, 512, 32767)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        # the table (1152 bytes of per-bucket words and 8 bytes a pair, in 256-byte steps) and a Q8L row per pair
        for T in (1, 80, 512):
            rows = T * NU * (4096 // 256) * Q8L
            assert rows + 1152 + 8 * T * NU <= _size(g, T) <= rows + 1152 + 8 * T * NU + 255, T
        assert _size(g, 80, K=14336, typ=g.TYPE_Q6_K) > _size(g, 80)
        # shapes mi355x_mul_mat_id refuses need nothing
        assert _size(g, 0) == 0 and _size(g, 32768) == 0 and _size(g, 4, K=500) == 0


def test_e_workspace_stands_between_the_shape_checks_and_the_device_check():
    import ggml_mi355x as g
    with _mode(g, g.MOE_PREFILL_GROUPED):
        need = int(g.lib().mi355x_mul_mat_id_workspace_size(g.TYPE_Q4_K, 512, NU, 3))
        assert need > 0
        for kw in (dict(), dict(ws=WS, ws_size=need - 1), dict(ws=WS, ws_size=64), dict(ws=None, ws_size=need),
                   dict(ws=WS + 8, ws_size=need + 8), dict(ne11=NU)):
            assert _mmid(g, **kw) == g.E_WORKSPACE, kw
        # after E_INVAL and E_UNSUPPORTED, whatever the workspace is
        for ws in (dict(), dict(ws=WS, ws_size=need)):
            assert _mmid(g, x=None, **ws) == g.E_INVAL
            assert _mmid(g, ne11=3, **ws) == g.E_INVAL
            assert _mmid(g, nb01=287, **ws) == g.E_INVAL
            assert _mmid(g, type=g.TYPE_Q8_K, **ws) == g.E_UNSUPPORTED
            assert _mmid(g, n_expert=65, **ws) == g.E_UNSUPPORTED
            assert _mmid(g, T=32768, **ws) == g.E_UNSUPPORTED
        # an empty shape launches nothing and needs nothing
        assert _mmid(g, T=0) == g.E_OK and _mmid(g, T=0, y=None) == g.E_INVAL
        assert _mmid(g, ne01=0) == g.E_WORKSPACE and _mmid(g, ne01=0, ws=WS, ws_size=need) == g.E_OK
        if not g.device_available():  # before E_NODEVICE
            assert _mmid(g, ws=WS, ws_size=need) == g.E_NODEVICE
            assert _mmid(g, ne11=NU, ws=WS, ws_size=need) == g.E_NODEVICE
            assert _mmid(g, T=1, ws=WS, ws_size=need) == g.E_NODEVICE
    with _mode(g, g.MOE_PREFILL_GEMV):  # the kq_gemv_id form never asks for one
        if not g.device_available():
            assert _mmid(g) == g.E_NODEVICE and _mmid(g, T=512, ids_stride=4) == g.E_NODEVICE
    with _mode(g, g.MOE_PREFILL_AUTO):
        if not g.device_available():
            assert _mmid(g) == g.E_NODEVICE  # 6 pairs: kq_gemv_id
            assert _mmid(g, T=512) == g.E_NODEVICE  # no workspace: AUTO runs kq_gemv_id, it refuses nothing
