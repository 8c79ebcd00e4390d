"""The Q3_K prefill selector without a device: its values, and that neither the workspace size nor the refusals of
a Q3_K mul_mat (on fake pointers: each is returned before any device access) depend on it."""
import pytest

import ggml_mi355x as g

W, X, Y, WS = 0x10000, 0x20000, 0x30000, 0x40000  # never dereferenced
MODES = ("Q3K_PREFILL_AUTO", "Q3K_PREFILL_GEMV", "Q3K_PREFILL_MMQ")


def test_selector_values():
    assert tuple(getattr(g, m) for m in MODES) == (0, 1, 2)
    first = g.q3k_prefill(g.Q3K_PREFILL_GEMV)
    try:
        assert first == g.Q3K_PREFILL_AUTO  # the default
        assert g.q3k_prefill(g.Q3K_PREFILL_MMQ) == g.Q3K_PREFILL_GEMV
        for bad in (-1, 3, 1 << 20):
            assert g.q3k_prefill(bad) == g.E_INVAL
            assert g.q3k_prefill(g.Q3K_PREFILL_MMQ) == g.Q3K_PREFILL_MMQ  # a refused value changes nothing
    finally:
        g.q3k_prefill(first)


@pytest.mark.parametrize("mode", MODES)
def test_sizes_and_refusals_do_not_depend_on_the_selector(mode):
    def mm(K, N, M, w=W, nb01=None, ws=WS, ws_size=1 << 30):
        nb01 = K // 256 * 110 if nb01 is None else nb01
        return g.lib().mi355x_mul_mat(g.TYPE_Q3_K, w, K, N, nb01, X, M, K * 4, Y, N * 4, ws, ws_size, None)

    prev = g.q3k_prefill(getattr(g, mode))
    try:
        for K, M in ((256, 1), (768, 15), (768, 16), (768, 63), (768, 64), (4096, 512), (32768, 2)):
            want = 0 if M == 1 else (M * (K // 256) * 304 + 255) // 256 * 256
            assert g.lib().mi355x_mul_mat_workspace_size(g.TYPE_Q3_K, K, 67, M) == want, (K, M)
        for M in (1, 15, 16, 64, 512):
            assert mm(256, 4, M, w=W + 1) == g.E_INVAL              # an odd address
            assert mm(256, 4, M, nb01=220) == g.E_UNSUPPORTED       # rows not packed
            assert mm(256 * 257, 4, M) == g.E_UNSUPPORTED           # K > 65536
            if M > 1:
                assert mm(768, 4, M, ws=None, ws_size=0) == g.E_WORKSPACE
                assert mm(768, 4, M, ws_size=3 * 292 * M - 1) == g.E_WORKSPACE
    finally:
        g.q3k_prefill(prev)
