"""mi355x_small_batch and its neighbours without a device: the selector, the constants, the
workspace size that does not depend on it, and the kq_rows_cols plan query."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def g():
    import ggml_mi355x as g
    prev = g.small_batch()
    yield g
    g.small_batch(prev)


def test_selector_round_trip(g):
    assert g.small_batch() == g.SMALL_BATCH_NODES == 0  # the default; -1 queries
    assert g.small_batch(g.SMALL_BATCH_FUSED) == g.SMALL_BATCH_NODES
    assert g.small_batch() == g.SMALL_BATCH_FUSED == 1
    for bad in (2, -2):
        assert g.small_batch(bad) == g.E_INVAL
        assert g.small_batch() == g.SMALL_BATCH_FUSED
    assert g.small_batch(g.SMALL_BATCH_NODES) == g.SMALL_BATCH_FUSED


def test_constants_in_header(g):
    text = open(os.path.join(ROOT, "include", "ggml_mi355x.h")).read()
    for name in ("SMALL_BATCH_NODES", "SMALL_BATCH_FUSED"):
        m = re.search(r"#define MI355X_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(g, name)


@pytest.mark.parametrize("ne11", [1, 2, 15, 16])
def test_workspace_size_is_the_same_in_both_modes(g, ne11):
    L = g.lib()
    sizes = []
    for mode in (g.SMALL_BATCH_NODES, g.SMALL_BATCH_FUSED):
        g.small_batch(mode)
        sizes.append(L.mi355x_mul_mat_workspace_size(g.TYPE_Q4_K, 2048, 64, ne11))
    want = 0 if ne11 == 1 else (ne11 * 8 * 304 + 255) // 256 * 256
    assert sizes == [want, want]


def test_rows_cols_plan_narrows_with_k(g):
    ncols = [p["ncol"] if p else 0 for p in (g.rows_cols_plan(k, 8) for k in (2048, 4096, 8192, 16384, 65536))]
    assert ncols == sorted(ncols, reverse=True) and ncols[0] == 8 and ncols[-1] == 0
    assert g.rows_cols_plan(2048, 15)["groups"] == 2 and g.rows_cols_plan(2048, 3)["ncol"] == 4
