"""Streamed attention (mi355x_attn_stream, csrc/kq_attn_stream.hip): which descriptors take it, on
the CPU (mi355x_attn_path: no launch, no device access), and the reference the GPU tests use past
the oracle's 8192-cell arrays.

Mode 0 (the default) changes nothing; mode 1 moves only the descriptors that are refused for their
cache size (n_ctx > 8192, or the per-head layout past 64 KB) onto the streamed kernels, for 32 <=
n_ctx <= 131072 in multiples of 32; mode 2 moves every valid descriptor."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]

TINY = (32, 4, 64)    # TinyLlama: n_head, n_head_kv, head_dim
L3_8B = (32, 8, 128)  # Llama-3-8B


@pytest.fixture(scope="module")
def g():
    import ggml_mi355x as g
    if not os.path.exists(g.LIB_PATH):
        pytest.skip("library not built")
    return g


@pytest.fixture
def stream_mode(g):
    """Sets mi355x_attn_stream for one test and puts the previous mode back."""
    prev = []

    def set_mode(mode):
        p = g.attn_stream(mode)
        if not prev:
            prev.append(p)
        return p
    yield set_mode
    if prev:
        g.attn_stream(prev[0])


def composed_attn_decode(O, q, k, v, k_cache, v_cache, pos, n_head, n_head_kv, head_dim, scale):
    """oracle.kqo_attn_decode composed in Python from the oracle's exported primitives, as the C
    function composes them (its 8192-entry arrays stop it at n_kv 8192; this has no limit): the new
    cell into both caches (fp32_to_fp16), vec_dot_f16 per (head, cell) of [0, n_kv), soft_max_row
    with the 0 / -INF causal mask and the scale, fp32_to_fp16 of the weights, vec_dot_f16 per
    output over [0, n_kv). q, k already roped; the caches are updated in place."""
    n_ctx = k_cache.shape[0]
    kvw = n_head_kv * head_dim
    q = np.ascontiguousarray(q, np.float32)
    k_cache[pos, :] = O.fp32_to_fp16(k)
    v_cache[:, pos] = O.fp32_to_fp16(v)
    n_kv = O.attn_n_kv(pos, n_ctx)
    mask = np.where(np.arange(n_kv) <= pos, np.float32(0.0), np.float32(-np.inf)).astype(np.float32)
    gsz = n_head // n_head_kv
    out = np.empty(n_head * head_dim, np.float32)
    for h in range(n_head):
        g0 = (h // gsz) * head_dim
        q16 = O.fp32_to_fp16(q[h * head_dim:(h + 1) * head_dim])
        krows = np.ascontiguousarray(k_cache[:n_kv, g0:g0 + head_dim])
        kq = np.array([O.vec_dot_f16(krows[c], q16) for c in range(n_kv)], np.float32)
        p16 = O.fp32_to_fp16(O.soft_max_row(kq, mask, scale))
        for d in range(head_dim):
            out[h * head_dim + d] = O.vec_dot_f16(v_cache[g0 + d, :n_kv], p16)
    assert kvw == k_cache.shape[1]
    return out


def test_mode0_is_todays_dispatch(g, stream_mode):
    assert stream_mode(0) in (0, 1, 2)
    assert g.attn_path(8192, *TINY) == g.E_UNSUPPORTED
    assert g.attn_path(16384, *TINY) == g.E_UNSUPPORTED
    assert g.attn_path(4096, *TINY) == g.ATTN_PATH_CELLS
    assert g.attn_path(256, *L3_8B) == g.ATTN_PATH_HEAD


def test_mode1_takes_only_the_size_refused(g, stream_mode):
    assert g.ATTN_PATH_STREAM == 7
    stream_mode(1)
    for n_ctx in (8192, 16384, 131072):
        assert g.attn_path(n_ctx, *TINY) == g.ATTN_PATH_STREAM, n_ctx
        assert g.attn_path(n_ctx, *L3_8B) == g.ATTN_PATH_STREAM, n_ctx
    assert g.attn_path(8160, *TINY) == g.ATTN_PATH_STREAM    # a multiple of 32, not of 64
    assert g.attn_path(7648, *TINY) == g.ATTN_PATH_STREAM    # <= 8192, past the 64 KB per-head layout
    assert g.attn_path(7072, *L3_8B) == g.ATTN_PATH_STREAM
    assert g.attn_path(131104, *TINY) == g.E_UNSUPPORTED     # past 131072
    assert g.attn_path(100, *TINY) == g.E_UNSUPPORTED        # n_ctx % 32
    assert g.attn_path(16384, 32, 4, 96) == g.E_UNSUPPORTED  # head_dim
    assert g.attn_path(16384, 32, 4, 64, cache_offset=8) == g.E_INVAL
    # every descriptor that runs today keeps its kernel
    assert g.attn_path(4096, *TINY) == g.ATTN_PATH_CELLS
    assert g.attn_path(7616, *TINY) == g.ATTN_PATH_CELLS
    assert g.attn_path(7040, *L3_8B) == g.ATTN_PATH_CELLS
    assert g.attn_path(256, *L3_8B) == g.ATTN_PATH_HEAD
    assert g.attn_path(1024, *TINY) == g.ATTN_PATH_SPLIT4


def test_mode2_takes_every_valid_descriptor(g, stream_mode):
    stream_mode(2)
    assert g.attn_path(256, *TINY) == g.ATTN_PATH_STREAM
    assert g.attn_path(32, *L3_8B) == g.ATTN_PATH_STREAM
    assert g.attn_path(4096, *TINY) == g.ATTN_PATH_STREAM
    assert g.attn_path(131072, *L3_8B) == g.ATTN_PATH_STREAM
    assert g.attn_path(131104, *TINY) == g.E_UNSUPPORTED
    assert g.attn_path(100, *TINY) == g.E_UNSUPPORTED
    assert g.attn_path(1024, 32, 4, 96) == g.E_UNSUPPORTED
    prev = g.attn_impl(g.ATTN_GROUP)  # the decode selector does not take a descriptor back
    try:
        assert g.attn_path(128, *TINY) == g.ATTN_PATH_STREAM
    finally:
        g.attn_impl(prev)


def test_invalid_mode_and_previous_value(g, stream_mode):
    stream_mode(0)
    assert g.attn_stream(1) == 0
    assert g.attn_stream(3) == g.E_INVAL and g.attn_stream(-1) == g.E_INVAL
    assert g.attn_stream(2) == 1  # the refused calls changed nothing
    assert g.attn_stream(0) == 2
    assert g.attn_path(8192, *TINY) == g.E_UNSUPPORTED


def test_debug_knob_reaches_the_selector(g, stream_mode):
    """bench.py reaches the selector through --knob only: ATTN_STREAM = 0 / 1 / 2 overrides the
    mode, any other value (its default -1) leaves mi355x_attn_stream's."""
    stream_mode(0)
    assert g.debug_knob("ATTN_STREAM", 1) == -1
    try:
        assert g.attn_path(16384, *TINY) == g.ATTN_PATH_STREAM
        assert g.attn_path(4096, *TINY) == g.ATTN_PATH_CELLS
        g.debug_knob("ATTN_STREAM", 2)
        assert g.attn_path(4096, *TINY) == g.ATTN_PATH_STREAM
        g.debug_knob("ATTN_STREAM", 0)
        g.attn_stream(2)
        assert g.attn_path(4096, *TINY) == g.ATTN_PATH_CELLS
    finally:
        g.debug_knob("ATTN_STREAM")
    assert g.attn_path(4096, *TINY) == g.ATTN_PATH_STREAM  # the selector's own mode again
    assert g.debug_knob("ATTN_STREAM_TILE", 7) == 0
    assert g.debug_knob("ATTN_STREAM_TILE") == 7


def test_supports_op_follows_the_mode(g, stream_mode):
    """ATTN_DECODE over a 16384-cell cache: refused by supports_op with the mode off, taken with it on;
    ATTN_BATCH keeps its 8192."""
    nh, nkv, hd, n_ctx = 8, 2, 64, 16384
    kvw = nkv * hd

    def attn_node(op, extra=()):
        q = g.make_tensor(g.TYPE_F32, nh * hd, 1, 0x10000)
        k = g.make_tensor(g.TYPE_F32, kvw, 1, 0x20000)
        v = g.make_tensor(g.TYPE_F32, kvw, 1, 0x30000)
        pos = g.make_tensor(g.TYPE_I32, 1, 1, 0x40000)
        kc = g.make_tensor(g.TYPE_F16, kvw, n_ctx, 0x1000000)
        vc = g.make_tensor(g.TYPE_F16, n_ctx, kvw, 0x2000000)
        tab = g.make_tensor(g.TYPE_F32, hd, n_ctx, 0x3000000)
        srcs = [q, k, v, pos, kc, vc, tab] + list(extra)
        node = g.make_tensor(g.TYPE_F32, nh * hd, 1, 0x50000, op=op, srcs=srcs, op_params=[nh, nkv, hd, 0])
        return node, srcs

    stream_mode(0)
    node, keep = attn_node(g.OP_ATTN_DECODE)
    assert not g.supports_op(node)
    stream_mode(1)
    assert g.supports_op(node)
    del keep


def test_composed_reference_equals_the_oracle_at_4096_cells():
    from oracle import kq_ops_oracle as O
    O.lib()
    hd, nh, nkv, n_ctx = 64, 2, 1, 4096
    rng = np.random.default_rng(4096)
    kvw = nkv * hd
    kc = rng.standard_normal((n_ctx, kvw)).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((kvw, n_ctx)).astype(np.float16).view(np.uint16)
    kc2, vc2 = kc.copy(), vc.copy()
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    for p, qs in ((0, 2.0), (33, 2.0), (2500, 40.0), (4095, 2.0)):
        q = (rng.standard_normal(nh * hd) * qs).astype(np.float32)
        k = (rng.standard_normal(kvw) * 2).astype(np.float32)
        v = rng.standard_normal(kvw).astype(np.float32)
        ref = O.attn_decode(q, k, v, kc, vc, p, nh, nkv, hd, scale)
        got = composed_attn_decode(O, q, k, v, kc2, vc2, p, nh, nkv, hd, scale)
        assert (got.view(np.uint32) == ref.view(np.uint32)).all(), p
    assert (kc == kc2).all() and (vc == vc2).all()
