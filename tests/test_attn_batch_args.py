"""CPU (no launch): the argument checks of mi355x_attn_batch, supports_op of the ATTN_BATCH node
and the adapter's cells_match promise (adapter/mi355x_ggml_mirror.hpp), compiled into a small
stand-alone program."""
import ctypes
import os
import subprocess

import pytest

import ggml_mi355x as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 20


def desc(n_ctx=64, n_head=4, n_head_kv=2, head_dim=64, n_kv=64, n_tokens=2, cells=BASE + 128, cells_type=g.TYPE_I32,
         mask=BASE + 256, mask_type=g.TYPE_F32, mask_row_bytes=None, rope_row=0, **ptr):
    """A well-formed descriptor over synthetic, aligned addresses (never dereferenced)."""
    a = g.AttnDesc(ptr.get("q", BASE), ptr.get("k", BASE + 4096), ptr.get("v", BASE + 8192), ptr.get("pos", BASE + 64),
                   ptr.get("rope_table", BASE + 12288), ptr.get("k_cache", BASE + (1 << 12)),
                   ptr.get("v_cache", BASE + (1 << 13)), ptr.get("out", BASE + (1 << 14)), n_ctx, n_head, n_head_kv,
                   head_dim, 0.125, rope_row)
    if mask_row_bytes is None:
        mask_row_bytes = n_kv * (2 if mask_type == g.TYPE_F16 else 4)
    return g.AttnBatchDesc(a, cells, cells_type, mask, mask_type, mask_row_bytes, n_kv, n_tokens)


def status(d):
    """mi355x_attn_batch's argument status without a launch (mi355x_attn_batch_path shares the checks)."""
    return g.lib().mi355x_attn_batch_path(ctypes.byref(d))


def test_well_formed_descriptor_passes():
    assert status(desc()) == g.ATTN_GROUP
    assert status(desc(mask_type=g.TYPE_F16, cells_type=g.TYPE_I64, n_kv=32, n_ctx=128)) == g.ATTN_GROUP
    assert status(desc(n_head=16, n_head_kv=1)) == g.ATTN_HEAD  # a group of more than 8 heads


@pytest.mark.parametrize("bad", [dict(cells=None), dict(mask=None), dict(q=None), dict(k=None), dict(v=None),
                                 dict(pos=None), dict(rope_table=None), dict(k_cache=None), dict(v_cache=None),
                                 dict(out=None),
                                 dict(cells_type=g.TYPE_F32), dict(cells_type=g.TYPE_F16), dict(mask_type=g.TYPE_I32),
                                 dict(mask_type=g.TYPE_Q4_K),
                                 dict(n_kv=40), dict(n_kv=0), dict(n_kv=16), dict(n_kv=96), dict(n_kv=-32),
                                 dict(mask_row_bytes=64 * 4 - 4), dict(mask_type=g.TYPE_F16, mask_row_bytes=64 * 2 - 2),
                                 dict(rope_row=1), dict(n_tokens=0), dict(n_tokens=-3)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_argument_errors_are_inval(bad):
    """A null pointer, a cells / mask type outside the list, n_kv % 32 != 0 / < 32 / > n_ctx, a mask
    row shorter than n_kv entries, rope_row != 0, n_tokens <= 0: MI355X_E_INVAL, from both entry
    points, before any device access (the addresses are synthetic; this host has no device)."""
    d = desc(**bad)
    assert status(d) == g.E_INVAL
    assert g.lib().mi355x_attn_batch(ctypes.byref(d), None) == g.E_INVAL
    assert g.lib().mi355x_attn_batch(None, None) == g.E_INVAL


def test_shapes_the_kernels_do_not_take_are_unsupported():
    assert status(desc(head_dim=96)) == g.E_UNSUPPORTED
    assert status(desc(n_tokens=70000)) == g.E_UNSUPPORTED


# ---------------------------------------------------------------- supports_op
def batch_node(hd=64, nh=4, nkv=2, n_ctx=64, n_kv=64, T=3, mask_type=g.TYPE_F16, cells_type=g.TYPE_I64, mask=True):
    kvw = nkv * hd
    keep = [g.make_tensor(g.TYPE_F32, nh * hd, T, BASE), g.make_tensor(g.TYPE_F32, kvw, T, BASE + (1 << 16)),
            g.make_tensor(g.TYPE_F32, kvw, T, BASE + (2 << 16)), g.make_tensor(g.TYPE_I32, T, 1, BASE + (3 << 16)),
            g.make_tensor(g.TYPE_F16, kvw, n_ctx, BASE + (4 << 16)), g.make_tensor(g.TYPE_F16, n_ctx, kvw, BASE + (5 << 16)),
            g.make_tensor(g.TYPE_F32, hd, n_ctx, BASE + (6 << 16)), g.make_tensor(cells_type, T, 1, BASE + (7 << 16)),
            g.make_tensor(mask_type, n_ctx, T + 2, BASE + (8 << 16))]
    srcs = keep if mask else keep[:8]
    node = g.make_tensor(g.TYPE_F32, nh * hd, T, BASE + (9 << 16), op=g.OP_ATTN_BATCH, srcs=srcs,
                         op_params=[nh, nkv, hd, g.f32_bits(0.125), n_kv])
    return node, keep


def test_supports_op_attn_batch():
    assert g.MAX_SRC == 10
    for kw in (dict(), dict(mask_type=g.TYPE_F32, cells_type=g.TYPE_I32), dict(hd=128, nh=2, nkv=2),
               dict(n_ctx=128, n_kv=32), dict(T=1)):
        node, keep = batch_node(**kw)
        assert g.supports_op(node), kw
    for kw in (dict(mask=False), dict(mask_type=g.TYPE_I32), dict(hd=96), dict(n_kv=40), dict(n_kv=128),
               dict(cells_type=g.TYPE_F32)):
        node, keep = batch_node(**kw)
        assert not g.supports_op(node), kw


# ---------------------------------------------------------------- cells_match (adapter header)
CELLS_MATCH_MAIN = r'''
#include <cstdio>
#include <vector>
#include "mi355x_ggml_mirror.hpp"
using mi355x_adapter::cells_match;
int main() {
    const int64_t T = 3, kvw = 4, kv_size = 16;
    std::vector<int64_t> k = {5, 0, 15}, v((size_t)(T * kvw));
    for (int64_t i = 0; i < T; ++i)
        for (int64_t ch = 0; ch < kvw; ++ch) v[(size_t)(i * kvw + ch)] = ch * kv_size + k[(size_t)i];
    std::printf("match %d\n", (int)cells_match(k.data(), v.data(), T, kvw, kv_size));
    std::vector<int64_t> moved = v;
    moved[(size_t)(1 * kvw + 2)] += 1;  // one V entry of token 1 on another cell
    std::printf("moved %d\n", (int)cells_match(k.data(), moved.data(), T, kvw, kv_size));
    std::vector<int64_t> k2 = k, v2 = v;
    k2[2] = kv_size;  // a cell past the cache, its V entries consistent with it
    for (int64_t ch = 0; ch < kvw; ++ch) v2[(size_t)(2 * kvw + ch)] = ch * kv_size + k2[2];
    std::printf("outside %d\n", (int)cells_match(k2.data(), v2.data(), T, kvw, kv_size));
    k2[2] = -1;
    for (int64_t ch = 0; ch < kvw; ++ch) v2[(size_t)(2 * kvw + ch)] = ch * kv_size + k2[2];
    std::printf("negative %d\n", (int)cells_match(k2.data(), v2.data(), T, kvw, kv_size));
    std::printf("empty %d\n", (int)cells_match(k.data(), v.data(), 0, kvw, kv_size));
    std::printf("null %d\n", (int)cells_match(nullptr, v.data(), T, kvw, kv_size));
    return 0;
}
'''


def test_cells_match(tmp_path):
    """The promise behind mi355x_lower_opts.cells_from_graph on host copies of the two SET_ROWS
    index operands: a matching pair holds; one moved V entry, a cell >= kv_size (or < 0) and an
    empty batch do not."""
    src = tmp_path / "cells_match.cpp"
    src.write_text(CELLS_MATCH_MAIN)
    out = tmp_path / "cells_match"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ggml-neon-opt_amd", "adapter"), str(src), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(ln.split() for ln in r.stdout.splitlines())
    assert got == {"match": "1", "moved": "0", "outside": "0", "negative": "0", "empty": "0", "null": "0"}
