"""GPU: streamed attention (mi355x_attn_stream; csrc/kq_attn_stream.hip: kq_attn_stream_scores,
kq_attn_stream_softmax, kq_attn_stream_kqv), every comparison bit-exact.

Up to n_kv 8192 the reference is the oracle's kqo_attn_decode; past its 8192-entry arrays it is
tests/test_attn_stream_dispatch.composed_attn_decode, the same composition of the oracle's
primitives (checked equal to kqo_attn_decode on the CPU there). The KQV ring holds 3 stages of
512 cells per wave, so the 2080-cell sweep crosses 4 chunk boundaries (ring depth + 1) with every
partial last chunk a multiple of 32 cells can leave."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_attn_stream_dispatch import composed_attn_decode
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "adapter", "bin", "longctx_test")
STREAM_KERNELS = ("kq_attn_stream_scores", "kq_attn_stream_softmax", "kq_attn_stream_kqv")


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


@pytest.fixture
def stream_mode():
    """Sets mi355x_attn_stream for one test and puts the previous mode back."""
    import ggml_mi355x as g
    prev = []

    def set_mode(mode):
        p = g.attn_stream(mode)
        assert p >= 0
        if not prev:
            prev.append(p)
    yield set_mode
    if prev:
        g.attn_stream(prev[0])


def rand_caches(rng, n_ctx, kvw):
    kc = rng.standard_normal((n_ctx, kvw), dtype=np.float32).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((kvw, n_ctx), dtype=np.float32).astype(np.float16).view(np.uint16)
    return kc, vc


def to_dev(a, dev):
    import torch
    return torch.from_numpy(a.view(np.int16).copy()).to(dev)


def scale_of(hd):
    return float(np.float32(1.0) / np.sqrt(np.float32(hd)))


def reference(O, q, k, v, kc_ref, vc_ref, p, nh, nkv, hd, tref):
    """kqo_attn_decode where its arrays hold n_kv, the composed form past them"""
    qr, kr = O.rope(q, hd, hd, p, tref), O.rope(k, hd, hd, p, tref)
    if O.attn_n_kv(p, kc_ref.shape[0]) <= 8192:
        return O.attn_decode(qr, kr, v, kc_ref, vc_ref, p, nh, nkv, hd, scale_of(hd))
    return composed_attn_decode(O, qr, kr, v, kc_ref, vc_ref, p, nh, nkv, hd, scale_of(hd))


def decode_positions(dev, O, hd, nh, nkv, n_ctx, positions, qscale, seed, rope_row=True, expect_stream=True):
    """Random caches, one decode step per position against the reference, caches compared after
    every step (the row and the column of the new cell, and everything at the end)."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(seed)
    kvw = nkv * hd
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    tref = O.rope_table(n_ctx, hd, 10000.0)
    kc_ref, vc_ref = rand_caches(rng, n_ctx, kvw)
    kc, vc = to_dev(kc_ref, dev), to_dev(vc_ref, dev)
    for i, p in enumerate(positions):
        q = (rng.standard_normal(nh * hd) * qscale).astype(np.float32)
        k = (rng.standard_normal(kvw) * 2).astype(np.float32)
        v = rng.standard_normal(kvw).astype(np.float32)
        pos = torch.tensor([p], dtype=torch.int32, device=dev)
        if i == 0:
            g.timing_enable(True)
        got = g.attn_decode(t(q, dev), t(k, dev), t(v, dev), pos, tab[p].contiguous() if rope_row else tab, kc, vc,
                            nh, nkv, hd, scale_of(hd), rope_row=rope_row).cpu().numpy()
        if i == 0:
            names = [r[0] for r in g.timing_read()]
            g.timing_enable(False)
            assert all(any(k_ in n for n in names) for k_ in STREAM_KERNELS) == expect_stream, names
        ref = reference(O, q, k, v, kc_ref, vc_ref, p, nh, nkv, hd, tref)
        assert bits_equal(got, ref), (p, first_mismatch(got, ref))
        assert (kc[p].cpu().numpy().view(np.uint16) == kc_ref[p]).all(), p
        assert (vc[:, p].cpu().numpy().view(np.uint16) == vc_ref[:, p]).all(), p
    assert (kc.cpu().numpy().view(np.uint16) == kc_ref).all()
    assert (vc.cpu().numpy().view(np.uint16) == vc_ref).all()


# ---------------------------------------------------------------- 1: forced sweep
@pytest.mark.parametrize("hd,nh,nkv", [(64, 2, 1), (128, 4, 1), (64, 6, 2)])
def test_forced_sweep_every_32_cells(dev, O, stream_mode, hd, nh, nkv):
    """Mode 2, n_ctx 2080 (a multiple of 32, not of 64), both caches fully random: one position per
    multiple of 32 of n_kv (31, 63, ..., 2079) plus 0, 32 and 33 — every length the last ring
    chunk can have, 4 chunk boundaries (512, 1024, 1536, 2048: ring depth 3 + 1), the 32-cell
    last score chunk; group sizes 2, 4 and 3."""
    import ggml_mi355x as g
    n_ctx = 2080
    stream_mode(2)
    assert g.attn_path(n_ctx, nh, nkv, hd) == g.ATTN_PATH_STREAM
    positions = sorted(set(range(31, n_ctx, 32)) | {0, 32, 33})
    assert positions[-1] == n_ctx - 1 and len(positions) == 68
    decode_positions(dev, O, hd, nh, nkv, n_ctx, positions, 2.0, 2080 + hd + nh, rope_row=(hd == 64))


# ---------------------------------------------------------------- 2: same bits as today's paths
@pytest.mark.parametrize("hd,nh,nkv,n_ctx", [(64, 32, 4, 4096), (128, 32, 8, 2048)])
def test_mode2_equals_mode0(dev, stream_mode, hd, nh, nkv, n_ctx):
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(n_ctx + hd)
    kvw = nkv * hd
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    kc0, vc0 = rand_caches(rng, n_ctx, kvw)
    caches = {m: (to_dev(kc0, dev), to_dev(vc0, dev)) for m in (0, 2)}
    for p in (0, 255, 1023, n_ctx - 1):
        q = t((rng.standard_normal(nh * hd) * 2).astype(np.float32), dev)
        k = t((rng.standard_normal(kvw) * 2).astype(np.float32), dev)
        v = t(rng.standard_normal(kvw).astype(np.float32), dev)
        pos = torch.tensor([p], dtype=torch.int32, device=dev)
        out = {}
        for m in (0, 2):
            stream_mode(m)
            assert (g.attn_path(n_ctx, nh, nkv, hd) == g.ATTN_PATH_STREAM) == (m == 2)
            out[m] = g.attn_decode(q, k, v, pos, tab[p].contiguous(), caches[m][0], caches[m][1], nh, nkv, hd,
                                   scale_of(hd), rope_row=True).cpu().numpy()
        assert np.isfinite(out[0]).all()
        assert bits_equal(out[2], out[0]), (p, first_mismatch(out[2], out[0]))
    assert torch.equal(caches[0][0], caches[2][0]) and torch.equal(caches[0][1], caches[2][1])


# ---------------------------------------------------------------- 3: soft_max's sum
@pytest.mark.parametrize("qscale", [0.05, 2.0, 40.0], ids=["flat", "normal", "peaked"])
def test_softmax_sum_tree_and_fallback(dev, O, stream_mode, qscale):
    """Flat scores (every group sum ~4: the exact tree), N(0, 2) scores (both sides of its bound)
    and very peaked ones (group sums far below the bound, exact zeros: the in-order sum over all
    groups, recomputed from the workspace), as tests/test_gpu_ops.py does for the other kernels."""
    stream_mode(2)
    decode_positions(dev, O, 64, 8, 2, 4096, [0, 37, 300, 1500, 2047, 3000, 4095], qscale, int(qscale * 100) + 7,
                     rope_row=False)


# ---------------------------------------------------------------- 4: past the wall
@pytest.mark.parametrize("hd,nh,nkv", [(64, 8, 2), (128, 8, 2)])
def test_mode1_8192_cells(dev, O, stream_mode, hd, nh, nkv):
    stream_mode(1)
    decode_positions(dev, O, hd, nh, nkv, 8192, [0, 33, 5000, 8159, 8160, 8191], 2.0, 8192 + hd)


@pytest.mark.parametrize("n_ctx", [16384, 32768])
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 4, 1)])
def test_mode1_past_8192_cells(dev, O, stream_mode, hd, nh, nkv, n_ctx):
    stream_mode(1)
    positions = [0, 8191, 8192, 8193, n_ctx // 2 + 7, n_ctx - 33, n_ctx - 1]
    decode_positions(dev, O, hd, nh, nkv, n_ctx, positions, 2.0, n_ctx + hd)


def test_mode1_16384_cells_peaked(dev, O, stream_mode):
    """q scaled by 40 over 16384 cells: the in-order sum over 4096 groups"""
    stream_mode(1)
    decode_positions(dev, O, 64, 4, 2, 16384, [16383], 40.0, 40)


def test_mode1_131072_cells(dev, O, stream_mode):
    """The largest cache: offsets of kvw * n_ctx * 2 = 32 MiB per cache here, cell and workspace
    indices past 2^16 in every kernel, 256 ring chunks per wave."""
    stream_mode(1)
    decode_positions(dev, O, 128, 2, 1, 131072, [100000, 131071], 2.0, 131072)


def test_default_still_refuses_long_caches(dev):
    import torch
    import ggml_mi355x as g
    assert g.attn_stream(0) == 0  # the default
    hd, nh, nkv, n_ctx = 64, 4, 2, 16384
    x = torch.ones(nh * hd, device=dev)
    tab = g.rope_table(n_ctx, hd, device=dev)
    kc = torch.zeros((n_ctx, nkv * hd), dtype=torch.int16, device=dev)
    vc = torch.zeros((nkv * hd, n_ctx), dtype=torch.int16, device=dev)
    with pytest.raises(g.Mi355xError):
        g.attn_decode(x, x[: nkv * hd], x[: nkv * hd], torch.tensor([5], dtype=torch.int32, device=dev), tab, kc, vc,
                      nh, nkv, hd, 0.125)


# ---------------------------------------------------------------- 5: positions outside the cache
@pytest.mark.parametrize("mode,n_ctx", [(1, 16384), (2, 256)])
@pytest.mark.parametrize("bad_pos", ["n_ctx", "-1"])
def test_bad_position_gives_nan_and_leaves_the_caches(dev, stream_mode, mode, n_ctx, bad_pos):
    import torch
    import ggml_mi355x as g
    hd, nh, nkv = 64, 4, 2
    stream_mode(mode)
    assert g.attn_path(n_ctx, nh, nkv, hd) == g.ATTN_PATH_STREAM
    rng = np.random.default_rng(n_ctx)
    kc0, vc0 = rand_caches(rng, n_ctx, nkv * hd)
    kc, vc = to_dev(kc0, dev), to_dev(vc0, dev)
    tab = g.rope_table(n_ctx, hd, device=dev)
    x = torch.ones(nh * hd, device=dev)
    p = n_ctx if bad_pos == "n_ctx" else -1
    out = g.attn_decode(x, x[: nkv * hd], x[: nkv * hd], torch.tensor([p], dtype=torch.int32, device=dev), tab, kc, vc,
                        nh, nkv, hd, 0.125)
    assert torch.isnan(out).all()
    assert (kc.cpu().numpy().view(np.uint16) == kc0).all() and (vc.cpu().numpy().view(np.uint16) == vc0).all()


# ---------------------------------------------------------------- 6: prompt
def prompt_equals_decode(dev, hd, nh, nkv, n_ctx, start, T, decode_mode, prompt_mode, tiles, seed):
    """attn_prompt under prompt_mode (once per ATTN_STREAM_TILE value) against attn_decode under
    decode_mode token by token, on the same random caches: outputs and both caches."""
    import torch
    import ggml_mi355x as g
    rng = np.random.default_rng(seed)
    kvw = nkv * hd
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    kc0, vc0 = rand_caches(rng, n_ctx, kvw)
    q = t((rng.standard_normal((T, nh * hd)) * 2).astype(np.float32), dev)
    k = t((rng.standard_normal((T, kvw)) * 2).astype(np.float32), dev)
    v = t(rng.standard_normal((T, kvw)).astype(np.float32), dev)
    pos = torch.arange(start, start + T, dtype=torch.int32, device=dev)
    prev = g.attn_stream(decode_mode)
    try:
        kc, vc = to_dev(kc0, dev), to_dev(vc0, dev)
        want = torch.stack([g.attn_decode(q[i], k[i], v[i], pos[i:i + 1], tab, kc, vc, nh, nkv, hd, scale_of(hd))
                            for i in range(T)]).cpu().numpy()
        assert np.isfinite(want).all()
        g.attn_stream(prompt_mode)
        for tile in tiles:
            kc2, vc2 = to_dev(kc0, dev), to_dev(vc0, dev)
            g.debug_knob("ATTN_STREAM_TILE", tile)
            g.timing_enable(True)
            try:
                got = g.attn_prompt(q, k, v, pos, tab, kc2, vc2, nh, nkv, hd, scale_of(hd)).cpu().numpy()
                names = [r[0] for r in g.timing_read()]
            finally:
                g.timing_enable(False)
                g.debug_knob("ATTN_STREAM_TILE")
            n_tiles = (T + tile - 1) // tile if tile else 1
            assert sum("kq_attn_stream_kqv" in n for n in names) == n_tiles, names
            assert sum("kq_kv_store" in n for n in names) == 1, names
            for i in range(T):
                assert bits_equal(got[i], want[i]), (tile, i, first_mismatch(got[i], want[i]))
            assert torch.equal(kc, kc2) and torch.equal(vc, vc2), tile
    finally:
        g.attn_stream(prev)


def test_prompt_tiles_equal_decode(dev):
    """Mode 2, 512 cells, 40 tokens at 100: one tile (0: by the workspace cap) and 6 tiles of 7"""
    prompt_equals_decode(dev, 64, 8, 2, 512, 100, 40, 0, 2, (0, 7), 512)
    prompt_equals_decode(dev, 128, 4, 1, 512, 100, 40, 0, 2, (7,), 513)


def test_prompt_past_the_wall_equals_decode(dev):
    """Mode 1, 8192 cells, 40 tokens at 8120 on random caches: equal to mode-1 attn_decode"""
    prompt_equals_decode(dev, 64, 8, 2, 8192, 8120, 40, 1, 1, (0,), 8192)


# ---------------------------------------------------------------- 7: the decode graph
HP_ARGS = (512, 2, 8, 2, 768, 1024)  # n_embd, n_layer, n_head, n_head_kv, n_ff, n_vocab (head_dim 64)


def fill_caches(dec, cache, seed):
    """The same random f16 bits in a LlamaDecoder's caches and (where given) the oracle's"""
    import torch
    rng = np.random.default_rng(seed)
    for i in range(len(dec.k_cache)):
        kc, vc = rand_caches(rng, dec.k_cache[i].shape[0], dec.k_cache[i].shape[1])
        dec.k_cache[i].copy_(torch.from_numpy(kc.view(np.int16)))
        dec.v_cache[i].copy_(torch.from_numpy(vc.view(np.int16)))
        if cache is not None:
            cache[i][0][:] = kc
            cache[i][1][:] = vc
    torch.cuda.synchronize()


def test_decode_graph_8192_cells(dev, O, stream_mode):
    """A 2-layer LlamaDecoder over 8192-cell random caches, mode 1, captured graph (the backend
    reserves the workspace before it captures): steps bit-exact with the oracle's decode_token, and
    a 40-token prompt at 8120 equal to the steps, logits and both caches."""
    import torch
    import ggml_mi355x as g
    from tests import llama_model as LM
    from ggml_mi355x.llama import LlamaDecoder, hparams
    hp = hparams(*HP_ARGS)
    n_ctx = 8192
    stream_mode(1)
    w = LM.build(hp, 81)
    wd = LM.to_device(w, dev)
    b = g.Backend()
    try:
        dec = LlamaDecoder(b, hp, wd, n_ctx, fuse=True)
        model, cache = LM.oracle_model(hp, w, n_ctx)
        fill_caches(dec, cache, 8)
        for i, (p, tok) in enumerate([(0, 3), (5, 1000), (8000, 17), (8190, 500), (8191, 7)]):
            dec.step(tok, p, use_graph=True)
            b.synchronize()
            ref, _ = O.decode_token(model, tok, p, cache)
            got = dec.logits.cpu().numpy()
            assert bits_equal(got, ref), (p, first_mismatch(got, ref))
        for i in range(hp["n_layer"]):
            assert (dec.k_cache[i].cpu().numpy().view(np.uint16) == cache[i][0]).all()
            assert (dec.v_cache[i].cpu().numpy().view(np.uint16) == cache[i][1]).all()
        # the prompt against the steps
        tokens = np.random.default_rng(40).integers(0, hp["n_vocab"], size=40).tolist()
        fill_caches(dec, None, 9)
        for j, tok in enumerate(tokens):
            dec.step(tok, 8120 + j, use_graph=True)
        b.synchronize()
        want = dec.logits.cpu().numpy().copy()
        kcs = [c.clone() for c in dec.k_cache]
        vcs = [c.clone() for c in dec.v_cache]
        fill_caches(dec, None, 9)
        lg = dec.prompt(tokens, 8120, use_graph=True)
        b.synchronize()
        got = lg.cpu().numpy().reshape(-1)
        assert np.isfinite(want).all()
        assert bits_equal(got, want.reshape(-1)), first_mismatch(got, want.reshape(-1))
        for i in range(hp["n_layer"]):
            assert torch.equal(dec.k_cache[i], kcs[i]) and torch.equal(dec.v_cache[i], vcs[i]), i
    finally:
        b.close()


def test_decode_graph_16384_cells(dev, O, stream_mode):
    """16384 cells: positions 0 and 8100 against the oracle (n_kv <= 8192), position 16383 with
    graph replay == eager and fused == unfused."""
    import ggml_mi355x as g
    from tests import llama_model as LM
    from ggml_mi355x.llama import LlamaDecoder, hparams
    hp = hparams(*HP_ARGS)
    n_ctx = 16384
    stream_mode(1)
    w = LM.build(hp, 163)
    wd = LM.to_device(w, dev)
    outs = {}
    for fuse in (True, False):
        b = g.Backend()
        try:
            dec = LlamaDecoder(b, hp, wd, n_ctx, fuse=fuse)
            model, cache = LM.oracle_model(hp, w, n_ctx)
            fill_caches(dec, cache, 16)
            if fuse:
                for p, tok in ((0, 11), (8100, 900)):
                    dec.step(tok, p, use_graph=True)
                    b.synchronize()
                    ref, _ = O.decode_token(model, tok, p, cache)
                    got = dec.logits.cpu().numpy()
                    assert bits_equal(got, ref), (p, first_mismatch(got, ref))
                fill_caches(dec, None, 16)
            for tag, use_graph in (("eager", False), ("capture", True), ("replay", True)):
                dec.step(77, n_ctx - 1, use_graph=use_graph)
                b.synchronize()
                outs[(fuse, tag)] = dec.logits.cpu().numpy().copy()
        finally:
            b.close()
    base = outs[(True, "eager")]
    assert np.isfinite(base).all()
    for key, got in outs.items():
        assert bits_equal(got, base), (key, first_mismatch(got, base))


# ---------------------------------------------------------------- 8: the ggml-backend option
ADAPTER_TOKENS = [7, 1000, 123, 1]
ADAPTER_POSITIONS = [0, 1, 8190, 8191]


@pytest.fixture(scope="module")
def adapter_files(tmp_path_factory):
    from tests.test_adapter import glue_inputs
    from ggml_mi355x.llama import hparams
    hp = hparams(*HP_ARGS)
    argv, w = glue_inputs(tmp_path_factory.mktemp("longctx"), hp, 8192, 43, ADAPTER_TOKENS)
    return hp, argv, w


def test_adapter_long_context_off_is_refused(dev, adapter_files):
    hp, argv, w = adapter_files
    assert os.path.exists(HARNESS), "tests/adapter/bin/longctx_test missing: run __graft_entry__.build()"
    r = subprocess.run([HARNESS] + argv + ["off", ",".join(map(str, ADAPTER_POSITIONS))], capture_output=True, text=True,
                       timeout=200)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "proc ok" in r.stdout and "refused -1" in r.stdout and "token" not in r.stdout


def test_adapter_long_context_on_computes(dev, adapter_files, stream_mode):
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder
    from tests import llama_model as LM
    hp, argv, w = adapter_files
    assert os.path.exists(HARNESS), "tests/adapter/bin/longctx_test missing: run __graft_entry__.build()"
    r = subprocess.run([HARNESS] + argv + ["on", ",".join(map(str, ADAPTER_POSITIONS))], capture_output=True, text=True,
                       timeout=200)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "proc ok" in r.stdout and "refused" not in r.stdout
    got = np.fromfile(argv[3], np.float32).reshape(len(ADAPTER_TOKENS), hp["n_vocab"])
    stream_mode(1)
    b = g.Backend()
    try:
        dec = LlamaDecoder(b, hp, LM.to_device(w, dev), 8192)
        for i, (tok, p) in enumerate(zip(ADAPTER_TOKENS, ADAPTER_POSITIONS)):
            dec.step(tok, p)
            b.synchronize()
            want = dec.logits.cpu().numpy()
            assert np.isfinite(want).all()
            assert bits_equal(got[i], want), (p, first_mismatch(got[i], want))
    finally:
        b.close()
