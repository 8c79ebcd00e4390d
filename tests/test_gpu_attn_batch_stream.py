"""GPU: the streamed form of mi355x_attn_batch (csrc/kq_attn_stream.hip: kq_attn_stream_scores /
_softmax / _kqv in their batch instantiations, after kq_kv_store_batch), selected by
mi355x_attn_stream: bit for bit against the oracle-composed reference of
tests/test_gpu_attn_batch.py (ref_attn_batch) and, wherever kq_attn_batch runs the descriptor too,
against kq_attn_batch itself (mode 0), outputs and both caches.

The sizes are the smallest at which each mechanism can go wrong: launch A works in 64-cell
chunks (the last may hold 32), launch C in 512-cell ring stages, two of them issued by the
prologue and three in the ring, so 1568 cells (3 stages + 32 cells) wrap it; the stage skip works
on whole stages of 16 block flags. Past the wall (8192 cells, 7616 at head_dim 64, 7040 at 128)
only the reference remains."""
import numpy as np
import pytest

from tests.test_gpu_attn_batch import NEG, Setup, out_equal, vis_mask
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

SHAPES = [(64, 4, 2), (128, 2, 2), (64, 8, 1)]  # hd, nh, nkv
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


def device_run(s, kc, vc, q, k, v, pos, cells, mask, n_kv, mask_dtype=np.float32, cells_dtype=np.int32, row_pad=0,
               t_pad=0):
    """The device side of Setup.run on the given caches (no reference)."""
    import torch
    import ggml_mi355x as g
    T = len(pos)
    m = np.full((T + t_pad, n_kv + row_pad), 3.0, mask_dtype)
    m[:T, :n_kv] = np.asarray(mask, np.float32).astype(mask_dtype)
    got = g.attn_batch(t(q, s.dev), t(k, s.dev), t(v, s.dev), t(np.asarray(pos, np.int32), s.dev),
                       t(np.asarray(cells, cells_dtype), s.dev), t(m, s.dev), s.tab, kc, vc, s.nh, s.nkv, s.hd, s.scale,
                       n_kv)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def streamed_vs_both(s, stream_mode, q, k, v, pos, cells, mask, n_kv, mode=2, **kw):
    """One batch under `mode` (which must take the streamed form) against the reference, and against
    kq_attn_batch (mode 0) on a copy of the caches. Returns the streamed output."""
    import torch
    import ggml_mi355x as g
    kc0, vc0 = s.kc.clone(), s.vc.clone()
    stream_mode(mode)
    assert g.attn_batch_path(s.n_ctx, s.nh, s.nkv, s.hd, n_kv) == g.ATTN_PATH_STREAM
    g.timing_enable(True)
    try:
        got, ref = s.run(q, k, v, pos, cells, mask, n_kv, **kw)
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
    assert all(any(k_ in n for n in names) for k_ in STREAM_KERNELS), names
    assert sum("kq_kv_store_batch" in n for n in names) == 1 and not any("kq_attn_batch" in n for n in names), names
    assert out_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()
    stream_mode(0)
    assert g.attn_batch_path(s.n_ctx, s.nh, s.nkv, s.hd, n_kv) in (g.ATTN_GROUP, g.ATTN_HEAD)
    want = device_run(s, kc0, vc0, q, k, v, pos, cells, mask, n_kv, **kw)
    assert out_equal(got, want), first_mismatch(got, want)
    assert torch.equal(kc0, s.kc) and torch.equal(vc0, s.vc)
    return got


# ---------------------------------------------------------------- 1: row lengths
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
@pytest.mark.parametrize("n_kv", [32, 64, 96, 512, 544, 1056, 1568])
def test_row_length_sweep(dev, O, stream_mode, hd, nh, nkv, n_kv):
    """n_kv = n_ctx: one 32-cell chunk, one whole chunk, a whole and a 32-cell one, the first ring
    stage's edge on both sides, the end of the prologue's two stages, and 3 stages + 32 cells (the
    ring wraps). Sequence A holds the even cells, B the odd ones; T = 3 (A's and B's newest tokens
    and one of A in the middle of the cache)."""
    s = Setup(dev, O, hd, nh, nkv, n_kv, 1100 + hd + nh + n_kv, cache="random")
    mid = 2 * (n_kv // 4)
    cells = [n_kv - 2, n_kv - 1, mid]
    rows = [range(0, n_kv, 2), range(1, n_kv, 2), range(0, mid + 1, 2)]
    q, k, v = s.qkv(3)
    got = streamed_vs_both(s, stream_mode, q, k, v, [n_kv // 2 - 1, 7, mid // 2], cells, vis_mask(3, n_kv, rows), n_kv)
    assert np.isfinite(got).all()


# ---------------------------------------------------------------- 2: nothing past the row
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
@pytest.mark.parametrize("n_kv", [32, 64])
def test_nothing_outside_the_row_is_read(dev, O, stream_mode, hd, nh, nkv, n_kv):
    """n_kv < n_ctx = 128 with every K and V entry of the cells >= n_kv an f16 NaN (0x7e00): the
    output stays finite and equal to the reference, so nothing past n_kv is read. The hidden
    cells inside [0, n_kv) hold large finite values (|x| about 1e3) that must not leak."""
    n_ctx, T = 128, 3
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 400 + hd + n_kv, cache="random")
    cells = [3, n_kv - 1, 17]
    seen = sorted({1, 2, 3, 8, 16, 17, 20, n_kv - 2, n_kv - 1})
    hidden = [c for c in range(n_kv) if c not in seen]
    big = (s.rng.choice([-1.0, 1.0], size=(len(hidden), s.kvw)) * s.rng.uniform(900.0, 1100.0, (len(hidden), s.kvw)))
    s.kc_ref[hidden] = big.astype(np.float16).view(np.uint16)
    s.vc_ref[:, hidden] = big.T.astype(np.float16).view(np.uint16)
    s.kc_ref[n_kv:] = 0x7e00
    s.vc_ref[:, n_kv:] = 0x7e00
    s.upload()
    q, k, v = s.qkv(T, qs=0.25)
    got = streamed_vs_both(s, stream_mode, q, k, v, [5, 6, 7], cells, vis_mask(T, n_kv, [seen] * T), n_kv)
    assert np.isfinite(got).all()


# ---------------------------------------------------------------- 3: mask forms, cell types
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
@pytest.mark.parametrize("mask_dtype,cells_dtype", [(np.float32, np.int32), (np.float16, np.int64),
                                                    (np.float32, np.int64), (np.float16, np.int32)],
                         ids=["f32-i32", "f16-i64", "f32-i64", "f16-i32"])
def test_mask_forms_and_cell_types(dev, O, stream_mode, hd, nh, nkv, mask_dtype, cells_dtype):
    """F16 and F32 masks whose row stride is larger than the row and which have more rows than
    tokens, with finite non-zero entries (-1.5 and +0.75, exact in f16) among the zeros — the
    mask is added to dot * scale, not tested for visibility — and I32 / I64 cell indices."""
    n_ctx, T = 64, 4
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 600 + hd + nh, cache="random")
    cells = [9, 33, 2, 50]
    mask = vis_mask(T, n_ctx, [range(0, 40), range(20, 64), [2, 3, 5, 60], range(64)])
    mask[0, 4] = mask[1, 33] = mask[3, 10] = -1.5
    mask[0, 9] = mask[1, 40] = mask[2, 5] = mask[3, 63] = 0.75
    q, k, v = s.qkv(T)
    streamed_vs_both(s, stream_mode, q, k, v, [0, 7, 3, 44], cells, mask, n_ctx, mask_dtype=mask_dtype,
                     cells_dtype=cells_dtype, row_pad=24, t_pad=3)


# ---------------------------------------------------------------- 4: a token without a cell
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
def test_out_of_range_cell(dev, O, stream_mode, hd, nh, nkv):
    """A cell outside [0, n_ctx) (or a position outside the rope table): that token's output row
    is all NaN, no cache byte changes for it, and the other tokens equal the reference."""
    n_ctx, T = 64, 5
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 900 + hd, cache="random")
    cells = [4, n_ctx + 5, 9, -1, 20]
    pos = [0, 1, 2, 3, n_ctx]
    mask = vis_mask(T, n_ctx, [range(0, 10), range(0, 10), range(5, 30), range(64), range(64)])
    q, k, v = s.qkv(T)
    got = streamed_vs_both(s, stream_mode, q, k, v, pos, cells, mask, n_ctx)
    assert np.isnan(got[[1, 3, 4]]).all() and np.isfinite(got[[0, 2]]).all()


# ---------------------------------------------------------------- 5: hidden chunks and stages
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_hidden_chunks_and_stages(dev, O, stream_mode, hd, nh, nkv):
    """n_kv = 1568: stages [0, 512), [512, 1024), [1024, 1536) and the 32-cell stage 3. Row 0:
    whole 64-cell chunks hidden (1, 10, 11 and the last, 32-cell one) inside visible stages. Row 1:
    stage 1 hidden. Row 2: stages 0 and 2 hidden. Row 3: stage 0, then one visible cell (the
    token's own) in the otherwise hidden stage 2, stages 1 and 3 hidden. Row 4: every cell. The
    hidden chunks' K rows and the hidden stages' V rows are not loaded; the bits are the
    reference's, which adds their exact zeros."""
    n_kv = n_ctx = 1568
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 1500 + hd + nh, cache="random")
    rows = [list(range(0, 64)) + list(range(128, 640)) + list(range(768, 1536)),
            list(range(0, 512)) + list(range(1024, 1568)),
            list(range(512, 1024)) + list(range(1536, 1568)),
            list(range(0, 512)) + [1024 + 17],
            list(range(n_kv))]
    cells = [5, 1567, 700, 1024 + 17, 1000]
    q, k, v = s.qkv(5)
    got = streamed_vs_both(s, stream_mode, q, k, v, [9, 40, 200, 3, 1500], cells, vis_mask(5, n_kv, rows), n_kv)
    assert np.isfinite(got).all()


# ---------------------------------------------------------------- 6: the sign of a zero
@pytest.mark.parametrize("hd,nh,nkv", [(64, 2, 2), (128, 4, 2)])
def test_sign_of_zero_behind_a_skipped_stage(dev, O, stream_mode, hd, nh, nkv):
    """tests/test_gpu_attn_batch.py's test_sign_of_zero_behind_a_skipped_block at stage size, the
    one corner where leaving out a hidden stage's V rows could change a bit: an f16 KQV accumulator
    lane that is -0 when the stage is reached. Stage 0 (cells 0 .. 511) is visible with weight
    about 2^-13 (mask -9) on V = -2^-14: every product underflows to -0. Stage 1 (512 .. 1023) is
    hidden and holds +1 on the even channels (ggml's fma(+1, +0, -0) turns the lane into +0) and
    -1 on the odd ones (it stays -0). Stage 2 holds the token's own cell (V = -0) among hidden
    cells of -1, which keep either sign. The reference gives +0.0 on the even channels and -0.0 on
    the odd ones, and so must the kernel, which does not load stage 1 in its first pass."""
    n_kv = n_ctx = 1056
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 1000 + hd)
    s.vc_ref[:, 0:512] = 0x8400
    s.vc_ref[0::2, 512:1024] = 0x3c00
    s.vc_ref[1::2, 512:1024] = 0xbc00
    s.vc_ref[:, 1025:1056] = 0xbc00
    s.upload()
    mask = np.full((1, n_kv), NEG, np.float32)
    mask[0, 0:512] = -9.0
    mask[0, 1024] = 0.0
    q = np.ones((1, nh * hd), np.float32)
    k = np.zeros((1, s.kvw), np.float32)
    v = np.full((1, s.kvw), -0.0, np.float32)
    stream_mode(2)
    got, ref = s.run(q, k, v, [0], [1024], mask, n_kv)
    bits = ref.view(np.uint32).reshape(nh, hd)
    assert (bits[:, 0::2] == 0).all() and (bits[:, 1::2] == 0x80000000).all()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all(), first_mismatch(got, ref)
    assert s.caches_equal()


# ---------------------------------------------------------------- 7: soft_max's sum
@pytest.mark.parametrize("qscale", [0.05, 2.0, 40.0], ids=["flat", "normal", "peaked"])
def test_softmax_sum_tree_and_fallback(dev, O, stream_mode, qscale):
    """4096 cells (every thread of launch B owns one group of four): flat scores (every group sum
    about 4: the exact tree), N(0, 2) ones (both sides of its bound) and very peaked ones (group
    sums far below the bound, exact zeros: the in-order sum over all groups, recomputed from the
    workspace), as tests/test_gpu_attn_stream.py does for decode. Row 0 sees every cell, row 1 the
    odd cells of [1024, 3072)."""
    hd, nh, nkv, n_kv = 64, 4, 2, 4096
    s = Setup(dev, O, hd, nh, nkv, n_kv, int(qscale * 100) + 7, cache="random")
    q, k, v = s.qkv(2, qs=qscale)
    rows = [range(n_kv), range(1025, 3072, 2)]
    got = streamed_vs_both(s, stream_mode, q, k, v, [4000, 11], [4095, 2001], vis_mask(2, n_kv, rows), n_kv)
    assert np.isfinite(got).all()


# ---------------------------------------------------------------- 8: token tiles
@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
def test_token_tiles(dev, O, stream_mode, hd, nh, nkv):
    """T = 5 in tiles of 2 tokens (ATTN_STREAM_TILE: 3 tiles, the last of one token, each with its
    own rows of the workspace and its own block flags) equals the run in one tile and the
    reference; the cells are stored once, before the first tile."""
    import torch
    import ggml_mi355x as g
    n_kv = n_ctx = 544
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 800 + hd, cache="random")
    cells = [540, 3, 541, 100, 543]
    rows = [range(0, 541, 2), [1, 3], range(1, 542, 2), range(64, 128), range(n_kv)]
    mask = vis_mask(5, n_kv, rows)
    q, k, v = s.qkv(5)
    kc0, vc0 = s.kc.clone(), s.vc.clone()
    stream_mode(2)
    g.debug_knob("ATTN_STREAM_TILE", 2)
    g.timing_enable(True)
    try:
        got, ref = s.run(q, k, v, [300, 1, 301, 50, 543], cells, mask, n_kv)
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
        g.debug_knob("ATTN_STREAM_TILE")
    assert sum("kq_attn_stream_kqv" in n for n in names) == 3 and sum("kq_kv_store_batch" in n for n in names) == 1, names
    assert bits_equal(got, ref), first_mismatch(got, ref)
    g.timing_enable(True)
    try:
        one = device_run(s, kc0, vc0, q, k, v, [300, 1, 301, 50, 543], cells, mask, n_kv)
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
    assert sum("kq_attn_stream_kqv" in n for n in names) == 1, names
    assert bits_equal(got, one), first_mismatch(got, one)
    assert s.caches_equal() and torch.equal(kc0, s.kc) and torch.equal(vc0, s.vc)


# ---------------------------------------------------------------- 9: past the wall
def past_the_wall(dev, O, stream_mode, hd, nh, nkv, n_ctx, n_kv, pos, cells, rows, seed):
    import ggml_mi355x as g
    stream_mode(0)
    assert g.attn_batch_path(n_ctx, nh, nkv, hd, n_kv) == g.E_UNSUPPORTED
    stream_mode(1)
    assert g.attn_batch_path(n_ctx, nh, nkv, hd, n_kv) == g.ATTN_PATH_STREAM == 7
    assert g.attn_batch_path(64, nh, nkv, hd, 64) in (g.ATTN_GROUP, g.ATTN_HEAD)  # what runs today keeps its form
    s = Setup(dev, O, hd, nh, nkv, n_ctx, seed, cache="random")
    if n_kv < n_ctx:  # nothing at or past n_kv is read
        s.kc_ref[n_kv:] = 0x7e00
        s.vc_ref[:, n_kv:] = 0x7e00
        s.upload()
    T = len(pos)
    q, k, v = s.qkv(T)
    g.timing_enable(True)
    try:
        got, ref = s.run(q, k, v, pos, cells, vis_mask(T, n_kv, rows), n_kv)
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
    assert all(any(k_ in n for n in names) for k_ in STREAM_KERNELS), names
    assert np.isfinite(ref).all()
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()
    # the default refuses the launch as it refuses the descriptor
    stream_mode(0)
    with pytest.raises(g.Mi355xError):
        device_run(s, s.kc, s.vc, q, k, v, pos, cells, vis_mask(T, n_kv, rows), n_kv)
    assert s.caches_equal()


def test_past_the_wall_8224_cells_three_sequences(dev, O, stream_mode):
    """n_ctx = n_kv = 8224 (one block past 8192; 17 ring stages, the last of 32 cells), head_dim
    64, three sequences in the cells = 0, 1, 2 mod 3."""
    n = 8224
    cells = [8220, 8221, 8222]
    past_the_wall(dev, O, stream_mode, 64, 4, 2, n, n, [2740, 100, 2], cells, [range(j, cells[j] + 1, 3) for j in range(3)],
                  8224)


def test_past_the_wall_short_row_in_a_long_cache(dev, O, stream_mode):
    """n_ctx = 16384 with n_kv = 1056: refused today for the cache's size alone; the V rows are
    n_ctx apart, the workspace rows n_kv; f16 NaN in every cell at or past n_kv."""
    rows = [range(0, 1056, 2), list(range(1, 300, 2)) + [1055]]
    past_the_wall(dev, O, stream_mode, 64, 8, 1, 16384, 1056, [527, 16383], [1054, 1055], rows, 16384)


def test_past_the_wall_16416_cells_head_dim_128(dev, O, stream_mode):
    """n_ctx = n_kv = 16416 (33 stages, the last of 32 cells), head_dim 128, MHA, T = 2: one row
    over every cell, one over two far-apart stretches with whole hidden stages between them."""
    n = 16416
    rows = [range(n), list(range(100, 700)) + list(range(16000, n))]
    past_the_wall(dev, O, stream_mode, 128, 2, 2, n, n, [16000, 31], [16415, 16001], rows, 16416)


# ---------------------------------------------------------------- 10: the graph
G_CTX, G_SEQ, G_STEPS = 8224, 3, 2
G_BASE = [0, 4096, 8192]  # each sequence's first cell: whole 32-cell blocks apart (tests/test_gpu_batch_token.py)
G_TOKENS = [[7, 1000], [511, 3], [2, 777]]  # [sequence][step]


def test_step_batch_past_the_wall_equals_each_sequence_alone(dev, stream_mode):
    """A 2-layer model over one cache of 8224 cells, three sequences at cells 0, 4096 and 8192 on,
    mode 1: two step_batch calls (the second replays the captured hipGraph with new inputs; the
    backend reserved the workspace before it captured) equal LlamaDecoder.step of each sequence
    alone on a cache of the same size, also at mode 1 (the streamed decode kernels). The argument
    for equal bits is tests/test_gpu_batch_token.py's: the other sequences are whole hidden
    32-cell blocks."""
    import torch
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    hp = hparams(512, 2, 8, 2, 768, 1024)
    w = LM.build(hp, 77)
    wd = LM.to_device(w, dev)
    stream_mode(1)
    assert g.attn_batch_path(G_CTX, hp["n_head"], hp["n_head_kv"], hp["head_dim"], G_CTX) == g.ATTN_PATH_STREAM
    b = g.Backend()
    try:
        alone = LlamaDecoder(b, hp, wd, G_CTX)
        want = [[None] * G_SEQ for _ in range(G_STEPS)]
        for s in range(G_SEQ):
            for c in alone.k_cache + alone.v_cache:
                c.zero_()
            torch.cuda.synchronize()
            for p in range(G_STEPS):
                alone.step(G_TOKENS[s][p], p, use_graph=True)
                b.synchronize()
                want[p][s] = alone.logits.cpu().numpy().copy()
        dec = LlamaDecoder(b, hp, wd, G_CTX)
        for p in range(G_STEPS):
            mask = np.full((G_SEQ, G_CTX), -np.inf, np.float32)
            for s in range(G_SEQ):
                mask[s, G_BASE[s]:G_BASE[s] + p + 1] = 0.0
            lg = dec.step_batch([G_TOKENS[s][p] for s in range(G_SEQ)], [p] * G_SEQ, [G_BASE[s] + p for s in range(G_SEQ)],
                                mask, G_CTX, use_graph=True)
            b.synchronize()
            got = lg.cpu().numpy()
            for s in range(G_SEQ):
                assert np.isfinite(want[p][s]).all()
                assert bits_equal(got[s], want[p][s]), (p, s, first_mismatch(got[s], want[p][s]))
        assert len(dec._batches) == 1  # one graph, replayed
    finally:
        b.close()
