"""GPU: mi355x_attn_batch (csrc/kq_attn_batch.hip) — the attention block of a batch whose KV
cells and mask come from the caller (ggml's SET_ROWS + MUL_MAT + SOFT_MAX(mask) + MUL_MAT with a
unified cache: several sequences, or cells that are not positions) — bit for bit against a
reference composed of the oracle's pieces only (oracle/kq_ops_oracle.py): per token, in batch
order, rope at pos[i] and fp32_to_fp16 into the cache arrays at cell cells[i]; then per token
and head vec_dot_f16 over cells [0, n_kv), soft_max_row(kq, mask row, scale), fp32_to_fp16 and
vec_dot_f16(v_cache row[:n_kv], p16). The inputs stay inside what those pieces restate: every
mask row leaves its own cell visible, n_kv % 32 == 0, cache contents inside [0, n_kv) finite.
Every comparison is on the uint32 / uint16 bits."""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

NEG = -np.inf
HEADS = [(4, 2), (2, 2)]
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


@pytest.fixture(params=[0, 1], ids=["group", "head"])
def batch_form(request):
    """Runs a test on both forms of kq_attn_batch: one workgroup per (kv group, token), the default
    where the group's rows fit, and one per (query head, token), forced by mi355x_attn_prompt_impl."""
    import ggml_mi355x as g
    prev = g.attn_prompt_impl(request.param)
    yield request.param
    g.attn_prompt_impl(prev)


def batch_lds(hd, n_kv, rows):
    """attn_batch_lds of csrc/kq_attn_batch.hip: q16 | w | p16 | scal per row, the mask row, the block flags."""
    return rows * (2 * hd + 6 * n_kv + 16) + 4 * n_kv + 4 * (n_kv // 32)


def ref_attn_batch(O, q, k, v, pos, cells, mask, tref, kc, vc, nh, nkv, hd, scale, n_kv):
    """The reference (module docstring); kc [n_ctx, kvw] / vc [kvw, n_ctx] uint16, updated in
    place. A token whose cell or position is outside the cache stores nothing: a NaN row."""
    L = O.lib()
    T, kvw, n_ctx, gsz = len(pos), nkv * hd, kc.shape[0], nh // nkv
    ok = [0 <= int(pos[i]) < tref.shape[0] and 0 <= int(cells[i]) < n_ctx for i in range(T)]
    for i in range(T):
        if ok[i]:
            kc[int(cells[i])] = O.fp32_to_fp16(O.rope(k[i], hd, hd, int(pos[i]), tref))
            vc[:, int(cells[i])] = O.fp32_to_fp16(v[i])
    out = np.full((T, nh * hd), np.nan, np.float32)
    kq = np.empty(n_kv, np.float32)
    vrow = np.empty(n_kv, np.uint16)
    for i in range(T):
        if not ok[i]:
            continue
        q16 = O.fp32_to_fp16(O.rope(q[i], hd, hd, int(pos[i]), tref))
        mrow = np.ascontiguousarray(mask[i, :n_kv], np.float32)
        for h in range(nh):
            g = h // gsz
            qp = q16.ctypes.data + 2 * h * hd
            for c in range(n_kv):  # O.vec_dot_f16(kc[c, g*hd:(g+1)*hd], q16[h*hd:(h+1)*hd])
                kq[c] = L.kqo_vec_dot_f16(hd, kc.ctypes.data + 2 * (c * kvw + g * hd), qp)
            p16 = O.fp32_to_fp16(O.soft_max_row(kq, mrow, scale))
            for d in range(hd):
                vrow[:] = vc[g * hd + d, :n_kv]
                out[i, h * hd + d] = L.kqo_vec_dot_f16(n_kv, vrow.ctypes.data, p16.ctypes.data)
    return out


class Setup:
    """Device and host state of one shape: rope tables, both caches (host copies are the reference's)."""

    def __init__(self, dev, O, hd, nh, nkv, n_ctx, seed, cache=None):
        import torch
        import ggml_mi355x as g
        self.dev, self.O, self.hd, self.nh, self.nkv, self.n_ctx = dev, O, hd, nh, nkv, n_ctx
        self.kvw = nkv * hd
        self.rng = np.random.default_rng(seed)
        self.scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
        self.tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
        self.tref = O.rope_table(n_ctx, hd, 10000.0)
        if cache == "random":  # every cell finite and non-zero, not only the cells the test writes
            self.kc_ref = self.rng.standard_normal((n_ctx, self.kvw)).astype(np.float16).view(np.uint16)
            self.vc_ref = self.rng.standard_normal((self.kvw, n_ctx)).astype(np.float16).view(np.uint16)
        else:
            self.kc_ref = np.zeros((n_ctx, self.kvw), np.uint16)
            self.vc_ref = np.zeros((self.kvw, n_ctx), np.uint16)
        self.upload()

    def upload(self):
        import torch
        self.kc = torch.from_numpy(self.kc_ref.view(np.int16).copy()).to(self.dev)
        self.vc = torch.from_numpy(self.vc_ref.view(np.int16).copy()).to(self.dev)

    def qkv(self, T, qs=2.0, ks=2.0):
        r = self.rng
        return ((r.standard_normal((T, self.nh * self.hd)) * qs).astype(np.float32),
                (r.standard_normal((T, self.kvw)) * ks).astype(np.float32),
                r.standard_normal((T, self.kvw)).astype(np.float32))

    def run(self, q, k, v, pos, cells, mask, n_kv, mask_dtype=np.float32, cells_dtype=np.int32, row_pad=0, t_pad=0):
        """One batch on the device and through the reference; both caches advance. Returns (got, ref)."""
        import torch
        import ggml_mi355x as g
        T = len(pos)
        mask = np.asarray(mask, np.float32)
        assert mask.shape == (T, n_kv) and all(mask[i, cells[i]] != NEG for i in range(T) if 0 <= cells[i] < n_kv)
        # rows padded to a larger stride, more rows than tokens; the padding holds finite junk
        m = np.full((T + t_pad, n_kv + row_pad), 3.0, mask_dtype)
        m[:T, :n_kv] = mask.astype(mask_dtype)
        got = g.attn_batch(t(q, self.dev), t(k, self.dev), t(v, self.dev), t(np.asarray(pos, np.int32), self.dev),
                           t(np.asarray(cells, cells_dtype), self.dev), t(m, self.dev), self.tab, self.kc, self.vc,
                           self.nh, self.nkv, self.hd, self.scale, n_kv)
        torch.cuda.synchronize()
        ref = ref_attn_batch(self.O, q, k, v, pos, cells, m[:T, :n_kv].astype(np.float32), self.tref, self.kc_ref,
                             self.vc_ref, self.nh, self.nkv, self.hd, self.scale, n_kv)
        return got.cpu().numpy(), ref

    def caches_equal(self):
        return (self.kc.cpu().numpy().view(np.uint16) == self.kc_ref).all() and \
               (self.vc.cpu().numpy().view(np.uint16) == self.vc_ref).all()


def out_equal(got, ref):
    """Bit equality; NaN rows (a token without a cell) only need to be NaN in both."""
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool((gn == rn).all()) and bool((got.view(np.uint32)[~gn] == ref.view(np.uint32)[~rn]).all())


def vis_mask(T, n_kv, rows):
    """rows[i]: the visible cells of token i -> additive mask (0 visible, -inf hidden)."""
    m = np.full((T, n_kv), NEG, np.float32)
    for i, cs in enumerate(rows):
        m[i, list(cs)] = 0.0
    return m


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("T", [1, 5])
def test_one_sequence_equals_prompt_kernel(dev, O, hd, nh, nkv, T):
    """cells == pos under the causal mask over n_kv = n_ctx cells: output and both caches are
    mi355x_attn_prompt's on the same inputs (which runs each row over pad32(pos + 1) <= n_kv
    cells) and the reference's. The cells after a query's position hold finite junk."""
    import torch
    import ggml_mi355x as g
    n_ctx = 64
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 100 + hd + nh + T, cache="random")
    pos = list(range(20, 20 + T))
    q, k, v = s.qkv(T)
    kc2, vc2 = s.kc.clone(), s.vc.clone()
    want = g.attn_prompt(t(q, dev), t(k, dev), t(v, dev), t(np.asarray(pos, np.int32), dev), s.tab, kc2, vc2, nh, nkv,
                         hd, s.scale)
    got, ref = s.run(q, k, v, pos, pos, vis_mask(T, n_ctx, [range(p + 1) for p in pos]), n_ctx)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert bits_equal(got, want.cpu().numpy()), first_mismatch(got, want.cpu().numpy())
    assert s.caches_equal()
    assert torch.equal(s.kc, kc2) and torch.equal(s.vc, vc2)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_two_sequences_interleaved(dev, O, batch_form, hd, nh, nkv):
    """Sequence A holds the even cells, B the odd ones; positions differ from cells (A's
    token j at cell 2j has position j, B's at cell 2j + 1 has position 10 + j). The caches fill
    through earlier batches of one token per sequence; every batch, the last included, has two
    mask rows with no cell in common."""
    n_ctx = 64
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 200 + hd + nh)
    for j in range(6):
        q, k, v = s.qkv(2)
        rows = [range(0, 2 * j + 1, 2), range(1, 2 * j + 2, 2)]
        got, ref = s.run(q, k, v, [j, 10 + j], [2 * j, 2 * j + 1], vis_mask(2, n_ctx, rows), n_ctx)
        assert bits_equal(got, ref), (j, first_mismatch(got, ref))
    assert s.caches_equal()


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_shifted_cache(dev, O, batch_form, hd, nh, nkv):
    """One sequence whose cells are a shuffled subset of the cache (the cell is not monotone
    in the position), causal in the position, with the cell of position 3 hidden from every
    later token (a removed cell inside the visible range)."""
    n_ctx, T = 64, 10
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 300 + hd + nh, cache="random")
    cells = [41, 7, 55, 12, 0, 63, 30, 31, 32, 5]
    pos = list(range(T))
    rows = [[cells[p] for p in range(i + 1) if p != 3 or i == 3] for i in range(T)]
    q, k, v = s.qkv(T)
    got, ref = s.run(q, k, v, pos, cells, vis_mask(T, n_ctx, rows), n_ctx)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
@pytest.mark.parametrize("n_kv", [32, 64])
def test_nothing_outside_the_row_is_read(dev, O, batch_form, hd, nh, nkv, n_kv):
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
    got, ref = s.run(q, k, v, [5, 6, 7], cells, vis_mask(T, n_kv, [seen] * T), n_kv)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2), (64, 8, 2)])
def test_block_skipping(dev, O, batch_form, hd, nh, nkv):
    """n_kv = 288: 9 blocks of 32 cells, past one 256-thread stride. Row 0: blocks 0 and 2
    visible with block 1 fully hidden between them, nothing after block 2. Row 1: block 0, one
    single visible cell in block 4, and the start of block 8. Row 2: every cell. The hidden
    blocks' K rows and V chunks are not loaded; the bits are the reference's, which adds their
    exact zeros."""
    n_kv = n_ctx = 288
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 500 + hd + nh, cache="random")
    rows = [list(range(0, 32)) + list(range(64, 96)),
            list(range(0, 32)) + [4 * 32 + 17] + list(range(256, 271)),
            list(range(n_kv))]
    cells = [70, 4 * 32 + 17, 287]
    q, k, v = s.qkv(3)
    got, ref = s.run(q, k, v, [9, 40, 200], cells, vis_mask(3, n_kv, rows), n_kv)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()


@pytest.mark.parametrize("hd,nh,nkv", [(64, 2, 2), (128, 4, 2)])
def test_sign_of_zero_behind_a_skipped_block(dev, O, batch_form, hd, nh, nkv):
    """The one corner where leaving out a hidden block's V chunk could change a bit: an f16 KQV
    accumulator lane that is -0 when the block is reached. Block 0 is visible with weight about
    2^-13 (mask -9) on V = -2^-14: every product underflows to -0. Block 1 is hidden and holds
    +1 on the even channels (ggml's fma(+1, +0, -0) turns the lane into +0) and -1 on the odd
    ones (it stays -0). Block 2 holds the token's own cell (V = -0) among hidden cells of -1,
    which keep either sign. The reference gives +0.0 on the even channels and -0.0 on the odd
    ones, and so must the kernel, which does not load block 1."""
    n_kv = n_ctx = 96
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 1000 + hd)
    s.vc_ref[:, 0:32] = 0x8400
    s.vc_ref[0::2, 32:64] = 0x3c00
    s.vc_ref[1::2, 32:64] = 0xbc00
    s.vc_ref[:, 65:96] = 0xbc00
    s.upload()
    mask = np.full((1, n_kv), NEG, np.float32)
    mask[0, 0:32] = -9.0
    mask[0, 64] = 0.0
    q = np.ones((1, nh * hd), np.float32)
    k = np.zeros((1, s.kvw), np.float32)
    v = np.full((1, s.kvw), -0.0, np.float32)
    got, ref = s.run(q, k, v, [0], [64], mask, n_kv)
    bits = ref.view(np.uint32).reshape(nh, hd)
    assert (bits[:, 0::2] == 0).all() and (bits[:, 1::2] == 0x80000000).all()
    assert (got.view(np.uint32) == ref.view(np.uint32)).all(), first_mismatch(got, ref)
    assert s.caches_equal()


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
@pytest.mark.parametrize("mask_dtype,cells_dtype", [(np.float32, np.int32), (np.float16, np.int64),
                                                    (np.float32, np.int64), (np.float16, np.int32)],
                         ids=["f32-i32", "f16-i64", "f32-i64", "f16-i32"])
def test_mask_forms_and_cell_types(dev, O, hd, nh, nkv, mask_dtype, cells_dtype):
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
    got, ref = s.run(q, k, v, [0, 7, 3, 44], cells, mask, n_ctx, mask_dtype=mask_dtype, cells_dtype=cells_dtype,
                     row_pad=24, t_pad=3)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()


def test_cache_size_boundary_between_the_forms(dev, O):
    """The group form (one workgroup per kv group and token) keeps q16 | w | p16 | scal per query
    head of the group, the mask row and the block flags in LDS: rows * (2 hd + 6 n_kv + 16) +
    4 n_kv + n_kv / 8 bytes <= 160 KB. With 8 heads in the group and head_dim 64 the largest
    n_kv is 3104; 3136 takes the per-head form (one row). Both give the reference's bits; two
    sequences (even / odd cells), T = 4."""
    import ggml_mi355x as g
    hd, nh, nkv, T = 64, 8, 1, 4
    fits = [n for n in range(32, 8192, 32) if batch_lds(hd, n, nh // nkv) <= LDS_MAX]
    edge = fits[-1]
    assert edge == 3104 and batch_lds(hd, edge + 32, 1) <= LDS_MAX
    for n_kv, form in ((edge, g.ATTN_GROUP), (edge + 32, g.ATTN_HEAD)):
        assert g.attn_batch_path(n_kv, nh, nkv, hd, n_kv) == form
        s = Setup(dev, O, hd, nh, nkv, n_kv, 700 + n_kv, cache="random")
        cells = [n_kv - 2, 1000, n_kv - 1, 2001]
        rows = [range(0, n_kv, 2), range(0, 1001, 2), range(1, n_kv, 2), range(1001, 2002, 2)]
        q, k, v = s.qkv(T)
        got, ref = s.run(q, k, v, [900, 17, 5, 0], cells, vis_mask(T, n_kv, rows), n_kv)
        assert bits_equal(got, ref), (n_kv, first_mismatch(got, ref))
        assert s.caches_equal()


def test_group_of_more_than_eight_heads_takes_the_head_form(dev, O):
    import ggml_mi355x as g
    hd, nh, nkv, n_ctx = 64, 16, 1, 64
    assert g.attn_batch_path(n_ctx, nh, nkv, hd, n_ctx) == g.ATTN_HEAD
    assert g.attn_batch_path(n_ctx, 8, nkv, hd, n_ctx) == g.ATTN_GROUP
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 800, cache="random")
    q, k, v = s.qkv(2)
    got, ref = s.run(q, k, v, [4, 9], [40, 11], vis_mask(2, n_ctx, [range(30, 50), [0, 11, 63]]), n_ctx)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 2, 2)])
def test_out_of_range_cell(dev, O, batch_form, hd, nh, nkv):
    """A cell outside [0, n_ctx) (or a position outside the rope table): that token's output row
    is all NaN, no cache byte changes for it, and the other tokens equal the reference."""
    n_ctx, T = 64, 5
    s = Setup(dev, O, hd, nh, nkv, n_ctx, 900 + hd, cache="random")
    cells = [4, n_ctx + 5, 9, -1, 20]
    pos = [0, 1, 2, 3, n_ctx]
    mask = vis_mask(T, n_ctx, [range(0, 10), range(0, 10), range(5, 30), range(64), range(64)])
    q, k, v = s.qkv(T)
    got, ref = s.run(q, k, v, pos, cells, mask, n_ctx)
    assert np.isnan(got[[1, 3, 4]]).all() and np.isfinite(got[[0, 2]]).all()
    assert out_equal(got, ref), first_mismatch(got, ref)
    assert s.caches_equal()
