"""CPU tests of the oracle (test infrastructure): C restatement vs independent numpy
restatement, committed golden vectors, quantizer edge cases, the restated
mul_mat scheduler. No GPU needed."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TYPES = (12, 13, 14)


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("K", [256, 768, 2048, 5632])
def test_c_vs_numpy_bit_exact(oracle, npo, type_, K):
    rng = np.random.default_rng(1000 + type_ * 7 + K)
    w = npo.random_blocks(rng, type_, 23, K)
    x = rng.standard_normal((3, K)).astype(np.float32) * np.float32(rng.uniform(1e-3, 1e3))
    q8 = oracle.quantize_q8_K(x)
    assert (q8 == npo.q8_K_to_bytes(npo.quantize_q8_K(x))).all()
    got = oracle.mul_mat(type_, w, x)
    ref = npo.mul_mat_q8(w, type_, K, npo.q8_K_from_bytes(q8, K // 256))
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    a, b = npo.block_partials(w, type_, K, npo.q8_K_from_bytes(q8, K // 256))
    for j in range(3):
        p = oracle.block_partials(type_, w, q8[j], K)
        assert (p[..., 0] == a[:, j]).all() and (p[..., 1] == b[:, j]).all()


def test_golden_manifest_and_replay(oracle):
    manifest = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    assert len(manifest) >= 7
    for name, sha in manifest.items():
        path = os.path.join(GOLDEN, name + ".npz")
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == sha, name
        z = np.load(path)  # allow_pickle defaults to False
        if name == "q8K_edges":
            assert (oracle.quantize_q8_K(z["x"]) == z["q8"]).all()
            assert (oracle.quantize_q8_K(z["x"], fused=False) == z["q8_unfused"]).all()
            continue
        t, K = int(z["type"]), int(z["K"])
        assert (oracle.quantize_q8_K(z["x"]) == z["q8"]).all(), name
        got = oracle.mul_mat(t, z["w"], z["x"])
        assert (got.view(np.uint32) == z["dst"].view(np.uint32)).all(), name
        for j in range(z["x"].shape[0]):
            assert (oracle.block_partials(t, z["w"], z["q8"][j], K) == z["partials"][j]).all()


def test_q8K_zero_block_and_ties(oracle, npo):
    x = np.zeros((1, 512), np.float32)
    x[0, 256 + 10] = -2.0
    x[0, 256 + 20] = 2.0
    q = npo.q8_K_from_bytes(oracle.quantize_q8_K(x), 2)
    assert q["d"][0, 0] == 0 and (q["qs"][0, 0] == 0).all() and (q["bsums"][0, 0] == 0).all()
    # first max is -2 -> iscale = +63.5 -> element 10 -> -127, element 20 -> +127 (clamped)
    assert q["qs"][0, 1, 10] == -127 and q["qs"][0, 1, 20] == 127
    assert q["d"][0, 1] > 0


def test_q8K_max_is_negative_127(oracle, npo):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 1024)).astype(np.float32)
    q = npo.q8_K_from_bytes(oracle.quantize_q8_K(x), 4)
    xb = x.reshape(4, 4, 256)
    idx = np.abs(xb).argmax(-1)
    qv = np.take_along_axis(q["qs"], idx[..., None], -1)[..., 0]
    assert (qv == -127).all()  # iscale = -127/max maps the block max to -127
    assert (q["qs"] >= -127).all() and (q["qs"] <= 127).all()
    assert (q["bsums"] == q["qs"].reshape(4, 4, 16, 16).astype(np.int32).sum(-1)).all()


def test_fused_vs_unfused_nearest_int_differ_rarely(oracle):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((64, 4096)).astype(np.float32)
    a = oracle.quantize_q8_K(x, fused=True)
    b = oracle.quantize_q8_K(x, fused=False)
    frac = (a != b).mean()
    assert frac < 1e-3  # double rounding is rare, but the build choice is pinned


@pytest.mark.parametrize("type_", [12, 14])
def test_neon_vs_generic_order(oracle, npo, type_):
    """The generic restatement (8 float lanes) shares every integer with the NEON one
    and differs only in fp32 rounding order."""
    rng = np.random.default_rng(7)
    K = 4096
    w = npo.random_blocks(rng, type_, 64, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    neon = oracle.mul_mat(type_, w, x, variant="neon")
    gen = oracle.mul_mat(type_, w, x, variant="generic")
    a, b = npo.block_partials(w, type_, K, npo.q8_K_from_bytes(oracle.quantize_q8_K(x), K // 256))
    scale = np.abs(neon).max() + 1e-30
    assert np.max(np.abs(neon - gen)) <= 1e-5 * scale


@pytest.mark.parametrize("type_", TYPES)
def test_dot_matches_dequantized_float_dot(oracle, npo, type_):
    """Semantic check of the block layouts: vec_dot == dequant(w) . dequant(q8) up to fp32 rounding."""
    rng = np.random.default_rng(3)
    K = 2048
    w = npo.random_blocks(rng, type_, 32, K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    q8 = oracle.quantize_q8_K(x)
    qq = npo.q8_K_from_bytes(q8, K // 256)
    xd = (qq["qs"].astype(np.float64) * qq["d"][..., None].astype(np.float64)).reshape(1, K)
    wd = npo.dequantize(w, type_, K)
    ref = wd @ xd[0]
    got = oracle.mul_mat(type_, w, x)[0]
    assert np.max(np.abs(got - ref)) <= 1e-5 * (np.abs(wd) @ np.abs(xd[0])).max()
    # the C dequant restatement agrees with the numpy one
    assert np.allclose(oracle.dequantize(type_, w, K), wd, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("n_threads", [2, 3, 8])
def test_mul_mat_threading_is_bit_identical(oracle, npo, n_threads):
    rng = np.random.default_rng(9)
    K, N = 2048, 300
    w = npo.random_blocks(rng, 12, N, K)
    x = rng.standard_normal((5, K)).astype(np.float32)
    one = oracle.mul_mat(12, w, x, n_threads=1)
    many = oracle.mul_mat(12, w, x, n_threads=n_threads)
    assert (one.view(np.uint32) == many.view(np.uint32)).all()


def test_fp16_roundtrip(oracle):
    L = oracle.lib()
    for h in [0x0000, 0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0x8001, 0xFBFF]:
        f = L.kqo_fp16_to_fp32(h)
        assert np.float32(f) == np.uint16(h).view(np.float16).astype(np.float32)
        assert L.kqo_fp32_to_fp16(f) == h


@pytest.mark.parametrize("type_", TYPES)
def test_simd_vec_dot_matches_scalar(oracle, npo, type_):
    """The AVX2 vec_dot of the CPU baseline (oracle/kq_cpu_simd.c) is bit-identical to
    the scalar NEON-order restatement: exact integer parts, the same fp32 chain —
    including extreme blocks (max scales, nibble 15, q8 +-127, fp16 subnormal d)."""
    rng = np.random.default_rng(21 + type_)
    K = 4096
    w = npo.random_blocks(rng, type_, 96, K)
    w[:8] = 0xFF                                   # every quant / scale bit set
    w[8:16, :] = rng.integers(0, 256, w[8:16].shape, dtype=np.uint8)  # any bytes, d/dmin included
    x = rng.standard_normal((3, K)).astype(np.float32)
    x[1, :256] = 0.0                               # all-zero activation block
    x[2, ::7] *= 1e4                               # saturating outliers
    a = oracle.mul_mat(type_, w, x, n_threads=1, variant="neon")
    for nt in (1, 5):
        b = oracle.mul_mat(type_, w, x, n_threads=nt, variant="simd")
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        assert same.all()
    q8 = oracle.quantize_q8_K(x[:1])[0]
    for r in range(0, 96, 11):
        assert np.float32(oracle.vec_dot(type_, w[r], q8, K, "simd")).view(np.uint32) == \
            np.float32(oracle.vec_dot(type_, w[r], q8, K, "neon")).view(np.uint32) or \
            np.isnan(oracle.vec_dot(type_, w[r], q8, K, "neon"))


def test_thread_pool_reuse_and_resize(oracle, npo):
    """The persistent worker pool gives the same bits across calls and thread counts."""
    rng = np.random.default_rng(31)
    K, N = 2048, 257
    w = npo.random_blocks(rng, 12, N, K)
    x = rng.standard_normal((2, K)).astype(np.float32)
    ref = oracle.mul_mat(12, w, x, n_threads=1)
    for nt in (4, 4, 7, 2, 7):
        got = oracle.mul_mat(12, w, x, n_threads=nt, variant="simd")
        assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def test_unpinned_choice_flip_rates(oracle, npo):
    """the three bit-deciding fp choices the reference's listings do not show
    ([U]), each against its alternatives at TinyLlama's shapes — how often
    the alternative would change an output. Whoever holds llama.cpp a3cb0474 can then tell
    which goldens an observed difference would force to be regenerated.
      * quantize_row_q8_K's nearest_int(iscale * x): fused (fmadd) vs unfused — about 2e-6 of
        the qs bytes (one activation row of 2048 in a few hundred), but a flipped byte changes
        every output of the GEMV that reads the row;
      * Q6_K `sum += d_all * y.d * (isum - 32 * isum_mins)`: fma vs no fma — half the rows;
      * Q5_K `sumf += d * sumi - dmin * sumi_mins`: which product gcc fuses — half the rows."""
    rng = np.random.default_rng(2024)
    K = 2048
    x = rng.standard_normal((1024, K)).astype(np.float32)
    a, b = oracle.quantize_q8_K(x, fused=True), oracle.quantize_q8_K(x, fused=False)
    A, B = a.reshape(1024, K // 256, 292), b.reshape(1024, K // 256, 292)
    byte_frac = (A[..., 4:260] != B[..., 4:260]).mean()
    assert 0 < byte_frac < 1e-4, byte_frac
    row = int(np.flatnonzero((A != B).any((1, 2)))[0])
    w = npo.random_blocks(rng, 12, 512, K)
    ya, yb = oracle.mul_mat_q8(12, w, a[row], K)[0], oracle.mul_mat_q8(12, w, b[row], K)[0]
    assert (ya.view(np.uint32) != yb.view(np.uint32)).mean() > 0.9

    q = oracle.quantize_q8_K(x[:1])
    w6 = npo.random_blocks(rng, 14, 1024, K)
    y0 = oracle.mul_mat_q8(14, w6, q, K)[0]
    with oracle.contraction_variant(1, 1):
        y1 = oracle.mul_mat_q8(14, w6, q, K)[0]
    f6 = (y0.view(np.uint32) != y1.view(np.uint32)).mean()
    assert 0.3 < f6 < 0.8, f6
    assert np.array_equal(oracle.mul_mat_q8(14, w6, q, K)[0].view(np.uint32), y0.view(np.uint32))  # restored

    w5 = npo.random_blocks(rng, 13, 1024, K)
    y0 = oracle.mul_mat_q8(13, w5, q, K)[0]
    for v, lo, hi in ((1, 0.3, 0.7), (2, 0.3, 0.7), (3, 0.5, 0.9)):
        with oracle.contraction_variant(0, v):
            y1 = oracle.mul_mat_q8(13, w5, q, K)[0]
        f5 = (y0.view(np.uint32) != y1.view(np.uint32)).mean()
        assert lo < f5 < hi, (v, f5)


# ---------------------------------------------------------------- super-block scale edges
def _scales_f16(npo, w, type_, K):
    """The fp16 bit patterns of d (and dmin) per row and block: list of (N, nb) uint16."""
    f = npo.split_blocks(w, type_, K)
    return [f["d"]] + ([f["dmin"]] if type_ in (12, 13) else [])


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("K", [256, 768])
def test_edge_blocks_produces_every_category(npo, type_, K):
    """Decoded back: sign, zero-ness, subnormality and range of d / dmin per category, so that an
    edit cannot quietly turn edge_blocks back into random_blocks."""
    ncat = len(npo.EDGE_CATS)
    N = 8 * ncat
    w = npo.edge_blocks(np.random.default_rng(type_ + K), type_, N, K)
    nb = K // 256
    assert w.shape == (N, nb * npo.BLOCK_BYTES[type_]) and w.dtype == np.uint8
    assert npo.EDGE_CATS_F16 == npo.EDGE_CATS[:-1] and npo.EDGE_CATS[-1] == "maxf16"
    fields = _scales_f16(npo, w, type_, K)
    seen_neg = {c: False for c in npo.EDGE_CATS}
    seen_pos = dict(seen_neg)
    zero_pairs = set()
    for r in range(N):
        cat = npo.edge_category(r)
        assert cat == npo.EDGE_CATS[r % ncat]
        for fi, h in enumerate(fields):
            bits = h[r]
            v = npo.fp16_to_f32(bits).astype(np.float64)
            mag, neg = bits & 0x7FFF, (bits >> 15).astype(bool)
            seen_neg[cat] |= bool(neg.any())
            seen_pos[cat] |= bool((~neg).any())
            if cat == "control":
                assert (~neg).all() and (mag >= 0x0400).all() and (v <= 2.0 ** -6).all()
            elif cat == "subnormal":
                assert (~neg).all() and (mag >= 1).all() and (mag < 0x0400).all()
                assert (v >= 2.0 ** -24).all() and (v < 2.0 ** -14).all()
            elif cat in ("zero", "negzero"):
                z = mag == 0
                want = np.arange(nb) % 2 == (r // ncat + fi) % 2
                assert (z == want).all(), (r, fi, bits)
                assert (bits[z] == (0x8000 if cat == "negzero" else 0)).all()
                assert (mag[~z] >= 0x0400).all() and (~neg[~z]).all()
            elif cat == "negative":
                assert neg.all() and (-v >= 2.0 ** -14).all() and (-v <= 2.0 ** -6).all()
            elif cat == "mixed":
                assert (np.abs(v) >= 2.0 ** -24).all() and (np.abs(v) <= 2.0 ** -6).all()
            elif cat == "saturated":
                assert (bits == 0x2400).all() and (v == 2.0 ** -6).all()
            elif cat == "large":
                assert (np.abs(v) >= 2.0 ** -6).all() and (np.abs(v) <= 4.0).all()
            elif cat == "maxf16":
                assert (np.abs(v) == 65504.0).all()
        if cat in ("zero", "negzero") and len(fields) == 2:
            for b in range(nb):
                zero_pairs.add((bool(fields[0][r, b] & 0x7FFF == 0), bool(fields[1][r, b] & 0x7FFF == 0)))
    for cat in ("mixed", "large", "maxf16"):
        assert seen_neg[cat] and seen_pos[cat], cat
    assert seen_neg["negative"] and seen_neg["negzero"] and not seen_neg["subnormal"] and not seen_neg["zero"]
    if type_ in (12, 13):
        assert zero_pairs == {(True, False), (False, True)}  # d = 0 with dmin != 0, and the reverse
    # the mixed rows reach the subnormals as well as the normals
    mixed = np.concatenate([h[5::ncat].ravel() for h in fields]) & 0x7FFF
    assert (mixed < 0x0400).any() and (mixed >= 0x0400).any()
    # saturated: scales, mins and quants at their maxima
    q, sc, mn, _ = npo.weights_int(w[6::ncat], type_, K)
    if type_ in (12, 13):
        assert (sc == 63).all() and (mn == 63).all() and (q == (15 if type_ == 12 else 31)).all()
    else:
        assert (q == 63).all() and (sc[..., 0::2] == 127).all() and (sc[..., 1::2] == -128).all()
    # the control rows are random_blocks' rows, byte for byte
    ref = npo.random_blocks(np.random.default_rng(type_ + K), type_, N, K)
    assert (w[0::ncat] == ref[0::ncat]).all()


def test_poison_blocks_and_edge_activations(npo):
    K = 768
    w = npo.random_blocks(np.random.default_rng(3), 14, 10, K)
    p = npo.poison_blocks(w, 14, K, [0, 4, 9], [0x7C00, 0xFC00, 0x7E00])
    d, d0 = npo.split_blocks(p, 14, K)["d"], npo.split_blocks(w, 14, K)["d"]
    assert d[0, 1] == 0x7C00 and d[4, 1] == 0xFC00 and d[9, 1] == 0x7E00
    d[[0, 4, 9], 1] = d0[[0, 4, 9], 1]
    assert (d == d0).all() and (p != w).sum() <= 6
    x = npo.edge_activations(np.random.default_rng(4), 7, K)
    assert x.dtype == np.float32 and x.shape == (7, K) and np.isfinite(x).all()
    assert (x[1, 256:512] == 0).all() and (x[1, :256] != 0).any()
    assert (x[2] == 1.0).all() and (x[3, 0::2] == 1.0).all() and (x[3, 1::2] == -1.0).all()
    assert np.abs(x[4, ::7]).max() > 1e3 and np.abs(x[4, 1::7]).max() < 10
    assert (x[6, 256:512] == 0).all()  # the forms repeat
    q8 = npo.quantize_q8_K(x[2:4])
    assert (np.abs(q8["qs"]) == 127).all()
    assert (npo.edge_activations(np.random.default_rng(4), 1, K, first=3)[0] == x[3]).all()


@pytest.mark.parametrize("type_", TYPES)
def test_edge_blocks_neon_equals_simd_and_finite(oracle, npo, type_):
    K = 768
    rng = np.random.default_rng(40 + type_)
    w = npo.edge_blocks(rng, type_, 3 * len(npo.EDGE_CATS), K)
    x = npo.edge_activations(rng, 5, K)
    a = oracle.mul_mat(type_, w, x, variant="neon")
    b = oracle.mul_mat(type_, w, x, variant="simd")
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert np.isfinite(a).all()
    ref = npo.mul_mat_q8(w, type_, K, npo.quantize_q8_K(x))
    assert (a.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("cat", range(8), ids=lambda c: "cat%d" % c)
def test_edge_mmf_emulation_within_bound_per_category(oracle, npo, type_, cat):
    """The condition the GPU test of the f16 path relies on, per category of EDGE_CATS_F16 and
    with only that category's rows in the bound (its second term takes the global max A, so
    one extreme row would loosen it for all): the emulation is finite and within mmf_bound of
    the bit-exact reference. maxf16 is outside the f16 path's domain: f16(d sc) overflows."""
    K = 768
    cats = npo.EDGE_CATS_F16
    rng = np.random.default_rng(60 + type_)
    w = npo.edge_blocks(rng, type_, 4 * len(cats), K, cats)[cat::len(cats)]
    x = npo.edge_activations(rng, 10, K)
    ref = oracle.mul_mat(type_, w, x).astype(np.float64)
    emu = npo.mmf_emulate(w, type_, K, x)
    bound = npo.mmf_bound(w, type_, K, x)
    assert np.isfinite(emu).all() and np.isfinite(bound).all(), cats[cat]
    assert (np.abs(emu - ref) <= bound).all(), (cats[cat], float((np.abs(emu - ref) / bound).max()))


def test_edge_mmf_domain_ends_before_maxf16(npo):
    w = npo.edge_blocks(np.random.default_rng(1), 12, 9, 256)[8:9]
    assert npo.edge_category(8) == "maxf16"
    x = npo.edge_activations(np.random.default_rng(2), 1, 256)
    with np.errstate(all="ignore"):
        assert not np.isfinite(npo.mmf_emulate(w, 12, 256, x)).all()
        # the activation side: 16 * max|x| <= 65504 holds for the 1e3-outlier row, not for a 1e5 outlier
        ok = npo.random_blocks(np.random.default_rng(3), 12, 4, 256)
        far = x.copy()
        far[0, 5] = 1e5
        assert np.isfinite(npo.mmf_emulate(ok, 12, 256, npo.edge_activations(np.random.default_rng(2), 5, 256))).all()
        assert not np.isfinite(npo.mmf_emulate(ok, 12, 256, far)).all()


@pytest.mark.parametrize("type_", TYPES)
def test_edge_large_rows_reach_past_64(npo, type_):
    """The `large` rows hold scales with |f16(d sc)| >= 64, where -1024 * f16(d sc) is past 65504 (an f16
    fma with that addend is non-finite there), and stay inside |d sc| max(q) <= 65504."""
    cats = npo.EDGE_CATS_F16
    w = npo.edge_blocks(np.random.default_rng([type_, 768, 80, 20]), type_, 80, 768, cats)[7::len(cats)]
    q, sc, _, f = npo.weights_int(w, type_, 768)
    dsc = np.abs((npo.fp16_to_f32(f["d"])[..., None] * sc.astype(np.float32)).astype(np.float16).astype(np.float64))
    assert dsc.max() >= 64 and dsc.max() * {12: 15, 13: 31, 14: 63}[type_] <= 65504
