"""GPU: prompt attention on the f16 matrix cores (mi355x_attn_prompt_precision(MI355X_ATTN_PROMPT_F16);
ggml-neon-opt_amd/csrc/kq_attn_mfma.hip: kq_attn_prompt_f16<HD> after the unchanged kq_kv_store) at the
op level, through the graph backend and through LlamaDecoder.prompt.

The inputs and junk-filled caches are those of tests/attn_prompt_ref.py. For every case: both caches
hold the reference's bits (the stores are the exact path's); every row of a token inside the cache is
within tests/attn_f16_ref.py's bound of its float64 emulation, built from q^ = f16(rope(q)) and the
caches after the stores; rows of tokens outside the cache are NaN; and the first call launched exactly
one kq_kv_store<HD> and one kq_attn_prompt_f16<HD>. Each case prints max |F16 - emu| / B and, where it
has the exact oracle's rows, max |exact - emu| / B (the distance between the two references)."""
import numpy as np
import pytest

from tests import attn_f16_ref as R
from tests.attn_prompt_ref import (MIXED, SHUFFLED, STRIDE_BATCH, case_reference, qkv, rand_caches, ref_attn_prompt,
                                   scale_of)
from tests.test_gpu_attn_stream import to_dev
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

HEAD_DIMS = [64, 128]
GRID_BATCHES = ((0,), (31, 32, 33), (63,), SHUFFLED)
GRID = [(2, 2), (6, 2), (8, 2), (8, 1)]
QSCALES = [0.05, 40.0, MIXED]
QSCALE_IDS = ["flat", "peaked", "mixed"]
_TABLES = {}


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


@pytest.fixture
def f16():
    """The selector at F16 for one test, EXACT (the default) afterwards."""
    import ggml_mi355x as g
    assert g.attn_prompt_precision(g.ATTN_PROMPT_F16) == g.ATTN_PROMPT_EXACT
    yield g
    g.attn_prompt_precision(g.ATTN_PROMPT_EXACT)


def rope_table(O, n_ctx, hd):
    if (n_ctx, hd) not in _TABLES:
        _TABLES[(n_ctx, hd)] = O.rope_table(n_ctx, hd, 10000.0)
    return _TABLES[(n_ctx, hd)]


def cache_mismatch(dev_cache, ref):
    bad = np.argwhere(dev_cache.cpu().numpy().view(np.uint16) != ref)
    return (len(bad), bad[:4].tolist()) if len(bad) else None


def stored(O, k, v, pos, kc0, vc0, hd):
    """The caches after kq_kv_store's rule: fp32_to_fp16(rope(k_i)) and fp32_to_fp16(v_i) into the cell
    of every token inside the cache (the stores of tests/attn_prompt_ref.py::ref_attn_prompt)."""
    kc, vc = kc0.copy(), vc0.copy()
    tref = rope_table(O, kc.shape[0], hd)
    for i, p in enumerate(pos):
        if 0 <= p < kc.shape[0]:
            kc[p] = O.fp32_to_fp16(O.rope(k[i], hd, hd, int(p), tref))
            vc[:, p] = O.fp32_to_fp16(v[i])
    return kc, vc


def check_rows(O, got, q, pos, kc, vc, nh, nkv, hd, tag, exact=None):
    """Every valid row within the bound of the emulation over the caches AFTER the stores; NaN rows
    outside the cache. Returns (max |got - emu| / B, max |exact - emu| / B or None)."""
    n_ctx = kc.shape[0]
    tref = rope_table(O, n_ctx, hd)
    worst, worst_exact = 0.0, None if exact is None else 0.0
    for i, p in enumerate(pos):
        if not 0 <= p < n_ctx:
            assert np.isnan(got[i]).all(), (tag, "token", i, "pos", p)
            continue
        qh = R.qhat(O.rope(q[i], hd, hd, int(p), tref))
        emu = R.emulate(qh, kc, vc, p, nh, nkv, hd, scale_of(hd))
        B = R.bound(qh, kc, vc, p, nh, nkv, hd, scale_of(hd))
        assert np.isfinite(got[i]).all(), (tag, "token", i, "pos", p)
        err = np.abs(got[i].astype(np.float64) - emu)
        worst = max(worst, float((err / B).max()))
        if exact is not None:
            worst_exact = max(worst_exact, float((np.abs(exact[i].astype(np.float64) - emu) / B).max()))
        j = int(np.argmax(err / B))
        assert (err <= B).all(), (tag, "token", i, "pos", p, "element", j, "err", err[j], "bound", B[j])
    return worst, worst_exact


def check_names(names, hd):
    assert len(names) == 2, names
    assert sum("kq_kv_store<%d>" % hd in n for n in names) == 1, names
    assert sum("kq_attn_prompt_f16<%d>" % hd in n for n in names) == 1, names


def call(g, dev, q, k, v, pos, tab, kc, vc, nh, nkv, hd):
    return g.attn_prompt(t(q.copy(), dev), t(k.copy(), dev), t(v.copy(), dev), t(np.asarray(pos, np.int32), dev), tab, kc,
                         vc, nh, nkv, hd, scale_of(hd)).cpu().numpy()


def run_steps(g, dev, O, hd, nh, nkv, n_ctx, kc0, vc0, steps, tag):
    """steps: (pos, q, k, v, exact rows or None, kc_after, vc_after) on the same evolving device caches."""
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    kc, vc = to_dev(kc0, dev), to_dev(vc0, dev)
    worst, worst_exact = 0.0, None
    for bi, (pos, q, k, v, exact, kc_ref, vc_ref) in enumerate(steps):
        if bi == 0:
            g.timing_enable(True)
        try:
            got = call(g, dev, q, k, v, pos, tab, kc, vc, nh, nkv, hd)
            if bi == 0:
                check_names([r[0] for r in g.timing_read()], hd)
        finally:
            if bi == 0:
                g.timing_enable(False)
        assert cache_mismatch(kc, kc_ref) is None, (tag, "k cache, batch", bi, cache_mismatch(kc, kc_ref))
        assert cache_mismatch(vc, vc_ref) is None, (tag, "v cache, batch", bi, cache_mismatch(vc, vc_ref))
        w, we = check_rows(O, got, q, pos, kc_ref, vc_ref, nh, nkv, hd, (tag, "batch", bi), exact)
        worst = max(worst, w)
        if we is not None:
            worst_exact = max(worst_exact or 0.0, we)
    print("%s: max |F16 - emu| / B = %.4f, max |exact - emu| / B = %s" % (tag, worst, worst_exact))
    return kc, vc, tab


def run_case(g, dev, O, hd, nh, nkv, n_ctx, batches, qscale=2.0):
    kc0, vc0, steps = case_reference(O, hd, nh, nkv, n_ctx, batches, qscale)
    return run_steps(g, dev, O, hd, nh, nkv, n_ctx, kc0, vc0, steps, (hd, nh, nkv, n_ctx, qscale))


# ---------------------------------------------------------------- op level
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", GRID)
def test_grid(dev, O, f16, hd, nh, nkv):
    """64 cells, group sizes 1, 3, 4, 8 (a workgroup's 4 waves in one, two and four kv groups; 6 heads:
    a workgroup with 2 idle waves): the first cell alone, three tokens across the tile boundary, the
    last cell alone and nine shuffled tokens, on evolving caches."""
    run_case(f16, dev, O, hd, nh, nkv, 64, GRID_BATCHES)


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("qscale", QSCALES, ids=QSCALE_IDS)
def test_scales(dev, O, f16, hd, qscale):
    """Flat, peaked and mixed q at (8, 2) over the 320-cell batch."""
    run_case(f16, dev, O, hd, 8, 2, 320, STRIDE_BATCH, qscale=qscale)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_stride_batch(dev, O, f16, hd):
    """320 cells, positions 250..289: 40 tokens are one full and one partial query tile (8 live lanes),
    whose cell loops have 9 and 10 tiles while single queries need 8, 9 or 10."""
    run_case(f16, dev, O, hd, 8, 2, 320, STRIDE_BATCH)


def moving_maximum_case(O, hd, where):
    """96 cells, 33 tokens at 63..95, (8, 2). Every q and the hot cells' K carry a large component in
    the last rope pair's first channel (the lowest frequency: 96 positions turn it by about 0.01 rad),
    so a hot cell's score exceeds every other by far more than the random part. where == "last": the
    batch's own cells are hot, each hotter than the one before it, so a query's largest score is its
    own cell, in its last tile, and its running maximum moves at every tile. where == "first": the
    junk cells 0..31 are hot and the batch's are not: the maximum is set in the first tile."""
    nh, nkv, n_ctx = 8, 2, 96
    rng = np.random.default_rng([hd, 96, 0 if where == "last" else 1])
    pos = tuple(range(63, 96))
    T, ch = len(pos), hd - 2
    q = rng.standard_normal((T, nh * hd)).astype(np.float32)
    k = rng.standard_normal((T, nkv * hd)).astype(np.float32)
    v = rng.standard_normal((T, nkv * hd)).astype(np.float32)
    kc0, vc0 = rand_caches(rng, n_ctx, nkv * hd)
    q.reshape(T, nh, hd)[:, :, ch] = 12.0
    if where == "last":
        k.reshape(T, nkv, hd)[:, :, ch] = (12.0 + 4.0 * np.arange(T, dtype=np.float32))[:, None]
    else:
        kc0 = kc0.copy()
        kc0.view(np.float16).reshape(n_ctx, nkv, hd)[:32, :, ch] = 24.0
    kc, vc = kc0.copy(), vc0.copy()
    exact = ref_attn_prompt(O, q, k, v, pos, kc, vc, rope_table(O, n_ctx, hd), nh, nkv, hd)
    # the property the case is built for, from the float64 scores
    tref = rope_table(O, n_ctx, hd)
    kf = kc.view(np.float16).astype(np.float64).reshape(n_ctx, nkv, hd)
    for i, p in enumerate(pos):
        qh = R.qhat(O.rope(q[i], hd, hd, p, tref)).astype(np.float64).reshape(nh, hd)
        for h in range(nh):
            s = kf[:p + 1, h // (nh // nkv)] @ qh[h]
            assert int(np.argmax(s)) // 32 == (p // 32 if where == "last" else 0), (where, p, h)
            if where == "last":  # the running maximum grows at every tile
                tiles = [s[c:c + 32].max() for c in range(0, p + 1, 32)]
                assert all(b > a for a, b in zip(tiles, tiles[1:])), (p, h, tiles)
    return kc0, vc0, [(pos, q, k, v, exact, kc, vc)]


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("where", ["last", "first"])
def test_moving_maximum(dev, O, f16, hd, where):
    kc0, vc0, steps = moving_maximum_case(O, hd, where)
    run_steps(f16, dev, O, hd, 8, 2, 96, kc0, vc0, steps, ("maximum in the %s tile" % where, hd))


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_outside_the_cache(dev, O, f16, hd):
    """Positions n_ctx and -1 inside a batch: NaN rows, no cell written (both caches keep the
    reference's bits everywhere), the neighbours' rows within the bound."""
    run_case(f16, dev, O, hd, 8, 2, 64, ((0, 1, 64, 3, -1),))


def test_long_cache(dev, O, f16):
    """4096 cells, head_dim 128, (8, 2), 64 tokens at 4032..4095: two full query tiles of 127 and 128
    cell tiles. Inputs and junk caches as tests/attn_prompt_ref.py draws them; the caches' reference is
    the stores' rule and the rows' the emulation (the exact oracle takes 19 s on this case: not run)."""
    hd, nh, nkv, n_ctx = 128, 8, 2, 4096
    rng = np.random.default_rng([hd, nh, nkv, n_ctx])
    pos = tuple(range(4032, 4096))
    kc0, vc0 = rand_caches(rng, n_ctx, nkv * hd)
    q, k, v = qkv(rng, len(pos), nh, nkv, hd, 2.0)
    kc, vc = stored(O, k, v, pos, kc0, vc0, hd)
    run_steps(f16, dev, O, hd, nh, nkv, n_ctx, kc0, vc0, [(pos, q, k, v, None, kc, vc)], "4096 cells")


def test_past_8192_cells(dev, O, f16):
    """16384 cells under attn_stream(1) (as decode needs there), head_dim 64, (4, 1), 32 tokens at the
    end: the matrix-core kernel, no streamed launch, no workspace. The oracle's arrays end at 8192 cells:
    the reference is the emulation alone (and the stores' rule for the caches)."""
    g = f16
    hd, nh, nkv, n_ctx = 64, 4, 1, 16384
    rng = np.random.default_rng(16384)
    pos = tuple(range(n_ctx - 32, n_ctx))
    q = (rng.standard_normal((32, nh * hd)) * 2).astype(np.float32)
    k = rng.standard_normal((32, nkv * hd)).astype(np.float32)
    v = rng.standard_normal((32, nkv * hd)).astype(np.float32)
    kc0, vc0 = rand_caches(rng, n_ctx, nkv * hd)
    kc, vc = stored(O, k, v, pos, kc0, vc0, hd)
    assert g.attn_stream(0) == 0
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    with pytest.raises(g.Mi355xError):  # refused for its size with the streamed mode off, as decode is
        call(g, dev, q, k, v, pos, tab, to_dev(kc0, dev), to_dev(vc0, dev), nh, nkv, hd)
    assert g.attn_stream(1) == 0
    try:
        run_steps(g, dev, O, hd, nh, nkv, n_ctx, kc0, vc0, [(pos, q, k, v, None, kc, vc)], "16384 cells")
    finally:
        g.attn_stream(0)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_deterministic_and_exact_path_untouched(dev, O, f16, hd):
    """Two F16 calls give the same bits; with the selector back at EXACT the same call gives the exact
    path's bits (the reference's) from the group kernel."""
    g = f16
    nh, nkv, n_ctx = 8, 2, 320
    kc0, vc0, steps = case_reference(O, hd, nh, nkv, n_ctx, STRIDE_BATCH, 2.0)
    pos, q, k, v, ref, kc_ref, vc_ref = steps[0]
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    kc, vc = to_dev(kc0, dev), to_dev(vc0, dev)
    a = call(g, dev, q, k, v, pos, tab, kc, vc, nh, nkv, hd)
    b = call(g, dev, q, k, v, pos, tab, kc, vc, nh, nkv, hd)
    assert bits_equal(a, b), first_mismatch(a, b)
    assert not bits_equal(a, ref)  # (the two precisions do differ on this case)
    assert g.attn_prompt_precision(g.ATTN_PROMPT_EXACT) == g.ATTN_PROMPT_F16
    g.timing_enable(True)
    try:
        c = call(g, dev, q, k, v, pos, tab, kc, vc, nh, nkv, hd)
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
        g.attn_prompt_precision(g.ATTN_PROMPT_F16)
    assert not any("f16" in n for n in names) and any("kq_attn_prompt_group<%d>" % hd in n for n in names), names
    assert bits_equal(c, ref), first_mismatch(c, ref)
    assert cache_mismatch(kc, kc_ref) is None and cache_mismatch(vc, vc_ref) is None


# ---------------------------------------------------------------- the graph backend
Q4_K = 12
GRAPH_T, GRAPH_E, GRAPH_OUT = 37, 512, 256
QUANTIZE = "kq_quantize_q8L"


@pytest.mark.parametrize("hd,nh,nkv,n_ctx", [(64, 8, 2, 64), (128, 8, 1, 128)])
def test_graph(dev, O, oracle, f16, hd, nh, nkv, n_ctx):
    """k = MUL_MAT(wk, x), v = MUL_MAT(wv, x), att = ATTN_DECODE(q, k, v, ...), o = MUL_MAT(wo, att) over
    37 tokens at 20..56 (shapes whose exact plan fuses the o-proj's quantization into the attention).
    Under F16: k, v and both caches keep the exact bits (the GEMM's KV-store epilogue still stores the
    cells: no kq_kv_store launch), the attention node's rows equal the direct mi355x_attn_prompt call's
    bits, the o-proj quantizes its activation itself (two kq_quantize_q8L launches), a replay equals the
    capture, and flipping the selector on the same backend and nodes plans again: EXACT gives the exact
    rows, F16 after it the F16 rows."""
    import torch
    g = f16
    from tests import llama_model as LM
    T, E, NO, kvw = GRAPH_T, GRAPH_E, GRAPH_OUT, nkv * hd
    rng = np.random.default_rng([hd, nh, nkv, n_ctx, 16])
    wk, wv = LM.kquant(rng, Q4_K, kvw, E), LM.kquant(rng, Q4_K, kvw, E)
    wo = LM.kquant(rng, Q4_K, NO, nh * hd)
    x = rng.standard_normal((T, E)).astype(np.float32)
    q = (rng.standard_normal((T, nh * hd)) * 2).astype(np.float32)
    pos = np.arange(20, 20 + T, dtype=np.int32)
    kc0, vc0 = rand_caches(rng, n_ctx, kvw)
    k_ref, v_ref = oracle.mul_mat(Q4_K, wk, x), oracle.mul_mat(Q4_K, wv, x)
    kc_ref, vc_ref = kc0.copy(), vc0.copy()
    att_exact = ref_attn_prompt(O, q, k_ref, v_ref, pos.tolist(), kc_ref, vc_ref, rope_table(O, n_ctx, hd), nh, nkv, hd)

    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    # the direct call on the same inputs
    att_direct = call(g, dev, q, k_ref, v_ref, pos, tab, to_dev(kc0, dev), to_dev(vc0, dev), nh, nkv, hd)
    check_rows(O, att_direct, q, pos.tolist(), kc_ref, vc_ref, nh, nkv, hd, "direct", att_exact)
    o_f16 = oracle.mul_mat(Q4_K, wo, att_direct)

    d = dict(wk=t(wk, dev), wv=t(wv, dev), wo=t(wo, dev), x=t(x, dev), q=t(q, dev), pos=t(pos, dev),
             kc=to_dev(kc0, dev), vc=to_dev(vc0, dev), kc0=to_dev(kc0, dev), vc0=to_dev(vc0, dev))
    for name, n in (("k", kvw), ("v", kvw), ("att", nh * hd), ("o", NO)):
        d[name] = torch.empty((T, n), dtype=torch.float32, device=dev)
    F32 = g.TYPE_F32
    xt = g.make_tensor(F32, E, T, d["x"].data_ptr())
    qt = g.make_tensor(F32, nh * hd, T, d["q"].data_ptr())
    post = g.make_tensor(g.TYPE_I32, T, 1, d["pos"].data_ptr())
    kct = g.make_tensor(g.TYPE_F16, kvw, n_ctx, d["kc"].data_ptr())
    vct = g.make_tensor(g.TYPE_F16, n_ctx, kvw, d["vc"].data_ptr())
    tabt = g.make_tensor(F32, hd, n_ctx, tab.data_ptr())
    wkt = g.make_tensor(Q4_K, E, kvw, d["wk"].data_ptr())
    wvt = g.make_tensor(Q4_K, E, kvw, d["wv"].data_ptr())
    wot = g.make_tensor(Q4_K, nh * hd, NO, d["wo"].data_ptr())
    kt = g.make_tensor(F32, kvw, T, d["k"].data_ptr(), op=g.OP_MUL_MAT, src0=wkt, src1=xt)
    vt = g.make_tensor(F32, kvw, T, d["v"].data_ptr(), op=g.OP_MUL_MAT, src0=wvt, src1=xt)
    att = g.make_tensor(F32, nh * hd, T, d["att"].data_ptr(), op=g.OP_ATTN_DECODE, srcs=[qt, kt, vt, post, kct, vct, tabt],
                        op_params=[nh, nkv, hd, g.f32_bits(scale_of(hd))])
    ot = g.make_tensor(F32, NO, T, d["o"].data_ptr(), op=g.OP_MUL_MAT, src0=wot, src1=att)
    nodes = [kt, vt, att, ot]
    be = g.Backend()
    try:
        be.set_fusion(True)
        # (precision, use_graph): eager, capture, replay under F16; EXACT on the same nodes; F16 again
        passes = [(g.ATTN_PROMPT_F16, 0), (g.ATTN_PROMPT_F16, 1), (g.ATTN_PROMPT_F16, 1), (g.ATTN_PROMPT_EXACT, 1),
                  (g.ATTN_PROMPT_F16, 1)]
        for pi, (prec, use_graph) in enumerate(passes):
            g.attn_prompt_precision(prec)
            d["kc"].copy_(d["kc0"])
            d["vc"].copy_(d["vc0"])
            for name in ("k", "v", "att", "o"):
                d[name].fill_(7.0)
            torch.cuda.synchronize()
            if pi == 0:
                g.timing_enable(True)
            try:
                assert be.graph_compute(nodes, use_graph=use_graph) == 0
                be.synchronize()
                if pi == 0:
                    names = [r[0] for r in g.timing_read()]
                    print("graph launches", names)
                    assert not any("kq_kv_store" in n for n in names), names  # the GEMM's epilogue stored the cells
                    assert sum("kq_attn_prompt_f16<%d>" % hd in n for n in names) == 1, names
                    assert not any("kq_attn_prompt_group" in n or "kq_attn_prompt<" in n for n in names), names
                    assert sum(QUANTIZE in n for n in names) == 2, names  # x, and att for the o-proj: unfused
            finally:
                if pi == 0:
                    g.timing_enable(False)
            got = {name: d[name].cpu().numpy() for name in ("k", "v", "att", "o")}
            assert bits_equal(got["k"], k_ref) and bits_equal(got["v"], v_ref), pi
            assert cache_mismatch(d["kc"], kc_ref) is None and cache_mismatch(d["vc"], vc_ref) is None, pi
            want, want_o = (att_direct, o_f16) if prec == g.ATTN_PROMPT_F16 else (att_exact, oracle.mul_mat(Q4_K, wo, att_exact))
            assert bits_equal(got["att"], want), (pi, first_mismatch(got["att"], want))
            assert bits_equal(got["o"], want_o), (pi, first_mismatch(got["o"], want_o))
    finally:
        be.close()
    assert not bits_equal(att_direct, att_exact)


# ---------------------------------------------------------------- LlamaDecoder.prompt
def oracle_logits(O, hp, w, n_ctx, tokens, marks, attention=None):
    """The oracle model's logits after the tokens at the marked counts, decoding one by one; `attention`
    replaces its attention block (oracle.kq_ops_oracle.attn_decode's signature) for the run."""
    from tests import llama_model as LM
    model, cache = LM.oracle_model(hp, w, n_ctx)
    keep, out = O.attn_decode, []
    if attention is not None:
        O.attn_decode = attention
    try:
        for p, tok in enumerate(tokens):
            lg, _ = O.decode_token(model, tok, p, cache)
            if p + 1 in marks:
                out.append(np.asarray(lg, np.float64).ravel())
    finally:
        O.attn_decode = keep
    return out, cache


def test_llama_prompt(dev, O, f16):
    """LlamaDecoder.prompt on the 2-layer synthetic model, 37 tokens and then 11 more from the cache.
    Layer 0's K and V caches equal the exact prompt's bit for bit (they do not depend on the
    attention); the logits are finite; and max |logits_F16 - logits_exact| <= 4 d_ref, where d_ref =
    max |logits(oracle model) - logits(oracle model with its attention replaced by the float64
    emulation)| is the distance between two references (the factor 4: the requantization steps between
    the layers). The exact prompt's logits are the oracle's, bit for bit."""
    import torch
    g = f16
    from tests.test_gpu_ops import _decoder
    from ggml_mi355x.llama import hparams
    hp = hparams(2048, 2, 32, 4, 5632, 4096)
    n_ctx, n1, n2 = 64, 37, 11
    nh, nkv, hd = hp["n_head"], hp["n_head_kv"], hp["head_dim"]
    tokens = np.random.default_rng(13).integers(0, hp["n_vocab"], size=n1 + n2).tolist()
    out = {}
    for name, prec in (("exact", g.ATTN_PROMPT_EXACT), ("f16", g.ATTN_PROMPT_F16)):
        g.attn_prompt_precision(prec)
        w, b, dec = _decoder(dev, hp, 7, n_ctx, True)
        try:
            lg1 = dec.prompt(tokens[:n1], 0)
            b.synchronize()
            lg1 = lg1.cpu().numpy().astype(np.float64).ravel()
            lg2 = dec.prompt(tokens[n1:], n1)
            b.synchronize()
            lg2 = lg2.cpu().numpy().astype(np.float64).ravel()
            out[name] = ([lg1, lg2], dec.k_cache[0].cpu().numpy().view(np.uint16), dec.v_cache[0].cpu().numpy().view(np.uint16))
        finally:
            b.close()
    g.attn_prompt_precision(g.ATTN_PROMPT_F16)
    assert np.array_equal(out["f16"][1], out["exact"][1]) and np.array_equal(out["f16"][2], out["exact"][2])
    assert all(np.isfinite(l).all() for l in out["f16"][0])

    def emulated(q, k, v, k_cache, v_cache, pos, n_head, n_head_kv, head_dim, scale, fast_threads=0):
        k_cache[pos, :] = O.fp32_to_fp16(k)
        v_cache[:, pos] = O.fp32_to_fp16(v)
        return R.emulate(R.qhat(q), k_cache, v_cache, pos, n_head, n_head_kv, head_dim, scale).astype(np.float32)

    ref, _ = oracle_logits(O, hp, w, n_ctx, tokens, (n1, n1 + n2))
    emu, _ = oracle_logits(O, hp, w, n_ctx, tokens, (n1, n1 + n2), attention=emulated)
    for a, r in zip(out["exact"][0], ref):
        assert np.array_equal(a, r)  # the default path stays bit-exact
    d_ref = max(float(np.abs(r - e).max()) for r, e in zip(ref, emu))
    seen = max(float(np.abs(a - r).max()) for a, r in zip(out["f16"][0], out["exact"][0]))
    print("d_ref = %.6g, max |logits_F16 - logits_exact| = %.6g" % (d_ref, seen))
    assert d_ref > 0
    assert seen <= 4.0 * d_ref
    torch.cuda.synchronize()
