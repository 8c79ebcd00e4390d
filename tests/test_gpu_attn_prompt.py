"""GPU: prompt attention (mi355x_attn_prompt; ggml-neon-opt_amd/csrc/kq_ops.hip: kq_kv_store,
kq_attn_prompt_group<HD, GSZ>, kq_attn_prompt<HD>) at the op level, and its two graph fusions (the KV-store
epilogue of the k / v GEMM, ggml-neon-opt_amd/csrc/kq_mmq.hip; the attention's Q8L output for the o-proj),
every comparison on bits and row by row.

The reference is tests/attn_prompt_ref.py (the oracle's pieces only: every valid cell of the batch stored
into junk-filled caches, then attn_decode per token in batch order; a token outside the cache stores
nothing and gets a NaN row). tests/test_ops_oracle.py::test_prompt_reference_equals_sequential_decode pins
that this equals decoding the tokens one by one in ascending position, outputs and caches.

Which kernel runs is restated from ggml-neon-opt_amd/csrc/kq_ops.hip (attn_prompt_group_ok): the group form
for group sizes up to 8 whose rows fit 160 KiB of LDS, gsz * (2 hd + 6 n_ctx + 16) bytes, under the default
selector; the per-head form otherwise. Every case reads the launch names of its first call and fails if
another form ran. The logged names carry HD only, so the group form's GSZ cannot be read from them: it
follows from the group size (launch_attn_prompt: GSZ 8 or 4 for those group sizes, 0, the run-time loop,
for every other). By that rule the grid (group sizes 1, 2, 3, 4, 8 at both head sizes) reaches all of
kq_attn_prompt_group<64|128, 8|4|0>, and the "head" runs, group size 16 and 3392 cells reach both
kq_attn_prompt<64|128>."""
import numpy as np
import pytest

from tests.attn_prompt_ref import MIXED, SHUFFLED, STRIDE_BATCH, case_reference, rand_caches, ref_attn_prompt, scale_of
from tests.test_gpu_attn_stream import to_dev
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

LDS_MAX = 160 * 1024
GROUP_MAX = 8
HEAD_DIMS = [64, 128]
GRID_BATCHES = ((0,), (31, 32, 33), (63,), SHUFFLED)
GRID = [(2, 2), (4, 2), (6, 2), (8, 2), (8, 1)]  # group sizes 1, 2, 3, 4, 8; (16, 1) has its own test
STRIDE_HEADS = [(6, 2), (8, 2), (8, 1), (16, 1)]  # group sizes 3, 4, 8, 16
QSCALES = [0.05, 2.0, 40.0, MIXED]
QSCALE_IDS = ["flat", "normal", "peaked", "mixed"]


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


@pytest.fixture(params=[0, 1], ids=["group", "head"])
def prompt_form(request):
    """Runs a test on both prompt-attention kernels (per kv group and token, the default where the
    group's rows fit; per query head and token, forced by mi355x_attn_prompt_impl)."""
    import ggml_mi355x as g
    prev = g.attn_prompt_impl(request.param)
    yield request.param
    g.attn_prompt_impl(prev)


def group_lds(hd, n_ctx, gsz):
    """attn_prompt_group_lds of ggml-neon-opt_amd/csrc/kq_ops.hip: q16 | w | p16 | scal per query head of the group."""
    return gsz * (2 * hd + 6 * n_ctx + 16)


def expected_form(hd, nh, nkv, n_ctx, selector):
    gsz = nh // nkv
    return "group" if gsz <= GROUP_MAX and group_lds(hd, n_ctx, gsz) <= LDS_MAX and selector == 0 else "head"


def instantiation(hd, nh, nkv, n_ctx, selector):
    """The kernel instantiation launch_attn_prompt picks (the logged name carries HD only)."""
    if expected_form(hd, nh, nkv, n_ctx, selector) == "head":
        return "kq_attn_prompt<%d>" % hd
    gsz = nh // nkv
    return "kq_attn_prompt_group<%d, %d>" % (hd, gsz if gsz in (4, 8) else 0)


def cache_mismatch(dev_cache, ref):
    """None where the device cache holds the reference's bits, else (count, first indices)."""
    bad = np.argwhere(dev_cache.cpu().numpy().view(np.uint16) != ref)
    return (len(bad), bad[:4].tolist()) if len(bad) else None


def check_rows(got, ref, pos, n_ctx, tag):
    for i, p in enumerate(pos):
        if 0 <= p < n_ctx:
            assert bits_equal(got[i], ref[i]), (tag, "token", i, "pos", p, first_mismatch(got[i], ref[i]))
        else:
            assert np.isnan(got[i]).all(), (tag, "token", i, "pos", p)


def check_form(names, hd, form):
    """Exactly one kq_kv_store and the expected attention kernel, nothing else."""
    assert sum("kq_kv_store<%d>" % hd in n for n in names) == 1 and len(names) == 2, names
    group = sum("kq_attn_prompt_group<%d>" % hd in n for n in names)
    head = sum("kq_attn_prompt<%d>" % hd in n for n in names)
    assert (group, head) == ((1, 0) if form == "group" else (0, 1)), (form, names)


def run_case(dev, O, hd, nh, nkv, n_ctx, batches, selector, qscale=2.0):
    """Every batch of the case through mi355x_attn_prompt on the same evolving device caches: each
    output row and both whole caches against the reference, the form from the first call's launches."""
    import ggml_mi355x as g
    assert g.attn_stream(0) == 0  # mode 0 (the default)
    form = expected_form(hd, nh, nkv, n_ctx, selector)
    kc0, vc0, steps = case_reference(O, hd, nh, nkv, n_ctx, batches, qscale)
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    kc, vc = to_dev(kc0, dev), to_dev(vc0, dev)
    for bi, (pos, q, k, v, ref, kc_ref, vc_ref) in enumerate(steps):
        if bi == 0:
            g.timing_enable(True)
        try:
            got = g.attn_prompt(t(q.copy(), dev), t(k.copy(), dev), t(v.copy(), dev), t(np.asarray(pos, np.int32), dev), tab,
                                kc, vc, nh, nkv, hd, scale_of(hd)).cpu().numpy()
            if bi == 0:
                names = [r[0] for r in g.timing_read()]
                print("launched", instantiation(hd, nh, nkv, n_ctx, selector), names)
                check_form(names, hd, form)
        finally:
            if bi == 0:
                g.timing_enable(False)
        check_rows(got, ref, pos, n_ctx, ("batch", bi))
        assert cache_mismatch(kc, kc_ref) is None, ("k cache, batch", bi, cache_mismatch(kc, kc_ref))
        assert cache_mismatch(vc, vc_ref) is None, ("v cache, batch", bi, cache_mismatch(vc, vc_ref))


# ---------------------------------------------------------------- 1a: the group-size grid
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", GRID)
def test_group_size_grid(dev, O, prompt_form, hd, nh, nkv):
    """64 cells, group sizes 1, 2, 3 (GSZ 0), 4 and 8 on both forms; four batches on the same evolving
    caches: the first cell alone, three tokens across the 32-cell boundary, the last cell alone, and
    nine tokens in shuffled order (the kernels take the latest tokens first and store every cell
    before any query runs: the result must not depend on the batch order)."""
    run_case(dev, O, hd, nh, nkv, 64, GRID_BATCHES, prompt_form)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_group_of_sixteen_takes_the_head_kernel(dev, O, hd):
    """Group size 16 is past the group kernel's 8 heads: the per-head kernel under the default selector."""
    assert expected_form(hd, 16, 1, 64, 0) == "head"
    run_case(dev, O, hd, 16, 1, 64, GRID_BATCHES, 0)


# ---------------------------------------------------------------- 1b: strides and tails
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", STRIDE_HEADS[:3])
def test_strides_and_tails(dev, O, prompt_form, hd, nh, nkv):
    """320 cells (no multiple of the 256-thread stride), 40 tokens at 250..289: n_kv 256, 288 and 320
    (= n_ctx, the clamp) in one batch, so the cell loops take a second, partial pass for some rows of
    the batch and not for others; group sizes 3, 4 and 8 on both forms."""
    run_case(dev, O, hd, nh, nkv, 320, STRIDE_BATCH, prompt_form)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_strides_and_tails_sixteen_heads(dev, O, hd):
    run_case(dev, O, hd, 16, 1, 320, STRIDE_BATCH, 0)


# ---------------------------------------------------------------- 1c: soft_max's sum
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("nh,nkv", [(6, 2), (8, 1)])
@pytest.mark.parametrize("qscale", QSCALES, ids=QSCALE_IDS)
def test_softmax_sum_tree_and_fallback(dev, O, prompt_form, hd, nh, nkv, qscale):
    """The 320-cell batch with q scaled as in tests/test_gpu_ops.py::test_attn_softmax_sum_tree_and_fallback
    (its docstring: flat scores keep every group sum near 4, the exact wave tree; N(0, 2) scores; very
    peaked ones put group sums far below the tree's bound: the in-order sum, which the group kernel runs
    one lane per row for all rows at once), over 64, 72 and 80 groups of 4 cells; group sizes 3 and 8.
    Here the flat and the N(0, 2) rows all take the tree and the peaked ones all take the in-order sum,
    so "mixed" scales the even heads by 40 and the odd ones by 0.05: every workgroup of the group kernel
    then holds rows of both kinds (tests/test_ops_oracle.py::test_prompt_softmax_cases_reach_both_sums
    restates the bound and pins which sum each case reaches)."""
    run_case(dev, O, hd, nh, nkv, 320, STRIDE_BATCH, prompt_form, qscale=qscale)


# ---------------------------------------------------------------- 1d: the LDS boundary
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("n_ctx,form", [(3360, "group"), (3392, "head")])
def test_lds_boundary_between_the_forms(dev, O, hd, n_ctx, form):
    """Eight heads in one group: their rows fit 160 KiB at 3360 cells and not at 3392, where the launch
    falls back to the per-head kernel by itself; both give the reference's bits."""
    assert expected_form(hd, 8, 1, n_ctx, 0) == form
    run_case(dev, O, hd, 8, 1, n_ctx, ((0, 3300, n_ctx - 33, n_ctx - 32, n_ctx - 1),), 0)


# ---------------------------------------------------------------- 1e: positions outside the cache
def bad_batch(n_ctx):
    return ((0, 1, n_ctx + 3, 3, -1),)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_bad_positions(dev, O, prompt_form, hd):
    """Tokens 2 and 4 have no cell: their rows are NaN, the other rows are the reference's bits, and
    every cell but 0, 1 and 3 keeps its junk (group size 4, both forms)."""
    run_case(dev, O, hd, 8, 2, 64, bad_batch(64), prompt_form)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_bad_positions_sixteen_heads(dev, O, hd):
    run_case(dev, O, hd, 16, 1, 64, bad_batch(64), 0)


# ---------------------------------------------------------------- 2: the two graph fusions
Q4_K, Q6_K = 12, 14
GRAPH_T, GRAPH_E, GRAPH_OUT = 37, 512, 256
# the activation quantizer's logged name (ggml-neon-opt_amd/csrc/kq_gemv_host.hip: launch_quantize_q8L)
QUANTIZE = "kq_quantize_q8L"


def whole_superblocks(hd, nh, nkv):
    """attn_prompt_q8_ok's first rule: a group's slice of the output row is whole 256-element superblocks."""
    return (nh // nkv) * hd % 256 == 0


def staging_fits(hd, n_ctx):
    """Its second: the group's score rows (gsz * n_ctx floats) hold the staged outputs (gsz * hd floats)."""
    return n_ctx >= hd


def run_graph(dev, O, oracle, hd, nh, nkv, n_ctx, v_type, q8_output, bad_token=None):
    """k = MUL_MAT(wk, x), v = MUL_MAT(wv, x), att = ATTN_DECODE(q, k, v, pos, kc, vc, tab), o = MUL_MAT(wo,
    att) over 37 tokens at 20..56, eager and replayed twice from junk caches each time: k, v, att, o and
    both caches row by row against oracle.mul_mat and the reference above. From the eager pass's launches:
    no kq_kv_store (the GEMM's epilogue stored the cells) and one activation quantize (x) where the
    attention writes the o-proj's Q8L rows, two where it cannot."""
    import torch
    import ggml_mi355x as g
    from tests import llama_model as LM
    T, E, NO, kvw = GRAPH_T, GRAPH_E, GRAPH_OUT, nkv * hd
    rng = np.random.default_rng([hd, nh, nkv, n_ctx, v_type, 0 if bad_token is None else 1 + bad_token])
    wk, wv = LM.kquant(rng, Q4_K, kvw, E), LM.kquant(rng, v_type, kvw, E)
    wo = LM.kquant(rng, Q4_K, NO, nh * hd)
    x = rng.standard_normal((T, E)).astype(np.float32)
    q = (rng.standard_normal((T, nh * hd)) * 2).astype(np.float32)
    pos = np.arange(20, 20 + T, dtype=np.int32)
    if bad_token is not None:
        pos[bad_token] = n_ctx + 1
    kc0, vc0 = rand_caches(rng, n_ctx, kvw)
    k_ref, v_ref = oracle.mul_mat(Q4_K, wk, x), oracle.mul_mat(v_type, wv, x)
    kc_ref, vc_ref = kc0.copy(), vc0.copy()
    att_ref = ref_attn_prompt(O, q, k_ref, v_ref, pos.tolist(), kc_ref, vc_ref, O.rope_table(n_ctx, hd, 10000.0), nh, nkv,
                              hd)
    good = [i for i in range(T) if i != bad_token]
    o_ref = oracle.mul_mat(Q4_K, wo, np.nan_to_num(att_ref))  # (the bad token's o row is not compared)

    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
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
    wvt = g.make_tensor(v_type, E, kvw, d["wv"].data_ptr())
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
        for pi, use_graph in enumerate((0, 1, 1)):
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
                    print("graph launches", instantiation(hd, nh, nkv, n_ctx, 0), names)
                    assert not any("kq_kv_store" in n for n in names), names
                    assert sum("kq_attn_prompt_group<%d>" % hd in n for n in names) == 1, names
                    assert sum(QUANTIZE in n for n in names) == (1 if q8_output else 2), names
            finally:
                if pi == 0:
                    g.timing_enable(False)
            got = {name: d[name].cpu().numpy() for name in ("k", "v", "att", "o")}
            for i in range(T):
                assert bits_equal(got["k"][i], k_ref[i]), (pi, "k", i, first_mismatch(got["k"][i], k_ref[i]))
                assert bits_equal(got["v"][i], v_ref[i]), (pi, "v", i, first_mismatch(got["v"][i], v_ref[i]))
            check_rows(got["att"], att_ref, pos.tolist(), n_ctx, ("pass", pi, "att"))
            for i in good:
                assert bits_equal(got["o"][i], o_ref[i]), (pi, "o", i, first_mismatch(got["o"][i], o_ref[i]))
            assert cache_mismatch(d["kc"], kc_ref) is None, ("k cache, pass", pi, cache_mismatch(d["kc"], kc_ref))
            assert cache_mismatch(d["vc"], vc_ref) is None, ("v cache, pass", pi, cache_mismatch(d["vc"], vc_ref))
    finally:
        be.close()


# (hd, n_head, n_head_kv, n_ctx, the Q8L output applies). Each rule of attn_prompt_q8_ok is the only one
# that fails in some case: (128, 6, 2) over 128 cells has room to stage its outputs, and only its 384
# outputs per group (1.5 superblocks) keep the Q8L output off; (128, 8, x) over 64 cells has whole
# superblocks, and only the 64-float score rows (head_dim 128 needs 128 cells) keep it off. The wo of
# group size 3 at head_dim 64 would have 384 columns, no whole superblocks: no such MUL_MAT exists.
GRAPH_SHAPES = [(64, 8, 2, 64, True), (64, 8, 1, 64, True), (128, 8, 2, 128, True), (128, 8, 1, 128, True),
                (128, 6, 2, 128, False), (128, 8, 2, 64, False), (128, 8, 1, 64, False), (128, 6, 2, 64, False)]


@pytest.mark.parametrize("v_type", [Q4_K, Q6_K], ids=["q4k-q4k", "q4k-q6k"])
@pytest.mark.parametrize("hd,nh,nkv,n_ctx,q8_output", GRAPH_SHAPES)
def test_graph_kv_epilogue_and_q8_output(dev, O, oracle, hd, nh, nkv, n_ctx, q8_output, v_type):
    """Group sizes 4 and 8 at both head sizes with the Q8L output; without it group size 3 over 128 cells
    (384 outputs per group: no whole superblocks, the only rule that fails there), group sizes 4 and 8 at
    head_dim 128 over 64 cells (only the staging room fails) and group size 3 over 64 cells (both); wk /
    wv Q4_K / Q4_K (kq_mmq) and Q4_K / Q6_K (kq_mmq_mixed). The o rows are exact either way."""
    assert expected_form(hd, nh, nkv, n_ctx, 0) == "group"
    assert q8_output == (whole_superblocks(hd, nh, nkv) and staging_fits(hd, n_ctx))
    off = [(whole_superblocks(s[0], s[1], s[2]), staging_fits(s[0], s[3])) for s in GRAPH_SHAPES if not s[4]]
    assert (False, True) in off and (True, False) in off  # each rule alone turns it off in some case
    run_graph(dev, O, oracle, hd, nh, nkv, n_ctx, v_type, q8_output)


@pytest.mark.parametrize("v_type", [Q4_K, Q6_K], ids=["q4k-q4k", "q4k-q6k"])
def test_graph_bad_position(dev, O, oracle, v_type):
    """Position 30 replaced by n_ctx + 1 (the epilogue's own range check): that token's att row is NaN,
    its cell and every other unowned cell keep their junk, every other att and o row is exact."""
    run_graph(dev, O, oracle, 64, 8, 2, 64, v_type, True, bad_token=10)
