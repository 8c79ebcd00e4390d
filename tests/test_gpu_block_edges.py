"""GPU: the super-block scales d / dmin that real GGUF files hold and the other tests' generators never
draw (oracle/kq_oracle_np.py edge_blocks: fp16 subnormals, +-0, negative and mixed signs, saturated scale
bytes, values up to +-65504; poison_blocks: +-inf and NaN), through every kernel that converts them:

  kq_ops.hip kq_get_rows                  test_get_rows_*
  kq_device.h records (kq_gemv)           test_gemv_* [tasks]
  kq_rows_device.h (kq_rows, kq_rows_dyn) test_gemv_* [rows, rows12, rows6, dyn, dyn6], test_gemv_stream_forms
  kq_mmq.hip (kq_mmq, kq_mmq_mixed)       test_prefill_exact, test_prefill_mixed_launch, test_poison_prefill_exact
  kq_mmf.hip (packed-f16 d * sc)          test_prefill_f16, test_poison_f16
  kq_attn_oproj.hip                       test_token_routes [oproj]
  kq_layer.hip                            test_token_routes [layer]

Bar: the exact paths on bits against the CPU oracle (ggml's vec_dot / dequantize_row restated); the f16 path
as tests/test_gpu_mmf.py holds it, per category. Row r of an edge matrix is of category
edge_category(r), which every failure message carries. Each reference is computed once per module.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_mmf import check as mmf_check
from tests.test_gpu_mmf import f16path  # noqa: F401  (fixture)
from tests.test_gpu_mmq_forms import MIXES, check_qkv_launch, forced, qkv_case  # noqa: F401  (forced: fixture)
from tests.test_gpu_parity import bits_equal, first_mismatch, t

pytestmark = pytest.mark.gpu

F32, Q4_K, Q5_K, Q6_K = 0, 12, 13, 14
QTYPES = [Q4_K, Q5_K, Q6_K]
QIDS = ["q4k", "q5k", "q6k"]


def npo_():
    from oracle import kq_oracle_np
    return kq_oracle_np


def categories(idx, n_rows, cats=None):
    """The categories of the matrix rows behind flat indices into an (M, n_rows) output."""
    npo = npo_()
    cats = npo.EDGE_CATS if cats is None else cats
    return sorted({npo.edge_category(int(i) % n_rows, cats) for i in idx})


def assert_bits(got, ref, n_rows, what):
    """got == ref on bits; the message names the categories of the first rows that differ."""
    mm = first_mismatch(got, ref)
    if mm is not None or not bits_equal(got, ref):
        raise AssertionError((what, "categories", categories(mm[1], n_rows) if mm else None, mm))


@functools.lru_cache(maxsize=None)
def edge_case(type_, K, N, M, first=0):
    """(w, x, oracle mul_mat) of an edge matrix with all nine categories on edge_activations."""
    from oracle import kq_oracle
    npo = npo_()
    rng = np.random.default_rng([type_, K, N, M, first])
    w = npo.edge_blocks(rng, type_, N, K)
    x = npo.edge_activations(rng, M, K, first)
    return w, x, kq_oracle.mul_mat(type_, w, x)


# ---------------------------------------------------------------- a: get_rows
GR_ROWS = 27  # three rows per category
GR_IDS = np.array([0, GR_ROWS - 1, 13, 13] + list(range(GR_ROWS)), np.int32)  # first, last, a repeat, every category


@functools.lru_cache(maxsize=None)
def get_rows_case(type_, K):
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    npo = npo_()
    rng = np.random.default_rng([type_, K, 7])
    if type_ == F32:
        table = rng.standard_normal((GR_ROWS, K)).astype(np.float32)
        table[1, :8] = [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-40, 3.4e38, -3.4e38]
    else:
        table = npo.edge_blocks(rng, type_, GR_ROWS, K)
    return table, kq_ops_oracle.get_rows(type_, table, K, GR_IDS)


def assert_get_rows(got, ref, K, what):
    mm = first_mismatch(got, ref)
    if mm is not None or not bits_equal(got, ref):
        rows = sorted({int(GR_IDS[i // K]) for i in mm[1]}) if mm else None
        raise AssertionError((what, "table rows", rows, "categories", categories(rows or [], GR_ROWS), mm))


@pytest.mark.parametrize("type_", [F32] + QTYPES, ids=["f32"] + QIDS)
@pytest.mark.parametrize("K", [256, 2304, 5632])
def test_get_rows_contiguous(dev, type_, K):
    """K = 256: one block, 224 threads past k. K = 2304: two chunks, the second of one block; the Q6_K row
    stride of 1890 B puts the odd rows off 16 B (the staging load's mis != 0). K = 5632: three chunks, the
    tail of six blocks; Q6_K stride 4620 B."""
    import ggml_mi355x as g
    table, ref = get_rows_case(type_, K)
    got = g.get_rows(type_, t(table, dev), K, t(GR_IDS, dev)).cpu().numpy()
    assert_get_rows(got, ref, K, (type_, K))


@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
@pytest.mark.parametrize("K", [256, 2304, 5632])
def test_get_rows_strided_view(dev, type_, K):
    """The table as a column view of a wider byte tensor: row_stride = row size + 6, the first row 2 bytes
    past a 16-byte boundary. The staging load reads whole 16-byte granules around a chunk, so the wide
    tensor keeps a spare row (more than 16 bytes) on both sides of the view."""
    import torch
    import ggml_mi355x as g
    table, ref = get_rows_case(type_, K)
    rs = table.shape[1]
    stride = rs + 6
    buf = torch.zeros(16 + (GR_ROWS + 2) * stride + 16, dtype=torch.uint8, device=dev)
    start = (-buf.data_ptr()) % 16 + (stride + 15) // 16 * 16  # a 16-byte boundary at least a row into buf
    view = buf[start:start + GR_ROWS * stride].view(GR_ROWS, stride)[:, 2:2 + rs]
    assert start >= 16 and buf.numel() - (start + GR_ROWS * stride) >= 16
    view.copy_(t(table, dev))
    assert view.stride(0) == stride and view.data_ptr() % 16 == 2
    got = g.get_rows(type_, view, K, t(GR_IDS, dev)).cpu().numpy()
    assert_get_rows(got, ref, K, (type_, K, "stride", stride))


# ---------------------------------------------------------------- b: decode GEMV
@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
@pytest.mark.parametrize("K,N", [(256, 27), (768, 45), (2304, 27)])
@pytest.mark.parametrize("M", [1, 3])
def test_gemv_one_type(dev, impl, type_, K, N, M):
    """One-type launches on every form of the decode GEMV. K = 2304: nine superblocks, Q6_K rows 2-byte
    aligned. M = 1 multiplies the alternating +-1 row (every q8 +-127), M = 3 the normal row, the row with a
    zero superblock and the +1 row."""
    import ggml_mi355x as g
    w, x, ref = edge_case(type_, K, N, M, 3 if M == 1 else 0)
    got = g.mul_mat(type_, t(w, dev), K, t(x, dev)).cpu().numpy()
    assert_bits(got, ref, N, (type_, K, N, M))


FUSED = [(Q4_K, 45), (Q6_K, 27), (Q5_K, 18)]


def test_gemv_fused_three_types(dev, impl):
    """Q4_K (45 rows) + Q6_K (27) + Q5_K (18) over one activation (the outlier row) at K = 768."""
    import torch
    import ggml_mi355x as g
    K = 768
    cases = [edge_case(ty, K, n, 1, 4) for ty, n in FUSED]
    x = cases[0][1]
    ys = [torch.full((n,), np.nan, device=dev) for _, n in FUSED]
    g.gemv_fused([(ty, t(c[0], dev), y) for (ty, _), c, y in zip(FUSED, cases, ys)], t(x[0], dev))
    from oracle import kq_oracle
    for (ty, n), c, y in zip(FUSED, cases, ys):
        assert_bits(y.cpu().numpy(), kq_oracle.mul_mat(ty, c[0], x)[0], n, ("fused", ty))


@pytest.fixture
def waves2():
    import ggml_mi355x as g
    prev = g.gemv_waves(2)
    yield
    g.gemv_waves(prev)


@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
def test_gemv_stream_forms(dev, waves2, type_):
    """The short-stream form (45 rows at K = 768: the plan says ROWS_SHORT) and the streaming loop, at the
    smallest launch for which the plan reports ROWS_LONG with two waves per workgroup at K = 2304 (the row
    count is searched through the plan, not assumed)."""
    import ggml_mi355x as g
    assert g.rows_stream_plan([(type_, 45)], 768)[2] == g.ROWS_SHORT
    K = 2304
    N = next((n for n in range(1, 40000) if g.rows_stream_plan([(type_, n)], K)[2] == g.ROWS_LONG), None)
    assert N is not None and N < 8192, N
    steps, depth, form = g.rows_stream_plan([(type_, N)], K)
    assert form == g.ROWS_LONG and steps > depth and g.rows_stream_plan([(type_, N - 1)], K)[2] == g.ROWS_SHORT
    for k, n, want in ((768, 45, g.ROWS_SHORT), (K, N, g.ROWS_LONG)):
        w, x, ref = edge_case(type_, k, n, 1, 3)
        g.timing_enable(True)
        try:
            got = g.mul_mat(type_, t(w, dev), k, t(x, dev)).cpu().numpy()
            names = [r[0] for r in g.timing_read()]
        finally:
            g.timing_enable(False)
        assert len(names) == 1 and names[0].startswith("kq::kq_rows<"), names
        assert g.rows_stream_plan([(type_, n)], k)[2] == want
        assert_bits(got, ref, n, (type_, k, n, "short" if want == g.ROWS_SHORT else "long"))


@pytest.mark.parametrize("pro", ["norm", "swiglu"])
def test_gemv_prologues_and_residual(dev, pro):
    """RMS_NORM -> MUL -> MUL_MAT(s) -> ADD and SWIGLU -> MUL_MAT -> ADD as one launch at K = 768 on edge
    weights: equal to the separate ops of the oracle."""
    import torch
    import ggml_mi355x as g
    from oracle import kq_oracle, kq_ops_oracle as O
    O.lib()
    npo = npo_()
    K = 768
    mats = [(Q4_K, 45), (Q6_K, 27)] if pro == "norm" else [(Q5_K, 45)]
    rng = np.random.default_rng(len(pro))
    x = npo.edge_activations(rng, 1, K, 4)[0]
    x2 = rng.uniform(0.5, 1.5, K).astype(np.float32) if pro == "norm" else rng.standard_normal(K).astype(np.float32)
    ws = [edge_case(ty, K, n, 1, 4)[0] for ty, n in mats]
    res = [rng.standard_normal(n).astype(np.float32) for _, n in mats]
    ys = [torch.full((n,), np.nan, device=dev) for _, n in mats]
    g.gemv_fused_ext([(ty, t(w, dev), y) for (ty, _), w, y in zip(mats, ws, ys)], t(x, dev),
                     prologue=g.PRO_RMS_NORM if pro == "norm" else g.PRO_SWIGLU, x2=t(x2, dev), eps=1e-5,
                     residual=[t(r, dev) for r in res])
    torch.cuda.synchronize()
    xin = O.mul(O.rms_norm(x, 1e-5), x2) if pro == "norm" else O.swiglu(x, x2)
    for (ty, n), w, r, y in zip(mats, ws, res, ys):
        assert_bits(y.cpu().numpy(), O.add(kq_oracle.mul_mat(ty, w, xin)[0], r), n, (pro, ty))


# ---------------------------------------------------------------- c: prefill GEMM, bit-exact path
MMQ_IDS = {0: "auto", 1: "tile64", 2: "tile128", 3: "tile128w", 4: "tile64w", 6: "tile192"}


MMQ_CASES = [(ty, m) for m in (0, 1, 2, 3, 4, 6) for ty in QTYPES if not (m == 6 and ty == Q6_K)]


@pytest.mark.parametrize("type_,mmq", MMQ_CASES, ids=["%s-%s" % (MMQ_IDS[m], QIDS[ty - Q4_K]) for ty, m in MMQ_CASES])
def test_prefill_exact(dev, forced, type_, mmq):
    """K = 768 (an odd superblock count), N = 90 (ten rows per category; a partial row tile at 64, 128 and
    192 rows), M = 20 (a partial column tile, every activation form four times). tile192 is a selector of
    Q4_K / Q5_K."""
    import ggml_mi355x as g
    forced(mmq)
    K, N, M = 768, 90, 20
    w, x, ref = edge_case(type_, K, N, M)
    g.timing_enable(True)
    try:
        got = g.mul_mat(type_, t(w, dev), K, t(x, dev)).cpu().numpy()
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
    assert sum("kq_mmq<%d>" % type_ in n for n in names) == 1, names
    assert_bits(got, ref, N, (type_, MMQ_IDS[mmq]))


def test_prefill_mixed_launch(dev, forced):
    """q (Q5_K) + k (Q5_K) + v (Q6_K) as one kq_mmq_mixed launch with the KV-cache epilogue, the weights with
    a random sign, +-0 and subnormals on their scales (tests/llama_model.py kquant(edges=True)): the route
    and the references of tests/test_gpu_mmq_forms.py (q / k / v on bits, the caches via cache_mismatch)."""
    forced(0)
    mix = MIXES[2]
    assert mix == (Q5_K, Q5_K, Q6_K)
    case = qkv_case(mix, True)
    plain = qkv_case(mix)
    assert not np.array_equal(case[0][0], plain[0][0]) and np.isfinite(case[5][0]).all()
    check_qkv_launch(dev, mix, case)


# ---------------------------------------------------------------- d: prefill GEMM, f16 path
@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
def test_prefill_f16(dev, oracle, npo, f16path, type_):
    """kq_mmf on the eight categories of its domain (EDGE_CATS_F16; maxf16 is outside: f16(d sc) overflows),
    ten rows each, all five activation forms (the 1e3-outlier rows are inside the domain). Held per category
    to tests/test_gpu_mmf.py's check: mmf_bound against the oracle, 2^-4 of it against the emulation, every
    output finite. Only one category's rows go into a bound: its second term takes the global max A."""
    import ggml_mi355x as g
    K, N, M = 768, 80, 20
    cats = npo.EDGE_CATS_F16
    rng = np.random.default_rng([type_, K, N, M])
    w = npo.edge_blocks(rng, type_, N, K, cats)
    x = npo.edge_activations(rng, M, K)
    g.timing_enable(True)
    try:
        got = g.mul_mat(type_, t(w, dev), K, t(x, dev)).cpu().numpy()
        names = [r[0] for r in g.timing_read()]
    finally:
        g.timing_enable(False)
    assert any("kq_mmf" in n for n in names) and not any("kq_mmq" in n for n in names), names
    failed = []
    for c, cat in enumerate(cats):
        rows = np.arange(c, N, len(cats))
        assert all(npo.edge_category(r, cats) == cat for r in rows)
        try:
            mmf_check(got, w, type_, K, x, oracle, npo, rows, np.arange(M))
        except AssertionError as e:
            nonfinite = int((~np.isfinite(got[:, rows])).sum())
            failed.append((cat, "non-finite outputs: %d" % nonfinite, str(e).splitlines()[0]))
    assert not failed, failed


# ---------------------------------------------------------------- e: non-finite scales stay in their row
P_K, P_N, P_M = 768, 70, 20
P_ROWS = [0, 33, 69]                  # first, middle and last of a tile
P_BITS = [0x7C00, 0xFC00, 0x7E00]     # +inf, -inf, NaN in the middle superblock's d


@functools.lru_cache(maxsize=None)
def poison_case(type_):
    from oracle import kq_oracle, kq_ops_oracle
    kq_ops_oracle.lib()
    npo = npo_()
    rng = np.random.default_rng([type_, 99])
    w = npo.poison_blocks(npo.random_blocks(rng, type_, P_N, P_K), type_, P_K, P_ROWS, P_BITS)
    x = npo.edge_activations(rng, P_M, P_K)
    ids = np.arange(P_N, dtype=np.int32)
    with np.errstate(all="ignore"):
        return w, x, kq_oracle.mul_mat(type_, w, x), kq_ops_oracle.get_rows(type_, w, P_K, ids)


def assert_poison(got, ref, row_of, what):
    """NaN exactly where the oracle has NaN (payload and sign not compared), the oracle's bits elsewhere;
    outside the poisoned rows the oracle has no NaN, so those rows are compared on bits."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32).reshape(np.shape(got))
    rows = row_of(np.arange(got.size)).reshape(got.shape)
    clean = ~np.isin(rows, P_ROWS)
    assert np.isfinite(ref[clean]).all() and not np.isfinite(ref[~clean]).all()
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = (gn != rn) | (~rn & (got.view(np.uint32) != ref.view(np.uint32)))
    if bad.any():
        i = np.flatnonzero(bad)[:5]
        raise AssertionError((what, "rows", rows.ravel()[i].tolist(), got.ravel()[i].tolist(), ref.ravel()[i].tolist()))


@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
def test_poison_get_rows(dev, type_):
    import ggml_mi355x as g
    w, _, _, ref = poison_case(type_)
    got = g.get_rows(type_, t(w, dev), P_K, t(np.arange(P_N, dtype=np.int32), dev)).cpu().numpy()
    assert_poison(got, ref, lambda i: i // P_K, ("get_rows", type_))


@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
def test_poison_gemv(dev, impl, type_):
    import ggml_mi355x as g
    w, x, ref, _ = poison_case(type_)
    got = g.mul_mat(type_, t(w, dev), P_K, t(x[:1], dev)).cpu().numpy()
    assert_poison(got, ref[:1], lambda i: i % P_N, ("gemv", type_))


@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
def test_poison_prefill_exact(dev, type_):
    import ggml_mi355x as g
    w, x, ref, _ = poison_case(type_)
    got = g.mul_mat(type_, t(w, dev), P_K, t(x, dev)).cpu().numpy()
    assert_poison(got, ref, lambda i: i % P_N, ("kq_mmq", type_))


@pytest.mark.parametrize("type_", QTYPES, ids=QIDS)
def test_poison_f16(dev, oracle, npo, f16path, type_):
    """kq_mmf: every other row within its bound (the check of tests/test_gpu_mmf.py), the poisoned rows
    non-finite in every column."""
    import ggml_mi355x as g
    w, x, _, _ = poison_case(type_)
    got = g.mul_mat(type_, t(w, dev), P_K, t(x, dev)).cpu().numpy()
    clean = np.array([r for r in range(P_N) if r not in P_ROWS])
    mmf_check(got, w, type_, P_K, x, oracle, npo, clean, np.arange(P_M))
    assert not np.isfinite(got[:, P_ROWS]).any(), got[:, P_ROWS]


# ---------------------------------------------------------------- f: a whole token on edge weights
TOK_CTX, TOK_SEED = 64, 41


def token_hp():
    from ggml_mi355x.llama import hparams
    return hparams(2048, 1, 32, 4, 1024, 1024)


@functools.lru_cache(maxsize=None)
def token_case(mix):
    """The model with edge scales on every matrix, 8 tokens, and the oracle's logits and last hidden state
    per token (kq_ops_oracle.decode_token)."""
    from oracle import kq_ops_oracle as O
    from tests import llama_model as LM
    O.lib()
    hp = token_hp()
    w = LM.build(hp, TOK_SEED, mix=mix, edges=True)
    model, cache = LM.oracle_model(hp, w, TOK_CTX)
    tokens = np.random.default_rng(TOK_SEED).integers(0, hp["n_vocab"], size=8).tolist()
    refs = []
    for p, tok in enumerate(tokens):
        logits, trace = O.decode_token(model, tok, p, cache)
        assert np.isfinite(logits).all()
        refs.append((np.array(logits, np.float32), np.array(trace[-1], np.float32)))
    return w, tokens, refs


@pytest.mark.parametrize("mix", ["q4_k_m", "q5_k_m"])
@pytest.mark.parametrize("route", ["nodes", "oproj", "layer"])
def test_token_routes(dev, mix, route):
    """One TinyLlama-width layer + a 1024-token head on edge weights, 8 tokens through the captured graph:
    the per-node fused launches, the attention + o-proj launch and the layer engine, each on bits against
    the oracle (logits and last hidden state), the launch names showing that the route's kernel ran. On
    the per-node route the same tokens as one prompt graph (the default, bit-exact precision) repeat the
    last token's logits."""
    import ggml_mi355x as g
    from tests import llama_model as LM
    from ggml_mi355x.llama import LlamaDecoder
    hp = token_hp()
    w, tokens, refs = token_case(mix)
    b = g.Backend()
    try:
        if route == "oproj":
            assert b.set_attn_oproj(True) == 0
        if route == "layer":
            assert b.set_layer_engine(True) == 0
        dec = LlamaDecoder(b, hp, LM.to_device(w, dev), TOK_CTX, fuse=True)
        g.timing_enable(True)
        try:
            dec.step(tokens[0], 0, use_graph=False)
            names = [r[0] for r in g.timing_read()]
        finally:
            g.timing_enable(False)
        b.synchronize()
        assert route != "nodes" or any("kq_get_rows" in n for n in names), names
        assert sum("kq_attn_oproj" in n for n in names) == (1 if route == "oproj" else 0), names
        assert sum("kq_layer" in n for n in names) == (1 if route == "layer" else 0), names
        assert any("kq_attn_decode" in n for n in names) == (route == "nodes"), names
        dec.reset()
        for p, tok in enumerate(tokens):
            dec.step(tok, p)
            b.synchronize()
            got, hid = dec.logits.cpu().numpy(), dec.last_hidden.cpu().numpy()
            assert bits_equal(hid, refs[p][1]), (route, p, "hidden", first_mismatch(hid, refs[p][1]))
            assert bits_equal(got, refs[p][0]), (route, p, "logits", first_mismatch(got, refs[p][0]))
        assert b.layer_error() == 0
        if route == "nodes":
            dec.reset()
            g.timing_enable(True)
            try:
                lg = dec.prompt(tokens, 0, use_graph=False)
                names = [r[0] for r in g.timing_read()]
            finally:
                g.timing_enable(False)
            b.synchronize()
            assert names and not any("kq_mmf" in n for n in names), names
            got = lg.cpu().numpy()
            assert bits_equal(got, refs[-1][0]), ("prompt", first_mismatch(got, refs[-1][0]))
    finally:
        b.close()
