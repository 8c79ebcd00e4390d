"""The rms_norm prologue of the decode GEMVs (kq_rows.hip RowsPrologue::norm / norm_late).

The norm interval skips its arithmetic on waves that hold no part of the row, totals the
superblock sums as a tree, and on the wide forms (32 and 64 lanes per superblock) stores the
quantized row from the fast total before the exactness guard, redoing it for an ambiguous row.
The redo is checked on the bytes of the workgroup's Q8_K row (mi355x_debug_rows_prologue),
bit-exact against the oracle's rms_norm, MUL and quantize_row_q8_K, with rows and epsilons for
which the fast and the sequential mean give different SCALES (SPLIT_CASES: the two means of an
order_split_rows row are neighbouring floats, and 1 / sqrt(mean + eps) is the same float for
both at eps = 0 and at most other eps), so a dropped or wrong redo multiplies every value by
another float. Every form is covered: (superblocks, waves) = (8, 6), (8, 12), (16, 12),
(16, 6), (32, 12) are the 32-, 64-, 32-, 16- and 16-lane forms. Then norm GEMVs through the
backend graph (RMS_NORM -> MUL -> MUL_MAT...), eager and replayed, on kq_rows, kq_rows_dyn and
the mixed-type q/k/v launch (kq_rows<7>, which picks the type's body per wave).
"""
import numpy as np
import pytest

from tests.adversarial import _seq_sumsq, order_split_rows
from tests.test_gpu_parity import bits_equal, first_mismatch
from tests.test_gpu_rows_prologue import check_blocks, run_prologue

gpu = pytest.mark.gpu

Q4, Q6 = 12, 14
# (superblocks, waves) -> lanes per superblock
FORMS = [((8, 6), 32), ((8, 12), 64), ((16, 12), 32), ((16, 6), 16), ((32, 12), 16)]
FORM_IDS = [f"nb{nb}w{w}" for (nb, w), _ in FORMS]

# (row of order_split_rows(n), eps) whose scale differs between the two means, per n: checked on
# the CPU by test_split_cases_separate_the_scale for every form that runs them
SPLIT_CASES = {2048: [(3, 1e-5), (0, 1e-3), (1, 1e-3), (4, 1e-3)],
               4096: [(1, 1e-5), (2, 1e-5), (3, 1e-5), (0, 1e-3), (5, 1e-3)],
               8192: [(4, 1e-5), (0, 1e-3), (2, 1e-3), (5, 1e-3)]}

_SPLIT = {}


def split_rows(n):
    """order_split_rows(n), built once per n and left unchanged."""
    if n not in _SPLIT:
        rows, ms, _ = order_split_rows(n)
        rows.setflags(write=False)
        _SPLIT[n] = (rows, ms)
    return _SPLIT[n]


def fast_mean(x, lanes):
    """numpy restatement of the prologue's fast order for a row of a power-of-two number of
    superblocks <= 64: the lane's 256 / lanes squares (float products) in order in double, a
    xor tree over the superblock's lanes, then a xor tree over the superblocks; the mean as
    the kernel rounds it (the double total times 1 / n, to float)."""
    x = np.asarray(x, np.float32)
    n = x.size
    nb, vp = n // 256, 256 // lanes
    assert nb & (nb - 1) == 0 and nb <= 64
    sums = []
    for b in range(nb):
        s = []
        for l in range(lanes):
            a = 0.0
            for v in x[256 * b + vp * l: 256 * b + vp * l + vp]:
                a += float(np.float32(v) * np.float32(v))
            s.append(a)
        step = 1
        while step < lanes:
            s = [s[i] + s[i ^ step] for i in range(lanes)]
            step *= 2
        sums.append(s[0])
    step = 1
    while step < nb:
        sums = [sums[i] + sums[i ^ step] for i in range(nb)]
        step *= 2
    return np.float32(sums[0] * (1.0 / n))


def norm_scale(mean, eps):
    """1.0f / sqrtf(mean + eps) in float arithmetic (add, sqrt and divide correctly rounded,
    as the kernel's and ggml's)."""
    return np.float32(1.0) / np.sqrt(np.float32(mean) + np.float32(eps))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_split_cases_separate_the_scale(form):
    """CPU only: for every (row, eps) of SPLIT_CASES the kernel's fast order (lanes per
    superblock of the form, superblocks as a tree) gives a float mean different from the
    sequential one AND a different scale 1 / sqrt(mean + eps), so a kernel that skipped the
    redo, or re-summed to the fast mean, would scale every value by another float."""
    (nb, _), lanes = form
    rows, ms = split_rows(256 * nb)
    assert len(SPLIT_CASES[256 * nb]) >= 4
    for r, eps in SPLIT_CASES[256 * nb]:
        assert ms[r] == np.float32(_seq_sumsq(rows[r]) / rows[r].size)
        fm = fast_mean(rows[r], lanes)
        assert fm != ms[r], (nb, lanes, r)
        assert norm_scale(fm, eps) != norm_scale(ms[r], eps), (nb, lanes, r, eps)


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


def norm_ref(oracle, O, x, w, eps):
    return oracle.quantize_q8_K(O.mul(O.rms_norm(x, eps), w))


@gpu
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_norm_prologue_image(dev, oracle, O, form):
    import ggml_mi355x as g
    (nb, waves), lanes = form
    K = 256 * nb
    assert g.rows_prologue_plan(K, waves) == (lanes, 1)
    rng = np.random.default_rng(1000 * nb + waves)
    w = rng.uniform(0.5, 1.5, K).astype(np.float32)

    def check(x, eps, what):
        got = run_prologue(g, dev, x, waves, prologue=g.PRO_RMS_NORM, x2=w, eps=eps)
        check_blocks(got, norm_ref(oracle, O, x, w, eps), (nb, waves, what))

    for rep in range(3):
        check((rng.standard_normal(K) * 3).astype(np.float32), 1e-5, ("random", rep))
    # the redo path of the wide forms (the sequential re-sum before the scale on 16 lanes)
    rows, _ = split_rows(K)
    for r, eps in SPLIT_CASES[K]:
        check(np.array(rows[r]), eps, ("order split", r, eps))
    x0 = (rng.standard_normal(K) * 3).astype(np.float32)
    for v, what in ((np.nan, "nan"), (np.inf, "inf")):
        for at in (0, K // 2 + 37, K - 1):
            x = x0.copy()
            x[at] = v
            check(x, 1e-5, (what, at))
    check(np.zeros(K, np.float32), 1e-5, "zero row")
    x = np.zeros(K, np.float32)
    x[K - 256:] = x0[K - 256:]
    check(x, 1e-5, "last superblock only")


# ---------------------------------------------------------------- norm GEMVs through the backend graph
def graph_case(g, be, x, nw, mats, eps):
    """RMS_NORM(x) -> MUL(norm weight) -> one MUL_MAT per (type, weights): (nodes, outputs)."""
    bufs = []

    def up(a=None, n=None):
        p = be.alloc(a.nbytes if a is not None else 4 * n)
        if a is not None:
            be.set_tensor(p, a)
        bufs.append(p)
        return p

    K = x.size
    xt = g.make_tensor(g.TYPE_F32, K, 1, up(x))
    nwt = g.make_tensor(g.TYPE_F32, K, 1, up(nw))
    n0 = g.make_tensor(g.TYPE_F32, K, 1, up(n=K), op=g.OP_RMS_NORM, src0=xt, op_params=[g.f32_bits(eps)])
    n1 = g.make_tensor(g.TYPE_F32, K, 1, up(n=K), op=g.OP_MUL, src0=n0, src1=nwt)
    outs = []
    for ty, wq in mats:
        wt = g.make_tensor(ty, K, wq.shape[0], up(wq))
        outs.append(g.make_tensor(g.TYPE_F32, wq.shape[0], 1, up(n=wq.shape[0]), op=g.OP_MUL_MAT, src0=wt, src1=n1))
    return [n0, n1] + outs, outs, bufs


def run_graph_case(g, be, oracle, O, x, nw, mats, eps, kernel):
    """Eager and two replays, outputs poisoned before each run; the one launch is `kernel`."""
    nodes, outs, bufs = graph_case(g, be, x, nw, mats, eps)
    xin = O.mul(O.rms_norm(x, eps), nw)
    refs = [oracle.mul_mat(ty, wq, xin[None])[0] for ty, wq in mats]
    be.synchronize()
    for run, use_graph in (("eager", 0), ("replay 1", 1), ("replay 2", 1)):
        for o in outs:
            be.set_tensor(o.data, np.full(o.ne[0], np.nan, np.float32))
        be.synchronize()
        if run == "eager":
            g.timing_enable(True)
        try:
            assert be.graph_compute(nodes, use_graph=use_graph) == 0
            be.synchronize()
            if run == "eager":
                names = [r[0] for r in g.timing_read()]
                assert names == [kernel], names
        finally:
            g.timing_enable(False)
        for o, ref in zip(outs, refs):
            h = np.zeros(o.ne[0], np.float32)
            be.get_tensor(h, o.data)
            be.synchronize()
            assert bits_equal(h, ref), (run, first_mismatch(h, ref))
    for p in bufs:
        be.free_buffer(p)


@pytest.fixture(params=[(0, 6), (0, 12), (3, 6), (3, 12)], ids=["rows6", "rows12", "dyn6", "dyn12"])
def kernel(request):
    import ggml_mi355x as g
    which, waves = request.param
    prev, prev_w = g.gemv_impl(which), g.gemv_waves(waves)
    yield "kq::kq_rows_dyn<1, true, 1>" if which == 3 else "kq::kq_rows<1, true, 1>"
    g.gemv_impl(prev)
    g.gemv_waves(prev_w)


@gpu
def test_norm_gemv_one_matrix(dev, oracle, npo, O, kernel):
    """One Q4_K matrix of 40 rows at K = 2048: some waves stream no rows, and at 6 waves two
    of them hold no part of the activation either."""
    import ggml_mi355x as g
    K, N = 2048, 40
    rng = np.random.default_rng(40)
    be = g.Backend(0)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    wq = npo.random_blocks(rng, Q4, N, K)
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    run_graph_case(g, be, oracle, O, x, nw, [(Q4, wq)], 1e-5, kernel)
    for r, eps in SPLIT_CASES[K][:2]:
        run_graph_case(g, be, oracle, O, np.array(split_rows(K)[0][r]), nw, [(Q4, wq)], eps, kernel)
    be.close()


@gpu
@pytest.mark.parametrize("K", [2048, 4096])
def test_norm_gemv_mixed_types(dev, oracle, npo, O, K):
    """The q/k/v launch with a Q6_K v (kq_rows<7>): Q4_K q (40 rows), Q4_K k (8), Q6_K v (8)."""
    import ggml_mi355x as g
    rng = np.random.default_rng(K)
    be = g.Backend(0)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
    mats = [(Q4, npo.random_blocks(rng, Q4, 40, K)), (Q4, npo.random_blocks(rng, Q4, 8, K)),
            (Q6, npo.random_blocks(rng, Q6, 8, K))]
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    run_graph_case(g, be, oracle, O, x, nw, mats, 1e-5, "kq::kq_rows<7, true, 1>")
    for r, eps in SPLIT_CASES[K][:2]:
        run_graph_case(g, be, oracle, O, np.array(split_rows(K)[0][r]), nw, mats, eps, "kq::kq_rows<7, true, 1>")
    be.close()
