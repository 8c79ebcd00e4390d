"""mi355x_small_batch FUSED below 16 columns, one backend graph per planner pattern, every output
against the CPU oracle by bits and every launch by name (eager runs under timing_enable): the
plain-layout prologues kq_rms_norm_q8L / kq_swiglu_q8L, their refusals, the M-column residual of
MmAdd, strided activations / outputs / residuals with poisoned gaps, the quantized-activation cache
(Q8State) kept and dropped, the joint layout that does not fit, and K past the widest layout.
K = 768 is three superblocks (a step that is not full); N = 70 and 9 leave a partial last wave.
M = 1 (kq_rows) and M = 16 (kq_mmq) are the boundaries on either side of kq_rows_cols."""
import numpy as np
import pytest

from tests.llama_model import kquant
from tests.test_gpu_parity import bits_equal, first_mismatch
from tests.test_gpu_rows_cols import _timed

pytestmark = pytest.mark.gpu

K, EPS = 768, 1e-5
COLS = [2, 8, 9, 15]
POISON = 0x7FC0BEEF  # a quiet NaN no kernel here produces: the words between strided columns


@pytest.fixture(autouse=True)
def fused():
    import ggml_mi355x as g
    prev = g.small_batch(g.SMALL_BATCH_FUSED)
    yield
    g.small_batch(prev)
    assert g.small_batch() == g.SMALL_BATCH_NODES


def _x(rng, M, k=K):
    """One column with an all-zero superblock (a Q8 block with d = 0), one column 1000 times the
    others and one with spikes (block scales far apart between neighbouring columns)."""
    x = rng.standard_normal((M, k)).astype(np.float32)
    x[0] *= 1000.0
    x[M - 1, ::97] *= 64.0
    x[M // 2, 256:512] = 0.0
    return x


class _Graph:
    """A backend, its device buffers and a node list. f32 tensors are [n, M] with rows `stride`
    floats apart; every buffer is filled with POISON before the run."""

    def __init__(self, seed):
        import ggml_mi355x as g
        self.g, self.be, self.rng = g, g.Backend(0), np.random.default_rng(seed)
        self.nodes, self.keep = [], []

    def _up(self, a):
        p = self.be.alloc(a.nbytes)
        self.be.set_tensor(p, np.ascontiguousarray(a))
        return p

    def _padded(self, M, n, stride, a=None):
        h = np.full((M, stride or n), POISON, np.uint32)
        if a is not None:
            h[:, :n] = np.ascontiguousarray(a, np.float32).view(np.uint32)
        return h

    def leaf(self, a, stride=None, data=None):
        a = np.atleast_2d(a)
        M, n = a.shape
        t = self.g.make_tensor(self.g.TYPE_F32, n, M, data or self._up(self._padded(M, n, stride, a)),
                               row_stride=4 * (stride or n))
        self.keep.append(t)
        return t

    def weight(self, type_, N, k=K):
        w = kquant(self.rng, type_, N, k, edges=True)
        t = self.g.make_tensor(type_, k, N, self._up(w))
        self.keep.append(t)
        return w, t

    def node(self, op, n, M, srcs, stride=None, data=None, params=None, flags=0):
        t = self.g.make_tensor(self.g.TYPE_F32, n, M, data or self._up(self._padded(M, n, stride)),
                               row_stride=4 * (stride or n), op=op, srcs=srcs, op_params=params, flags=flags)
        self.nodes.append(t)
        return t

    def mm(self, wt, x, N, M, **kw):
        return self.node(self.g.OP_MUL_MAT, N, M, [wt, x], **kw)

    def run(self, expect=0):
        rc, names = _timed(lambda: self.be.graph_compute(self.nodes, use_graph=0))
        assert rc == expect, rc
        self.be.synchronize()
        return names

    def words(self, t):
        """The tensor's whole buffer, gaps included, as uint32 [M, stride]."""
        h = np.zeros((t.ne[1], t.nb[1] // 4), np.uint32)
        self.be.get_tensor(h, t.data)
        self.be.synchronize()
        return h

    def check(self, t, ref, what=""):
        h, n = self.words(t), t.ne[0]
        got = np.ascontiguousarray(h[:, :n]).view(np.float32)
        assert bits_equal(got, ref), (what, first_mismatch(got, ref))
        assert (h[:, n:] == POISON).all(), (what, "the gap between two columns was written")

    def close(self):
        self.be.close()


@pytest.fixture
def new_graph():
    """_Graph(seed) whose backend is closed after the test, passed or failed."""
    made = []

    def make(seed):
        made.append(_Graph(seed))
        return made[-1]
    yield make
    for c in made:
        c.close()


def _count(names, part):
    return sum(part in n for n in names)


def _check_launches(names, M, prologue, quantize):
    """2 .. 15 columns: one kq_rows_cols behind `prologue` (or `quantize` kq_quantize_q8L launches),
    never the per-node path. 1 column: kq_rows. 16: kq_mmq. Neither boundary launches kq_rows_cols."""
    assert not any("kq_gemv<" in n or "kq_quantize_q8K" in n for n in names), names
    if M == 1:
        assert _count(names, "kq_rows_cols") == 0 and _count(names, "kq::kq_rows<") == 1, names
        return
    assert _count(names, "kq_rows_cols") == (1 if M < 16 else 0) and (_count(names, "kq_mmq") > 0) == (M >= 16), names
    assert _count(names, "kq_quantize") == quantize, names
    if prologue:
        assert _count(names, prologue) == 1, names


# ------------------------------------------------------------------ RMS_NORM -> MUL -> three MUL_MATs
def _norm_graph(c, oracle, M, flags=0, extra_reader=False):
    from oracle import kq_ops_oracle as O
    g = c.g
    x, nw = _x(c.rng, M), c.rng.uniform(0.5, 1.5, K).astype(np.float32)
    n0 = c.node(g.OP_RMS_NORM, K, M, [c.leaf(x)], params=[g.f32_bits(EPS)])
    n1 = c.node(g.OP_MUL, K, M, [n0, c.leaf(nw)], flags=flags)
    normed = np.stack([O.mul(O.rms_norm(row, EPS), nw) for row in x])
    out = []
    for type_, N in ((12, 70), (12, 9), (14, 70)):
        w, wt = c.weight(type_, N)
        out.append((c.mm(wt, n1, N, M), oracle.mul_mat(type_, w, normed)))
    if extra_reader:
        r = c.rng.standard_normal((M, K)).astype(np.float32)
        out.append((c.node(g.OP_ADD, K, M, [n1, c.leaf(r)]), np.stack([O.add(a, b) for a, b in zip(normed, r)])))
    return n1, normed, out


@pytest.mark.parametrize("M", [1] + COLS + [16])
def test_norm_prologue(dev, new_graph, oracle, M):
    """The normed activation is never written as f32: kq_rms_norm_q8L leaves its Q8L blocks (the plain
    layout below 16 columns, kq_mmq's at 16) and the three matrices (Q4_K, Q4_K, Q6_K) run in one launch."""
    c = new_graph(100 + M)
    _, _, out = _norm_graph(c, oracle, M)
    names = c.run()
    _check_launches(names, M, "kq_rms_norm_q8L", 0)
    for i, (t, ref) in enumerate(out):
        c.check(t, ref, i)


@pytest.mark.parametrize("why", ["output", "reader"])
@pytest.mark.parametrize("M", COLS)
def test_norm_prologue_refused(dev, new_graph, oracle, M, why):
    """The MUL's output is a graph output, or an ADD after the matrices reads it too: the f32 tensor must
    exist, so the prologue is refused and the activation is quantized from it, once, for one launch."""
    c = new_graph(200 + M)
    n1, normed, out = _norm_graph(c, oracle, M, flags=c.g.FLAG_OUTPUT if why == "output" else 0,
                                  extra_reader=why == "reader")
    names = c.run()
    assert _count(names, "kq_rms_norm_q8L") == 0, names
    _check_launches(names, M, None, 1)
    c.check(n1, normed, "normed")
    for i, (t, ref) in enumerate(out):
        c.check(t, ref, i)


@pytest.mark.parametrize("mode", ["fused", "nodes"])
@pytest.mark.parametrize("where", ["norm_src", "norm_mul", "swiglu"])
def test_prologue_over_strided_rows_is_refused_whole(dev, new_graph, where, mode):
    """Both prologues and the elementwise kernels behind them (kq_rms_norm, kq_mul, kq_swiglu) walk packed
    rows, so an activation with rows K + 8 floats apart has no right result on this backend: supports_op
    refuses the RMS_NORM, MUL or SWIGLU node and graph_compute returns E_UNSUPPORTED before any launch,
    under FUSED and under NODES alike. Nothing is written: every output keeps its poison."""
    import ggml_mi355x as g
    prev = g.small_batch(g.SMALL_BATCH_FUSED if mode == "fused" else g.SMALL_BATCH_NODES)
    try:
        c, M, S = new_graph(5), 3, K + 8
        x = _x(c.rng, M)
        if where == "swiglu":
            act = c.node(g.OP_SWIGLU, K, M, [c.leaf(x, stride=S), c.leaf(x[::-1], stride=S)], stride=S)
        else:
            n0 = c.node(g.OP_RMS_NORM, K, M, [c.leaf(x, stride=S if where == "norm_src" else None)],
                        params=[g.f32_bits(EPS)])
            act = c.node(g.OP_MUL, K, M, [n0, c.leaf(x[0])], stride=S if where == "norm_mul" else None)
        assert not g.supports_op(act if where != "norm_src" else n0)
        y = c.mm(c.weight(12, 9)[1], act, 9, M)
        assert c.run(expect=g.E_UNSUPPORTED) == []
        assert (c.words(y) == POISON).all() and (c.words(act) == POISON).all()
    finally:
        g.small_batch(prev)


# ------------------------------------------------------------------ SWIGLU -> MUL_MAT -> ADD
def _swiglu_graph(c, oracle, M, N=70, res_stride=None, out_stride=None):
    from oracle import kq_ops_oracle as O
    g = c.g
    gate, up = _x(c.rng, M), c.rng.standard_normal((M, K)).astype(np.float32)
    gt, ut = c.leaf(gate), c.leaf(up)
    sw = c.node(g.OP_SWIGLU, K, M, [gt, ut])
    h = np.stack([O.swiglu(a, b) for a, b in zip(gate, up)])
    w, wt = c.weight(14, N)
    mm = c.mm(wt, sw, N, M)
    res = c.rng.standard_normal((M, N)).astype(np.float32) * np.arange(1, M + 1, dtype=np.float32)[:, None]
    rt = c.leaf(res, stride=res_stride)
    ad = c.node(g.OP_ADD, N, M, [mm, rt], stride=out_stride)
    ref = np.stack([O.add(a, b) for a, b in zip(oracle.mul_mat(14, w, h), res)])
    return (gt, ut, sw, h), (rt, res), (ad, ref)


@pytest.mark.parametrize("M", [1] + COLS + [16])
def test_swiglu_prologue_and_m_column_residual(dev, new_graph, oracle, M):
    """kq_swiglu_q8L, then the Q6_K matrix with the ADD folded in: a residual of M columns, every column
    different (and scaled by its index), so a residual column stride of 0 or of one column shows."""
    c = new_graph(300 + M)
    _, _, (ad, ref) = _swiglu_graph(c, oracle, M)
    names = c.run()
    _check_launches(names, M, "kq_swiglu_q8L", 0)
    assert _count(names, "kq_add") == 0 and _count(names, "kq::kq_swiglu") == (0 if M == 1 else 1), names
    c.check(ad, ref)


@pytest.mark.parametrize("M", COLS)
def test_mm_add_strided_residual_and_output(dev, new_graph, oracle, M):
    """MmAdd's res_cs and y_cs: the residual's columns N + 4 floats apart, the output's N + 8."""
    c = new_graph(400 + M)
    _, (rt, res), (ad, ref) = _swiglu_graph(c, oracle, M, res_stride=70 + 4, out_stride=70 + 8)
    before = c.words(rt)
    names = c.run()
    _check_launches(names, M, "kq_swiglu_q8L", 0)
    assert _count(names, "kq_add") == 0, names
    c.check(ad, ref)
    assert (c.words(rt) == before).all()


@pytest.mark.parametrize("M", COLS)
def test_mm_multi_strided_activation_and_outputs(dev, new_graph, oracle, M):
    """MmMulti: two matrices on an f32 activation with nb[1] = (K + 8) * 4, outputs with nb[1] = (N + 4) * 4."""
    c = new_graph(600 + M)
    x = _x(c.rng, M)
    xt = c.leaf(x, stride=K + 8)
    out = []
    for type_, N in ((12, 70), (14, 9)):
        w, wt = c.weight(type_, N)
        out.append((c.mm(wt, xt, N, M, stride=N + 4), oracle.mul_mat(type_, w, x)))
    before = c.words(xt)
    names = c.run()
    _check_launches(names, M, None, 1)
    for i, (t, ref) in enumerate(out):
        c.check(t, ref, i)
    assert (c.words(xt) == before).all()


# ------------------------------------------------------------------ the quantized activation, kept and dropped
@pytest.mark.parametrize("M", COLS)
def test_activation_requantized_after_a_matrix_wrote_over_it(dev, new_graph, oracle, M):
    """The M-column form of test_fusion_respects_reused_buffers_and_views. A and B on x share a launch;
    C (N = K, through a second descriptor of x's bytes, so that it is a launch of its own) reuses x's
    blocks and writes its output over x; D on tensor x must then read C's output, not the blocks of
    the old contents: Q8State::drop_if_overlaps after C, a second kq_quantize_q8L before D."""
    c = new_graph(700 + M)
    x = _x(c.rng, M)
    xt = c.leaf(x)
    xv = c.leaf(x, data=xt.data)
    (wa, at), (wb, bt), (wc, ct), (wd, dt) = c.weight(12, 70), c.weight(14, 9), c.weight(12, K), c.weight(13, 70)
    a, b = c.mm(at, xt, 70, M), c.mm(bt, xt, 9, M)
    cc = c.mm(ct, xv, K, M, data=xt.data)
    d = c.mm(dt, xt, 70, M)
    names = c.run()
    assert _count(names, "kq_rows_cols") == 3 and _count(names, "kq_quantize_q8L") == 2 and len(names) == 5, names
    c_ref = oracle.mul_mat(12, wc, x)
    c.check(a, oracle.mul_mat(12, wa, x), "A")
    c.check(b, oracle.mul_mat(14, wb, x), "B")
    c.check(cc, c_ref, "C")
    c.check(d, oracle.mul_mat(13, wd, c_ref), "D")


@pytest.mark.parametrize("between", ["nothing", "add"])
@pytest.mark.parametrize("M", COLS)
def test_activation_kept_until_another_node_runs(dev, new_graph, oracle, M, between):
    """The complement: A and B on x, then C on x into a buffer of its own. With nothing between the
    launches (C reads x through a second descriptor of its bytes, so it is a launch of its own) C runs on
    the blocks A and B read: no second kq_quantize_q8L. With an unrelated ADD of two other tensors in
    between, the cache is reset and C quantizes again: the executor's rule is that any launch other than
    a batched MUL_MAT may have written the workspace or the activation (enqueue: `q8 = Q8State()`), and
    it does not ask what the node writes. That rule costs one launch here and is asserted as it is."""
    from oracle import kq_ops_oracle as O
    c = new_graph(800 + M)
    g = c.g
    x = _x(c.rng, M)
    xt = c.leaf(x)
    (wa, at), (wb, bt), (wc, ct) = c.weight(12, 70), c.weight(14, 9), c.weight(13, 70)
    a, b = c.mm(at, xt, 70, M), c.mm(bt, xt, 9, M)
    if between == "add":
        p, q = (c.rng.standard_normal((M, 64)).astype(np.float32) for _ in range(2))
        s = c.node(g.OP_ADD, 64, M, [c.leaf(p), c.leaf(q)])
    cc = c.mm(ct, xt if between == "add" else c.leaf(x, data=xt.data), 70, M)
    names = c.run()
    extra = 1 if between == "add" else 0
    assert _count(names, "kq_rows_cols") == 2 and _count(names, "kq_quantize_q8L") == 1 + extra, names
    assert _count(names, "kq_add") == extra and len(names) == 3 + 2 * extra, names
    c.check(a, oracle.mul_mat(12, wa, x), "A")
    c.check(b, oracle.mul_mat(14, wb, x), "B")
    c.check(cc, oracle.mul_mat(13, wc, x), "C")
    if between == "add":
        c.check(s, np.stack([O.add(u, v) for u, v in zip(p, q)]), "ADD")


# ------------------------------------------------------------------ layouts that do not fit
def test_joint_layout_refused_runs_one_launch_per_matrix(dev, new_graph, oracle):
    """rows_cols_plan takes one matrix, so the shape comes from plan_rows_cols' rules read in the source:
    a launch's layout depends on its matrices only through the widest ring of their types and through
    rows_per_wave, and n matrices of one type and N rows each split the waves as one matrix of n * N rows
    does. So at the widest K with a layout, four Q4_K matrices of N rows are refused together exactly
    where the planner refuses one of 4 N rows: N is the first such count (rows_per_wave 3 where one
    alone has 1). enqueue_cols_mm then quantizes once and launches each matrix alone.
    Why not 16 rows a matrix: with so few rows every wave holds one row, alone or together
    (rows_split_waves gives each matrix at least as many waves as rows), so rows_per_wave is 1 either way
    and the joint layout is the layout of its widest-ring matrix alone: it fits whenever each alone fits.
    Only rows_per_wave can grow in a joint launch, and that takes more rows than waves: 4 x 1025 rows of
    K = 15872 (37 MB of Q4_K, well under a second on the host and the device)."""
    import ggml_mi355x as g
    M = 3
    Kw = max(k for k in range(256, 1 << 15, 256) if g.rows_cols_plan(k, M) is not None)
    N = next(n for n in range(1, 1 << 16) if g.rows_cols_plan(Kw, M, n_rows=4 * n) is None)
    assert g.rows_cols_plan(Kw, M, n_rows=N)["rows_per_wave"] == 1 and g.rows_cols_plan(Kw, M, n_rows=3 * N) is not None
    c = new_graph(9)
    x = _x(c.rng, M, Kw)
    xt = c.leaf(x)
    out = []
    for _ in range(4):
        w, wt = c.weight(12, N, Kw)
        out.append((c.mm(wt, xt, N, M), oracle.mul_mat(12, w, x)))
    names = c.run()
    assert names == ["kq::kq_quantize_q8L"] + ["kq::kq_rows_cols<2>"] * 4, names
    for i, (t, ref) in enumerate(out):
        c.check(t, ref, i)


def test_past_the_widest_layout(dev, new_graph, oracle):
    """M = 4, N = 5. K = 16128 is the first K without a layout for a matrix of 4096 rows, but these five
    rows (one per wave, one chain batch) still have one there: a single kq_rows_cols<2>. The first K at
    which the planner refuses five rows too runs on the per-node path: kq_quantize_q8K and the GEMV, no
    kq_rows_cols. Oracle bits at both."""
    import ggml_mi355x as g
    M, N = 4, 5
    assert g.rows_cols_plan(16128, M) is None and g.rows_cols_plan(16128 - 256, M) is not None
    assert g.rows_cols_plan(16128, M, n_rows=N)["ncol"] == 2
    none = next(k for k in range(16128, 1 << 16, 256) if g.rows_cols_plan(k, M, n_rows=N) is None)
    for Kp, want in ((16128, ["kq::kq_quantize_q8L", "kq::kq_rows_cols<2>"]), (none, None)):
        c = new_graph(Kp)
        x = _x(c.rng, M, Kp)
        w, wt = c.weight(12, N, Kp)
        t = c.mm(wt, c.leaf(x), N, M)
        names = c.run()
        if want:
            assert names == want, (Kp, names)
        else:
            assert len(names) == 2 and names[0] == "kq::kq_quantize_q8K" and "kq_rows_cols" not in names[1], (Kp, names)
        c.check(t, oracle.mul_mat(12, w, x), Kp)
