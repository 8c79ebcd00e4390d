"""The short-stream form of the decode GEMV (kq_rows<..., SH = true>, kq_rows.hip).

A launch whose waves stream no more steps than their ring holds, and whose rows one chain batch
covers, issues its whole stream before the prologue's barrier and then runs the steps
straight-line; lane r keeps row r's result for the residual add and the store. The integer
sums, the records and the chain are the generic form's, so every output is bit-identical to
the oracle (ggml's vec_dot row by row, rms_norm / MUL / ADD / swiglu as ggml computes them)
AND to the generic form of the same library (knob GEMV_SHORT = 0), through graph_compute,
eager and replayed.

Shapes: K = 256 (16 rows per step), K = 2048 at 8 / 300 / 2048 rows (waves of 0, 1 and 2 rows),
K = 4096 (a row per step), K = 5632 (a row spans two steps), each in Q4_K, Q5_K and Q6_K; the
Q6_K tensors start at row 1 of their buffer where that is off a 16-byte boundary. The ring
boundary (exactly D steps: short; D + 1: the generic loop), the mixed q/k/v launch with the
norm prologue, gate + up with the SWIGLU epilogue over a row count that is no multiple of 4,
the residual ADD of o-proj and down, and a row whose norm is redone in ggml's order.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch
from tests.test_gpu_rows_norm import SPLIT_CASES, split_rows

gpu = pytest.mark.gpu

Q4, Q5, Q6 = 12, 13, 14
DEPTH = {Q4: 3, Q5: 3, Q6: 2}


@pytest.fixture(scope="module")
def O():
    from oracle import kq_ops_oracle
    kq_ops_oracle.lib()
    return kq_ops_oracle


@pytest.fixture(scope="module")
def be(dev):
    import ggml_mi355x as g
    b = g.Backend(0)
    yield b
    b.close()


class Case:
    """x [-> RMS_NORM -> MUL(norm weight)] -> one MUL_MAT per matrix [-> ADD(residual) each]
    [-> SWIGLU(gate, up)], as graph nodes with their oracle outputs."""

    def __init__(self, g, be, oracle, O, rng, K, mats, norm=False, residual=False, swiglu=False, x=None, eps=1e-5):
        self.be, self.bufs = be, []
        x = (rng.standard_normal(K) * 3).astype(np.float32) if x is None else np.array(x, np.float32)
        xt = g.make_tensor(g.TYPE_F32, K, 1, self.up(x))
        nodes, xin, src = [], x, xt
        if norm:
            nw = rng.uniform(0.5, 1.5, K).astype(np.float32)
            n0 = g.make_tensor(g.TYPE_F32, K, 1, self.up(n=K), op=g.OP_RMS_NORM, src0=xt, op_params=[g.f32_bits(eps)])
            src = g.make_tensor(g.TYPE_F32, K, 1, self.up(n=K), op=g.OP_MUL, src0=n0,
                                src1=g.make_tensor(g.TYPE_F32, K, 1, self.up(nw)))
            nodes += [n0, src]
            xin = O.mul(O.rms_norm(x, eps), nw)
        mms, refs = [], []
        for ty, wq in mats:
            N, rowb = wq.shape[0], wq.shape[1]
            # Q6_K: the tensor starts at row 1 of its buffer, off a 16-byte boundary where the
            # row size allows (the kernels take 4-byte aligned Q6_K rows)
            lead = 1 if ty == Q6 and rowb % 16 and rowb % 4 == 0 else 0
            buf = np.concatenate([np.zeros((lead, rowb), np.uint8), wq])
            wt = g.make_tensor(ty, K, N, self.up(buf) + lead * rowb)
            mms.append(g.make_tensor(g.TYPE_F32, N, 1, self.up(n=N), op=g.OP_MUL_MAT, src0=wt, src1=src))
            refs.append(oracle.mul_mat(ty, wq, xin[None])[0])
        nodes += mms
        self.outs, self.refs = list(mms), refs
        if residual:
            self.outs, self.refs = [], []
            for mm, ref in zip(mms, refs):
                r = rng.standard_normal(ref.size).astype(np.float32)
                ad = g.make_tensor(g.TYPE_F32, ref.size, 1, self.up(n=ref.size), op=g.OP_ADD, src0=mm,
                                   src1=g.make_tensor(g.TYPE_F32, ref.size, 1, self.up(r)))
                nodes.append(ad)
                self.outs.append(ad)
                self.refs.append(O.add(ref, r))
        if swiglu:
            N = refs[0].size
            sg = g.make_tensor(g.TYPE_F32, N, 1, self.up(n=N), op=g.OP_SWIGLU, src0=mms[0], src1=mms[1])
            nodes.append(sg)
            self.outs, self.refs = [sg], [O.swiglu(refs[0], refs[1])]
        self.nodes = nodes

    def up(self, a=None, n=None):
        p = self.be.alloc(a.nbytes if a is not None else 4 * n)
        if a is not None:
            self.be.set_tensor(p, np.ascontiguousarray(a))
        self.bufs.append(p)
        return p

    def run(self, g, use_graph, names=None):
        be = self.be
        for o in self.outs:
            be.set_tensor(o.data, np.full(o.ne[0], np.nan, np.float32))
        be.synchronize()
        if names is not None:
            g.timing_enable(True)
        try:
            assert be.graph_compute(self.nodes, use_graph=use_graph) == 0
            be.synchronize()
            if names is not None:
                names += [r[0] for r in g.timing_read()]
        finally:
            g.timing_enable(False)
        got = []
        for o in self.outs:
            h = np.zeros(o.ne[0], np.float32)
            be.get_tensor(h, o.data)
            got.append(h)
        be.synchronize()
        return got

    def free(self):
        for p in self.bufs:
            self.be.free_buffer(p)


def check(g, case, kernel, what):
    """Knob on and off, eager and replayed: one launch `kernel`, every output the oracle's bits
    (so the two forms give equal bytes)."""
    try:
        for knob in (1, 0):
            g.debug_knob("GEMV_SHORT", knob)
            for run, use_graph in (("eager", 0), ("replay 1", 1), ("replay 2", 1)):
                names = [] if run == "eager" else None
                got = case.run(g, use_graph, names)
                if names is not None:
                    assert names == [kernel], (what, knob, names)
                for h, ref in zip(got, case.refs):
                    assert bits_equal(h, ref), (what, "short" if knob else "generic", run, first_mismatch(h, ref))
    finally:
        g.debug_knob("GEMV_SHORT")  # back to the default
        case.free()


def tmask(mats):
    m = 0
    for ty, _ in mats:
        m |= 1 << (ty - Q4)
    return m if m in (1, 2, 4) else 7


def kernel_name(mats, pro):
    return f"kq::kq_rows<{tmask(mats)}, true, {pro}>"


SHAPES = [(256, 300), (2048, 8), (2048, 300), (2048, 2048), (4096, 300), (5632, 300)]


@gpu
@pytest.mark.parametrize("ty", [Q4, Q5, Q6], ids=["q4k", "q5k", "q6k"])
@pytest.mark.parametrize("K,N", SHAPES, ids=[f"k{k}n{n}" for k, n in SHAPES])
def test_short_one_matrix(dev, be, oracle, npo, O, ty, K, N):
    import ggml_mi355x as g
    rng = np.random.default_rng(100 * K + N + ty)
    steps, depth, form = g.rows_stream_plan([(ty, N)], K)
    assert form == g.ROWS_SHORT and steps <= depth, (steps, depth, form)
    mats = [(ty, npo.random_blocks(rng, ty, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats), kernel_name(mats, 0), (ty, K, N))


@pytest.fixture
def waves2(dev):
    """Two waves per workgroup, so that few rows fill every wave to the ring's depth: yields
    the launch's waves."""
    import torch
    import ggml_mi355x as g
    prev = g.gemv_waves(2)
    yield 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    g.gemv_waves(prev)


@gpu
@pytest.mark.parametrize("ty", [Q4, Q5, Q6], ids=["q4k", "q5k", "q6k"])
@pytest.mark.parametrize("over", [0, 1], ids=["D", "D+1"])
def test_ring_boundary(dev, be, oracle, npo, O, waves2, ty, over):
    """K = 4096, a row per step: D x waves rows give every wave exactly D steps (the short
    form, the whole ring issued before the barrier); one more row gives one wave D + 1 and the
    launch the generic loop. Both give the oracle's bits, with the knob on and off."""
    import ggml_mi355x as g
    K, D = 4096, DEPTH[ty]
    N = D * waves2 + over
    assert g.rows_stream_plan([(ty, N)], K) == (D + over, D, g.ROWS_LONG if over else g.ROWS_SHORT)
    rng = np.random.default_rng(7 * N + ty)
    mats = [(ty, npo.random_blocks(rng, ty, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats), kernel_name(mats, 0), (ty, N))


@gpu
def test_short_mixed_qkv_norm(dev, be, oracle, npo, O):
    """The q/k/v launch of TinyLlama's shape: Q4_K q (2048 rows) and k (256), Q6_K v (256), behind
    the norm prologue; then a row whose norm is redone in ggml's order (order_split_rows)."""
    import ggml_mi355x as g
    K = 2048
    shape = [(Q4, 2048), (Q4, 256), (Q6, 256)]
    assert g.rows_stream_plan(shape, K)[2] == g.ROWS_SHORT
    rng = np.random.default_rng(2560)
    mats = [(ty, npo.random_blocks(rng, ty, n, K)) for ty, n in shape]
    check(g, Case(g, be, oracle, O, rng, K, mats, norm=True), kernel_name(mats, 1), "q/k/v")
    r, eps = SPLIT_CASES[K][0]
    check(g, Case(g, be, oracle, O, rng, K, mats, norm=True, x=split_rows(K)[0][r], eps=eps), kernel_name(mats, 1),
          ("q/k/v order split", r, eps))


@gpu
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "none"])
def test_short_gate_up_swiglu(dev, be, oracle, npo, O, norm):
    """gate + up with the SWIGLU epilogue: 1537 rows each (no multiple of 4: the last row takes
    ggml's scalar tail; enough rows for gate and up to take half the launch's waves each, which
    pairs them in one workgroup), the up wave reading its gate partner's staged rows."""
    import ggml_mi355x as g
    K, N = 2048, 1537
    assert g.rows_stream_plan([(Q4, N), (Q4, N)], K)[2] == g.ROWS_SHORT
    rng = np.random.default_rng(1537 + norm)
    mats = [(Q4, npo.random_blocks(rng, Q4, N, K)), (Q4, npo.random_blocks(rng, Q4, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats, norm=norm, swiglu=True), kernel_name(mats, 1 if norm else 0),
          ("gate + up", norm))


@gpu
@pytest.mark.parametrize("ty,K,N", [(Q4, 2048, 2048), (Q6, 5632, 2048), (Q4, 5632, 300)],
                         ids=["o-proj", "down-q6k", "down-q4k"])
def test_short_residual_add(dev, be, oracle, npo, O, ty, K, N):
    """MUL_MAT -> ADD(residual): the add from the lane's register (o-proj, down)."""
    import ggml_mi355x as g
    assert g.rows_stream_plan([(ty, N)], K)[2] == g.ROWS_SHORT
    rng = np.random.default_rng(K + N + ty)
    mats = [(ty, npo.random_blocks(rng, ty, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats, residual=True), kernel_name(mats, 0), (ty, K, N))


@gpu
def test_short_norm_order_split_one_matrix(dev, be, oracle, npo, O):
    """One Q4_K matrix behind the norm prologue on a row whose fast and sequential means differ
    (the redo path), 40 rows: most waves stream nothing and issue the dummy step."""
    import ggml_mi355x as g
    K, N = 2048, 40
    assert g.rows_stream_plan([(Q4, N)], K)[2] == g.ROWS_SHORT
    rng = np.random.default_rng(40)
    mats = [(Q4, npo.random_blocks(rng, Q4, N, K))]
    r, eps = SPLIT_CASES[K][1]
    check(g, Case(g, be, oracle, O, rng, K, mats, norm=True, x=split_rows(K)[0][r], eps=eps), kernel_name(mats, 1),
          ("order split", r, eps))
