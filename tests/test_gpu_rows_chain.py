"""The fp32 chain of the decode GEMV (rows_chain, kq_rows_device.h) at its three sites: the
short-stream form's one batch, the generic loop's replay per batch, and kq_rows_dyn's replay.

The quad leaders store what the chain consumes as floats (RowRec: the conversions, and for Q5_K
the whole per-superblock term, are computed by the leader) and lane r replays row r's records
in superblock order, four records read at a time. None of that may change a bit: every output
is compared on bits with the oracle (ggml's vec_dot row by row, rms_norm / MUL / ADD / swiglu as
ggml computes them), with the knob GEMV_SHORT on and off (so the short and the generic form give
equal bytes), through graph_compute eager and replayed.

Inputs are npo.random_blocks' default (d and dmin spread over [2^-14, 2^-6]) and at least 300
rows per case: on such records swapping two adjacent superblocks of the Q4_K chain changes the
bits of 11-50 % of the rows, so a reordered or mis-grouped chain cannot pass by chance.

nb sweep: K = 256 nb around the loop's group of G = 4 (G - 1, G, G + 1, 2 G + 1), around 8, 16
and 32, one to three records, TinyLlama's 22, and nb = 33, which lies past the
fused-quantization limit (the Q8L-row kernel, the generic loop). 300 rows, so waves with and
without rows occur; each in Q4_K, Q5_K and Q6_K (Q6_K tensors start at row 1 of their buffer
where that is off a 16-byte boundary), on kq_rows and on kq_rows_dyn.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import bits_equal, first_mismatch
from tests.test_gpu_rows_short import Case

gpu = pytest.mark.gpu

Q4, Q5, Q6 = 12, 13, 14
G = 4  # records read at a time (rows_chain's unrolled loop)
NBS = sorted({1, 2, 3, 7, 8, 9, 15, 16, 17, 22, 31, 32, 33} | {G - 1, G, G + 1, 2 * G + 1})
FUSED_NB = 32  # K <= 8192: quantization fused into the launch
ROWS, DYN = 0, 3  # gemv_impl: by launch (kq_rows where it fits) / kq_rows_dyn for every one-type launch


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


@pytest.fixture(params=[ROWS, DYN], ids=["rows", "dyn"])
def kimpl(request, dev):
    import ggml_mi355x as g
    prev = g.gemv_impl(request.param)
    yield request.param
    g.gemv_impl(prev)


def check(g, case, what, kernel=None):
    """Knob GEMV_SHORT on and off, eager and replayed twice: every output the oracle's bits, sign
    bits and NaN payloads included (so both forms give equal bytes). `kernel`: the name every
    GEMV launch of the eager run starts with."""
    try:
        for knob in (1, 0):
            g.debug_knob("GEMV_SHORT", knob)
            for run, use_graph in (("eager", 0), ("replay 1", 1), ("replay 2", 1)):
                names = [] if run == "eager" else None
                got = case.run(g, use_graph, names)
                if names is not None and kernel is not None:
                    rows = [n for n in names if "kq_rows" in n]
                    assert rows and all(n.startswith(kernel) for n in rows), (what, knob, names)
                for h, ref in zip(got, case.refs):
                    assert bits_equal(h, ref), (what, "short" if knob else "generic", run, first_mismatch(h, ref))
    finally:
        g.debug_knob("GEMV_SHORT")  # back to the default
        case.free()


def kernel_of(kimpl):
    return "kq::kq_rows_dyn<" if kimpl == DYN else "kq::kq_rows<"


@gpu
@pytest.mark.parametrize("ty", [Q4, Q5, Q6], ids=["q4k", "q5k", "q6k"])
@pytest.mark.parametrize("nb", NBS, ids=[f"nb{n}" for n in NBS])
def test_chain_nb_sweep(dev, be, oracle, npo, O, kimpl, ty, nb):
    import ggml_mi355x as g
    K, N = 256 * nb, 300
    pl = g.rows_plan([(ty, N)], K, fusedq=nb <= FUSED_NB)
    assert pl["dyn"] == (kimpl == DYN), pl
    if nb > FUSED_NB:
        assert pl["sh"] == 0, pl  # the Q8L-row kernels exist in the generic form only
    rng = np.random.default_rng(1000 * nb + ty)
    mats = [(ty, npo.random_blocks(rng, ty, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats), (ty, nb, kimpl), kernel_of(kimpl))


BATCHES = [(Q6, 32000, 2048), (Q4, 11264, 2048)]


@gpu
@pytest.mark.parametrize("ty,N,K", BATCHES, ids=["head-q6k", "q4k-11264"])
def test_chain_batches(dev, be, oracle, npo, O, kimpl, ty, N, K):
    """Launches whose waves hold several chain batches, the last one partial: the head (Q6_K
    32000 x 2048: 11 rows per wave in batches of 8) and Q4_K 11264 x 2048, on kq_rows (short where
    the plan says so, and the generic loop with the knob off) and on kq_rows_dyn (units of two
    rows gathered into batches of 8)."""
    import ggml_mi355x as g
    pl = g.rows_plan([(ty, N)], K)
    assert pl["dyn"] == (kimpl == DYN), pl
    if ty == Q6 and kimpl == ROWS:
        assert pl["rpw"] > pl["bR"] and pl["rpw"] % pl["bR"], pl
    if kimpl == DYN:
        assert pl["rpw"] > pl["bR"] and pl["rpw"] % pl["bR"], pl
    rng = np.random.default_rng(N + K + ty)
    mats = [(ty, npo.random_blocks(rng, ty, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats), (ty, N, K, kimpl), kernel_of(kimpl))


@gpu
def test_chain_mixed_qkv_norm(dev, be, oracle, npo, O):
    """The mixed q/k/v launch (Q4_K, Q4_K, Q6_K) behind the norm prologue: the chain per type in
    one kernel."""
    import ggml_mi355x as g
    K = 2048
    rng = np.random.default_rng(81)
    mats = [(ty, npo.random_blocks(rng, ty, n, K)) for ty, n in [(Q4, 2048), (Q4, 256), (Q6, 256)]]
    check(g, Case(g, be, oracle, O, rng, K, mats, norm=True), "q/k/v", "kq::kq_rows<7, true, 1>")


@gpu
def test_chain_gate_up_swiglu(dev, be, oracle, npo, O):
    """gate + up with the SWIGLU epilogue over 1537 rows each (no multiple of 4): the up wave's
    chain result in its lane against its gate partner's staged rows."""
    import ggml_mi355x as g
    K, N = 2048, 1537
    rng = np.random.default_rng(82)
    mats = [(Q4, npo.random_blocks(rng, Q4, N, K)), (Q4, npo.random_blocks(rng, Q4, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats, swiglu=True), "gate + up", "kq::kq_rows<1, true, 0>")


@gpu
@pytest.mark.parametrize("nb", [8, 22], ids=["nb8", "nb22"])
def test_chain_residual_add(dev, be, oracle, npo, O, kimpl, nb):
    """MUL_MAT -> ADD(residual) at nb = 8 (o-proj) and nb = 22 (down: five groups and two): the
    residual's register is in flight across the chain."""
    import ggml_mi355x as g
    K, N = 256 * nb, 2048
    rng = np.random.default_rng(83 + nb)
    mats = [(Q4, npo.random_blocks(rng, Q4, N, K))]
    check(g, Case(g, be, oracle, O, rng, K, mats, residual=True), ("residual", nb, kimpl), kernel_of(kimpl))


def special_x(kind, K, rng):
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    if kind == "zero":
        x[:] = 0.0
    elif kind == "nan":
        x[K // 2 + 5] = np.nan
    elif kind == "inf":
        x[K // 3 + 1] = np.inf
    return x


@gpu
@pytest.mark.parametrize("kind", ["zero", "zero-rows", "nan", "inf"])
@pytest.mark.parametrize("ty", [Q4, Q5, Q6], ids=["q4k", "q5k", "q6k"])
def test_chain_zeros_and_nonfinite(dev, be, oracle, npo, O, kimpl, ty, kind):
    """An all-zero activation, rows whose blocks are all zero bytes (scales, quants, d and dmin),
    an activation with one NaN and one with one Inf, at nb = 9 (two groups and one) and nb = 22:
    bits_equal compares the sign of every zero and every NaN too."""
    import ggml_mi355x as g
    for nb in (9, 22):
        K, N = 256 * nb, 300
        rng = np.random.default_rng(17 * nb + ty)
        wq = npo.random_blocks(rng, ty, N, K)
        if kind == "zero-rows":
            wq[::3] = 0               # whole rows of zero blocks
            wq[1, : wq.shape[1] // 2] = 0  # and a row whose first half is
        x = special_x(kind, K, rng)
        check(g, Case(g, be, oracle, O, rng, K, [(ty, wq)], x=x), (kind, ty, nb, kimpl), kernel_of(kimpl))
