"""GPU: the launch sequence the backend plans for a graph (csrc/kq_plan.hip plan_launches, run
by csrc/kq_backend.hip enqueue) stays what tests/golden/launch_plans.json records: for every
case below the list of (kernel name, algorithmic bytes) of one eager run under timing_enable,
after one warming run. The golden file was recorded with this module's recorder
(`python -m tests.test_gpu_plan [path]`) before the planner was split out of kq_backend.hip;
a planner change that moves a launch regenerates it on purpose, never as a side effect.

The cases use the smallest llama that has every launch kind: two TinyLlama-width layers,
n_ctx 64. Also here: the activation image in the backend workspace is re-made when an exact
GEMM replaced it between two f16 GEMMs on the same activation (Q8State::set)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
HP = (2048, 2, 32, 4, 5632, 4096)
N_CTX = 64


def _timed(run):
    import ggml_mi355x as g
    g.timing_enable(True)
    try:
        run()
        return [[r[0], int(r[1])] for r in g.timing_read()]
    finally:
        g.timing_enable(False)


def _llama(dev, mix="q4_k_m", fuse=True):
    from ggml_mi355x.llama import hparams
    from tests.test_gpu_ops import _decoder
    _, b, dec = _decoder(dev, hparams(*HP), 3, N_CTX, fuse, mix=mix)
    return b, dec


def _decode(dev, fuse=True, setup=None):
    b, dec = _llama(dev, fuse=fuse)
    if setup:
        setup(b)
    dec.step(5, 0)
    b.synchronize()
    rows = _timed(lambda: dec.step(6, 1, use_graph=False))
    assert b.layer_error() == 0
    b.close()
    return rows


def _attn_oproj(b):
    assert b.set_attn_oproj(True) == 0


def _layer_engine(b):
    assert b.set_layer_engine(True) == 0


def _prompt(dev, precision):
    import ggml_mi355x as g
    prev = g.prefill_precision(getattr(g, precision))
    try:
        b, dec = _llama(dev, mix="q5_k_m")
        tokens = np.random.default_rng(12).integers(0, HP[5], size=32).tolist()
        dec.prompt(tokens, 0)
        b.synchronize()
        rows = _timed(lambda: dec.prompt(tokens, 0, use_graph=False))
        b.close()
        return rows
    finally:
        g.prefill_precision(prev)


def _step_batch(dev):
    b, dec = _llama(dev)
    n_kv = 32
    mask = np.full((3, n_kv), -np.inf, np.float32)
    for s in range(3):
        mask[s, s] = 0.0
    args = ([1, 2, 3], [0, 0, 0], [0, 1, 2], mask, n_kv)
    dec.step_batch(*args)
    b.synchronize()
    rows = _timed(lambda: dec.step_batch(*args, use_graph=False))
    b.close()
    return rows


def _reused_buffer_graph(view_offset):
    """The graph of test_gpu_ops.test_fusion_respects_reused_buffers_and_views: MUL, ADD, a
    GEMV into the first node's buffer, its ADD, and an ADD that reads the GEMV through a view."""
    import ggml_mi355x as g
    from oracle import kq_oracle_np as npo
    K, N = 1024, 512
    rng = np.random.default_rng(view_offset)
    be = g.Backend()
    w = npo.random_blocks(rng, 12, N, K)

    def buf(a=None, n=None):
        p = be.alloc((a.size if a is not None else n) * (a.itemsize if a is not None else 4))
        if a is not None:
            be.set_tensor(p, a)
        return p

    wt = g.make_tensor(12, K, N, buf(w))
    P = buf(n=max(K, N))
    xt = g.make_tensor(g.TYPE_F32, K, 1, buf(rng.standard_normal(K).astype(np.float32)))
    w0t = g.make_tensor(g.TYPE_F32, K, 1, buf(rng.uniform(0.5, 1.5, K).astype(np.float32)))
    n0 = g.make_tensor(g.TYPE_F32, K, 1, P, op=g.OP_MUL, src0=xt, src1=w0t)
    n1 = g.make_tensor(g.TYPE_F32, K, 1, buf(n=K), op=g.OP_ADD, src0=n0, src1=xt)
    n2 = g.make_tensor(g.TYPE_F32, N, 1, P, op=g.OP_MUL_MAT, src0=wt, src1=n1)
    rt = g.make_tensor(g.TYPE_F32, N, 1, buf(rng.standard_normal(N).astype(np.float32)))
    n3 = g.make_tensor(g.TYPE_F32, N, 1, buf(n=N), op=g.OP_ADD, src0=n2, src1=rt)
    nv = N - view_offset
    view = g.make_tensor(g.TYPE_F32, nv, 1, P + 4 * view_offset)
    r2t = g.make_tensor(g.TYPE_F32, nv, 1, buf(rng.standard_normal(nv).astype(np.float32)))
    n4 = g.make_tensor(g.TYPE_F32, nv, 1, buf(n=nv), op=g.OP_ADD, src0=view, src1=r2t)
    nodes = [n0, n1, n2, n3, n4]
    keep = [xt, w0t, wt, rt, view, r2t]
    assert be.graph_compute(nodes, use_graph=1) == 0
    be.synchronize()

    def run():
        assert be.graph_compute(nodes, use_graph=0) == 0
    rows = _timed(run)
    be.close()
    del keep
    return rows


CASES = {
    "decode_fused": lambda dev: _decode(dev),
    "decode_unfused": lambda dev: _decode(dev, fuse=False),
    "decode_attn_oproj": lambda dev: _decode(dev, setup=_attn_oproj),
    "decode_layer_engine": lambda dev: _decode(dev, setup=_layer_engine),
    "prompt32_q5km_exact": lambda dev: _prompt(dev, "PREFILL_EXACT"),
    "prompt32_q5km_f16": lambda dev: _prompt(dev, "PREFILL_F16"),
    "step_batch_3seq": _step_batch,
    "reused_buffer_view0": lambda dev: _reused_buffer_graph(0),
    "reused_buffer_view64": lambda dev: _reused_buffer_graph(64),
}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_plan_unchanged(dev, golden, case):
    got = CASES[case](dev)
    want = golden[case]
    assert len(want) > 0
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:4] + [len(got), len(want)]


def test_exact_gemm_between_two_f16_gemms_on_one_activation(dev, npo):
    """PREFILL_F16, one activation x (K 256, M 16), three MUL_MAT -> ADD pairs (N 64): a Q6_K
    weight A (kq_mmf, images x into the workspace), a small Q4_K weight (the exact kq_mmq:
    Q8L blocks of x replace the image), then A again with the first pair's residual. The third
    pair must image x again: its output equals the first pair's bit for bit (kq_mmf repeats
    its bits run to run: test_gpu_mmf.test_llama_prompt_f16). Before Q8State::set assigned
    every field the state still said "f16 image of x" after the exact GEMM, and the third GEMM
    read Q8L bytes as f16."""
    import ggml_mi355x as g
    K, M, N = 256, 16, 64
    rng = np.random.default_rng(41)
    prev = g.prefill_precision(g.PREFILL_F16)
    be = g.Backend()
    try:
        def dev_buf(a):
            p = be.alloc(a.nbytes)
            be.set_tensor(p, a)
            return p

        x = rng.standard_normal((M, K)).astype(np.float32)
        xt = g.make_tensor(g.TYPE_F32, K, M, dev_buf(x))
        wa = g.make_tensor(14, K, N, dev_buf(npo.random_blocks(rng, 14, N, K)))
        wb = g.make_tensor(12, K, N, dev_buf(npo.random_blocks(rng, 12, N, K)))
        res = g.make_tensor(g.TYPE_F32, N, M, dev_buf(rng.standard_normal((M, N)).astype(np.float32)))
        res_b = g.make_tensor(g.TYPE_F32, N, M, dev_buf(rng.standard_normal((M, N)).astype(np.float32)))
        nodes, outs = [], []
        for w, r in ((wa, res), (wb, res_b), (wa, res)):
            mm = g.make_tensor(g.TYPE_F32, N, M, be.alloc(M * N * 4), op=g.OP_MUL_MAT, src0=w, src1=xt)
            ad = g.make_tensor(g.TYPE_F32, N, M, be.alloc(M * N * 4), op=g.OP_ADD, src0=mm, src1=r)
            nodes += [mm, ad]
            outs.append(ad)

        def run():
            assert be.graph_compute(nodes, use_graph=0) == 0
        names = [r[0] for r in _timed(run)]
        gemms = [n for n in names if "kq_mmf" in n or "kq_mmq" in n]
        assert len(gemms) == 3 and "kq_mmf" in gemms[0] and "kq_mmq" in gemms[1] and "kq_mmf" in gemms[2], names
        assert not any("kq_add" in n for n in names), names  # the ADDs ran as the GEMMs' epilogues
        be.synchronize()
        got = []
        for ad in outs:
            h = np.zeros((M, N), np.float32)
            be.get_tensor(h, ad.data)
            be.synchronize()
            got.append(h)
        assert np.isfinite(got[0]).all()
        bad = int((got[2].view(np.uint32) != got[0].view(np.uint32)).sum())
        print("third output: words differing from the first:", bad, "of", M * N)
        assert bad == 0, bad
    finally:
        be.close()
        g.prefill_precision(prev)


if __name__ == "__main__":  # record the golden file (run from the repository root: python -m tests.test_gpu_plan)
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "ggml-neon-opt_amd"))
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    device = torch.device("cuda:0")
    plans = {name: CASES[name](device) for name in sorted(CASES)}
    with open(out, "w") as f:
        json.dump(plans, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", {k: len(v) for k, v in plans.items()}, "->", out)
