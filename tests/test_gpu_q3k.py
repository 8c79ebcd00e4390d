"""Q3_K on the device against tests/q3k_ref.py, by bits: kq_gemv_q3k through mul_mat and mul_mat_q8
(1 to 33 columns), vec_dot, get_rows, the backend graph and a LlamaDecoder with a Q3_K_M-like mix.
The rule was restated from ggml, not compared with ggml's own output; no real Q3_K file is read."""
import functools

import numpy as np
import pytest

from tests import q3k_ref as R
from tests.test_gpu_parity import bits_equal, first_mismatch, t
from tests.test_gpu_rows_cols import _timed

pytestmark = pytest.mark.gpu
Q3, Q4 = 11, 12


@functools.lru_cache(maxsize=None)
def _case(K, N, M):  # (weights, x, the oracle's Q8_K rows of x, reference (M, N)); a smaller M is a prefix
    from oracle import kq_oracle as KO
    rng = np.random.default_rng(K * 1000 + N)
    w = R.weights(rng, N, K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[0, :256] = 1.0  # saturated Q8_K against the forced W = +128 block: the largest |isum|
    x[M // 2, K - 256:] = 0.0  # a superblock with d = 0
    q8 = KO.quantize_q8_K(x)
    return w, x, q8, R.mul_mat_q8(w, K, q8)


def _at(dev, w, offset):
    import torch
    buf = torch.zeros(w.size + 16, dtype=torch.uint8, device=dev)
    buf[offset:offset + w.size].copy_(t(w.reshape(-1), dev))
    return buf[offset:offset + w.size].view(w.shape)


def _check(dev, K, N, M, offset, Mref):
    import ggml_mi355x as g
    w, x, q8, ref = _case(K, N, Mref)
    wd = _at(dev, w, offset)
    got, names = _timed(lambda: g.mul_mat(Q3, wd, K, t(x[:M], dev)).cpu().numpy())
    assert bits_equal(got, ref[:M]), first_mismatch(got, ref[:M])
    want = ["kq::kq_gemv_q3k<1, true>"] if M == 1 else ["kq::kq_quantize_q8K", names[-1]]
    assert names == want and "kq_gemv_q3k" in names[-1], names
    got = g.mul_mat_q8(Q3, wd, K, t(q8[:M], dev)).cpu().numpy()
    assert bits_equal(got, ref[:M]), first_mismatch(got, ref[:M])


@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("M", [1, 2, 8, 15])
@pytest.mark.parametrize("N", [1, 9, 67])
@pytest.mark.parametrize("K", [256, 768, 8448])
def test_gemv(dev, K, N, M, offset):
    """K: one block; an odd count (rows at 2-byte alignment); past one 8-block step, the last one partial."""
    _check(dev, K, N, M, offset, 15)


@pytest.mark.parametrize("K,N,M", [(K, N, M) for K in (256, 768) for N in (33, 130) for M in (16, 33)] + [(256, 0, 8)])
def test_batched_and_many_rows(dev, K, N, M):
    """16 and more columns: the GEMV over groups of 8 (33: four groups and a group of one). N = 0: so
    many rows that a wave flushes its staged results and goes on (q3k_plan: rows_per_wave > flush_rows)."""
    import ggml_mi355x as g
    N = N or g.q3k_plan(K, 1 << 22, M)["waves"] * (g.q3k_plan(K, 1, M)["flush_rows"] + 1) + 5
    _check(dev, K, N, M, 2 if M == 8 else 0, M if M == 8 else 33)


def test_vec_dot_and_get_rows(dev):
    import ggml_mi355x as g
    w, x, q8, ref = _case(768, 9, 15)
    s, row, col = np.zeros(1, np.float32), np.ascontiguousarray(w[4]), np.ascontiguousarray(q8[3])
    g.vec_dot_q3_K_q8_K(768, s.ctypes.data, 0, row.ctypes.data, 0, col.ctypes.data, 0, 1)
    assert bits_equal(s, ref[3, 4:5])
    ids = np.array([0, 8, 3, 3], np.int32)  # first, last, repeated
    got = g.get_rows(Q3, _at(dev, w, 2), 768, t(ids, dev)).cpu().numpy()
    assert bits_equal(got, R.dequantize(w, 768)[ids]), first_mismatch(got, R.dequantize(w, 768)[ids])


@pytest.mark.parametrize("type_", [Q3, Q4])
def test_backend_graph(dev, oracle, type_):
    """GET_ROWS -> RMS_NORM -> MUL -> MUL_MAT. Q3_K in both places: single nodes. Q4_K: the plan of before."""
    import torch
    import ggml_mi355x as g
    from oracle import kq_ops_oracle as O
    from tests.llama_model import kquant
    K, N, V, eps = 768, 67, 9, 1e-5
    rng = np.random.default_rng(type_)
    make = (lambda n: R.weights(rng, n, K)) if type_ == Q3 else (lambda n: kquant(rng, type_, n, K, edges=True))
    table, w, nw = make(V), make(N), rng.uniform(0.8, 1.2, K).astype(np.float32)
    dv = [t(a, dev) for a in (table, w, nw, np.array([V - 1], np.int32))]
    out = [torch.zeros(n, dtype=torch.float32, device=dev) for n in (K, K, K, N)]
    tab, wt, nwt, ids = (g.make_tensor(ty, ne0, ne1, d.data_ptr()) for ty, ne0, ne1, d in
                         ((type_, K, V, dv[0]), (type_, K, N, dv[1]), (g.TYPE_F32, K, 1, dv[2]), (g.TYPE_I32, 1, 1, dv[3])))
    n0 = g.make_tensor(g.TYPE_F32, K, 1, out[0].data_ptr(), op=g.OP_GET_ROWS, src0=tab, src1=ids)
    n1 = g.make_tensor(g.TYPE_F32, K, 1, out[1].data_ptr(), op=g.OP_RMS_NORM, src0=n0, op_params=[g.f32_bits(eps)])
    n2 = g.make_tensor(g.TYPE_F32, K, 1, out[2].data_ptr(), op=g.OP_MUL, src0=n1, src1=nwt)
    n3 = g.make_tensor(g.TYPE_F32, N, 1, out[3].data_ptr(), op=g.OP_MUL_MAT, src0=wt, src1=n2, flags=g.FLAG_OUTPUT)
    torch.cuda.synchronize()
    be = g.Backend()
    _, names = _timed(lambda: (be.graph_compute([n0, n1, n2, n3], use_graph=0), be.synchronize()))
    got = out[3].cpu().numpy()
    be.close()
    row = R.dequantize(table[V - 1:], K)[0] if type_ == Q3 else O.get_rows(type_, table, K, [V - 1])[0]
    cur = O.mul(O.rms_norm(row, eps), nw)
    ref = R.mul_mat(w, K, cur)[0] if type_ == Q3 else oracle.mul_mat(type_, w, cur)[0]
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert names == ["kq::kq_get_rows"] + (["kq::kq_rows<1, true, 1>"] if type_ == Q4 else [names[1], "kq::kq_gemv_q3k<1, true>"])


def test_llama_decoder_q3_k_m_mix(dev):
    """Two layers, E = 256, FF = 512, V = 512 in a Q3_K_M-like mix. step at positions 0..2, then a 17-token
    prompt (GEMVs of 17 columns: two groups of 8 and one of one) against the composed reference."""
    import ggml_mi355x as g
    from ggml_mi355x.llama import LlamaDecoder, hparams
    from tests import llama_model as LM
    hp, n_ctx = hparams(256, 2, 4, 2, 512, 512), 32
    w, rng = LM.build(hp, 7), np.random.default_rng(11)
    mix = {"token_embd": Q3, "output": 14, "attn_q": Q3, "attn_k": Q3, "ffn_gate": Q3, "ffn_up": Q3, "attn_v": 13,
           "attn_output": Q4, "ffn_down": Q4}
    for name, (_, old) in [(k, v) for k, v in w.items() if isinstance(v, tuple)]:
        ty, K = mix[name.split(".")[-1]], hp["n_ff"] if name.endswith("ffn_down") else hp["n_embd"]
        w[name] = (ty, R.weights(rng, old.shape[0], K) if ty == Q3 else LM.kquant(rng, ty, old.shape[0], K, edges=True))
    b = g.Backend()
    dec = LlamaDecoder(b, hp, LM.to_device(w, dev), n_ctx)
    logits_of = lambda out: (b.synchronize(), out.cpu().numpy().reshape(-1))[1]  # noqa: E731
    model, cache = LM.oracle_model(hp, w, n_ctx)
    for pos, tok in enumerate([5, 300, 511]):
        ref = R.decode_token(model, tok, pos, cache)
        got = logits_of(dec.step(tok, pos))
        assert bits_equal(got, ref), (pos, first_mismatch(got, ref))
    tokens = np.random.default_rng(2).integers(0, 512, size=17).tolist()
    got, names = _timed(lambda: logits_of(dec.prompt(tokens, 3, use_graph=False)))
    for i, tok in enumerate(tokens):
        ref = R.decode_token(model, tok, 3 + i, cache)
    assert bits_equal(got, ref), first_mismatch(got, ref)
    assert "kq::kq_gemv_q3k<8, false>" in names, names
    b.close()
