"""The Q3_K rule in numpy, restated from ggml's ARM NEON kernel and dequantize_row_q3_K (not compared
with ggml's own output). block_q3_K: hmask[32] @0, qs[64] @32, scales[12] @96, d (f16) @108.
e = 128n + 32j + l: q = ((qs[32n + l] >> 2j) & 3) - (0 if (hmask[l] >> (4n + j)) & 1 else 4); group
is = e / 16: sc = (lo4 | hi2 << 4) - 32, lo4 = scales[is] & 15 (is < 8) or scales[is - 8] >> 4, hi2 =
(scales[8 + (is & 3)] >> 2 (is >> 2)) & 3. vec_dot, per superblock in order from sumf = 0: isum = sum
sc * sum_16 q * y8, d_i = y.d * f32(x.d), sumf = fmaf(d_i, (float)isum, sumf). dequantize: (d * sc) * q."""
import numpy as np

from oracle import kq_oracle as KO, kq_oracle_np as NP, kq_ops_oracle as O

Q3_K, BLOCK, F32 = 11, 110, np.float32


def weights_int(w, K):
    b = np.ascontiguousarray(w, np.uint8).reshape(w.shape[0], K // 256, BLOCK)
    i = b.astype(np.int32)
    hm, qs, s = i[..., 0:32], i[..., 32:96], i[..., 96:108]
    e = np.arange(256)
    n, j, l = e // 128, (e // 32) & 3, e % 32
    q = ((qs[..., 32 * n + l] >> (2 * j)) & 3) - np.where((hm[..., l] >> (4 * n + j)) & 1, 0, 4)
    g = np.arange(16)
    lo4 = np.where(g < 8, s[..., g & 7] & 15, s[..., g & 7] >> 4)
    sc = (lo4 | (((s[..., 8 + (g & 3)] >> (2 * (g >> 2))) & 3) << 4)) - 32
    d = b[..., 108:110].copy().view(np.float16)[..., 0].astype(F32)
    return q, sc, d


def mul_mat_q8(w, K, q8):
    q, sc, d = weights_int(w, K)
    nb = K // 256
    y = NP.q8_K_from_bytes(q8, nb)
    wq = (q.reshape(q.shape[:2] + (16, 16)) * sc[..., None]).reshape(q.shape).astype(np.int64)  # sc * q
    out = np.zeros((y["d"].shape[0], w.shape[0]), F32)
    for i in range(nb):
        isum = y["qs"][:, i].astype(np.int64) @ wq[:, i].T  # (M, N), exact
        di = (y["d"][:, i, None] * d[None, :, i]).astype(F32)
        out = NP.fma_f32(di, isum.astype(F32), out)
    return out


def mul_mat(w, K, x):
    return mul_mat_q8(w, K, KO.quantize_q8_K(np.atleast_2d(x)))


def dequantize(w, K):
    q, sc, d = weights_int(w, K)
    dl = (d[..., None] * sc.astype(F32)).astype(F32)
    return (np.repeat(dl, 16, axis=-1) * q.astype(F32)).astype(F32).reshape(w.shape[0], K)


def weights(rng, N, K):
    """Random bytes, d with llama_model._edge_scales' edges; block 0 of row 0 all zero but d (sc = -32,
    q = -4: W = +128 everywhere), the last block of the last row all 0xFF but d."""
    from tests.llama_model import _edge_scales
    nb = K // 256
    raw = rng.integers(0, 256, size=(N, nb, BLOCK), dtype=np.uint8)
    d = _edge_scales(rng, rng.uniform(0.75, 1.25, size=(N, nb)) / np.sqrt(K * 1400.0))  # E[(sc q)^2] ~ 1400
    raw[0, 0, :108], raw[-1, -1, :108] = 0, 0xFF
    raw[..., 108:110] = d.astype(np.float16).view(np.uint8).reshape(N, nb, 2)
    return raw.reshape(N, nb * BLOCK)


def _mm(tw, x):
    return (mul_mat(tw[1], x.size, x) if tw[0] == Q3_K else KO.mul_mat(tw[0], tw[1], np.atleast_2d(x)))[0]


def decode_token(model, token, pos, cache):
    """kq_ops_oracle.decode_token from its per-op wrappers; Q3_K matmuls / get_rows from this file"""
    hp = model["hp"]
    E, hd, eps = hp["n_embd"], hp["head_dim"], hp["eps"]
    t, w = model["tok_embd"]
    x = dequantize(w[token:token + 1], E)[0] if t == Q3_K else O.get_rows(t, w, E, [token])[0]
    scale = float(F32(1.0) / np.sqrt(F32(hd)))
    for L, (kc, vc) in zip(model["layers"], cache):
        cur = O.mul(O.rms_norm(x, eps), L["attn_norm"])
        q = O.rope(_mm(L["wq"], cur), hd, hd, pos, model["rope_table"])
        k = O.rope(_mm(L["wk"], cur), hd, hd, pos, model["rope_table"])
        att = O.attn_decode(q, k, _mm(L["wv"], cur), kc, vc, pos, hp["n_head"], hp["n_head_kv"], hd, scale)
        ffn_inp = O.add(_mm(L["wo"], att), x)
        cur = O.mul(O.rms_norm(ffn_inp, eps), L["ffn_norm"])
        x = O.add(_mm(L["w_down"], O.swiglu(_mm(L["w_gate"], cur), _mm(L["w_up"], cur))), ffn_inp)
    return _mm(model["output"], O.mul(O.rms_norm(x, eps), model["output_norm"]))
