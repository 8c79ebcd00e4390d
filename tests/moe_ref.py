"""The mixture-of-experts FFN of llm_build_llama (build_moe_ffn [U], taken when llama.expert_count > 0:
Mixtral) restated in numpy on top of the CPU oracle — test infrastructure; the rule mi355x_moe_route,
mi355x_mul_mat_id and mi355x_moe_combine state in include/ggml_mi355x.h. Facts about upstream are
marked [U]. For one row `cur` (the ffn_norm output) of a layer:

  logits[e] = ggml_vec_dot_f32(gate_inp[e], cur) in its NEON order [U]: 4 accumulators of 4 lanes
      stepping 16 floats, acc[j] = vfmaq_f32(acc[j], x, y) (acc + x * y, fused); the reduction
      acc0 += acc2, acc1 += acc3, acc0 += acc1, then vaddvq: (l0 + l1) + (l2 + l3). n_embd % 16 == 0
      is required, so the scalar tail never runs.
  probs = soft_max(logits), no mask, scale 1 [U]: oracle.kq_ops_oracle.soft_max_row (ggml_v_expf for
      the first n & ~3 entries, libm's expf for the tail: with n_expert == 2 both entries are tail).
  ids = top_k(probs, n_used) [U]: ggml_top_k is a view of the first n_used entries of
      ggml_argsort(probs, DESC), and the argsort of the pinned build is the exchange sort
          for i: for j > i: if p[idx[i]] < p[idx[j]]: swap(idx[i], idx[j])
      (ggml_compute_forward_argsort_f32 [U]); that decides exact ties, and not as "smallest index
      first": position i receives the first strict maximum in the array's current order, and every
      swap moves a smaller value back into the tail.
  w = probs[ids]; w /= (float)(the sum of w accumulated in a double in slot order) [U]: norm_w = true for
      the llama arch, ggml_sum_rows (ggml_vec_sum_f32 in ggml_float) and ggml_div. No scale_w, no clamp.
  up = mul_mat_id(up_exps, cur, ids); gate = mul_mat_id(gate_exps, cur, ids); par = swiglu(gate, up);
  ex = mul_mat_id(down_exps, par, ids) [U]: ggml_compute_forward_mul_mat_id quantizes every src1 row
      to Q8_K and for token t, slot s computes dst[:, s, t] = W[ids[s, t]] . q8(src1[:, s % ne11, t]),
      each row by ggml_vec_dot_q*_K_q8_K: oracle.kq_oracle.mul_mat.
  ex[:, s] *= w[s]; out = ex[:, 0]; out = out + ex[:, s] for s = 1 .. (f32, slot order) [U].
  cur = out + ffn_inp, as in the dense arm.
NaN router logits are unspecified."""
import numpy as np

from oracle import kq_oracle as KO
from oracle import kq_oracle_np as N
from oracle import kq_ops_oracle as O

F32 = np.float32


def vec_dot_f32(x, y):
    """ggml_vec_dot_f32, NEON order; len % 16 == 0."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    assert x.size == y.size and x.size % 16 == 0
    acc = np.zeros(16, F32)  # acc[4 j + l]: accumulator j, lane l
    for s in range(x.size // 16):
        acc = N.fma_f32(x[16 * s:16 * s + 16], y[16 * s:16 * s + 16], acc)
    a = acc.reshape(4, 4)
    a0 = a[0] + a[2]
    a1 = a[1] + a[3]
    a0 = a0 + a1
    return F32(F32(a0[0] + a0[1]) + F32(a0[2] + a0[3]))


def router_logits(gate_inp, cur):
    """gate_inp f32 [n_expert, n_embd], cur [n_embd] -> f32 [n_expert]."""
    return np.array([vec_dot_f32(g, cur) for g in np.asarray(gate_inp, F32)], F32)


def argsort_desc(p):
    """ggml's descending argsort of the pinned build: the exchange sort, ties as it leaves them."""
    idx = list(range(len(p)))
    for i in range(len(p)):
        for j in range(i + 1, len(p)):
            if p[idx[i]] < p[idx[j]]:
                idx[i], idx[j] = idx[j], idx[i]
    return np.array(idx, np.int32)


def route_probs(probs, n_used):
    """(ids int32 [n_used], w f32 [n_used]) of a row of probabilities."""
    probs = np.asarray(probs, F32)
    ids = argsort_desc(probs)[:n_used]
    w = probs[ids]
    s = np.float64(0.0)
    for v in w:
        s += np.float64(v)
    return ids, (w / F32(s)).astype(F32)


def route(gate_inp, cur, n_used):
    """(ids, w, probs) of one row."""
    probs = O.soft_max_row(router_logits(gate_inp, cur))
    ids, w = route_probs(probs, n_used)
    return ids, w, probs


def mul_mat_id(type_, experts, x, ids):
    """experts uint8 [n_expert, N, row bytes]; x f32 [T, ne11, K]; ids int [T, n_used] -> f32 [T, n_used, N].
    An id outside [0, n_expert) gives a NaN row (the device's convention; upstream asserts)."""
    x, ids = np.asarray(x, F32), np.asarray(ids)
    T, ne11, _ = x.shape
    n_used = ids.shape[1]
    out = np.empty((T, n_used, experts.shape[1]), F32)
    for t in range(T):
        for s in range(n_used):
            e = int(ids[t, s])
            if not 0 <= e < experts.shape[0]:
                out[t, s] = np.nan
                continue
            out[t, s] = KO.mul_mat(type_, np.ascontiguousarray(experts[e]), x[t, s % ne11][None])[0]
    return out


def combine(ex, w):
    """ex f32 [n_used, n], w f32 [n_used] -> f32 [n]: products first, then the sums in slot order."""
    ex = [O.mul(np.asarray(e, F32), np.full(len(e), w[s], F32)) for s, e in enumerate(ex)]
    out = ex[0]
    for e in ex[1:]:
        out = O.add(out, e)
    return out


def moe_ffn(layer, cur, n_used):
    """One row through a layer's MoE FFN (before the residual). layer: "gate_inp" f32 [n_expert, n_embd],
    "up_exps" / "gate_exps" / "down_exps" (type, uint8 [n_expert, rows, row bytes]). Returns (out, ids, w)."""
    ids, w, _ = route(layer["gate_inp"], cur, n_used)
    x = np.asarray(cur, F32)[None, None]
    up = mul_mat_id(layer["up_exps"][0], layer["up_exps"][1], x, ids[None])[0]
    gate = mul_mat_id(layer["gate_exps"][0], layer["gate_exps"][1], x, ids[None])[0]
    par = np.stack([O.swiglu(gate[s], up[s]) for s in range(n_used)])
    ex = mul_mat_id(layer["down_exps"][0], layer["down_exps"][1], par[None], ids[None])[0]
    return combine(ex, w), ids, w


def decode_token_moe(model, token, pos, cache, trace=None):
    """oracle.kq_ops_oracle.decode_token with the MoE FFN: `model` as tests/moe_model.oracle_model builds it
    (each layer: the attention's entries and gate_inp / up_exps / gate_exps / down_exps). Returns the logits;
    `trace` (a list) receives per layer a dict(ids, w, x)."""
    hp = model["hp"]
    E, hd, eps = hp["n_embd"], hp["head_dim"], hp["eps"]
    t, w = model["tok_embd"]
    x = O.get_rows(t, w, E, [token])[0]
    scale = F32(1.0) / np.sqrt(F32(hd))
    for li, L in enumerate(model["layers"]):
        cur = O.mul(O.rms_norm(x, eps), L["attn_norm"])
        q = KO.mul_mat(L["wq"][0], L["wq"][1], cur)[0]
        k = KO.mul_mat(L["wk"][0], L["wk"][1], cur)[0]
        v = KO.mul_mat(L["wv"][0], L["wv"][1], cur)[0]
        q = O.rope(q, hd, hd, pos, model["rope_table"])
        k = O.rope(k, hd, hd, pos, model["rope_table"])
        kc, vc = cache[li]
        att = O.attn_decode(q, k, v, kc, vc, pos, hp["n_head"], hp["n_head_kv"], hd, float(scale))
        ffn_inp = O.add(KO.mul_mat(L["wo"][0], L["wo"][1], att)[0], x)
        cur = O.mul(O.rms_norm(ffn_inp, eps), L["ffn_norm"])
        out, ids, wts = moe_ffn(L, cur, hp["n_expert_used"])
        x = O.add(out, ffn_inp)
        if trace is not None:
            trace.append(dict(ids=ids, w=wts, x=x))
    cur = O.mul(O.rms_norm(x, eps), model["output_norm"])
    return KO.mul_mat(model["output"][0], model["output"][1], cur)[0]
