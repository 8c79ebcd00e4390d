"""The reference of the prompt-attention tests (tests/test_gpu_attn_prompt.py on the GPU, the CPU checks
of its meaning in tests/test_ops_oracle.py), composed of the oracle's pieces only
(oracle/kq_ops_oracle.py): both caches start with random finite f16 bits in every cell; every token with
a position inside [0, n_ctx) writes fp32_to_fp16(rope(k_i)) and fp32_to_fp16(v_i) into its cell; then,
per token in batch order, row i is attn_decode(rope(q_i), rope(k_i), v_i, caches, pos_i). A token outside
the cache writes nothing and gets a NaN row. Positions inside one batch are distinct (duplicates would
race on the cell). No GPU, no torch."""
import numpy as np

SHUFFLED = (5, 3, 4, 40, 31, 32, 33, 63, 0)
STRIDE_BATCH = (tuple(range(250, 290)),)  # of 320 cells: n_kv 256, 288 and 320 = n_ctx
MIXED = "mixed"  # q scaled by 40 on the even query heads and by 0.05 on the odd ones


def scale_of(hd):
    return float(np.float32(1.0) / np.sqrt(np.float32(hd)))


def rand_caches(rng, n_ctx, kvw):
    kc = rng.standard_normal((n_ctx, kvw), dtype=np.float32).astype(np.float16).view(np.uint16)
    vc = rng.standard_normal((kvw, n_ctx), dtype=np.float32).astype(np.float16).view(np.uint16)
    return kc, vc


def ref_attn_prompt(O, q, k, v, pos, kc, vc, tref, nh, nkv, hd):
    """The reference (module docstring); kc [n_ctx, kvw] / vc [kvw, n_ctx] uint16, updated in place."""
    T, n_ctx = len(pos), kc.shape[0]
    ok = [0 <= int(p) < n_ctx for p in pos]
    kr = [O.rope(k[i], hd, hd, int(pos[i]), tref) if ok[i] else None for i in range(T)]
    for i in range(T):
        if ok[i]:
            kc[int(pos[i])] = O.fp32_to_fp16(kr[i])
            vc[:, int(pos[i])] = O.fp32_to_fp16(v[i])
    out = np.full((T, nh * hd), np.nan, np.float32)
    for i in range(T):
        if ok[i]:
            out[i] = O.attn_decode(O.rope(q[i], hd, hd, int(pos[i]), tref), kr[i], v[i], kc, vc, int(pos[i]), nh, nkv,
                                   hd, scale_of(hd))
            assert np.isfinite(out[i]).all(), (i, pos[i])  # non-finite attention is out of scope
    return out


def qkv(rng, T, nh, nkv, hd, qscale):
    if qscale == MIXED:
        qscale = np.repeat(np.where(np.arange(nh) % 2 == 0, 40.0, 0.05), hd)
    return ((rng.standard_normal((T, nh * hd)) * qscale).astype(np.float32),
            rng.standard_normal((T, nkv * hd)).astype(np.float32),
            rng.standard_normal((T, nkv * hd)).astype(np.float32))


_REFERENCES = {}


def case_reference(O, hd, nh, nkv, n_ctx, batches, qscale):
    """Inputs and reference of one case, computed once and shared by the tests that run it (read-only):
    (kc0, vc0, [(pos, q, k, v, out, kc_after, vc_after) per batch]); the caches evolve over the batches."""
    key = (hd, nh, nkv, n_ctx, batches, qscale)
    if key not in _REFERENCES:
        rng = np.random.default_rng([hd, nh, nkv, n_ctx, len(batches), 1 if qscale == MIXED else int(qscale * 100)])
        tref = O.rope_table(n_ctx, hd, 10000.0)
        kc0, vc0 = rand_caches(rng, n_ctx, nkv * hd)
        kc, vc = kc0.copy(), vc0.copy()
        steps = []
        for pos in batches:
            q, k, v = qkv(rng, len(pos), nh, nkv, hd, qscale)
            out = ref_attn_prompt(O, q, k, v, pos, kc, vc, tref, nh, nkv, hd)
            steps.append((pos, q, k, v, out, kc.copy(), vc.copy()))
        for a in [kc0, vc0] + [a for s in steps for a in s[1:]]:
            a.setflags(write=False)
        _REFERENCES[key] = (kc0, vc0, steps)
    return _REFERENCES[key]
