"""mi355x_attn_prompt_precision(MI355X_ATTN_PROMPT_F16)'s rule (include/ggml_mi355x.h,
ggml-neon-opt_amd/csrc/kq_attn_mfma.hip) in numpy — test infrastructure, no GPU, no torch.

The operands are the exact path's: both caches hold the bits kq_kv_store writes (K uint16
[n_ctx, n_head_kv * hd], V uint16 [n_head_kv * hd, n_ctx], transposed), and the query operand is
q^ = f16(rope(q)), the same f32 rope and RNE conversion as the exact kernels (qhat below takes the
roped f32 row). For one token at position p (0 <= p < n_ctx), head h, kv head g = h // gsz:

emulate (float64):
    s_c = scale * sum_d q^_d K[c][g][d]   for cells c <= p
    m = max s_c;  w_c = exp(s_c - m);  l = sum w_c
    emu_d = sum_c w_c V[g][d][c] / l
Cells c > p contribute nothing, whatever finite bits they hold.

bound (float64), per output element d:
    D   = 2^-23 * hd * scale * max_c sum_d |q^_d K_cd|      f32 accumulation of the dot in any order, the scale multiply
    eps = 2^-10 + 4 D                                       one f16 rounding of each p (2^-11), the exp argument and
                                                            the sum's error, 2x room
    B_d = eps * sum_c w_c |V_dc| / l
          + 2^-24 * sum_{c<=p} |V_dc| / l                   p flushed to zero in f16
          + 2^-24 * (ceil(n/32) + 32) * sum_c w_c |V_dc| / l    f32 accumulation of O over n = p + 1 cells in tiles

restate_f32 (float32): the kernel's own operation order — 32-cell tiles; per tile the f32 dot times
scale, the mask as a select to -inf, the running maximum updated BEFORE the tile's weights are formed
(so p = exp2((s - m) * log2 e) lies in [0, 1]; a row still all masked uses 0 as its maximum), O and l
rescaled by exp(m_old - m_new) at every tile, p rounded to f16 once for the second product, l summing
the unrounded p per lane half, the second product over the tile's cells in the permuted k order of the
accumulator fragment (PERM), one divide by l at the end. Its `mutate` argument produces the three wrong
kernels the bound must reject (tests/test_attn_f16_rule.py): "mask" (c < p instead of c <= p),
"rescale" (O and l not rescaled when the maximum moves), "vorder" (V's cells in natural k order against
P's permuted order)."""
import numpy as np

TILE = 32
LOG2E = np.float32(1.44269504088896341)
# k index 16 s + 8 hf + j of the second product -> cell 16 s + 8 (j >> 2) + 4 hf + (j & 3) of the tile
PERM = np.array([16 * s + 8 * (j >> 2) + 4 * hf + (j & 3) for s in range(2) for hf in range(2) for j in range(8)])
# the lane half that holds a cell of the tile: register i of half hf is cell (i & 3) + 8 (i >> 2) + 4 hf
HALF = (np.arange(TILE) >> 2) & 1


def qhat(q_roped):
    """f16(rope(q)) of a roped f32 row, as float16."""
    return np.asarray(q_roped, np.float32).astype(np.float16)


def _f16(bits):
    a = np.asarray(bits)
    return a.view(np.float16) if a.dtype == np.uint16 else a.astype(np.float16)


def _groups(qh, kc, vc, pos, nh, nkv, hd):
    """Per kv head g: q [gsz, hd], K [n, hd], V [hd, n] of the cells c <= pos, float64."""
    n, gsz = int(pos) + 1, nh // nkv
    q = np.asarray(qh, np.float16).astype(np.float64).reshape(nkv, gsz, hd)
    k, v = _f16(kc), _f16(vc)
    for g in range(nkv):
        yield q[g], k[:n, g * hd:(g + 1) * hd].astype(np.float64), v[g * hd:(g + 1) * hd, :n].astype(np.float64)


def _soft_max(q, k, scale):
    s = float(scale) * (q @ k.T)  # [gsz, n]
    w = np.exp(s - s.max(axis=1, keepdims=True))
    return w, w.sum(axis=1, keepdims=True)


def emulate(qh, kc, vc, pos, nh, nkv, hd, scale):
    """The float64 emulation of one token: [nh * hd]."""
    out = []
    for q, k, v in _groups(qh, kc, vc, pos, nh, nkv, hd):
        w, l = _soft_max(q, k, scale)
        out.append((w @ v.T) / l)
    return np.concatenate(out).reshape(nh * hd)


def bound(qh, kc, vc, pos, nh, nkv, hd, scale):
    """B of one token: [nh * hd] float64."""
    n = int(pos) + 1
    out = []
    for q, k, v in _groups(qh, kc, vc, pos, nh, nkv, hd):
        w, l = _soft_max(q, k, scale)
        delta = 2.0 ** -23 * hd * float(scale) * (np.abs(q) @ np.abs(k).T).max(axis=1, keepdims=True)
        eps = 2.0 ** -10 + 4.0 * delta
        wv = (w @ np.abs(v).T) / l
        av = np.abs(v).sum(axis=1)[None, :] / l
        out.append(eps * wv + 2.0 ** -24 * av + 2.0 ** -24 * (-(-n // TILE) + 32) * wv)
    return np.concatenate(out).reshape(nh * hd)


def restate_f32(qh, kc, vc, pos, nh, nkv, hd, scale, mutate=None):
    """The kernel's operation order in float32 for one token: [nh * hd] float32. kc / vc are the WHOLE
    caches: the last tile reads the cells after pos too and masks them."""
    assert mutate in (None, "mask", "rescale", "vorder")
    f32 = np.float32
    pos, gsz = int(pos), nh // nkv
    n_kv = (pos + TILE) // TILE * TILE
    q = np.asarray(qh, np.float16).astype(f32).reshape(nh, hd)
    kall = np.repeat(_f16(kc)[:n_kv].astype(f32).reshape(n_kv, nkv, hd).transpose(1, 0, 2), gsz, axis=0)  # [nh, n_kv, hd]
    vall = np.repeat(_f16(vc)[:, :n_kv].astype(f32).reshape(nkv, hd, n_kv), gsz, axis=0)                  # [nh, hd, n_kv]
    scale = f32(scale)
    o = np.zeros((nh, hd), f32)
    m = np.full(nh, -np.inf, f32)
    l = np.zeros((nh, 2), f32)  # per lane half
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for c0 in range(0, n_kv, TILE):
            cells = c0 + np.arange(TILE)
            s = (kall[:, c0:c0 + TILE, :] * q[:, None, :]).sum(axis=2, dtype=f32) * scale  # [nh, 32]
            seen = cells < pos if mutate == "mask" else cells <= pos
            s = np.where(seen[None, :], s, f32(-np.inf))
            mn = np.maximum(m, s.max(axis=1))
            mu = np.where(np.isneginf(mn), f32(0.0), mn)
            alpha = np.exp2((m - mu) * LOG2E).astype(f32)
            if mutate == "rescale":
                alpha = np.ones_like(alpha)
            m = mn
            p = np.exp2((s - mu[:, None]) * LOG2E).astype(f32)  # in [0, 1]
            assert (p <= 1.0).all() and np.isfinite(p).all()
            ps = np.zeros((nh, 2), f32)
            for c in range(TILE):  # each half sums its 16 registers in order
                ps[:, HALF[c]] += p[:, c]
            l = l * alpha[:, None] + ps
            p16 = p.astype(np.float16).astype(f32)
            vt = vall[:, :, c0:c0 + TILE]
            acc = o * alpha[:, None]
            for kk in range(TILE):
                vcell = kk if mutate == "vorder" else PERM[kk]
                acc = acc + vt[:, :, vcell] * p16[:, PERM[kk], None]
            o = acc
        out = o * (f32(1.0) / (l[:, 0] + l[:, 1]))[:, None]
    return out.reshape(nh * hd)
