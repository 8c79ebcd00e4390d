"""mi355x_kv_shift's rule (include/ggml_mi355x.h) in numpy plus libm's fmaf, both forms, on copies
of the caches — test infrastructure. A cached K element pair (k0, k1), the f16 bits at channels
2i, 2i + 1 of a KV head, shifted by an integer delta:
    x0 = f32(k0); x1 = f32(k1)
    (c, s) = table[|delta|][i]; if delta < 0: s = -s
    k0' = f16_rne(fmaf(x0, c, -(x1 * s))); k1' = f16_rne(fmaf(x0, s, x1 * c))
delta == 0: the cell keeps its bits; |delta| >= the table's rows: NaN bits (0x7e00) in the whole
row. The fused multiply-add is libm's fmaf on float32 (one rounding), never a float64 product:
rounding the exact sum to double and then to float can differ from rounding it once.
Caches: K uint16 [n_ctx, n_head_kv * head_dim], V uint16 [n_head_kv * head_dim, n_ctx]; table
float32 [n_pos, head_dim / 2, 2] (cos, sin)."""
import ctypes
import ctypes.util

import numpy as np

NAN_BITS = 0x7e00

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_libm.fmaf.restype = ctypes.c_float
_fmaf = np.frompyfunc(lambda a, b, c: _libm.fmaf(a, b, c), 3, 1)


def fmaf(a, b, c):
    """libm's fmaf element by element on float32 arrays."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    return np.asarray(_fmaf(a, b, c), dtype=np.float32)


def shift_row(row, delta, table, head_dim):
    """One K row (uint16 [kvw]), or several ([n, kvw]), shifted by the one delta: a new array."""
    row = np.array(row, dtype=np.uint16)
    delta = int(delta)
    if delta == 0:
        return row
    if abs(delta) >= table.shape[0]:
        return np.full_like(row, NAN_BITS)
    with np.errstate(all="ignore"):
        x = row.view(np.float16).astype(np.float32).reshape(-1, head_dim // 2, 2)
        c = table[abs(delta), :, 0][None, :]
        s = table[abs(delta), :, 1][None, :]
        if delta < 0:
            s = -s
        x0, x1 = x[..., 0], x[..., 1]
        y0 = fmaf(x0, c, -(x1 * s))
        y1 = fmaf(x0, s, x1 * c)
        out = np.stack([y0, y1], axis=-1).astype(np.float16)
    return out.reshape(row.shape).view(np.uint16)


def shift_deltas(k, delta, table, head_dim):
    """The DELTAS form: K cell c shifted by delta[c] for c < len(delta); a new K cache."""
    k, delta = np.array(k, dtype=np.uint16), np.asarray(delta, dtype=np.int64)
    for d in np.unique(delta).tolist():
        cells = np.nonzero(delta == d)[0]
        k[cells] = shift_row(k[cells], d, table, head_dim)
    return k


def shift_discard(k, v, table, head_dim, keep, discard, n_past):
    """The DISCARD form: for c in [keep, n_past - discard), K cell c = cell c + discard shifted by
    -discard and V cell c = V cell c + discard; new (K, V) caches."""
    k0, v0 = np.array(k, dtype=np.uint16), np.array(v, dtype=np.uint16)
    k, v = k0.copy(), v0.copy()
    if n_past - discard > keep:
        k[keep:n_past - discard] = shift_row(k0[keep + discard:n_past], -discard, table, head_dim)
        v[:, keep:n_past - discard] = v0[:, keep + discard:n_past]
    return k, v


def random_cache(rng, shape):
    """Random finite f16 bits: every exponent but the all-ones one, both signs, subnormals too."""
    bits = rng.integers(0, 1 << 16, size=shape, dtype=np.uint32).astype(np.uint16)
    inf_nan = (bits & 0x7c00) == 0x7c00
    bits[inf_nan] &= np.uint16(0xbfff)  # exponent 30 instead: finite
    return bits
