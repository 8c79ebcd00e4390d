"""The log-probability rule (include/ggml_mi355x.h, mi355x_logprob_rows), restated in numpy plus the
oracle's v_expf: the reference the device's records must equal bit for bit.

  ref_record(x, t)        one row's record (max, x_target, argmax, pad, sum) as a numpy void scalar
  ref_records(x2d, ts)    a structured array, one record per row
  ref_sum(x)              (argmax, max, S) of a row
  tree_sum(q)             the rule's f64 tree over quad sums
  value(records)          float64 log-probabilities: x_target - max - log(sum), libm's log

Every f32 step is one numpy float32 operation, the quad sums are (e0 + e1) + (e2 + e3) in f32, and
the tree is `t = t[0::2] + t[1::2]` in float64 from 65536 leaves down to one value."""
import math

import numpy as np

MAX_N = 262144
LEAVES = MAX_N // 4
DTYPE = np.dtype([("max", "<f4"), ("x_target", "<f4"), ("argmax", "<i4"), ("pad", "<i4"), ("sum", "<f8")])
NAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def v_expf(d):
    """The oracle's kqo_v_expf, value by value."""
    from oracle import kq_ops_oracle as O
    f = O.lib().kqo_v_expf
    return np.array([f(v) for v in np.ascontiguousarray(d, dtype=np.float32).ravel().tolist()], np.float32)


def ref_argmax(x):
    return int(np.argmax(np.where(np.isnan(x), -np.inf, x)))


def exp_terms(x, m):
    """e_i = 0 where d_i == -inf, else v_expf(d_i), d_i = x_i - m in f32."""
    with np.errstate(all="ignore"):
        d = (np.asarray(x, dtype=np.float32) - np.float32(m)).astype(np.float32)
    e = np.zeros(d.shape, np.float32)
    live = ~np.isneginf(d)
    e[live] = v_expf(d[live])
    return e


def quad_sums(e, leaves=LEAVES):
    """(e_4j + e_4j+1) + (e_4j+2 + e_4j+3) in f32 over e padded with +0.0f to 4 * leaves entries."""
    p = np.zeros(4 * leaves, np.float32)
    p[:len(e)] = e
    with np.errstate(all="ignore"):
        return ((p[0::4] + p[1::4]).astype(np.float32) + (p[2::4] + p[3::4]).astype(np.float32)).astype(np.float32)


def tree_sum(q):
    """The perfect adjacent-pair tree over len(q) leaves (a power of two), each node one f64 add."""
    t = np.asarray(q, dtype=np.float32).astype(np.float64)
    assert len(t) & (len(t) - 1) == 0
    with np.errstate(all="ignore"):
        while len(t) > 1:
            t = t[0::2] + t[1::2]
    return float(t[0])


def ref_sum(x):
    x = np.asarray(x, dtype=np.float32)
    assert 1 <= len(x) <= MAX_N
    a = ref_argmax(x)
    m = x[a]
    return a, m, tree_sum(quad_sums(exp_terms(x, m)))


def ref_record(x, t):
    x = np.asarray(x, dtype=np.float32)
    a, m, S = ref_sum(x)
    r = np.zeros((), DTYPE)
    r["max"], r["argmax"], r["pad"], r["sum"] = m, a, 0, S
    r["x_target"] = x[int(t)] if 0 <= int(t) < len(x) else NAN
    return r


def ref_records(x2d, targets):
    return np.array([ref_record(row, t) for row, t in zip(x2d, targets)], DTYPE)


def value(records):
    r = np.asarray(records)
    logs = np.array([math.log(s) if s > 0 else (-math.inf if s == 0 else math.nan) for s in r["sum"].ravel().tolist()],
                    np.float64).reshape(r.shape)
    with np.errstate(all="ignore"):
        return r["x_target"].astype(np.float64) - r["max"].astype(np.float64) - logs


def same_records(got, want):
    """Bit for bit: max, x_target, argmax, pad and the 8 bytes of sum."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def first_mismatch(got, want):
    for i, (g, w) in enumerate(zip(np.atleast_1d(got), np.atleast_1d(want))):
        if g.tobytes() != w.tobytes():
            return i, g, w, float(g["sum"]).hex(), float(w["sum"]).hex()
    return None
