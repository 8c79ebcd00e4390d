"""The sampler's rule (include/ggml_mi355x.h, mi355x_sample), restated in numpy float32 plus the
oracle's v_expf: the reference the device must equal token for token, with no tolerance.

  ref_topk(x, k)                       the candidates: sorted(non-NaN i, key=(-ordered value, i))[:k]
  ref_sample(x, u, top_k, top_p, min_p, temp)   the token
  ref_trace(...)                       the token with the intermediate values (the CPU tests)
  chain(x, c, u, top_p, min_p, temp)   the rule's steps on given candidates

Every arithmetic step is one numpy float32 operation (one rounding, nothing contracted, a
correctly rounded division) and every sum runs in candidate order."""
import numpy as np

F = np.float32


def v_expf(d):
    from oracle import kq_ops_oracle as O
    return np.asarray(O.v_expf(np.ascontiguousarray(d, dtype=np.float32)), dtype=np.float32)


def ref_argmax(x):
    return int(np.argmax(np.where(np.isnan(x), -np.inf, x)))


def ref_topk(x, k):
    """Indices of the min(k, non-NaN entries) largest entries, larger value first (-0.0 == +0.0:
    numpy's float compare), among equal values the smaller index."""
    x = np.asarray(x, dtype=np.float32)
    ok = np.flatnonzero(~np.isnan(x))
    v = x[ok] + F(0.0)  # -0.0 -> +0.0 (the sort key only)
    order = np.lexsort((ok, -v.astype(np.float64)))  # by -value, then by index (f64: exact, -(-inf) fine)
    return ok[order][:k].astype(np.int64)


def ref_topk_out(x, k):
    """(idx int32 [k], val f32 [k]) as mi355x_topk writes them: -1 / the NaN 0x7fc00000 past m."""
    c = ref_topk(x, k)
    idx = np.full(k, -1, np.int32)
    val = np.full(k, np.array([0x7fc00000], np.uint32).view(np.float32)[0], np.float32)
    idx[:len(c)] = c
    val[:len(c)] = np.asarray(x, dtype=np.float32)[c]
    return idx, val


def seq_sums(v):
    """Running sums v_0, v_0 + v_1, ... in order, one float32 add each."""
    out = np.empty(len(v), np.float32)
    acc = F(0.0)
    for i, t in enumerate(v):
        acc = F(t) if i == 0 else F(acc + F(t))
        out[i] = acc
    return out


def ref_trace(x, u, top_k=40, top_p=0.95, min_p=0.05, temp=0.8):
    x = np.asarray(x, dtype=np.float32)
    return chain(x, ref_topk(x, top_k), u, top_p, min_p, temp)


def chain(x, c, u, top_p, min_p, temp, expf=v_expf):
    """The rule's steps on the sorted candidates c (indices into x). expf: the exponential; anything
    but v_expf is not the rule (tools/generate_bench.py times the host loop with numpy's)."""
    u, top_p, min_p, temp = F(u), F(top_p), F(min_p), F(temp)
    m = len(c)
    tr = dict(c=c, m=m)
    if m == 0:
        return dict(tr, token=0)
    l = x[c]
    if temp == 0 or m == 1 or not np.isfinite(l[0]):
        return dict(tr, token=int(c[0]))
    with np.errstate(all="ignore"):
        d = (l - l[0]).astype(np.float32)
        e = np.where(np.isneginf(d), F(0.0), expf(d)).astype(np.float32)
        S = seq_sums(e)[-1]
        p = (e / S).astype(np.float32)
        fails = np.flatnonzero(~(e >= min_p))
        qa = int(fails[0]) if len(fails) else m
        qb = m
        if top_p < 1:
            reached = np.flatnonzero(seq_sums(p) >= top_p)
            qb = int(reached[0]) + 1 if len(reached) else m
        q = max(1, min(qa, qb))
        t = (d / temp).astype(np.float32)
        f = np.where(np.isneginf(t), F(0.0), expf(t)).astype(np.float32)
        run = seq_sums(f[:q])
        Fq = run[-1]
        r = F(u * Fq)
        over = np.flatnonzero(run > r)
    k = int(over[0]) if len(over) else q - 1
    return dict(tr, token=int(c[k]), k=k, q=q, qa=qa, qb=qb, e=e, p=p, f=f, F=Fq, S=S, r=r)


def ref_sample(x, u, top_k=40, top_p=0.95, min_p=0.05, temp=0.8):
    return ref_trace(x, u, top_k, top_p, min_p, temp)["token"]


def draws(seed, n):
    """The draws table of LlamaDecoder.generate(sampler=Sampler(seed=...)): entry p picks the token
    that will stand at position p. seed: an int, or [seed, i] for sequence i of a batch."""
    return np.random.Generator(np.random.PCG64(seed)).random(n, dtype=np.float32)
