"""tests/moe_ref.py against brute force: the properties of the MoE rule (include/ggml_mi355x.h,
mi355x_moe_route / mi355x_mul_mat_id / mi355x_moe_combine) that the GPU tests rely on. No device."""
import numpy as np

from oracle import kq_oracle as KO
from oracle import kq_oracle_np as N
from oracle import kq_ops_oracle as O
from tests import moe_ref as M

F32 = np.float32


def test_vec_dot_f32_is_the_neon_order():
    rng = np.random.default_rng(1)
    for n in (16, 256, 512):
        x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
        # brute force: 16 scalar chains, element by element
        acc = [F32(0)] * 16
        for i in range(n):
            acc[i % 16] = N.fma_f32(x[i], y[i], acc[i % 16])[()]
        lanes = [F32(F32(acc[l] + acc[8 + l]) + F32(acc[4 + l] + acc[12 + l])) for l in range(4)]
        want = F32(F32(lanes[0] + lanes[1]) + F32(lanes[2] + lanes[3]))
        got = M.vec_dot_f32(x, y)
        assert got.view(np.uint32) == want.view(np.uint32)
        assert abs(float(got) - float(np.dot(x.astype(np.float64), y.astype(np.float64)))) < 1e-3
    # the order matters: a plain sequential sum gives other bits somewhere
    x, y = rng.standard_normal(512).astype(F32), rng.standard_normal(512).astype(F32)
    seq = F32(0)
    for i in range(512):
        seq = N.fma_f32(x[i], y[i], seq)[()]
    assert M.vec_dot_f32(x, y).view(np.uint32) != seq.view(np.uint32)


def test_probs_are_soft_max_row():
    rng = np.random.default_rng(2)
    for ne in (2, 8, 64):
        gi = rng.standard_normal((ne, 256)).astype(F32)
        cur = rng.standard_normal(256).astype(F32)
        _, _, probs = M.route(gi, cur, 1)
        want = O.soft_max_row(np.array([M.vec_dot_f32(g, cur) for g in gi], F32))
        assert (probs.view(np.uint32) == want.view(np.uint32)).all()
        assert abs(float(probs.astype(np.float64).sum()) - 1.0) < 1e-5


def test_tie_free_top_k_is_argsort():
    rng = np.random.default_rng(3)
    for ne, k in ((2, 1), (8, 2), (64, 8), (8, 8)):
        for _ in range(20):
            p = rng.permutation(ne).astype(F32) / F32(ne * 2)  # distinct
            ids, w = M.route_probs(p, k)
            assert (ids == np.argsort(-p, kind="stable")[:k]).all()
            assert (np.diff(w) < 0).all()  # descending


def test_tied_row_follows_the_exchange_sort():
    # [a, b, b, a] with b > a. Pass 0 swaps 0 <-> 1: [b, a, b, a] as values, idx [1, 0, 2, 3]; pass 1 at
    # position 1 (value a) meets position 2 (b): swap: idx [1, 2, 0, 3]; pass 2: position 2 holds idx 0 (a),
    # position 3 idx 3 (a): no swap. The tied a's come out as [0, 3], the tied b's as [1, 2].
    p = np.array([0.1, 0.4, 0.4, 0.1], F32)
    assert M.argsort_desc(p).tolist() == [1, 2, 0, 3]
    # where "smallest index first" fails: [a, c, b, b', a'] ... a displaced value lands behind its twin
    p = np.array([0.2, 0.3, 0.2, 0.3], F32)
    # pass 0: idx0 (0.2) < idx1 (0.3): swap -> [1, 0, 2, 3]; 0.3 < 0.2? no; 0.3 < 0.3? no.
    # pass 1: position 1 = idx 0 (0.2): vs idx 2 (0.2) no; vs idx 3 (0.3) swap -> [1, 3, 2, 0]
    # pass 2: position 2 = idx 2 (0.2) vs idx 0 (0.2): no. The tied 0.2's come out as [2, 0]: larger index first.
    assert M.argsort_desc(p).tolist() == [1, 3, 2, 0]
    assert M.argsort_desc(p).tolist() != np.argsort(-p, kind="stable").tolist()
    ids, w = M.route_probs(p, 3)
    assert ids.tolist() == [1, 3, 2]
    # all equal: nothing ever swaps
    assert M.argsort_desc(np.full(8, 0.125, F32)).tolist() == list(range(8))
    # two identical router rows give tied probabilities, bit for bit
    rng = np.random.default_rng(4)
    gi = rng.standard_normal((8, 256)).astype(F32)
    gi[5] = gi[2]
    cur = rng.standard_normal(256).astype(F32)
    _, _, probs = M.route(gi, cur, 2)
    assert probs[5].view(np.uint32) == probs[2].view(np.uint32)


def test_weights_sum_to_one_within_an_ulp():
    rng = np.random.default_rng(5)
    for ne, k in ((2, 1), (2, 2), (8, 2), (64, 8)):
        for _ in range(200):
            probs = O.soft_max_row((rng.standard_normal(ne) * 3).astype(F32))
            ids, w = M.route_probs(probs, k)
            s = float(w.astype(np.float64).sum())
            assert abs(s - 1.0) <= 2.0 ** -23, (ne, k, s)  # 1 ulp of 1.0
            if k == 1:
                assert w[0] == F32(1.0)
            # the rule's own arithmetic, restated
            d = np.float64(0)
            for v in probs[ids]:
                d += np.float64(v)
            assert (w.view(np.uint32) == (probs[ids] / F32(d)).view(np.uint32)).all()


def test_mul_mat_id_is_mul_mat_on_the_gathered_expert():
    rng = np.random.default_rng(6)
    K, Nr, ne, T, nu = 512, 12, 4, 3, 2
    for typ in (N.Q4_K, N.Q5_K, N.Q6_K):
        ex = np.stack([N.random_blocks(rng, typ, Nr, K) for _ in range(ne)])
        ids = np.array([[0, 3], [2, 2], [3, 1]], np.int32)
        for ne11 in (1, nu):
            x = rng.standard_normal((T, ne11, K)).astype(F32)
            got = M.mul_mat_id(typ, ex, x, ids)
            assert got.shape == (T, nu, Nr)
            for t in range(T):
                for s in range(nu):
                    want = KO.mul_mat(typ, ex[ids[t, s]], x[t, s % ne11][None])[0]
                    assert (got[t, s].view(np.uint32) == want.view(np.uint32)).all()
    bad = M.mul_mat_id(N.Q4_K, np.stack([N.random_blocks(rng, N.Q4_K, 4, 256)] * 2), rng.standard_normal((1, 1, 256)).astype(F32),
                       np.array([[1, 2]]))
    assert np.isfinite(bad[0, 0]).all() and np.isnan(bad[0, 1]).all()


def test_combine_order_is_pinned():
    # (a + b) + c != a + (b + c): 1 + 2^-24 + 2^-24 in f32, weights 1
    a, b, c = F32(1.0), F32(2.0 ** -24), F32(2.0 ** -24)
    assert F32(F32(a + b) + c) != F32(a + F32(b + c))
    ex = np.array([[a], [b], [c]], F32)
    out = M.combine(ex, np.ones(3, F32))
    assert out[0] == F32(F32(a + b) + c) == F32(1.0)
    out = M.combine(ex[::-1], np.ones(3, F32))
    assert out[0] == F32(F32(c + b) + a) and out[0] != F32(1.0)
    # products are rounded before they are added (no fused multiply-add)
    e = np.array([[F32(1.0 + 2.0 ** -12)], [F32(-1.0)]], F32)
    w = np.array([F32(1.0 + 2.0 ** -12), F32(1.0)], F32)
    out = M.combine(e, w)
    assert out[0] == F32(F32(e[0, 0] * w[0]) + F32(e[1, 0] * w[1]))
    assert float(out[0]) != float(np.float64(e[0, 0]) * np.float64(w[0]) - 1.0)
    # n_used == 1: the product alone
    assert M.combine(np.array([[F32(3.0)]], F32), np.array([F32(0.5)]))[0] == F32(1.5)
