"""The MoE layer at Mixtral-8x7B's shapes on one MI355X: synthetic Q4_K_M weights (n_embd 4096, n_ff 14336,
8 experts, 2 used, 32 layers unless --layers), warm launches, the rounds interleaved in one session.

1. kq_gemv_id alone (up, gate, down; one token, 2 slots): us and GB/s of the bytes the selected experts
   occupy, beside kq_rows on a dense Q4_K matrix of the same byte count, and the ratio. Successive launches
   rotate over 4 disjoint expert pairs / 4 dense matrices (264 MB), so none finds its bytes in the cache.
2. kq_moe_route and kq_moe_combine alone, beside a minimal launch (mi355x_add of 16 floats).
3. ms/token of LlamaDecoder.step on the model (captured graph, positions 0 .. steps - 1).
Prints one JSON line per part; profiles/moe.txt keeps a run's output.

    python tools/moe_bench.py [--layers 32] [--rounds 5] [--steps 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ggml-neon-opt_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402
from ggml_mi355x.llama import LlamaDecoder, hparams  # noqa: E402

E, F, NE, NU, V = 4096, 14336, 8, 2, 32000
BB = {g.TYPE_Q4_K: 144, g.TYPE_Q6_K: 210}
W2 = {g.TYPE_Q4_K: 66727.0, g.TYPE_Q6_K: 1.865e6}  # E[w^2] / d^2 of random quants (tests/llama_model.py)


def kquant(dev, typ, rows, K, experts=None):
    """Random blocks on the device whose scales keep the activations' RMS O(1)."""
    nb, B = K // 256, BB[typ]
    n = rows * (experts or 1)
    raw = torch.randint(0, 256, (n, nb, B), dtype=torch.uint8, device=dev)
    d = (torch.rand((n, nb), device=dev) * 0.5 + 0.75) / float(np.sqrt(1.0208 * K * W2[typ]))
    if typ == g.TYPE_Q4_K:
        raw[..., 0:2] = d.to(torch.float16).view(torch.uint8).view(n, nb, 2)
        raw[..., 2:4] = (d * 7.5).to(torch.float16).view(torch.uint8).view(n, nb, 2)
    else:
        raw[..., 208:210] = d.to(torch.float16).view(torch.uint8).view(n, nb, 2)
    raw = raw.view(n, nb * B)
    return raw.view(experts, rows, nb * B) if experts else raw


_calls = {}


def timed(fn, pattern, rounds):
    """us of the launches whose kernel name contains `pattern`, one value a round. fn gets a number that goes
    up by one per timed call of its pattern, by which the GEMVs of part 1 rotate over their 4 operands (264 MB
    in all); the warm call before the rounds takes the operand two ahead, not the one timed next."""
    fn(_calls.get(pattern, 0) + 2)
    out = []
    for _ in range(rounds):
        _calls[pattern] = _calls.get(pattern, 0) + 1
        g.timing_enable(True)
        fn(_calls[pattern])
        rows = [r for r in g.timing_read() if pattern in r[0]]
        g.timing_enable(False)
        out.append(sum(r[2] for r in rows) * 1e3 / max(1, len(rows)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    p50 = lambda v: round(float(np.median(v)), 2)  # noqa: E731

    # ---- 1. the expert GEMVs beside kq_rows on the same bytes
    up = kquant(dev, g.TYPE_Q4_K, F, E, NE)
    down = kquant(dev, g.TYPE_Q4_K, E, F, NE)
    # every launch reads other bytes than the 3 before it: 4 disjoint expert pairs, 4 dense matrices, 264 MB each
    # way, more than the 256 MB Infinity Cache, so the figures are HBM streams, not cache hits
    dense_up = [kquant(dev, g.TYPE_Q4_K, NU * F, E) for _ in range(NE // NU)]     # each the bytes of 2 experts' up
    dense_down = [kquant(dev, g.TYPE_Q4_K, NU * E, F) for _ in range(NE // NU)]
    x = torch.randn((1, 1, E), device=dev)
    par = torch.randn((1, NU, F), device=dev)
    recs = []
    for i in range(NE // NU):
        r = torch.zeros((1, 2 * NU), dtype=torch.int32, device=dev)
        r[0, :NU] = torch.tensor([NU * i + 1, NU * i], dtype=torch.int32)
        recs.append(r)
    rec = recs[0]
    res = {}
    for name, ex, xx, K, dn, xd in (("up", up, x, E, dense_up, x[0, 0]), ("down", down, par, F, dense_down, par[0, 0])):
        t_id, t_rows = [], []
        for _ in range(a.rounds):  # interleaved
            t_id += timed(lambda i: g.mul_mat_id(g.TYPE_Q4_K, ex, K, xx, recs[i % len(recs)], NU), "kq_gemv_id", 1)
            t_rows += timed(lambda i: g.mul_mat(g.TYPE_Q4_K, dn[i % len(dn)], K, xd), "kq_rows", 1)
        nbytes = NU * ex.shape[1] * ex.shape[2]
        res[name] = dict(gemv_id_us=p50(t_id), gemv_id_GBs=round(nbytes / p50(t_id) / 1e3, 1), rows_us=p50(t_rows),
                         rows_GBs=round(nbytes / p50(t_rows) / 1e3, 1), ratio=round(p50(t_rows) / p50(t_id), 3),
                         bytes=nbytes, gemv_id_all=[round(v, 2) for v in t_id], rows_all=[round(v, 2) for v in t_rows])
    print(json.dumps(dict(part="gemv_id", gate="as up (same shape)", **res)), flush=True)

    # ---- 2. the router and the combine beside a minimal launch
    gi = torch.randn((NE, E), device=dev) * (2.0 / 64.0)
    ex3 = torch.randn((1, NU, E), device=dev)
    small = torch.zeros(16, device=dev)
    r = dict(route_us=p50(timed(lambda i: g.moe_route(gi, x[0], NU, records=rec), "kq_moe_route", a.rounds)),
             combine_us=p50(timed(lambda i: g.moe_combine(ex3, rec, NU), "kq_moe_combine", a.rounds)),
             minimal_launch_us=p50(timed(lambda i: g.add(small, small), "", a.rounds)))
    print(json.dumps(dict(part="route_combine", **r)), flush=True)
    del up, down, dense_up, dense_down

    # ---- 3. the token
    L = a.layers
    hp = hparams(E, L, 32, 8, F, V, freq_base=1e6, n_expert=NE, n_expert_used=NU)
    w = {"token_embd": (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, V, E)), "output": (g.TYPE_Q6_K, kquant(dev, g.TYPE_Q6_K, V, E)),
         "output_norm": torch.ones(E, device=dev)}
    for i in range(L):
        p = f"blk.{i}."
        more = i < L // 8 or i >= 7 * L // 8 or (i - L // 8) % 3 == 2
        w[p + "attn_norm"] = torch.ones(E, device=dev)
        w[p + "ffn_norm"] = torch.ones(E, device=dev)
        w[p + "attn_q"] = (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, E, E))
        w[p + "attn_k"] = (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, 1024, E))
        vt = g.TYPE_Q6_K if more else g.TYPE_Q4_K
        w[p + "attn_v"] = (vt, kquant(dev, vt, 1024, E))
        w[p + "attn_output"] = (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, E, E))
        w[p + "ffn_gate_inp"] = torch.randn((NE, E), device=dev) * (2.0 / 64.0)
        w[p + "ffn_gate_exps"] = (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, F, E, NE))
        w[p + "ffn_up_exps"] = (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, F, E, NE))
        w[p + "ffn_down_exps"] = (vt, kquant(dev, vt, E, F, NE))
    gb = sum((v[1] if isinstance(v, tuple) else v).numel() * (1 if isinstance(v, tuple) else 4) for v in w.values()) / 1e9
    b = g.Backend()
    dec = LlamaDecoder(b, hp, w, 256)
    ms = []
    for _ in range(a.rounds):
        dec.step(1, 0)
        b.synchronize()
        t0 = time.perf_counter()
        for s in range(1, a.steps + 1):
            lg = dec.step(1 + s % 100, s)
        b.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    finite = bool(torch.isfinite(lg).all())
    print(json.dumps(dict(part="token", layers=L, weights_GB=round(gb, 2), ms_per_token_p50=round(float(np.median(ms)), 4),
                          ms_all=[round(v, 4) for v in ms], logits_finite=finite)), flush=True)
    b.close()


if __name__ == "__main__":
    main()
