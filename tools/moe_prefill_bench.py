"""MoE prefill at Mixtral-8x7B's shapes on one MI355X: one synthetic layer (up / gate 14336 x 4096 Q4_K, down
4096 x 14336 Q6_K, 8 experts of which 2 are used, about 0.9 GB), mi355x_mul_mat_id in both forms, warm launches,
rounds of MOE_PREFILL_GEMV and MOE_PREFILL_GROUPED interleaved in one session.

Per T in --tokens and per form: the p50 over the rounds of each MUL_MAT_ID launch (kq_gemv_id, or kq_mmq_id), of
kq_moe_group and of the two kq_quantize_q8L launches a layer needs (up and gate share one, down has its own), and the
layer's sum: 3 kq_gemv_id against kq_moe_group + 2 kq_quantize_q8L + 3 kq_mmq_id, which is what the graph backend
launches. Beside them kq_mmq on ONE dense matrix of the same type and rows with M = T * 2 columns: the same MFMA work
with no ragged tiles and an eighth of the weight bytes, the ceiling of the grouped form. Routing: uniform random
ids, and at the largest T also the skewed case (every token on experts 0 and 1).
"p0": the smallest measured pair count from which grouped was not slower than gemv in every round, there and at
every larger T (kMoeGroupedMinPairs is chosen from it). One JSON line per (T, routing), then the "p0" line;
profiles/moe_prefill.txt keeps a run's output.

    python tools/moe_prefill_bench.py [--tokens 8,16,32,64,128,512] [--rounds 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ggml-neon-opt_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402
from tools.moe_bench import kquant  # noqa: E402

E, F, NE, NU = 4096, 14336, 8, 2


def launches(fn):
    """[(kernel name, us)] of the launches fn makes."""
    g.timing_enable(True)
    fn()
    rows = [(r[0], r[2] * 1e3) for r in g.timing_read()]
    g.timing_enable(False)
    return rows


def one(rows, pattern):
    us = [t for n, t in rows if pattern in n]
    assert len(us) == 1, (pattern, rows)
    return us[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="8,16,32,64,128,512")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    tokens = [int(t) for t in a.tokens.split(",")]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    mats = {"up": (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, F, E, NE), E), "gate": (g.TYPE_Q4_K, kquant(dev, g.TYPE_Q4_K, F, E, NE), E),
            "down": (g.TYPE_Q6_K, kquant(dev, g.TYPE_Q6_K, E, F, NE), F)}
    dense = {"up": kquant(dev, g.TYPE_Q4_K, F, E), "down": kquant(dev, g.TYPE_Q6_K, E, F)}
    p50 = lambda v: round(float(np.median(v)), 2)  # noqa: E731
    wins = {}
    cases = [(T, "uniform") for T in tokens] + [(max(tokens), "experts_0_1")]
    for T, routing in cases:
        P = T * NU
        ids = np.stack([rng.permutation(NE)[:NU] for _ in range(T)]) if routing == "uniform" else np.tile([0, 1], (T, 1))
        rec = torch.zeros((T, 2 * NU), dtype=torch.int32, device=dev)
        rec[:, :NU] = torch.from_numpy(ids.astype(np.int32)).to(dev)
        x = {"up": torch.randn((T, 1, E), device=dev), "down": torch.randn((T, NU, F), device=dev)}
        x["gate"] = x["up"]
        xd = {"up": torch.randn((P, E), device=dev), "down": x["down"].view(P, F)}  # M = P columns of the dense GEMM
        out = {k: torch.empty((T, NU, m[1].shape[1]), device=dev) for k, m in mats.items()}
        call = {k: (lambda k=k: g.mul_mat_id(mats[k][0], mats[k][1], mats[k][2], x[k], rec, NU, out=out[k])) for k in mats}
        t = {f: {k: [] for k in ("up", "gate", "down", "group", "quant_up", "quant_down", "layer")} for f in ("gemv", "grouped")}
        t["dense"] = {"up": [], "down": []}
        for r in range(a.rounds + 1):  # round 0 warms every shape and is dropped
            for form, impl in (("gemv", g.MOE_PREFILL_GEMV), ("grouped", g.MOE_PREFILL_GROUPED)):
                prev = g.moe_prefill(impl)
                rows = {k: launches(call[k]) for k in ("up", "gate", "down")}
                g.moe_prefill(prev)
                if not r:
                    continue
                kern = "kq_gemv_id" if form == "gemv" else "kq_mmq_id"
                us = {k: one(rows[k], kern) for k in rows}
                if form == "grouped":
                    us["group"] = one(rows["up"], "kq_moe_group")
                    us["quant_up"] = one(rows["up"], "kq_quantize_q8L")
                    us["quant_down"] = one(rows["down"], "kq_quantize_q8L")
                us["layer"] = sum(us.values())
                for k, v in us.items():
                    t[form][k].append(v)
            for k in ("up", "down"):
                rows = launches(lambda k=k: g.mul_mat(mats[k][0], dense[k], mats[k][2], xd[k]))
                if r:
                    t["dense"][k].append(one(rows, "kq_mmq<"))
        # the Q6_K tile shapes of kq_mmq_id on `down` forced by the MMQ_ID_Q6 knob, interleaved (the library
        # takes 128 x 128 from 128 pairs an expert on average, 128 x 64 below)
        shapes = {"128x64": 3, "128x128": 1, "64x128": 2}
        t["down_q6_tiles"] = {s: [] for s in shapes}
        prev = g.moe_prefill(g.MOE_PREFILL_GROUPED)
        for r in range(a.rounds + 1):
            for s, v in shapes.items():
                g.debug_knob("MMQ_ID_Q6", v)
                us = one(launches(call["down"]), "kq_mmq_id")
                if r:
                    t["down_q6_tiles"][s].append(us)
        g.debug_knob("MMQ_ID_Q6")  # (NaN: back to the default)
        g.moe_prefill(prev)
        res = {f: {k: p50(v) for k, v in t[f].items() if v} for f in t}
        never_slower = all(gr <= gv for gr, gv in zip(t["grouped"]["layer"], t["gemv"]["layer"]))
        if routing == "uniform":
            wins[P] = never_slower
        print(json.dumps(dict(T=T, pairs=P, routing=routing, rounds=a.rounds, us_p50=res,
                              layer_speedup=round(res["gemv"]["layer"] / res["grouped"]["layer"], 2),
                              grouped_never_slower=never_slower,
                              layer_all={f: [round(v, 1) for v in t[f]["layer"]] for f in ("gemv", "grouped")})), flush=True)
    p0 = None
    for P in sorted(wins, reverse=True):
        if not wins[P]:
            break
        p0 = P
    print(json.dumps(dict(p0=p0, note="smallest measured pair count from which grouped is never slower, up to the largest")),
          flush=True)


if __name__ == "__main__":
    main()
