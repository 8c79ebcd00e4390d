"""kq_gemv_q3k and kq_mmq's Q3_K body beside the Q4_K / Q6_K kernels at the same N x K, in one session:
device-event times (mi355x_timing) of interleaved rounds, medians and ranges, GB/s of the weight bytes.

  python tools/q3k_bench.py [--rounds 5] [--reps 40] [--prefill 512] [--sweep 16,24,32,48,64] [--out profiles/q3k.txt]

Decode (M = 1): TinyLlama's and Llama-3-8B's q, gate + up (two launches), down and output.
Prefill (M = --prefill, 0: skip): Q3_K on kq_mmq (q3k_prefill's default) and on the GEMV over column groups
(Q3K_PREFILL_GEMV), beside kq_mmq on Q4_K / Q6_K.
Sweep (--sweep, "": skip): the two Q3_K paths at each M, kq_mmq forced from 16 columns (Q3K_PREFILL_MMQ):
where they cross."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]

MODELS = {"tinyllama": (2048, 5632, 32000), "llama3-8b": (4096, 14336, 128256)}


def shapes(E, F, V):
    return [("q", [(E, E)]), ("gate+up", [(F, E), (F, E)]), ("down", [(E, F)]), ("output", [(V, E)])]


def main():
    import torch
    import ggml_mi355x as g
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--prefill", type=int, default=512)
    ap.add_argument("--sweep", default="16,24,32,48,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not g.device_available():
        raise SystemExit("q3k_bench: no gfx950 device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = [f"# q3k_bench: {a.rounds} interleaved rounds x {a.reps} launches, device events; us = median of the "
             f"round medians [min .. max], GB/s = weight bytes / median"]

    def weights(type_, N, K):
        raw = rng.integers(0, 256, size=(N, K // 256 * g.BLOCK_BYTES[type_]), dtype=np.uint8)
        return torch.from_numpy(raw).to(dev)

    def once(type_, mats, x):
        """device time of the launches of one call over every matrix (us)"""
        g.timing_enable(True)
        for w, K in mats:
            g.mul_mat(type_, w, K, x)
        rows = g.timing_read()
        g.timing_enable(False)
        return sum(r[2] for r in rows) * 1e3, "+".join(sorted({r[0] for r in rows}))

    def measure(variants, nk, M):
        """variants: (label, type, q3k_prefill mode). Interleaved rounds; {label: median us}, one line each."""
        x = torch.from_numpy(rng.standard_normal((M, nk[0][1])).astype(np.float32)).to(dev)
        mats = {ty: [(weights(ty, N, K), K) for N, K in nk] for ty in {v[1] for v in variants}}

        def timed(v):
            prev = g.q3k_prefill(v[2])
            try:
                return once(v[1], mats[v[1]], x)
            finally:
                g.q3k_prefill(prev)

        for v in variants:  # warm-up: code objects, workspaces
            timed(v)
        meds, kern = {v[0]: [] for v in variants}, {}
        for _ in range(a.rounds):
            for v in variants:  # interleaved
                ts = []
                for _ in range(a.reps):
                    us, kern[v[0]] = timed(v)
                    ts.append(us)
                meds[v[0]].append(statistics.median(ts))
        res = {}
        for label, ty, _ in variants:
            res[label] = med = statistics.median(meds[label])
            wb = sum(N * K // 256 * g.BLOCK_BYTES[ty] for N, K in nk)
            lines.append(f"{tag} {label:9s} {med:9.2f} us [{min(meds[label]):9.2f} .. {max(meds[label]):9.2f}] "
                         f"{wb / med / 1e3:8.1f} GB/s  {kern[label]}")
        return res, meds

    Q3, AUTO, GEMV, MMQ = g.TYPE_Q3_K, g.Q3K_PREFILL_AUTO, g.Q3K_PREFILL_GEMV, g.Q3K_PREFILL_MMQ
    for M in [1] + ([a.prefill] if a.prefill else []):
        variants = [("q3_K", Q3, AUTO), ("q4_K", g.TYPE_Q4_K, AUTO)]
        if M > 1:
            variants += [("q6_K", g.TYPE_Q6_K, AUTO), ("q3_K gemv", Q3, GEMV)]
        lines.append(f"## M = {M}")
        for model, (E, F, V) in MODELS.items():
            for name, nk in shapes(E, F, V):
                tag = f"{model:10s} {name:8s}"
                res, meds = measure(variants, nk, M)
                lines.append(f"{tag} q3_K / q4_K = {res['q3_K'] / res['q4_K']:.3f}")
                if M > 1:  # round by round: the GEMM against the GEMV over groups, and against Q4_K's GEMM
                    lines.append(f"{tag} q3_K / q3_K gemv per round: " +
                                 " ".join(f"{p / q:.3f}" for p, q in zip(meds["q3_K"], meds["q3_K gemv"])))
                    lines.append(f"{tag} q3_K / q4_K per round: " +
                                 " ".join(f"{p / q:.3f}" for p, q in zip(meds["q3_K"], meds["q4_K"])))
    for M in [int(v) for v in a.sweep.split(",") if v]:
        lines.append(f"## sweep M = {M}: kq_mmq forced (Q3K_PREFILL_MMQ) against kq_gemv_q3k")
        for model, (E, F, V) in MODELS.items():
            for name, nk in shapes(E, F, V)[:3]:
                tag = f"{model:10s} {name:8s}"
                res, _ = measure([("q3_K mmq", Q3, MMQ), ("q3_K gemv", Q3, GEMV)], nk, M)
                lines.append(f"{tag} mmq / gemv = {res['q3_K mmq'] / res['q3_K gemv']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
