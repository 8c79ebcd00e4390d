"""kq_gemv_q3k beside the Q4_K / Q6_K kernels at the same N x K, in one session: device-event
times (mi355x_timing) of interleaved rounds, medians and ranges, GB/s of the weight bytes.

  python tools/q3k_bench.py [--rounds 5] [--reps 40] [--prefill 512] [--out profiles/q3k.txt]

Decode (M = 1): TinyLlama's and Llama-3-8B's q, gate + up (two launches), down and output.
Prefill (M = --prefill, 0: skip): Q3_K runs the GEMV over column groups, beside kq_mmq."""
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

    for M in [1] + ([a.prefill] if a.prefill else []):
        types = [g.TYPE_Q3_K, g.TYPE_Q4_K] + ([g.TYPE_Q6_K] if M > 1 else [])
        lines.append(f"## M = {M}")
        for model, (E, F, V) in MODELS.items():
            for name, nk in shapes(E, F, V):
                x = torch.from_numpy(rng.standard_normal((M, nk[0][1])).astype(np.float32)).to(dev)
                mats = {ty: [(weights(ty, N, K), K) for N, K in nk] for ty in types}
                for ty in types:  # warm-up: code objects, workspaces
                    once(ty, mats[ty], x)
                meds = {ty: [] for ty in types}
                kern = {}
                for _ in range(a.rounds):
                    for ty in types:  # interleaved
                        ts = []
                        for _ in range(a.reps):
                            us, kern[ty] = once(ty, mats[ty], x)
                            ts.append(us)
                        meds[ty].append(statistics.median(ts))
                res = {}
                for ty in types:
                    med = statistics.median(meds[ty])
                    wb = sum(N * K // 256 * g.BLOCK_BYTES[ty] for N, K in nk)
                    res[ty] = med
                    lines.append(f"{model:10s} {name:8s} {g.TYPE_NAMES[ty]:5s} {med:9.2f} us [{min(meds[ty]):9.2f} .. "
                                 f"{max(meds[ty]):9.2f}] {wb / med / 1e3:8.1f} GB/s  {kern[ty]}")
                lines.append(f"{model:10s} {name:8s} q3_K / q4_K = {res[g.TYPE_Q3_K] / res[g.TYPE_Q4_K]:.3f}")
                del mats
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
