"""Streamed decode attention (mi355x_attn_stream: kq_attn_stream_scores + _softmax + _kqv) per
position, launch-event timed, TinyLlama (hd 64, 32/4 heads) and Llama-3-8B (hd 128, 32/8):
 A  mode 2 against mode 0 (today's kernel: the split over cells) at 4096 and 6144 cells, the
    rounds of the two interleaved in one process;
 B  mode 1 at 8192, 16384, 32768 and 131072 cells at the last position: us per launch and the
    achieved K + V cache bytes/s (the live cells of both caches, 2 * n_kv * kvw * 2 bytes, read
    once per token by the scores and the KQV launches) against the 8 TB/s HBM peak.
Prints one line per case; --out FILE also writes them there."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--max-ctx", type=int, default=131072)
args = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(mode, call, reps):
    """Per-kernel launch times (us) of `reps` calls under mi355x_attn_stream(mode)"""
    prev = g.attn_stream(mode)
    try:
        call()
        torch.cuda.synchronize()
        g.timing_enable(True)
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        rows = g.timing_read()
    finally:
        g.timing_enable(False)
        g.attn_stream(prev)
    per = {}
    for r in rows:
        per.setdefault(r[0].replace("kq::", ""), []).append(r[2] * 1000.0)  # ms -> us
    return per


def setup(hd, nh, nkv, n_ctx):
    kvw = nkv * hd
    kc = (torch.randn(n_ctx, kvw, device=dev) * 0.5).half().view(torch.int16)
    vc = (torch.randn(kvw, n_ctx, device=dev) * 0.5).half().view(torch.int16)
    tab = g.rope_table(n_ctx, hd, 10000.0, 1.0, device=dev)
    return kc, vc, tab, torch.randn(nh * hd, device=dev), torch.randn(kvw, device=dev), torch.randn(kvw, device=dev)


SHAPES = (("tinyllama", 64, 32, 4), ("llama3-8b", 128, 32, 8))
say("# A: mode 2 (streamed) against mode 0 (the default kernel), us per launch: median [min] over "
    f"{args.rounds} interleaved rounds x {args.reps} calls")
for name, hd, nh, nkv in SHAPES:
    for n_ctx in (4096, 6144):
        kc, vc, tab, q, k, v = setup(hd, nh, nkv, n_ctx)
        for p in (n_ctx // 2 - 1, n_ctx - 1):
            pos = torch.tensor([p], dtype=torch.int32, device=dev)
            row = tab[p].contiguous()
            call = lambda: g.attn_decode(q, k, v, pos, row, kc, vc, nh, nkv, hd, 0.125, rope_row=True)  # noqa: E731
            acc = {0: {}, 2: {}}
            for _ in range(args.rounds):
                for mode in (0, 2):
                    for kn, vals in timed(mode, call, args.reps).items():
                        acc[mode].setdefault(kn, []).extend(vals)
            out = {}
            for mode in (0, 2):
                per = {kn: (float(np.median(v_)), float(np.min(v_))) for kn, v_ in acc[mode].items()}
                out[mode] = (sum(m for m, _ in per.values()), sum(lo for _, lo in per.values()), per)
            say(f"{name} n_ctx {n_ctx} pos {p}: default {out[0][0]:.2f} [{out[0][1]:.2f}] us  streamed {out[2][0]:.2f} "
                f"[{out[2][1]:.2f}] us  ratio {out[2][0] / out[0][0]:.3f}")
            for mode in (0, 2):
                say("    mode %d: %s" % (mode, ", ".join(f"{kn} {m:.2f}" for kn, (m, _) in sorted(out[mode][2].items()))))
        del kc, vc, tab

say("# B: mode 1 past the wall, last position: us per launch (median), live K + V bytes / total time")
for name, hd, nh, nkv in SHAPES:
    for n_ctx in (8192, 16384, 32768, 131072):
        if n_ctx > args.max_ctx:
            continue
        kc, vc, tab, q, k, v = setup(hd, nh, nkv, n_ctx)
        p = n_ctx - 1
        pos = torch.tensor([p], dtype=torch.int32, device=dev)
        row = tab[p].contiguous()
        call = lambda: g.attn_decode(q, k, v, pos, row, kc, vc, nh, nkv, hd, 0.125, rope_row=True)  # noqa: E731
        per = {kn: float(np.median(v_)) for kn, v_ in timed(1, call, 2 * args.reps).items()}
        total = sum(per.values())
        nbytes = 2.0 * n_ctx * nkv * hd * 2
        say(f"{name} n_ctx {n_ctx}: {total:.1f} us ({', '.join(f'{kn} {m:.1f}' for kn, m in sorted(per.items()))})  "
            f"K+V {nbytes / 1e6:.1f} MB -> {nbytes / total / 1e6:.2f} TB/s = {nbytes / total / 1e6 / 8.0 * 100:.1f} % of 8 TB/s")
        del kc, vc, tab
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
