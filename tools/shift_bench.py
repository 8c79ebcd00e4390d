"""The context shift next to the only alternative there was before it, on one box in one session:
LlamaDecoder.shift (one kq_kv_shift launch a layer, DISCARD form) against prompt() over the kept
tokens, on TinyLlama shapes with synthetic weights at n_ctx 4096, keep 256 and generate(keep=)'s
default discard (n_ctx - keep) // 2 = 1920, so 2176 tokens stay. Rounds of both are interleaved.

    python tools/shift_bench.py [--n-ctx 4096] [--keep 256] [--rounds 5] [--reps 10]

Per round: shift() with its captured graph warm, between two events on the backend stream (the
median of `reps`), and by the host clock from the call to the end of a synchronize; prompt() of the
n_ctx - discard kept tokens by the same host clock (its graph warm too; it stages its inputs on the
host first, which is part of what a user pays). Then the kq_kv_shift launches alone by
mi355x_timing (eager): microseconds a launch, and the bytes the launch must move (every moved K
and V cell read once and written once) over that time, against the 8 TB/s HBM peak.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ggml-neon-opt_amd"))

import torch  # noqa: E402

import bench  # noqa: E402
import ggml_mi355x as g  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def wall_ms(be, fn):
    be.synchronize()
    t0 = time.perf_counter()
    fn()
    be.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ctx", type=int, default=4096)
    ap.add_argument("--keep", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    n_ctx, keep = args.n_ctx, args.keep
    discard = (n_ctx - keep) // 2
    kept = n_ctx - discard
    dev = torch.device("cuda:0")
    be = g.Backend()
    tk = bench.Token("tinyllama-1.1b", dev, 0x51A7, be, n_ctx)
    dec, hp = tk.dec, tk.hp
    kvw, n_layer = hp["n_head_kv"] * hp["head_dim"], hp["n_layer"]
    for c in dec.k_cache + dec.v_cache:  # finite values of a cache's size: what a full cache holds
        c.copy_((torch.randn(c.shape, device=dev) * 0.5).half().view(torch.int16))
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(be.stream)
    tokens = tk.tokens[:kept]

    def shift():
        dec.shift(n_ctx, keep, discard)

    def reprompt():
        dec.prompt(tokens, 0)

    for _ in range(3):  # warm-up: both graphs captured, code objects loaded
        shift()
        reprompt()
    be.synchronize()
    rounds = []
    for _ in range(args.rounds):
        ev = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            be.synchronize()
            e0.record(stream)
            shift()
            e1.record(stream)
            be.synchronize()
            ev.append(e0.elapsed_time(e1))
        rounds.append({"shift_events_ms_p50": round(statistics.median(ev), 4), "shift_wall_ms": round(wall_ms(be, shift), 4),
                       "reprompt_wall_ms": round(wall_ms(be, reprompt), 3)})
    for r in rounds:
        r["shift_below_reprompt"] = r["shift_wall_ms"] < r["reprompt_wall_ms"] and r["shift_events_ms_p50"] < r["reprompt_wall_ms"]
    # the launches alone
    us = []
    for _ in range(args.reps):
        g.timing_enable(True)
        dec.shift(n_ctx, keep, discard, use_graph=False)
        rows = g.timing_read()
        g.timing_enable(False)
        assert len(rows) == n_layer and all("kq_kv_shift" in r[0] for r in rows), [r[0] for r in rows]
        us += [r[2] * 1e3 for r in rows]
    moved = n_ctx - discard - keep
    launch_bytes = moved * kvw * 2 * 4  # K and V cells of 2-byte elements, each read once and written once
    p50 = statistics.median(us)
    out = {"lib": os.path.relpath(g.LIB_PATH, ROOT), "model": "tinyllama-1.1b (synthetic weights)", "n_ctx": n_ctx, "keep": keep,
           "discard": discard, "kept_tokens": kept, "moved_cells": moved, "layers": n_layer, "rounds": rounds,
           "shift_below_reprompt_in_every_round": all(r["shift_below_reprompt"] for r in rounds),
           "kq_kv_shift_launch": {"us_p50": round(p50, 2), "us_min": round(min(us), 2), "layer_sum_us_p50": round(p50 * n_layer, 1),
                                  "workgroups": kvw // 32 + kvw, "k_workgroups": kvw // 32, "bytes": launch_bytes,
                                  "GBps_p50": round(launch_bytes / p50 / 1e3, 1),
                                  "share_of_hbm_peak": round(launch_bytes / p50 / 1e3 / HBM_PEAK_GBPS, 4)}}
    print(json.dumps(out))
    be.close()
    if not out["shift_below_reprompt_in_every_round"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
