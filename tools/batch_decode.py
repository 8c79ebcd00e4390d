"""Multi-sequence decode throughput: LlamaDecoder.step_batch (one graph of T tokens, one per
sequence, ATTN_BATCH nodes reading cells and mask from the inputs) against the same number of
tokens through step() one sequence at a time on separate decoders — TinyLlama width, bench.py's
synthetic Q4_K_M weights, hipGraph replay — and the kq_attn_batch launch beside
kq_attn_prompt_group on a causal single-sequence batch of the same T and n_kv.

    python tools/batch_decode.py [--cells 512,2048] [--seqs 1,2,4,8] [--steps 64] [--warmup 16] [--reps 3]
                                 [--form auto|head] [--attn-stream]

The caches are pre-filled with random finite f16 values up to `cells` cells per sequence; in the
batch decoder the sequences are interleaved (sequence s holds the cells c with c % n_seq == s).
A (cells, n_seq) pair whose cache (n_seq * (cells + steps), rounded up to 32) is larger than the
attention kernels take (7616 cells at head_dim 64) is reported as "not run", unless --attn-stream
sets mi355x_attn_stream mode 1: then such caches (up to 131072 cells) run on the streamed kernels,
on both sides where the size needs it, and the attention launch is also timed in its streamed form
(mode 2) at the sizes kq_attn_batch takes. Each figure is the
median of `reps` windows of `steps` steps after `warmup` steps, every window ending in a stream
synchronise. Prints one line per measurement and a JSON summary at the end."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402
from bench import Token  # noqa: E402
from ggml_mi355x.llama import LlamaDecoder  # noqa: E402

MAX_CTX = 7616  # check_attn: 6 hd + 6 n_ctx + 64 hd + 16 + 2 n_ctx <= 64 KB at head_dim 64


def fill(dec, gen):
    for c in dec.k_cache + dec.v_cache:
        c.copy_((torch.randn(c.shape, device=c.device, generator=gen) * 0.5).to(torch.float16).view(torch.int16))


def median_window(run, sync, steps, warmup, reps):
    for i in range(warmup):
        run(i)
    sync()
    out = []
    for r in range(reps):
        t0 = time.perf_counter()
        for i in range(steps):
            run(warmup + r * steps + i)
        sync()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)), out


def batch_side(tk, be, cells, n_seq, steps, warmup, reps, gen):
    total = warmup + reps * steps
    n_ctx = (n_seq * (cells + total) + 31) // 32 * 32
    if n_ctx > MAX_CTX:
        return None
    dec = LlamaDecoder(be, tk.hp, tk.w, n_ctx)
    fill(dec, gen)
    toks = np.random.default_rng(1).integers(0, tk.hp["n_vocab"], size=(total, n_seq))
    seq_of = np.arange(n_ctx) % n_seq
    form = g.attn_batch_path(n_ctx, tk.hp["n_head"], tk.hp["n_head_kv"], tk.hp["head_dim"], n_ctx)

    def run(i):
        p = cells + i  # every sequence is at position p; its token goes to cell p * n_seq + s
        cl = [p * n_seq + s for s in range(n_seq)]
        mask = np.where((seq_of[None, :] == np.arange(n_seq)[:, None]) & (np.arange(n_ctx)[None, :] < (p + 1) * n_seq),
                        np.float32(0.0), np.float32(-np.inf))
        dec.step_batch(toks[i].tolist(), [p] * n_seq, cl, mask, n_ctx)

    med, wins = median_window(run, be.synchronize, steps, warmup, reps)
    del dec
    torch.cuda.empty_cache()
    return dict(n_ctx=n_ctx, form={g.ATTN_GROUP: "group", g.ATTN_HEAD: "head", g.ATTN_PATH_STREAM: "stream"}[form],
                s_per_step=med / steps,
                tok_s=n_seq * steps / med, windows_s=wins)


def sequential_side(tk, be, cells, n_seq, steps, warmup, reps, gen):
    total = warmup + reps * steps
    n_ctx = (cells + total + 31) // 32 * 32
    decs = [LlamaDecoder(be, tk.hp, tk.w, n_ctx) for _ in range(n_seq)]
    for d in decs:
        fill(d, gen)
    toks = np.random.default_rng(1).integers(0, tk.hp["n_vocab"], size=(total, n_seq))

    def run(i):
        for s, d in enumerate(decs):
            d.step(int(toks[i, s]), cells + i)

    med, wins = median_window(run, be.synchronize, steps, warmup, reps)
    del decs
    torch.cuda.empty_cache()
    return dict(n_ctx=n_ctx, s_per_step=med / steps, tok_s=n_seq * steps / med, windows_s=wins)


def kernel_side(hp, dev, T, n_kv, reps, gen, stream=False):
    """The attention launch alone, op level: T tokens of one sequence at the last T cells of a
    cache of n_kv cells under the causal mask, through mi355x_attn_batch and mi355x_attn_prompt;
    stream: also mi355x_attn_batch in its streamed form (mode 2 for the one measurement)."""
    hd, nh, nkv = hp["head_dim"], hp["n_head"], hp["n_head_kv"]
    kvw = nkv * hd
    tab = g.rope_table(n_kv, hd, hp["freq_base"], 1.0, device=dev)
    q = torch.randn(T, nh * hd, device=dev, generator=gen)
    k = torch.randn(T, kvw, device=dev, generator=gen)
    v = torch.randn(T, kvw, device=dev, generator=gen)
    kc = (torch.randn(n_kv, kvw, device=dev, generator=gen) * 0.5).to(torch.float16).view(torch.int16)
    vc = (torch.randn(kvw, n_kv, device=dev, generator=gen) * 0.5).to(torch.float16).view(torch.int16)
    pos = torch.arange(n_kv - T, n_kv, dtype=torch.int32, device=dev)
    mask = torch.where(torch.arange(n_kv, device=dev)[None, :] <= pos[:, None], 0.0, float("-inf")).to(torch.float32)
    scale = 1.0 / float(hd) ** 0.5
    out = {}
    sides = [("batch", lambda: g.attn_batch(q, k, v, pos, pos, mask, tab, kc, vc, nh, nkv, hd, scale, n_kv)),
             ("prompt", lambda: g.attn_prompt(q, k, v, pos, tab, kc, vc, nh, nkv, hd, scale))]
    if stream:
        sides.append(("batch_stream", sides[0][1]))
    for name, fn in sides:
        prev = g.attn_stream(2) if name == "batch_stream" else None
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g.timing_enable(True)
        for _ in range(reps):
            fn()
        rows = g.timing_read()
        g.timing_enable(False)
        if prev is not None:
            g.attn_stream(prev)
        per = {}
        for kn, _, ms in rows:
            per.setdefault(kn, []).append(ms)
        out[name] = {kn: round(float(np.median(v_)) * 1e3, 2) for kn, v_ in per.items()}  # us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="512,2048")
    ap.add_argument("--seqs", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", default="tinyllama-1.1b")
    ap.add_argument("--form", default="auto", choices=["auto", "head"],
                    help="head: one attention workgroup per query head and token at every size (attn_prompt_impl)")
    ap.add_argument("--attn-stream", action="store_true",
                    help="mi355x_attn_stream mode 1: caches past the attention kernels' sizes run on the streamed kernels")
    args = ap.parse_args()
    if not g.device_available():
        raise SystemExit("batch_decode: no gfx950 device (the measurement does not fall back)")
    dev = torch.device("cuda:0")
    if args.attn_stream:
        global MAX_CTX
        MAX_CTX = 131072  # kAttnStreamMaxCtx
        g.attn_stream(1)
    if args.form == "head":
        g.attn_prompt_impl(g.ATTN_HEAD)
    be = g.Backend()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    tk = Token(args.model, dev, 0x51A7, be, 32)
    res = []
    for cells in [int(c) for c in args.cells.split(",")]:
        for n_seq in [int(s) for s in args.seqs.split(",")]:
            b = batch_side(tk, be, cells, n_seq, args.steps, args.warmup, args.reps, gen)
            s = sequential_side(tk, be, cells, n_seq, args.steps, args.warmup, args.reps, gen)
            row = dict(cells_per_seq=cells, n_seq=n_seq, batch=b, sequential=s)
            if b is not None:
                row["kernels_us"] = kernel_side(tk.hp, dev, n_seq, b["n_ctx"], 20, gen, args.attn_stream)
            res.append(row)
            bt = "not run (cache too large)" if b is None else \
                f"{b['tok_s']:8.1f} tok/s ({b['s_per_step'] * 1e3:.3f} ms/step, n_kv {b['n_ctx']}, {b['form']} form)"
            print(f"cells/seq {cells:5d} seqs {n_seq}: step_batch {bt} | sequential step() {s['tok_s']:8.1f} tok/s "
                  f"({s['s_per_step'] * 1e3:.3f} ms/step)" +
                  (f" | attention us {row['kernels_us']}" if b is not None else ""), flush=True)
    print(json.dumps(dict(model=args.model, steps=args.steps, warmup=args.warmup, reps=args.reps, results=res)))
    be.close()


if __name__ == "__main__":
    main()
