"""Greedy generation of several sequences on the device against the loops on the host, on one
box, interleaved: TinyLlama width, bench.py's synthetic Q4_K_M weights, hipGraph replay, 4 and 8
sequences of 2048 pre-filled cells each (random finite f16 values), 128 steps per window from
position 2048, wall time between two synchronizations. The sequences are interleaved in the
cache (sequence s holds the cells c with c % n_seq == s: cell_stride = n_seq).

  a  LlamaDecoder.generate_batch at every --chunks value (the ARGMAX_BATCH node stages the next
     step on the device; inputs staged once per window)
  b  the step_batch loop with tokens and masks known beforehand (the floor of a host-fed loop:
     step_batch still copies its input block, the mask included, every step)
  c  what a user writes without generate_batch: step_batch, synchronize, the logits to the host,
     numpy's argmax per row, the new cell shown in the host's mask, which step_batch copies again

    python tools/generate_batch_bench.py [--seqs 4,8] [--cells 2048] [--rounds 5] [--chunks 32,128]
                                         [--attn-stream]

--sampler adds the sampling leg to the same session (rounds interleaved with a, b, c):
  s  generate_batch(sampler=Sampler()) at every --chunks value (the SAMPLE_BATCH node; llama.cpp's
     default chain)
  h  (c) with sampled tokens: per row the rule of tests/sample_ref.py on the candidates of a numpy
     argpartition top-k (numpy's exp in place of the rule's v_expf, which only makes the loop faster)

A cache (n_seq * (cells + steps), rounded up to 32) larger than the attention kernels take (7616
cells at head_dim 64) is reported as "not run" unless --attn-stream sets mi355x_attn_stream mode 1.
Also times the kq_argmax_rows launch alone (event timing, the matrix written by the launch just
before) at 8 x 32000 and 8 x 128256, beside kq_argmax on one such row. Prints one line per
measurement and a JSON summary at the end."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402
from bench import Token  # noqa: E402
from ggml_mi355x.llama import LlamaDecoder, Sampler  # noqa: E402

MAX_CTX = 7616  # check_attn: 6 hd + 6 n_ctx + 64 hd + 16 + 2 n_ctx <= 64 KB at head_dim 64
STEPS = 128


def start_inputs(n_seq, cells, n_ctx):
    """Every sequence at position `cells`: its token goes to cell cells * n_seq + s; row s shows the
    sequence's cells up to that one, every later cell is hidden in every row."""
    c = np.arange(n_ctx)
    mask = np.where((c[None, :] % n_seq == np.arange(n_seq)[:, None]) & (c[None, :] < (cells + 1) * n_seq),
                    np.float32(0.0), np.float32(-np.inf))
    return [cells] * n_seq, [cells * n_seq + s for s in range(n_seq)], mask


def timed(be, fn):
    be.synchronize()
    t0 = time.perf_counter()
    fn()
    be.synchronize()
    return (time.perf_counter() - t0) * 1e3 / STEPS


def rows_argmax(lg):
    return np.argmax(np.where(np.isnan(lg), -np.inf, lg), axis=1)


def measure(tk, be, n_seq, cells, rounds, chunks, gen, sampler=None):
    n_ctx = (n_seq * (cells + STEPS) + 31) // 32 * 32
    if n_ctx > MAX_CTX:
        return None
    dec = LlamaDecoder(be, tk.hp, tk.w, n_ctx)
    for c in dec.k_cache + dec.v_cache:
        c.copy_((torch.randn(c.shape, device=c.device, generator=gen) * 0.5).to(torch.float16).view(torch.int16))
    torch.cuda.synchronize()
    pos0, cells0, mask0 = start_inputs(n_seq, cells, n_ctx)
    tok0 = list(range(1, n_seq + 1))
    known = np.random.default_rng(1).integers(0, tk.hp["n_vocab"], size=(STEPS, n_seq))
    known_masks = []  # (b): every step's mask built beforehand
    m = mask0.copy()
    for i in range(STEPS):
        known_masks.append(m.copy())
        for s in range(n_seq):
            if cells0[s] + (i + 1) * n_seq < n_ctx:
                m[s, cells0[s] + (i + 1) * n_seq] = 0.0

    def run_a(chunk):
        return timed(be, lambda: dec.generate_batch(tok0, pos0, cells0, mask0, STEPS, n_ctx, cell_stride=n_seq, chunk=chunk))

    def run_b():
        def body():
            for i in range(STEPS):
                dec.step_batch(known[i].tolist(), [cells + i] * n_seq, [c + i * n_seq for c in cells0], known_masks[i],
                               n_ctx)
        return timed(be, body)

    def run_c():
        def body():
            tok, pos, cl, mask = list(tok0), list(pos0), list(cells0), mask0.copy()
            for _ in range(STEPS):
                lg = dec.step_batch(tok, pos, cl, mask, n_ctx)
                be.synchronize()
                tok = rows_argmax(lg.cpu().numpy()).tolist()
                for s in range(n_seq):
                    pos[s] += 1
                    cl[s] += n_seq
                    if cl[s] < n_ctx:
                        mask[s, cl[s]] = 0.0
        return timed(be, body)

    def run_s(chunk):
        return timed(be, lambda: dec.generate_batch(tok0, pos0, cells0, mask0, STEPS, n_ctx, cell_stride=n_seq, chunk=chunk,
                                                    sampler=sampler))

    def run_h():
        from generate_bench import host_topk
        from tests import sample_ref as R
        draws = [sampler.draws(n_ctx + 1, s) for s in range(n_seq)]

        def body():
            tok, pos, cl, mask = list(tok0), list(pos0), list(cells0), mask0.copy()
            for _ in range(STEPS):
                lg = dec.step_batch(tok, pos, cl, mask, n_ctx)
                be.synchronize()
                lg = lg.cpu().numpy()
                for s in range(n_seq):
                    tok[s] = R.chain(lg[s], host_topk(lg[s], sampler.top_k), draws[s][pos[s] + 1], sampler.top_p,
                                     sampler.min_p, sampler.temp, expf=np.exp)["token"]
                    pos[s] += 1
                    cl[s] += n_seq
                    if cl[s] < n_ctx:
                        mask[s, cl[s]] = 0.0
        return timed(be, body)

    fns = {f"a_chunk{c}": (lambda c=c: run_a(c)) for c in chunks}
    fns.update(b=run_b, c=run_c)
    if sampler is not None:
        fns.update({f"s_chunk{c}": (lambda c=c: run_s(c)) for c in chunks})
        fns["h"] = run_h
    for fn in fns.values():  # capture + warm
        fn()
    res = {v: [] for v in fns}
    for _ in range(rounds):
        for v, fn in fns.items():
            res[v].append(fn())
    # the device's tokens against the host loop's, once (exact: the same graph feeds both)
    got = dec.generate_batch(tok0, pos0, cells0, mask0, 8, n_ctx, cell_stride=n_seq)
    tok, pos, cl, mask, ref = list(tok0), list(pos0), list(cells0), mask0.copy(), [[] for _ in range(n_seq)]
    for _ in range(8):
        lg = dec.step_batch(tok, pos, cl, mask, n_ctx)
        be.synchronize()
        tok = rows_argmax(lg.cpu().numpy()).tolist()
        for s in range(n_seq):
            ref[s].append(tok[s])
            pos[s] += 1
            cl[s] += n_seq
            mask[s, cl[s]] = 0.0
    form = g.attn_batch_path(n_ctx, tk.hp["n_head"], tk.hp["n_head_kv"], tk.hp["head_dim"], n_ctx)
    del dec
    torch.cuda.empty_cache()
    med = {v: statistics.median(x) for v, x in res.items()}
    return dict(n_seq=n_seq, cells_per_seq=cells, n_kv=n_ctx,
                form={g.ATTN_GROUP: "group", g.ATTN_HEAD: "head", g.ATTN_PATH_STREAM: "stream"}.get(form, str(form)),
                input_block_bytes=4 * (3 * n_seq + n_seq * n_ctx), logits_bytes=4 * n_seq * tk.hp["n_vocab"],
                tokens_equal_host_loop=bool(got == ref),
                ms_per_step={v: [round(x, 4) for x in r] for v, r in res.items()},
                median_ms_per_step={v: round(x, 4) for v, x in med.items()},
                tok_s={v: round(n_seq * 1e3 / x, 1) for v, x in med.items()},
                spread_b_ms=round(max(res["b"]) - min(res["b"]), 4))


def argmax_rows_launch_us(dev, n, rows, reps=200):
    """Median event time of the kq_argmax_rows launch over [rows, n] and of kq_argmax over one such
    row; an elementwise launch writes the matrix just before."""
    a = torch.randn(rows * n, device=dev)
    b = torch.randn(rows * n, device=dev)
    x = torch.empty(rows * n, device=dev)
    ws = torch.zeros(g.argmax_rows_workspace_size(n, rows), dtype=torch.uint8, device=dev)
    ws1 = torch.zeros(g.argmax_workspace_size(n), dtype=torch.uint8, device=dev)
    out = torch.zeros(rows, dtype=torch.int32, device=dev)
    out1 = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("kq_argmax_rows", lambda: g.argmax_rows(x.view(rows, n), out=out, workspace=ws)),
                     ("kq_argmax", lambda: g.argmax(x[:n], out=out1, workspace=ws1))):
        for _ in range(10):
            g.add(a, b, out=x)
            fn()
        torch.cuda.synchronize()
        g.timing_enable(True)
        for _ in range(reps):
            g.add(a, b, out=x)
            fn()
        rows_t = g.timing_read()
        g.timing_enable(False)
        ms = [r[2] for r in rows_t if "argmax" in r[0]]
        assert len(ms) == reps
        res[name] = {"us_p50": round(statistics.median(ms) * 1e3, 2), "us_min": round(min(ms) * 1e3, 2)}
    want = torch.argmax(x.view(rows, n), dim=1).cpu()
    assert (out.cpu() == want).all() and int(out1.cpu()[0]) == int(want[0])
    res["workgroups_per_row"] = g.argmax_plan(n)[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="4,8")
    ap.add_argument("--cells", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", default="32,128")
    ap.add_argument("--model", default="tinyllama-1.1b")
    ap.add_argument("--sampler", action="store_true", help="add the sampling leg (s, h)")
    ap.add_argument("--attn-stream", action="store_true",
                    help="mi355x_attn_stream mode 1: caches past the attention kernels' sizes run on the streamed kernels")
    args = ap.parse_args()
    if not g.device_available():
        raise SystemExit("generate_batch_bench: no gfx950 device (the measurement does not fall back)")
    dev = torch.device("cuda:0")
    if args.attn_stream:
        global MAX_CTX
        MAX_CTX = 131072  # kAttnStreamMaxCtx
        g.attn_stream(1)
    be = g.Backend()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    tk = Token(args.model, dev, 0x51A7, be, 32)
    chunks = [int(c) for c in args.chunks.split(",")]
    res = []
    for n_seq in [int(s) for s in args.seqs.split(",")]:
        r = measure(tk, be, n_seq, args.cells, args.rounds, chunks, gen, Sampler(seed=1) if args.sampler else None)
        res.append(r if r is not None else dict(n_seq=n_seq, cells_per_seq=args.cells, not_run="cache too large"))
        if r is None:
            print(f"seqs {n_seq} cells/seq {args.cells}: not run (cache too large; --attn-stream)", flush=True)
            continue
        m = r["median_ms_per_step"]
        print(f"seqs {n_seq} cells/seq {args.cells} n_kv {r['n_kv']} ({r['form']} form): " +
              " | ".join(f"{v} {m[v]:.3f} ms/step {r['tok_s'][v]:.0f} tok/s" for v in m) +
              f" | spread of b {r['spread_b_ms']:.3f} ms | tokens equal the host loop's: {r['tokens_equal_host_loop']}",
              flush=True)
    launch = {f"{rows}x{n}": argmax_rows_launch_us(dev, n, rows) for rows, n in ((8, 32000), (8, 128256))}
    for k, v in launch.items():
        print(f"launch alone {k}: kq_argmax_rows {v['kq_argmax_rows']['us_p50']} us (min {v['kq_argmax_rows']['us_min']}), "
              f"kq_argmax on one row {v['kq_argmax']['us_p50']} us (min {v['kq_argmax']['us_min']}), "
              f"{v['workgroups_per_row']} workgroups per row", flush=True)
    print(json.dumps(dict(model=args.model, steps=STEPS, rounds=args.rounds, lib=os.path.relpath(g.LIB_PATH, ROOT),
                          results=res, launch_us=launch)))
    be.close()


if __name__ == "__main__":
    main()
