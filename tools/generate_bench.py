"""Greedy generation on the device against the loops on the host, on one box, interleaved: the
bench's TinyLlama-1.1B Q4_K_M decode token (synthetic weights of the real shapes), 128 tokens
after 8 warm-up tokens from an empty cache, wall time between two synchronizations.

  a  step loop with tokens known beforehand (bench.py's headline path)
  b  LlamaDecoder.generate (the ARGMAX node stages the next token on the device)
  c  what a user wrote before generate: step, synchronize, logits to the host, numpy argmax

Prints one JSON line: ms per token of every round, the run-to-run spread of (a) (max - min over
the rounds), the gate (median c - median b > that spread), b against a, and kq_argmax's own
launch time (event timing, the vector written by the launch just before) at 32000 and 128256
entries for every --slices value (ARGMAX_SLICE; 0: the library's default).

    python tools/generate_bench.py [--rounds 5] [--variants a,b,c] [--chunk 32]
                                   [--slices 0,512,1024,2048,4096]

`in_token_us`: the launches of one eager generated token by event timing (kq_argmax behind the
head GEMV that wrote its logits, and the whole token's launches summed).

With an older library under MI355X_LIB only --variants a runs (no generate in it).

--sampler: the sampling leg instead, three timings in one session, rounds interleaved:
  b  LlamaDecoder.generate, greedy
  s  LlamaDecoder.generate(sampler=Sampler()) (llama.cpp's default chain; the SAMPLE node)
  h  the loop a user writes for sampled tokens: step, synchronize, logits to the host, the rule of
     tests/sample_ref.py on the candidates of a numpy argpartition top-k (numpy's exp in place of
     the rule's v_expf, which only makes the host loop faster)
and kq_topk's own launch time (event timing, behind the launch that wrote the vector) at 32000 and
128256 entries for the plain top-k (k 40) and the sampled token, next to kq_argmax on the same
vector in the same run. Under a KQ_SAMPLE_DIAG variant library (make variant-sample) the same
launch stops early, which splits its time: 1: no merge on the last arriver, 2: no sampling tail.

--penalties: the penalties' leg, three timings in one session, rounds interleaved:
  s  LlamaDecoder.generate(sampler=Sampler()): no edits, the node list without PENALIZE
  p  the same with repeat_penalty 1.1 over the last 64 tokens (a PENALIZE node before the SAMPLE node)
  h  the host-sampling loop of --sampler with the penalties' rule in numpy float32 before the top-k
and kq_penalize_rows' own launch time (event timing, behind the launch that wrote the logits) at
last_n 64 / 256 / 1024 and n_bias 0 / 256 for 1 x 32000, 1 x 128256 and 8 x 128256 logits (every
window entry another token: the most owners), next to kq_topk on the same vector sizes in the same run.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ggml-neon-opt_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import ggml_mi355x as g  # noqa: E402

WARM, STEPS = 8, 128


def timed(be, fn):
    be.synchronize()
    t0 = time.perf_counter()
    fn()
    be.synchronize()
    return (time.perf_counter() - t0) * 1e3 / STEPS


def run_a(tk, be):
    tk.dec.reset()
    torch.cuda.synchronize()
    for i in range(WARM):
        tk.dec.step(tk.tokens[i], i)

    def body():
        for i in range(WARM, WARM + STEPS):
            tk.dec.step(tk.tokens[i], i)
    return timed(be, body)


def run_b(tk, be, chunk=32):
    tk.dec.reset()
    torch.cuda.synchronize()
    tok = tk.dec.generate(tk.tokens[0], 0, WARM)[-1]
    return timed(be, lambda: tk.dec.generate(tok, WARM, STEPS, chunk=chunk))


def host_loop(tk, be, tok, pos, n):
    for p in range(pos, pos + n):
        tk.dec.step(tok, p)
        be.synchronize()
        x = tk.dec.logits.cpu().numpy()
        tok = int(np.argmax(np.where(np.isnan(x), -np.inf, x)))
    return tok


def run_c(tk, be):
    tk.dec.reset()
    torch.cuda.synchronize()
    tok = host_loop(tk, be, tk.tokens[0], 0, WARM)
    return timed(be, lambda: host_loop(tk, be, tok, WARM, STEPS))


def in_token_us(tk, be, reps=20):
    """Event times of one eager generated token's launches: kq_argmax's median and the token's sum."""
    tk.dec.reset()
    torch.cuda.synchronize()
    tk.dec.generate(tk.tokens[0], 0, 2, use_graph=False)
    am, tot = [], []
    for i in range(reps):
        g.timing_enable(True)
        tk.dec.generate(tk.tokens[i], 2 + i, 1, use_graph=False)
        rows = g.timing_read()
        g.timing_enable(False)
        am += [r[2] for r in rows if "argmax" in r[0]]
        tot.append(sum(r[2] for r in rows))
    return {"kq_argmax_p50": round(statistics.median(am) * 1e3, 2), "launches_sum_p50": round(statistics.median(tot) * 1e3, 1)}


def argmax_launch_us(dev, n, slice_, reps=200):
    """Median event time of the kq_argmax launch; an elementwise launch writes x just before."""
    prev = g.debug_knob("ARGMAX_SLICE", slice_)
    try:
        a = torch.randn(n, device=dev)
        b = torch.randn(n, device=dev)
        x = torch.empty(n, device=dev)
        ws = torch.zeros(g.argmax_workspace_size(n), dtype=torch.uint8, device=dev)
        out = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for _ in range(10):
            g.add(a, b, out=x)
            g.argmax(x, out=out, workspace=ws)
        torch.cuda.synchronize()
        g.timing_enable(True)
        for _ in range(reps):
            g.add(a, b, out=x)
            g.argmax(x, out=out, workspace=ws)
        rows = g.timing_read()
        g.timing_enable(False)
        ms = [r[2] for r in rows if "argmax" in r[0]]
        assert len(ms) == reps and int(out.cpu()[0]) == int(torch.argmax(x).cpu())
        return {"slice": g.argmax_plan(n)[1], "workgroups": g.argmax_plan(n)[0],
                "us_p50": round(statistics.median(ms) * 1e3, 2), "us_min": round(min(ms) * 1e3, 2)}
    finally:
        g.debug_knob("ARGMAX_SLICE", prev if prev else float("nan"))


def host_topk(x, k):
    """The k largest entries by numpy's argpartition, sorted by (-value, index): ref_topk's
    candidates on finite logits, which is all the timed loop meets. Not the rule in general: a NaN
    counts as -inf here (the rule never takes one), and a k-th value of -inf takes every entry."""
    x = np.where(np.isnan(x), -np.inf, x)
    k = min(k, x.size)
    part = np.argpartition(-x, k - 1)[:k]
    kth = x[part].min()
    cand = np.flatnonzero(x >= kth)  # (ties at the k-th value: all of them, the smallest indices win)
    return cand[np.lexsort((cand, -x[cand]))][:k]


def host_sample_loop(tk, be, tok, pos, n, sp, draws):
    from tests import sample_ref as R
    for p in range(pos, pos + n):
        tk.dec.step(tok, p)
        be.synchronize()
        x = tk.dec.logits.cpu().numpy()
        tok = R.chain(x, host_topk(x, sp.top_k), draws[p + 1], sp.top_p, sp.min_p, sp.temp, expf=np.exp)["token"]
    return tok


def topk_launch_us(dev, n, reps=200):
    """Median event times of kq_argmax, kq_topk (k 40) and the sampled token's kq_topk on one vector
    that an elementwise launch writes just before."""
    a, b, x = torch.randn(n, device=dev) * 4, torch.randn(n, device=dev) * 4, torch.empty(n, device=dev)
    ws1 = torch.zeros(g.argmax_workspace_size(n), dtype=torch.uint8, device=dev)
    ws = torch.zeros(g.topk_workspace_size(n), dtype=torch.uint8, device=dev)
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    u = torch.full((1,), 0.37, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    res = {"workgroups": g.argmax_plan(n)[0]}
    for name, fn in (("kq_argmax", lambda: g.argmax(x, out=out, workspace=ws1)),
                     ("kq_topk_k40", lambda: g.topk(x, 40, workspace=ws)),
                     ("kq_topk_sample", lambda: g.sample(x, u, out=out, workspace=ws))):
        for _ in range(10):
            g.add(a, b, out=x)
            fn()
        torch.cuda.synchronize()
        g.timing_enable(True)
        for _ in range(reps):
            g.add(a, b, out=x)
            fn()
        rows = g.timing_read()
        g.timing_enable(False)
        ms = [r[2] for r in rows if "argmax" in r[0] or "topk" in r[0]]
        assert len(ms) == reps
        res[name] = {"us_p50": round(statistics.median(ms) * 1e3, 2), "us_min": round(min(ms) * 1e3, 2)}
    return res


def sampler_leg(args, dev, be, tk):
    from ggml_mi355x.llama import Sampler
    sp = Sampler(seed=1)
    draws = sp.draws(tk.dec.n_ctx + 1)

    def run_s(t, b):
        t.dec.reset()
        torch.cuda.synchronize()
        tok = t.dec.generate(t.tokens[0], 0, WARM, sampler=sp)[-1]
        return timed(b, lambda: t.dec.generate(tok, WARM, STEPS, chunk=args.chunk, sampler=sp))

    def run_h(t, b):
        t.dec.reset()
        torch.cuda.synchronize()
        tok = host_sample_loop(t, b, t.tokens[0], 0, WARM, sp, draws)
        return timed(b, lambda: host_sample_loop(t, b, tok, WARM, STEPS, sp, draws))

    fns = {"b": lambda t, b: run_b(t, b, args.chunk), "s": run_s, "h": run_h}
    for fn in fns.values():  # capture + warm
        fn(tk, be)
    res = {v: [] for v in fns}
    for _ in range(args.rounds):
        for v, fn in fns.items():
            res[v].append(fn(tk, be))
    med = {v: statistics.median(x) for v, x in res.items()}
    out = {"model": "tinyllama-1.1b", "leg": "sampler", "tokens": STEPS, "warmup": WARM, "rounds": args.rounds,
           "chunk": args.chunk, "lib": os.path.relpath(g.LIB_PATH, ROOT),
           "sampler": dict(top_k=sp.top_k, top_p=sp.top_p, min_p=sp.min_p, temp=sp.temp),
           "ms_per_token": {v: [round(x, 4) for x in r] for v, r in res.items()},
           "median_ms_per_token": {v: round(m, 4) for v, m in med.items()},
           "h_minus_s_ms": round(med["h"] - med["s"], 4), "s_minus_b_ms": round(med["s"] - med["b"], 4),
           "sampled_generate_below_host_loop_in_every_round": bool(max(res["s"]) < min(res["h"])),
           "launch_us": {str(n): topk_launch_us(dev, n) for n in (32000, 128256)}}
    print(json.dumps(out))


def host_penalize(x, win, sp):
    """mi355x_penalize_rows' rule without a bias list on one row, in place, vectorized over the
    window's distinct tokens (float32, one rounding per operation)."""
    F = np.float32
    w = np.asarray(win, dtype=np.int64)
    t, c = np.unique(w[(w >= 0) & (w < x.size)], return_counts=True)
    v = x[t]
    v = np.where(v <= 0, v * F(sp.repeat_penalty), v / F(sp.repeat_penalty))
    x[t] = v - (c.astype(F) * F(sp.freq_penalty) + F(sp.presence_penalty))
    return x


def host_penalized_loop(tk, be, tok, pos, n, sp, draws, hist):
    from tests import sample_ref as R
    for p in range(pos, pos + n):
        tk.dec.step(tok, p)
        be.synchronize()
        hist[p] = tok
        x = host_penalize(tk.dec.logits.cpu().numpy(), hist[max(0, p - sp.repeat_last_n + 1):p + 1], sp)
        tok = R.chain(x, host_topk(x, sp.top_k), draws[p + 1], sp.top_p, sp.min_p, sp.temp, expf=np.exp)["token"]
    return tok


def penalize_launch_us(dev, n, rows, last_n, n_bias, reps=200):
    """Median event time of the kq_penalize_rows launch on [rows, n] logits that an elementwise
    launch writes just before; every window entry and every list entry names another token."""
    gen = torch.Generator().manual_seed(n + rows + last_n + n_bias)
    a, b = torch.randn((rows, n), device=dev) * 4, torch.randn((rows, n), device=dev) * 4
    x = torch.empty((rows, n), device=dev)
    n_hist = 2048
    hist = torch.stack([torch.randperm(n, generator=gen)[:n_hist] for _ in range(rows)]).to(torch.int32).to(dev)
    end = torch.full((rows,), n_hist - 1, dtype=torch.int32, device=dev)
    bias = None
    if n_bias:
        bias = (torch.randperm(n, generator=gen)[:n_bias].to(torch.int32).to(dev), torch.randn(n_bias, device=dev))
    torch.cuda.synchronize()

    def fn():
        g.add(a.view(-1), b.view(-1), out=x.view(-1))
        g.penalize_rows(x, hist, end, last_n=last_n, repeat=1.1, bias=bias)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    g.timing_enable(True)
    for _ in range(reps):
        fn()
    rows_ = g.timing_read()
    g.timing_enable(False)
    ms = [r[2] for r in rows_ if "penalize" in r[0]]
    assert len(ms) == reps
    return {"us_p50": round(statistics.median(ms) * 1e3, 2), "us_min": round(min(ms) * 1e3, 2)}


def penalties_leg(args, dev, be, tk):
    from ggml_mi355x.llama import Sampler
    s0, sp = Sampler(seed=1), Sampler(seed=1, repeat_penalty=1.1, repeat_last_n=64)
    assert not s0.edits() and sp.edits()
    draws = sp.draws(tk.dec.n_ctx + 1)

    def run_gen(t, b, s):
        t.dec.reset()
        torch.cuda.synchronize()
        toks = t.dec.generate(t.tokens[0], 0, WARM, sampler=s)
        return timed(b, lambda: t.dec.generate(toks[-1], WARM, STEPS, chunk=args.chunk, sampler=s,
                                               context=[t.tokens[0]] + toks[:-1]))

    def run_h(t, b):
        t.dec.reset()
        torch.cuda.synchronize()
        hist = [-1] * (t.dec.n_ctx + 1)
        tok = host_penalized_loop(t, b, t.tokens[0], 0, WARM, sp, draws, hist)
        return timed(b, lambda: host_penalized_loop(t, b, tok, WARM, STEPS, sp, draws, hist))

    fns = {"s": lambda t, b: run_gen(t, b, s0), "p": lambda t, b: run_gen(t, b, sp), "h": run_h}
    for fn in fns.values():  # capture + warm
        fn(tk, be)
    res = {v: [] for v in fns}
    for _ in range(args.rounds):
        for v, fn in fns.items():
            res[v].append(fn(tk, be))
    med = {v: statistics.median(x) for v, x in res.items()}
    launch = {}
    for rows, n in ((1, 32000), (1, 128256), (8, 128256)):
        launch[f"{rows}x{n}"] = {f"last_n{ln}_bias{nb}": penalize_launch_us(dev, n, rows, ln, nb)
                                 for ln in (64, 256, 1024) for nb in (0, 256)}
    out = {"model": "tinyllama-1.1b", "leg": "penalties", "tokens": STEPS, "warmup": WARM, "rounds": args.rounds,
           "chunk": args.chunk, "lib": os.path.relpath(g.LIB_PATH, ROOT),
           "penalties": dict(repeat_penalty=sp.repeat_penalty, repeat_last_n=sp.repeat_last_n),
           "ms_per_token": {v: [round(x, 4) for x in r] for v, r in res.items()},
           "median_ms_per_token": {v: round(m, 4) for v, m in med.items()},
           "p_minus_s_ms": round(med["p"] - med["s"], 4), "h_minus_p_ms": round(med["h"] - med["p"], 4),
           "penalised_generate_below_host_loop_in_every_round": bool(max(res["p"]) < min(res["h"])),
           "kq_penalize_rows_us": launch,
           "kq_topk_us": {str(n): topk_launch_us(dev, n) for n in (32000, 128256)}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="a,b,c")
    ap.add_argument("--slices", default="0,512,1024,2048,4096")
    ap.add_argument("--chunk", type=int, default=32, help="generate's steps between two synchronizations")
    ap.add_argument("--sampler", action="store_true", help="the sampling leg: generate greedy / sampled / the host loop")
    ap.add_argument("--launch-only", action="store_true", help="with --sampler: only the launches alone (diag variants)")
    ap.add_argument("--penalties", action="store_true", help="the penalties' leg: sampled generate without / with, the host loop")
    args = ap.parse_args()
    variants = args.variants.split(",")
    dev = torch.device("cuda:0")
    if args.sampler and args.launch_only:
        print(json.dumps({"lib": os.path.relpath(g.LIB_PATH, ROOT),
                          "launch_us": {str(n): topk_launch_us(dev, n) for n in (32000, 128256)}}))
        return
    be = g.Backend(0)
    tk = bench.Token("tinyllama-1.1b", dev, 0x51A7, be, 160)
    if args.sampler or args.penalties:
        (sampler_leg if args.sampler else penalties_leg)(args, dev, be, tk)
        be.close()
        return
    fns = {"a": run_a, "b": lambda t, b: run_b(t, b, args.chunk), "c": run_c}
    for v in variants:  # capture + warm
        fns[v](tk, be)
    res = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            res[v].append(fns[v](tk, be))
    med = {v: statistics.median(x) for v, x in res.items()}
    out = {"model": "tinyllama-1.1b", "tokens": STEPS, "warmup": WARM, "rounds": args.rounds, "chunk": args.chunk,
           "lib": os.path.relpath(g.LIB_PATH, ROOT),
           "ms_per_token": {v: [round(x, 4) for x in r] for v, r in res.items()},
           "median_ms_per_token": {v: round(m, 4) for v, m in med.items()}}
    if "a" in res:
        out["spread_a_ms"] = round(max(res["a"]) - min(res["a"]), 4)
    if all(v in res for v in "abc"):
        out["c_minus_b_ms"] = round(med["c"] - med["b"], 4)
        out["b_minus_a_ms"] = round(med["b"] - med["a"], 4)
        out["gate_b_faster_than_c_by_more_than_spread_a"] = bool(med["c"] - med["b"] > out["spread_a_ms"])
    if "b" in res:
        out["in_token_us"] = in_token_us(tk, be)
    if "b" in res and args.slices:
        out["kq_argmax_us"] = {str(n): [argmax_launch_us(dev, n, int(s)) for s in args.slices.split(",")]
                               for n in (32000, 128256)}
    print(json.dumps(out))
    be.close()


if __name__ == "__main__":
    main()
