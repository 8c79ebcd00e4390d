"""Prompt attention on the f16 matrix cores (mi355x_attn_prompt_precision F16: kq_kv_store +
kq_attn_prompt_f16) against the exact path (EXACT: kq_kv_store + kq_attn_prompt_group, or the streamed
kernels past 8192 cells), on one box in one session, rounds interleaved.

    python tools/attn_prompt_f16_bench.py [--ends 512,2048,4096,16384] [--models tinyllama-1.1b,llama-3-8b]
                                          [--rounds 5] [--reps 10] [--no-prompt]

Op level: one 512-token batch whose last token sits at cell `end - 1` of a cache of `end` cells (random
finite caches, N(0, 2) scores), mi355x_attn_prompt by event timing (mi355x_timing_enable): the sum of the
call's launches, per precision the median over the round's calls; ends past 8192 run under
mi355x_attn_stream(1). `f16_below_exact_every_round` is the issue's gate from 2048 cells up.
Whole prompt (unless --no-prompt): LlamaDecoder.prompt of 512 tokens from an empty cache on synthetic
weights of the real shapes (bench.py's Token), hipGraph replay, device events around --reps replays.
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ggml-neon-opt_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import ggml_mi355x as g  # noqa: E402

N_TOK = 512
PRECISIONS = (("exact", g.ATTN_PROMPT_EXACT), ("f16", g.ATTN_PROMPT_F16))


class OpCase:
    def __init__(self, model, end, dev):
        h = bench.HPARAMS[model]
        self.model, self.end = model, end
        self.nh, self.nkv = h["n_head"], h["n_head_kv"]
        self.hd = bench.MODELS[model]["E"] // self.nh
        kvw = self.nkv * self.hd
        gen = torch.Generator(device=dev)
        gen.manual_seed(end * 131 + self.hd)
        self.q = torch.randn((N_TOK, self.nh * self.hd), device=dev, generator=gen) * 2
        self.k = torch.randn((N_TOK, kvw), device=dev, generator=gen)
        self.v = torch.randn((N_TOK, kvw), device=dev, generator=gen)
        self.kc = torch.randn((end, kvw), device=dev, generator=gen).half().view(torch.int16)
        self.vc = torch.randn((kvw, end), device=dev, generator=gen).half().view(torch.int16)
        self.pos = torch.arange(end - N_TOK, end, dtype=torch.int32, device=dev)
        self.tab = g.rope_table(end, self.hd, h["freq_base"], 1.0, device=dev)
        self.out = torch.empty((N_TOK, self.nh * self.hd), device=dev)
        self.medians = {name: [] for name, _ in PRECISIONS}
        self.kernels = {}

    def run(self):
        g.attn_prompt(self.q, self.k, self.v, self.pos, self.tab, self.kc, self.vc, self.nh, self.nkv, self.hd,
                      1.0 / math.sqrt(self.hd), out=self.out)

    def timed(self, name, reps):
        g.timing_enable(True)
        for _ in range(reps):
            self.run()
        rows = g.timing_read()
        g.timing_enable(False)
        per = len(rows) // reps
        assert per * reps == len(rows) and per >= 2, (len(rows), reps)
        self.kernels[name] = sorted(set(r[0] for r in rows))
        self.medians[name].append(statistics.median(sum(r[2] for r in rows[i * per:(i + 1) * per]) * 1e3
                                                     for i in range(reps)))


def op_level(args, dev):
    cases = [OpCase(m, e, dev) for m in args.models for e in args.ends]
    g.attn_stream(1)  # only the caches past 8192 cells change their kernels
    for c in cases:  # warm-up, and the two precisions on the same inputs
        outs = {}
        for name, p in PRECISIONS:
            g.attn_prompt_precision(p)
            c.run()
            c.run()
            torch.cuda.synchronize()
            outs[name] = c.out.clone()
        c.max_diff = float((outs["f16"] - outs["exact"]).abs().max())
        assert math.isfinite(c.max_diff) and c.max_diff < 0.05, (c.model, c.end, c.max_diff)
    for _ in range(args.rounds):
        for c in cases:
            for name, p in PRECISIONS:
                g.attn_prompt_precision(p)
                c.timed(name, args.reps if c.end <= 8192 else max(2, args.reps // 4))
    g.attn_prompt_precision(g.ATTN_PROMPT_EXACT)
    g.attn_stream(0)
    out = {}
    for c in cases:
        ex, f = c.medians["exact"], c.medians["f16"]
        out["%s@%d" % (c.model, c.end)] = {
            "exact_us_rounds": [round(v, 1) for v in ex], "f16_us_rounds": [round(v, 1) for v in f],
            "exact_us": round(statistics.median(ex), 1), "f16_us": round(statistics.median(f), 1),
            "speedup": round(statistics.median(ex) / statistics.median(f), 2),
            "f16_below_exact_every_round": all(b < a for a, b in zip(ex, f)),
            "max_abs_diff": c.max_diff, "kernels": c.kernels}
    return out


def whole_prompt(args, dev):
    from ggml_mi355x.llama import LlamaDecoder
    out = {}
    for model in args.models:
        be = g.Backend(torch.cuda.current_device())
        tk = bench.Token(model, dev, 0x51A7, be, 128)
        toks = np.random.default_rng(0x5EED).integers(0, tk.hp["n_vocab"], size=N_TOK).tolist()
        decs, ms, logits = {}, {name: [] for name, _ in PRECISIONS}, {}
        for name, p in PRECISIONS:
            g.attn_prompt_precision(p)
            decs[name] = LlamaDecoder(be, tk.hp, tk.w, N_TOK)
            lg = decs[name].prompt(toks, 0)  # capture
            be.synchronize()
            logits[name] = lg.float().cpu().numpy().ravel().copy()
        st = torch.cuda.ExternalStream(be.stream)
        for _ in range(args.rounds):
            for name, p in PRECISIONS:
                g.attn_prompt_precision(p)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(args.reps):
                    decs[name].prompt(toks, 0)
                e1.record(st)
                be.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.reps)
        g.attn_prompt_precision(g.ATTN_PROMPT_EXACT)
        ex, f = statistics.median(ms["exact"]), statistics.median(ms["f16"])
        out[model] = {"exact_ms_rounds": [round(v, 3) for v in ms["exact"]], "f16_ms_rounds": [round(v, 3) for v in ms["f16"]],
                      "exact_ms": round(ex, 3), "f16_ms": round(f, 3), "exact_tok_s": round(N_TOK / ex * 1e3, 1),
                      "f16_tok_s": round(N_TOK / f * 1e3, 1), "speedup": round(ex / f, 3),
                      "logits_max_abs_diff": float(np.abs(logits["f16"] - logits["exact"]).max()),
                      "logits_max_abs": float(np.abs(logits["exact"]).max())}
        del decs, tk, be
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ends", default="512,2048,4096,16384")
    ap.add_argument("--models", default="tinyllama-1.1b,llama-3-8b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-prompt", action="store_true")
    args = ap.parse_args()
    args.ends = [int(v) for v in args.ends.split(",")]
    args.models = args.models.split(",")
    dev = torch.device("cuda:0")
    out = {"lib": os.path.relpath(g.LIB_PATH, ROOT), "tokens": N_TOK, "rounds": args.rounds, "reps": args.reps,
           "op": op_level(args, dev)}
    if not args.no_prompt:
        out["pp512"] = whole_prompt(args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
