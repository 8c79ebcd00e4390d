"""Perplexity of a llama model over a text of token ids, llama-perplexity's procedure [U] with the
log-probabilities taken on the device (LlamaDecoder.perplexity: 24 bytes a token come back).

    python tools/perplexity.py MODEL TOKENS.npy [--ctx 512] [--batch 512] [--bos ID] [--chunks N]
                               [--host] [--compare ROUNDS]

MODEL: a llama-architecture GGUF file (Q4_K / Q5_K / Q6_K matrices, read with the project's
reader), or the name of a bench model (bench.py's synthetic weights of the real shapes, e.g.
tinyllama-1.1b). TOKENS.npy: the text as token ids (there is no tokenizer in this project).
Prints the running estimate after each chunk in llama-perplexity's `[i]ppl` style, then the final
figure, the share of scored tokens that were the model's first choice, and tokens/s.

--host: the same graph, but every batch's logits (n_tok x n_vocab floats) copied to the host and
the rule of include/ggml_mi355x.h applied there in numpy (numpy's exp in place of the rule's
v_expf, which only makes the host path faster): what a user had to write before.
--compare R: both ways on the same text in one session, R rounds interleaved after one warm-up
pass each; one JSON line with the seconds of every round."""
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

import ggml_mi355x as g  # noqa: E402
from ggml_mi355x.llama import MOE_ROUTER, LlamaDecoder, gguf_hparams, layer_mats, ppl_of  # noqa: E402

KQUANTS = (g.TYPE_Q4_K, g.TYPE_Q5_K, g.TYPE_Q6_K)


def load_gguf(path, dev):
    """(hparams, LlamaDecoder's weights dict on the device) of a llama-architecture GGUF file."""
    from ggml_mi355x.gguf import GGUFFile
    with GGUFFile(path) as f:
        hp = gguf_hparams(f)  # (llama.expert_count > 0: a MoE model, its layers' FFN the expert tensors)
        if hp is None:
            raise SystemExit(f"{path}: not a llama-architecture model file")
        L = hp["n_layer"]

        def mat(name, table=False):
            t = f.tensors[name]["type"]
            if t == g.TYPE_F32 and table:
                return t, f.to_device(name, dev).view(torch.float32)
            if t not in KQUANTS:
                raise SystemExit(f"{path}: {name} has ggml type {t}; the matrices must be Q4_K, Q5_K or Q6_K")
            return t, f.to_device(name, dev)

        def vec(name):
            return f.to_device(name, dev).view(torch.float32).reshape(-1)

        w = {"token_embd": mat("token_embd.weight", table=True), "output_norm": vec("output_norm.weight")}
        w["output"] = mat("output.weight" if "output.weight" in f.tensors else "token_embd.weight")  # (tied embeddings)
        for i in range(L):
            for m in layer_mats(hp):
                w[f"blk.{i}.{m}"] = mat(f"blk.{i}.{m}.weight")
            if hp.get("n_expert", 0):  # the router, f32 [n_expert, n_embd]
                w[f"blk.{i}.{MOE_ROUTER}"] = vec(f"blk.{i}.{MOE_ROUTER}.weight").view(hp["n_expert"], hp["n_embd"])
            for n in ("attn_norm", "ffn_norm"):
                w[f"blk.{i}.{n}"] = vec(f"blk.{i}.{n}.weight")
        torch.cuda.synchronize()
        return hp, w


def host_records(x, targets):
    """The rule on logits x [T, V] (V % 4 == 0) in numpy, numpy's exp for v_expf: records [T]."""
    T, V = x.shape
    a = np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1)
    m = x[np.arange(T), a]
    with np.errstate(all="ignore"):
        d = x - m[:, None]
        e = np.where(np.isneginf(d), np.float32(0.0), np.exp(d)).astype(np.float32)
        q = (e[:, 0::4] + e[:, 1::4]) + (e[:, 2::4] + e[:, 3::4])
        leaves = 1
        while leaves < q.shape[1]:
            leaves *= 2
        t = np.zeros((T, leaves), np.float64)  # (the tree over fewer leaves: absent ones add +0.0 exactly)
        t[:, :q.shape[1]] = q
        while t.shape[1] > 1:
            t = t[:, 0::2] + t[:, 1::2]
    rec = np.zeros(T, g.logprob_dtype())
    tg = np.asarray(targets, dtype=np.int64)
    inside = (tg >= 0) & (tg < V)
    rec["max"], rec["argmax"], rec["sum"] = m, a, t[:, 0]
    rec["x_target"] = np.where(inside, x[np.arange(T), np.where(inside, tg, 0)], np.float32(np.nan))
    return rec


def host_perplexity(dec, be, tokens, n_ctx, n_batch, bos=None, progress=None):
    """LlamaDecoder.perplexity's loop with the logits copied out and host_records on them."""
    first, nll, count, hits = n_ctx // 2, 0.0, 0, 0
    n_chunk = len(tokens) // n_ctx
    for c in range(n_chunk):
        chunk = [int(t) for t in tokens[c * n_ctx:(c + 1) * n_ctx]]
        tg = chunk[1:] + [-1]
        if bos is not None:
            chunk[0] = bos
        for j in range(0, n_ctx, n_batch):
            part = chunk[j:j + n_batch]
            dec.logprobs(part, start_pos=j, targets=tg[j:j + n_batch], records=True)  # runs the graph, synchronizes
            x = dec._prompt_graph(len(part), all_rows=True)["logits"].cpu().numpy()
            rec = host_records(x, tg[j:j + len(part)])
            lo, hi = max(first, j), min(n_ctx - 1, j + len(part))
            if lo >= hi:
                continue
            for v in g.logprob_value(rec[lo - j:hi - j]).tolist():
                nll += -v
            count += hi - lo
            hits += int((rec["argmax"][lo - j:hi - j] == tg[lo:hi]).sum())
        if progress is not None:
            progress(c + 1, n_chunk, nll, count)
    return dict(ppl=ppl_of(nll, count), nll=nll, count=count, top1=hits / count)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model", help="a llama-architecture GGUF file, or a bench model's name (synthetic weights)")
    ap.add_argument("tokens", help=".npy file of token ids")
    ap.add_argument("--ctx", type=int, default=512, help="tokens per chunk (llama-perplexity's n_ctx)")
    ap.add_argument("--batch", type=int, default=512, help="tokens per batch")
    ap.add_argument("--bos", type=int, default=None, help="this id replaces each chunk's first token")
    ap.add_argument("--chunks", type=int, default=0, help="score only the first N chunks (0: all)")
    ap.add_argument("--host", action="store_true", help="logits to the host and the rule in numpy instead")
    ap.add_argument("--compare", type=int, default=0, metavar="ROUNDS", help="device and host, interleaved rounds")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tokens = np.load(args.tokens).astype(np.int64).ravel()
    if args.chunks > 0:
        tokens = tokens[:args.chunks * args.ctx]
    be = g.Backend(0)
    if os.path.exists(args.model):
        hp, w = load_gguf(args.model, dev)
        dec = LlamaDecoder(be, hp, w, args.ctx)
    else:
        import bench
        if args.model not in bench.MODELS:
            raise SystemExit(f"{args.model}: neither a file nor one of {sorted(bench.MODELS)}")
        dec = bench.Token(args.model, dev, 0x51A7, be, args.ctx).dec
    n_chunk = len(tokens) // args.ctx
    tokens = tokens[:n_chunk * args.ctx].tolist()

    def show(i, n, nll, count):
        print(f"[{i}]{ppl_of(nll, count):.4f},", end="\n" if i == n else "", flush=True)

    def device(progress=None):
        return dec.perplexity(tokens, n_ctx=args.ctx, n_batch=args.batch, bos=args.bos, progress=progress)

    def host(progress=None):
        return host_perplexity(dec, be, tokens, args.ctx, args.batch, bos=args.bos, progress=progress)

    def timed(fn, **kw):
        be.synchronize()
        t0 = time.perf_counter()
        r = fn(**kw)
        return r, time.perf_counter() - t0

    if args.compare > 0:
        res = {"device": device(), "host": host()}  # warm-up: graphs built and captured
        secs = {"device": [], "host": []}
        for _ in range(args.compare):
            for name, fn in (("device", device), ("host", host)):
                r, s = timed(fn)
                assert r == res[name]
                secs[name].append(round(s, 5))
        n = n_chunk * args.ctx
        print(json.dumps({"model": args.model, "n_ctx": args.ctx, "n_batch": args.batch, "chunks": n_chunk,
                          "n_vocab": dec.hp["n_vocab"], "seconds": secs,
                          "median_tokens_per_s": {k: round(n / statistics.median(v), 1) for k, v in secs.items()},
                          "bytes_to_host_per_batch": {"device": 24 * min(args.batch, args.ctx),
                                                      "host": 4 * dec.hp["n_vocab"] * min(args.batch, args.ctx)},
                          "ppl": {k: v["ppl"] for k, v in res.items()}, "top1": {k: v["top1"] for k, v in res.items()}}))
        be.close()
        return
    print(f"perplexity: {n_chunk} chunks of {args.ctx} tokens, batches of {args.batch}, "
          f"{'host' if args.host else 'device'} log-probabilities")
    r, s = timed(host if args.host else device, progress=show)
    print(f"Final estimate: PPL = {r['ppl']:.4f} over {r['count']} tokens (nll {r['nll']:.4f}, top-1 {100 * r['top1']:.2f} %)")
    print(f"{n_chunk * args.ctx / s:.1f} tokens/s ({s:.3f} s, the first chunk builds and captures its graphs)")
    be.close()


if __name__ == "__main__":
    main()
