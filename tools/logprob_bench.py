"""kq_logsum_rows next to kq_argmax_rows on the same matrix, on one box in one session: the two
launches of mi355x_logprob_rows by event timing (mi355x_timing_enable), the matrix written by an
elementwise launch just before them, rounds of all shapes interleaved.

    python tools/logprob_bench.py [--shapes 8x32000,8x128256,512x32000,512x128256] [--rounds 5] [--reps 20]

Prints one JSON line: per shape the median and minimum of each launch in microseconds over all
rounds, the spread of the rounds' medians, and the bytes each launch reads over its median time
(rows x n x 4 bytes; the logits of 512 x 128256 are 263 MB, more than the chip's caches hold)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ggml-neon-opt_amd"))

import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402


class Shape:
    def __init__(self, rows, n, dev):
        self.rows, self.n = rows, n
        self.a = torch.randn(rows * n, device=dev) * 4
        self.b = torch.randn(rows * n, device=dev) * 4
        self.x = torch.empty(rows * n, device=dev)
        self.tg = torch.randint(0, n, (rows,), dtype=torch.int32, device=dev)
        self.out = torch.zeros(24 * rows, dtype=torch.uint8, device=dev)
        self.ws = torch.zeros(g.logprob_workspace_size(n, rows), dtype=torch.uint8, device=dev)
        self.us = {"kq_argmax_rows": [], "kq_logsum_rows": []}
        self.medians = {"kq_argmax_rows": [], "kq_logsum_rows": []}

    def run(self, L, stream):
        g.add(self.a, self.b, out=self.x)
        rc = L.mi355x_logprob_rows(self.x.data_ptr(), self.n, self.rows, self.n, self.tg.data_ptr(), self.out.data_ptr(),
                                   self.ws.data_ptr(), self.ws.numel(), stream)
        assert rc == 0, rc

    def check(self):
        x = self.x.view(self.rows, self.n)
        rec = self.out.cpu().numpy().view(g.logprob_dtype())
        assert (rec["argmax"] == torch.argmax(x, dim=1).cpu().numpy()).all()
        lp = g.logprob_value(rec)
        ref = torch.log_softmax(x.double(), dim=1).cpu().numpy()[range(self.rows), self.tg.cpu().numpy()]
        assert abs(lp - ref).max() < 1e-5, abs(lp - ref).max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x32000,8x128256,512x32000,512x128256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = g.lib()
    stream = torch.cuda.current_stream().cuda_stream
    shapes = [Shape(*[int(v) for v in s.split("x")], dev) for s in args.shapes.split(",")]
    torch.cuda.synchronize()
    for s in shapes:  # warm-up and a check of what is timed
        for _ in range(3):
            s.run(L, stream)
        torch.cuda.synchronize()
        s.check()
    for _ in range(args.rounds):
        for s in shapes:
            g.timing_enable(True)
            for _ in range(args.reps):
                s.run(L, stream)
            rows = g.timing_read()
            g.timing_enable(False)
            for k in s.us:
                us = [r[2] * 1e3 for r in rows if r[0].endswith(k)]
                assert len(us) == args.reps, (k, len(us))
                s.us[k] += us
                s.medians[k].append(statistics.median(us))
    out = {"lib": os.path.relpath(g.LIB_PATH, ROOT), "rounds": args.rounds, "reps": args.reps, "shapes": {}}
    for s in shapes:
        mb = s.rows * s.n * 4 / 1e6
        out["shapes"][f"{s.rows}x{s.n}"] = {
            "logits_MB": round(mb, 2), "workgroups_per_row": (s.n + 1023) // 1024,
            **{k: {"us_p50": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                   "round_medians_us": [round(m, 2) for m in s.medians[k]],
                   "GBps_p50": round(mb / statistics.median(v) * 1e3, 1)} for k, v in s.us.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
