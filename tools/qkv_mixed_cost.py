"""The q/k/v launch with the norm prologue, mixed types against one type (diagnostic): q and k
Q4_K with v Q6_K (kq_rows<7, true, 1>, its type branch behind the argument fetch) against all
three Q4_K (kq_rows<1, true, 1>), at TinyLlama's and Llama-3-8B's shapes. Median per-launch
kernel time from the library's launch events, weights rotated over > 600 MB.
    MI355X_LIB=ggml-neon-opt_amd/lib/variants/libNAME.so python tools/qkv_mixed_cost.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402
from bench import random_kquant  # noqa: E402

Q4, Q6 = 12, 14


def main(reps=60):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    tag = os.path.basename(os.environ.get("MI355X_LIB", "default"))
    for label, K, rows in (("tl qkv", 2048, (2048, 256, 256)), ("l3 qkv", 4096, (4096, 1024, 1024))):
        for kind, types in (("one type", (Q4, Q4, Q4)), ("mixed", (Q4, Q4, Q6))):
            mats = list(zip(types, rows))
            nbytes = sum(n * (K // 256) * g.BLOCK_BYTES[t] for t, n in mats)
            nbuf = max(2, int(np.ceil(640e6 / nbytes)))
            wsets = [[random_kquant(t, n, K, gen, dev) for t, n in mats] for _ in range(nbuf)]
            x = torch.randn(K, device=dev, generator=gen)
            x2 = torch.rand(K, device=dev, generator=gen) + 0.5
            ys = [torch.empty(n, device=dev) for _, n in mats]

            def call(i):
                g.gemv_fused_ext([(t, w, y) for (t, _), w, y in zip(mats, wsets[i % nbuf], ys)], x,
                                 prologue=g.PRO_RMS_NORM, x2=x2, eps=1e-5)
            for i in range(nbuf):
                call(i)
            meds = []
            for _ in range(3):
                g.timing_enable(True)
                for i in range(reps):
                    call(i)
                rows_ = g.timing_read()
                g.timing_enable(False)
                meds.append(float(np.median([r[2] for r in rows_]) * 1e3))
            print(f"{tag:18s} {label} K={K} {kind:8s} {rows_[0][0]:26s} " + " ".join(f"{m:5.2f}" for m in meds) + " us",
                  flush=True)
            del wsets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
