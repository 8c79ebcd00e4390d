"""In-kernel timeline of one GEMV launch (diagnostic build path): per-wave
s_memrealtime stamps at entry / after prologue / after main loop / exit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ggml-neon-opt_amd")]
# stamps exist only in the diagnostic build:
#   make -C ggml-neon-opt_amd variant NAME=diag VFLAGS="-DKQ_ROWS_DIAG=1 -DKQ_GEMV_DIAG=1"
os.environ.setdefault("MI355X_LIB", os.path.join(ROOT, "ggml-neon-opt_amd/lib/variants/libdiag.so"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ggml_mi355x as g  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knobs  # noqa: E402
knobs.apply_env()  # the MI355X_* A/B environment -> explicit library calls

from bench import random_kquant  # noqa: E402

SHAPES = [("tl q", 12, 2048, 2048), ("tl 8rows", 12, 2048, 8), ("tl gate+up", 12, 2048, 11264),
          ("tl down", 12, 5632, 2048), ("tl out q6", 14, 2048, 32000), ("l3 up", 12, 4096, 14336),
          ("70b down", 12, 28672, 8192)]


PRO = os.environ.get("STAMPS_PRO", "none")  # none | norm | swiglu: fused prologue (kq_rows only)
# STAMPS_SLEEP=1: a spin kernel (torch.cuda._sleep, ~10 ms) ahead of the burst, so the burst's
# launches queue behind it and run back to back, as in the graph-replayed token. Without it
# the GPU idles between the eager launches of a short kernel and its XCDs wake in turn
# (tools/xcd_skew.hip: 0.1 .. 1.4 us apart), which the entry stamps then show.
SLEEP = os.environ.get("STAMPS_SLEEP", "0") == "1"
# STAMPS_SHAPES="tl q,l3 up": only these rows of SHAPES
ONLY = [v.strip() for v in os.environ.get("STAMPS_SHAPES", "").split(",") if v.strip()]
SLOTS = 16  # stamp slots per wave of kq_rows (kq_rows.hip ROWS_STAMP_SLOTS)


def main(impl):
    g.gemv_impl(impl)
    pro = {"none": g.PRO_NONE, "norm": g.PRO_RMS_NORM, "swiglu": g.PRO_SWIGLU}[PRO]
    tag = ("rows " if impl == 0 else "tasks") + ("" if PRO == "none" else "/" + PRO)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    buf = torch.zeros(1 << 20, dtype=torch.int64, device=dev)
    for label, typ, K, N in SHAPES:
        if ONLY and label not in ONLY:
            continue
        ws = [random_kquant(typ, N, K, gen, dev) for _ in range(max(2, int(600e6 // (N * K // 256 * 144))))]
        x = torch.randn(1, K, device=dev)
        x2 = torch.rand(K, device=dev) + 0.5
        y = torch.empty(1, N, device=dev)

        def mm(w):
            if pro == g.PRO_NONE:
                g.mul_mat(typ, w, K, x, out=y)
            else:
                g.gemv_fused_ext([(typ, w, y[0])], x[0], prologue=pro, x2=x2, eps=1e-5)
        for w in ws:
            mm(w)
        res, nres, sres = [], [], []
        for r in range(5):
            buf.zero_()
            torch.cuda.synchronize()
            if SLEEP:
                torch.cuda._sleep(20_000_000)
            # warm the clocks with a burst; stamps of the LAST launch of the burst survive
            for i in range(60):
                if i == 59:
                    g.lib().mi355x_diag_stamps(buf.data_ptr(), buf.numel() * 8)
                mm(ws[(r * 60 + i) % len(ws)])
            torch.cuda.synchronize()
            g.lib().mi355x_diag_stamps(None, 0)
            st = buf.cpu().numpy().astype(np.int64).reshape(-1, SLOTS if impl == 0 else 8)  # (kq_gemv, kq_kernels.hip: 8 slots)
            if os.environ.get("STAMPS_DUMP") and r == 4:  # raw per-(block, wave) rows for offline analysis
                np.save(os.environ["STAMPS_DUMP"] + "_" + label.replace(" ", "_") + ".npy", st[:256 * 12])
            st = st[st[:, 0] != 0]
            t0 = st[:, 0].min()
            rel = (st - t0) * 10 / 1000.0  # 100 MHz ticks -> us
            med = lambda v: float(np.median(v))  # noqa: E731
            if impl == 0:  # kq_rows: [entry, ring filled, loop end, exit, x landed, x quantized, first step, arguments fetched]
                ok = rel[:, 4] > 0
                # slot 7: the stamp after the entry's one scalar wait (kq_rows; builds before it
                # leave 0, kq_rows_dyn keeps its unit count there): x-wait = argument fetch +
                # the rest of the activation fetch
                ha = ok & (st[:, 7] >= t0)
                args = med(rel[ha, 7] - rel[ha, 0]) if ha.any() else float("nan")
                res.append((len(st), rel[:, 0].max(), med(rel[ok, 4] - rel[ok, 0]), med(rel[ok, 5] - rel[ok, 4]),
                            med(rel[:, 1] - rel[:, 5]), med(rel[ok, 6] - rel[ok, 1]),
                            med(rel[:, 1] - rel[:, 0]), med(rel[:, 2] - rel[:, 1]), np.max(rel[:, 2] - rel[:, 1]),
                            rel[:, 3].max(), rel[:, 2].max(), med(rel[:, 2]), args))
                # the norm interval of the waves that hold a part of the row (slot 12: passes of x
                # held): [8] x landed, [9] sums published, [10] barrier passed, [11] scale known,
                # [4] transformed; waves without x: their whole prologue
                # the interval after the barrier of the waves that stream rows: [1] barrier passed,
                # [13] first step's wait passed, [6] first record written, [14] chain started (the
                # last step's records written), [2] chain done, [15] stores issued, [3] exit
                hs = (st[:, 13] >= t0) & (st[:, 15] >= t0) & (st[:, 14] >= t0)
                if hs.any():
                    sres.append((med(rel[hs, 13] - rel[hs, 1]), med(rel[hs, 6] - rel[hs, 13]), med(rel[hs, 14] - rel[hs, 6]),
                                 med(rel[hs, 2] - rel[hs, 14]), med(rel[hs, 15] - rel[hs, 2]), med(rel[hs, 3] - rel[hs, 15]),
                                 med(rel[hs, 3] - rel[hs, 1]), float(np.max(rel[hs, 3] - rel[hs, 1])), float(hs.sum()) / len(st)))
                hx = ok & (st[:, 12] > 0) & (st[:, 11] >= t0)
                if PRO == "norm" and hx.any():
                    nx = ok & (st[:, 10] >= t0) & (st[:, 12] == 0)
                    nres.append((med(rel[hx, 8] - rel[hx, 0]), med(rel[hx, 9] - rel[hx, 8]), med(rel[hx, 10] - rel[hx, 9]),
                                 med(rel[hx, 11] - rel[hx, 10]), med(rel[hx, 4] - rel[hx, 11]), med(rel[hx, 5] - rel[hx, 4]),
                                 med(rel[hx, 1] - rel[hx, 0]), float(hx.sum()) / len(st),
                                 med(rel[nx, 1] - rel[nx, 0]) if nx.any() else float("nan")))
                continue
            res.append((len(st), rel[:, 0].max(), med(rel[:, 4] - rel[:, 0]), med(rel[:, 5] - rel[:, 4]),
                        med(rel[:, 6] - rel[:, 5]), med(rel[:, 1] - rel[:, 6]),
                        med(rel[:, 1] - rel[:, 0]), med(rel[:, 2] - rel[:, 1]), np.max(rel[:, 2] - rel[:, 1]),
                        rel[:, 3].max()))
        a = np.array(res)[1:].mean(0)
        if impl == 0:
            print(f"{tag} {label:12s} waves={int(a[0]):5d} start_spread={a[1]:5.2f}us | x-wait {a[2]:4.2f} (args {a[12]:4.2f}) quant {a[3]:4.2f} "
                  f"barrier+fill {a[4]:4.2f} = prologue {a[6]:4.2f} | first step {a[5]:4.2f} loop med/max={a[7]:5.2f}/{a[8]:5.2f} "
                  f"loop end med/max={a[11]:6.2f}/{a[10]:6.2f} end={a[9]:6.2f}us")
            if sres:
                c = np.array(sres)[1:].mean(0)
                print(f"{tag} {label:12s}   after the barrier, waves with rows ({c[8]:4.2f} of all): first wait {c[0]:4.2f} | first "
                      f"record {c[1]:4.2f} | later steps {c[2]:4.2f} | chain {c[3]:4.2f} | stores {c[4]:4.2f} | exit {c[5]:4.2f} | "
                      f"barrier -> exit med/max {c[6]:4.2f}/{c[7]:4.2f}")
            if nres:
                b = np.array(nres)[1:].mean(0)
                print(f"{tag} {label:12s}   norm interval, waves with x ({b[7]:4.2f} of all): x landed {b[0]:4.2f} | sums published "
                      f"{b[1]:4.2f} | barrier passed {b[2]:4.2f} | scale known {b[3]:4.2f} | transformed {b[4]:4.2f} | quantized "
                      f"{b[5]:4.2f} | prologue {b[6]:4.2f}; waves without x: prologue {b[8]:4.2f}")
            continue
        print(f"{tag} {label:12s} waves={int(a[0]):5d} start_spread={a[1]:5.2f}us | lookup {a[2]:4.2f} issue {a[3]:4.2f} "
              f"wait {a[4]:4.2f} quant {a[5]:4.2f} = prologue {a[6]:4.2f} | loop med/max={a[7]:5.2f}/{a[8]:5.2f} "
              f"end={a[9]:6.2f}us")


if __name__ == "__main__":
    for impl in ((0,) if PRO != "none" or "rows" in sys.argv else (0, 1)):
        main(impl)
