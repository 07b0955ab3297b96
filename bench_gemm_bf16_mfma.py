"""Per-shape batched-decode GEMM bench: the bf16-weight MFMA kernel
(ops.skinny_gemm_bf16_mfma) against what ops.decode_linear runs for the same
(n, shape) with the route off (the bf16 GEMV or F.linear / hipBLASLt): the
"parent".

The method is bench_gemm_fp8_mfma.py's: both paths are captured in a HIP
graph that walks a ring of weight copies of 768 MB or more (beyond the 256 MB
last-level cache, so every call streams its weights from HBM as a decode step
does) and replayed; the graphs alternate in windows of >= 0.5 s, three each;
the median per-call time, the spread (max - min) / median and W bytes over
time are printed, one JSON line per (n, shape, row_tiles, k_splits).

--sweep-batches times every (row_tiles, k_splits) of --row-tiles x --k-splits
at those n, without the parent; the configuration with the smallest summed
median then runs against the parent at every n of --batches ("pick": true).
With an empty --sweep-batches the kernel runs with the launcher's own choice
(row_tiles = k_splits = 0)."""
import argparse
import json

import torch

from bench_gemm_fp8_mfma import RING_BYTES, SHAPES, graph_of, window
from skypilot_amd import ops


def timed(graphs, calls, seconds, repeats):
    """Median and spread per graph, the graphs alternating."""
    ts = [[] for _ in graphs]
    for _ in range(repeats):
        for g, c, t in zip(graphs, calls, ts):
            t.append(window(g, c, seconds))
    out = []
    for t in ts:
        t.sort()
        med = t[len(t) // 2]
        out.append((med, (t[-1] - t[0]) / med))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,4,8,16,32,48,64")
    ap.add_argument("--sweep-batches", default="4,16,64")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--row-tiles", default="1,2,4")
    ap.add_argument("--k-splits", default="1,2,4,8")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops.native()
    ops.set_bf16_decode_max_batch(1)      # the parent: the route off
    torch.manual_seed(0)
    ints = lambda s: [int(v) for v in s.split(",") if v]
    cfgs = [(tr, ks) for tr in ints(args.row_tiles)
            for ks in ints(args.k_splits)]
    want = args.shapes.split(",")
    for name, o, i in [s for s in SHAPES if s[0] in want]:
        copies = max(1, -(-RING_BYTES // (2 * o * i)))
        w = [(torch.randn(o, i, device="cuda") * 0.02).bfloat16()
             for _ in range(copies)]
        wb = 2 * o * i

        def new_graph(x, tr, ks):
            return graph_of(
                lambda c: ops.skinny_gemm_bf16_mfma(x, w[c], tr, ks), copies)

        pick, total = (0, 0), {}
        for n in ints(args.sweep_batches):
            x = (torch.randn(n, i, device="cuda") * 0.5).bfloat16()
            gs = [new_graph(x, tr, ks) for tr, ks in cfgs]
            res = timed(gs, [copies] * len(gs), args.window, args.repeats)
            for (tr, ks), (med, spread) in zip(cfgs, res):
                total[tr, ks] = total.get((tr, ks), 0.0) + med
                print(json.dumps({
                    "shape": name, "O": o, "I": i, "n": n, "row_tiles": tr,
                    "k_splits": ks, "mfma_us": round(med * 1e6, 2),
                    "mfma_spread": round(spread, 4),
                    "mfma_w_GBps": round(wb / med / 1e9)}), flush=True)
            del gs
        if total:
            pick = min(total, key=total.get)
        for n in ints(args.batches):
            x = (torch.randn(n, i, device="cuda") * 0.5).bfloat16()
            g_old = graph_of(lambda c: ops.decode_linear(x, w[c]), copies)
            g_new = new_graph(x, *pick)
            (mo, so), (mn, sn) = timed([g_old, g_new], [copies] * 2,
                                       args.window, args.repeats)
            print(json.dumps({
                "shape": name, "O": o, "I": i, "n": n, "pick": True,
                "row_tiles": pick[0], "k_splits": pick[1],
                "parent_us": round(mo * 1e6, 2),
                "parent_spread": round(so, 4),
                "parent_w_GBps": round(wb / mo / 1e9),
                "mfma_us": round(mn * 1e6, 2), "mfma_spread": round(sn, 4),
                "mfma_w_GBps": round(wb / mn / 1e9),
                "mfma_TFLOPs": round(2 * n * o * i / mn / 1e12, 1),
                "speedup": round(mo / mn, 3)}), flush=True)
            del g_old, g_new
        del w


if __name__ == "__main__":
    main()
