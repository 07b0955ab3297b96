"""Per-shape GEMM bench beyond 64 tokens: the fp8-weight LDS-shared MFMA GEMM
(ops.gemm_fp8_w8) against F.linear on the bf16 weight (hipBLASLt), which is
what ops.linear and ops.decode_linear run for these token counts without the
fp8 prefill route.

The method is bench_gemm_fp8_mfma.py's: both paths are captured in a HIP
graph that walks a ring of weight copies larger than the 256 MB last-level
cache, so every call streams its weights from HBM as a layer of a real model
does.  The graphs alternate in windows of >= 0.5 s, three times; the median
per-call time and the spread (max - min) / median of the repeats are printed,
one JSON line per (shape, n, row_tiles)."""
import argparse
import json

import torch
import torch.nn.functional as F

from skypilot_amd import ops
from bench_gemm_fp8_mfma import RING_BYTES, graph_of, window

# llama3-8b projections [O, I]
SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096),
          ("down", 4096, 14336)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="65,96,128,192,256,512,2048")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--row-tiles", default="0",
                    help="row tiles per wave to time, comma separated "
                         "(0: the launcher's own choice)")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops.native()
    torch.manual_seed(0)
    want = args.shapes.split(",")
    trs = [int(t) for t in args.row_tiles.split(",")]
    for name, o, i in [s for s in SHAPES if s[0] in want]:
        copies = max(1, -(-RING_BYTES // (o * i)))
        w = [(torch.randn(o, i, device="cuda") * 0.02).bfloat16()
             for _ in range(max(1, copies // 2))]
        q = [ops.quantize_fp8_rowwise(w[c % len(w)]) for c in range(copies)]
        q = [(a.clone(), b.clone()) for a, b in q]
        for n in [int(t) for t in args.tokens.split(",")]:
            x = (torch.randn(n, i, device="cuda") * 0.5).bfloat16()
            with torch.no_grad():
                g_old = graph_of(lambda c: F.linear(x, w[c % len(w)]), len(w))
                g_new = [graph_of(
                    lambda c, tr=tr: ops.gemm_fp8_w8(x, *q[c], tr), copies)
                    for tr in trs]
            told, tnew = [], [[] for _ in trs]
            for _ in range(args.repeats):
                told.append(window(g_old, len(w), args.window))
                for g, t in zip(g_new, tnew):
                    t.append(window(g, copies, args.window))
            told.sort()
            mo = told[len(told) // 2]
            for tr, t in zip(trs, tnew):
                t.sort()
                mn = t[len(t) // 2]
                print(json.dumps({
                    "shape": name, "O": o, "I": i, "n": n, "row_tiles": tr,
                    "bf16_us": round(mo * 1e6, 2),
                    "bf16_spread": round((told[-1] - told[0]) / mo, 4),
                    "bf16_TFLOPs": round(2 * n * o * i / mo / 1e12, 1),
                    "fp8_us": round(mn * 1e6, 2),
                    "fp8_spread": round((t[-1] - t[0]) / mn, 4),
                    "fp8_w_GBps": round(o * i / mn / 1e9),
                    "fp8_TFLOPs": round(2 * n * o * i / mn / 1e12, 1),
                    "vs_bf16": round(mo / mn, 3)}), flush=True)
            del g_old, g_new
        del w, q


if __name__ == "__main__":
    main()
