"""Per-shape prefill GEMM bench: ops.gemm_mxfp4_a8 (MXFP8 quantiser plus the
block-scaled MFMA GEMM, as a caller pays for it) against F.linear on the bf16
weight, which is what ops.linear runs without the fp4 prefill route.

Every (shape, n) is warmed up first; then the two paths, and the quantiser
alone, alternate in windows of >= 0.5 s of back-to-back calls between device
events, three times.  The median per-call time and the spread (max - min) /
median of the repeats are printed, one JSON line per (shape, n).  TF/s is
2 * n * I * O over the whole call."""
import argparse
import json

import torch
import torch.nn.functional as F

from skypilot_amd import ops

# llama3-8b projections [O, I]
SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096),
          ("down", 4096, 14336)]


def window(fn, seconds):
    """Per-call seconds of fn over a window of at least `seconds`."""
    def run(k):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    est = run(5) / 5
    k = max(5, int(seconds / est) + 1)
    return run(k) / k


def median_spread(ts):
    ts = sorted(ts)
    m = ts[len(ts) // 2]
    return m, (ts[-1] - ts[0]) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="128,512,2048,8192")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops.native()
    torch.manual_seed(0)
    want = args.shapes.split(",")
    tokens = [int(t) for t in args.tokens.split(",")]
    for name, o, i in [s for s in SHAPES if s[0] in want]:
        w = (torch.randn(o, i, device="cuda") * 0.02).bfloat16()
        codes, exps = ops.quantize_mxfp4(w)
        xs = {n: (torch.randn(n, i, device="cuda") * 0.5).bfloat16()
              for n in tokens}
        paths = {n: (lambda x=xs[n]: F.linear(x, w),
                     lambda x=xs[n]: ops.gemm_mxfp4_a8(x, codes, exps),
                     lambda x=xs[n]: ops.quantize_mxfp8_rows(x))
                 for n in tokens}
        with torch.no_grad():
            for n in tokens:            # warm up every shape first
                for fn in paths[n]:
                    window(fn, 0.05)
            for n in tokens:
                ts = [[], [], []]
                for _ in range(args.repeats):
                    for t, fn in zip(ts, paths[n]):
                        t.append(window(fn, args.window))
                (mb, sb), (m4, s4), (mq, _) = (median_spread(t) for t in ts)
                print(json.dumps({
                    "shape": name, "O": o, "I": i, "n": n,
                    "bf16_us": round(mb * 1e6, 1), "bf16_spread": round(sb, 4),
                    "fp4_us": round(m4 * 1e6, 1), "fp4_spread": round(s4, 4),
                    "quant_share": round(mq / m4, 3),
                    "bf16_TFLOPs": round(2 * n * o * i / mb / 1e12, 1),
                    "fp4_TFLOPs": round(2 * n * o * i / m4 / 1e12, 1),
                    "vs_bf16": round(mb / m4, 3)}), flush=True)
        del w, codes, exps, xs, paths


if __name__ == "__main__":
    main()
