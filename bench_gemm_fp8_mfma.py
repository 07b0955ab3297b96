"""Per-shape batched-decode GEMM bench: the fp8-weight MFMA kernel
(ops.skinny_gemm_fp8_mfma) against what ops.decode_linear runs for the same
(n, shape) with bf16 weights (the skinny GEMV or F.linear / hipBLASLt).

Both paths are timed the way the decode step runs them: captured in a HIP
graph and replayed.  Each graph walks a ring of weight copies larger than
the 256 MB last-level cache, so every call streams its weights from HBM as
a decode step does.  The two graphs alternate in windows of >= 0.5 s, three
times; the median per-call time, the spread (max - min) / median of the
repeats, and W bytes over time are printed, one JSON line per (n, shape)."""
import argparse
import json
import time

import torch

from skypilot_amd import ops

SHAPES = [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096),
          ("down", 4096, 14336), ("lm_head", 128256, 4096)]
RING_BYTES = 768 << 20


def graph_of(fn, copies):
    for c in range(copies):       # warm-up: code objects, GEMM algorithms
        fn(c)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in range(copies):
            fn(c)
    g.replay()
    torch.cuda.synchronize()
    return g


def window(g, calls, seconds):
    """Per-call seconds over a window of at least `seconds`."""
    reps, t = 1, 0.0
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            g.replay()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if t >= seconds:
            return t / (reps * calls)
        reps = max(reps * 2, int(reps * 1.2 * seconds / max(t, 1e-6)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,8,16,32,64")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--row-tiles", default="0",
                    help="row tiles per wave to time, comma separated "
                         "(0: the kernel's own choice)")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ops.native()
    torch.manual_seed(0)
    want = args.shapes.split(",")
    for name, o, i in [s for s in SHAPES if s[0] in want]:
        copies = max(1, -(-RING_BYTES // (o * i)))
        w = [(torch.randn(o, i, device="cuda") * 0.02).bfloat16()
             for _ in range(max(1, copies // 2))]
        q = [ops.quantize_fp8_rowwise(w[c % len(w)]) for c in range(copies)]
        q = [(a.clone(), b.clone()) for a, b in q]
        for n in [int(b) for b in args.batches.split(",")]:
            x = (torch.randn(n, i, device="cuda") * 0.5).bfloat16()
            g_old = graph_of(
                lambda c: ops.decode_linear(x, w[c % len(w)]), len(w))
            trs = [int(t) for t in args.row_tiles.split(",")]
            g_new = [graph_of(
                lambda c, tr=tr: ops.skinny_gemm_fp8_mfma(x, *q[c], tr),
                copies) for tr in trs]
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
                    "parent_us": round(mo * 1e6, 2),
                    "parent_spread": round((told[-1] - told[0]) / mo, 4),
                    "parent_w_GBps": round(2 * o * i / mo / 1e9),
                    "mfma_us": round(mn * 1e6, 2),
                    "mfma_spread": round((t[-1] - t[0]) / mn, 4),
                    "mfma_w_GBps": round(o * i / mn / 1e9),
                    "mfma_TFLOPs": round(2 * n * o * i / mn / 1e12, 1),
                    "speedup": round(mo / mn, 3)}), flush=True)
            del g_old, g_new
        del w, q


if __name__ == "__main__":
    main()
