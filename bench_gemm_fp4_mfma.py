"""Per-shape decode GEMM bench: the MXFP4-weight MFMA kernel
(ops.skinny_gemm_fp4_mfma) against what ops.decode_linear runs for the same
(n, shape) (1) with bf16 weights and (2) with fp8 weights registered and
set_fp8_decode_max_batch(64).

The method is bench_gemm_fp8_mfma.py's: every path is captured in a HIP graph
and replayed; each graph walks a ring of weight copies larger than the 256 MB
last-level cache, so every call streams its weights from HBM as a decode step
does.  The graphs alternate in windows of >= 0.5 s, three times; the median
per-call time and the spread (max - min) / median of the repeats are printed,
one JSON line per (n, shape, row_tiles)."""
import argparse
import json

import torch

from bench_gemm_fp8_mfma import RING_BYTES, SHAPES, graph_of, window
from skypilot_amd import ops


def median_spread(ts):
    ts = sorted(ts)
    m = ts[len(ts) // 2]
    return m, (ts[-1] - ts[0]) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16,32,48,64")
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
    trs = [int(t) for t in args.row_tiles.split(",")]
    ops.set_fp8_decode_max_batch(64)
    for name, o, i in [s for s in SHAPES if s[0] in want]:
        # bf16 ring, fp8 ring (the registered copies of it) and fp4 ring all
        # hold at least RING_BYTES.
        nbf = max(1, -(-RING_BYTES // (2 * o * i)))
        w = [(torch.randn(o, i, device="cuda") * 0.02).bfloat16()
             for _ in range(nbf)]
        w8 = [w[c % nbf].clone() for c in range(2 * nbf)]
        n4 = 4 * nbf
        q = [ops.quantize_mxfp4(t) for t in w]
        q = [tuple(t.clone() for t in q[c % nbf]) for c in range(n4)]
        # The fp8 copies are registered under w8's addresses only: w itself
        # keeps the bf16 path.
        ops.clear_fp8_weights()
        for t in w8:
            ops.register_fp8_weight(t)
        for n in [int(b) for b in args.batches.split(",")]:
            x = (torch.randn(n, i, device="cuda") * 0.5).bfloat16()
            g_bf = graph_of(lambda c: ops.decode_linear(x, w[c]), nbf)
            g_f8 = graph_of(lambda c: ops.decode_linear(x, w8[c]), len(w8))
            g_f4 = [graph_of(
                lambda c, tr=tr: ops.skinny_gemm_fp4_mfma(x, *q[c], tr), n4)
                for tr in trs]
            tbf, tf8, tf4 = [], [], [[] for _ in trs]
            for _ in range(args.repeats):
                tbf.append(window(g_bf, nbf, args.window))
                tf8.append(window(g_f8, len(w8), args.window))
                for g, t in zip(g_f4, tf4):
                    t.append(window(g, n4, args.window))
            (mb, sb), (m8, s8) = median_spread(tbf), median_spread(tf8)
            for tr, t in zip(trs, tf4):
                m4, s4 = median_spread(t)
                print(json.dumps({
                    "shape": name, "O": o, "I": i, "n": n, "row_tiles": tr,
                    "bf16_us": round(mb * 1e6, 2), "bf16_spread": round(sb, 4),
                    "fp8_us": round(m8 * 1e6, 2), "fp8_spread": round(s8, 4),
                    "fp4_us": round(m4 * 1e6, 2), "fp4_spread": round(s4, 4),
                    "fp4_w_GBps": round(o * i * 17 / 32 / m4 / 1e9),
                    "fp4_TFLOPs": round(2 * n * o * i / m4 / 1e12, 1),
                    "vs_bf16": round(mb / m4, 3),
                    "vs_fp8": round(m8 / m4, 3)}), flush=True)
            del g_bf, g_f8, g_f4
        ops.clear_fp8_weights()
        del w, w8, q
    ops.set_fp8_decode_max_batch(2)


if __name__ == "__main__":
    main()
