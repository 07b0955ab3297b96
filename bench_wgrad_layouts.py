"""Which operand layout should the weight-gradient GEMM run in?

dW [out, in] = dy^T x with dy [M, out], x [M, in], M = tokens.  Three
ways to ask the library for it, timed as GEMMs alone on the Llama-3-8B
training shapes (docs/BENCHMARKS.md, "Weight-gradient layouts"):

  (a) dy.t() @ x            today's call: neither operand contiguous
                            along the contraction (Ailk_Bjlk)
  (b) F.linear(dyT, xT)     both transposed first: the forward's layout
  (c) dyT @ x               dy transposed only: the dgrad layout

and, separately, what the transposes cost: t().contiguous(), the
extension's transpose_bf16, and a same-size copy_ as the yardstick.

Protocol: device events, windows of >= 0.5 s, five rounds, the arms of a
shape alternating inside a round; median of the rounds, and for arm (a)
also min..max.  FLOPs and bytes come from the shapes.
"""
import argparse
import json
import statistics

import torch
import torch.nn.functional as F

HBM_TBS = 6.0   # what a transpose at copy speed is projected to reach


def window(fn, n):
    """Milliseconds per call over n back-to-back calls (device events)."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def run_arms(arms, rounds, min_window_s):
    """arms: {name: fn}.  Returns {name: [ms per round]}."""
    counts = {}
    for name, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = window(fn, 5)
        counts[name] = max(5, int(min_window_s * 1e3 / ms) + 1)
    out = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():   # alternate inside the round
            out[name].append(window(fn, counts[name]))
    return out


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=6 * 4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    M = args.tokens
    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096),
              ("gate_up", 28672, 4096), ("down", 4096, 14336)]
    try:
        from skypilot_amd import ops
        native = ops.native()
    except Exception:  # noqa: BLE001 - the layout question needs no kernel
        native = None

    torch.manual_seed(0)
    results = []
    for name, O, I in shapes:
        dy = (torch.randn(M, O, device=dev) * 0.1).bfloat16()
        x = (torch.randn(M, I, device=dev) * 0.1).bfloat16()
        dyT, xT = dy.t().contiguous(), x.t().contiguous()
        flops = 2.0 * M * O * I
        gemm_bytes = 2.0 * (M * O + M * I + O * I)
        arms = {"a": lambda: dy.t() @ x,
                "b": lambda: F.linear(dyT, xT),
                "c": lambda: dyT @ x}
        if name == "qkv":   # today's three separate products
            parts = [p.contiguous() for p in dy.split([4096, 1024, 1024], 1)]
            arms["a_split"] = lambda: [p.t() @ x for p in parts]
        g = run_arms(arms, args.rounds, args.window)

        dy_copy, x_copy = torch.empty_like(dy), torch.empty_like(x)
        tarms = {"dy_torch": lambda: dy.t().contiguous(),
                 "x_torch": lambda: x.t().contiguous(),
                 "dy_copy": lambda: dy_copy.copy_(dy),
                 "x_copy": lambda: x_copy.copy_(x)}
        if native is not None:
            tarms["dy_native"] = lambda: native.transpose_bf16(dy)
            tarms["x_native"] = lambda: native.transpose_bf16(x)
        t = run_arms(tarms, args.rounds, args.window)

        dy_rw, x_rw = 4.0 * M * O, 4.0 * M * I   # bytes read + written
        proj_dy = dy_rw / (HBM_TBS * 1e12) * 1e3
        proj_x = x_rw / (HBM_TBS * 1e12) * 1e3
        a = med(g["a"])
        row = {
            "shape": name, "out": O, "in": I, "tokens": M,
            "flops": flops, "gemm_bytes": gemm_bytes,
            "gemm_ms": {k: med(v) for k, v in g.items()},
            "gemm_a_min_max_ms": [min(g["a"]), max(g["a"])],
            "gemm_pflops": {k: flops / med(v) / 1e12 for k, v in g.items()},
            "transpose_ms": {k: med(v) for k, v in t.items()},
            "transpose_tbs": {
                k: (dy_rw if k.startswith("dy") else x_rw) / med(v) / 1e9
                for k, v in t.items()},
            "projected_transpose_ms": {"dy": proj_dy, "x": proj_x},
            "net_ms_vs_a": {"b": a - med(g["b"]) - proj_dy - proj_x,
                            "c": a - med(g["c"]) - proj_dy},
        }
        results.append(row)
        print(f"--- {name}: out {O} in {I} tokens {M}  "
              f"{flops / 1e12:.3f} TFLOP  GEMM operands {gemm_bytes / 1e9:.2f}"
              f" GB  dy r+w {dy_rw / 1e9:.2f} GB  x r+w {x_rw / 1e9:.2f} GB")
        for k, v in g.items():
            extra = (f"  min..max {min(v):.3f}..{max(v):.3f}"
                     if k == "a" else "")
            print(f"  gemm ({k:7s}) {med(v):7.3f} ms  "
                  f"{flops / med(v) / 1e12:6.3f} PF/s{extra}")
        for k, v in t.items():
            b = dy_rw if k.startswith("dy") else x_rw
            print(f"  move {k:10s} {med(v):7.3f} ms  {b / med(v) / 1e9:5.2f}"
                  " TB/s")
        print(f"  net vs (a) after transposes projected at {HBM_TBS} TB/s: "
              f"(b) {row['net_ms_vs_a']['b']:+.3f} ms  "
              f"(c) {row['net_ms_vs_a']['c']:+.3f} ms")
        del dy, x, dyT, xT, dy_copy, x_copy, arms, tarms
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
