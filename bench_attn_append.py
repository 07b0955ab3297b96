#!/usr/bin/env python3
"""Append-attention kernel bench (attn_append_kernel) on one MI355X.

1. Same work as the 64-tile forward: q_start = 0, q_len = Sq = S = 4032
   (a multiple of 64, not of 256, so ops.attention runs
   attn_fwd_swapped_kernel), B = 2, Hq 32 / Hkv 8.  Both kernels are timed
   in one process in alternating rounds after warm-up; the forward's own
   round-to-round spread is printed next to the ratio.
2. One chunk late in a long prompt: Sq = 512 at q_start = 3584, same
   heads, in TF/s by the causal-trapezoid FLOP count.
"""
from __future__ import annotations

import argparse
import statistics
import time

import torch

from skypilot_amd import ops

D = 128


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def append_flops(n, Hq, q_start, q_len):
    """QK^T + PV over the causal trapezoid: row i sees q_start + i + 1
    kv rows; 2 matmuls x 2 FLOPs per MAC."""
    pairs = q_len * q_start + q_len * (q_len + 1) // 2
    return 2 * 2 * n * Hq * pairs * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    C = ops.native()
    scale = D ** -0.5
    n, Hq, Hkv = 2, 32, 8

    def i32(vals):
        return torch.tensor(vals, dtype=torch.int32, device=dev)

    def rnd(*shape):
        return (torch.randn(*shape, device=dev) * 0.5).bfloat16()

    # ---- 1. identical work: append at q_start 0 vs the 64-tile forward
    S = 4032
    q, k, v = rnd(n, S, Hq, D), rnd(n, S, Hkv, D), rnd(n, S, Hkv, D)
    slots, zeros, full = i32([0, 1]), i32([0, 0]), i32([S, S])

    def fwd():
        return C.attn_fwd(q, k, v, scale, True)[0]

    def app():
        # k, v double as a 2-slot cache with S_max = S
        return C.attn_append(q, k, v, slots, zeros, full, scale)

    diff = (fwd().float() - app().float()).abs().max().item()
    t_fwd, t_app = [], []
    for _ in range(args.rounds):
        t_fwd.append(timeit(fwd, args.iters))
        t_app.append(timeit(app, args.iters))
    fl = append_flops(n, Hq, 0, S)
    mf, ma = statistics.median(t_fwd), statistics.median(t_app)
    spread = (max(t_fwd) - min(t_fwd)) / mf
    print(f"same work, n={n} S={S} Hq={Hq} Hkv={Hkv}: "
          f"max |append - fwd| = {diff:.3e}")
    print(f"  attn_fwd_swapped_kernel  median {mf*1e3:7.3f} ms "
          f"({fl/mf/1e12:6.1f} TF/s)  min {min(t_fwd)*1e3:7.3f} "
          f"max {max(t_fwd)*1e3:7.3f}  spread {spread*100:5.2f} %")
    print(f"  attn_append_kernel       median {ma*1e3:7.3f} ms "
          f"({fl/ma/1e12:6.1f} TF/s)  min {min(t_app)*1e3:7.3f} "
          f"max {max(t_app)*1e3:7.3f}")
    print(f"  append / fwd = {ma/mf:6.4f}  "
          f"(allowance: 1 + spread + 0.10 = {1 + spread + 0.10:6.4f})")

    # ---- 2. one chunk at the end of a 4096-token prompt
    Sq, q_start, S_max = 512, 3584, 4096
    qc = rnd(n, Sq, Hq, D)
    kc, vc = rnd(n, S_max, Hkv, D), rnd(n, S_max, Hkv, D)
    starts, lens = i32([q_start] * n), i32([Sq] * n)

    def chunk():
        return C.attn_append(qc, kc, vc, slots, starts, lens, scale)

    t_ch = [timeit(chunk, args.iters) for _ in range(args.rounds)]
    mc = statistics.median(t_ch)
    flc = append_flops(n, Hq, q_start, Sq)
    print(f"chunk, n={n} Sq={Sq} q_start={q_start} Hq={Hq} Hkv={Hkv}: "
          f"median {mc*1e3:7.3f} ms ({flc/mc/1e12:6.1f} TF/s)  "
          f"min {min(t_ch)*1e3:7.3f} max {max(t_ch)*1e3:7.3f}")


if __name__ == "__main__":
    main()
