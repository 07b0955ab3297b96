#!/usr/bin/env python3
"""Kernel times of the decode advance step: ops.decode_advance (argmax)
against ops.decode_sample_advance in its four modes, on [1, 128256]
and [64, 128256] bf16 logits.

Device events around --launches back-to-back launches, --rounds rounds
with the variants interleaved in one process; prints the median and the
minimum per launch.  The logits stay in cache between launches, as they
do in the decode graph, where the lm-head GEMV has just written them."""
from __future__ import annotations

import argparse
import statistics

import torch

from skypilot_amd import ops

MODES = {            # temperature, top_p, top_k
    "greedy": (0.0, 1.0, 0),
    "T only": (0.8, 1.0, 0),
    "top_p 0.9": (0.8, 0.9, 0),
    "top_k 40 + top_p 0.9": (0.8, 0.9, 40),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = "cuda"
    for b in [int(x) for x in args.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(b)
        logits = (torch.randn(b, args.vocab, device=dev, generator=g)
                  * 4).bfloat16()
        stage = torch.zeros(6, b, dtype=torch.int32, device=dev)
        ring = torch.zeros(8, b, dtype=torch.long, device=dev)
        ctr = torch.zeros(1, dtype=torch.long, device=dev)
        variants = {"decode_advance": lambda: ops.decode_advance(
            logits, stage, ring, ctr)}
        for name, (T, p, k) in MODES.items():
            samp = ops.pack_samp(b, T, p, k, list(range(b)))[:5] \
                .contiguous().to(dev)
            variants[f"sample_advance {name}"] = (
                lambda samp=samp: ops.decode_sample_advance(
                    logits, stage, ring, ctr, samp))
        times = {k: [] for k in variants}
        for fn in variants.values():     # warm up every variant
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in variants.items():
                stage.zero_()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(
                    e0.elapsed_time(e1) * 1e3 / args.launches)
        base = statistics.median(times["decode_advance"])
        print(f"logits [{b}, {args.vocab}] bf16, us per launch "
              f"(median / min of {args.rounds} x {args.launches}):")
        for name, ts in times.items():
            med = statistics.median(ts)
            print(f"  {name:38s} {med:8.1f} / {min(ts):8.1f}   "
                  f"{med / base:5.2f}x decode_advance", flush=True)


if __name__ == "__main__":
    main()
