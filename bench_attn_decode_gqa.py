#!/usr/bin/env python3
"""Grouped split-KV decode attention bench on one MI355X (docs/BENCHMARKS.md,
"Grouped split-KV decode").

attn_decode_qkv / attn_decode_qkv_fp8 (one block per sequence and q head,
the parent) against attn_decode_qkv_gqa / attn_decode_qkv_gqa_fp8 (one block
per sequence, kv head and kv range) at (n, kv_len) in (64, 4096),
(64, 1024), (8, 4096), (1, 4096) with Hq 32 / Hkv 8, and (8, 4096) with
Hq 64 / Hkv 8.  K/V bytes per second count each cache row once.

--split-sweep also times the new kernels with split_rows 128, 256 and 512
at (64, 4096) and (1, 4096): the measurement behind kDecodeSplitRows.

Timing as bench_kv_fp8.py: device events around a window of back-to-back
launches of at least --window seconds, five rounds, parent and new
alternating (parent, new, parent again); medians, and the parent's spread
over its ten windows, which a difference has to beat.
"""
from __future__ import annotations

import argparse
import statistics

import torch

from bench_kv_fp8 import compare, kv_bytes, window, calibrate
from skypilot_amd import ops

D = 128
SHAPES = ((64, 4096, 32, 8), (64, 1024, 32, 8), (8, 4096, 32, 8),
          (1, 4096, 32, 8), (8, 4096, 64, 8))
CONDITIONS = ((64, 4096, 32), (1, 4096, 32))


def make(n, L, Hq, Hkv, dev):
    kc = (torch.randn(n, L, Hkv, D, device=dev) * 0.5).bfloat16()
    vc = (torch.randn(n, L, Hkv, D, device=dev) * 0.5).bfloat16()
    k8, ke = ops.kv_quantize(kc)
    v8, ve = ops.kv_quantize(vc)
    qkv = torch.randn(n, (Hq + 2 * Hkv) * D, device=dev).bfloat16()
    half = D // 2
    fr = torch.outer(torch.arange(L, device=dev).float(),
                     1.0 / 500000.0 ** (torch.arange(half, device=dev).float()
                                        / half))
    tail = (fr.cos().contiguous(), fr.sin().contiguous(),
            torch.full((n,), L - 1, dtype=torch.int32, device=dev),
            torch.full((n,), L, dtype=torch.int32, device=dev),
            torch.arange(n, dtype=torch.int32, device=dev), Hq, Hkv,
            D ** -0.5)
    return {False: (qkv, kc, vc) + tail, True: (qkv, k8, v8, ke, ve) + tail}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--split-sweep", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C = ops.native()
    torch.manual_seed(0)
    ok = True
    for n, L, Hq, Hkv in SHAPES:
        a = make(n, L, Hq, Hkv, dev)
        for fp8 in (False, True):
            parent = C.attn_decode_qkv_fp8 if fp8 else C.attn_decode_qkv
            new = C.attn_decode_qkv_gqa_fp8 if fp8 else C.attn_decode_qkv_gqa
            base_fn = lambda: parent(*a[fp8])
            new_fn = lambda: new(*a[fp8])
            diff = (base_fn().float() - new_fn().float()).abs().max().item()
            tb, tn, tr = compare(base_fn, new_fn, args.rounds, args.window)
            mb, mn = statistics.median(tb + tr), statistics.median(tn)
            spread = max(tb + tr) - min(tb + tr)
            by = kv_bytes(n * L, Hkv, fp8)
            tag = (f"n={n} kv={L} Hq={Hq} Hkv={Hkv} "
                   f"{'fp8' if fp8 else 'bf16'}")
            print(f"{tag}: per-head {mb*1e6:8.1f} us ({by/mb/1e12:5.2f} TB/s)"
                  f"  grouped {mn*1e6:8.1f} us ({by/mn/1e12:5.2f} TB/s)  "
                  f"x{mb/mn:5.2f}  parent spread {spread*1e6:6.1f} us  "
                  f"max |diff| {diff:.2e}", flush=True)
            if (n, L, Hq) in CONDITIONS:
                held = mn < mb - spread
                ok = ok and held
                print(f"  condition: grouped median below the parent's by "
                      f"more than its spread: {'holds' if held else 'FAILS'}")
            if args.split_sweep and (n, L, Hq) in CONDITIONS:
                for R in (128, 256, 512):
                    fn = lambda: new(*a[fp8], R)
                    it = calibrate(fn, args.window)
                    t = statistics.median(window(fn, it) for _ in range(3))
                    print(f"  split_rows {R:4d}: {t*1e6:8.1f} us", flush=True)
        del a
    print("conditions:", "hold" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
