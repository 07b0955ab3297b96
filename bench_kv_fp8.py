#!/usr/bin/env python3
"""FP8 KV-cache kernel bench on one MI355X (docs/BENCHMARKS.md, "FP8 KV
cache").

1. Decode attention: attn_decode_qkv (bf16 cache) vs attn_decode_qkv_fp8,
   Hq 32 / Hkv 8, (n, kv_len) in (64, 4096), (64, 1024), (8, 4096),
   (1, 4096).  K/V bytes per second from the shapes.
2. Append attention: attn_append vs attn_append_fp8 at
   bench_attn_append.py's two shapes.
3. kv_write_fp8 at [16, 512, 8, 128] beside the bf16 slice copies it
   replaces.
4. --logits: |delta logit| between an fp8-cache and a bf16-cache run of the
   debug model over 64 teacher-forced decode steps.

Timing: device events around a window of back-to-back launches, sized after
a warm-up so that it lasts at least --window seconds; the versions alternate
inside each round (bf16, fp8, bf16 again), and the second bf16 window shows
the spread a difference has to beat.
"""
from __future__ import annotations

import argparse
import statistics

import torch

from skypilot_amd import ops

D = 128


def window(fn, iters):
    """Seconds per call over one window of `iters` calls (device events)."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / iters


def calibrate(fn, seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = window(fn, 5)
    return max(5, int(seconds / t) + 1)


def compare(base, new, rounds, seconds):
    """Alternating rounds -> (base times, new times, base repeat times)."""
    it_b, it_n = calibrate(base, seconds), calibrate(new, seconds)
    tb, tn, tr = [], [], []
    for _ in range(rounds):
        tb.append(window(base, it_b))
        tn.append(window(new, it_n))
        tr.append(window(base, it_b))
    return tb, tn, tr


def report(label, names, times, nbytes):
    tb, tn, tr = times
    mb, mn, mr = (statistics.median(t) for t in times)
    spread = (max(tb + tr) - min(tb + tr)) / mb
    for name, t, m, by in ((names[0], tb, mb, nbytes[0]),
                           (names[1], tn, mn, nbytes[1]),
                           (names[0] + " (repeat)", tr, mr, nbytes[0])):
        print(f"  {name:34s} median {m*1e6:9.1f} us  min {min(t)*1e6:9.1f} "
              f"max {max(t)*1e6:9.1f}  {by/m/1e12:6.3f} TB/s")
    print(f"  {label}: fp8 / bf16 = {mn/mb:6.4f}  (bf16 repeat / bf16 = "
          f"{mr/mb:6.4f}, bf16 spread {spread*100:5.2f} %)")
    return mb, mn, spread


def kv_bytes(rows, Hkv, fp8):
    """K and V bytes of `rows` cache rows: 2 bytes per element, or one
    byte per element plus one exponent byte per (row, kv head)."""
    return 2 * rows * Hkv * (D + 1 if fp8 else 2 * D)


def bench_decode(args, dev):
    C = ops.native()
    Hq, Hkv, scale = 32, 8, D ** -0.5
    ok = True
    for n, L in ((64, 4096), (64, 1024), (8, 4096), (1, 4096)):
        S_max = L
        kc = (torch.randn(n, S_max, Hkv, D, device=dev) * 0.5).bfloat16()
        vc = (torch.randn(n, S_max, Hkv, D, device=dev) * 0.5).bfloat16()
        k8, ke = ops.kv_quantize(kc)      # plain torch, on the device
        v8, ve = ops.kv_quantize(vc)
        qkv = (torch.randn(n, (Hq + 2 * Hkv) * D, device=dev)).bfloat16()
        half = D // 2
        fr = torch.outer(torch.arange(S_max, device=dev).float(),
                         1.0 / 500000.0 ** (torch.arange(
                             half, device=dev).float() / half))
        cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
        pos = torch.full((n,), L - 1, dtype=torch.int32, device=dev)
        lens = torch.full((n,), L, dtype=torch.int32, device=dev)
        slots = torch.arange(n, dtype=torch.int32, device=dev)

        def bf16():
            return C.attn_decode_qkv(qkv, kc, vc, cos, sin, pos, lens, slots,
                                     Hq, Hkv, scale)

        def fp8():
            return C.attn_decode_qkv_fp8(qkv, k8, v8, ke, ve, cos, sin, pos,
                                         lens, slots, Hq, Hkv, scale)

        diff = (bf16().float() - fp8().float()).abs().max().item()
        print(f"decode attention n={n} kv_len={L} Hq={Hq} Hkv={Hkv}: "
              f"max |fp8 - bf16 output| = {diff:.3e}")
        mb, mn, _ = report(
            f"decode ({n}, {L})", ("attn_decode_qkv_kernel",
                                   "attn_decode_qkv_fp8_kernel"),
            compare(bf16, fp8, args.rounds, args.window),
            (kv_bytes(n * L, Hkv, False), kv_bytes(n * L, Hkv, True)))
        if (n, L) == (64, 4096):
            ok = mn <= mb
            print(f"  condition (64, 4096): fp8 median <= bf16 median: "
                  f"{'holds' if ok else 'FAILS'}")
        del kc, vc, k8, v8
    return ok


def bench_append(args, dev):
    C = ops.native()
    n, Hq, Hkv, scale = 2, 32, 8, D ** -0.5

    def i32(vals):
        return torch.tensor(vals, dtype=torch.int32, device=dev)

    for Sq, q_start, S_max in ((4032, 0, 4032), (512, 3584, 4096)):
        q = (torch.randn(n, Sq, Hq, D, device=dev) * 0.5).bfloat16()
        k8, ke = ops.kv_quantize(torch.randn(n, S_max, Hkv, D) * 0.5)
        v8, ve = ops.kv_quantize(torch.randn(n, S_max, Hkv, D) * 0.5)
        kt = ops.kv_dequantize(k8, ke).bfloat16().to(dev)
        vt = ops.kv_dequantize(v8, ve).bfloat16().to(dev)
        k8, ke, v8, ve = (t.to(dev) for t in (k8, ke, v8, ve))
        idx = (i32([0, 1]), i32([q_start] * n), i32([Sq] * n))

        def bf16():
            return C.attn_append(q, kt, vt, *idx, scale)

        def fp8():
            return C.attn_append_fp8(q, k8, v8, ke, ve, *idx, scale)

        same = torch.equal(bf16(), fp8())
        print(f"append attention n={n} Sq={Sq} q_start={q_start} Hq={Hq} "
              f"Hkv={Hkv}: outputs bit-identical: {same}")
        rows = n * (q_start + Sq)
        report(f"append Sq={Sq}", ("attn_append_kernel",
                                   "attn_append_fp8_kernel"),
               compare(bf16, fp8, args.rounds, args.window),
               (kv_bytes(rows, Hkv, False), kv_bytes(rows, Hkv, True)))


def bench_write(args, dev):
    n, S, Hkv, S_max = 16, 512, 8, 1024
    k = (torch.randn(n, S, Hkv, D, device=dev) * 0.5).bfloat16()
    v = (torch.randn(n, S, Hkv, D, device=dev) * 0.5).bfloat16()
    kc = torch.zeros(n, S_max, Hkv, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    k8 = torch.zeros(n, S_max, Hkv, D, dtype=torch.uint8, device=dev)
    v8 = torch.zeros_like(k8)
    ke = torch.zeros(n, S_max, Hkv, dtype=torch.uint8, device=dev)
    ve = torch.zeros_like(ke)
    slots = torch.arange(n, dtype=torch.int32, device=dev)
    starts = torch.full((n,), 100, dtype=torch.int32, device=dev)
    lens = torch.full((n,), S, dtype=torch.int32, device=dev)

    def copies():  # what the bf16 cache does: two slice copies per sequence
        for i in range(n):
            kc[i, 100:100 + S] = k[i]
            vc[i, 100:100 + S] = v[i]

    def write():
        ops.kv_write_fp8(k, v, k8, v8, ke, ve, slots, starts, lens)

    rows = n * S
    print(f"cache write [{n}, {S}, {Hkv}, {D}] (bytes: bf16 read + write)")
    report("kv write", (f"{2 * n} bf16 slice copies", "kv_write_fp8_kernel"),
           compare(copies, write, args.rounds, args.window),
           (2 * kv_bytes(rows, Hkv, False),
            kv_bytes(rows, Hkv, False) + kv_bytes(rows, Hkv, True)))


@torch.no_grad()
def logit_deltas(dev, steps=64):
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import InferenceContext
    from skypilot_amd.serve.kv_cache import KVCache
    model = build_model("llama-debug", device=str(dev)).eval()
    prompt = [(7 * i + 3) % 500 + 1 for i in range(100)]
    L, pad = len(prompt), 128
    toks = torch.zeros(1, pad, dtype=torch.long, device=dev)
    toks[0, :L] = torch.tensor(prompt, device=dev)
    caches = {kd: KVCache(model.cfg, 1, 256, dev, kv_dtype=kd)
              for kd in ("bf16", "fp8")}
    for kd, cache in caches.items():
        first = model(toks, torch.arange(pad, dtype=torch.int32, device=dev),
                      InferenceContext(cache=cache, mode="prefill",
                                       prefill_slots=[0], prefill_lens=[L]))
    tok = int(first[0, L - 1].argmax())
    deltas, agree = [], 0
    for i in range(steps):
        out = {}
        for kd, cache in caches.items():
            p = L + i
            ctx = InferenceContext(
                cache=cache, mode="decode",
                slots=torch.zeros(1, dtype=torch.long, device=dev),
                pos=torch.tensor([p], device=dev),
                kv_lens=torch.tensor([p + 1], dtype=torch.int32, device=dev),
                slot_ids_i32=torch.zeros(1, dtype=torch.int32, device=dev))
            out[kd] = model(torch.tensor([[tok]], device=dev),
                            torch.tensor([p], dtype=torch.int32, device=dev),
                            ctx)[0, 0].float()
        deltas.append((out["fp8"] - out["bf16"]).abs())
        agree += int(out["fp8"].argmax() == out["bf16"].argmax())
        tok = int(out["bf16"].argmax())     # teacher forcing: bf16's token
    d = torch.stack(deltas)
    scale = out["bf16"].abs().mean().item()
    print(f"llama-debug, {steps} decode steps after a {L}-token prompt, fp8 "
          f"vs bf16 KV cache: mean |delta logit| = {d.mean().item():.4e}, "
          f"max = {d.max().item():.4e} (mean |logit| {scale:.3f}); argmax "
          f"agrees on {agree}/{steps} steps")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5,
                    help="least seconds per timed window")
    ap.add_argument("--only", default="decode,append,write,logits")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    what = args.only.split(",")
    ok = True
    if "decode" in what:
        ok = bench_decode(args, dev)
    if "append" in what:
        bench_append(args, dev)
    if "write" in what:
        bench_write(args, dev)
    if "logits" in what:
        logit_deltas(dev)
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
