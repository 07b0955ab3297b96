#!/usr/bin/env python3
"""Multi-token verify attention and speculative decoding bench on one MI355X
(docs/BENCHMARKS.md, "Speculative decoding").

Kernel: ops.attn_verify at n in {1, 8, 64}, kv length 4096, Hq 32 / Hkv 8,
T in {2, 4, 8}, against the two ways the project could serve the same
tokens before: (a) ops.attn_append on the T tokens padded to a 64-row
chunk, (b) T calls of the grouped decode kernel, one per token.  Timing as
bench_kv_fp8.py: device events around windows of back-to-back launches of
at least --window seconds, the three candidates alternating for --rounds
rounds; medians, and the verify kernel's spread over its windows.

End to end (--e2e, llama3-8b with random weights, one stream, greedy):
tokens per second of Engine(), of Engine(speculative=4) with an oracle
drafter that proposes what the plain engine produced, and with ngram_draft.
The wall clock runs from submit to completion, after a warm-up request has
captured the graphs; accepted / drafted is printed beside each rate, since
the rate of a speculative engine is that of its drafts.
"""
from __future__ import annotations

import argparse
import statistics
import time

import torch

from bench_kv_fp8 import calibrate, kv_bytes, window
from skypilot_amd import ops

D = 128
HQ, HKV, KV_LEN = 32, 8, 4096


def make(n, T, dev):
    L = KV_LEN
    kc = (torch.randn(n, L, HKV, D, device=dev) * 0.5).bfloat16()
    vc = (torch.randn(n, L, HKV, D, device=dev) * 0.5).bfloat16()
    slots = torch.arange(n, dtype=torch.int32, device=dev)
    start = torch.full((n,), L - T, dtype=torch.int32, device=dev)
    q = torch.randn(n, T, HQ, D, device=dev).bfloat16()
    q64 = torch.zeros(n, 64, HQ, D, device=dev, dtype=torch.bfloat16)
    q64[:, :T] = q
    lens = torch.full((n,), T, dtype=torch.int32, device=dev)
    half = D // 2
    fr = torch.outer(torch.arange(L, device=dev).float(),
                     1.0 / 500000.0 ** (torch.arange(half, device=dev).float()
                                        / half))
    cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
    qkv = torch.randn(T, n, (HQ + 2 * HKV) * D, device=dev).bfloat16()
    pos = [torch.full((n,), L - T + t, dtype=torch.int32, device=dev)
           for t in range(T)]
    scale = D ** -0.5
    C = ops.native()

    def verify():
        return C.attn_verify(q, kc, vc, slots, start, scale)

    def append():
        return C.attn_append(q64, kc, vc, slots, start, lens, scale)

    kvl = [p + 1 for p in pos]

    def decode_t():
        for t in range(T):
            C.attn_decode_qkv_gqa(qkv[t], kc, vc, cos, sin, pos[t], kvl[t],
                                  slots, HQ, HKV, scale)

    diff = (verify()[:, :T].float() - append()[:, :T].float()).abs().max()
    return verify, append, decode_t, diff.item()


def bench_kernel(args, dev):
    for n in (1, 8, 64):
        for T in (2, 4, 8):
            fns = make(n, T, dev)
            diff = fns[3]
            its = [calibrate(f, args.window) for f in fns[:3]]
            times = [[], [], []]
            for _ in range(args.rounds):
                for i in range(3):
                    times[i].append(window(fns[i], its[i]))
            mv, ma, md = (statistics.median(t) for t in times)
            spread = max(times[0]) - min(times[0])
            by = kv_bytes(n * KV_LEN, HKV, False)
            print(f"n={n:2d} T={T}: verify {mv*1e6:8.1f} us "
                  f"({by/mv/1e12:5.2f} TB/s, spread {spread*1e6:5.1f} us)  "
                  f"append-64 {ma*1e6:8.1f} us (x{ma/mv:5.2f})  "
                  f"{T} x grouped decode {md*1e6:8.1f} us (x{md/mv:5.2f})  "
                  f"max |verify - append| {diff:.2e}", flush=True)
            del fns


def run_engine(model, prompt, max_tokens, **kw):
    from skypilot_amd.serve.engine import Engine, Request
    eng = Engine("llama3-8b", device="cuda:0", max_seq=2048, max_batch=2,
                 model=model, **kw)
    eng.start()
    try:
        out, dt = None, None
        for timed in (False, True):  # the first request captures the graphs
            req = Request(prompt_ids=list(prompt), max_tokens=max_tokens)
            t0 = time.perf_counter()
            eng.submit(req)
            assert req.done.wait(600), "request did not complete"
            torch.cuda.synchronize()
            dt, out = time.perf_counter() - t0, req.out_ids
            if not timed:
                base = dict(eng.stats)
    finally:
        eng.stop()
    stats = {k: eng.stats[k] - base[k]
             for k in ("spec_steps", "spec_drafted", "spec_accepted")}
    return out, len(out) / dt, stats


def bench_e2e(args):
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.speculative import ngram_draft
    model = build_model("llama3-8b", device="cuda:0")
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(0, 128000, (128,), generator=g).tolist()
    want, rate, _ = run_engine(model, prompt, args.tokens)
    print(f"e2e plain:            {rate:7.1f} tok/s (prefill included)",
          flush=True)
    full = prompt + want

    def oracle(ids, k):
        return full[len(ids):len(ids) + k]

    for name, drafter in (("oracle", oracle), ("ngram", ngram_draft)):
        got, r, st = run_engine(model, prompt, args.tokens, speculative=4,
                                drafter=drafter)
        same = sum(a == b for a, b in zip(got, want))
        print(f"e2e speculative=4 {name:6s}: {r:7.1f} tok/s (x{r/rate:4.2f})  "
              f"steps {st['spec_steps']} drafted {st['spec_drafted']} "
              f"accepted {st['spec_accepted']}  tokens equal to plain "
              f"{same}/{len(want)}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--tokens", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    bench_kernel(args, dev)
    if args.e2e:
        bench_e2e(args)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
