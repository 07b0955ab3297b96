#!/usr/bin/env python3
"""Cost of the decode penalties (docs/KERNELS.md "Decode penalties").

Default: kernel times of ops.penalize_logits on [1, 128256] and
[64, 128256] bf16 logits, for off rows (the copy alone) and for
histories of 128, 1,024 and 4,096 tokens, next to a same-size copy_.
Device events around --launches back-to-back launches, --rounds rounds
with the variants interleaved in one process; prints the median and the
minimum per launch.  The logits stay in cache between launches, as they
do in the decode graph, where the lm-head GEMV has just written them.

--engine MODEL: greedy decode tok/s of the serving engine at --streams
concurrent requests for penalties=False, penalties=True with no request
using them, and penalties=True with every request using them; --repeats
rounds with the three cases alternating, so the spread of one case is
on the page next to the differences between them."""
from __future__ import annotations

import argparse
import statistics
import threading
import time

import torch

from skypilot_amd import ops

HISTORIES = (128, 1024, 4096)


def kernel_times(args):
    dev = "cuda"
    V = args.vocab
    for b in [int(x) for x in args.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(b)
        logits = (torch.randn(b, V, device=dev, generator=g) * 4).bfloat16()
        out = torch.empty_like(logits)
        cnt = ops.penalty_workspace(b, V, dev)
        s_max = max(HISTORIES)
        # tokens drawn like a model's output: a few hundred frequent ids
        hist = torch.randint(0, V, (b, s_max), device=dev, generator=g,
                             dtype=torch.int32)
        hist[:, ::2] = torch.randint(0, 300, (b, s_max // 2), device=dev,
                                     generator=g, dtype=torch.int32)
        slot = torch.arange(b, dtype=torch.int32, device=dev)
        tok = torch.zeros(b, dtype=torch.int32, device=dev)
        plen = torch.full((b,), 64, dtype=torch.int32, device=dev)

        def f32(v):
            return torch.full((b,), v, dtype=torch.float32, device=dev)

        def variant(p, alpha, beta, rho):
            pos = torch.full((b,), p, dtype=torch.int32, device=dev)
            pars = (f32(alpha), f32(beta), f32(rho))
            return lambda: ops.penalize_logits(
                logits, out, hist, cnt, tok, pos, slot, plen, *pars)

        variants = {"copy_": lambda: out.copy_(logits),
                    "penalize off rows": variant(0, 0.0, 0.0, 1.0)}
        for h in HISTORIES:
            variants[f"penalize history {h}"] = variant(h - 1, 0.5, 0.3, 1.2)
        times = {k: [] for k in variants}
        for fn in variants.values():     # warm up every variant
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in variants.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(
                    e0.elapsed_time(e1) * 1e3 / args.launches)
        assert not cnt.view(torch.int32).any()
        base = statistics.median(times["copy_"])
        print(f"logits [{b}, {V}] bf16, us per launch "
              f"(median / min of {args.rounds} x {args.launches}):")
        for name, ts in times.items():
            med = statistics.median(ts)
            print(f"  {name:26s} {med:8.1f} / {min(ts):8.1f}   "
                  f"{med / base:5.2f}x copy_", flush=True)


def engine_rates(args):
    from skypilot_amd.serve.engine import Engine, Request
    streams = [int(x) for x in args.streams.split(",")]
    prompt = list(range(2, 2 + args.prompt_len))
    cases = {"penalties=False": (False, {}),
             "penalties=True, unused": (True, {}),
             "penalties=True, every request": (
                 True, dict(frequency_penalty=0.5, presence_penalty=0.2,
                            repetition_penalty=1.1))}
    engines, model = {}, None
    for name, (on, _) in cases.items():
        engines[name] = Engine(args.model, device="cuda:0", max_seq=4096,
                               max_batch=max(streams), model=model,
                               hbm_budget_gb=None, penalties=on)
        model = engines[name].model    # one set of weights for all three
    rates = {(name, nb): [] for name in cases for nb in streams}
    for eng in engines.values():    # the idle ones only poll their queue
        eng.start()
    for rep in range(args.repeats + 1):     # round 0 warms up and captures
        for name, (_, kw) in cases.items():
            eng = engines[name]
            for nb in streams:
                reqs = [Request(prompt_ids=list(prompt),
                                max_tokens=args.gen_len, **kw)
                        for _ in range(nb)]
                t0 = time.perf_counter()
                threads = [threading.Thread(
                    target=lambda r=r: eng.submit(r).done.wait(1200))
                    for r in reqs]
                for t in threads:
                    t.start()
                for t in threads:
                    t.join()
                dt = time.perf_counter() - t0
                if rep:
                    rates[name, nb].append(
                        sum(len(r.out_ids) for r in reqs) / dt)
    for eng in engines.values():
        eng.stop()
    print(f"{args.model} greedy decode tok/s, prompt {args.prompt_len}, "
          f"{args.gen_len} tokens per request "
          f"(median, min..max of {args.repeats}):")
    for (name, nb), rs in rates.items():
        print(f"  {name:30s} {nb:3d} streams  {statistics.median(rs):9.1f}  "
              f"{min(rs):9.1f} .. {max(rs):9.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--engine", dest="model", default=None, metavar="MODEL")
    ap.add_argument("--streams", default="1,64")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_penalties.py needs a GPU")
    if args.model:
        engine_rates(args)
    else:
        kernel_times(args)


if __name__ == "__main__":
    main()
