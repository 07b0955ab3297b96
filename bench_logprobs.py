#!/usr/bin/env python3
"""Token log-probabilities: kernel times and their cost in the graphed
decode step.

Kernel part: ops.token_logprobs with N in {0, 5, 20} on [1, 128256],
[64, 128256] and [1, 152064] bf16 logits, and for scale
ops.sample_tokens in top-k + top-p mode on the same logits.  Device
events around --launches back-to-back launches, --rounds rounds with the
variants interleaved in one process; prints the median and the spread
(min .. max) per launch.  The logits stay in cache between launches, as
they do in the decode graph, where the lm-head GEMV has just written
them.

Engine part (--model, default llama3-8b; "none" skips it): the graphed
single-stream greedy decode step in three configurations that share one
set of weights: max_logprobs=0; max_logprobs=20 with a request that does
not ask; max_logprobs=20 with a request that asks for 20.  Time per
token is (finished_at - first_token_at) / (tokens - 1) of one request,
--rounds requests per configuration, interleaved."""
from __future__ import annotations

import argparse
import statistics

import torch

from skypilot_amd import ops

SHAPES = [(1, 128256), (64, 128256), (1, 152064)]
NS = [0, 5, 20]


def _spread(ts):
    return (f"{statistics.median(ts):8.1f}   ({min(ts):.1f} .. "
            f"{max(ts):.1f})")


def bench_kernels(launches: int, rounds: int) -> None:
    dev = "cuda"
    C = ops.native()
    for b, V in SHAPES:
        g = torch.Generator(device=dev).manual_seed(b)
        logits = (torch.randn(b, V, device=dev, generator=g) * 4).bfloat16()
        ids = torch.randint(0, V, (b,), device=dev, generator=g)
        out = (torch.empty(b, device=dev),
               torch.empty(b, ops.LOGPROB_TOP, device=dev),
               torch.empty(b, ops.LOGPROB_TOP, dtype=torch.int32,
                           device=dev))
        variants = {}
        for N in NS:
            n_top = torch.full((b,), N, dtype=torch.int32, device=dev)
            variants[f"token_logprobs N={N}"] = (
                lambda n_top=n_top: C.token_logprobs(logits, ids, n_top,
                                                     *out))
        blk = ops.pack_samp(b, 0.8, 0.9, 40, list(range(b))).to(dev)
        samp, cnt = blk[:5].contiguous(), blk[5].contiguous()
        variants["sample_tokens top_k 40 + top_p 0.9"] = (
            lambda: C.sample_tokens(logits, samp, cnt))
        times = {k: [] for k in variants}
        for fn in variants.values():     # warm up every variant
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in variants.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / launches)
        print(f"logits [{b}, {V}] bf16, us per launch: median (min .. max) "
              f"of {rounds} x {launches}")
        for name, ts in times.items():
            print(f"  {name:38s} {_spread(ts)}", flush=True)


def bench_engine(model_name: str, tokens: int, rounds: int) -> None:
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model(model_name, device="cuda", dtype=torch.bfloat16)
    configs = {
        "max_logprobs=0": (0, None),
        "max_logprobs=20, not asked": (20, None),
        "max_logprobs=20, logprobs=20": (20, 20),
    }
    engines = {}
    for name, (mx, _) in configs.items():
        engines[name] = Engine(model_name, device="cuda", max_seq=1024,
                               max_batch=2, model=model, max_logprobs=mx)
        engines[name].start()
    prompt = list(range(1, 33))
    times = {k: [] for k in configs}
    try:
        for rnd in range(rounds + 1):    # round 0 captures and warms up
            for name, (_, ask) in configs.items():
                r = engines[name].submit(Request(
                    prompt_ids=prompt, max_tokens=tokens, logprobs=ask))
                assert r.done.wait(600)
                assert len(r.out_ids) == tokens
                assert len(r.out_logprobs) == (tokens if ask else 0)
                if rnd:
                    times[name].append((r.finished_at - r.first_token_at)
                                       * 1e6 / (tokens - 1))
    finally:
        for e in engines.values():
            e.stop()
    print(f"{model_name} graphed single-stream decode, us per token: "
          f"median (min .. max) of {rounds} requests of {tokens} tokens")
    for name, ts in times.items():
        print(f"  {name:38s} {_spread(ts)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--tokens", type=int, default=257)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_logprobs needs a GPU"
    bench_kernels(args.launches, args.rounds)
    if args.model != "none":
        bench_engine(args.model, args.tokens, args.rounds)


if __name__ == "__main__":
    main()
