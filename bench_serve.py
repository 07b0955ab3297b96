#!/usr/bin/env python3
"""Serving throughput bench: continuous-batching decode tokens/s for the
bundled Llama engine on one MI355X (the per-replica number behind
BASELINE config 4).  --prefill-chunk turns on chunked prefill;
--stall-prompts adds the probe of what a running stream sees when long
prompts arrive mid-decode."""
from __future__ import annotations

import argparse
import threading
import time

import torch


def stall_probe(eng, prompt, args):
    """One short-prompt stream decodes; once it has 32 tokens,
    --stall-prompts long prompts arrive together.  Reports the stream's
    largest gap between consecutive tokens before and after the arrival
    (tokens reach the host in groups while chained graph replays run, so
    the gap before the arrival is one such group, not one token)."""
    import queue

    from skypilot_amd.serve.engine import Request
    # warm the decode graph bucket the stream shares with the newcomers
    warm = [eng.submit(Request(prompt_ids=[2, 3, 4], max_tokens=8))
            for _ in range(args.stall_prompts + 1)]
    for r in warm:
        r.done.wait(600)
    q = queue.Queue()
    stream = eng.submit(Request(prompt_ids=[2, 3, 4, 5], max_tokens=512,
                                stream_queue=q))
    stamps, arrival, late = [], None, []
    while True:
        tok = q.get(timeout=600)
        if tok is None:
            break
        stamps.append(time.perf_counter())
        if len(stamps) == 32:
            arrival = stamps[-1]
            late = [eng.submit(Request(prompt_ids=list(prompt),
                                       max_tokens=8))
                    for _ in range(args.stall_prompts)]
    for r in late:
        r.done.wait(600)
    gaps = [(b - a, b) for a, b in zip(stamps, stamps[1:])]
    before = max(g for g, t in gaps if t <= arrival)
    after = max(g for g, t in gaps if t > arrival)
    ttft = sorted(r.first_token_at - r.created for r in late)
    print(f"stall probe: {args.stall_prompts} x {args.prompt_len}-token "
          f"prompts arrive mid-stream (prefill_chunk "
          f"{args.prefill_chunk}): running stream's max inter-token gap "
          f"{before*1e3:6.1f} ms before, {after*1e3:6.1f} ms after; "
          f"newcomers' ttft p50 {ttft[len(ttft)//2]*1e3:6.1f} ms "
          f"({len(stream.out_ids)} stream tokens)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=128)
    ap.add_argument("--batches", default="1,8,32,64")
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--fp8", action="store_true",
                    help="rowwise e4m3fn decode weights")
    ap.add_argument("--prefill-chunk", type=int, default=None,
                    help="chunked prefill: tokens per append forward "
                         "(multiple of 64); default whole-prompt prefill")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--seed", type=int, default=None,
                    help="request i of a batch uses seed + i")
    ap.add_argument("--device-sampling", action="store_true",
                    help="sample in the decode graph instead of on the host")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="KV cache format (fp8: e4m3fn rows with "
                         "power-of-two row scales)")
    ap.add_argument("--stall-prompts", type=int, default=0,
                    help="after the batches, also measure what a running "
                         "stream sees when this many --prompt-len prompts "
                         "arrive mid-decode (largest inter-token gap)")
    args = ap.parse_args()
    if ((args.top_k > 0 or args.seed is not None)
            and not args.device_sampling):
        ap.error("--top-k and --seed need --device-sampling")

    from skypilot_amd.serve.engine import Engine
    eng = Engine(args.model,
                 device="cuda:0" if torch.cuda.is_available() else "cpu",
                 max_seq=4096, max_batch=args.max_batch,
                 prefill_chunk=args.prefill_chunk,
                 device_sampling=args.device_sampling,
                 kv_dtype=args.kv_dtype)
    print(f"kv_dtype={args.kv_dtype} max_batch={eng.max_batch} "
          f"kv_cache_bytes={eng.cache.bytes_needed(eng.cfg, eng.cache.max_batch, eng.max_seq, args.kv_dtype)}")
    if args.fp8:
        print(f"fp8 decode weights: {eng.enable_fp8_decode()} tensors")
    eng.start()
    prompt = list(range(2, 2 + args.prompt_len))
    # warmup
    eng.generate(prompt, max_tokens=8)

    from skypilot_amd.serve.engine import Request
    for nb in [int(x) for x in args.batches.split(",")]:
        results = []
        ttfts = []
        t0 = time.perf_counter()

        def worker(i):
            req = eng.submit(Request(
                prompt_ids=list(prompt), max_tokens=args.gen_len,
                temperature=args.temperature, top_p=args.top_p,
                top_k=args.top_k,
                seed=None if args.seed is None else args.seed + i))
            req.done.wait(1200)
            results.append(len(req.out_ids))
            if req.first_token_at:
                ttfts.append(req.first_token_at - req.created)

        threads = [threading.Thread(target=worker, args=(i,))
                   for i in range(nb)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        dt = time.perf_counter() - t0
        toks = sum(results)
        ttfts.sort()
        p50 = ttfts[len(ttfts) // 2] * 1e3 if ttfts else 0
        p95 = ttfts[int(len(ttfts) * 0.95)] * 1e3 if ttfts else 0
        print(f"concurrency {nb:3d}: {toks} tokens in {dt:6.2f}s = "
              f"{toks/dt:8.1f} tok/s decode | ttft p50 {p50:6.1f} ms "
              f"p95 {p95:6.1f} ms (prompt {args.prompt_len}, "
              f"prefill_chunk {args.prefill_chunk}, temperature "
              f"{args.temperature}, top_p {args.top_p}, top_k "
              f"{args.top_k}, device_sampling {args.device_sampling})",
              flush=True)
    if args.stall_prompts:
        stall_probe(eng, prompt, args)
    print(f"graph buckets captured: {eng.stats['graph_buckets']} "
          f"(use_graphs={eng.use_graphs})")
    eng.stop()


if __name__ == "__main__":
    main()
