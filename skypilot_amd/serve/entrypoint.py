"""OpenAI-compatible inference entrypoint for the bundled Llama models.

This is the `run:` command of the shipped serving task YAML:

    python -m skypilot_amd.serve.entrypoint --model llama3-8b --port $PORT

Endpoints: /health, /v1/models, /v1/completions, /v1/chat/completions,
/stats.  With no network on the pool there are no pretrained weights or
tokenizer files; the server runs random-init weights with a byte-level
tokenizer (data: synthetic) — the serving bench measures engine/kernel
throughput, not sample quality.  A checkpoint dir produced by the
bundled trainer can be loaded with --checkpoint-dir.
"""
from __future__ import annotations

import argparse
import math
import os
import time
from typing import List, Optional

import uvicorn
from fastapi import FastAPI, HTTPException
from pydantic import BaseModel

from skypilot_amd.serve.engine import Engine, Request


class ByteTokenizer:
    """Byte-level fallback tokenizer (ids 0-255 + BOS=256, EOS=257)."""
    BOS = 256
    EOS = 257

    def encode(self, text: str) -> List[int]:
        return [self.BOS] + list(text.encode("utf-8", errors="replace"))

    def decode(self, ids: List[int]) -> str:
        return bytes(i for i in ids if 0 <= i < 256).decode(
            "utf-8", errors="replace")

    def token(self, i: int) -> str:
        """One token as a string that names it uniquely (the keys of a
        top_logprobs entry): the character for ASCII, ``bytes:\\xNN`` for
        a byte that is no text on its own, ``<|id|>`` for the rest."""
        if 0 <= i < 128:
            return chr(i)
        if i < 256:
            return f"bytes:\\x{i:02x}"
        return f"<|{i}|>"

    def token_bytes(self, i: int) -> List[int]:
        return [i] if 0 <= i < 256 else []


def _num(v: Optional[float]) -> Optional[float]:
    """A log-probability for JSON: -inf and NaN become null."""
    return v if v is not None and math.isfinite(v) else None


class CompletionRequest(BaseModel):
    model: str = ""
    prompt: str = ""
    max_tokens: int = 64
    temperature: float = 0.0
    top_p: float = 1.0
    top_k: int = 0
    seed: Optional[int] = None
    stop: Optional[List[str]] = None
    stream: bool = False
    # number of alternatives per token (0: the chosen token only); needs
    # a server started with --max-logprobs
    logprobs: Optional[int] = None
    # prefix the text with the prompt; with logprobs also score its tokens
    echo: bool = False


class ChatMessage(BaseModel):
    role: str
    content: str


class ChatRequest(BaseModel):
    model: str = ""
    messages: List[ChatMessage] = []
    max_tokens: int = 64
    temperature: float = 0.0
    top_p: float = 1.0
    top_k: int = 0
    seed: Optional[int] = None
    logprobs: bool = False
    top_logprobs: Optional[int] = None


def create_app(engine: Engine, model_name: str) -> FastAPI:
    app = FastAPI(title="skypilot-amd inference")
    tok = ByteTokenizer()

    @app.get("/health")
    def health():
        return {"ok": True, "model": model_name,
                "max_batch": engine.max_batch}

    @app.get("/stats")
    def stats():
        return {**engine.stats, "active": len(engine.active),
                "free_slots": len(engine.free_slots)}

    @app.get("/v1/models")
    def models():
        return {"object": "list",
                "data": [{"id": model_name, "object": "model"}]}

    def _complete(prompt: str, req, logprobs=None, prompt_logprobs=False):
        ids = tok.encode(prompt)
        t0 = time.time()
        r = Request(prompt_ids=ids, max_tokens=req.max_tokens,
                    temperature=req.temperature, top_p=req.top_p,
                    top_k=req.top_k, seed=req.seed, logprobs=logprobs,
                    prompt_logprobs=prompt_logprobs)
        try:
            engine.submit(r)
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        if not r.done.wait(300.0):
            raise HTTPException(status_code=504,
                                detail="generation timed out")
        # r.seed: the seed the device sampler used (None on the host path)
        return r, time.time() - t0

    def _top_dict(top):
        # value-descending; ids are distinct, and so are their names
        return {tok.token(t): _num(v) for t, v in top}

    def _completion_logprobs(r, n_out: int, echo: bool):
        """The `logprobs` object of /v1/completions for the first n_out
        generated tokens, after the prompt's when `echo`.  Prompt tokens
        carry their own log-probability (null for the first) and no
        alternatives."""
        ids = list(r.out_ids[:n_out])
        lps = [_num(v) for v in r.out_logprobs[:n_out]]
        tops = [_top_dict(t) for t in r.out_top[:n_out]]
        if echo:
            ids = list(r.prompt_ids) + ids
            lps = [_num(v) for v in r.prompt_lps] + lps
            tops = [None] * len(r.prompt_ids) + tops
        return {"tokens": [tok.token(i) for i in ids],
                "token_logprobs": lps, "top_logprobs": tops,
                "text_offset": [len(tok.decode(ids[:k]))
                                for k in range(len(ids))]}

    @app.post("/v1/completions")
    def completions(req: CompletionRequest):
        if req.stream:
            import json as _json
            import queue as _queue

            from fastapi.responses import StreamingResponse
            from skypilot_amd.serve.engine import Request as _Req
            q = _queue.Queue()
            r = _Req(prompt_ids=tok.encode(req.prompt),
                     max_tokens=req.max_tokens,
                     temperature=req.temperature, top_p=req.top_p,
                     top_k=req.top_k, seed=req.seed, stream_queue=q,
                     logprobs=req.logprobs)
            try:
                engine.submit(r)
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))

            def sse():
                k = 0  # index of the token in r.out_ids
                while True:
                    item = q.get(timeout=600)
                    if item is None:
                        yield "data: [DONE]\n\n"
                        return
                    choice = {"index": 0, "text": tok.decode([item]),
                              "finish_reason": None}
                    if req.logprobs is not None:
                        # the engine appends a token's entry before it
                        # queues the token
                        choice["logprobs"] = {
                            "tokens": [tok.token(item)],
                            "token_logprobs": [_num(r.out_logprobs[k])],
                            "top_logprobs": [_top_dict(r.out_top[k])],
                            "text_offset": [len(tok.decode(r.out_ids[:k]))]}
                    k += 1
                    chunk = {"id": "cmpl-local",
                             "object": "text_completion",
                             "model": model_name,
                             "choices": [choice]}
                    yield f"data: {_json.dumps(chunk)}\n\n"

            return StreamingResponse(sse(), media_type="text/event-stream")
        r, dt = _complete(
            req.prompt, req, logprobs=req.logprobs,
            prompt_logprobs=req.echo and req.logprobs is not None)
        out, n_prompt, seed = r.out_ids, len(r.prompt_ids), r.seed
        text = tok.decode(out)
        finish = "length"
        n_kept = len(out)
        for stop in req.stop or []:
            i = text.find(stop)
            if i >= 0:
                text = text[:i]
                finish = "stop"
                # the tokens whose text survives: those that begin
                # before the cut
                n_kept = sum(len(tok.decode(out[:k])) < i
                             for k in range(len(out)))
                break
        choice = {"index": 0, "text": text, "finish_reason": finish}
        if req.echo:
            choice["text"] = tok.decode(r.prompt_ids) + text
        if req.logprobs is not None:
            choice["logprobs"] = _completion_logprobs(r, n_kept, req.echo)
        return {
            "id": "cmpl-local", "object": "text_completion",
            "model": model_name, "seed": seed,
            "choices": [choice],
            "usage": {"prompt_tokens": n_prompt,
                      "completion_tokens": len(out),
                      "total_tokens": n_prompt + len(out),
                      "latency_s": dt},
        }

    @app.post("/v1/chat/completions")
    def chat(req: ChatRequest):
        prompt = "\n".join(f"{m.role}: {m.content}" for m in req.messages)
        if req.top_logprobs is not None and not req.logprobs:
            raise HTTPException(status_code=400,
                                detail="top_logprobs needs logprobs: true")
        r, dt = _complete(
            prompt, req,
            logprobs=(req.top_logprobs or 0) if req.logprobs else None)
        out, n_prompt, seed = r.out_ids, len(r.prompt_ids), r.seed
        choice = {"index": 0,
                  "message": {"role": "assistant",
                              "content": tok.decode(out)},
                  "finish_reason": "length"}
        if req.logprobs:
            def entry(t, v):
                return {"token": tok.token(t), "logprob": _num(v),
                        "bytes": tok.token_bytes(t)}
            choice["logprobs"] = {"content": [
                {**entry(t, v), "top_logprobs": [entry(*p) for p in top]}
                for t, v, top in zip(out, r.out_logprobs, r.out_top)]}
        return {
            "id": "chatcmpl-local", "object": "chat.completion",
            "model": model_name, "seed": seed,
            "choices": [choice],
            "usage": {"prompt_tokens": n_prompt,
                      "completion_tokens": len(out),
                      "total_tokens": n_prompt + len(out),
                      "latency_s": dt},
        }

    return app


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--port", type=int,
                    default=int(os.environ.get("PORT", 8000)))
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--max-seq", type=int, default=4096)
    ap.add_argument("--max-batch", type=int, default=None)
    ap.add_argument("--prefill-chunk", type=int, default=None,
                    help="prefill prompts in chunks of this many tokens "
                         "(a multiple of 64) between decode steps, so a "
                         "long prompt does not stall running streams; "
                         "default: whole-prompt prefill")
    ap.add_argument("--device-sampling", action="store_true",
                    help="draw tokens with the seeded sampling kernel "
                         "(needed for top_k and seed; sampled requests "
                         "chain graph replays like greedy ones)")
    ap.add_argument("--max-logprobs", type=int, default=0,
                    help="let requests ask for token log-probabilities "
                         "with up to this many alternatives per token "
                         "(at most 20); 0, the default, leaves them off")
    ap.add_argument("--device", default=None)
    ap.add_argument("--fp8-decode", action="store_true",
                    help="quantize weights to rowwise e4m3fn for the "
                         "decode GEMVs (~2x single-stream decode)")
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel degree; run under torchrun "
                         "with one rank per GPU (70B serving: --tp 8)")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16",
                    help="KV cache format: fp8 stores e4m3fn rows with "
                         "power-of-two row scales (about half the cache "
                         "bytes: twice the slots or context, half the "
                         "decode-attention traffic)")
    return ap


def main():
    args = build_parser().parse_args()
    if args.tp > 1:
        # TP serving (BASELINE config 5's serve twin): every rank builds
        # its shard; rank 0 leads (scheduler + HTTP), others follow the
        # broadcast step plan.  Launched by the gang driver as
        # torchrun --nproc-per-node TP ... --tp TP.
        import torch
        import torch.distributed as dist
        from skypilot_amd.parallel.tp import build_tp_model
        rank = int(os.environ.get("RANK", "0"))
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        if not dist.is_initialized():
            dist.init_process_group(backend)
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
        device = args.device or (
            f"cuda:{int(os.environ.get('LOCAL_RANK', rank))}"
            if torch.cuda.is_available() else "cpu")
        shard = build_tp_model(args.model, tp=args.tp, rank=rank,
                               device=device)
        engine = Engine(args.model, device=device, max_seq=args.max_seq,
                        max_batch=args.max_batch, model=shard,
                        tp_rank=rank, tp_world=args.tp,
                        prefill_chunk=args.prefill_chunk,
                        device_sampling=args.device_sampling,
                        kv_dtype=args.kv_dtype,
                        max_logprobs=args.max_logprobs)
        if args.fp8_decode:
            engine.enable_fp8_decode()
        if rank > 0:
            engine.follower_loop()
            return
        engine.start()
        app = create_app(engine, args.model)
        print(f"serving {args.model} tp={args.tp} on "
              f"{args.host}:{args.port} (max_batch={engine.max_batch})",
              flush=True)
        uvicorn.run(app, host=args.host, port=args.port,
                    log_level="warning")
        return
    engine = Engine(args.model, device=args.device, max_seq=args.max_seq,
                    max_batch=args.max_batch,
                    prefill_chunk=args.prefill_chunk,
                    device_sampling=args.device_sampling,
                    kv_dtype=args.kv_dtype,
                        max_logprobs=args.max_logprobs)
    if args.fp8_decode:
        n8 = engine.enable_fp8_decode()
        print(f"fp8 decode weights: {n8} tensors quantized", flush=True)
    engine.start()
    app = create_app(engine, args.model)
    print(f"serving {args.model} on {args.host}:{args.port} "
          f"(max_batch={engine.max_batch})", flush=True)
    uvicorn.run(app, host=args.host, port=args.port, log_level="warning")


if __name__ == "__main__":
    main()
