"""Inference engine — continuous batching over a slot-based KV cache.

MI355X-native serving core for the bundled OpenAI-compatible entrypoint
(no reference counterpart; SkyPilot points users at vLLM images,
SURVEY.md §2.11).  Prefill runs the causal flash kernel (prompt padded
to the 64-row tile); decode steps batch every active sequence into one
forward through the decode-attention kernel.  max_batch is sized to the
288 GB HBM budget (KVCache.sized_for_memory).

With ``prefill_chunk`` set, prompts are prefilled in chunks of that many
tokens through the append-attention kernel (ops.attn_append), one chunk
forward per loop iteration between decode steps, so a running stream
waits for one chunk and never for a whole prompt.

With ``device_sampling`` set, tokens are drawn by the seeded sampling
kernel (ops.sample_tokens / ops.decode_sample_advance: temperature,
top-k, top-p, a per-request seed) instead of the host's torch sampler:
sampled requests then chain graph replays like greedy ones, and a
request's token at a position depends only on its seed, the position
and the logits.

With ``max_logprobs`` > 0, requests may ask for log-probabilities
(``Request.logprobs`` / ``prompt_logprobs``): the model's raw
distribution, temperature 1 and no filter, whatever the request samples
with (ops.token_logprobs; docs/KERNELS.md "Token log-probabilities").
In the graph path ops.decode_logprobs is captured behind the advance
kernel and its rings are read in the chunk's one sync.
"""
from __future__ import annotations

import math
import os
import queue
import random
import threading
import time
import uuid
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from skypilot_amd import ops
from skypilot_amd.models.llama import build_model
from skypilot_amd.serve.kv_cache import KV_DTYPES, KVCache


@dataclass
class InferenceContext:
    cache: KVCache
    mode: str  # "prefill" | "decode" | "append"
    prefill_slot: int = -1
    prefill_len: int = 0
    # batched prefill: one row per new sequence (all rows share
    # positions 0..pad; rows beyond a sequence's true length are
    # ignored at sampling and never written to the cache)
    prefill_slots: Optional[list] = None
    prefill_lens: Optional[list] = None
    slots: Optional[torch.Tensor] = None        # int64 [n] (decode)
    pos: Optional[torch.Tensor] = None          # int64 [n] write positions
    kv_lens: Optional[torch.Tensor] = None      # int32 [n] incl. new token
    slot_ids_i32: Optional[torch.Tensor] = None  # int32 [n]
    # append (chunked prefill): row i of sequence b is the token at
    # position append_start[b] + i; rows >= append_lens[b] are padding.
    # int32 [n] device tensors for the kernel, host lists for the cache
    # writes.
    append_slots: Optional[torch.Tensor] = None
    append_start: Optional[torch.Tensor] = None
    append_lens: Optional[torch.Tensor] = None
    append_slots_l: Optional[list] = None
    append_start_l: Optional[list] = None
    append_lens_l: Optional[list] = None
    # append: return the logits of every row, [n, sq, V], instead of the
    # last valid row's [n, 1, V] (prompt log-probabilities)
    all_rows: bool = False
    # fp8 cache, whole-prompt prefill: (slots, starts, lens) int32 device
    # tensors of the batch's cache write, built by the first layer
    kv_write_idx: Optional[tuple] = None


@dataclass
class Request:
    prompt_ids: List[int]
    max_tokens: int = 64
    temperature: float = 0.0
    top_p: float = 1.0
    # top_k <= 0 turns the filter off.  top_k and seed need
    # Engine(device_sampling=True): there submit() fills in a random seed
    # when none is given, so a response can report the one that was
    # used; without it submit() rejects a request that sets either.
    top_k: int = 0
    seed: Optional[int] = None
    stop_id: Optional[int] = None
    # Log-probabilities need Engine(max_logprobs=N).  logprobs: how many
    # alternatives per generated token (0: the chosen token only, at most
    # N); prompt_logprobs: also score the prompt's own tokens.
    logprobs: Optional[int] = None
    prompt_logprobs: bool = False
    stream_queue: Optional["queue.Queue"] = None  # per-token streaming
    id: str = field(default_factory=lambda: uuid.uuid4().hex[:12])
    out_ids: List[int] = field(default_factory=list)
    # results, aligned with out_ids: the chosen token's log-probability
    # and the top `logprobs` (id, log-probability) pairs
    out_logprobs: List[float] = field(default_factory=list)
    out_top: List[List[Tuple[int, float]]] = field(default_factory=list)
    # prompt_lps[i]: log-probability of prompt_ids[i] given the tokens
    # before it; entry 0 is None
    prompt_lps: List[Optional[float]] = field(default_factory=list)
    done: threading.Event = field(default_factory=threading.Event)
    created: float = field(default_factory=time.time)
    first_token_at: Optional[float] = None
    finished_at: Optional[float] = None


@dataclass
class _Prefilling:
    """A request whose prompt is being prefilled chunk by chunk."""
    req: Request
    slot: int
    done: int = 0  # prompt tokens already in the cache


class Engine:
    def __init__(self, model_name: str, device: Optional[str] = None,
                 max_seq: int = 4096, max_batch: Optional[int] = None,
                 hbm_budget_gb: Optional[float] = None,
                 use_graphs: bool = True, model=None, tp_group=None,
                 tp_rank: int = 0, tp_world: int = 1,
                 prefill_chunk: Optional[int] = None,
                 device_sampling: bool = False,
                 kv_dtype: str = "bf16", max_logprobs: int = 0):
        # 0 keeps the decode graph and the staged block as they are
        # without the feature; N > 0 adds the log-probability kernel to
        # the graph and lets a request ask for up to N alternatives.
        if (isinstance(max_logprobs, bool)
                or not isinstance(max_logprobs, int)
                or not 0 <= max_logprobs <= ops.LOGPROB_TOP):
            raise ValueError(
                f"max_logprobs must be an int in [0, {ops.LOGPROB_TOP}], "
                f"got {max_logprobs!r}")
        self.max_logprobs = max_logprobs
        # "fp8" stores the KV cache as e4m3fn rows with power-of-two row
        # scales (docs/KERNELS.md "FP8 KV cache"): 129 instead of 256
        # bytes per (token, kv head) row.
        if kv_dtype not in KV_DTYPES:
            raise ValueError(
                f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        # Chunked prefill: None keeps whole-prompt prefills (_prefill).
        # The append kernel tiles the chunk by 64 rows.
        if prefill_chunk is not None and (
                isinstance(prefill_chunk, bool)
                or not isinstance(prefill_chunk, int)
                or prefill_chunk <= 0 or prefill_chunk % 64 != 0):
            raise ValueError(
                "prefill_chunk must be None or a positive multiple of 64, "
                f"got {prefill_chunk!r}")
        self.prefill_chunk = prefill_chunk
        # False keeps the host sampler (_sample: torch's generator, one
        # replay per host sync for sampled batches).
        self.device_sampling = bool(device_sampling)
        self.prefilling: List[_Prefilling] = []
        self.device = torch.device(device or (
            "cuda" if torch.cuda.is_available() else "cpu"))
        dtype = torch.bfloat16
        # Tensor-parallel serving (BASELINE config 5's serve twin): a
        # pre-built TP shard is passed in; rank 0 leads (scheduler +
        # HTTP), ranks > 0 mirror its forwards via broadcast step plans
        # (see follower_loop).  All ranks hold identical activations
        # after each block's all-reduce, so token selection needs no
        # extra communication.
        self.tp_group = tp_group
        self.tp_rank = tp_rank
        # TP participation is EXPLICIT (tp_world > 1): a process may be
        # part of a distributed group for other reasons (e.g. a non-TP
        # engine built alongside) and must not broadcast step plans.
        self.tp_world = tp_world
        if model is not None:
            self.model = model
        else:
            self.model = build_model(model_name, device=str(self.device),
                                     dtype=dtype)
        self.model.eval()
        self.cfg = getattr(self.model, "cfg_shard", self.model.cfg)
        self.max_seq = min(max_seq, self.cfg.max_seq_len)
        if max_batch is None:
            if hbm_budget_gb is None:
                if self.device.type == "cuda":
                    free, total = torch.cuda.mem_get_info(self.device)
                    hbm_budget_gb = (free / 1e9) * 0.8
                else:
                    hbm_budget_gb = 0.5
            self.cache = KVCache.sized_for_memory(
                self.cfg, self.max_seq, int(hbm_budget_gb * 1e9),
                self.device, kv_dtype=kv_dtype)
        else:
            # +1 slot when graphs are on: the graph-padding scratch slot
            # must not cost a unit of serving concurrency.
            extra = 1 if (use_graphs and self.device.type == "cuda") else 0
            self.cache = KVCache(self.cfg, max_batch + extra, self.max_seq,
                                 self.device, kv_dtype=kv_dtype)
        self.max_batch = self.cache.max_batch
        self.free_slots = list(range(self.max_batch))
        self.active: Dict[int, Request] = {}  # slot -> request
        self.pending: "queue.Queue[Request]" = queue.Queue()
        self._stop = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self.stats = {"requests": 0, "tokens_generated": 0,
                      "prefill_tokens": 0, "graph_buckets": []}
        # hipGraph decode: the whole decode forward (~7 kernels/layer +
        # head = ~230 launches for 8B) replays as ONE graph launch per
        # power-of-two batch bucket.  Low-concurrency decode is
        # launch-bound, so this is the serving latency lever.  Padded
        # rows point at a reserved scratch slot so their K/V writes
        # never touch a live sequence.
        self.use_graphs = (use_graphs and self.device.type == "cuda"
                           and self.max_batch >= 2)
        self._graphs: Dict[int, tuple] = {}
        self._scratch_slot = -1
        if self.use_graphs:
            self._scratch_slot = self.free_slots.pop()
            self.max_batch -= 1

    def enable_fp8_decode(self, min_bytes: int = 1 << 20) -> int:
        """Quantize every large linear weight to row-wise e4m3fn and
        route the decode GEMVs through the fp8 kernel (half the streamed
        bytes on the weight-bandwidth-bound decode path; prefill stays
        bf16).  Returns the number of weights registered."""
        from skypilot_amd import ops as _ops
        n = 0
        for name, p in self.model.named_parameters():
            if (p.ndim == 2 and p.dtype == torch.bfloat16
                    and p.numel() * 2 >= min_bytes
                    and p.shape[1] % 1024 == 0
                    and "embed" not in name):
                _ops.register_fp8_weight(p.data)
                n += 1
        # The decode path lazily packs [q|k|v] into a single GEMV weight
        # (models/llama.py _wqkv) that is NOT a named parameter —
        # materialize and register it here too (it is ~10% of the
        # streamed decode bytes).
        for blk in getattr(self.model, "blocks", []):
            a = getattr(blk, "attn", None)
            if a is None or not hasattr(a, "wq"):
                continue
            if getattr(a, "_wqkv", None) is None and a.wq.weight.is_cuda:
                a._wqkv = torch.cat(
                    [a.wq.weight, a.wk.weight, a.wv.weight], dim=0)
            if (getattr(a, "_wqkv", None) is not None
                    and a._wqkv.shape[1] % 1024 == 0):
                _ops.register_fp8_weight(a._wqkv)
                n += 1
        return n

    # ------------------------------------------------------------------
    def submit(self, req: Request) -> Request:
        self._check_sampling(req)
        self._check_logprobs(req)
        if len(req.prompt_ids) >= self.max_seq:
            req.prompt_ids = req.prompt_ids[-(self.max_seq - 1 -
                                              req.max_tokens):]
        self.stats["requests"] += 1
        self.pending.put(req)
        return req

    def _check_sampling(self, req: Request) -> None:
        """Validate and normalise a request's sampling parameters here,
        once, so that everything past submit() — the engine thread, the
        graph's parameter block, the TP plan — sees plain finite floats,
        an int32 top_k and a 63-bit seed.  Raises ValueError."""
        for name in ("temperature", "top_p"):
            v = getattr(req, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            try:
                v = float(v)
            except OverflowError:
                v = math.inf
            if not math.isfinite(v):
                raise ValueError(f"{name} must be finite, got {v!r}")
            setattr(req, name, v)
        if req.temperature < 0:
            raise ValueError(
                f"temperature must be >= 0, got {req.temperature!r}")
        if isinstance(req.top_k, bool) or not isinstance(req.top_k, int):
            raise ValueError(f"top_k must be an int, got {req.top_k!r}")
        # the kernel takes an int32; <= 0 and >= vocabulary both mean off
        req.top_k = max(0, min(req.top_k, 2 ** 31 - 1))
        if req.seed is not None and (isinstance(req.seed, bool)
                                     or not isinstance(req.seed, int)):
            raise ValueError(f"seed must be an int, got {req.seed!r}")
        if not self.device_sampling:
            # the host sampler has neither: refuse rather than drop them
            if req.top_k > 0 or req.seed is not None:
                raise ValueError(
                    "top_k and seed need device sampling "
                    "(Engine(device_sampling=True) / --device-sampling)")
            return
        if req.seed is None:
            req.seed = random.getrandbits(63)
        req.seed %= 1 << 63

    def _check_logprobs(self, req: Request) -> None:
        """Validate a request's log-probability fields against
        max_logprobs.  Raises ValueError."""
        n = req.logprobs
        if n is not None and (isinstance(n, bool) or not isinstance(n, int)
                              or n < 0):
            raise ValueError(
                f"logprobs must be None or an int >= 0, got {n!r}")
        if not isinstance(req.prompt_logprobs, bool):
            raise ValueError("prompt_logprobs must be a bool, got "
                             f"{req.prompt_logprobs!r}")
        if n is None and not req.prompt_logprobs:
            return
        if self.max_logprobs == 0:
            raise ValueError(
                "logprobs and prompt_logprobs need an engine with "
                "log-probabilities on (Engine(max_logprobs=N) / "
                "--max-logprobs N)")
        if n is not None and n > self.max_logprobs:
            raise ValueError(
                f"logprobs = {n} exceeds this engine's max_logprobs = "
                f"{self.max_logprobs}")

    def _record_logprobs(self, logits: torch.Tensor, reqs: List[Request],
                         ids: List[int]) -> None:
        """Append out_logprobs / out_top for the tokens `ids` chosen from
        `logits` [n, V], for the requests that asked: first tokens after
        a prefill and every token of the eager decode step."""
        rows = [i for i, r in enumerate(reqs) if r.logprobs is not None]
        if not rows:
            return
        lp, tlp, tid = ops.token_logprobs(
            logits[rows].contiguous(), [ids[i] for i in rows],
            [reqs[i].logprobs for i in rows])
        lp, tlp, tid = lp.tolist(), tlp.tolist(), tid.tolist()
        for j, i in enumerate(rows):
            self._append_logprobs(reqs[i], lp[j], tid[j], tlp[j])

    @staticmethod
    def _append_logprobs(req: Request, lp: float, top_ids: List[int],
                         top_lps: List[float]) -> None:
        req.out_logprobs.append(lp)
        req.out_top.append([(t, v) for t, v in zip(top_ids, top_lps)
                            if t >= 0][:req.logprobs])

    def _record_prompt_logprobs(self, req: Request, logits: torch.Tensor,
                                ids: List[int]) -> None:
        """Extend req.prompt_lps by the log-probabilities of the prompt
        tokens `ids` under `logits` [len(ids), V], row j being the logits
        of the position before ids[j]."""
        if not req.prompt_lps:
            req.prompt_lps.append(None)
        if ids:
            lp, _, _ = ops.token_logprobs(logits.contiguous(), ids, 0)
            req.prompt_lps.extend(lp.tolist())

    def generate(self, prompt_ids: List[int], max_tokens: int = 64,
                 temperature: float = 0.0,
                 timeout: float = 300.0, top_p: float = 1.0,
                 top_k: int = 0, seed: Optional[int] = None) -> List[int]:
        req = self.submit(Request(prompt_ids=prompt_ids,
                                  max_tokens=max_tokens,
                                  temperature=temperature, top_p=top_p,
                                  top_k=top_k, seed=seed))
        if not req.done.wait(timeout):
            raise TimeoutError("generation timed out")
        return req.out_ids

    def start(self):
        if self._thread is None:
            self._thread = threading.Thread(target=self._loop, daemon=True)
            self._thread.start()

    def stop(self):
        self._stop.set()
        if self._thread is not None:
            self._thread.join(timeout=10)
            self._thread = None
        if self.tp_world > 1 and self.tp_rank == 0:
            self._tp_bcast({"op": "stop"})

    # ------------------------------------------------------------------
    @torch.no_grad()
    def _prefill(self, reqs: List[Request]) -> None:
        """Batched prefill: all admitted prompts run as ONE padded
        causal forward (serial per-prompt prefills dominated the ramp
        at high concurrency: 64 x ~9 ms before the first decode)."""
        n = len(reqs)
        slots = [self.free_slots.pop() for _ in range(n)]
        lens = [len(r.prompt_ids) for r in reqs]
        self._tp_bcast({"op": "prefill", "slots": slots, "lens": lens,
                        "prompts": [r.prompt_ids for r in reqs]})
        pad = (max(lens) + 63) // 64 * 64
        toks = torch.zeros(n, pad, dtype=torch.long, device=self.device)
        for i, r in enumerate(reqs):
            toks[i, :lens[i]] = torch.tensor(r.prompt_ids,
                                             device=self.device)
        positions = torch.arange(pad, dtype=torch.int32,
                                 device=self.device).repeat(n)  # [n*pad]
        ctx = InferenceContext(cache=self.cache, mode="prefill",
                               prefill_slots=slots, prefill_lens=lens)
        logits = self.model(toks, positions, ctx)
        last = logits[torch.arange(n), torch.tensor(lens) - 1]  # [n, V]
        first = self._sample_batch(last, reqs, [l - 1 for l in lens])
        self._record_logprobs(last, reqs, first)
        for i, req in enumerate(reqs):
            if req.prompt_logprobs:
                self._record_prompt_logprobs(
                    req, logits[i, :lens[i] - 1], req.prompt_ids[1:])
        for i, (req, slot) in enumerate(zip(reqs, slots)):
            next_id = first[i]
            self.cache.lens[slot] = lens[i]
            req.out_ids.append(next_id)
            if req.stream_queue is not None:
                req.stream_queue.put(next_id)
            req.first_token_at = time.time()
            self.active[slot] = req
            self.stats["prefill_tokens"] += lens[i]
            self._maybe_finish(slot, req, next_id)

    # -------------------------- chunked prefill ------------------------
    @torch.no_grad()
    def _append_forward(self, slots, starts, lens, chunks,
                        all_rows: bool = False) -> torch.Tensor:
        """One append forward: sequence i adds tokens chunks[i] (lens[i]
        of them) at positions starts[i].. to cache slot slots[i].
        Returns the logits of each sequence's last valid row, [n, 1, V],
        or with `all_rows` those of every row, [n, sq, V].  The leader
        and the TP followers run exactly this; only the leader sets
        all_rows (the lm_head is replicated and follows the last
        collective, so the followers need not)."""
        n = len(slots)
        sq = max(64, (max(lens) + 63) // 64 * 64)
        toks = torch.zeros(n, sq, dtype=torch.long, device=self.device)
        for i, ids in enumerate(chunks):
            toks[i, :lens[i]] = torch.tensor(ids, dtype=torch.long,
                                             device=self.device)

        def i32(vals):
            return torch.tensor(vals, dtype=torch.int32, device=self.device)

        start_t = i32(starts)
        # padding rows stay inside the rope tables
        positions = (start_t[:, None] + torch.arange(
            sq, dtype=torch.int32, device=self.device)[None, :]).clamp_(
                max=self.cfg.max_seq_len - 1).reshape(-1)
        ctx = InferenceContext(
            cache=self.cache, mode="append", append_slots=i32(slots),
            append_start=start_t, append_lens=i32(lens),
            append_slots_l=list(slots), append_start_l=list(starts),
            append_lens_l=list(lens), all_rows=all_rows)
        return self.model(toks, positions, ctx)

    @torch.no_grad()
    def _append_step(self) -> None:
        """Advance up to 16 prefilling requests by one chunk each, in one
        forward; requests whose prompt is now complete sample their first
        token and join the decode set."""
        batch = self.prefilling[:16]
        slots = [e.slot for e in batch]
        starts = [e.done for e in batch]
        lens = [min(self.prefill_chunk, len(e.req.prompt_ids) - e.done)
                for e in batch]
        chunks = [e.req.prompt_ids[s:s + l]
                  for e, s, l in zip(batch, starts, lens)]
        self._tp_bcast({"op": "append", "slots": slots, "starts": starts,
                        "lens": lens, "chunks": chunks})
        all_rows = any(e.req.prompt_logprobs for e in batch)
        logits = self._append_forward(slots, starts, lens, chunks, all_rows)
        ends = [s + l for s, l in zip(starts, lens)]
        if all_rows:
            # Row j of a chunk predicts the prompt token at start + j + 1;
            # the chunk's last valid row predicts the next chunk's first
            # token, or past the prompt the token sampled below.
            for i, e in enumerate(batch):
                if e.req.prompt_logprobs:
                    ids = e.req.prompt_ids[starts[i] + 1:ends[i] + 1]
                    self._record_prompt_logprobs(
                        e.req, logits[i, :len(ids)], ids)
            logits = logits[torch.arange(len(batch)),
                            torch.tensor(lens) - 1].unsqueeze(1)
        fin = [i for i, e in enumerate(batch)
               if ends[i] >= len(e.req.prompt_ids)]
        first = {}
        if fin:
            fin_reqs = [batch[i].req for i in fin]
            fin_ids = self._sample_batch(logits[fin, 0], fin_reqs,
                                         [ends[i] - 1 for i in fin])
            self._record_logprobs(logits[fin, 0], fin_reqs, fin_ids)
            first = dict(zip(fin, fin_ids))
        for i, e in enumerate(batch):
            e.done += lens[i]
            self.stats["prefill_tokens"] += lens[i]
            if e.done < len(e.req.prompt_ids):
                continue
            req, slot = e.req, e.slot
            next_id = first[i]
            self.cache.lens[slot] = e.done
            req.out_ids.append(next_id)
            if req.stream_queue is not None:
                req.stream_queue.put(next_id)
            req.first_token_at = time.time()
            self.active[slot] = req
            self._maybe_finish(slot, req, next_id)
        self.prefilling = [e for e in self.prefilling
                           if e.done < len(e.req.prompt_ids)]

    # -------------------------- hipGraph decode ------------------------
    # Max chained graph replays between host syncs (SKY_DECODE_CHUNK to
    # tune; measured flat 8..32 at 1 stream, so 8 keeps token-streaming
    # latency low).
    CHUNK = int(os.environ.get("SKY_DECODE_CHUNK", "8"))

    def _bucket(self, n: int) -> int:
        b = 1
        while b < n:
            b <<= 1
        return b

    def _get_graph(self, b: int):
        """Lazily capture the decode forward for batch bucket `b`."""
        if b in self._graphs:
            return self._graphs[b]
        dev = self.device
        # All six per-step inputs travel as ONE pinned-host -> device
        # copy of an int32 [6, b] block; the unpack (casts/views) is
        # captured inside the graph.  Rows: 0 toks, 1 positions,
        # 2 slots, 3 pos, 4 kv_lens, 5 slot_i32.  With device sampling
        # the block is [11, b]: rows 6..10 are the sampling parameters
        # (temperature bits, top_p bits, top_k, seed_lo, seed_hi), so
        # they change between replays without a recapture and ride in
        # the same copy.
        # With max_logprobs > 0 one more row at the end holds each
        # sequence's n_top (-1: did not ask, and padding).
        rows = (11 if self.device_sampling else 6) + (
            1 if self.max_logprobs else 0)
        st = {
            "host": torch.zeros(rows, b, dtype=torch.int32,
                                pin_memory=True),
            "block": torch.zeros(rows, b, dtype=torch.int32, device=dev),
        }
        st["stage"] = st["block"][:6]
        st["samp"] = st["block"][6:11 if self.device_sampling else 6]
        if self.max_logprobs:
            st["ntop"] = st["block"][rows - 1]
            st["ntop"].fill_(-1)
        st["stage"][2] = self._scratch_slot
        st["stage"][5] = self._scratch_slot
        st["stage"][4] = 1

        def unpack():
            stg = st["stage"]
            return (stg[0].long().view(b, 1), stg[1],
                    InferenceContext(
                        cache=self.cache, mode="decode",
                        slots=stg[2].long(), pos=stg[3].long(),
                        kv_lens=stg[4], slot_ids_i32=stg[5]))

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warmup on a side stream (autotune etc.)
                toks, positions, ctx = unpack()
                self.model(toks, positions, ctx)
        torch.cuda.current_stream().wait_stream(side)
        st["ring"] = torch.zeros(self.CHUNK, b, dtype=torch.long,
                                 device=dev)
        st["ctr"] = torch.zeros(1, dtype=torch.long, device=dev)
        if self.max_logprobs:
            top = ops.LOGPROB_TOP
            st["lp_ring"] = torch.zeros(self.CHUNK, b, dtype=torch.float32,
                                        device=dev)
            st["top_lp_ring"] = torch.zeros(
                self.CHUNK, b, top, dtype=torch.float32, device=dev)
            st["top_id_ring"] = torch.zeros(
                self.CHUNK, b, top, dtype=torch.int32, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            toks, positions, ctx = unpack()
            st["out"] = self.model(toks, positions, ctx)
            # Self-advancing state: the fused advance kernel does the
            # argmax AND feeds it back into the token stage + bumps
            # positions/pos/kv_lens + stores the token in the ring, so
            # greedy decode replays CHUNK times with zero host work in
            # between (torch's argmax alone measured 43 us/step —
            # profiles/r02_fp8_decode_kernel_stats.txt).  The ctr
            # increment stays a separate captured op so the kernel's
            # ring-row read is ordered before it.
            if self.device_sampling:
                ops.decode_sample_advance(st["out"][:, 0], st["stage"],
                                          st["ring"], st["ctr"],
                                          st["samp"])
            else:
                ops.decode_advance(st["out"][:, 0], st["stage"],
                                   st["ring"], st["ctr"])
            # Log-probabilities of the token just chosen (stage[0]), from
            # the same logits, into ring row ctr % CHUNK: after the
            # advance kernel and before the ctr increment.
            if self.max_logprobs:
                ops.decode_logprobs(st["out"][:, 0], st["stage"],
                                    st["ntop"], st["lp_ring"],
                                    st["top_lp_ring"], st["top_id_ring"],
                                    st["ctr"])
            st["ctr"] += 1
        self._graphs[b] = (g, st)
        self.stats["graph_buckets"] = sorted(self._graphs)
        return self._graphs[b]

    @torch.no_grad()
    def _decode_step(self) -> None:
        slots = sorted(self.active.keys())
        if not slots:
            return
        reqs = [self.active[s] for s in slots]
        n = len(slots)
        lens = [self.cache.lens[s] for s in slots]
        tok_l = [r.out_ids[-1] for r in reqs]
        if self.use_graphs:
            b = self._bucket(n)
            all_greedy = all(r.temperature == 0 for r in reqs)
            # in-graph sampling chains sampled rows like greedy ones
            chain = all_greedy or self.device_sampling
            chunk = 1
            if (chain and self.pending.empty()
                    and not self.prefilling):
                rem = min(r.max_tokens - len(r.out_ids) for r in reqs)
                cap = min(self.max_seq - 2 - l for l in lens)
                chunk = max(1, min(self.CHUNK, rem, cap))
            # TP: the plan must go out BEFORE capture — _get_graph's
            # warmup forwards contain all-reduces that need every rank
            # participating (the follower captures on receipt).
            samp = self._samp_rows(reqs)
            # n_top per row for the in-graph log-probabilities; a batch
            # the host samples from takes them from the logits below
            ntop = None
            if self.max_logprobs:
                ntop = [r.logprobs if chain and r.logprobs is not None
                        else -1 for r in reqs]
            want_lp = ntop is not None and any(v >= 0 for v in ntop)
            self._tp_bcast({"op": "decode", "graph": True, "bucket": b,
                            "slots": slots, "lens": lens, "toks": tok_l,
                            "chunk": chunk, "samp": samp, "ntop": ntop})
            try:
                g, st = self._get_graph(b)
            except Exception as e:  # capture unsupported -> eager forever
                if self.tp_world > 1:
                    raise  # followers already committed to the graph plan
                import sys
                print(f"[engine] hipGraph capture failed, falling back "
                      f"to eager decode: {e!r}", file=sys.stderr)
                self.use_graphs = False
                return self._decode_step()
            self._stage_inputs(st, slots, lens, tok_l, samp, ntop)
            for _ in range(chunk):
                g.replay()
            if chain:
                ring = st["ring"][:chunk, :n].tolist()  # one sync/chunk
                if want_lp:  # same sync: the replays have finished
                    lp_r = st["lp_ring"][:chunk, :n].tolist()
                    tlp_r = st["top_lp_ring"][:chunk, :n].tolist()
                    tid_r = st["top_id_ring"][:chunk, :n].tolist()
                for t in range(chunk):
                    for i, slot in enumerate(slots):
                        if slot not in self.active:  # finished earlier t
                            continue
                        req = self.active[slot]
                        next_id = ring[t][i]
                        self.cache.lens[slot] += 1
                        req.out_ids.append(next_id)
                        if req.logprobs is not None:
                            self._append_logprobs(req, lp_r[t][i],
                                                  tid_r[t][i], tlp_r[t][i])
                        if req.stream_queue is not None:
                            req.stream_queue.put(next_id)
                        self.stats["tokens_generated"] += 1
                        self._maybe_finish(slot, req, next_id)
                return
            logits = st["out"]  # [b, 1, V]
        else:
            self._tp_bcast({"op": "decode", "graph": False,
                            "slots": slots, "lens": lens, "toks": tok_l,
                            "chunk": 1, "samp": self._samp_rows(reqs)})
            toks = torch.tensor([[t] for t in tok_l], dtype=torch.long,
                                device=self.device)
            slots_t = torch.tensor(slots, dtype=torch.long,
                                   device=self.device)
            pos_t = torch.tensor(lens, dtype=torch.long,
                                 device=self.device)
            positions = torch.tensor(lens, dtype=torch.int32,
                                     device=self.device)
            kv_lens = torch.tensor([l + 1 for l in lens],
                                   dtype=torch.int32, device=self.device)
            ctx = InferenceContext(
                cache=self.cache, mode="decode", slots=slots_t, pos=pos_t,
                kv_lens=kv_lens, slot_ids_i32=slots_t.int())
            logits = self.model(toks, positions, ctx)  # [n, 1, V]
        # Device sampling draws the whole batch in one kernel call.  On
        # the host path greedy rows batch into one argmax + one sync and
        # sampled rows (temperature > 0) go through _sample individually.
        # (The chained graph path already returned above.)
        batch_ids = None
        if self.device_sampling:
            # counter = position of each row's input token
            batch_ids = self._sample_batch(logits[:n, 0], reqs, lens)
        elif all(r.temperature == 0 for r in reqs):
            batch_ids = logits[:n, 0].argmax(-1).tolist()
        if batch_ids is None:
            batch_ids = [self._sample(logits[i, 0], r.temperature, r.top_p)
                         for i, r in enumerate(reqs)]
        self._record_logprobs(logits[:n, 0], reqs, batch_ids)
        for i, slot in enumerate(slots):
            self.cache.lens[slot] += 1
            req = self.active[slot]
            next_id = batch_ids[i]
            req.out_ids.append(next_id)
            if req.stream_queue is not None:
                req.stream_queue.put(next_id)
            self.stats["tokens_generated"] += 1
            self._maybe_finish(slot, req, next_id)

    def _samp_rows(self, reqs: List[Request]):
        """Per-row (temperature, top_p, top_k, seed) for the device
        sampler — what the TP decode plan carries; None when off."""
        if not self.device_sampling:
            return None
        return [(r.temperature, r.top_p, r.top_k, r.seed) for r in reqs]

    def _stage_inputs(self, st, slots, lens, tok_l, samp,
                      ntop=None) -> None:
        """Fill the pinned host block for one graph step and start its
        copy to the device (the leader and the TP followers share this).
        Padding rows point at the scratch slot and are greedy."""
        n = len(slots)
        scr = self._scratch_slot
        h = st["host"].numpy()
        h[0, :n] = tok_l
        h[0, n:] = 0
        h[1, :n] = lens
        h[1, n:] = 0
        h[2, :n] = slots
        h[2, n:] = scr
        h[3] = h[1]
        h[4] = h[1] + 1
        h[5] = h[2]
        if self.device_sampling:
            hf = h.view("float32")
            hu = h.view("uint32")
            hf[6, :n] = [r[0] for r in samp]
            hf[7, :n] = [r[1] for r in samp]
            h[8, :n] = [r[2] for r in samp]
            hu[9, :n] = [r[3] & 0xFFFFFFFF for r in samp]
            hu[10, :n] = [r[3] >> 32 for r in samp]
            h[6:, n:] = 0  # temperature 0: padding rows take the argmax
        if self.max_logprobs:
            h[-1, :n] = ntop if ntop is not None else -1
            h[-1, n:] = -1
        st["ctr"].zero_()
        st["block"].copy_(st["host"], non_blocking=True)

    def _sample_batch(self, logits: torch.Tensor, reqs: List[Request],
                      positions: List[int]) -> List[int]:
        """Next token of each request from `logits` [n, V], the logits
        of the tokens at `positions`: first tokens after a prefill and
        every token of the eager decode step."""
        if not self.device_sampling:
            return [self._sample(logits[i], r.temperature, r.top_p)
                    for i, r in enumerate(reqs)]
        toks, _ = ops.sample_tokens(
            logits, [r.temperature for r in reqs],
            [r.top_p for r in reqs], [r.top_k for r in reqs],
            [r.seed for r in reqs], positions)
        return toks.tolist()

    def _sample(self, logits: torch.Tensor, temperature: float,
                top_p: float = 1.0) -> int:
        if temperature and temperature > 0:
            probs = (logits.float() / temperature).softmax(-1)
            if top_p < 1.0:
                sp, idx = probs.sort(descending=True)
                keep = (sp.cumsum(0) - sp) <= top_p
                keep[0] = True
                probs = torch.zeros_like(probs).scatter(
                    0, idx[keep], sp[keep])
                probs = probs / probs.sum()
            return int(torch.multinomial(probs, 1).item())
        return int(logits.argmax().item())

    def _maybe_finish(self, slot: int, req: Request, last_id: int) -> None:
        if (len(req.out_ids) >= req.max_tokens or
                (req.stop_id is not None and last_id == req.stop_id) or
                self.cache.lens[slot] + 1 >= self.max_seq):
            del self.active[slot]
            self.cache.free(slot)
            self.free_slots.append(slot)
            req.finished_at = time.time()
            if req.stream_queue is not None:
                req.stream_queue.put(None)  # end-of-stream marker
            req.done.set()

    # ---------------------- tensor-parallel plumbing -------------------
    def _tp_bcast(self, obj) -> None:
        if self.tp_world > 1 and self.tp_rank == 0:
            dist.broadcast_object_list([obj], src=0, group=self.tp_group)

    def follower_loop(self) -> None:
        """TP rank > 0: execute the leader's broadcast step plan.  The
        follower keeps no scheduler state — every forward's slots/
        lengths/tokens arrive in the plan, and its KV cache stays
        consistent because it runs the identical deterministic
        forwards."""
        assert self.tp_world > 1 and self.tp_rank > 0
        while True:
            lst = [None]
            dist.broadcast_object_list(lst, src=0, group=self.tp_group)
            msg = lst[0]
            if msg["op"] == "stop":
                return
            if msg["op"] == "prefill":
                self._follow_prefill(msg)
            elif msg["op"] == "append":
                self._follow_append(msg)
            else:
                self._follow_decode(msg)

    @torch.no_grad()
    def _follow_prefill(self, msg) -> None:
        slots, lens = msg["slots"], msg["lens"]
        n = len(slots)
        pad = (max(lens) + 63) // 64 * 64
        toks = torch.zeros(n, pad, dtype=torch.long, device=self.device)
        for i, ids in enumerate(msg["prompts"]):
            toks[i, :lens[i]] = torch.tensor(ids, device=self.device)
        positions = torch.arange(pad, dtype=torch.int32,
                                 device=self.device).repeat(n)
        ctx = InferenceContext(cache=self.cache, mode="prefill",
                               prefill_slots=slots, prefill_lens=lens)
        self.model(toks, positions, ctx)

    @torch.no_grad()
    def _follow_append(self, msg) -> None:
        self._append_forward(msg["slots"], msg["starts"], msg["lens"],
                             msg["chunks"])

    @torch.no_grad()
    def _follow_decode(self, msg) -> None:
        slots, lens, tok_l = msg["slots"], msg["lens"], msg["toks"]
        if msg["graph"]:
            g, st = self._get_graph(msg["bucket"])
            self._stage_inputs(st, slots, lens, tok_l, msg.get("samp"),
                               msg.get("ntop"))
            for _ in range(msg["chunk"]):
                g.replay()
            torch.cuda.synchronize()
            return
        toks = torch.tensor([[t] for t in tok_l], dtype=torch.long,
                            device=self.device)
        slots_t = torch.tensor(slots, dtype=torch.long, device=self.device)
        pos_t = torch.tensor(lens, dtype=torch.long, device=self.device)
        positions = torch.tensor(lens, dtype=torch.int32,
                                 device=self.device)
        kv_lens = torch.tensor([l + 1 for l in lens], dtype=torch.int32,
                               device=self.device)
        ctx = InferenceContext(cache=self.cache, mode="decode",
                               slots=slots_t, pos=pos_t, kv_lens=kv_lens,
                               slot_ids_i32=slots_t.int())
        self.model(toks, positions, ctx)

    def _loop(self):
        try:
            self._loop_inner()
        except Exception:
            # A fatal engine error must not leave TP followers blocked
            # in their broadcast receive forever.
            if self.tp_world > 1 and self.tp_rank == 0:
                try:
                    self._tp_bcast({"op": "stop"})
                except Exception:  # noqa: BLE001
                    pass
            raise

    def _loop_inner(self):
        while not self._stop.is_set():
            did = False
            if self.prefill_chunk is not None:
                # Chunked prefill: admission only takes a slot; each
                # iteration runs one chunk forward, then one decode step.
                while self.free_slots and not self.pending.empty():
                    try:
                        req = self.pending.get_nowait()
                    except queue.Empty:
                        break
                    self.prefilling.append(
                        _Prefilling(req, self.free_slots.pop()))
                if self.prefilling:
                    self._append_step()
                    did = True
                if self.active:
                    self._decode_step()
                    did = True
                if not did:
                    time.sleep(0.005)
                continue
            # Admit pending requests while slots are free — batched
            # (up to 16 per prefill forward).
            batch: List[Request] = []
            while (self.free_slots and len(batch) < len(self.free_slots)
                   and len(batch) < 16 and not self.pending.empty()):
                try:
                    batch.append(self.pending.get_nowait())
                except queue.Empty:
                    break
            if batch:
                self._prefill(batch)
                did = True
            if self.active:
                self._decode_step()
                did = True
            if not did:
                time.sleep(0.005)
