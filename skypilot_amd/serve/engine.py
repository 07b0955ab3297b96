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

With ``penalties`` set, requests may carry ``presence_penalty``,
``frequency_penalty`` and ``repetition_penalty``: the engine keeps every
sequence's token ids by position in ``hist`` and ops.penalize_logits
(docs/KERNELS.md "Decode penalties") writes a penalised copy of the
logits that the sampler or the argmax reads, inside the decode graph and
in the eager steps alike.  Log-probabilities keep describing the raw
logits.

With ``speculative`` = K > 0, a step of greedy requests drafts K tokens
per sequence (serve/speculative.py: prompt lookup, or ``drafter``) and
verifies K + 1 in one forward over the decode GEMMs and the multi-token
attention kernel (ops.attn_verify; docs/KERNELS.md "Multi-token verify
attention"); the tokens are those of token-by-token greedy decode.
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
from skypilot_amd.serve.speculative import accept, ngram_draft, pad_draft


@dataclass
class InferenceContext:
    cache: KVCache
    mode: str  # "prefill" | "decode" | "append" | "verify"
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
    # decode: "per_head" or "grouped" (Engine(decode_attn=...))
    decode_attn: str = "per_head"
    # verify (speculative decoding): tokens [n, verify_t]; row b * T + t is
    # the token at position verify_start[b] + t.  verify_start int32 [n]
    # (slot_ids_i32 holds the [n] slots), verify_row_slots int32 [n * T].
    verify_t: int = 0
    verify_start: Optional[torch.Tensor] = None
    verify_row_slots: Optional[torch.Tensor] = None


DECODE_ATTN = ("per_head", "grouped")


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
    # Penalties need Engine(penalties=True).  presence and frequency act
    # on the tokens generated so far, repetition (> 0, 1 is off) on every
    # token of the prompt and the output (docs/KERNELS.md "Decode
    # penalties").
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0
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
                 kv_dtype: str = "bf16", max_logprobs: int = 0,
                 decode_attn: str = "per_head", penalties: bool = False,
                 speculative: int = 0, drafter=None):
        # Speculative decoding: K > 0 drafts K tokens per sequence
        # (drafter(ids, k) -> list, ngram_draft by default) and verifies
        # K + 1 in one forward (_verify_step); 0 keeps every path, graph
        # and staged block as they are.
        if (isinstance(speculative, bool) or not isinstance(speculative, int)
                or not 0 <= speculative <= 7):
            raise ValueError(
                f"speculative must be an int in [0, 7], got {speculative!r}")
        if speculative and kv_dtype == "fp8":
            raise ValueError(
                "speculative decoding does not serve the fp8 KV cache")
        if speculative and tp_world > 1:
            raise ValueError(
                "speculative decoding does not serve tensor-parallel models")
        self.speculative = speculative
        self.drafter = drafter if drafter is not None else ngram_draft
        self._verify_graphs: Dict[int, tuple] = {}
        # False keeps the decode graph, the staged block and every code
        # path as they are without the feature, and submit() rejects a
        # request that sets a penalty.
        self.penalties = bool(penalties)
        # "grouped" runs decode attention through the grouped split-KV
        # kernel (docs/KERNELS.md "Grouped split-KV decode"); the default
        # keeps the per-head kernels and the decode graph as they are.
        if decode_attn not in DECODE_ATTN:
            raise ValueError(
                f"decode_attn must be one of {DECODE_ATTN}, got "
                f"{decode_attn!r}")
        self.decode_attn = decode_attn
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
        group = self.cfg.num_heads // self.cfg.num_kv_heads
        if decode_attn == "grouped" and group > ops.GQA_MAX_GROUP:
            raise ValueError(
                f'decode_attn="grouped" takes at most {ops.GQA_MAX_GROUP} q '
                f"heads per kv head, the model has {group}")
        if speculative and (speculative + 1) * group > ops.VERIFY_MAX_COLS:
            raise ValueError(
                f"speculative = {speculative} needs (K + 1) * group = "
                f"{(speculative + 1) * group} columns, the verify kernel "
                f"takes {ops.VERIFY_MAX_COLS}")
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
                      "prefill_tokens": 0, "graph_buckets": [],
                      "spec_steps": 0, "spec_drafted": 0, "spec_accepted": 0}
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
        # Penalties: token ids by position for every cache slot, and on
        # the GPU the kernel's all-zero count workspace, sized for the
        # largest graph bucket and shared by all buckets and by the eager
        # steps (one step runs at a time, and each leaves it all zero).
        self.hist: Optional[torch.Tensor] = None
        self._pen_cnt: Optional[torch.Tensor] = None
        if self.penalties:
            if self.max_seq > ops.PENALTY_MAX_SEQ:
                raise ValueError(
                    f"penalties need max_seq <= {ops.PENALTY_MAX_SEQ}, got "
                    f"{self.max_seq}")
            self.hist = torch.zeros(self.cache.max_batch, self.max_seq,
                                    dtype=torch.int32, device=self.device)
            if self.device.type == "cuda":
                self._pen_cnt = ops.penalty_workspace(
                    self._bucket(max(self.max_batch, 1)),
                    self.cfg.vocab_size, self.device)

    def enable_fp8_decode(self, min_bytes: int = 1 << 20,
                          max_batch: int = 2) -> int:
        """Quantize every large linear weight to row-wise e4m3fn and
        route the decode GEMVs through the fp8 kernel (half the streamed
        bytes on the weight-bandwidth-bound decode path; prefill stays
        bf16).  max_batch (2..64) is the largest decode batch the fp8
        weights serve: above 2 the batched steps run the fp8 MFMA GEMM
        (ops.set_fp8_decode_max_batch).  Returns the number of weights
        registered."""
        from skypilot_amd import ops as _ops
        self._claim_decode_weights("fp8")
        _ops.set_fp8_decode_max_batch(max_batch)
        self._fp8_registered = self._register_decode_weights(
            _ops.register_fp8_weight, min_bytes, 1024)
        return self._fp8_registered

    def enable_fp8_prefill(self, min_tokens="measured",
                           min_bytes: int = 1 << 20) -> int:
        """Serve prefill, prompt chunks, verify steps and decode batches of
        at least min_tokens tokens (decode_linear: above 64 rows) from the
        row-wise fp8 weights too: ops.linear, ops.qkv_linear and
        ops.decode_linear run ops.gemm_fp8_w8 (ops.set_fp8_prefill).
        "measured" takes the per-shape token ranges of the benchmark, an int
        forces one threshold.  Registers the fp8 weights if enable_fp8_decode
        has not (every large linear weight with I % 128 == 0; decode steps
        then read the ones their kernels accept as well).  lm_head's prefill
        GEMM, training and the tensor-parallel model keep bf16.  Returns the
        number of weights registered."""
        from skypilot_amd import ops as _ops
        self._claim_decode_weights("fp8")
        if getattr(self, "_fp8_registered", None) is None:
            self._fp8_registered = self._register_decode_weights(
                _ops.register_fp8_weight, min_bytes, 128)
        _ops.set_fp8_prefill(min_tokens)
        return self._fp8_registered

    def enable_fp4_decode(self, min_bytes: int = 1 << 20,
                          max_batch: int = 64) -> int:
        """Quantize every large linear weight to MXFP4 (ops.quantize_mxfp4,
        4.25 bits per weight) and route decode batches of 1..max_batch
        tokens through the fp4 MFMA GEMM where its measured table has it
        winning (ops.set_fp4_decode_max_batch); prefill stays bf16 unless
        enable_fp4_prefill.  The
        weights are the ones enable_fp8_decode takes, with I % 128 == 0.
        One engine serves fp8 or fp4 decode weights, not both.  Returns the
        number of weights registered."""
        from skypilot_amd import ops as _ops
        self._claim_decode_weights("fp4")
        _ops.set_fp4_decode_max_batch(max_batch)
        self._fp4_registered = self._register_decode_weights(
            _ops.register_fp4_weight, min_bytes, 128)
        return self._fp4_registered

    def enable_fp4_prefill(self, min_tokens="measured",
                           min_bytes: int = 1 << 20) -> int:
        """Serve prefill and prompt chunks of at least min_tokens tokens from
        the MXFP4 weights too: ops.linear and ops.qkv_linear quantise their
        input to MXFP8 and run the block-scaled MFMA GEMM
        (ops.gemm_mxfp4_a8, ops.set_fp4_prefill).  "measured" takes the
        per-shape thresholds of the benchmark, an int forces one.  Registers
        the weights enable_fp4_decode would if they are not registered yet
        (decode steps then read them as well); lm_head and the
        tensor-parallel model keep bf16.  Returns the number of weights
        registered."""
        from skypilot_amd import ops as _ops
        self._claim_decode_weights("fp4")
        if getattr(self, "_fp4_registered", None) is None:
            self._fp4_registered = self._register_decode_weights(
                _ops.register_fp4_weight, min_bytes, 128)
        _ops.set_fp4_prefill(min_tokens)
        return self._fp4_registered

    def enable_bf16_mfma_decode(self, max_batch: int = 64) -> None:
        """Route decode batches of 2..max_batch tokens over plain bf16
        weights through the bf16 MFMA GEMM where its measured table has it
        winning (ops.set_bf16_decode_max_batch).  It changes no weights, and
        tensors registered as fp8 or fp4 keep their own routes."""
        from skypilot_amd import ops as _ops
        _ops.set_bf16_decode_max_batch(max_batch)

    def _claim_decode_weights(self, fmt: str) -> None:
        have = getattr(self, "_decode_weight_format", fmt)
        if have != fmt:
            raise ValueError(
                f"enable_{fmt}_decode: this engine already serves {have} "
                f"decode weights")
        self._decode_weight_format = fmt

    def _register_decode_weights(self, register, min_bytes: int,
                                 k_multiple: int) -> int:
        n = 0
        for name, p in self.model.named_parameters():
            if (p.ndim == 2 and p.dtype == torch.bfloat16
                    and p.numel() * 2 >= min_bytes
                    and p.shape[1] % k_multiple == 0
                    and "embed" not in name):
                register(p.data)
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
                    and a._wqkv.shape[1] % k_multiple == 0):
                register(a._wqkv)
                n += 1
        return n

    # ------------------------------------------------------------------
    def submit(self, req: Request) -> Request:
        self._check_sampling(req)
        self._check_logprobs(req)
        self._check_penalties(req)
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

    def _check_penalties(self, req: Request) -> None:
        """Validate and normalise a request's penalties to plain finite
        floats, as _check_sampling does.  Raises ValueError."""
        for name in ("presence_penalty", "frequency_penalty",
                     "repetition_penalty"):
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
        if req.repetition_penalty <= 0:
            raise ValueError("repetition_penalty must be > 0, got "
                             f"{req.repetition_penalty!r}")
        if not self.penalties and self._pen_row(req)[:3] != (0.0, 0.0, 1.0):
            # refuse rather than drop them
            raise ValueError(
                "presence_penalty, frequency_penalty and repetition_penalty "
                "need an engine with penalties on (Engine(penalties=True) / "
                "--penalties)")

    @staticmethod
    def _pen_row(req: Request) -> tuple:
        """(presence, frequency, repetition, prompt length): one row of
        the penalty parameters, what the TP decode plan carries."""
        return (req.presence_penalty, req.frequency_penalty,
                req.repetition_penalty, len(req.prompt_ids))

    def _pen_rows(self, reqs: List[Request]):
        return [self._pen_row(r) for r in reqs] if self.penalties else None

    def _hist_put(self, slot: int, start: int, ids: List[int]) -> None:
        """Admission: prompt ids into hist[slot, start:start + len(ids)]."""
        if self.penalties and ids:
            self.hist[slot, start:start + len(ids)] = torch.tensor(
                ids, dtype=torch.int32, device=self.device)

    def _penalize(self, logits: torch.Tensor, pen, slots: List[int],
                  positions: List[int], toks: List[int]) -> torch.Tensor:
        """The eager steps' ops.penalize_logits: `logits` [n, V] of the
        tokens `toks` at `positions` of cache slots `slots`, `pen` the
        rows of _pen_rows.  Returns the penalised copy, or `logits`
        itself when no row sets a penalty (hist is then left alone, as
        the op leaves it for an off row)."""
        if pen is None or all(r[:3] == (0.0, 0.0, 1.0) for r in pen):
            return logits
        idx = torch.tensor([toks, positions, slots, [r[3] for r in pen]],
                           dtype=torch.int32, device=self.device)
        par = torch.tensor([[r[k] for r in pen] for k in range(3)],
                           dtype=torch.float32, device=self.device)
        logits = logits.contiguous()
        return ops.penalize_logits(
            logits, torch.empty_like(logits), self.hist, self._pen_cnt,
            idx[0], idx[1], idx[2], idx[3], par[0], par[1], par[2])

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
        for slot, r in zip(slots, reqs):
            self._hist_put(slot, 0, r.prompt_ids)
        # the first token is drawn under the prompt's penalties: the input
        # token is the prompt's last, nothing is generated yet
        pen = self._penalize(last, self._pen_rows(reqs), slots,
                             [l - 1 for l in lens],
                             [r.prompt_ids[-1] for r in reqs])
        first = self._sample_batch(pen, reqs, [l - 1 for l in lens])
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
            self._hist_put(slots[i], starts[i], ids)

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
            fin_pos = [ends[i] - 1 for i in fin]
            pen = self._penalize(
                logits[fin, 0], self._pen_rows(fin_reqs),
                [slots[i] for i in fin], fin_pos,
                [r.prompt_ids[-1] for r in fin_reqs])
            fin_ids = self._sample_batch(pen, fin_reqs, fin_pos)
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
        # With penalties four rows follow the sampling parameters:
        # presence bits, frequency bits, repetition bits, prompt length
        # (padding rows: 0, 0, 1.0, 0 — off).
        nsamp = 11 if self.device_sampling else 6
        rows = nsamp + (4 if self.penalties else 0) + (
            1 if self.max_logprobs else 0)
        st = {
            "host": torch.zeros(rows, b, dtype=torch.int32,
                                pin_memory=True),
            "block": torch.zeros(rows, b, dtype=torch.int32, device=dev),
        }
        st["stage"] = st["block"][:6]
        st["samp"] = st["block"][6:nsamp]
        if self.penalties:
            st["pen"] = st["block"][nsamp:nsamp + 4]
            st["pen"][2] = torch.ones(
                b, device=dev).view(torch.int32)  # repetition 1.0
            st["pen_out"] = torch.empty(b, self.cfg.vocab_size,
                                        dtype=torch.bfloat16, device=dev)
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
                        kv_lens=stg[4], slot_ids_i32=stg[5],
                        decode_attn=self.decode_attn))

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
            # With penalties the advance kernel reads the penalised copy
            # of the logits: the input token stage[0] at position stage[1]
            # goes into hist, and the row's history decides the values.
            src = st["out"][:, 0]
            if self.penalties:
                stg, pen = st["stage"], st["pen"]
                src = ops.penalize_logits(
                    src, st["pen_out"], self.hist, self._pen_cnt, stg[0],
                    stg[1], stg[5], pen[3], pen[0].view(torch.float32),
                    pen[1].view(torch.float32), pen[2].view(torch.float32))
            if self.device_sampling:
                ops.decode_sample_advance(src, st["stage"], st["ring"],
                                          st["ctr"], st["samp"])
            else:
                ops.decode_advance(src, st["stage"], st["ring"], st["ctr"])
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
        pen = self._pen_rows(reqs)
        penalised = None  # [n, V] when the graph has made it already
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
                            "chunk": chunk, "samp": samp, "ntop": ntop,
                            "pen": pen})
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
            self._stage_inputs(st, slots, lens, tok_l, samp, ntop, pen)
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
            if self.penalties:
                penalised = st["pen_out"][:n]
        else:
            self._tp_bcast({"op": "decode", "graph": False,
                            "slots": slots, "lens": lens, "toks": tok_l,
                            "chunk": 1, "samp": self._samp_rows(reqs),
                            "pen": pen})
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
                kv_lens=kv_lens, slot_ids_i32=slots_t.int(),
                decode_attn=self.decode_attn)
            logits = self.model(toks, positions, ctx)  # [n, 1, V]
        # Device sampling draws the whole batch in one kernel call.  On
        # the host path greedy rows batch into one argmax + one sync and
        # sampled rows (temperature > 0) go through _sample individually.
        # (The chained graph path already returned above.)
        # Tokens come from the penalised logits (the input token of each
        # row sits at position lens[i]); log-probabilities from the raw.
        if penalised is None:
            penalised = self._penalize(logits[:n, 0], pen, slots, lens,
                                       tok_l)
        batch_ids = None
        if self.device_sampling:
            # counter = position of each row's input token
            batch_ids = self._sample_batch(penalised, reqs, lens)
        elif all(r.temperature == 0 for r in reqs):
            batch_ids = penalised.argmax(-1).tolist()
        if batch_ids is None:
            batch_ids = [self._sample(penalised[i], r.temperature, r.top_p)
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

    # ----------------------- speculative decoding ----------------------
    def _verify_forward(self, toks, start, slots):
        """The verify forward and its argmax: toks int [b, T], start and
        slots int32 [b] device tensors -> token ids [b, T] (ties to the
        lowest index, as decode_advance has them).  Captured once per
        bucket with use_graphs, run as it is in eager mode."""
        b, T = toks.shape
        positions = (start[:, None] + torch.arange(
            T, dtype=torch.int32, device=self.device)[None, :]).reshape(-1)
        ctx = InferenceContext(
            cache=self.cache, mode="verify", slot_ids_i32=slots,
            verify_t=T, verify_start=start,
            verify_row_slots=slots[:, None].repeat(1, T).reshape(-1))
        return self.model(toks.long(), positions, ctx).argmax(-1)

    def _get_verify_graph(self, b: int):
        """Lazily capture _verify_forward for batch bucket `b`.  The step's
        inputs travel as one pinned-host -> device copy of an int32
        [T + 2, b] block: rows 0..T-1 the token rows, row T q_start, row
        T + 1 the slot.  Padding rows verify zeros at the start of the
        scratch slot."""
        if b in self._verify_graphs:
            return self._verify_graphs[b]
        T = self.speculative + 1
        st = {
            "host": torch.zeros(T + 2, b, dtype=torch.int32,
                                pin_memory=True),
            "block": torch.zeros(T + 2, b, dtype=torch.int32,
                                 device=self.device),
        }
        st["block"][T + 1] = self._scratch_slot

        def run():
            blk = st["block"]
            return self._verify_forward(blk[:T].t(), blk[T], blk[T + 1])

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warmup on a side stream, as _get_graph
                run()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st["ids"] = run()
        self._verify_graphs[b] = (g, st)
        self.stats["spec_graph_buckets"] = sorted(self._verify_graphs)
        return self._verify_graphs[b]

    @torch.no_grad()
    def _verify_step(self) -> bool:
        """One speculative step for every active sequence, or False when
        the step has to be an ordinary _decode_step: a request that
        samples, sets a penalty or wants log-probabilities, work pending
        or prefilling, a sequence within K + 1 rows of max_seq - 1, or no
        draft at all."""
        K = self.speculative
        slots = sorted(self.active.keys())
        reqs = [self.active[s] for s in slots]
        if (not slots or not self.pending.empty() or self.prefilling
                or any(r.temperature != 0 or r.logprobs is not None
                       or self._pen_row(r)[:3] != (0.0, 0.0, 1.0)
                       for r in reqs)):
            return False
        lens = [self.cache.lens[s] for s in slots]
        if any(l + K + 1 > self.max_seq - 1 for l in lens):
            return False
        drafts = [list(self.drafter(r.prompt_ids + r.out_ids, K))[:K]
                  for r in reqs]
        if not any(drafts):
            return False
        n, T = len(slots), K + 1
        rows = [[r.out_ids[-1]] + pad_draft(d, K, r.out_ids[-1])
                for r, d in zip(reqs, drafts)]
        if self.use_graphs:
            g, st = self._get_verify_graph(self._bucket(n))
            h = st["host"].numpy()
            h[:T, :n] = list(zip(*rows))
            h[:T + 1, n:] = 0
            h[T, :n] = lens
            h[T + 1, :n] = slots
            h[T + 1, n:] = self._scratch_slot
            st["block"].copy_(st["host"], non_blocking=True)
            g.replay()
            ids = st["ids"][:n].tolist()  # the step's one sync
        else:
            def i32(vals):
                return torch.tensor(vals, dtype=torch.int32,
                                    device=self.device)
            ids = self._verify_forward(i32(rows), i32(lens),
                                       i32(slots)).tolist()
        self.stats["spec_steps"] += 1
        for i, (slot, req) in enumerate(zip(slots, reqs)):
            out = accept(drafts[i], ids[i], req.stop_id,
                         req.max_tokens - len(req.out_ids))
            self.stats["spec_drafted"] += len(drafts[i])
            self.stats["spec_accepted"] += len(out) - 1
            # Rows past the new length stay in the cache as stale rows.
            for next_id in out:
                self.cache.lens[slot] += 1
                req.out_ids.append(next_id)
                if req.stream_queue is not None:
                    req.stream_queue.put(next_id)
                self.stats["tokens_generated"] += 1
                self._maybe_finish(slot, req, next_id)
        return True

    def _step_active(self) -> None:
        """One step for the active sequences: a verify step where
        speculative decoding is on and applies, else a decode step."""
        if not (self.speculative and self._verify_step()):
            self._decode_step()

    def _samp_rows(self, reqs: List[Request]):
        """Per-row (temperature, top_p, top_k, seed) for the device
        sampler — what the TP decode plan carries; None when off."""
        if not self.device_sampling:
            return None
        return [(r.temperature, r.top_p, r.top_k, r.seed) for r in reqs]

    def _stage_inputs(self, st, slots, lens, tok_l, samp,
                      ntop=None, pen=None) -> None:
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
        if self.penalties:
            k = 11 if self.device_sampling else 6
            hf = h.view("float32")
            for j in range(3):
                hf[k + j, :n] = [r[j] for r in pen]
            h[k + 3, :n] = [r[3] for r in pen]
            hf[k:k + 2, n:] = 0.0  # padding rows are off
            hf[k + 2, n:] = 1.0
            h[k + 3, n:] = 0
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
            self._hist_put(slots[i], 0, ids)
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
                               msg.get("ntop"), msg.get("pen"))
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
                               slot_ids_i32=slots_t.int(),
                               decode_attn=self.decode_attn)
        logits = self.model(toks, positions, ctx)
        # keeps this rank's hist equal to the leader's
        self._penalize(logits[:, 0], msg.get("pen"), slots, lens, tok_l)

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
                    self._step_active()
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
                self._step_active()
                did = True
            if not did:
                time.sleep(0.005)
