"""Llama-3 model family, written MI355X-first.

Differences from a stock HF/torchtitan implementation, driven by the
CDNA4 kernels in :mod:`skypilot_amd.ops`:

* tensors stay in ``[B, S, H, D]`` layout end-to-end — the attention
  kernels read strided rows directly, so there are no head transposes;
* RMSNorm / RoPE / attention / cross-entropy are the fused HIP kernels;
* GEMMs are hipBLASLt through ``F.linear``; in training the block
  projections go through ``ops.linear`` / ``ops.qkv_linear``, whose
  backward picks the weight gradient's operand layout per shape;
* RoPE cos/sin tables are precomputed fp32 buffers (on-device trig would
  make the op VALU-bound — guide Appendix B).

Reference parity: SkyPilot bundles no models (it launches user programs,
SURVEY.md §2.11); these are the bundled train/serve entrypoint models the
north star requires.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn

from skypilot_amd import ops


@dataclass
class LlamaConfig:
    name: str = "llama3-8b"
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    max_seq_len: int = 8192
    tie_embeddings: bool = False
    # Qwen2-style families put biases on the q/k/v projections only
    attn_bias: bool = False


CONFIGS = {
    "llama3-8b": LlamaConfig(),
    "llama3-70b": LlamaConfig(
        name="llama3-70b", hidden_size=8192, intermediate_size=28672,
        num_layers=80, num_heads=64, num_kv_heads=8),
    # Qwen2 dense family (same RMSNorm+RoPE+GQA+SwiGLU skeleton with
    # q/k/v biases and a 1e6 rope base; reference architecture is
    # public — weights are random-init here, no network).
    "qwen2-7b": LlamaConfig(
        name="qwen2-7b", vocab_size=152064, hidden_size=3584,
        intermediate_size=18944, num_layers=28, num_heads=28,
        num_kv_heads=4, rope_theta=1000000.0, norm_eps=1e-6,
        max_seq_len=32768, attn_bias=True),
    "qwen2-debug": LlamaConfig(
        name="qwen2-debug", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_heads=2,
        num_kv_heads=1, head_dim=128, rope_theta=1000000.0,
        max_seq_len=512, attn_bias=True),
    # Small configs for tests / smoke.
    "llama-debug": LlamaConfig(
        name="llama-debug", vocab_size=512, hidden_size=256,
        intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1,
        head_dim=128, max_seq_len=512),
    "llama-smoke": LlamaConfig(
        name="llama-smoke", vocab_size=4096, hidden_size=1024,
        intermediate_size=2816, num_layers=4, num_heads=8, num_kv_heads=4,
        head_dim=128, max_seq_len=2048),
}


def rope_tables(cfg: LlamaConfig, device, dtype=torch.float32):
    half = cfg.head_dim // 2
    inv_freq = 1.0 / (cfg.rope_theta ** (
        torch.arange(0, half, dtype=torch.float32, device=device) / half))
    t = torch.arange(cfg.max_seq_len, dtype=torch.float32, device=device)
    freqs = torch.outer(t, inv_freq)  # [S, D/2]
    return freqs.cos().to(dtype).contiguous(), freqs.sin().to(dtype).contiguous()


def prefill_cache_write(attn, k, v, infer_ctx):
    """Whole-prompt prefill: store the (unpadded) K/V rows of each
    sequence of the batch for decode.  With an fp8 cache this is one
    quantising write per layer; the prefill's own attention still runs on
    the unquantised K/V.  Shared by Attention and TPAttention."""
    slots = (infer_ctx.prefill_slots
             if infer_ctx.prefill_slots is not None
             else [infer_ctx.prefill_slot])
    lens = (infer_ctx.prefill_lens
            if infer_ctx.prefill_lens is not None
            else [infer_ctx.prefill_len])
    cache = infer_ctx.cache
    if cache.kv_dtype == "fp8":
        if infer_ctx.kv_write_idx is None:  # built once per forward
            def i32(vals):
                return torch.tensor(vals, dtype=torch.int32, device=k.device)
            infer_ctx.kv_write_idx = (i32(slots), i32([0] * len(slots)),
                                      i32(lens))
        cache.write_rows_fp8(attn.layer_idx, k, v, *infer_ctx.kv_write_idx)
        return
    for i, (slot, ln) in enumerate(zip(slots, lens)):
        cache.write_prefill(attn.layer_idx, slot, k[i:i + 1], v[i:i + 1], ln)


def append_attention(attn, q, k, v, infer_ctx):
    """Chunked prefill (infer_ctx.mode == "append"): row i of sequence b
    is the token at position append_start[b] + i.  The chunk's valid K/V
    rows go into the cache first; attention then reads K/V from the cache
    only, so the chunk sees the rows earlier chunks left there.  Shared
    by Attention and the tensor-parallel TPAttention."""
    cache = infer_ctx.cache
    if cache.kv_dtype == "fp8":
        # one quantising write for the whole batch, then the fp8 kernel;
        # the chunk attends its own rows as the cache holds them
        li = attn.layer_idx
        cache.write_rows_fp8(li, k, v, infer_ctx.append_slots,
                             infer_ctx.append_start, infer_ctx.append_lens)
        return ops.attn_append_fp8(q, cache.k[li], cache.v[li],
                                   cache.k_exp[li], cache.v_exp[li],
                                   infer_ctx.append_slots,
                                   infer_ctx.append_start,
                                   infer_ctx.append_lens, attn.scale)
    for i, (slot, start, ln) in enumerate(zip(infer_ctx.append_slots_l,
                                              infer_ctx.append_start_l,
                                              infer_ctx.append_lens_l)):
        cache.write_append(attn.layer_idx, slot, start, k[i:i + 1],
                           v[i:i + 1], ln)
    return ops.attn_append(q, cache.k[attn.layer_idx],
                           cache.v[attn.layer_idx], infer_ctx.append_slots,
                           infer_ctx.append_start, infer_ctx.append_lens,
                           attn.scale)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        h, d = cfg.hidden_size, cfg.head_dim
        self.n_q, self.n_kv = cfg.num_heads, cfg.num_kv_heads
        self.wq = nn.Linear(h, self.n_q * d, bias=cfg.attn_bias)
        self.wk = nn.Linear(h, self.n_kv * d, bias=cfg.attn_bias)
        self.wv = nn.Linear(h, self.n_kv * d, bias=cfg.attn_bias)
        self.wo = nn.Linear(self.n_q * d, h, bias=False)
        self.scale = 1.0 / math.sqrt(d)
        self._wqkv = None  # lazy fused [q|k|v] weight for the decode GEMV
        self._bqkv = None  # packed [q|k|v] bias (attn_bias families)

    def packed_qkv(self):
        """Lazily build the fused decode-GEMV weight (and bias)."""
        if self._wqkv is None:
            self._wqkv = torch.cat(
                [self.wq.weight, self.wk.weight, self.wv.weight],
                0).contiguous()
            if self.wq.bias is not None:
                self._bqkv = torch.cat(
                    [self.wq.bias, self.wk.bias, self.wv.bias],
                    0).contiguous()
        return self._wqkv

    def forward(self, x, cos, sin, positions, infer_ctx=None,
                qkv=None):
        d = self.cfg.head_dim
        if x is None:  # decode with a precomputed (norm-fused) qkv
            B, S = qkv.shape[0], 1
        else:
            B, S, _ = x.shape
        decode = infer_ctx is not None and infer_ctx.mode == "decode"
        if decode:
            # One packed qkv GEMV, then one fused rope+cache-write
            # kernel (decode_fused.hip) — replaces 3 GEMVs + rope x2 +
            # scatter x2.  Decode GEMMs route via ops.decode_linear
            # (skinny GEMV vs hipBLASLt per measured thresholds).
            cache = infer_ctx.cache
            if qkv is None:
                qkv = ops.decode_linear(x.reshape(B, -1),
                                        self.packed_qkv())
            qkv = qkv.reshape(B, -1)  # [B,1,width] from norm-fused GEMV
            if self._bqkv is not None:
                qkv = qkv + self._bqkv
            # fused rope + cache-write + attention: one kernel instead
            # of rope_kvwrite + attn_decode (the current token's k/v is
            # attended from registers; the cache row is written for
            # future steps by one block per kv head).
            li = self.layer_idx
            if cache.kv_dtype == "fp8":
                o = ops.attn_decode_qkv_fp8(
                    qkv, cache.k[li], cache.v[li], cache.k_exp[li],
                    cache.v_exp[li], cos, sin, positions, infer_ctx.kv_lens,
                    infer_ctx.slot_ids_i32, self.n_q, self.n_kv, self.scale)
            else:
                o = ops.attn_decode_qkv(
                    qkv, cache.k[li], cache.v[li], cos, sin, positions,
                    infer_ctx.kv_lens, infer_ctx.slot_ids_i32, self.n_q,
                    self.n_kv, self.scale)
            return ops.decode_linear(o.reshape(B, self.n_q * d),
                                     self.wo.weight).view(B, S, -1)
        # F.linear forwards; the backward's weight gradients go through
        # the extension's linear_wgrad (one packed product for q, k and v)
        q, k, v = ops.qkv_linear(x, self.wq.weight, self.wk.weight,
                                 self.wv.weight, self.wq.bias, self.wk.bias,
                                 self.wv.bias)
        q = q.view(B, S, self.n_q, d)
        k = k.view(B, S, self.n_kv, d)
        v = v.view(B, S, self.n_kv, d)
        q = ops.rope(q.reshape(B * S, self.n_q, d), cos, sin,
                     positions).view(B, S, self.n_q, d)
        k = ops.rope(k.reshape(B * S, self.n_kv, d), cos, sin,
                     positions).view(B, S, self.n_kv, d)
        if infer_ctx is None:
            o = ops.attention(q, k, v, self.scale, causal=True)
        elif infer_ctx.mode == "append":
            o = append_attention(self, q, k, v, infer_ctx)
        else:  # prefill: plain causal attention over the prompt; the
            # (unpadded) K/V rows land in the cache for decode.  Rows of
            # a batched prefill are independent sequences.
            prefill_cache_write(self, k, v, infer_ctx)
            o = ops.attention(q, k, v, self.scale, causal=True)
        return ops.linear(o.reshape(B, S, self.n_q * d), self.wo.weight)


class MLP(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        h, m = cfg.hidden_size, cfg.intermediate_size
        self.w_gate_up = nn.Linear(h, 2 * m, bias=False)  # fused gate|up GEMM
        self.w_down = nn.Linear(m, h, bias=False)
        self.m = m

    def forward(self, x, infer_ctx=None):
        decode = infer_ctx is not None and infer_ctx.mode == "decode"
        lin = ops.decode_linear if decode else ops.linear
        return lin(ops.swiglu(lin(x, self.w_gate_up.weight)),
                   self.w_down.weight)

    def down_from_gu(self, gu):
        """Decode path with a precomputed (norm-fused) gate_up GEMV."""
        return ops.decode_linear(ops.swiglu(gu), self.w_down.weight)

    # (decode path is driven from Llama.forward's fused-residual loop)


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig, layer_idx: int):
        super().__init__()
        self.attn = Attention(cfg)
        self.attn.layer_idx = layer_idx
        self.mlp = MLP(cfg)
        self.attn_norm = nn.Parameter(torch.ones(cfg.hidden_size))
        self.mlp_norm = nn.Parameter(torch.ones(cfg.hidden_size))
        self.eps = cfg.norm_eps

    def forward(self, x, cos, sin, positions, infer_ctx=None):
        x = x + self.attn(ops.rmsnorm(x, self.attn_norm, self.eps), cos, sin,
                          positions, infer_ctx)
        x = x + self.mlp(ops.rmsnorm(x, self.mlp_norm, self.eps),
                         infer_ctx)
        return x


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.embed = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.blocks = nn.ModuleList(
            Block(cfg, i) for i in range(cfg.num_layers))
        self.final_norm = nn.Parameter(torch.ones(cfg.hidden_size))
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        if cfg.tie_embeddings:
            self.lm_head.weight = self.embed.weight
        self._rope = None

    def _tables(self, device):
        if self._rope is None or self._rope[0].device != device:
            self._rope = rope_tables(self.cfg, device)
        return self._rope

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor = None,
                infer_ctx=None) -> torch.Tensor:
        B, S = tokens.shape
        cos, sin = self._tables(tokens.device)
        if positions is None:
            positions = torch.arange(S, dtype=torch.int32,
                                     device=tokens.device)
            positions = positions.unsqueeze(0).expand(B, S).reshape(-1)
        x = self.embed(tokens)
        if infer_ctx is not None and infer_ctx.mode == "decode":
            # Fused-residual decode loop: every residual add rides in
            # the next rmsnorm_res kernel (one launch instead of two),
            # including the final-norm + lm-head hand-off.
            # Norm-fused decode loop: each rmsnorm_res rides INSIDE the
            # following fp8 GEMV (one launch; decode is dispatch-gap
            # bound) — falls back to rmsnorm_res + GEMV when fp8 is
            # off.  The attention/MLP modules accept the precomputed
            # qkv / gate_up projections.
            res = None
            for blk in self.blocks:
                if not hasattr(blk.attn, "_wqkv"):
                    # TP blocks keep the classic split projections
                    if res is None:
                        h = ops.rmsnorm(x, blk.attn_norm, blk.eps)
                    else:
                        x, h = ops.rmsnorm_res(x, res, blk.attn_norm,
                                               blk.eps)
                    a = blk.attn(h, cos, sin, positions, infer_ctx)
                    x, h2 = ops.rmsnorm_res(x, a, blk.mlp_norm, blk.eps)
                    res = blk.mlp(h2, infer_ctx)
                    continue
                x, qkv = ops.decode_norm_linear(
                    x, res, blk.attn_norm, blk.eps, blk.attn.packed_qkv())
                a = blk.attn(None, cos, sin, positions, infer_ctx,
                             qkv=qkv)
                x, gu = ops.decode_norm_linear(
                    x, a, blk.mlp_norm, blk.eps, blk.mlp.w_gate_up.weight)
                res = blk.mlp.down_from_gu(gu)
            _, logits = ops.decode_norm_linear(
                x, res, self.final_norm, self.cfg.norm_eps,
                self.lm_head.weight)
            return logits
        for blk in self.blocks:
            x = blk(x, cos, sin, positions, infer_ctx)
        if (infer_ctx is not None and infer_ctx.mode == "append"
                and not getattr(infer_ctx, "all_rows", False)):
            # Only the last valid row of each chunk can be sampled from:
            # gather it before the norm and the vocab-sized GEMM.  -> [n,1,V]
            # (all_rows keeps every row: prompt log-probabilities.)
            last = (infer_ctx.append_lens.long() - 1).clamp(min=0)
            x = x[torch.arange(B, device=x.device), last].unsqueeze(1)
        x = ops.rmsnorm(x, self.final_norm, self.cfg.norm_eps)
        return self.lm_head(x)

    def loss(self, tokens: torch.Tensor, targets: torch.Tensor):
        """Forward + fused cross entropy (logit grads computed in-kernel)."""
        logits = self.forward(tokens)
        return ops.fused_cross_entropy(
            logits.reshape(-1, self.cfg.vocab_size), targets.reshape(-1))

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def flops_per_token(self, seq_len: int) -> float:
        """Training (fwd+bwd) FLOPs per token, attention included."""
        c = self.cfg
        return 6 * self.num_params() + \
            6 * c.num_layers * 2 * seq_len * c.num_heads * c.head_dim


def build_model(name: str, device="cpu", dtype=torch.bfloat16,
                seed: int = 0) -> Llama:
    cfg = CONFIGS[name]
    torch.manual_seed(seed)
    with torch.device("meta" if device != "cpu" else "cpu"):
        model = Llama(cfg)
    if device != "cpu":
        model = model.to_empty(device=device)
        with torch.no_grad():
            for p in model.parameters():
                p.normal_(0.0, 0.02)
    return model.to(dtype)
