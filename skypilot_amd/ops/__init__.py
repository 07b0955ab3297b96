"""skypilot_amd.ops — MI355X-native fused ops for the bundled trainer.

Each op routes to the hand-written CDNA4 HIP kernels (``_C.so``, built
in-tree by :mod:`skypilot_amd.ops.build`) whenever the tensors live on a
GPU.  On a GPU box a missing/unloadable extension is a **hard error** —
there is deliberately no silent eager fallback (the driver verifies the
native code actually loaded).  On CPU (the no-GPU CI container) the ops
fall back to plain fp32 PyTorch reference implementations, which are also
what the GPU numerics tests compare the kernels against.

Reference parity note: SkyPilot itself ships no kernels (SURVEY.md
§2.11); these ops are the MI355X-native additions the north star
requires for the bundled Llama train/serve entrypoints.
"""
from __future__ import annotations

import importlib.util
import math
import os
from pathlib import Path

import torch

_C = None
_LOAD_ERR: Exception | None = None


def _load():
    global _C, _LOAD_ERR
    if _C is not None:
        return _C
    so = Path(__file__).resolve().parent / "_C.so"
    try:
        if not so.exists():
            raise ImportError(
                f"native extension {so} not built; run "
                "`python -m skypilot_amd.ops.build`")
        spec = importlib.util.spec_from_file_location("skypilot_amd.ops._C",
                                                      so)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _C = mod
    except Exception as e:  # noqa: BLE001
        _LOAD_ERR = e
        raise
    return _C


def native():
    """The native module; raises loudly if unavailable."""
    return _load()


def native_available() -> bool:
    try:
        _load()
        return True
    except Exception:  # noqa: BLE001
        return False


def _require_native(opname: str):
    try:
        return _load()
    except Exception as e:  # noqa: BLE001
        raise RuntimeError(
            f"skypilot_amd.ops.{opname}: tensor is on GPU but the native "
            f"CDNA4 extension failed to load ({e}). Refusing to fall back "
            "to eager PyTorch on the GPU path.") from e


# ===========================================================================
# Reference (CPU / verification) implementations — plain fp32 PyTorch.
# ===========================================================================
def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
             positions: torch.Tensor, backward: bool = False) -> torch.Tensor:
    # x: [..., T, H, D]; cos/sin: [S, D/2]; positions: [T]
    D = x.shape[-1]
    xf = x.float()
    c = cos[positions]  # [T, D/2]
    s = sin[positions] * (-1.0 if backward else 1.0)
    c = c.unsqueeze(-2)  # [T, 1, D/2]
    s = s.unsqueeze(-2)
    x1, x2 = xf[..., : D // 2], xf[..., D // 2:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return out.to(x.dtype)


def attention_ref(q, k, v, scale: float, causal: bool = True):
    # q: [B,S,Hq,D], k/v: [B,S,Hkv,D] -> [B,S,Hq,D]
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf = q.float().permute(0, 2, 1, 3)  # B,Hq,S,D
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    att = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        mask = torch.triu(torch.ones(S, S, dtype=torch.bool,
                                     device=q.device), 1)
        att = att.masked_fill(mask, float("-inf"))
    p = att.softmax(-1)
    out = torch.matmul(p, vf)
    return out.permute(0, 2, 1, 3).to(q.dtype)


def cross_entropy_ref(logits: torch.Tensor, targets: torch.Tensor,
                      ignore_index: int = -100) -> torch.Tensor:
    return torch.nn.functional.cross_entropy(
        logits.float(), targets.long(), ignore_index=ignore_index,
        reduction="mean")


# ===========================================================================
# Autograd wrappers.
# ===========================================================================
class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        if x.is_cuda:
            C = _require_native("rmsnorm")
            inv_rms = torch.empty(x.numel() // x.shape[-1],
                                  device=x.device, dtype=torch.float32)
            y = C.rmsnorm_fwd(x.contiguous(), w.contiguous(), inv_rms, eps)
            ctx.save_for_backward(x, w, inv_rms)
            ctx.native = True
            return y
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        ctx.native = False
        return rmsnorm_ref(x, w, eps)

    @staticmethod
    def backward(ctx, dy):
        if ctx.native:
            x, w, inv_rms = ctx.saved_tensors
            C = native()
            dx, dw = C.rmsnorm_bwd(x.contiguous(), w.contiguous(),
                                   dy.contiguous(), inv_rms)
            return dx, dw.to(w.dtype), None
        x, w = ctx.saved_tensors
        xf, wf, dyf = x.float(), w.float(), dy.float()
        H = x.shape[-1]
        inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + ctx.eps)
        dot = (dyf * wf * xf).sum(-1, keepdim=True)
        dx = inv * (dyf * wf - xf * inv * inv * dot / H)
        dw = (dyf * xf * inv).reshape(-1, H).sum(0)
        return dx.to(x.dtype), dw.to(w.dtype), None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    """y = x * rsqrt(mean(x^2) + eps) * w over the last dim H.  On GPU H
    must be a multiple of 8, and backward additionally needs H <= 16384
    (one row's columns are held in registers); other widths raise."""
    return _RMSNormFn.apply(x, w, eps)


class _RoPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, positions):
        ctx.save_for_backward(cos, sin, positions)
        if x.is_cuda:
            C = _require_native("rope")
            return C.rope(x.contiguous(), cos, sin, positions, False)
        return rope_ref(x, cos, sin, positions)

    @staticmethod
    def backward(ctx, dy):
        cos, sin, positions = ctx.saved_tensors
        if dy.is_cuda:
            C = native()
            return C.rope(dy.contiguous(), cos, sin, positions,
                          True), None, None, None
        return rope_ref(dy, cos, sin, positions, backward=True), \
            None, None, None


def rope(x, cos, sin, positions):
    """Rotary embedding of x [..., T, H, D] (D even) with fp32 tables
    cos/sin [S, D/2]; positions [T] broadcasts over leading dims.  On GPU
    positions must be int32 and the tables fp32 and contiguous (the
    kernel raises otherwise)."""
    if x.is_cuda and x.dim() > 3:  # the kernel reads one position per token
        positions = positions.expand(x.shape[:-2]).reshape(-1)
    return _RoPEFn.apply(x, cos, sin, positions)


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, causal):
        ctx.scale, ctx.causal = scale, causal
        if q.is_cuda:
            C = _require_native("attention")
            # The kernels index dense [B,S,H,D]; backward gets the same
            # dense tensors the forward ran on.
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            O, lse = C.attn_fwd(q, k, v, scale, causal)
            ctx.save_for_backward(q, k, v, O, lse)
            ctx.native = True
            return O
        ctx.save_for_backward(q, k, v)
        ctx.native = False
        return attention_ref(q, k, v, scale, causal)

    @staticmethod
    def backward(ctx, dO):
        if ctx.native:
            q, k, v, O, lse = ctx.saved_tensors
            C = native()
            dq, dk, dv = C.attn_bwd(q, k, v, O, dO.contiguous(), lse,
                                    ctx.scale, ctx.causal)
            return dq, dk, dv, None, None
        q, k, v = ctx.saved_tensors
        with torch.enable_grad():
            qd = q.detach().requires_grad_()
            kd = k.detach().requires_grad_()
            vd = v.detach().requires_grad_()
            out = attention_ref(qd, kd, vd, ctx.scale, ctx.causal)
            gq, gk, gv = torch.autograd.grad(out, (qd, kd, vd), dO)
        return gq, gk, gv, None, None


def attention(q, k, v, scale=None, causal=True):
    """Flash attention, layout [B, S, H, D] with GQA (Hq multiple of Hkv)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return _AttentionFn.apply(q, k, v, scale, causal)


class _CrossEntropyFn(torch.autograd.Function):
    """Fused CE: forward computes mean loss AND writes d_logits into the
    logits buffer (scaled by 1/n_valid); backward scales by grad_output."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        if logits.is_cuda:
            C = _require_native("cross_entropy")
            n_valid = int((targets != ignore_index).sum().item())
            n_valid = max(n_valid, 1)
            logits = logits.contiguous()
            loss = C.cross_entropy_fused(logits, targets.int(),
                                         1.0 / n_valid, ignore_index)
            ctx.save_for_backward(logits)  # now holds d_logits
            ctx.native = True
            return loss.sum() / n_valid
        ctx.native = False
        ctx.save_for_backward(logits, targets)
        ctx.ignore_index = ignore_index
        return cross_entropy_ref(logits, targets, ignore_index)

    @staticmethod
    def backward(ctx, g):
        if ctx.native:
            (dlogits,) = ctx.saved_tensors
            if not (isinstance(g, torch.Tensor) and g.numel() == 1
                    and float(g) == 1.0):
                dlogits = dlogits * g
            return dlogits, None, None
        logits, targets = ctx.saved_tensors
        with torch.enable_grad():
            ld = logits.detach().requires_grad_()
            loss = cross_entropy_ref(ld, targets, ctx.ignore_index)
            (gl,) = torch.autograd.grad(loss, (ld,), g)
        return gl, None, None


def fused_cross_entropy(logits, targets, ignore_index: int = -100):
    """NB: on GPU the logits buffer is overwritten with its gradient."""
    return _CrossEntropyFn.apply(logits, targets, ignore_index)


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        if gu.is_cuda:
            C = _require_native("swiglu")
            return C.swiglu_fwd(gu.contiguous())
        M = gu.shape[-1] // 2
        g, u = gu.float().split(M, dim=-1)
        return (torch.nn.functional.silu(g) * u).to(gu.dtype)

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        if gu.is_cuda:
            C = native()
            return C.swiglu_bwd(gu.contiguous(), dy.contiguous())
        M = gu.shape[-1] // 2
        g, u = gu.float().split(M, dim=-1)
        dyf = dy.float()
        sg = torch.sigmoid(g)
        silu = g * sg
        dg = dyf * u * (sg + silu * (1 - sg))
        du = dyf * silu
        return torch.cat([dg, du], dim=-1).to(gu.dtype)


def swiglu(gu):
    """Fused silu(gate) * up over a fused [.., 2M] gate|up tensor.  On
    GPU M must be a multiple of 8 (16-byte vectors); other widths raise."""
    return _SwiGLUFn.apply(gu)


# ---- linear layers of the training path -----------------------------------
# The forward and the input gradient are the library calls autograd would
# make.  The weight gradient dW = dy^T x has neither operand contiguous
# along its contraction (the tokens), the layout the library GEMM is
# slowest in, so it goes through the extension's linear_wgrad, which may
# transpose operands first (docs/KERNELS.md "Weight gradients").  `route`:
# -1 the measured per-shape table, 0 the library call as it was, 1 both
# operands transposed, 2 dy only.
def _rows(t):
    return t.reshape(-1, t.shape[-1])


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, route):
        ctx.save_for_backward(x, w)
        ctx.route = route
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2 = _rows(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ w).view(x.shape)
        if ctx.needs_input_grad[1]:
            dw = native().linear_wgrad(dy2.contiguous(),
                                       _rows(x).contiguous(), ctx.route)
        if ctx.needs_input_grad[2]:
            db = dy2.sum(0)
        return dx, dw, db, None


def linear(x, w, b=None, route: int = -1):
    """F.linear(x, w, b) whose bf16 GPU backward takes the weight
    gradient through linear_wgrad.  Forward values are F.linear's own."""
    if not (x.is_cuda and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16):
        return torch.nn.functional.linear(x, w, b)
    _require_native("linear")
    return _LinearFn.apply(x, w, b, route)


class _QKVLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wq, wk, wv, bq, bk, bv, route):
        ctx.save_for_backward(x, wq, wk, wv)
        ctx.route = route
        lin = torch.nn.functional.linear
        return lin(x, wq, bq), lin(x, wk, bk), lin(x, wv, bv)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x, wq, wk, wv = ctx.saved_tensors
        outs = [wq.shape[0], wk.shape[0], wv.shape[0]]
        # dq|dk|dv side by side: dx and the weight gradient are then one
        # GEMM each over the packed width, summed in fp32 and rounded once
        dy = torch.cat([_rows(dq), _rows(dk), _rows(dv)], dim=1)
        need = ctx.needs_input_grad
        dx = None
        if need[0]:
            dx = (dy @ torch.cat([wq, wk, wv], dim=0)).view(x.shape)
        dws = [None, None, None]
        if need[1] or need[2] or need[3]:
            dws = native().linear_wgrad(dy, _rows(x).contiguous(),
                                        ctx.route).split(outs, dim=0)
        dbs = [None, None, None]
        if need[4] or need[5] or need[6]:
            dbs = [d if need[4 + i] else None
                   for i, d in enumerate(dy.sum(0).split(outs))]
        return (dx, *dws, *dbs, None)


def qkv_linear(x, wq, wk, wv, bq=None, bk=None, bv=None, route: int = -1):
    """The q, k and v projections of one input as one autograd node:
    (F.linear(x, wq, bq), F.linear(x, wk, bk), F.linear(x, wv, bv)).  The
    bf16 GPU backward packs dq|dk|dv once and forms dx and the three
    weight gradients as one GEMM each (no elementwise adds, one bf16
    rounding per element)."""
    lin = torch.nn.functional.linear
    if not (x.is_cuda and x.dtype == torch.bfloat16
            and wq.dtype == torch.bfloat16):
        return lin(x, wq, bq), lin(x, wk, bk), lin(x, wv, bv)
    _require_native("qkv_linear")
    return _QKVLinearFn.apply(x, wq, wk, wv, bq, bk, bv, route)


def attn_decode_ref(q, kc, vc, kv_lens, slot_ids, scale):
    """q: [B, Hq, D]; kc/vc: [slots, S_max, Hkv, D]."""
    B, Hq, D = q.shape
    Hkv = kc.shape[2]
    rep = Hq // Hkv
    out = torch.empty_like(q)
    for i in range(B):
        slot = int(slot_ids[i])
        L = int(kv_lens[i])
        k = kc[slot, :L].float()  # [L, Hkv, D]
        v = vc[slot, :L].float()
        kf = k.repeat_interleave(rep, dim=1)  # [L, Hq, D]
        vf = v.repeat_interleave(rep, dim=1)
        att = torch.einsum("hd,lhd->hl", q[i].float(), kf) * scale
        p = att.softmax(-1)
        out[i] = torch.einsum("hl,lhd->hd", p, vf).to(q.dtype)
    return out


def attn_decode(q, kc, vc, kv_lens, slot_ids, scale):
    """Decode attention over the KV cache (no autograd)."""
    if q.is_cuda:
        C = _require_native("attn_decode")
        return C.attn_decode(q.contiguous(), kc, vc, kv_lens.int(),
                             slot_ids.int(), scale)
    return attn_decode_ref(q, kc, vc, kv_lens, slot_ids, scale)


def attn_append_ref(q, kc, vc, slot_ids, q_start, q_lens, scale):
    """q: [n, Sq, Hq, D] new (roped) rows; kc/vc: [slots, S_max, Hkv, D]
    with the chunk's own K/V already written at [slot, start:start+len].
    Row i < q_lens[b] attends cache rows kv <= q_start[b] + i and
    kv < min(q_start[b] + q_lens[b], S_max); rows >= q_lens[b] are
    padding and come back as zeros."""
    n, Sq, Hq, D = q.shape
    S_max, Hkv = kc.shape[1], kc.shape[2]
    rep = Hq // Hkv
    out = torch.zeros_like(q)
    for b in range(n):
        slot, start, ln = int(slot_ids[b]), int(q_start[b]), int(q_lens[b])
        if ln == 0:
            continue
        L = min(start + ln, S_max)
        # same op order as attention_ref, per sequence: [Hq, rows, D]
        qf = q[b, :ln].float().permute(1, 0, 2)
        kf = kc[slot, :L].float().permute(1, 0, 2).repeat_interleave(
            rep, dim=0)
        vf = vc[slot, :L].float().permute(1, 0, 2).repeat_interleave(
            rep, dim=0)
        att = torch.matmul(qf, kf.transpose(-1, -2)) * scale  # [Hq, ln, L]
        pos = start + torch.arange(ln, device=q.device)
        mask = torch.arange(L, device=q.device)[None, :] > pos[:, None]
        p = att.masked_fill(mask, float("-inf")).softmax(-1)
        out[b, :ln] = torch.matmul(p, vf).permute(1, 0, 2).to(q.dtype)
    return out


def attn_append(q, kc, vc, slot_ids, q_start, q_lens, scale):
    """Attention of a chunk of new tokens over the slot KV cache (chunked
    prefill, attention_append.hip; no autograd).  q [n, Sq, Hq, 128] with
    Sq % 64 == 0; slot_ids / q_start / q_lens are int32 [n] tensors on
    q's device (the GPU path never syncs on them).  The caller writes the
    chunk's K/V rows into the cache first.  Valid rows match
    attn_append_ref; padding rows are finite but unspecified on GPU."""
    if q.is_cuda:
        C = _require_native("attn_append")
        return C.attn_append(q.contiguous(), kc, vc, slot_ids, q_start,
                             q_lens, scale)
    return attn_append_ref(q, kc, vc, slot_ids, q_start, q_lens, scale)


# ---- FP8 KV cache (docs/KERNELS.md "FP8 KV cache") ------------------------
# A row is the 128 values of one (token, kv head), K or V: 128 OCP e4m3fn
# codes plus one E8M0 exponent byte e, scale 2^(e-127).  The two functions
# below are the definition, in plain torch with integer bit arithmetic;
# the kernels (kv_fp8.h) reproduce them bit for bit.
def kv_quantize(x: torch.Tensor):
    """x [..., D] -> (codes uint8 [..., D], exp uint8 [...]).  With
    amax = max |x_i| in fp32, n is the smallest integer with
    amax <= 448 * 2^n, clamped to [-126, 127] (0 for amax == 0); exp =
    n + 127 and code_i = e4m3fn(x_i * 2^-n), round to nearest even.  Both
    scalings are by a power of two and exact.  Rows holding NaN or Inf
    give unspecified contents."""
    xf = x.detach().float()
    amax = xf.abs().amax(-1)
    u = amax.contiguous().view(torch.int32) & 0x7FFFFFFF
    # 448 = 1.75 * 2^8, and 0x600000 is the fp32 mantissa of 1.75
    n = (u >> 23) - 135 + ((u & 0x7FFFFF) > 0x600000).to(torch.int32)
    n = n.clamp(-126, 127)
    n = torch.where(u == 0, torch.zeros_like(n), n)
    # 2^-n from its fp32 bits (n <= 121 for a finite amax)
    inv = ((127 - n).clamp(min=1) << 23).view(torch.float32)
    codes = (xf * inv.unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.contiguous(), (n + 127).to(torch.uint8)


def kv_dequantize(codes: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """codes uint8 [..., D], exp uint8 [...] -> code * 2^(exp-127) as
    fp32 (every such value is exactly representable in bf16)."""
    scale = (exp.to(torch.int32) << 23).view(torch.float32)
    return codes.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)


def kv_write_fp8(k, v, kc, vc, ke, ve, slot_ids, starts, lens):
    """Quantise rows of k, v [n, S, Hkv, 128] bf16 into the FP8 cache
    (kc, vc uint8 [slots, S_max, Hkv, 128]; ke, ve uint8 [slots, S_max,
    Hkv]): row i < lens[b] of sequence b goes to [slot_ids[b],
    starts[b] + i].  Rows at or past lens[b] or S_max are skipped, and so
    is a sequence whose slot is outside [0, slots) or whose start is
    negative.  slot_ids / starts / lens are int32 [n] on k's device; the
    GPU path (kv_write_fp8.hip, one launch) never syncs on them."""
    if k.is_cuda:
        C = _require_native("kv_write_fp8")
        C.kv_write_fp8(k.contiguous(), v.contiguous(), kc, vc, ke, ve,
                       slot_ids, starts, lens)
        return
    n, S = k.shape[0], k.shape[1]
    slots, S_max = kc.shape[0], kc.shape[1]
    for b in range(n):
        slot, start, ln = int(slot_ids[b]), int(starts[b]), int(lens[b])
        if slot < 0 or slot >= slots or start < 0:
            continue
        ln = min(ln, S, S_max - start)
        if ln <= 0:
            continue
        kc[slot, start:start + ln], ke[slot, start:start + ln] = \
            kv_quantize(k[b, :ln])
        vc[slot, start:start + ln], ve[slot, start:start + ln] = \
            kv_quantize(v[b, :ln])


def _kv_dequant_slots(kc, vc, ke, ve, slot_ids):
    """Dequantised copies of the slots in use, and their new indices."""
    idx = torch.as_tensor(slot_ids, device=kc.device).long()
    ok = (idx >= 0) & (idx < kc.shape[0])
    idx = torch.where(ok, idx, torch.zeros_like(idx))
    local = torch.where(ok, torch.arange(idx.numel(), device=kc.device),
                        torch.full_like(idx, -1))
    return (kv_dequantize(kc[idx], ke[idx]), kv_dequantize(vc[idx], ve[idx]),
            local)


def attn_decode_fp8(q, kc, vc, ke, ve, kv_lens, slot_ids, scale):
    """attn_decode over the dequantised rows of an FP8 cache.  CPU only:
    the GPU model path runs the fused attn_decode_qkv_fp8 and there is no
    unfused HIP kernel."""
    if q.is_cuda:
        raise RuntimeError(
            "skypilot_amd.ops.attn_decode_fp8 has no HIP kernel; the GPU "
            "path is attn_decode_qkv_fp8")
    kd, vd, local = _kv_dequant_slots(kc, vc, ke, ve, slot_ids)
    return attn_decode_ref(q, kd, vd, kv_lens, local, scale)


def attn_decode_qkv_fp8(qkv, kc, vc, ke, ve, cos, sin, positions, kv_lens,
                        slot_ids, Hq, Hkv, scale):
    """attn_decode_qkv over the FP8 KV cache (attention_decode_fp8.hip):
    rope of q and k in fp32, the current k and v quantised and written at
    (slot, position), attention over the dequantised rows 0..position, the
    current one included - the output is a function of the cache contents
    after the call.  CPU: the same composed from kv_quantize, the
    references and attn_decode_fp8."""
    D = kc.shape[3]
    if qkv.is_cuda:
        C = _require_native("attn_decode_qkv_fp8")
        return C.attn_decode_qkv_fp8(qkv.contiguous(), kc, vc, ke, ve, cos,
                                     sin, positions.int(), kv_lens.int(),
                                     slot_ids.int(), Hq, Hkv, scale)
    n = qkv.shape[0]
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    qr = rope_ref(q.reshape(n, Hq, D).float(), cos, sin, positions.long())
    kr = rope_ref(k.reshape(n, Hkv, D).float(), cos, sin, positions.long())
    sl, pos = slot_ids.long(), positions.long()
    kc[sl, pos], ke[sl, pos] = kv_quantize(kr)
    vc[sl, pos], ve[sl, pos] = kv_quantize(v.reshape(n, Hkv, D))
    return attn_decode_fp8(qr, kc, vc, ke, ve, kv_lens, slot_ids,
                           scale).to(qkv.dtype)


def attn_append_fp8(q, kc, vc, ke, ve, slot_ids, q_start, q_lens, scale):
    """attn_append over the FP8 KV cache (attention_append.hip): on the
    GPU bit-identical to attn_append on a bf16 cache holding
    kv_dequantize of the same codes.  The caller writes the chunk's rows
    first (kv_write_fp8)."""
    if q.is_cuda:
        C = _require_native("attn_append_fp8")
        return C.attn_append_fp8(q.contiguous(), kc, vc, ke, ve, slot_ids,
                                 q_start, q_lens, scale)
    kd, vd, local = _kv_dequant_slots(kc, vc, ke, ve, slot_ids)
    lens = torch.where(local < 0, torch.zeros_like(local),
                       torch.as_tensor(q_lens).long())
    return attn_append_ref(q, kd, vd, local.clamp(min=0), q_start, lens,
                           scale)


# ---- fp8 decode weights (serving) -------------------------
# Per-output-row e4m3fn quantization: W_row ~= scale_r * fp8(W_row/scale_r).
# Registered weights reroute decode_linear through the fp8 GEMV (half the
# streamed bytes on the weight-bandwidth-bound decode step).
_FP8_WEIGHTS: dict = {}


def quantize_fp8_rowwise(w: torch.Tensor):
    """bf16 [O, I] -> (uint8 e4m3fn [O, I], fp32 scale [O])."""
    wf = w.float()
    scale = wf.abs().amax(dim=1).clamp(min=1e-8) / 448.0
    q = (wf / scale[:, None]).clamp(-448.0, 448.0)
    q8 = q.to(torch.float8_e4m3fn).view(torch.uint8)
    return q8.contiguous(), scale.contiguous()


def register_fp8_weight(w: torch.Tensor) -> None:
    """Quantize and register a weight for fp8 decode GEMV routing."""
    q8, scale = quantize_fp8_rowwise(w)
    _FP8_WEIGHTS[w.data_ptr()] = (q8, scale)


def clear_fp8_weights() -> None:
    _FP8_WEIGHTS.clear()


def decode_linear(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """F.linear for the decode step: y = x @ W^T with x [.., n, in],
    n <= 8.  On GPU this runs the weight-bandwidth-bound skinny GEMV
    (skinny_gemm.hip, ~3x hipBLASLt on these shapes); otherwise (CPU,
    n > 8, odd inner dim) it falls back to F.linear.  No autograd —
    inference only."""
    lead = x.shape[:-1]
    n = 1
    for d in lead:
        n *= d
    i, o = x.shape[-1], weight.shape[0]
    wbytes = 2 * i * o
    # Measured routing (bench_gemv.py on MI355X, docs/BENCHMARKS.md):
    # n=1 always wins (W streams at 6.5-7.3 TB/s; hipBLASLt floors at
    # ~19 us/GEMM); n>=2 wins on small-W shapes (launch-bound for
    # hipBLASLt) and, via the R=4 multi-row variant, on vocab-sized
    # projections (O >= 100k) up to n<=4.
    use_native = (n == 1 or wbytes <= 34_000_000
                  or (o >= 100_000 and n <= 4))
    # fp8 pays only while the step is weight-bandwidth-bound: at n >= 3
    # the bf16 multirow GEMV amortizes the weight stream and fp8's
    # unpack VALU cost dominates (measured: @8 streams 1521 -> 1069
    # tok/s with fp8 everywhere).
    if (x.is_cuda and x.dtype == torch.bfloat16 and 1 <= n <= 2
            and i % 1024 == 0 and _FP8_WEIGHTS):
        ent = _FP8_WEIGHTS.get(weight.data_ptr())
        # data_ptr can be recycled after a free; require matching shape
        if ent is not None and tuple(ent[0].shape) != tuple(weight.shape):
            ent = None
        if ent is not None:
            C = _require_native("skinny_gemm_fp8")
            y = C.skinny_gemm_fp8(x.reshape(n, i).contiguous(), ent[0],
                                  ent[1])
            return y.view(*lead, o)
    if (use_native and x.is_cuda and x.dtype == torch.bfloat16
            and 1 <= n <= 8 and i % 512 == 0):
        C = _require_native("skinny_gemm")
        y = C.skinny_gemm(x.reshape(n, i).contiguous(), weight)
        return y.view(*lead, o)
    return torch.nn.functional.linear(x, weight)


def decode_norm_linear(x, res, norm_w, eps, weight):
    """Fused rmsnorm(x [+ res]) * norm_w -> fp8 GEMV in ONE kernel
    (skinny_gemm.hip norm-fused variant) — decode is dispatch-gap
    bound, so deleting the rmsnorm_res launch saves its kernel time
    AND the ~5 us graph-replay gap.  Returns (x2, y) with x2 = x+res
    (x itself when res is None).  Falls back to rmsnorm_res +
    decode_linear when the fp8 table or shape doesn't apply."""
    lead = x.shape[:-1]
    n = 1
    for d in lead:
        n *= d
    i = x.shape[-1]
    o = weight.shape[0]
    # MEASURED NEGATIVE as the default path (371 -> 246 tok/s @1):
    # the dot loop's x reads moved from global (4-deep vm pipeline,
    # latency hidden under the nontemporal weight stream) to flat-LDS
    # loads, which serialize on lgkmcnt and stall the stream.  The
    # launch+gap saving (~10 us) never amortized the per-block slowdown.
    # Kept as a tested lib op behind SKY_FP8_NORM_FUSED=1.
    fused_on = os.environ.get("SKY_FP8_NORM_FUSED", "0") == "1"
    if (fused_on and x.is_cuda and x.dtype == torch.bfloat16
            and 1 <= n <= 2 and i % 1024 == 0 and i <= 4096
            and o % 2 == 0 and _FP8_WEIGHTS):
        ent = _FP8_WEIGHTS.get(weight.data_ptr())
        if ent is not None and tuple(ent[0].shape) != tuple(weight.shape):
            ent = None
        if ent is not None:
            C = _require_native("skinny_gemm_fp8_norm")
            res2 = (res.reshape(n, i).contiguous() if res is not None
                    else torch.empty(0, dtype=x.dtype, device=x.device))
            x2, y = C.skinny_gemm_fp8_norm(
                x.reshape(n, i).contiguous(), res2,
                norm_w.to(x.dtype).contiguous(), eps, ent[0], ent[1],
                res is not None)
            return x2.view(*lead, i), y.view(*lead, o)
    if res is None:
        return x, decode_linear(rmsnorm(x, norm_w, eps), weight)
    x2, h = rmsnorm_res(x, res, norm_w, eps)
    return x2, decode_linear(h, weight)


def rmsnorm_res(x, res, weight, eps: float = 1e-5):
    """Fused (x + res, rmsnorm(x + res) * w) for the decode step (one
    kernel instead of add + norm; decode_fused.hip).  No autograd."""
    if x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 256 == 0:
        C = _require_native("rmsnorm_res")
        # the kernel reads bf16 weights; .to() of a bf16 weight is a no-op
        x2, h = C.rmsnorm_res(x.contiguous(), res.contiguous(),
                              weight.to(x.dtype).contiguous(), eps)
        return x2, h
    x2 = (x + res)
    return x2, rmsnorm(x2, weight, eps)


def decode_advance(logits, stage, ring, ctr):
    """Fused greedy decode advance: per-row argmax over `logits`
    [b, 1, V] plus the in-graph state bump — ring token store,
    stage[0] next-token feedback, stage[1]/[3]/[4] increments — in one
    launch (decode_fused.hip; replaces torch argmax+index_copy+copy_+
    3 adds; tie-break matches torch.argmax).  GPU-only: the decode
    graph never runs on CPU."""
    C = _require_native("decode_advance")
    C.decode_advance(logits.contiguous(), stage, ring, ctr)


# ---- seeded decode sampling (docs/KERNELS.md "Decode sampling") -----------
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10: 4 counter words and 2 key words in, 4 words out."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for r in range(10):
        if r:
            k0 = (k0 + 0x9E3779B9) & _M32
            k1 = (k1 + 0xBB67AE85) & _M32
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _M32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _M32)
    return (c0, c1, c2, c3)


def sample_uniform(seed: int, counter: int) -> float:
    """u in [0, 1) for one draw: the top 24 bits of Philox word 0."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((int(counter) & _M32, 0, 0, 0),
                      (seed & _M32, seed >> 32))[0]
    return (x >> 8) * 2.0 ** -24


def sample_row_reference(row, temperature, top_p, top_k, seed, counter):
    """One row of the sampling definition in fp64.  Returns a dict with
    the token and tau, and for sampled rows also the kept mask, the
    index-order prefix sums C over the kept set, Z_K and t = u * Z_K
    (what the GPU tests need to judge a kernel's token)."""
    l = row.detach().to("cpu").float().double().reshape(-1)
    V = l.numel()
    T, p, k = float(temperature), float(top_p), int(top_k)
    nan = torch.isnan(l)
    greedy_src = torch.where(nan, torch.full_like(l, float("-inf")), l)
    amax = int(greedy_src.argmax())      # first maximum; 0 if all -inf/NaN
    m = float(greedy_src[amax])
    out = {"token": amax, "tau": float("-inf"), "kept": None}
    if not T > 0 or bool(nan.any()) or not math.isfinite(m):
        return out
    w = torch.exp((l - m) / T)
    w[l == float("-inf")] = 0.0
    Z = float(w.sum())
    tau = float("-inf")
    if 0 < k < V:
        tau = max(tau, float(torch.sort(l, descending=True).values[k - 1]))
    if p < 1.0:
        if p <= 0.0:
            tau = max(tau, m)
        else:
            vals, inv = torch.unique(l, return_inverse=True)  # ascending
            gm = torch.zeros_like(vals).index_add_(0, inv, w)
            above = gm.flip(0).cumsum(0)   # mass at or above, descending
            hit = (above >= p * Z).nonzero()
            i = int(hit[0]) if hit.numel() else vals.numel() - 1
            tau = max(tau, float(vals.flip(0)[i]))
    kept = l >= tau
    C = torch.where(kept, w, torch.zeros_like(w)).cumsum(0)
    ZK = float(C[-1])
    t = sample_uniform(seed, counter) * ZK
    hit = (kept & (C > t)).nonzero()
    tok = int(hit[0]) if hit.numel() else int(kept.nonzero()[-1])
    out.update(token=tok, tau=tau, kept=kept, C=C, ZK=ZK, t=t)
    return out


def pack_samp(n, temperature, top_p, top_k, seed, counter=0):
    """CPU int32 [6, n]: temperature bits, top_p bits, top_k, seed_lo,
    seed_hi, counter.  Rows 0..4 are the `samp` block that
    decode_sample_advance takes, row 5 the counters of sample_tokens.
    Each argument is a scalar or n per-row values; top_k is clamped to
    int32 (any value outside [1, V) turns the filter off)."""
    def rowvec(x, dtype):
        if isinstance(x, torch.Tensor):
            t = x.detach().to(device="cpu").to(dtype).reshape(-1)
        else:
            t = torch.tensor(x, dtype=dtype).reshape(-1)
        return t.expand(n) if t.numel() == 1 else t

    def wrap64(x):
        if isinstance(x, torch.Tensor):
            return x
        if isinstance(x, (list, tuple)):
            return [wrap64(v) for v in x]
        x = int(x) & 0xFFFFFFFFFFFFFFFF
        return x - (1 << 64) if x >= (1 << 63) else x

    def wrap32(x):
        if isinstance(x, torch.Tensor):
            return x
        if isinstance(x, (list, tuple)):
            return [wrap32(v) for v in x]
        x = int(x) & _M32
        return x - (1 << 32) if x >= (1 << 31) else x

    def clamp_k(x):
        if isinstance(x, torch.Tensor):
            return x
        if isinstance(x, (list, tuple)):
            return [clamp_k(v) for v in x]
        return max(0, min(int(x), 2 ** 31 - 1))

    sd = rowvec(wrap64(seed), torch.int64)
    blk = torch.empty(6, n, dtype=torch.int32)
    blk[0] = rowvec(temperature, torch.float32).contiguous().view(torch.int32)
    blk[1] = rowvec(top_p, torch.float32).contiguous().view(torch.int32)
    blk[2] = rowvec(clamp_k(top_k), torch.int64).clamp(
        0, 2 ** 31 - 1).to(torch.int32)
    blk[3] = (sd & _M32).to(torch.int32)      # wraps to the low 32 bits
    blk[4] = (sd >> 32).to(torch.int32)
    blk[5] = rowvec(wrap32(counter), torch.int64).to(torch.int32)
    return blk


def sample_tokens_reference(logits, temperature, top_p, top_k, seed,
                            counter):
    """fp64 CPU reference of the decode sampling definition: logits
    [n, V] and per-row (or scalar) parameters -> (tokens int64 [n],
    tau fp32 [n]).  temperature and top_p are taken at fp32 precision,
    as the kernel receives them."""
    logits = logits.reshape(-1, logits.shape[-1])
    n = logits.shape[0]
    blk = pack_samp(n, temperature, top_p, top_k, seed, counter)
    Ts = blk[0].view(torch.float32).tolist()
    ps = blk[1].view(torch.float32).tolist()
    ks = blk[2].tolist()
    los, his, cs = blk[3].tolist(), blk[4].tolist(), blk[5].tolist()
    toks, taus = [], []
    for i in range(n):
        sd = ((his[i] & _M32) << 32) | (los[i] & _M32)
        r = sample_row_reference(logits[i], Ts[i], ps[i], ks[i], sd, cs[i])
        toks.append(r["token"])
        taus.append(r["tau"])
    return (torch.tensor(toks, dtype=torch.long),
            torch.tensor(taus, dtype=torch.float32))


def sample_tokens(logits, temperature, top_p, top_k, seed, counter):
    """Seeded temperature / top-k / top-p sampling of each row of
    `logits` [n, V] (decode_sample.hip on GPU, the fp64 reference on
    CPU).  Parameters are per-row tensors/lists or scalars; `counter` is
    the position of the token whose logits these are.  Returns (tokens
    int64 [n], tau fp32 [n]) — tau is the value threshold of the kept
    set, -inf when no filter is on or the row is greedy."""
    if not logits.is_cuda:
        return sample_tokens_reference(logits, temperature, top_p, top_k,
                                       seed, counter)
    C = _require_native("sample_tokens")
    if logits.dtype != torch.bfloat16 or logits.dim() != 2:
        raise ValueError("sample_tokens: logits must be bf16 [n, V] on GPU")
    n = logits.shape[0]
    blk = pack_samp(n, temperature, top_p, top_k, seed,
                    counter).to(logits.device)
    toks, tau = C.sample_tokens(logits.contiguous(), blk[:5], blk[5])
    return toks, tau


def decode_sample_advance(logits, stage, ring, ctr, samp):
    """decode_advance with seeded sampling: each row's token is drawn
    from `logits` [b, V] under samp [5, b] (temperature bits, top_p
    bits, top_k, seed_lo, seed_hi) with Philox counter stage[1], then
    the same ring store and stage bump as decode_advance
    (decode_sample.hip).  Rows with temperature 0 take the argmax.
    GPU-only: the decode graph never runs on CPU."""
    C = _require_native("decode_sample_advance")
    C.decode_sample_advance(logits.contiguous(), stage, ring, ctr, samp)


# ---- token log-probabilities (docs/KERNELS.md "Token log-probabilities") ---
LOGPROB_TOP = 20
_LOG2E_F32 = float(torch.tensor(1.44269504088896340736, dtype=torch.float32))


def _logprob_rowvec(x, n, dtype):
    if isinstance(x, torch.Tensor):
        t = x.detach().to(device="cpu").to(dtype).reshape(-1)
    else:
        t = torch.tensor(x, dtype=dtype).reshape(-1)
    if t.numel() == 1:
        t = t.expand(n)
    if t.numel() != n:
        raise ValueError(f"expected one value or {n} per-row values, got "
                         f"{t.numel()}")
    return t.contiguous()


def token_logprobs_reference(logits, ids, n_top):
    """fp64 CPU reference of the log-probability definition.  logits
    [n, V] (taken at their bf16/fp32 value), ids [n] chosen tokens, n_top
    scalar or [n] -> (lp fp32 [n], top_lp fp32 [n, 20], top_ids int32
    [n, 20]).

    Per row: m = max l, Z_q = sum floor(exp2((l - m) * log2e) * 2^40) as
    an integer (log2e the fp32 constant), lse = m + ln(Z_q * 2^-40),
    lp_j = fp32(l_j - lse).  The top list is the first min(N, V) tokens
    by (value descending, index ascending), padded with (-1, NaN).  A
    row with a NaN or an infinite maximum, an id outside [0, V) and a row
    that is off (n_top < 0) give NaN / -1."""
    l2 = logits.detach().to("cpu").float().double()
    l2 = l2.reshape(-1, l2.shape[-1])
    n, V = l2.shape
    ids_l = _logprob_rowvec(ids, n, torch.int64).tolist()
    nt_l = _logprob_rowvec(n_top, n, torch.int64).tolist()
    lp = torch.full((n,), float("nan"), dtype=torch.float32)
    top_lp = torch.full((n, LOGPROB_TOP), float("nan"), dtype=torch.float32)
    top_ids = torch.full((n, LOGPROB_TOP), -1, dtype=torch.int32)
    for i in range(n):
        N = min(nt_l[i], LOGPROB_TOP)
        if N < 0:
            continue
        l = l2[i]
        m = float(l.max())           # NaN if the row holds one
        if not math.isfinite(m):
            continue
        w = torch.floor(torch.exp2((l - m) * _LOG2E_F32) * 2.0 ** 40)
        zq = int(w.to(torch.int64).sum())
        lse = m + math.log(float(zq) * 2.0 ** -40)
        vals = (l - lse).float()
        if 0 <= ids_l[i] < V:
            lp[i] = vals[ids_l[i]]
        k = min(N, V)
        if k > 0:
            # stable and descending: equal values keep ascending indices
            order = torch.sort(l, descending=True, stable=True).indices[:k]
            top_ids[i, :k] = order.to(torch.int32)
            top_lp[i, :k] = vals[order]
    return lp, top_lp, top_ids


def token_logprobs(logits, ids, n_top, out=None):
    """Log-probabilities under each row of `logits` [n, V] at temperature
    1 with no filter: the value of the chosen token ids[i] and the top
    n_top[i] (<= 20) tokens (decode_sample.hip on GPU, the fp64 reference
    on CPU).  `n_top` is a scalar or per-row; -1 turns a row off.
    Returns (lp fp32 [n], top_lp fp32 [n, 20], top_ids int32 [n, 20]);
    unused entries are (-1, NaN).  On GPU `out` may give the three result
    tensors, whose off rows are then left untouched."""
    if not logits.is_cuda:
        return token_logprobs_reference(logits, ids, n_top)
    C = _require_native("token_logprobs")
    if logits.dtype != torch.bfloat16 or logits.dim() != 2:
        raise ValueError("token_logprobs: logits must be bf16 [n, V] on GPU")
    n, dev = logits.shape[0], logits.device
    if not (isinstance(ids, torch.Tensor) and ids.is_cuda):
        ids = _logprob_rowvec(ids, n, torch.int64).to(dev)
    if not (isinstance(n_top, torch.Tensor) and n_top.is_cuda):
        n_top = _logprob_rowvec(n_top, n, torch.int32).to(dev)
    if out is None:
        out = (torch.full((n,), float("nan"), dtype=torch.float32,
                          device=dev),
               torch.full((n, LOGPROB_TOP), float("nan"),
                          dtype=torch.float32, device=dev),
               torch.full((n, LOGPROB_TOP), -1, dtype=torch.int32,
                          device=dev))
    lp, top_lp, top_ids = out
    C.token_logprobs(logits.contiguous(), ids, n_top, lp, top_lp, top_ids)
    return lp, top_lp, top_ids


def decode_logprobs(logits, stage, n_top, lp_ring, top_lp_ring, top_id_ring,
                    ctr):
    """In-graph token_logprobs for the decode step, captured after the
    advance kernel and before ctr += 1: the chosen token of row i is
    stage[0, i], the results go to row ctr % chunk of the three rings
    (decode_sample.hip).  stage is only read.  GPU-only: the decode
    graph never runs on CPU."""
    C = _require_native("decode_logprobs")
    C.decode_logprobs(logits.contiguous(), stage, n_top, lp_ring,
                      top_lp_ring, top_id_ring, ctr)


def decode_swiglu_down(gu, weight):
    """silu(gate)*up followed by the down projection.  MEASURED
    NEGATIVE as a fused GEMV (skinny_gemm_swiglu kept for reference):
    fusing an elementwise producer into a GEMV recomputes it once PER
    OUTPUT ROW (O x M silu evaluations instead of M) — 289 -> 248
    tok/s single-stream.  The separate swiglu kernel + GEMV stays."""
    return decode_linear(swiglu(gu), weight)


def attn_decode_qkv(qkv, kc, vc, cos, sin, positions, kv_lens, slot_ids,
                    Hq, Hkv, scale):
    """Fused rope + KV-cache write + decode attention from the RAW
    packed qkv GEMV output (attention_decode.hip): the current token's
    roped k / raw v stay in registers for this step's attention (no
    write->read hazard) while one block per kv head writes the cache
    row for future steps.  Replaces rope_kvwrite + attn_decode (two
    launches -> one).  CPU/odd-D fallback composes the two ops."""
    D = kc.shape[3]
    if qkv.is_cuda and qkv.dtype == torch.bfloat16 and D == 128:
        C = _require_native("attn_decode_qkv")
        return C.attn_decode_qkv(qkv.contiguous(), kc, vc, cos, sin,
                                 positions.int(), kv_lens.int(),
                                 slot_ids.int(), Hq, Hkv, scale)
    q = rope_kvwrite(qkv, kc, vc, cos, sin, positions, slot_ids, Hq, Hkv)
    return attn_decode(q, kc, vc, kv_lens, slot_ids, scale)


def rope_kvwrite(qkv, kc, vc, cos, sin, positions, slot_ids, Hq, Hkv):
    """Packed-qkv rope + KV-cache scatter (decode_fused.hip): applies
    rope to the q and k segments of qkv [n, (Hq+2*Hkv)*D], writes the
    roped k and raw v rows into the caches at (slot_ids, positions),
    and returns contiguous roped q [n, Hq, D].  No autograd."""
    D = kc.shape[3]
    n = qkv.shape[0]
    if qkv.is_cuda and qkv.dtype == torch.bfloat16 and D == 128:
        C = _require_native("rope_kvwrite")
        return C.rope_kvwrite(qkv.contiguous(), kc, vc, cos, sin,
                              positions.int(), slot_ids.int(), Hq, Hkv)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    qr = rope(q.reshape(n, Hq, D), cos, sin, positions)
    kr = rope(k.reshape(n, Hkv, D), cos, sin, positions)
    pos = positions.long()
    kc[slot_ids.long(), pos] = kr
    vc[slot_ids.long(), pos] = v.reshape(n, Hkv, D)
    return qr


__all__ = [
    "rmsnorm", "rope", "attention", "fused_cross_entropy", "attn_decode",
    "swiglu", "linear", "qkv_linear",
    "decode_linear", "rmsnorm_res", "rope_kvwrite",
    "decode_swiglu_down",
    "native", "native_available", "rmsnorm_ref", "rope_ref",
    "attention_ref", "cross_entropy_ref", "attn_decode_ref",
    "attn_append", "attn_append_ref",
    "kv_quantize", "kv_dequantize", "kv_write_fp8", "attn_decode_qkv_fp8",
    "attn_append_fp8", "attn_decode_fp8",
]
