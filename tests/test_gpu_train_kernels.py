"""Elementwise fp64 checks of the per-step training kernels.

rmsnorm.hip, rope.hip, swiglu.hip, cross_entropy.hip and adamw.hip are
compared element by element with an fp64 evaluation of the same formula
on the same (bf16-rounded) inputs.  A whole-tensor norm cannot see one
wrong row, a dropped tail vector or a missing weight decay; a per-element
bound can.  The bound is built from what the kernel legitimately loses:

* a bf16 output (unit roundoff 2^-8) may be off by ``2 * 2^-8 * |ref|``
  per rounding it goes through;
* fp32 arithmetic may be off by ``4 * K * 2^-24 * A``: K is the number of
  terms reduced into the element (1 for pointwise ops), A the same formula
  evaluated with the absolute values of its terms (so cancellation is
  charged to the terms, not to the small result), and 4 covers FMA
  contraction and the few-ulp ``__expf``/``__logf``/``rsqrtf``;
* ``1e-30`` absolute lets values flushed to zero compare equal.

Every element has to be inside the bound; none is excluded.  Each check
prints the largest error it saw as a fraction of the bound (``pytest -s``).

The unmarked tests at the end run without a GPU: they pin the fp64
references to the package's own CPU fallbacks, and they feed the checker
results with one deliberate defect each to show that it rejects them.
"""
import functools
import math

import pytest
import torch

from _fp64_check import (TINY, U16, U32, bf16_values, check, f32, rejects,
                         tol_bf16, tol_f32, within)
from skypilot_amd import ops
from skypilot_amd.train.optim import FusedAdamW

gpu = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


# ===========================================================================
# fp64 references.  Each returns the result and the absolute-value
# evaluation A that scales its fp32 tolerance.
# ===========================================================================
def rmsnorm_fwd64(x, w, eps):
    x, w = x.double(), w.double()
    inv = torch.rsqrt(x.pow(2).mean(-1) + f32(eps))
    y = x * inv[:, None] * w
    return y, inv


def rmsnorm_bwd64(x, w, dy, inv):
    x, w, dy, inv = x.double(), w.double(), dy.double(), inv.double()
    H = x.shape[-1]
    inv = inv[:, None]
    t = dy * w * x
    k = t.sum(-1, keepdim=True) * inv * inv / H
    k_abs = t.abs().sum(-1, keepdim=True) * inv * inv / H
    dx = inv * (dy * w - x * k)
    A_dx = inv * ((dy * w).abs() + x.abs() * k_abs)
    s = dy * x * inv
    return dx, A_dx, s.sum(0), s.abs().sum(0)


def rope64(x, cos, sin, pos, backward=False):
    """x [T, H, D]; cos/sin [S, D/2]; pos [T]."""
    x = x.double()
    half = x.shape[-1] // 2
    c = cos.double()[pos.long()][:, None, :]
    s = sin.double()[pos.long()][:, None, :] * (-1.0 if backward else 1.0)
    x1, x2 = x[..., :half], x[..., half:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    A = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                   (x2 * c).abs() + (x1 * s).abs()], -1)
    return y, A


def swiglu64(gu, dy=None):
    gu = gu.double()
    M = gu.shape[-1] // 2
    g, u = gu[..., :M], gu[..., M:]
    sg = 1.0 / (1.0 + torch.exp(-g))
    y = g * sg * u
    if dy is None:
        return y
    d = dy.double()
    dg = d * u * (sg + g * sg * (1 - sg))
    # 1 - sg is itself a difference of two terms
    A_dg = (d * u).abs() * (sg + g.abs() * sg * (1 + sg))
    du = d * g * sg
    return y, torch.cat([dg, du], -1), torch.cat([A_dg, du.abs()], -1)


def cross_entropy64(logits, targets, grad_scale, ignore_index=-100):
    """Per-row loss [N] (+ its A) and d_logits * grad_scale (+ its A).
    Ignored rows are defined as zero loss and zero gradient."""
    l = logits.double()
    N, V = l.shape
    valid = targets != ignore_index
    tgt = torch.where(valid, targets, torch.zeros_like(targets)).long()
    mx = l.max(-1).values
    logse = torch.log(torch.exp(l - mx[:, None]).sum(-1))
    tl = l.gather(1, tgt[:, None])[:, 0]
    loss = (logse + mx - tl) * valid
    A_loss = (logse.abs() + mx.abs() + tl.abs()) * valid
    p = torch.exp(l - (logse + mx)[:, None])
    onehot = torch.zeros_like(p).scatter_(1, tgt[:, None], 1.0)
    grad = (p - onehot) * grad_scale * valid[:, None]
    A_grad = (p + onehot) * abs(grad_scale) * valid[:, None]
    return loss, A_loss, grad, A_grad


def adamw64(p0, grads, lr, betas, eps, wd, grad_scale, decay,
            first_step=1):
    """The AdamW recurrence, written out.  p0: initial fp32 master values
    per tensor; grads[s][i]: gradient of tensor i at step s; decay[i]:
    whether tensor i is decayed.  Returns states[s][i] = (master, m, v)
    after step s.  Hyper-parameters are rounded to fp32 first, as the
    kernel receives them."""
    lr, b1, b2, eps, wd = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), \
        f32(wd)
    p = [t.double().clone() for t in p0]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    states = []
    for s, gs in enumerate(grads):
        step = first_step + s
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        for i, g in enumerate(gs):
            g = g.double() * grad_scale
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            upd = (m[i] / bc1) / (torch.sqrt(v[i] / bc2) + eps)
            p[i] = p[i] - lr * (upd + (wd if decay[i] else 0.0) * p[i])
        states.append([(p[i].clone(), m[i].clone(), v[i].clone())
                       for i in range(len(p))])
    return states


# ===========================================================================
# Cases: inputs (CPU, bf16-rounded) and their references, built once.
# ===========================================================================
RMS_SHAPES = [
    (1, 8), (3, 264),
    (5, 2048), (5, 2056),    # bwd NV 1 -> 2 (nvec 256 | 257)
    (2, 4104), (2, 8200),    # bwd NV 4 (nvec 513), NV 8 (nvec 1025)
    (2, 16384),              # widest row the backward kernel holds
    (513, 264),              # bwd grid cap 512: block 0 does rows 0 and 512
    (2049, 264),             # fwd grid cap 2048: block 0 does rows 0, 2048
    (1300, 512),             # bwd: two or three rows per block
]
RMS_EPS = [1e-5, 1e-6]


@functools.lru_cache(maxsize=None)
def rms_case(rows, H):
    g = torch.Generator().manual_seed(1000 + 31 * rows + H)
    x = torch.randn(rows, H, generator=g) * 2
    if rows >= 2:
        # Rows with very different 1/rms (about 5e-4 and 3e2, where eps
        # matters): an inv_rms applied to the wrong row cannot hide.  In
        # the grid-stride shapes both belong to block 0.
        x[0] *= 1e3
        x[-1] *= 1e-3
    w = torch.randn(H, generator=g) * 0.5 + 1
    dy = torch.randn(rows, H, generator=g)
    return bf16_values(x), bf16_values(w), bf16_values(dy)


ROPE_CASES = [
    # (T, H, D)
    (4100, 9, 128),   # 36900 rows > 32768: second pass of the vector loop
    (1, 1, 128),
    (7, 3, 256),      # vector kernel, 8 pairs per lane
    (7, 3, 32), (7, 3, 64), (7, 3, 96),   # scalar kernel, D % 32 == 0
    (7, 3, 80),                           # scalar kernel, D % 32 != 0
]


@functools.lru_cache(maxsize=None)
def rope_case(T, H, D):
    g = torch.Generator().manual_seed(2000 + 7 * T + 3 * H + D)
    half = D // 2
    S = T + 5  # the table is longer than the batch
    inv_freq = 1.0 / (10000.0 ** (torch.arange(half).double() / half))
    freqs = torch.outer(torch.arange(S).double(), inv_freq)
    cos, sin = freqs.cos().float(), freqs.sin().float()
    # random, repeated, non-monotonic; first and last table row included
    pos = torch.randint(0, S, (T,), generator=g, dtype=torch.int32)
    pos[-1] = S - 1
    if T >= 3:
        pos[0] = 0
        pos[2] = pos[1]
    # Neighbouring (token, head) rows differ in magnitude, so a store that
    # spills into the next row leaves a value of the wrong size there.
    scale = 2.0 ** ((torch.arange(T * H) * 7) % 11 - 5).double()
    x = torch.randn(T, H, D, generator=g) * scale.view(T, H, 1).float()
    return bf16_values(x), cos, sin, pos


SWIGLU_SHAPES = [(1, 8), (3, 520), (257, 1032)]


@functools.lru_cache(maxsize=None)
def swiglu_case(rows, M):
    g = torch.Generator().manual_seed(3000 + rows + M)
    gate = torch.randn(rows, M, generator=g) * 3
    up = torch.randn(rows, M, generator=g) * 2
    # Saturating gates (sigmoid -> 0 or 1, __expf(100) = inf) next to
    # large up values, in the first and in the last vector of a row.
    special = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0])
    gate[0, :5] = special
    up[0, :5] *= 1e3
    gate[-1, -5:] = special
    up[-1, -5:] = torch.tensor([1e4, -3e4, 2e4, -1e4, 5e4])
    dy = torch.randn(rows, M, generator=g)
    return bf16_values(torch.cat([gate, up], -1)), bf16_values(dy)


CE_CASES = ["tiny", "tail", "tail80", "stride"]
IGN = -100


@functools.lru_cache(maxsize=None)
def ce_case(name):
    g = torch.Generator().manual_seed(4000 + len(name) + ord(name[-1]))
    if name == "tiny":
        N, V = 3, 8
        logits = torch.randn(N, V, generator=g) * 2
        logits[2] = 1.5                     # a row of equal logits
        targets = torch.tensor([0, 7, 3])
    elif name in ("tail", "tail80"):
        N, V = 5, 1003                      # V % 8 == 3: scalar tail
        logits = torch.randn(N, V, generator=g) * 2
        logits[4] = -2.25
        # column 0, last column, inside the tail, ignored, middle
        targets = torch.tensor([0, V - 1, V - 2, IGN, 500])
        if name == "tail80":
            # row maximum about +80, minimum about -80
            lo = logits.min(-1, keepdim=True).values
            hi = logits.max(-1, keepdim=True).values
            logits[:4] = ((logits - lo) / (hi - lo) * 160 - 80)[:4]
    else:
        N, V = 2051, 520                    # grid cap 2048
        logits = torch.randn(N, V, generator=g) * 2
        targets = torch.randint(0, V, (N,), generator=g)
        targets[torch.randperm(N, generator=g)[:40]] = IGN
        # block b does rows b and b + 2048:
        targets[0], targets[2048] = IGN, 3      # ignored then valid
        targets[1], targets[2049] = 5, IGN      # valid then ignored
        targets[2], targets[2050] = IGN, IGN    # ignored then ignored
    return bf16_values(logits), targets.int()


ADAMW_SHAPES = [(1,), (3,), (31,), (65536,), (65537,), (131077,),
                (256, 512)]
ADAMW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
ADAMW_GRAD_SCALE = 0.25
ADAMW_STEPS = 4


@functools.lru_cache(maxsize=None)
def adamw_case():
    """The issue fixes the state tolerance as purely relative
    (16 * 2^-24 * step), which fp32 can only meet where nothing cancels.
    So each element keeps the sign of its gradient over the steps (fresh
    magnitudes, spread over about three decades) and parameters start
    with |p| in [0.5, 2]: then m, v and the master weight are sums of
    same-signed or dominated terms, and the bound is the kernel's to
    meet."""
    g = torch.Generator().manual_seed(5000)
    p0, grads = [], [[] for _ in range(ADAMW_STEPS)]
    for s in ADAMW_SHAPES:
        sign = torch.randint(0, 2, s, generator=g) * 2.0 - 1
        p0.append(bf16_values((torch.rand(s, generator=g) * 1.5 + 0.5)
                              * (torch.randint(0, 2, s, generator=g) * 2.0
                                 - 1)))
        for st in range(ADAMW_STEPS):
            mag = torch.exp(torch.randn(s, generator=g) * 1.5)
            grads[st].append(bf16_values(sign * mag))
    decay = [len(s) >= 2 for s in ADAMW_SHAPES]
    ref = adamw64(p0, grads, ADAMW["lr"], ADAMW["betas"], ADAMW["eps"],
                  ADAMW["weight_decay"], ADAMW_GRAD_SCALE, decay)
    return p0, grads, decay, ref


def adamw_tol(ref, step):
    return 16 * U32 * step * ref.abs() + TINY


def run_adamw(device, bucket_views, check_fn=check, **overrides):
    """Drive FusedAdamW for ADAMW_STEPS steps and compare the fp32 state
    with the fp64 recurrence after every step.  bucket_views=True hands
    the gradients over the way the bucketed DDP does: ``p._sky_grad``
    views into one flat bf16 buffer, here at element offsets of 2 mod 4
    (4-byte but not 8-byte aligned), which the optimizer answers with its
    per-tensor launch path."""
    p0, grads, decay, ref = adamw_case()
    params = [p.bfloat16().to(device).requires_grad_() for p in p0]
    kw = dict(ADAMW, decay_2d_only=True)
    grad_scale = overrides.pop("grad_scale", ADAMW_GRAD_SCALE)
    first_step = overrides.pop("first_step", 1)
    kw.update(overrides)
    opt = FusedAdamW(params, **kw)
    opt.step_count = first_step - 1
    assert opt.decay_mask == decay
    if bucket_views:
        offs, off = [], 2
        for p in params:
            offs.append(off)
            off = (off + p.numel() + 3) // 4 * 4 + 2
        flat = torch.zeros(off, dtype=torch.bfloat16, device=device)
        bufs = [flat[o:o + p.numel()].view_as(p)
                for o, p in zip(offs, params)]
        for p, b in zip(params, bufs):
            assert b.data_ptr() % 8 == 4
            p._sky_grad = b
    else:
        bufs = [torch.empty_like(p) for p in params]
        for p, b in zip(params, bufs):
            p.grad = b
    for s in range(ADAMW_STEPS):
        for b, gr in zip(bufs, grads[s]):
            b.copy_(gr.bfloat16())
        opt.step(grad_scale=grad_scale)
        if device.type == "cuda":
            # the launch path that was meant is the one that ran
            assert (opt._mt is None) == bucket_views
            assert (opt._mt_meta(opt._grads()) is None) == bucket_views
        for i, shape in enumerate(ADAMW_SHAPES):
            tag = f"adamw{'/views' if bucket_views else ''} step {s + 1} " \
                  f"{shape}"
            rp, rm, rv = ref[s][i]
            assert opt.master[i].dtype == torch.float32
            check_fn(f"{tag} master", opt.master[i], rp, adamw_tol(rp, s + 1))
            check_fn(f"{tag} exp_avg", opt.exp_avg[i], rm,
                     adamw_tol(rm, s + 1))
            check_fn(f"{tag} exp_avg_sq", opt.exp_avg_sq[i], rv,
                     adamw_tol(rv, s + 1))
            assert torch.equal(params[i].detach(),
                               opt.master[i].bfloat16()), tag
    return opt, params


# ===========================================================================
# GPU tests.
# ===========================================================================
@gpu
@pytest.mark.parametrize("eps", RMS_EPS)
@pytest.mark.parametrize("rows,H", RMS_SHAPES)
def test_rmsnorm_fwd_bwd_fp64(rows, H, eps):
    C = ops.native()
    x, w, dy = rms_case(rows, H)
    xg, wg, dyg = (t.bfloat16().to(dev()) for t in (x, w, dy))
    inv_g = torch.full((rows,), float("nan"), device=dev())
    y = C.rmsnorm_fwd(xg, wg, inv_g, eps)
    y_ref, inv_ref = rmsnorm_fwd64(x, w, eps)
    tag = f"rmsnorm ({rows},{H}) eps={eps}"
    # mean(x^2) reduces H terms into inv, and through it into y
    check(f"{tag} inv_rms", inv_g, inv_ref, tol_f32(inv_ref, K=H))
    check(f"{tag} y", y, y_ref, tol_bf16(y_ref, y_ref.abs(), K=H))

    dx, dw = C.rmsnorm_bwd(xg, wg, dyg, inv_g)
    assert dw.dtype == torch.float32
    # backward takes inv_rms as an input: the reference uses the same one
    dx_ref, A_dx, dw_ref, A_dw = rmsnorm_bwd64(x, w, dy, inv_g.cpu())
    check(f"{tag} dx", dx, dx_ref, tol_bf16(dx_ref, A_dx, K=H))
    check(f"{tag} dw", dw, dw_ref, tol_f32(A_dw, K=rows))


@gpu
@pytest.mark.parametrize("T,H,D", ROPE_CASES)
def test_rope_fwd_bwd_fp64(T, H, D):
    C = ops.native()
    x, cos, sin, pos = rope_case(T, H, D)
    xg = x.bfloat16().to(dev())
    cg, sg, pg = cos.to(dev()), sin.to(dev()), pos.to(dev())
    tag = f"rope ({T},{H},{D})"
    y = C.rope(xg, cg, sg, pg, False)
    y_ref, A = rope64(x, cos, sin, pos)
    check(f"{tag} fwd", y, y_ref, tol_bf16(y_ref, A))
    b = C.rope(xg, cg, sg, pg, True)
    b_ref, A_b = rope64(x, cos, sin, pos, backward=True)
    check(f"{tag} bwd", b, b_ref, tol_bf16(b_ref, A_b))

    # Round trip: y = bf16(R x) carries one rounding e with
    # |e| <= 2^-8 |y|, the way back maps it to |c||e1| + |s||e2| and
    # rounds once more; cos^2 + sin^2 = 1 only to fp32 accuracy.
    z = C.rope(y, cg, sg, pg, True)
    _, A_e = rope64(y_ref.abs(), cos.abs(), sin.abs(), pos, backward=True)
    x64 = x.double()
    half = D // 2
    xsum = x64[..., :half].abs() + x64[..., half:].abs()
    tol = (1 + 2 ** -6) * U16 * (A_e + x64.abs()) \
        + 16 * U32 * torch.cat([xsum, xsum], -1) + TINY
    check(f"{tag} round trip", z, x64, tol)

    if T >= 3:
        # Rows are independent: without the first and last token the
        # rest comes out bit-identical (nothing leaked across a row end).
        inner = C.rope(xg[1:-1], cg, sg, pg[1:-1], False)
        assert torch.equal(inner, y[1:-1]), tag


@gpu
@pytest.mark.parametrize("D", [64, 128])
def test_rope_autograd_and_batched_positions(D):
    """ops.rope: backward is the -sin kernel, and a [T] position vector
    broadcasts over a leading batch dimension as on the CPU."""
    T, H = 7, 3
    x, cos, sin, pos = rope_case(T, H, D)
    cg, sg, pg = cos.to(dev()), sin.to(dev()), pos.to(dev())
    xg = x.bfloat16().to(dev()).requires_grad_()
    y = ops.rope(xg, cg, sg, pg)
    y_ref, A = rope64(x, cos, sin, pos)
    check(f"ops.rope D={D} fwd", y, y_ref, tol_bf16(y_ref, A))
    dy = torch.flip(x, (0,))
    y.backward(dy.bfloat16().to(dev()))
    g_ref, A_g = rope64(dy, cos, sin, pos, backward=True)
    check(f"ops.rope D={D} bwd", xg.grad, g_ref, tol_bf16(g_ref, A_g))

    x4 = torch.stack([x, dy]).bfloat16().to(dev())      # [2, T, H, D]
    y4 = ops.rope(x4, cg, sg, pg)
    dy_ref, A_dy = rope64(dy, cos, sin, pos)
    check(f"ops.rope D={D} 4-D", y4, torch.stack([y_ref, dy_ref]),
          tol_bf16(torch.stack([y_ref, dy_ref]), torch.stack([A, A_dy])))


@gpu
@pytest.mark.parametrize("rows,M", SWIGLU_SHAPES)
def test_swiglu_fwd_bwd_fp64(rows, M):
    C = ops.native()
    gu, dy = swiglu_case(rows, M)
    gug, dyg = gu.bfloat16().to(dev()), dy.bfloat16().to(dev())
    y_ref, dgu_ref, A_dgu = swiglu64(gu, dy)
    tag = f"swiglu ({rows},{M})"
    y = C.swiglu_fwd(gug)
    check(f"{tag} y", y, y_ref, tol_bf16(y_ref, y_ref.abs()))
    dgu = C.swiglu_bwd(gug, dyg)
    check(f"{tag} dgu", dgu, dgu_ref, tol_bf16(dgu_ref, A_dgu))


def ce_loss_tol(A_loss, V):
    return tol_f32(A_loss, K=V)


@gpu
@pytest.mark.parametrize("name", CE_CASES)
def test_cross_entropy_kernel_fp64(name):
    C = ops.native()
    logits, targets = ce_case(name)
    N, V = logits.shape
    gs = 0.37
    buf = logits.bfloat16().to(dev())
    loss = C.cross_entropy_fused(buf, targets.to(dev()), gs, IGN)
    loss_ref, A_loss, grad_ref, A_grad = cross_entropy64(logits, targets,
                                                         f32(gs))
    tag = f"cross_entropy {name} ({N},{V})"
    check(f"{tag} loss", loss, loss_ref, ce_loss_tol(A_loss, V))
    # sum(exp) reduces V terms into every gradient element
    check(f"{tag} grad", buf, grad_ref, tol_bf16(grad_ref, A_grad, K=V))
    ign = targets == IGN
    assert torch.all(loss.cpu()[ign] == 0)
    assert torch.all(buf.cpu()[ign] == 0)


@gpu
@pytest.mark.parametrize("name", CE_CASES)
def test_cross_entropy_autograd_fp64(name):
    """ops.fused_cross_entropy: mean loss, and backward of 3 * loss."""
    logits, targets = ce_case(name)
    N, V = logits.shape
    n_valid = int((targets != IGN).sum())
    lg = logits.bfloat16().to(dev()).requires_grad_()
    loss = ops.fused_cross_entropy(lg, targets.to(dev()), IGN)
    (3.0 * loss).backward()
    loss_ref, A_loss, grad_ref, A_grad = cross_entropy64(
        logits, targets, f32(1.0 / n_valid))
    tag = f"fused_cross_entropy {name}"
    # per-row losses, then an fp32 sum of N of them
    mean_tol = (ce_loss_tol(A_loss, V).sum() + tol_f32(A_loss.sum(), K=N)) \
        / n_valid
    check(f"{tag} loss", loss, loss_ref.sum() / n_valid, mean_tol)
    # d_logits is rounded to bf16 by the kernel and again by the scaling
    check(f"{tag} grad", lg.grad, 3 * grad_ref,
          tol_bf16(3 * grad_ref, 3 * A_grad, K=V, roundings=2))
    assert torch.all(lg.grad.cpu()[targets == IGN] == 0)


@gpu
def test_cross_entropy_all_rows_ignored():
    """Defined as zero loss and zero gradient (torch returns NaN)."""
    C = ops.native()
    logits, _ = ce_case("tail")
    targets = torch.full((logits.shape[0],), IGN, dtype=torch.int32,
                         device=dev())
    buf = logits.bfloat16().to(dev())
    loss = C.cross_entropy_fused(buf, targets, 1.0, IGN)
    assert torch.all(loss == 0) and torch.all(buf == 0)
    lg = logits.bfloat16().to(dev()).requires_grad_()
    mean = ops.fused_cross_entropy(lg, targets, IGN)
    (3.0 * mean).backward()
    assert mean.item() == 0.0
    assert torch.all(lg.grad == 0)


def _assert_decay_only_2d(opt):
    """The reference decays the matrix and nothing else.  Show that the
    distinction is visible: the state must NOT match a reference with the
    decay mask inverted."""
    p0, grads, decay, _ = adamw_case()
    inverted = adamw64(p0, grads, ADAMW["lr"], ADAMW["betas"], ADAMW["eps"],
                       ADAMW["weight_decay"], ADAMW_GRAD_SCALE,
                       [not d for d in decay])
    for i in range(len(ADAMW_SHAPES)):
        rp = inverted[-1][i][0]
        ok, _, _ = within(opt.master[i], rp, adamw_tol(rp, ADAMW_STEPS))
        assert not ok, ADAMW_SHAPES[i]


@gpu
@pytest.mark.parametrize("bucket_views", [False, True],
                         ids=["multi_tensor", "per_tensor_views"])
def test_adamw_fp64(bucket_views):
    opt, _ = run_adamw(dev(), bucket_views)
    _assert_decay_only_2d(opt)


@gpu
def test_argument_validation():
    """Every shape or dtype the kernels cannot handle is rejected before
    a launch."""
    C = ops.native()
    d = dev()

    def bf(*shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=d)

    def f(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=d)

    pos2 = torch.zeros(2, dtype=torch.int32, device=d)
    bad_calls = {
        # rope
        "rope odd D": lambda: C.rope(bf(2, 1, 7), f(4, 3), f(4, 3), pos2,
                                     False),
        "rope positions count": lambda: C.rope(
            bf(2, 3, 2, 8), f(4, 4), f(4, 4), pos2, False),
        "rope cos dtype": lambda: C.rope(
            bf(2, 1, 8), f(4, 4, dtype=torch.float64), f(4, 4), pos2, False),
        "rope sin dtype": lambda: C.rope(
            bf(2, 1, 8), f(4, 4), f(4, 4, dtype=torch.bfloat16), pos2,
            False),
        "rope cos strided": lambda: C.rope(
            bf(2, 1, 8), f(4, 8)[:, ::2], f(4, 4), pos2, False),
        "rope sin on cpu": lambda: C.rope(
            bf(2, 1, 8), f(4, 4), torch.zeros(4, 4), pos2, False),
        "rope table width": lambda: C.rope(
            bf(2, 1, 8), f(4, 8), f(4, 8), pos2, False),
        # rmsnorm
        "rmsnorm_fwd w size": lambda: C.rmsnorm_fwd(bf(2, 16), bf(8), f(2),
                                                    1e-5),
        "rmsnorm_bwd w size": lambda: C.rmsnorm_bwd(bf(2, 16), bf(8),
                                                    bf(2, 16), f(2)),
        "rmsnorm_bwd H % 8": lambda: C.rmsnorm_bwd(bf(2, 12), bf(12),
                                                   bf(2, 12), f(2)),
        "rmsnorm_bwd H > 16384": lambda: C.rmsnorm_bwd(
            bf(1, 16392), bf(16392), bf(1, 16392), f(1)),
        "rmsnorm_bwd dy dtype": lambda: C.rmsnorm_bwd(bf(2, 16), bf(16),
                                                      f(2, 16), f(2)),
        "rmsnorm_bwd dy strided": lambda: C.rmsnorm_bwd(
            bf(2, 16), bf(16), bf(2, 32)[:, ::2], f(2)),
        "rmsnorm_bwd dy shape": lambda: C.rmsnorm_bwd(bf(2, 16), bf(16),
                                                      bf(4, 8), f(2)),
        "rmsnorm_bwd inv dtype": lambda: C.rmsnorm_bwd(
            bf(2, 16), bf(16), bf(2, 16), f(2, dtype=torch.float64)),
        "rmsnorm_bwd inv count": lambda: C.rmsnorm_bwd(bf(2, 16), bf(16),
                                                       bf(2, 16), f(1)),
        # swiglu
        "swiglu_fwd odd width": lambda: C.swiglu_fwd(bf(2, 15)),
        "swiglu_fwd M % 8": lambda: C.swiglu_fwd(bf(2, 24)),
        "swiglu_bwd M % 8": lambda: C.swiglu_bwd(bf(2, 24), bf(2, 12)),
        "swiglu_bwd dy dtype": lambda: C.swiglu_bwd(bf(2, 16), f(2, 8)),
        "swiglu_bwd dy shape": lambda: C.swiglu_bwd(bf(2, 16), bf(2, 16)),
    }
    for name, call in bad_calls.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name}: accepted")


# ===========================================================================
# CPU part 1: the fp64 references agree with the package's CPU fallbacks.
# The fallbacks compute in fp32; given fp32 tensors (holding bf16 values)
# they also return fp32, so only the fp32 term of the bound applies.
# ===========================================================================
@pytest.mark.parametrize("rows,H", [(1, 8), (3, 264), (5, 2056)])
def test_rmsnorm_reference_matches_cpu_fallback(rows, H):
    x, w, dy = rms_case(rows, H)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = ops.rmsnorm(xr, wr, 1e-5)
    y.backward(dy)
    y_ref, inv = rmsnorm_fwd64(x, w, 1e-5)
    dx_ref, A_dx, dw_ref, A_dw = rmsnorm_bwd64(x, w, dy, inv)
    check("cpu rmsnorm y", y, y_ref, tol_f32(y_ref.abs(), K=H))
    check("cpu rmsnorm dx", xr.grad, dx_ref, tol_f32(A_dx, K=H))
    check("cpu rmsnorm dw", wr.grad, dw_ref, tol_f32(A_dw, K=max(rows, H)))


@pytest.mark.parametrize("T,H,D", [(1, 1, 128), (7, 3, 64), (7, 3, 80)])
def test_rope_reference_matches_cpu_fallback(T, H, D):
    x, cos, sin, pos = rope_case(T, H, D)
    xr = x.clone().requires_grad_()
    y = ops.rope(xr, cos, sin, pos)
    y.backward(torch.flip(x, (0,)))
    y_ref, A = rope64(x, cos, sin, pos)
    g_ref, A_g = rope64(torch.flip(x, (0,)), cos, sin, pos, backward=True)
    check("cpu rope fwd", y, y_ref, tol_f32(A))
    check("cpu rope bwd", xr.grad, g_ref, tol_f32(A_g))


@pytest.mark.parametrize("rows,M", [(1, 8), (3, 520)])
def test_swiglu_reference_matches_cpu_fallback(rows, M):
    gu, dy = swiglu_case(rows, M)
    gr = gu.clone().requires_grad_()
    y = ops.swiglu(gr)
    y.backward(dy)
    y_ref, dgu_ref, A_dgu = swiglu64(gu, dy)
    check("cpu swiglu y", y, y_ref, tol_f32(y_ref.abs()))
    check("cpu swiglu dgu", gr.grad, dgu_ref, tol_f32(A_dgu))


@pytest.mark.parametrize("name", ["tiny", "tail"])
def test_cross_entropy_reference_matches_cpu_fallback(name):
    logits, targets = ce_case(name)
    N, V = logits.shape
    n_valid = int((targets != IGN).sum())
    lr = logits.clone().requires_grad_()
    loss = ops.fused_cross_entropy(lr, targets, IGN)
    (3.0 * loss).backward()
    loss_ref, A_loss, grad_ref, A_grad = cross_entropy64(
        logits, targets, 1.0 / n_valid)
    mean_tol = (ce_loss_tol(A_loss, V).sum() + tol_f32(A_loss.sum(), K=N)) \
        / n_valid
    check("cpu ce loss", loss, loss_ref.sum() / n_valid, mean_tol)
    check("cpu ce grad", lr.grad, 3 * grad_ref, tol_f32(3 * A_grad, K=V))
    assert torch.all(lr.grad[targets == IGN] == 0)


@pytest.mark.parametrize("bucket_views", [False, True])
def test_adamw_reference_matches_cpu_fallback(bucket_views):
    opt, _ = run_adamw(torch.device("cpu"), bucket_views)
    _assert_decay_only_2d(opt)


# ===========================================================================
# CPU part 2: the checker rejects known-wrong results, one defect each.
# ===========================================================================
def _collect_failures(log):
    def fn(name, got, ref, tol):
        if rejects(got, ref, tol):
            log.append(name)
    return fn


def test_checker_rejects_adamw_without_weight_decay():
    log = []
    run_adamw(torch.device("cpu"), False, check_fn=_collect_failures(log),
              weight_decay=0.0)
    assert any("(256, 512) master" in n and "step 1" in n for n in log)
    # the undecayed 1-D tensors and all moments are still right
    assert all("(256, 512) master" in n for n in log), log


def test_checker_rejects_adamw_ignoring_grad_scale():
    """Adam's update barely depends on the gradient's scale, so the
    parameters alone would not show this; the moments do."""
    log = []
    run_adamw(torch.device("cpu"), False, check_fn=_collect_failures(log),
              grad_scale=1.0)
    for shape in ADAMW_SHAPES:
        assert f"adamw step 1 {shape} exp_avg" in log
        assert f"adamw step 1 {shape} exp_avg_sq" in log


def test_checker_rejects_adamw_bias_correction_of_wrong_step():
    log = []
    run_adamw(torch.device("cpu"), False, check_fn=_collect_failures(log),
              first_step=2)
    # the recurrence of the moments does not know the step: only the
    # master weights are off, from the first step on
    for shape in ADAMW_SHAPES:
        assert f"adamw step 1 {shape} master" in log
    assert all("master" in n for n in log), log


def test_checker_rejects_flipped_sin():
    x, cos, sin, pos = rope_case(7, 3, 64)
    y_ref, A = rope64(x, cos, sin, pos)
    good = ops.rope_ref(x.bfloat16(), cos, sin, pos)
    flipped = ops.rope_ref(x.bfloat16(), cos, sin, pos, backward=True)
    assert not rejects(good, y_ref, tol_bf16(y_ref, A))
    assert rejects(flipped, y_ref, tol_bf16(y_ref, A))


def test_checker_rejects_neighbouring_rows_inv_rms():
    rows, H = 3, 264
    x, w, _ = rms_case(rows, H)
    y_ref, inv_ref = rmsnorm_fwd64(x, w, 1e-5)
    inv = inv_ref.float()
    assert not rejects(inv, inv_ref, tol_f32(inv_ref, K=H))
    inv[1] = inv[2]
    assert rejects(inv, inv_ref, tol_f32(inv_ref, K=H))
    y = (x.double() * inv.double()[:, None] * w.double()).bfloat16()
    assert rejects(y, y_ref, tol_bf16(y_ref, y_ref.abs(), K=H))
    # same with two ordinary rows whose rms differs by a few per cent
    x2 = bf16_values(torch.randn(4, H, generator=torch.Generator()
                                 .manual_seed(7)))
    y2_ref, inv2_ref = rmsnorm_fwd64(x2, w, 1e-5)
    inv2 = inv2_ref.float()
    inv2[1] = inv2[2]
    assert rejects(inv2, inv2_ref, tol_f32(inv2_ref, K=H))


def test_checker_rejects_unwritten_ce_tail_columns():
    logits, targets = ce_case("tail")
    N, V = logits.shape
    _, _, grad_ref, A_grad = cross_entropy64(logits, targets, 0.37)
    tol = tol_bf16(grad_ref, A_grad, K=V)
    grad = grad_ref.bfloat16()
    assert not rejects(grad, grad_ref, tol)
    # the kernel works in place: an unwritten column still holds its logit
    grad[:, V - V % 8:] = logits[:, V - V % 8:].bfloat16()
    assert rejects(grad, grad_ref, tol)
    # ... and zeros there are rejected as well
    grad[:, V - V % 8:] = 0
    assert rejects(grad, grad_ref, tol)


def test_checker_rejects_unwritten_last_row():
    rows, H = 2049, 264
    x, w, _ = rms_case(rows, H)
    y_ref, _ = rmsnorm_fwd64(x, w, 1e-5)
    tol = tol_bf16(y_ref, y_ref.abs(), K=H)
    y = y_ref.bfloat16()
    assert not rejects(y, y_ref, tol)
    y[-1] = 0
    ok, _, worst = within(y, y_ref, tol)
    assert not ok and worst // H == rows - 1


def emulate_rope_kernel_vec(x, cos, sin, pos):
    """The index arithmetic of rope_kernel_vec, lane by lane, as the
    launcher used it for every D % 32 == 0: 16 lanes per row, lane `sub`
    starts at pair sub * (D/2/16) and moves FOUR pairs per trip.  Buffers
    are padded so that an access past the end is recorded instead of
    raised.  Stores land in lane order.  Returns y, the flat indices
    where a later store changed an earlier one, and the highest index
    stored to."""
    T, H, D = x.shape
    half, rows, pad = D // 2, T * H, 8
    ppl = half // 16
    z = torch.zeros(pad, dtype=torch.float64)
    xf = torch.cat([x.double().reshape(-1), z])
    ct = torch.cat([cos.double().reshape(-1), z])
    st = torch.cat([sin.double().reshape(-1), z])
    y = torch.full((rows * D + pad,), float("nan"), dtype=torch.float64)
    clobbered, top = set(), -1
    for row in range(rows):
        tab = int(pos[row // H]) * half
        for sub in range(16):
            for p in range(0, ppl, 4):
                i = sub * ppl + p
                for k in range(4):
                    a, b = xf[row * D + i + k], xf[row * D + i + half + k]
                    c, s = ct[tab + i + k], st[tab + i + k]
                    for idx, val in ((row * D + i + k, a * c - b * s),
                                     (row * D + i + half + k, b * c + a * s)):
                        if not math.isnan(y[idx]) and y[idx] != val:
                            clobbered.add(idx)
                        y[idx] = val
                        top = max(top, idx)
    return y[:rows * D].reshape(T, H, D), clobbered, top


def test_checker_rejects_rope_vec_kernel_at_d64():
    """Why rope_launch keeps the vector kernel to D % 128 == 0.

    At D = 64 a lane owns 2 pairs but loads, rotates and stores 4.  Lanes
    0..14 merely repeat their neighbour's first two pairs with the right
    operands.  Lane 15 starts at pair 30 and runs on to 33: it treats
    x[32..33] (second half) as first-half elements, pairs them with the
    NEXT row's x[0..1] and the next table row's first two columns, stores
    the result to y[32..33] (racing with lane 0's correct store) and to
    y[64..65], which is the next row's y[0..1]; in the last row that is
    4 bytes past the end of x and y."""
    T, H = 7, 3
    # D = 128: the emulation is the kernel the trainer runs, and is right
    x, cos, sin, pos = rope_case(T, H, 128)
    y, clobbered, top = emulate_rope_kernel_vec(x, cos, sin, pos)
    y_ref, A = rope64(x, cos, sin, pos)
    assert not clobbered and top == T * H * 128 - 1
    assert not rejects(y, y_ref, tol_f32(A))

    D = 64
    x, cos, sin, pos = rope_case(T, H, D)
    y, clobbered, top = emulate_rope_kernel_vec(x, cos, sin, pos)
    y_ref, A = rope64(x, cos, sin, pos)
    rows = T * H
    assert top == rows * D + 1                  # two bf16 past the end
    expect = {r * D + c for r in range(rows) for c in (32, 33)} \
        | {r * D + c for r in range(1, rows) for c in (0, 1)}
    assert clobbered == expect
    ok, _, worst = within(y.bfloat16(), y_ref, tol_bf16(y_ref, A))
    assert not ok and worst % D in (32, 33)
    # everything lane 15 did not touch is right
    mask = torch.ones(D, dtype=torch.bool)
    mask[32:34] = False
    assert not rejects(y[..., mask].bfloat16(), y_ref[..., mask],
                       tol_bf16(y_ref, A)[..., mask])
