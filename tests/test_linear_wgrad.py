"""Weight gradients through linear_wgrad (docs/KERNELS.md "Weight
gradients"): the bf16 transpose kernel bit for bit, linear_wgrad and the
backward of ops.linear / ops.qkv_linear element by element against fp64
on the bf16-rounded inputs (the rule of _fp64_check.py, no element
excluded), and the model's loss and gradients with each route forced.

Bounds.  dW and db reduce K = M tokens in fp32 and round once to bf16:
tol_bf16(ref, A, K=M, roundings=1).  dx of ops.linear reduces K = out
terms and rounds once.  dx of ops.qkv_linear sums the q, k and v terms:
tol_bf16(ref, A, K=sum of the three outs, roundings=3), one rounding per
accumulated term, all charged to |ref|.  Only a dx whose partial sums are
never rounded to bf16 can meet that where the three terms cancel (a dx
accumulated by two beta = 1 GEMMs into a bf16 tensor was measured at 2.65
times this bound), which is why ops.qkv_linear forms dx as one GEMM over
the packed dq|dk|dv.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from _fp64_check import TINY, U16, U32, check, f32, tol_bf16
from skypilot_amd import ops
from skypilot_amd.models.llama import build_model

gpu = pytest.mark.gpu
ROUTES = [0, 1, 2]


def dev():
    return torch.device("cuda:0")


def rand_bf16(*shape, seed, scale=1.0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16().to(device)


def bits(t):
    return t.contiguous().view(torch.int16)


# ===========================================================================
# transpose_bf16 / transpose_bf16_out
# ===========================================================================
def any_bits(R, C, seed):
    """Every bf16 bit pattern is fair game for a copy, NaNs included."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2 ** 15, 2 ** 15, (R, C), generator=g,
                      dtype=torch.int16)
    return v.to(dev()).view(torch.bfloat16)


# (4160, 4096) is 4,160 tiles, more than the launch's 4,096 blocks: the
# grid-stride loop takes a second trip
@gpu
@pytest.mark.parametrize("R,C", [(64, 64), (64, 192), (320, 128),
                                 (4160, 4096)])
def test_transpose_bit_exact(R, C):
    x = any_bits(R, C, seed=R + C)
    y = ops.native().transpose_bf16(x)
    assert y.shape == (C, R) and y.is_contiguous()
    assert torch.equal(bits(y), bits(x.t().contiguous()))


@gpu
def test_transpose_out_writes_only_its_rows():
    R, C, pad = 320, 128, 64
    x = any_bits(R, C, seed=7)
    buf = torch.full((pad + C + pad, R), 0x5A5A, dtype=torch.int16,
                     device=dev()).view(torch.bfloat16)
    ops.native().transpose_bf16_out(x, buf[pad:pad + C])
    b = bits(buf)
    assert torch.equal(b[pad:pad + C], bits(x.t().contiguous()))
    assert bool((b[:pad] == 0x5A5A).all())
    assert bool((b[pad + C:] == 0x5A5A).all())


@gpu
def test_transpose_rejects_bad_arguments():
    C = ops.native()
    x = any_bits(128, 64, seed=1)
    with pytest.raises(RuntimeError, match="transpose_bf16: X must be"):
        C.transpose_bf16(x.float())
    with pytest.raises(RuntimeError,
                       match="transpose_bf16: X must be contiguous"):
        C.transpose_bf16(any_bits(64, 128, seed=2).t())
    with pytest.raises(RuntimeError, match="transpose_bf16: X dims"):
        C.transpose_bf16(any_bits(96, 64, seed=3))
    with pytest.raises(RuntimeError, match="transpose_bf16: X dims"):
        C.transpose_bf16(any_bits(64, 96, seed=3))
    ok = torch.empty(64, 128, dtype=torch.bfloat16, device=dev())
    with pytest.raises(RuntimeError, match="transpose_bf16_out: X dims"):
        C.transpose_bf16_out(any_bits(96, 64, seed=3),
                             torch.empty(64, 96, dtype=torch.bfloat16,
                                         device=dev()))
    with pytest.raises(RuntimeError, match="transpose_bf16_out: Y must be"):
        C.transpose_bf16_out(x, ok.float())
    with pytest.raises(RuntimeError, match="transpose_bf16_out: Y must be"):
        C.transpose_bf16_out(x, ok.cpu())
    with pytest.raises(RuntimeError,
                       match="transpose_bf16_out: Y must be contiguous"):
        C.transpose_bf16_out(
            x, torch.empty(64, 256, dtype=torch.bfloat16,
                           device=dev())[:, :128])
    with pytest.raises(RuntimeError,
                       match=r"transpose_bf16_out: Y must be \[64, 128\]"):
        C.transpose_bf16_out(x, torch.empty(128, 64, dtype=torch.bfloat16,
                                            device=dev()))
    odd = any_bits(1, 128 * 64 + 1, seed=4).view(-1)[1:].view(128, 64)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 2
    with pytest.raises(RuntimeError, match="transpose_bf16: X must start on "
                       "a 16-byte boundary"):
        C.transpose_bf16(odd)
    with pytest.raises(RuntimeError, match="transpose_bf16_out: Y must start "
                       "on a 16-byte boundary"):
        C.transpose_bf16_out(
            x, torch.empty(64 * 128 + 1, dtype=torch.bfloat16,
                           device=dev())[1:].view(64, 128))
    # a misaligned operand of linear_wgrad is the library's, on any route
    good = rand_bf16(128 * 64 + 1, seed=5, device=dev())[1:].view(128, 64)
    xg = rand_bf16(128, 64, seed=6, device=dev())
    assert torch.equal(C.linear_wgrad(good, xg, 1),
                       C.linear_wgrad(good, xg, 0))
    # nothing above was launched: a good call still works
    C.transpose_bf16_out(x, ok)
    assert torch.equal(bits(ok), bits(x.t().contiguous()))


# ===========================================================================
# linear_wgrad
# ===========================================================================
@functools.lru_cache(maxsize=None)
def wgrad_case(M, outs, I):
    """dy parts [M, out_i], x [M, I] (bf16, CPU) and per part the fp64
    dW = dy^T x with its absolute-value evaluation."""
    x = rand_bf16(M, I, seed=3 * M + I)
    dys = tuple(rand_bf16(M, o, seed=5 * M + o + 17 * n, scale=0.25)
                for n, o in enumerate(outs))
    refs = tuple((dy.double().t() @ x.double(),
                  dy.double().abs().t() @ x.double().abs()) for dy in dys)
    return dys, x, refs


@gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("M,O,I", [(64, 64, 64), (192, 128, 320),
                                   (8192, 256, 256)])
def test_linear_wgrad_fp64(M, O, I, route):
    (dy,), x, ((ref, A),) = wgrad_case(M, (O,), I)
    dW = ops.native().linear_wgrad(dy.to(dev()), x.to(dev()), route)
    assert dW.shape == (O, I) and dW.dtype == torch.bfloat16
    assert dW.is_contiguous()
    check(f"linear_wgrad route {route} M={M}", dW, ref,
          tol_bf16(ref, A, K=M, roundings=1))


@gpu
@pytest.mark.parametrize("route", ROUTES)
def test_linear_wgrad_packed_fp64(route):
    M, outs, I = 192, (256, 128, 128), 320
    dys, x, refs = wgrad_case(M, outs, I)
    dWs = ops.native().linear_wgrad_packed([d.to(dev()) for d in dys],
                                           x.to(dev()), route)
    assert len(dWs) == 3
    for n, (dW, (ref, A)) in enumerate(zip(dWs, refs)):
        assert dW.shape == (outs[n], I) and dW.is_contiguous()
        check(f"linear_wgrad_packed route {route} part {n}", dW, ref,
              tol_bf16(ref, A, K=M, roundings=1))
    if route:   # row views of one [sum out, I] result
        base = dWs[0].data_ptr()
        assert dWs[1].data_ptr() == base + 2 * outs[0] * I
        assert dWs[2].data_ptr() == base + 2 * (outs[0] + outs[1]) * I


@gpu
@pytest.mark.parametrize("route", [-1] + ROUTES)
def test_linear_wgrad_fallback_is_autograd(route):
    """in = 96 is no multiple of the 64-wide tile: every route makes the
    library call autograd makes."""
    M, O, I = 64, 64, 96
    x = rand_bf16(M, I, seed=1, device=dev())
    dy = rand_bf16(M, O, seed=2, device=dev())
    w = torch.zeros(O, I, dtype=torch.bfloat16, device=dev(),
                    requires_grad=True)
    F.linear(x, w).backward(dy)
    assert torch.equal(ops.native().linear_wgrad(dy, x, route), w.grad)


@gpu
def test_linear_wgrad_table_leaves_unlisted_shapes_to_the_library():
    (dy,), x, _ = wgrad_case(192, (128,), 320)
    C = ops.native()
    dy, x = dy.to(dev()), x.to(dev())
    assert torch.equal(C.linear_wgrad(dy, x), C.linear_wgrad(dy, x, 0))


@gpu
def test_linear_wgrad_table_routes_a_listed_shape():
    """4096 x 14336 (down) is listed with route 2 from 8,192 tokens up,
    keyed on the sum of the outs; below that it is the library's call.
    The library gives the same bits on routes 0 and 2 at this shape, so
    the route taken is read off the scratch it allocates: route 2 holds
    the transposed dy [out, M] beside the result, route 0 nothing."""
    C = ops.native()
    M, O, I = 8192, 4096, 14336
    dy = rand_bf16(M, O, seed=41, scale=0.25, device=dev())
    x = rand_bf16(M, I, seed=42, device=dev())
    halves = [h.contiguous() for h in dy.split(O // 2, dim=1)]

    def scratch(fn):
        fn()    # warm: the library's workspace is allocated once
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        peak = torch.cuda.max_memory_allocated() - before - 2 * O * I
        return peak, (out if isinstance(out, torch.Tensor)
                      else torch.cat(list(out)))

    dyT = 2 * O * M
    lib, _ = scratch(lambda: C.linear_wgrad(dy, x, 0))
    dy_only, dW2 = scratch(lambda: C.linear_wgrad(dy, x, 2))
    assert lib < dyT <= dy_only
    table, dW = scratch(lambda: C.linear_wgrad(dy, x))
    assert table == dy_only and torch.equal(dW, dW2)
    table, dW = scratch(lambda: C.linear_wgrad_packed(halves, x))
    assert dyT <= table and torch.equal(dW, dW2)
    M = 4096    # below the table's 8,192 tokens
    dyT = 2 * O * M
    table, dW = scratch(lambda: C.linear_wgrad(dy[:M], x[:M]))
    assert table < dyT
    assert torch.equal(dW, C.linear_wgrad(dy[:M], x[:M], 0))


@gpu
def test_linear_wgrad_rejects_bad_arguments():
    C = ops.native()
    x = rand_bf16(64, 64, seed=1, device=dev())
    dy = rand_bf16(64, 128, seed=2, device=dev())
    with pytest.raises(RuntimeError, match="linear_wgrad: route"):
        C.linear_wgrad(dy, x, 3)
    with pytest.raises(RuntimeError, match="linear_wgrad: dy must be bf16"
                       "|linear_wgrad: dy must be BFloat16"):
        C.linear_wgrad(dy.float(), x, 1)
    with pytest.raises(RuntimeError, match="linear_wgrad: x must be contig"):
        C.linear_wgrad(dy, rand_bf16(64, 64, seed=1, device=dev()).t(), 1)
    with pytest.raises(RuntimeError, match=r"linear_wgrad: dy must be \[M"):
        C.linear_wgrad(rand_bf16(128, 64, seed=2, device=dev()), x, 1)


# ===========================================================================
# ops.linear / ops.qkv_linear backward.  The projection shapes of
# llama-debug and qwen2-debug (hidden 256, q 256, k = v 128, MLP 512),
# M = 128 tokens as [2, 64, in]; qwen2-debug has the q/k/v biases.
# ===========================================================================
B, S = 2, 64


@functools.lru_cache(maxsize=None)
def linear_case(O, I, bias):
    M = B * S
    x = rand_bf16(M, I, seed=O + I)
    w = rand_bf16(O, I, seed=O + 2 * I, scale=0.05)
    b = rand_bf16(O, seed=O + 3 * I) if bias else None
    dy = rand_bf16(M, O, seed=2 * O + I, scale=0.25)
    d, xd, wd = dy.double(), x.double(), w.double()
    return dict(x=x, w=w, b=b, dy=dy,
                dW=(d.t() @ xd, d.abs().t() @ xd.abs()),
                db=(d.sum(0), d.abs().sum(0)),
                dx=(d @ wd, d.abs() @ wd.abs()))


def leaf(t):
    return None if t is None else t.to(dev()).requires_grad_()


@gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("O,I", [(256, 256), (1024, 256), (256, 512)])
def test_ops_linear_backward_fp64(O, I, bias, route):
    c = linear_case(O, I, bias)
    M = B * S
    x, w, b = leaf(c["x"].view(B, S, I)), leaf(c["w"]), leaf(c["b"])
    y = ops.linear(x, w, b, route=route)
    assert torch.equal(y, F.linear(x, w, b))
    y.backward(c["dy"].to(dev()).view(B, S, O))
    tag = f"ops.linear {O}x{I} route {route}"
    check(tag + " dW", w.grad, c["dW"][0],
          tol_bf16(*c["dW"], K=M, roundings=1))
    check(tag + " dx", x.grad.view(M, I), c["dx"][0],
          tol_bf16(*c["dx"], K=O, roundings=1))
    if bias:
        check(tag + " db", b.grad, c["db"][0],
              tol_bf16(*c["db"], K=M, roundings=1))


@gpu
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("O,I", [(256, 256), (1024, 256), (256, 512)])
def test_ops_linear_route0_is_autograd(O, I, bias):
    c = linear_case(O, I, bias)
    dy = c["dy"].to(dev()).view(B, S, O)
    x, w, b = leaf(c["x"].view(B, S, I)), leaf(c["w"]), leaf(c["b"])
    ops.linear(x, w, b, route=0).backward(dy)
    x2, w2, b2 = leaf(c["x"].view(B, S, I)), leaf(c["w"]), leaf(c["b"])
    F.linear(x2, w2, b2).backward(dy)
    assert torch.equal(x.grad, x2.grad)
    assert torch.equal(w.grad, w2.grad)
    if bias:
        assert torch.equal(b.grad, b2.grad)


QKV_OUTS = (256, 128, 128)


@functools.lru_cache(maxsize=None)
def qkv_case(bias):
    I = 256
    M = B * S
    x = rand_bf16(M, I, seed=11)
    ws = [rand_bf16(o, I, seed=12 + n, scale=0.05)
          for n, o in enumerate(QKV_OUTS)]
    bs = [rand_bf16(o, seed=22 + n) if bias else None
          for n, o in enumerate(QKV_OUTS)]
    dys = [rand_bf16(M, o, seed=32 + n, scale=0.25)
           for n, o in enumerate(QKV_OUTS)]
    xd = x.double()
    terms = [d.double() @ w.double() for d, w in zip(dys, ws)]
    A = sum(d.double().abs() @ w.double().abs() for d, w in zip(dys, ws))
    ref = sum(terms)
    return dict(x=x, ws=ws, bs=bs, dys=dys,
                dx=(ref, tol_bf16(ref, A, K=sum(QKV_OUTS), roundings=3)),
                dW=[(d.double().t() @ xd, d.double().abs().t() @ xd.abs())
                    for d in dys],
                db=[(d.double().sum(0), d.double().abs().sum(0))
                    for d in dys])


@gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("bias", [False, True])
def test_ops_qkv_linear_backward_fp64(bias, route):
    c = qkv_case(bias)
    M, I = B * S, 256
    x = leaf(c["x"].view(B, S, I))
    ws = [leaf(w) for w in c["ws"]]
    bs = [leaf(b) for b in c["bs"]]
    outs = ops.qkv_linear(x, *ws, *bs, route=route)
    for y, w, b in zip(outs, ws, bs):
        assert torch.equal(y, F.linear(x, w, b))
    torch.autograd.backward(
        outs, [d.to(dev()).view(B, S, -1) for d in c["dys"]])
    tag = f"ops.qkv_linear route {route}"
    check(tag + " dx", x.grad.view(M, I), *c["dx"])
    for n in range(3):
        check(f"{tag} dW{n}", ws[n].grad, c["dW"][n][0],
              tol_bf16(*c["dW"][n], K=M, roundings=1))
        if bias:
            check(f"{tag} db{n}", bs[n].grad, c["db"][n][0],
                  tol_bf16(*c["db"][n], K=M, roundings=1))


# ===========================================================================
# The model
# ===========================================================================
def model_batch(vocab, device):
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(0, vocab, (2, 129), generator=g).to(device)
    return tok[:, :-1].contiguous(), tok[:, 1:].contiguous()


def run_model_forced(monkeypatch, route):
    """llama-debug loss and gradients with every ops.linear /
    ops.qkv_linear of the model at `route`.  Also returns, per parameter,
    what reached its layer in this run: (kind, input, dy)."""
    model = build_model("llama-debug", device="cuda:0", seed=3)
    name_of = {id(p): n for n, p in model.named_parameters()}
    seen = {}
    real_linear, real_qkv, real_norm = ops.linear, ops.qkv_linear, ops.rmsnorm

    def watch(kind, x, w, y):
        y.register_hook(
            lambda g: seen.__setitem__(name_of[id(w)],
                                       (kind, x.detach(), g.detach())))

    def linear(x, w, b=None):
        y = real_linear(x, w, b, route=route)
        watch("linear", x, w, y)
        return y

    def qkv_linear(x, wq, wk, wv, bq=None, bk=None, bv=None):
        ys = real_qkv(x, wq, wk, wv, bq, bk, bv, route=route)
        for w, y in zip((wq, wk, wv), ys):
            watch("linear", x, w, y)
        return ys

    def rmsnorm(x, w, eps=1e-5):
        y = real_norm(x, w, eps)
        watch(("norm", eps), x, w, y)
        return y

    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "qkv_linear", qkv_linear)
    monkeypatch.setattr(ops, "rmsnorm", rmsnorm)
    model.lm_head.register_forward_hook(
        lambda m, i, y: watch("linear", i[0], m.weight, y))
    model.embed.register_forward_hook(
        lambda m, i, y: watch("embed", i[0], m.weight, y))
    loss = model.loss(*model_batch(model.cfg.vocab_size, dev()))
    loss.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    return loss.detach(), grads, seen


def param_grad64(kind, x, dy, shape):
    """fp64 gradient of one parameter from its layer's input and dy, and
    the bound of a kernel that sums the M rows in fp32 and rounds once."""
    d = dy.reshape(-1, dy.shape[-1]).double()
    M = d.shape[0]
    if kind == "embed":
        # rows of dy added at their token's row.  torch's embedding
        # backward (not a kernel of this package) adds them in bf16: a
        # row that n tokens hit is rounded n times, each time as a partial
        # sum no larger than A.
        idx = x.reshape(-1)
        ref = torch.zeros(shape, dtype=torch.float64,
                          device=d.device).index_add_(0, idx, d)
        A = torch.zeros_like(ref).index_add_(0, idx, d.abs())
        n = torch.bincount(idx, minlength=shape[0]).double()[:, None]
        return ref.cpu(), (2 * U16 * n * A + 4 * M * U32 * A + TINY).cpu()
    else:
        x2 = x.reshape(-1, x.shape[-1]).double()
        if kind == "linear":
            ref, A = d.t() @ x2, d.abs().t() @ x2.abs()
        else:               # rmsnorm weight: sum over rows of dy x inv_rms
            inv = torch.rsqrt(x2.pow(2).mean(-1, keepdim=True) + f32(kind[1]))
            s = d * x2 * inv
            ref, A = s.sum(0), s.abs().sum(0)
    return ref.cpu(), tol_bf16(ref, A, K=M, roundings=1).cpu()


@gpu
def test_model_routes_match_route0_and_fp64(monkeypatch):
    """Loss bit-equal to route 0 (the forward is unchanged), and every
    parameter gradient, on every route, inside the fp64 bound of the
    gradient formed from the input and dy of its own layer."""
    loss0 = None
    for route in ROUTES:
        with monkeypatch.context() as mp:
            loss, grads, seen = run_model_forced(mp, route)
        if route == 0:
            loss0 = loss
        assert torch.equal(loss, loss0)
        assert seen.keys() == grads.keys() and len(grads) == 19
        for n, g in grads.items():
            kind, x, dy = seen[n]
            check(f"route {route} {n}", g,
                  *param_grad64(kind, x, dy, g.shape))


@pytest.mark.parametrize("name", ["llama-debug", "qwen2-debug"])
def test_cpu_model_is_the_f_linear_composition(monkeypatch, name):
    """Without a GPU ops.linear and ops.qkv_linear are F.linear itself:
    loss and gradients are bit-equal to the model written with F.linear,
    as it was before these ops existed."""
    def run():
        model = build_model(name, seed=3)
        loss = model.loss(*model_batch(model.cfg.vocab_size, "cpu"))
        loss.backward()
        return loss.detach(), {n: p.grad
                               for n, p in model.named_parameters()}

    loss, grads = run()
    monkeypatch.setattr(ops, "linear", F.linear)
    monkeypatch.setattr(
        ops, "qkv_linear",
        lambda x, wq, wk, wv, bq=None, bk=None, bv=None:
        (F.linear(x, wq, bq), F.linear(x, wk, bk), F.linear(x, wv, bv)))
    loss_ref, grads_ref = run()
    assert torch.equal(loss, loss_ref)
    assert grads.keys() == grads_ref.keys()
    for n in grads:
        assert torch.equal(grads[n], grads_ref[n]), n


def test_cpu_ops_are_plain_f_linear():
    x = torch.randn(4, 8, requires_grad=True)
    w = torch.randn(6, 8, requires_grad=True)
    b = torch.randn(6)
    y = ops.linear(x, w, b)
    assert torch.equal(y, F.linear(x, w, b))
    plain = type(F.linear(x, w, b).grad_fn).__name__
    assert type(y.grad_fn).__name__ == plain
    q, k, v = ops.qkv_linear(x, w, w[:2], w[2:4], b, None, None)
    assert [type(t.grad_fn).__name__ for t in (q, k, v)] == [
        plain, type(F.linear(x, w[:2]).grad_fn).__name__,
        type(F.linear(x, w[2:4]).grad_fn).__name__]
    assert torch.equal(q, y)
    assert torch.equal(k, F.linear(x, w[:2]))
    assert torch.equal(v, F.linear(x, w[2:4]))
