"""ops.gemm_mxfp4_a8 and ops.quantize_mxfp8_rows (gemm_mxfp4_a8.hip): the
quantiser bit for bit against ops.quantize_mxfp8, the block-scaled MFMA GEMM
against fp64 element by element, its exact k / nibble / scale mapping, its
batch invariance, the routing of ops.linear / ops.qkv_linear and the engine."""
import pytest
import torch
import torch.nn.functional as F

from skypilot_amd import ops
from _fp64_check import check, tol_bf16
from test_mxfp8_reference import EDGE_EXPS, edge_blocks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(n, I, O, seed=0):
    """W as test_skinny_gemm_fp4_mfma_gpu._inputs; X = randn times a power of
    two drawn per block from 2^-6 .. 2^6 (a constant scale would hide a wrong
    block index)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(-6, 7, (n, I // 32, 1), generator=g).float()
    x = (torch.randn(n, I // 32, 32, generator=g) * 2.0 ** p).reshape(n, I)
    codes = torch.randint(0, 256, (O, I // 2), generator=g).to(torch.uint8)
    exps = torch.randint(112, 133, (O, I // 32), generator=g).to(torch.uint8)
    return x.bfloat16(), codes, exps


def _run(x, codes, exps):
    return ops.gemm_mxfp4_a8(x.to(DEV), codes.to(DEV), exps.to(DEV)).cpu()


@pytest.mark.parametrize("n,I", [(1, 128), (65, 128), (129, 128), (1, 640),
                                 (65, 640), (129, 640), (7, 32)])
def test_quantiser_is_bit_exact(n, I):
    x = edge_blocks() if I == 32 else _inputs(n, I, 128, seed=n + I)[0]
    codes, exps = (t.cpu() for t in ops.quantize_mxfp8_rows(x.to(DEV)))
    n_pad = -(-n // 128) * 128
    assert codes.shape == (n_pad, I) and exps.shape == (n_pad, I // 32)
    want_c, want_e = ops.quantize_mxfp8(x)
    if I == 32:
        assert want_e.reshape(-1).tolist() == EDGE_EXPS
    assert torch.equal(exps[:n], want_e) and torch.equal(codes[:n], want_c)
    assert not codes[n:].any() and (exps[n:] == 127).all()


# Tiles are 128 tokens x 128 features x 128 k: one row, both sides of one and
# of two token tiles; 1, 2 and 5 chunks (prologue only, both buffers, odd
# count); one and three feature tiles.
@pytest.mark.parametrize("n,I,O", [
    (1, 128, 128), (127, 256, 128), (128, 640, 128), (129, 128, 384),
    (257, 256, 384), (1, 640, 384), (127, 640, 384), (128, 128, 384),
    (129, 640, 128), (257, 640, 384),
])
def test_fp64_elementwise(n, I, O):
    x, codes, exps = _inputs(n, I, O, seed=n + I + O)
    xd = ops.dequantize_mxfp8(*ops.quantize_mxfp8(x)).double()
    w = ops.dequantize_mxfp4(codes, exps).double()
    ref = xd @ w.t()
    A = xd.abs() @ w.abs().t()
    check(f"mxfp4 x mxfp8 n={n} I={I} O={O}", _run(x, codes, exps), ref,
          tol_bf16(ref, A, K=I, roundings=1))


def test_one_hot_rows_return_the_weights():
    """X[t, k_t] = 2^((k_t // 32) % 7 - 3) with k_t running over every k of 5
    chunks: Y[t, :] is bf16(w[:, k_t] * X[t, k_t]) exactly (+0 for -0), which
    pins the nibble order, the k bijection of both operands and both
    scale-to-block mappings at once."""
    I, O = 640, 384
    _, codes, exps = _inputs(1, I, O, seed=7)
    s = 2.0 ** ((torch.arange(I) // 32) % 7 - 3)
    want = (ops.dequantize_mxfp4(codes, exps) * s).bfloat16().t() + 0.0
    got = _run(torch.diag(s).bfloat16(), codes, exps)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_batch_invariance_and_isolation():
    x, codes, exps = _inputs(257, 640, 384, seed=3)
    y = _run(x, codes, exps)
    for t in (0, 127, 128, 256):
        assert torch.equal(_run(x[t:t + 1], codes, exps)[0], y[t]), t
    assert torch.equal(_run(x[:129], codes, exps), y[:129])
    x[5] = float("nan")
    keep = torch.arange(257) != 5
    assert torch.equal(_run(x, codes, exps)[keep], y[keep])


def test_linear_routing():
    g = torch.Generator().manual_seed(11)
    ws = [(0.05 * torch.randn(o, 256, generator=g)).bfloat16().to(DEV)
          for o in (384, 128, 128, 200)]
    bs = [torch.randn(w.shape[0], generator=g).bfloat16().to(DEV) for w in ws]
    x200, x64 = ((torch.randn(2, n // 2, 256, generator=g)).bfloat16().to(DEV)
                 for n in (200, 64))
    try:
        with torch.no_grad():
            ops.set_fp4_prefill(128)   # on, nothing registered
            assert torch.equal(ops.linear(x200, ws[0]), F.linear(x200, ws[0]))
            for w in ws:
                ops.register_fp4_weight(w)
            ops.set_fp4_prefill(None)  # registered, off
            assert torch.equal(ops.linear(x200, ws[0]), F.linear(x200, ws[0]))
            q, k, v = ops.qkv_linear(x200, *ws[:3], *bs[:3])
            assert torch.equal(k, F.linear(x200, ws[1], bs[1]))
            ops.set_fp4_prefill(128)
            fp4 = [ops.gemm_mxfp4_a8(x200.reshape(200, 256),
                                     *ops._FP4_WEIGHTS[w.data_ptr()])
                   .view(2, 100, -1) for w in ws[:3]]
            assert torch.equal(ops.linear(x200, ws[0]), fp4[0])
            assert not torch.equal(fp4[0], F.linear(x200, ws[0]))
            assert torch.equal(ops.linear(x200, ws[0], bs[0]), fp4[0] + bs[0])
            for got, y, b in zip(ops.qkv_linear(x200, *ws[:3], *bs[:3]), fp4,
                                 bs):
                assert torch.equal(got, y + b)
            # below the threshold, O % 128 != 0: the parent's bits
            assert torch.equal(ops.linear(x64, ws[0]), F.linear(x64, ws[0]))
            assert torch.equal(ops.linear(x200, ws[3]), F.linear(x200, ws[3]))
        xg = x200.clone().requires_grad_()
        y = ops.linear(xg, ws[0])       # grad enabled
        assert y.requires_grad and torch.equal(y, F.linear(x200, ws[0]))
    finally:
        ops.set_fp4_prefill(None)
        ops.clear_fp4_weights()


@pytest.mark.parametrize("msg,make", [
    ("I must be a positive multiple of 128",
     lambda x, c, e: (x[:, :64].contiguous(), c[:, :32].contiguous(),
                      e[:, :2].contiguous())),
    ("O must be a positive multiple of 128", lambda x, c, e: (x, c[:64], e[:64])),
    ("X must start on a 16-byte",
     lambda x, c, e: (x.reshape(-1)[1:257].view(1, 256), c, e)),
    ("X must be BFloat16", lambda x, c, e: (x.float(), c, e)),
    ("X must be contiguous", lambda x, c, e: (x.t().contiguous().t(), c, e)),
    ("X must be \\[N, I\\]", lambda x, c, e: (x[None], c, e)),
    ("codes must be on GPU", lambda x, c, e: (x, c.cpu(), e)),
    ("codes must be Byte", lambda x, c, e: (x, c.view(torch.int8), e)),
    ("codes must be \\[O, I/2\\]",
     lambda x, c, e: (x, c[:, :64].contiguous(), e)),
    ("exps must be \\[O, I/32\\]", lambda x, c, e: (x, c, e[:64])),
])
def test_binding_rejects_bad_arguments(msg, make):
    x, codes, exps = (t.to(DEV) for t in _inputs(4, 256, 128))
    with pytest.raises(RuntimeError, match="gemm_mxfp4_a8: " + msg):
        ops.gemm_mxfp4_a8(*make(x, codes, exps))


@pytest.mark.parametrize("prefill_chunk", [None, 64])
def test_engine_prefills_from_fp4_weights(prefill_chunk):
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model("llama-smoke", device=DEV)
    outs = []
    try:
        for _ in range(2):
            eng = Engine("llama-smoke", device=DEV, max_seq=256, max_batch=8,
                         model=model, prefill_chunk=prefill_chunk)
            assert eng.enable_fp4_prefill(min_tokens=64) > 0
            with pytest.raises(ValueError, match="already serves fp4"):
                eng.enable_fp8_decode()
            reqs = [eng.submit(Request(
                prompt_ids=[2 + (7 * i + j) % 4000 for j in range(n)],
                max_tokens=4)) for i, n in enumerate((70, 113, 128, 200))]
            eng.start()
            try:
                for r in reqs:
                    assert r.done.wait(120), "request did not complete"
            finally:
                eng.stop()
            outs.append([r.out_ids for r in reqs])
    finally:
        ops.set_fp4_prefill(None)
        ops.clear_fp4_weights()
        ops.clear_fp8_weights()
    assert all(len(o) == 4 for o in outs[0]) and outs[0] == outs[1]
