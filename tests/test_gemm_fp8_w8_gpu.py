"""ops.gemm_fp8_w8 (gemm_fp8_w8.hip) against fp64 element by element, its
exact k mapping, its batch invariance, its routing and the engine."""
import pytest
import torch
import torch.nn.functional as F

from skypilot_amd import ops
from _fp64_check import check, tol_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(n, I, O, seed=0):
    """Codes and scales of quantize_fp8_rowwise on random bf16; bf16 X = 0.5
    randn with rows 0, n // 2 and n - 1 scaled by 2^10."""
    g = torch.Generator().manual_seed(seed)
    w8, scale = ops.quantize_fp8_rowwise(
        (0.05 * torch.randn(O, I, generator=g)).bfloat16())
    x = 0.5 * torch.randn(n, I, generator=g)
    x[[0, n // 2, n - 1]] *= 1024.0
    return x.bfloat16(), w8, scale


def _run(x, w8, scale):
    return ops.gemm_fp8_w8(x.to(DEV), w8.to(DEV), scale.to(DEV)).cpu()


# n crosses the 128-token tile edge (257: three tiles); I = 640 is five k
# chunks, the last one restaged; O = 192 is three feature blocks.
@pytest.mark.parametrize("O", [64, 192])
@pytest.mark.parametrize("I", [128, 640])
@pytest.mark.parametrize("n", [1, 65, 127, 128, 129, 257])
def test_fp64_elementwise(n, I, O):
    x, w8, scale = _inputs(n, I, O, seed=n + I + O)
    w, s = w8.view(torch.float8_e4m3fn).float().double(), scale.double()
    ref = (x.double() @ w.t()) * s
    A = (x.double().abs() @ w.abs().t()) * s
    check(f"fp8 w8 n={n} I={I} O={O}", _run(x, w8, scale), ref,
          tol_bf16(ref, A, K=I, roundings=1))


def test_one_hot_rows_return_the_weights():
    """X = the 256 identity rows over I = 256: Y[k, :] is bf16(scale *
    e4m3(W8[:, k])) exactly, which pins the k bijection and the swizzle."""
    _, w8, scale = _inputs(1, 256, 192, seed=7)
    want = (w8.view(torch.float8_e4m3fn).float() * scale[:, None]).bfloat16().t()
    got = _run(torch.eye(256).bfloat16(), w8, scale)
    assert torch.equal(got.float(), want.float())


def test_batch_invariance_and_isolation():
    x, w8, scale = _inputs(200, 640, 192, seed=3)
    y200 = _run(x, w8, scale)
    for tr in (1, 2):       # three 64-row blocks: TR = 2 leaves one half empty
        dev = [t.to(DEV) for t in (x, w8, scale)]
        assert torch.equal(ops.gemm_fp8_w8(*dev, tr).cpu(), y200), tr
    # NaN rows 65.., in the batch or in memory behind a 65-row X, do not leak
    x[65:] = float("nan")
    ynan = _run(x, w8, scale)
    assert torch.equal(ynan[:65], y200[:65]) and ynan[65:].isnan().all()
    assert torch.equal(_run(x.to(DEV)[:65], w8, scale), y200[:65])


@pytest.mark.parametrize("msg,make", [
    ("N must be 1\\.\\.", lambda x, w, s: (x[:0], w, s)),
    ("I must be a positive multiple of 128",
     lambda x, w, s: (x[:, :64].contiguous(), w[:, :64].contiguous(), s)),
    ("O must be a multiple of 64", lambda x, w, s: (x, w[:32], s[:32])),
    ("X must start on a 16-byte",
     lambda x, w, s: (x.reshape(-1)[1:257].view(1, 256), w, s)),
    ("X must be BFloat16", lambda x, w, s: (x.float(), w, s)),
    ("W8 must be \\[O, I\\]", lambda x, w, s: (x, w[:, :128].contiguous(), s)),
    ("row_tiles must be 0, 1 or 2", lambda x, w, s: (x, w, s, 4)),
])
def test_binding_rejects_bad_arguments(msg, make):
    x, w8, scale = (t.to(DEV) for t in _inputs(4, 256, 64))
    with pytest.raises(RuntimeError, match="gemm_fp8_w8: " + msg):
        ops.gemm_fp8_w8(*make(x, w8, scale))


def test_linear_and_decode_linear_routing():
    g = torch.Generator().manual_seed(11)
    w, wq, wk, wodd = ((0.05 * torch.randn(o, 256, generator=g)).bfloat16().to(DEV)
                       for o in (384, 128, 64, 200))
    b = torch.randn(384, generator=g).bfloat16().to(DEV)
    x = torch.randn(2, 40, 256, generator=g).bfloat16().to(DEV)
    x80 = x.reshape(80, 256)
    try:
        with torch.no_grad():
            lin, dec = F.linear(x, w), ops.decode_linear(x80, w)
            for t in (w, wq, wk, wodd):
                ops.register_fp8_weight(t)
            assert torch.equal(ops.linear(x, w), lin)       # route off
            assert torch.equal(ops.decode_linear(x80, w), dec)
            ops.set_fp8_prefill(1)
            y = ops.gemm_fp8_w8(x80, *ops._FP8_WEIGHTS[w.data_ptr()])
            assert torch.equal(ops.linear(x, w), y.view(2, 40, 384))
            assert not torch.equal(y, dec)
            assert torch.equal(ops.linear(x, w, b), y.view(2, 40, 384) + b)
            assert torch.equal(ops.decode_linear(x80, w), y)
            for got, t in zip(ops.qkv_linear(x, w, wq, wk), (w, wq, wk)):
                assert torch.equal(got.reshape(80, -1), ops.gemm_fp8_w8(
                    x80, *ops._FP8_WEIGHTS[t.data_ptr()]))
            # O % 64 != 0; 64 rows in decode_linear; below the threshold
            ops.set_fp8_prefill(81)
            assert torch.equal(ops.linear(x, w), lin)
            ops.set_fp8_prefill(1)
            assert torch.equal(ops.linear(x, wodd), F.linear(x, wodd))
            assert torch.equal(ops.decode_linear(x80[:64], w),
                               F.linear(x80[:64], w))
        y = ops.linear(x.clone().requires_grad_(), w)       # grad enabled
        assert y.requires_grad and torch.equal(y, lin)
    finally:
        ops.set_fp8_prefill(None)
        ops.clear_fp8_weights()


def _snap_to_fp8(w):
    """In place: weights that quantize_fp8_rowwise represents exactly
    (power-of-two row scale, the row's largest element at +-448)."""
    wf = w.float()
    s = torch.exp2(torch.ceil(torch.log2(wf.abs().amax(1, keepdim=True) / 448)))
    q = (wf / s).to(torch.float8_e4m3fn).float()
    idx = wf.abs().argmax(1, keepdim=True)
    q.scatter_(1, idx, 448 * wf.gather(1, idx).sign())
    w.copy_((q * s).bfloat16())


@pytest.mark.parametrize("prefill_chunk", [None, 64])
def test_engine_prefills_from_fp8_weights(prefill_chunk):
    """The twin holds the dequantised fp8 weights in bf16 (exact after
    _snap_to_fp8) and takes F.linear: the engines differ by the order of the
    fp32 sums only, so a GEMM output may land on the neighbouring bf16 value,
    2^-7 relative.  Nine GEMM outputs lead to a logit (four per block,
    lm_head); taken as independent, two logits move apart by sqrt(2 * 9) *
    2^-7 = 3.3 % of the largest |logit|.  At seed 0 the CPU reference's
    smallest top-2 margin is 6.2 % of it (asserted below)."""
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model("llama-debug", device="cpu", seed=0)
    prompts = [[2 + (7 * i + 3 * j) % 500 for j in range(n)]
               for i, n in enumerate((70, 130))]
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in name:
                _snap_to_fp8(p.data)
        for ids in prompts:
            ids = list(ids)
            for _ in range(4):
                lg = model(torch.tensor([ids]))[0, -1].float()
                top = lg.topk(2).values
                assert top[0] - top[1] > 18 ** 0.5 * 2.0 ** -7 * lg.abs().max()
                ids.append(int(lg.argmax()))
    model = model.to(DEV)
    outs = []
    try:
        for fp8 in (False, True):
            eng = Engine("llama-debug", device=DEV, max_seq=256, max_batch=4,
                         model=model, prefill_chunk=prefill_chunk)
            if fp8:
                assert eng.enable_fp8_prefill(min_tokens=1,
                                              min_bytes=1 << 16) == 15
                w = model.blocks[0].mlp.w_down.weight
                q8, s = ops._FP8_WEIGHTS[w.data_ptr()]
                assert torch.equal(
                    q8.view(torch.float8_e4m3fn).float() * s[:, None], w.float())
            reqs = [eng.submit(Request(prompt_ids=p, max_tokens=4))
                    for p in prompts]
            eng.start()
            try:
                for r in reqs:
                    assert r.done.wait(120), "request did not complete"
            finally:
                eng.stop()
            outs.append([r.out_ids for r in reqs])
    finally:
        ops.set_fp8_prefill(None)
        ops.clear_fp8_weights()
    assert all(len(o) == 4 for o in outs[0]) and outs[0] == outs[1]
