"""ops.skinny_gemm_fp8_mfma (skinny_gemm_fp8_mfma.hip): the fp8-weight decode
GEMM on the matrix cores, against fp64 element by element, its exact k
mapping, its batch invariance, its routing and the engine."""
import pytest
import torch

from skypilot_amd import ops
from _fp64_check import check, tol_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(n, I, O, seed=0):
    """bf16 X = 0.5 randn, W8 uniform over the 254 finite e4m3 codes
    (subnormals and +-0 included), scales that are no powers of two."""
    g = torch.Generator().manual_seed(seed)
    x = (0.5 * torch.randn(n, I, generator=g)).bfloat16()
    r = torch.randint(0, 254, (O, I), generator=g)
    w8 = (r + (r >= 127)).to(torch.uint8)      # skips 0x7F and 0xFF
    scale = (torch.rand(O, generator=g) * 0.02 + 0.003).float()
    return x, w8, scale


def _w64(w8):
    return w8.view(torch.float8_e4m3fn).float().double()


def _run(x, w8, scale):
    return ops.skinny_gemm_fp8_mfma(x.to(DEV), w8.to(DEV), scale.to(DEV)).cpu()


# One k chunk (three waves idle); 5 and 33 chunks (neither the 4-wave split
# nor the 2-unit chunk divides them); O = 80, 272: tile counts 5 and 17;
# O = 6160 / 16400: two / four row tiles per wave with a tile count they do
# not divide (last block partly empty).  n covers every NT, full and ragged
# column tiles; n = 16 at O = 6160 is the one-tile side of that threshold.
@pytest.mark.parametrize("n,I,O", [
    (1, 128, 16), (3, 128, 16), (64, 128, 16),
    (16, 640, 80), (17, 640, 80), (48, 640, 80),
    (1, 4224, 272), (3, 4224, 272), (17, 4224, 272), (64, 4224, 272),
    (33, 640, 16400), (64, 128, 16400), (16, 128, 6160), (48, 640, 6160),
])
def test_fp64_elementwise(n, I, O):
    x, w8, scale = _inputs(n, I, O, seed=n + I + O)
    w, s = _w64(w8), scale.double()
    ref = (x.double() @ w.t()) * s
    A = (x.double().abs() @ w.abs().t()) * s
    check(f"fp8 mfma n={n} I={I} O={O}", _run(x, w8, scale), ref,
          tol_bf16(ref, A, K=I, roundings=1))


@pytest.mark.parametrize("O", [80, 16400])
def test_one_hot_rows_return_the_weights(O):
    """X[t, k_t] = 1 with k_t running over every k of 5 chunks, 64 at a time:
    Y[t, :] is bf16(scale * e4m3(W8[:, k_t])) exactly (+0 for -0 codes: the
    accumulator starts at +0), which pins the k bijection and the conversion."""
    I = 640
    _, w8, scale = _inputs(1, I, O, seed=7)
    want = (w8.view(torch.float8_e4m3fn).float() * scale[:, None]).bfloat16().t()
    eye = torch.eye(I).bfloat16()
    got = torch.cat([_run(eye[k:k + 64].contiguous(), w8, scale)
                     for k in range(0, I, 64)])
    assert torch.equal(got.float(), want.float())


def test_batch_invariance_and_isolation():
    x, w8, scale = _inputs(64, 4224, 272, seed=3)
    y64 = _run(x, w8, scale)
    for t in (0, 16, 17, 63):
        assert torch.equal(_run(x[t:t + 1], w8, scale)[0], y64[t]), t
    assert torch.equal(_run(x[:17], w8, scale), y64[:17])
    dev = [t.to(DEV) for t in (x, w8, scale)]
    for tr in (1, 2, 4):     # 17 row tiles: the last block is partly empty
        assert torch.equal(ops.skinny_gemm_fp8_mfma(*dev, tr).cpu(), y64), tr
    x[5] = float("nan")
    ynan = _run(x, w8, scale)
    keep = torch.arange(64) != 5
    assert torch.equal(ynan[keep], y64[keep])
    assert ynan[5].isnan().all()


def test_decode_linear_routing():
    """O = 16384 is the class the measured table routes at every n; the
    256-row weight is in a class that is not routed at n = 64 and keeps the
    bf16 path there (docs/BENCHMARKS.md)."""
    g = torch.Generator().manual_seed(11)
    w = (0.05 * torch.randn(16384, 1024, generator=g)).bfloat16().to(DEV)
    ws = w[:256].clone()
    xs = {n: (0.5 * torch.randn(n, 1024, generator=g)).bfloat16().to(DEV)
          for n in (2, 4, 64)}
    plain4, plain64s = ops.decode_linear(xs[4], w), ops.decode_linear(xs[64], ws)
    for bad in (1, 65, 2.5, None):
        with pytest.raises(ValueError, match="set_fp8_decode_max_batch"):
            ops.set_fp8_decode_max_batch(bad)
    try:
        ops.register_fp8_weight(w)
        ops.register_fp8_weight(ws)
        w8, scale = ops._FP8_WEIGHTS[w.data_ptr()]
        gemv2 = ops.native().skinny_gemm_fp8(xs[2], w8, scale)
        assert torch.equal(ops.decode_linear(xs[4], w), plain4)
        assert torch.equal(ops.decode_linear(xs[2], w), gemv2)
        ops.set_fp8_decode_max_batch(64)
        assert torch.equal(ops.decode_linear(xs[2], w), gemv2)
        for n in (4, 64):
            assert torch.equal(ops.decode_linear(xs[n], w),
                               ops.skinny_gemm_fp8_mfma(xs[n], w8, scale)), n
        assert not torch.equal(ops.decode_linear(xs[4], w), plain4)
        assert torch.equal(ops.decode_linear(xs[64], ws), plain64s)
    finally:
        ops.set_fp8_decode_max_batch(2)
        ops.clear_fp8_weights()


def test_binding_rejects_bad_arguments():
    x, w8, scale = (t.to(DEV) for t in _inputs(4, 256, 32))
    f = ops.skinny_gemm_fp8_mfma
    for msg, args in {
        "N must be 1..64": (x.repeat(17, 1), w8, scale),
        "I must be a positive multiple of 128":
            (x[:, :64].contiguous(), w8[:, :64].contiguous(), scale),
        "O must be a multiple of 16": (x, w8[:24], scale[:24]),
        "X must start on a 16-byte": (x.reshape(-1)[1:257].view(1, 256), w8,
                                      scale),
        "X must be BFloat16": (x.float(), w8, scale),
        "scale must have O": (x, w8, scale[:16]),
    }.items():
        with pytest.raises(RuntimeError, match="skinny_gemm_fp8_mfma: " + msg):
            f(*args)


def test_engine_graph_and_eager_agree_at_batch_4():
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model("llama-smoke", device=DEV)
    outs = []
    try:
        for use_graphs in (True, False):
            eng = Engine("llama-smoke", device=DEV, max_seq=256, max_batch=8,
                         model=model, use_graphs=use_graphs)
            assert eng.enable_fp8_decode(max_batch=4) > 0
            reqs = [eng.submit(Request(prompt_ids=[2 + i, 3, 4, 5],
                                       max_tokens=12)) for i in range(4)]
            eng.start()
            try:
                for r in reqs:
                    assert r.done.wait(120), "request did not complete"
            finally:
                eng.stop()
            if use_graphs:
                assert max(eng.stats["graph_buckets"]) >= 4
            outs.append([r.out_ids for r in reqs])
    finally:
        ops.set_fp8_decode_max_batch(2)
        ops.clear_fp8_weights()
    assert all(len(o) == 12 for o in outs[0]) and outs[0] == outs[1]
