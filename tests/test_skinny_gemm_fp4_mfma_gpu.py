"""ops.skinny_gemm_fp4_mfma (skinny_gemm_fp4_mfma.hip): the MXFP4-weight
decode GEMM on the matrix cores, against fp64 element by element, its exact
k / nibble / block-scale mapping, its batch invariance, its routing and the
engine."""
import pytest
import torch

from skypilot_amd import ops
from _fp64_check import check, tol_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(n, I, O, seed=0):
    """bf16 X = 0.5 randn, codes uniform over all 16 values, and an exponent
    byte drawn independently per block from 112..132 (a constant scale would
    hide a wrong block index)."""
    g = torch.Generator().manual_seed(seed)
    x = (0.5 * torch.randn(n, I, generator=g)).bfloat16()
    codes = torch.randint(0, 256, (O, I // 2), generator=g).to(torch.uint8)
    exps = torch.randint(112, 133, (O, I // 32), generator=g).to(torch.uint8)
    return x, codes, exps


def _run(x, codes, exps, row_tiles=0):
    return ops.skinny_gemm_fp4_mfma(x.to(DEV), codes.to(DEV), exps.to(DEV),
                                    row_tiles).cpu()


# One k chunk (three waves idle); 5 and 33 chunks (the 4-wave split divides
# neither); O = 80, 272: tile counts 5 and 17.  O = 6160 / 16400: two / four
# row tiles per wave with a tile count they do not divide (last block partly
# empty), on each side of the launcher's thresholds O = 6144 and O = 16384.
@pytest.mark.parametrize("n,I,O", [
    (1, 128, 16), (3, 128, 16), (64, 128, 16),
    (16, 640, 80), (17, 640, 80), (48, 640, 80),
    (1, 4224, 272), (17, 4224, 272), (64, 4224, 272),
    (17, 640, 6128), (16, 128, 6160), (17, 640, 6160), (48, 640, 6160),
    (33, 640, 16368), (33, 640, 16400), (64, 128, 16400),
])
def test_fp64_elementwise(n, I, O):
    x, codes, exps = _inputs(n, I, O, seed=n + I + O)
    w = ops.dequantize_mxfp4(codes, exps).double()
    ref = x.double() @ w.t()
    A = x.double().abs() @ w.abs().t()
    check(f"fp4 mfma n={n} I={I} O={O}", _run(x, codes, exps), ref,
          tol_bf16(ref, A, K=I, roundings=1))


@pytest.mark.parametrize("O", [80, 6160, 16400])
def test_one_hot_rows_return_the_weights(O):
    """X[t, k_t] = 1 with k_t running over every k of 5 chunks, 64 rows at a
    time: Y[t, :] is bf16(dequantize_mxfp4(...)[:, k_t]) exactly (+0 for -0
    codes: the accumulator starts at +0), which pins the nibble order, the k
    bijection and the scale-to-block mapping at once."""
    I = 640
    _, codes, exps = _inputs(1, I, O, seed=7)
    want = ops.dequantize_mxfp4(codes, exps).bfloat16().t() + 0.0
    eye = torch.eye(I).bfloat16()
    got = torch.cat([_run(eye[k:k + 64].contiguous(), codes, exps)
                     for k in range(0, I, 64)])
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_batch_invariance_and_isolation():
    x, codes, exps = _inputs(64, 4224, 272, seed=3)
    y64 = _run(x, codes, exps)
    for t in (0, 16, 17, 63):
        assert torch.equal(_run(x[t:t + 1], codes, exps)[0], y64[t]), t
    assert torch.equal(_run(x[:17], codes, exps), y64[:17])
    for tr in (1, 2, 4):     # 17 row tiles: the last block is partly empty
        assert torch.equal(_run(x, codes, exps, tr), y64), tr
    x[5] = float("nan")
    ynan = _run(x, codes, exps)
    keep = torch.arange(64) != 5
    assert torch.equal(ynan[keep], y64[keep])
    assert ynan[5].isnan().all()


def test_decode_linear_routing():
    """O = 16384 is in the class the measured table routes up to n = 48 and
    not at n = 64, which keeps the parent's path (docs/BENCHMARKS.md)."""
    g = torch.Generator().manual_seed(11)
    w = (0.05 * torch.randn(16384, 1024, generator=g)).bfloat16().to(DEV)
    xs = {n: (0.5 * torch.randn(n, 1024, generator=g)).bfloat16().to(DEV)
          for n in (1, 4, 48, 64)}
    plain = {n: ops.decode_linear(xs[n], w) for n in xs}
    for bad in (0, 65, 2.5, None):
        with pytest.raises(ValueError, match="set_fp4_decode_max_batch"):
            ops.set_fp4_decode_max_batch(bad)
    for n in xs:    # nothing registered: the same bits as before
        assert torch.equal(ops.decode_linear(xs[n], w), plain[n]), n
    try:
        ops.register_fp4_weight(w)
        codes, exps = ops._FP4_WEIGHTS[w.data_ptr()]
        for n in (1, 4, 48):
            y = ops.decode_linear(xs[n], w)
            assert torch.equal(
                y, ops.skinny_gemm_fp4_mfma(xs[n], codes, exps)), n
            assert not torch.equal(y, plain[n]), n
        assert torch.equal(ops.decode_linear(xs[64], w), plain[64])
        ops.set_fp4_decode_max_batch(2)
        assert torch.equal(ops.decode_linear(xs[4], w), plain[4])
    finally:
        ops.set_fp4_decode_max_batch(64)
        ops.clear_fp4_weights()


@pytest.mark.parametrize("msg,make", [
    ("N must be 1..64", lambda x, c, e: (x.repeat(17, 1)[:65], c, e)),
    ("I must be a positive multiple of 128",
     lambda x, c, e: (x[:, :64].contiguous(), c[:, :32].contiguous(),
                      e[:, :2].contiguous())),
    ("O must be a positive multiple of 16", lambda x, c, e: (x, c[:24], e[:24])),
    ("X must start on a 16-byte",
     lambda x, c, e: (x.reshape(-1)[1:257].view(1, 256), c, e)),
    ("X must be BFloat16", lambda x, c, e: (x.float(), c, e)),
    ("codes must be Byte", lambda x, c, e: (x, c.view(torch.int8), e)),
    ("codes must be \\[O, I/2\\]",
     lambda x, c, e: (x, c[:, :64].contiguous(), e)),
    ("exps must be \\[O, I/32\\]", lambda x, c, e: (x, c, e[:16])),
])
def test_binding_rejects_bad_arguments(msg, make):
    x, codes, exps = (t.to(DEV) for t in _inputs(4, 256, 32))
    with pytest.raises(RuntimeError, match="skinny_gemm_fp4_mfma: " + msg):
        ops.skinny_gemm_fp4_mfma(*make(x, codes, exps))


def test_engine_graph_and_eager_agree_at_batch_4():
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model("llama-smoke", device=DEV)
    outs = []
    try:
        for use_graphs in (True, False):
            eng = Engine("llama-smoke", device=DEV, max_seq=256, max_batch=8,
                         model=model, use_graphs=use_graphs)
            assert eng.enable_fp4_decode(max_batch=4) > 0
            with pytest.raises(ValueError, match="already serves fp4"):
                eng.enable_fp8_decode()
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
        ops.set_fp4_decode_max_batch(64)
        ops.clear_fp4_weights()
        ops.clear_fp8_weights()
    assert all(len(o) == 12 for o in outs[0]) and outs[0] == outs[1]
