"""The CPU side of the fp8-weight GEMM beyond 64 tokens: set_fp8_prefill's
argument check, the fallback's value and the engine's registration."""
import pytest
import torch

from skypilot_amd import ops


def test_set_fp8_prefill_validates():
    for bad in (0, -3, 2.5, True, "always"):
        with pytest.raises(ValueError, match="set_fp8_prefill"):
            ops.set_fp8_prefill(bad)
    assert ops._FP8_PREFILL is None and "set_fp8_prefill" in ops.__all__


def test_cpu_fallback_is_the_dequantised_matmul():
    g = torch.Generator().manual_seed(0)
    w8, scale = ops.quantize_fp8_rowwise(
        (0.05 * torch.randn(64, 128, generator=g)).bfloat16())
    x = torch.randn(70, 128, generator=g).bfloat16()
    w = w8.view(torch.float8_e4m3fn).float() * scale[:, None]
    assert torch.equal(ops.gemm_fp8_w8(x, w8, scale),
                       (x.float() @ w.t()).bfloat16())


def test_enable_fp8_prefill_registers_once():
    from skypilot_amd.serve.engine import Engine
    try:
        eng = Engine("llama-debug", device="cpu", max_seq=64, max_batch=2)
        # 2 blocks x (q, k, v, o, gate|up, down) + lm_head
        assert eng.enable_fp8_prefill(min_tokens=65, min_bytes=1 << 16) == 13
        assert ops._FP8_PREFILL == 65
        assert eng.enable_fp8_prefill() == 13 and len(ops._FP8_WEIGHTS) == 13
        assert ops._FP8_PREFILL == "measured"
    finally:
        ops.set_fp8_prefill(None)
        ops.clear_fp8_weights()
