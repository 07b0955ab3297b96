"""ops.skinny_gemm_bf16_mfma off the GPU: the fallback and the switch."""
import pytest
import torch

from skypilot_amd import ops


def test_cpu_fallback_and_setter():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 128, generator=g).bfloat16()
    w = torch.randn(16, 128, generator=g).bfloat16()
    want = (x.float() @ w.float().t()).bfloat16()
    assert torch.equal(ops.skinny_gemm_bf16_mfma(x, w), want)
    assert ops._BF16_MAX_BATCH == 1
    for bad in (0, 65, 2.5, None, True):
        with pytest.raises(ValueError, match="set_bf16_decode_max_batch"):
            ops.set_bf16_decode_max_batch(bad)
    try:
        ops.set_bf16_decode_max_batch(64)
        assert torch.equal(ops.decode_linear(x, w),
                           torch.nn.functional.linear(x, w))
    finally:
        ops.set_bf16_decode_max_batch(1)
