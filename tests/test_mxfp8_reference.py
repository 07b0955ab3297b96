"""ops.quantize_mxfp8 / ops.dequantize_mxfp8: the MXFP8 activation format in
plain torch (e4m3fn codes in blocks of 32 k, one E8M0 exponent byte each),
and the CPU form of ops.gemm_mxfp4_a8."""
import pytest
import torch

from skypilot_amd import ops


def edge_blocks():
    """[7, 32] bf16, one block a row: amax exactly 448 * 2^n (n = 0, 5, -9),
    the next bf16 above 448, a zero block, one large value over 31 tiny ones
    that land on e4m3 subnormals, their ties and zero, and a block below the
    clamp of n (all codes +-0)."""
    x = torch.zeros(7, 32)
    x[0, :4] = torch.tensor([448.0, -1.0, 0.40625, 17.0])
    x[1, :3] = torch.tensor([448.0 * 32, -3.0, 100.0])
    x[2, :3] = torch.tensor([448.0 / 512, 0.001, -0.5])
    x[3, :3] = torch.tensor([450.0, 448.0, -30.0])         # n = 1
    x[5, 0] = 448.0
    x[5, 1:] = torch.arange(1, 32) * 2.0 ** -11 * (-1.0) ** torch.arange(31)
    x[6] = 2.0 ** -120 * (-1.0) ** torch.arange(32)
    return x.bfloat16()


EDGE_EXPS = [127, 132, 118, 128, 127, 127, 27]


def test_block_exponent_at_the_rules_edges():
    codes, exps = ops.quantize_mxfp8(edge_blocks())
    assert exps.reshape(-1).tolist() == EDGE_EXPS
    assert codes[:3, 0].tolist() == [0x7E] * 3 and codes[3, :2].tolist() == [
        0x76, 0x76]                     # 225 and 224 at scale 2: both 224
    assert not codes[4].any() and codes[6].tolist() == [0, 0x80] * 16


def test_subnormals_ties_and_zeros():
    """Block 5 at n = 0: value i * 2^-11 is code RNE(i / 4) in units of 2^-9,
    sign kept (a tie at i = 2, 6, 10, ... goes to the even code)."""
    codes = ops.quantize_mxfp8(edge_blocks())[0][5, 1:].tolist()
    want = [0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 6,
            6, 6, 6, 6, 7, 7, 7, 8, 8]
    assert [c & 0x7F for c in codes] == want
    assert [c >> 7 for c in codes] == [i % 2 for i in range(31)]


def test_round_trip_of_representable_values():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 256, (8, 256), generator=g).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x7E        # no NaN codes
    codes[:, 31::32] = 0x7E                      # amax 448: n is the exponent
    exps = torch.randint(60, 200, (8, 8), generator=g).to(torch.uint8)
    x = ops.dequantize_mxfp8(codes, exps)
    assert torch.equal(x, x.bfloat16().float())
    c2, e2 = ops.quantize_mxfp8(x.bfloat16())
    assert torch.equal(e2, exps)
    assert torch.equal(ops.dequantize_mxfp8(c2, e2), x)
    cp, ep = ops.quantize_mxfp8_rows(x.bfloat16())
    assert cp.shape == (128, 256) and ep.shape == (128, 8)
    assert torch.equal(cp[:8], c2) and torch.equal(ep[:8], e2)
    assert not cp[8:].any() and (ep[8:] == 127).all()
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.quantize_mxfp8(torch.zeros(2, 48).bfloat16())


def test_cpu_gemm_is_its_formula_and_routing_stays_off_the_cpu():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(5, 256, generator=g) * 3).bfloat16()
    w = (0.05 * torch.randn(128, 256, generator=g)).bfloat16()
    codes, exps = ops.quantize_mxfp4(w)
    want = (ops.dequantize_mxfp8(*ops.quantize_mxfp8(x))
            @ ops.dequantize_mxfp4(codes, exps).t())
    assert torch.equal(ops.gemm_mxfp4_a8(x, codes, exps), want.bfloat16())
    before = ops.linear(x, w)
    try:
        ops.register_fp4_weight(w)
        ops.set_fp4_prefill(1)
        with torch.no_grad():
            assert torch.equal(ops.linear(x, w), before)
    finally:
        ops.set_fp4_prefill(None)
        ops.clear_fp4_weights()
    for bad in (0, 2.5, True, "on"):
        with pytest.raises(ValueError, match="set_fp4_prefill"):
            ops.set_fp4_prefill(bad)
