"""ops.quantize_mxfp4 / ops.dequantize_mxfp4: the MXFP4 weight format in
plain torch (e2m1 codes in blocks of 32 k, one E8M0 exponent byte each)."""
import pytest
import torch

from skypilot_amd import ops

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _block(values, amax=6.0):
    """One 32-wide bf16 block holding `values`, its amax pinned by the last
    element (6.0 gives n = 0, so codes are those of the values themselves)."""
    row = torch.zeros(32)
    row[:len(values)] = torch.tensor(values)
    row[31] = amax
    return row.bfloat16().reshape(1, 32)


def _nibbles(codes):
    return torch.stack([codes & 15, codes >> 4], -1).reshape(codes.shape[0], -1)


def test_all_16_codes_round_trip():
    codes = (torch.arange(16) | (torch.arange(16).flip(0) << 4)).to(torch.uint8)
    codes = codes.reshape(1, 16)
    exps = torch.tensor([[127]], dtype=torch.uint8)
    w = ops.dequantize_mxfp4(codes, exps)
    want = torch.tensor(GRID + [-v for v in GRID])
    assert torch.equal(w[0, 0::2], want) and torch.equal(w[0, 1::2], want.flip(0))
    w[0, 31] = 6.0                      # pin the scale: the block holds a 6
    c2, e2 = ops.quantize_mxfp4(w.bfloat16())
    assert int(e2) == 127
    assert torch.equal(ops.dequantize_mxfp4(c2, e2), w)
    for e in (27, 120, 227):            # the scale is 2^(e-127), exactly
        exps[0, 0] = e
        assert torch.equal(ops.dequantize_mxfp4(codes, exps)[0, 0::2],
                           want * 2.0 ** (e - 127))


def test_ties_go_to_the_even_code():
    mids = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    even = [0, 2, 2, 4, 4, 6, 6]
    codes, exps = ops.quantize_mxfp4(_block(mids + [-m for m in mids]))
    assert int(exps) == 127
    got = _nibbles(codes)[0, :14].tolist()
    assert got[:7] == even
    assert [c & 7 for c in got[7:]] == even and all(c & 8 for c in got[8:])


@pytest.mark.parametrize("amax,e", [(6.0, 127), (6.5, 128), (3.0, 126),
                                    (6.03125, 128), (0.0, 127)])
def test_block_exponent(amax, e):
    """amax 6 and 6.5 take neighbouring exponents; a zero block gives 127."""
    assert int(ops.quantize_mxfp4(_block([], amax))[1]) == e


def test_scaled_amax_range_and_half_step_error():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 256, generator=g)
         * torch.logspace(-6, 6, 64, base=2.0)[:, None]).bfloat16()
    codes, exps = ops.quantize_mxfp4(w)
    assert codes.shape == (64, 128) and exps.shape == (64, 8)
    scale = 2.0 ** (exps.double() - 127)
    blocks = w.double().reshape(64, 8, 32)
    ratio = blocks.abs().amax(-1) / scale
    assert (ratio > 3).all() and (ratio <= 6).all()
    # half the gap to the neighbouring grid value: .25 below 2, .5 below 4, 1
    a = blocks.abs() / scale[..., None]
    half = torch.where(a < 2, 0.25, torch.where(a < 4, 0.5, 1.0))
    err = (ops.dequantize_mxfp4(codes, exps).double().reshape(64, 8, 32)
           - blocks).abs() / scale[..., None]
    assert (err <= half).all()


def test_decode_linear_unchanged_on_cpu_with_a_weight_registered():
    g = torch.Generator().manual_seed(1)
    w = (0.05 * torch.randn(32, 128, generator=g)).bfloat16()
    x = torch.randn(3, 128, generator=g).bfloat16()
    before = ops.decode_linear(x, w)
    try:
        ops.register_fp4_weight(w)
        assert torch.equal(ops.decode_linear(x, w), before)
        codes, exps = ops._FP4_WEIGHTS[w.data_ptr()]
        y = ops.skinny_gemm_fp4_mfma(x, codes, exps)
        want = x.float() @ ops.dequantize_mxfp4(codes, exps).t()
        assert torch.equal(y, want.bfloat16())
    finally:
        ops.clear_fp4_weights()
    for bad in (0, 65, 2.5, None):
        with pytest.raises(ValueError, match="set_fp4_decode_max_batch"):
            ops.set_fp4_decode_max_batch(bad)
