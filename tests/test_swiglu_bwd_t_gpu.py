"""swiglu_bwd_t (swiglu.hip): swiglu_bwd that also writes the transposed
gradient.  Nothing changes arithmetic, so every comparison is bit-exact:
dgu against swiglu_bwd, dguT against dgu's transpose."""
import pytest
import torch

from skypilot_amd import ops

gpu = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def inputs(rows, M, seed):
    g = torch.Generator().manual_seed(seed)
    gu = (torch.randn(rows, 2 * M, generator=g) * 3).bfloat16().to(dev())
    dy = (torch.randn(rows, M, generator=g) * 3).bfloat16().to(dev())
    return gu, dy


# 64: one tile; 192: three tiles a side, nine tiles per half, so a block's
# second half-tile lands next to another block's first
@gpu
@pytest.mark.parametrize("rows", [64, 192])
@pytest.mark.parametrize("M", [64, 192])
def test_matches_swiglu_bwd_and_its_transpose(rows, M):
    C = ops.native()
    gu, dy = inputs(rows, M, seed=rows + M)
    ref = C.swiglu_bwd(gu, dy)
    dgu, dguT = C.swiglu_bwd_t(gu, dy)
    assert dgu.shape == (rows, 2 * M) and dgu.is_contiguous()
    assert dguT.shape == (2 * M, rows) and dguT.is_contiguous()
    assert torch.equal(bits(dgu), bits(ref))
    assert torch.equal(bits(dguT), bits(ref.t()))


# 3,200 tiles: more than the launch's 3,072 blocks, so the grid-stride loop
# takes a second trip and the LDS image is reused across tiles
@gpu
def test_more_tiles_than_blocks():
    C = ops.native()
    gu, dy = inputs(2560, 5120, seed=3)
    ref = C.swiglu_bwd(gu, dy)
    dgu, dguT = C.swiglu_bwd_t(gu, dy)
    assert torch.equal(bits(dgu), bits(ref))
    assert torch.equal(bits(dguT), bits(ref.t()))


@gpu
def test_rejects_shapes_off_the_tile():
    C = ops.native()
    for rows, M in ((32, 64), (64, 96)):
        gu, dy = inputs(rows, M, seed=1)
        with pytest.raises(RuntimeError, match="swiglu_bwd_t: rows and M"):
            C.swiglu_bwd_t(gu, dy)
    gu, dy = inputs(64, 64, seed=2)
    with pytest.raises(RuntimeError, match="swiglu_bwd_t: gu must be"):
        C.swiglu_bwd_t(gu, dy[:, :32].contiguous())
    with pytest.raises(RuntimeError, match="swiglu_bwd_t: dy must be"):
        C.swiglu_bwd_t(gu, dy.float())


def run_mlp(fused, route):
    """One gate|up + swiglu + sum backward at `route`; (y, dx, dw)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 64, 128, generator=g).bfloat16().to(dev())
    w = (torch.randn(256, 128, generator=g) * 0.1).bfloat16().to(dev())
    x.requires_grad_()
    w.requires_grad_()
    if fused:
        # linear_swiglu takes the table route; force one as the model test
        # of test_linear_wgrad.py does, through ops.linear
        real = ops.linear
        ops.linear = lambda x, w, b=None: real(x, w, b, route=route)
        try:
            y = ops.linear_swiglu(x, w)
        finally:
            ops.linear = real
    else:
        y = ops.swiglu(ops.linear(x, w, route=route))
    y.backward(torch.ones_like(y) * 0.5)
    return y.detach(), x.grad, w.grad


@gpu
@pytest.mark.parametrize("route", [0, 1, 2])
def test_linear_swiglu_equals_the_two_ops(route):
    """The fused node's forward, dx and dW are those of swiglu(linear()),
    whether its backward hands the transposed gradient over (1, 2) or not
    (0)."""
    for a, b in zip(run_mlp(True, route), run_mlp(False, route)):
        assert torch.equal(bits(a), bits(b))
