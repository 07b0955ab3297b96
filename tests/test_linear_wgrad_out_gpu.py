"""linear_wgrad(dy, x, route, dyT=, out=): a weight gradient written into a
caller's tensor (a gradient-bucket view) and from a dy the caller already
transposed.  Both run the library product the plain call runs, so every
comparison is bit-exact."""
import pytest
import torch

from skypilot_amd import ops

gpu = pytest.mark.gpu
GUARD = 4096
PATTERN = 0x5A5A
SHAPES = [(128, 128, 64), (256, 64, 192)]      # M, out, in


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def operands(M, O, I):
    g = torch.Generator().manual_seed(M + O + I)
    dy = torch.randn(M, O, generator=g).bfloat16().to(dev())
    x = torch.randn(M, I, generator=g).bfloat16().to(dev())
    return dy, x


def guarded(O, I):
    """A flat buffer of a known pattern and the [O, I] view in its middle, as
    a DDP bucket holds one parameter's gradient among others."""
    flat = torch.full((GUARD + O * I + GUARD,), PATTERN, dtype=torch.int16,
                      device=dev()).view(torch.bfloat16)
    return flat, flat[GUARD:GUARD + O * I].view(O, I)


@gpu
@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("M,O,I", SHAPES)
def test_out_equals_plain_call_and_stays_in_its_view(route, M, O, I):
    C = ops.native()
    dy, x = operands(M, O, I)
    ref = C.linear_wgrad(dy, x, route)
    flat, view = guarded(O, I)
    got = C.linear_wgrad(dy, x, route, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(bits(view), bits(ref))
    f = bits(flat)
    assert bool((f[:GUARD] == PATTERN).all())
    assert bool((f[GUARD + O * I:] == PATTERN).all())


@gpu
@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("M,O,I", SHAPES)
def test_dyT_equals_plain_call(route, M, O, I):
    """Routes 1 and 2 use the given transpose; route 0 ignores it (here a
    wrong one, which must not show)."""
    C = ops.native()
    dy, x = operands(M, O, I)
    ref = C.linear_wgrad(dy, x, route)
    dyT = dy.t().contiguous() if route else torch.zeros(
        O, M, dtype=torch.bfloat16, device=dev())
    assert torch.equal(bits(C.linear_wgrad(dy, x, route, dyT=dyT)), bits(ref))
    flat, view = guarded(O, I)
    C.linear_wgrad(dy, x, route, dyT=dyT, out=view)
    assert torch.equal(bits(view), bits(ref))


@gpu
def test_rejects_bad_out_and_dyT():
    C = ops.native()
    M, O, I = SHAPES[0]
    dy, x = operands(M, O, I)
    z = torch.zeros
    kw = dict(dtype=torch.bfloat16, device=dev())
    with pytest.raises(RuntimeError, match=r"linear_wgrad: out must be \[out"):
        C.linear_wgrad(dy, x, 1, out=z(O, I + 64, **kw))
    with pytest.raises(RuntimeError, match=r"linear_wgrad: out must be \[out"):
        C.linear_wgrad(dy, x, 0, out=z(O * I, **kw))
    with pytest.raises(RuntimeError, match="linear_wgrad: out must be contig"):
        C.linear_wgrad(dy, x, 2, out=z(I, O, **kw).t())
    with pytest.raises(RuntimeError, match="linear_wgrad: out must be"):
        C.linear_wgrad(dy, x, 2, out=z(O, I, dtype=torch.float32,
                                       device=dev()))
    with pytest.raises(RuntimeError, match=r"linear_wgrad: dyT must be \[out"):
        C.linear_wgrad(dy, x, 1, dyT=z(M, O + 64, **kw))
    with pytest.raises(RuntimeError, match="linear_wgrad: dyT must be contig"):
        C.linear_wgrad(dy, x, 1, dyT=dy.t())
