"""Pipelined attention dK/dV backward kernel (attn_bwd dkv_variant 1 and
2) against the fp32 reference and, bit for bit, against the plain v3 dkv
kernel (dkv_variant 0); plus the v1 backward kernels after the Dvec
relayout to [B,Hq,S]."""
import functools

import pytest
import torch

from skypilot_amd import ops

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5
TOL = 0.08  # test_attention_shape_fuzz's backward tolerance

# (B, S, Hq, Hkv, causal): the smallest shapes at which each mechanism of
# the pipelined kernel can go wrong.
SHAPES = [
    (1, 128, 1, 1, True),    # one kv tile, one head: prologue + 4 tiles,
                             # waves 1-3 skip tiles but take the barriers
    (1, 128, 4, 1, False),   # prefetch across the q-head boundary
    (2, 256, 8, 2, True),    # two kv tiles, B > 1, flagship GQA ratio
    (1, 384, 5, 1, True),    # odd tile count, odd group, Hkv = 1
    (3, 640, 6, 2, True),    # odd tile count, B*Hkv > 1: block-order remap
    (1, 512, 4, 4, False),   # group 1, non-causal
]


@functools.lru_cache(maxsize=None)
def _case(B, S, Hq, Hkv, causal):
    """Inputs, forward results and the fp32 reference gradients; computed
    once per shape and shared (read-only) by the tests below."""
    g = torch.Generator(device="cuda").manual_seed(1000 * S + 10 * Hq + B)

    def rnd(*shape):
        return (torch.randn(*shape, device="cuda", generator=g)
                * 0.5).bfloat16()

    q, k, v = rnd(B, S, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
    dO = rnd(B, S, Hq, D)
    C = ops.native()
    O, lse = C.attn_fwd(q, k, v, SCALE, causal)
    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    ops.attention_ref(qf, kf, vf, SCALE, causal=causal).backward(dO.float())
    return (q, k, v, O, dO, lse), (qf.grad, kf.grad, vf.grad)


def _bwd(args, causal, variant):
    return ops.native().attn_bwd(*args, SCALE, causal, variant)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dkv_matches_reference(shape, variant):
    args, ref = _case(*shape)
    got = _bwd(args, shape[4], variant)
    for name, a, r in zip(("dQ", "dK", "dV"), got, ref):
        torch.testing.assert_close(a.float(), r, atol=TOL, rtol=TOL,
                                   msg=lambda m: f"{name} {shape}: {m}")


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dkv_pipelined_bit_identical(shape, variant):
    """Same MFMA sequence and accumulation order: dK, dV (and dQ, which
    the dkv variant does not touch) equal the plain v3 kernel's bits."""
    args, _ = _case(*shape)
    base = _bwd(args, shape[4], 0)
    got = _bwd(args, shape[4], variant)
    for name, a, b in zip(("dQ", "dK", "dV"), got, base):
        assert torch.equal(a, b), f"{name} differs from variant 0 at {shape}"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dkv_pipelined_deterministic(shape):
    args, _ = _case(*shape)
    first = _bwd(args, shape[4], 1)
    second = _bwd(args, shape[4], 1)
    for name, a, b in zip(("dQ", "dK", "dV"), first, second):
        assert torch.equal(a, b), f"{name} not reproducible at {shape}"


def test_default_variant_is_a_v3_kernel():
    """dkv_variant omitted (-1) must agree bit for bit with the explicit
    variants — whichever of them the default resolves to."""
    shape = (2, 256, 8, 2, True)
    args, _ = _case(*shape)
    C = ops.native()
    dflt = C.attn_bwd(*args, SCALE, True)
    base = _bwd(args, True, 0)
    for a, b in zip(dflt, base):
        assert torch.equal(a, b)


def test_v1_kernels_after_dvec_relayout():
    """S % 128 != 0 routes to the v1 dkv/dq kernels, which read Dvec in
    its new [B,Hq,S] layout."""
    shape = (2, 192, 4, 4, False)
    args, ref = _case(*shape)
    got = _bwd(args, False, -1)
    for name, a, r in zip(("dQ", "dK", "dV"), got, ref):
        torch.testing.assert_close(a.float(), r, atol=TOL, rtol=TOL,
                                   msg=lambda m: f"{name} {shape}: {m}")
