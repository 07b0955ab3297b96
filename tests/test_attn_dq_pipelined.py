"""Pipelined attention dQ backward kernel (attn_bwd dq_variant 1) against
the fp32 reference and, bit for bit, against the plain v3 dq kernel
(dq_variant 0)."""
import functools

import pytest
import torch

from skypilot_amd import ops

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5
TOL = 0.08  # test_attn_dkv_pipelined's backward tolerance

# (B, S, Hq, Hkv, causal): the smallest shapes at which each mechanism of
# the pipelined kernel can go wrong.
SHAPES = [
    (1, 128, 1, 1, True),    # one unpaired q tile, two kv tiles; waves 0-1
                             # skip the second but take barrier + staging
    (1, 256, 1, 1, True),    # one paired block: the pair boundary reloads
                             # Q/dO/lse/Dvec and keeps the buffer parity
    (1, 128, 4, 1, False),   # non-causal, group of 4
    (2, 512, 8, 2, True),    # two paired blocks per head, B > 1, GQA 4
    (1, 384, 5, 1, True),    # odd q-tile count: unpaired causal grid
    (3, 640, 6, 2, True),    # the same with B*Hkv > 1
    (1, 512, 4, 4, False),   # eight kv tiles non-causal, group 1
]


def _inputs(B, S, Hq, Hkv):
    g = torch.Generator(device="cuda").manual_seed(1000 * S + 10 * Hq + B)

    def rnd(*shape):
        return (torch.randn(*shape, device="cuda", generator=g)
                * 0.5).bfloat16()

    q, k, v = rnd(B, S, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
    return q, k, v, rnd(B, S, Hq, D)


@functools.lru_cache(maxsize=None)
def _case(B, S, Hq, Hkv, causal):
    """Inputs, forward results, the fp32 reference dQ and the gradients of
    both dq variants; computed once per shape and shared (read-only)."""
    q, k, v, dO = _inputs(B, S, Hq, Hkv)
    C = ops.native()
    O, lse = C.attn_fwd(q, k, v, SCALE, causal)
    qf = q.float().requires_grad_(True)
    ops.attention_ref(qf, k.float(), v.float(), SCALE,
                      causal=causal).backward(dO.float())
    args = (q, k, v, O, dO, lse)
    return args, qf.grad, _bwd(args, causal, 0), _bwd(args, causal, 1)


def _bwd(args, causal, dq_variant):
    return ops.native().attn_bwd(*args, SCALE, causal, dq_variant=dq_variant)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dq_matches_reference(shape):
    _, ref, _, got = _case(*shape)
    torch.testing.assert_close(got[0].float(), ref, atol=TOL, rtol=TOL,
                               msg=lambda m: f"dQ {shape}: {m}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dq_pipelined_bit_identical(shape):
    """Same MFMA sequence and accumulation order: dQ (and dK, dV, which
    the dq variant does not touch) equal the plain v3 kernel's bits."""
    _, _, base, got = _case(*shape)
    for name, a, b in zip(("dQ", "dK", "dV"), got, base):
        assert torch.equal(a, b), f"{name} differs from variant 0 at {shape}"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dq_pipelined_deterministic(shape):
    args, _, _, first = _case(*shape)
    second = _bwd(args, shape[4], 1)
    for name, a, b in zip(("dQ", "dK", "dV"), first, second):
        assert torch.equal(a, b), f"{name} not reproducible at {shape}"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_default_dq_variant_is_a_v3_kernel(shape):
    """dq_variant omitted (-1) agrees bit for bit with an explicit variant
    (the two are themselves bit-identical, tested above)."""
    args, _, base, got = _case(*shape)
    dflt = ops.native().attn_bwd(*args, SCALE, shape[4])
    for name, a, b, c in zip(("dQ", "dK", "dV"), dflt, base, got):
        assert torch.equal(a, b) or torch.equal(a, c), \
            f"default {name} matches neither dq variant at {shape}"


def test_dq_variant_range_checked():
    args = _case(1, 128, 1, 1, True)[0]
    with pytest.raises(RuntimeError, match="dq_variant"):
        _bwd(args, True, 2)


@pytest.mark.parametrize("shape", [(1, 128, 1, 1, True),
                                   (1, 512, 4, 4, False)], ids=str)
def test_staging_stays_inside_the_sequence(shape):
    """The last iteration stages a tile unconditionally.  K and V are the
    leading S rows of buffers whose following rows are NaN: a staged row
    past S of the last batch would reach the output (NaN * 0 is NaN even
    under the causal mask's zero probabilities) or at least change it."""
    B, S, Hq, Hkv, causal = shape
    args, _, _, want = _case(*shape)
    q, k, v, O, dO, lse = args
    pad = 128

    def padded(t):
        buf = torch.full((B, S + pad, Hkv, D), float("nan"),
                         dtype=t.dtype, device=t.device)
        buf[:, :S] = t
        view = buf[:, :S]
        assert view.is_contiguous()  # B == 1
        return view

    got = _bwd((q, padded(k), padded(v), O, dO, lse), causal, 1)
    for name, a, b in zip(("dQ", "dK", "dV"), got, want):
        assert torch.isfinite(a.float()).all(), f"{name} not finite"
        assert torch.equal(a, b), f"{name} differs from the unpadded call"
