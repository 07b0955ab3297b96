"""The training attention kernels element by element against fp64
(tests/_attn_fp64.py has the references, the bound and its derivation).

Forward (C.attn_fwd): O and lse.  Backward (C.attn_bwd): dQ, dK, dV from
the *reference's* O and lse, so a forward error can neither mask nor cause
a backward one; then chained through ops.attention.  The v3 kernels are
held to two references: the declared-operand one, which carries the
precision, and the plain one, which proves that the declared operand is
bf16(x * qs).  The 64-tile kernels re-round nothing; the plain reference
is their declared one.

Routes: S % 256 == 0 runs the v3 forward, S % 128 == 0 the v3 backward
(dkv_variant 0, 1, 2 and dq_variant 0, 1), every other S % 64 == 0 the
64-tile kernels.

    fwd 64-tile + bwd 64-tile   S = 64, 192, 320   1, 3, 5 tiles
    fwd 64-tile + bwd v3        S = 128, 384, 640  dq grid unpaired at odd
                                                   tile counts
    fwd v3      + bwd v3        S = 256, 512, 768  causal grids paired

Each route meets each input family once and each head shape once; run
with ``-s`` for the worst err/tol per kernel and reference."""
import functools

import pytest
import torch

import _attn_fp64 as af
from _fp64_check import check, within
from skypilot_amd import ops

pytestmark = pytest.mark.gpu

SCALE = af.SCALE
ROUTES = [(64, 192, 320), (128, 384, 640), (256, 512, 768)]
HEADS = [(1, 1, 1), (1, 4, 1), (2, 8, 2), (1, 5, 1), (3, 6, 2), (1, 4, 4)]


def _cases():
    """(family, B, S, Hq, Hkv, causal): per route, family i takes head
    shape (i + route) % 6 -- nine families cover the six shapes -- and the
    route's sizes in turn; the shapes with 16 and 18 q heads take the
    route's middle size, and causal alternates."""
    out = []
    for r, sizes in enumerate(ROUTES):
        for i, fam in enumerate(af.FAMILIES):
            B, Hq, Hkv = HEADS[(i + r) % 6]
            S = sizes[1] if B * Hq >= 16 else sizes[i % 3]
            out.append((fam, B, S, Hq, Hkv, (i + r) % 2 == 0))
    return out


CASES = _cases()
assert all(S <= 768 and B * Hq <= 18 for _, B, S, Hq, _, _ in CASES)
for _r, _sizes in enumerate(ROUTES):
    _mine = [c for c in CASES if c[2] in _sizes]
    assert {c[0] for c in _mine} == set(af.FAMILIES)
    assert {(c[1], c[3], c[4]) for c in _mine} == set(HEADS)
    assert {c[2] for c in _mine} == set(_sizes)
    assert {c[5] for c in _mine} == {True, False}


def _fwd_kernel(S):
    return "fwd_v3" if S % 256 == 0 else "fwd64"


def _bwd_v3(S):
    return S % 128 == 0


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


@functools.lru_cache(maxsize=None)
def _fwd_case(case):
    """CPU inputs and the forward references [(name, ref)], declared
    first; computed once per case and shared read-only."""
    fam, B, S, Hq, Hkv, causal = case
    q, k, v, dO = af.make_inputs(fam, B, S, Hq, Hkv)
    kern = _fwd_kernel(S)
    if kern == "fwd_v3":
        refs = [("declared", af.fwd_ref(q, k, v, SCALE, causal, operand="q",
                                        r_P=af.R_P)),
                ("plain", af.fwd_ref(q, k, v, SCALE, causal, rerounded=True,
                                     r_P=af.R_P))]
    else:
        refs = [("plain", af.fwd_ref(q, k, v, SCALE, causal,
                                     r_P=af.R_P))]
    return (q, k, v, dO), kern, refs


@functools.lru_cache(maxsize=None)
def _fwd_run(case):
    (q, k, v, _), _, _ = _fwd_case(case)
    O, lse = ops.native().attn_fwd(*_cuda(q, k, v), SCALE, case[5])
    return O.cpu(), lse.cpu()


def _given(case):
    """The backward's given inputs: O = bf16(ref O), lse = fp32(ref lse)
    of the plain reference, in the kernels' layout (CPU)."""
    _, _, refs = _fwd_case(case)
    plain = dict(refs)["plain"]
    O = plain.O.permute(0, 2, 1, 3).bfloat16().contiguous()
    return O, plain.lse.float()


def _bwd_refs(case, O, lse, extra=None):
    """[(name, ref, gradients it judges)] for the route's backward."""
    fam, B, S, Hq, Hkv, causal = case
    (q, k, v, dO), _, _ = _fwd_case(case)
    args = (q, k, v, O, dO, lse, SCALE, causal)
    if not _bwd_v3(S):
        return [("plain", af.bwd_ref(*args, r_P=af.R_P,
                                     extra_delta=extra), ("dQ", "dK", "dV"))]
    return [
        ("declared", af.bwd_ref(*args, operand="q", extra_delta=extra),
         ("dQ",)),
        ("declared", af.bwd_ref(*args, operand="k", r_P=af.R_P,
                                extra_delta=extra), ("dK", "dV")),
        ("plain", af.bwd_ref(*args, rerounded=True, r_P=af.R_P,
                             extra_delta=extra), ("dQ", "dK", "dV")),
    ]


@functools.lru_cache(maxsize=None)
def _bwd_case(case):
    O, lse = _given(case)
    return O, lse, _bwd_refs(case, O, lse)


def _variants(S):
    """(dkv_variant, dq_variant) runs that reach every backward kernel."""
    return [(0, 0), (1, 1), (2, 1)] if _bwd_v3(S) else [(-1, -1)]


def _bwd_names(S, dkv, dq):
    if not _bwd_v3(S):
        return {"dQ": "dq64", "dK": "dkv64", "dV": "dkv64"}
    return {"dQ": f"dq_v3[{dq}]", "dK": f"dkv_v3[{dkv}]",
            "dV": f"dkv_v3[{dkv}]"}


def _check_grads(tag, case, grads, refs, names):
    for rname, ref, judged in refs:
        for gname in judged:
            got = af.to_heads(grads[gname])
            check(f"{names[gname]} {gname} vs {rname} {tag}", got,
                  getattr(ref, gname), getattr(ref, "tol_" + gname))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward(case):
    fam, B, S, Hq, Hkv, causal = case
    _, kern, refs = _fwd_case(case)
    O, lse = _fwd_run(case)
    for rname, ref in refs:
        check(f"{kern} O vs {rname} {case}", af.to_heads(O), ref.O, ref.tol_O)
        check(f"{kern} lse vs {rname} {case}", lse.double(), ref.lse,
              ref.tol_lse)
    if fam == "equal":
        # q = 0: p is exactly uniform, lse_i = ln(i + 1) or ln S
        n = torch.arange(1, S + 1).double() if causal else \
            torch.full((S,), float(S), dtype=torch.float64)
        want = n.log().expand(B, Hq, S)
        check(f"{kern} lse vs ln(n) {case}", lse.double(), want,
              refs[0][1].tol_lse)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_backward_isolated(case):
    S, causal = case[2], case[5]
    (q, k, v, dO), _, _ = _fwd_case(case)
    O, lse, refs = _bwd_case(case)
    dev = _cuda(q, k, v, O, dO, lse)
    for dkv, dq in _variants(S):
        got = ops.native().attn_bwd(*dev, SCALE, causal, dkv_variant=dkv,
                                    dq_variant=dq)
        grads = dict(zip(("dQ", "dK", "dV"), (g.cpu() for g in got)))
        _check_grads(str(case), case, grads, refs, _bwd_names(S, dkv, dq))


# One GQA shape per route, both maskings among them.
CHAINED = [("unit", 2, 192, 8, 2, True), ("flat", 1, 384, 4, 1, False),
           ("unit", 1, 512, 4, 1, True)]


@pytest.mark.parametrize("case", CHAINED, ids=str)
def test_backward_chained(case):
    """Gradients through ops.attention.  The backward kernel receives the
    forward kernel's O and lse.  O is a given input of the backward
    formula, so the reference takes the kernel's O as it is; lse stays the
    reference's, and since p scales by exp(lse_ref - lse_kernel) the score
    error of every q row is widened by the forward's own lse tolerance."""
    fam, B, S, Hq, Hkv, causal = case
    (q, k, v, dO), _, frefs = _fwd_case(case)
    qd, kd, vd = (t.cuda().requires_grad_() for t in (q, k, v))
    out = ops.attention(qd, kd, vd, SCALE, causal)
    out.backward(dO.cuda())
    plain = dict(frefs)["plain"]
    check(f"chained O vs plain {case}", af.to_heads(out), plain.O,
          plain.tol_O)
    refs = _bwd_refs(case, out.detach().cpu(), plain.lse.float(),
                     extra=plain.tol_lse)
    grads = {"dQ": qd.grad.cpu(), "dK": kd.grad.cpu(), "dV": vd.grad.cpu()}
    names = {g: "chained " + n for g, n in _bwd_names(S, -1, -1).items()}
    _check_grads(str(case), case, grads, refs, names)


@pytest.mark.parametrize("S", [192, 256, 384])
def test_dead_rows_contribute_exactly_nothing(S):
    """lse = -inf marks a q row with no visible key.  Every q row of kv
    head 0's group is dead: its dK, dV and those rows' dQ are exactly 0.
    In kv head 1's group single rows are dead: their dQ is exactly 0, and
    dK/dV stay inside the bound of the reference without those rows."""
    case = ("unit", 1, S, 4, 2, True)
    (q, k, v, dO), _, _ = _fwd_case(case)
    O, lse = _given(case)
    O, lse = O.clone(), lse.clone()
    dead = torch.zeros(1, 4, S, dtype=torch.bool)
    dead[:, :2] = True
    dead[:, 2, ::7] = True
    dead[:, 3, S - 33:] = True
    lse[dead] = float("-inf")
    O[dead.permute(0, 2, 1)] = 0
    refs = _bwd_refs(case, O, lse)
    dev = _cuda(q, k, v, O, dO, lse)
    for dkv, dq in _variants(S):
        dQ, dK, dV = (g.cpu() for g in ops.native().attn_bwd(
            *dev, SCALE, True, dkv_variant=dkv, dq_variant=dq))
        tag = f"S={S} dkv={dkv} dq={dq}"
        for name, g in (("dQ", dQ), ("dK", dK), ("dV", dV)):
            assert torch.isfinite(g.float()).all(), f"{name} {tag}"
        assert (af.to_heads(dQ)[dead] == 0).all(), f"dQ of dead rows {tag}"
        assert (dK[:, :, 0] == 0).all() and (dV[:, :, 0] == 0).all(), \
            f"dK/dV of the dead group {tag}"
        _check_grads(f"dead rows {tag}", case,
                     {"dQ": dQ, "dK": dK, "dV": dV}, refs,
                     _bwd_names(S, dkv, dq))


# ---------------------------------------------------------------------------
# Rounding bias.  P rounded to nearest before the MFMA errs symmetrically:
# with every row of V equal, O = (sum_l bf16(p_l)) v / (sum_l p_l) returns v
# up to the last rounding, and the mean signed relative error over the
# tensor vanishes (the CPU emulation gives exactly 0).  A truncated P loses
# half a bf16 ulp of every weight on average: a mean of about -2^-8.7 (the
# emulation: -2.1e-3 to -2.4e-3).  2^-11 lies a factor 5 below that.
# ---------------------------------------------------------------------------
BIAS = 2.0 ** -11


def _ulp_bf16(x):
    return torch.exp2(torch.floor(torch.log2(x.abs())) - 7)


def _mean_signed(got, ref):
    nz = ref != 0
    return float(((got - ref)[nz] / ref[nz]).mean())


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "const_v"],
                         ids=str)
def test_rounding_bias_forward(case):
    (q, k, v, _), kern, _ = _fwd_case(case)
    O = af.to_heads(_fwd_run(case)[0])
    want = af._expand(af._heads(v), case[3])
    bias = _mean_signed(O, want)
    off = (O - want).abs() / _ulp_bf16(want)
    print(f"[bias] {kern} O {case}: mean signed rel err {bias:.3g}, "
          f"{float((off > 0).double().mean()):.1%} of elements off v, "
          f"worst {float(off.max()):.3g} ulp")
    assert float(off.max()) <= 1.0, "an O element is beyond one ulp of v"
    assert abs(bias) <= BIAS, f"mean signed relative error {bias:.3g}"


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "const_dO"],
                         ids=str)
def test_rounding_bias_dkv(case):
    """dV = sum p^T dO with every row of dO equal: dV_ld = dO_d * sum_i
    p_il, held against the declared-operand fp64 reference (whose scores
    the kernel's agree with to fp32 accuracy).  Unlike O with constant V,
    dV does not equal a bf16 input (sum_i p_il is not 1), so there is no
    one-ulp test against an exact value here: every element is held to the
    general bound and the tensor to the mean signed relative error."""
    S, causal = case[2], case[5]
    (q, k, v, dO), _, _ = _fwd_case(case)
    O, lse, refs = _bwd_case(case)
    ref = next(r for _, r, judged in refs if "dV" in judged)
    dev = _cuda(q, k, v, O, dO, lse)
    for dkv, dq in _variants(S):
        dV = af.to_heads(ops.native().attn_bwd(
            *dev, SCALE, causal, dkv_variant=dkv, dq_variant=dq)[2])
        bias = _mean_signed(dV, ref.dV)
        kern = _bwd_names(S, dkv, dq)["dV"]
        print(f"[bias] {kern} dV {case}: mean signed rel err {bias:.3g}")
        assert within(dV, ref.dV, ref.tol_dV)[0]
        assert abs(bias) <= BIAS, \
            f"{kern}: mean signed relative error {bias:.3g}"
