"""CPU tests of tests/_attn_fp64.py: the fp64 attention references are
pinned to ops.attention_ref + autograd, the fp32/bf16 emulations of both
forward kernels stay inside the derived bound on every input family, and
the checker rejects planted defects.  No GPU.

For each defect the test also prints whether the former
``assert_close(atol=rtol=0.05 / 0.08)`` check would have accepted it;
no assertion rests on that."""
import functools

import pytest
import torch

import _attn_fp64 as af
from _fp64_check import check, f32, rejects, within
from skypilot_amd import ops

SCALE = af.SCALE
SC = f32(SCALE)   # the scale as the kernels receive it


def _old_accepts(got, ref, tol):
    return bool(((got - ref).abs() <= tol + tol * ref.abs()).all())


# ---------------------------------------------------------------------------
# The reference is the definition: ops.attention_ref + autograd + logsumexp.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_reference_matches_attention_ref_and_autograd(causal):
    B, S, Hq, Hkv = 2, 128, 4, 2
    q, k, v, dO = af.make_inputs("unit", B, S, Hq, Hkv)
    r = af.fwd_ref(q, k, v, SCALE, causal)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    out = ops.attention_ref(qd, kd, vd, SCALE, causal=causal)
    # attention_ref computes in fp32: agreement at fp32 accuracy
    torch.testing.assert_close(r.O, af.to_heads(out), atol=2e-6, rtol=2e-5)
    rep = Hq // Hkv
    att = torch.einsum("bihd,bjhd->bhij", q.double(),
                       k.double().repeat_interleave(rep, dim=2)) * SC
    if causal:
        att = att.masked_fill(af._mask(S), float("-inf"))
    torch.testing.assert_close(r.lse, torch.logsumexp(att, -1),
                               atol=1e-12, rtol=1e-12)

    # backward from the exact O / lse (kept in fp64: no bf16/fp32 rounding
    # of the given inputs) against autograd of the fp64 softmax
    qe, ke, ve = (t.double().requires_grad_() for t in (q, k, v))
    s = torch.einsum("bihd,bjhd->bhij", qe,
                     ke.repeat_interleave(rep, dim=2)) * SC
    if causal:
        s = s.masked_fill(af._mask(S), float("-inf"))
    o = torch.einsum("bhij,bjhd->bihd", s.softmax(-1),
                     ve.repeat_interleave(rep, dim=2))
    gq, gk, gv = torch.autograd.grad(o, (qe, ke, ve), dO.double())
    b = af.bwd_ref(q, k, v, o.detach(), dO, r.lse, SCALE, causal)
    for name, got, want in (("dQ", b.dQ, gq), ("dK", b.dK, gk),
                            ("dV", b.dV, gv)):
        torch.testing.assert_close(got, af.to_heads(want), atol=1e-10,
                                   rtol=1e-9, msg=lambda m: f"{name}: {m}")
    # and against the fp32 attention_ref's autograd at fp32 accuracy
    gq32, gk32, gv32 = torch.autograd.grad(out, (qd, kd, vd), dO.double())
    for got, want in ((b.dQ, gq32), (b.dK, gk32), (b.dV, gv32)):
        torch.testing.assert_close(got, af.to_heads(want), atol=2e-5,
                                   rtol=2e-4)


def test_declared_operand_is_the_kernels_prescale():
    """bf16(fp32(x) * qs) with qs formed in fp32; the declared reference
    differs from the plain one by less than the plain bound's 2^-8 term
    allows, and is not identical to it."""
    q, k, v, _ = af.make_inputs("unit", 1, 128, 2, 1)
    qs = af.qs_of(SCALE)
    assert qs.dtype == torch.float32
    assert torch.equal(af.reround(q, SCALE), (q.float() * qs).bfloat16())
    plain = af.fwd_ref(q, k, v, SCALE, True, rerounded=True)
    decl = af.fwd_ref(q, k, v, SCALE, True, operand="q")
    assert not torch.equal(plain.O, decl.O)
    assert within(decl.O, plain.O, plain.tol_O)[0]
    assert within(decl.lse, plain.lse, plain.tol_lse)[0]


# ---------------------------------------------------------------------------
# Clean emulations stay inside the bound on every family.
# ---------------------------------------------------------------------------
EMU_SHAPE = (1, 256, 2, 1)


@functools.lru_cache(maxsize=None)
def _family(family, causal, shape=EMU_SHAPE):
    q, k, v, dO = af.make_inputs(family, *shape)
    plain64 = af.fwd_ref(q, k, v, SCALE, causal, r_P=af.R_P)
    plain = af.fwd_ref(q, k, v, SCALE, causal, rerounded=True,
                       r_P=af.R_P)
    decl = af.fwd_ref(q, k, v, SCALE, causal, operand="q",
                      r_P=af.R_P)
    return (q, k, v, dO), plain64, plain, decl


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", af.FAMILIES)
def test_emulations_inside_bound(family, causal):
    (q, k, v, _), plain64, plain, decl = _family(family, causal)
    tag = f"{family} causal={causal}"
    O, lse = af.emu_fwd64(q, k, v, SCALE, causal)
    check(f"emu fwd64 O   plain    {tag}", O, plain64.O, plain64.tol_O)
    check(f"emu fwd64 lse plain    {tag}", lse, plain64.lse, plain64.tol_lse)
    O, lse = af.emu_fwd_v3(q, k, v, SCALE, causal)
    for name, r in (("plain", plain), ("declared", decl)):
        check(f"emu fwd_v3 O   {name:8s} {tag}", O, r.O, r.tol_O)
        check(f"emu fwd_v3 lse {name:8s} {tag}", lse, r.lse, r.tol_lse)


def test_equal_family_is_the_running_mean():
    (q, k, v, _), plain64, _, decl = _family("equal", True)
    S = q.shape[1]
    want = torch.arange(1, S + 1).double().log()
    for r in (plain64, decl):
        assert (r.lse - want).abs().max() < 1e-14
        mean = af._expand(af._heads(v), q.shape[2]).cumsum(2) / \
            torch.arange(1, S + 1).double().view(1, 1, S, 1)
        assert (r.O - mean).abs().max() < 1e-13


def test_truncated_p_is_biased_and_rounded_p_is_not():
    """The rounding-bias test of the GPU suite, on the emulation: with all
    rows of V equal, a truncated P pulls O below v (mean signed relative
    error near -2^-8.7), a P rounded to nearest does not."""
    q, k, v, _ = af.make_inputs("const_v", 1, 192, 1, 1)
    want = af.to_heads(v)
    for trunc in (True, False):
        O, _ = af.emu_fwd64(q, k, v, SCALE, True, trunc=trunc)
        bias = ((O - want) / want).mean().item()
        print(f"[bias] emu fwd64 trunc={trunc}: mean signed rel err "
              f"{bias:.3g}")
        assert (abs(bias) > 2.0 ** -11) == trunc


# ---------------------------------------------------------------------------
# Planted defects.
# ---------------------------------------------------------------------------
def _report(name, got, ref, tol, old_tol, must=True):
    ok, worst, _ = within(got, ref, tol)
    outside = float(((got - ref).abs() > tol).double().mean())
    print(f"[defect] {name}: worst err/tol {worst:.3g}, {outside:.1%} of "
          f"elements outside; old atol=rtol={old_tol} check "
          f"{'ACCEPTS' if _old_accepts(got, ref, old_tol) else 'rejects'} it")
    assert not (ok and must), f"{name} not rejected"


FWD_DEFECTS = [
    ("no_l_rescale", "rising", True),
    ("diag_plus", "flat", True),
    ("diag_minus", "flat", True),
    ("skip_last_row", "flat", False),
    ("skip_last_row", "rising", True),
    ("drop_last_tile", "flat", False),
    ("drop_last_tile", "unit", True),
]


@pytest.mark.parametrize("defect,family,causal", FWD_DEFECTS)
def test_forward_defect_rejected(defect, family, causal):
    (q, k, v, _), _, plain, decl = _family(family, causal)
    O, lse = af.emu_fwd_v3(q, k, v, SCALE, causal, defect=defect)
    clean, _ = af.emu_fwd_v3(q, k, v, SCALE, causal)
    assert within(clean, decl.O, decl.tol_O)[0]
    # Both bounds must reject, with one exception: a skipped kv row S-1
    # under the causal mask changes the last q row only, and there needs a
    # family that puts weight on that row.  On the rising family the scores
    # reach 48 nats, so the plain bound's 2^-8 * sum|q k| * scale term is
    # about 0.4 nat: it cannot tell a weight of 1 from one of 0.6, and the
    # plain check is reported only (the declared-operand bound rejects).
    _report(f"{defect} ({family}, causal={causal}) O vs declared", O, decl.O,
            decl.tol_O, 0.05)
    _report(f"{defect} ({family}, causal={causal}) O vs plain", O, plain.O,
            plain.tol_O, 0.05,
            must=(defect, family, causal) != ("skip_last_row", "rising", True))


def test_no_l_rescale_is_invisible_on_flat_inputs():
    """Why the rising family exists: on randn * 0.5 inputs the deferred
    rescale never runs after tile 0 and the defect changes nothing."""
    (q, k, v, _), _, _, decl = _family("flat", True)
    O, _ = af.emu_fwd_v3(q, k, v, SCALE, True, defect="no_l_rescale")
    clean, _ = af.emu_fwd_v3(q, k, v, SCALE, True)
    assert torch.equal(O, clean)


def test_lse_in_log2_units_rejected():
    (q, k, v, _), plain64, plain, decl = _family("unit", True)
    for name, r in (("plain64", plain64), ("plain", plain),
                    ("declared", decl)):
        assert rejects(r.lse * af.LOG2E, r.lse, r.tol_lse), name
    print("[defect] lse_log2 (forward output): rejected; the old check "
          "never compared lse")


BWD_SHAPE = (2, 128, 4, 2)
BWD_DEFECTS = ["lse_log2", "no_dvec", "dk_no_scale", "dq_scale_twice",
               "first_head_only", "kvh_mod", "batch0_k"]
# which gradients each defect must move
BWD_HITS = {"lse_log2": ("dQ", "dK", "dV"), "no_dvec": ("dQ", "dK"),
            "dk_no_scale": ("dK",), "dq_scale_twice": ("dQ",),
            "first_head_only": ("dK", "dV"), "kvh_mod": ("dQ", "dK", "dV"),
            "batch0_k": ("dQ", "dK", "dV")}


@functools.lru_cache(maxsize=None)
def _bwd_case(causal):
    q, k, v, dO = af.make_inputs("unit", *BWD_SHAPE)
    f = af.fwd_ref(q, k, v, SCALE, causal)
    O = af._bf(f.O).permute(0, 2, 1, 3).bfloat16()
    lse = f.lse.float()
    args = (q, k, v, O, dO, lse)
    refs = {"declared64": af.bwd_ref(*args, SCALE, causal,
                                     r_P=af.R_P),
            "plain": af.bwd_ref(*args, SCALE, causal, rerounded=True),
            "declared_q": af.bwd_ref(*args, SCALE, causal, operand="q"),
            "declared_k": af.bwd_ref(*args, SCALE, causal, operand="k")}
    return args, refs


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("defect", BWD_DEFECTS)
def test_backward_defect_rejected(defect, causal):
    args, refs = _bwd_case(causal)
    bad = af.bwd_ref(*args, SCALE, causal, defect=defect)
    for gname in BWD_HITS[defect]:
        got = af._bf(getattr(bad, gname)).double()
        for rname, r in refs.items():
            if (rname, gname) in (("declared_q", "dK"), ("declared_q", "dV"),
                                  ("declared_k", "dQ")):
                continue   # each declared reference checks its own kernel
            _report(f"{defect} (causal={causal}) {gname} vs {rname}", got,
                    getattr(r, gname), getattr(r, "tol_" + gname), 0.08)


@pytest.mark.parametrize("causal", [True, False])
def test_backward_references_agree_within_bounds(causal):
    """The bf16-rounded plain gradients pass every bound (the checker does
    not reject a correct result), and the declared references sit inside
    the plain bound."""
    _, refs = _bwd_case(causal)
    plain = refs["plain"]
    for gname in ("dQ", "dK", "dV"):
        got = af._bf(getattr(refs["declared64"], gname)).double()
        check(f"bf16(plain {gname}) vs declared64 causal={causal}", got,
              getattr(refs["declared64"], gname),
              getattr(refs["declared64"], "tol_" + gname))
    check("declared_q dQ vs plain", refs["declared_q"].dQ, plain.dQ,
          plain.tol_dQ)
    check("declared_k dK vs plain", refs["declared_k"].dK, plain.dK,
          plain.tol_dK)
    check("declared_k dV vs plain", refs["declared_k"].dV, plain.dV,
          plain.tol_dV)


def test_dead_rows_contribute_nothing_in_the_reference():
    (q, k, v, O, dO, lse), _ = _bwd_case(True)
    lse = lse.clone()
    lse[:, :2] = float("-inf")        # both q heads of kv head 0
    r = af.bwd_ref(q, k, v, O, dO, lse, SCALE, True)
    assert torch.isfinite(r.dQ).all() and torch.isfinite(r.tol_dQ).all()
    assert (r.dQ[:, :2] == 0).all() and (r.dK[:, 0] == 0).all() \
        and (r.dV[:, 0] == 0).all()
    assert (r.dK[:, 1] != 0).any()
