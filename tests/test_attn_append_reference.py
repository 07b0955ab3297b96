"""CPU tests of tests/_attn_append_fp64.py: the fp64 reference of chunked
prefill is pinned to ops.attn_append_ref and to _attn_fp64.fwd_ref, the
emulation of attn_append_kernel's rounding scheme stays inside the derived
bound on every case of the GPU file, and the checker rejects planted
defects.  No GPU.

For each defect the test prints (``pytest -s``) whether the checks of
test_attn_append_gpu.py (``rel_err < 2e-2`` plus ``assert_close(atol =
rtol = 0.05)`` per sequence) would have accepted it."""
import functools

import pytest
import torch

import _attn_append_fp64 as aa
import _attn_fp64 as af
from _fp64_check import within
from skypilot_amd import ops

SCALE = aa.SCALE


# ---------------------------------------------------------------------------
# The reference is the definition.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(aa.GEOMS))
def test_reference_matches_attn_append_ref(geom):
    """ops.attn_append_ref evaluates the same definition in fp32.  Given
    the inputs as fp32 it rounds nothing to bf16, so it is held to the
    bound without its bf16 terms (tol_f32: accumulation over the row's
    terms and the softmax's response to fp32 scores)."""
    case = next(c for c in aa.CASES if c[0] == geom and c[1] == "unit")
    c = aa.build_case(case)
    got = ops.attn_append_ref(c.q.float(), c.kc.float(), c.vc.float(),
                              c.slot_ids, c.starts, c.lens, SCALE)
    assert got.dtype == torch.float32
    assert torch.count_nonzero(got[torch.tensor(c.lens) == 0]) == 0
    worst = 0.0
    for b, r in enumerate(aa.case_refs(case)):
        if r is None:
            continue
        ok, ratio, _ = within(aa.seq_rows(got, b, c.lens[b]), r.O, r.tol_f32)
        worst = max(worst, ratio)
        assert ok, (case, b, ratio)
    print(f"[fp64] attn_append_ref vs fp64 {case}: worst err/tol "
          f"{worst:.3g}")


@pytest.mark.parametrize("family", ["unit", "rising"])
def test_reference_is_fwd_ref_at_start_zero(family):
    """q_start = 0, q_len = L: causal attention, reference and bound."""
    L, Hq, Hkv = 128, 4, 2
    q, k, v, _ = af.make_inputs(family, 1, L, Hq, Hkv)
    nan = float("nan")
    kc = torch.full((3, 150, Hkv, aa.D), nan, dtype=torch.bfloat16)
    vc = torch.full((3, 150, Hkv, aa.D), nan, dtype=torch.bfloat16)
    kc[1, :L], vc[1, :L] = k[0], v[0]
    r = aa.ref_seq(q[0], kc, vc, 1, 0, L, SCALE)
    want = af.fwd_ref(q, k, v, SCALE, True)
    torch.testing.assert_close(r.O, want.O[0], atol=1e-14, rtol=1e-13)
    torch.testing.assert_close(r.tol_O, want.tol_O[0], atol=1e-16,
                               rtol=1e-12)


def test_reference_positions_and_truncation():
    """Independent of ref_seq's masking code: each valid row, on its own,
    is a softmax over an explicit list of visible rows."""
    case = next(c for c in aa.CASES if c[0] == "A" and c[1] == "flat")
    c = aa.build_case(case)
    refs = aa.case_refs(case)
    sc = torch.tensor(SCALE, dtype=torch.float32).double()
    group = c.Hq // c.Hkv
    for b, (start, ln) in enumerate(zip(c.starts, c.lens)):
        for i in {0, ln // 2, ln - 1} if ln else ():
            vis = [kv for kv in range(c.S_max)
                   if kv <= start + i and kv < start + ln]
            for h in (0, c.Hq - 1):
                K = c.kc[c.slot_ids[b], vis, h // group].double()
                V = c.vc[c.slot_ids[b], vis, h // group].double()
                p = ((K @ c.q[b, i, h].double()) * sc).softmax(0)
                assert (refs[b].O[h, i] - p @ V).abs().max() < 1e-13


# ---------------------------------------------------------------------------
# The clean emulation is inside the bound on every case of the GPU file.
# ---------------------------------------------------------------------------
def _worst(case, got):
    """(worst err/tol over the valid rows, the sequence that has it)."""
    c = aa.build_case(case)
    worst, where = 0.0, None
    for b, r in enumerate(aa.case_refs(case)):
        if r is None:
            continue
        _, ratio, _ = within(aa.seq_rows(got, b, c.lens[b]), r.O, r.tol_O)
        if ratio > worst:
            worst, where = ratio, b
    return worst, where


@functools.lru_cache(maxsize=None)
def _clean(case):
    return aa.emu_case(case)


_emu_worst = {}


@pytest.mark.parametrize("case", aa.CASES, ids=str)
def test_emulation_inside_bound(case):
    c = aa.build_case(case)
    got = _clean(case)
    worst, b = _worst(case, got)
    _emu_worst[case] = worst
    print(f"[fp64] emu attn_append {case}: worst err/tol {worst:.3g} in "
          f"sequence {(c.starts[b], c.lens[b])}; over the cases so far "
          f"{max(_emu_worst.values()):.3g}")
    assert worst <= 1.0
    assert torch.isfinite(got).all()
    for b, ln in enumerate(c.lens):     # padding-only tiles
        first = -(-ln // aa.BM) * aa.BM
        assert torch.count_nonzero(got[b, first:]) == 0


# ---------------------------------------------------------------------------
# Planted defects.
# ---------------------------------------------------------------------------
def _old_accepts(out, ref):
    """test_attn_append_gpu._check_valid for one sequence: out and ref are
    its valid rows, ref rounded to bf16 as attn_append_ref returns it."""
    ref = ref.bfloat16().double()
    err = ((out - ref).norm() / (ref.norm() + 1e-12)).item()
    return err < 2e-2 and \
        bool(((out - ref).abs() <= 0.05 + 0.05 * ref.abs()).all())


# One row, or the rows of one wave, wrong.
FEW_ROWS = ("mask_from_wave_last", "need_mask_off_by_one", "skip_last_row")


@pytest.mark.parametrize("defect", [d for d in aa.DEFECTS if d != "p_trunc"])
def test_defect_rejected(defect):
    """The fp64 check rejects the defect on at least one sequence of the
    GPU case list.  The line printed names the first such case and
    sequence, in how many sequences the defect changes a valid row, how
    many of those the fp64 check rejects, and how many of the rejected
    ones the former check accepts."""
    changed, rejected, old_ok = 0, [], []
    for case in aa.CASES:
        c = aa.build_case(case)
        got, clean = aa.emu_case(case, defect=defect), _clean(case)
        for b, r in enumerate(aa.case_refs(case)):
            if r is None or torch.equal(got[b, :c.lens[b]],
                                        clean[b, :c.lens[b]]):
                continue
            changed += 1
            out = aa.seq_rows(got, b, c.lens[b])
            ok, ratio, _ = within(out, r.O, r.tol_O)
            if not ok:
                where = (case, (c.starts[b], c.lens[b]), ratio)
                rejected.append(where)
                if _old_accepts(out, r.O):
                    old_ok.append(where)
    print(f"[defect] {defect}: changes {changed} sequences, fp64 check "
          f"rejects {len(rejected)}"
          + (f", first {rejected[0][0]} sequence {rejected[0][1]} err/tol "
             f"{rejected[0][2]:.3g}" if rejected else "")
          + f"; old check ACCEPTS {len(old_ok)} of the rejected"
          + (f", e.g. {old_ok[0][0]} sequence {old_ok[0][1]} err/tol "
             f"{old_ok[0][2]:.3g}" if old_ok else ""))
    assert rejected, f"{defect}: no case of the GPU list rejects it"
    if defect in FEW_ROWS:
        assert old_ok, f"{defect}: the old check rejects it wherever the " \
            "new one does"


def test_truncated_p_is_caught_by_the_bias_test():
    """P truncation moves every element by less than the bound allows
    (r_P would be 2); the rounding-bias test of the GPU file catches it:
    const_v on geometry C, |mean signed relative error| <= 2^-11."""
    case = next(c for c in aa.CASES if c[0] == "C" and c[1] == "const_v")
    for defect in (None, "p_trunc"):
        got = aa.emu_case(case, defect=defect)
        bias, _ = aa.const_v_bias(aa.build_case(case), got)
        worst, _ = _worst(case, got)
        print(f"[bias] emu attn_append {case} defect={defect}: mean signed "
              f"rel err {bias:.3g}, worst err/tol {worst:.3g}")
        assert (abs(bias) > 2.0 ** -11) == (defect == "p_trunc")


def test_moved_diagonal_is_invisible_with_constant_v():
    """Why the families are combined: with every row of V equal, O = v
    whatever the weights are."""
    for case in (c for c in aa.CASES if c[1] == "const_v"):
        for defect in ("diag_plus", "diag_no_start"):
            worst, _ = _worst(case, aa.emu_case(case, defect=defect))
            print(f"[defect] {defect} on {case}: worst err/tol {worst:.3g}")
            assert worst <= 1.0
