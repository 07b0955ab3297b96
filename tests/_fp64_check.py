"""The elementwise fp64 checker shared by test_gpu_train_kernels.py and
test_gpu_decode_kernels.py (docs/TESTING.md, "Tolerance rule").

A kernel result is compared element by element with an fp64 evaluation of
the same formula on the same (bf16-rounded) inputs.  The bound is built
from what the kernel legitimately loses:

* a bf16 output (unit roundoff 2^-8) may be off by ``2 * 2^-8 * |ref|``
  per rounding it goes through;
* fp32 arithmetic may be off by ``4 * K * 2^-24 * A``: K is the number of
  terms reduced into the element (1 for pointwise ops), A the same formula
  evaluated with the absolute values of its terms (so cancellation is
  charged to the terms, not to the small result), and 4 covers FMA
  contraction and the few-ulp ``__expf``/``__logf``/``rsqrtf``;
* ``1e-30`` absolute lets values flushed to zero compare equal.

Every element has to be inside the bound; none is excluded.  Each check
prints the largest error it saw as a fraction of the bound (``pytest -s``).
"""
import torch

U16 = 2.0 ** -8    # bf16 unit roundoff
U32 = 2.0 ** -24   # fp32 unit roundoff
TINY = 1e-30


def f32(v):
    """A Python float as the kernel receives it: rounded to fp32."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def tol_bf16(ref, A, K=1, roundings=1):
    return roundings * 2 * U16 * ref.abs() + 4 * K * U32 * A + TINY


def tol_f32(A, K=1):
    return 4 * K * U32 * A + TINY


def within(got, ref, tol):
    """(ok, worst err/tol, flat index of the worst element)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ratio = (got - ref).abs() / tol
    ratio = torch.where(torch.isfinite(ratio), ratio,
                        torch.full_like(ratio, float("inf")))
    if ratio.numel() == 0:
        return True, 0.0, -1
    worst = int(ratio.argmax())
    r = float(ratio.reshape(-1)[worst])
    return r <= 1.0, r, worst


def check(name, got, ref, tol):
    ok, r, worst = within(got, ref, tol)
    print(f"[fp64] {name}: worst err/tol = {r:.3g}")
    if not ok:
        g = got.detach().cpu().double().reshape(-1)
        bad = int(((g - ref.reshape(-1)).abs() > tol.reshape(-1)).sum()
                  + (~torch.isfinite(g)).sum())
        idx, rest = [], worst
        for n in reversed(ref.shape):
            rest, i = divmod(rest, n)
            idx.insert(0, i)
        idx = tuple(idx)
        raise AssertionError(
            f"{name}: {bad} of {g.numel()} elements out of tolerance; worst "
            f"at {idx}: got {g[worst].item()!r}, ref "
            f"{ref.reshape(-1)[worst].item()!r}, tol "
            f"{tol.reshape(-1)[worst].item():.3g} (err/tol {r:.3g})")
    return r


def rejects(got, ref, tol):
    ok, _, _ = within(got, ref, tol)
    return not ok


def bf16_values(t):
    """Round to bf16 and return as fp32 (what a bf16 kernel input holds)."""
    return t.bfloat16().float()
