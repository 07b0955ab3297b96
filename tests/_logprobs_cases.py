"""Tolerance, inputs and comparison shared by test_logprobs_reference.py
and test_logprobs_gpu.py (docs/KERNELS.md "Token log-probabilities").

Tolerance of one log-probability against the fp64 reference:

    tol(lp_ref, V) = 2^-22 + V*2^-40 + 2^-22*log2(max(V, 2))
                     + 2^-23*|lp_ref|

* ``2^-22``: one ulp of ``v_exp_f32``, as a relative error of Z.
* ``V*2^-40``: the fixed-point truncation of the V weights, against a
  total of at least 1.
* ``2^-22*log2(V)``: the fp32 roundings of ``(l - m)`` and of the product
  with ``log2e``, each a relative 2^-24 of an exponent of magnitude
  ``log2(1/p_j)``, weighted by each element's share ``p_j`` of Z: at most
  the entropy in bits, which is at most ``log2(V)``.
* ``2^-23*|lp|``: the final fp32 rounding of the result, with a factor 2.

An fp32 emulation of the definition on the CPU (``torch.exp2`` in fp32,
not the GPU instruction), compared with fp64 ``logsumexp`` for V from 1
to 152,064, scales 0.01 to 64 and offsets 0, 30 and -200, stayed within
0.46 of this bound; its ``lse`` error was at most 6e-8.

Non-finite values (-inf for a -inf logit, NaN for unused entries,
degenerate rows and ids outside the row) have to match exactly.
"""
import math

import torch

import _fp64_check as fc
from skypilot_amd import ops

TOP = 20


def tol(lp_ref, V):
    lp_ref = torch.as_tensor(lp_ref, dtype=torch.float64)
    return (2.0 ** -22 + V * 2.0 ** -40
            + 2.0 ** -22 * math.log2(max(V, 2))
            + 2.0 ** -23 * lp_ref.abs())


def make_rows(n, V, scale, seed):
    """bf16 normal rows."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, V, generator=g) * scale).bfloat16()


def make_ids(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (n,), generator=g)


def same_nonfinite(got, ref):
    """NaN and +-inf entries are the same entries."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return (torch.equal(torch.isnan(got), torch.isnan(ref))
            and torch.equal(got == math.inf, ref == math.inf)
            and torch.equal(got == -math.inf, ref == -math.inf))


def check_lp(name, got, ref, V):
    """Every finite reference value within tol, every other one equal.
    Returns the worst err/tol."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert same_nonfinite(got, ref), (name, got, ref)
    fin = torch.isfinite(ref)
    if not bool(fin.any()):
        return 0.0
    return fc.check(name, got[fin], ref[fin], tol(ref[fin], V))


def check_result(name, got, ref, V):
    """(lp, top_lp, top_ids) of the op against the reference's: values
    within tol, ids equal.  Returns the worst err/tol."""
    lp, top_lp, top_ids = got
    rlp, rtop_lp, rtop_ids = ref
    bad = (top_ids.cpu() != rtop_ids).nonzero().tolist()
    assert not bad, (name, bad[:5], top_ids.cpu()[bad[0][0]].tolist(),
                     rtop_ids[bad[0][0]].tolist())
    return max(check_lp(name + " lp", lp, rlp, V),
               check_lp(name + " top_lp", top_lp, rtop_lp, V))


def plain_reference(logits, ids):
    """fp64 log_softmax gathered at ids: the definition without the
    fixed-point sum."""
    ls = torch.log_softmax(logits.double(), dim=-1)
    return ls.gather(1, torch.as_tensor(ids).reshape(-1, 1)).reshape(-1)


def broken_references(logits, ids):
    """Two wrong chosen-token references for the negative control: the
    largest element left out of Z, and lse off by 1e-4."""
    l = logits.double()
    amax = l.argmax(dim=-1, keepdim=True)
    lse_less = torch.logsumexp(
        l.scatter(1, amax, float("-inf")), dim=-1)
    picked = l.gather(1, torch.as_tensor(ids).reshape(-1, 1)).reshape(-1)
    return picked - lse_less, plain_reference(logits, ids) - 1e-4


def tie_block_row(V, seed=5):
    """Three values above a block of 40 equal values above everything
    else.  The ties sit in the segments of waves 0, 5 and 15 of a
    16-wave block (a wave owns ceil(V/16) rounded up to 2048 elements),
    the last of which is cut short by V and ends in the row's last
    element.  Returns (row bf16 [V], the three top ids in order, the tie
    ids ascending)."""
    seg = (-(-V // 16) + 2047) // 2048 * 2048
    assert 15 * seg < V < 16 * seg
    g = torch.Generator().manual_seed(seed)
    row = (torch.randn(V, generator=g) * 0.25 - 4.0).bfloat16()
    top3 = [seg + 7, V - 2, 3]
    for v, j in zip((5.0, 4.0, 3.0), top3):
        row[j] = v
    last = 15 * seg
    ties = ([1, 9, 64, 511]
            + [5 * seg + j for j in (0, 8, 513, seg - 1)]
            + [last + j for j in range(0, 8 * 27, 8)]
            + [V - 9, V - 8, V - 7, V - 3, V - 1])
    assert len(ties) == 40 and sorted(set(ties)) == ties
    assert not set(ties) & set(top3)
    row[ties] = 2.0
    return row, top3, ties


def ref(logits, ids, n_top):
    return ops.token_logprobs_reference(logits, ids, n_top)
