"""fp64 references, derived bounds, input families and CPU emulations for
the training attention kernels (attention_fwd.hip, attention_fwd_v3.hip,
attention_bwd.hip, attention_bwd_v3.hip).  Used by
test_attn_train_reference.py (CPU) and test_attn_train_gpu.py (GPU).

Reference
---------
Plain torch fp64 per (batch, q-head) on the bf16-rounded inputs, written
from the definition; GQA maps q-head ``qh`` to kv-head ``qh // (Hq//Hkv)``.

    s = scale * q k^T          (causal: l > i masked)
    lse_i = logsumexp_l s_il   p = exp(s - lse)      O = p v

The backward is the formula the kernels implement.  ``O``, ``lse`` and
``dO`` are *given inputs* and ``p = exp(s - lse)`` is not renormalised:

    Dvec_i = sum_d dO_id O_id      dP = dO v^T      dS = p * (dP - Dvec)
    dV = sum_group p^T dO   dK = scale * sum_group dS^T q   dQ = scale * dS k

Two references per v3 kernel
----------------------------
The v3 kernels multiply one operand of the S pass by
``qs = fp32(scale) * fp32(log2 e)`` and round the product back to bf16:
``Q`` in attn_fwd_v3 and in both dq kernels, ``K`` in both dkv kernels.
The re-rounded operand feeds the S pass only; ``dS^T q`` and ``dS k`` use
the original operands.  ``operand=None`` is the *plain* reference above;
``operand="q"`` / ``"k"`` is the *declared-operand* reference: the same
fp64 formula with that operand replaced by ``bf16(fp32(x) * qs)`` and the
scores taken in log2 units (``s = ln2 * q' k^T``).  The 64-tile kernels
re-round nothing: the plain reference is their declared one.

Bound
-----
Built from ``tol_bf16`` / ``tol_f32`` (``_fp64_check.py``: ``2 * 2^-8 *
|ref|`` per bf16 output rounding, ``4 * K * 2^-24 * A`` for K fp32 terms
with A the formula over absolute values) plus what a softmax adds:

* Score error ``d_il``, the sum of
    ``4 * 128 * 2^-24 * sum_d |q_d k_d| * scale``   fp32 dot product,
    ``4 * 2^-24 * |s_il - m_i|``                    exp argument,
    ``4 * 2^-24 * |lse_i| * log2 e``                backward only (lse is
                                                    converted and subtracted),
    ``2^-8 * sum_d |q_d k_d| * scale``              against the plain
        reference of a kernel that re-rounds an operand: each product
        q_d k_d moves by at most one bf16 unit roundoff.
  A perturbed weight is ``p_l * exp(d_l)``.
* Forward: the normalised weights move, to first order, a weighted sum
  ``sum_l p_l t_l`` by at most ``sum_l p_l d_l |t_l| + (sum_l p_l d_l) * A``
  (numerator and normaliser), ``A = sum_l p_l |t_l|``; the factor
  ``exp(2 * max_l d_l)`` covers the higher orders, since every ratio of
  perturbed to exact normalised weights lies in ``exp(+-2 max d)``.
* Backward: ``p`` is not renormalised, so the error of ``p`` is
  ``ep = p * (exp(d) - 1)`` exactly and no normaliser term appears.
* ``P`` is rounded to bf16 before the PV / P^T dO MFMA: ``r_P * 2^-8 * A``
  with ``r_P = 1`` for round-to-nearest and 2 for truncation (``R_P``
  below).  ``dS`` is rounded to nearest: ``2^-8 * sum |dS * term|``.
* ``dS = p (dP - Dvec)`` inherits ``ep * |dP - Dvec|`` plus
  ``(p + ep) * (e_dP + e_Dvec)`` with the fp32 dot-product errors
  ``e_dP = 4 * 128 * 2^-24 * sum_d |dO v|``, ``e_Dvec = 4 * 128 * 2^-24 *
  sum_d |dO O|``.
* Accumulation ``4 * (n + 4) * 2^-24 * A`` over the n terms reduced, and
  the output rounding ``2 * 2^-8 * |ref|``.
* ``lse`` (fp32): ``sum_l p_l d_l + 4 * (L + 4) * 2^-24 + 4 * 2^-24 *
  (|m| + |ln l|)`` (weights, the sum, and the final ``m + ln l``).

Every element is held to the bound; none is excluded.  The bound is never
tuned to what a kernel returns.

Input families (``make_inputs``) are built in fp64 and rounded to bf16,
deterministic per (family, shape).
"""
import math
import types
import zlib

import torch

from _fp64_check import U16, U32, tol_bf16, tol_f32

D = 128
SCALE = D ** -0.5
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)

# P rounding before the PV / P^T dO MFMA: every kernel rounds to nearest
# (cvt_pk in the v3 kernels, f2bf in the 64-tile kernels), r_P = 1.
R_P = 1

FAMILIES = ("flat", "unit", "rising", "creeping", "falling", "peaked",
            "equal", "const_v", "const_dO")


def qs_of(scale):
    """fp32(scale) * fp32(log2 e) in fp32, as the v3 kernels form it."""
    return torch.tensor(scale, dtype=torch.float32) * \
        torch.tensor(1.44269504088896340736, dtype=torch.float32)


def reround(x, scale):
    """bf16(fp32(x) * qs): the declared S-pass operand of a v3 kernel."""
    return (x.float() * qs_of(scale)).bfloat16()


def _heads(x):
    """[B,S,H,D] -> fp64 [B,H,S,D]."""
    return x.double().permute(0, 2, 1, 3)


def _expand(kv, Hq, kv_of=None):
    """fp64 [B,Hkv,S,D] -> [B,Hq,S,D] with kvh = qh // group."""
    Hkv = kv.shape[1]
    idx = torch.arange(Hq) // (Hq // Hkv)
    if kv_of is not None:
        idx = torch.tensor([kv_of(h) for h in range(Hq)])
    return kv[:, idx]


def _group_sum(x, Hkv, first_only=False):
    """[B,Hq,S,D] -> [B,Hkv,S,D], summing each GQA group."""
    B, Hq, S, Dd = x.shape
    x = x.reshape(B, Hkv, Hq // Hkv, S, Dd)
    return x[:, :, 0] if first_only else x.sum(2)


def _mask(S):
    return torch.triu(torch.ones(S, S, dtype=torch.bool), 1)


def _scores(q, k, scale, causal, operand, kv_of=None, batch_of=None):
    """Natural-unit scores [B,Hq,S,S] (masked: -inf) and sum_d|q_d k_d|
    times the same multiplier."""
    Hq = q.shape[2]
    if operand == "q":
        q, mul = reround(q, scale), LN2
    elif operand == "k":
        k, mul = reround(k, scale), LN2
    else:
        assert operand is None
        mul = torch.tensor(scale, dtype=torch.float32).double().item()
    Q, K = _heads(q), _expand(_heads(k), Hq, kv_of)
    if batch_of is not None:
        K = K[[batch_of(b) for b in range(K.shape[0])]]
    s = (Q @ K.transpose(-1, -2)) * mul
    absqk = (Q.abs() @ K.abs().transpose(-1, -2)) * mul
    if causal:
        s = s.masked_fill(_mask(s.shape[-1]), float("-inf"))
    return s, absqk


def _finite(x):
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x))


def _n_q(S, causal):
    """Terms reduced into q row i: i + 1 causal, S otherwise.  [S,1]."""
    n = torch.arange(1, S + 1).double() if causal else \
        torch.full((S,), float(S), dtype=torch.float64)
    return n.unsqueeze(1)


def to_heads(x):
    """A kernel's [B,S,H,D] result as fp64 [B,H,S,D], the layout of every
    reference and bound here."""
    return x.detach().cpu().double().permute(0, 2, 1, 3)


# ---------------------------------------------------------------------------
# Forward
# ---------------------------------------------------------------------------
def fwd_ref(q, k, v, scale, causal, operand=None, rerounded=False, r_P=R_P,
            kv_of=None, batch_of=None):
    """O [B,Hq,S,D], lse [B,Hq,S] and their bounds.  ``rerounded`` adds the
    2^-8 score term (plain reference of a kernel that re-rounds an
    operand)."""
    assert not (rerounded and operand is not None)
    B, S, Hq, _ = q.shape
    s, absqk = _scores(q, k, scale, causal, operand, kv_of, batch_of)
    V = _expand(_heads(v), Hq, kv_of)
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = (m + l.log()).squeeze(-1)
    O = p @ V

    d = 4 * 128 * U32 * absqk + 4 * U32 * _finite(s - m).abs()
    if rerounded:
        d = d + U16 * absqk
    d = torch.where(torch.isfinite(s), d, torch.zeros_like(d))
    n = _n_q(S, causal)
    A = p @ V.abs()
    pd = p * d
    dbar = pd.sum(-1, keepdim=True)
    dmax = d.max(-1, keepdim=True).values
    soft = (pd @ V.abs() + dbar * A) * torch.exp(2 * dmax)
    tol_O = tol_bf16(O, A, K=n + 4) + r_P * U16 * A + soft
    tol_lse = (dbar + tol_f32(torch.ones_like(dbar), K=n + 4)
               + 4 * U32 * (m.abs() + l.log().abs())).squeeze(-1)
    return types.SimpleNamespace(O=O, lse=lse, tol_O=tol_O, tol_lse=tol_lse)


# ---------------------------------------------------------------------------
# Backward
# ---------------------------------------------------------------------------
def bwd_ref(q, k, v, O, dO, lse, scale, causal, operand=None,
            rerounded=False, r_P=R_P, extra_delta=None, defect=None):
    """dQ [B,Hq,S,D], dK, dV [B,Hkv,S,D] and their bounds from the given
    O (bf16), dO (bf16) and lse (fp32, [B,Hq,S]).  ``extra_delta``
    [B,Hq,S] widens the score error per q row (a chained forward's lse
    tolerance).  ``defect`` plants a named bug (test_attn_train_reference)."""
    assert not (rerounded and operand is not None)
    B, S, Hq, _ = q.shape
    Hkv = k.shape[2]
    sc = torch.tensor(scale, dtype=torch.float32).double().item()
    kv_of = (lambda h: h % Hkv) if defect == "kvh_mod" else None
    batch_of = (lambda b: 0) if defect == "batch0_k" else None
    s, absqk = _scores(q, k, scale, causal, operand, kv_of, batch_of)
    Q, K, V = _heads(q), _expand(_heads(k), Hq, kv_of), \
        _expand(_heads(v), Hq, kv_of)
    Oh, dOh = _heads(O), _heads(dO)
    L = lse.detach().cpu().double().unsqueeze(-1)
    if defect == "lse_log2":
        L = L * LOG2E
    dead = torch.isinf(L) & (L < 0)          # lse = -inf: the row is off
    p = torch.where(dead | ~torch.isfinite(s), torch.zeros_like(s),
                    (s - _finite(L)).exp())
    Dvec = (dOh * Oh).sum(-1, keepdim=True)
    dP = dOh @ V.transpose(-1, -2)
    dS = p * (dP if defect == "no_dvec" else dP - Dvec)
    first = defect == "first_head_only"
    dV = _group_sum(p.transpose(-1, -2) @ dOh, Hkv, first)
    dK = _group_sum(dS.transpose(-1, -2) @ Q, Hkv, first) * \
        (1.0 if defect == "dk_no_scale" else sc)
    dQ = (dS @ K) * (sc * sc if defect == "dq_scale_twice" else sc)
    if defect is not None:
        return types.SimpleNamespace(dQ=dQ, dK=dK, dV=dV)

    m = s.max(-1, keepdim=True).values
    d = (4 * 128 * U32 * absqk + 4 * U32 * _finite(s - m).abs()
         + 4 * U32 * _finite(L).abs() * LOG2E)
    if rerounded:
        d = d + U16 * absqk
    if extra_delta is not None:
        d = d + extra_delta.double().unsqueeze(-1)
    ep = p * torch.expm1(d)
    e_dP = 4 * 128 * U32 * (dOh.abs() @ V.abs().transpose(-1, -2))
    e_Dv = 4 * 128 * U32 * (dOh.abs() * Oh.abs()).sum(-1, keepdim=True)
    e_dS = ep * (dP - Dvec).abs() + (p + ep) * (e_dP + e_Dv)

    group = Hq // Hkv
    n_q = _n_q(S, causal)
    n_kv = (group * (S - torch.arange(S).double()) if causal else
            torch.full((S,), float(group * S), dtype=torch.float64)
            ).unsqueeze(1)
    pT, dST, eT = (x.transpose(-1, -2) for x in (p, dS.abs(), e_dS))
    A_v = _group_sum(pT @ dOh.abs(), Hkv)
    tol_dV = (tol_bf16(dV, A_v, K=n_kv + 4) + r_P * U16 * A_v
              + _group_sum(ep.transpose(-1, -2) @ dOh.abs(), Hkv))
    A_k = sc * _group_sum(dST @ Q.abs(), Hkv)
    tol_dK = (tol_bf16(dK, A_k, K=n_kv + 4) + U16 * A_k
              + sc * _group_sum(eT @ Q.abs(), Hkv))
    A_q = sc * (dS.abs() @ K.abs())
    tol_dQ = (tol_bf16(dQ, A_q, K=n_q + 4) + U16 * A_q
              + sc * (e_dS @ K.abs()))
    return types.SimpleNamespace(dQ=dQ, dK=dK, dV=dV, tol_dQ=tol_dQ,
                                 tol_dK=tol_dK, tol_dV=tol_dV)


# ---------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------
def _unit_e():
    """The fixed +-1 direction of the rising / creeping / falling /
    peaked families."""
    g = torch.Generator().manual_seed(20240607)
    return torch.where(torch.rand(D, generator=g, dtype=torch.float64) < 0.5,
                       -1.0, 1.0).double()


def make_inputs(family, B, S, Hq, Hkv, scale=SCALE):
    """(q, k, v, dO) as CPU bf16 tensors in the kernels' layout."""
    assert family in FAMILIES, family
    g = torch.Generator().manual_seed(
        zlib.crc32(repr((family, B, S, Hq, Hkv)).encode()))

    def rnd(H, f=1.0):
        return torch.randn(B, S, H, D, generator=g, dtype=torch.float64) * f

    amp = 0.5 if family in ("flat", "const_v", "const_dO") else 1.0
    q, k, v, dO = rnd(Hq, amp), rnd(Hkv, amp), rnd(Hkv, amp), rnd(Hq, amp)
    e = _unit_e()
    ramp = (torch.arange(S).double() / 64.0).view(1, S, 1, 1)
    if family in ("rising", "creeping", "falling"):
        nats = {"rising": 12.0, "creeping": 3.0, "falling": -12.0}[family]
        c = nats / (scale * D)     # q.k moves by D*c per 64 rows
        q = 0.5 * q + e
        k = 0.5 * k + e * ramp * c
    elif family == "peaked":
        # scores of about +-60: q = a e, k_l = +-a e, scale * D * a^2 = 60
        a = math.sqrt(60.0 / (scale * D))
        sign = torch.where(
            torch.rand(B, S, Hkv, 1, generator=g, dtype=torch.float64) < 0.5,
            -1.0, 1.0).double()
        q = 0.1 * q + a * e
        k = 0.1 * k + a * e * sign
    elif family == "equal":
        q = torch.zeros_like(q)
    elif family == "const_v":
        v = v[:, :1, :1].expand(B, S, Hkv, D).contiguous() * 2
    elif family == "const_dO":
        dO = dO[:, :1, :1].expand(B, S, Hq, D).contiguous() * 2
    return tuple(t.bfloat16() for t in (q, k, v, dO))


# ---------------------------------------------------------------------------
# fp32/bf16 CPU emulations of the forward kernels' rounding schemes
# ---------------------------------------------------------------------------
def _bf(x):
    return x.float().bfloat16().float()


def _trunc(x):
    x = x.float().contiguous()
    return (x.view(torch.int32) & (-65536)).view(torch.float32)


def _emu_heads(fn, q, k, v, scale, causal, **kw):
    B, S, Hq, _ = q.shape
    group = Hq // k.shape[2]
    O = torch.empty(B, Hq, S, D, dtype=torch.float64)
    lse = torch.empty(B, Hq, S, dtype=torch.float64)
    for b in range(B):
        for h in range(Hq):
            o, l = fn(q[b, :, h].float(), k[b, :, h // group].float(),
                      v[b, :, h // group].float(), scale, causal, **kw)
            O[b, h], lse[b, h] = o.double(), l.double()
    return O, lse


def _emu64_head(q, k, v, scale, causal, trunc=False):
    """attn_fwd_swapped_kernel: 64-row kv tiles, -inf mask, natural-unit
    exp, rescale on every tile, l summed from the unrounded P."""
    S = q.shape[0]
    s = (q @ k.T) * torch.tensor(scale, dtype=torch.float32)
    if causal:
        s = s.masked_fill(_mask(S), float("-inf"))
    m = torch.full((S, 1), float("-inf"))
    l = torch.zeros(S, 1)
    o = torch.zeros(S, D)
    for t in range(S // 64):
        st = s[:, t * 64:(t + 1) * 64]
        m_new = torch.maximum(m, st.max(-1, keepdim=True).values)
        m_safe = torch.where(torch.isinf(m_new), torch.zeros_like(m), m_new)
        corr = torch.where(torch.isinf(m), torch.zeros_like(m),
                           (m - m_safe).exp())
        m = m_new
        e = torch.where(torch.isinf(st), torch.zeros_like(st),
                        (st - m_safe).exp())
        l = l * corr + e.sum(-1, keepdim=True)
        o = o * corr + (_trunc(e) if trunc else _bf(e)) @ v[t * 64:(t + 1) * 64]
    return _bf(o / l), (m + l.log()).squeeze(-1)


def emu_fwd64(q, k, v, scale, causal, trunc=False):
    return _emu_heads(_emu64_head, q, k, v, scale, causal, trunc=trunc)


def _emu_v3_head(q, k, v, scale, causal, defect=None):
    """attn_fwd_v3_kernel: Q' = bf16(q * qs), exp2 softmax over 64-row kv
    tiles, -30000 mask fill, a wave of 32 q rows rescales only when one of
    its rows' maximum grew by more than 8, P rounded to nearest, l summed
    from the unrounded P, lse = ln2 * m + ln l.

    defect: no_l_rescale | diag_plus | diag_minus | skip_last_row |
    drop_last_tile."""
    S = q.shape[0]
    s = reround(q, scale).float() @ k.T
    rows = torch.arange(S).unsqueeze(1)
    cols = torch.arange(S).unsqueeze(0)
    if causal:
        off = {"diag_plus": 1, "diag_minus": -1}.get(defect, 0)
        s = s.masked_fill(cols > rows + off, -30000.0)
    if defect == "skip_last_row":
        s[:, S - 1] = -30000.0
    m = torch.full((S, 1), float("-inf"))
    l = torch.zeros(S, 1)
    o = torch.zeros(S, D)
    wave_last = (rows // 32) * 32 + 31       # last q row of the row's wave
    for t in range(S // 64):
        st = s[:, t * 64:(t + 1) * 64]
        active = (t <= (wave_last >> 6)) if causal else torch.ones_like(rows, dtype=torch.bool)
        if defect == "drop_last_tile" and t == S // 64 - 1:
            active = active & (rows < S - 128)
        pm = st.max(-1, keepdim=True).values
        need = ((pm - m) > 8.0) & active
        need = need.view(S // 32, 32, 1).any(1, keepdim=True) \
            .expand(-1, 32, -1).reshape(S, 1) & active
        m_new = torch.maximum(m, pm)
        corr = torch.where(torch.isinf(m), torch.zeros_like(m),
                           torch.exp2(m - m_new))
        corr = torch.where(need, corr, torch.ones_like(corr))
        o = o * corr
        if defect != "no_l_rescale":
            l = l * corr
        m = torch.where(need, m_new, m)
        e = torch.where(active, torch.exp2(st - m), torch.zeros_like(st))
        l = l + e.sum(-1, keepdim=True)
        o = o + _bf(e) @ v[t * 64:(t + 1) * 64]
    return _bf(o / l), (0.69314718055994530942 * m + l.log()).squeeze(-1)


def emu_fwd_v3(q, k, v, scale, causal, defect=None):
    return _emu_heads(_emu_v3_head, q, k, v, scale, causal, defect=defect)
