"""fp64 reference, derived bound, cases and a CPU emulation for the
chunked-prefill attention kernels (attn_append_kernel and
attn_append_fp8_kernel: attention_append.hip, attn_append_body.h).  Used
by test_attn_append_reference.py (CPU) and test_attn_append_fp64_gpu.py.

Reference
---------
Plain torch fp64 per sequence and q head, written from the definition in
``ops.attn_append_ref``'s docstring, on the bf16 values as stored.  Row
``i < q_len`` of sequence ``b`` sits at position ``q_start + i`` and attends
the rows ``kv <= q_start + i``, ``kv < kv_len = min(q_start + q_len,
S_max)`` of cache slot ``slot_ids[b]``, kv head ``qh // (Hq // Hkv)``:

    s = scale * q k^T      p = softmax over the visible rows      O = p v

Rows ``>= q_len`` of the chunk are padding and have no reference.

Bound
-----
The kernel has the structure of the 64-tile training forward
(attn_fwd_swapped_kernel): fp32 MFMA dot products, natural-unit
``__expf``, ``P`` rounded to nearest by ``f2bf`` before the PV MFMA, ``l``
summed from the unrounded ``P``, a rescale on every kv tile, one bf16
rounding of ``O``.  It re-rounds no operand, so the bound is ``tol_O`` of
``_attn_fp64.fwd_ref`` for the plain reference with ``r_P = 1`` and without
the ``2^-8 * sum|q k|`` score term (the derivation of each term is in
``_attn_fp64.py``), unchanged in form:

    d_l   = 4 * 128 * 2^-24 * sum_d |q_d k_ld| * scale     fp32 dot product
          + 4 * 2^-24 * |s_l - m|                          exp argument
    A     = sum_l p_l |v_l|
    tol_O = 2 * 2^-8 * |O| + 4 * (n + 4) * 2^-24 * A + 1e-30   tol_bf16
          + 2^-8 * A                                       P to bf16, nearest
          + (sum_l p_l d_l |v_l| + (sum_l p_l d_l) * A) * exp(2 max_l d_l)

The one change is ``n``, the number of terms reduced into the row: the rows
the q row sees, ``min(q_start + i + 1, kv_len)``, where the training
forward has ``i + 1``.  Every valid element is held to the bound and none
is excluded; the bound is not tuned to what a kernel returns.

Cases
-----
``GEOMS`` holds three geometries, each a list of ``(q_start, q_len)``; the
comment beside each sequence says which edge of the kernel it reaches.
``CASES`` lets each geometry meet each input family once and each head
shape at least once.  A sequence with ``kv_len = L`` takes ``(q, k, v)`` of
``_attn_fp64.make_inputs`` at ``S = L``: ``k``, ``v`` fill rows ``[0, L)`` of
its slot and the chunk is rows ``[q_start, q_start + q_len)`` of ``q`` (rows
at or past ``S_max`` repeat the last one), so the ramps of the rising /
creeping / falling families sit at absolute positions.  The cache has one
slot per sequence and two spare ones, in permuted order, with the sequence
that ends at ``S_max`` in the last slot, and NaN in every row at or past
each ``kv_len`` and in the spare slots.

Emulation
---------
``emu_append`` follows the kernel's rounding scheme in fp32/bf16 on the
CPU: 64-row q tiles, kv tiles of 64 counted from slot row 0 up to
``kv_end``, the mask decision per wave of 16 rows, the mask at the capped
absolute position and at ``kv_len``, ``P`` to bf16 by nearest, ``l`` from
the unrounded ``P``, ``O = bf16(o * (1 / l))``.  The kernel clamps the row
index of a partial tile to ``kv_len - 1``; the emulation instead reads the
slot's own rows (NaN in the test cache) and NaN past ``S_max``, which is
the same for the clean kernel (K's score there is masked, V is staged as
zeros) and lets a defect that drops either precaution show.  ``defect=``
plants one of ``DEFECTS``.
"""
import functools
import types
import zlib

import torch

import _attn_fp64 as af
from _fp64_check import U16, U32, f32, tol_bf16, tol_f32

D = af.D
SCALE = af.SCALE
BM = BN = 64

FAMILIES = ("flat", "unit", "rising", "creeping", "falling", "peaked",
            "equal", "const_v")
HEADS = [(1, 1), (4, 1), (8, 2), (5, 1), (6, 2), (4, 4)]

GEOMS = {
    # two q tiles, S_max no multiple of the kv tile
    "A": dict(S_max=200, Sq=128, seqs=[
        (72, 128),   # ends at S_max, last slot: the partial tile is the
                     # last rows of the allocation
        (0, 128),    # plain causal attention, kv_len % 64 == 0
        (37, 1),     # one decode step
        (100, 65),   # partial second q tile from an unaligned start
        (0, 1),      # kv_len = 1
        (63, 1),     # kv_len = 64: the fast path of the only tile, and
                     # kvbase + 63 == wave_pos0
        (64, 1),     # a second kv tile holding one row
        (1, 63),     # kv_len = 64, fast path, diagonal shifted by 1
        (48, 16),    # kv_len = 64, fast path, one wave valid
        (0, 64),     # one whole q tile
        (15, 17),    # q_start mod 16 = 15, 0, 1 at kv_len = 32: the
        (16, 16),    # diagonal against the wave boundary
        (17, 15),
        (47, 17),    # the diagonal crosses the kv tile edge inside a wave
        (136, 64),   # ends at S_max from an aligned chunk
        (190, 20),   # cut at S_max: rows 10..19 sit at capped positions
        (199, 1),    # the row at position S_max - 1
        (50, 0),     # empty
    ]),
    # S_max one whole tile
    "B": dict(S_max=64, Sq=64, seqs=[
        (0, 64), (63, 1), (0, 1),
        (60, 10),    # cut at S_max = 64
    ]),
    # three q tiles; the last kv tile holds one row
    "C": dict(S_max=321, Sq=192, seqs=[
        (129, 192),  # ends at S_max, last slot
        (0, 192),
        (64, 130),   # partial third q tile
    ]),
}


def _cases():
    """(geometry, family, Hq, Hkv): in geometry g family i takes head shape
    (i + g) % 6, so the eight families cover the six shapes."""
    return [(name, fam) + HEADS[(i + g) % 6]
            for g, name in enumerate(GEOMS)
            for i, fam in enumerate(FAMILIES)]


CASES = _cases()
for _g in GEOMS:
    assert {c[1] for c in CASES if c[0] == _g} == set(FAMILIES)
    assert {c[2:] for c in CASES if c[0] == _g} == set(HEADS)


def kv_len_of(start, ln, S_max):
    return min(start + ln, S_max)


# ---------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build_case(case):
    """CPU inputs of a case, shared read-only: q [n,Sq,Hq,D] bf16 (padding
    rows zero), kc / vc [slots,S_max,Hkv,D] bf16 (NaN wherever the kernel
    must not read), slot_ids / starts / lens as lists."""
    geom, family, Hq, Hkv = case
    G = GEOMS[geom]
    S_max, Sq, seqs = G["S_max"], G["Sq"], G["seqs"]
    n, slots = len(seqs), len(seqs) + 2
    starts = [s for s, _ in seqs]
    lens = [l for _, l in seqs]
    # the first sequence that reaches S_max goes to the last slot, the
    # others to a permutation of the rest; two slots stay spare
    last = next(b for b, (s, l) in enumerate(seqs) if l and s + l >= S_max)
    g = torch.Generator().manual_seed(zlib.crc32(geom.encode()))
    free = torch.randperm(slots - 1, generator=g).tolist()
    slot_ids = [slots - 1] * n
    for b, s in zip([b for b in range(n) if b != last], free):
        slot_ids[b] = s
    assert len(set(slot_ids)) == n
    assert sum(s != b for b, s in enumerate(slot_ids)) > n // 2

    nan = float("nan")
    q = torch.zeros(n, Sq, Hq, D, dtype=torch.bfloat16)
    kc = torch.full((slots, S_max, Hkv, D), nan, dtype=torch.bfloat16)
    vc = torch.full((slots, S_max, Hkv, D), nan, dtype=torch.bfloat16)
    for b, (start, ln) in enumerate(seqs):
        if ln == 0:
            continue
        L = kv_len_of(start, ln, S_max)
        # batch entry b of a (b + 1)-batch: sequences of equal kv_len get
        # different data
        qf, kf, vf, _ = af.make_inputs(family, b + 1, L, Hq, Hkv)
        rows = (start + torch.arange(ln)).clamp(max=L - 1)
        q[b, :ln] = qf[b][rows]
        kc[slot_ids[b], :L] = kf[b]
        vc[slot_ids[b], :L] = vf[b]
    return types.SimpleNamespace(
        case=case, q=q, kc=kc, vc=vc, slot_ids=slot_ids, starts=starts,
        lens=lens, S_max=S_max, Sq=Sq, n=n, slots=slots, Hq=Hq, Hkv=Hkv,
        last=last)


# ---------------------------------------------------------------------------
# Reference and bound
# ---------------------------------------------------------------------------
def ref_seq(q, kc, vc, slot, start, ln, scale):
    """One sequence: q [>=ln, Hq, D] (its chunk), the cache, its slot.
    Returns O, tol_O and tol_f32 (the bound without its bf16 terms), fp64
    [Hq, ln, D]."""
    Hq, Hkv, S_max = q.shape[1], kc.shape[2], kc.shape[1]
    L = kv_len_of(start, ln, S_max)
    kvh = torch.arange(Hq) // (Hq // Hkv)
    Q = q[:ln].double().permute(1, 0, 2)                     # [Hq, ln, D]
    K = kc[slot, :L].double().permute(1, 0, 2)[kvh]          # [Hq, L, D]
    V = vc[slot, :L].double().permute(1, 0, 2)[kvh]
    sc = f32(scale)
    s = (Q @ K.transpose(-1, -2)) * sc
    absqk = (Q.abs() @ K.abs().transpose(-1, -2)) * sc
    pos = start + torch.arange(ln, dtype=torch.int64)
    hidden = torch.arange(L)[None, :] > pos[:, None]         # [ln, L]
    s = s.masked_fill(hidden, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    p = e / e.sum(-1, keepdim=True)
    O = p @ V

    d = 4 * 128 * U32 * absqk + 4 * U32 * af._finite(s - m).abs()
    d = torch.where(hidden, torch.zeros_like(d), d)
    n_vis = (pos + 1).clamp(max=L).double().unsqueeze(1)     # [ln, 1]
    A = p @ V.abs()
    pd = p * d
    dbar = pd.sum(-1, keepdim=True)
    dmax = d.max(-1, keepdim=True).values
    soft = (pd @ V.abs() + dbar * A) * torch.exp(2 * dmax)
    tol = tol_bf16(O, A, K=n_vis + 4) + af.R_P * U16 * A + soft
    # an fp32 evaluation without bf16 roundings: accumulation and softmax
    tol32 = tol_f32(A, K=n_vis + 4) + soft
    return types.SimpleNamespace(O=O, tol_O=tol, tol_f32=tol32)


def ref_batch(q, kc, vc, slot_ids, starts, lens, scale=SCALE):
    """[ref_seq or None (empty)] per sequence."""
    return [ref_seq(q[b], kc, vc, slot_ids[b], starts[b], lens[b], scale)
            if lens[b] > 0 else None for b in range(len(lens))]


@functools.lru_cache(maxsize=None)
def case_refs(case):
    c = build_case(case)
    return ref_batch(c.q, c.kc, c.vc, c.slot_ids, c.starts, c.lens)


def seq_rows(out, b, ln):
    """Valid rows of sequence b of a kernel result [n,Sq,Hq,D] as fp64
    [Hq, ln, D], the references' layout."""
    return out[b, :ln].detach().cpu().double().permute(1, 0, 2)


def const_v_bias(c, got):
    """Family const_v: every visible V row of a sequence is the same v, so
    O = v up to the roundings.  (mean signed relative error of the valid
    rows of ``got`` against v, share of elements that differ from v)."""
    num, off, den = 0.0, 0, 0
    kvh = torch.arange(c.Hq) // (c.Hq // c.Hkv)
    for b, ln in enumerate(c.lens):
        if ln == 0:
            continue
        want = c.vc[c.slot_ids[b], 0].double()[kvh][:, None, :]
        diff = seq_rows(got, b, ln) - want
        num += float((diff / want).sum())
        off += int((diff != 0).sum())
        den += diff.numel()
    return num / den, off / den


# ---------------------------------------------------------------------------
# CPU emulation of the kernel's rounding scheme
# ---------------------------------------------------------------------------
DEFECTS = (
    "diag_no_start",       # the diagonal at i, ignoring q_start
    "diag_plus",           # the diagonal one row late
    "diag_minus",          # ... one row early
    "mask_from_wave_last",  # need_mask from the wave's last row
    "need_mask_off_by_one",  # need_mask: kvbase + 63 > wave_pos0 + 1
    "skip_last_row",       # row kv_len - 1 masked
    "no_kvlen_mask",       # rows >= kv_len masked by the diagonal only
    "v_not_zeroed",        # V rows past kv_len staged as they are
    "drop_last_tile",      # the last partial kv tile dropped
    "kv_end_no_tile",      # kv_end = min(kv_len, q_start + qbase)
    "slot_b",              # slot b read instead of slot_ids[b]
    "kvh_mod",             # kvh = qh % Hkv
    "no_l_rescale",        # l not rescaled by corr
    "qtile_unreversed",    # tile qt stored where tile gridDim.x-1-qt goes
    "p_trunc",             # P truncated to bf16
)


def _emu_seq(q, kslot, vslot, start, ln, S_max, scale, defect):
    """q [Hq,Sq,D], kslot / vslot [Hq,S_max,D] fp32 -> [Hq,Sq,D] fp32
    holding bf16 values; padding-only tiles are zero."""
    Hq, Sq, _ = q.shape
    out = torch.zeros(Hq, Sq, D)
    ql = min(max(ln, 0), Sq)
    if start < 0:
        ql = 0
    kv_len = min(start + ql, S_max)
    sc = torch.tensor(scale, dtype=torch.float32)
    n_q = Sq // BM
    lane = torch.arange(BM)
    nan = float("nan")
    for qt in range(n_q):
        qbase = qt * BM
        if qbase >= ql:
            continue
        first = start + qbase
        if defect == "diag_no_start":
            first = qbase
        my_pos = (first + lane).clamp(max=S_max)
        wave_pos0 = (first + 16 * (lane // 16)).clamp(max=S_max)
        kv_end = min(kv_len, start + qbase +
                     (0 if defect == "kv_end_no_tile" else BM))
        n_kv = (kv_end + BN - 1) // BN
        if defect == "drop_last_tile" and kv_end % BN:
            n_kv -= 1
        qt_rows = q[:, qbase:qbase + BM]
        m = torch.full((Hq, BM, 1), float("-inf"))
        l = torch.zeros(Hq, BM, 1)
        o = torch.zeros(Hq, BM, D)
        for kt in range(n_kv):
            kvbase = kt * BN
            kv = kvbase + torch.arange(BN)
            inside = (kv < S_max).view(1, BN, 1)
            idx = kv.clamp(max=S_max - 1)
            K = torch.where(inside, kslot[:, idx], torch.tensor(nan))
            V = torch.where(inside, vslot[:, idx], torch.tensor(nan))
            if defect != "v_not_zeroed":
                V = torch.where((kv < kv_len).view(1, BN, 1), V,
                                torch.zeros(()))
            s = (qt_rows @ K.transpose(-1, -2)) * sc
            decide = wave_pos0 + {"mask_from_wave_last": 15,
                                  "need_mask_off_by_one": 1}.get(defect, 0)
            need = (kvbase + BN - 1 > decide) | (kvbase + BN > kv_len)
            off = {"diag_plus": 1, "diag_minus": -1}.get(defect, 0)
            hide = kv[None, :] > (my_pos + off)[:, None]
            if defect != "no_kvlen_mask":
                hide = hide | (kv >= kv_len)[None, :]
            if defect == "skip_last_row":
                hide = hide | (kv == kv_len - 1)[None, :]
            s = torch.where((need[:, None] & hide)[None],
                            torch.tensor(float("-inf")), s)
            m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
            m_safe = torch.where(torch.isinf(m_new) & (m_new < 0),
                                 torch.zeros_like(m), m_new)
            corr = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m),
                               (m - m_safe).exp())
            m = m_new
            e = torch.where(torch.isinf(s) & (s < 0), torch.zeros_like(s),
                            (s - m_safe).exp())
            rs = e.sum(-1, keepdim=True)
            l = (l if defect == "no_l_rescale" else l * corr) + rs
            p = af._trunc(e) if defect == "p_trunc" else af._bf(e)
            o = o * corr + p @ V
        inv_l = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        dst = (n_q - 1 - qt) * BM if defect == "qtile_unreversed" else qbase
        out[:, dst:dst + BM] = af._bf(o * inv_l)
    return out


def emu_append(q, kc, vc, slot_ids, starts, lens, scale=SCALE, defect=None):
    """The batch through _emu_seq: fp32 [n,Sq,Hq,D] holding bf16 values."""
    assert defect is None or defect in DEFECTS, defect
    n, Sq, Hq, _ = q.shape
    slots, S_max, Hkv = kc.shape[:3]
    kvh = torch.arange(Hq) % Hkv if defect == "kvh_mod" else \
        torch.arange(Hq) // (Hq // Hkv)
    out = torch.zeros(n, Sq, Hq, D)
    for b in range(n):
        slot = b if defect == "slot_b" else slot_ids[b]
        if slot < 0 or slot >= slots:
            continue
        kslot = kc[slot].float().permute(1, 0, 2)[kvh]
        vslot = vc[slot].float().permute(1, 0, 2)[kvh]
        o = _emu_seq(q[b].float().permute(1, 0, 2), kslot, vslot, starts[b],
                     lens[b], S_max, scale, defect)
        out[b] = o.permute(1, 0, 2)
    return out


def emu_case(case, defect=None):
    c = build_case(case)
    return emu_append(c.q, c.kc, c.vc, c.slot_ids, c.starts, c.lens,
                      defect=defect)
