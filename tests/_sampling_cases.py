"""Shared case builders for the decode-sampling tests (CPU reference and
GPU kernel).  Everything here is computed in fp64 straight from the
definition in docs/KERNELS.md, independently of ops.sample_row_reference.
"""
import torch


def make_rows(b, V, seed, scale=4.0):
    """bf16 logits [b, V] ~ randn * scale, with a tied group planted in
    every row (three equal values near the upper quartile)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(b, V, generator=g) * scale).bfloat16()
    for i in range(b):
        srt = x[i].float().sort(descending=True).values
        v = srt[max(1, V // 8)]
        idx = torch.randperm(V, generator=g)[:3]
        x[i, idx] = v.bfloat16()
    return x


def distinct_desc(row, T):
    """(values descending, mass at or above each value, Z) in fp64."""
    l = row.float().double()
    w = torch.exp((l - l.max()) / T)
    vals = sorted(set(l.tolist()), reverse=True)
    pos = {v: i for i, v in enumerate(vals)}
    gm = [0.0] * len(vals)
    for lv, wv in zip(l.tolist(), w.tolist()):
        gm[pos[lv]] += wv
    cum, run = [], 0.0
    for m in gm:
        run += m
        cum.append(run)
    return vals, cum, run


def top_p_cases(row, T, min_gap, want=6):
    """[(top_p, expected tau)]: top_p is the midpoint between two
    consecutive cumulative masses (over distinct values, descending), so
    tau must be the lower of the two values.  Only boundaries whose
    midpoint sits more than min_gap * Z from both masses are used —
    min_gap is the caller's bound on how far its summation (and the fp32
    rounding of top_p itself) can be from the exact masses."""
    vals, cum, Z = distinct_desc(row, T)
    ok = [i for i in range(len(vals) - 1)
          if (cum[i + 1] - cum[i]) / (2 * Z) > min_gap]
    step = max(1, len(ok) // want)
    picks = sorted(set(ok[:2] + ok[::step][:want] + ok[-1:]))
    out = []
    for i in picks:
        p = float(torch.tensor((cum[i] + cum[i + 1]) / (2 * Z),
                               dtype=torch.float32))
        out.append((p, vals[i + 1]))
    return out


def top_k_cases(row):
    """[(top_k, expected tau)] at, just below and just above the first
    group of tied values, and one above the group."""
    srt = sorted(row.float().double().tolist(), reverse=True)
    r0 = next(i for i in range(1, len(srt) - 1) if srt[i] == srt[i + 1]
              and srt[i] != srt[i - 1])
    g = 1
    while r0 + g < len(srt) and srt[r0 + g] == srt[r0]:
        g += 1
    ks = [k for k in (r0, r0 + 1, r0 + g - 1, r0 + g, r0 + g + 1)
          if 0 < k < len(srt)]
    return [(k, srt[k - 1]) for k in sorted(set(ks))]
