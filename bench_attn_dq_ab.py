"""A/B timer for the two v3 dq backward kernels.

Shape B6 S4096 Hq32 Hkv8 D128 causal (the bench.py micro-batch).  Both
`dq_variant`s run in one process, alternating round by round after a
warm-up of both; device events around `attn_bwd` (pre + dkv + dq, dkv
fixed at its default), so the difference between the arms is dq.  Prints
per-arm median / min / max, variant 0's spread `(max - min) / median`,
and whether variant 1's slowest round beats variant 0's fastest; asserts
that dQ, dK and dV of the two arms are bit-identical.

AB_ROUNDS (6) and AB_CALLS (4) size the measurement."""
import os
import statistics
import sys

import torch

if not torch.cuda.is_available():
    sys.exit("bench_attn_dq_ab.py needs a GPU: the dq kernels are HIP "
             "kernels for gfx950 and there is no fallback")

from skypilot_amd import ops  # noqa: E402

B, S, Hq, Hkv, D = 6, 4096, 32, 8, 128
SCALE = D ** -0.5
ROUNDS = max(6, int(os.environ.get("AB_ROUNDS", 6)))
CALLS = max(4, int(os.environ.get("AB_CALLS", 4)))
# causal 3-matmul count of the dq kernel with its 128-row diagonal tiles.
DQ_FLOP = 3 * 2.0 * B * Hq * D * S * (S + 128) / 2

dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)


def rnd(*shape):
    return (torch.randn(*shape, device=dev, generator=g) * 0.5).bfloat16()


q, k, v = rnd(B, S, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
dO = rnd(B, S, Hq, D)
C = ops.native()
O, lse = C.attn_fwd(q, k, v, SCALE, True)


def bwd(variant):
    return C.attn_bwd(q, k, v, O, dO, lse, SCALE, True, -1, variant)


# warm-up of both arms, and the bit-identity check.
outs = {}
for variant in (0, 1):
    for _ in range(3):
        outs[variant] = bwd(variant)
torch.cuda.synchronize()
for name, a, b in zip(("dQ", "dK", "dV"), outs[0], outs[1]):
    assert torch.equal(a, b), f"{name} differs between dq_variant 0 and 1"
del outs
print(f"[dq A/B B={B} S={S} Hq={Hq} Hkv={Hkv} causal] dQ/dK/dV "
      "bit-identical between the arms")

times = {0: [], 1: []}  # ms per call, one entry per round
for _ in range(ROUNDS):
    for variant in (0, 1):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(CALLS):
            bwd(variant)
        stop.record()
        stop.synchronize()
        times[variant].append(start.elapsed_time(stop) / CALLS)

med = {}
for variant in (0, 1):
    t = times[variant]
    med[variant] = statistics.median(t)
    print(f"dq_variant={variant}: attn_bwd median {med[variant]:.3f} ms  "
          f"min {min(t):.3f}  max {max(t):.3f}  ({ROUNDS} rounds x {CALLS} "
          "calls)")
spread = (max(times[0]) - min(times[0])) / med[0]
saving = med[0] - med[1]
print(f"variant 0 spread (max - min) / median: {spread * 100:.2f} %")
print(f"dq saving (median 0 - median 1): {saving:.3f} ms per call; dq is "
      f"{DQ_FLOP / 1e12:.2f} TFLOP, so a dq kernel of t ms runs at "
      f"{DQ_FLOP / 1e9:.0f} / t TF/s (per-kernel times: rocprofv3 "
      "--kernel-trace --stats on this script)")
wins = max(times[1]) < min(times[0])
print("variant 1 slowest round < variant 0 fastest round: "
      f"{'yes' if wins else 'no'} ({max(times[1]):.3f} vs "
      f"{min(times[0]):.3f} ms)")
sys.stdout.flush()
