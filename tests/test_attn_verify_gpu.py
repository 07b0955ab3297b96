"""attn_verify_kernel (attention_verify.hip) against the plain fp64
reference, element by element, and Engine(speculative=K) end to end.

Bound: rows64 of test_attn_decode_gqa_gpu.py, unchanged, with the rows each
token sees (kv <= q_start + t).  Q is given roped and in bf16, so rows64's
q-rounding term 2^-8 * Ad is slack here, not a hazard.  The arithmetic is the
grouped decode kernel's: bf16 MFMA products into fp32, P rounded to nearest
before the PV MFMA, L + 4 + splits merged terms; a masked score adds an exact
zero.  No element is excluded.

Case style of get_case("strips_385") there: NaN in K and V at and past
q_start + T and in the spare slots, permuted slots, the last slot full to
S_max = 385."""
import functools

import pytest
import torch

from _fp64_check import check
from skypilot_amd import ops
from test_attn_decode_gqa_gpu import n_splits, rows64
from test_gpu_decode_kernels import (D, NAN, SCALE, _bf, _expect_rejections,
                                     _z, assert_bits_equal, dev, gen)
from test_kv_fp8_cpu import PROMPT

pytestmark = pytest.mark.gpu

S_MAX = 385
# (Hq, Hkv, T): two column blocks full and partly filled, one block, odd
# groups, the widest group
SHAPES = [(8, 2, 8), (8, 2, 5), (8, 1, 4), (7, 1, 4), (2, 1, 2), (16, 1, 2)]


def q_starts(T):
    """Tokens that see only each other; 1; the T rows across the 32-row
    strip edge; across the 128-row wave step and, with split_rows = 128,
    the split edge (early tokens see nothing in the last split); 250; the
    last row is row S_max - 1."""
    return [0, 1, 30, 126, 127, 250, S_MAX - T]


@functools.lru_cache(maxsize=None)
def get_case(Hq, Hkv, T):
    g = gen(2385 + 100 * Hq + 10 * Hkv + T)
    starts = q_starts(T)
    n = len(starts)
    slots = n + 3
    perm = torch.randperm(slots - 1, generator=g)[:n].tolist()
    perm[-1] = slots - 1
    kc = torch.full((slots, S_MAX, Hkv, D), NAN)
    vc = torch.full((slots, S_MAX, Hkv, D), NAN)
    for s0, slot in zip(starts, perm):
        kc[slot, :s0 + T] = torch.randn(s0 + T, Hkv, D, generator=g)
        vc[slot, :s0 + T] = torch.randn(s0 + T, Hkv, D, generator=g)
    return dict(Hq=Hq, Hkv=Hkv, T=T, starts=starts,
                q=torch.randn(n, T, Hq, D, generator=g).bfloat16(),
                kc=kc.bfloat16(), vc=vc.bfloat16(),
                slot_ids=torch.tensor(perm, dtype=torch.int32),
                q_start=torch.tensor(starts, dtype=torch.int32))


def run(c, split_rows, rows=None):
    rows = list(range(len(c["starts"]))) if rows is None else rows
    g = lambda t: t.to(dev())
    out = ops.attn_verify(g(c["q"][rows]), g(c["kc"]), g(c["vc"]),
                          g(c["slot_ids"][rows]), g(c["q_start"][rows]),
                          SCALE, split_rows)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("split_rows", [-1, 128])
@pytest.mark.parametrize("Hq,Hkv,T", SHAPES)
def test_attn_verify_fp64(Hq, Hkv, T, split_rows):
    c = get_case(Hq, Hkv, T)
    out = run(c, split_rows)
    splits = n_splits(S_MAX, split_rows)
    refs, tols = [], []
    for b, s0 in enumerate(c["starts"]):
        slot = int(c["slot_ids"][b])
        K, V = c["kc"][slot].double(), c["vc"][slot].double()
        for t in range(T):
            q = c["q"][b, t].double()
            r, tol = rows64(q, q.abs(), K[:s0 + t + 1], V[:s0 + t + 1],
                            splits)
            refs.append(r)
            tols.append(tol)
    shape = out.shape
    check(f"attn_verify Hq={Hq} Hkv={Hkv} T={T} R={split_rows}", out,
          torch.stack(refs).view(shape), torch.stack(tols).view(shape))


def test_row_of_a_batch_equals_the_sequence_alone():
    """Splits depend on S_max only: n = 7 against n = 1, bit for bit."""
    c = get_case(8, 2, 8)
    batch = run(c, 128)
    for b in range(len(c["starts"])):
        assert_bits_equal(run(c, 128, rows=[b])[0], batch[b],
                          f"sequence {b} alone")


def _i32(*shape, **kw):
    return _z(*shape, dtype=torch.int32, **kw)


@pytest.mark.parametrize("pattern,kw", [
    ("Q must be BFloat16", dict(Q=lambda: _z(2, 4, 4, D))),
    (r"Q must be \[n, T, Hq, 128\]", dict(Q=lambda: _bf(2, 4, 4 * D))),
    (r"Q must be \[n, T, Hq, 128\]", dict(Q=lambda: _bf(2, 4, 4, 64))),
    ("Q must be contiguous",
     dict(Q=lambda: _bf(2, 4, 4, 2 * D)[..., ::2])),
    ("Kc must be BFloat16", dict(Kc=lambda: _z(3, 16, 2, D))),
    ("Kc must be on GPU", dict(Kc=lambda: _bf(3, 16, 2, D).cpu())),
    (r"Kc must be \[slots, S_max, Hkv, 128\]",
     dict(Kc=lambda: _bf(3, 16, 2 * D))),
    ("Vc must have Kc's shape", dict(Vc=lambda: _bf(3, 8, 2, D))),
    ("Hq = 3 must be a positive multiple of Hkv = 2",
     dict(Q=lambda: _bf(2, 4, 3, D))),
    ("T = 1 must be at least 2", dict(Q=lambda: _bf(2, 1, 4, D))),
    (r"T \* \(Hq / Hkv\) = 64 exceeds 32", dict(Q=lambda: _bf(2, 8, 16, D))),
    ("split_rows must be -1 or a positive multiple of 128, got 100",
     dict(split_rows=100)),
    ("slot_ids must be Int",
     dict(slot_ids=lambda: _z(2, dtype=torch.int64))),
    (r"q_start must be a \[B\] = \[2\] tensor", dict(q_start=lambda: _i32(3))),
    ("q_start must be on GPU", dict(q_start=lambda: _i32(2, device="cpu"))),
])
def test_attn_verify_rejects_bad_inputs(pattern, kw):
    C = ops.native()
    v = dict(Q=lambda: _bf(2, 4, 4, D), Kc=lambda: _bf(3, 16, 2, D),
             Vc=lambda: _bf(3, 16, 2, D), slot_ids=lambda: _i32(2),
             q_start=lambda: _i32(2), split_rows=-1)

    def call(**over):
        a = {k: f() if callable(f) else f for k, f in dict(v, **over).items()}
        return lambda: C.attn_verify(a["Q"], a["Kc"], a["Vc"], a["slot_ids"],
                                     a["q_start"], SCALE, a["split_rows"])

    call()()
    _expect_rejections({pattern: ("attn_verify: " + pattern, call(**kw))})


@functools.lru_cache(maxsize=None)
def _model():
    from skypilot_amd.models.llama import build_model
    return build_model("llama-debug", device="cuda:0")


def _generate(**kw):
    from skypilot_amd.serve.engine import Engine, Request
    eng = Engine("llama-debug", device="cuda:0", max_seq=256, max_batch=4,
                 model=_model(), **kw)
    req = eng.submit(Request(prompt_ids=list(PROMPT), max_tokens=24))
    eng.start()
    try:
        assert req.done.wait(120), "request did not complete"
    finally:
        eng.stop()
    return req.out_ids, eng


@functools.lru_cache(maxsize=None)
def _plain_tokens():
    return tuple(_generate()[0])


@pytest.mark.parametrize("use_graphs", [True, False],
                         ids=["graph", "eager"])
@pytest.mark.parametrize("right", [True, False], ids=["oracle", "wrong"])
def test_engine_speculative_gives_the_plain_tokens(right, use_graphs):
    """24 greedy tokens from a 100-token prompt: an oracle drafter proposes
    what the non-speculative engine produced, a wrong one never does; both
    must emit exactly those tokens."""
    want = list(_plain_tokens())
    full = list(PROMPT) + want

    def drafter(ids, k):
        nxt = full[len(ids):len(ids) + k]
        return nxt if right else [(t + 1) % 512 for t in nxt]

    got, eng = _generate(speculative=3, drafter=drafter,
                         use_graphs=use_graphs)
    assert eng.use_graphs == use_graphs
    assert bool(eng.stats.get("spec_graph_buckets")) == use_graphs
    assert len(want) == 24 and got == want
    assert eng.stats["spec_steps"] > 0
    if right:
        assert eng.stats["spec_accepted"] > 0
        assert eng.stats["spec_steps"] < len(got)
    else:
        assert eng.stats["spec_accepted"] == 0
