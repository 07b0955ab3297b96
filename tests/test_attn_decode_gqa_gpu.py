"""attn_decode_gqa_kernel / attn_decode_gqa_fp8_kernel and the combine
kernel (attention_decode_gqa.hip) against the plain fp64 reference, element
by element, on the cases of test_gpu_decode_kernels.py plus one that sits on
the strip (32), 4-wave-step (128) and split edges.

Bound: attn_rows64's, with the terms tests/_attn_fp64.py uses for MFMA
kernels.  q (and the score of the current k) is rounded to bf16, one unit
roundoff per product: 2^-8 * Ad_l joins delta_l.  P is rounded to nearest
before the PV MFMA: 2^-8 * A.  The sums merge through L + 4 + splits terms.
No element is excluded."""
import functools

import pytest
import torch

from _fp64_check import TINY, U16, U32, check, tol_f32
from skypilot_amd import ops
from test_gpu_decode_kernels import (ATTN_CASES, D, NAN, SCALE, _bf,
                                     _decode_args, _expect_rejections, _z,
                                     assert_bits_equal, attn_case,
                                     check_attn_decode_qkv, dev, fused_case,
                                     gen, to_gpu_bf16)
from test_gpu_train_kernels import rope64
from test_kv_fp8_cpu import PROMPT, assert_codes_equal, exponent_by_definition
from test_kv_fp8_gpu import POISON_CODE, e4m3_spacing, quantize_poisoned

pytestmark = pytest.mark.gpu

STRIP_LENS = [32, 33, 128, 129, 130, 256, 257, 385]
CASES = ATTN_CASES + [("strips_385", 8, 2)]
SPLIT_ROWS = [-1, 128, 256]


@functools.lru_cache(maxsize=None)
def get_case(name, Hq, Hkv):
    """fused_case of an ATTN_CASES entry, or of strips_385: the same style
    (NaN at and past kv_len and in the spare slots, permuted slots, the
    last slot full to S_max = 385)."""
    if name != "strips_385":
        return fused_case(attn_case(name, Hq, Hkv))
    g = gen(1385)
    lens, S_max = STRIP_LENS, 385
    B = len(lens)
    slots = B + 3
    perm = torch.randperm(slots - 1, generator=g)[:B].tolist()
    perm[lens.index(S_max)] = slots - 1
    kc = torch.full((slots, S_max, Hkv, D), NAN)
    vc = torch.full((slots, S_max, Hkv, D), NAN)
    for L, slot in zip(lens, perm):
        kc[slot, :L] = torch.randn(L, Hkv, D, generator=g)
        vc[slot, :L] = torch.randn(L, Hkv, D, generator=g)
    q = torch.randn(B, Hq, D, generator=g).bfloat16().float()
    return fused_case(dict(
        name=name, Hq=Hq, Hkv=Hkv, S_max=S_max, lens=lens, q=q,
        kc=kc.bfloat16(), vc=vc.bfloat16(),
        kv_lens=torch.tensor(lens, dtype=torch.int32),
        slot_ids=torch.tensor(perm, dtype=torch.int32)))


def n_splits(S_max, split_rows):
    R = ops.native().DECODE_SPLIT_ROWS if split_rows < 0 else split_rows
    return -(-S_max // R)


def rows64(q, Aq, K, V, splits):
    """fp64 attention of q [Hq, D] over K, V [L, Hkv, D] and the bound of
    the module docstring."""
    rep = q.shape[0] // K.shape[1]
    Kx, Vx = K.repeat_interleave(rep, 1), V.repeat_interleave(rep, 1)
    d = torch.einsum("hd,lhd->hl", q, Kx) * SCALE
    Ad = torch.einsum("hd,lhd->hl", Aq, Kx.abs()) * SCALE
    p = torch.softmax(d, -1)
    delta = (4 * D * U32 + U16) * Ad + \
        4 * U32 * (d - d.max(-1, keepdim=True).values).abs()
    ref = torch.einsum("hl,lhd->hd", p, Vx)
    A = torch.einsum("hl,lhd->hd", p, Vx.abs())
    tol = (2 * U16 * ref.abs() + U16 * A + TINY
           + (2 * delta.max(-1).values[:, None]
              + 4 * (K.shape[0] + 4 + splits) * U32) * A)
    return ref, tol


def run(fc, fp8, split_rows, rows=None):
    """The op on (a subset of) the case's sequences, on fresh copies of its
    cache.  Returns out and the cache tensors after the call, on the CPU."""
    C = ops.native()
    rows = list(range(len(fc["lens"]))) if rows is None else rows
    g = lambda t: t.to(dev())
    idx = (g(fc["cos"]), g(fc["sin"]), g(fc["positions"][rows]),
           g(fc["kv_lens"][rows]), g(fc["slot_ids"][rows]))
    qkv = to_gpu_bf16(fc["qkv"][rows])
    if fp8:
        cache = [g(t) for t in (*quantize_poisoned(fc["kc"]),
                                *quantize_poisoned(fc["vc"]))]
        kc, ke, vc, ve = cache
        out = C.attn_decode_qkv_gqa_fp8(qkv, kc, vc, ke, ve, *idx, fc["Hq"],
                                        fc["Hkv"], SCALE, split_rows)
    else:
        cache = [g(fc["kc"]), g(fc["vc"])]
        out = C.attn_decode_qkv_gqa(qkv, *cache, *idx, fc["Hq"], fc["Hkv"],
                                    SCALE, split_rows)
    torch.cuda.synchronize()
    return out.cpu(), [t.cpu() for t in cache]


def only_k_row(tag, got, ref, tol):
    """check_attn_decode_qkv's cache part: its output check has the
    per-head kernel's bound, ours is checked with rows64."""
    if tag.endswith(" K row"):
        check(tag, got, ref, tol)


@pytest.mark.parametrize("split_rows", SPLIT_ROWS)
@pytest.mark.parametrize("name,Hq,Hkv", CASES)
def test_attn_decode_qkv_gqa_fp64(name, Hq, Hkv, split_rows):
    fc = get_case(name, Hq, Hkv)
    out, (kc, vc) = run(fc, False, split_rows)
    splits = n_splits(fc["S_max"], split_rows)
    q64, Aq = rope64(fc["q"], fc["cos"], fc["sin"], fc["positions"])
    k64, _ = rope64(fc["cur_k"], fc["cos"], fc["sin"], fc["positions"])
    refs, tols = [], []
    for b, L in enumerate(fc["lens"]):
        s = int(fc["slot_ids"][b])
        K = torch.cat([fc["kc"][s, :L - 1].double(), k64[b][None]])
        V = torch.cat([fc["vc"][s, :L - 1].double(),
                       fc["cur_v"][b].double()[None]])
        r, t = rows64(q64[b], Aq[b], K, V, splits)
        refs.append(r)
        tols.append(t)
    check(f"attn_decode_qkv_gqa {name} Hq={Hq} Hkv={Hkv} R={split_rows}",
          out, torch.stack(refs), torch.stack(tols))
    # kv_len == 1 bit-equal to v, the written row, every other byte
    check_attn_decode_qkv(fc, out, kc, vc, check_fn=only_k_row)


@pytest.mark.parametrize("split_rows", SPLIT_ROWS)
@pytest.mark.parametrize("name,Hq,Hkv", CASES)
def test_attn_decode_qkv_gqa_fp8_fp64(name, Hq, Hkv, split_rows):
    """Reference: attention over the dequantised cache as it is after the
    call, rows 0..p (dequantisation is exact); row p and the untouched
    bytes as test_attn_decode_qkv_fp8_fp64 checks them."""
    fc = get_case(name, Hq, Hkv)
    before = [*quantize_poisoned(fc["kc"]), *quantize_poisoned(fc["vc"])]
    out, after = run(fc, True, split_rows)
    kc, ke, vc, ve = after
    slot, pos = fc["slot_ids"].long(), fc["positions"].long()
    assert bool((before[0][slot, pos] == POISON_CODE).all())
    tag = f"attn_decode_qkv_gqa_fp8 {name} Hq={Hq} Hkv={Hkv} R={split_rows}"
    splits = n_splits(fc["S_max"], split_rows)
    q64, Aq = rope64(fc["q"], fc["cos"], fc["sin"], fc["positions"])
    refs, tols = [], []
    for b, L in enumerate(fc["lens"]):
        s = int(slot[b])
        K = ops.kv_dequantize(kc[s, :L], ke[s, :L]).double()
        V = ops.kv_dequantize(vc[s, :L], ve[s, :L]).double()
        assert bool(torch.isfinite(K).all() and torch.isfinite(V).all())
        r, t = rows64(q64[b], Aq[b], K, V, splits)
        refs.append(r)
        tols.append(t)
        if L == 1:
            assert_bits_equal(out[b], V[0].bfloat16().repeat_interleave(
                Hq // Hkv, dim=0), f"{tag} kv_len=1")
    check(tag, out, torch.stack(refs), torch.stack(tols))

    want_vc, want_ve = ops.kv_quantize(fc["cur_v"].bfloat16())
    assert_codes_equal(vc[slot, pos], want_vc, tag + " V row")
    assert torch.equal(ve[slot, pos], want_ve), tag + " V exponent"
    # K row: quantised from the fp32 rope, so the exponent is that of some
    # amax within rope's error, and each element the nearest grid point
    k64, Ak = rope64(fc["cur_k"], fc["cos"], fc["sin"], fc["positions"])
    t_k = tol_f32(Ak, K=2)
    amax, t_amax = k64.abs().amax(-1), t_k.amax(-1)
    e_got = ke[slot, pos]
    for b in range(amax.shape[0]):
        for h in range(Hkv):
            lo = exponent_by_definition(
                max(float(amax[b, h] - t_amax[b, h]), 0.0)) + 127
            hi = exponent_by_definition(
                float(amax[b, h] + t_amax[b, h])) + 127
            assert min(lo, hi) <= int(e_got[b, h]) <= max(lo, hi), (
                tag, b, h, lo, hi, int(e_got[b, h]))
    s = 2.0 ** (e_got.double() - 127)[..., None]
    check(tag + " K row", ops.kv_dequantize(kc[slot, pos], e_got).double(),
          k64, 0.5 * e4m3_spacing(k64.abs() / s) * s + t_k)
    for nm, got, old in zip(("Kc", "Ke", "Vc", "Ve"), after, before):
        rest = got.clone()
        rest[slot, pos] = old[slot, pos]
        assert torch.equal(rest, old), f"{tag} untouched {nm}"


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_row_of_a_batch_equals_the_sequence_alone(fp8):
    """Splits depend on S_max only: n = 8 against n = 1, bit for bit."""
    fc = get_case("strips_385", 8, 2)
    batch, _ = run(fc, fp8, 128)
    for b in range(len(fc["lens"])):
        alone, _ = run(fc, fp8, 128, rows=[b])
        assert_bits_equal(alone[0], batch[b], f"sequence {b} alone")


def test_attn_decode_qkv_gqa_rejects_bad_inputs():
    C = ops.native()
    a = _decode_args()
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev())

    def call(fp8=False, split_rows=-1, **kw):
        v = dict(a, **kw)
        tail = (v["cos"], v["sin"], v["positions"], v["kv_lens"],
                v["slot_ids"], v["Hq"], v["Hkv"], SCALE, split_rows)
        if fp8:
            return lambda: C.attn_decode_qkv_gqa_fp8(
                v["qkv"], v.get("Kc8", u8(3, 8, 2, D)), u8(3, 8, 2, D),
                u8(3, 8, 2), u8(3, 8, 2), *tail)
        return lambda: C.attn_decode_qkv_gqa(v["qkv"], v["Kc"], v["Vc"],
                                             *tail)

    call()()
    call(fp8=True)()
    g32 = dict(qkv=_bf(2, 34 * D), Kc=_bf(3, 8, 1, D), Vc=_bf(3, 8, 1, D),
               Hq=32, Hkv=1)
    _expect_rejections({
        "group 32": ("attn_decode_qkv_gqa: group Hq / Hkv = 32 exceeds 16",
                     call(**g32)),
        "split 100": ("attn_decode_qkv_gqa: split_rows must be -1 or a "
                      "positive multiple of 128, got 100",
                      call(split_rows=100)),
        "split 100 fp8": ("attn_decode_qkv_gqa_fp8: split_rows must be -1",
                          call(fp8=True, split_rows=100)),
        "Kc fp32": ("attn_decode_qkv_gqa: Kc must be BFloat16",
                    call(Kc=_z(3, 8, 2, D))),
        "Kc bf16": ("attn_decode_qkv_gqa_fp8: Kc must be Byte",
                    call(fp8=True, Kc8=_bf(3, 8, 2, D))),
    })


def test_engine_grouped_graph_and_eager_decode_agree():
    """No atomics and fixed splits: graphed and eager decode give the same
    24 greedy tokens from a 100-token prompt."""
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model("llama-debug", device="cuda:0")
    assert len(PROMPT) == 100
    outs = []
    for use_graphs in (True, False):
        eng = Engine("llama-debug", device="cuda:0", max_seq=256,
                     max_batch=4, model=model, decode_attn="grouped",
                     use_graphs=use_graphs)
        req = eng.submit(Request(prompt_ids=list(PROMPT), max_tokens=24))
        eng.start()
        try:
            assert req.done.wait(120), "request did not complete"
        finally:
            eng.stop()
        assert eng.use_graphs == use_graphs
        outs.append(req.out_ids)
    assert len(outs[0]) == 24 and outs[0] == outs[1]
