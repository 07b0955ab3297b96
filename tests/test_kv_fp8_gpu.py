"""The FP8 KV-cache kernels on the GPU (kv_write_fp8.hip,
attention_decode_fp8.hip, attn_append_fp8_kernel in attention_append.hip)
against ops.kv_quantize / kv_dequantize and the fp64 checker of
test_gpu_decode_kernels.py, their bindings' rejections, and the engine with
kv_dtype="fp8".

Wherever a cache row must not be read it holds the poison: codes 0x7F
(e4m3fn NaN) and exponent 0xFF (scale +Inf).  Shapes are the suite's small
ones; every bound is derived beside its check."""
import functools
import math

import pytest
import torch

from _fp64_check import check, tol_f32
from skypilot_amd import ops
from test_gpu_decode_kernels import (ATTN_CASES, SCALE, _bf, _decode_args,
                                     _expect_rejections, _z, assert_bits_equal,
                                     attn_case, attn_rows64, attn_tol, dev,
                                     fused_case, to_gpu_bf16)
from test_gpu_train_kernels import rope64
from test_kv_fp8_cpu import (PROMPT, all_code_rows, assert_codes_equal,
                             check_prompt_rows, exponent_by_definition,
                             tie_row)

pytestmark = pytest.mark.gpu

D = 128
POISON_CODE, POISON_EXP = 0x7F, 0xFF


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev())


def _u8(*shape, fill=0):
    return torch.full(shape, fill, dtype=torch.uint8, device=dev())


def quantize_poisoned(cache):
    """A bf16 cache whose unused rows are NaN -> codes and exponents with
    the poison in those rows."""
    codes, exps = ops.kv_quantize(torch.nan_to_num(cache.float()))
    dead = torch.isnan(cache.float()).any(-1)
    codes[dead] = POISON_CODE
    exps[dead] = POISON_EXP
    return codes, exps


# ===========================================================================
# kv_write_fp8.
# ===========================================================================
def byte_pattern(shape, offset):
    n = math.prod(shape)
    return ((torch.arange(n) * 7 + offset) % 251).to(torch.uint8).reshape(shape)


@pytest.mark.parametrize("Hkv", [1, 2])
def test_kv_write_fp8_bits_and_untouched_bytes(Hkv):
    g = torch.Generator().manual_seed(40 + Hkv)
    S, S_max, slots = 64, 70, 5
    # 0: ends exactly at S_max in the last slot; 1: empty; 2: 7 rows of
    # overflow past S_max dropped; 3, 4: slots the cache does not have;
    # 5: negative start
    slot_ids = [slots - 1, 2, 1, -1, slots, 0]
    starts = [S_max - 64, 3, 40, 0, 0, -2]
    lens = [64, 0, 37, 10, 10, 10]
    n = len(lens)
    mult = 10.0 ** torch.randint(-3, 3, (n, S, Hkv, 1), generator=g).float()
    k = torch.randn(n, S, Hkv, D, generator=g) * mult
    v = torch.randn(n, S, Hkv, D, generator=g) * mult
    k[0, 0, 0] = tie_row()[0][0]
    k[0, 1:3, 0] = all_code_rows(-20)[0]
    v[0, 3:5, 0] = all_code_rows(9)[0]
    v[2, 0, 0] = 0.0                                   # a zero row
    k, v = k.bfloat16(), v.bfloat16()
    before = dict(kc=byte_pattern((slots, S_max, Hkv, D), 0),
                  vc=byte_pattern((slots, S_max, Hkv, D), 101),
                  ke=byte_pattern((slots, S_max, Hkv), 17),
                  ve=byte_pattern((slots, S_max, Hkv), 5))
    want = {name: t.clone() for name, t in before.items()}
    for b in (0, 2):
        rows = min(lens[b], S_max - starts[b])
        dst = slice(starts[b], starts[b] + rows)
        want["kc"][slot_ids[b], dst], want["ke"][slot_ids[b], dst] = \
            ops.kv_quantize(k[b, :rows])
        want["vc"][slot_ids[b], dst], want["ve"][slot_ids[b], dst] = \
            ops.kv_quantize(v[b, :rows])
    assert want["kc"][slots - 1, S_max - 1].ne(
        before["kc"][slots - 1, S_max - 1]).any()      # the last row is hit
    got = {name: t.to(dev()) for name, t in before.items()}
    ops.kv_write_fp8(k.to(dev()), v.to(dev()), got["kc"], got["vc"],
                     got["ke"], got["ve"], _i32(slot_ids), _i32(starts),
                     _i32(lens))
    torch.cuda.synchronize()
    tag = f"kv_write_fp8 Hkv={Hkv} "
    assert_codes_equal(got["kc"], want["kc"], tag + "K codes")
    assert_codes_equal(got["vc"], want["vc"], tag + "V codes")
    assert torch.equal(got["ke"].cpu(), want["ke"]), tag + "K exponents"
    assert torch.equal(got["ve"].cpu(), want["ve"]), tag + "V exponents"
    # the special rows, by their known codes
    assert_codes_equal(got["kc"][slots - 1, starts[0], 0], tie_row()[1][0],
                       tag + "tie row")
    assert_codes_equal(got["kc"][slots - 1, starts[0] + 1:starts[0] + 3, 0],
                       all_code_rows(-20)[1], tag + "all-code rows")
    assert got["ke"][slots - 1, starts[0] + 1, 0].item() == 127 - 20
    assert got["ve"][slots - 1, starts[0] + 3, 0].item() == 127 + 9
    assert got["ve"][1, 40, 0].item() == 127                   # zero row


# ===========================================================================
# attn_decode_qkv_fp8.
# ===========================================================================
def e4m3_spacing(y):
    """Spacing of the e4m3fn grid at y >= 0: 2^-9 below 2^-6 (subnormals),
    else 2^(floor(log2 y) - 3)."""
    e = torch.floor(torch.log2(y.clamp(min=2.0 ** -6)))
    return 2.0 ** (e - 3)


@pytest.mark.parametrize("name,Hq,Hkv", ATTN_CASES)
def test_attn_decode_qkv_fp8_fp64(name, Hq, Hkv):
    C = ops.native()
    fc = fused_case(attn_case(name, Hq, Hkv))
    kc0, ke0 = quantize_poisoned(fc["kc"])
    vc0, ve0 = quantize_poisoned(fc["vc"])
    slot, pos = fc["slot_ids"].long(), fc["positions"].long()
    assert bool((kc0[slot, pos] == POISON_CODE).all())  # row p starts poisoned
    kc, vc, ke, ve = (t.to(dev()) for t in (kc0, vc0, ke0, ve0))
    out = C.attn_decode_qkv_fp8(
        to_gpu_bf16(fc["qkv"]), kc, vc, ke, ve, fc["cos"].to(dev()),
        fc["sin"].to(dev()), fc["positions"].to(dev()),
        fc["kv_lens"].to(dev()), fc["slot_ids"].to(dev()), Hq, Hkv, SCALE)
    torch.cuda.synchronize()
    kc, vc, ke, ve = kc.cpu(), vc.cpu(), ke.cpu(), ve.cpu()
    tag = f"attn_decode_qkv_fp8 {name} Hq={Hq} Hkv={Hkv}"
    group = Hq // Hkv

    # Output: attention over the dequantised cache as it is after the call,
    # rows 0..p.  Dequantisation is exact, so the bound is attn_tol itself.
    q64, Aq = rope64(fc["q"], fc["cos"], fc["sin"], fc["positions"])
    refs, tols = [], []
    for b, L in enumerate(fc["lens"]):
        s = int(slot[b])
        K = ops.kv_dequantize(kc[s, :L], ke[s, :L]).double()
        V = ops.kv_dequantize(vc[s, :L], ve[s, :L]).double()
        assert bool(torch.isfinite(K).all() and torch.isfinite(V).all())
        r, t = attn_rows64(q64[b], Aq[b], K, V)
        refs.append(r)
        tols.append(t)
        if L == 1:      # the current token alone: its dequantised v
            assert_bits_equal(out[b], V[0].bfloat16().repeat_interleave(
                group, dim=0), f"{tag} kv_len=1")
    ref, fp32 = torch.stack(refs), torch.stack(tols)
    check(tag, out, ref, attn_tol(ref, fp32))

    # Written V row: quantised from the raw bf16, no arithmetic before it.
    want_vc, want_ve = ops.kv_quantize(fc["cur_v"].bfloat16())
    assert_codes_equal(vc[slot, pos], want_vc, tag + " V row")
    assert torch.equal(ve[slot, pos], want_ve), tag + " V exponent"

    # Written K row: quantised from the kernel's fp32 rope.  Rope is a
    # 2-term sum, so each roped element, and with it amax, is within
    # tol_f32(A, K=2) of the fp64 value: the exponent may be that of any
    # amax in that interval.
    k64, Ak = rope64(fc["cur_k"], fc["cos"], fc["sin"], fc["positions"])
    t_k = tol_f32(Ak, K=2)
    amax = k64.abs().amax(-1)
    t_amax = t_k.amax(-1)
    e_got = ke[slot, pos]
    for b in range(amax.shape[0]):
        for h in range(Hkv):
            lo = exponent_by_definition(
                max(float(amax[b, h] - t_amax[b, h]), 0.0)) + 127
            hi = exponent_by_definition(
                float(amax[b, h] + t_amax[b, h])) + 127
            # amax == 0 has exponent 127 by definition, above that of
            # the tiny amax next to it: take the interval either way round
            assert min(lo, hi) <= int(e_got[b, h]) <= max(lo, hi), (
                tag, b, h, lo, hi, int(e_got[b, h]))
    # With the stored scale s every element is the nearest grid point of
    # the fp32 value: half a grid step at |k64| / s plus rope's error.
    s = 2.0 ** (e_got.double() - 127)[..., None]
    deq = ops.kv_dequantize(kc[slot, pos], e_got).double()
    assert bool(torch.isfinite(deq).all())
    check(tag + " K row", deq, k64,
          0.5 * e4m3_spacing(k64.abs() / s) * s + t_k)

    # Nothing else: every other code and exponent byte is as before.
    for nm, after, before in (("Kc", kc, kc0), ("Vc", vc, vc0),
                              ("Ke", ke, ke0), ("Ve", ve, ve0)):
        rest = after.clone()
        rest[slot, pos] = before[slot, pos]
        assert torch.equal(rest, before), f"{tag} untouched {nm}"


# ===========================================================================
# attn_append_fp8.
# ===========================================================================
SLOTS, S_MAX = 5, 200
# ends at S_MAX in the last slot; aligned full chunk; one row; a partial
# second q tile from an unaligned start; an empty sequence
RAGGED = dict(slots=[4, 0, 2, 1, 3], starts=[72, 0, 37, 100, 50],
              lens=[128, 128, 1, 65, 0])


@functools.lru_cache(maxsize=None)
def _append_case(Hq, Hkv):
    g = torch.Generator().manual_seed(300 + 10 * Hq + Hkv)
    slots, starts, lens = RAGGED["slots"], RAGGED["starts"], RAGGED["lens"]
    kv_lens = [min(s + l, S_MAX) if l else 0 for s, l in zip(starts, lens)]
    assert kv_lens[0] == S_MAX and slots[0] == SLOTS - 1 and S_MAX % 64
    kc = torch.full((SLOTS, S_MAX, Hkv, D), float("nan"))
    vc = torch.full((SLOTS, S_MAX, Hkv, D), float("nan"))
    for s, L in zip(slots, kv_lens):
        mult = 4.0 ** torch.randint(-2, 3, (L, Hkv, 1), generator=g).float()
        kc[s, :L] = torch.randn(L, Hkv, D, generator=g) * 0.5 * mult
        vc[s, :L] = torch.randn(L, Hkv, D, generator=g) * 0.5 * mult
    k8, ke = quantize_poisoned(kc)
    v8, ve = quantize_poisoned(vc)
    # the bf16 twin: the dequantised rows, NaN where the poison is
    dead = (ke == POISON_EXP)[..., None]
    kt = torch.where(dead, torch.tensor(float("nan")),
                     ops.kv_dequantize(k8, ke)).bfloat16()
    vt = torch.where(dead, torch.tensor(float("nan")),
                     ops.kv_dequantize(v8, ve)).bfloat16()
    live = ~dead.expand_as(kt)
    assert torch.equal(kt.float()[live], ops.kv_dequantize(k8, ke)[live])
    q = (torch.randn(len(lens), 128, Hq, D, generator=g) * 0.5).bfloat16()
    args = (_i32(slots), _i32(starts), _i32(lens), SCALE)
    out8 = ops.attn_append_fp8(q.to(dev()), k8.to(dev()), v8.to(dev()),
                               ke.to(dev()), ve.to(dev()), *args)
    out16 = ops.attn_append(q.to(dev()), kt.to(dev()), vt.to(dev()), *args)
    torch.cuda.synchronize()
    return out8.cpu(), out16.cpu()


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
def test_attn_append_fp8_is_attn_append_on_the_dequantised_cache(Hq, Hkv):
    out8, out16 = _append_case(Hq, Hkv)
    assert out8.shape == out16.shape and out8.dtype == torch.bfloat16
    assert bool(torch.isfinite(out8.float()).all())    # padding rows too
    for b, ln in enumerate(RAGGED["lens"]):
        assert_bits_equal(out8[b, :ln], out16[b, :ln],
                          f"attn_append_fp8 Hq={Hq} Hkv={Hkv} seq {b}")
    assert torch.count_nonzero(out8[4]) == 0            # the empty sequence


# ===========================================================================
# Bindings.
# ===========================================================================
def _fp8_args(B=2, Hq=4, Hkv=2, slots=3, S_max=8):
    a = _decode_args(B, Hq, Hkv, slots, S_max)
    a.update(Kc=_u8(slots, S_max, Hkv, D), Vc=_u8(slots, S_max, Hkv, D),
             Ke=_u8(slots, S_max, Hkv, fill=127),
             Ve=_u8(slots, S_max, Hkv, fill=127))
    return a


def _cache_rejections(op, call):
    """What every op checks of the four cache tensors (3 slots, 8 rows,
    2 kv heads in the baseline)."""
    wide = _u8(3, 8, 4, D)
    return {
        "Kc bf16": (op + "Kc must be Byte", call(Kc=_bf(3, 8, 2, D))),
        "Vc int8": (op + "Vc must be Byte",
                    call(Vc=torch.zeros(3, 8, 2, D, dtype=torch.int8,
                                        device=dev()))),
        "Kc on cpu": (op + "Kc must be on GPU",
                      call(Kc=torch.zeros(3, 8, 2, D, dtype=torch.uint8))),
        "Kc strided": (op + "Kc must be contiguous",
                       call(Kc=wide[:, :, :2], Vc=wide[:, :, 2:])),
        "Kc 3-D": (op + "Kc must be", call(Kc=_u8(3, 8, 2 * D))),
        "Kc head dim": (op + "Kc head dim must be 128",
                        call(Kc=_u8(3, 8, 2, 64), Vc=_u8(3, 8, 2, 64))),
        "Vc shape": (op + "Vc must have Kc's shape",
                     call(Vc=_u8(3, 9, 2, D))),
        "no rows": (op + "Kc must hold at least one slot and one row",
                    call(Kc=_u8(3, 0, 2, D), Vc=_u8(3, 0, 2, D),
                         Ke=_u8(3, 0, 2), Ve=_u8(3, 0, 2))),
        "Ke fp32": (op + "Ke must be Byte", call(Ke=_z(3, 8, 2))),
        "Ve on cpu": (op + "Ve must be on GPU",
                      call(Ve=torch.zeros(3, 8, 2, dtype=torch.uint8))),
        "Ke rows": (op + r"Ke must be \[slots, S_max, Hkv\]",
                    call(Ke=_u8(3, 9, 2))),
        "Ve 4-D": (op + r"Ve must be \[slots, S_max, Hkv\]",
                   call(Ve=_u8(3, 8, 2, 1))),
        "Ke strided": (op + "Ke must be contiguous",
                       call(Ke=_u8(3, 8, 4)[:, :, ::2])),
    }


def test_attn_decode_qkv_fp8_rejects_bad_inputs():
    C = ops.native()
    a = _fp8_args()

    def call(**kw):
        v = dict(a, **kw)
        return lambda: C.attn_decode_qkv_fp8(
            v["qkv"], v["Kc"], v["Vc"], v["Ke"], v["Ve"], v["cos"], v["sin"],
            v["positions"], v["kv_lens"], v["slot_ids"], v["Hq"], v["Hkv"],
            SCALE)

    call()()
    op = "attn_decode_qkv_fp8: "
    bad = _cache_rejections(op, call)
    bad.update({
        "qkv fp32": (op + "qkv must be BFloat16", call(qkv=_z(2, 8 * D))),
        "qkv width": (op + "qkv must be", call(qkv=_bf(2, 7 * D))),
        "qkv strided": (op + "qkv must be contiguous",
                        call(qkv=_bf(2, 16 * D)[:, ::2])),
        "Hq = 0": (op + "Hq = 0 and Hkv = 2 must be positive",
                   call(qkv=_bf(2, 4 * D), Hq=0)),
        "Hkv mismatch": (op + r"Hkv = 1 must equal Kc.size\(2\)",
                         call(qkv=_bf(2, 6 * D), Hkv=1)),
        "Hq % Hkv": (op + "Hq = 3 must be a positive multiple",
                     call(qkv=_bf(2, 7 * D), Hq=3)),
        "cos bf16": (op + "cos must be Float", call(cos=_bf(8, D // 2))),
        "sin width": (op + r"sin must be \[rows, 64\]", call(sin=_z(8, D))),
        "cos short": (op + "cos has 7 rows", call(cos=_z(7, D // 2))),
        "positions int64": (op + "positions must be Int",
                            call(positions=_z(2, dtype=torch.int64))),
        "kv_lens count": (op + r"kv_lens must be a \[B\]",
                          call(kv_lens=_z(1, dtype=torch.int32))),
        "slot_ids on cpu": (op + "slot_ids must be on GPU",
                            call(slot_ids=torch.zeros(2, dtype=torch.int32))),
    })
    _expect_rejections(bad)


def test_kv_write_fp8_rejects_bad_inputs():
    C = ops.native()
    a = _fp8_args()
    a.update(k=_bf(2, 4, 2, D), v=_bf(2, 4, 2, D),
             starts=_z(2, dtype=torch.int32), lens=_z(2, dtype=torch.int32))

    def call(**kw):
        v = dict(a, **kw)
        return lambda: C.kv_write_fp8(v["k"], v["v"], v["Kc"], v["Vc"],
                                      v["Ke"], v["Ve"], v["slot_ids"],
                                      v["starts"], v["lens"])

    call()()
    op = "kv_write_fp8: "
    bad = _cache_rejections(op, call)
    bad.update({
        "k fp32": (op + "k must be BFloat16", call(k=_z(2, 4, 2, D))),
        "v on cpu": (op + "v must be on GPU",
                     call(v=torch.zeros(2, 4, 2, D, dtype=torch.bfloat16))),
        "k 3-D": (op + r"k must be \[n, S, Hkv, 128\]",
                  call(k=_bf(2, 4, 2 * D))),
        "k head dim": (op + r"k must be \[n, S, Hkv, 128\]",
                       call(k=_bf(2, 4, 2, 64), v=_bf(2, 4, 2, 64))),
        "k strided": (op + "k must be contiguous",
                      call(k=_bf(2, 4, 4, D)[:, :, ::2])),
        "v shape": (op + "v must have k's shape", call(v=_bf(2, 5, 2, D))),
        "Hkv mismatch": (op + r"Hkv = 1 must equal Kc.size\(2\)",
                         call(k=_bf(2, 4, 1, D), v=_bf(2, 4, 1, D))),
        "slot_ids int64": (op + "slot_ids must be Int",
                           call(slot_ids=_z(2, dtype=torch.int64))),
        "starts count": (op + r"starts must be a \[B\]",
                         call(starts=_z(3, dtype=torch.int32))),
        "lens on cpu": (op + "lens must be on GPU",
                        call(lens=torch.zeros(2, dtype=torch.int32))),
    })
    _expect_rejections(bad)


def test_attn_append_fp8_rejects_bad_inputs():
    C = ops.native()
    a = _fp8_args()
    a.update(Q=_bf(2, 64, 4, D), q_start=_z(2, dtype=torch.int32),
             q_lens=_z(2, dtype=torch.int32))

    def call(**kw):
        v = dict(a, **kw)
        return lambda: C.attn_append_fp8(v["Q"], v["Kc"], v["Vc"], v["Ke"],
                                         v["Ve"], v["slot_ids"], v["q_start"],
                                         v["q_lens"], SCALE)

    assert torch.count_nonzero(call()()) == 0   # empty sequences: zeros
    op = "attn_append_fp8: "
    bad = _cache_rejections(op, call)
    bad.update({
        "Q fp16": (op + "Q must be BFloat16",
                   call(Q=_z(2, 64, 4, D, dtype=torch.float16))),
        "Q on cpu": (op + "Q must be on GPU",
                     call(Q=torch.zeros(2, 64, 4, D, dtype=torch.bfloat16))),
        "Q 3-D": (op + r"Q must be \[n, Sq, Hq, 128\]",
                  call(Q=_bf(2, 64, 4 * D))),
        "Q head dim": (op + r"Q must be \[n, Sq, Hq, 128\]",
                       call(Q=_bf(2, 64, 4, 64))),
        "Q strided": (op + "Q must be contiguous",
                      call(Q=_bf(2, 4, 64, D).transpose(1, 2))),
        "Sq 96": (op + "chunk length Sq must be a positive multiple of 64",
                  call(Q=_bf(2, 96, 4, D))),
        "Hq % Hkv": (op + "Hq = 3 must be a positive multiple",
                     call(Q=_bf(2, 64, 3, D))),
        "slot_ids int64": (op + "slot_ids must be Int",
                           call(slot_ids=_z(2, dtype=torch.int64))),
        "q_start count": (op + r"q_start must be a \[B\]",
                          call(q_start=_z(3, dtype=torch.int32))),
        "q_lens on cpu": (op + "q_lens must be on GPU",
                          call(q_lens=torch.zeros(2, dtype=torch.int32))),
    })
    _expect_rejections(bad)


def test_attn_decode_fp8_has_no_gpu_path():
    a = _fp8_args()
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.attn_decode_fp8(a["Q"], a["Kc"], a["Vc"], a["Ke"], a["Ve"],
                            a["kv_lens"], a["slot_ids"], SCALE)


# ===========================================================================
# Engine (debug model).
# ===========================================================================
@pytest.fixture(scope="module")
def debug_model():
    from skypilot_amd.models.llama import build_model
    return build_model("llama-debug", device="cuda:0")


def _generate(model, name="llama-debug", max_tokens=12, fp8_weights=False,
              **kw):
    from skypilot_amd.serve.engine import Engine, Request
    eng = Engine(name, device="cuda:0", max_seq=256, max_batch=4, model=model,
                 kv_dtype="fp8", **kw)
    if fp8_weights:
        assert eng.enable_fp8_decode() > 0
    plans = []
    eng._tp_bcast = plans.append
    req = eng.submit(Request(prompt_ids=list(PROMPT), max_tokens=max_tokens))
    eng.start()
    try:
        assert req.done.wait(120), "request did not complete"
    finally:
        eng.stop()
    return eng, req, plans


def test_engine_fp8_graph_and_eager_decode_agree(debug_model):
    eng_g, req_g, _ = _generate(debug_model, use_graphs=True)
    eng_e, req_e, _ = _generate(debug_model, use_graphs=False)
    assert eng_g.use_graphs and not eng_e.use_graphs
    assert eng_g.stats["graph_buckets"] == [1]
    assert len(req_g.out_ids) == 12
    assert req_g.out_ids == req_e.out_ids


def test_engine_fp8_chunked_prefill_cache_rows(debug_model):
    eng, req, plans = _generate(debug_model, prefill_chunk=64, max_tokens=4)
    assert len(req.out_ids) == 4
    appends = [p for p in plans if p["op"] == "append"]
    assert [p["lens"][0] for p in appends] == [64, 36]
    with torch.no_grad():
        check_prompt_rows(debug_model, eng.cache, appends[0]["slots"][0],
                          PROMPT, 64, device="cuda:0")


def test_engine_fp8_weights_with_fp8_cache():
    from skypilot_amd.models.llama import build_model
    model = build_model("llama-smoke", device="cuda:0")
    try:
        _, req, _ = _generate(model, name="llama-smoke", max_tokens=8,
                              fp8_weights=True)
    finally:
        ops.clear_fp8_weights()
    assert len(req.out_ids) == 8
    assert all(0 <= t < model.cfg.vocab_size for t in req.out_ids)


def test_tp_attention_decode_over_fp8_cache_matches_its_cpu_path():
    """TPAttention ropes q and k before the cache step, so on the GPU it
    runs the fused kernel with an identity rope row.  Same inputs through
    its CPU composition (write_decode + attn_decode_fp8): the written
    rows are equal to the bit (k * 1 - k' * 0 is exact) and the outputs
    agree within the bf16 output rounding of two fp32 evaluations."""
    from types import SimpleNamespace

    from skypilot_amd.models.llama import CONFIGS
    from skypilot_amd.parallel.tp import TPAttention
    from skypilot_amd.serve.engine import InferenceContext
    from skypilot_amd.serve.kv_cache import KVCache
    cfg = CONFIGS["llama-debug"]
    g = torch.Generator().manual_seed(77)
    B, lens, slots = 3, [1, 9, 40], [2, 0, 3]
    Hq, Hkv = cfg.num_heads, cfg.num_kv_heads
    q = torch.randn(B, 1, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, 1, Hkv, D, generator=g).bfloat16()
    v = torch.randn(B, 1, Hkv, D, generator=g).bfloat16()
    hist = [(torch.randn(L - 1, Hkv, D, generator=g).bfloat16(),
             torch.randn(L - 1, Hkv, D, generator=g).bfloat16())
            for L in lens]
    outs, caches = {}, {}
    for device in ("cpu", "cuda:0"):
        cache = KVCache(cfg, 4, 48, device, kv_dtype="fp8")
        for (hk, hv), s, L in zip(hist, slots, lens):
            cache.k[0][s, :L - 1], cache.k_exp[0][s, :L - 1] = (
                t.to(device) for t in ops.kv_quantize(hk))
            cache.v[0][s, :L - 1], cache.v_exp[0][s, :L - 1] = (
                t.to(device) for t in ops.kv_quantize(hv))
        pos = torch.tensor(lens, device=device) - 1
        ctx = InferenceContext(
            cache=cache, mode="decode",
            slots=torch.tensor(slots, device=device), pos=pos,
            kv_lens=torch.tensor(lens, dtype=torch.int32, device=device),
            slot_ids_i32=torch.tensor(slots, dtype=torch.int32,
                                      device=device))
        attn = SimpleNamespace(cfg=cfg, n_q=Hq, n_kv=Hkv, layer_idx=0,
                               scale=SCALE)
        outs[device] = TPAttention._decode_fp8(
            attn, q.to(device), k.to(device), v.to(device), ctx).cpu()
        caches[device] = cache
    for name in ("k", "v", "k_exp", "v_exp"):
        assert torch.equal(getattr(caches["cuda:0"], name)[0].cpu(),
                           getattr(caches["cpu"], name)[0]), name
    a, b = outs["cuda:0"].float().reshape(B, Hq, D), outs["cpu"].float()
    assert bool(((a - b).abs() <= 2 * 2.0 ** -8 * b.abs() + 1e-3).all()), (
        float((a - b).abs().max()))
