"""attn_append_kernel (attention_append.hip) on the GPU: ragged batches
over a NaN-poisoned slot cache against the CPU fp32 reference, against
the existing forward and decode kernels, the binding's rejections, and
the engine with prefill_chunk set.

Shapes are the smallest that cross every boundary of the kernel: two q
tiles (Sq = 128), S_max = 200 (no multiple of the 64-row kv tile), a
sequence that ends exactly at S_max in the last slot, unaligned starts,
a partial second q tile, a single row, an empty sequence."""
import functools

import pytest
import torch

from skypilot_amd import ops

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5
SLOTS, S_MAX = 5, 200


def dev():
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev())


def _poisoned_cache(g, Hkv, slots, kv_lens):
    """[SLOTS, S_MAX, Hkv, D] K and V on the CPU: random rows below each
    used slot's kv_len, NaN everywhere else (unused slots included)."""
    kc = torch.full((SLOTS, S_MAX, Hkv, D), float("nan")).bfloat16()
    vc = torch.full((SLOTS, S_MAX, Hkv, D), float("nan")).bfloat16()
    for s, L in zip(slots, kv_lens):
        kc[s, :L] = (torch.randn(L, Hkv, D, generator=g) * 0.5).bfloat16()
        vc[s, :L] = (torch.randn(L, Hkv, D, generator=g) * 0.5).bfloat16()
    return kc, vc


def _check_valid(out, ref, lens):
    for b, ln in enumerate(lens):
        if ln == 0:
            continue
        err = rel_err(out[b, :ln], ref[b, :ln])
        print(f"seq {b} q_len {ln}: rel_err {err:.3e}")
        assert err < 2e-2, (b, err)
        torch.testing.assert_close(out[b, :ln].float(), ref[b, :ln].float(),
                                   atol=0.05, rtol=0.05)


RAGGED = dict(slots=[4, 0, 2, 1], starts=[72, 0, 37, 100],
              lens=[128, 128, 1, 65])


@functools.lru_cache(maxsize=None)
def _ragged_case(Hq, Hkv):
    """Inputs, kernel output (on the CPU) and CPU reference of the ragged
    batch; computed once per head shape, read-only for the tests."""
    g = torch.Generator().manual_seed(100 * Hq + Hkv)
    slots, starts, lens = RAGGED["slots"], RAGGED["starts"], RAGGED["lens"]
    kv_lens = [min(s + l, S_MAX) for s, l in zip(starts, lens)]
    assert kv_lens[0] == S_MAX and slots[0] == SLOTS - 1
    kc, vc = _poisoned_cache(g, Hkv, slots, kv_lens)
    q = (torch.randn(4, 128, Hq, D, generator=g) * 0.5).bfloat16()
    ref = ops.attn_append_ref(q, kc, vc, slots, starts, lens, SCALE)
    qd, kcd, vcd = q.to(dev()), kc.to(dev()), vc.to(dev())
    out = ops.attn_append(qd, kcd, vcd, _i32(slots), _i32(starts),
                          _i32(lens), SCALE)
    torch.cuda.synchronize()
    return qd, kcd, vcd, out.cpu(), ref


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (2, 2)])
def test_ragged_batch_over_poisoned_cache(Hq, Hkv):
    _, _, _, out, ref = _ragged_case(Hq, Hkv)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    # padding rows included: nothing of the NaN rows may leak
    assert torch.isfinite(out.float()).all()
    _check_valid(out, ref, RAGGED["lens"])


def test_single_row_matches_decode_kernel():
    """The q_len = 1 sequence (start 37, slot 2) is one decode step."""
    qd, kcd, vcd, out, _ = _ragged_case(8, 2)
    # the decode kernel is not under test here: give it a clean cache
    dec = ops.attn_decode(qd[2, 0:1].contiguous(), torch.nan_to_num(kcd),
                          torch.nan_to_num(vcd), _i32([38]), _i32([2]),
                          SCALE)
    err = rel_err(out[2, 0], dec[0].cpu())
    print(f"append row vs decode kernel: rel_err {err:.3e}")
    assert err < 2e-2


def test_empty_sequence():
    g = torch.Generator().manual_seed(7)
    Hq, Hkv = 8, 2
    slots, starts, lens = [3, 1], [50, 10], [0, 64]
    kc, vc = _poisoned_cache(g, Hkv, slots, [0, 74])
    q = (torch.randn(2, 64, Hq, D, generator=g) * 0.5).bfloat16()
    ref = ops.attn_append_ref(q, kc, vc, slots, starts, lens, SCALE)
    out = ops.attn_append(q.to(dev()), kc.to(dev()), vc.to(dev()),
                          _i32(slots), _i32(starts), _i32(lens), SCALE).cpu()
    assert torch.isfinite(out.float()).all()
    _check_valid(out, ref, lens)


def test_matches_existing_forward():
    """q_start = 0, q_len = Sq = 192: the same work as ops.attention
    (S = 192 runs the 64-tile forward kernel) on the same K/V."""
    g = torch.Generator().manual_seed(8)
    n, S, Hq, Hkv = 2, 192, 8, 2
    slots = [3, 1]
    kc, vc = _poisoned_cache(g, Hkv, slots, [S, S])
    q = (torch.randn(n, S, Hq, D, generator=g) * 0.5).bfloat16().to(dev())
    kcd, vcd = kc.to(dev()), vc.to(dev())
    out = ops.attn_append(q, kcd, vcd, _i32(slots), _i32([0, 0]),
                          _i32([S, S]), SCALE)
    k = kcd[slots, :S].contiguous()
    v = vcd[slots, :S].contiguous()
    fwd = ops.attention(q, k, v, SCALE, causal=True)
    err = rel_err(out, fwd)
    print(f"append vs attention forward: rel_err {err:.3e}")
    assert err < 2e-2
    torch.testing.assert_close(out.float(), fwd.float(), atol=0.05,
                               rtol=0.05)


def _valid_args(n=2, Sq=64, Hq=4, Hkv=2, d=D):
    q = torch.zeros(n, Sq, Hq, d, dtype=torch.bfloat16, device=dev())
    kc = torch.zeros(3, 100, Hkv, d, dtype=torch.bfloat16, device=dev())
    vc = torch.zeros_like(kc)
    return dict(q=q, kc=kc, vc=vc, slot_ids=_i32([0, 1]),
                q_start=_i32([0, 0]), q_lens=_i32([64, 64]))


def _bad_non_gpu(name):
    def make():
        a = _valid_args()
        a[name] = a[name].cpu()
        return a
    return make


def _bad_dtype(name, dtype):
    def make():
        a = _valid_args()
        a[name] = a[name].to(dtype)
        return a
    return make


def _bad_non_contiguous(name):
    def make():
        a = _valid_args()
        t = a[name]
        a[name] = torch.zeros(t.shape[0], t.shape[2], t.shape[1], t.shape[3],
                              dtype=t.dtype, device=dev()).transpose(1, 2)
        assert not a[name].is_contiguous() and a[name].shape == t.shape
        return a
    return make


def _bad_head_dim():
    return _valid_args(d=64)


def _bad_sq():
    a = _valid_args(Sq=96)
    a["q_lens"] = _i32([64, 64])
    return a


def _bad_vc_shape():
    a = _valid_args()
    a["vc"] = torch.zeros(3, 101, 2, D, dtype=torch.bfloat16, device=dev())
    return a


def _bad_gqa():
    return _valid_args(Hq=3, Hkv=2)


def _bad_index_len(name):
    def make():
        a = _valid_args()
        a[name] = _i32([0, 0, 0])
        return a
    return make


REJECTIONS = {
    "q-not-on-gpu": _bad_non_gpu("q"),
    "kc-not-on-gpu": _bad_non_gpu("kc"),
    "vc-not-on-gpu": _bad_non_gpu("vc"),
    "q-not-bf16": _bad_dtype("q", torch.float16),
    "kc-not-bf16": _bad_dtype("kc", torch.float32),
    "vc-not-bf16": _bad_dtype("vc", torch.float16),
    "q-not-contiguous": _bad_non_contiguous("q"),
    "kc-not-contiguous": _bad_non_contiguous("kc"),
    "vc-not-contiguous": _bad_non_contiguous("vc"),
    "head-dim-64": _bad_head_dim,
    "sq-96": _bad_sq,
    "vc-shape": _bad_vc_shape,
    "hq-3-hkv-2": _bad_gqa,
    "slot-ids-int64": _bad_dtype("slot_ids", torch.int64),
    "q-start-int64": _bad_dtype("q_start", torch.int64),
    "q-lens-int64": _bad_dtype("q_lens", torch.int64),
    "slot-ids-not-on-gpu": _bad_non_gpu("slot_ids"),
    "q-start-not-on-gpu": _bad_non_gpu("q_start"),
    "q-lens-not-on-gpu": _bad_non_gpu("q_lens"),
    "slot-ids-length": _bad_index_len("slot_ids"),
    "q-start-length": _bad_index_len("q_start"),
    "q-lens-length": _bad_index_len("q_lens"),
}


def test_binding_accepts_the_valid_baseline():
    """The arguments every rejection case starts from do launch."""
    a = _valid_args()
    out = ops.native().attn_append(a["q"], a["kc"], a["vc"], a["slot_ids"],
                                   a["q_start"], a["q_lens"], SCALE)
    assert out.shape == a["q"].shape
    assert torch.count_nonzero(out) == 0  # V is all zeros


@pytest.mark.parametrize("case", sorted(REJECTIONS))
def test_binding_rejects(case):
    a = REJECTIONS[case]()
    with pytest.raises(RuntimeError, match="attn_append"):
        ops.native().attn_append(a["q"], a["kc"], a["vc"], a["slot_ids"],
                                 a["q_start"], a["q_lens"], SCALE)


def test_engine_chunked_prefill_gpu():
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine
    model = build_model("llama-smoke", device="cuda:0")
    prompt = [(7 * i + 3) % 4000 + 1 for i in range(150)]
    outs = {}
    for chunk in (None, 64):
        eng = Engine("llama-smoke", device="cuda:0", max_seq=256,
                     max_batch=4, prefill_chunk=chunk, model=model)
        eng.start()
        try:
            outs[chunk] = eng.generate(prompt, max_tokens=8)
        finally:
            eng.stop()
    matches = sum(a == b for a, b in zip(outs[64], outs[None]))
    print(f"chunked vs unchunked engine: {matches}/8 tokens equal")
    assert len(outs[64]) == 8
    assert matches >= 6, outs
