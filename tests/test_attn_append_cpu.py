"""Chunked prefill on the CPU reference path: ops.attn_append_ref against
the existing references, the model's append mode against its whole-prompt
prefill, and the engine with prefill_chunk set (scheduling, TP plan)."""
import pytest
import torch

from skypilot_amd import ops
from skypilot_amd.models.llama import build_model
from skypilot_amd.serve.engine import Engine, InferenceContext, Request
from skypilot_amd.serve.kv_cache import KVCache

D = 128
SCALE = D ** -0.5


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32)


def _rnd(g, *shape):
    return (torch.randn(*shape, generator=g) * 0.5).bfloat16()


def test_ref_matches_attention_ref():
    """q_start = 0, q_len = Sq: plain causal attention over the same K/V."""
    g = torch.Generator().manual_seed(0)
    n, S, Hq, Hkv = 2, 128, 4, 2
    q, k, v = _rnd(g, n, S, Hq, D), _rnd(g, n, S, Hkv, D), _rnd(g, n, S, Hkv, D)
    # slots used out of order, cache longer than the chunk, NaN behind it
    kc = torch.full((3, 200, Hkv, D), float("nan")).bfloat16()
    vc = torch.full((3, 200, Hkv, D), float("nan")).bfloat16()
    slots = [2, 0]
    for i, s in enumerate(slots):
        kc[s, :S], vc[s, :S] = k[i], v[i]
    out = ops.attn_append_ref(q, kc, vc, _i32(slots), _i32([0, 0]),
                              _i32([S, S]), SCALE)
    ref = ops.attention_ref(q, k, v, SCALE, causal=True)
    assert out.dtype == torch.bfloat16
    torch.testing.assert_close(out.float(), ref.float())
    # the public op is the reference on CPU
    out2 = ops.attn_append(q, kc, vc, _i32(slots), _i32([0, 0]),
                           _i32([S, S]), SCALE)
    assert torch.equal(out2, out)


def test_ref_matches_decode_ref():
    """q_len = 1 is one decode step with kv_lens = q_start + 1.  Both are
    fp32 evaluations of the same sums in different orders, rounded to
    bf16: they may land on neighbouring bf16 values (2^-8 relative), never
    further apart."""
    g = torch.Generator().manual_seed(1)
    n, Hq, Hkv, S_max = 3, 4, 2, 200
    kc, vc = _rnd(g, 4, S_max, Hkv, D), _rnd(g, 4, S_max, Hkv, D)
    q = _rnd(g, n, 64, Hq, D)
    slots, starts = [3, 1, 0], [37, 0, 199]
    out = ops.attn_append_ref(q, kc, vc, _i32(slots), _i32(starts),
                              _i32([1, 1, 1]), SCALE)
    dec = ops.attn_decode_ref(q[:, 0].contiguous(), kc, vc,
                              _i32([s + 1 for s in starts]), _i32(slots),
                              SCALE)
    torch.testing.assert_close(out[:, 0].float(), dec.float(),
                               rtol=2.0 ** -8, atol=1e-6)
    assert torch.count_nonzero(out[:, 1:]) == 0  # padding rows are zeros


def test_ref_ragged_masks_and_padding():
    """Unaligned start, partial chunk, empty sequence and a chunk that runs
    past S_max, against a per-row dense softmax."""
    g = torch.Generator().manual_seed(2)
    Hq, Hkv, S_max, Sq = 2, 1, 100, 64
    kc, vc = _rnd(g, 3, S_max, Hkv, D), _rnd(g, 3, S_max, Hkv, D)
    q = _rnd(g, 3, Sq, Hq, D)
    slots, starts, lens = [1, 2, 0], [37, 5, 90], [20, 0, 30]
    out = ops.attn_append_ref(q, kc, vc, _i32(slots), _i32(starts),
                              _i32(lens), SCALE)
    assert torch.isfinite(out.float()).all()
    assert torch.count_nonzero(out[0, 20:]) == 0
    assert torch.count_nonzero(out[1]) == 0
    for b, i in [(0, 0), (0, 19), (2, 0), (2, 9), (2, 29)]:
        hi = min(starts[b] + i + 1, min(starts[b] + lens[b], S_max))
        kk = kc[slots[b], :hi, 0].float()
        vv = vc[slots[b], :hi, 0].float()
        p = ((q[b, i].float() @ kk.T) * SCALE).softmax(-1)
        torch.testing.assert_close(out[b, i].float(),
                                   (p @ vv).bfloat16().float(),
                                   rtol=2.0 ** -8, atol=1e-6)


# ---------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def model():
    m = build_model("llama-debug", device="cpu")
    m.eval()
    return m


def _append_ctx(cache, slots, starts, lens):
    return InferenceContext(
        cache=cache, mode="append", append_slots=_i32(slots),
        append_start=_i32(starts), append_lens=_i32(lens),
        append_slots_l=slots, append_start_l=starts, append_lens_l=lens)


@torch.no_grad()
def test_model_append_chunks_match_prefill(model):
    cfg = model.cfg
    g = torch.Generator().manual_seed(3)
    L = 150
    prompt = torch.randint(1, cfg.vocab_size, (L,), generator=g)

    cache_a = KVCache(cfg, 2, 256, "cpu")
    pad = (L + 63) // 64 * 64
    toks = torch.zeros(1, pad, dtype=torch.long)
    toks[0, :L] = prompt
    ctx = InferenceContext(cache=cache_a, mode="prefill", prefill_slots=[1],
                           prefill_lens=[L])
    logits_a = model(toks, torch.arange(pad, dtype=torch.int32), ctx)[0, L - 1]

    cache_b = KVCache(cfg, 2, 256, "cpu")
    done = 0
    for ln in (64, 64, 22):
        toks = torch.zeros(1, 64, dtype=torch.long)
        toks[0, :ln] = prompt[done:done + ln]
        positions = (done + torch.arange(64, dtype=torch.int32)).clamp(
            max=cfg.max_seq_len - 1)
        out = model(toks, positions, _append_ctx(cache_b, [1], [done], [ln]))
        assert out.shape == (1, 1, cfg.vocab_size)
        done += ln
    logits_b = out[0, 0]

    err = rel_err(logits_b, logits_a)
    print(f"last-row logits rel_err {err:.3e}")
    assert err < 2e-2
    assert torch.equal(cache_b.k[0][1, :L], cache_a.k[0][1, :L])
    assert torch.equal(cache_b.v[0][1, :L], cache_a.v[0][1, :L])
    for layer in range(cfg.num_layers):
        for a, b in ((cache_a.k, cache_b.k), (cache_a.v, cache_b.v)):
            torch.testing.assert_close(b[layer][1, :L].float(),
                                       a[layer][1, :L].float(),
                                       atol=0.05, rtol=0.05)
    # the other slot was never written
    assert torch.count_nonzero(cache_b.k[0][0]) == 0


# --------------------------------------------------------------- engine level
def _greedy_no_cache(model, prompt_ids, n):
    ids = list(prompt_ids)
    for _ in range(n):
        logits = model(torch.tensor([ids]))
        ids.append(int(logits[0, -1].argmax()))
    return ids[len(prompt_ids):]


LONG = [(7 * i + 3) % 500 + 1 for i in range(150)]
SHORT = [[2, 4, 6], [10, 20, 30, 40], [7]]


def _run_all(eng, prompts, max_tokens):
    reqs = [Request(prompt_ids=list(p), max_tokens=max_tokens)
            for p in prompts]
    for r in reqs:  # all queued before the loop starts: one admission
        eng.submit(r)
    eng.start()
    try:
        for r in reqs:
            assert r.done.wait(120), "request did not complete"
    finally:
        eng.stop()
    return reqs


@pytest.fixture(scope="module")
def chunked_run(model):
    """One chunked engine run shared by the tests below: the leader's TP
    plans are collected on the way."""
    eng = Engine("llama-debug", device="cpu", max_seq=256, max_batch=4,
                 prefill_chunk=64, model=model)
    plans = []
    eng._tp_bcast = plans.append
    reqs = _run_all(eng, [LONG] + SHORT, 8)
    return eng, reqs, plans


def test_engine_chunked_prefill(chunked_run, model):
    eng, reqs, plans = chunked_run
    assert all(len(r.out_ids) == 8 for r in reqs)
    assert not eng.prefilling and not eng.active
    assert sorted(eng.free_slots) == [0, 1, 2, 3]
    for r, p in zip(reqs[1:], SHORT):
        assert r.out_ids == _greedy_no_cache(model, p, 8), p
    plain = Engine("llama-debug", device="cpu", max_seq=256, max_batch=4,
                   model=model)
    ref = _run_all(plain, [LONG], 8)[0].out_ids
    matches = sum(a == b for a, b in zip(reqs[0].out_ids, ref))
    print(f"long prompt: {matches}/8 tokens equal the unchunked engine's")
    assert matches >= 6, (reqs[0].out_ids, ref)
    # the long prompt went through in 64 / 64 / 22
    appends = [p for p in plans if p["op"] == "append"]
    assert [p["lens"][0] for p in appends] == [64, 64, 22]
    assert [p["starts"][0] for p in appends] == [0, 64, 128]
    # short prompts finished in the first chunk; the long one did not
    # hold them back: they decoded while it was still prefilling
    first_decode = next(i for i, p in enumerate(plans) if p["op"] == "decode")
    last_append = max(i for i, p in enumerate(plans) if p["op"] == "append")
    assert first_decode < last_append
    assert reqs[1].first_token_at <= reqs[0].first_token_at


def test_engine_rejects_bad_prefill_chunk():
    for bad in (100, 0, -64, 64.0):
        with pytest.raises(ValueError):
            Engine("llama-debug", device="cpu", max_seq=256, max_batch=4,
                   prefill_chunk=bad)


def test_follower_replays_append_plans(chunked_run, model):
    """A TP follower fed the leader's "append" plans ends with the same
    cache rows (the followers keep no scheduler state)."""
    lead, _, plans = chunked_run
    fol = Engine("llama-debug", device="cpu", max_seq=256, max_batch=4,
                 prefill_chunk=64, model=model)
    used = {}  # slot -> prompt length; decode rows come after it
    for p in plans:
        if p["op"] != "append":
            continue
        fol._follow_append(p)
        for s, st, ln in zip(p["slots"], p["starts"], p["lens"]):
            used[s] = max(used.get(s, 0), st + ln)
    assert sorted(used.values()) == [1, 3, 4, 150]
    for slot, ln in used.items():
        for layer in range(model.cfg.num_layers):
            assert torch.equal(fol.cache.k[layer][slot, :ln],
                               lead.cache.k[layer][slot, :ln])
            assert torch.equal(fol.cache.v[layer][slot, :ln],
                               lead.cache.v[layer][slot, :ln])
            assert torch.count_nonzero(fol.cache.k[layer][slot, :ln]) > 0
