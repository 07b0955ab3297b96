"""Speculative decoding without a GPU: the drafter and the acceptance rule by
known answers, Engine(speculative=...)'s constructor checks, ops.attn_verify
against attn_append_ref, and the CPU engine end to end."""
import dataclasses

import pytest
import torch

from skypilot_amd import ops
from skypilot_amd.models.llama import CONFIGS, Llama, build_model
from skypilot_amd.serve.engine import Engine, Request
from skypilot_amd.serve.speculative import accept, ngram_draft

PROMPT = [(7 * i + 3) % 500 for i in range(20)]


@pytest.mark.parametrize("ids,k,want", [
    # the 3-gram (1 2 3) matches at 0; the 1-gram 3 also matches later
    ([1, 2, 3, 9, 8, 3, 7, 1, 2, 3], 2, [9, 8]),
    # most recent occurrence of (5 6): the one followed by 2
    ([5, 6, 1, 5, 6, 2, 4, 5, 6], 3, [2, 4, 5]),
    ([1, 2, 3, 4], 3, []),                 # nothing repeats
    ([4, 7, 4], 3, [7, 4]),                # match near the end: truncated
    ([3, 3], 4, [3]),
    ([1, 2, 1, 2], 0, []),
    ([9], 3, []),
], ids=["longest", "recent", "none", "truncated", "pair", "k0", "single"])
def test_ngram_draft(ids, k, want):
    assert ngram_draft(ids, k) == want


@pytest.mark.parametrize("draft,argmax,stop_id,room,want", [
    ([5, 6, 7], [1, 2, 3, 4], None, 9, [1]),            # none accepted
    ([5, 6, 7], [5, 6, 3, 4], None, 9, [5, 6, 3]),      # some
    ([5, 6, 7], [5, 6, 7, 4], None, 9, [5, 6, 7, 4]),   # all, plus one
    ([5, 6, 7], [5, 6, 7, 4], 6, 9, [5, 6]),            # stop inside the run
    ([5, 6, 7], [5, 6, 7, 4], None, 2, [5, 6]),         # max_tokens reached
    ([5], [5, 5, 5, 5], None, 9, [5, 5]),               # padding is not draft
    ([], [8, 8], None, 9, [8]),
], ids=["none", "some", "all", "stop", "room", "short", "empty"])
def test_accept(draft, argmax, stop_id, room, want):
    assert accept(draft, argmax, stop_id, room) == want


def test_constructor_rejections():
    def eng(**kw):
        return Engine("llama-debug", device="cpu", max_batch=2, **kw)
    for bad in (-1, 8, 2.0, True, "3"):
        with pytest.raises(ValueError, match="speculative must be an int"):
            eng(speculative=bad)
    with pytest.raises(ValueError, match="fp8 KV cache"):
        eng(speculative=2, kv_dtype="fp8")
    with pytest.raises(ValueError, match="tensor-parallel"):
        eng(speculative=2, tp_world=2)
    cfg = dataclasses.replace(CONFIGS["llama-debug"], num_heads=16,
                              num_kv_heads=1, hidden_size=256)
    model = Llama(cfg)
    with pytest.raises(ValueError, match=r"\(K \+ 1\) \* group = 48"):
        eng(speculative=2, model=model)
    eng(speculative=1, model=model)
    eng(model=model)


def test_attn_verify_cpu_is_attn_append_ref():
    g = torch.Generator().manual_seed(5)
    n, T, Hq, Hkv, S_max = 3, 4, 4, 2, 24
    q = torch.randn(n, T, Hq, 128, generator=g).bfloat16()
    kc = torch.randn(5, S_max, Hkv, 128, generator=g).bfloat16()
    vc = torch.randn(5, S_max, Hkv, 128, generator=g).bfloat16()
    slot = torch.tensor([4, 0, 2], dtype=torch.int32)
    start = torch.tensor([0, 7, S_max - T], dtype=torch.int32)
    got = ops.attn_verify(q, kc, vc, slot, start, 0.1)
    want = ops.attn_append_ref(q, kc, vc, slot, start,
                               torch.full((n,), T, dtype=torch.int32), 0.1)
    assert torch.equal(got, want)
    # token t sees rows <= start + t only
    kc[slot.long(), (start + T - 1).long()] = float("nan")
    again = ops.attn_verify(q, kc, vc, slot, start, 0.1)
    assert torch.equal(again[:, :T - 1], want[:, :T - 1])
    assert "attn_verify" in ops.__all__ and ops.VERIFY_MAX_COLS == 32


def _run(model, **kw):
    eng = Engine("llama-debug", device="cpu", max_seq=96, max_batch=2,
                 model=model, **kw)
    req = eng.submit(Request(prompt_ids=list(PROMPT), max_tokens=14))
    eng.start()
    try:
        assert req.done.wait(120), "request did not complete"
    finally:
        eng.stop()
    return req.out_ids, eng.stats


def test_engine_oracle_drafts_give_the_plain_tokens():
    """The bf16 debug model: on this prompt the 1-row and the 4-row CPU
    GEMMs pick the same tokens (the engine's bf16 cache takes no fp32
    model)."""
    model = build_model("llama-debug")
    want, _ = _run(model)
    full = PROMPT + want

    def oracle(ids, k):
        return full[len(ids):len(ids) + k]

    def wrong(ids, k):
        return [(t + 1) % 512 for t in oracle(ids, k)]

    got, stats = _run(model, speculative=3, drafter=oracle)
    assert len(want) == 14 and got == want
    assert stats["spec_accepted"] > 0 and stats["spec_steps"] < len(got)
    got, stats = _run(model, speculative=3, drafter=wrong)
    assert got == want
    assert stats["spec_accepted"] == 0 and stats["spec_steps"] > 0
