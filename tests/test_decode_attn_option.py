"""Engine(decode_attn=...) without a GPU: on the CPU the grouped ops are the
per-head compositions, so the tokens are the default's; bad values and
groups the kernel cannot take are rejected at construction."""
import dataclasses

import pytest

from skypilot_amd.models.llama import CONFIGS, Llama
from skypilot_amd.serve.engine import Engine, Request

PROMPT = [(7 * i + 3) % 500 for i in range(20)]


def _tokens(**kw):
    eng = Engine("llama-debug", device="cpu", max_seq=64, max_batch=2, **kw)
    req = eng.submit(Request(prompt_ids=list(PROMPT), max_tokens=6))
    eng.start()
    try:
        assert req.done.wait(120), "request did not complete"
    finally:
        eng.stop()
    return req.out_ids


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_grouped_generates_the_default_tokens(kv_dtype):
    import torch
    torch.manual_seed(0)
    want = _tokens(kv_dtype=kv_dtype)
    torch.manual_seed(0)
    got = _tokens(kv_dtype=kv_dtype, decode_attn="grouped")
    assert len(got) == 6 and got == want


def test_bad_value_raises():
    with pytest.raises(ValueError, match="decode_attn must be one of"):
        Engine("llama-debug", device="cpu", max_batch=2, decode_attn="gqa")


def test_group_above_16_raises():
    cfg = dataclasses.replace(CONFIGS["llama-debug"], num_heads=32,
                              num_kv_heads=1, hidden_size=256)
    model = Llama(cfg)
    with pytest.raises(ValueError, match="at most 16 q heads per kv head"):
        Engine("llama-debug", device="cpu", max_batch=2, model=model,
               decode_attn="grouped")
    Engine("llama-debug", device="cpu", max_batch=2, model=model)
