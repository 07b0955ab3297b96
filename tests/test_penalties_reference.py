"""Decode penalties off the GPU: ops.penalize_logits_reference on rows
worked out by hand, the engine's and the API's validation, and a CPU
engine whose hist holds every token by position (docs/KERNELS.md "Decode
penalties")."""
import pytest
import torch

from skypilot_amd import ops
from skypilot_amd.serve.engine import Engine, Request

NEG_INF = float("-inf")


def _ref(logits, hist, tok, pos, P, alpha, beta, rho, slot=0):
    return ops.penalize_logits_reference(
        torch.tensor([logits]).bfloat16(), hist, [tok], [pos], [slot], [P],
        [alpha], [beta], [rho])


def test_reference_hand_computed_row():
    # positions 0..4: prompt [1, 2], generated [3, 3], input token 1 at p=4
    hist = torch.tensor([[1, 2, 3, 3, 9, 5, 5]], dtype=torch.int32)
    l = [4.0, 2.0, -2.0, 1.0, 0.0, 8.0, NEG_INF]
    value, seen, count = _ref(l, hist, tok=1, pos=4, P=2, alpha=0.5,
                              beta=0.25, rho=2.0)
    assert hist.tolist() == [[1, 2, 3, 3, 1, 5, 5]]     # recorded at [0, 4]
    assert seen[0].tolist() == [False, True, True, True, False, False, False]
    assert count[0].tolist() == [0, 1, 0, 2, 0, 0, 0]
    assert value[0].tolist() == [
        4.0,                        # unseen
        2.0 / 2 - 0.25 - 0.5,       # prompt and generated once: all three
        -2.0 * 2,                   # prompt only, negative: rho only
        1.0 / 2 - 2 * 0.25 - 0.5,   # generated twice
        0.0, 8.0, NEG_INF]          # unseen; 5 lies past p and is stale


@pytest.mark.parametrize("l, want", [(3.0, 1.5), (-3.0, -6.0), (0.0, 0.0),
                                     (NEG_INF, NEG_INF)])
def test_reference_repetition_by_sign(l, want):
    hist = torch.zeros(1, 4, dtype=torch.int32)
    value, seen, _ = _ref([l, 7.0], hist, tok=0, pos=0, P=1, alpha=0.0,
                          beta=0.0, rho=2.0)
    assert seen[0].tolist() == [True, False]
    assert value[0].tolist() == [want, 7.0]


def test_reference_neg_inf_generated_token_and_clamped_prompt_len():
    hist = torch.zeros(1, 4, dtype=torch.int32)
    value, _, count = _ref([NEG_INF, 1.0], hist, tok=0, pos=1, P=0,
                           alpha=1.0, beta=1.0, rho=1.0)
    assert count[0].tolist() == [2, 0] and value[0].tolist() == [NEG_INF, 1.0]
    _, seen, count = _ref([1.0, 1.0], hist, tok=0, pos=1, P=6, alpha=1.0,
                          beta=1.0, rho=1.0)      # P clamps to p + 1 = 2
    assert count[0].tolist() == [0, 0] and seen[0].tolist() == [True, False]


@pytest.mark.parametrize("kw", [
    dict(alpha=0.0, beta=0.0, rho=1.0),             # off
    dict(alpha=1.0, beta=0.0, rho=1.0, slot=1),     # slot outside hist
    dict(alpha=1.0, beta=0.0, rho=1.0, pos=4),      # position outside hist
])
def test_reference_off_rows_leave_hist_alone(kw):
    hist = torch.full((1, 4), 1, dtype=torch.int32)
    kw = {"pos": 2, **kw}
    value, seen, _ = _ref([1.0, 2.0], hist, tok=0, P=0, **kw)
    assert not seen.any() and value[0].tolist() == [1.0, 2.0]
    assert hist.tolist() == [[1, 1, 1, 1]]


def test_cpu_op_is_the_reference_rounded_to_bf16():
    hist = torch.tensor([[1, 1, 0]], dtype=torch.int32)
    logits = torch.tensor([[1.0, 3.0, 5.0]]).bfloat16()
    out = torch.empty_like(logits)
    idx = torch.tensor([[1], [2], [0], [0]], dtype=torch.int32)
    par = torch.tensor([[0.0], [0.1], [1.0]])
    ops.penalize_logits(logits, out, hist, None, *idx, *par)
    want = torch.tensor([[1.0, 3.0 - 3 * float(par[1, 0]), 5.0]]).bfloat16()
    assert torch.equal(out, want) and hist.tolist() == [[1, 1, 1]]


def _engine(**kw):
    return Engine("llama-debug", device="cpu", max_seq=256, max_batch=4, **kw)


@pytest.mark.parametrize("kw", [dict(presence_penalty=0.5),
                                dict(frequency_penalty=-0.5),
                                dict(repetition_penalty=1.1)])
def test_submit_rejects_penalties_when_off(kw):
    with pytest.raises(ValueError, match="--penalties"):
        _engine().submit(Request(prompt_ids=[1, 2], **kw))


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0),
                                dict(presence_penalty=float("nan")),
                                dict(frequency_penalty=float("inf")),
                                dict(presence_penalty="1"),
                                dict(frequency_penalty=True)])
def test_submit_rejects_bad_values(kw):
    with pytest.raises(ValueError, match="_penalty"):
        _engine(penalties=True).submit(Request(prompt_ids=[1, 2], **kw))


@pytest.mark.parametrize("prefill_chunk", [None, 64])
def test_cpu_engine_keeps_every_token_in_hist(prefill_chunk):
    prompt = [(7 * i) % 500 for i in range(70)]
    eng = _engine(penalties=True, prefill_chunk=prefill_chunk)
    plain = _engine()       # same seed, same weights
    reqs = [Request(prompt_ids=list(prompt), max_tokens=12,
                    frequency_penalty=1.5, repetition_penalty=1.3),
            Request(prompt_ids=list(prompt), max_tokens=12)]
    for e, r in ((eng, reqs[0]), (plain, reqs[1])):
        e.submit(r)
        e.start()
        try:
            assert r.done.wait(120)
        finally:
            e.stop()
    pen, raw = (r.out_ids for r in reqs)
    assert len(pen) == 12 and pen != raw     # the penalties changed tokens
    want = prompt + pen[:-1]
    rows = [h[:len(want)].tolist() for h in eng.hist]
    assert rows.count(want) == 1             # the request's slot


@pytest.fixture(scope="module")
def clients():
    from fastapi.testclient import TestClient
    from skypilot_amd.serve.entrypoint import create_app
    on, off = _engine(penalties=True), _engine()
    on.start()
    off.start()
    with TestClient(create_app(on, "llama-debug")) as a, \
            TestClient(create_app(off, "llama-debug")) as b:
        yield a, b
    on.stop()
    off.stop()


def _post(c, chat, **body):
    if chat:
        return c.post("/v1/chat/completions", json={
            "messages": [{"role": "user", "content": "aaaa"}],
            "max_tokens": 3, **body})
    return c.post("/v1/completions",
                  json={"prompt": "aaaa", "max_tokens": 3, **body})


@pytest.mark.parametrize("chat", [False, True])
def test_api_fields(clients, chat):
    on, off = clients
    ok = dict(presence_penalty=-2.0, frequency_penalty=2.0,
              repetition_penalty=1.2)
    assert _post(on, chat, **ok).status_code == 200
    for bad in (dict(presence_penalty=2.5), dict(frequency_penalty=-2.5),
                dict(repetition_penalty=0.0), dict(presence_penalty="x")):
        assert _post(on, chat, **bad).status_code == 422
    r = _post(off, chat, frequency_penalty=0.5)
    assert r.status_code == 400 and "--penalties" in r.json()["detail"]
    assert _post(off, chat, presence_penalty=0.0).status_code == 200
