"""CPU tests of token log-probabilities: the fp64 reference of the
definition (ops.token_logprobs_reference), the engine's eager paths on
llama-debug, and the OpenAI API fields.  The tolerance and its derivation
are in _logprobs_cases.py."""
import math

import pytest
import torch

import _fp64_check as fc
import _logprobs_cases as lc
from skypilot_amd import ops
from skypilot_amd.serve.engine import Engine, InferenceContext, Request

TOP = lc.TOP
NEG_INF = float("-inf")


# ------------------------------ reference ----------------------------------
@pytest.mark.parametrize("scale", [1.0, 16.0])
@pytest.mark.parametrize("n,V", [(1, 1), (3, 7), (2, 513), (3, 4099),
                                 (1, 128256)])
def test_reference_against_log_softmax(n, V, scale):
    logits = lc.make_rows(n, V, scale, seed=V)
    ids = lc.make_ids(n, V, seed=V + 1)
    lp, top_lp, top_ids = ops.token_logprobs(logits, ids, 20)
    assert lp.dtype == torch.float32 and top_lp.dtype == torch.float32
    assert top_ids.dtype == torch.int32
    assert top_lp.shape == top_ids.shape == (n, TOP)
    lc.check_lp("chosen", lp, lc.plain_reference(logits, ids), V)
    k = min(20, V)
    ls = torch.log_softmax(logits.double(), -1)
    lc.check_lp("top", top_lp[:, :k], ls.gather(1, top_ids[:, :k].long()), V)
    assert torch.isnan(top_lp[:, k:]).all() and (top_ids[:, k:] == -1).all()
    # the negative control
    good = lc.plain_reference(logits, ids)
    for wrong in lc.broken_references(logits, ids):
        keep = torch.isfinite(wrong) & (wrong != good)
        if bool(keep.any()):
            assert fc.rejects(lp[keep], wrong[keep], lc.tol(wrong[keep], V))


@pytest.mark.parametrize("V", [7, 513, 128256])
def test_top_order_is_a_stable_sort(V):
    logits = lc.make_rows(2, V, 1.0, seed=V + 9)
    for N in (1, 5, 20):
        _, _, top_ids = lc.ref(logits, [0, 0], N)
        for i in range(2):
            vals = logits[i].double().tolist()
            want = sorted(range(V), key=lambda j: (-vals[j], j))[:N]
            assert top_ids[i, :len(want)].tolist() == want
            assert (top_ids[i, len(want):] == -1).all()


def test_ties_straddling_the_cut():
    row, top3, ties = lc.tie_block_row(128256)
    for N in (5, 20):
        _, top_lp, top_ids = lc.ref(row[None], [0], N)
        assert top_ids[0, :N].tolist() == top3 + ties[:N - 3]
        assert len(set(top_lp[0, 3:N].tolist())) == 1
    # -0 and +0 are one value: index order decides
    z = torch.tensor([[0.0, -0.0, 1.0, -0.0, 0.0]]).bfloat16()
    assert lc.ref(z, [0], 4)[2][0, :4].tolist() == [2, 0, 1, 3]


def test_all_equal_row():
    V = 1000
    logits = torch.full((1, V), -2.5).bfloat16()
    lp, top_lp, top_ids = lc.ref(logits, [V - 1], 20)
    assert top_ids[0].tolist() == list(range(20))
    want = torch.full((1,), -math.log(V), dtype=torch.float64)
    lc.check_lp("all-equal", lp, want, V)
    assert (top_lp[0] == lp[0]).all()


def test_n_top_edges():
    logits = lc.make_rows(4, 7, 1.0, seed=1)
    ids = [0, 6, 3, 3]
    lp, top_lp, top_ids = lc.ref(logits, ids, [0, 20, 1000, -1])
    assert torch.isfinite(lp[:3]).all() and math.isnan(float(lp[3]))
    assert (top_ids[0] == -1).all() and torch.isnan(top_lp[0]).all()
    for i in (1, 2):                       # N >= V; above 20 counts as 20
        assert sorted(top_ids[i, :7].tolist()) == list(range(7))
        assert (top_ids[i, 7:] == -1).all()
        assert abs(float(top_lp[i, :7].double().exp().sum()) - 1) < 1e-6
    assert (top_ids[3] == -1).all() and torch.isnan(top_lp[3]).all()
    # scalar and per-row n_top agree
    a = lc.ref(logits, ids, 5)
    b = lc.ref(logits, ids, [5, 5, 5, 5])
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in zip(a, b))


def test_neg_inf_logits():
    V = 513
    logits = torch.full((1, V), NEG_INF).bfloat16()
    logits[0, [500, 2, 257, 64]] = torch.tensor(
        [0.5, 2.0, -1.0, 0.5]).bfloat16()
    lp, top_lp, top_ids = lc.ref(logits, [7], 20)
    assert float(lp[0]) == NEG_INF
    assert top_ids[0].tolist() == [2, 64, 500, 257] + [
        j for j in range(18) if j != 2][:16]
    assert torch.isfinite(top_lp[0, :4]).all()
    assert (top_lp[0, 4:] == NEG_INF).all()


def test_degenerate_rows_and_ids_outside():
    V = 64
    logits = lc.make_rows(6, V, 1.0, seed=4)
    logits[1, 63] = float("nan")
    logits[2, 0] = float("inf")
    logits[3] = NEG_INF
    ids = [5, 5, 0, 5, -1, V]
    lp, top_lp, top_ids = lc.ref(logits, ids, 5)
    assert math.isfinite(float(lp[0]))
    for i in (1, 2, 3):
        assert math.isnan(float(lp[i]))
        assert torch.isnan(top_lp[i]).all() and (top_ids[i] == -1).all()
    for i in (4, 5):                       # id outside [0, V)
        assert math.isnan(float(lp[i]))
        assert (top_ids[i, :5] >= 0).all()
        assert torch.isfinite(top_lp[i, :5]).all()


# ------------------------------- engine ------------------------------------
PROMPT = [(37 * i + 11) % 500 + 1 for i in range(150)]   # 64 + 64 + 22
MAX_TOKENS = 5
V_DEBUG = 512


def _engine(**kw):
    return Engine("llama-debug", device="cpu", max_seq=256, max_batch=4, **kw)


def _run(eng, *reqs):
    for r in reqs:
        eng.submit(r)
    eng.start()
    try:
        for r in reqs:
            assert r.done.wait(120)
    finally:
        eng.stop()
    return reqs


@torch.no_grad()
def _engine_logits(prefill_chunk, out_ids, all_rows):
    """The forwards the engine ran for PROMPT and then `out_ids`, rebuilt
    on a second engine with the same weights: the logits [L + T - 1, V]
    of every prompt position and of every fed-back token but the last."""
    eng = _engine(prefill_chunk=prefill_chunk)
    L, slot = len(PROMPT), 3
    if prefill_chunk is None:
        pad = (L + 63) // 64 * 64
        toks = torch.zeros(1, pad, dtype=torch.long)
        toks[0, :L] = torch.tensor(PROMPT)
        ctx = InferenceContext(cache=eng.cache, mode="prefill",
                               prefill_slots=[slot], prefill_lens=[L])
        rows = [eng.model(toks, torch.arange(pad, dtype=torch.int32),
                          ctx)[0, :L]]
    else:
        rows = []
        for s in range(0, L, prefill_chunk):
            n = min(prefill_chunk, L - s)
            lg = eng._append_forward([slot], [s], [n], [PROMPT[s:s + n]],
                                     all_rows)
            rows.append(lg[0, :n] if all_rows else lg[0])
    for t, tok in enumerate(out_ids[:-1]):
        at = torch.tensor([L + t])
        ctx = InferenceContext(
            cache=eng.cache, mode="decode", slots=torch.tensor([slot]),
            pos=at, kv_lens=(at + 1).int(),
            slot_ids_i32=torch.tensor([slot], dtype=torch.int32))
        rows.append(eng.model(torch.tensor([[tok]]), at.int(), ctx)[0])
    return torch.cat(rows)


@pytest.mark.parametrize("prefill_chunk", [None, 64])
def test_engine_logprobs_match_its_own_logits(prefill_chunk):
    (plain,) = _run(_engine(prefill_chunk=prefill_chunk),
                    Request(prompt_ids=list(PROMPT), max_tokens=MAX_TOKENS))
    # one request per engine: the rebuilt forwards have batch 1 too
    (both,) = _run(
        _engine(prefill_chunk=prefill_chunk, max_logprobs=5),
        Request(prompt_ids=list(PROMPT), max_tokens=MAX_TOKENS, logprobs=5,
                prompt_logprobs=True))
    (gen_only,) = _run(
        _engine(prefill_chunk=prefill_chunk, max_logprobs=5),
        Request(prompt_ids=list(PROMPT), max_tokens=MAX_TOKENS, logprobs=0))
    assert plain.out_logprobs == [] and plain.prompt_lps == []
    assert both.out_ids == plain.out_ids == gen_only.out_ids
    assert len(both.out_ids) == MAX_TOKENS
    assert gen_only.prompt_lps == []
    assert all(top == [] for top in gen_only.out_top)
    assert len(gen_only.out_logprobs) == MAX_TOKENS

    L = len(PROMPT)
    logits = _engine_logits(prefill_chunk, both.out_ids, all_rows=True)
    assert logits.dtype == torch.bfloat16 and logits.shape[0] == L + 4
    ls = torch.log_softmax(logits.double(), -1)
    # prompt: position i under the logits of position i - 1
    assert both.prompt_lps[0] is None and len(both.prompt_lps) == L
    want = ls[torch.arange(L - 1), torch.tensor(PROMPT[1:])]
    lc.check_lp("prompt_lps", torch.tensor(both.prompt_lps[1:]), want,
                V_DEBUG)
    # generated tokens
    assert len(both.out_logprobs) == len(both.out_top) == MAX_TOKENS
    want = ls[torch.arange(L - 1, L + 4), torch.tensor(both.out_ids)]
    lc.check_lp("out_logprobs", torch.tensor(both.out_logprobs), want,
                V_DEBUG)
    for t, (tok, lp, top) in enumerate(zip(both.out_ids, both.out_logprobs,
                                           both.out_top)):
        assert len(top) == 5
        assert top[0] == (tok, lp)              # greedy: the top-1 id
        vals = logits[L - 1 + t].double().tolist()
        assert [j for j, _ in top] == sorted(
            range(V_DEBUG), key=lambda j: (-vals[j], j))[:5]
    # the request that only scores its output went through the gathered
    # last-row forward when chunked
    logits = _engine_logits(prefill_chunk, gen_only.out_ids, all_rows=False)
    ls = torch.log_softmax(logits[-MAX_TOKENS:].double(), -1)
    want = ls[torch.arange(MAX_TOKENS), torch.tensor(gen_only.out_ids)]
    lc.check_lp("out_logprobs, gathered", torch.tensor(gen_only.out_logprobs),
                want, V_DEBUG)


def test_engine_sampled_request_reports_raw_distribution():
    """Host-sampled tokens: the log-probability is that of the sampled
    token at temperature 1, and the alternatives are the raw top."""
    (r,) = _run(_engine(max_logprobs=3),
                Request(prompt_ids=[5, 6, 7], max_tokens=6, temperature=1.5,
                        logprobs=3))
    assert len(r.out_logprobs) == len(r.out_top) == 6
    for tok, lp, top in zip(r.out_ids, r.out_logprobs, r.out_top):
        assert len(top) == 3 and lp <= top[0][1]
        assert all(v == lp for t, v in top if t == tok)


def test_engine_rejects():
    for bad in (-1, 21, True, 2.0, None):
        with pytest.raises(ValueError, match="max_logprobs"):
            _engine(max_logprobs=bad)
    off = _engine()
    for kw in (dict(logprobs=0), dict(logprobs=3),
               dict(prompt_logprobs=True)):
        with pytest.raises(ValueError, match="max-logprobs"):
            off.submit(Request(prompt_ids=[1, 2], **kw))
    on = _engine(max_logprobs=5)
    with pytest.raises(ValueError, match="exceeds"):
        on.submit(Request(prompt_ids=[1, 2], logprobs=6))
    for bad in (-1, True, 1.5):
        with pytest.raises(ValueError, match="logprobs"):
            on.submit(Request(prompt_ids=[1, 2], logprobs=bad))
    on.submit(Request(prompt_ids=[1, 2], logprobs=5))
    assert on.pending.qsize() == 1 and off.pending.qsize() == 0


def test_truncated_prompt_is_the_one_scored():
    eng = Engine("llama-debug", device="cpu", max_seq=64, max_batch=2,
                 max_logprobs=1)
    (r,) = _run(eng, Request(prompt_ids=[(3 * i) % 500 for i in range(100)],
                             max_tokens=4, logprobs=0, prompt_logprobs=True))
    assert len(r.prompt_ids) < 64
    assert len(r.prompt_lps) == len(r.prompt_ids)
    assert r.prompt_lps[0] is None
    assert all(math.isfinite(v) for v in r.prompt_lps[1:])


# -------------------------------- API --------------------------------------
@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient
    from skypilot_amd.serve.entrypoint import create_app
    eng = _engine(max_logprobs=5)
    eng.start()
    with TestClient(create_app(eng, "llama-debug")) as c:
        yield c
    eng.stop()


def _check_completion_logprobs(lp, n, n_top):
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs",
                       "text_offset"}
    assert all(len(lp[k]) == n for k in lp)
    assert all(isinstance(t, str) for t in lp["tokens"])
    assert lp["text_offset"] == sorted(lp["text_offset"])
    for tok, v, top in zip(lp["tokens"], lp["token_logprobs"],
                           lp["top_logprobs"]):
        if top is None:
            continue
        assert len(top) == n_top and v <= 0
        assert list(top.values()) == sorted(top.values(), reverse=True)
        if tok in top:
            assert top[tok] == v


def test_api_completions(client):
    body = {"prompt": "hello", "max_tokens": 6}
    plain = client.post("/v1/completions", json=body).json()
    assert "logprobs" not in plain["choices"][0]
    r = client.post("/v1/completions", json={**body, "logprobs": 2}).json()
    ch = r["choices"][0]
    assert ch["text"] == plain["choices"][0]["text"]
    _check_completion_logprobs(ch["logprobs"], 6, 2)
    assert ch["logprobs"]["text_offset"][0] == 0
    # greedy: the chosen token leads its alternatives
    for tok, top in zip(ch["logprobs"]["tokens"],
                        ch["logprobs"]["top_logprobs"]):
        assert next(iter(top)) == tok
    r0 = client.post("/v1/completions", json={**body, "logprobs": 0}).json()
    assert r0["choices"][0]["logprobs"]["top_logprobs"] == [{}] * 6
    assert (r0["choices"][0]["logprobs"]["token_logprobs"]
            == ch["logprobs"]["token_logprobs"])


def test_api_echo(client):
    body = {"prompt": "hello", "max_tokens": 4, "echo": True}
    r = client.post("/v1/completions", json={**body, "logprobs": 1}).json()
    ch = r["choices"][0]
    n_prompt = r["usage"]["prompt_tokens"]
    assert n_prompt == 6 and ch["text"].startswith("hello")
    lp = ch["logprobs"]
    _check_completion_logprobs(lp, n_prompt + 4, 1)
    assert lp["token_logprobs"][0] is None
    assert all(v is not None and v <= 0 for v in lp["token_logprobs"][1:])
    assert lp["tokens"][1:6] == list("hello")
    assert lp["top_logprobs"][:n_prompt] == [None] * n_prompt
    assert lp["text_offset"][1:7] == [0, 1, 2, 3, 4, 5]
    # echo without logprobs only prefixes the text
    r = client.post("/v1/completions", json=body).json()
    assert r["choices"][0]["text"].startswith("hello")
    assert "logprobs" not in r["choices"][0]


def test_api_stop_cuts_the_lists(client):
    body = {"prompt": "stop here", "max_tokens": 24, "logprobs": 1}
    full = client.post("/v1/completions", json=body).json()["choices"][0]
    text, offs = full["text"], full["logprobs"]["text_offset"]
    # a character whose first occurrence is as late as possible
    cut, stop = max((text.find(ch), ch) for ch in set(text))
    assert cut > 0, text
    ch = client.post("/v1/completions",
                     json={**body, "stop": [stop]}).json()["choices"][0]
    assert ch["finish_reason"] == "stop" and ch["text"] == text[:cut]
    n = sum(o < cut for o in offs)
    assert 0 < n < 24
    _check_completion_logprobs(ch["logprobs"], n, 1)
    for k in ch["logprobs"]:
        assert ch["logprobs"][k] == full["logprobs"][k][:n]


def test_api_chat(client):
    body = {"messages": [{"role": "user", "content": "yo"}],
            "max_tokens": 3}
    r = client.post("/v1/chat/completions", json=body).json()
    assert "logprobs" not in r["choices"][0]
    r = client.post("/v1/chat/completions",
                    json={**body, "logprobs": True, "top_logprobs": 3}).json()
    content = r["choices"][0]["logprobs"]["content"]
    assert len(content) == 3
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert e["logprob"] <= 0 and isinstance(e["bytes"], list)
        assert len(e["top_logprobs"]) == 3
        assert e["top_logprobs"][0]["token"] == e["token"]   # greedy
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]
        assert set(e["top_logprobs"][0]) == {"token", "logprob", "bytes"}
    r = client.post("/v1/chat/completions",
                    json={**body, "logprobs": True}).json()
    assert [e["top_logprobs"] for e in
            r["choices"][0]["logprobs"]["content"]] == [[]] * 3
    assert client.post("/v1/chat/completions",
                       json={**body, "top_logprobs": 3}).status_code == 400


def test_api_stream_carries_each_entry(client):
    import json
    body = {"prompt": "ab", "max_tokens": 3, "logprobs": 2}
    whole = client.post("/v1/completions", json=body).json()["choices"][0]
    with client.stream("POST", "/v1/completions",
                       json={**body, "stream": True}) as resp:
        lines = [l for l in "".join(resp.iter_text()).split("\n\n") if l]
    assert lines[-1] == "data: [DONE]" and len(lines) == 4
    for k, line in enumerate(lines[:3]):
        lp = json.loads(line[len("data: "):])["choices"][0]["logprobs"]
        for key in ("tokens", "token_logprobs", "top_logprobs",
                    "text_offset"):
            assert lp[key] == whole["logprobs"][key][k:k + 1]


def test_api_400(client):
    from fastapi.testclient import TestClient
    from skypilot_amd.serve.entrypoint import create_app
    r = client.post("/v1/completions",
                    json={"prompt": "a", "max_tokens": 2, "logprobs": 6})
    assert r.status_code == 400 and "max_logprobs = 5" in r.json()["detail"]
    r = client.post("/v1/chat/completions",
                    json={"messages": [{"role": "user", "content": "a"}],
                          "max_tokens": 2, "logprobs": True,
                          "top_logprobs": 6})
    assert r.status_code == 400 and "max_logprobs = 5" in r.json()["detail"]
    with TestClient(create_app(_engine(), "llama-debug")) as c:   # off
        for body in ({"logprobs": 1}, {"logprobs": 0, "echo": True}):
            r = c.post("/v1/completions",
                       json={"prompt": "a", "max_tokens": 2, **body})
            assert r.status_code == 400
            assert "--max-logprobs" in r.json()["detail"]


class _FixedEngine:
    """Answers every request with two tokens whose values are not
    finite."""
    stats = {}
    active = {}
    free_slots = []
    max_batch = 1

    def submit(self, r):
        r.out_ids = [65, 300]
        r.out_logprobs = [NEG_INF, float("nan")]
        r.out_top = [[(66, -0.5), (65, NEG_INF)], [(300, float("nan"))]]
        r.prompt_lps = [None] + [NEG_INF] * (len(r.prompt_ids) - 1)
        if r.stream_queue is not None:
            for t in r.out_ids + [None]:
                r.stream_queue.put(t)
        r.done.set()
        return r


def test_api_null_for_non_finite_values():
    from fastapi.testclient import TestClient
    from skypilot_amd.serve.entrypoint import create_app
    with TestClient(create_app(_FixedEngine(), "fixed")) as c:
        r = c.post("/v1/completions", json={"prompt": "a", "logprobs": 2,
                                            "echo": True})
        assert r.status_code == 200 and "NaN" not in r.text
        assert "Infinity" not in r.text
        lp = r.json()["choices"][0]["logprobs"]
        assert lp["token_logprobs"] == [None, None, None, None]
        assert lp["top_logprobs"][2:] == [{"B": -0.5, "A": None},
                                          {"<|300|>": None}]
        r = c.post("/v1/chat/completions",
                   json={"messages": [{"role": "user", "content": "a"}],
                         "logprobs": True, "top_logprobs": 2})
        assert r.status_code == 200 and "NaN" not in r.text
        content = r.json()["choices"][0]["logprobs"]["content"]
        assert [e["logprob"] for e in content] == [None, None]
        assert content[0]["top_logprobs"][1] == {
            "token": "A", "logprob": None, "bytes": [65]}
        assert content[1]["bytes"] == []
        with c.stream("POST", "/v1/completions",
                      json={"prompt": "a", "logprobs": 2,
                            "stream": True}) as resp:
            body = "".join(resp.iter_text())
        assert "NaN" not in body and "Infinity" not in body
        import json
        first = json.loads(body.split("\n\n")[0][len("data: "):])
        assert first["choices"][0]["logprobs"] == {
            "tokens": ["A"], "token_logprobs": [None],
            "top_logprobs": [{"B": -0.5, "A": None}], "text_offset": [0]}
