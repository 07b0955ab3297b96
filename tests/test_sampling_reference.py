"""Decode sampling on the CPU: the Philox stream, the fp64 reference of
the sampling definition (docs/KERNELS.md), and the engine / API plumbing
of temperature, top_p, top_k and seed with device_sampling on."""
import pytest
import torch

import _sampling_cases as sc
from skypilot_amd import ops
from skypilot_amd.serve.engine import Engine, Request


def _hex(words):
    return " ".join(f"{w:08x}" for w in words)


def test_philox_known_answers():
    assert _hex(ops.philox4x32_10((0, 0, 0, 0), (0, 0))) == \
        "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(ops.philox4x32_10((ones,) * 4, (ones,) * 2)) == \
        "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(ops.philox4x32_10(
        (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
        (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # u uses the top 24 bits of word 0, seed split low/high into the key
    assert ops.sample_uniform(0, 0) == (0x6627E8D5 >> 8) * 2.0 ** -24
    assert ops.sample_uniform((0x299F31D0 << 32) | 0xA4093822, 5) == \
        (ops.philox4x32_10((5, 0, 0, 0),
                           (0xA4093822, 0x299F31D0))[0] >> 8) * 2.0 ** -24


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_threshold_matches_definition(T):
    rows = sc.make_rows(3, 512, seed=100)
    n = 0
    for row in rows:
        # top_p reaches the reference as fp32: keep the midpoint further
        # than its rounding (2^-24) from both masses
        for p, want in sc.top_p_cases(row, T, min_gap=1e-6):
            _, tau = ops.sample_tokens(row[None], T, p, 0, 1, 0)
            assert float(tau[0]) == want, (T, p)
            n += 1
        for k, want in sc.top_k_cases(row):
            _, tau = ops.sample_tokens(row[None], T, 1.0, k, 1, 0)
            assert float(tau[0]) == want, (T, k)
            n += 1
        # both on: the larger threshold wins
        (p, wp), (k, wk) = sc.top_p_cases(row, T, 1e-6)[2], \
            sc.top_k_cases(row)[1]
        _, tau = ops.sample_tokens(row[None], T, p, k, 1, 0)
        assert float(tau[0]) == max(wp, wk)
    assert n >= 3 * 8
    row = rows[0]
    top = float(row.float().max())
    # filters off, top_p <= 0, top_k == 1, greedy
    assert float(ops.sample_tokens(row[None], T, 1.0, 0, 1, 0)[1]) == \
        float("-inf")
    assert float(ops.sample_tokens(row[None], T, 1.0, 512, 1, 0)[1]) == \
        float("-inf")
    assert float(ops.sample_tokens(row[None], T, 0.0, 0, 1, 0)[1]) == top
    assert float(ops.sample_tokens(row[None], T, 1.0, 1, 1, 0)[1]) == top
    tok, tau = ops.sample_tokens(row[None], 0.0, 0.5, 5, 1, 0)
    assert int(tok) == int(row.float().argmax())
    assert float(tau) == float("-inf")


def test_token_always_in_kept_set_and_range():
    rows = sc.make_rows(4, 512, seed=7)
    for i, row in enumerate(rows):
        for c in (0, 1, 2 ** 31 - 1):
            r = ops.sample_row_reference(row, 0.8, 0.9, 40, 11 + i, c)
            assert 0 <= r["token"] < 512
            assert bool(r["kept"][r["token"]])
    bad = torch.full((3, 16), float("-inf"))
    bad[1] = float("nan")
    bad[2, 3] = 1.0
    bad[2, 9] = float("nan")
    toks, _ = ops.sample_tokens(bad, 1.0, 0.9, 4, 3, 0)
    assert toks.tolist() == [0, 0, 3]   # argmax, NaN never wins


@pytest.mark.parametrize("seed,expect", [(1, 4.64), (2, 9.14),
                                         (12345, 6.70)])
def test_distribution_chi_square(seed, expect):
    p = torch.tensor([.4, .2, .15, .1, .06, .05, .03, .01],
                     dtype=torch.float64)
    logits = p.log().float()
    n = 16384
    toks, _ = ops.sample_tokens(logits.expand(n, 8), 1.0, 1.0, 0, seed,
                                list(range(n)))
    cnt = torch.bincount(toks, minlength=8).double()
    exact = torch.softmax(logits.double(), 0)
    chi2 = float(((cnt - n * exact) ** 2 / (n * exact)).sum())
    print(f"seed {seed}: chi-square {chi2:.3f}")
    assert chi2 < 24.32          # p = 0.001 at 7 degrees of freedom
    assert abs(chi2 - expect) < 0.01   # the stream is deterministic


# ------------------------------ engine -------------------------------------
@pytest.fixture(scope="module")
def engine():
    eng = Engine("llama-debug", device="cpu", max_seq=256, max_batch=4,
                 device_sampling=True)
    eng.start()
    yield eng
    eng.stop()


def _greedy_no_cache(model, prompt_ids, n):
    ids = list(prompt_ids)
    for _ in range(n):
        logits = model(torch.tensor([ids]))
        ids.append(int(logits[0, -1].argmax()))
    return ids[len(prompt_ids):]


def _sampled_no_cache(model, prompt_ids, n, T, top_p, top_k, seed):
    ids = list(prompt_ids)
    for _ in range(n):
        logits = model(torch.tensor([ids]))
        tok, _ = ops.sample_tokens_reference(
            logits[0, -1][None], T, top_p, top_k, seed, len(ids) - 1)
        ids.append(int(tok))
    return ids[len(prompt_ids):]


PROMPT = [1, 5, 9, 200, 3]
KW = dict(max_tokens=8, temperature=0.9, top_p=0.9, top_k=40)


def test_engine_seeded_generate_is_reproducible(engine):
    a = engine.generate(PROMPT, seed=7, **KW)
    b = engine.generate(PROMPT, seed=7, **KW)
    assert a == b and len(a) == 8
    with torch.no_grad():
        want = _sampled_no_cache(engine.model, PROMPT, 8, 0.9, 0.9, 40, 7)
    assert a == want, (a, want)


def test_engine_seeds_differ(engine):
    assert engine.generate(PROMPT, seed=7, **KW) != \
        engine.generate(PROMPT, seed=8, **KW)


def test_engine_greedy_with_flag_on(engine):
    with torch.no_grad():
        want = _greedy_no_cache(engine.model, PROMPT, 8)
    assert engine.generate(PROMPT, max_tokens=8) == want
    # a sampled neighbour in the batch does not disturb a greedy row
    reqs = [engine.submit(Request(prompt_ids=list(PROMPT), max_tokens=8)),
            engine.submit(Request(prompt_ids=[11, 13], max_tokens=8,
                                  temperature=0.9, seed=3))]
    for r in reqs:
        assert r.done.wait(60)
    assert reqs[0].out_ids == want
    assert len(reqs[1].out_ids) == 8


def test_engine_assigns_and_reduces_seed(engine):
    r = engine.submit(Request(prompt_ids=[2, 3], max_tokens=2,
                              temperature=0.7))
    assert r.done.wait(60)
    assert isinstance(r.seed, int) and 0 <= r.seed < 2 ** 63
    r = engine.submit(Request(prompt_ids=[2, 3], max_tokens=2,
                              temperature=0.7, seed=2 ** 63 + 5))
    assert r.done.wait(60)
    assert r.seed == 5


@pytest.mark.parametrize("kw", [
    dict(temperature=-0.5), dict(temperature=float("nan")),
    dict(temperature=float("inf")), dict(temperature=10 ** 400),
    dict(top_p=float("nan")), dict(top_p=-float("inf")),
    dict(top_p=10 ** 400), dict(top_k=2.5), dict(top_k=True),
    dict(seed="x")])
def test_engine_rejects_bad_parameters(engine, kw):
    with pytest.raises(ValueError):
        engine.submit(Request(prompt_ids=[1, 2], max_tokens=2, **kw))


def test_huge_top_k_is_clamped_and_engine_survives(engine):
    """top_k beyond int32 (pydantic keeps 10**30) is clamped at submit:
    it means "off", and the engine thread keeps serving."""
    kw = dict(max_tokens=6, temperature=0.9, top_p=0.9, seed=5)
    r = engine.submit(Request(prompt_ids=list(PROMPT), top_k=10 ** 30,
                              **kw))
    assert r.top_k == 2 ** 31 - 1
    assert r.done.wait(60)
    assert r.out_ids == engine.generate(PROMPT, top_k=0, **kw)
    r = engine.submit(Request(prompt_ids=list(PROMPT), top_k=-10 ** 30,
                              **kw))
    assert r.top_k == 0 and r.done.wait(60)
    assert engine._thread.is_alive()
    assert len(engine.generate(PROMPT, max_tokens=3)) == 3
    # the op clamps too, for callers that do not go through submit()
    row = sc.make_rows(1, 512, seed=3)
    a, ta = ops.sample_tokens(row, 0.9, 1.0, 10 ** 30, 5, 0)
    b, tb = ops.sample_tokens(row, 0.9, 1.0, 0, 5, 0)
    assert int(a) == int(b) and float(ta) == float(tb) == float("-inf")


def test_api_seed_top_k_top_p(engine):
    from fastapi.testclient import TestClient
    from skypilot_amd.serve.entrypoint import create_app
    app = create_app(engine, "llama-debug")
    body = {"max_tokens": 6, "temperature": 0.9, "top_p": 0.9,
            "top_k": 40, "seed": 21}
    with TestClient(app) as c:
        comp = [c.post("/v1/completions",
                       json={"prompt": "ab", **body}).json()
                for _ in range(2)]
        assert comp[0]["choices"] == comp[1]["choices"]
        assert comp[0]["usage"]["completion_tokens"] == 6
        assert comp[0]["seed"] == 21
        chat = [c.post("/v1/chat/completions",
                       json={"messages": [{"role": "user",
                                           "content": "yo"}],
                             **body}).json() for _ in range(2)]
        assert chat[0]["choices"] == chat[1]["choices"]
        assert chat[0]["usage"]["completion_tokens"] == 6
        # the non-streaming path honours top_p: a tiny nucleus is greedy
        greedy = c.post("/v1/completions",
                        json={"prompt": "ab", "max_tokens": 6}).json()
        tiny = c.post("/v1/completions",
                      json={"prompt": "ab", "max_tokens": 6,
                            "temperature": 0.9, "top_p": 1e-6}).json()
        assert tiny["choices"] == greedy["choices"]
        chat_tiny = c.post("/v1/chat/completions",
                           json={"messages": [{"role": "user",
                                               "content": "yo"}],
                                 "max_tokens": 6, "temperature": 0.9,
                                 "top_p": 1e-6}).json()
        chat_greedy = c.post("/v1/chat/completions",
                             json={"messages": [{"role": "user",
                                                 "content": "yo"}],
                                   "max_tokens": 6}).json()
        assert chat_tiny["choices"] == chat_greedy["choices"]
        bad = c.post("/v1/completions",
                     json={"prompt": "ab", "temperature": -1.0})
        assert bad.status_code == 400
        huge = c.post("/v1/completions",
                      json={"prompt": "ab", "max_tokens": 4,
                            "temperature": 0.9, "top_k": 10 ** 30,
                            "seed": 21})
        assert huge.status_code == 200
        assert huge.json()["usage"]["completion_tokens"] == 4
        after = c.post("/v1/completions",
                       json={"prompt": "ab", "max_tokens": 6}).json()
        assert after["choices"] == greedy["choices"]


def test_api_host_path_honours_top_p():
    """The default (host-sampling) engine's non-streaming path passes
    top_p through as well."""
    from fastapi.testclient import TestClient
    from skypilot_amd.serve.entrypoint import create_app
    eng = Engine("llama-debug", device="cpu", max_seq=256, max_batch=2)
    eng.start()
    try:
        with TestClient(create_app(eng, "llama-debug")) as c:
            greedy = c.post("/v1/completions",
                            json={"prompt": "ab", "max_tokens": 6}).json()
            tiny = c.post("/v1/completions",
                          json={"prompt": "ab", "max_tokens": 6,
                                "temperature": 0.9,
                                "top_p": 1e-6}).json()
            assert tiny["choices"] == greedy["choices"]
            assert tiny["seed"] is None
            # top_k and seed are refused, not dropped, without the flag
            for extra in ({"top_k": 5}, {"seed": 1}):
                bad = c.post("/v1/completions",
                             json={"prompt": "ab", "max_tokens": 2,
                                   "temperature": 0.9, **extra})
                assert bad.status_code == 400
                assert "device sampling" in bad.json()["detail"]
            with pytest.raises(ValueError):
                eng.generate([1, 2], max_tokens=2, top_k=3)
    finally:
        eng.stop()
