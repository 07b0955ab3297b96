"""ops.penalize_logits (decode_penalty.hip) element by element against
its fp64 reference, and the engine's graph path against its eager path
(docs/KERNELS.md "Decode penalties").

Seen tokens are held to tol_bf16(ref, A, K=1, roundings=1) with
A = |l| * max(rho, 1/rho) + |beta| * c + |alpha|: one bf16 rounding of
the result, fp32 arithmetic on three terms.  Everything else is compared
bit for bit."""
import pytest
import torch

import _fp64_check as fc
from skypilot_amd import ops

pytestmark = pytest.mark.gpu

#            presence, frequency, repetition
OFF = (0.0, 0.0, 1.0)
PARAMS = [(0.7, 0.3, 1.3), (-0.5, -0.2, 0.8), (0.0, 0.05, 1.0)]


def _case(V, L, seed=0):
    """One batch over histories of L tokens (p = L - 1): an off row, a row
    whose slot and one whose position lie outside hist, and four live rows
    with prompt lengths 0, L, L + 4 (clamped) and L // 2.  Every hist entry
    is an in-range id, so whatever lies past p is poison; ids -1 and V sit
    inside the live histories."""
    g = torch.Generator().manual_seed(seed + 7 * V + L)
    slots, s_max, p = 5, L + 7, L - 1
    hist = torch.randint(0, V, (slots, s_max), generator=g, dtype=torch.int32)
    hot = 7 % V
    if L >= 3:
        hist[1:, L // 3] = -1
        hist[1:, L // 3 + 1] = V
    if L >= 2500:
        hist[1, 100:2100] = hot      # 2,000 times, all generated (P = 0)
        hist[4, 400:2400] = hot      # in the prompt and in the output
    logits = (torch.randn(7, V, generator=g) * 4).bfloat16()
    if V > 8:
        logits[3, hot] = float("-inf")
    #        off  slot>=slots  pos>=S_max  ----------- live -----------
    slot = [0,    slots,       1,          1,   2,   3,      4]
    pos = [p,     p,           s_max,      p,   p,   p,      p]
    plen = [0,    0,           0,          0,   L,   L + 4,  L // 2]
    par = [OFF,   PARAMS[0],   PARAMS[0],  PARAMS[0], PARAMS[1], PARAMS[2],
           PARAMS[0]]
    tok = torch.randint(0, V, (7,), generator=g).tolist()
    tok[3], tok[5] = hot, V          # the hot id once more; an ignored id
    return logits, hist, tok, pos, slot, plen, par


def _run(logits, hist, tok, pos, slot, plen, par, cnt=None):
    dev = "cuda"
    n, V = logits.shape
    i32 = torch.tensor([tok, pos, slot, plen], dtype=torch.int32, device=dev)
    f32 = torch.tensor(par, dtype=torch.float32, device=dev).t().contiguous()
    if cnt is None:
        cnt = ops.penalty_workspace(n + 1, V, dev)
    h = hist.to(dev)
    x = logits.to(dev)
    out = torch.full_like(x, 7.0)
    ops.penalize_logits(x, out, h, cnt, *i32, *f32)
    torch.cuda.synchronize()
    assert not cnt.view(torch.int32).any(), "cnt is not all zero again"
    return out.cpu(), h.cpu()


@pytest.mark.parametrize("L", [1, 1023, 1025, 2500])
@pytest.mark.parametrize("V", [1, 1003, 4096])
def test_kernel_matches_reference(V, L):
    logits, hist, tok, pos, slot, plen, par = _case(V, L)
    want_hist = hist.clone()
    ref, seen, count = ops.penalize_logits_reference(
        logits, want_hist, tok, pos, slot, plen, *zip(*par))
    got, got_hist = _run(logits, hist, tok, pos, slot, plen, par)
    # hist changed at [s, p] of the live rows and nowhere else
    assert torch.equal(got_hist, want_hist)
    assert (want_hist != hist).sum() <= 4
    assert not seen[:3].any() and seen[[3, 4, 6]].any(dim=1).all()
    if L >= 2500:
        assert count[3, 7 % V] >= 2001 and 0 < count[6, 7 % V] < 2000
    # unseen tokens and off rows: the input's bits
    assert torch.equal(got.view(torch.int16)[~seen],
                       logits.view(torch.int16)[~seen])
    # seen tokens: non-finite values exactly, the rest inside the bound
    alpha, beta, rho = (torch.tensor(v, dtype=torch.float32).double()[:, None]
                        for v in zip(*par))
    A = (logits.double().abs() * torch.maximum(rho, 1 / rho)
         + beta.abs() * count + alpha.abs())
    fin = seen & torch.isfinite(ref)
    assert torch.equal(got.double()[seen & ~fin], ref[seen & ~fin])
    fc.check(f"penalize_logits V={V} L={L}", got[fin], ref[fin],
             fc.tol_bf16(ref, A, K=1, roundings=1)[fin])


def test_two_runs_are_bit_equal_and_share_the_workspace():
    case = _case(4096, 2500, seed=1)
    cnt = ops.penalty_workspace(8, 4096, "cuda")
    a, _ = _run(*case, cnt=cnt)
    b, _ = _run(*case, cnt=cnt)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_binding_rejects():
    dev = "cuda"
    x = torch.zeros(2, 16, dtype=torch.bfloat16, device=dev)
    i = torch.zeros(2, dtype=torch.int32, device=dev)
    f = torch.ones(2, device=dev)
    for out, s_max, rows, msg in [(x, 8, 2, "out must not alias logits"),
                                  (None, 65536, 2, "at most 65535"),
                                  (None, 8, 1, "cnt must be")]:
        hist = torch.zeros(2, s_max, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="penalize_logits: .*" + msg):
            ops.penalize_logits(
                x, torch.empty_like(x) if out is None else out, hist,
                ops.penalty_workspace(rows, 16, dev), i, i, i, i, f, f, f)


# ------------------------------ engine -------------------------------------
PROMPT = [(7 * i) % 500 for i in range(40)]
MAX_TOKENS = 20


def _engine_tokens(penalties, use_graphs, with_penalised):
    """out_ids of a plain greedy request, decoded next to a penalised one
    with the same prompt when `with_penalised` (whose out_ids come first)."""
    from skypilot_amd.serve.engine import Engine, Request
    eng = Engine("llama-debug", device="cuda:0", max_seq=256, max_batch=4,
                 penalties=penalties, use_graphs=use_graphs)
    eng.CHUNK = 8
    reqs = [Request(prompt_ids=list(PROMPT), max_tokens=MAX_TOKENS)]
    if with_penalised:
        reqs.insert(0, Request(prompt_ids=list(PROMPT),
                               max_tokens=MAX_TOKENS, frequency_penalty=1.5,
                               repetition_penalty=1.3))
    for r in reqs:      # all queued before the loop starts: one prefill
        eng.submit(r)
    eng.start()
    try:
        for r in reqs:
            assert r.done.wait(120)
        assert bool(eng.stats["graph_buckets"]) == use_graphs
    finally:
        eng.stop()
    if with_penalised:   # hist holds every token of the request by position
        want = PROMPT + reqs[0].out_ids[:-1]
        assert [h[:len(want)].tolist() for h in eng.hist].count(want) == 1
    return [r.out_ids for r in reqs]


def test_engine_graph_path_equals_eager_path():
    pen_g, plain_g = _engine_tokens(True, True, True)
    pen_e, plain_e = _engine_tokens(True, False, True)
    (alone,) = _engine_tokens(False, True, False)
    assert len(pen_g) == MAX_TOKENS and pen_g == pen_e
    assert plain_g == plain_e == alone
    assert pen_g != plain_g      # the penalties changed the tokens
