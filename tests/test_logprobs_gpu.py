"""GPU tests of the token log-probability kernel (decode_sample.hip:
ops.token_logprobs, ops.decode_logprobs) against the fp64 reference of
its definition (ops.token_logprobs_reference), and of the engine's
in-graph log-probabilities.

Values are compared with the tolerance derived in _logprobs_cases.py;
top ids have to be equal, in every case: the order (value descending,
index ascending) is total.

Worst err/tol measured on an MI355X over all cases below: 0.108
(V = 7 at scale 16; 0.00085 at V = 128256).
"""
import functools
import math

import pytest
import torch

import _fp64_check as fc
import _logprobs_cases as lc
from skypilot_amd import ops

pytestmark = pytest.mark.gpu

TOP = lc.TOP
SHAPES = [(1, 1), (3, 7), (2, 513), (3, 4099), (2, 128256)]
SCALES = [1.0, 16.0]
NS = [0, 1, 5, 20]
NEG_INF = float("-inf")


def _mixed(n):
    return [(-1, 20, 0, 5, 1)[(i + 1) % 5] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _case(n, V, scale):
    """Rows, chosen ids and the reference for every n_top setting."""
    logits = lc.make_rows(n, V, scale, seed=17 * V + int(scale))
    ids = lc.make_ids(n, V, seed=V + 1)
    refs = {N: lc.ref(logits, ids, N) for N in NS}
    refs["mixed"] = lc.ref(logits, ids, _mixed(n))
    return logits, ids, refs


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,V", SHAPES)
def test_against_reference(n, V, scale):
    logits, ids, refs = _case(n, V, scale)
    dev = logits.cuda()
    worst = 0.0
    for N, ref in refs.items():
        n_top = _mixed(n) if N == "mixed" else N
        got = ops.token_logprobs(dev, ids, n_top)
        worst = max(worst, lc.check_result(f"V={V} N={N}", got, ref, V))
    print(f"[logprobs] n={n} V={V} scale={scale}: worst err/tol {worst:.3g}")
    # the negative control: a reference that drops the largest element
    # from Z, or whose lse is off by 1e-4, is told apart at this V
    lp = ops.token_logprobs(dev, ids, 0)[0]
    good = lc.plain_reference(logits, ids)
    for wrong in lc.broken_references(logits, ids):
        keep = torch.isfinite(wrong) & (wrong != good)
        if bool(keep.any()):
            assert fc.rejects(lp.cpu()[keep], wrong[keep],
                              lc.tol(wrong[keep], V))


def test_large_rows_hold_ties_in_the_top():
    tied = 0
    for scale in SCALES:
        logits, _, refs = _case(2, 128256, scale)
        top = refs[20][2].long()
        vals = logits.float().gather(1, top)
        tied += int((vals[:, 1:] == vals[:, :-1]).sum())
    assert tied > 0


def test_all_equal_row():
    V = 128256
    logits = torch.full((1, V), 1.5).bfloat16()
    for N in (1, 5, 20):
        got = ops.token_logprobs(logits.cuda(), [V - 1], N)
        lc.check_result(f"all-equal N={N}", got, lc.ref(logits, [V - 1], N), V)
        assert got[2][0].tolist() == list(range(N)) + [-1] * (TOP - N)


@pytest.mark.parametrize("N", [5, 20])
def test_ties_across_wave_segments(N):
    V = 128256
    row, top3, ties = lc.tie_block_row(V)
    logits = row[None]
    got = ops.token_logprobs(logits.cuda(), [ties[-1]], N)
    lc.check_result(f"tie block N={N}", got, lc.ref(logits, [ties[-1]], N), V)
    assert got[2][0, :N].tolist() == top3 + ties[:N - 3]


def test_more_than_the_row_holds():
    for n, V in [(1, 1), (3, 7)]:
        logits, ids, _ = _case(n, V, 1.0)
        got = ops.token_logprobs(logits.cuda(), ids, 20)
        lc.check_result(f"N>V V={V}", got, lc.ref(logits, ids, 20), V)
        assert (got[2][:, V:] == -1).all() and (got[2][:, :V] >= 0).all()
        assert torch.isnan(got[1][:, V:]).all()


def test_fewer_finite_values_than_asked():
    V = 513
    logits = torch.full((2, V), NEG_INF).bfloat16()
    logits[0, [500, 2, 257, 64]] = torch.tensor(
        [0.5, 2.0, -1.0, 0.5]).bfloat16()
    logits[1] = lc.make_rows(1, V, 1.0, seed=3)[0]
    ids = [7, 7]                       # row 0: a -inf token
    got = ops.token_logprobs(logits.cuda(), ids, 20)
    lc.check_result("-inf entries", got, lc.ref(logits, ids, 20), V)
    assert got[2][0].tolist() == [2, 64, 500, 257] + [
        j for j in range(18) if j != 2][:16]
    assert got[1][0, 4:].tolist() == [NEG_INF] * 16
    assert float(got[0][0]) == NEG_INF


def test_degenerate_rows():
    V = 4099
    logits = lc.make_rows(5, V, 1.0, seed=11)
    logits[1, 4098] = float("nan")
    logits[2, 0] = float("inf")
    logits[3] = NEG_INF
    ids = [5, 5, 0, 5, 4098]
    ref = lc.ref(logits, ids, 5)
    got = ops.token_logprobs(logits.cuda(), ids, 5)
    lc.check_result("degenerate", got, ref, V)
    for i in (1, 2, 3):
        assert math.isnan(float(got[0][i]))
        assert torch.isnan(got[1][i]).all() and (got[2][i] == -1).all()
    for i in (0, 4):
        assert math.isfinite(float(got[0][i]))
        assert (got[2][i, :5] >= 0).all()


def test_chosen_id_outside_the_row():
    V = 513
    logits = lc.make_rows(4, V, 1.0, seed=12)
    ids = [3, -1, V, 512]
    ref = lc.ref(logits, ids, 5)
    got = ops.token_logprobs(logits.cuda(), ids, 5)
    lc.check_result("id outside", got, ref, V)
    lp = got[0].tolist()
    assert math.isnan(lp[1]) and math.isnan(lp[2])
    assert math.isfinite(lp[0]) and math.isfinite(lp[3])
    # the top list does not depend on the chosen id
    assert (got[2][:, :5] >= 0).all()


@pytest.mark.parametrize("pad", [8, 3])
@pytest.mark.parametrize("n,V", [(3, 7), (2, 513), (3, 4099)])
def test_no_read_outside_the_rows(n, V, pad):
    """The rows sit inside a NaN-filled allocation: a read past a row's
    ends, or past the last row, makes its result NaN."""
    logits, ids, refs = _case(n, V, 1.0)
    buf = torch.full((n * V + 2 * pad + 4096,), float("nan"),
                     dtype=torch.bfloat16, device="cuda")
    inner = buf[pad:pad + n * V].view(n, V)
    for i in range(n):   # each row alone, between NaNs on both sides
        buf.fill_(float("nan"))
        buf[pad:pad + V] = logits[i].cuda()
        got = ops.token_logprobs(buf[pad:pad + V].view(1, V), ids[i:i + 1],
                                 20)
        ref = tuple(t[i:i + 1] for t in refs[20])
        lc.check_result(f"NaN frame row {i}", got, ref, V)
    buf.fill_(float("nan"))
    inner.copy_(logits)
    got = ops.token_logprobs(inner, ids, 20)
    lc.check_result("NaN frame batch", got, refs[20], V)


def test_off_rows_keep_their_contents():
    n, V = 3, 4099
    logits, ids, refs = _case(n, V, 1.0)
    out = (torch.full((n,), 123.0, device="cuda"),
           torch.full((n, TOP), 45.0, device="cuda"),
           torch.full((n, TOP), 67, dtype=torch.int32, device="cuda"))
    n_top = [5, -1, 20]
    ops.token_logprobs(logits.cuda(), ids, n_top, out=out)
    assert float(out[0][1]) == 123.0
    assert (out[1][1] == 45.0).all() and (out[2][1] == 67).all()
    for i, N in ((0, 5), (2, 20)):
        lc.check_result(f"on row {i}", tuple(t[i:i + 1] for t in out),
                        tuple(t[i:i + 1] for t in refs[N]), V)
    # n_top above 20 counts as 20
    got = ops.token_logprobs(logits.cuda(), ids, 1000)
    lc.check_result("n_top > 20", got, refs[20], V)


def test_determinism_and_batch_invariance():
    for V, scale in [(4099, 1.0), (128256, 16.0)]:
        rows = lc.make_rows(3, V, scale, seed=21).cuda()
        ids = [V // 2, 1, V - 1]
        a = ops.token_logprobs(rows, ids, [20, 5, 20])
        b = ops.token_logprobs(rows, ids, [20, 5, 20])
        one = ops.token_logprobs(rows[2:3].clone(), ids[2:], 20)
        for x, y, z in zip(a, b, one):
            # bit-equal: compare the raw words, NaNs included
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            assert torch.equal(x[2:3].view(torch.int32),
                               z.view(torch.int32))


@pytest.mark.parametrize("ctr0", [0, 5, -3])
def test_decode_logprobs_ring(ctr0):
    b, V, chunk = 3, 4099, 4
    logits = lc.make_rows(b, V, 1.0, seed=31).cuda()
    stage = torch.tensor([[9, 9, 9], [4, 5, 6], [0, 1, 2], [4, 5, 6],
                          [5, 6, 7], [0, 1, 2]], dtype=torch.int32,
                         device="cuda")
    ring = torch.full((chunk, b), -7, dtype=torch.long, device="cuda")
    ctr = torch.tensor([ctr0], dtype=torch.long, device="cuda")
    n_top = torch.tensor([5, -1, 20], dtype=torch.int32, device="cuda")
    lp_ring = torch.full((chunk, b), 123.0, device="cuda")
    tlp_ring = torch.full((chunk, b, TOP), 45.0, device="cuda")
    tid_ring = torch.full((chunk, b, TOP), 67, dtype=torch.int32,
                          device="cuda")
    slot = ctr0 % chunk                    # Python's %: in [0, chunk)
    if ctr0 >= 0:
        ops.decode_advance(logits, stage, ring, ctr)
        assert ring[slot].tolist() == logits.float().argmax(-1).tolist()
    else:
        # the greedy advance kernel takes no negative counter; the
        # sampling one wraps it as decode_logprobs does
        samp = torch.zeros(5, b, dtype=torch.int32, device="cuda")
        ops.decode_sample_advance(logits, stage, ring, ctr, samp)
        assert ring[slot].tolist() == logits.float().argmax(-1).tolist()
    after = stage.clone()
    ops.decode_logprobs(logits, stage, n_top, lp_ring, tlp_ring, tid_ring,
                        ctr)
    assert torch.equal(stage, after) and int(ctr) == ctr0
    want = ops.token_logprobs(logits, stage[0].long(), n_top)
    for i in (0, 2):
        assert torch.equal(lp_ring[slot, i].view(torch.int32),
                           want[0][i].view(torch.int32))
        assert torch.equal(tlp_ring[slot, i].view(torch.int32),
                           want[1][i].view(torch.int32))
        assert torch.equal(tid_ring[slot, i], want[2][i])
    # the greedy token is the top-1 id
    assert int(tid_ring[slot, 0, 0]) == int(stage[0, 0])
    # the off row and the other ring rows keep the sentinel
    lp_ring[slot, [0, 2]] = 123.0
    tlp_ring[slot, [0, 2]] = 45.0
    tid_ring[slot, [0, 2]] = 67
    assert (lp_ring == 123.0).all() and (tlp_ring == 45.0).all()
    assert (tid_ring == 67).all()


def test_binding_checks():
    C = ops.native()
    b, V = 2, 64

    def args(**kw):
        d = dict(
            logits=torch.zeros(b, V, dtype=torch.bfloat16, device="cuda"),
            ids=torch.zeros(b, dtype=torch.long, device="cuda"),
            n_top=torch.zeros(b, dtype=torch.int32, device="cuda"),
            lp=torch.zeros(b, device="cuda"),
            top_lp=torch.zeros(b, TOP, device="cuda"),
            top_ids=torch.zeros(b, TOP, dtype=torch.int32, device="cuda"))
        d.update(kw)
        return list(d.values())

    C.token_logprobs(*args())
    for bad in [
        dict(logits=torch.zeros(b, V, device="cuda")),               # dtype
        dict(logits=torch.zeros(b, 1, V, dtype=torch.bfloat16,
                                device="cuda")),                     # rank
        dict(logits=torch.zeros(b, V, dtype=torch.bfloat16)),        # device
        dict(logits=torch.zeros(V, b, dtype=torch.bfloat16,
                                device="cuda").t()),             # contiguity
        dict(logits=torch.zeros(b, 0, dtype=torch.bfloat16,
                                device="cuda")),                     # V = 0
        dict(ids=torch.zeros(b, dtype=torch.int32, device="cuda")),
        dict(ids=torch.zeros(b + 1, dtype=torch.long, device="cuda")),
        dict(ids=torch.zeros(b, dtype=torch.long)),
        dict(n_top=torch.zeros(b, dtype=torch.long, device="cuda")),
        dict(n_top=torch.zeros(b, 1, dtype=torch.int32, device="cuda")),
        dict(lp=torch.zeros(b, dtype=torch.float64, device="cuda")),
        dict(lp=torch.zeros(b + 1, device="cuda")),
        dict(top_lp=torch.zeros(b, TOP - 1, device="cuda")),
        dict(top_lp=torch.zeros(b, TOP, dtype=torch.bfloat16,
                                device="cuda")),
        dict(top_ids=torch.zeros(b, TOP, dtype=torch.long, device="cuda")),
        dict(top_ids=torch.zeros(b * TOP, dtype=torch.int32,
                                 device="cuda")),
    ]:
        with pytest.raises(RuntimeError, match="token_logprobs"):
            C.token_logprobs(*args(**bad))

    def dargs(**kw):
        d = dict(
            logits=torch.zeros(b, V, dtype=torch.bfloat16, device="cuda"),
            stage=torch.zeros(6, b, dtype=torch.int32, device="cuda"),
            n_top=torch.zeros(b, dtype=torch.int32, device="cuda"),
            lp_ring=torch.zeros(4, b, device="cuda"),
            top_lp_ring=torch.zeros(4, b, TOP, device="cuda"),
            top_id_ring=torch.zeros(4, b, TOP, dtype=torch.int32,
                                    device="cuda"),
            ctr=torch.zeros(1, dtype=torch.long, device="cuda"))
        d.update(kw)
        return list(d.values())

    C.decode_logprobs(*dargs())
    for bad in [
        dict(logits=torch.zeros(b, V, device="cuda")),
        dict(logits=torch.zeros(b, 1, V, dtype=torch.bfloat16,
                                device="cuda")),
        dict(stage=torch.zeros(5, b, dtype=torch.int32, device="cuda")),
        dict(stage=torch.zeros(6, b, dtype=torch.long, device="cuda")),
        dict(stage=torch.zeros(6, b, dtype=torch.int32)),
        dict(n_top=torch.zeros(b + 1, dtype=torch.int32, device="cuda")),
        dict(lp_ring=torch.zeros(4, b + 1, device="cuda")),
        dict(lp_ring=torch.zeros(0, b, device="cuda")),
        dict(top_lp_ring=torch.zeros(3, b, TOP, device="cuda")),
        dict(top_lp_ring=torch.zeros(4, b, TOP, dtype=torch.float64,
                                     device="cuda")),
        dict(top_id_ring=torch.zeros(4, b, TOP - 1, dtype=torch.int32,
                                     device="cuda")),
        dict(top_id_ring=torch.zeros(4, b, TOP, dtype=torch.long,
                                     device="cuda")),
        dict(ctr=torch.zeros(1, dtype=torch.int32, device="cuda")),
        dict(ctr=torch.zeros(2, dtype=torch.long, device="cuda")),
    ]:
        with pytest.raises(RuntimeError, match="decode_logprobs"):
            C.decode_logprobs(*dargs(**bad))
    # V is bounded as for the sampler: the fixed-point sum must fit 64 bits
    wide = torch.zeros(1, 2 ** 23 + 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="2\\^23"):
        C.token_logprobs(wide, *[t[:1].contiguous() for t in args()[1:]])
    with pytest.raises(RuntimeError, match="2\\^23"):
        d = dargs()
        C.decode_logprobs(wide, d[1][:, :1].contiguous(), d[2][:1],
                          d[3][:, :1].contiguous(),
                          d[4][:, :1].contiguous(),
                          d[5][:, :1].contiguous(), d[6])
    with pytest.raises(ValueError):
        ops.token_logprobs(torch.zeros(b, V, device="cuda"), [0, 0], 0)


# ------------------------------ engine -------------------------------------
PROMPTS = [list(range(1, 33)), list(range(40, 90)), list(range(7, 27))]
MAX_TOKENS = 20


def _run_engine(max_logprobs, ask):
    """Three requests decoded together in chains of 8: greedy, seeded
    sampled, greedy.  `ask` gives each request's logprobs field."""
    from skypilot_amd.serve.engine import Engine, Request
    eng = Engine("llama-debug", device="cuda:0", max_seq=256, max_batch=4,
                 device_sampling=True, max_logprobs=max_logprobs)
    eng.CHUNK = 8
    reqs = [
        Request(prompt_ids=PROMPTS[0], max_tokens=MAX_TOKENS,
                logprobs=ask[0]),
        Request(prompt_ids=PROMPTS[1], max_tokens=MAX_TOKENS,
                temperature=0.9, top_p=0.9, top_k=40, seed=7,
                logprobs=ask[1]),
        Request(prompt_ids=PROMPTS[2], max_tokens=MAX_TOKENS,
                logprobs=ask[2]),
    ]
    for r in reqs:      # all queued before the loop starts: one prefill
        eng.submit(r)
    eng.start()
    try:
        for r in reqs:
            assert r.done.wait(120)
        assert eng.stats["graph_buckets"]
    finally:
        eng.stop()
    return reqs


def test_engine_logprobs_in_graph():
    V = 512
    base = _run_engine(0, [None, None, None])
    reqs = _run_engine(5, [5, 3, None])
    for r, r0 in zip(reqs, base):
        assert r.out_ids == r0.out_ids and len(r.out_ids) == MAX_TOKENS
    assert reqs[2].out_logprobs == [] and reqs[2].out_top == []
    assert reqs[2].prompt_lps == []
    for r, N in zip(reqs[:2], (5, 3)):
        assert len(r.out_logprobs) == len(r.out_top) == len(r.out_ids)
        for tok, lp, top in zip(r.out_ids, r.out_logprobs, r.out_top):
            assert len(top) == N
            assert math.isfinite(lp) and lp <= 0.0
            lps = [v for _, v in top]
            assert lps == sorted(lps, reverse=True)
            for t, v in top:
                if t == tok:
                    assert v == lp
            t = float(lc.tol(min(lps), V))
            assert sum(math.exp(v) for v in lps) <= 1.0 + t
            if r.temperature == 0:
                assert top[0][0] == tok and top[0][1] == lp
    assert reqs[1].out_ids != base[0].out_ids   # the sampled one sampled
