"""GPU tests of the seeded decode-sampling kernel (decode_sample.hip)
against the fp64 reference of the sampling definition
(ops.sample_row_reference), and of the engine's in-graph sampling.

Tolerance.  A kernel token j' is accepted when j' is in the kept set K
and its prefix-sum interval [C_{j'-1}, C_{j'}] (reference, fp64, index
order over K) comes within EPS * Z_K of t = u * Z_K.  EPS = 6e-5 is
twice (V/256 + 16) * 2^-24 at V = 128256, the worst-case fp32 error of
a 256-thread partial-sum-plus-tree accumulation.  The kernel's own
layout stays well inside that: it sums 2^-40 fixed-point weights
exactly (truncation <= V * 2^-40 = 1.2e-7 of the total) and its
exp2-based weights are within a few 2^-22 relative of the reference's,
so the bound is kept as stated rather than widened or re-derived.  The
same EPS is the margin the top_p thresholds keep from the cumulative
masses in the tau test.
"""
import functools
import math

import pytest
import torch

import _sampling_cases as sc
from skypilot_amd import ops

pytestmark = pytest.mark.gpu

EPS = 6e-5
SHAPES = [(1, 128256), (4, 4096), (8, 512), (3, 1000)]
NEG_INF = float("-inf")


@functools.lru_cache(maxsize=None)
def _rows(b, V):
    return sc.make_rows(b, V, seed=1000 + V)


@functools.lru_cache(maxsize=None)
def _tau_cases(b, V):
    """(logits [n, V], T, top_p, top_k, expected tau) for every threshold
    case of every row, flattened into one batch."""
    rows = _rows(b, V)
    idx, Ts, ps, ks, want = [], [], [], [], []
    for i in range(b):
        for T in (0.5, 1.0, 2.0):
            p_cases = sc.top_p_cases(rows[i], T, min_gap=EPS, want=4)
            # every (row, T) must bring its own top_p boundaries (a row
            # that one token dominates at T = 0.5 has only two whose
            # margin exceeds EPS; test_tau_exact checks the total)
            assert len(p_cases) >= 2, (b, V, i, T, len(p_cases))
            for p, tau in p_cases:
                idx.append(i), Ts.append(T), ps.append(p), ks.append(0)
                want.append(tau)
            for k, tau in sc.top_k_cases(rows[i]):
                idx.append(i), Ts.append(T), ps.append(1.0), ks.append(k)
                want.append(tau)
    logits = rows[idx].contiguous()
    _, ref_tau = ops.sample_tokens_reference(logits, Ts, ps, ks, 1, 0)
    assert ref_tau.tolist() == [float(torch.tensor(w, dtype=torch.float32))
                                for w in want]
    return logits, Ts, ps, ks, ref_tau


@pytest.mark.parametrize("b,V", SHAPES)
def test_tau_exact(b, V):
    logits, Ts, ps, ks, ref_tau = _tau_cases(b, V)
    n_p = sum(k == 0 for k in ks)
    assert n_p >= 9 * b and len(Ts) - n_p >= 9 * b, (n_p, len(Ts))
    _, tau = ops.sample_tokens(logits.cuda(), Ts, ps, ks, 1, 0)
    bad = (tau.cpu() != ref_tau).nonzero().flatten().tolist()
    assert not bad, [(Ts[i], ps[i], ks[i], float(tau[i]),
                      float(ref_tau[i])) for i in bad[:5]]


PARAMS = [(1.0, 1.0, 0), (0.7, 0.9, 0), (1.0, 1.0, 40), (1.0, 0.9, 40),
          (0.5, 1.0, 0)]


def _admissible(r):
    """Indices the reference admits for one draw."""
    C, kept, t, tol = r["C"], r["kept"], r["t"], EPS * r["ZK"]
    prev = torch.cat([torch.zeros(1, dtype=C.dtype), C[:-1]])
    return kept & (prev - tol <= t) & (t <= C + tol)


@functools.lru_cache(maxsize=None)
def _token_cases(b, V):
    rows = _rows(b, V)
    draws = 8 if V > 4096 else 16
    idx, Ts, ps, ks, seeds, ctrs, refs = [], [], [], [], [], [], []
    for i in range(b):
        for (T, p, k) in PARAMS:
            for d in range(draws):
                seed, ctr = 7919 * (i + 1) + len(idx), 3 * d + i
                idx.append(i), Ts.append(T), ps.append(p), ks.append(k)
                seeds.append(seed), ctrs.append(ctr)
                refs.append(ops.sample_row_reference(
                    rows[i], float(torch.tensor(T, dtype=torch.float32)),
                    float(torch.tensor(p, dtype=torch.float32)), k, seed,
                    ctr))
    return rows[idx].contiguous(), Ts, ps, ks, seeds, ctrs, refs


@pytest.mark.parametrize("b,V", [s for s in SHAPES if s[1] <= 4096])
def test_reference_is_rarely_ambiguous(b, V):
    """On the reference alone: at most 5% of the draws admit more than
    one token, so the exact-match check below covers nearly all."""
    refs = _token_cases(b, V)[-1]
    multi = sum(int(_admissible(r).sum()) > 1 for r in refs)
    print(f"V={V}: {multi}/{len(refs)} draws admit more than one token")
    assert multi <= 0.05 * len(refs)


@pytest.mark.parametrize("b,V", SHAPES)
def test_token_against_reference(b, V):
    logits, Ts, ps, ks, seeds, ctrs, refs = _token_cases(b, V)
    toks, tau = ops.sample_tokens(logits.cuda(), Ts, ps, ks, seeds, ctrs)
    toks = toks.tolist()
    exact = 0
    for i, (j, r) in enumerate(zip(toks, refs)):
        assert 0 <= j < V
        ok = _admissible(r)
        assert bool(r["kept"][j]), (i, j, "not in K")
        assert bool(ok[j]), (i, j, r["token"], Ts[i], ps[i], ks[i])
        if int(ok.sum()) == 1:
            assert j == r["token"]
            exact += 1
    print(f"V={V}: {exact}/{len(refs)} exact matches")


def test_support_and_coverage():
    g = torch.Generator().manual_seed(5)
    row = torch.randn(512, generator=g).bfloat16()
    row[100], row[37] = 10.0, 9.625     # masses ~ .59 / .41 at T = 1
    logits = row[None].expand(64, 512).contiguous().cuda()
    seeds = list(range(1000, 1064))
    toks, tau = ops.sample_tokens(logits, 1.0, 1.0, 2, seeds, 17)
    assert set(toks.tolist()) == {100, 37}
    assert tau.tolist() == [9.625] * 64
    ref, _ = ops.sample_tokens_reference(row[None].expand(64, 512), 1.0,
                                         1.0, 2, seeds, 17)
    assert toks.cpu().tolist() == ref.tolist()


def _samp_block(Ts, ps, ks, seeds):
    b = len(Ts)
    return ops.pack_samp(b, Ts, ps, ks, seeds)[:5].contiguous()


def test_greedy_rows_equal_decode_advance():
    """All-greedy samp: stage and ring bit-equal to ops.decode_advance on
    the same logits, ties at the maximum included (the case of
    test_decode_advance_fused)."""
    torch.manual_seed(11)
    for b, V, chunk in [(1, 128256, 8), (4, 4096, 8), (8, 512, 4),
                        (3, 1000, 3)]:
        logits = (torch.randn(b, V, device="cuda") * 2).bfloat16()
        logits[0, 7] = 40.0
        logits[0, V - 3] = 40.0
        stage = torch.randint(0, 100, (6, b), dtype=torch.int32,
                              device="cuda")
        ring = torch.zeros(chunk, b, dtype=torch.long, device="cuda")
        ctr = torch.tensor([5], dtype=torch.long, device="cuda")
        s0, r0 = stage.clone(), ring.clone()
        ops.decode_advance(logits, s0, r0, ctr)
        samp = _samp_block([0.0] * b, [0.9] * b, [5] * b,
                           list(range(b))).cuda()
        ops.decode_sample_advance(logits, stage, ring, ctr, samp)
        torch.cuda.synchronize()
        assert int(stage[0, 0]) == 7
        assert torch.equal(stage, s0), (b, V)
        assert torch.equal(ring, r0), (b, V)


def test_mixed_batch_state_bump():
    b, V, chunk = 8, 4096, 4
    logits = _rows(4, V)[[0, 1, 2, 3, 0, 1, 2, 3]].contiguous().cuda()
    Ts = [0.0, 0.8, 0.0, 1.0, 0.7, 0.0, 1.3, 0.0]
    ps = [1.0, 0.9, 0.5, 1.0, 0.95, 1.0, 0.8, 1.0]
    ks = [0, 40, 3, 0, 0, 0, 100, 7]
    seeds = [(1 << 40) + 17 * i for i in range(b)]
    stage = torch.randint(0, 100, (6, b), dtype=torch.int32, device="cuda")
    ring = torch.full((chunk, b), -1, dtype=torch.long, device="cuda")
    ctr = torch.tensor([6], dtype=torch.long, device="cuda")
    before = stage.clone()
    g_stage, g_ring = stage.clone(), ring.clone()
    ops.decode_advance(logits, g_stage, g_ring, ctr)
    want, _ = ops.sample_tokens(logits, Ts, ps, ks, seeds,
                                before[1].tolist())
    ops.decode_sample_advance(logits, stage, ring, ctr,
                              _samp_block(Ts, ps, ks, seeds).cuda())
    torch.cuda.synchronize()
    greedy = [i for i in range(b) if Ts[i] == 0]
    assert torch.equal(stage[:, greedy], g_stage[:, greedy])
    assert torch.equal(ring[:, greedy], g_ring[:, greedy])
    # the reference chain of the state bump, all rows
    assert torch.equal(stage[0], want.int())
    assert torch.equal(ring[6 % chunk], want)
    rest = [r for r in range(chunk) if r != 6 % chunk]
    assert bool((ring[rest] == -1).all())
    for r in (1, 3, 4):
        assert torch.equal(stage[r], before[r] + 1)
    for r in (2, 5):
        assert torch.equal(stage[r], before[r])
    # sampled rows draw what the reference admits at counter = stage[1]
    for i in range(b):
        if Ts[i] == 0:
            continue
        r = ops.sample_row_reference(
            logits[i].cpu(), float(torch.tensor(Ts[i], dtype=torch.float32)),
            float(torch.tensor(ps[i], dtype=torch.float32)), ks[i],
            seeds[i], int(before[1, i]))
        assert bool(_admissible(r)[int(want[i])]), i


def test_hazard_rows():
    V = 1000
    base = _rows(3, V)[0].clone()
    rows = {
        "all_neg_inf": torch.full((V,), NEG_INF).bfloat16(),
        "has_nan": base.clone(),
        "all_nan": torch.full((V,), float("nan")).bfloat16(),
        "all_equal": torch.full((V,), 1.5).bfloat16(),
        "plus_inf": base.clone(),
        "plain": base,
    }
    rows["has_nan"][123] = float("nan")
    rows["plus_inf"][77] = float("inf")
    params = [(1.0, 0.0, 0), (1.0, 1.0, 1), (0.9, 0.9, 40), (1.0, 1.0, 0),
              (1e-30, 1.0, 0), (1e30, 0.5, 0)]
    names, Ts, ps, ks, ctrs = [], [], [], [], []
    for name in rows:
        for (T, p, k) in params:
            for c in (0, 2 ** 31 - 1):
                names.append(name), Ts.append(T), ps.append(p)
                ks.append(k), ctrs.append(c)
    logits = torch.stack([rows[n] for n in names])
    toks, tau = ops.sample_tokens(logits.cuda(), Ts, ps, ks, 99, ctrs)
    toks = toks.tolist()
    for i, j in enumerate(toks):
        assert 0 <= j < V, (names[i], j)
        r = ops.sample_row_reference(
            rows[names[i]], float(torch.tensor(Ts[i], dtype=torch.float32)),
            float(torch.tensor(ps[i], dtype=torch.float32)), ks[i], 99,
            ctrs[i])
        if r["kept"] is None:       # degenerate row: the argmax rule
            assert j == r["token"], (names[i], j, r["token"])
            assert float(tau[i]) == NEG_INF
        else:
            assert bool(r["kept"][j]), (names[i], Ts[i], ps[i], ks[i], j)
            assert bool(_admissible(r)[j]), (names[i], Ts[i], ps[i], ks[i])
    first = {n: names.index(n) for n in rows}
    assert toks[first["all_neg_inf"]] == 0
    assert toks[first["all_nan"]] == 0
    # top_p = 0 and top_k = 1 keep only the maximum value
    for j in toks[first["plain"]:first["plain"] + 4]:
        assert float(base[j]) == float(base.float().max())
    assert len(toks) == 2 * len(params) * len(rows)


def test_batch_invariance_and_determinism():
    V = 4096
    rows = _rows(4, V)
    one = rows[1:2].contiguous().cuda()
    many = rows[[0, 2, 3, 0, 2, 1, 3, 0]].contiguous().cuda()  # row 5 = 1
    args = (0.9, 0.95, 50)
    seeds8 = [5, 6, 7, 8, 9, 424242, 10, 11]
    ctr8 = [1, 2, 3, 4, 5, 77, 6, 7]
    a, _ = ops.sample_tokens(one, *args, 424242, 77)
    m1, t1 = ops.sample_tokens(many, *args, seeds8, ctr8)
    m2, t2 = ops.sample_tokens(many, *args, seeds8, ctr8)
    assert int(a[0]) == int(m1[5])
    assert torch.equal(m1, m2) and torch.equal(t1, t2)


def test_binding_checks():
    logits = torch.zeros(2, 64, dtype=torch.bfloat16, device="cuda")
    stage = torch.zeros(6, 2, dtype=torch.int32, device="cuda")
    ring = torch.zeros(4, 2, dtype=torch.long, device="cuda")
    ctr = torch.zeros(1, dtype=torch.long, device="cuda")
    samp = torch.zeros(5, 2, dtype=torch.int32, device="cuda")
    ops.decode_sample_advance(logits, stage, ring, ctr, samp)
    for bad in [
        dict(logits=logits.float()), dict(stage=stage[:5].contiguous()),
        dict(samp=torch.zeros(4, 2, dtype=torch.int32, device="cuda")),
        dict(samp=samp.long()), dict(ring=ring[:, :1].contiguous()),
        dict(ring=ring.int()), dict(stage=stage.t().contiguous().t()),
    ]:
        kw = dict(logits=logits, stage=stage, ring=ring, ctr=ctr, samp=samp)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.native().decode_sample_advance(
                kw["logits"], kw["stage"], kw["ring"], kw["ctr"],
                kw["samp"])
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.native().sample_tokens(logits, samp, cnt)
    with pytest.raises(RuntimeError):
        ops.native().sample_tokens(logits, samp, cnt.long())
    with pytest.raises(RuntimeError):
        ops.native().sample_tokens(logits, samp[:, :1].contiguous(), cnt)
    # V is bounded so that a row's 2^40-scaled weights cannot wrap 64 bits
    wide = torch.zeros(1, 2 ** 23 + 8, dtype=torch.bfloat16, device="cuda")
    one = torch.zeros(5, 1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="2\\^23"):
        ops.native().sample_tokens(wide, one, cnt[:1].contiguous())
    with pytest.raises(RuntimeError, match="2\\^23"):
        ops.native().decode_sample_advance(
            wide, stage[:, :1].contiguous(), ring[:, :1].contiguous(), ctr,
            one)


# ------------------------------ engine -------------------------------------
def _engine(chunk=None, **kw):
    from skypilot_amd.serve.engine import Engine
    eng = Engine("llama-smoke", device="cuda:0", max_seq=256, max_batch=2,
                 **kw)
    if chunk is not None:
        eng.CHUNK = chunk
    eng.start()
    return eng


PROMPT = list(range(1, 33))
SAMPLED = dict(max_tokens=24, temperature=0.9, top_p=0.9, top_k=40, seed=7)


def test_engine_sampling_in_graph():
    eng = _engine(device_sampling=True)
    calls = []
    step = eng._decode_step

    def counted():
        calls.append(1)
        return step()

    eng._decode_step = counted
    try:
        assert eng.CHUNK == 8
        out1 = eng.generate(PROMPT, **SAMPLED)
        n_first = len(calls)
        out2 = eng.generate(PROMPT, **SAMPLED)
        greedy_on = eng.generate(PROMPT, max_tokens=24)
        assert eng.stats["graph_buckets"]
    finally:
        eng.stop()
    assert out1 == out2 and len(out1) == 24
    # 23 decode tokens in chains of 8: the sampled request chained
    assert n_first <= math.ceil(23 / 8), n_first
    assert len(calls) <= 3 * math.ceil(23 / 8)

    eng = _engine(chunk=1, device_sampling=True)
    try:
        out_c1 = eng.generate(PROMPT, **SAMPLED)
    finally:
        eng.stop()
    assert out_c1 == out1

    eng = _engine()
    try:
        greedy_off = eng.generate(PROMPT, max_tokens=24)
    finally:
        eng.stop()
    assert greedy_on == greedy_off
    assert out1 != greedy_off    # the sampled request did sample
