"""ops.skinny_gemm_bf16_mfma (skinny_gemm_bf16_mfma.hip): the bf16-weight
decode GEMM on the matrix cores, against fp64 element by element, its exact k
mapping, its batch invariance, its routing and the engine."""
import pytest
import torch

from skypilot_amd import ops
from _fp64_check import check, tol_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(n, I, O, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ((0.5 * torch.randn(n, I, generator=g)).bfloat16(),
            (0.05 * torch.randn(O, I, generator=g)).bfloat16())


def _run(x, w, tr=0, ks=0):
    return ops.skinny_gemm_bf16_mfma(x.to(DEV), w.to(DEV), tr, ks).cpu()


# I = 128: one chunk (ring and second LDS buffer idle; k_splits 2 and 4 leave
# blocks with no chunk); 640 and 4224: 5 and 33 chunks, which neither the ring
# depth nor any k_splits divides, the steady loop and every tail length.
# O = 16, 80, 272: 1, 5 and 17 row tiles, fewer than one block and counts no
# 64*TR divides.  n covers every NT, full and ragged.  The 0, 0 rows take the
# launcher's choice, the last four on both sides of its two row-tile
# thresholds (two tiles for 6144 <= O < 65536); _PLAN_KS is the k split count
# its rule gives them (the fewest of 1, 2, 4, 8 that make 192 blocks).
_PLAN_KS = {272: 8, 6128: 2, 6160: 4, 65520: 1, 65552: 1}


@pytest.mark.parametrize("n,I,O,tr,ks", [
    (1, 128, 16, 1, 1), (3, 128, 16, 2, 4), (64, 128, 16, 4, 2),
    (16, 640, 80, 1, 2), (17, 640, 80, 2, 1), (48, 640, 80, 4, 4),
    (1, 4224, 272, 1, 4), (3, 4224, 272, 2, 2), (17, 4224, 272, 4, 1),
    (48, 4224, 272, 2, 4), (64, 4224, 272, 1, 2), (64, 4224, 272, 4, 4),
    (64, 4224, 272, 0, 0), (3, 640, 6128, 0, 0), (48, 640, 6160, 0, 0),
    (33, 128, 65520, 0, 0), (17, 128, 65552, 0, 0),
])
def test_fp64_elementwise(n, I, O, tr, ks):
    x, w = _inputs(n, I, O, seed=n + I + O)
    ref = x.double() @ w.double().t()
    A = x.double().abs() @ w.double().abs().t()
    check(f"bf16 mfma n={n} I={I} O={O} tr={tr} ks={ks}", _run(x, w, tr, ks),
          ref, tol_bf16(ref, A, K=I + (ks or _PLAN_KS[O]), roundings=1))


@pytest.mark.parametrize("ks", [1, 4])
def test_one_hot_rows_return_the_weights(ks):
    """X[t, k_t] = 1 with k_t running over every k of 5 chunks, 64 rows at a
    time: Y[t, :] is W[:, k_t] exactly, which pins the W lane mapping against
    the order X is staged in LDS for every k."""
    I = 640
    _, w = _inputs(1, I, 80, seed=7)
    eye = torch.eye(I).bfloat16()
    got = torch.cat([_run(eye[k:k + 64].contiguous(), w, 0, ks)
                     for k in range(0, I, 64)])
    assert torch.equal(got.float(), w.t().float())


def test_batch_invariance_and_isolation():
    """At the launcher's own choice (k splits > 1 for this shape, so the
    partials and the combine kernel run)."""
    x, w = _inputs(64, 4224, 272, seed=3)
    y64 = _run(x, w)
    for t in (0, 16, 17, 63):
        assert torch.equal(_run(x[t:t + 1], w)[0], y64[t]), t
    assert torch.equal(_run(x[:17], w), y64[:17])
    xd, wd = x.to(DEV), w.to(DEV)

    def scratch():   # the binding's two allocations, in its order (8 k splits)
        return (torch.empty(64, 272, dtype=torch.bfloat16, device=DEV),
                torch.empty(8, 64, 272, device=DEV))
    scratch()[1].fill_(float("nan"))
    # freed, the caching allocator hands the same blocks out again: the
    # partials of the next call come out of NaN memory
    assert scratch()[1].isnan().all()
    assert torch.equal(ops.skinny_gemm_bf16_mfma(xd, wd).cpu(), y64)
    x[5] = float("nan")
    ynan = _run(x, w)
    keep = torch.arange(64) != 5
    assert torch.equal(ynan[keep], y64[keep])
    assert ynan[5].isnan().all()


def test_decode_linear_routing(monkeypatch):
    """First the measured table as it stands (docs/BENCHMARKS.md: "deep" at
    NT = 3): 40 rows on a [16, 8320] weight.  Then the table is patched to
    one entry, "square" at NT = 1, so that the rest does not move with it: a
    routed (class, NT) returns the op's bits; an unrouted NT, an unrouted
    class and any n above m keep the old ones."""
    g = torch.Generator().manual_seed(11)
    deep = (0.05 * torch.randn(16, 8320, generator=g)).bfloat16().to(DEV)
    xd = (0.5 * torch.randn(40, 8320, generator=g)).bfloat16().to(DEV)
    w = (0.05 * torch.randn(512, 1024, generator=g)).bfloat16().to(DEV)
    wide = (0.05 * torch.randn(16384, 128, generator=g)).bfloat16().to(DEV)
    xs = {n: (0.5 * torch.randn(n, 1024, generator=g)).bfloat16().to(DEV)
          for n in (1, 4, 9, 17)}
    xw = xs[4][:, :128].contiguous()
    old = {n: ops.decode_linear(x, w) for n, x in xs.items()}
    oldw, oldd = ops.decode_linear(xw, wide), ops.decode_linear(xd, deep)
    assert torch.equal(oldd, torch.nn.functional.linear(xd, deep))
    for n in (1, 4):
        assert torch.equal(old[n], ops.native().skinny_gemm(xs[n], w)), n
    assert torch.equal(old[9], torch.nn.functional.linear(xs[9], w))
    for bad in (0, 65, 2.5, None, True):
        with pytest.raises(ValueError, match="set_bf16_decode_max_batch"):
            ops.set_bf16_decode_max_batch(bad)
    try:
        ops.set_bf16_decode_max_batch(64)
        assert torch.equal(ops.decode_linear(xd, deep),
                           ops.skinny_gemm_bf16_mfma(xd, deep))
        ops.set_bf16_decode_max_batch(32)
        assert torch.equal(ops.decode_linear(xd, deep), oldd)
        ops.set_bf16_decode_max_batch(64)
        monkeypatch.setattr(ops, "_BF16_MFMA_ROUTES",
                            {"wide": (), "deep": (), "square": (1,)})
        for n in (4, 9):
            assert torch.equal(ops.decode_linear(xs[n], w),
                               ops.skinny_gemm_bf16_mfma(xs[n], w)), n
        for n in (1, 17):
            assert torch.equal(ops.decode_linear(xs[n], w), old[n]), n
        assert torch.equal(ops.decode_linear(xw, wide), oldw)
        ops.set_bf16_decode_max_batch(8)
        assert torch.equal(ops.decode_linear(xs[9], w), old[9])
    finally:
        ops.set_bf16_decode_max_batch(1)


def test_binding_rejects_bad_arguments():
    x, w = (t.to(DEV) for t in _inputs(4, 256, 32))
    f = ops.skinny_gemm_bf16_mfma
    for msg, args in {
        "N must be 1..64, got 0": (x[:0], w),
        "N must be 1..64, got 65": (torch.zeros(65, 256, dtype=x.dtype,
                                                device=DEV), w),
        "I must be a positive multiple of 128":
            (x[:, :64].contiguous(), w[:, :64].contiguous()),
        "O must be a positive multiple of 16": (x, w[:24]),
        "X must start on a 16-byte": (x.reshape(-1)[1:257].view(1, 256), w),
        "W must be BFloat16": (x, w.float()),
        "W must be .O, I. with I = 256": (x, w[:, :128].contiguous()),
        "row_tiles must be 0, 1, 2 or 4, got -1": (x, w, -1),
        "row_tiles must be 0, 1, 2 or 4, got 3": (x, w, 3),
        "k_splits must be 0, 1, 2, 4 or 8, got -2": (x, w, 0, -2),
        "k_splits must be 0, 1, 2, 4 or 8, got 16": (x, w, 0, 16),
    }.items():
        with pytest.raises(RuntimeError, match="skinny_gemm_bf16_mfma: " + msg):
            f(*args)


def test_engine_graph_and_eager_agree_at_batch_4(monkeypatch):
    """Every class routed at NT = 1 for the test, so that each linear of the
    decode step that the kernel's shapes admit runs it."""
    monkeypatch.setattr(ops, "_BF16_MFMA_ROUTES",
                        {"wide": (1,), "deep": (1,), "square": (1,)})
    from skypilot_amd.models.llama import build_model
    from skypilot_amd.serve.engine import Engine, Request
    model = build_model("llama-smoke", device=DEV)
    outs = []
    try:
        for use_graphs in (True, False):
            eng = Engine("llama-smoke", device=DEV, max_seq=256, max_batch=8,
                         model=model, use_graphs=use_graphs)
            eng.enable_bf16_mfma_decode(max_batch=4)
            reqs = [eng.submit(Request(prompt_ids=[2 + i, 3, 4, 5],
                                       max_tokens=12)) for i in range(4)]
            eng.start()
            try:
                for r in reqs:
                    assert r.done.wait(120), "request did not complete"
            finally:
                eng.stop()
            if use_graphs:
                assert max(eng.stats["graph_buckets"]) >= 4
            outs.append([r.out_ids for r in reqs])
    finally:
        ops.set_bf16_decode_max_batch(1)
    assert all(len(o) == 12 for o in outs[0]) and outs[0] == outs[1]
