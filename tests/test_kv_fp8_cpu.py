"""FP8 KV cache on the CPU: ops.kv_quantize / kv_dequantize against the
format's definition (written here independently, from e4m3fn_table), the
cache's sizing, and the model and engine with kv_dtype="fp8": what each
write path (whole-prompt prefill, chunked prefill, decode, follower replay)
leaves in the cache.

The helpers at the top (definition, special rows, the layer-0 recomputation)
are also what tests/test_kv_fp8_gpu.py checks the kernels against."""
import math

import pytest
import torch

from skypilot_amd import ops
from skypilot_amd.models.llama import CONFIGS, build_model
from skypilot_amd.serve.engine import Engine, InferenceContext, Request
from skypilot_amd.serve.kv_cache import KVCache
from test_gpu_decode_kernels import e4m3fn_table

D = 128
TABLE = e4m3fn_table()
FINITE = [b for b in range(256) if b not in (0x7F, 0xFF)]
POS = TABLE[:0x7F]                      # 0 .. 448, ascending with the code


def canon(codes):
    """-0 may be stored as either zero code: compare with 0x80 as 0x00."""
    return torch.where(codes == 0x80, torch.zeros_like(codes), codes)


def assert_codes_equal(got, want, what):
    g, w = canon(got.cpu()), canon(want.cpu())
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} of {g.numel()} bytes differ, first at "
        f"{tuple(bad[0].tolist())}: got {int(g[tuple(bad[0])])}, want "
        f"{int(w[tuple(bad[0])])}")


def exponent_by_definition(amax):
    """Smallest n with amax <= 448 * 2^n in [-126, 127]; 0 for amax 0."""
    if amax == 0:
        return 0
    n = -126
    while n < 127 and amax > 448.0 * 2.0 ** n:
        n += 1
    return n


def code_by_definition(y):
    """e4m3fn code of y (|y| <= 448) from the table: the nearest value,
    ties to the even code."""
    a = abs(y)
    i = int(torch.searchsorted(POS, torch.tensor(a, dtype=torch.float64)))
    if i == len(POS):
        i -= 1
    if i > 0:
        lo, hi = float(POS[i - 1]), float(POS[i])
        if a - lo < hi - a or (a - lo == hi - a and (i - 1) % 2 == 0):
            i -= 1
    return i | (0x80 if math.copysign(1.0, y) < 0 else 0)


def quantize_by_definition(x):
    """x [rows, width] -> (codes, exp) in fp64 / exact integer steps."""
    x = x.double()
    codes = torch.zeros(x.shape, dtype=torch.uint8)
    exps = torch.zeros(x.shape[0], dtype=torch.uint8)
    for r in range(x.shape[0]):
        n = exponent_by_definition(float(x[r].abs().max()))
        exps[r] = n + 127
        for i in range(x.shape[1]):
            codes[r, i] = code_by_definition(float(x[r, i]) * 2.0 ** -n)
    return codes, exps


def all_code_rows(n):
    """Two rows of 128 holding the 254 finite codes times 2^n (codes
    0x00..0x7E and 0x80..0xFE, each padded with one zero): +-448 are there,
    so each row's scale is exactly 2^n.  -> (values fp32, codes)."""
    codes = torch.tensor([list(range(0x00, 0x7F)) + [0],
                          list(range(0x80, 0xFF)) + [0]], dtype=torch.uint8)
    return (TABLE[codes.long()] * 2.0 ** n).float(), codes


def tie_row():
    """448 and four bf16-representable midpoints -> (values, codes)."""
    vals = torch.zeros(1, D)
    want = torch.zeros(1, D, dtype=torch.uint8)
    code_of = {float(TABLE[b]): b for b in range(0x7F)}
    for i, (v, to) in enumerate([(448.0, 448.0), (1.0625, 1.0),
                                 (1.1875, 1.25), (2.0 ** -10, 0.0),
                                 (3 * 2.0 ** -10, 2.0 ** -8),
                                 (-1.0625, -1.0), (-3 * 2.0 ** -10,
                                                   -2.0 ** -8)]):
        vals[0, i] = v
        want[0, i] = code_of[abs(to)] | (0x80 if to < 0 else 0)
    assert torch.equal(vals.bfloat16().float(), vals)
    return vals, want


# ------------------------------------------------------------- the format
@pytest.mark.parametrize("n", [-20, 0, 9])
def test_all_finite_codes_round_trip(n):
    row = (TABLE[FINITE] * 2.0 ** n).float()[None]      # one row of 254
    assert n != 0 or float(row.abs().max()) == 448.0
    codes, exp = ops.kv_quantize(row)
    assert int(exp[0]) == n + 127
    assert_codes_equal(codes[0], torch.tensor(FINITE, dtype=torch.uint8),
                       f"all codes, n={n}")
    back = ops.kv_dequantize(codes, exp)
    assert torch.equal(back, row)
    assert back.dtype == torch.float32
    # the two 128-wide rows the GPU test uses
    vals, want = all_code_rows(n)
    codes, exp = ops.kv_quantize(vals.bfloat16())
    assert exp.tolist() == [n + 127] * 2
    assert_codes_equal(codes, want, f"all-code rows, n={n}")


def test_exponent_edges():
    row = torch.zeros(3, D)
    row[0, 5] = 450.0           # just past 448: the next power of two
    row[1, 7] = -448.0
    codes, exp = ops.kv_quantize(row)
    assert exp.tolist() == [128, 127, 127]
    assert torch.count_nonzero(codes[2]) == 0      # zero row: codes 0, e 127
    assert int(codes[1, 7]) == 0xFE and int(codes[0, 5]) == code_by_definition(
        225.0)
    # the bit formula against the definition around every boundary
    for k in (-130, -126, -125, -3, 0, 1, 100, 119):
        for a in (448.0 * 2.0 ** k, 448.0 * 2.0 ** k * (1 + 2.0 ** -23),
                  448.0 * 2.0 ** k * (1 - 2.0 ** -24)):
            a32 = torch.tensor(a, dtype=torch.float32)
            if not torch.isfinite(a32) or a32 == 0:
                continue
            r = torch.zeros(1, D)
            r[0, 0] = a32
            want = exponent_by_definition(float(a32.double())) + 127
            assert int(ops.kv_quantize(r)[1][0]) == want, (k, a)


def test_ties_go_to_even():
    vals, want = tie_row()
    codes, exp = ops.kv_quantize(vals.bfloat16())
    assert int(exp[0]) == 127
    assert_codes_equal(codes, want, "tie row")


@pytest.mark.parametrize("mult", [1e-3, 1.0, 37.0, 449.0])
def test_random_rows(mult):
    g = torch.Generator().manual_seed(int(mult * 1000) % 9973)
    x = (torch.randn(24, D, generator=g) * mult).bfloat16()
    codes, exp = ops.kv_quantize(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape
    assert exp.dtype == torch.uint8 and exp.shape == x.shape[:-1]
    want_c, want_e = quantize_by_definition(x)
    assert torch.equal(exp, want_e)
    assert_codes_equal(codes, want_c, f"random rows x{mult}")
    s = 2.0 ** (exp.double() - 127)
    ratio = x.double().abs().amax(-1) / s
    assert bool((ratio > 224).all()) and bool((ratio <= 448).all())
    deq = ops.kv_dequantize(codes, exp)
    err = (deq.double() - x.double()).abs()
    bound = torch.maximum(2.0 ** -4 * x.double().abs(),
                          (2.0 ** -10 * s)[:, None])
    assert bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(deq.bfloat16().float(), deq)


def test_quantize_keeps_leading_dims_and_takes_fp32():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 4, D, generator=g)           # fp32, unrounded
    codes, exp = ops.kv_quantize(x)
    want_c, want_e = quantize_by_definition(x.reshape(-1, D))
    assert torch.equal(exp.reshape(-1), want_e)
    assert_codes_equal(codes.reshape(-1, D), want_c, "fp32 rows")


# ------------------------------------------------------------------ sizing
def test_bytes_needed_and_sizing():
    cfg = CONFIGS["llama3-8b"]
    assert KVCache.bytes_needed(cfg, 1, 1) == 131072
    assert KVCache.bytes_needed(cfg, 1, 1, "bf16") == 131072
    assert KVCache.bytes_needed(cfg, 1, 1, "fp8") == 66048
    assert KVCache.bytes_needed(cfg, 3, 5, "fp8") == (
        2 * cfg.num_layers * 3 * 5 * cfg.num_kv_heads * (128 + 1))
    small = CONFIGS["llama-debug"]
    budget = 40 * KVCache.bytes_needed(small, 1, 64) + 1234
    a = KVCache.sized_for_memory(small, 64, budget, "cpu")
    b = KVCache.sized_for_memory(small, 64, budget, "cpu", kv_dtype="fp8")
    assert a.max_batch == 40 and a.kv_dtype == "bf16"
    assert b.max_batch >= math.floor(1.9 * a.max_batch)
    assert KVCache.bytes_needed(small, b.max_batch, 64, "fp8") <= budget
    assert b.k[0].dtype == torch.uint8
    assert b.k[0].shape == (b.max_batch, 64, 1, 128)
    assert b.k_exp[0].shape == b.v_exp[1].shape == (b.max_batch, 64, 1)
    assert a.k[0].dtype == torch.bfloat16 and a.k_exp == []


# ------------------------------------------------------- the ops' CPU paths
def test_kv_write_fp8_cpu_rules():
    g = torch.Generator().manual_seed(5)
    n, S, Hkv, slots, S_max = 5, 8, 2, 3, 10
    k = torch.randn(n, S, Hkv, D, generator=g).bfloat16()
    v = torch.randn(n, S, Hkv, D, generator=g).bfloat16()
    kc = torch.full((slots, S_max, Hkv, D), 0x7F, dtype=torch.uint8)
    vc, ke = kc.clone(), torch.full((slots, S_max, Hkv), 0xFF,
                                    dtype=torch.uint8)
    ve = ke.clone()
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    # full rows; overflow past S_max dropped; bad slots / start skipped
    ops.kv_write_fp8(k, v, kc, vc, ke, ve, i32([0, 2, -1, 3, 1]),
                     i32([0, 5, 0, 0, -2]), i32([3, 8, 8, 8, 8]))
    wc, we = ops.kv_quantize(k)
    assert torch.equal(kc[0, :3], wc[0, :3]) and torch.equal(ke[0, :3],
                                                             we[0, :3])
    assert torch.equal(kc[2, 5:], wc[1, :5]) and torch.equal(ke[2, 5:],
                                                             we[1, :5])
    assert torch.equal(vc[2, 5:], ops.kv_quantize(v)[0][1, :5])
    assert bool((kc[0, 3:] == 0x7F).all()) and bool((ke[0, 3:] == 0xFF).all())
    assert bool((kc[1] == 0x7F).all()) and bool((ve[1] == 0xFF).all())
    assert bool((kc[2, :5] == 0x7F).all())


def test_attn_decode_qkv_fp8_cpu_is_write_then_attend():
    g = torch.Generator().manual_seed(6)
    B, Hq, Hkv, slots, S_max = 3, 4, 2, 4, 12
    lens = [1, 5, 12]
    sl = torch.tensor([3, 0, 2], dtype=torch.int32)
    kc = torch.full((slots, S_max, Hkv, D), 0x7F, dtype=torch.uint8)
    vc = kc.clone()
    ke = torch.full((slots, S_max, Hkv), 0xFF, dtype=torch.uint8)
    ve = ke.clone()
    for b, L in enumerate(lens):
        s = int(sl[b])
        kc[s, :L - 1], ke[s, :L - 1] = ops.kv_quantize(
            torch.randn(L - 1, Hkv, D, generator=g))
        vc[s, :L - 1], ve[s, :L - 1] = ops.kv_quantize(
            torch.randn(L - 1, Hkv, D, generator=g))
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).bfloat16()
    half = D // 2
    fr = torch.outer(torch.arange(S_max).float(),
                     1.0 / 10000 ** (torch.arange(half).float() / half))
    cos, sin = fr.cos(), fr.sin()
    pos = torch.tensor(lens, dtype=torch.int32) - 1
    kvl = torch.tensor(lens, dtype=torch.int32)
    out = ops.attn_decode_qkv_fp8(qkv, kc, vc, ke, ve, cos, sin, pos, kvl, sl,
                                  Hq, Hkv, D ** -0.5)
    assert out.shape == (B, Hq, D) and out.dtype == torch.bfloat16
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], -1)
    kr = ops.rope_ref(k.reshape(B, Hkv, D).float(), cos, sin, pos.long())
    wc, we = ops.kv_quantize(kr)
    assert torch.equal(kc[sl.long(), pos.long()], wc)
    assert torch.equal(ke[sl.long(), pos.long()], we)
    assert torch.equal(vc[sl.long(), pos.long()],
                       ops.kv_quantize(v.reshape(B, Hkv, D))[0])
    qr = ops.rope_ref(q.reshape(B, Hq, D).float(), cos, sin, pos.long())
    ref = ops.attn_decode_ref(qr, ops.kv_dequantize(kc, ke),
                              ops.kv_dequantize(vc, ve), kvl, sl, D ** -0.5)
    assert torch.equal(out, ref.bfloat16())
    # kv_len 1: the dequantised current v
    want = ops.kv_dequantize(vc, ve)[3, 0].bfloat16()
    assert torch.equal(out[0], want.repeat_interleave(Hq // Hkv, 0))


# -------------------------------------------------------- model and engine
@pytest.fixture(scope="module")
def model():
    return build_model("llama-debug")


PROMPT = [(7 * i + 3) % 500 + 1 for i in range(100)]   # crosses one chunk


def layer0_rows(model, toks, positions):
    """K (roped, bf16) and V rows of layer 0 for a prefill / append
    forward over toks [1, S] at `positions` [S]: embedding -> norm ->
    wk / wv -> rope, through the same ops as Attention.forward."""
    blk, cfg = model.blocks[0], model.cfg
    cos, sin = model._tables(toks.device)
    lin = torch.nn.functional.linear
    h = ops.rmsnorm(model.embed(toks), blk.attn_norm, blk.eps)
    S, d = toks.shape[1], cfg.head_dim
    k = lin(h, blk.attn.wk.weight, blk.attn.wk.bias).view(
        1, S, cfg.num_kv_heads, d)
    v = lin(h, blk.attn.wv.weight, blk.attn.wv.bias).view(
        1, S, cfg.num_kv_heads, d)
    k = ops.rope(k.reshape(S, cfg.num_kv_heads, d), cos, sin,
                 positions).view(1, S, cfg.num_kv_heads, d)
    return k[0], v[0]


def expected_prompt_rows(model, ids, chunk, device="cpu"):
    """kv_quantize of the layer-0 prompt rows, recomputed chunk by chunk
    with the engine's padding (whole prompt when chunk is None)."""
    parts, done = [], 0
    while done < len(ids):
        ln = len(ids) - done if chunk is None else min(chunk, len(ids) - done)
        S = max(64, (ln + 63) // 64 * 64)
        toks = torch.zeros(1, S, dtype=torch.long, device=device)
        toks[0, :ln] = torch.tensor(ids[done:done + ln], device=device)
        positions = (done + torch.arange(S, dtype=torch.int32,
                                         device=device)).clamp_(
            max=model.cfg.max_seq_len - 1)
        k, v = layer0_rows(model, toks, positions)
        parts.append((k[:ln], v[:ln]))
        done += ln
    k = torch.cat([p[0] for p in parts])
    v = torch.cat([p[1] for p in parts])
    return ops.kv_quantize(k), ops.kv_quantize(v)


def check_prompt_rows(model, cache, slot, ids, chunk, device="cpu"):
    (kc, ke), (vc, ve) = expected_prompt_rows(model, ids, chunk, device)
    L = len(ids)
    assert_codes_equal(cache.k[0][slot, :L], kc, "layer-0 K codes")
    assert torch.equal(cache.k_exp[0][slot, :L].cpu(), ke.cpu())
    assert_codes_equal(cache.v[0][slot, :L], vc, "layer-0 V codes")
    assert torch.equal(cache.v_exp[0][slot, :L].cpu(), ve.cpu())


def expected_decode_row(model, tok, pos):
    """Layer-0 row of one decode step on the CPU path: the packed qkv
    GEMV of the normed embedding, k roped in fp32, both quantised."""
    blk, cfg = model.blocks[0], model.cfg
    cos, sin = model._tables(torch.device("cpu"))
    x = model.embed(torch.tensor([[tok]]))
    _, qkv = ops.decode_norm_linear(x, None, blk.attn_norm, blk.eps,
                                    blk.attn.packed_qkv())
    d, Hq, Hkv = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    _, k, v = qkv.reshape(1, -1).split([Hq * d, Hkv * d, Hkv * d], -1)
    kr = ops.rope_ref(k.reshape(1, Hkv, d).float(), cos, sin,
                      torch.tensor([pos]))
    return ops.kv_quantize(kr[0]), ops.kv_quantize(v.reshape(Hkv, d))


def run_one(model, kv_dtype, chunk, max_tokens=6, **kw):
    eng = Engine("llama-debug", device="cpu", max_seq=256, max_batch=3,
                 prefill_chunk=chunk, model=model, kv_dtype=kv_dtype, **kw)
    plans = []
    eng._tp_bcast = plans.append
    req = eng.submit(Request(prompt_ids=list(PROMPT), max_tokens=max_tokens))
    eng.start()
    try:
        assert req.done.wait(120), "request did not complete"
    finally:
        eng.stop()
    return eng, req, plans


@pytest.fixture(scope="module")
def fp8_runs(model):
    return {chunk: run_one(model, "fp8", chunk) for chunk in (None, 64)}


def test_first_token_and_logits_do_not_depend_on_the_cache(model, fp8_runs):
    """Whole-prompt prefill attends the unquantised K/V."""
    cfg = model.cfg
    pad = (len(PROMPT) + 63) // 64 * 64
    toks = torch.zeros(1, pad, dtype=torch.long)
    toks[0, :len(PROMPT)] = torch.tensor(PROMPT)
    positions = torch.arange(pad, dtype=torch.int32)
    logits = {}
    with torch.no_grad():
        for kd in ("bf16", "fp8"):
            cache = KVCache(cfg, 2, 256, "cpu", kv_dtype=kd)
            ctx = InferenceContext(cache=cache, mode="prefill",
                                   prefill_slots=[1],
                                   prefill_lens=[len(PROMPT)])
            logits[kd] = model(toks, positions, ctx)
    assert torch.equal(logits["fp8"], logits["bf16"])
    _, req8, _ = fp8_runs[None]
    _, req16, _ = run_one(model, "bf16", None, max_tokens=1)
    assert req8.out_ids[0] == req16.out_ids[0]
    assert req8.out_ids[0] == int(
        logits["bf16"][0, len(PROMPT) - 1].argmax())


@pytest.mark.parametrize("chunk", [None, 64])
def test_layer0_cache_contents(model, fp8_runs, chunk):
    eng, req, plans = fp8_runs[chunk]
    assert len(req.out_ids) == 6
    first = plans[0]
    assert first["op"] == ("prefill" if chunk is None else "append")
    slot = first["slots"][0]
    if chunk is not None:
        appends = [p for p in plans if p["op"] == "append"]
        assert [p["lens"][0] for p in appends] == [64, 36]
    with torch.no_grad():
        check_prompt_rows(model, eng.cache, slot, PROMPT, chunk)
        # decode-written rows: token i is fed at position len + i
        L = len(PROMPT)
        for i, tok in enumerate(req.out_ids[:-1]):
            (kc, ke), (vc, ve) = expected_decode_row(model, tok, L + i)
            what = f"decode row {L + i}"
            assert_codes_equal(eng.cache.k[0][slot, L + i], kc, what + " K")
            assert torch.equal(eng.cache.k_exp[0][slot, L + i], ke), what
            assert_codes_equal(eng.cache.v[0][slot, L + i], vc, what + " V")
            assert torch.equal(eng.cache.v_exp[0][slot, L + i], ve), what
    # nothing past the last fed token, nothing in the other slots
    end = L + len(req.out_ids) - 1
    for layer in range(model.cfg.num_layers):
        for codes, exps in ((eng.cache.k, eng.cache.k_exp),
                            (eng.cache.v, eng.cache.v_exp)):
            assert torch.count_nonzero(codes[layer][slot, end:]) == 0
            assert bool((exps[layer][slot, end:] == 127).all())
            for other in set(range(3)) - {slot}:
                assert torch.count_nonzero(codes[layer][other]) == 0


@pytest.mark.parametrize("chunk", [None, 64])
def test_follower_replay_leaves_the_leaders_cache(model, fp8_runs, chunk):
    lead, _, plans = fp8_runs[chunk]
    ops_seen = {p["op"] for p in plans}
    assert ops_seen == {"prefill" if chunk is None else "append", "decode"}
    fol = Engine("llama-debug", device="cpu", max_seq=256, max_batch=3,
                 prefill_chunk=chunk, model=model, kv_dtype="fp8")
    for p in plans:
        if p["op"] == "prefill":
            fol._follow_prefill(p)
        elif p["op"] == "append":
            fol._follow_append(p)
        elif p["op"] == "decode":
            fol._follow_decode(p)
    for layer in range(model.cfg.num_layers):
        for name in ("k", "v", "k_exp", "v_exp"):
            assert torch.equal(getattr(fol.cache, name)[layer],
                               getattr(lead.cache, name)[layer]), (layer,
                                                                   name)


def test_fp8_and_bf16_engines_agree_mostly(model, fp8_runs):
    """Not a bound on quantisation error (none can be derived): the run
    completes and the greedy tokens are printed beside the bf16 ones."""
    _, req8, _ = fp8_runs[None]
    _, req16, _ = run_one(model, "bf16", None)
    same = sum(a == b for a, b in zip(req8.out_ids, req16.out_ids))
    print(f"fp8 vs bf16 cache: {same}/6 greedy tokens equal")
    assert len(req8.out_ids) == len(req16.out_ids) == 6


# ---------------------------------------------------------------- validation
def test_engine_rejects_unknown_kv_dtype():
    for bad in ("int4", "fp16", None, 8):
        with pytest.raises(ValueError, match="kv_dtype"):
            Engine("llama-debug", device="cpu", max_seq=64, max_batch=2,
                   kv_dtype=bad)
    with pytest.raises(ValueError, match="kv_dtype"):
        KVCache(CONFIGS["llama-debug"], 1, 8, "cpu", kv_dtype="int4")


def test_entrypoint_parses_kv_dtype():
    from skypilot_amd.serve.entrypoint import build_parser
    assert build_parser().parse_args([]).kv_dtype == "bf16"
    assert build_parser().parse_args(["--kv-dtype", "fp8"]).kv_dtype == "fp8"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--kv-dtype", "int4"])


# ------------------------------------------------------- tensor parallelism
def _tp_fp8_worker(rank, world, port, q):
    import os
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from skypilot_amd.parallel.tp import build_tp_model
        shard = build_tp_model("llama-smoke", tp=world, rank=rank,
                               device="cpu", seed=3)
        eng = Engine("llama-smoke", device="cpu", max_seq=128, max_batch=2,
                     model=shard, tp_rank=rank, tp_world=world,
                     kv_dtype="fp8")
        assert eng.cache.kv_dtype == "fp8"
        assert eng.cache.k[0].shape[2] == shard.cfg_shard.num_kv_heads
        if rank > 0:
            eng.follower_loop()  # exits on the leader's stop broadcast
        else:
            eng.start()
            out = eng.generate([5, 9, 200, 3], max_tokens=4)
            eng.stop()
            assert len(out) == 4
        # prompt and decode rows are in the slot, as codes and exponents
        slot = eng.cache.max_batch - 1
        assert bool((eng.cache.k[0][slot, :7] != 0).any(-1).all())
        assert torch.count_nonzero(eng.cache.k[0][slot, 7:]) == 0
        codes = eng.cache.k[0][slot, :7].clone()
        q.put((rank, "ok", codes if rank == 0 else None))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, f"{e}\n{traceback.format_exc()}", None))
    finally:
        dist.destroy_process_group()


def test_tp_leader_and_follower_with_fp8_cache():
    """TP=2 over gloo with kv_dtype="fp8": the follower is built with the
    same value, mirrors the plans and ends with its shard's rows."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_fp8_worker, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    for rank, res, _ in results:
        assert res == "ok", f"rank {rank}: {res}"
