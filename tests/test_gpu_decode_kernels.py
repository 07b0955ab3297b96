"""Elementwise fp64 checks of the decode (serving) kernels.

skinny_gemm.hip (bf16, SwiGLU-fused, fp8, norm-fused fp8),
attention_decode.hip (attn_decode, attn_decode_qkv) and decode_fused.hip
(rmsnorm_res, rope_kvwrite, decode_advance) are compared element by
element with a plain fp64 evaluation of the same formula on the CPU, on
the same bf16-rounded (for fp8: fp8-decoded) inputs, under the tolerance
rule of docs/TESTING.md (tests/_fp64_check.py).  Wherever the result is
determined exactly - a one-hot GEMV, an fp8 byte, a copied V row, a
residual sum, a cache element that must not change - bit patterns are
compared instead.  KV-cache rows that a kernel must not read hold NaN.

Each bound is derived next to its test and was fixed before the kernels
were run against it.  `pytest -s` prints every check's worst err/tol.

The unmarked tests run without a GPU: they pin the fp64 references to the
package's own CPU paths, and they feed the checker results with one
planted defect each to show that it rejects them.
"""
import functools

import pytest
import torch

from _fp64_check import (TINY, U16, U32, bf16_values, check, f32, rejects,
                         tol_bf16, tol_f32, within)
from skypilot_amd import ops
from test_gpu_train_kernels import rope64, swiglu64

gpu = pytest.mark.gpu

D = 128
SCALE = f32(D ** -0.5)   # the kernels receive the softmax scale as fp32


def dev():
    return torch.device("cuda:0")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    """bf16 tensor -> its bit patterns (so NaN and -0 compare as stored)."""
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_bits_equal(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at "
        f"{tuple(bad[0].tolist())}")


def to_gpu_bf16(t):
    return t.bfloat16().to(dev())


# ===========================================================================
# fp64 references.
# ===========================================================================
def linear64(x, w):
    """y = x @ w^T and the absolute-value evaluation of the same sum."""
    x, w = x.double(), w.double()
    return x @ w.t(), x.abs() @ w.abs().t()


def e4m3fn_table():
    """All 256 OCP e4m3fn bytes from the definition: 1 sign, 4 exponent
    (bias 7), 3 mantissa bits; exponent 0 is subnormal, m * 2^-9; there
    is no infinity, and S.1111.111 (0x7F, 0xFF) is NaN."""
    vals = []
    for b in range(256):
        s = -1.0 if b & 0x80 else 1.0
        e, m = (b >> 3) & 0xF, b & 7
        if e == 0xF and m == 7:
            vals.append(float("nan"))
        elif e == 0:
            vals.append(s * m * 2.0 ** -9)
        else:
            vals.append(s * (1 + m / 8.0) * 2.0 ** (e - 7))
    return torch.tensor(vals, dtype=torch.float64)


FP8_NAN_BYTES = (0x7F, 0xFF)


def fp8_linear64(x, w8, scale, table=None):
    """y = x @ decode(w8)^T * scale[o] (+ absolute-value evaluation)."""
    table = e4m3fn_table() if table is None else table
    w = table[w8.long()]
    y, A = linear64(x, w)
    s = scale.double()[None, :]
    return y * s, A * s.abs()


def rmsnorm_res64(x, r, w, eps):
    """The formula of rmsnorm_res_kernel: t = x + r; the mean of squares
    is taken over the unrounded t; the bf16-rounded t (which is x_out)
    is what gets normalised.  Returns x_out as a bf16 tensor and h.
    x_out: the sum of two bf16 values is exact in fp32 unless their
    exponents differ by more than 16, and then it cannot land on a bf16
    rounding tie, so bf16(fp32 sum) is bf16 of the exact sum."""
    t = x.double() + r.double()
    x_out = (x.float() + r.float()).bfloat16()
    inv = torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + f32(eps))
    return x_out, x_out.double() * inv * w.double()


def attn_rows64(q, Aq, K, V, scale=SCALE):
    """Softmax attention of q [Hq, D] over rows K, V [L, Hkv, D] in fp64,
    and the fp32 part of its bound.

    The kernel's output is sum_l p_l v_l / sum_l p_l with p_l =
    exp(d_l - m).  Its score d_l is a 128-term fp32 dot product, off by
    at most 4 * 128 * 2^-24 * sum_i |q_i k_li| * scale; `__expf` adds an
    argument error of 4 * 2^-24 * |d_l - m|.  Either perturbs p_l
    relatively by delta_l.  Numerator and denominator each move by at
    most max_l delta_l relatively (to the numerator's A), and are fp32
    sums of L terms merged through at most 4 more (chains, waves), so

        fp32 part = (2 * max_l delta_l + 4 * (L + 4) * 2^-24) * A,
        A = sum_l p_l |v_ld|   (p_l the fp64 softmax weights).

    Aq is the absolute-value evaluation of q (|q|, or rope's A when the
    kernel ropes q itself), so that rope's own fp32 error is charged to
    its terms.  The same bound serves attn_decode and attn_decode_qkv."""
    Hq, L = q.shape[0], K.shape[0]
    if L == 0:
        z = torch.zeros(Hq, D, dtype=torch.float64)
        return z, z.clone()
    rep = Hq // K.shape[1]
    Kx = K.repeat_interleave(rep, dim=1)
    Vx = V.repeat_interleave(rep, dim=1)
    d = torch.einsum("hd,lhd->hl", q, Kx) * scale
    Ad = torch.einsum("hd,lhd->hl", Aq, Kx.abs()) * scale
    m = d.max(-1, keepdim=True).values
    p = torch.softmax(d, -1)
    delta = 4 * D * U32 * Ad + 4 * U32 * (d - m).abs()
    ref = torch.einsum("hl,lhd->hd", p, Vx)
    A = torch.einsum("hl,lhd->hd", p, Vx.abs())
    fp32 = (2 * delta.max(-1).values[:, None] + 4 * (L + 4) * U32) * A
    return ref, fp32


def attn_decode64(q, kc, vc, kv_lens, slot_ids, row_filter=None):
    """attn_decode over the slot cache: (ref, fp32 part of the bound).
    row_filter(L) -> indices of the cache rows to use (planted defects)."""
    refs, tols = [], []
    for b in range(q.shape[0]):
        L, slot = int(kv_lens[b]), int(slot_ids[b])
        rows = torch.arange(L) if row_filter is None else row_filter(L)
        qb = q[b].double()
        r, t = attn_rows64(qb, qb.abs(), kc[slot, rows].double(),
                           vc[slot, rows].double())
        refs.append(r)
        tols.append(t)
    return torch.stack(refs), torch.stack(tols)


def attn_tol(ref, fp32_part, out_bf16=True):
    return (2 * U16 * ref.abs() if out_bf16 else 0) + fp32_part + TINY


# ===========================================================================
# bf16 GEMV (skinny_gemm).
# ===========================================================================
GEMV_I = [512, 1536, 2048, 2560, 3584, 4096]
GEMV_O = [1, 3, 4, 5, 130]
MR_I = [512, 1536]
MR_O = [16384, 16388]


@functools.lru_cache(maxsize=None)
def gemv_case(I, O, seed=0):
    g = gen(100 + I + O + seed)
    x = bf16_values(torch.randn(8, I, generator=g) * 0.5)
    w = bf16_values(torch.randn(O, I, generator=g) * 0.05)
    y, A = linear64(x, w)
    return x, w, y, A


@gpu
@pytest.mark.parametrize("I", GEMV_I)
def test_skinny_gemm_single_row_fp64(I):
    """skinny_gemm_kernel<N>: every N, main loop only (2048, 4096), tail
    only (512, 1536), main loop then tail (2560 = 2048 + 512, 3584 =
    2048 + 3 * 512), full (4, 130 -> 33 blocks, last one half full) and
    partial (1, 3, 5) last blocks.  K = I fp32 terms per output; the
    dot2 instruction's internal rounding is within the 4 of the rule."""
    C = ops.native()
    x, w, y, A = gemv_case(I, max(GEMV_O))
    xg, wg = to_gpu_bf16(x), to_gpu_bf16(w)
    for O in GEMV_O:
        for N in range(1, 9):
            got = C.skinny_gemm(xg[:N].contiguous(), wg[:O].contiguous())
            check(f"skinny_gemm N={N} I={I} O={O}", got, y[:N, :O],
                  tol_bf16(y[:N, :O], A[:N, :O], K=I))


@gpu
@pytest.mark.parametrize("I", MR_I)
def test_skinny_gemm_multirow_fp64(I):
    """skinny_gemm_multirow_kernel<N,4> (N >= 2, O >= 16384, O % 4 == 0)
    for every N, with a full last block (16384) and a partial one
    (16388 = 1024 * 16 + 4: only wave 0 of the last block has rows), and
    the dispatcher's way back to the single-row kernel at O = 16386."""
    C = ops.native()
    x, w, y, A = gemv_case(I, max(MR_O))
    xg, wg = to_gpu_bf16(x), to_gpu_bf16(w)
    for O in MR_O + [16386]:
        for N in ([2, 8] if O == 16386 else range(2, 9)):
            got = C.skinny_gemm(xg[:N].contiguous(), wg[:O].contiguous())
            check(f"skinny_gemm multirow N={N} I={I} O={O}", got,
                  y[:N, :O], tol_bf16(y[:N, :O], A[:N, :O], K=I))


def onehot_columns(I):
    return [0, 7, 8, 511, 512, I - 513, I - 8, I - 1]


@gpu
@pytest.mark.parametrize("O", [130, 16388], ids=["single_row", "multirow"])
def test_skinny_gemm_one_hot_is_exact(O):
    """x[b] one-hot at column c_b: y[b, o] is W[o, c_b] to the bit (every
    other product is a zero).  First and last element of a lane's
    8-vector, of a 512-chunk, of the main loop and of the tail, one
    column per batch row: lane, chunk and batch indexing with no
    tolerance."""
    C = ops.native()
    I, N = 2560, 8
    cols = onehot_columns(I)
    w = (torch.randn(O, I, generator=gen(7 + O)) * 0.05).bfloat16()
    x = torch.zeros(N, I)
    x[torch.arange(N), torch.tensor(cols)] = 1.0
    got = C.skinny_gemm(to_gpu_bf16(x), w.to(dev()))
    assert_bits_equal(got, w[:, cols].t(), f"one-hot GEMV O={O}")


@gpu
def test_decode_linear_flattens_lead_dims():
    x, w, y, A = gemv_case(3584, 130)
    x3 = to_gpu_bf16(x[:6]).reshape(2, 3, 3584)
    got = ops.decode_linear(x3, to_gpu_bf16(w))
    assert got.shape == (2, 3, 130)
    check("decode_linear [2,3,3584]", got.reshape(6, 130), y[:6],
          tol_bf16(y[:6], A[:6], K=3584))


# ===========================================================================
# SwiGLU-fused GEMV.
# ===========================================================================
SWIGLU_M = [512, 2048, 2560, 3584]
SWIGLU_O = [1, 5, 8]
GATES = [-100.0, -20.0, 0.0, 20.0, 100.0]


@functools.lru_cache(maxsize=None)
def swiglu_gemv_case(M):
    g = gen(300 + M)
    gate = torch.randn(4, M, generator=g) * 2
    up = torch.randn(4, M, generator=g)
    # saturating gates in the first vector, across a lane boundary and in
    # the last 512-chunk (the tail loop where there is one)
    for b in range(4):
        for start in (0, 6 + b, M - 5):
            gate[b, start:start + 5] = torch.tensor(GATES)
    w = bf16_values(torch.randn(max(SWIGLU_O), M, generator=g) * 0.05)
    gu = bf16_values(torch.cat([gate, up], -1))
    s = swiglu64(gu)
    y, A = linear64(s, w)
    return gu, w, y, A


@gpu
@pytest.mark.parametrize("M", SWIGLU_M)
def test_skinny_gemm_swiglu_fp64(M):
    """y = (silu(g) * u) @ W^T with silu(g) * u kept in fp32: M terms per
    output, A from |silu(g) u| |w|.  `__expf(100)` is inf, so silu(-100)
    must come out as -100 / inf = -0, not as a NaN."""
    C = ops.native()
    gu, w, y, A = swiglu_gemv_case(M)
    gug, wg = to_gpu_bf16(gu), to_gpu_bf16(w)
    for O in SWIGLU_O:
        for N in range(1, 5):
            got = C.skinny_gemm_swiglu(gug[:N].contiguous(),
                                       wg[:O].contiguous())
            check(f"skinny_gemm_swiglu N={N} M={M} O={O}", got, y[:N, :O],
                  tol_bf16(y[:N, :O], A[:N, :O], K=M))
    # every gate -100: each term is w * (-0 * u) = +-0, so is the sum
    allneg = torch.cat([torch.full((1, M), -100.0), gu[:1, M:]], -1)
    got = C.skinny_gemm_swiglu(to_gpu_bf16(allneg), wg)
    assert torch.all(got.cpu() == 0), got


# ===========================================================================
# fp8 GEMV.
# ===========================================================================
FP8_MR_I = [16, 1024, 1040, 2048, 2064, 3072, 4112]
FP8_MR_O = [2, 6, 130]
FP8_SR_I = [16, 1040, 3088, 4096, 4112, 5120]
FP8_SR_O = [1, 5, 129]


def random_fp8_bytes(shape, g):
    """Uniform over the 254 bytes that are numbers."""
    b = torch.randint(0, 254, shape, generator=g)
    b = b + (b >= 0x7F).long()          # skip 0x7F; 254 -> 0xFF excluded
    assert int(b.max()) <= 0xFE and not bool((b == 0x7F).any())
    return b.to(torch.uint8)


@functools.lru_cache(maxsize=None)
def fp8_case(I, O):
    g = gen(500 + I + O)
    x = bf16_values(torch.randn(8, I, generator=g) * 0.5)
    w8 = random_fp8_bytes((O, I), g)
    scale = (torch.rand(O, generator=g) + 0.5) * 2.0 ** -6
    y, A = fp8_linear64(x, w8, scale)
    return x, w8, scale, y, A


def run_fp8_random(I, Os):
    C = ops.native()
    x, w8, scale, y, A = fp8_case(I, max(Os))
    xg, wg, sg = to_gpu_bf16(x), w8.to(dev()), scale.to(dev())
    for O in Os:
        for N in range(1, 9):
            got = C.skinny_gemm_fp8(xg[:N].contiguous(),
                                    wg[:O].contiguous(),
                                    sg[:O].contiguous())
            check(f"skinny_gemm_fp8 N={N} I={I} O={O}", got, y[:N, :O],
                  tol_bf16(y[:N, :O], A[:N, :O], K=I))


@gpu
@pytest.mark.parametrize("I", FP8_MR_I)
def test_skinny_gemm_fp8_multirow_fp64(I):
    """skinny_gemm_fp8_mr_kernel<N,2> (even O): one lane only (16), tail
    only (1024), main loop only (2048), and the lengths at which lanes
    split differently between the 2048-stride main loop and the 1024
    tail (1040, 2064, 3072, 4112).  K = I; the product with scale[o] is
    one more fp32 operation, inside the rule's factor."""
    run_fp8_random(I, FP8_MR_O)


@gpu
@pytest.mark.parametrize("I", FP8_SR_I)
def test_skinny_gemm_fp8_single_row_fp64(I):
    """skinny_gemm_fp8_kernel<N>, reached through odd O: 4096-stride
    main loop, 1024 tail, and the lengths where only lane 0 takes one
    more trip (1040, 3088, 4112)."""
    run_fp8_random(I, FP8_SR_O)


@gpu
@pytest.mark.parametrize("O", [256, 255], ids=["multirow", "single_row"])
@pytest.mark.parametrize("pow2_scale", [False, True])
def test_skinny_gemm_fp8_byte_table_is_exact(O, pow2_scale):
    """W8[o, i] = (o + i) % 256 and x[b] one-hot at column b: y[b, o]
    is the decoded byte (o + b) % 256 times scale[o].  Every e4m3fn
    value is a bf16 value (test_fp8_table_matches_torch) and scale is a
    power of two, so the result is exact and compared by bits: a wrong
    bias, a flushed subnormal or a swapped byte of a packed conversion
    cannot hide.  The byte 0x80 decodes to -0; a sum that also holds +0
    terms is +0 (round to nearest), which `+ 0.0` gives the reference."""
    C = ops.native()
    I, N = 256, 8
    w8 = (torch.arange(256)[:, None] + torch.arange(I)[None, :]) % 256
    for nan_byte in FP8_NAN_BYTES:
        w8[w8 == nan_byte] = 0
    w8 = w8.to(torch.uint8)[:O].contiguous()
    scale = 2.0 ** ((torch.arange(O) % 7) - 3).float() if pow2_scale \
        else torch.ones(O)
    x = torch.zeros(N, I)
    x[torch.arange(N), torch.arange(N)] = 1.0
    got = C.skinny_gemm_fp8(to_gpu_bf16(x), w8.to(dev()), scale.to(dev()))
    want = e4m3fn_table()[w8[:, :N].long()].t() * scale.double()[None, :]
    want = want + 0.0
    assert torch.equal(want.bfloat16().double(), want)      # exact in bf16
    assert_bits_equal(got, want.bfloat16(), f"fp8 byte table O={O}")


def test_fp8_table_matches_torch():
    table = e4m3fn_table()
    theirs = torch.arange(256, dtype=torch.uint8).view(
        torch.float8_e4m3fn).double()
    nan = torch.isnan(table)
    assert nan.nonzero().reshape(-1).tolist() == list(FP8_NAN_BYTES)
    assert torch.equal(torch.isnan(theirs), nan)
    assert torch.equal(table[~nan], theirs[~nan])
    assert torch.equal(torch.signbit(table[~nan]),
                       torch.signbit(theirs[~nan]))      # 0x80 is -0
    assert table[~nan].abs().max() == 448
    # every e4m3fn number is a bf16 number
    assert torch.equal(table[~nan].bfloat16().double(), table[~nan])


def test_quantize_fp8_rowwise_edges():
    """An all-zero row and a row with a single non-zero element round
    trip, and a row's largest element decodes to exactly +-448 * scale."""
    g = gen(41)
    w = torch.randn(5, 64, generator=g).bfloat16()
    w[1] = 0
    w[2] = 0
    w[2, 17] = -3.0
    w[3, 5] = 100.0          # one dominant element among ordinary ones
    q8, scale = ops.quantize_fp8_rowwise(w)
    assert q8.dtype == torch.uint8 and scale.dtype == torch.float32
    dec = e4m3fn_table()[q8.long()]
    assert not torch.isnan(dec).any()
    back = dec * scale.double()[:, None]
    assert torch.all(back[1] == 0) and torch.all(q8[1] == 0)
    mask = torch.ones(64, dtype=torch.bool)
    mask[17] = False
    assert torch.all(back[2][mask] == 0)
    assert q8[2, 17] == 0xFE                      # -448
    check("fp8 single element", back[2, 17:18].float(),
          w[2, 17:18].double(), tol_f32(w[2, 17:18].double().abs()))
    for r in (0, 2, 3, 4):
        j = int(w[r].float().abs().argmax())
        sign = 1.0 if w[r, j] > 0 else -1.0
        assert back[r, j].item() == sign * 448 * scale[r].double().item()
        # the grid's spacing is at most 2^-3 relative (3 mantissa bits)
        assert torch.all((back[r] - w[r].double()).abs()
                         <= 2.0 ** -4 * w[r].double().abs()
                         + 2.0 ** -10 * scale[r].double())


# ===========================================================================
# Norm-fused fp8 GEMV.
# ===========================================================================
NORM_I = [1024, 2048, 3072, 4096]
NORM_O = [2, 6, 10, 130]
EPS = 1e-5


def fp8_norm64(x, res, nw, w8, scale, eps=EPS):
    """The formula of skinny_gemm_fp8_norm_kernel with its roundings:
    t = x + res; sum of squares over the unrounded t; the bf16-rounded t
    (xout) is normalised; the product tb * inv * nw is rounded to bf16
    (it is staged in LDS as bf16) before the fp8 dot."""
    t = x.double() + (res.double() if res is not None else 0.0)
    xout = (x.float() + (res.float() if res is not None else 0.0)).bfloat16()
    inv = torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + f32(eps))
    xn = (xout.double() * inv * nw.double()).bfloat16()
    y, A = fp8_linear64(xn, w8, scale)
    return xout, y, A


@functools.lru_cache(maxsize=None)
def fp8_norm_case(I):
    g = gen(700 + I)
    x = torch.randn(2, I, generator=g)
    x[1] *= 30        # the two rows have very different 1/rms
    x = bf16_values(x)
    res = bf16_values(torch.randn(2, I, generator=g) * 0.5)
    nw = bf16_values(torch.randn(I, generator=g) * 0.2 + 1)
    w8 = random_fp8_bytes((max(NORM_O), I), g)
    scale = (torch.rand(max(NORM_O), generator=g) + 0.5) * 2.0 ** -6
    return x, res, nw, w8, scale


@gpu
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("I", NORM_I)
def test_skinny_gemm_fp8_norm_fp64(I, with_res):
    """xout is bf16(x + res) to the bit.  y: the reference carries the
    kernel's two inner bf16 roundings (of t, of the normalised product)
    explicitly, because a dot product of rounded terms is not a rounded
    dot product.  The kernel forms the product in fp32, the reference in
    fp64, so a product close to a bf16 tie may round the other way: one
    bf16 ulp of one of I terms, far below the 4 * I * 2^-24 * A that the
    dot is given.  rsqrtf's error scales all of y, hence roundings = 2:
    one for the bf16 output, one for what moves y as a whole."""
    C = ops.native()
    x, res, nw, w8, scale = fp8_norm_case(I)
    xg, rg, nwg = to_gpu_bf16(x), to_gpu_bf16(res), to_gpu_bf16(nw)
    empty = torch.empty(0, dtype=torch.bfloat16, device=dev())
    for O in NORM_O:
        wg, sg = w8[:O].to(dev()), scale[:O].to(dev())
        for N in (1, 2):
            r = res[:N] if with_res else None
            xout_ref, y, A = fp8_norm64(x[:N], r, nw, w8[:O], scale[:O])
            xout, got = C.skinny_gemm_fp8_norm(
                xg[:N].contiguous(), rg[:N].contiguous() if with_res
                else empty, nwg, EPS, wg, sg, with_res)
            tag = f"fp8_norm N={N} I={I} O={O} res={with_res}"
            assert_bits_equal(xout, xout_ref, tag + " xout")
            check(tag, got, y, tol_bf16(y, A, K=I, roundings=2))


# ===========================================================================
# rmsnorm_res.
# ===========================================================================
RES_H = [2048, 4096, 6144, 8192,      # vector path, nv = 1..4
         256, 2304, 3584, 7936]       # scalar path, 1, 9, 14, 31 chunks


@functools.lru_cache(maxsize=None)
def rmsnorm_res_case(rows, H):
    g = gen(900 + 7 * rows + H)
    x = torch.randn(rows, H, generator=g)
    r = torch.randn(rows, H, generator=g) * 0.5
    if rows >= 3:
        x[1] *= 100     # a neighbour's inv would be 100x off
        r[1] *= 100
    w = torch.randn(H, generator=g) * 0.2 + 1
    return bf16_values(x), bf16_values(r), bf16_values(w)


def check_rmsnorm_res(tag, x_out, h_out, x, r, w, roundings=1,
                      check_fn=check):
    """h reduces H squares into every element; all its terms are
    positive, so A = |h|."""
    H = x.shape[-1]
    x_ref, h_ref = rmsnorm_res64(x, r, w, EPS)
    assert_bits_equal(x_out, x_ref, tag + " x_out")
    check_fn(tag + " h_out", h_out, h_ref,
             tol_bf16(h_ref, h_ref.abs(), K=H, roundings=roundings))


@gpu
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("H", RES_H)
def test_rmsnorm_res_fp64(rows, H):
    C = ops.native()
    x, r, w = rmsnorm_res_case(rows, H)
    xg, rg, wg = to_gpu_bf16(x), to_gpu_bf16(r), to_gpu_bf16(w)
    x_out, h_out = C.rmsnorm_res(xg, rg, wg, EPS)
    check_rmsnorm_res(f"rmsnorm_res ({rows},{H})", x_out, h_out, x, r, w)
    # 3-D input through the wrapper: same rows, same bits
    x3, h3 = ops.rmsnorm_res(xg.view(rows, 1, H), rg.view(rows, 1, H), wg,
                             EPS)
    assert x3.shape == (rows, 1, H) and h3.shape == (rows, 1, H)
    assert_bits_equal(x3.view(rows, H), x_out, "3-D x_out")
    assert_bits_equal(h3.view(rows, H), h_out, "3-D h_out")


# ===========================================================================
# rope_kvwrite.
# ===========================================================================
GROUPS = [(1, 1), (8, 2), (7, 1), (8, 1)]


def rope_tables(S, theta=10000.0):
    half = D // 2
    inv_freq = 1.0 / (theta ** (torch.arange(half).double() / half))
    freqs = torch.outer(torch.arange(S).double(), inv_freq)
    return freqs.cos().float(), freqs.sin().float()


def pattern_cache(slots, S_max, Hkv, offset):
    """A cache in which every element is a different finite bf16 value
    (per 30000): a stray or misplaced write is visible."""
    n = slots * S_max * Hkv * D
    b = ((torch.arange(n) + offset) % 30000 + 1).to(torch.int16)
    return b.view(torch.bfloat16).reshape(slots, S_max, Hkv, D)


@functools.lru_cache(maxsize=None)
def rope_kvwrite_case(Hq, Hkv):
    n, S_max, slots = 5, 8, 7
    g = gen(1100 + 10 * Hq + Hkv)
    qkv = bf16_values(torch.randn(n, (Hq + 2 * Hkv) * D, generator=g))
    cos, sin = rope_tables(S_max)
    # first and last table row; the last slot's last row is the final
    # row of the cache; two tokens share a position; slot != token index
    positions = torch.tensor([S_max - 1, 0, 3, S_max - 1, 1],
                             dtype=torch.int32)
    slot_ids = torch.tensor([slots - 1, 2, 0, 4, 5], dtype=torch.int32)
    return dict(n=n, S_max=S_max, slots=slots, Hq=Hq, Hkv=Hkv, qkv=qkv,
                cos=cos, sin=sin, positions=positions, slot_ids=slot_ids,
                kc0=pattern_cache(slots, S_max, Hkv, 0),
                vc0=pattern_cache(slots, S_max, Hkv, 12345))


def check_rope_kvwrite(case, q, kc, vc, out_bf16=True, check_fn=check):
    """q and the written K rows against rope64 (a rotation is a 2-term
    sum: K = 2), V rows and every unwritten cache element by bits (by
    value when out_bf16 is False: the fp32 CPU fallback)."""
    n, Hq, Hkv = case["n"], case["Hq"], case["Hkv"]
    tol = tol_bf16 if out_bf16 else (lambda ref, A, K: tol_f32(A, K))
    qs, ks, vs = case["qkv"].split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    pos, slot = case["positions"], case["slot_ids"].long()
    tag = f"rope_kvwrite Hq={Hq} Hkv={Hkv}"
    q_ref, A_q = rope64(qs.reshape(n, Hq, D), case["cos"], case["sin"], pos)
    assert q.shape == (n, Hq, D)
    check_fn(tag + " q", q, q_ref, tol(q_ref, A_q, K=2))
    k_ref, A_k = rope64(ks.reshape(n, Hkv, D), case["cos"], case["sin"], pos)
    check_fn(tag + " K rows", kc.cpu()[slot, pos.long()], k_ref,
             tol(k_ref, A_k, K=2))
    same = assert_bits_equal if out_bf16 else \
        (lambda a, b, what: check_fn(what, a, b.double(),
                                     torch.full(b.shape, TINY).double()))
    same(vc.cpu()[slot, pos.long()], vs.reshape(n, Hkv, D).to(vc.dtype),
         tag + " V rows")
    # everything else: restore the written rows and compare whole caches
    for name, after, before in (("Kc", kc, case["kc0"]),
                                ("Vc", vc, case["vc0"])):
        rest = after.detach().cpu().clone()
        rest[slot, pos.long()] = before.to(rest.dtype)[slot, pos.long()]
        same(rest, before.to(rest.dtype), f"{tag} untouched {name}")


@gpu
@pytest.mark.parametrize("Hq,Hkv", GROUPS)
def test_rope_kvwrite_fp64(Hq, Hkv):
    C = ops.native()
    case = rope_kvwrite_case(Hq, Hkv)
    kc, vc = case["kc0"].to(dev()), case["vc0"].to(dev())
    q = C.rope_kvwrite(to_gpu_bf16(case["qkv"]), kc, vc,
                       case["cos"].to(dev()), case["sin"].to(dev()),
                       case["positions"].to(dev()),
                       case["slot_ids"].to(dev()), Hq, Hkv)
    check_rope_kvwrite(case, q, kc, vc)


# ===========================================================================
# attn_decode and attn_decode_qkv.
# ===========================================================================
NAN = float("nan")
ATTN_CASES = [("all_lens", Hq, Hkv) for Hq, Hkv in GROUPS] + [
    ("ragged_1030", 8, 2), ("monotone", 2, 1), ("span60", 2, 1),
    ("equal", 2, 1)]
RANGE_LENS = [1, 5, 16, 17, 33, 48]


@functools.lru_cache(maxsize=None)
def attn_case(name, Hq, Hkv):
    """q [B, Hq, D], a cache whose rows at and beyond kv_len and whose
    unused slots are NaN, permuted slots with spares, and the last slot
    full to S_max.

    all_lens: one sequence per kv_len 0..48 (every kv_len mod 16, the
        4-wave x 4-chain main loop from kv_len 13 on, and its tail).
    ragged_1030: 1023, 1024, 1025, 1030 rows, S_max = 1030.
    monotone: scores rise by 0.5 per row, so every row of every chain
        raises the running maximum and rescales the accumulator.
    span60: scores spread over about +-60: exp(d - m) underflows to 0.
    equal: every score the same (uniform weights)."""
    g = gen(1300 + len(name) + 10 * Hq + Hkv)
    if name == "all_lens":
        lens, S_max = list(range(49)), 48
    elif name == "ragged_1030":
        lens, S_max = [1023, 1030, 1024, 1025], 1030
    else:
        lens, S_max = RANGE_LENS, 48
    B, spare = len(lens), 4
    slots = B + spare
    perm = torch.randperm(slots - 1, generator=g)[:B].tolist()
    perm[lens.index(S_max)] = slots - 1     # last slot, full to S_max
    assert len(set(perm)) == B
    q = torch.randn(B, Hq, D, generator=g)
    kc = torch.full((slots, S_max, Hkv, D), NAN)
    vc = torch.full((slots, S_max, Hkv, D), NAN)
    for b, (L, slot) in enumerate(zip(lens, perm)):
        k = torch.randn(L, Hkv, D, generator=g)
        if name in ("monotone", "span60", "equal"):
            # the heads of a group share q's direction: k_l = a_l * u
            # with q . u * scale = 1 gives the score a_l for each head
            # (times the head's factor)
            q0 = torch.randn(D, generator=g)
            fac = 1 + 0.25 * torch.arange(Hq)
            q[b] = fac[:, None] * q0[None, :]
            u = q0 / (q0.pow(2).sum() * SCALE)
            if name == "monotone":
                a = 0.5 * torch.arange(L)
            elif name == "span60":
                a = 48 * torch.cos(2.4 * torch.arange(L) + 0.3)
            else:
                a = torch.ones(L)
            k = (a[:, None] * u[None, :])[:, None, :].expand(L, Hkv, D)
        kc[slot, :L] = k
        vc[slot, :L] = torch.randn(L, Hkv, D, generator=g)
    return dict(name=name, Hq=Hq, Hkv=Hkv, S_max=S_max, lens=lens,
                q=bf16_values(q), kc=kc.bfloat16(), vc=vc.bfloat16(),
                kv_lens=torch.tensor(lens, dtype=torch.int32),
                slot_ids=torch.tensor(perm, dtype=torch.int32))


def check_attn_decode(case, out, check_fn=check):
    tag = f"attn_decode {case['name']} Hq={case['Hq']} Hkv={case['Hkv']}"
    ref, fp32 = attn_decode64(case["q"], case["kc"], case["vc"],
                              case["kv_lens"], case["slot_ids"])
    check_fn(tag, out, ref, attn_tol(ref, fp32))
    group = case["Hq"] // case["Hkv"]
    for b, L in enumerate(case["lens"]):
        if L == 0:      # nothing to attend to: zeros
            assert torch.all(out[b].cpu() == 0), (tag, b)
        if L == 1:      # one row with weight exp(0) / 1: that V row
            v = case["vc"][int(case["slot_ids"][b]), 0]
            assert_bits_equal(out[b], v.repeat_interleave(group, dim=0),
                              f"{tag} kv_len=1")


@gpu
@pytest.mark.parametrize("name,Hq,Hkv", ATTN_CASES)
def test_attn_decode_fp64(name, Hq, Hkv):
    C = ops.native()
    case = attn_case(name, Hq, Hkv)
    if name == "span60":
        d = torch.einsum("hd,lhd->hl", case["q"][-1].double(),
                         case["kc"][int(case["slot_ids"][-1]), :48]
                         .double().repeat_interleave(Hq // Hkv, 1)) * SCALE
        assert d.max() > 45 and d.min() < -45 and d.max() - d.min() > 110
    out = C.attn_decode(to_gpu_bf16(case["q"]), case["kc"].to(dev()),
                        case["vc"].to(dev()), case["kv_lens"].to(dev()),
                        case["slot_ids"].to(dev()), SCALE)
    check_attn_decode(case, out)


def fused_case(case):
    """The same sequences for attn_decode_qkv: the row at kv_len - 1
    leaves the cache (NaN there before the call) and arrives as the raw
    k and v of the current token in the packed qkv; positions =
    kv_len - 1.  The sequence of length 0 has no current token and is
    left out.  Rope is the identity table where the case prescribes the
    scores, a real table otherwise."""
    keep = [b for b, L in enumerate(case["lens"]) if L >= 1]
    lens = [case["lens"][b] for b in keep]
    slot_ids = case["slot_ids"][keep]
    kc, vc = case["kc"].clone(), case["vc"].clone()
    pos = torch.tensor(lens) - 1
    cur_k = kc[slot_ids.long(), pos].float()       # [B, Hkv, D]
    cur_v = vc[slot_ids.long(), pos].float()
    kc[slot_ids.long(), pos] = NAN
    vc[slot_ids.long(), pos] = NAN
    B = len(keep)
    qkv = torch.cat([case["q"][keep].reshape(B, -1), cur_k.reshape(B, -1),
                     cur_v.reshape(B, -1)], -1)
    if case["name"] in ("monotone", "span60", "equal"):
        cos = torch.ones(case["S_max"], D // 2)
        sin = torch.zeros(case["S_max"], D // 2)
    else:
        cos, sin = rope_tables(case["S_max"])
    return dict(case, lens=lens, slot_ids=slot_ids, kc=kc, vc=vc, qkv=qkv,
                cur_k=cur_k, cur_v=cur_v, cos=cos, sin=sin,
                q=case["q"][keep], positions=pos.int(),
                kv_lens=torch.tensor(lens, dtype=torch.int32))


def attn_decode_qkv64(fc, include_current=True):
    """The kernel ropes q and the current k in fp32 and attends them
    from registers, unrounded: so does the reference, in fp64."""
    q64, Aq = rope64(fc["q"], fc["cos"], fc["sin"], fc["positions"])
    k64, Ak = rope64(fc["cur_k"], fc["cos"], fc["sin"], fc["positions"])
    refs, tols = [], []
    for b, L in enumerate(fc["lens"]):
        slot = int(fc["slot_ids"][b])
        K = fc["kc"][slot, :L - 1].double()
        V = fc["vc"][slot, :L - 1].double()
        if include_current:
            K = torch.cat([K, k64[b][None]])
            V = torch.cat([V, fc["cur_v"][b].double()[None]])
        r, t = attn_rows64(q64[b], Aq[b], K, V)
        refs.append(r)
        tols.append(t)
    return torch.stack(refs), torch.stack(tols), k64, Ak


def check_attn_decode_qkv(fc, out, kc, vc, check_fn=check):
    tag = f"attn_decode_qkv {fc['name']} Hq={fc['Hq']} Hkv={fc['Hkv']}"
    ref, fp32, k64, Ak = attn_decode_qkv64(fc)
    check_fn(tag, out, ref, attn_tol(ref, fp32))
    slot, pos = fc["slot_ids"].long(), fc["positions"].long()
    group = fc["Hq"] // fc["Hkv"]
    for b, L in enumerate(fc["lens"]):
        if L == 1:      # the current token alone: its raw v
            assert_bits_equal(
                out[b], fc["cur_v"][b].bfloat16().repeat_interleave(
                    group, dim=0), f"{tag} kv_len=1")
    # the cache row written for later steps
    check_fn(tag + " K row", kc.cpu()[slot, pos], k64, tol_bf16(k64, Ak, K=2))
    assert_bits_equal(vc.cpu()[slot, pos], fc["cur_v"].bfloat16(),
                      tag + " V row")
    # ... and nothing else, NaN rows included
    for name, after, before in (("Kc", kc, fc["kc"]), ("Vc", vc, fc["vc"])):
        rest = after.detach().cpu().clone()
        rest[slot, pos] = before[slot, pos]
        assert_bits_equal(rest, before, f"{tag} untouched {name}")


@gpu
@pytest.mark.parametrize("name,Hq,Hkv", ATTN_CASES)
def test_attn_decode_qkv_fp64(name, Hq, Hkv):
    C = ops.native()
    fc = fused_case(attn_case(name, Hq, Hkv))
    kc, vc = fc["kc"].to(dev()), fc["vc"].to(dev())
    out = C.attn_decode_qkv(
        to_gpu_bf16(fc["qkv"]), kc, vc, fc["cos"].to(dev()),
        fc["sin"].to(dev()), fc["positions"].to(dev()),
        fc["kv_lens"].to(dev()), fc["slot_ids"].to(dev()), Hq, Hkv, SCALE)
    check_attn_decode_qkv(fc, out, kc, vc)


# ===========================================================================
# decode_advance.
# ===========================================================================
def advance_rows():
    g = gen(1500)
    rows = {}
    r = torch.randn(257, generator=g)
    r[256] = 9.0
    rows["V=257, maximum in the last column (second trip of thread 0)"] = r
    r = torch.randn(1000, generator=g)
    r[999] = 9.0
    rows["V=1000, maximum at V-1"] = r
    rows["all negative"] = -torch.rand(1000, generator=g) - 0.5
    r = torch.full((600,), -1.0)
    r[300], r[44], r[511] = 0.0, -0.0, 0.0
    rows["+0 / -0 tie: lowest index"] = r
    return rows


@gpu
@pytest.mark.parametrize("which", range(4))
def test_decode_advance_edges(which):
    """Argmax edges, with ctr = 2^33 + 5 and chunk = 8: the ring row is
    ctr % chunk = 5 in 64-bit arithmetic."""
    name, row = list(advance_rows().items())[which]
    logits = torch.stack([row, row.flip(0)]).bfloat16()
    b, V = logits.shape
    want = torch.argmax(logits.float(), -1)
    if which == 3:
        assert want.tolist() == [44, 88]     # torch: the first of the zeros
    stage0 = torch.arange(6 * b, dtype=torch.int32).reshape(6, b) * 3
    stage = stage0.clone().to(dev())
    ring = torch.full((8, b), -7, dtype=torch.long, device=dev())
    ctr = torch.tensor([2 ** 33 + 5], dtype=torch.long, device=dev())
    ops.decode_advance(logits.to(dev()), stage, ring, ctr)
    ref_stage = stage0.clone()
    ref_stage[0] = want.int()
    for r in (1, 3, 4):
        ref_stage[r] += 1
    ref_ring = torch.full((8, b), -7, dtype=torch.long)
    ref_ring[5] = want
    assert torch.equal(stage.cpu(), ref_stage), name
    assert torch.equal(ring.cpu(), ref_ring), name
    assert int(ctr) == 2 ** 33 + 5


# ===========================================================================
# Binding validation: every rejection fires before a launch.  Values held
# in device memory (slot ids, positions) are the caller's: no test here
# passes one out of range.  Two kinds of check have no case: a tensor on a
# second GPU (the suite runs on one) and the grid limits (2^31 rows).
# ===========================================================================
def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=dev())


def _z(*shape, dtype=torch.float32, device=None):
    return torch.zeros(*shape, dtype=dtype, device=device or dev())


def _expect_rejections(bad_calls):
    for name, (pattern, call) in bad_calls.items():
        with pytest.raises(RuntimeError, match=pattern):
            call()
            pytest.fail(f"{name}: accepted")


def _decode_args(B=2, Hq=4, Hkv=2, slots=3, S_max=8):
    return dict(Q=_bf(B, Hq, D), qkv=_bf(B, (Hq + 2 * Hkv) * D),
                Kc=_bf(slots, S_max, Hkv, D), Vc=_bf(slots, S_max, Hkv, D),
                cos=_z(S_max, D // 2), sin=_z(S_max, D // 2),
                positions=_z(B, dtype=torch.int32),
                kv_lens=_z(B, dtype=torch.int32),
                slot_ids=_z(B, dtype=torch.int32), Hq=Hq, Hkv=Hkv)


@gpu
def test_attn_decode_rejects_bad_inputs():
    C = ops.native()
    a = _decode_args()

    def call(**kw):
        v = dict(a, **kw)
        return lambda: C.attn_decode(v["Q"], v["Kc"], v["Vc"], v["kv_lens"],
                                     v["slot_ids"], SCALE)

    call()()    # the baseline is accepted
    wide = _bf(3, 8, 4, D)
    _expect_rejections({
        "Q fp32": ("attn_decode: Q must be BFloat16", call(Q=_z(2, 4, D))),
        "Q 2-D": (r"attn_decode: Q must be \[B, Hq, 128\]",
                  call(Q=_bf(2, 4 * D))),
        "Q head dim": (r"attn_decode: Q must be \[B, Hq, 128\]",
                       call(Q=_bf(2, 4, 64))),
        "Kc on cpu": ("attn_decode: Kc must be on GPU",
                      call(Kc=torch.zeros(3, 8, 2, D,
                                          dtype=torch.bfloat16))),
        "Kc strided view": ("attn_decode: Kc must be contiguous",
                            call(Kc=wide[:, :, :2], Vc=wide[:, :, 2:])),
        "Vc fp32": ("attn_decode: Vc must be BFloat16",
                    call(Vc=_z(3, 8, 2, D))),
        "Vc shape": ("attn_decode: Vc must have Kc's shape",
                     call(Vc=_bf(3, 9, 2, D))),
        "Kc 3-D": ("attn_decode: Kc must be", call(Kc=_bf(3, 8, 2 * D))),
        "no slots": ("attn_decode: Kc must hold at least one slot",
                     call(Kc=_bf(0, 8, 2, D), Vc=_bf(0, 8, 2, D))),
        "Kc head dim": ("attn_decode: Kc head dim must be 128",
                        call(Kc=_bf(3, 8, 2, 64), Vc=_bf(3, 8, 2, 64))),
        "Hq % Hkv": ("attn_decode: Hq = 4 must be a positive multiple",
                     call(Kc=_bf(3, 8, 3, D), Vc=_bf(3, 8, 3, D))),
        "kv_lens int64": ("attn_decode: kv_lens must be Int",
                          call(kv_lens=_z(2, dtype=torch.int64))),
        "kv_lens count": (r"attn_decode: kv_lens must be a \[B\]",
                          call(kv_lens=_z(3, dtype=torch.int32))),
        "slot_ids on cpu": ("attn_decode: slot_ids must be on GPU",
                            call(slot_ids=torch.zeros(
                                2, dtype=torch.int32))),
        "slot_ids 2-D": (r"attn_decode: slot_ids must be a \[B\]",
                         call(slot_ids=_z(2, 1, dtype=torch.int32))),
    })


@gpu
def test_attn_decode_qkv_rejects_bad_inputs():
    C = ops.native()
    a = _decode_args()

    def call(**kw):
        v = dict(a, **kw)
        return lambda: C.attn_decode_qkv(
            v["qkv"], v["Kc"], v["Vc"], v["cos"], v["sin"], v["positions"],
            v["kv_lens"], v["slot_ids"], v["Hq"], v["Hkv"], SCALE)

    call()()
    wide = _bf(3, 8, 4, D)
    op = "attn_decode_qkv: "
    _expect_rejections({
        "qkv fp32": (op + "qkv must be BFloat16", call(qkv=_z(2, 8 * D))),
        "qkv width": (op + "qkv must be", call(qkv=_bf(2, 7 * D))),
        "Hq = 0": (op + "Hq = 0 and Hkv = 2 must be positive",
                   call(qkv=_bf(2, 4 * D), Hq=0)),
        "no rows": (op + "Kc must hold at least one slot and one row",
                    call(Kc=_bf(3, 0, 2, D), Vc=_bf(3, 0, 2, D))),
        "qkv strided": (op + "qkv must be contiguous",
                        call(qkv=_bf(2, 16 * D)[:, ::2])),
        "Kc strided view": (op + "Kc must be contiguous",
                            call(Kc=wide[:, :, :2], Vc=wide[:, :, 2:])),
        "Vc on cpu": (op + "Vc must be on GPU",
                      call(Vc=torch.zeros(3, 8, 2, D,
                                          dtype=torch.bfloat16))),
        "Vc shape": (op + "Vc must have Kc's shape",
                     call(Vc=_bf(4, 8, 2, D))),
        "Hkv mismatch": (op + r"Hkv = 1 must equal Kc.size\(2\)",
                         call(qkv=_bf(2, 6 * D), Hkv=1)),
        "Hq % Hkv": (op + "Hq = 3 must be a positive multiple",
                     call(qkv=_bf(2, 7 * D), Hq=3)),
        "cos bf16": (op + "cos must be Float",
                     call(cos=_bf(8, D // 2))),
        "sin width": (op + r"sin must be \[rows, 64\]",
                      call(sin=_z(8, D))),
        "cos short": (op + "cos has 7 rows", call(cos=_z(7, D // 2))),
        "sin strided": (op + "sin must be contiguous",
                        call(sin=_z(8, D)[:, ::2])),
        "positions int64": (op + "positions must be Int",
                            call(positions=_z(2, dtype=torch.int64))),
        "kv_lens count": (op + r"kv_lens must be a \[B\]",
                          call(kv_lens=_z(1, dtype=torch.int32))),
        "slot_ids on cpu": (op + "slot_ids must be on GPU",
                            call(slot_ids=torch.zeros(
                                2, dtype=torch.int32))),
    })


@gpu
def test_rope_kvwrite_rejects_bad_inputs():
    C = ops.native()
    a = _decode_args()

    def call(**kw):
        v = dict(a, **kw)
        return lambda: C.rope_kvwrite(
            v["qkv"], v["Kc"], v["Vc"], v["cos"], v["sin"], v["positions"],
            v["slot_ids"], v["Hq"], v["Hkv"])

    call()()
    wide = _bf(3, 8, 4, D)
    op = "rope_kvwrite: "
    _expect_rejections({
        "qkv on cpu": (op + "qkv must be on GPU",
                       call(qkv=torch.zeros(2, 8 * D,
                                            dtype=torch.bfloat16))),
        "qkv width": (op + "qkv must be", call(qkv=_bf(2, 9 * D))),
        "Hkv = 0": (op + "Hq = 4 and Hkv = 0 must be positive",
                    call(qkv=_bf(2, 4 * D), Hkv=0)),
        "Kc strided view": (op + "Kc must be contiguous",
                            call(Kc=wide[:, :, :2], Vc=wide[:, :, 2:])),
        "Kc fp16": (op + "Kc must be BFloat16",
                    call(Kc=_z(3, 8, 2, D, dtype=torch.float16))),
        "Vc shape": (op + "Vc must have Kc's shape",
                     call(Vc=_bf(3, 8, 1, D))),
        "Hkv mismatch": (op + r"Hkv = 1 must equal Kc.size\(2\)",
                         call(qkv=_bf(2, 6 * D), Hkv=1)),
        "cos fp64": (op + "cos must be Float",
                     call(cos=_z(8, D // 2, dtype=torch.float64))),
        "sin short": (op + "sin has 4 rows", call(sin=_z(4, D // 2))),
        "positions int64": (op + "positions must be Int",
                            call(positions=_z(2, dtype=torch.int64))),
        "positions count": (op + r"positions must be a \[B\]",
                            call(positions=_z(5, dtype=torch.int32))),
        "slot_ids int64": (op + "slot_ids must be Int",
                           call(slot_ids=_z(2, dtype=torch.int64))),
        "slot_ids on cpu": (op + "slot_ids must be on GPU",
                            call(slot_ids=torch.zeros(
                                2, dtype=torch.int32))),
    })


@gpu
def test_rmsnorm_res_rejects_bad_inputs():
    C = ops.native()
    x, r, w = _bf(2, 512), _bf(2, 512), _bf(512)
    C.rmsnorm_res(x, r, w, EPS)
    op = "rmsnorm_res: "
    _expect_rejections({
        "x fp32": (op + "x must be BFloat16",
                   lambda: C.rmsnorm_res(_z(2, 512), r, w, EPS)),
        "x scalar": (op + r"x must be \[..., H\], got a scalar",
                     lambda: C.rmsnorm_res(_bf(()), _bf(()), w, EPS)),
        "H % 256": (op + "H must be a multiple of 256",
                    lambda: C.rmsnorm_res(_bf(2, 384), _bf(2, 384),
                                          _bf(384), EPS)),
        "H > 8192": (op + "H must be a multiple of 256",
                     lambda: C.rmsnorm_res(_bf(1, 8448), _bf(1, 8448),
                                           _bf(8448), EPS)),
        "res shape": (op + "res must have x's shape",
                      lambda: C.rmsnorm_res(x, _bf(1, 512), w, EPS)),
        "res strided": (op + "res must be contiguous",
                        lambda: C.rmsnorm_res(x, _bf(2, 1024)[:, ::2], w,
                                              EPS)),
        "res on cpu": (op + "res must be on GPU",
                       lambda: C.rmsnorm_res(
                           x, torch.zeros(2, 512, dtype=torch.bfloat16), w,
                           EPS)),
        "w fp32": (op + "w must be BFloat16",
                   lambda: C.rmsnorm_res(x, r, _z(512), EPS)),
        "w size": (op + "w must have H = 512",
                   lambda: C.rmsnorm_res(x, r, _bf(256), EPS)),
        "w strided": (op + "w must be contiguous",
                      lambda: C.rmsnorm_res(x, r, _bf(1024)[::2], EPS)),
    })
    # the wrapper hands an fp32 norm weight over as bf16
    x2, h = ops.rmsnorm_res(x + 1, r, torch.ones(512, device=dev()), EPS)
    assert torch.all(x2 == 1) and torch.all(h == 1)


@gpu
def test_skinny_gemm_fp8_rejects_bad_inputs():
    C = ops.native()
    x = _bf(2, 1024)
    w8 = _z(6, 1024, dtype=torch.uint8)
    sc = _z(6)
    nw = _bf(1024)
    none = _bf(0)
    C.skinny_gemm_fp8(x, w8, sc)
    C.skinny_gemm_fp8(x, w8.view(torch.float8_e4m3fn), sc)
    C.skinny_gemm_fp8_norm(x, none, nw, EPS, w8, sc, False)
    op = "skinny_gemm_fp8: "
    _expect_rejections({
        "X fp32": (op + "X must be BFloat16",
                   lambda: C.skinny_gemm_fp8(_z(2, 1024), w8, sc)),
        "X 3-D": (op + r"X must be \[N, I\]",
                  lambda: C.skinny_gemm_fp8(_bf(1, 2, 1024), w8, sc)),
        "N = 9": (op + "N must be 1..8",
                  lambda: C.skinny_gemm_fp8(_bf(9, 1024), w8, sc)),
        "I % 16": (op + "I must be a positive multiple of 16",
                   lambda: C.skinny_gemm_fp8(
                       _bf(2, 1000), _z(6, 1000, dtype=torch.uint8), sc)),
        "W8 int8": (op + "W8 must be uint8 or float8_e4m3fn",
                    lambda: C.skinny_gemm_fp8(
                        x, _z(6, 1024, dtype=torch.int8), sc)),
        "W8 bf16": (op + "W8 must be uint8 or float8_e4m3fn",
                    lambda: C.skinny_gemm_fp8(x, _bf(6, 1024), sc)),
        "W8 inner dim": (op + r"W8 must be \[O, I\] with I = 1024",
                         lambda: C.skinny_gemm_fp8(
                             x, _z(6, 2048, dtype=torch.uint8), sc)),
        "W8 strided": (op + "W8 must be contiguous",
                       lambda: C.skinny_gemm_fp8(
                           x, _z(6, 2048, dtype=torch.uint8)[:, ::2], sc)),
        "W8 on cpu": (op + "W8 must be on GPU",
                      lambda: C.skinny_gemm_fp8(
                          x, torch.zeros(6, 1024, dtype=torch.uint8), sc)),
        "scale fp64": (op + "scale must be Float",
                       lambda: C.skinny_gemm_fp8(
                           x, w8, _z(6, dtype=torch.float64))),
        "scale count": (op + "scale must have O = 6",
                        lambda: C.skinny_gemm_fp8(x, w8, _z(5))),
        "O = 0": (op + "W8 must have at least one row",
                  lambda: C.skinny_gemm_fp8(
                      x, _z(0, 1024, dtype=torch.uint8), _z(0))),
    })
    op = "skinny_gemm_fp8_norm: "
    _expect_rejections({
        "x fp32": (op + "x must be BFloat16",
                   lambda: C.skinny_gemm_fp8_norm(
                       _z(2, 1024), none, nw, EPS, w8, sc, False)),
        "I = 5120": (op + "I must be 1024, 2048, 3072 or 4096",
                     lambda: C.skinny_gemm_fp8_norm(
                         _bf(2, 5120), none, _bf(5120), EPS,
                         _z(6, 5120, dtype=torch.uint8), sc, False)),
        "N = 3": (op + "N must be 1 or 2",
                  lambda: C.skinny_gemm_fp8_norm(
                      _bf(3, 1024), none, nw, EPS, w8, sc, False)),
        "odd O": (op + "O must be even",
                  lambda: C.skinny_gemm_fp8_norm(
                      x, none, nw, EPS, _z(5, 1024, dtype=torch.uint8),
                      _z(5), False)),
        "W8 inner dim": (op + r"W8 must be \[O, I\] with I = 1024",
                         lambda: C.skinny_gemm_fp8_norm(
                             x, none, nw, EPS,
                             _z(6, 2048, dtype=torch.uint8), sc, False)),
        "W8 fp32": (op + "W8 must be uint8 or float8_e4m3fn",
                    lambda: C.skinny_gemm_fp8_norm(
                        x, none, nw, EPS, _z(6, 1024), sc, False)),
        "scale count": (op + "scale must have O = 6",
                        lambda: C.skinny_gemm_fp8_norm(
                            x, none, nw, EPS, w8, _z(4), False)),
        "scale on cpu": (op + "scale must be on GPU",
                         lambda: C.skinny_gemm_fp8_norm(
                             x, none, nw, EPS, w8, torch.zeros(6), False)),
        "nw fp32": (op + "nw must be BFloat16",
                    lambda: C.skinny_gemm_fp8_norm(
                        x, none, _z(1024), EPS, w8, sc, False)),
        "nw size": (op + "nw must have I = 1024",
                    lambda: C.skinny_gemm_fp8_norm(
                        x, none, _bf(2048), EPS, w8, sc, False)),
        "res shape": (op + "res must be empty or have x's shape",
                      lambda: C.skinny_gemm_fp8_norm(
                          x, _bf(1, 1024), nw, EPS, w8, sc, True)),
        "res fp32": (op + "res must be BFloat16",
                     lambda: C.skinny_gemm_fp8_norm(
                         x, _z(2, 1024), nw, EPS, w8, sc, True)),
    })


@gpu
def test_decode_advance_rejects_bad_inputs():
    C = ops.native()
    lg = _bf(2, 64)
    st = _z(6, 2, dtype=torch.int32)
    ring = _z(8, 2, dtype=torch.int64)
    ctr = _z(1, dtype=torch.int64)
    C.decode_advance(lg, st, ring, ctr)
    op = "decode_advance: "
    _expect_rejections({
        "logits fp32": (op + "logits must be BFloat16",
                        lambda: C.decode_advance(_z(2, 64), st, ring, ctr)),
        "logits scalar": (op + r"logits must be \[b, V\], got a scalar",
                          lambda: C.decode_advance(_bf(()), st, ring, ctr)),
        "logits strided": (op + "logits must be contiguous",
                           lambda: C.decode_advance(_bf(2, 128)[:, ::2], st,
                                                    ring, ctr)),
        "stage int64": (op + "stage must be Int",
                        lambda: C.decode_advance(
                            lg, _z(6, 2, dtype=torch.int64), ring, ctr)),
        "stage rows": (op + r"stage must be \[6, b\]",
                       lambda: C.decode_advance(
                           lg, _z(5, 2, dtype=torch.int32), ring, ctr)),
        "stage 1-D": (op + r"stage must be \[6, b\]",
                      lambda: C.decode_advance(
                          lg, _z(12, dtype=torch.int32), ring, ctr)),
        "ring int32": (op + "ring must be Long",
                       lambda: C.decode_advance(
                           lg, st, _z(8, 2, dtype=torch.int32), ctr)),
        "ring width": (op + r"ring must be \[chunk >= 1, b\]",
                       lambda: C.decode_advance(
                           lg, st, _z(8, 3, dtype=torch.int64), ctr)),
        "ring empty": (op + r"ring must be \[chunk >= 1, b\]",
                       lambda: C.decode_advance(
                           lg, st, _z(0, 2, dtype=torch.int64), ctr)),
        "ctr on cpu": (op + "ctr must be on GPU",
                       lambda: C.decode_advance(
                           lg, st, ring, torch.zeros(1, dtype=torch.int64))),
        "ctr int32": (op + "ctr must be Long",
                      lambda: C.decode_advance(
                          lg, st, ring, _z(1, dtype=torch.int32))),
        "ctr two": (op + "ctr must hold one element",
                    lambda: C.decode_advance(
                        lg, st, ring, _z(2, dtype=torch.int64))),
    })


# ===========================================================================
# CPU part 1: the fp64 references agree with the package's own CPU paths.
# Those compute in fp32; given fp32 tensors (holding bf16 values) they
# return fp32, so only the fp32 part of each bound applies.
# ===========================================================================
def test_linear_reference_matches_f_linear():
    x, w, y, A = gemv_case(512, 5)
    got = torch.nn.functional.linear(x, w)
    check("cpu F.linear", got, y, tol_f32(A, K=512))
    got = ops.decode_linear(x[:2].reshape(2, 1, 512), w)
    check("cpu decode_linear", got.reshape(2, 5), y[:2],
          tol_f32(A[:2], K=512))


def test_attention_reference_matches_attn_decode_ref():
    case = attn_case("all_lens", 8, 2)
    keep = [1, 2, 16, 17, 48]       # attn_decode_ref needs kv_len >= 1
    q, lens, slots = case["q"][keep], case["kv_lens"][keep], \
        case["slot_ids"][keep]
    got = ops.attn_decode(q, case["kc"].float(), case["vc"].float(), lens,
                          slots, SCALE)
    assert got.dtype == torch.float32
    ref, fp32 = attn_decode64(q, case["kc"], case["vc"], lens, slots)
    check("cpu attn_decode_ref", got, ref, attn_tol(ref, fp32, False))


def test_fused_attention_reference_matches_cpu_fallback():
    """ops.attn_decode_qkv on the CPU composes rope_kvwrite (which
    rounds the roped q and k to the tensors' dtype: fp32 here) and
    attn_decode_ref."""
    fc = fused_case(attn_case("all_lens", 8, 2))
    keep = [0, 1, 15, 16, 47]
    sub = dict(fc, lens=[fc["lens"][b] for b in keep], q=fc["q"][keep],
               cur_k=fc["cur_k"][keep], cur_v=fc["cur_v"][keep],
               positions=fc["positions"][keep],
               slot_ids=fc["slot_ids"][keep])
    kc, vc = fc["kc"].float(), fc["vc"].float()
    got = ops.attn_decode_qkv(fc["qkv"][keep], kc, vc, fc["cos"], fc["sin"],
                              sub["positions"], fc["kv_lens"][keep],
                              sub["slot_ids"], 8, 2, SCALE)
    ref, fp32, k64, Ak = attn_decode_qkv64(sub)
    check("cpu attn_decode_qkv", got, ref, attn_tol(ref, fp32, False))
    slot, pos = sub["slot_ids"].long(), sub["positions"].long()
    check("cpu attn_decode_qkv K row", kc[slot, pos], k64, tol_f32(Ak, K=2))
    assert torch.equal(vc[slot, pos], sub["cur_v"])


@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (7, 1)])
def test_rope_kvwrite_reference_matches_cpu_fallback(Hq, Hkv):
    case = rope_kvwrite_case(Hq, Hkv)
    kc, vc = case["kc0"].float(), case["vc0"].float()
    q = ops.rope_kvwrite(case["qkv"], kc, vc, case["cos"], case["sin"],
                         case["positions"], case["slot_ids"], Hq, Hkv)
    check_rope_kvwrite(case, q, kc, vc, out_bf16=False)


@pytest.mark.parametrize("rows,H", [(1, 256), (3, 2304)])
def test_rmsnorm_res_reference_matches_cpu_fallback(rows, H):
    """The fallback adds in bf16 (x_out to the bit) and takes the mean
    of squares over that ROUNDED sum where the kernel uses the unrounded
    one: each square moves by at most 2 * 2^-8 relatively and so does
    their mean, which is half that in inv - one more rounding's worth."""
    x, r, w = rmsnorm_res_case(rows, H)
    x_out, h = ops.rmsnorm_res(x.bfloat16(), r.bfloat16(), w.bfloat16(), EPS)
    check_rmsnorm_res("cpu rmsnorm_res", x_out, h, x, r, w, roundings=2)


# ===========================================================================
# CPU part 2: the checker rejects known-wrong results, one defect each,
# emulated in torch and judged against the same reference and bound.
# ===========================================================================
def test_checker_rejects_gemv_without_its_tail():
    """I = 2560: the 2048-wide main loop runs once, the 512 tail is
    skipped."""
    I = 2560
    x, w, y, A = gemv_case(I, 130)
    tol = tol_bf16(y, A, K=I)
    assert not rejects(y.bfloat16(), y, tol)
    short, _ = linear64(x[:, :2048], w[:, :2048])
    assert rejects(short.bfloat16(), y, tol)


def test_checker_rejects_gemv_dropping_one_lanes_vector():
    """8 of 2560 columns (lane 37's vector of the tail chunk) missing."""
    I = 2560
    x, w, y, A = gemv_case(I, 130)
    xd = x.clone()
    xd[:, 2048 + 37 * 8:2048 + 38 * 8] = 0
    got, _ = linear64(xd, w)
    assert rejects(got.bfloat16(), y, tol_bf16(y, A, K=I))
    # the exact probe sees it without a tolerance
    cols = onehot_columns(I)
    onehot = torch.zeros(8, I)
    onehot[torch.arange(8), torch.tensor(cols)] = 1.0
    lane_of_last = ((I - 1) % 512) // 8
    onehot[:, 2048 + lane_of_last * 8:] = 0          # that lane's tail vector
    got, _ = linear64(onehot, w)
    assert not torch.equal(got.bfloat16(), w[:, cols].t().bfloat16())


def test_checker_rejects_unwritten_rows_of_partial_last_block():
    """O = 16388: the last block's wave 0 owns rows 16384..16387.  Left
    unwritten they hold whatever the allocation held; zeros are the
    kindest case."""
    x, w, y, A = gemv_case(512, 20, seed=1)
    tol = tol_bf16(y, A, K=512)
    got = y.bfloat16()
    assert not rejects(got, y, tol)
    got[:, 16:] = 0
    ok, _, worst = within(got, y, tol)
    assert not ok and worst % 20 >= 16


def test_checker_rejects_fp8_decoded_with_bias_8():
    """The e4m3fnuz reading of the same bytes: every normal value halved."""
    x, w8, scale, y, A = fp8_case(1040, 6)
    tol = tol_bf16(y, A, K=1040)
    assert not rejects(y.bfloat16(), y, tol)
    got, _ = fp8_linear64(x, w8, scale, table=e4m3fn_table() / 2)
    assert rejects(got.bfloat16(), y, tol)


def test_checker_rejects_fp8_subnormals_flushed():
    table = e4m3fn_table()
    flushed = table.clone()
    flushed[(torch.arange(256) & 0x78) == 0] = 0.0
    assert int((flushed != table).sum()) == 14 + 2      # + the two NaN
    g = gen(43)
    I = 1040
    x = bf16_values(torch.randn(2, I, generator=g) * 0.5)
    w8 = random_fp8_bytes((4, I), g)
    # row 0 holds subnormals only
    w8[0] = (torch.randint(1, 8, (I,), generator=g)
             + 0x80 * torch.randint(0, 2, (I,), generator=g)).to(torch.uint8)
    scale = torch.ones(4)
    y, A = fp8_linear64(x, w8, scale)
    got, _ = fp8_linear64(x, w8, scale, table=flushed)
    ok, _, worst = within(got.bfloat16(), y, tol_bf16(y, A, K=I))
    assert not ok and worst % 4 == 0
    # (among normal values a flushed subnormal can stay below the fp32
    # bound: that is what the exact byte-table test is for)


def test_checker_rejects_attention_reading_past_kv_len():
    case = attn_case("all_lens", 8, 2)
    ref, fp32 = attn_decode64(case["q"], case["kc"], case["vc"],
                              case["kv_lens"], case["slot_ids"])
    tol = attn_tol(ref, fp32)
    assert not rejects(ref.bfloat16(), ref, tol)
    S_max = case["S_max"]
    over, _ = attn_decode64(
        case["q"], case["kc"], case["vc"], case["kv_lens"],
        case["slot_ids"],
        row_filter=lambda L: torch.arange(min(L + 1, S_max)))
    # the row past kv_len is NaN, and so is every output that used it
    for b, L in enumerate(case["lens"]):
        assert rejects(over[b].bfloat16(), ref[b], tol[b]) == (L < S_max)
    # a finite stale row there is caught by the bound as well
    kc, vc = case["kc"].clone(), case["vc"].clone()
    g = gen(47)
    stale = torch.isnan(kc)
    kc[stale] = torch.randn(int(stale.sum()), generator=g).bfloat16()
    vc[stale] = torch.randn(int(stale.sum()), generator=g).bfloat16()
    over, _ = attn_decode64(
        case["q"], kc, vc, case["kv_lens"], case["slot_ids"],
        row_filter=lambda L: torch.arange(min(L + 1, S_max)))
    for b, L in enumerate(case["lens"]):
        assert rejects(over[b].bfloat16(), ref[b], tol[b]) == (L < S_max)


def test_checker_rejects_attention_dropping_chains_at_the_merge():
    """Row s belongs to wave s % 4 and, inside the 16-row main loop, to
    chain (s // 4) % 4; the tail rows all go to chain 0.  A merge that
    keeps chain 0 only loses every main-loop row of chains 1..3."""
    case = attn_case("all_lens", 8, 2)

    def chain0_rows(L):
        s = torch.arange(L)
        w = s % 4
        per_wave = (L - w + 3) // 4             # rows of that wave
        in_main = (s // 4) < (per_wave // 4) * 4
        return s[~in_main | ((s // 4) % 4 == 0)]

    ref, fp32 = attn_decode64(case["q"], case["kc"], case["vc"],
                              case["kv_lens"], case["slot_ids"])
    got, _ = attn_decode64(case["q"], case["kc"], case["vc"],
                           case["kv_lens"], case["slot_ids"],
                           row_filter=chain0_rows)
    tol = attn_tol(ref, fp32)
    for b, L in enumerate(case["lens"]):
        # from 13 rows on, wave 0 runs the main loop
        assert rejects(got[b].bfloat16(), ref[b], tol[b]) == (L >= 13), L


def test_checker_rejects_fused_attention_without_current_token():
    fc = fused_case(attn_case("all_lens", 8, 2))
    ref, fp32, _, _ = attn_decode_qkv64(fc)
    got, _, _, _ = attn_decode_qkv64(fc, include_current=False)
    tol = attn_tol(ref, fp32)
    assert not rejects(ref.bfloat16(), ref, tol)
    for b in range(len(fc["lens"])):
        assert rejects(got[b].bfloat16(), ref[b], tol[b]), fc["lens"][b]


def test_checker_rejects_rope_kvwrite_indexing_cache_by_token():
    case = rope_kvwrite_case(8, 2)
    kc, vc = case["kc0"].clone(), case["vc0"].clone()
    by_token = torch.arange(case["n"], dtype=torch.int32)
    q = ops.rope_kvwrite(case["qkv"].bfloat16(), kc, vc, case["cos"],
                         case["sin"], case["positions"], by_token, 8, 2)
    with pytest.raises(AssertionError):
        check_rope_kvwrite(case, q, kc, vc)
    # the same emulation with the right slots passes
    kc, vc = case["kc0"].clone(), case["vc0"].clone()
    q = ops.rope_kvwrite(case["qkv"].bfloat16(), kc, vc, case["cos"],
                         case["sin"], case["positions"], case["slot_ids"],
                         8, 2)
    check_rope_kvwrite(case, q, kc, vc)


def test_checker_rejects_rmsnorm_res_with_neighbours_inv():
    rows, H = 3, 3584
    x, r, w = rmsnorm_res_case(rows, H)
    x_out, h_ref = rmsnorm_res64(x, r, w, EPS)
    tol = tol_bf16(h_ref, h_ref.abs(), K=H)
    assert not rejects(h_ref.bfloat16(), h_ref, tol)
    t = x.double() + r.double()
    inv = torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + f32(EPS))
    h = x_out.double() * inv.roll(1, 0) * w.double()
    assert rejects(h.bfloat16(), h_ref, tol)
    # two ordinary rows whose rms differs by a few per cent
    g = gen(53)
    x2 = bf16_values(torch.randn(2, H, generator=g))
    x2[1] = bf16_values(x2[1] * 1.05)
    r2 = torch.zeros(2, H)
    xo2, h2_ref = rmsnorm_res64(x2, r2, w, EPS)
    inv2 = torch.rsqrt(x2.double().pow(2).mean(-1, keepdim=True) + f32(EPS))
    h2 = xo2.double() * inv2.flip(0) * w.double()
    assert rejects(h2.bfloat16(), h2_ref,
                   tol_bf16(h2_ref, h2_ref.abs(), K=H))
