"""attn_append_kernel and attn_append_fp8_kernel (attention_append.hip,
attn_append_body.h) element by element against fp64.
tests/_attn_append_fp64.py has the reference, the bound with its
derivation, the geometries and why each sequence is in them.

Every valid row of every case is held to the bound; the FP8 kernel is held
to the same reference directly, over ``ops.kv_dequantize`` of its codes
(which is exact).  Beside that: a sequence alone or in another slot gives
the bits it gives in its batch, NaN in the padding rows of ``q`` changes
no valid row, the kernel's guards turn an index the cache cannot hold into
an empty sequence, and the rounding bias of ``O`` with constant ``V`` is
at most 2^-11.  Run with ``-s`` for the worst err/tol per case; measured
on an MI355X: attn_append_kernel 0.59, attn_append_fp8_kernel 0.64, bias
exactly 0 with every element of O equal to v."""
import functools
import types

import pytest
import torch

import _attn_append_fp64 as aa
from _fp64_check import check, within
from skypilot_amd import ops
from test_gpu_decode_kernels import assert_bits_equal, dev
from test_kv_fp8_gpu import POISON_EXP, quantize_poisoned

pytestmark = pytest.mark.gpu

SCALE = aa.SCALE
KINDS = ("bf16", "fp8")
KERNEL = {"bf16": "attn_append_kernel", "fp8": "attn_append_fp8_kernel"}
BIAS = 2.0 ** -11    # round-to-nearest P (test_attn_train_gpu.py)


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev())


@functools.lru_cache(maxsize=None)
def _inputs(kind, case):
    """The case for one kernel: its CPU inputs, the device cache tensors in
    the op's argument order and the per-sequence references.  The FP8
    cache is the bf16 one with every row scaled by a power of 4 of its
    own, quantised, with the poison in the dead rows; its references run
    on the dequantised codes."""
    c = aa.build_case(case)
    if kind == "bf16":
        return c, (c.kc.to(dev()), c.vc.to(dev())), aa.case_refs(case)
    g = torch.Generator().manual_seed(300 + 10 * c.Hq + c.Hkv)
    parts, deq = [], []
    for cache in (c.kc, c.vc):
        mult = 4.0 ** torch.randint(-2, 3, cache.shape[:3] + (1,),
                                    generator=g).float()
        codes, exps = quantize_poisoned(cache.float() * mult)
        parts += [codes, exps]
        deq.append(ops.kv_dequantize(codes, exps).bfloat16())
    (k8, ke, v8, ve), (kd, vd) = parts, deq
    dead = ke == POISON_EXP
    assert torch.equal(dead, torch.isnan(c.kc.float()).any(-1))
    assert bool(torch.isnan(kd.float())[dead].all()) and \
        bool(torch.isfinite(kd.float())[~dead].all())
    assert torch.equal(kd.float()[~dead], ops.kv_dequantize(k8, ke)[~dead])
    c8 = types.SimpleNamespace(**dict(vars(c), kc=kd, vc=vd))
    refs = aa.ref_batch(c.q, kd, vd, c.slot_ids, c.starts, c.lens)
    return c8, tuple(t.to(dev()) for t in (k8, v8, ke, ve)), refs


def _launch(kind, q, cache, slot_ids, starts, lens):
    fn = ops.attn_append if kind == "bf16" else ops.attn_append_fp8
    out = fn(q.to(dev()), *cache, _i32(slot_ids), _i32(starts), _i32(lens),
             SCALE)
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _out(kind, case):
    c, cache, _ = _inputs(kind, case)
    return _launch(kind, c.q, cache, c.slot_ids, c.starts, c.lens)


def _check_seqs(tag, out, seqs):
    """seqs: [(label, batch index, q_len, ref)].  Every valid element inside
    the bound; one line with the worst err/tol."""
    worst, where = 0.0, None
    for label, b, ln, r in seqs:
        ok, ratio, _ = within(aa.seq_rows(out, b, ln), r.O, r.tol_O)
        if ratio > worst:
            worst, where = ratio, label
        if not ok:
            check(f"{tag} sequence {label}", aa.seq_rows(out, b, ln), r.O,
                  r.tol_O)
    print(f"[fp64] {tag}: worst err/tol = {worst:.3g} (sequence {where})")
    return worst


@pytest.mark.parametrize("case", aa.CASES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_against_fp64(kind, case):
    c, _, refs = _inputs(kind, case)
    out = _out(kind, case)
    assert out.shape == c.q.shape and out.dtype == torch.bfloat16
    # padding rows: q is zero there, their attention is finite
    assert bool(torch.isfinite(out.float()).all())
    for b, ln in enumerate(c.lens):     # padding-only tiles, empty sequence
        first = -(-ln // aa.BM) * aa.BM
        assert torch.count_nonzero(out[b, first:]) == 0, (b, ln)
    _check_seqs(f"{KERNEL[kind]} {case}", out,
                [((c.starts[b], c.lens[b]), b, c.lens[b], r)
                 for b, r in enumerate(refs) if r is not None])


ALONE = next(c for c in aa.CASES if c[0] == "A" and c[1] == "unit")


@pytest.mark.parametrize("kind", KINDS)
def test_sequence_alone_and_in_another_slot(kind):
    """No atomics, and nothing in a block depends on n or on which slot
    holds the rows: n = 1 gives the batch's bits, from the sequence's own
    slot and from a spare slot holding a copy of its rows."""
    c, cache, _ = _inputs(kind, ALONE)
    batch = _out(kind, ALONE)
    spare = sorted(set(range(c.slots)) - set(c.slot_ids))[0]
    assert spare != c.slots - 1
    for b, (start, ln) in enumerate(zip(c.starts, c.lens)):
        if ln == 0:
            continue
        moved = tuple(t.clone() for t in cache)
        for t in moved:
            t[spare] = t[c.slot_ids[b]]
        for name, cch, slot in (("alone", cache, c.slot_ids[b]),
                                ("moved", moved, spare)):
            one = _launch(kind, c.q[b:b + 1], cch, [slot], [start], [ln])
            assert_bits_equal(one[0, :ln], batch[b, :ln],
                              f"{KERNEL[kind]} {name} {(start, ln)}")


@pytest.mark.parametrize("geom", list(aa.GEOMS))
@pytest.mark.parametrize("kind", KINDS)
def test_nan_in_the_padding_rows_of_q(kind, geom):
    """Each lane owns one q column through both MFMAs and the softmax
    shuffles stay inside a column: garbage in rows >= q_len reaches no
    valid row."""
    case = next(c for c in aa.CASES if c[0] == geom and c[1] == "unit")
    c, cache, _ = _inputs(kind, case)
    q = c.q.clone()
    for b, ln in enumerate(c.lens):
        q[b, ln:] = float("nan")
    got = _launch(kind, q, cache, c.slot_ids, c.starts, c.lens)
    clean = _out(kind, case)
    for b, ln in enumerate(c.lens):
        assert_bits_equal(got[b, :ln], clean[b, :ln],
                          f"{KERNEL[kind]} {case} sequence {b}")
        first = -(-ln // aa.BM) * aa.BM
        assert torch.count_nonzero(got[b, first:]) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_guards(kind):
    """A slot outside [0, slots), a negative q_start or a negative q_len
    make the sequence empty (all zeros, no cache row read); q_len > Sq is
    Sq; q_start = 2^31 - 1 overflows nothing: kv_len = S_max and every row
    sees all S_max rows.  The good sequences of the batch are untouched."""
    c, cache, refs = _inputs(kind, ALONE)
    full = c.slots - 1                       # (72, 128): all S_max rows live
    assert c.slot_ids[0] == full and (c.starts[0], c.lens[0]) == (72, c.Sq)
    assert bool(torch.isfinite(c.kc[full].float()).all())
    big = 2 ** 31 - 1
    extra = [  # (slot, q_start, q_len, q taken from sequence)
        (-1, 0, 64, 1), (c.slots, 0, 64, 1), (full, -1, 64, 1),
        (full, 0, -5, 1), (full, 72, c.Sq + 7, 0), (full, big, 64, None)]
    q_big = c.q[0].clone()
    q_big[64:] = 0
    q = torch.cat([c.q] + [(q_big if src is None else c.q[src])[None]
                           for *_, src in extra])
    out = _launch(kind, q, cache,
                  c.slot_ids + [e[0] for e in extra],
                  c.starts + [e[1] for e in extra],
                  c.lens + [e[2] for e in extra])
    tag = KERNEL[kind] + " guards"
    assert_bits_equal(out[:c.n], _out(kind, ALONE), tag + ": good sequences")
    for i in range(4):
        assert torch.count_nonzero(out[c.n + i]) == 0, (tag, extra[i])
    assert_bits_equal(out[c.n + 4], out[0], tag + ": q_len = Sq + 7")
    assert bool(torch.isfinite(out[c.n + 5].float()).all())
    assert torch.count_nonzero(out[c.n + 5, 64:]) == 0
    r = aa.ref_seq(q_big, c.kc, c.vc, full, big, 64, SCALE)
    # every row sees the whole slot: row 0 of the chunk is no exception
    r0 = aa.ref_seq(q_big, c.kc, c.vc, full, c.S_max - 1, 1, SCALE)
    assert float((r.O[:, :1] - r0.O).abs().max()) < 1e-13
    _check_seqs(tag + " q_start = 2^31 - 1", out,
                [((big, 64), c.n + 5, 64, r),
                 ((72, c.Sq + 7), c.n + 4, c.Sq, refs[0])])


def test_rounding_bias():
    """P rounded to nearest errs symmetrically: with every row of V equal
    the mean signed relative error of O vanishes; a truncated P gives
    about -2e-3 (test_attn_append_reference.py, on the emulation)."""
    case = next(c for c in aa.CASES if c[0] == "C" and c[1] == "const_v")
    c, _, _ = _inputs("bf16", case)
    bias, off = aa.const_v_bias(c, _out("bf16", case))
    print(f"[bias] attn_append_kernel O {case}: mean signed rel err "
          f"{bias:.3g}, {off:.1%} of elements off v")
    assert abs(bias) <= BIAS, f"mean signed relative error {bias:.3g}"
