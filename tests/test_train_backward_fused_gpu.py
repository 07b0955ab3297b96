"""The training backward with gradients written where their consumers want
them: ops.linear_swiglu in the MLP and BucketedDDP(direct_wgrad=True), against
the model composed of ops.linear + ops.swiglu under direct_wgrad=False.
Nothing changes arithmetic: losses and gradients are compared bit for bit
(0 + g and g differ only for g = -0, which torch.equal takes as equal)."""
import pytest
import torch

from skypilot_amd import ops
from skypilot_amd.parallel.ddp import BucketedDDP
from skypilot_amd.train.trainer import TrainConfig, Trainer

gpu = pytest.mark.gpu


def run_steps(monkeypatch, device, seq_len, new, grad_accum=1, bucket_mb=64,
              steps=2):
    """Losses and every parameter's _sky_grad after each of `steps`
    train_steps on fixed batches (the second step starts from buckets that
    the first one filled, which is where skipping a zero fill can go wrong).  new=False: the MLP as it was (two ops)
    and every weight gradient through the DDP's hook."""
    with monkeypatch.context() as mp:
        # rmsnorm_bwd sums the norm-weight gradient with fp32 atomics, whose
        # order moves its last bits from run to run of one build.  Both arms
        # take the plain-torch norm instead, which is reproducible, so that
        # every parameter can be held to bit equality over two steps.
        mp.setattr(ops, "rmsnorm",
                   lambda x, w, eps=1e-5: ops.rmsnorm_ref(x, w, eps))
        if not new:
            mp.setattr(ops, "linear_swiglu",
                       lambda x, w: ops.swiglu(ops.linear(x, w)))
        tr = Trainer(TrainConfig(model="llama-debug", micro_batch=2,
                                 seq_len=seq_len, device=device, seed=5,
                                 grad_accum=grad_accum, bucket_mb=bucket_mb,
                                 direct_wgrad=new))
        out = []
        for _ in range(steps):
            loss = tr.train_step()
            grads = {n: p._sky_grad.clone()
                     for n, p in tr.model.named_parameters()}
            assert all(p.grad is None for p in tr.model.parameters())
            out.append((loss, grads))
    return tr, out


def assert_same(a, b):
    for (la, ga), (lb, gb) in zip(a, b):
        assert la == lb
        assert ga.keys() == gb.keys()
        for n in ga:
            assert torch.equal(ga[n], gb[n]), n


# bucket_mb = 0 gives every parameter a bucket of its own, so the buckets of
# the o, gate|up and down weights are written in place whole and the second
# step does not zero them; 64 puts the whole model in one bucket, which is
# zeroed as ever
@gpu
@pytest.mark.parametrize("seq_len", [128, 256])
@pytest.mark.parametrize("bucket_mb", [64, 0])
def test_step_equals_composed_model_on_hook_path(monkeypatch, seq_len,
                                                 bucket_mb):
    _, ref = run_steps(monkeypatch, "cuda", seq_len, new=False,
                       bucket_mb=bucket_mb)
    tr, got = run_steps(monkeypatch, "cuda", seq_len, new=True,
                        bucket_mb=bucket_mb)
    assert_same(got, ref)
    direct = [b for b in tr.ddp.buckets if len(b.direct) == len(b.params)]
    # per layer wo, w_gate_up and w_down; q, k and v stay on the hook
    assert len(direct) == (3 * tr.model.cfg.num_layers if bucket_mb == 0
                           else 0)
    tr.ddp.zero_grad()
    assert all(not b.zeroed for b in direct)
    assert all(b.zeroed for b in tr.ddp.buckets if b not in direct)


@gpu
@pytest.mark.parametrize("seq_len", [128, 256])
def test_grad_accum_second_micro_step_takes_the_hook(monkeypatch, seq_len):
    _, ref = run_steps(monkeypatch, "cuda", seq_len, new=False, grad_accum=2,
                       bucket_mb=0)
    _, got = run_steps(monkeypatch, "cuda", seq_len, new=True, grad_accum=2,
                       bucket_mb=0)
    assert_same(got, ref)


class _Two(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(2)
        self.a = torch.nn.Parameter(torch.randn(64, 64, generator=g).bfloat16())
        self.b = torch.nn.Parameter(torch.randn(64, 64, generator=g).bfloat16())


@gpu
def test_unzeroed_bucket_survives_a_change_of_path():
    """A bucket written in place in one step is not zeroed for the next.  If
    its parameter then comes through the hook after all, the gradient is
    copied, not added to the old one; if it gets no gradient, finish()
    zeroes it."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(128, 64, generator=g).bfloat16().to("cuda:0")
    dy = torch.randn(128, 64, generator=g).bfloat16().to("cuda:0")
    lin = torch.nn.functional.linear
    # per step: the call that uses a, the one that uses b (None: unused),
    # and whether zero_grad is to skip the two buckets
    plan = [(ops.linear, ops.linear, False),    # both written in place
            (lin, None, True),                  # a through the hook, b unused
            (ops.linear, lin, False)]           # so both were zeroed again

    def run(direct):
        m = _Two().to("cuda:0")
        ddp = BucketedDDP(m, bucket_bytes=0, direct_wgrad=direct)
        out = []
        for fa, fb, skipped in plan:
            ddp.zero_grad()
            if direct:
                assert [not b.zeroed for b in ddp.buckets] == [skipped] * 2
            ddp.mark_step_start()
            y = (fa(x, m.a) * dy).sum()
            if fb is not None:
                y = y + (fb(x, m.b) * dy).sum()
            y.backward()
            ddp.finish()
            assert m.a.grad is None and m.b.grad is None
            out.append((m.a._sky_grad.clone(), m.b._sky_grad.clone()))
        return out

    ref, got = run(False), run(True)
    for (ra, rb), (ga, gb) in zip(ref, got):
        assert torch.equal(ga, ra) and torch.equal(gb, rb)
    assert bool((got[0][1] != 0).any()) and bool((got[1][1] == 0).all())
