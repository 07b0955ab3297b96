"""Without a GPU ops.linear_swiglu is swiglu(linear()) and
BucketedDDP(direct_wgrad=True) is the hook path: no weight asks for its
bucket view, and every bucket is zeroed every step."""
import torch

from skypilot_amd import ops
from skypilot_amd.train.trainer import TrainConfig, Trainer


def test_linear_swiglu_is_the_composition():
    assert "linear_swiglu" in ops.__all__
    g = torch.Generator().manual_seed(1)
    outs = []
    for fused in (True, False):
        x = torch.randn(3, 5, 16, generator=g.manual_seed(1)).requires_grad_()
        w = torch.randn(24, 16, generator=g).requires_grad_()
        y = (ops.linear_swiglu(x, w) if fused
             else ops.swiglu(ops.linear(x, w)))
        y.square().sum().backward()
        outs.append((y.detach(), x.grad, w.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_direct_wgrad_on_cpu_is_the_hook_path():
    runs = []
    for direct in (True, False):
        tr = Trainer(TrainConfig(model="llama-debug", micro_batch=1,
                                 seq_len=32, device="cpu", seed=7,
                                 grad_accum=2, bucket_mb=0,
                                 direct_wgrad=direct))
        losses = [tr.train_step() for _ in range(2)]
        assert all(b.zeroed and not b.direct for b in tr.ddp.buckets)
        assert all(p.grad is None for p in tr.model.parameters())
        runs.append((losses, [p._sky_grad.clone()
                              for p in tr.model.parameters()]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
