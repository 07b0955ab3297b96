"""Bucketed data parallelism over RCCL/xGMI — MI355X-native DDP.

Not a wrapper around ``torch.nn.parallel.DistributedDataParallel``: as
each parameter's gradient is accumulated, a post-accumulate hook moves it
into a flat per-bucket bf16 buffer and the bucket all-reduces
asynchronously the moment its last grad lands — communication overlaps
the rest of backward.  The fused AdamW consumes the bucket views
directly (``p._sky_grad`` attribute), so gradients are never re-gathered.

Bucket size defaults to 64 MiB: xGMI is point-to-point (7 links x
~153 GB/s per MI355X), so ring all-reduce is per-link bound and wants
fewer, larger transfers than an NVSwitch fabric.
The all-reduce SUMs; averaging is folded into the fused AdamW's
grad_scale so no extra pass over the gradients is needed.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

DEFAULT_BUCKET_BYTES = 64 << 20


def _initialized() -> bool:
    return dist.is_available() and dist.is_initialized()


class GradBucket:
    def __init__(self, params, device, dtype):
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.flat = torch.zeros(self.numel, device=device, dtype=dtype)
        self.views = {}
        off = 0
        for p in params:
            self.views[p] = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.pending = 0
        self.work = None
        # direct_wgrad bookkeeping (BucketedDDP): `zeroed` says zero_grad
        # cleared flat for the current step; `fresh` holds the parameters
        # with no gradient in flat yet this step; `counted` those whose
        # gradient of the current backward is in; `direct` those whose first
        # gradient of the step was written in place by its producer.
        self.zeroed = True
        self.fresh = set()
        self.counted = set()
        self.direct = set()


class _WgradSink:
    """What BucketedDDP(direct_wgrad=True) offers a weight as
    ``p._sky_wgrad_sink``.  A backward that can write its weight gradient
    anywhere (ops.linear) asks ``take()`` for the bucket view: it gets one
    only for the step's first gradient of that parameter, writes dW into it,
    returns no gradient to autograd and calls ``done()``, which does the
    bookkeeping of the post-accumulate hook that then never runs."""

    def __init__(self, ddp, p):
        self.ddp, self.p = ddp, p

    def take(self):
        b = self.ddp._p2b[self.p]
        if self.p not in b.fresh:
            return None
        b.fresh.discard(self.p)
        b.direct.add(self.p)
        return b.views[self.p]

    def done(self):
        self.ddp._grad_landed(self.p)


class BucketedDDP:
    """Gradient-summing DDP with comm/compute overlap.

    Usage per step:
        ddp.zero_grad(); then per micro-step
        ddp.mark_step_start(); loss.backward(); ddp.finish()
    After ``finish`` each param's gradient (summed over ranks) is in
    ``p._sky_grad``; divide-by-world is folded into the optimizer via
    ``ddp.grad_scale``.

    ``direct_wgrad=True``: 2-D parameters that appear once in the model get
    a ``_sky_wgrad_sink`` (_WgradSink), through which ops.linear's backward
    writes the step's first weight gradient straight into the bucket view
    instead of into a fresh tensor that the hook then adds onto zeros.  A
    bucket all of whose parameters were written that way in the last step
    is not zeroed for the next one; a parameter of such a bucket that is
    not written in place after all has its first gradient copied rather
    than added, or is zeroed in ``finish`` if it gets none.  The values are
    those of the hook path, except that ``0 + g`` turns a ``-0`` into
    ``+0`` and ``g`` alone does not.  ``False`` is the hook path for every
    parameter.
    """

    def __init__(self, model: torch.nn.Module,
                 bucket_bytes: int = DEFAULT_BUCKET_BYTES,
                 process_group=None, direct_wgrad: bool = True):
        self.model = model
        self.group = process_group
        self.direct_wgrad = direct_wgrad
        self.world = dist.get_world_size(process_group) if _initialized() else 1
        params = [p for p in model.parameters() if p.requires_grad]
        # Reverse registration order approximates backward completion order,
        # so early buckets fill (and start reducing) first.
        params = list(reversed(params))
        self.buckets: list[GradBucket] = []
        cur, cur_bytes = [], 0
        for p in params:
            cur.append(p)
            cur_bytes += p.numel() * p.element_size()
            if cur_bytes >= bucket_bytes:
                self.buckets.append(GradBucket(cur, p.device, p.dtype))
                cur, cur_bytes = [], 0
        if cur:
            self.buckets.append(GradBucket(cur, cur[0].device, cur[0].dtype))
        # A tied parameter gets gradients from two layers in one backward:
        # the second would be added after the sink counted the first, maybe
        # after the bucket's all-reduce has started.  It stays on the hook.
        uses = {}
        for _, p in model.named_parameters(remove_duplicate=False):
            uses[p] = uses.get(p, 0) + 1
        self._p2b = {}
        for b in self.buckets:
            for p in b.params:
                self._p2b[p] = b
                p._sky_grad = b.views[p]
                p.register_post_accumulate_grad_hook(self._hook)
                if direct_wgrad and p.dim() == 2 and uses.get(p, 0) == 1:
                    p._sky_wgrad_sink = _WgradSink(self, p)
                elif hasattr(p, "_sky_wgrad_sink"):
                    del p._sky_wgrad_sink   # an earlier DDP's
        self._accumulating = False
        if self.world > 1:
            for p in model.parameters():
                dist.broadcast(p.data, src=self._rank0(), group=self.group)

    def _rank0(self) -> int:
        return 0 if self.group is None else dist.get_global_rank(self.group, 0)

    def _grad_landed(self, p):
        """p's gradient of this backward is in its bucket."""
        b = self._p2b[p]
        if p in b.counted:   # a second gradient in one backward
            return
        b.counted.add(p)
        b.pending -= 1
        if b.pending == 0 and self.world > 1 and not self._accumulating:
            b.work = dist.all_reduce(b.flat, op=dist.ReduceOp.SUM,
                                     group=self.group, async_op=True)

    def _hook(self, p):
        if p.grad is None:
            # autograd still visits the parameter when its producer returned
            # no gradient, having written it through the sink
            return
        b = self._p2b[p]
        # Accumulate: zero_grad() clears the flat buffers at the start of
        # each optimizer step, so add_ is correct for both the
        # single-micro-step case and every micro-step of grad accumulation.
        # (copy_ on the final micro-step would overwrite the accumulated
        # sum from earlier micro-steps.)  Only the step's first gradient
        # into a bucket that zero_grad() skipped is copied.
        if p in b.fresh and not b.zeroed:
            b.views[p].copy_(p.grad)
        else:
            b.views[p].add_(p.grad)
        b.fresh.discard(p)
        p.grad = None  # free eagerly; flat buffer is the only grad storage
        self._grad_landed(p)

    def mark_step_start(self, accumulating: bool = False):
        """Call before each backward. ``accumulating=True`` defers the
        all-reduce (gradient accumulation micro-steps)."""
        self._accumulating = accumulating
        for b in self.buckets:
            b.pending = len(b.params)
            b.counted.clear()
            b.work = None

    def zero_grad(self):
        for b in self.buckets:
            # every parameter written in place last step: expect the same
            # again and leave the old values to be overwritten
            b.zeroed = not (self.direct_wgrad
                            and len(b.direct) == len(b.params))
            if b.zeroed:
                b.flat.zero_()
            b.fresh = set(b.params)
            b.direct.clear()

    def finish(self):
        """Wait for outstanding bucket reductions (call after backward)."""
        for b in self.buckets:
            if not b.zeroed and b.fresh and not self._accumulating:
                # the expectation failed: no gradient this step after all
                assert b.work is None
                for p in b.fresh:
                    b.views[p].zero_()
                b.fresh.clear()
            if b.work is not None:
                b.work.wait()
            elif self.world > 1 and not self._accumulating:
                dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group)

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world
