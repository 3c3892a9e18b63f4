"""A training step and a validation pass whose tails stay on the device: what the reference's train_epoch / validate_epoch do
after the classifier (accuracy, CrossEntropyLoss, clip_grad_norm_(max_norm=2.0), Adam.step, the AverageMeters), with no host read
of a device value until Meters.report().

GradScaler is not reproduced.  The reference wraps its fp32 loop in one (no autocast region is active around the forward), where
the scale is a power of two that multiplies the loss and divides the gradients again exactly; its only effect there is that a step
whose gradients hold an Inf or a NaN is skipped -- which is optim.Adam(skip_nonfinite=True), decided on the device from the norm
that the clipping takes anyway.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import torch
from torch import Tensor

from . import ops, optim


class Meters:
    """The running meters of an epoch as ONE device float64 [8] (include/isg_optim.h, ISG_TOT_*), advanced by ops.cross_entropy
    and optim.Adam.step inside their own launches.  report() is the single device-to-host copy."""

    def __init__(self, device):
        self.totals = torch.zeros(8, dtype=torch.float64, device=device)

    def reset(self) -> None:
        self.totals.zero_()

    @staticmethod
    def summarize(totals: Sequence[float]) -> dict:
        """The reference's two AverageMeters from the totals.  `losses.update(loss.item(), B)` runs only for a loss that is not NaN:
        avg = sum(loss_i * B_i) / sum(B_i) over those steps (0 before the first, as AverageMeter starts).
        `ans_short.update(acc1_i, B_i)` with acc1_i = 100 * correct_i / B_i runs every step: avg = 100 * sum(correct_i) / sum(B_i)."""
        t = [float(v) for v in totals]
        return {"loss": t[0] / t[1] if t[1] > 0 else 0.0,
                "acc1": 100.0 * t[2] / t[3] if t[3] > 0 else 0.0,
                "steps": int(t[4]), "skipped_steps": int(t[6]), "nonfinite_losses": int(t[5]), "rows": int(t[3])}

    def report(self, group=None) -> dict:
        """The meters on the host.  With a process group (torch.distributed.group.WORLD for the default one) the loss sums, the
        rows, the correct answers and the nonfinite losses -- slots 0-3 and 5 -- are summed over its ranks first, in one
        all-reduce; `steps` and `skipped_steps` (slots 4 and 6) stay this rank's: every rank takes the same steps, and skips the
        same ones, because the skip is decided from the same reduced gradients."""
        totals = self.totals
        if group is not None:
            import torch.distributed as dist
            idx = torch.tensor([0, 1, 2, 3, 5], device=totals.device)
            summed = totals[idx]
            dist.all_reduce(summed, group=group)
            totals = totals.clone()
            totals[idx] = summed
        return self.summarize(totals.cpu().tolist())


def _logits(model, inputs, seed: Optional[int]) -> Tensor:
    kw = {} if seed is None else {"seed": seed}
    if isinstance(inputs, dict):
        out = model(**inputs, **kw)
    elif isinstance(inputs, (tuple, list)):
        out = model(*inputs, **kw)
    else:
        out = model(inputs, **kw)
    return out[0] if isinstance(out, tuple) else out


def train_step(model, optimizer, inputs, labels: Tensor, meters: Meters, seed: Optional[int] = None, sync=None, accumulate: int = 1,
               micro: int = 0) -> ops.CrossEntropy:
    """One step of the reference's train_epoch body, in its order: n_train_steps += B, the forward (`inputs`: a dict of keyword
    arguments, a tuple of positional ones, or the model's single argument; the logits are the output or its first entry), the loss
    with the meters, zero_grad, the backward, optimizer.step().  Nothing here waits for the device.

    `sync` (a distributed.GradSync; the optimizer was built with grad_sync=sync): after the backward the gradients are packed into
    the sync's bucket, averaged over the ranks in one all-reduce, and the optimizer steps from the bucket.  The seed becomes
    seed * world + rank, so dropout and the samplers' noise differ from rank to rank.
    `accumulate` > 1 (needs an active sync; GradSync(..., force=True) on one GPU): the call is micro-batch `micro` of `accumulate`.
    Every micro-batch adds its gradients / accumulate into the bucket (micro 0 overwrites it); the all-reduce and the optimizer's
    step run on the last one only."""
    accumulate, micro = int(accumulate), int(micro)
    if accumulate < 1 or not 0 <= micro < accumulate:
        raise ValueError(f"train_step: micro-batch {micro} of {accumulate}")
    active = sync is not None and sync.active
    if accumulate > 1 and not active:
        raise ValueError("train_step: accumulate > 1 adds the micro-batches' gradients in a GradSync's bucket; pass sync=GradSync(..., "
                         "force=True) and build the optimizer with grad_sync=sync")
    if active and getattr(optimizer, "grad_sync", None) is not sync:
        raise ValueError("train_step: the optimizer does not read this sync's bucket; build it as optim.Adam(..., grad_sync=sync)")
    if active and seed is not None:
        seed = seed * sync.world + sync.rank
    model.n_train_steps = getattr(model, "n_train_steps", 0) + labels.size(0)
    logits = _logits(model, inputs, seed)
    res = ops.cross_entropy(logits, labels, totals=meters.totals)
    optimizer.zero_grad()
    res.loss.backward()
    if active:
        sync.pack(accumulate=micro > 0, scale=1.0 / accumulate)
        if micro < accumulate - 1:
            return res
        sync.reduce()
    if isinstance(optimizer, optim.Adam):
        optimizer.step(totals=meters.totals)
    else:
        optimizer.step()
    return res


def validate(model, batches: Iterable, meters: Meters, seed: Optional[int] = None, group=None) -> Optional[dict]:
    """The reference's validate_epoch: eval mode, no_grad, forward and loss of every (inputs, labels) of `batches` into the meters.
    The model's mode is restored.  Nothing here waits for the device -- unless a process group is given: then every rank ran its
    own share of the batches, and meters.report(group), the meters summed over the ranks as AverageMeter.synchronize_between_processes
    sums them, is returned."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for inputs, labels in batches:
                model.n_valid_steps = getattr(model, "n_valid_steps", 0) + labels.size(0)
                ops.cross_entropy(_logits(model, inputs, seed), labels, totals=meters.totals)
    finally:
        model.train(was_training)
    return None if group is None else meters.report(group)
