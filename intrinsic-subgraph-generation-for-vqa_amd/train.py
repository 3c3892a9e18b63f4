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

    def report(self) -> dict:
        return self.summarize(self.totals.cpu().tolist())


def _logits(model, inputs, seed: Optional[int]) -> Tensor:
    kw = {} if seed is None else {"seed": seed}
    if isinstance(inputs, dict):
        out = model(**inputs, **kw)
    elif isinstance(inputs, (tuple, list)):
        out = model(*inputs, **kw)
    else:
        out = model(inputs, **kw)
    return out[0] if isinstance(out, tuple) else out


def train_step(model, optimizer, inputs, labels: Tensor, meters: Meters, seed: Optional[int] = None) -> ops.CrossEntropy:
    """One step of the reference's train_epoch body, in its order: n_train_steps += B, the forward (`inputs`: a dict of keyword
    arguments, a tuple of positional ones, or the model's single argument; the logits are the output or its first entry), the loss
    with the meters, zero_grad, the backward, optimizer.step().  Nothing here waits for the device."""
    model.n_train_steps = getattr(model, "n_train_steps", 0) + labels.size(0)
    logits = _logits(model, inputs, seed)
    res = ops.cross_entropy(logits, labels, totals=meters.totals)
    optimizer.zero_grad()
    res.loss.backward()
    if isinstance(optimizer, optim.Adam):
        optimizer.step(totals=meters.totals)
    else:
        optimizer.step()
    return res


def validate(model, batches: Iterable, meters: Meters, seed: Optional[int] = None) -> None:
    """The reference's validate_epoch: eval mode, no_grad, forward and loss of every (inputs, labels) of `batches` into the meters.
    The model's mode is restored.  Nothing here waits for the device."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for inputs, labels in batches:
                model.n_valid_steps = getattr(model, "n_valid_steps", 0) + labels.size(0)
                ops.cross_entropy(_logits(model, inputs, seed), labels, totals=meters.totals)
    finally:
        model.train(was_training)
