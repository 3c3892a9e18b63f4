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


class TypedMeters(Meters):
    """Meters with a device float64 [G, 8] table beside the [8] one: a row per group of `types` (a datasets.gqa.QuestionTypes), slots
    ISG_GRP_* of include/isg_eval.h, advanced by ops.group_meters in validate(); `overall` holds the same slots over all rows (its
    hits at k give the overall acc@k).  The three blocks are ONE allocation, so report() stays a single device-to-host copy (and a
    single all-reduce).  `status` (int32 [2]) counts group ids outside the id space; it is not part of the report."""

    def __init__(self, device, types, k: int = 5):
        self.types, self.k = types, int(k)
        G = int(types.num_groups)
        if not 1 <= G <= ops.EVAL_GROUPS_MAX or self.k < 1:
            raise ValueError(f"TypedMeters: {G} groups (1 to {ops.EVAL_GROUPS_MAX}), k = {k} (>= 1)")
        self._all = torch.zeros(16 + G * ops.GROUP_SLOTS, dtype=torch.float64, device=device)
        self.totals = self._all[:8]
        self.overall = self._all[8:16]
        self.groups = self._all[16:].view(G, ops.GROUP_SLOTS)
        self.status = torch.zeros(2, dtype=torch.int32, device=device)

    def reset(self) -> None:
        self._all.zero_()
        self.status.zero_()

    def summarize(self, totals: Sequence[float]) -> dict:
        """Meters.summarize of the first 8 entries, then `acc@k` = 100 * hits at k / rows of the pass (the reference's
        accuracy(topk=(1, k)) through its AverageMeter) from the next 8, and `by_type`: {facet: {name: {loss, acc1, acc@k, rows}}}
        from the [G, 8] rows behind them.  A group without rows reports 0, as an AverageMeter that was never updated;
        its loss is the mean of the finite row losses (the overall `loss` is the reference's mean of batch means)."""
        t = [float(v) for v in totals]
        out = Meters.summarize(t[:8])
        key = f"acc@{self.k}"
        by_type, base = {f: {} for f in self.types.facets}, 16
        for g, (facet, name) in enumerate(self.types.group_names):
            rows, loss, bad, hit1, hitk = t[base + g * ops.GROUP_SLOTS:base + g * ops.GROUP_SLOTS + 5]
            by_type[facet][name] = {"loss": loss / (rows - bad) if rows - bad > 0 else 0.0,
                                    "acc1": 100.0 * hit1 / rows if rows > 0 else 0.0,
                                    key: 100.0 * hitk / rows if rows > 0 else 0.0, "rows": int(rows)}
        out[key] = 100.0 * t[8 + 4] / t[3] if t[3] > 0 else 0.0
        out["by_type"] = by_type
        return out

    def report(self, group=None) -> dict:
        """As Meters.report; with a process group the overall block and the [G, 8] table are summed over the ranks in the same
        single all-reduce as slots 0-3 and 5."""
        both = self._all
        if group is not None:
            import torch.distributed as dist
            idx = torch.cat([torch.tensor([0, 1, 2, 3, 5], device=both.device), torch.arange(8, both.numel(), device=both.device)])
            summed = both[idx]
            dist.all_reduce(summed, group=group)
            both = both.clone()
            both[idx] = summed
        return self.summarize(both.cpu().tolist())


def _logits(model, inputs, seed: Optional[int]) -> Tensor:
    kw = {} if seed is None else {"seed": seed}
    if isinstance(inputs, dict):
        out = model(**inputs, **kw)
    elif isinstance(inputs, (tuple, list)):
        out = model(*inputs, **kw)
    else:
        out = model(inputs, **kw)
    return out[0] if isinstance(out, tuple) else out


class SharedScenes(torch.nn.Module):
    """A model seen through ISubGVQA.forward_shared: forward(**inputs) returns its 5-tuple (the GraphInstances is dropped), so
    train_step and validate drive a batch of distinct scene graphs with a graph index like any other batch.  The step counters
    are the wrapped model's."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    @property
    def n_train_steps(self):
        return self.model.n_train_steps

    @n_train_steps.setter
    def n_train_steps(self, value):
        self.model.n_train_steps = value

    @property
    def n_valid_steps(self):
        return self.model.n_valid_steps

    @n_valid_steps.setter
    def n_valid_steps(self, value):
        self.model.n_valid_steps = value

    def forward(self, **inputs):
        return self.model.forward_shared(**inputs)[0]


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
    sums them, is returned.

    A batch may be (inputs, labels, groups): groups is the int32 [B, F] of QuestionTypes.encode, on the host (pinned: the copy is
    asynchronous) or already on the device.  With a TypedMeters the pass adds ops.answer_rank and ops.group_meters behind the loss:
    three launches more per batch, still no wait.  With plain Meters the groups are not looked at."""
    typed = isinstance(meters, TypedMeters)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                inputs, labels = batch[0], batch[1]
                model.n_valid_steps = getattr(model, "n_valid_steps", 0) + labels.size(0)
                logits = _logits(model, inputs, seed)
                res = ops.cross_entropy(logits, labels, totals=meters.totals)
                if typed:
                    if len(batch) < 3 or batch[2] is None:
                        raise ValueError("validate: TypedMeters needs (inputs, labels, groups) batches (QuestionTypes.encode)")
                    groups = batch[2].to(logits.device, non_blocking=True)
                    rank = ops.answer_rank(logits, labels, k=meters.k).rank
                    ops.group_meters(res.row_loss, rank, groups, meters.groups, k=meters.k, status=meters.status,
                                     overall=meters.overall)
    finally:
        model.train(was_training)
    return None if group is None else meters.report(group)
