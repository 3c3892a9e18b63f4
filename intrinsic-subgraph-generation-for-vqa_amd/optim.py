"""Adam on the library's multi-tensor kernels (include/isg_optim.h): the gradient norm, torch's clipping rule, the nonfinite-step
skip that GradScaler gives the reference's fp32 loop, and the update -- with no host read of a device value anywhere.

`Adam` IS a torch.optim.Adam: param_groups, state_dict(), load_state_dict(), zero_grad() and schedulers (torch's, ignite's) are
torch's own code, and a reference checkpoint's "optimizer" entry loads.  Only step() is replaced.  One step launches

  * one isg_mt_sqnorm pair over ALL groups' gradients when max_grad_norm or skip_nonfinite is set: the norm, the coefficient
    min(1, max_norm / (norm + 1e-6)) and a finite flag stay on the device (last_grad_norm, last_clip);
  * one isg_mt_adam pair per param group, with that group's lr / betas / eps / weight_decay as kernel arguments (a scheduler that
    writes param_groups[i]["lr"] just works).  Its one-thread prologue advances the step counter and forms the bias corrections
    in double; on a nonfinite norm it marks the step skipped instead, and params, moments and counter keep their bits.

The per-parameter state is torch's (`exp_avg`, `exp_avg_sq`, `step`); `step` is ONE device float64 0-dim tensor that every
parameter's entry refers to, so the layout stays torch's while the kernels advance one counter.  state_dict() hands out a copy
per entry (a plain torch.optim.Adam that loads it counts every entry on its own); after load_state_dict the counter is taken from
the first entry and shared again.  `amsgrad`, `maximize`, tensor learning rates and sparse gradients are
not built and refused.

The kernels read the tensors through a device table of addresses.  It is staged through a FRESH pinned buffer and copied without
a sync whenever an address changed since the last step (zero_grad(set_to_none=True) frees the gradients; the caching allocator
usually hands the same blocks back, and then nothing is sent).  A staging buffer is never rewritten: torch's pinned allocator
keeps a block that a pending copy reads out of circulation until the copy has run.

With `grad_sync` (a distributed.GradSync that is active) the gradient column of the table holds the addresses of the sync's bucket
slots, for every parameter of the sync's set -- also one whose local p.grad is None, which steps with the other ranks' average.
The norm is then the norm of the AVERAGED gradients (DistributedDataParallel followed by clip_grad_norm_), identical on every
rank, and so is the decision to skip; the slots never move, so the table is sent once per run.

When the norm is taken (either option set), a nonfinite norm always skips the step: with skip_nonfinite=False and a
max_grad_norm, torch would multiply every gradient by NaN instead; that is not reproduced.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib, ops

# launches since import, by entry point: tests count them (no norm launch without max_grad_norm / skip_nonfinite)
LAUNCHES = {"sqnorm": 0, "adam": 0, "table_copies": 0}


def chunk_prefix(numels: Sequence[int], chunk: int) -> List[int]:
    """[T + 1] chunk counts in front of each tensor, as include/isg_optim.h defines the table's third array: tensor t owns the
    chunks prefix[t] .. prefix[t + 1] - 1, ceil(numel / chunk) of them (none for an empty tensor)."""
    out = [0]
    for n in numels:
        out.append(out[-1] + (int(n) + chunk - 1) // chunk)
    return out


def _check_param(p: Tensor, name: str) -> None:
    """Refuse what the kernels do not take, naming the parameter."""
    if not p.is_cuda:
        raise _lib.IsgError(f"optim.Adam: {name} lives on {p.device}; the optimizer's kernels run on the GPU and have no CPU fallback")
    if p.dtype != torch.float32:
        raise TypeError(f"optim.Adam: {name} is {p.dtype}; the kernels update fp32 parameters")
    if not p.is_contiguous():
        raise ValueError(f"optim.Adam: {name} is not contiguous; the kernels address a parameter as one flat array")


class Adam(torch.optim.Adam):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled: bool = False, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = True, amsgrad: bool = False,
                 grad_sync=None):
        if amsgrad:
            raise NotImplementedError("optim.Adam: amsgrad=True is not built (no max_exp_avg_sq in the kernel)")
        if isinstance(lr, Tensor):
            raise TypeError("optim.Adam: a tensor lr would be read on the host every step; pass a float")
        self.decoupled, self.skip_nonfinite = bool(decoupled), bool(skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_sync = grad_sync
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False)
        first = self.param_groups[0]["params"][0]
        dev = self._device = first.device
        for group in self.param_groups:
            for p in group["params"]:
                if p.device != dev:
                    raise ValueError(f"optim.Adam: parameters on {dev} and on {p.device}; one optimizer drives one device")
        self._step = torch.zeros((), dtype=torch.float64, device=dev)       # every state entry's "step"
        self._clip = torch.zeros(4, dtype=torch.float32, device=dev)        # {norm, coef, finite, 0}
        self._state = torch.zeros(4, dtype=torch.float64, device=dev)       # the prologue's {bc1, bc2, applies, step}
        self.skipped_steps = torch.zeros((), dtype=torch.float64, device=dev)
        self.last_grad_norm: Optional[Tensor] = None                        # device views of _clip once a norm was taken
        self.last_clip: Optional[Tensor] = None
        self._parts: Optional[Tensor] = None
        self._table: Optional[Tensor] = None
        self._table_key = None
        self._prefix: List[int] = [0]

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        gi = len(self.param_groups) - 1
        names = group.get("param_names")
        for i, p in enumerate(group["params"]):
            name = f"parameter '{names[i]}'" if names else f"parameter {i} of group {gi} (shape {tuple(p.shape)})"
            _check_param(p, name)
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("optim.Adam: amsgrad and maximize are not built")

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def _init_state(self, p: Tensor) -> dict:
        st = self.state[p]
        if len(st) == 0:
            st["step"] = self._step
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    def _share_step(self) -> None:
        """One counter for every entry again: torch's load_state_dict copies each entry's `step` on its own."""
        first = next((st["step"] for st in self.state.values() if "step" in st), None)
        if first is not None:
            self._step = torch.as_tensor(first).detach().to(device=self._device, dtype=torch.float64).reshape(()).clone()
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = self._step
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st and not (st[k].is_contiguous() and st[k].dtype == torch.float32 and st[k].device == p.device):
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()

    def state_dict(self):
        """torch's state_dict with every entry's `step` a copy of its own (a device-side clone): a plain torch.optim.Adam that
        loads it adds 1 to each entry per step, and entries that shared one tensor -- torch.save keeps the sharing -- would count
        every parameter."""
        sd = super().state_dict()
        sd["state"] = {k: {**st, "step": self._step.clone()} if "step" in st else st for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._share_step()
        self._table_key = None

    # ---- the step -------------------------------------------------------------------------------------------------------------
    def _rows(self):
        """[(param, grad, exp_avg, exp_avg_sq addresses, numel)] of the parameters that have a gradient, group after group, and
        each group's (first row, end row)."""
        rows, spans = [], []
        sync = self.grad_sync if self.grad_sync is not None and self.grad_sync.active else None
        for gi, group in enumerate(self.param_groups):
            r0 = len(rows)
            if isinstance(group["lr"], Tensor):
                raise TypeError("optim.Adam: a tensor lr would be read on the host every step; write a float into param_groups")
            for i, p in enumerate(group["params"]):
                if sync is not None:
                    if not sync.knows(p):
                        raise ValueError(f"optim.Adam: parameter {i} of group {gi} (shape {tuple(p.shape)}) is not among grad_sync's parameters")
                    if sync.has(p):               # the reduced gradient in its bucket slot, whether or not this rank had one
                        st = self._init_state(p)
                        rows.append((p.data_ptr(), sync.grad_ptr(p), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()))
                    continue
                g = p.grad
                if g is None:
                    continue                      # as torch: a parameter without a gradient sits this step out
                if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device:
                    raise ValueError(f"optim.Adam: the gradient of parameter {i} of group {gi} (shape {tuple(p.shape)}) is not a dense "
                                     "contiguous fp32 tensor on the parameter's device")
                st = self._init_state(p)
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()))
            spans.append((r0, len(rows)))
        return rows, spans

    def _send_table(self, rows, chunk: int) -> None:
        T = len(rows)
        self._prefix = chunk_prefix([r[4] for r in rows], chunk)
        flat = [a for r in rows for a in r[:4]] + [r[4] for r in rows] + self._prefix
        host = torch.tensor(flat, dtype=torch.int64)
        if self._device.type == "cuda":
            host = host.pin_memory()              # fresh per send: never rewritten under a pending copy
        if self._table is None or self._table.numel() != len(flat):
            self._table = torch.empty(len(flat), dtype=torch.int64, device=self._device)
        self._table.copy_(host, non_blocking=True)
        LAUNCHES["table_copies"] += 1
        assert self._table.numel() == 6 * T + 1

    @torch.no_grad()
    def step(self, closure=None, *, totals: Optional[Tensor] = None):
        """One step.  `totals` (train.Meters.totals) counts a skipped step in its slot 6; without it `skipped_steps` does."""
        from . import _lib_optim
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows, spans = self._rows()
        T = len(rows)
        if T == 0:
            return loss
        lib = _lib_optim.load()
        key = tuple(rows)
        if key != self._table_key:
            self._send_table(rows, int(lib.isg_mt_chunk_elems()))
            self._table_key = key
        base, prefix, stream = self._table.data_ptr(), self._prefix, ops._stream()
        table, numel, pref = base, base + 32 * T, base + 40 * T
        clip = 0
        if self.max_grad_norm is not None or self.skip_nonfinite:
            need = int(lib.isg_mt_sqnorm_parts(prefix[T]))
            if self._parts is None or self._parts.numel() < need:
                self._parts = torch.empty(need, dtype=torch.float64, device=self._device)
            clip = self._clip.data_ptr()
            _lib.check(lib.isg_mt_sqnorm(table, numel, pref, T, prefix[T], self._parts.data_ptr(), self.max_grad_norm or 0.0, clip,
                                         stream), "isg_mt_sqnorm")
            LAUNCHES["sqnorm"] += 1
            if self.last_grad_norm is None:
                self.last_grad_norm, self.last_clip = self._clip[0], self._clip[1]
        skipped = self.skipped_steps if totals is None else totals
        skipped_ptr = skipped.data_ptr() + (0 if totals is None else 8 * 6)
        if totals is not None and (totals.dtype != torch.float64 or totals.numel() != 8 or totals.device != self._device):
            raise ValueError("optim.Adam.step: totals is train.Meters.totals, a float64 [8] on the optimizer's device")
        advance = 1
        for group, (r0, r1) in zip(self.param_groups, spans):
            if r1 == r0:
                continue
            b1, b2 = group["betas"]
            _lib.check(lib.isg_mt_adam(table + 32 * r0, numel + 8 * r0, pref + 8 * r0, r1 - r0, prefix[r1] - prefix[r0], clip,
                                       self._step.data_ptr(), self._state.data_ptr(), skipped_ptr, advance, float(group["lr"]),
                                       float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                       int(self.decoupled), stream), "isg_mt_adam")
            LAUNCHES["adam"] += 1
            advance = 0
        return loss
