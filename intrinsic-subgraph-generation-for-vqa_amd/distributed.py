"""Data-parallel sharding of a PyG-style batch by graph, and the logits all-gather.

The reference scales out with DDP only: every rank owns an independent Batch with LOCAL node / graph
indices (main.py:72-94, datasets/build.py:44-49).  Inference needs no gradient exchange, so the only
collective of this path is one all-gather of answer logits [B_local, 1842] per step (RCCL over xGMI when
the process group backend is "nccl"; gloo in the CPU tests).  Because of reference quirks Q1/Q3/Q4 a
shard's result is defined as the CPU path run on that shard ALONE: shards are re-indexed
locally and nothing else crosses ranks.

Training exchanges gradients: GradSync packs every gradient, scaled by 1 / world, into ONE persistent flat fp32
bucket (isg_mt_pack, include/isg_dist.h), all-reduces the bucket once per step, and optim.Adam(grad_sync=...) takes the norm and
the update from the reduced bucket in place.  What replaces DistributedDataParallel(...) is in INTEGRATION.md.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .synthetic import FullWorkload, Workload


def graph_ranges(nodes_per_graph: Tensor, edges_per_graph: Optional[Tensor], world: int, balance: bool = False
                 ) -> List[Tuple[int, int]]:
    """Contiguous graph ranges [lo, hi) per rank.  balance=False: equal graph counts (cfg4);
    balance=True: equalise sum(nodes + edges) per rank (cfg5, skewed graphs)."""
    B = nodes_per_graph.numel()
    if not balance or edges_per_graph is None:
        step = (B + world - 1) // world
        return [(min(r * step, B), min((r + 1) * step, B)) for r in range(world)]
    cost = (nodes_per_graph + edges_per_graph).double().cumsum(0)
    total = float(cost[-1]) if B else 0.0
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        i = int(torch.searchsorted(cost, torch.tensor(target, dtype=torch.double)))   # graph holding the target
        below = float(cost[i - 1]) if i > 0 else 0.0
        above = float(cost[i]) if i < B else total
        c = i if (target - below) <= (above - target) else i + 1                       # nearer boundary
        cuts.append(min(max(c, cuts[-1]), B))
    cuts.append(B)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def shard_workload(wl, rank: int, world: int, balance: bool = False):
    """Rank `rank`'s contiguous graph range of `wl` (a Workload, or the full model's FullWorkload with its questions), re-indexed
    locally (works on any device)."""
    if isinstance(wl, FullWorkload):
        return _shard_full_workload(wl, rank, world, balance)
    B = wl.glf.size(0)
    npg = torch.bincount(wl.batch, minlength=B)
    eg = wl.batch[wl.edge_index[1]]
    epg = torch.bincount(eg, minlength=B)
    lo, hi = graph_ranges(npg.cpu(), epg.cpu(), world, balance)[rank]
    ptr = torch.zeros(B + 1, dtype=torch.long, device=wl.batch.device)
    ptr[1:] = npg.cumsum(0)
    n_lo, n_hi = int(ptr[lo]), int(ptr[hi])
    emask = (eg >= lo) & (eg < hi)
    return Workload(x=wl.x[n_lo:n_hi].contiguous(), edge_index=(wl.edge_index[:, emask] - n_lo).contiguous(),
                    edge_attr=wl.edge_attr[emask].contiguous(), batch=(wl.batch[n_lo:n_hi] - lo).contiguous(),
                    instr=wl.instr[:, lo:hi].contiguous(), glf=wl.glf[lo:hi].contiguous(), num_graphs=hi - lo,
                    max_nodes=int(npg[lo:hi].max()) if hi > lo else 0,
                    max_edges=int(epg[lo:hi].max()) if hi > lo else 0)


def _shard_full_workload(wl: FullWorkload, rank: int, world: int, balance: bool) -> FullWorkload:
    B = wl.questions.size(0)
    if wl.added_sym_edge.numel() != B:
        raise ValueError("shard_workload: a FullWorkload is cut by graph only where it holds one added_sym_edge entry per graph")
    npg = torch.bincount(wl.batch, minlength=B)
    eg = wl.batch[wl.edge_index[1]]
    epg = torch.bincount(eg, minlength=B)
    lo, hi = graph_ranges(npg.cpu(), epg.cpu(), world, balance)[rank]
    ptr = torch.zeros(B + 1, dtype=torch.long, device=wl.batch.device)
    ptr[1:] = npg.cumsum(0)
    n_lo, n_hi = int(ptr[lo]), int(ptr[hi])
    emask = (eg >= lo) & (eg < hi)
    return FullWorkload(x=wl.x[n_lo:n_hi].contiguous(), edge_index=(wl.edge_index[:, emask] - n_lo).contiguous(),
                        edge_attr=wl.edge_attr[emask].contiguous(), batch=(wl.batch[n_lo:n_hi] - lo).contiguous(),
                        x_bbox=wl.x_bbox[n_lo:n_hi].contiguous(), added_sym_edge=wl.added_sym_edge[lo:hi].contiguous(),
                        questions=wl.questions[lo:hi].contiguous(), att_mask=wl.att_mask[lo:hi].contiguous(),
                        max_nodes=int(npg[lo:hi].max()) if hi > lo else 0, max_edges=int(epg[lo:hi].max()) if hi > lo else 0,
                        graph_sizes=torch.stack([npg[lo:hi], epg[lo:hi]]).cpu())


def all_gather_logits(logits: Tensor, out: Optional[Tensor] = None, group=None, async_op: bool = False):
    """[B_local, A] on every rank -> [world*B_local, A] (equal shard sizes) via all_gather_into_tensor.

    async_op=True returns (out, work): the collective runs on the communicator's own stream behind the producer of
    `logits`, so the next batch's kernels overlap it; call work.wait() before reading `out` or reusing either buffer
    (keep `logits` referenced until then)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return (logits, None) if async_op else logits
    world = dist.get_world_size(group)
    if out is None:
        out = torch.empty((world * logits.size(0),) + tuple(logits.shape[1:]), dtype=logits.dtype,
                          device=logits.device)
    work = dist.all_gather_into_tensor(out, logits.contiguous(), group=group, async_op=async_op)
    return (out, work) if async_op else out


def all_gather_logits_ragged(logits: Tensor, group=None) -> Tensor:
    """Unequal shard sizes (balanced partitions): gather sizes, pad to the maximum, gather, trim."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return logits
    world = dist.get_world_size(group)
    n = torch.tensor([logits.size(0)], dtype=torch.long, device=logits.device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(s) for s in sizes]
    m = max(sizes)
    pad = torch.zeros((m,) + tuple(logits.shape[1:]), dtype=logits.dtype, device=logits.device)
    pad[: logits.size(0)] = logits
    out = torch.empty((world * m,) + tuple(logits.shape[1:]), dtype=logits.dtype, device=logits.device)
    dist.all_gather_into_tensor(out, pad, group=group)
    return torch.cat([out[r * m: r * m + sizes[r]] for r in range(world)])


class GatherPipeline:
    """The per-step collective of the N > 1 path with up to `depth` all-gathers in flight (option 2): step i's
    gather runs on the communicator's stream into buffer i % (depth + 1) while the following steps' kernels run, so a
    collective up to `depth` steps long (a ring over per-link-bound xGMI) stays hidden.  `what` = "logits": BASELINE
    north_star's collective, fp32 [B_local, A] per rank (main.py:72-94 is the reference's DDP shape); "answers": the arg-max
    answers [B_local] i64 only (what the reference's evaluation reduces, utils/misc.py:40-48) -- opt-in.

    ragged=True (BASELINE configs[4]: partitions balanced by sum(nodes + edges) hold different graph counts): the ranks' row
    counts are exchanged ONCE, here; every step then gathers rows padded to the largest count (a padded staging buffer per
    in-flight slot, its pad rows zero) and `rows(buf)` trims the result.  force_collective=True issues the collective on a
    one-rank group too (tests/test_gpu_rccl_single_rank.py: this class against RCCL on one MI355X)."""

    def __init__(self, b_local: int, answers: int, device, what: str = "logits", depth: int = 2, group=None,
                 ragged: bool = False, force_collective: bool = False):
        import torch.distributed as dist
        if what not in ("logits", "answers"):
            raise ValueError(f"GatherPipeline: what = {what!r}")
        self.what, self.depth, self.group = what, max(1, int(depth)), group
        up = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if up else 1
        self.active = self.world > 1 or (bool(force_collective) and up)
        self.b_local, self.answers, self.ragged = int(b_local), int(answers), bool(ragged)
        self.sizes = [self.b_local] * self.world
        if self.ragged and self.active:
            n = torch.tensor([self.b_local], dtype=torch.long, device=device)
            got = [torch.zeros_like(n) for _ in range(self.world)]
            dist.all_gather(got, n, group=group)
            self.sizes = [int(v) for v in got]
        elif self.active and self.world > 1:          # equal shards are the caller's promise: hold it to that, once
            n = torch.tensor([self.b_local], dtype=torch.long, device=device)
            lo, hi = n.clone(), n.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
            if int(lo) != int(hi):
                raise ValueError(f"GatherPipeline: shards of {int(lo)}..{int(hi)} rows need ragged=True")
        self.b_max = max(self.sizes)
        shape = (self.world * self.b_max, self.answers) if what == "logits" else (self.world * self.b_max,)
        dtype = torch.float32 if what == "logits" else torch.int64
        self.buffers = [torch.empty(shape, dtype=dtype, device=device) for _ in range(self.depth + 1)] if self.active else []
        self.stage = ([torch.zeros(shape[:0] + (self.b_max,) + shape[1:], dtype=dtype, device=device) for _ in range(self.depth + 1)]
                      if self.active and self.b_local < self.b_max else [])
        self.pending = []          # (work, input kept alive), oldest first

    def drain(self, keep: int = 0) -> None:
        while len(self.pending) > keep:
            work, _keep = self.pending.pop(0)
            work.wait()

    def submit(self, i: int, logits: Tensor) -> Tensor:
        """Queue step i's gather behind the producer of `logits`; returns the buffer it lands in (valid after drain())."""
        if not self.active:
            return logits
        if logits.size(0) != self.b_local:
            raise ValueError(f"GatherPipeline.submit: {logits.size(0)} rows, built for {self.b_local}")
        self.drain(self.depth - 1)     # the oldest gather's buffer (and staging slot) is free again, its input may be released
        src = logits if self.what == "logits" else logits.argmax(dim=1)
        if self.stage:
            st = self.stage[i % (self.depth + 1)]
            st[: self.b_local].copy_(src)          # on the producer's stream; rows beyond b_local stay zero
            src = st
        import torch.distributed as dist
        out = self.buffers[i % (self.depth + 1)]
        work = dist.all_gather_into_tensor(out, src.contiguous(), group=self.group, async_op=True)
        self.pending.append((work, src))
        return out

    def rows(self, buf: Tensor) -> List[Tensor]:
        """The ranks' rows of a gathered buffer (views; rank r's padding trimmed)."""
        if not self.active:
            return [buf]
        return [buf[r * self.b_max: r * self.b_max + self.sizes[r]] for r in range(self.world)]

    def describe(self) -> dict:
        row = self.answers * 4 if self.what == "logits" else 8
        per = self.b_max * row
        d = {"collective": f"all_gather_into_tensor(logits[B_local,{self.answers}] f32)" if self.what == "logits"
             else "all_gather_into_tensor(answers[B_local] i64)",
             "bytes_per_rank": per, "bytes_received_per_rank": (self.world - 1) * per, "in_flight": self.depth}
        if self.ragged:
            d.update(ragged=True, rows_per_rank=list(self.sizes), padded_rows=self.b_max,
                     payload_bytes_per_rank=[n * row for n in self.sizes])
        return d


# ---- data-parallel training: one flat gradient bucket ----------------------------------------------------------------------------
# launches and sends since import: tests and tools/time_train_ddp.py count them
LAUNCHES = {"pack": 0, "reduce": 0, "src_copies": 0}


def bucket_layout(numels: Sequence[int], align: int = 64) -> Tuple[List[int], int]:
    """(offsets, total) of the slots of tensors of `numels` elements in one flat buffer, in elements: every slot starts on a
    multiple of `align` (64 fp32 = 256 B: a slot and a gradient that torch allocated share their offset from a 16-byte boundary,
    so the pack, the norm and Adam take their float4 bodies), slots follow one another in order and never overlap; `total` is the
    end of the last slot rounded up to `align`.  An empty tensor owns an empty slot at the next slot's offset."""
    if align < 1:
        raise ValueError(f"bucket_layout: align = {align}")
    offsets, off = [], 0
    for n in numels:
        n = int(n)
        if n < 0:
            raise ValueError(f"bucket_layout: numel {n}")
        offsets.append(off)
        off += (n + align - 1) // align * align
    return offsets, off


def union_mask(mask: Sequence[bool], group=None, device=None) -> List[bool]:
    """The element-wise OR of every rank's `mask` over `group`: ONE all-gather of the T flags (uint8, on `device`: the GPU for an
    nccl group, the host for gloo) and one copy to the host.  Without an initialised process group the mask comes back as it is."""
    import torch.distributed as dist
    mask = [bool(m) for m in mask]
    if not (dist.is_available() and dist.is_initialized()):
        return mask
    world = dist.get_world_size(group)
    mine = torch.tensor(mask, dtype=torch.uint8, device=device)
    if mine.numel() == 0:
        return mask
    out = torch.empty(world * mine.numel(), dtype=torch.uint8, device=mine.device)
    dist.all_gather_into_tensor(out, mine, group=group)
    return [bool(v) for v in out.view(world, -1).amax(dim=0).cpu().tolist()]


def _named(params) -> List[Tuple[str, Tensor]]:
    out = []
    for i, item in enumerate(params):
        if isinstance(item, tuple):
            name, p = item
            out.append((f"parameter '{name}'", p))
        else:
            out.append((f"parameter {i} (shape {tuple(item.shape)})", item))
    return out


class GradSync:
    """The gradients of `params` (an iterable of parameters, or of (name, parameter) as named_parameters() gives them), averaged
    over the ranks of `group` in one flat fp32 bucket.

      sync = GradSync(model.named_parameters())
      opt = optim.Adam(model.parameters(), ..., grad_sync=sync)
      loss.backward(); sync.pack(); sync.reduce(); opt.step()            # train.train_step(..., sync=sync) does this

    pack() launches isg_mt_pack once: slot = grad / world (times `scale`; `accumulate=True` adds into the slot with one fmaf, for
    micro-batches).  reduce() is ONE all-reduce (SUM) of the whole bucket, ordered behind the pack on the current stream:
    torch.distributed.all_reduce(bucket, group=group), or `all_reduce(bucket)` -- the hook for another transport, a callable that
    sums a tensor in place over the ranks.  The optimizer then reads the reduced gradients where they lie (grad_ptr); nothing is
    unpacked, p.grad keeps the local gradient.  Neither call reads a device value on the host.

    The parameter set is fixed at the first pack(): the union over the ranks of the parameters that have a gradient there (one
    all-gather of a T-bit mask; with an `all_reduce` hook the mask goes through the hook once, as a [T] fp32 tensor on the
    parameters' device, and is read back once).  From then on a member whose local grad is None packs zeros and is still stepped
    with the other ranks' average -- DistributedDataParallel(find_unused_parameters=True) -- and a parameter outside the set that
    receives a gradient raises an error that names it.  Slots start on multiples of 64 elements; the padding between them is
    zeroed once, stays zero under a sum and adds nothing to a norm taken over the slots.

    `world` defaults to the group's size (1 without a process group), `rank` to the group's rank (0).  With world 1 and
    force=False the sync is inactive: pack() and reduce() return at once and the optimizer reads p.grad as it does without one.
    The all-reduce is not overlapped with the backward and nothing here is captured into a hipGraph."""

    def __init__(self, params, group=None, world: Optional[int] = None, all_reduce: Optional[Callable[[Tensor], None]] = None,
                 force: bool = False, rank: Optional[int] = None):
        import torch.distributed as dist
        from . import optim
        self.named = _named(params)
        if not self.named:
            raise ValueError("GradSync: no parameters")
        self.params = [p for _, p in self.named]
        self.group, self.all_reduce = group, all_reduce
        up = dist.is_available() and dist.is_initialized()
        self.world = int(world) if world is not None else (dist.get_world_size(group) if up else 1)
        self.rank = int(rank) if rank is not None else (dist.get_rank(group) if up else 0)
        if self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError(f"GradSync: rank {self.rank} of world {self.world}")
        self.active = self.world > 1 or bool(force)
        self.device = self.params[0].device
        for name, p in self.named:
            optim._check_param(p, f"GradSync: {name}")
            if p.device != self.device:
                raise ValueError(f"GradSync: {name} lives on {p.device}, the first parameter on {self.device}; one bucket, one device")
        self._index = {id(p): i for i, p in enumerate(self.params)}
        if len(self._index) != len(self.params):
            raise ValueError("GradSync: a parameter is listed twice")
        self.bucket: Optional[Tensor] = None
        self.members: Optional[List[int]] = None          # indices into params of the set, fixed at the first pack()
        self._slot = {}                                   # id(param) -> (offset, numel)
        self._table: Optional[Tensor] = None              # device int64 [4 T + 1]: src | dst | numel | chunk_prefix
        self._src_key = None
        self._chunks = 0

    # ---- the set and the bucket -----------------------------------------------------------------------------------------------
    def _agree(self, mask: List[bool]) -> List[bool]:
        if self.all_reduce is not None:
            t = torch.tensor([1.0 if m else 0.0 for m in mask], dtype=torch.float32).to(self.device)
            self.all_reduce(t)
            return [v > 0.0 for v in t.cpu().tolist()]
        return union_mask(mask, self.group, self.device) if self.world > 1 else mask

    def _fix_set(self) -> None:
        from . import _lib_optim, optim
        mask = self._agree([p.grad is not None for p in self.params])
        self.members = [i for i, m in enumerate(mask) if m]
        numels = [self.params[i].numel() for i in self.members]
        offsets, total = bucket_layout(numels)
        self.bucket = torch.zeros(total, dtype=torch.float32, device=self.device)       # the padding is zeroed here, once
        assert self.bucket.data_ptr() % 16 == 0
        self._slot = {id(self.params[i]): (o, n) for i, o, n in zip(self.members, offsets, numels)}
        prefix = optim.chunk_prefix(numels, int(_lib_optim.load().isg_mt_chunk_elems()))
        self._chunks = prefix[-1]
        T, base = len(numels), self.bucket.data_ptr()
        self._table = torch.zeros(4 * T + 1, dtype=torch.int64, device=self.device)
        fixed = [base + 4 * o for o in offsets] + numels + prefix
        self._send(self._table[T:], fixed)

    def _send(self, dst: Tensor, values: List[int]) -> None:
        host = torch.tensor(values, dtype=torch.int64)
        if self.device.type == "cuda":
            host = host.pin_memory()                      # fresh per send: never rewritten under a pending copy
        dst.copy_(host, non_blocking=True)

    def _sources(self) -> List[int]:
        src = []
        for i, (name, p) in enumerate(self.named):
            g = p.grad
            if id(p) not in self._slot:
                if g is not None:
                    raise RuntimeError(f"GradSync: {name} received a gradient but had none on any rank at the first pack(); the "
                                       "set of synchronised parameters is fixed there")
                continue
            if g is None:
                src.append(0)                             # unused on this rank in this step: zeros
                continue
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device:
                raise ValueError(f"GradSync: the gradient of {name} is not a dense contiguous fp32 tensor on the parameter's device")
            src.append(g.data_ptr())
        return src

    # ---- the step -------------------------------------------------------------------------------------------------------------
    def pack(self, accumulate: bool = False, scale: float = 1.0) -> None:
        """bucket slot = (scale / world) * grad, or += with accumulate=True (train_step's micro-batches pass scale = 1 /
        accumulate).  One launch; the source addresses are sent only when one changed since the last pack."""
        if not self.active:
            return
        from . import _lib, _lib_dist, ops
        if self.members is None:
            self._fix_set()
        src = self._sources()
        T = len(src)
        if T == 0:
            return
        key = tuple(src)
        if key != self._src_key:
            self._send(self._table[:T], src)
            self._src_key = key
            LAUNCHES["src_copies"] += 1
        base = self._table.data_ptr()
        _lib.check(_lib_dist.load().isg_mt_pack(base, base + 8 * T, base + 16 * T, base + 24 * T, T, self._chunks,
                                                float(scale) / self.world, int(bool(accumulate)), ops._stream()), "isg_mt_pack")
        LAUNCHES["pack"] += 1

    def reduce(self) -> None:
        """One all-reduce (SUM) of the whole bucket, behind the pack in the current stream's order."""
        if not self.active:
            return
        if self.bucket is None:
            raise RuntimeError("GradSync.reduce: nothing was packed yet")
        if self.bucket.numel() == 0:
            return
        if self.all_reduce is not None:
            self.all_reduce(self.bucket)
        else:
            import torch.distributed as dist
            dist.all_reduce(self.bucket, group=self.group)
        LAUNCHES["reduce"] += 1

    def has(self, p: Tensor) -> bool:
        """Whether p belongs to the synchronised set (known after the first pack())."""
        if self.members is None:
            raise RuntimeError("GradSync: the parameter set is fixed by the first pack()")
        return id(p) in self._slot

    def knows(self, p: Tensor) -> bool:
        return id(p) in self._index

    def grad(self, p: Tensor) -> Tensor:
        """The averaged gradient of p after reduce(): a view of its slot, in p's shape."""
        if not self.has(p):
            raise KeyError("GradSync.grad: the parameter is not in the synchronised set")
        o, n = self._slot[id(p)]
        return self.bucket[o:o + n].view(p.shape)

    def grad_ptr(self, p: Tensor) -> int:
        if not self.has(p):
            raise KeyError("GradSync.grad_ptr: the parameter is not in the synchronised set")
        return self.bucket.data_ptr() + 4 * self._slot[id(p)][0]

    # ---- the replicas ---------------------------------------------------------------------------------------------------------
    def broadcast_params(self, src: int = 0) -> None:
        """Every parameter takes rank `src`'s values (a global rank, as torch.distributed.broadcast counts): the start of training,
        as DistributedDataParallel's constructor does."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            if self.world == 1:
                return
            raise RuntimeError("GradSync.broadcast_params needs an initialised process group")
        with torch.no_grad():
            for p in self.params:
                dist.broadcast(p.data, src=src, group=self.group)

    def params_in_sync(self) -> Tensor:
        """A device flag (uint8 0-dim, 1 = in sync) and no host read: every rank sums its parameters and their squares in float64,
        the two checksums are all-reduced with MAX and with MIN, and the flag is set where both differences are exactly 0."""
        import torch.distributed as dist
        with torch.no_grad():
            sums = torch.stack([torch.stack([p.sum(dtype=torch.float64), (p.double() * p).sum()]) if p.numel() else
                                torch.zeros(2, dtype=torch.float64, device=self.device) for p in self.params]).sum(dim=0)
            if not (dist.is_available() and dist.is_initialized()):
                if self.world == 1:
                    return torch.ones((), dtype=torch.uint8, device=self.device)
                raise RuntimeError("GradSync.params_in_sync needs an initialised process group")
            hi, lo = sums.clone(), sums.clone()
            dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
            return ((hi - lo) == 0).all().to(torch.uint8)
