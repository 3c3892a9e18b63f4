"""The semantics of isg_subgraph_cut restated with plain torch ops on the CPU: flags, cumsum, nonzero, bincount.  Every result is
an integer, so the GPU tests compare with it exactly.  Not a test module: tests/test_subgraph_cpu.py checks it against a known
answer written out by hand, tests/test_gpu_subgraph.py checks the kernel against it."""
from typing import NamedTuple

import torch


class Restated(NamedTuple):
    node_new: torch.Tensor       # int32 [N]
    edge_new: torch.Tensor       # int32 [E]
    node_id: torch.Tensor        # int64 [N']
    edge_id: torch.Tensor        # int64 [E']
    edge_index: torch.Tensor     # int64 [2, E']
    batch: torch.Tensor          # int64 [N']
    ptr: torch.Tensor            # int32 [B + 1]
    sel: torch.Tensor            # int32 [B, table_k]
    counts: tuple                # (N', E')


def ptr_of(batch: torch.Tensor, B: int) -> torch.Tensor:
    """int64 [B + 1] node range per graph of a sorted batch vector."""
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = torch.bincount(batch, minlength=B).cumsum(0)
    return ptr


def restate(node_mask, edge_index, batch, B, threshold=0.0, complement=False, table_k=0) -> Restated:
    mask = node_mask.detach().cpu().reshape(-1).float()
    ei, batch = edge_index.cpu().long(), batch.cpu().long()
    N, E = mask.numel(), ei.size(1)
    keep = (mask > threshold) != bool(complement)                      # a NaN compares false
    node_new = torch.where(keep, keep.long().cumsum(0) - 1, torch.full((N,), -1)).to(torch.int32)
    node_id = torch.nonzero(keep).reshape(-1)
    s, d = ei[0], ei[1]
    inside = (s >= 0) & (s < N) & (d >= 0) & (d < N)
    ekeep = inside.clone()
    if N > 0:
        ekeep = inside & keep[s.clamp(0, N - 1)] & keep[d.clamp(0, N - 1)]
    edge_new = torch.where(ekeep, ekeep.long().cumsum(0) - 1, torch.full((E,), -1)).to(torch.int32)
    edge_id = torch.nonzero(ekeep).reshape(-1)
    sub_ei = node_new.long()[ei[:, edge_id]].reshape(2, -1)
    sub_batch = batch[node_id]
    ptr = ptr_of(batch, B)
    excl = torch.zeros(N + 1, dtype=torch.int64)
    excl[1:] = keep.long().cumsum(0)
    sub_ptr = excl[ptr].to(torch.int32)
    sel = torch.full((B, table_k), -1, dtype=torch.int32)
    if table_k > 0 and node_id.numel() > 0:
        j = torch.arange(node_id.numel()) - sub_ptr.long()[sub_batch]      # place among the graph's kept nodes
        first = j < table_k
        sel[sub_batch[first], j[first]] = (node_id - ptr[sub_batch])[first].to(torch.int32)
    return Restated(node_new, edge_new, node_id, edge_id, sub_ei, sub_batch, sub_ptr, sel, (int(keep.sum()), int(ekeep.sum())))
