"""Attention dropout of the GATv2 message passing (include/isg_mp_train.h), restated in plain torch on the host.

TEST INFRASTRUCTURE ONLY.  The keep mask comes from oracle.philox.philox4x32_10 (imported, not changed): edge e (its ORIGINAL id,
the column of edge_index) and head h are kept iff
    uniform24(word[h & 3] of philox4x32_10((e, h >> 2, 0x1571, 0x9E37), (seed & 0xffffffff, seed >> 32))) >= p     (in fp32)
and a kept weight is multiplied by the fp32 value 1.0f / (1.0f - p).  message_passing() is oracle.model.gatv2_message_passing with
that factor between the softmax and the aggregation -- out_i = sum_e x_l[j] * ((alpha_e * r_e) * m_e) -- in the dtype of its
operands (float64: the reference; float32: the yardstick), differentiable by torch autograd; alpha is returned BEFORE dropout.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import philox
from oracle import primitives as P


def inv_keep(p: float) -> float:
    """1.0f / (1.0f - p) as the entry points form it: one fp32 subtraction, one fp32 division."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed: int, E: int, H: int, p: float, edge_ids=None) -> torch.Tensor:
    """bool [E, H]: row e is edge e's, or edge edge_ids[e]'s."""
    seed = int(seed) & (2 ** 64 - 1)
    e = np.arange(E, dtype=np.uint64) if edge_ids is None else np.asarray(edge_ids, dtype=np.int64).astype(np.uint64)
    keep = np.zeros((E, H), dtype=bool)
    for hq in range((H + 3) // 4):                         # one Philox block serves four heads
        words = philox.philox4x32_10((e, np.full(E, hq, dtype=np.uint64), philox.C2, philox.C3), (seed & 0xFFFFFFFF, seed >> 32))
        for w in range(4):
            h = 4 * hq + w
            if h < H:
                keep[:, h] = philox.uniform24(words[w]) >= np.float32(p)
    return torch.from_numpy(keep)


def factor(seed: int, E: int, H: int, p: float, dtype=torch.float32, edge_ids=None) -> torch.Tensor:
    """r [E, H] = keep * (1.0f / (1.0f - p)): the fp32 value, held in `dtype`."""
    return keep_mask(seed, E, H, p, edge_ids).to(dtype) * torch.tensor(inv_keep(p), dtype=dtype)


def message_passing(x_l, x_r, e_proj, att, edge_index, edge_mask, negative_slope, r):
    """x_l, x_r [N, H, C]; e_proj [E, H, C]; att [1, H, C]; edge_mask [E, 1] or None; r [E, H] (factor()) or None.
    -> (out [N, H, C], alpha [E, H] before dropout)."""
    N = x_l.size(0)
    src, dst = edge_index[0], edge_index[1]
    x_j = x_l.index_select(0, src)
    x = x_r.index_select(0, dst) + x_j
    x = x + e_proj
    if edge_mask is not None:
        x = x * edge_mask.unsqueeze(-1)
    x = F.leaky_relu(x, negative_slope)
    if edge_mask is not None:
        x = x * edge_mask.unsqueeze(-1)
    alpha = P.pyg_softmax((x * att).sum(dim=-1), dst, N)
    w = alpha if r is None else alpha * r
    if edge_mask is not None:
        w = w * edge_mask
    return P.scatter_sum(x_j * w.unsqueeze(-1), dst, N), alpha
