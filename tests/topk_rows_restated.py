"""The per-graph node budget and the samplers with a k per row (include/isg_topk_rows.h), restated in torch on the
CPU: what the kernels compute, written before any kernel.  Rows are dense, padded with 0.0 (the pads take part in the selection,
quirk Q1), and every row carries a loop count of its own."""
import torch

F32_TINY = torch.finfo(torch.float32).tiny


def budget(n, ratio, k_min, k_cap):
    """k_rows int32 [B] = min(k_cap, max(k_min, ceil(ratio * n))) with the product as ONE fp32 multiplication: the formula of the
    reference's comment (masking.py:113), clamped."""
    n = torch.as_tensor(n)
    c = torch.ceil(torch.tensor(ratio, dtype=torch.float32) * n.float())
    return c.clamp(min=float(k_min), max=float(k_cap)).to(torch.int32)


def dense_rows(rows, nmax):
    """[B, nmax] fp32: every row's values first, then 0.0."""
    out = torch.zeros(len(rows), nmax, dtype=torch.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.as_tensor(r, dtype=torch.float32)
    return out


def threshold_rows(dense, k_rows, k_cap):
    """Row b: 1.0 where dense[b] >= its k-th largest value, k = clamp(k_rows[b], 0, k_cap); all ones where k >= nmax.  The k-th
    largest is found as the kernel finds it: k rounds of `largest value not yet taken`, duplicates taken one at a time."""
    B, nmax = dense.shape
    out = torch.zeros_like(dense)
    for b in range(B):
        k = min(max(int(k_rows[b]), 0), k_cap)
        if k >= nmax:
            out[b] = 1.0
            continue
        taken = torch.zeros(nmax, dtype=torch.bool)
        thresh = float("-inf")
        for _ in range(k):
            v = dense[b].masked_fill(taken, float("-inf"))
            thresh = v.max().item()
            taken[int(torch.nonzero(v == thresh)[0])] = True
        out[b] = (dense[b] >= thresh).float()
    return out


def gumbel_rows(dense, noise, k_rows, k_cap, tau):
    """(out, khot) [B, nmax]: row b runs min(k, nmax) rounds of the relaxation (gumbel_scheme.py:70-81) and takes the hard top-k of
    khot with that k (ties towards the lower index), k = clamp(k_rows[b], 0, k_cap)."""
    B, nmax = dense.shape
    k = torch.as_tensor(k_rows).long().clamp(0, k_cap).clamp(max=nmax)          # every row's loop count
    flat = dense + noise
    khot, onehot = torch.zeros_like(flat), torch.zeros_like(flat)
    for it in range(int(k.max()) if B else 0):
        live = (it < k)[:, None]                                                # the rows still in their loop
        step = flat + torch.log(torch.max(1.0 - onehot, torch.tensor([F32_TINY])))
        flat = torch.where(live, step, flat)
        onehot = torch.where(live, torch.softmax(flat / tau, dim=1), onehot)
        khot = torch.where(live, khot + onehot, khot)
    hard = torch.zeros_like(khot)
    for b in range(B):
        if int(k[b]):
            hard[b, torch.topk(khot[b], int(k[b])).indices] = 1.0
    return hard - khot + khot, khot
