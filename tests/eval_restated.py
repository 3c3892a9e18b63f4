"""The semantics of include/isg_eval.h restated with torch in float64 and plain loops.  Not a test module: tests/test_eval_cpu.py
holds it to cases written out by hand, tests/test_gpu_eval.py holds the kernels to it.  The grouped co-occurrence fold applies
tests/token_coo_restated.py's add_totals to the questions of every group."""
import math

import torch

from token_coo_restated import TOTALS, add_totals

SLOTS = 8


def restate_rank(logits, labels, ignore_index=-100):
    """int32 [B]: the classes that beat the label (a tie goes to the lower index); -1 ignored; A for a bad label or a NaN row."""
    x = torch.as_tensor(logits).double()
    B, A = x.shape
    out = []
    for b, l in enumerate(torch.as_tensor(labels).tolist()):
        if l == ignore_index:
            out.append(-1)
        elif not 0 <= l < A or bool(torch.isnan(x[b]).any()):
            out.append(A)
        else:
            idx = torch.arange(A)
            out.append(int(((x[b] > x[b, l]) | ((x[b] == x[b, l]) & (idx < l))).sum()))
    return torch.tensor(out, dtype=torch.int32)


def restate_top(logits, K, lse=None):
    """(ids int64 [B, K], prob float64 [B, K] or None): the K best classes, value descending and index ascending among equals;
    id -1 / prob 0 beyond A and on a NaN row.  prob = exp(x - lse) in float64, a NaN where that is one (inf - inf)."""
    x = torch.as_tensor(logits).double()
    B, A = x.shape
    ids = torch.full((B, K), -1, dtype=torch.int64)
    prob = None if lse is None else torch.zeros(B, K, dtype=torch.float64)
    for b in range(B):
        if bool(torch.isnan(x[b]).any()):
            continue
        row = x[b].tolist()
        order = sorted(range(A), key=lambda a: (-row[a], a))[:K]        # -inf sorts last, +inf first; equal values by index
        for r, a in enumerate(order):
            ids[b, r] = a
            if prob is not None:
                d = row[a] - float(lse[b])
                prob[b, r] = math.exp(d) if d == d and d != math.inf else (math.nan if d != d else math.inf)
    return ids, prob


def add_group_meters(totals, row_loss, rank, groups, G, k):
    """`totals` (float64 [G, 8] or None for zeros) with a batch added: a new tensor.  Loss sums in float64 over the rows ascending."""
    t = torch.zeros(G, SLOTS, dtype=torch.float64) if totals is None else torch.as_tensor(totals).double().clone()
    loss, rank = torch.as_tensor(row_loss).float().tolist(), torch.as_tensor(rank).tolist()
    for b, ids in enumerate(torch.as_tensor(groups).tolist()):
        if rank[b] < 0:
            continue
        for g in ids:
            if not 0 <= g < G:
                continue                                   # -1: none; anything else outside [0, G): a bad id, skipped
            t[g, 0] += 1
            if math.isfinite(loss[b]):
                t[g, 1] += loss[b]
            else:
                t[g, 2] += 1
            t[g, 3] += int(rank[b] == 0)
            t[g, 4] += int(rank[b] < k)
    return t


def bad_ids(groups, G):
    """(bad ids, first bad row or None) of a batch."""
    bad = [(b, g) for b, ids in enumerate(torch.as_tensor(groups).tolist()) for g in ids if g < -1 or g >= G]
    return len(bad), (bad[0][0] if bad else None)


def add_coo_groups(totals, table, qflags, groups, G):
    """`totals` (a list of G lists of TOTALS ints, or None for zeros) with a batch added: add_totals over the questions of every
    group alone, a question as often as its facets name the group."""
    table = torch.as_tensor(table)
    groups = torch.as_tensor(groups).tolist()
    out = []
    for g in range(G):
        rows = [b for b, ids in enumerate(groups) for i in ids if i == g]
        sub = table[rows].view(len(rows), 8)
        flags = None if qflags is None else [int(qflags[b]) for b in rows]
        out.append(add_totals(None if totals is None else totals[g], sub, flags))
    assert all(len(r) == TOTALS for r in out)
    return out
