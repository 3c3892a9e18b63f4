"""The semantics of isg_induced_size / isg_induced_fill (include/ext/isg_induced.h) restated as a plain loop over the instances,
in torch and Python integers on the CPU: the checker of tests/test_induced_cpu.py and tests/test_gpu_induced.py.  Not a test
module.  Instance q is graph index[q] minus the nodes its row of keep bits leaves out: the kept nodes in order, the edges with
both ends kept in their original order, renumbered; an index outside [0, G) makes an empty instance."""
from typing import NamedTuple

import torch


class Restated(NamedTuple):
    ptr: torch.Tensor          # int32 [Q + 1]
    eptr: torch.Tensor         # int32 [Q + 1]
    batch: torch.Tensor        # int64 [N']
    edge_index: torch.Tensor   # int64 [2, E']
    node_src: torch.Tensor     # int64 [N']
    edge_src: torch.Tensor     # int64 [E']
    status: torch.Tensor       # int32 [4] = (N', E', bad_index, bad_grouping)


def bit(keep_row, i: int) -> bool:
    """Bit i of a row of 32-bit words (a list of Python ints, taken modulo 2^32); False beyond the row."""
    w = i >> 5
    return w < len(keep_row) and bool(((keep_row[w] & 0xFFFFFFFF) >> (i & 31)) & 1)


def pack(flags, W: int) -> torch.Tensor:
    """A list of rows of booleans -> int32 [Q, W] words (bit i & 31 of word i >> 5); flags beyond 32 W are dropped."""
    out = torch.zeros(len(flags), W, dtype=torch.int64)
    for q, row in enumerate(flags):
        for i, f in enumerate(row):
            if f and i < 32 * W:
                out[q, i >> 5] |= 1 << (i & 31)
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


def induce(batch, edge_index, index, keep, G) -> Restated:
    """batch int64 [N] (sorted), edge_index int64 [2, E] (grouped by graph, in graph order), index [Q], keep int32 [Q, W] or None
    -> the instance batch.  For a grouped edge list only: bad_grouping is reported, the outputs are then not the kernels'."""
    N, E = batch.numel(), edge_index.size(1)
    nptr = [0] * (G + 1)
    for g in batch.tolist():
        nptr[g + 1] += 1
    for g in range(G):
        nptr[g + 1] += nptr[g]
    eg = [int(batch[edge_index[1, e]]) for e in range(E)]
    bad_grouping = int(any(eg[e] < eg[e - 1] for e in range(1, E)) or
                       any(int(batch[edge_index[0, e]]) != eg[e] for e in range(E)))
    edges_of = [[e for e in range(E) if eg[e] == g] for g in range(G)]
    rows = None if keep is None else [[int(v) for v in r] for r in keep.tolist()]
    ptr, eptr, b, src, dst, ns, es = [0], [0], [], [], [], [], []
    bad_index = 0
    for q, g in enumerate(int(v) for v in index.tolist()):
        if not 0 <= g < G:
            bad_index = 1
            ptr.append(ptr[-1])
            eptr.append(eptr[-1])
            continue
        n0, n_g = nptr[g], nptr[g + 1] - nptr[g]
        kept = [i for i in range(n_g) if rows is None or bit(rows[q], i)]
        rank = {i: r for r, i in enumerate(kept)}
        b += [q] * len(kept)
        ns += [n0 + i for i in kept]
        m = 0
        for e in edges_of[g]:
            s, d = int(edge_index[0, e]) - n0, int(edge_index[1, e]) - n0
            if s in rank and d in rank:
                es.append(e)
                src.append(ptr[-1] + rank[s])
                dst.append(ptr[-1] + rank[d])
                m += 1
        ptr.append(ptr[-1] + len(kept))
        eptr.append(eptr[-1] + m)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    return Restated(torch.tensor(ptr, dtype=torch.int32), torch.tensor(eptr, dtype=torch.int32), i64(b),
                    torch.stack([i64(src), i64(dst)]), i64(ns), i64(es),
                    torch.tensor([ptr[-1], eptr[-1], bad_index, bad_grouping], dtype=torch.int32))


def node_flags(keep, index, sizes):
    """bool rows: flags[q][i] for i < n of graph index[q] -- the bits as a list per instance (an index out of range: no nodes)."""
    rows = None if keep is None else [[int(v) for v in r] for r in keep.tolist()]
    out = []
    for q, g in enumerate(int(v) for v in index.tolist()):
        n = sizes[g] if 0 <= g < len(sizes) else 0
        out.append([rows is None or bit(rows[q], i) for i in range(n)])
    return out
