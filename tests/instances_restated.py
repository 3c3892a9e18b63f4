"""The semantics of isg_instances_size / isg_instances_fill (include/isg_instances.h) restated as a plain loop over the questions,
in torch on the CPU: the checker of tests/test_instances_cpu.py and tests/test_gpu_instances.py.  Instance q is a copy of graph
index[q]: its nodes in order, its edges in their original order, renumbered; an index outside [0, G) makes an empty instance."""
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


def graph_ptr(batch, G):
    """int64 [G + 1]: node range of every graph of a sorted batch vector."""
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(batch, minlength=G).cumsum(0)])


def edge_ranges(batch, edge_index, G):
    """([G + 1] edge range of every graph, bad_grouping) of an edge list whose graphs are contiguous and in order."""
    E = edge_index.size(1)
    g = batch[edge_index[1]] if E else torch.zeros(0, dtype=torch.int64)
    bad = bool(E) and (bool((g[1:] < g[:-1]).any()) or bool((batch[edge_index[0]] != g).any()))
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(g, minlength=G).cumsum(0)]), int(bad)


def expand(batch, edge_index, index, G) -> Restated:
    """batch int64 [N] (sorted), edge_index int64 [2, E] (grouped by graph), index [Q] -> the instance batch.  For a grouped edge
    list only: bad_grouping is reported, the outputs are then not what the kernels leave."""
    nptr = graph_ptr(batch, G)
    eptr, bad_grouping = edge_ranges(batch, edge_index, G)
    ptr, eptr_out, b, ei, ns, es = [0], [0], [], [], [], []
    bad_index = 0
    for q, g in enumerate(int(v) for v in index.tolist()):
        if 0 <= g < G:
            n0, n1, e0, e1 = int(nptr[g]), int(nptr[g + 1]), int(eptr[g]), int(eptr[g + 1])
            b += [q] * (n1 - n0)
            ns += list(range(n0, n1))
            es += list(range(e0, e1))
            ei.append(edge_index[:, e0:e1] - n0 + ptr[-1])
            ptr.append(ptr[-1] + n1 - n0)
            eptr_out.append(eptr_out[-1] + e1 - e0)
        else:
            bad_index = 1
            ptr.append(ptr[-1])
            eptr_out.append(eptr_out[-1])
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)
    return Restated(torch.tensor(ptr, dtype=torch.int32), torch.tensor(eptr_out, dtype=torch.int32), i64(b),
                    torch.cat(ei, 1) if ei else torch.zeros(2, 0, dtype=torch.int64), i64(ns), i64(es),
                    torch.tensor([ptr[-1], eptr_out[-1], bad_index, bad_grouping], dtype=torch.int32))
