"""Graphs, indices and keep bits shared by tests/test_induced_cpu.py and tests/test_gpu_induced.py, and the CHAIN of the two
existing restatements (tests/instances_restated.py's expansion, a mask made from the bits, tests/subgraph_restated.py's cut) that
the induced-instance operator replaces.  Not a test module; both restatements are imported read-only."""
import torch

import induced_restated as IR
import instances_restated as R
import subgraph_restated as S

NODE_SIZES = (0, 1, 2, 31, 32, 33, 64, 65, 130)      # the word boundary (32) and the lane boundary (64 nodes = 2 words; 65)
EDGE_COUNTS = (0, 63, 64, 65, 129)                   # the ballot-chunk boundaries
LOOPS = (2, [(0, 0), (0, 1), (0, 1), (1, 1), (1, 0), (0, 1)])      # self loops and parallel edges, written out
BITS = ("all", "none", "zero", "loo", "alternating", "random", "beyond")


def make_graphs(spec, seed):
    """spec: per graph (nodes, edges) or (nodes, [(src, dst) local pairs]) -> (batch int64 [N], edge_index int64 [2, E], sizes);
    a graph's edges are random pairs of its own nodes (so self loops and parallel edges occur) and contiguous, graphs in order."""
    gen = torch.Generator().manual_seed(seed)
    batch, src, dst, lo = [], [], [], 0
    for g, (n, e) in enumerate(spec):
        batch += [g] * n
        if isinstance(e, list):
            src.append(lo + torch.tensor([p[0] for p in e], dtype=torch.int64))
            dst.append(lo + torch.tensor([p[1] for p in e], dtype=torch.int64))
        elif e:
            assert n > 0
            src.append(lo + torch.randint(0, n, (e,), generator=gen))
            dst.append(lo + torch.randint(0, n, (e,), generator=gen))
        lo += n
    ei = torch.stack([torch.cat(src), torch.cat(dst)]) if src else torch.zeros(2, 0, dtype=torch.int64)
    return torch.tensor(batch, dtype=torch.int64), ei, [n for n, _ in spec]


def spec_of(G, Q):
    if G == 1:
        return [(130, 129)] if Q <= 2 else [(33, 65)]
    if G == 3:
        return [(65, 64), LOOPS, (32, 0)]            # (the third: a graph without edges)
    spec = [(NODE_SIZES[g % 9], EDGE_COUNTS[(g // 2) % 5] if NODE_SIZES[g % 9] else 0) for g in range(G)]
    spec[11] = LOOPS
    assert {n for n, _ in spec} >= set(NODE_SIZES) and {e for _, e in spec if not isinstance(e, list)} >= set(EDGE_COUNTS)
    assert any(n > 0 and e == 0 for n, e in spec if not isinstance(e, list))
    return spec


def index_of(G, Q, seed):
    """Random with repeats; the largest graph is always among them."""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, G, (Q,), generator=gen)
    idx[Q // 2] = G - 1 if G != 70 else 8            # (n = 130 in the 70-graph spec)
    return idx


def words_min(sizes):
    return max(1, (max(sizes) + 31) // 32)


def bits_of(kind, index, sizes, W, seed):
    """keep int32 [Q, W] or None.  all: every word -1 (bits beyond n_g set too); none: keep is None; zero: no bit; loo: instance q
    lacks local node q mod n; alternating: even nodes; random; beyond: random below n_g, every bit at or beyond n_g set."""
    Q = index.numel()
    if kind == "none":
        return None
    if kind == "all":
        return torch.full((Q, W), -1, dtype=torch.int32)
    if kind == "zero":
        return torch.zeros(Q, W, dtype=torch.int32)
    gen = torch.Generator().manual_seed(seed)
    flags = []
    for q, g in enumerate(index.tolist()):
        n = sizes[g] if 0 <= g < len(sizes) else 0
        if kind == "loo":
            row = [i != q % max(n, 1) for i in range(n)]
        elif kind == "alternating":
            row = [i % 2 == 0 for i in range(n)]
        else:
            row = (torch.rand(n, generator=gen) < 0.6).tolist()
        if kind == "beyond":
            row += [True] * (32 * W - n)
        flags.append(row)
    return IR.pack(flags, W)


def chain(batch, edge_index, index, keep, G):
    """What the two steps give: expand every graph whole (instances_restated), build the float mask from the bits, cut
    (subgraph_restated) -> an induced_restated.Restated.  Indices must lie in [0, G)."""
    x = R.expand(batch, edge_index, index, G)
    Q = index.numel()
    local = x.node_src - R.graph_ptr(batch, G)[index.long()][x.batch]
    if keep is None:
        mask = torch.ones(x.batch.numel())
    else:
        W = keep.size(1)
        word = keep.long()[x.batch, (local >> 5).clamp(max=W - 1)] & 0xFFFFFFFF
        mask = (((word >> (local & 31)) & 1).bool() & (local < 32 * W)).float()
    c = S.restate(mask, x.edge_index, x.batch, Q)
    eptr = torch.zeros(Q + 1, dtype=torch.int64)
    if c.edge_id.numel():
        eptr[1:] = torch.bincount(c.batch[c.edge_index[1]], minlength=Q).cumsum(0)
    return IR.Restated(c.ptr, eptr.to(torch.int32), c.batch, c.edge_index, x.node_src[c.node_id], x.edge_src[c.edge_id],
                       torch.tensor([c.counts[0], c.counts[1], 0, int(x.status[3])], dtype=torch.int32))


def assert_same(got, want, what):
    for k in IR.Restated._fields:
        a, b = (got[k] if isinstance(got, dict) else getattr(got, k)).cpu(), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{what}: {k} differs"
