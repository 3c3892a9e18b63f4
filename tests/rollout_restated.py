"""Attention rollout (include/ext/isg_rollout.h) restated as a Python loop over nodes and out-slots, in float64,
with the header's rules written out: a slot whose edge id lies outside [0, E) or whose destination lies outside its source's
graph range contributes nothing; ptr and rowptr_s are clamped and made non-decreasing; a graph beyond `nmax` gets NaN rows and is
otherwise skipped.  rollout_fp32 is the same walk with every operation rounded to fp32 in the order the header states -- for
diagnostics (the kernel's bits are a function of the inputs: it should equal them), no test's reference.

Plain lists and CPU tensors in, CPU tensors out; no GPU, nothing of the package is imported."""
import numpy as np
import torch


def source_csr(edge_index, N):
    """(rowptr_s int32 [N + 1], eid_s int32 [E], dst_s int32 [E]): the out-edges of every node in edge-id order."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    order = torch.argsort(src, stable=True)
    counts = torch.bincount(src, minlength=N)[:N] if src.numel() else torch.zeros(N, dtype=torch.long)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    return rowptr.int(), order.int(), dst[order].int()


def _ranges(ptr, N):
    out = []
    for g in range(len(ptr) - 1):
        lo = max(0, min(int(ptr[g]), N))
        out.append((lo, max(lo, min(int(ptr[g + 1]), N))))
    return out


def rollout(ptr, rowptr_s, eid_s, dst_s, alphas, start, masks=None, residual=0.5, nmax=None):
    """-> (relevance float64 [N], flow float64 [L, E]).  alphas: L tensors [E, H] (any strides); masks: None or L entries, each
    None or a tensor of N values; nmax: None = no bound.  The flow of a skipped slot's edge stays 0."""
    L, N = len(alphas), len(start)
    E = int(alphas[0].shape[0])
    H = int(alphas[0].shape[1])
    ptr, rowptr_s, eid_s, dst_s = ([int(v) for v in t] for t in (ptr, rowptr_s, eid_s, dst_s))
    lam = float(np.float32(residual))
    abar = [a.double().sum(dim=1).div(H).tolist() if E else [] for a in alphas]
    ms = [None if masks is None or masks[l] is None else masks[l].double().reshape(-1).tolist() for l in range(L)]
    r = [float(v) for v in torch.as_tensor(start).double().reshape(-1).tolist()]
    rel = [0.0] * N
    flow = [[0.0] * E for _ in range(L)]
    for lo, hi in _ranges(ptr, N):
        if nmax is not None and hi - lo > nmax:
            for s in range(lo, hi):
                rel[s] = float("nan")
            continue
        cur = {s: r[s] for s in range(lo, hi)}
        for l in range(L - 1, -1, -1):
            nxt = {}
            for s in range(lo, hi):
                jlo = max(0, min(rowptr_s[s], E))
                jhi = max(jlo, min(rowptr_s[s + 1], E))
                acc = lam * cur[s]
                for j in range(jlo, jhi):
                    e, d = eid_s[j], dst_s[j]
                    if e < 0 or e >= E or d < lo or d >= hi:
                        continue
                    w = abar[l][e] * (1.0 if ms[l] is None else ms[l][s] * ms[l][d])
                    f = (1.0 - lam) * w * cur[d]
                    flow[l][e] = f
                    acc += f
                nxt[s] = acc
            cur = nxt
        for s in range(lo, hi):
            rel[s] = cur[s]
    return torch.tensor(rel, dtype=torch.float64), torch.tensor(flow, dtype=torch.float64).reshape(L, E)


def rollout_fp32(ptr, rowptr_s, eid_s, dst_s, alphas, start, masks=None, residual=0.5, nmax=None):
    """The same walk in the kernel's fp32 order: heads added h ascending, one multiplication by fp32(1 / H), (a * m[src]) *
    m[dst], (fp32(1 - lambda) * w) * r[dst], the node's sum from lambda * r[s] slot by slot.  -> fp32 tensors."""
    f32 = np.float32
    L, N = len(alphas), len(start)
    E, H = int(alphas[0].shape[0]), int(alphas[0].shape[1])
    ptr, rowptr_s, eid_s, dst_s = ([int(v) for v in t] for t in (ptr, rowptr_s, eid_s, dst_s))
    lam = f32(residual)
    one_minus, inv_h = f32(1.0) - lam, f32(1.0) / f32(H)
    al = [a.float().numpy() for a in alphas]
    ms = [None if masks is None or masks[l] is None else masks[l].float().reshape(-1).numpy() for l in range(L)]
    r = torch.as_tensor(start).float().reshape(-1).numpy()
    rel = np.zeros(N, dtype=f32)
    flow = np.zeros((L, E), dtype=f32)
    for lo, hi in _ranges(ptr, N):
        if nmax is not None and hi - lo > nmax:
            rel[lo:hi] = np.nan
            continue
        cur = r[lo:hi].copy()
        for l in range(L - 1, -1, -1):
            nxt = np.zeros_like(cur)
            for s in range(lo, hi):
                jlo = max(0, min(rowptr_s[s], E))
                jhi = max(jlo, min(rowptr_s[s + 1], E))
                acc = f32(lam * cur[s - lo])
                for j in range(jlo, jhi):
                    e, d = eid_s[j], dst_s[j]
                    if e < 0 or e >= E or d < lo or d >= hi:
                        continue
                    t = al[l][e, 0]
                    for h in range(1, H):
                        t = f32(t + al[l][e, h])
                    w = f32(t * inv_h)
                    if ms[l] is not None:
                        w = f32(f32(w * ms[l][s]) * ms[l][d])
                    f = f32(f32(one_minus * w) * cur[d - lo])
                    flow[l, e] = f
                    acc = f32(acc + f)
                nxt[s - lo] = acc
            cur = nxt
        rel[lo:hi] = cur
    return torch.from_numpy(rel), torch.from_numpy(flow)


def softmax_by_destination(logits, dst, N):
    """alpha [E, H] = exp(logit) / sum over the edges into the same destination, in float64, rounded to fp32 at the end."""
    ex = logits.double().exp()
    den = torch.zeros(N, logits.size(1), dtype=torch.float64).index_add_(0, dst.long(), ex)
    return (ex / den.index_select(0, dst.long())).float()


def make_graphs(sizes, degrees, seed, self_loops=True):
    """A batch of len(sizes) graphs, graph g with sizes[g] nodes.  Every node gets a self loop first (when asked for), then node i
    of a graph draws its out-degree from `degrees` (cycled with an offset per graph) and that many destinations inside its graph,
    with repeats (parallel edges).  The edge list is then shuffled, so that a node's out-slots are no run of edge ids.
    -> (ptr list [B + 1], batch int64 [N], edge_index int64 [2, E], the largest out-degree)."""
    gen = torch.Generator().manual_seed(seed)
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    src, dst = [], []
    for g, n in enumerate(sizes):
        for i in range(n):
            s = ptr[g] + i
            if self_loops:
                src.append(s)
                dst.append(s)
            k = degrees[(i + g) % len(degrees)]
            if k:
                src += [s] * k
                dst += (ptr[g] + torch.randint(0, n, (k,), generator=gen)).tolist()
    ei = torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)]
    N = ptr[-1]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long)) if N else torch.zeros(0, dtype=torch.long)
    dmax = int(torch.bincount(ei[0], minlength=max(N, 1)).max()) if ei.size(1) else 0
    return ptr, batch, ei, dmax
