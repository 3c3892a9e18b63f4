"""Attention dropout of the GATv2 message passing (include/isg_mp_train.h) on a real MI355X.

The reference is tests/mp_dropout_restated.py: the oracle's message passing with r(e, h) = keep(e, h) / (1 - p) between the softmax
and the aggregation, the keep mask from oracle.philox under the rule of include/isg_train.h keyed by (original edge id, head).
  1  the mask a kernel draws is that rule's, read back bit by bit from `out` on in-degree-1 graphs, on all three forward kernels
  2  p = 0 through the new entry points is the old entry points' launch: every result bit-equal
  3  alpha at p > 0 has the bits of alpha at p = 0
  4  forward and every gradient against float64 under the rule of tests/test_gpu_backward_fp64.py (its Judge, its constants), the
     float32 yardstick being the restatement in float32 with the same mask; which kernel a case reaches is asserted on the host
  5  a (destination, head) whose in-edges are all dropped holds +0 + bias
  6  two calls give the same bits; the mask follows the edge id, not the CSR slot or the order of edge_index
  7  MGAT / AnswerModel in train(): seeded, counted, eval() untouched, a training step runs
  8  the strict twin library gives the fast library's bits
"""
import ctypes
import functools
import math
import os

import pytest
import torch

import mp_dropout_restated as R
import test_gpu_backward_fp64 as B64
from conftest import ROOT

gpu = pytest.mark.gpu      # every test that launches; the host test of the cases runs everywhere

STRICT = os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc", "libisg_hip_strict.so")
P_DROP, SEED = 0.3, 0xC0FFEE1234567
SLOPE = 0.2

# ---- constants of csrc/isg_mp_graph.hip (launch_mp_graph, launch_mp_graph_flat) restated: which forward kernel a shape takes ------
GK_NCAP_S, GK_ECAP_S, GK_NCAP_L, GK_ECAP_L = 64, 256, 256, 1024


def forward_kernel(H, C, B, nmax, emax):
    """"chunk" (gatv2_mp_kernel), "grouped" (gatv2_mp_graph_kernel) or "flat" (gatv2_mp_graph_flat_kernel)."""
    if B <= 0 or nmax <= 0 or nmax > GK_NCAP_L or emax > GK_ECAP_L:
        return "chunk"
    HS = next((hs for hs in (8, 4, 2, 1) if H % hs == 0 and hs * C * 4 <= 1280), 1)
    G, Q = 64 // HS, C // 4
    passes = (Q + G - 1) // G
    if passes > 2:
        return "chunk"
    if HS == 1 and H > 1 and passes == 2 and Q * 10 < G * passes * 7:
        flat_passes = (2 * Q + 63) // 64
        return "flat" if nmax <= GK_NCAP_S and emax <= GK_ECAP_S and H % 2 == 0 and flat_passes in (2, 3, 4) else "chunk"
    return "grouped"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


# ---- topologies ------------------------------------------------------------------------------------------------------------------
BATCH8 = [5, 40, 17, 9, 33, 12, 26, 8]


@functools.lru_cache(maxsize=None)
def topology(name):
    """(batch [N], edge_index [2, E] in shuffled order, graphs).  "hub" is tests/test_gpu_backward_fp64.py's."""
    if name == "hub":
        return B64.topology("hub")
    sizes = {"batch8": BATCH8, "one300": [300]}[name]
    gen = torch.Generator().manual_seed({"batch8": 31, "one300": 32}[name])
    src, dst, off = [], [], 0
    for n in sizes:
        for v in range(n):
            src.append(off + v); dst.append(off + v)
        for _ in range(2 * n):
            src.append(off + int(torch.randint(0, n, (1,), generator=gen))); dst.append(off + int(torch.randint(0, n, (1,), generator=gen)))
        off += n
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ei = torch.tensor([src, dst], dtype=torch.long)
    return batch, ei[:, torch.randperm(ei.size(1), generator=gen)], len(sizes)


def bounds(name):
    batch, ei, B = topology(name)
    nmax = int(torch.bincount(batch, minlength=B).max())
    emax = int(torch.bincount(batch[ei[1]], minlength=B).max())
    return B, nmax, emax


# (topology, H, C, the forward kernel it claims)
SHAPES = [("hub", 4, 8, "chunk"), ("hub", 8, 4, "chunk"), ("batch8", 4, 128, "grouped"), ("batch8", 4, 300, "flat"),
          ("one300", 2, 16, "chunk")]
CASES = [(t, H, C, mk) for (t, H, C, _) in SHAPES for mk in B64.MASK_KINDS]
PER_KERNEL = [("batch8", 4, 128, "edge"), ("batch8", 4, 300, "node"), ("one300", 2, 16, "edge"), ("hub", 8, 4, "node")]


def _id(case):
    return "-".join(str(v) for v in case)


def test_cases_reach_the_kernels_they_claim():
    """On the host, from the restated constants: the forward kernel of every shape, more than one channel pass in the backward at
    C = 300, the hub's branches (asserted by the file the topology comes from), and that the cases cover what the list names."""
    for topo, H, C, want in SHAPES:
        assert forward_kernel(H, C, *bounds(topo)) == want, (topo, H, C)
        assert C % 4 == 0 and 1 <= B64.passes(H, C) <= 8
    assert {k for *_, k in SHAPES} == {"chunk", "grouped", "flat"}
    assert B64.passes(4, 300) > 1 and B64.passes(4, 128) == 2 and B64.passes(8, 4) == 1
    B, nmax, emax = bounds("hub")
    assert emax > GK_ECAP_L                                              # beyond the per-graph tables: the node-chunk kernel
    B64.test_topologies_reach_the_branches_they_claim()                     # MP_ECAP straddled, parked pairs, degree-0 nodes
    B, nmax, emax = bounds("batch8")
    assert B == 8 and 5 <= min(BATCH8) and nmax == max(BATCH8) == 40 <= GK_NCAP_S and emax <= GK_ECAP_S
    assert bounds("one300")[1] == 300 > GK_NCAP_L
    assert {forward_kernel(H, C, *bounds(t)) for t, H, C, _ in PER_KERNEL} == {"chunk", "grouped", "flat"}
    assert {H for _, H, _, _ in SHAPES} >= {2, 4, 8}                        # H = 8: the second Philox block
    # the in-degree-1 batch of test 1: 25 graphs of 40 nodes
    assert forward_kernel(8, 4, 25, 40, 40) == "grouped" and forward_kernel(1, 4, 25, 40, 40) == "grouped"
    assert all(forward_kernel(H, 300, 25, 40, 40) == "flat" for H in (2, 4, 8))
    # every case has dropped and kept pairs
    for topo, H, C, mk in CASES:
        keep = R.keep_mask(SEED, topology(topo)[1].size(1), H, P_DROP)
        assert 0.2 < 1.0 - float(keep.float().mean()) < 0.4


@functools.lru_cache(maxsize=None)
def inputs(case):
    topo, H, C, mk = case
    if topo == "hub":
        return B64.mp_inputs((topo, H, C, mk, SLOPE))
    batch, ei, B = topology(topo)
    N, E = batch.numel(), ei.size(1)
    gen = torch.Generator().manual_seed(20000 * B64.MASK_KINDS.index(mk) + 1000 * H + C + 7)
    r = lambda *s: torch.randn(*s, generator=gen)
    t = {"x_l": r(N, H * C), "x_r": r(N, H * C), "e_proj": r(E, H * C), "att": r(1, H, C) / math.sqrt(C), "bias": r(H * C),
         "w": r(N, H * C), "mask": None}
    if mk != "none":
        t["mask"] = B64.fractional_mask(N if mk == "node" else E, gen)
    return t


@functools.lru_cache(maxsize=None)
def oracle(case, dtype, p=P_DROP, seed=SEED):
    """{"out", "alpha", "grads" (x_l, x_r, e_proj, att, bias), "d mask"} of the restatement in `dtype` on the CPU."""
    topo, H, C, mk = case
    batch, ei, _ = topology(topo)
    t = inputs(case)
    N, E = batch.numel(), ei.size(1)
    leaves = [t[k].to(dtype).clone().requires_grad_(True) for k in ("x_l", "x_r", "e_proj", "att", "bias")]
    m = em = None
    with B64._one_thread():
        if mk != "none":
            m = t["mask"].to(dtype).clone().requires_grad_(True)
            em = B64._NodeToEdge.apply(m, ei) if mk == "node" else m
        r = R.factor(seed, E, H, p, dtype) if p > 0 else None
        out, alpha = R.message_passing(leaves[0].view(N, H, C), leaves[1].view(N, H, C), leaves[2].view(E, H, C), leaves[3], ei, em,
                                       SLOPE, r)
        out = out.reshape(N, H * C) + leaves[4]
        (out * t["w"].to(dtype)).sum().backward()
    return {"out": out.detach(), "alpha": alpha.detach(), "grads": [B64._grad(v) for v in leaves],
            "d mask": None if m is None else B64._grad(m)}


def on_device(case, dev):
    from isubgvqa_amd import ops
    topo, H, C, mk = case
    batch, ei, B = topology(topo)
    t = inputs(case)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    ten = {k: (None if v is None else v.to(dev)) for k, v in t.items()}
    return plan, ten


# ---- 4: forward and every gradient against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
@gpu
def test_forward_and_every_gradient_against_float64(dev, case):
    from isubgvqa_amd import ops
    topo, H, C, mk = case
    r64, r32 = oracle(case, torch.float64), oracle(case, torch.float32)
    plan, t = on_device(case, dev)
    judge = B64.Judge(_id(case) + f"-p{P_DROP}", B64.MP_CAP)
    gpu = [t[k].clone().requires_grad_(True) for k in ("x_l", "x_r", "e_proj", "att", "bias")]
    kw, m = {}, None
    if mk != "none":
        m = t["mask"].clone().requires_grad_(True)
        kw["node_mask" if mk == "node" else "edge_mask"] = m
    ops.reset_counters()
    out, alpha = ops.gatv2_mp(gpu[0], gpu[1], gpu[2], gpu[3], plan, H, bias=gpu[4], negative_slope=SLOPE, dropout_p=P_DROP,
                              dropout_seed=SEED, **kw)
    assert ops.counters()["mp_dropout"] == 1
    judge("forward", out, r64["out"], r32["out"])
    judge("alpha (before dropout)", alpha, r64["alpha"], r32["alpha"])
    (out * t["w"]).sum().backward()
    for name, a, b64, b32 in zip(B64.MP_NAMES, gpu, r64["grads"], r32["grads"]):
        assert a.grad is not None, name
        judge(name, a.grad.view(b64.shape), b64, b32)
    if m is not None:
        assert m.grad is not None, "d mask"
        judge(f"d {mk} mask", m.grad, r64["d mask"], r32["d mask"])
    # dropout is in the result: the same call without it differs, and its reference differs from this one
    with torch.no_grad():
        plain, alpha0 = ops.gatv2_mp(*[v.detach() for v in gpu[:4]], plan, H, bias=gpu[4].detach(), negative_slope=SLOPE,
                                     **{k: v.detach() for k, v in kw.items()})
    assert not torch.equal(plain, out.detach())
    assert torch.equal(alpha0, alpha), "alpha at p > 0 is not the p = 0 softmax, bit for bit"          # 3, on every case
    judge.done()


# ---- raw entry points: p = 0, alpha, the strict twin ----------------------------------------------------------------------------------
def raw_pair(fwd, bwd, case, dev, extra):
    """One forward and one backward through the C entry points `fwd` / `bwd` (the old ones: extra = (); the new: extra = (p, seed)).
    Buffers are pre-filled with NaN: an element a kernel leaves unwritten fails every comparison."""
    topo, H, C, mk = case
    plan, t = on_device(case, dev)
    N, E, HC = plan.N, plan.E, H * C
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, alpha = nan(N, HC), nan(E, H)
    p = lambda v: 0 if v is None else v.data_ptr()
    nm = t["mask"].reshape(-1).contiguous() if mk == "node" else None
    em = t["mask"].reshape(-1).contiguous() if mk == "edge" else None
    att = t["att"].reshape(-1).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    rc = fwd(p(t["x_l"]), p(t["x_r"]), p(t["e_proj"]), p(att), p(t["bias"]), p(plan.rowptr), p(plan.eid), p(plan.src), p(nm), p(em),
             p(out), p(alpha), N, E, H, C, SLOPE, p(plan.ptr), p(plan.eptr), p(plan.dst), plan.B, plan.nmax, plan.emax, HC, HC, HC,
             *extra, st)
    assert rc == 0, rc
    rowptr_s, eid_s, dst_s = plan.source_csr()
    d_xl, d_xr, d_e, part, d_m = nan(N, HC), nan(N, HC), nan(E, HC), nan((N + 15) // 16, HC), nan(E)
    rc = bwd(p(t["x_l"]), p(t["x_r"]), p(t["e_proj"]), p(att), p(alpha), p(t["w"]), p(plan.rowptr), p(plan.eid), p(plan.src),
             p(rowptr_s), p(eid_s), p(dst_s), p(nm), p(em), p(d_xl), p(d_xr), p(d_e), p(part), p(d_m) if mk != "none" else 0,
             N, E, H, C, SLOPE, *extra, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = {"out": out, "alpha": alpha, "d x_l": d_xl, "d x_r": d_xr, "d e_proj": d_e, "d att (partial rows)": part,
           "d bias": t["w"].sum(0)}                 # d bias is the column sum of grad_out in the wrapper: no kernel forms it
    if mk != "none":
        res["d edge mask"] = d_m
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), f"{k}: an element was not written"
    return res


@pytest.mark.parametrize("case", PER_KERNEL, ids=_id)
@gpu
def test_p0_is_the_old_path_bit_for_bit(dev, case):
    from isubgvqa_amd import _lib, _lib_mp_train
    old, new = _lib.load(), _lib_mp_train.load()
    want = raw_pair(old.isg_gatv2_mp_fwd, old.isg_gatv2_mp_bwd, case, dev, ())
    got = raw_pair(new.isg_gatv2_mp_fwd_dropout, new.isg_gatv2_mp_bwd_dropout, case, dev, (0.0, SEED))
    assert set(got) == set(want) and len(got) >= 7
    for k in want:
        assert torch.equal(got[k], want[k]), f"{_id(case)}: {k} at p = 0 differs from the existing entry point"


@pytest.mark.parametrize("case", PER_KERNEL, ids=_id)
@gpu
def test_alpha_is_untouched_and_the_strict_twin_agrees(dev, case):
    from isubgvqa_amd import _lib, _lib_mp_train
    old, new = _lib.load(), _lib_mp_train.load()
    plain = raw_pair(old.isg_gatv2_mp_fwd, old.isg_gatv2_mp_bwd, case, dev, ())
    fast = raw_pair(new.isg_gatv2_mp_fwd_dropout, new.isg_gatv2_mp_bwd_dropout, case, dev, (P_DROP, SEED))
    again = raw_pair(new.isg_gatv2_mp_fwd_dropout, new.isg_gatv2_mp_bwd_dropout, case, dev, (P_DROP, SEED))
    assert torch.equal(fast["alpha"], plain["alpha"]), "dropout touched the softmax"
    assert not torch.equal(fast["out"], plain["out"]) and not torch.equal(fast["d x_l"], plain["d x_l"])
    other = raw_pair(new.isg_gatv2_mp_fwd_dropout, new.isg_gatv2_mp_bwd_dropout, case, dev, (P_DROP, SEED + 1))
    assert torch.equal(other["alpha"], plain["alpha"]) and not torch.equal(other["out"], fast["out"])
    assert os.path.exists(STRICT), "csrc/libisg_hip_strict.so is missing: __graft_entry__.build() makes it beside the library"
    strict = _lib.bind(ctypes.CDLL(STRICT), _lib_mp_train.SIGNATURES)
    assert strict.isg_mp_train_abi_version() == _lib_mp_train.ABI_VERSION
    twin = raw_pair(strict.isg_gatv2_mp_fwd_dropout, strict.isg_gatv2_mp_bwd_dropout, case, dev, (P_DROP, SEED))
    for k in fast:
        assert torch.equal(again[k], fast[k]), f"{_id(case)}: {k}: two calls differ"
        assert torch.equal(twin[k], fast[k]), f"{_id(case)}: {k}: the strict twin differs"
    # and they are what the wrappers return
    from isubgvqa_amd import ops
    topo, H, C, mk = case
    plan, t = on_device(case, dev)
    kw = {} if mk == "none" else {("node_mask" if mk == "node" else "edge_mask"): t["mask"]}
    with torch.no_grad():
        out, alpha = ops.gatv2_mp(t["x_l"], t["x_r"], t["e_proj"], t["att"], plan, H, bias=t["bias"], negative_slope=SLOPE,
                                  dropout_p=P_DROP, dropout_seed=SEED, **kw)
        g = ops.gatv2_mp_backward(t["x_l"], t["x_r"], t["e_proj"], t["att"], alpha, t["w"], plan, H, negative_slope=SLOPE,
                                  want_mask_grad=mk != "none", dropout_p=P_DROP, dropout_seed=SEED, **kw)
    assert torch.equal(out, fast["out"]) and torch.equal(alpha, fast["alpha"])
    assert torch.equal(g[0], fast["d x_l"]) and torch.equal(g[1], fast["d x_r"]) and torch.equal(g[2], fast["d e_proj"])
    assert torch.equal(g[3], fast["d att (partial rows)"].sum(0))
    if mk != "none":
        assert torch.equal(g[5], fast["d edge mask"])


# ---- 1: the mask is the host rule's --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def indegree_one(graphs=25, n=40):
    """E = N = 1000: every node has exactly one in-edge, from a node of its graph; edge e goes to node perm[e], so an edge's id is
    neither its destination nor its CSR slot."""
    gen = torch.Generator().manual_seed(77)
    N = graphs * n
    dst = torch.randperm(N, generator=gen)
    src = (dst // n) * n + torch.randint(0, n, (N,), generator=gen)
    return torch.repeat_interleave(torch.arange(graphs), n), torch.stack([src, dst]), graphs


@pytest.mark.parametrize("H", [1, 2, 4, 8])
@gpu
def test_the_mask_is_the_host_rules(dev, H):
    """x_l = 1, att = 0: alpha is 1 on every edge (in-degree 1), out[dst_e, h * C] = keep(e, h) / (1 - p) exactly."""
    from isubgvqa_amd import ops
    batch, ei, B = indegree_one()
    N = E = batch.numel()
    assert E == 1000 and bool((torch.bincount(ei[1], minlength=N) == 1).all()) and not torch.equal(ei[1], torch.arange(N))
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    runs = [("chunk", 4), ("graph", 4)] + ([("graph", 300)] if H > 1 else [])          # node-chunk, grouped, flat
    for kernel, C in runs:
        ones, zeros = torch.ones(N, H * C, device=dev), torch.zeros(N, H * C, device=dev)
        att = torch.zeros(1, H, C, device=dev)
        for seed in (0, 0x9E3779B97F4A7C15, 2 ** 64 - 1):
            for p in (0.1, 0.5):
                with torch.no_grad():
                    out, alpha = ops.gatv2_mp(ones, zeros, zeros[:E], att, plan, H, kernel=kernel, dropout_p=p, dropout_seed=seed)
                assert bool((alpha == 1.0).all())
                got = out.view(N, H, C)[ei[1].to(dev)].cpu()                        # row e: the destination of edge e
                want = R.factor(seed, E, H, p)                                      # fp32: 0 or 1.0f / (1.0f - p)
                assert torch.equal(got[:, :, 0] != 0, R.keep_mask(seed, E, H, p)), (kernel, C, hex(seed), p)
                assert torch.equal(got, want[:, :, None].expand(E, H, C).contiguous()), (kernel, C, hex(seed), p)
                frac = 1.0 - float((got[:, :, 0] != 0).float().mean())
                assert abs(frac - p) < 4 * math.sqrt(p * (1 - p) / (E * H)) + 1e-9, (frac, p)      # four standard deviations


# ---- 5: rows whose in-edges are all dropped ------------------------------------------------------------------------------------------
@gpu
def test_rows_whose_in_edges_are_all_dropped_hold_the_bias(dev):
    from isubgvqa_amd import ops
    gen = torch.Generator().manual_seed(5)
    N, E, H, C, p = 120, 200, 4, 8, 0.5
    ei = torch.randint(0, N, (2, E), generator=gen)
    batch = torch.zeros(N, dtype=torch.long)
    indeg = torch.bincount(ei[1], minlength=N)
    # the seed is chosen here, on the host: the first under which some (destination with in-edges, head) keeps nothing
    for seed in range(64):
        kept = torch.zeros(N, H).index_add(0, ei[1], R.keep_mask(seed, E, H, p).float())
        dead = (kept == 0) & (indeg > 0)[:, None]
        if bool(dead.any()):
            break
    assert bool(dead.any()) and bool(((kept > 0) & (indeg > 0)[:, None]).any()), "a condition on the input, not on the kernel"
    x_l, x_r, e = (torch.randn(n, H * C, generator=gen).to(dev) for n in (N, N, E))
    att, bias = torch.randn(1, H, C, generator=gen).to(dev), torch.randn(H * C, generator=gen).to(dev)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=1)
    assert forward_kernel(H, C, 1, N, E) == "grouped"
    for kernel in ("graph", "chunk"):
        for b in (bias, None):
            with torch.no_grad():
                out, _ = ops.gatv2_mp(x_l, x_r, e, att, plan, H, bias=b, kernel=kernel, dropout_p=p, dropout_seed=seed)
            rows = out.view(N, H, C).cpu()[dead]
            want = torch.zeros(H, C) + (0.0 if b is None else b.view(H, C).cpu())
            assert torch.equal(rows, want.expand(N, H, C)[dead]), kernel
            assert not bool(torch.signbit(rows[rows == 0]).any()), "a dropped term left a negative zero"
            live = out.view(N, H, C).cpu()[(kept > 0) & (indeg > 0)[:, None]]
            assert not torch.equal(live, want.expand(N, H, C)[(kept > 0) & (indeg > 0)[:, None]])


# ---- 6: the mask follows the edge id ----------------------------------------------------------------------------------------------------
@gpu
def test_the_mask_follows_the_edge_id_not_the_slot_or_the_order(dev):
    """x_l = 1, att = 0 on "batch8": every term of a destination's sum is the same number or zero, so the sum does not depend on
    the order of its slots and `out` is a function of the kept in-edges alone.  A plan built from a shuffled edge_index whose slots
    carry the ORIGINAL edge ids gives the same bits, on either kernel.  Between the node-chunk and the per-graph kernel the kept
    pairs are the same; their alpha = 1 / deg is an IEEE division in one and the hardware reciprocal in the other, so the values
    agree to a few ulps, not to the bit (as without dropout)."""
    from isubgvqa_amd import ops
    batch, ei, B = topology("batch8")
    N, E, H, C = batch.numel(), ei.size(1), 4, 8
    ones, zeros, att = torch.ones(N, H * C, device=dev), torch.zeros(max(N, E), H * C, device=dev), torch.zeros(1, H, C, device=dev)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    run = lambda pl, kernel: ops.gatv2_mp(ones, zeros[:N], zeros[:E], att, pl, H, kernel=kernel, dropout_p=0.5, dropout_seed=SEED)[0]
    with torch.no_grad():
        base = run(plan, "graph")
        base_of = {"graph": base, "chunk": run(plan, "chunk")}
        assert torch.equal(run(plan, "graph"), base) and torch.equal(run(plan, "chunk"), base_of["chunk"])       # two identical calls
        assert torch.equal(base_of["chunk"] != 0, base != 0) and float((base_of["chunk"] - base).abs().max()) <= 4e-7 * float(base.max())
        # what the rule says: (kept in-edges) * (1 / deg) * (1 / (1 - p)), each product rounded as the kernel rounds it
        kept = torch.zeros(N, H).index_add(0, ei[1], R.keep_mask(SEED, E, H, 0.5).float())
        assert torch.equal(base.view(N, H, C)[:, :, 0].cpu() != 0, kept != 0)
        perm = torch.randperm(E, generator=torch.Generator().manual_seed(3))
        assert not torch.equal(perm, torch.arange(E))
        shuffled = ops.GraphPlan.build(batch.to(dev), ei[:, perm].to(dev), num_graphs=B)
        moved = run(shuffled, "graph")                   # new edge k is old edge perm[k] under its NEW id k: another mask
        assert not torch.equal(moved, base)
        shuffled.eid.copy_(perm.to(dev)[shuffled.eid.long()].int())        # the slots carry the original ids again
        for kernel in ("graph", "chunk"):
            assert torch.equal(run(shuffled, kernel), base_of[kernel]), kernel


# ---- 7: module level ---------------------------------------------------------------------------------------------------------------------
def _mgat(attn_dropout, dev, seed=0):
    from isubgvqa_amd.models.mgat import MGAT
    torch.manual_seed(seed)
    m = MGAT(channels=128, num_ins=2, heads=4, use_instr=True, masking_thresholds=[1.0, 0.15], use_topk=True, sampler_type="gumbel",
             sample_k=5, attn_dropout=attn_dropout)
    for conv in m.convs:
        conv.mask.gate_dropout = 0.0          # torch's own dropout on the gate (out of scope) would draw from the device generator
    return m.to(dev)


def _run_mgat(m, wl, seed):
    return m(x=wl.x, edge_index=wl.edge_index, instr_vectors=wl.instr, global_language_feats=wl.glf, edge_attr=wl.edge_attr,
             batch=wl.batch, return_masks=True, seed=seed)[0]


@gpu
def test_mgat_trains_with_seeded_attention_dropout(dev):
    from isubgvqa_amd import ops, synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=24, channels=128, layers=2, masks=(1.0, 0.15), sampler="gumbel", sample_k=5, seed=5)
    wl = synthetic.make_workload(cfg).to(dev)
    w = torch.randn(wl.x.size(0), 128, generator=torch.Generator().manual_seed(2)).to(dev)
    m = _mgat(0.2, dev).train()

    def step(seed):
        m.zero_grad(set_to_none=True)
        ops.reset_counters()
        h = _run_mgat(m, wl, seed)
        (h * w).sum().backward()
        assert ops.counters()["mp_dropout"] == 2
        return h.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}

    h1, g1 = step(11)
    h2, g2 = step(11)
    h3, g3 = step(12)
    assert bool(torch.isfinite(h1).all()) and torch.equal(h1, h2) and set(g1) == set(g2) and len(g1) > 10
    # mask.ques_nn is the one exception to bit equality, with or without dropout: its gradient arrives through torch's backward of
    # the gate's row gather q[batch], an atomic scatter-add whose order differs from run to run (measured at attn_dropout = 0 as
    # well: 1e-7 of the largest entry).  Every other gradient repeats to the bit.
    loose = [k for k in g1 if ".mask.ques_nn." in k]
    assert 0 < len(loose) <= 4 and len(g1) - len(loose) > 10
    for k in g1:
        if k in loose:
            assert float((g1[k] - g2[k]).abs().max()) <= 1e-5 * float(g1[k].abs().max()), k
        else:
            assert torch.equal(g1[k], g2[k]), f"{k}: the same seed gave another gradient"
    assert not torch.equal(h1, h3) and any(not torch.equal(g1[k], g3[k]) for k in g1 if k not in loose)
    # train() under no_grad drops too: the fused routes have no dropout and were not taken
    ops.reset_counters()
    with torch.no_grad():
        hn = _run_mgat(m, wl, 11)
    assert ops.counters()["mp_dropout"] == 2 and not torch.equal(hn, _run_mgat_eval(m, wl, 11))
    m.train()
    # without a seed the base comes from torch's CPU generator: torch.manual_seed reproduces a run
    with torch.no_grad():
        torch.manual_seed(4); a = _run_mgat_noise(m, wl)
        torch.manual_seed(4); b = _run_mgat_noise(m, wl)
        c = _run_mgat_noise(m, wl)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # eval(): bit-equal to a model built without dropout
    ops.reset_counters()
    plain = _mgat(0.0, dev).eval()
    assert all(torch.equal(x, y) for x, y in zip(plain.state_dict().values(), m.state_dict().values()))
    assert torch.equal(_run_mgat_eval(m, wl, 11), _run_mgat_eval(plain, wl, 11)) and ops.counters()["mp_dropout"] == 0


def _run_mgat_eval(m, wl, seed):
    m.eval()
    with torch.no_grad():
        return _run_mgat(m, wl, seed)


def _run_mgat_noise(m, wl):
    """No seed for the layers: explicit sampler noise, so that only the dropout's base seed is drawn."""
    noises = {1: torch.zeros(wl.glf.size(0), int(torch.bincount(wl.batch).max()), device=wl.x.device)}
    return m(x=wl.x, edge_index=wl.edge_index, instr_vectors=wl.instr, global_language_feats=wl.glf, edge_attr=wl.edge_attr,
             batch=wl.batch, return_masks=True, noises=noises)[0]


@gpu
def test_a_training_step_with_attention_dropout_leaves_finite_parameters(dev):
    from isubgvqa_amd import ops, optim, synthetic, train
    cfg = synthetic.WorkloadConfig(num_graphs=32, channels=64, layers=3, masks=(1.0, 0.15, 0.15), sampler="gumbel", sample_k=5, seed=123)
    wl = synthetic.make_workload(cfg).to(dev)
    torch.manual_seed(0)
    model = synthetic.AnswerModel(cfg.channels, cfg.layers, cfg.masks, cfg.sampler, cfg.sample_k, attn_dropout=0.1).to(dev).train()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    target = torch.randint(0, 1842, (cfg.num_graphs,), generator=torch.Generator().manual_seed(1)).to(dev)
    opt = optim.Adam(model.parameters(), lr=2e-3, max_grad_norm=2.0)
    meters = train.Meters(dev)
    ops.reset_counters()
    train.train_step(model, opt, wl, target, meters, seed=7)
    torch.cuda.synchronize()
    assert ops.counters()["mp_dropout"] == cfg.layers
    rep = meters.report()
    assert rep["steps"] == 1 and rep["skipped_steps"] == 0 and rep["nonfinite_losses"] == 0
    after = dict(model.named_parameters())
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert any(not torch.equal(before[k], v.detach()) for k, v in after.items() if "gat_seq.convs" in k), "no layer moved"
