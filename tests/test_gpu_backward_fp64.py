"""Training gradients of the HIP path against the CPU oracle in float64, on every code path of the backward kernels.

Reference: `oracle/model.py` / `oracle/primitives.py` evaluated on the CPU in float64 and differentiated by torch autograd
(the reference's node -> edge mask rule, gradient to the destination only, restated below so that it keeps float64).
Yardstick: the SAME oracle call in float32 on the CPU.  For every forward result and every gradient tensor

    e_k  = max |kernel - ref64| / max |ref64|          e_32 = max |oracle32 - ref64| / max |ref64|

and the test asserts  e_k <= max(F * e_32, FLOOR)  and, beside it, the absolute cap the older tests use (2e-4 message
passing, 3e-4 tail kernels, 2e-3 Linear).  FLOOR = 2e-6 is a few dozen fp32 ulps of the largest entry, for tensors whose fp32
sample happens to be lucky.  Where the float64 reference is identically zero the kernel's result must be exact zeros.

Measured on the MI355X (e_k / e_32 per tensor and case; "above the floor" = the rows with e_k > FLOOR, where F decides).  The
table is from the run that found the two findings below, with F = 8 then and dW on torch below 4096 rows; the "hub" node masks of
that run were zero on the hub in three of five cases (now HUB_MASK there, see mp_inputs), and those rows and the Linear row are to
be recorded again from this tree:

    part                          tensors                           max e_k    e_32 range        max ratio   above the floor
    message passing "hub"         d x_l, d x_r, d e_proj, d att     3.0e-6     1.0e-7 .. 5.1e-6  1.8         0.6
                                  d node mask / d edge mask         8.0e-7     1.1e-7 .. 5.0e-6  2.5         --
                                  d bias, forward                   2.2e-6     6.5e-8 .. 2.2e-6  1.6         1.0
    message passing "small"       all six gradients, forward        8.1e-7     7.4e-8 .. 5.7e-7  2.4         --
    message passing edge shapes   all                               3.2e-7     3.5e-8 .. 3.7e-7  2.2         --
    node_to_edge_mask_backward    d node mask                       1.2e-7     1.2e-7            1.0         --
    layer tail                    d ins, d c, d h, d weight, d mask 2.3e-6     1.2e-7 .. 2.8e-6  2.5         0.8
                                  d mean_scale (a cancelling sum)   2.8e-5     9.0e-8 .. 2.8e-5  1.4         1.1
                                  d bias                            1.1e-6     6.0e-8 .. 1.9e-7  9.5         --
    pooling (both variants)       d xn, d q, d mask, forward        6.5e-7     3.9e-8 .. 7.8e-6  2.1         --
    instruction gate, node gates  d x / d xn, d instr / d q, forward 1.1e-6    8.2e-8 .. 2.1e-6  1.9         --
    autograd.linear               dX, dW, db, forward               7.5e-7     5.7e-8 .. 6.2e-7  2.1         --

F = 4: the smallest of 2, 4, 8 that leaves a factor of 2 over the largest ratio among the rows it decides (1.1).  One ratio above
4 remains, below the floor: d bias of the layer tail (1.1e-6).  tail_bwd_kernel adds the up to 1024 rows of a graph into one fp32
accumulator per channel, torch's CPU sum is a cascade of short chains (e_32 = 6e-8 .. 1.9e-7); sqrt(1024) * 2^-24 / 2 = 1e-6.

Two findings of the first run are fixed in this tree rather than covered by F:
  * isg_gatv2_mp_bwd, "hub" with a node mask (H = 2, C = 16): d x_r 3.5e-5 (13 x e_32), d node mask 8.3e-6 (16 x), d att
    9.6e-6 (5 x), d e_proj 1.4e-5.  The stored alpha of the 1100-edge destination sum to 1 + 2.4e-6 / 1 + 3.9e-6 (the forward's
    fp32 denominator), and da_e = alpha_e (dalpha_e - sum alpha dalpha) passes that residue times S to every edge with one sign,
    where d x_r and d mask are cancelling sums.  The kernel now divides S by the sum of the alphas and keeps both sums in fp64;
    the same case: 1.6e-6, 5.4e-7, 1.3e-6, 3.0e-6.
  * _Linear.backward, M = 16383 (dW through torch below the switch): 2.6e-6 .. 4.0e-6, 6 .. 10 x e_32; 2.3e-6 (6.7 x) at
    M = 4095.  One fp32 chain over the rows: sqrt(M) * 3.7e-8.  The switch to isg_linear_wgrad moved from 16384 to 2048 rows
    (autograd.WGRAD_MIN_ROWS), below which that chain stays under the floor (1.1e-6 at 2047 rows); the shapes "switch-1" and
    "switch" are the two sides of that constant, whatever it is.

Which shape reaches which branch is asserted on the host by `test_topologies_reach_the_branches_they_claim` (no GPU), from
the constants of csrc/isg_mp.hpp restated below.
"""
import functools
import math

import pytest
import torch

# ---- constants of csrc/isg_mp.hpp and the channel-pass count of csrc/isg_mp_bwd.hip (launch_bwd), restated --------------
MP_NPB = 16      # destination nodes per workgroup
MP_ECAP = 1024   # CSR slots of a workgroup staged in LDS; slots beyond are read from global memory
MP_LCAP = 32     # in-edges of a destination whose (dal, raw) stay in LDS; beyond that they are parked in d_e_proj


def passes(H, C):
    """P of gatv2_mp_bwd_*_kernel<H, P>: float4 columns of a head (C / 4) over the 64 / H lanes of its group."""
    G, Q = 64 // H, C // 4
    return (Q + G - 1) // G


FLOOR = 2e-6
F = 4
MP_CAP, TAIL_CAP, LINEAR_CAP = 2e-4, 3e-4, 2e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


# ---- the rule -------------------------------------------------------------------------------------------------------------
class Judge:
    """Collects every comparison of one test; prints each figure before anything is asserted."""

    def __init__(self, case, cap):
        self.case, self.cap, self.bad = case, cap, []

    def __call__(self, name, got, ref64, ref32):
        got = got.detach().cpu()
        if tuple(got.shape) != tuple(ref64.shape):
            self.bad.append(f"{name}: shape {tuple(got.shape)}, reference {tuple(ref64.shape)}")
            return
        if got.numel() == 0:
            return
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f"{name}: not finite")
            return
        scale = float(ref64.abs().max())
        if scale == 0.0:                      # the formula says zero: exact zeros, nothing left unwritten
            worst = float(got.abs().max())
            print(f"[fp64] {self.case} | {name} | exact zero expected, max |kernel| = {worst:.3e}")
            if worst != 0.0:
                self.bad.append(f"{name}: reference is identically zero, kernel has {worst:.3e}")
            return
        e_k = float((got.double() - ref64).abs().max()) / scale
        e_32 = float((ref32.double() - ref64).abs().max()) / scale
        bound = max(F * e_32, FLOOR)
        print(f"[fp64] {self.case} | {name} | e_k={e_k:.3e} e_32={e_32:.3e} ratio={e_k / max(e_32, 1e-30):.2f}")
        if not e_k <= bound:
            self.bad.append(f"{name}: e_k = {e_k:.3e} > max({F} * e_32, floor) = {bound:.3e}  (e_32 = {e_32:.3e})")
        if not e_k < self.cap:
            self.bad.append(f"{name}: e_k = {e_k:.3e} is not below the absolute cap {self.cap}")

    def zeros(self, name, got, shape):
        got = got.detach().cpu()
        if tuple(got.shape) != tuple(shape) or (got.numel() and float(got.abs().max()) != 0.0):
            self.bad.append(f"{name}: expected exact zeros of shape {tuple(shape)}")

    def done(self):
        assert not self.bad, f"{self.case}:\n  " + "\n  ".join(self.bad)


class _one_thread:
    """The oracle's tensors are small: on one thread, torch's intra-op pool costs more here than it gives."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def _grad(t):
    return torch.zeros_like(t) if t.grad is None else t.grad.detach()


def fractional_mask(n, gen):
    """~30 % exact zeros (a few of them -0.0), the rest in [0.25, 1.75], some of them straight-through values
    (hard - khot) + khot, which sit an ulp beside 1."""
    m = 0.25 + 1.5 * torch.rand(n, 1, generator=gen)
    khot = torch.rand(n, 1, generator=gen)
    st = (torch.ones(n, 1) - khot) + khot
    m = torch.where(torch.rand(n, 1, generator=gen) < 0.2, st, m)
    u = torch.rand(n, 1, generator=gen)
    m = torch.where(u < 0.3, torch.zeros(n, 1), m)
    m = torch.where(u < 0.05, torch.full((n, 1), -0.0), m)
    m[int(u.argmin())] = -0.0      # a short mask has a -0.0 too
    return m


class _NodeToEdge(torch.autograd.Function):
    """NodeMaskToEdgeMask of the reference (sampling/node_edge_masks.py:7-19) in the dtype of the mask: the product of both
    ends forward, the edge-mask gradient scattered to the DESTINATION only backward."""

    @staticmethod
    def forward(ctx, mask, edge_index):
        ctx.save_for_backward(edge_index)
        ctx.n = mask.shape[0]
        return mask[edge_index[0]] * mask[edge_index[1]]

    @staticmethod
    def backward(ctx, g):
        from oracle import primitives as P
        (edge_index,) = ctx.saved_tensors
        return P.scatter_sum(g, edge_index[1], ctx.n), None


# ==========================================================================================================================
# Part 1: message passing
# ==========================================================================================================================
def _draw(gen, n, ban=None):
    while True:
        v = int(torch.randint(0, n, (1,), generator=gen))
        if v != ban:
            return v


HUB_SIZES = [20, 1, 16, 17, 3]
HUB_NODE, HUB_IN, SENDER, SENDER_OUT, NO_IN, NO_OUT = 3, 1100, 5, 40, 7, 9      # all in graph 0
HUB_MASK, SENDER_MASK = 1.625, 0.75     # the node masks of the "hub" runs on those two nodes: fractional, one above 1
MASKED_OUT = 0                          # ... and a node of graph 0 they mask out, so the hub has dead in-slots on both sides too
MIN_LIVE = 16                           # live (m_e != 0) hub in-slots demanded on EACH side of slot MP_ECAP, and sender out-edges
MASK_KINDS = ("none", "node", "edge")
SMALL_SIZES = [5, 1, 9, 17, 3]
SMALL_HUB = 40


@functools.lru_cache(maxsize=None)
def topology(name):
    """(batch[N], edge_index[2, E], number of graphs).  Edge order shuffled."""
    gen = torch.Generator().manual_seed({"hub": 11, "small": 12, "n16": 13, "n17": 14}.get(name, 15))
    if name in ("e0", "singles", "n0"):
        sizes = {"e0": [5, 3], "singles": [1] * 5, "n0": []}[name]
        batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))
        return batch, torch.zeros(2, 0, dtype=torch.long), len(sizes)
    sizes = {"hub": HUB_SIZES, "small": SMALL_SIZES, "n16": [16], "n17": [17]}[name]
    hub = name == "hub"
    src, dst, off = [], [], 0
    for g, n in enumerate(sizes):
        special = hub and g == 0
        for v in range(n):
            if not (special and v in (NO_IN, NO_OUT)):      # the two degree-0 nodes have no self-loop either
                src.append(off + v); dst.append(off + v)
        for _ in range(2 * n):
            src.append(off + _draw(gen, n, NO_OUT if special else None))
            dst.append(off + _draw(gen, n, NO_IN if special else None))
        if special:
            for _ in range(HUB_IN):
                src.append(_draw(gen, n, NO_OUT)); dst.append(HUB_NODE)
            for _ in range(SENDER_OUT):
                src.append(SENDER); dst.append(_draw(gen, n, NO_IN))
            for k in (0, 4, 19, 23, 31):                    # a few edges twice (self-loops and random ones)
                src.append(src[k]); dst.append(dst[k])
        if name == "small" and g == 0:
            for _ in range(SMALL_HUB):                      # beyond the per-wave LDS strip
                src.append(_draw(gen, n)); dst.append(0)
        off += n
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ei = torch.tensor([src, dst], dtype=torch.long)
    return batch, ei[:, torch.randperm(ei.size(1), generator=gen)], len(sizes)


HUB_HC = [(4, 8), (8, 4), (2, 16), (1, 32), (4, 300)]
HUB_CASES = [("hub", H, C, mk, 0.2) for (H, C) in HUB_HC for mk in MASK_KINDS]
SMALL_FULL = [(H, 4 * P * (64 // H)) for H in (1, 2, 4, 8) for P in range(1, 9)]        # every pass full
SMALL_PARTIAL = [(1, 300), (2, 200), (4, 300), (8, 12)]                                # last pass partial
SMALL_CASES = ([("small", H, C, "edge", 0.2) for (H, C) in SMALL_FULL + SMALL_PARTIAL]
               + [("small", 4, 8, "edge", 1.5), ("small", 4, 8, "edge", 0.0)])
EDGE_CASES = [("n16", 4, 8, "node", 0.2), ("n17", 4, 8, "node", 0.2), ("e0", 4, 8, "none", 0.2),
              ("n0", 4, 8, "none", 0.2), ("singles", 2, 16, "none", 0.2)]
MP_NAMES = ("d x_l", "d x_r", "d e_proj", "d att", "d bias")


def _mp_id(case):
    topo, H, C, mk, slope = case
    return f"{topo}-H{H}-C{C}-P{passes(H, C)}-{mk}" + ("" if slope == 0.2 else f"-slope{slope}")


@functools.lru_cache(maxsize=None)
def mp_inputs(case):
    topo, H, C, mk, slope = case
    batch, ei, B = topology(topo)
    N, E = batch.numel(), ei.size(1)
    gen = torch.Generator().manual_seed(10000 * MASK_KINDS.index(mk) + 1000 * H + C)
    r = lambda *s: torch.randn(*s, generator=gen)
    t = {"x_l": r(N, H * C), "x_r": r(N, H * C), "e_proj": r(E, H * C), "att": r(1, H, C) / math.sqrt(C), "bias": r(H * C),
         "w": r(N, H * C), "mask": None}
    if mk == "node":
        t["mask"] = fractional_mask(N, gen)
        if topo == "hub":       # a zero on the hub would zero m_e on all its in-edges, and with it everything the parking carries
            t["mask"][HUB_NODE], t["mask"][SENDER], t["mask"][MASKED_OUT] = HUB_MASK, SENDER_MASK, 0.0
    elif mk == "edge":
        t["mask"] = fractional_mask(E, gen)
    return t


def edge_mask_of(case):
    """m_e per edge id as the kernels form it: the edge mask itself, or the product of the node mask at both ends."""
    topo, _, _, mk, _ = case
    _, ei, _ = topology(topo)
    m = mp_inputs(case)["mask"]
    return m[:, 0] if mk == "edge" else m[ei[0], 0] * m[ei[1], 0]


@functools.lru_cache(maxsize=None)
def mp_oracle(case, dtype):
    """{"out", "grads" (x_l, x_r, e_proj, att, bias), "d mask"} of the oracle in `dtype` on the CPU."""
    from oracle import model as OM
    topo, H, C, mk, slope = case
    batch, ei, _ = topology(topo)
    t = mp_inputs(case)
    N, E = batch.numel(), ei.size(1)
    leaves = [t[k].to(dtype).clone().requires_grad_(True) for k in ("x_l", "x_r", "e_proj", "att", "bias")]
    m = em = None
    with _one_thread():
        if mk != "none":
            m = t["mask"].to(dtype).clone().requires_grad_(True)
            em = _NodeToEdge.apply(m, ei) if mk == "node" else m
        out, _ = OM.gatv2_message_passing(leaves[0].view(N, H, C), leaves[1].view(N, H, C), leaves[2].view(E, H, C),
                                          leaves[3], ei, em, slope)
        out = out.reshape(N, H * C) + leaves[4]
        (out * t["w"].to(dtype)).sum().backward()
    return {"out": out.detach(), "grads": [_grad(v) for v in leaves], "d mask": None if m is None else _grad(m)}


def run_mp_case(case, dev):
    from isubgvqa_amd import ops
    topo, H, C, mk, slope = case
    batch, ei, B = topology(topo)
    t = mp_inputs(case)
    r64, r32 = mp_oracle(case, torch.float64), mp_oracle(case, torch.float32)
    N, E = batch.numel(), ei.size(1)
    judge = Judge(_mp_id(case), MP_CAP)

    gpu = [t[k].to(dev).requires_grad_(True) for k in ("x_l", "x_r", "e_proj", "att", "bias")]
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    kw, m = {}, None
    if mk != "none":
        m = t["mask"].to(dev).requires_grad_(True)
        kw["node_mask" if mk == "node" else "edge_mask"] = m
    out, alpha = ops.gatv2_mp(gpu[0], gpu[1], gpu[2], gpu[3], plan, H, bias=gpu[4], negative_slope=slope, **kw)
    judge("forward", out, r64["out"], r32["out"])
    w = t["w"].to(dev)
    (out * w).sum().backward()
    for name, a, b64, b32 in zip(MP_NAMES, gpu, r64["grads"], r32["grads"]):
        assert a.grad is not None, name
        judge(name, a.grad.view(b64.shape), b64, b32)
    if m is not None:
        assert m.grad is not None, "d mask"
        judge(f"d {mk} mask", m.grad, r64["d mask"], r32["d mask"])

    # the operator itself: twice on the same input (fixed order, no atomics: the bits repeat), and under a mask without the
    # mask gradient
    with torch.no_grad():
        ins = [v.detach() for v in gpu[:4]]
        dkw = {k: v.detach() for k, v in kw.items()}
        call = lambda want: ops.gatv2_mp_backward(*ins, alpha.detach(), w, plan, H, negative_slope=slope,
                                                  want_mask_grad=want, **dkw)
        a, b = call(mk != "none"), call(mk != "none")
        for i, name in enumerate(MP_NAMES + ("d edge mask",)):
            if a[i] is None:
                assert b[i] is None and mk == "none", name
            elif not torch.equal(a[i], b[i]):
                judge.bad.append(f"{name}: two calls on the same input differ in their bits")
        if mk != "none":
            c = call(False)
            assert c[5] is None
            for name, got, b64, b32 in zip(MP_NAMES, c, r64["grads"], r32["grads"]):
                judge(name + " (no mask gradient)", got.view(b64.shape), b64, b32)
    return judge, [v.grad for v in gpu]


@pytest.mark.gpu
@pytest.mark.parametrize("case", HUB_CASES, ids=_mp_id)
def test_mp_backward_hub(dev, case):
    """A block of 16 destinations beyond MP_ECAP slots, a destination whose parked pairs straddle that boundary, a node
    without in-edges, one without out-edges, a source hub, duplicate edges; fractional masks with their gradient."""
    judge, _ = run_mp_case(case, dev)
    judge.done()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL_CASES, ids=_mp_id)
def test_mp_backward_every_instantiation(dev, case):
    """Every (H, P) instantiation of the two backward kernels once, one partial last pass per H, and slopes outside
    (0, 1)."""
    judge, _ = run_mp_case(case, dev)
    judge.done()


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=_mp_id)
def test_mp_backward_edge_shapes(dev, case):
    """N = 16 (one full block), N = 17 (a block of one node), no edges at all, no nodes at all, only 1-node graphs."""
    topo, H, C, mk, slope = case
    batch, ei, _ = topology(topo)
    N, E = batch.numel(), ei.size(1)
    judge, grads = run_mp_case(case, dev)
    if E == 0:      # without an edge the output is the bias: everything but d bias is exactly zero
        for name, g, shape in zip(MP_NAMES[:4], grads, [(N, H * C), (N, H * C), (0, H * C), (1, H, C)]):
            judge.zeros(name, g, shape)
        assert tuple(grads[4].shape) == (H * C,)
    judge.done()


@pytest.mark.gpu
def test_mp_backward_refuses_what_it_has_no_kernel_for(dev):
    """More than 8 channel passes (H = 8, C = 260) and a head count outside {1, 2, 4, 8}: the library's error from the host
    side of the call, before any launch."""
    from isubgvqa_amd import _lib, ops
    batch, ei, B = topology("small")
    N, E = batch.numel(), ei.size(1)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    for H, C in [(8, 260), (3, 8), (16, 4)]:
        assert H not in (1, 2, 4, 8) or passes(H, C) > 8
        z = lambda *s: torch.zeros(*s, device=dev)
        with pytest.raises(_lib.IsgError, match="isg_gatv2_mp_bwd"):
            ops.gatv2_mp_backward(z(N, H * C), z(N, H * C), z(E, H * C), z(1, H, C), z(E, H), z(N, H * C), plan, H)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_node_to_edge_mask_backward_on_the_hub(dev):
    """The 1100-edge destination and the node without an in-edge, against index_add_ by destination in float64."""
    from isubgvqa_amd import ops
    batch, ei, B = topology("hub")
    N, E = batch.numel(), ei.size(1)
    d_edge = torch.randn(E, generator=torch.Generator().manual_seed(5))
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    got = ops.node_to_edge_mask_backward(d_edge.to(dev), plan)
    ref64 = torch.zeros(N, dtype=torch.float64).index_add_(0, ei[1], d_edge.double())
    ref32 = torch.zeros(N).index_add_(0, ei[1], d_edge)
    judge = Judge("node_to_edge_mask_backward hub", MP_CAP)
    judge("d node mask", got, ref64, ref32)
    assert float(got[NO_IN]) == 0.0 and float(ref64[NO_IN]) == 0.0
    assert torch.equal(got, ops.node_to_edge_mask_backward(d_edge.to(dev), plan))
    judge.done()


# ==========================================================================================================================
# Part 2: layer tail, pooling, instruction gate, node gate
# ==========================================================================================================================
TAIL_SIZES = [5, 1, 0, 2, 63, 64, 65, 0, 255, 256, 257, 1024, 1, 17]        # N = 2010; two empty graphs; TB_NCAP = 1024
TAIL_ZERO_GRAPH = 6                                                      # its mask is all zero in the masked runs
TAIL_C = [4, 64, 68, 128, 132, 300, 1024]                                # both sides of the tb_block steps; TB_CCAP
TAIL_CASES = [(C, masked) for C in TAIL_C for masked in (False, True)]
TAIL_OPS = ("tail", "pool out+gate", "pool out", "instr gate", "node gate dbl", "node gate")
EPS = 1e-5


def _tail_batch():
    return torch.repeat_interleave(torch.arange(len(TAIL_SIZES)), torch.tensor(TAIL_SIZES))


@functools.lru_cache(maxsize=None)
def tail_inputs(case):
    """op -> (leaves, weights of the loss, one per output)"""
    C, masked = case
    B, batch = len(TAIL_SIZES), _tail_batch()
    N = batch.numel()
    gen = torch.Generator().manual_seed(7 * C + int(masked))
    r = lambda *s: torch.randn(*s, generator=gen)
    u = lambda *s: 0.5 + torch.rand(*s, generator=gen)
    mask = None
    if masked:
        mask = fractional_mask(N, gen)
        mask[batch == TAIL_ZERO_GRAPH] = 0.0
    opt = [mask] if masked else []
    return {"tail": ([r(B, C), r(N, C), r(N, C), u(C), r(C), u(C)] + opt, [r(N, C)]),
            "pool out+gate": ([r(N, C), r(B, C)] + opt, [r(B, C), r(N, 1)]),
            "pool out": ([r(N, C), r(B, C)] + opt, [r(B, C)]),
            "instr gate": ([r(N, C), r(B, C)], [r(N, C)]),
            "node gate dbl": ([r(N, C), r(B, C)], [r(N, 1)]),
            "node gate": ([r(N, C), r(B, C)], [r(N, 1)])}


def _tail_oracle_op(op, leaves, masked, batch, B):
    from oracle import model as OM
    from oracle import primitives as P
    if op == "tail":
        ins, c, h, weight, bias, ms = leaves[:6]
        v = OM.scatter_scaled_dot_product_attention(ins, c, c, batch, B)
        y = P.graph_norm(v, batch, weight, bias, ms, EPS, num_graphs=B) + h
        return (leaves[6] * y if masked else y,)
    if op.startswith("pool"):
        xn, q = leaves[:2]
        x = xn * leaves[2] if masked else xn
        gate = P.pyg_softmax((x * q[batch]).sum(-1, keepdim=True) / math.sqrt(x.size(1)), batch, B)
        out = P.scatter_sum(gate * x, batch, B)
        return (out, gate) if op == "pool out+gate" else (out,)
    if op == "instr gate":
        return (P.gelu(leaves[0] * leaves[1][batch]),)
    xn, q = leaves
    idx = batch[batch] if op == "node gate dbl" else batch
    return (P.gelu((xn * q[idx]).sum(-1, keepdim=True) / math.sqrt(xn.size(1))),)


@functools.lru_cache(maxsize=None)
def tail_oracle(case, op, dtype):
    """(outputs, gradients of the leaves) of one operator in `dtype` on the CPU"""
    C, masked = case
    batch = _tail_batch()
    ins, ws = tail_inputs(case)[op]
    leaves = [v.to(dtype).clone().requires_grad_(True) for v in ins]
    with _one_thread():
        outs = _tail_oracle_op(op, leaves, masked, batch, len(TAIL_SIZES))
        sum((o * w.to(dtype)).sum() for o, w in zip(outs, ws)).backward()
    return [o.detach() for o in outs], [_grad(v) for v in leaves]


def _tail_hip_op(op, leaves, masked, batch, plan):
    from isubgvqa_amd import ops
    if op == "tail":
        ins, c, h, weight, bias, ms = leaves[:6]
        return (ops.mgat_layer_tail(ins, c, h, plan, weight, bias, ms, EPS, node_mask=leaves[6] if masked else None),)
    if op.startswith("pool"):
        out, gate = ops.global_attn_pool(leaves[0], leaves[1], plan, leaves[2] if masked else None)
        return (out, gate) if op == "pool out+gate" else (out,)
    if op == "instr gate":
        return (ops.instr_gate(leaves[0], leaves[1], batch, plan=plan),)
    return (ops.node_gate(leaves[0], leaves[1], batch, op == "node gate dbl", plan=plan),)


TAIL_LEAF_NAMES = {"tail": ("d ins", "d c", "d h", "d weight", "d bias", "d mean_scale", "d mask"),
                   "pool": ("d xn", "d q", "d mask"), "instr gate": ("d x", "d instr"), "node gate": ("d xn", "d q")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: f"C{c[0]}-{'masked' if c[1] else 'unmasked'}")
def test_tail_pool_and_gate_backward(dev, case):
    """Graphs of 63 / 64 / 65, 255 / 256 / 257 and 1024 nodes and two empty ones; widths on both sides of the 64- and
    128-thread steps and at the 1024-channel cap; a fractional node mask that is all zero on one graph; pooling with and
    without a gradient into the gate."""
    from isubgvqa_amd import ops
    C, masked = case
    batch = _tail_batch()
    B = len(TAIL_SIZES)
    plan = ops.GraphPlan.build(batch.to(dev), None, num_graphs=B)
    empty = [g for g, n in enumerate(TAIL_SIZES) if n == 0]
    judge = Judge(f"C={C} {'masked' if masked else 'unmasked'}", TAIL_CAP)
    for op in TAIL_OPS:
        ins, ws = tail_inputs(case)[op]
        o64, g64 = tail_oracle(case, op, torch.float64)
        o32, g32 = tail_oracle(case, op, torch.float32)
        leaves = [v.to(dev).requires_grad_(True) for v in ins]
        outs = _tail_hip_op(op, leaves, masked, batch.to(dev), plan)
        for i, (o, a, b) in enumerate(zip(outs, o64, o32)):
            judge(f"{op}: forward #{i}", o, a, b)
        sum((o * w.to(dev)).sum() for o, w in zip(outs, ws)).backward()
        names = TAIL_LEAF_NAMES[op.split(" out")[0] if op.startswith("pool") else op.replace(" dbl", "")]
        for name, v, a, b in zip(names, leaves, g64, g32):
            assert v.grad is not None, f"{op}: {name}"
            judge(f"{op}: {name}", v.grad, a, b)
        if op in ("tail", "instr gate") or op.startswith("pool"):      # the per-graph rows of an empty graph: exact zeros
            row = leaves[0].grad if op == "tail" else leaves[1].grad
            judge.zeros(f"{op}: rows of the empty graphs", row[empty], (len(empty), C))
    judge.done()


# ==========================================================================================================================
# Part 3: autograd.linear
# ==========================================================================================================================
LINEAR_SHAPES = [(5, 36, 20), (16383, 36, 20), (16384, 36, 20), (300, 128, 130), (300, 128, 131),
                 ("switch-1", 36, 20), ("switch", 36, 20)]     # the last two: both sides of autograd.WGRAD_MIN_ROWS
LINEAR_CASES = [(s, bias, gelu) for s in LINEAR_SHAPES for bias in (False, True) for gelu in (False, True)]


def _linear_rows(M):
    """The row count of a shape: a number, or a side of the switch of dW to the split-M kernel."""
    if isinstance(M, int):
        return M
    from isubgvqa_amd import autograd as AG
    return AG.WGRAD_MIN_ROWS - 1 if M == "switch-1" else AG.WGRAD_MIN_ROWS


def _linear_id(case):
    (M, K, N), bias, gelu = case
    return f"M{M}-K{K}-N{N}" + ("-bias" if bias else "") + ("-gelu" if gelu else "")


@functools.lru_cache(maxsize=None)
def linear_inputs(case):
    (M, K, N), bias, gelu = case
    M = _linear_rows(M)
    gen = torch.Generator().manual_seed(M + 3 * N + int(bias) + 2 * int(gelu))
    r = lambda *s: torch.randn(*s, generator=gen)
    return [r(M, K), r(N, K) / math.sqrt(K)] + ([r(N)] if bias else []), r(M, N)


@functools.lru_cache(maxsize=None)
def linear_oracle(case, dtype):
    _, bias, gelu = case
    ins, w = linear_inputs(case)
    leaves = [v.to(dtype).clone().requires_grad_(True) for v in ins]
    with _one_thread():
        z = leaves[0] @ leaves[1].t()
        if bias:
            z = z + leaves[2]
        y = torch.nn.functional.gelu(z) if gelu else z
        (y * w.to(dtype)).sum().backward()
    return y.detach(), [_grad(v) for v in leaves]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LINEAR_CASES, ids=_linear_id)
def test_linear_backward(dev, case):
    """dW on torch and on the split-M kernel (both sides of the switch, and of M = 16384 where the switch used to be), dX on
    the HIP kernel (N % 4 == 0) and on torch, GELU back-propagated through the kept pre-activation; against a float64
    matmul."""
    from isubgvqa_amd import autograd as AG
    _, bias, gelu = case
    ins, w = linear_inputs(case)
    y64, g64 = linear_oracle(case, torch.float64)
    y32, g32 = linear_oracle(case, torch.float32)
    leaves = [v.to(dev).requires_grad_(True) for v in ins]
    y = AG.linear(leaves[0], leaves[1], leaves[2] if bias else None, gelu)
    judge = Judge(_linear_id(case), LINEAR_CAP)
    judge("forward", y, y64, y32)
    (y * w.to(dev)).sum().backward()
    for name, v, a, b in zip(("dX", "dW", "db"), leaves, g64, g32):
        assert v.grad is not None, name
        judge(name, v.grad, a, b)
    judge.done()


# ==========================================================================================================================
# Host test: the shapes reach the branches they claim, and the reference alone is sound on every case
# ==========================================================================================================================
def _csr(case_topo):
    batch, ei, _ = topology(case_topo)
    N = batch.numel()
    indeg = torch.bincount(ei[1], minlength=N)
    outdeg = torch.bincount(ei[0], minlength=N)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), indeg.cumsum(0)])
    return N, ei, indeg, outdeg, rowptr


def test_topologies_reach_the_branches_they_claim():
    # ---- "hub": the global fall-back beyond MP_ECAP, parking across that boundary, degree-0 nodes, duplicates, a source hub
    N, ei, indeg, outdeg, rowptr = _csr("hub")
    assert N == sum(HUB_SIZES) == 57
    slots_block0 = int(rowptr[MP_NPB] - rowptr[0])
    assert slots_block0 > MP_ECAP, slots_block0
    assert int(rowptr[HUB_NODE]) < MP_ECAP < int(rowptr[HUB_NODE + 1])          # the hub's slots straddle the boundary
    assert int(rowptr[HUB_NODE]) + MP_LCAP < MP_ECAP                           # ... and are parked on both sides of it
    later = [i for i in range(HUB_NODE + 1, MP_NPB) if indeg[i] > 0]
    assert len(later) >= 10 and all(int(rowptr[i]) >= MP_ECAP for i in later)   # destinations read through global src / eid
    assert HUB_NODE < MP_NPB and int(indeg.max()) == int(indeg[HUB_NODE]) >= HUB_IN > MP_LCAP
    assert int(indeg[NO_IN]) == 0 and int(outdeg[NO_IN]) > 0
    assert int(outdeg[NO_OUT]) == 0 and int(indeg[NO_OUT]) > 0
    assert int(outdeg[SENDER]) >= SENDER_OUT
    key = ei[0] * N + ei[1]
    uniq, counts = torch.unique(key, return_counts=True)
    assert int((counts > 1).sum()) > 0
    assert sorted(ei[1].tolist()) != ei[1].tolist()                             # shuffled, not CSR order already
    assert {(H, C) for _, H, C, _, _ in HUB_CASES} == set(HUB_HC) and {H for H, _ in HUB_HC} == {1, 2, 4, 8}
    assert (8, 4) in HUB_HC                        # the narrowest row: parked pair and the lane's float4 share 16 bytes
    assert {mk for *_, mk, _ in HUB_CASES} == {"none", "node", "edge"}
    # ---- "small": a parked destination in every instantiation, every (H, P) enumerated
    N, ei, indeg, outdeg, rowptr = _csr("small")
    assert int(indeg.max()) > MP_LCAP and int(rowptr[MP_NPB] - rowptr[0]) <= MP_ECAP
    seen = {(H, passes(H, C)) for _, H, C, _, _ in SMALL_CASES}
    assert seen >= {(H, P) for H in (1, 2, 4, 8) for P in range(1, 9)}, sorted(seen)
    for H, C in SMALL_FULL:
        assert C % 4 == 0 and C // 4 == passes(H, C) * (64 // H)
    for H in (1, 2, 4, 8):
        assert any(h == H and (C // 4) % (64 // H) != 0 for h, C in SMALL_PARTIAL), H
    for _, H, C, _, _ in HUB_CASES + SMALL_CASES + EDGE_CASES:
        assert C % 4 == 0 and 1 <= passes(H, C) <= 8
    assert {s for *_, s in SMALL_CASES} >= {0.0, 0.2, 1.5}
    # ---- edge shapes
    assert topology("n16")[0].numel() == MP_NPB and topology("n17")[0].numel() == MP_NPB + 1
    assert topology("e0")[0].numel() > 0 and topology("e0")[1].size(1) == 0
    assert topology("n0")[0].numel() == 0 and topology("singles")[1].size(1) == 0
    # ---- masks: fractional, with exact zeros, -0.0, values above 1 and straight-through values beside 1
    for case in HUB_CASES:
        m = mp_inputs(case)["mask"]
        if m is not None:
            frac = float((m == 0).float().mean())
            assert 0.15 < frac < 0.45 and bool((torch.signbit(m) & (m == 0)).any()) and float(m.max()) > 1.25
            nz = m[m != 0]
            assert float(nz.min()) >= 0.25 and float(nz.max()) <= 1.75
            assert bool(((nz - 1).abs() < 1e-6).any())
    # ... and they leave the hub alive: m_e != 0 on in-slots of the hub on BOTH sides of slot MP_ECAP (what is parked there
    # is then not a row of zeros) and on out-edges of the source hub; a node mask is fractional and non-zero on both nodes
    N, ei, indeg, outdeg, rowptr = _csr("hub")
    slot_eid = torch.argsort(ei[1], stable=True)            # CSR by destination, ascending edge id inside a row (include/isg.h)
    hub_slots = torch.arange(int(rowptr[HUB_NODE]), int(rowptr[HUB_NODE + 1]))
    assert bool((ei[1][slot_eid[hub_slots]] == HUB_NODE).all())
    parked = hub_slots[MP_LCAP:]                            # the first MP_LCAP slots of a destination stay in LDS
    for case in HUB_CASES:
        if case[3] == "none":
            continue
        if case[3] == "node":
            m = mp_inputs(case)["mask"]
            assert float(m[HUB_NODE]) == HUB_MASK > 1 and 0 < float(m[SENDER]) == SENDER_MASK < 1
        live = edge_mask_of(case) != 0
        live_slots = live[slot_eid[parked]]
        below, beyond = live_slots[parked < MP_ECAP], live_slots[parked >= MP_ECAP]
        assert int(below.sum()) >= MIN_LIVE and int(beyond.sum()) >= MIN_LIVE, (_mp_id(case), int(below.sum()), int(beyond.sum()))
        assert int((~below).sum()) > 0 and int((~beyond).sum()) > 0        # masked-out slots on both sides too
        assert int(live[ei[0] == SENDER].sum()) >= MIN_LIVE, _mp_id(case)
    # ---- the reference alone: finite in float64 and float32 on every message-passing case
    for case in HUB_CASES + SMALL_CASES + EDGE_CASES:
        for dtype in (torch.float64, torch.float32):
            ref = mp_oracle(case, dtype)
            for v in [ref["out"]] + ref["grads"] + ([] if ref["d mask"] is None else [ref["d mask"]]):
                assert v.dtype == dtype and bool(torch.isfinite(v).all()), (_mp_id(case), dtype)
    # ---- tail shapes
    assert sum(TAIL_SIZES) == 2010 and max(TAIL_SIZES) == 1024 and TAIL_SIZES.count(0) == 2
    assert {63, 64, 65, 255, 256, 257} <= set(TAIL_SIZES) and {64, 68, 128, 132, 1024} <= set(TAIL_C)
    m = tail_inputs((4, True))["tail"][0][6]
    assert float(m[_tail_batch() == TAIL_ZERO_GRAPH].abs().max()) == 0.0 and TAIL_SIZES[TAIL_ZERO_GRAPH] > 0
    for op in TAIL_OPS:
        for dtype in (torch.float64, torch.float32):
            outs, grads = tail_oracle((68, True), op, dtype)
            assert all(v.dtype == dtype and bool(torch.isfinite(v).all()) for v in outs + grads), (op, dtype)
