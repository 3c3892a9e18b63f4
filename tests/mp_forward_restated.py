"""The GATv2 message-passing forward restated on the CPU: its formula, generic in the dtype, its kernel dispatch as a pure function,
and the case tables of tests/test_mp_forward_cases_cpu.py and tests/test_gpu_mp_forward_fp64.py.  Not a test module.

The formula (mgat_v2_conv.py:243-279 through oracle.model.gatv2_message_passing): every function takes `dt` and evaluates in it from
the same float32 (or half-rounded) inputs -- torch.float64 is the reference, torch.float32 the yardstick.  Nothing here knows a
summation order: segment sums are index_add.

The dispatch, from the constants of csrc/isg_mp.hpp, csrc/isg_mp.hip (mp_fwd, launch_mp) and csrc/isg_mp_graph.hip (launch_mp_graph,
launch_mp_graph_flat, launch_sized, launch_flat_sized) under the default environment (none of ENV_SWITCHES set):

    route(H, C, nmax, emax, B, rows_dtype, form, kernel, masked) ->
        ("grouped", HS, P, exact, "S" | "L", lrows) | ("flat", P, lrows) | ("chunk", H, P) | "unsupported"

`form` names the entry point: "rows" isg_gatv2_mp_fwd (half rows: _f16), "rowmax" _rowmax, "planes" _planes, "logits" _logits without
row maxima (half rows: _logits_f16), "logits_rowmax" _logits with them, "logits_planes" _logits_planes.  `kernel` is ops.gatv2_mp's
argument: "chunk" hands no per-graph arrays over.  "unsupported" is ISG_EUNSUPPORTED from that entry point.  `masked` chooses the
MASKED instantiation and nothing else; it is part of what a case covers (instantiation()).
"""
import functools
import math
from typing import NamedTuple

import torch

from test_gpu_backward_fp64 import fractional_mask

# ---- csrc/isg_mp.hpp, csrc/isg_mp_graph.hip ---------------------------------------------------------------------------------
MP_NPB, MP_ECAP, MP_LCAP = 16, 1024, 32
GK_NCAP_S, GK_ECAP_S, GK_NCAP_L, GK_ECAP_L = 64, 256, 256, 1024
GK_WAVES = 8
LDS_BUDGET = 40 * 1024          # ISG_MP_LDS_KB / ISG_MPF_LDS_KB default
SLICE_BYTES = 1280              # largest row slice of a workgroup of the grouped kernel
ENV_SWITCHES = ("ISG_MP_LDS_KB", "ISG_MPF_LDS_KB", "ISG_MP_FLAGS", "ISG_MP_FORCE_GRAPH", "ISG_MP_NO_FLAT")
FORMS = ("rows", "rowmax", "planes", "logits", "logits_rowmax", "logits_planes")
ST = 0.99999994                 # a straight-through mask's "one": 1 - 2^-24
SLOPE = 0.2


def _static_bytes(HS, ncap, ecap):
    return ecap * 16 + ecap * HS * 4 + (ncap + 4) * 4


def _window(HS, C, nmax, ncap, ecap):
    """lrows of launch_sized / launch_flat_sized, or None where the 8-row floor refuses the launch."""
    row, static = HS * C * 4, _static_bytes(HS, ncap, ecap)
    if LDS_BUDGET < static + 8 * row:
        return None
    return min((LDS_BUDGET - static) // row, nmax)


def heads_per_workgroup(H, C):
    for hs in (8, 4, 2, 1):
        if H % hs == 0 and hs * C * 4 <= SLICE_BYTES:
            return hs
    return 1


def _graph_route(H, C, nmax, emax, f16, form):
    """launch_mp_graph: a route, or None = ISG_EUNSUPPORTED (mp_fwd then looks at the node-chunk kernel)."""
    Q = C // 4
    if nmax <= 0 or nmax > GK_NCAP_L or emax < 0 or emax > GK_ECAP_L:
        return None
    HS = heads_per_workgroup(H, C)
    G = 64 // HS
    P = (Q + G - 1) // G
    if P > 2:
        return None
    rowmax, planes = form in ("rowmax", "logits_rowmax"), form in ("planes", "logits_planes")
    if HS == 1 and H > 1 and P == 2 and Q * 10 < G * P * 7:
        if rowmax:
            return None
        if f16 or nmax > GK_NCAP_S or emax > GK_ECAP_S or H % 2:
            return None
        if planes and H != 4:
            return None
        Pf = (2 * Q + 63) // 64
        if Pf not in (2, 3, 4):
            return None
        lrows = _window(2, C, nmax, GK_NCAP_S, GK_ECAP_S)
        return None if lrows is None else ("flat", Pf, lrows)
    if planes:
        return None
    small = nmax <= GK_NCAP_S and emax <= GK_ECAP_S
    lrows = _window(HS, C, nmax, *((GK_NCAP_S, GK_ECAP_S) if small else (GK_NCAP_L, GK_ECAP_L)))
    if lrows is None:
        return None
    return ("grouped", HS, P, Q == G * P, "S" if small else "L", lrows)


def route(H, C, nmax, emax, B, rows_dtype, form, kernel, masked):
    assert form in FORMS and kernel in ("graph", "chunk") and rows_dtype in (torch.float32, torch.float16)
    f16 = rows_dtype == torch.float16
    if H <= 0 or C <= 0 or C % 4:
        return "unsupported"
    if f16 and form not in ("rows", "logits"):
        return "unsupported"                                    # no such entry point
    if form in ("planes", "logits_planes") and H != 4:
        return "unsupported"
    if form.startswith("logits") and emax == 0:                 # E == 0
        return "unsupported"
    if kernel == "graph" and B > 0 and nmax > 0:
        r = _graph_route(H, C, nmax, emax, f16, form)
        if r is not None:
            return r
    if form != "rows" or f16:                                   # row maxima / logits in / planes / half rows: per-graph kernels only
        return "unsupported"
    if H not in (1, 2, 4, 8):
        return "unsupported"
    P = (C // 4 + 64 // H - 1) // (64 // H)
    return ("chunk", H, P) if P <= 8 else "unsupported"


def instantiation(r, masked, f16=False):
    """The template instantiation a route launches, as a hashable name (dropout instantiations are not this file's)."""
    if r == "unsupported":
        return None
    if r[0] == "chunk":
        return ("chunk", r[1], r[2])
    if r[0] == "flat":
        return ("flat", r[1], bool(masked))
    return ("grouped", r[1], r[2], r[3], r[4], bool(masked), bool(f16))


def all_instantiations():
    """Every instantiation without dropout the dispatch tables of the three kernels name."""
    out = {("chunk", H, P) for H in (1, 2, 4, 8) for P in range(1, 9)}
    out |= {("flat", P, m) for P in (2, 3, 4) for m in (False, True)}
    out |= {("grouped", HS, P, x, tab, m, f) for HS in (1, 2, 4, 8) for P in (1, 2) for x in (False, True) for tab in "SL"
            for m in (False, True) for f in (False, True)}
    return out


# Instantiations no supported input reaches (each grouped entry stands for its four MASKED x F16 instantiations, each flat entry for
# its two MASKED ones).  Why: EXACT at P = 2 needs C / 4 = 2 * 64 / HS, i.e. HS * C = 512 > 320 = the slice limit, unless HS = 1;
# on the 256 / 1024 tables the static LDS alone is 50 192 bytes at HS = 8 and 33 808 at HS = 4, and the launch needs 8 rows beside it
# inside 40 960: impossible at HS = 8, C <= 52 at HS = 4 (so neither P = 2 nor the exact C = 64); the flat rule admits 256 < C <= 356,
# where ceil(2 * (C / 4) / 64) = 3 always.  They are dead code under the default environment: ISG_MP_LDS_KB above 40 brings the
# grouped ones back, nothing brings back the flat P = 2 and P = 4.
UNREACHABLE = {
    "grouped": ((2, 2, True, "S"), (2, 2, True, "L"), (4, 2, True, "S"), (4, 2, True, "L"), (8, 2, True, "S"), (8, 2, True, "L"),
                (4, 1, True, "L"), (4, 2, False, "L"), (8, 1, False, "L"), (8, 1, True, "L"), (8, 2, False, "L")),
    "flat": (2, 4),
}


def unreachable_instantiations():
    out = {("grouped", *k, m, f) for k in UNREACHABLE["grouped"] for m in (False, True) for f in (False, True)}
    return out | {("flat", P, m) for P in UNREACHABLE["flat"] for m in (False, True)}


# ---- the formula ------------------------------------------------------------------------------------------------------------
def cast(dt, *ts):
    return tuple(None if t is None else t.detach().to(dt) for t in ts)


def edge_mask_of(dt, ei, node_mask=None, edge_mask=None):
    """[E, 1] in dt or None: the edge mask itself, or NodeMaskToEdgeMask's product of both ends (node_edge_masks.py:7-10)."""
    if edge_mask is not None:
        return cast(dt, edge_mask)[0].reshape(-1, 1)
    if node_mask is None:
        return None
    m = cast(dt, node_mask)[0].reshape(-1)
    return (m[ei[0]] * m[ei[1]]).reshape(-1, 1)


def logits_of(dt, x_l, x_r, e_proj, att, ei, H, C, em, slope=SLOPE):
    """[E, H]: att . leaky_relu((x_r[dst] + x_l[src] + e_proj) * m_e) * m_e, in edge-id order."""
    x_l, x_r, e_proj, att = cast(dt, x_l, x_r, e_proj, att)
    E = ei.size(1)
    x = (x_r[ei[1]] + x_l[ei[0]] + e_proj).view(E, H, C)
    if em is not None:
        x = x * em.unsqueeze(-1)
    x = torch.nn.functional.leaky_relu(x, slope)
    if em is not None:
        x = x * em.unsqueeze(-1)
    return (x * att.view(1, H, C)).sum(-1)


def row_maxima(out, H):
    return out.view(out.size(0), H, -1).abs().amax(2)


def forward(dt, t, ei, N, H, C, slope=SLOPE):
    """{"out" [N, H*C] with the bias, "alpha" [E, H], "logits" [E, H], "rowmax" [N, H]} of the inputs t in dt."""
    from oracle import model as OM
    E = ei.size(1)
    em = edge_mask_of(dt, ei, t.get("node_mask"), t.get("edge_mask"))
    x_l, x_r, e_proj, att, bias = cast(dt, t["x_l"], t["x_r"], t["e_proj"], t["att"], t["bias"])
    out, alpha = OM.gatv2_message_passing(x_l.view(N, H, C), x_r.view(N, H, C), e_proj.view(E, H, C), att.view(1, H, C), ei, em, slope)
    out = out.reshape(N, H * C) + bias
    return {"out": out, "alpha": alpha, "logits": logits_of(dt, x_l, x_r, e_proj, att, ei, H, C, em, slope), "rowmax": row_maxima(out, H)}


def from_logits(dt, logits, t, ei, N, H, C):
    """The same result from GIVEN logits [E, H] (edge-id order): softmax per destination with + 1e-16, alpha * m_e, aggregation of
    x_l rows, bias."""
    from oracle import primitives as P
    em = edge_mask_of(dt, ei, t.get("node_mask"), t.get("edge_mask"))
    lg, x_l, bias = cast(dt, logits, t["x_l"], t["bias"])
    alpha = P.pyg_softmax(lg, ei[1], N)
    w = alpha if em is None else alpha * em
    out = P.scatter_sum(x_l[ei[0]].view(-1, H, C) * w.unsqueeze(-1), ei[1], N).reshape(N, H * C) + bias
    return {"out": out, "alpha": alpha, "logits": lg, "rowmax": row_maxima(out, H)}


# ---- topologies -------------------------------------------------------------------------------------------------------------
NO_IN, NO_OUT, SINGLE = 1, 2, 3         # local nodes of every graph of at least 5 nodes: never a destination (and no self loop);
                                        # never a source (no self loop); exactly one in-edge, from node 0 (no self loop)


class Topo(NamedTuple):
    sizes: tuple                        # nodes per graph
    slots: dict = {}                    # graph -> exact number of CSR slots (in-edges) it is padded to
    hub: dict = {}                      # graph -> in-edges added to its local node 0
    extra: float = 2.0                  # random edges per node


TOPOLOGIES = {
    # 1-node graphs (the first with only its self loop), an empty graph in the middle, trailing ones; a 40-edge hub (beyond a wave's
    # LDS strip of MP_LCAP logits) in the 17-node graph; 35 slots = 3 (mod 4) in the 9-node graph
    "small": Topo((1, 1, 5, 0, 9, 17, 3, 0, 0), slots={4: 35}, hub={5: 40}),
    "n16": Topo((16,)),
    "n17": Topo((17,)),
    "e0": Topo((5, 3), extra=-1.0),
    # the small tables at their edge: 64 nodes and exactly 256 slots; windows of 14 rows (flat kernel, C = 300): 14 / 15 nodes
    "t64": Topo((64, 14, 15, 0, 3), slots={0: 256}, extra=1.5),
    # windows of 33 rows (HS = 2, C = 128, small tables) and 14 rows
    "win": Topo((33, 0, 34, 14, 15, 1), extra=1.5),
    "t65": Topo((65, 14, 15, 3), extra=1.0),                            # one node past the small tables
    "e257": Topo((64, 3), slots={0: 257}, extra=1.5),                   # one slot past them
    "t256": Topo((256, 14, 15), slots={0: 1024}, extra=1.0),            # the large tables at their edge
    "t257": Topo((257, 3), extra=1.0),                                  # one node past: the batch leaves the per-graph kernels
    "e1025": Topo((40, 3), slots={0: 1025}),                            # one slot past
    # 1100 in-edges on node 0 of a 20-node graph: the first 16-node block of the chunk kernel holds more than MP_ECAP slots and the
    # hub's segment straddles slot 1024
    "hub": Topo((20, 5), hub={0: 1100}),
}


def _draw(gen, n, ban=()):
    while True:
        v = int(torch.randint(0, n, (1,), generator=gen))
        if v not in ban:
            return v


@functools.lru_cache(maxsize=None)
def topology(name):
    """(batch [N], edge_index [2, E] in shuffled order, sizes): duplicate edges, self loops on all but the chosen nodes."""
    tp = TOPOLOGIES[name]
    gen = torch.Generator().manual_seed(100 + sorted(TOPOLOGIES).index(name))
    src, dst, off, lone = [], [], 0, True
    for g, n in enumerate(tp.sizes):
        first = len(src)
        add = lambda s, d: (src.append(off + s), dst.append(off + d))
        special = n >= 5
        no_src, no_dst = ((NO_OUT,), (NO_IN, SINGLE)) if special else ((), ())
        if tp.extra >= 0:
            for v in range(n):
                if not (special and v in (NO_IN, NO_OUT, SINGLE)):
                    add(v, v)
            if n == 1 and not lone:
                add(0, 0)                                       # the second one-node graph: its self loop twice
            lone = lone and n != 1
            if special:
                add(0, SINGLE), add(NO_IN, 0), add(4, NO_OUT)
            if n >= 2:
                add(n - 1, 0), add(0, n - 1), add(0, 0)         # the last node (beyond a window of n - 1 rows) as source; a duplicate
                for _ in range(int(tp.extra * n)):
                    add(_draw(gen, n, no_src), _draw(gen, n, no_dst))
                add(src[-1] - off, dst[-1] - off)               # a random edge twice
            for _ in range(tp.hub.get(g, 0)):
                add(_draw(gen, n, no_src), 0)
            want = tp.slots.get(g)
            if want is not None:
                assert len(src) - first <= want, (name, g, len(src) - first)
                while len(src) - first < want:
                    add(_draw(gen, n, no_src), _draw(gen, n, no_dst))
        off += n
    batch = torch.repeat_interleave(torch.arange(len(tp.sizes)), torch.tensor(tp.sizes, dtype=torch.long))
    ei = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    return batch, ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous(), tp.sizes


@functools.lru_cache(maxsize=None)
def csr(name):
    """The CSR by destination a GraphPlan holds, built with torch: {"rowptr" [N+1], "eid" [E] (stable in edge id), "deg" [N],
    "ptr" [B+1], "eptr" [B+1], "nmax", "emax", "B", "N", "E"}."""
    batch, ei, sizes = topology(name)
    N, E, B = batch.numel(), ei.size(1), len(sizes)
    deg = torch.bincount(ei[1], minlength=N)
    rowptr = torch.zeros(N + 1, dtype=torch.long)
    rowptr[1:] = deg.cumsum(0)
    ptr = torch.zeros(B + 1, dtype=torch.long)
    ptr[1:] = torch.tensor(sizes).cumsum(0)
    eptr = rowptr[ptr]
    return {"rowptr": rowptr, "eid": torch.sort(ei[1], stable=True).indices, "deg": deg, "ptr": ptr, "eptr": eptr, "N": N, "E": E,
            "B": B, "nmax": max(sizes), "emax": int((eptr[1:] - eptr[:-1]).max())}


# ---- classes ----------------------------------------------------------------------------------------------------------------
# "far" is "shift" at + 100: exp(100) is beyond float32, so a softmax without its `- mx` gives inf / inf there, where at + 32 it
# gives the right value to a few 1e-6 (exp(40) = 2e17 is an ordinary float)
CLASSES = ("plain", "sharp", "shift", "mask01", "edge01", "frac", "dead", "far")
MASK_OF = {"plain": None, "sharp": None, "shift": None, "mask01": "node", "edge01": "edge", "frac": "edge", "dead": "edge", "far": None}
SHARP, SHIFT, FAR, SHIFT_SCALE = 8.0, 32.0, 100.0, 0.25


def classes_of(topo):
    return ("plain", "mask01") if csr(topo)["E"] == 0 else CLASSES


def dead_parts(topo):
    """(the destination whose in-edges the "dead" class masks, the graph it masks completely or None)."""
    c = csr(topo)
    sizes = TOPOLOGIES[topo].sizes
    big = max(range(c["B"]), key=lambda g: sizes[g])
    rest = [g for g in range(c["B"]) if g != big and sizes[g] >= 2 and int(c["eptr"][g + 1] - c["eptr"][g]) > 0]
    return int(c["ptr"][big]), (rest[-1] if rest else None)


@functools.lru_cache(maxsize=None)
def inputs(topo, H, C, cls):
    """float32 inputs of one class: x_l, x_r [N, H*C], e_proj [E, H*C], att [1, H, C], bias [H*C], node_mask [N, 1] / edge_mask
    [E, 1] or None."""
    batch, ei, sizes = topology(topo)
    N, E = batch.numel(), ei.size(1)
    gen = torch.Generator().manual_seed(100000 * CLASSES.index(cls) + 1000 * H + C + 7 * sorted(TOPOLOGIES).index(topo))
    r = lambda *s: torch.randn(*s, generator=gen)
    t = {"x_l": r(N, H * C), "x_r": r(N, H * C), "e_proj": r(E, H * C), "att": r(1, H, C) / math.sqrt(C), "bias": r(H * C),
         "node_mask": None, "edge_mask": None}
    if cls == "sharp":
        t["att"] = t["att"] * SHARP
    elif cls in ("shift", "far"):   # every logit moves to about + SHIFT: x_r along sign(att), the rows scaled down so that a channel
        for k in ("x_l", "x_r", "e_proj"):                      # stays on the branch of the leaky ReLU its shift puts it on
            t[k] = t[k] * SHIFT_SCALE
        gain = t["att"].clamp(min=0).sum(2, keepdim=True) - SLOPE * t["att"].clamp(max=0).sum(2, keepdim=True)
        step = (SHIFT if cls == "shift" else FAR) / gain                                   # (channels of negative att sit on the ReLU's negative branch)
        t["x_r"] = t["x_r"] + (step * t["att"].sign()).reshape(1, H * C)
    elif cls == "mask01":
        m = (torch.rand(N, 1, generator=gen) > 0.4).float()
        m[(m > 0) & (torch.rand(N, 1, generator=gen) > 0.7)] = ST
        t["node_mask"] = m
    elif cls == "edge01":
        t["edge_mask"] = (torch.rand(E, 1, generator=gen) > 0.4).float()
    elif cls == "frac":
        t["edge_mask"] = fractional_mask(E, gen)
    elif cls == "dead":
        m = (torch.rand(E, 1, generator=gen) > 0.3).float()
        node, graph = dead_parts(topo)
        m[ei[1] == node] = 0.0
        if graph is not None:
            m[batch[ei[1]] == graph] = 0.0
        t["edge_mask"] = m
    return t


def half_rounded(t):
    return {k: (v.half().float() if k in ("x_l", "x_r", "e_proj") else v) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def reference(topo, H, C, cls, dt, half=False):
    """forward() of a case and class in dt; half: on the half-rounded feature rows."""
    batch, ei, _ = topology(topo)
    t = inputs(topo, H, C, cls)
    return forward(dt, half_rounded(t) if half else t, ei, batch.numel(), H, C)


@functools.lru_cache(maxsize=None)
def reference_from_logits(topo, H, C, cls, dt, half=False):
    """(the float64 formula's logits rounded to float32, from_logits() of them in dt)."""
    batch, ei, _ = topology(topo)
    t = inputs(topo, H, C, cls)
    lg = reference(topo, H, C, cls, torch.float64, half)["logits"].float()
    return lg, from_logits(dt, lg, half_rounded(t) if half else t, ei, batch.numel(), H, C)


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    family: str         # the kernel the "rows" form reaches: "chunk", "grouped", "flat"
    topo: str
    H: int
    C: int
    kernel: str         # ops.gatv2_mp's argument
    want: tuple         # what route() must say for fp32 rows, without lrows: the branch the case is there for

    @property
    def id(self):
        return f"{self.topo}-H{self.H}-C{self.C}-{self.kernel}"


# node-chunk kernel: every (H, P), the last pass full (odd P) or partly filled (even P: 4 channels short)
CHUNK_HP = [(H, P, 4 * P * (64 // H) - (4 if P % 2 == 0 else 0)) for H in (1, 2, 4, 8) for P in range(1, 9)]
CHUNK_CASES = [Case("chunk", "small", H, C, "chunk", ("chunk", H, P)) for H, P, C in CHUNK_HP]
CHUNK_CASES += [Case("chunk", topo, 4, 44, "chunk", ("chunk", 4, 1)) for topo in ("n16", "n17", "e0", "hub", "t65", "win")]
CHUNK_CASES += [Case("chunk", "hub", 8, 16, "chunk", ("chunk", 8, 1)), Case("chunk", "hub", 1, 300, "chunk", ("chunk", 1, 2))]
# ... and what leaves the per-graph kernels with kernel="graph": tables, the window's 8-row floor, 2 < P, the flat rule's leftovers
CHUNK_CASES += [Case("chunk", "t257", 4, 128, "graph", ("chunk", 4, 2)), Case("chunk", "e1025", 4, 128, "graph", ("chunk", 4, 2)),
                Case("chunk", "hub", 4, 32, "graph", ("chunk", 4, 1)), Case("chunk", "t65", 8, 16, "graph", ("chunk", 8, 1)),
                Case("chunk", "t65", 4, 72, "graph", ("chunk", 4, 2)), Case("chunk", "small", 1, 516, "graph", ("chunk", 1, 3)),
                Case("chunk", "t65", 4, 300, "graph", ("chunk", 4, 5)), Case("chunk", "small", 4, 300, "chunk", ("chunk", 4, 5))]

# grouped kernel: a width for every reachable (HS, P, exact); H = 3 and H = 16 have no node-chunk kernel behind them
GROUPED_WIDTHS = {(1, 1, False): (1, 100), (1, 1, True): (1, 256), (1, 2, False): (1, 300), (1, 2, True): (1, 512),
                  (2, 1, False): (2, 36), (2, 1, True): (4, 128), (2, 2, False): (2, 132),
                  (4, 1, False): (4, 32), (4, 1, True): (4, 64), (4, 2, False): (4, 72),
                  (8, 1, False): (8, 16), (8, 1, True): (8, 32), (8, 2, False): (8, 36)}
GROUPED_L = [k for k in GROUPED_WIDTHS if k[0] <= 2 or k == (4, 1, False)]
GROUPED_CASES = [Case("grouped", "small", *GROUPED_WIDTHS[k], "graph", ("grouped", *k, "S")) for k in GROUPED_WIDTHS]
GROUPED_CASES += [Case("grouped", "t65", *GROUPED_WIDTHS[k], "graph", ("grouped", *k, "L")) for k in GROUPED_L]
GROUPED_CASES += [
    Case("grouped", "small", 3, 20, "graph", ("grouped", 1, 1, False, "S")), Case("grouped", "small", 16, 8, "graph", ("grouped", 8, 1, False, "S")),
    Case("grouped", "small", 4, 360, "graph", ("grouped", 1, 2, False, "S")),          # just past the flat rule (Q = 90)
    Case("grouped", "n16", 4, 128, "graph", ("grouped", 2, 1, True, "S")), Case("grouped", "n17", 4, 128, "graph", ("grouped", 2, 1, True, "S")),
    Case("grouped", "e0", 4, 128, "graph", ("grouped", 2, 1, True, "S")),
    Case("grouped", "t64", 4, 128, "graph", ("grouped", 2, 1, True, "S")), Case("grouped", "t64", 8, 36, "graph", ("grouped", 8, 2, False, "S")),
    Case("grouped", "win", 4, 128, "graph", ("grouped", 2, 1, True, "S")), Case("grouped", "win", 2, 132, "graph", ("grouped", 2, 2, False, "S")),
    Case("grouped", "e257", 4, 32, "graph", ("grouped", 4, 1, False, "L")), Case("grouped", "e257", 1, 100, "graph", ("grouped", 1, 1, False, "L")),
    Case("grouped", "t256", 4, 128, "graph", ("grouped", 2, 1, True, "L")), Case("grouped", "t256", 1, 512, "graph", ("grouped", 1, 2, True, "L")),
]
# flat kernel (256 < C <= 356, H even): the edges of the rule, the reference's C = 300, two heads in all
FLAT_CASES = [Case("flat", topo, H, C, "graph", ("flat", 3)) for topo, H, C in
              [("small", 4, 300), ("small", 4, 260), ("small", 4, 356), ("small", 2, 268), ("small", 8, 300), ("t64", 4, 300),
               ("win", 4, 300), ("n16", 4, 300), ("e0", 4, 300)]]
CASES = CHUNK_CASES + GROUPED_CASES + FLAT_CASES

# the windows the issue names: lrows of (H, C) on the small and the large tables, and the graphs that sit at lrows / lrows + 1
WINDOWS = [("win", 4, 128, 33), ("win", 4, 300, 14), ("t64", 4, 300, 14), ("t65", 4, 128, 14), ("t256", 4, 128, 14)]


def case_route(case, form="rows", rows_dtype=torch.float32, masked=False):
    c = csr(case.topo)
    return route(case.H, case.C, c["nmax"], c["emax"], c["B"], rows_dtype, form, case.kernel, masked)
