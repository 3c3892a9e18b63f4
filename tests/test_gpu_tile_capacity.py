"""The graph-tile kernels on tiles filled to their caps: 64 nodes and 256 in-edge CSR slots (ops.TILE_CONV_NODES / TILE_CONV_EDGES).

The batches elsewhere in the suite add one self-loop and ~1.5 extra in-edges per node, so their tiles fill 64 nodes long before 256
slots.  Here a builder takes an explicit (nodes, slots) count per graph, so that the tiles reach the code that only runs near the slot
cap: the layer kernel's fourth 64-slot chunk (its next-tile request then comes mid-tile), tiles and nodes without in-edges, the
heaviest ordering class of `tiles_heavy_first`, and graphs that straddle either cap.  Each named batch checks its own fill, so an edit
to the builder cannot silently drop that coverage; the one CPU test checks the same fills with the host restatement of the packer."""
import math

import pytest
import torch

NCAP, ECAP = 64, 256


def G(nodes, slots, hub=None, loops=True):
    """One graph of `nodes` nodes and `slots` in-edges (= CSR slots).  loops: one self-loop per node (then slots >= nodes), the rest
    random pairs; hub: every edge beyond the self-loops goes into that node (None: destinations uniform)."""
    assert nodes >= 0 and slots >= (nodes if loops else 0) and (nodes > 0 or slots == 0)
    return (nodes, slots, hub, loops)


def capacity_topology(graphs, gen):
    """(batch [N], edge_index [2, E] in a shuffled order) of the graphs G(...) in the order given."""
    batch, src, dst, off = [], [], [], 0
    for g, (n, e, hub, loops) in enumerate(graphs):
        batch += [g] * n
        m = e
        if loops:
            src += range(off, off + n)
            dst += range(off, off + n)
            m -= n
        if m:
            src += (torch.randint(0, n, (m,), generator=gen) + off).tolist()
            dst += ([off + hub] * m) if hub is not None else (torch.randint(0, n, (m,), generator=gen) + off).tolist()
        off += n
    ei = torch.tensor([src, dst], dtype=torch.long).view(2, -1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    return torch.tensor(batch, dtype=torch.long), ei


def _groups_of_exactly(gen, count, slots=ECAP):
    """`count` runs of 1-6 consecutive graphs holding together at most 64 nodes and exactly `slots` slots: each run is one tile (the
    next graph has a slot, so it cannot join a full tile)."""
    out = []
    for _ in range(count):
        k = int(torch.randint(1, 7, (1,), generator=gen))
        n = torch.randint(1, NCAP // k + 1, (k,), generator=gen)
        e = n.clone()
        e += torch.bincount(torch.randint(0, k, (slots - int(n.sum()),), generator=gen), minlength=k)
        out += [G(int(a), int(b)) for a, b in zip(n, e)]
    return out


def named_graphs(name):
    """The graph lists of the capacity batches (deterministic)."""
    gen = torch.Generator().manual_seed({"exact": 1, "chunk": 2, "empty": 3, "dense": 4, "straddle": 5}[name])
    if name == "exact":          # every tile exactly 256 slots
        gs = [G(8, 32)] * 8                       # 64 nodes and 256 slots at once
        gs += [G(64, 256), G(2, 256, hub=0)]      # both caps by one graph; node 0 with in-degree 255
        gs += _groups_of_exactly(gen, 40)
        gs += [G(40, 256, hub=1)] + _groups_of_exactly(gen, 8)
        return gs
    if name == "chunk":          # 33+ nodes per graph: no two graphs share a tile, each graph's slots are its tile's
        gs = []
        for s in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255):
            gs.append(G(int(torch.randint(33, min(s, NCAP) + 1, (1,), generator=gen)), s))
            gs.append(G(33 + s % 31, s, loops=False))
        gs.append(G(40, 255, hub=1))     # node 1's segment: slots 1..216, across the 64-, 128- and 192-slot boundaries
        gs.append(G(36, 193, hub=35))    # the last node's segment reaches into the fourth chunk
        return gs
    if name == "empty":
        return [G(20, 130), G(20, 60), G(24, 66),
                G(20, 256, hub=5, loops=False),          # a full tile: 19 of 20 nodes without in-edges, before and after the hub
                G(64, 0, loops=False),                   # a tile with 64 nodes and no slot at all
                G(30, 200, loops=False), G(34, 56, hub=33, loops=False),      # 64 nodes, 256 slots, nodes without in-edges
                G(10, 100), G(10, 0, loops=False), G(10, 156),               # a graph without edges inside a full tile
                G(40, 0, loops=False), G(24, 0, loops=False),                # another tile without slots, between full ones
                G(3, 3), G(50, 253, hub=0)]
    if name == "dense":          # 4-24 nodes, 4-10 in-edges per node: tiles fill by slots; > 1024 graphs, > 2 x 256 tiles
        n = torch.randint(4, 25, (1500,), generator=gen)
        d = torch.randint(4, 11, (1500,), generator=gen)
        return [G(int(a), int(a * b)) for a, b in zip(n, d)]
    if name == "straddle":       # graphs at and just beyond either cap among small ones
        small = lambda k: [G(int(a), int(a) * 3) for a in torch.randint(4, 21, (k,), generator=gen)]
        return small(30) + [G(64, 256)] + small(30) + [G(64, 257)] + small(30) + [G(65, 200)] + small(30) + [G(40, 300)] + small(30)
    raise KeyError(name)


NAMES = ("exact", "chunk", "empty", "dense", "straddle")


def graph_counts(batch, ei, B):
    return torch.bincount(batch, minlength=B).tolist(), torch.bincount(batch[ei[1]], minlength=B).tolist()


def host_tiles(sizes, slots, ncap=NCAP, ecap=ECAP, chunk=1024):
    """Host restatement of isg_tile_plan's tile_info: greedy packing, a chunk of 1024 graphs closes a tile, a graph beyond a cap
    is a tile of its own without rows or slots."""
    info, g, B, r, e = [], 0, len(sizes), 0, 0
    while g < B:
        end_chunk = min((g // chunk + 1) * chunk, B)
        n, s, k = sizes[g], slots[g], g + 1
        while k < end_chunk and n + sizes[k] <= ncap and s + slots[k] <= ecap:
            n += sizes[k]; s += slots[k]; k += 1
        info.append([r, 0, e, 0] if (n > ncap or s > ecap) else [r, n, e, s])
        r += sum(sizes[g:k]); e += sum(slots[g:k])
        g = k
    return info


def heavy_first(info):
    """tiles_heavy_first's order: descending 32-slot class (capped at 8 = a full tile), ties in tile order."""
    return sorted(info, key=lambda w: -min((w[3] + 31) // 32, 8))


def check_fill(name, info, sizes, slots):
    """What each batch is for, from its tile descriptors [first node, nodes, first slot, slots]: returns the printed summary."""
    per = [w[3] for w in info]
    cls = [0] * 5          # tiles per 64-slot class: no slot, 1-64, 65-128, 129-192, 193-256
    for s in per:
        cls[(s + 63) // 64] += 1
    big = [g for g in range(len(sizes)) if sizes[g] > NCAP or slots[g] > ECAP]
    line = f"{name}: {len(info)} tiles, largest {max(per)} slots, per 64-slot class [0, 1-64, 65-128, 129-192, 193-256] {cls}"
    assert max(per) == (255 if name == "chunk" else ECAP), line
    if name == "exact":
        assert all(s == ECAP for s in per), line
        assert [NCAP, ECAP] in [w[1::2] for w in info], line                 # both caps in one tile
    if name == "chunk":
        want = sorted([63, 64, 65, 127, 128, 129, 191, 192, 193, 255] * 2 + [255, 193])
        assert sorted(per) == want, line
    if name == "empty":
        assert sum(1 for w in info if w[1] > 0 and w[3] == 0) == 2, line    # tiles with nodes and no slot
        assert sum(1 for s in per if s == ECAP) >= 3, line
        assert any(sizes[g] > 0 and slots[g] == 0 for g in range(len(sizes))), line
    if name == "dense":
        assert len(sizes) > 1024 and len(info) > 2 * 256, line
        assert cls[4] > len(info) // 2, line                                  # most tiles hold 193-256 slots
        assert sum(1 for s in per if s == ECAP) > 0, line                     # class 8 of the heavy-first order
        assert all(cls[1:]), line
    if name == "straddle":
        assert [(sizes[g], slots[g]) for g in big] == [(64, 257), (65, 200), (40, 300)], line
        assert sum(1 for w in info if w[1] == NCAP and w[3] == ECAP) == 1, line
    else:
        assert not big, line
    if name in ("exact", "chunk", "dense"):
        assert cls[0] == 0, line
    return line


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_capacity_batches_reach_their_fills_on_the_host_packer():
    """The builder's counts are the graphs' true counts, and every named batch reaches the fill it is meant to have."""
    for name in NAMES:
        graphs = named_graphs(name)
        batch, ei = capacity_topology(graphs, torch.Generator().manual_seed(7))
        sizes, slots = graph_counts(batch, ei, len(graphs))
        assert sizes == [g[0] for g in graphs] and slots == [g[1] for g in graphs], name
        assert torch.equal(batch[ei[0]], batch[ei[1]]), name                 # every edge inside its graph
        print(check_fill(name, host_tiles(sizes, slots), sizes, slots))


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    from isubgvqa_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_TOPO = {}


def capacity_batch(name):
    """(graphs, batch, edge_index, nodes per graph, slots per graph) of a named batch, built once per session."""
    if name not in _TOPO:
        graphs = named_graphs(name)
        batch, ei = capacity_topology(graphs, torch.Generator().manual_seed(7))
        _TOPO[name] = (graphs, batch, ei) + graph_counts(batch, ei, len(graphs))
    return _TOPO[name]


def device_fill(name, plan, sizes, slots):
    """isg_tile_plan's descriptors at the shipped caps equal the host packer's, and the batch reaches its fill."""
    _, nt, cap, info = plan.tiles(NCAP, ECAP)
    T = int(nt.item())
    got = info[:T].cpu().tolist()
    assert T <= cap and got == host_tiles(sizes, slots), name
    return check_fill(name, got, sizes, slots)


def _mixed_open():
    """The mixed mode's profitability gate open: the straddle batch is far smaller than the batches it pays for."""
    from isubgvqa_amd import ops
    return ops.configured(mixed_max_fraction=0.9, mixed_min_nodes=0)


def _layer_case(dev, name, H, K, mask, seed):
    """Inputs of one MaskingGATv2Conv on a capacity batch: node rows scaled per graph over nine binades (a destination's sources
    are in its graph, so its output row has that graph's magnitude), a small bias (a row's size is its own, not the bias')."""
    from isubgvqa_amd.models.layers import GlorotLinear
    graphs, batch, ei, sizes, slots = capacity_batch(name)
    gen = torch.Generator().manual_seed(seed)
    N, E, B, C = batch.numel(), ei.size(1), len(graphs), 128
    x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-4, 5, (B,), generator=gen).float())[batch][:, None]
    ea = torch.randn(E, K, generator=gen)
    w = torch.randn(H * C, K, generator=gen) * 0.1
    att, bias = torch.randn(1, H, C, generator=gen), torch.randn(H * C, generator=gen) * 2.0 ** -6
    nm = (torch.rand(N, generator=gen) < 0.7).float() if mask == "node" else None
    em = (torch.rand(E, generator=gen) < 0.7).float() if mask == "edge" else None
    torch.manual_seed(seed)
    lin_l, lin_r = GlorotLinear(128, H * C, bias=True), GlorotLinear(128, H * C, bias=True)
    with torch.no_grad():
        lin_l.bias.add_(0.1 * torch.randn(H * C, generator=gen))
        lin_r.bias.add_(0.1 * torch.randn(H * C, generator=gen))
    return dict(batch=batch, ei=ei, sizes=sizes, slots=slots, x=x, ea=ea, w=w, att=att, bias=bias, nm=nm, em=em,
                lin_l=lin_l.to(dev), lin_r=lin_r.to(dev), N=N, E=E, B=B, H=H, C=C)


def _run_chain(dev, cs, plan):
    """layer_conv, then linear_fused + tile_conv on the same input, then the edge-logits pair on the same x_l / x_r."""
    from isubgvqa_amd import ops
    d = lambda t: None if t is None else t.to(dev)
    H = cs["H"]
    xd, ead, wd, attd, bd, nmd, emd = d(cs["x"]), d(cs["ea"]), d(cs["w"]), d(cs["att"]), d(cs["bias"]), d(cs["nm"]), d(cs["em"])
    with torch.no_grad():
        lay = ops.gatv2_layer_conv(xd, cs["lin_l"], cs["lin_r"], ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd,
                                   want_rowmax=True)
        x_l, x_r = ops.linear_fused(xd, (cs["lin_l"], cs["lin_r"]))
        til = ops.gatv2_tile_conv(x_l, x_r, ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd, want_rowmax=True)
        pair = ops.gatv2_mp_edge_logits(x_l, x_r, ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd, want_rowmax=True)
        lg = ops.gatv2_edge_logits(x_l, x_r, ead, wd, attd, plan, H, node_mask=nmd, edge_mask=emd)
    assert lay is not None and til is not None and pair is not None and lg is not None
    return lay, til, pair, lg, x_l, x_r


def _assert_chain_equal(what, lay, til, pair, rows=None, edges=None):
    """EQUAL out, alpha and row maxima along layer_conv == linear_fused + tile_conv == the pair (on `rows` / `edges` only: the
    straddle batch's graphs beyond a tile run on the per-graph kernels from a projection of their own)."""
    from isubgvqa_amd import ops
    r = (lambda t: t) if rows is None else (lambda t: t[rows])
    e = (lambda t: t) if edges is None else (lambda t: t[edges])
    for (o1, a1), (o2, a2), tag in ((lay, til, "layer_conv vs linear_fused + tile_conv"), (til, pair, "tile_conv vs the pair")):
        assert torch.equal(r(o1), r(o2)), f"{what}: {tag}: out differs by {(r(o1) - r(o2)).abs().max().item():.3e}"
        assert torch.equal(e(a1), e(a2)), f"{what}: {tag}: alpha differs by {(e(a1) - e(a2)).abs().max().item():.3e}"
        assert torch.equal(r(ops.row_maxima(o1)), r(ops.row_maxima(o2))), f"{what}: {tag}: row maxima"


def _formula(cs, x_l, x_r, emask, dt):
    """att . leaky(x_r[dst] + x_l[src] + lin_edge(edge_attr)) with the mask before and after (mgat_v2_conv.py:253-271), per edge id."""
    src, dst = cs["ei"]
    E, H, C = cs["E"], cs["H"], cs["C"]
    z = (x_r.to(dt)[dst] + x_l.to(dt)[src]) + cs["ea"].to(dt) @ cs["w"].to(dt).t()
    if emask is not None:
        z = z * emask.to(dt)[:, None]
    z = torch.nn.functional.leaky_relu(z, 0.2)
    if emask is not None:
        z = z * emask.to(dt)[:, None]
    return (z.view(E, H, C) * cs["att"].to(dt).view(1, H, C)).sum(-1)


def _softmax(lg, dst, N):
    """Softmax over every destination's in-edges, + 1e-16 in the denominator like the kernels (pyg_softmax)."""
    idx = dst[:, None].expand(-1, lg.size(1))
    mx = torch.full((N, lg.size(1)), -float("inf"), dtype=lg.dtype).scatter_reduce(0, idx, lg, "amax")
    ex = (lg - mx[dst]).exp()
    return ex / (torch.zeros(N, lg.size(1), dtype=lg.dtype).index_add(0, dst, ex)[dst] + 1e-16)


def _aggregate(cs, alpha, x_l, emask, dt):
    """(sum over in-edges of alpha * mask * x_l[src] + bias, the same sum of absolute values: each row's own magnitude)."""
    src, dst = cs["ei"]
    N, E, H, C = cs["N"], cs["E"], cs["H"], cs["C"]
    wgt = alpha.to(dt) if emask is None else alpha.to(dt) * emask.to(dt)[:, None]
    msg = x_l.to(dt)[src].view(E, H, C) * wgt[:, :, None]
    b = cs["bias"].to(dt).view(1, H, C)
    out = torch.zeros(N, H, C, dtype=dt).index_add(0, dst, msg) + b
    mag = torch.zeros(N, H, C, dtype=dt).index_add(0, dst, msg.abs()) + b.abs()
    return out, mag


def _check_fp64(what, cs, plan, out, alpha, lg, x_l, x_r):
    """The tile kernels' results against an fp64 evaluation of the same layer on the same x_l / x_r, bounded by what a plain fp32
    evaluation of it loses (the yardsticks of test_gpu_ops.py::test_edge_logits_pair_matches_the_unfused_kernels_and_the_oracle),
    out per (row, head) relative to that row's own magnitude.  Returns the measured numbers."""
    from isubgvqa_amd import ops
    N, E, H, C = cs["N"], cs["E"], cs["H"], cs["C"]
    src, dst = cs["ei"]
    emask = cs["em"] if cs["em"] is not None else (None if cs["nm"] is None else cs["nm"][src] * cs["nm"][dst])
    xl, xr = x_l.cpu(), x_r.cpu()
    ref64, ref32 = _formula(cs, xl, xr, emask, torch.float64), _formula(cs, xl, xr, emask, torch.float32)
    eid = plan.eid.cpu().long()
    e_k = (lg.cpu().double() - ref64[eid]).abs().max().item()
    e_32 = (ref32.double() - ref64).abs().max().item()
    a64 = _softmax(ref64, dst, N)
    a32s = _softmax(ref32, dst, N)
    a_32 = (a32s.double() - a64).abs().max().item()
    da = (alpha.cpu().double() - a64).abs()
    a_k = da.max().item()
    # alpha as far off as the kernel's own logits allow: alpha_j = exp(l_j - lse), so a logit error of at most e_k moves alpha_j by
    # a factor within exp(+-2 e_k); the softmax itself (exp2, reciprocal, the sum of up to 256 terms) adds 1e-5 of it, + 3e-6
    a_lim = a64 * (math.expm1(2.0 * e_k) + 1e-5) + 3e-6
    a_rel = (da / a_lim).max().item()
    o64, mag = _aggregate(cs, a64, xl, emask, torch.float64)
    o32, _ = _aggregate(cs, a32s, xl, emask, torch.float32)
    mag = mag.amax(2).clamp_min(1e-30)
    rel = lambda o: ((o.double().view(N, H, C) - o64).abs().amax(2) / mag).max().item()
    o_k, o_32 = rel(out.cpu()), rel(o32)
    nums = {"logit_err": e_k, "logit_err_fp32": e_32, "alpha_err": a_k, "alpha_err_fp32": a_32, "alpha_err_over_bound": a_rel,
            "out_rel_err": o_k, "out_rel_err_fp32": o_32}
    print(f"    {what}: logits {e_k:.2e} (fp32 {e_32:.2e}), alpha {a_k:.2e} (fp32 {a_32:.2e}; {a_rel:.2f} of its bound), "
          f"out per row {o_k:.2e} (fp32 {o_32:.2e})")
    assert e_k <= 2.0 * e_32 + 1e-6, (what, nums)
    # (not 2 x the fp32 softmax's own loss: with logits up to |500| the kernel's logit error is an fp32 formula's, and two draws of
    # that rounding differ by 3x in the alpha they give -- the bound above follows alpha from the logits instead)
    assert a_rel <= 1.0 and a_k <= 4.0 * a_32 + 3e-6, (what, nums)
    assert o_k <= max(4.0 * o_32, 1e-5), (what, nums)
    assert torch.equal(ops.row_maxima(out), out.view(N, H, C).abs().amax(2)), what
    lonely = torch.bincount(dst, minlength=N) == 0          # no in-edge: exactly the bias
    if bool(lonely.any()):
        got = out.cpu()[lonely]
        assert torch.equal(got, cs["bias"].expand_as(got)), what
    return nums


FP64_BATCHES = ("exact", "chunk", "empty", "straddle")     # (dense: ~150 000 slots, bit equality only)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [None, "node", "edge"])
@pytest.mark.parametrize("H,K", [(4, 128), (4, 36), (2, 128), (2, 36), (1, 128), (1, 36)])
def test_layer_and_tile_conv_at_capacity_match_the_pair_and_fp64(dev, mask, H, K):
    """gatv2_layer_conv == linear_fused + gatv2_tile_conv == the edge-logits pair bit for bit, and against fp64, on every capacity
    batch (straddle with the mixed mode's gate open: its graphs beyond a tile go to the per-graph kernels).  The projection runs on
    isg_linear_f16x3 (the panel kernel at every M, no small-batch kernel), the form the layer kernel restates."""
    from isubgvqa_amd import ops
    with ops.configured(skinny=False, gemm_kernel="panel", rows_kernel_min_edges=0, h3p_min_m=8192), _mixed_open():
        for i, name in enumerate(FP64_BATCHES + ("dense",)):
            if name == "dense" and (mask, H, K) not in ((None, 4, 128), ("edge", 2, 36), ("node", 1, 128)):
                continue
            cs = _layer_case(dev, name, H, K, mask, 1000 + 10 * i + H + K)
            plan = ops.GraphPlan.build(cs["batch"].to(dev), cs["ei"].to(dev), num_graphs=cs["B"])
            line = device_fill(name, plan, cs["sizes"], cs["slots"])
            assert ops.layer_conv_supported(plan, H, cs["C"], 128, K), name
            assert plan.tile_mode(NCAP, ECAP) == ("mixed" if name == "straddle" else "tiles"), name
            lay, til, pair, lg, x_l, x_r = _run_chain(dev, cs, plan)
            print(f"{line}; H={H} K={K} mask={mask}")
            rows = edges = None
            if name == "straddle":
                sub = plan.oversize(NCAP, ECAP)
                assert sub.gids.cpu().tolist() == [g for g in range(cs["B"]) if cs["sizes"][g] > NCAP or cs["slots"][g] > ECAP]
                keep = torch.ones(cs["N"], dtype=torch.bool)
                keep[sub.nodes.cpu()] = False
                rows, edges = keep.to(dev), keep[cs["ei"][1]].to(dev)
            _assert_chain_equal(name, lay, til, pair, rows, edges)
            if name != "dense":
                _check_fp64(name, cs, plan, lay[0], lay[1], lg, x_l, x_r)


@pytest.mark.gpu
def test_capacity_order_and_repeatability(dev):
    """On the dense batch: the order tiles_heavy_first returns is the host restatement (class 8 included); the layer and tile kernels
    give the same bits with the heavy-first order on and off, and on a second launch."""
    from isubgvqa_amd import ops
    with ops.configured(skinny=False, gemm_kernel="panel", rows_kernel_min_edges=0, h3p_min_m=8192):
        cs = _layer_case(dev, "dense", 4, 128, "edge", 77)
        plan = ops.GraphPlan.build(cs["batch"].to(dev), cs["ei"].to(dev), num_graphs=cs["B"])
        print(device_fill("dense", plan, cs["sizes"], cs["slots"]))
        T = int(plan.tiles(NCAP, ECAP)[1].item())
        info = host_tiles(cs["sizes"], cs["slots"])
        heavy = plan.tiles_heavy_first(NCAP, ECAP)[:T].cpu().tolist()
        assert heavy == heavy_first(info)
        assert sum(1 for w in heavy if w[3] == ECAP) > 0 and heavy[0][3] > 224
        with ops.configured(tile_heavy_first=False):
            assert plan.tiles_heavy_first(NCAP, ECAP)[:T].cpu().tolist() == info
            off = _run_chain(dev, cs, plan)
        on1 = _run_chain(dev, cs, plan)
        on2 = _run_chain(dev, cs, plan)
    for other, tag in ((off, "heavy-first off"), (on2, "second launch")):
        for k in range(3):          # layer_conv, tile_conv, pair: (out, alpha)
            assert torch.equal(on1[k][0], other[k][0]) and torch.equal(on1[k][1], other[k][1]), (tag, k)
            assert torch.equal(ops.row_maxima(on1[k][0]), ops.row_maxima(other[k][0])), (tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize("masked,with_next", [(False, True), (True, True)])
def test_dense_tail_on_capacity_plans(dev, masked, with_next):
    """isg_mgat_dense_tail on tiles filled by slots (few nodes per tile) against the un-fused chain and the CPU oracle."""
    from test_gpu_ops import _dense_tail_case
    for i, name in enumerate(("exact", "chunk", "empty", "dense")):
        graphs, batch, ei, sizes, slots = capacity_batch(name)
        assert _dense_tail_case(dev, sizes, 300 + i, masked, with_next, topology=(batch, ei)) is not None, name


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_readout_tile_on_capacity_plans(dev, masked):
    """isg_readout_tile on capacity plans against ops.mlp + isg_global_attn_pool and the CPU oracle's GlobalAttention."""
    from isubgvqa_amd import ops
    from isubgvqa_amd.models import GlobalAttention
    from oracle import model as OM
    gen = torch.Generator().manual_seed(51)
    torch.manual_seed(3)
    pool = GlobalAttention(128, 128)
    with torch.no_grad():
        for p in pool.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    sd = {"p." + k: v.detach().clone() for k, v in pool.state_dict().items()}
    pool = pool.to(dev).eval()
    for name in ("exact", "chunk", "empty", "dense"):
        graphs, batch, ei, sizes, slots = capacity_batch(name)
        N, B = batch.numel(), len(graphs)
        x = torch.randn(N, 128, generator=gen) * torch.rand(N, 1, generator=gen).mul(3).exp()
        u = torch.randn(B, 128, generator=gen)
        mask = (torch.rand(N, 1, generator=gen) < 0.6).float() if masked else None
        plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
        d = lambda t: None if t is None else t.to(dev)
        with torch.no_grad():
            assert ops.readout_tile_supported(plan, pool.node_nn, 128), name
            out, gate = pool(d(x), d(u), batch.to(dev), return_mask=True, node_mask=d(mask), plan=plan)
            xn = ops.mlp(pool.node_nn, d(x))
            ref_out, ref_gate = ops.global_attn_pool(xn.contiguous(), ops.mlp(pool.ques_nn, d(u)).contiguous(), plan, d(mask))
            want_out, want_gate = OM.global_attention_forward(sd, "p", x, u, batch, mask, size=B)
        scale = max(want_out.abs().max().item(), 1.0)
        e_or, e_un = (out.cpu() - want_out).abs().max().item(), (ref_out.cpu() - want_out).abs().max().item()
        print(f"readout {name}: vs oracle {e_or:.2e}, un-fused vs oracle {e_un:.2e}")
        assert e_or <= max(2e-5 * scale, 3.0 * e_un), (name, e_or, e_un)
        assert e_or <= 1e-4 * scale, (name, e_or, scale)
        assert (gate.cpu().view(-1) - want_gate.view(-1)).abs().max().item() <= 2e-5, name
        assert torch.allclose(out, ref_out, atol=1e-4 * scale, rtol=0) and torch.allclose(gate, ref_gate, atol=2e-5, rtol=0), name


@pytest.mark.gpu
def test_tile_plan_and_edge_planes_as_one_launch_at_capacity(dev):
    """isg_tile_plan_edge_planes (one launch) against isg_tile_plan + isg_edge_planes on every capacity batch: every output equal."""
    from isubgvqa_amd import ops
    gen = torch.Generator().manual_seed(61)
    for name in NAMES:
        graphs, batch, ei, sizes, slots = capacity_batch(name)
        B, E = len(graphs), ei.size(1)
        ea = torch.randn(E, 128, generator=gen).to(dev)
        p1 = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
        p2 = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
        (tp1, nt1, cap1, info1), (pl1, inv1) = p1.tiles_and_edge_planes(ea, NCAP, ECAP)
        print(device_fill(name, p2, sizes, slots))
        tp2, nt2, cap2, info2 = p2.tiles(NCAP, ECAP)
        pl2, inv2 = p2.edge_planes(ea)
        T = int(nt1.item())
        assert T == int(nt2.item()) and cap1 == cap2, name
        assert torch.equal(tp1[:T + 1], tp2[:T + 1]) and torch.equal(info1[:T], info2[:T]), name
        assert torch.equal(p1.tiles_heavy_first(NCAP, ECAP)[:T], p2.tiles_heavy_first(NCAP, ECAP)[:T]), name
        assert torch.equal(pl1[:E], pl2[:E]) and torch.equal(inv1[:E], inv2[:E]), name


def capacity_workload(name, graphs_count=None, seed=0):
    """A synthetic.Workload (C = 128, 3 layers) on a capacity batch's topology, the first `graphs_count` graphs of it."""
    from isubgvqa_amd import synthetic
    graphs = named_graphs(name)[:graphs_count]
    gen = torch.Generator().manual_seed(seed)
    batch, ei = capacity_topology(graphs, gen)
    B, N, E, C, L = len(graphs), batch.numel(), ei.size(1), 128, 3
    sizes = torch.stack([torch.bincount(batch, minlength=B), torch.bincount(batch[ei[1]], minlength=B)])
    return synthetic.Workload(torch.randn(N, C, generator=gen), ei, torch.randn(E, C, generator=gen), batch,
                              torch.randn(L, B, C, generator=gen), torch.randn(B, C, generator=gen), B, int(sizes[0].max()),
                              int(sizes[1].max()), sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["gumbel", "imle"])
def test_model_on_a_dense_capacity_batch_matches_the_oracle(dev, sampler):
    """AnswerModel (C = 128, 3 layers) on 800 graphs of the dense batch against OM.mgat_pool_classify: top-k masks bit-exact, logits
    < LOGIT_TOL, gate to 1e-5, and every node through the tile kernels (3 layer kernels, 3 dense tails, the read-out)."""
    from isubgvqa_amd import ops, synthetic
    from test_gpu_models import LOGIT_TOL, _run_both_wl
    wl = capacity_workload("dense", 800, seed=11)
    cfg = synthetic.WorkloadConfig(num_graphs=wl.num_graphs, channels=128, layers=3, sampler=sampler, seed=13)
    plan = ops.GraphPlan.build(wl.batch.to(dev), wl.edge_index.to(dev), num_graphs=wl.num_graphs)
    info = plan.tiles(NCAP, ECAP)[3][:int(plan.tiles(NCAP, ECAP)[1].item())].cpu()
    assert int((info[:, 3] > 192).sum()) > info.size(0) // 2 and int(info[:, 3].max()) == ECAP
    ops.reset_counters()
    (rl, rm, rg), (gl, gm, gg) = _run_both_wl(cfg, wl, dev)
    c = ops.counters()
    err = (gl - rl).abs().max().item()
    print(f"dense capacity batch, {sampler}: {wl.x.size(0)} nodes, {wl.edge_index.size(1)} edges, max |logit diff| {err:.2e}, {c}")
    assert c["tile_nodes"] == 7 * wl.x.size(0) and c["oversize_nodes"] == 0, c
    assert torch.equal(gm > 0.5, rm > 0.5), "top-k mask indices must be bit-exact"
    assert err < LOGIT_TOL
    assert torch.allclose(gg, rg, atol=1e-5)


@pytest.mark.gpu
def test_model_on_the_straddle_batch_under_mixed_dispatch(dev):
    """The straddle batch under mixed dispatch: (64, 256) stays on the tile kernels, (64, 257), (65, 200) and (40, 300) -- a graph
    within the node cap beyond the slot cap -- go to the per-graph kernels; logits, masks and gate against the oracle."""
    from isubgvqa_amd import ops, synthetic
    from test_gpu_models import LOGIT_TOL, _forced_mixed, _run_both_wl
    wl = capacity_workload("straddle", seed=12)
    cfg = synthetic.WorkloadConfig(num_graphs=wl.num_graphs, channels=128, layers=3, sampler="imle", seed=14)
    sizes, slots = wl.graph_sizes.tolist()
    big = [g for g in range(wl.num_graphs) if sizes[g] > NCAP or slots[g] > ECAP]
    assert [(sizes[g], slots[g]) for g in big] == [(64, 257), (65, 200), (40, 300)]
    plan = _forced_mixed(lambda: ops.GraphPlan.build(wl.batch.to(dev), wl.edge_index.to(dev), num_graphs=wl.num_graphs))
    assert _forced_mixed(lambda: plan.tile_mode(NCAP, ECAP)) == "mixed"
    assert plan.oversize(NCAP, ECAP).gids.cpu().tolist() == big
    ops.reset_counters()
    (rl, rm, rg), (gl, gm, gg) = _forced_mixed(lambda: _run_both_wl(cfg, wl, dev))
    c = ops.counters()
    n_big = sum(sizes[g] for g in big)
    print(f"straddle batch under mixed dispatch: {c}")
    # every tile-kernel call counts the nodes of the graphs beyond a tile as the per-graph kernels'; those are exactly the three
    assert c["oversize_nodes"] > 0 and c["oversize_nodes"] % n_big == 0, c
    assert c["tile_nodes"] == (c["oversize_nodes"] // n_big) * (wl.x.size(0) - n_big), c
    assert torch.equal(gm > 0.5, rm > 0.5)
    assert (gl - rl).abs().max() < LOGIT_TOL, (gl - rl).abs().max()
    assert (gl[big] - rl[big]).abs().max() < LOGIT_TOL
    assert torch.allclose(gg, rg, atol=1e-5)
