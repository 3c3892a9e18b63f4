"""isg_gatv2_layer_conv's masked launches walk only the live slots: a slot whose mask is +-0 has the logit +0 and
leaves its destination's sum unchanged, so skipping its edge product, logit epilogue and aggregation product changes no bit.

Every case runs twice, in two child processes (the wrapper reads ISG_LC_DENSE_MASK once per process): the live-slot walk and
ISG_LC_DENSE_MASK=1, the walk over every slot.  out, alpha and the row maxima must be EQUAL, and the live-slot walk must also equal
linear_fused + gatv2_tile_conv, which the kernel is documented to equal.  The batches reach the cases the compaction has edges at:
no live slot, every slot live (tiles of 256 slots), one live slot per tile, live slots only in a tile's last 64-slot chunk, live
counts of 32 / 33 / 64 / 65 in a tile (the half-chunk and chunk edges), fractional and straight-through masks, -0.0, destinations
without in-edges and graphs without a picked node."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCAP, ECAP = 64, 256


# ----------------------------------------------------------------------------------------------------------------- batches
def topology(graphs, gen):
    """(batch [N], edge_index [2, E] shuffled) of graphs given as (nodes, in-edges, self-loops?): with self-loops every node has an
    in-edge, the rest are random pairs inside the graph."""
    batch, src, dst, off = [], [], [], 0
    for g, (n, e, loops) in enumerate(graphs):
        batch += [g] * n
        m = e
        if loops:
            src += range(off, off + n)
            dst += range(off, off + n)
            m -= n
        if m:
            src += (torch.randint(0, n, (m,), generator=gen) + off).tolist()
            dst += (torch.randint(0, n, (m,), generator=gen) + off).tolist()
        off += n
    ei = torch.tensor([src, dst], dtype=torch.long).view(2, -1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    return torch.tensor(batch, dtype=torch.long), ei


def full_tiles(gen, count):
    """`count` runs of 1-6 graphs holding together <= 64 nodes and exactly 256 slots (each run is one tile)."""
    out = []
    for _ in range(count):
        k = int(torch.randint(1, 7, (1,), generator=gen))
        n = torch.randint(1, NCAP // k + 1, (k,), generator=gen)
        e = n.clone() + torch.bincount(torch.randint(0, k, (ECAP - int(n.sum()),), generator=gen), minlength=k)
        out += [(int(a), int(b), True) for a, b in zip(n, e)]
    return out


def dense_graphs(gen, count):
    """4-24 nodes, 4-10 in-edges per node: tiles fill by slots, most past 192."""
    n = torch.randint(4, 25, (count,), generator=gen)
    d = torch.randint(4, 11, (count,), generator=gen)
    return [(int(a), int(a * b), True) for a, b in zip(n, d)]


def sparse_graphs(gen, count):
    """Graphs without self-loops and with few edges: many destinations without an in-edge."""
    n = torch.randint(2, 30, (count,), generator=gen)
    return [(int(a), int(torch.randint(0, int(a) + 1, (1,), generator=gen)), False) for a in n]


def straight_through(khot, picked):
    """The sampler's value (hard - khot) + khot in fp32: exactly +0 where not picked, 1 +- an ulp or so where picked."""
    hard = picked.float()
    return (hard - khot) + khot


def tile_slots(batch, ei, B):
    """Host tile plan (isg_tile_plan's greedy packing, 1024-graph chunks) -> per tile (first slot, slots) in CSR slot order, and the
    CSR order itself: slot -> edge id (destination-major, edge id order within a destination)."""
    sizes = torch.bincount(batch, minlength=B).tolist()
    slots = torch.bincount(batch[ei[1]], minlength=B).tolist()
    tiles, g, e = [], 0, 0
    while g < B:
        end = min((g // 1024 + 1) * 1024, B)
        n, s, k = sizes[g], slots[g], g + 1
        while k < end and n + sizes[k] <= NCAP and s + slots[k] <= ECAP:
            n += sizes[k]; s += slots[k]; k += 1
        if n <= NCAP and s <= ECAP:
            tiles.append((e, s))
        e += sum(slots[g:k])
        g = k
    order = torch.argsort(ei[1] * ei.size(1) + torch.arange(ei.size(1)))
    return tiles, order


def edge_mask_from_slots(ei, B, batch, pick):
    """An edge mask that is 1 exactly on the slots pick(tile index, slots in the tile, generator) returns, per tile."""
    tiles, order = tile_slots(batch, ei, B)
    em = torch.zeros(ei.size(1))
    gen = torch.Generator().manual_seed(11)
    for t, (e0, ne) in enumerate(tiles):
        for j in pick(t, ne, gen):
            em[order[e0 + j]] = 1.0
    return em


def case_inputs(name):
    """(batch, edge_index, B, node_mask or None, edge_mask or None) of a named case (deterministic)."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "bench":            # BASELINE configs[1]'s masked layer: k = 5 of each graph's nodes, straight-through values
        from isubgvqa_amd import synthetic
        wl = synthetic.make_workload(synthetic.CFG2)
        batch, ei, B = wl.batch, wl.edge_index, wl.num_graphs
        sizes = torch.bincount(batch, minlength=B)
        score = torch.rand(batch.numel(), generator=gen)
        rank = torch.empty_like(score)
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
        for g in range(B):
            s = score[ptr[g]:ptr[g + 1]]
            rank[ptr[g]:ptr[g + 1]] = torch.argsort(torch.argsort(s, descending=True)).float()
        khot = torch.rand(batch.numel(), generator=gen) * 0.9 + 0.05
        return batch, ei, B, straight_through(khot, rank < 5), None
    if name in ("zeros", "ones", "fractional", "negzero", "edge_random"):
        graphs = full_tiles(gen, 12) + dense_graphs(gen, 300) + sparse_graphs(gen, 60)
        batch, ei = topology(graphs, gen)
        B, N, E = len(graphs), batch.numel(), ei.size(1)
        if name == "zeros":
            return batch, ei, B, torch.zeros(N), None
        if name == "ones":
            return batch, ei, B, torch.ones(N), None
        if name == "fractional":   # 0, 0.5, 1 - 2^-24, 1 + 2^-23, 1
            vals = torch.tensor([0.0, 0.5, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0])
            return batch, ei, B, vals[torch.randint(0, 5, (N,), generator=gen)], None
        if name == "negzero":      # unpicked nodes at -0.0, some at +0.0
            m = torch.where(torch.rand(N, generator=gen) < 0.3, 1.0, -0.0)
            m = torch.where(torch.rand(N, generator=gen) < 0.2, torch.zeros(N), m)
            return batch, ei, B, m, None
        return batch, ei, B, None, (torch.rand(E, generator=gen) < 0.7).float()
    if name == "graphs_unpicked":  # whole graphs without a picked node, destinations without in-edges
        graphs = sparse_graphs(gen, 200) + dense_graphs(gen, 100)
        batch, ei = topology(graphs, gen)
        B, N = len(graphs), batch.numel()
        keep = (torch.rand(B, generator=gen) < 0.5)[batch]
        return batch, ei, B, (keep & (torch.rand(N, generator=gen) < 0.4)).float(), None
    graphs = full_tiles(gen, 16) + dense_graphs(gen, 400)
    batch, ei = topology(graphs, gen)
    B = len(graphs)
    if name == "one_per_tile":
        pick = lambda t, ne, g: [int(torch.randint(0, ne, (1,), generator=g))] if ne else []
    elif name == "last_chunk":     # only in the tile's last 64-slot chunk (tiles of more than 192 slots: the fourth)
        pick = lambda t, ne, g: [j for j in range(64 * ((ne - 1) // 64), ne) if torch.rand(1, generator=g).item() < 0.5] if ne else []
    elif name == "chunk_edges":    # exactly 32, 33, 64 or 65 live slots, wherever the tile has them
        def pick(t, ne, g):
            k = min((32, 33, 64, 65)[t % 4], ne)
            return torch.randperm(ne, generator=g)[:k].tolist()
    else:
        raise KeyError(name)
    return batch, ei, B, None, edge_mask_from_slots(ei, B, batch, pick)


CASES = ("bench", "zeros", "ones", "one_per_tile", "last_chunk", "chunk_edges", "fractional", "edge_random", "negzero",
         "graphs_unpicked")


def test_case_batches_reach_their_fills():
    """The slot-pattern cases pick what they say (host tile plan); the full-tile batches hold tiles of exactly 256 slots."""
    for name in ("one_per_tile", "last_chunk", "chunk_edges"):
        batch, ei, B, nm, em = case_inputs(name)
        tiles, order = tile_slots(batch, ei, B)
        live = [int(em[order[e0:e0 + ne]].sum()) for e0, ne in tiles]
        assert max(ne for _, ne in tiles) == ECAP, name
        if name == "one_per_tile":
            assert all(c == (1 if ne else 0) for c, (_, ne) in zip(live, tiles))
        elif name == "last_chunk":
            for (e0, ne) in tiles:
                first = 64 * ((ne - 1) // 64) if ne else 0
                assert em[order[e0:e0 + first]].sum() == 0
            assert sum(1 for (_, ne), c in zip(tiles, live) if ne > 192 and c > 0) >= 8
        else:
            for t, ((_, ne), c) in enumerate(zip(tiles, live)):
                assert c == min((32, 33, 64, 65)[t % 4], ne)
            assert {c for c in live} >= {32, 33, 64, 65}


# ------------------------------------------------------------------------------------------------------------ child process
def run_cases(out_path):
    """Child: every case on cuda:0 under this process's ISG_LC_DENSE_MASK; the default walk also runs linear_fused + tile_conv
    and repeats the bench case, saving whether its bits repeat."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import ops
    from isubgvqa_amd.models.layers import GlorotLinear
    dev = torch.device("cuda:0")
    dense = os.environ.get("ISG_LC_DENSE_MASK") == "1"
    H, C, K = 4, 128, 128
    res = {}
    for ci, name in enumerate(CASES):
        batch, ei, B, nm, em = case_inputs(name)
        gen = torch.Generator().manual_seed(100 + ci)
        N, E = batch.numel(), ei.size(1)
        x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-3, 4, (B,), generator=gen).float())[batch][:, None]
        ea = torch.randn(E, K, generator=gen)
        w = torch.randn(H * C, K, generator=gen) * 0.1
        att, bias = torch.randn(1, H, C, generator=gen), torch.randn(H * C, generator=gen) * 2.0 ** -6
        torch.manual_seed(ci)
        lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
        d = lambda t: None if t is None else t.to(dev)
        plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
        csr_as_restated = torch.equal(tile_slots(batch, ei, B)[1], plan.eid.cpu().long())
        xd, ead, wd, attd, bd, nmd, emd = d(x), d(ea), d(w), d(att), d(bias), d(nm), d(em)
        with torch.no_grad():
            def layer():
                o, a = ops.gatv2_layer_conv(xd, lin_l, lin_r, ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd,
                                            want_rowmax=True)
                return o.cpu(), a.cpu(), ops.row_maxima(o).cpu()
            r = {"layer": layer()}
            if not dense:
                # the projection on isg_linear_f16x3 at every M (the panel kernel, no small-batch kernel): the form the layer
                # kernel restates
                with ops.configured(skinny=False, gemm_kernel="panel", rows_kernel_min_edges=0, h3p_min_m=8192):
                    x_l, x_r = ops.linear_fused(xd, (lin_l, lin_r))
                    o, a = ops.gatv2_tile_conv(x_l, x_r, ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd,
                                               want_rowmax=True)
                r["tile"] = (o.cpu(), a.cpu(), ops.row_maxima(o).cpu())
                if name == "bench":
                    r["repeats_equal"] = all(all(torch.equal(p, q) for p, q in zip(r["layer"], layer())) for _ in range(3))
        r["csr_as_restated"] = csr_as_restated
        res[name] = r
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def both_walks(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    d = tmp_path_factory.mktemp("mask_skip")
    out = {}
    for tag, flag in (("live", None), ("dense", "1")):
        env = dict(os.environ)
        env.pop("ISG_LC_DENSE_MASK", None)
        if flag:
            env["ISG_LC_DENSE_MASK"] = flag
        path = str(d / f"{tag}.pt")
        subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.abspath(__file__), path], env=env, cwd=ROOT, check=True, timeout=600)
        out[tag] = torch.load(path)
    return out


def _equal(what, r1, r2):
    for t1, t2, part in zip(r1, r2, ("out", "alpha", "row maxima")):
        assert t1.shape == t2.shape, f"{what}: {part} shape"
        assert torch.equal(t1, t2), f"{what}: {part} differs by {(t1 - t2).abs().nan_to_num(1e30).max().item():.3e}"
        assert torch.equal(torch.signbit(t1), torch.signbit(t2)), f"{what}: {part}: signed zeros differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_live_slot_walk_equals_the_dense_walk_and_tile_conv(both_walks, name):
    live, dense = both_walks["live"][name], both_walks["dense"][name]
    assert live["csr_as_restated"], f"{name}: the host restatement of the CSR slot order is not the plan's"
    _equal(f"{name}: live-slot walk vs ISG_LC_DENSE_MASK=1", live["layer"], dense["layer"])
    _equal(f"{name}: live-slot walk vs linear_fused + tile_conv", live["layer"], live["tile"])
    assert torch.isfinite(live["layer"][0]).all() and torch.isfinite(live["layer"][1]).all(), name


@pytest.mark.gpu
def test_live_slot_walk_repeats_its_bits(both_walks):
    assert both_walks["live"]["bench"]["repeats_equal"]


if __name__ == "__main__":
    run_cases(sys.argv[1])
