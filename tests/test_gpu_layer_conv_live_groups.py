"""isg_gatv2_layer_conv's masked, live launches work on GROUPS of tiles: one node product for the rows that a
live slot of the group names, one edge product per 64 live slots of the group, then softmax and aggregation tile by tile.  A
product element does not depend on the column its row sits in, so the group size changes no bit.

Every case runs in child processes, one after another (the wrapper reads ISG_LC_GROUP once per process): the default group size,
ISG_LC_GROUP=1 (the per-tile kernel, as before the grouped form) and every forced size from 2 to 6, the largest the kernel
takes (the wrapper itself picks at most 4).  out, alpha, the row maxima and the dead-row flags must be EQUAL as bit patterns
between all of them, and the default must also equal linear_fused + gatv2_tile_conv.  One child pair runs BASELINE configs[1]'s
model: logits, mask and gate of the default equal ISG_LC_GROUP=1's.

The batches reach what the grouping has edges at; the child restates the kernel's walk (a workgroup takes every ngrp-th entry
of the heavy-first tile list, G at a time) and builds edge masks on it, and test_case_batches_reach_their_fills asserts that
they hold what they say: groups with exactly 32 / 33 / 64 / 65 named rows (the second 32-row block, the fall-back to single
tiles), groups with 64 / 65 live slots inside 64 rows (the second chunk), groups and a whole batch without a live slot, every
slot live with tiles of 256 slots (more than 64 rows: the fall-back), one tile, tile counts no group size divides, a live slot
whose source is no live slot's destination (edge_mask form), fractional and straight-through masks, -0.0, destinations without
in-edges, and a mixed plan with oversize graphs (whose own rows the per-graph kernels write: every group size gives the same
bits there too, and the comparison with linear_fused + gatv2_tile_conv is bit for bit on the rows inside tiles)."""
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCAP, ECAP, H = 64, 256, 4
GROUPS = (2, 3, 4, 5, 6)
RUNS = ("default", "1") + tuple(str(g) for g in GROUPS)
BORROWED = ("bench", "zeros", "ones", "fractional", "negzero", "edge_random", "graphs_unpicked")
CASES = BORROWED + ("rows_g2", "rows_g4", "slots_g2", "slots_g4", "sparse_groups", "one_tile", "mixed")


def _mask_skip():
    """The batches of tests/test_gpu_layer_conv_mask_skip.py (loaded by path: tests/ is no package)."""
    spec = importlib.util.spec_from_file_location("_lc_mask_skip", os.path.join(ROOT, "tests", "test_gpu_layer_conv_mask_skip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def walk_groups(T, cap, G, cus):
    """The grouped kernel's work items: workgroup w of a head walks tiles w, w + ngrp, ... of the heavy-first list, G at a time
    (csrc/isg_layer_conv.hip: grid = 8 H gpx, ngrp = 8 gpx)."""
    gpx = max(1, (cus // 8) // H)
    gpx = min(gpx, (cap + 7) // 8)
    ngrp = 8 * gpx
    out = []
    for w in range(min(ngrp, T)):
        seq = list(range(w, T, ngrp))
        out += [seq[i:i + G] for i in range(0, len(seq), G)]
    return out


def group_fills(heavy, src, dst, live, groups):
    """Per group (rows that a live slot names, live slots), counted the way the kernel does: per tile, rows relative to the tile
    and clamped into it."""
    fills = []
    for grp in groups:
        rows, n = 0, 0
        for t in grp:
            r0, nr, e0, ne = heavy[t]
            ne = min(ne, ECAP)
            lv = live[e0:e0 + ne].nonzero().flatten() + e0
            n += lv.numel()
            named = torch.cat([src[lv] - r0, dst[lv] - r0]).clamp(0, max(nr - 1, 0))
            rows += named.unique().numel()
        fills.append((rows, n))
    return fills


def greedy_mask(heavy, src, dst, groups, mode):
    """Live slots (CSR order) picked group by group.  rows: slots are added while the named rows stay within the group's target
    (32, 33, 64, 65 in turn) until it is met.  slots: until 64 or 65 (in turn) are live, inside 60 rows.  sparse: one slot
    with src != dst in every eighth tile."""
    live = torch.zeros(src.numel(), dtype=torch.bool)
    s_l, d_l = src.tolist(), dst.tolist()
    for gi, grp in enumerate(groups):
        if mode == "sparse":
            for t in grp:
                r0, nr, e0, ne = heavy[t]
                cand = [s for s in range(e0, e0 + min(ne, ECAP)) if s_l[s] != d_l[s]]
                if t % 8 == 0 and cand:
                    live[cand[len(cand) // 2]] = True
            continue
        row_target = (32, 33, 64, 65)[gi % 4] if mode == "rows" else 60
        slot_target = (64, 65)[gi % 2] if mode == "slots" else 1 << 30
        named, n = set(), 0
        for t in grp:
            r0, nr, e0, ne = heavy[t]
            for s in range(e0, e0 + min(ne, ECAP)):
                new = named | {(t, s_l[s]), (t, d_l[s])}
                if len(new) > row_target or n >= slot_target or (mode == "rows" and len(named) == row_target):
                    continue
                named, n = new, n + 1
                live[s] = True
    return live


# ------------------------------------------------------------------------------------------------------------ child process
def build_case(name, ms, ops, dev, cus, want_facts):
    """(batch, edge_index, B, node_mask, edge_mask, plan, facts) of a case; the masks of the walk-built cases come from the plan."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 5)
    nm = em = None
    if name in BORROWED:
        batch, ei, B, nm, em = ms.case_inputs(name)
    elif name == "one_tile":
        batch, ei = ms.topology([(23, 90, True)], gen)
        B = 1
        nm = (torch.rand(23, generator=gen) < 0.4).float()
    elif name == "mixed":          # graphs beyond 64 nodes / 256 slots among ordinary ones: the plan is mixed
        graphs = ms.dense_graphs(gen, 150) + [(70, 200, True)] + ms.sparse_graphs(gen, 30) + [(200, 700, True), (30, 400, True)] + \
            ms.dense_graphs(gen, 150)
        batch, ei = ms.topology(graphs, gen)
        B = len(graphs)
        nm = ms.straight_through(torch.rand(batch.numel(), generator=gen) * 0.9 + 0.05, torch.rand(batch.numel(), generator=gen) < 0.3)
    else:
        graphs = ms.full_tiles(gen, 16) + ms.dense_graphs(gen, 1000) + ms.sparse_graphs(gen, 40)
        batch, ei = ms.topology(graphs, gen)
        B = len(graphs)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    plan.require_csr()
    _, ntiles, cap, _ = plan.tiles(NCAP, ECAP)
    T = int(ntiles.item())
    heavy = plan.tiles_heavy_first(NCAP, ECAP).cpu().tolist()[:T]
    src, dst, eid = plan.src.cpu().long(), plan.dst.cpu().long(), plan.eid.cpu().long()
    if em is None and nm is None:
        G = int(name[-1]) if name[-2:-1] == "g" else 4
        live = greedy_mask(heavy, src, dst, walk_groups(T, cap, G, cus), name.split("_")[0])
        em = torch.zeros(ei.size(1))
        em[eid[live]] = 1.0
    if not want_facts:
        return batch, ei, B, nm, em, plan, None
    mask_at_slot = em[eid] if em is not None else nm[src] * nm[dst]
    live = (mask_at_slot.view(torch.int32) & 0x7fffffff) != 0
    rowptr = plan.rowptr.cpu().long()
    live_dst = torch.zeros(batch.numel(), dtype=torch.bool)
    live_dst[dst[live]] = True
    facts = {"T": T, "tile_mode": plan.tile_mode(NCAP, ECAP), "max_slots": max([min(w[3], ECAP) for w in heavy] or [0]),
             "no_in_edge": int((rowptr[1:] == rowptr[:-1]).sum()), "src_not_a_live_dst": int((~live_dst[src[live]]).sum()),
             "fills": {G: group_fills(heavy, src, dst, live, walk_groups(T, cap, G, cus)) for G in GROUPS}}
    if facts["tile_mode"] == "mixed":      # rows and edges of the graphs that fit a tile: what the tile kernels compute
        big = torch.zeros(B, dtype=torch.bool)
        big[plan.oversize(NCAP, ECAP).gids.cpu().long()] = True
        facts["rows_in_tiles"], facts["edges_in_tiles"] = ~big[batch], ~big[batch[ei[1]]]
    return batch, ei, B, nm, em, plan, facts


def run_case(ci, name, ms, ops, dev, cus, forced):
    """One case's results under this process's ISG_LC_GROUP (the default also: linear_fused + tile_conv, the batch's fills)."""
    from isubgvqa_amd.models.layers import GlorotLinear
    C, K = 128, 128
    batch, ei, B, nm, em, plan, facts = build_case(name, ms, ops, dev, cus, forced is None)
    gen = torch.Generator().manual_seed(300 + ci)
    N, E = batch.numel(), ei.size(1)
    x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-3, 4, (B,), generator=gen).float())[batch][:, None]
    ea = torch.randn(E, K, generator=gen)
    w = torch.randn(H * C, K, generator=gen) * 0.1
    att, bias = torch.randn(1, H, C, generator=gen), torch.randn(H * C, generator=gen) * 2.0 ** -6
    torch.manual_seed(ci)
    lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
    d = lambda t: None if t is None else t.to(dev)
    xd, ead, wd, attd, bd, nmd, emd = d(x), d(ea), d(w), d(att), d(bias), d(nm), d(em)
    with torch.no_grad():
        o, a = ops.gatv2_layer_conv(xd, lin_l, lin_r, ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd, want_rowmax=True)
        dead = ops.dead_rows(o)
        r = {"layer": (o.cpu(), a.cpu(), ops.row_maxima(o).cpu(), None if dead is None else dead.cpu()), "mask": (nm, em)}
        if forced is None:
            with ops.configured(skinny=False, gemm_kernel="panel", rows_kernel_min_edges=0, h3p_min_m=8192):
                x_l, x_r = ops.linear_fused(xd, (lin_l, lin_r))
                o, a = ops.gatv2_tile_conv(x_l, x_r, ead, wd, attd, plan, H, bias=bd, node_mask=nmd, edge_mask=emd, want_rowmax=True)
            r["tile"] = (o.cpu(), a.cpu(), ops.row_maxima(o).cpu())
            r["facts"] = facts
    return r


def run_cases(out_path):
    """Child: every case on cuda:0 under this process's ISG_LC_GROUP; the default and ISG_LC_GROUP=1 also run BASELINE
    configs[1]'s model."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import ops, synthetic
    ms = _mask_skip()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    forced = os.environ.get("ISG_LC_GROUP")
    res = {}
    for ci, name in enumerate(CASES):
        # a batch as small as "mixed" is dispatched as mixed only with the node floor of that dispatch lowered
        with ops.configured(mixed_min_nodes=0):
            res[name] = run_case(ci, name, ms, ops, dev, cus, forced)
    if forced in (None, "1"):
        wl = synthetic.make_workload(synthetic.CFG2).to(dev)
        net = synthetic.build_answer_model(synthetic.CFG2).to(dev).eval()
        with torch.no_grad():
            res["model"] = tuple(t.cpu() for t in net(wl, seed=1000))
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    d = tmp_path_factory.mktemp("live_groups")
    out = {}
    for tag in RUNS:
        env = dict(os.environ)
        env.pop("ISG_LC_GROUP", None)
        env.pop("ISG_LC_DENSE_MASK", None)
        if tag != "default":
            env["ISG_LC_GROUP"] = tag
        path = str(d / f"g{tag}.pt")
        subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.abspath(__file__), path], env=env,
                       cwd=ROOT, check=True, timeout=900)
        out[tag] = torch.load(path)
    return out


def _equal(what, r1, r2):
    for t1, t2, part in zip(r1, r2, ("out", "alpha", "row maxima", "dead rows")):
        if t1 is None or t2 is None:
            assert t1 is None and t2 is None, f"{what}: {part} missing on one side"
            continue
        assert t1.shape == t2.shape and t1.dtype == t2.dtype, f"{what}: {part} shape"
        if t1.dtype == torch.float32:        # bit patterns: signed zeros and NaN payloads count
            diff = (t1.view(torch.int32) != t2.view(torch.int32))
            assert not diff.any(), f"{what}: {part}: {int(diff.sum())} values differ, by up to {(t1 - t2).abs().nan_to_num(1e30).max().item():.3e}"
        else:
            assert torch.equal(t1, t2), f"{what}: {part} differs"


@pytest.mark.gpu
def test_case_batches_reach_their_fills(runs):
    f = {name: runs["default"][name]["facts"] for name in CASES}
    for G in (2, 4):
        rows = {r for r, n in f[f"rows_g{G}"]["fills"][G]}
        assert rows >= {32, 33, 64, 65}, (G, sorted(rows))
        slots = {n for r, n in f[f"slots_g{G}"]["fills"][G] if r <= NCAP}
        assert slots >= {64, 65}, (G, sorted(slots))
    for G in GROUPS:
        fills = f["sparse_groups"]["fills"][G]
        assert any(n == 0 for r, n in fills) and any(n > 0 for r, n in fills), G
        assert all(n == 0 for r, n in f["zeros"]["fills"][G])
        assert any(r > NCAP for r, n in f["ones"]["fills"][G]), G                 # the fall-back to single tiles
        assert any(f[name]["T"] % G for name in CASES), G                         # a short last group
    assert f["ones"]["max_slots"] == ECAP and f["rows_g4"]["max_slots"] == ECAP
    assert f["sparse_groups"]["src_not_a_live_dst"] > 0
    assert f["one_tile"]["T"] == 1
    assert f["mixed"]["tile_mode"] == "mixed" and f["bench"]["tile_mode"] == "tiles" and f["mixed"]["T"] > 1
    assert f["graphs_unpicked"]["no_in_edge"] > 0
    assert f["bench"]["T"] > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_group_size_changes_no_bit(runs, name):
    base = runs["default"][name]
    for tag in RUNS[1:]:
        other = runs[tag][name]
        for m1, m2 in zip(base["mask"], other["mask"]):
            assert (m1 is None and m2 is None) or torch.equal(m1, m2), f"{name}: the case's mask is not the same in every process"
        _equal(f"{name}: default vs ISG_LC_GROUP={tag}", base["layer"], other["layer"])
    layer, tile = base["layer"][:3], base["tile"]
    if "rows_in_tiles" in base["facts"]:
        # a mixed plan's oversize graphs are projected and convolved per graph by BOTH callers, each with its own Linear: the
        # two agree to rounding there, and bit for bit where the tile kernels ran
        rows, edges = base["facts"]["rows_in_tiles"], base["facts"]["edges_in_tiles"]
        assert 0 < rows.sum() < rows.numel()
        layer, tile = [(t[0][rows], t[1][edges], t[2][rows]) for t in (layer, tile)]
        assert torch.allclose(base["layer"][0], base["tile"][0], rtol=0, atol=1e-3)
    _equal(f"{name}: default vs linear_fused + tile_conv", layer, tile)
    assert torch.isfinite(base["layer"][0]).all() and torch.isfinite(base["layer"][1]).all(), name


@pytest.mark.gpu
def test_model_is_the_same_with_and_without_groups(runs):
    for t1, t2, part in zip(runs["default"]["model"], runs["1"]["model"], ("logits", "mask", "gate")):
        assert t1.dtype == t2.dtype and torch.equal(t1, t2), f"configs[1] {part}: default vs ISG_LC_GROUP=1"
        if t1.dtype == torch.float32:
            assert torch.equal(t1.view(torch.int32), t2.view(torch.int32)), part


if __name__ == "__main__":
    run_cases(sys.argv[1])
