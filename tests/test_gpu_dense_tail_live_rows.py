"""isg_mgat_dense_tail's live-row form: after a masked isg_gatv2_layer_conv launch the rows whose aggregation
accumulators stayed all-zero bits are `+0 + bias`, one and the same vector, and x_proj is local to a row -- so a workgroup runs
x_proj once for the live rows of a group of tiles plus ONE dead row, and then each tile's tail.  That changes no bit.

Every case runs twice, in two child processes (the wrapper reads ISG_DT_DENSE_ROWS once per process): the live-row form and
ISG_DT_DENSE_ROWS=1, the existing form with the flags ignored.  Every output of ops.mgat_dense_tail (h', the gated rows, their
planes and inverse scales) and, for the bench workload, the model's logits must be EQUAL as bit patterns (int32 views: NaNs
compare).  The flags themselves are checked against torch: (row, head) is flagged iff that slice of the conv output equals
`+0 + bias` bit for bit (`+0 + -0.0` is `+0`: a dead row under a bias of -0.0 holds +0).  That "iff" holds where no live term is
so small that the bias absorbs it (the flag is about the accumulators, not about the sum): the cases keep their logits small.

The batches: the bench workload's masked layer; no node picked / every node picked; tiles of 64 rows whose groups' lists hold
31, 32, 33, 64 and 65 rows (the row-block edge and the fall-back edge; the tile count is not a multiple of the group); a single
tile; a mixed plan's empty tile; more than eight graphs per tile; conv bias absent and with -0.0; NaN and Inf in the features of
an unpicked node with picked neighbours.  Each runs as a last layer (no mask, no next gate) and as an inner interpretable one
(node_mask, ins_next, rows and planes wanted), and at group sizes 1-4 where the case is about the groups."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_layer_conv_mask_skip as ms          # batch builders and the host restatement of the tile plan

NCAP, ECAP = 64, 256
LIST_EDGES = (31, 32, 33, 64, 65)


def host_tiles(batch, ei, B):
    """(first node, nodes) per tile: isg_tile_plan's greedy packing in 1024-graph chunks; a graph beyond a cap is an empty tile."""
    sizes = torch.bincount(batch, minlength=B).tolist()
    slots = torch.bincount(batch[ei[1]], minlength=B).tolist()
    tiles, g, r = [], 0, 0
    while g < B:
        end = min((g // 1024 + 1) * 1024, B)
        n, s, k = sizes[g], slots[g], g + 1
        while k < end and n + sizes[k] <= NCAP and s + slots[k] <= ECAP:
            n += sizes[k]; s += slots[k]; k += 1
        tiles.append((r, n if n <= NCAP and s <= ECAP else 0))
        r += sum(sizes[g:k])
        g = k
    return tiles


def list_rows(tiles, dead, group):
    """Rows of every group's list: its live rows plus one when it has a dead row."""
    out = []
    for t0 in range(0, len(tiles), group):
        rows = torch.cat([torch.arange(r, r + n) for r, n in tiles[t0:t0 + group]] + [torch.zeros(0, dtype=torch.long)])
        if rows.numel():
            d = dead[rows]
            out.append(int((~d).sum()) + int(d.any()))
    return out


def case_inputs(name):
    """(batch, edge_index, B, node_mask, groups to run, conv bias kind, poison) of a named case (deterministic)."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "bench":
        batch, ei, B, nm, _ = ms.case_inputs("bench")
        return batch, ei, B, nm, (None, 1, 2, 4), "bias", False
    if name == "list_edges":
        # 11 tiles of four 16-node graphs with self-loops (64 rows, 128 slots): a picked node has a live self-loop, an unpicked one
        # no live in-slot, so at group = 2 the picks below give lists of 31, 32, 33, 64 and 65 rows; the eleventh tile is a group
        # of its own, every row live
        graphs = [(16, 32, True)] * 44
        batch, ei = ms.topology(graphs, gen)
        nm = torch.zeros(batch.numel())
        for grp, rows in enumerate(LIST_EDGES):
            pick = torch.randperm(128, generator=gen)[:rows - 1] + 128 * grp
            nm[pick] = 1.0
        nm[640:] = 1.0
        return batch, ei, 44, nm, (2, 3, 1, 4), "bias", False
    if name == "tiny_graphs":      # 2-4 nodes: 16-32 graphs per tile, past the eight whose instruction rows are staged in LDS
        n = torch.randint(2, 5, (600,), generator=gen)
        graphs = [(int(a), 2 * int(a), True) for a in n]
    elif name == "single_tile":
        graphs = [(23, 60, True)]
    elif name == "mixed":          # graphs beyond a tile among small ones: empty tiles, their rows written by other kernels
        graphs = ms.dense_graphs(gen, 60) + [(100, 240, True)] + ms.sparse_graphs(gen, 40) + [(40, 300, True)] + ms.dense_graphs(gen, 30)
    else:
        graphs = ms.full_tiles(gen, 8) + ms.dense_graphs(gen, 200) + ms.sparse_graphs(gen, 60)
    batch, ei = ms.topology(graphs, gen)
    B, N = len(graphs), batch.numel()
    nm = (torch.rand(N, generator=gen) < 0.15).float()
    if name == "none_picked":
        nm = torch.zeros(N)
    elif name == "all_picked":
        nm = torch.ones(N)
    groups = (None, 3) if name in ("no_bias", "negzero_bias", "nan_inf", "mixed") else (None, 1, 3, 4)
    kind = {"no_bias": "none", "negzero_bias": "negzero"}.get(name, "bias")
    return batch, ei, B, nm, groups, kind, name == "nan_inf"


CASES = ("bench", "none_picked", "all_picked", "list_edges", "single_tile", "mixed", "tiny_graphs", "random", "no_bias",
         "negzero_bias", "nan_inf")


def test_case_batches_reach_their_fills():
    """Host side of the cases: full tiles, the tile count against the groups, graphs per tile, the mixed plan's empty tiles."""
    batch, ei, B, nm, groups, _, _ = case_inputs("list_edges")
    tiles = host_tiles(batch, ei, B)
    assert len(tiles) == 11 and all(n == 64 for _, n in tiles) and all(len(tiles) % g for g in (2, 3, 4))
    batch, ei, B, *_ = case_inputs("tiny_graphs")
    tiles = host_tiles(batch, ei, B)
    first_graph = [int(batch[r]) for r, n in tiles if n] + [B]
    assert max(b - a for a, b in zip(first_graph, first_graph[1:])) > 8
    batch, ei, B, *_ = case_inputs("mixed")
    assert sum(1 for _, n in host_tiles(batch, ei, B) if n == 0) == 2
    assert len(host_tiles(*case_inputs("single_tile")[:3])) == 1


# ------------------------------------------------------------------------------------------------------------ child process
def bits(t):
    return None if t is None else t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def run_cases(out_path):
    """Child: every case on cuda:0 under this process's ISG_DT_DENSE_ROWS."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import ops, synthetic
    from isubgvqa_amd.models.layers import GlorotLinear, GraphNorm
    dev = torch.device("cuda:0")
    H, C, K = 4, 128, 128
    res = {}
    for ci, name in enumerate(CASES):
        batch, ei, B, nm, groups, kind, poison = case_inputs(name)
        gen = torch.Generator().manual_seed(500 + ci)
        N, E = batch.numel(), ei.size(1)
        x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-3, 4, (B,), generator=gen).float())[batch][:, None]
        if poison:     # an unpicked node with a picked out-neighbour gets a NaN, another an Inf (values, nothing faults)
            cand = torch.unique(ei[0][(nm[ei[0]] == 0) & (nm[ei[1]] != 0) & (ei[0] != ei[1])])
            assert cand.numel() >= 2
            x[cand[0], 5] = float("nan")
            x[cand[1], 77] = float("inf")
        ea = torch.randn(E, K, generator=gen)
        w = torch.randn(H * C, K, generator=gen) * 0.1
        # logits of a few units: the flag speaks of the accumulators' bits, and a live term of weight 1e-15 that the bias absorbs
        # leaves a row EQUAL to +0 + bias that is rightly flagged live -- with these weights no term is that small
        att = torch.randn(1, H, C, generator=gen) * 0.05
        bias = torch.randn(H * C, generator=gen) * 2.0 ** -6
        if kind == "negzero":
            bias[torch.rand(H * C, generator=gen) < 0.5] = -0.0
        ins, ins_next = torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen)
        h = torch.randn(N, C, generator=gen)
        tail_mask = (torch.rand(N, generator=gen) < 0.5).float()
        torch.manual_seed(ci)
        lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
        x_proj = torch.nn.Sequential(torch.nn.Linear(H * C, 256), torch.nn.GELU(), torch.nn.Linear(256, C), torch.nn.GELU()).to(dev)
        bn = GraphNorm(C).to(dev)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(C, generator=gen) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=gen) * 0.1)
            bn.mean_scale.copy_(torch.rand(C, generator=gen) + 0.5)
        d = lambda t: None if t is None else t.to(dev)
        r = {}
        with torch.no_grad(), ops.configured(mixed_max_fraction=0.9, mixed_min_nodes=0):
            plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
            r["tile_mode"] = plan.tile_mode(NCAP, ECAP)
            conv, _ = ops.gatv2_layer_conv(d(x), lin_l, lin_r, d(ea), d(w), d(att), plan, H, bias=None if kind == "none" else d(bias),
                                           node_mask=d(nm), want_rowmax=True)
            dead = ops.dead_rows(conv)
            assert dead is not None and ops.row_maxima(conv) is not None
            r["conv"], r["dead"] = bits(conv), dead.cpu()
            r["bias"] = bits(torch.zeros(H * C) + (torch.zeros(H * C) if kind == "none" else bias))
            assert ops.dense_tail_supported(plan, x_proj, H * C, C)
            for grp in groups:
                for inner in (False, True):
                    out = ops.mgat_dense_tail(conv, x_proj, d(ins), d(h), plan, bn.weight, bn.bias, bn.mean_scale, bn.eps,
                                              node_mask=d(tail_mask) if inner else None, ins_next=d(ins_next) if inner else None,
                                              want_rows=inner, want_planes=inner, group=grp)
                    assert out is not None
                    h_out, xg, xp = out
                    r[(grp, inner)] = (bits(h_out), bits(xg), None if xp is None else bits(xp.planes[:N]),
                                       None if xp is None else bits(xp.inv[:N]))
            if name == "bench":
                wl = synthetic.make_workload(synthetic.CFG2).to(dev)
                model = synthetic.build_answer_model(synthetic.CFG2).to(dev).eval()
                r["logits"] = bits(model(wl, seed=1000)[0])
        res[name] = r
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def both_forms(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    d = tmp_path_factory.mktemp("live_rows")
    out = {}
    for tag, flag in (("live", None), ("dense", "1")):
        env = dict(os.environ)
        env.pop("ISG_DT_DENSE_ROWS", None)
        if flag:
            env["ISG_DT_DENSE_ROWS"] = flag
        path = str(d / f"{tag}.pt")
        subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.abspath(__file__), path], env=env,
                       cwd=ROOT, check=True, timeout=900)
        out[tag] = torch.load(path)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_live_row_form_equals_the_dense_form(both_forms, name):
    live, dense = both_forms["live"][name], both_forms["dense"][name]
    assert torch.equal(live["conv"], dense["conv"]) and torch.equal(live["dead"], dense["dead"]), f"{name}: the legs' inputs differ"
    keys = [k for k in live if isinstance(k, tuple)]
    assert keys and sorted(map(str, keys)) == sorted(str(k) for k in dense if isinstance(k, tuple))
    ref = {inner: dense[(keys[0][0], inner)] for inner in (False, True)}      # (the dense form ignores the group)
    for k in keys:
        for part, a, b in zip(("h'", "gated rows", "planes", "inverse scales"), live[k], ref[k[1]]):
            assert (a is None) == (b is None), f"{name} {k}: {part}"
            if a is not None:
                assert a.shape == b.shape and torch.equal(a, b), \
                    f"{name} group={k[0]} inner={k[1]}: {part}: {(a != b).sum().item()} words differ from ISG_DT_DENSE_ROWS=1"
        for part, a, b in zip(("h'", "gated rows", "planes", "inverse scales"), dense[k], ref[k[1]]):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"{name} {k}: the dense form depends on group"
    if name == "bench":
        assert torch.equal(live["logits"], dense["logits"]), "the model's logits differ between the two forms"
    assert live["tile_mode"] == ("mixed" if name == "mixed" else "tiles"), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_dead_row_flags_say_which_rows_are_plus_zero_plus_bias(both_forms, name):
    r = both_forms["live"][name]
    batch, ei, B, nm, groups, kind, poison = case_inputs(name)
    conv, dead, bias = r["conv"], r["dead"].bool(), r["bias"]
    N = conv.size(0)
    is_bias = (conv.view(N, 4, 128) == bias.view(1, 4, 128)).all(dim=2)
    rows = torch.zeros(N, dtype=torch.bool)          # rows inside a tile (a mixed plan's oversize graphs are never flagged)
    for r0, n in host_tiles(batch, ei, B):
        rows[r0:r0 + n] = True
    assert torch.equal(dead[rows], is_bias[rows]), f"{name}: {(dead[rows] != is_bias[rows]).sum().item()} flags are not (out == +0 + bias)"
    assert not dead[~rows].any(), name
    row_dead = dead.all(dim=1)
    if name == "none_picked":
        assert row_dead.all()
    if name == "all_picked":
        assert not row_dead[torch.bincount(ei[1], minlength=N) > 0].any()
    if not poison:     # with weights of ordinary size a row is dead exactly when no in-slot has both ends picked
        live_in = torch.bincount(ei[1], weights=((nm[ei[0]] != 0) & (nm[ei[1]] != 0)).double(), minlength=N) > 0
        assert torch.equal(row_dead[rows], ~live_in[rows]), name
    if name == "list_edges":
        assert list_rows(host_tiles(batch, ei, B), row_dead, 2) == list(LIST_EDGES) + [64]
    if poison:
        fin = torch.isfinite(conv.view(torch.float32)).all(dim=1)
        assert not (row_dead & ~fin).any(), "a row that a NaN or Inf reached is flagged dead"


if __name__ == "__main__":
    run_cases(sys.argv[1])
