"""The grouped, masked isg_gatv2_layer_conv aggregates only the rows that a live slot reaches: per sub-group of
tiles ONE softmax + aggregation pass over the list of live-destination rows, and every other row written as the constant it is
known to be (+0 + bias, dead, its row maximum, alpha = 1 / in-degree).  No bit may move.

Child processes run one after another (the wrapper reads its switches once per process): the default first, which saves out,
alpha, the row maxima and the dead-row flags of every case; then ISG_LC_AGG_ALL_ROWS=1 (the per-tile aggregation over all 64
rows, as before), ISG_LC_GROUP=1 (the per-tile kernel), ISG_LC_GROUP=2, ISG_LC_GROUP=6 and ISG_LC_TABLES=0 (the kernel scans the
tiles itself), each of which loads the default's tensors and counts, per case and tensor, the values whose BIT PATTERNS differ
(int32 views: signed zeros and NaN payloads count).  Every count must be zero.  The default and ISG_LC_AGG_ALL_ROWS=1 also run
BASELINE configs[1]'s model at 512 graphs: logits, mask and gate must be equal.

A workgroup walks every ngrp-th tile of the plan's list, G at a time, and ngrp is 64 on the MI355X with four heads: groups of
more than one tile exist from 65 tiles on, groups of six from 321.  So every batch is 400 tiles -- the few tiles a case is named
for in front, plain ones behind them -- each tile one graph of 36 to 64 nodes (no two share a tile), which is also what makes the
default process run the grouped kernel at all (lc_group_rule, restated in group_rule).
test_case_batches_hold_what_they_are_named_for restates the live-destination sets on the host and asserts that each batch holds
what it says."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCAP, ECAP, C, K = 64, 256, 128, 128
TILES = 400
MI355X_CUS = 256
RUNS = (("default", {}), ("agg_all", {"ISG_LC_AGG_ALL_ROWS": "1"}), ("g1", {"ISG_LC_GROUP": "1"}), ("g2", {"ISG_LC_GROUP": "2"}),
        ("g6", {"ISG_LC_GROUP": "6"}), ("tables0", {"ISG_LC_TABLES": "0"}))
SWITCHES = ("ISG_LC_AGG_ALL_ROWS", "ISG_LC_GROUP", "ISG_LC_TABLES", "ISG_LC_DENSE_MASK")
# run name -> (batch, heads, bias: "random" / None / "negzero")
CASES = {"none_picked": ("none_picked", 4, "random"), "all_picked": ("all_picked", 4, "random"),
         "one_per_tile": ("one_per_tile", 4, "random"), "source_only": ("source_only", 4, "random"), "hub": ("hub", 4, "random"),
         "mixed_rounds": ("mixed_rounds", 4, "random"), "edge_mask": ("edge_mask", 4, "random"), "no_bias": ("picked", 4, None),
         "negzero_bias": ("picked", 4, "negzero"), "heads_1": ("one_per_tile", 1, "random"), "heads_2": ("one_per_tile", 2, "random"),
         "holes": ("holes", 4, "random")}
PARTS = ("out", "alpha", "row maxima", "dead rows")
ROUND_DEGREES = (1, 4, 5, 8, 13)
MASK_VALUES = (1.0, 0.5, 0.0, -0.0)


# ----------------------------------------------------------------------------------------------------------------- batches
def plain_graph(gen):
    """36 to 56 nodes, a self-loop each, 30 to 100 more in-edges between random pairs: one tile of its own."""
    n = int(torch.randint(36, 57, (1,), generator=gen))
    m = int(torch.randint(30, 101, (1,), generator=gen))
    pairs = torch.randint(0, n, (2, m), generator=gen).t().tolist()
    return n, [(i, i) for i in range(n)] + [tuple(p) for p in pairs]


def graph_with_in_degrees(n, degrees, gen):
    """A graph of n nodes whose row r has degrees[r] in-edges from random sources."""
    edges = []
    for r, deg in enumerate(degrees):
        edges += [(int(s), r) for s in torch.randint(0, n, (deg,), generator=gen)]
    return n, edges


def assemble(graphs, gen):
    """(batch, edge_index with the edge ids shuffled, [(first node, nodes)] per graph)."""
    batch, src, dst, spans, off = [], [], [], [], 0
    for g, (n, edges) in enumerate(graphs):
        assert len(edges) <= ECAP or n > NCAP
        batch += [g] * n
        src += [off + s for s, _ in edges]
        dst += [off + d for _, d in edges]
        spans.append((off, n))
        off += n
    ei = torch.tensor([src, dst], dtype=torch.long).view(2, -1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    return torch.tensor(batch, dtype=torch.long), ei, spans


def csr(ei, N):
    """(slot -> edge id in destination-major order, edge ids ascending within a destination; row pointers)."""
    E = ei.size(1)
    order = torch.argsort(ei[1] * E + torch.arange(E))
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(ei[1], minlength=N).cumsum(0)])
    return order, rowptr


def live_edges(ei, nm, em):
    """Per edge id: the slot's mask has bits other than a sign (the kernel's test)."""
    m = em if em is not None else nm[ei[0]] * nm[ei[1]]
    return (m.view(torch.int32) & 0x7fffffff) != 0


def straight_through(gen, N, share):
    """A sampler's node mask: exactly +0 where not picked, 1 +- an ulp or so where picked."""
    khot = torch.rand(N, generator=gen) * 0.9 + 0.05
    hard = (torch.rand(N, generator=gen) < share).float()
    return (hard - khot) + khot


def case_inputs(batch_name):
    """{batch, ei, B, spans, nm, em} of a named batch (deterministic, host only)."""
    gen = torch.Generator().manual_seed(sum(map(ord, batch_name)) + 18)
    special = []
    if batch_name == "none_picked":        # in-degrees 0, 1, 3, 4, 5, 9 and 64 among the rows of the first three tiles
        for _ in range(3):
            special.append(graph_with_in_degrees(40, [0, 1, 3, 4, 5, 9, 64] + [1] * 33, gen))
    elif batch_name == "all_picked":       # two tiles of 64 rows and 256 slots
        for _ in range(2):
            pairs = torch.randint(0, 64, (2, 192), generator=gen).t().tolist()
            special.append((64, [(i, i) for i in range(64)] + [tuple(p) for p in pairs]))
    elif batch_name == "hub":              # row 7 holds all 256 slots of its tile
        special.append(graph_with_in_degrees(40, [0] * 7 + [256] + [0] * 32, gen))
    elif batch_name == "mixed_rounds":     # eight rows of each in-degree in turn: every wave's octets hold all five
        for _ in range(2):
            special.append(graph_with_in_degrees(40, [ROUND_DEGREES[(r // 8) % 5] for r in range(40)], gen))
    graphs = special + [plain_graph(gen) for _ in range(TILES - len(special))]
    if batch_name == "holes":              # a graph beyond a tile in the middle: the plan is mixed, its tile is empty
        n, m = 70, 200
        graphs[TILES // 2] = (n, [(i, i) for i in range(n)] + [tuple(p) for p in torch.randint(0, n, (2, m - n), generator=gen).t().tolist()])
    batch, ei, spans = assemble(graphs, gen)
    N, E = batch.numel(), ei.size(1)
    order, rowptr = csr(ei, N)
    nm = em = None
    if batch_name == "none_picked":
        nm = torch.zeros(N)
    elif batch_name == "all_picked":
        nm = torch.ones(N)
    elif batch_name in ("picked", "holes"):
        nm = straight_through(gen, N, 0.13)
    elif batch_name == "edge_mask":
        em = torch.tensor(MASK_VALUES)[torch.multinomial(torch.tensor([0.05, 0.05, 0.45, 0.45]), E, replacement=True, generator=gen)]
    else:
        em = torch.zeros(E)
        for t, (r0, n) in enumerate(spans):
            slots = order[rowptr[r0]:rowptr[r0 + n]]          # the tile's edge ids in CSR slot order
            s, d = ei[0, slots], ei[1, slots]
            loops, cross = slots[s == d], slots[s != d]
            if batch_name == "one_per_tile":                  # tile 0: a self-loop; the others: a slot between two rows
                em[loops[0] if t == 0 else cross[int(torch.randint(0, cross.numel(), (1,), generator=gen))]] = 1.0
            elif batch_name == "source_only":                 # up to three slots whose sources are no live slot's destination
                S, D = set(), set()
                for e in cross.tolist():
                    a, b = int(ei[0, e]), int(ei[1, e])
                    if a not in D and b not in S and len(D) < 3 and b not in D:
                        S.add(a); D.add(b)
                        em[e] = 1.0
            elif batch_name == "hub":                         # every third slot of the hub; one slot of every fourth plain tile
                if t == 0:
                    em[slots[::3]] = 1.0
                elif t % 4 == 0:
                    em[cross[0]] = 1.0
            elif batch_name == "mixed_rounds":                # live and dead slots in turn within each row; tile 1 also has
                if t < 2:                                     # neighbours with a live slot (every plain tile with t % 6 == 1)
                    for r in range(r0, r0 + n):
                        em[order[rowptr[r]:rowptr[r + 1]][::2]] = 1.0
                elif t % 6 == 1:
                    em[cross[0]] = 1.0
    return {"batch": batch, "ei": ei, "B": len(graphs), "spans": spans, "nm": nm, "em": em}


def tile_sets(c):
    """Per graph that fits a tile: (live-destination rows, rows a live slot names, in-degrees, live slots), rows relative to it."""
    batch, ei, spans = c["batch"], c["ei"], c["spans"]
    order, rowptr = csr(ei, batch.numel())
    live = live_edges(ei, c["nm"], c["em"])
    out = []
    for r0, n in spans:
        if n > NCAP:
            out.append(None)
            continue
        slots = order[rowptr[r0]:rowptr[r0 + n]]
        lv = slots[live[slots]]
        ldst = set((ei[1, lv] - r0).tolist())
        touch = ldst | set((ei[0, lv] - r0).tolist())
        out.append((ldst, touch, (rowptr[r0 + 1:r0 + n + 1] - rowptr[r0:r0 + n]).tolist(), int(lv.numel())))
    return out


def walk_groups(T, cap, G, H, cus=MI355X_CUS):
    """The grouped kernel's work items (csrc/isg_layer_conv.hip: grid = 8 H gpx, ngrp = 8 gpx): workgroup w of a head walks
    entries w, w + ngrp, ... of the tile list, G at a time."""
    gpx = max(1, (cus // 8) // H)
    gpx = max(1, min(gpx, (cap + 7) // 8))
    ngrp = 8 * gpx
    out = []
    for w in range(min(ngrp, T)):
        seq = list(range(w, T, ngrp))
        out += [seq[i:i + G] for i in range(0, len(seq), G)]
    return out


def group_rule(N, E, H, cap, cus=MI355X_CUS):
    """lc_group_rule (csrc/isg_layer_conv.hip): the tiles per group that the wrapper picks when ISG_LC_GROUP is not set."""
    gpx = max(1, min(max(1, (cus // 8) // H), (cap + 7) // 8))
    tiles = max((N + NCAP - 1) // NCAP, (E + ECAP - 1) // ECAP)
    return max(1, min(6, (min(tiles, cap) + 8 * gpx - 1) // (8 * gpx)))


def test_case_batches_hold_what_they_are_named_for():
    sets = {}
    for name in sorted({b for b, _, _ in CASES.values()}):
        c = case_inputs(name)
        assert c["B"] == TILES and all(n >= 33 for _, n in c["spans"]), name        # one graph per tile
        sets[name] = (c, tile_sets(c))
    for name, (batch_name, H, _) in CASES.items():                                 # the default process runs the grouped kernel
        c = sets[batch_name][0]
        assert group_rule(c["batch"].numel(), c["ei"].size(1), H, TILES) > 1, name
    # groups of six tiles and of one in a workgroup's walk, with four heads and with two; with one head groups of two
    sizes = lambda H, G: {len(g) for g in walk_groups(TILES, TILES, G, H)}
    assert sizes(4, 6) >= {6, 1} and sizes(2, 6) >= {3, 4} and sizes(1, 6) == {1, 2} and sizes(4, 2) >= {2, 1}
    c, s = sets["none_picked"]
    assert all(not ld and not tc and nl == 0 for ld, tc, _, nl in s)               # every row is a fill
    for t in range(3):
        assert set(s[t][2]) >= {0, 1, 3, 4, 5, 9, 64}
    c, s = sets["all_picked"]
    assert len(s[0][0]) == 64 and len(s[1][0]) == 64 and s[0][3] == ECAP           # a pass of 64 rows
    assert all(len(tc) >= 33 for _, tc, _, _ in s)                                 # any two tiles: more than 64 named rows
    assert all(ld == {r for r, deg in enumerate(degs) if deg} for ld, _, degs, _ in s)
    c, s = sets["one_per_tile"]
    assert all(nl == 1 and len(ld) == 1 for ld, _, _, nl in s)                     # lists of 6 rows and of 1
    assert s[0][1] == s[0][0] and all(len(tc) == 2 for _, tc, _, _ in s[1:])       # tile 0: a self-loop
    c, s = sets["source_only"]
    assert all(len(ld) == 3 and len(tc - ld) >= 1 for ld, tc, _, _ in s)           # named for the product, yet fills
    live = live_edges(c["ei"], None, c["em"])
    srcs = set(c["ei"][0, live].tolist())
    assert any(d not in srcs for d in c["ei"][1, live].tolist())                   # the reverse: a destination that is no source
    c, s = sets["hub"]
    assert s[0][0] == {7} and s[0][2][7] == ECAP and s[0][3] == 86 and sum(s[0][2]) == ECAP
    assert any(nl == 0 for _, _, _, nl in s[1:]) and any(nl == 1 for _, _, _, nl in s[1:])
    c, s = sets["mixed_rounds"]
    live = live_edges(c["ei"], None, c["em"])
    order, rowptr = csr(c["ei"], c["batch"].numel())
    for t in range(2):
        ld, _, degs, nl = s[t]
        assert ld == set(range(40)) and 0 < nl < sum(degs)
        for w in range(8):             # list entry i goes to wave i & 7: wherever the tile's rows start in the list, a wave's
            for first in range(8):     # octets hold every in-degree
                assert {degs[r] for r in range(40) if (r + first) % 8 == w} == set(ROUND_DEGREES)
        r0 = c["spans"][t][0]
        row = live[order[rowptr[r0 + 39]:rowptr[r0 + 40]]].tolist()                # an in-degree of 13: live and dead in turn
        assert len(row) == 13 and row == [i % 2 == 0 for i in range(13)]
    assert s[2][3] == 0 and s[7][3] == 1
    c, s = sets["edge_mask"]
    assert c["nm"] is None and {v.item() for v in c["em"].view(torch.int32)} == {v.item() for v in torch.tensor(MASK_VALUES).view(torch.int32)}
    assert any(0 < len(ld) < len(tc) for ld, tc, _, _ in s)
    c, s = sets["picked"]
    assert any(not ld for ld, _, _, _ in s) and any(ld for ld, _, _, _ in s)
    c, s = sets["holes"]
    assert s[TILES // 2] is None and sum(x is None for x in s) == 1
    b = make_bias("negzero", 4, torch.Generator().manual_seed(1))
    assert int((b.view(torch.int32) == -2 ** 31).sum()) == b.numel() // 2


def make_bias(mode, H, gen):
    if mode is None:
        return None
    bias = torch.randn(H * C, generator=gen) * 2.0 ** -6
    if mode == "negzero":
        bias[::2] = -0.0
    return bias


# ------------------------------------------------------------------------------------------------------------ child process
def run_cases(out_path, ref_path):
    """Child: every case on cuda:0 under this process's switches.  Without ref_path (the default) the tensors are saved; with it
    they are compared with the saved ones and the counts of differing bit patterns are saved."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import _lib_masked, ops, synthetic
    from isubgvqa_amd.models.layers import GlorotLinear
    dev = torch.device("cuda:0")
    ref = torch.load(ref_path) if ref_path else None
    mlib = _lib_masked.load()
    res, batches = {}, {}
    for ci, (name, (batch_name, H, bias_mode)) in enumerate(CASES.items()):
        if batch_name not in batches:
            batches[batch_name] = case_inputs(batch_name)
        c = batches[batch_name]
        batch, ei, B, nm, em = c["batch"], c["ei"], c["B"], c["nm"], c["em"]
        gen = torch.Generator().manual_seed(900 + ci)
        N, E = batch.numel(), ei.size(1)
        x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-3, 4, (B,), generator=gen).float())[batch][:, None]
        ea = torch.randn(E, K, generator=gen)
        w = torch.randn(H * C, K, generator=gen) * 0.1
        att, bias = torch.randn(1, H, C, generator=gen), make_bias(bias_mode, H, gen)
        torch.manual_seed(ci)
        lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
        d = lambda t: None if t is None else t.to(dev)
        # a batch with one graph beyond a tile is dispatched as mixed only with that dispatch's floors lowered
        with torch.no_grad(), ops.configured(mixed_max_fraction=0.9, mixed_min_nodes=0):
            plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
            o, a = ops.gatv2_layer_conv(d(x), lin_l, lin_r, d(ea), d(w), d(att), plan, H, bias=d(bias), node_mask=d(nm),
                                        edge_mask=d(em), want_rowmax=True)
            dead = ops.dead_rows(o)
            got = (o.cpu(), a.cpu(), ops.row_maxima(o).cpu(), dead.cpu())
            _, ntiles, cap, _ = plan.tiles(NCAP, ECAP)
            facts = {"group": int(mlib.isg_gatv2_layer_conv_group(N, E, H, cap)), "tile_mode": plan.tile_mode(NCAP, ECAP),
                     "T": int(ntiles.item()), "cap": int(cap), "N": N, "E": E,
                     "cus": torch.cuda.get_device_properties(0).multi_processor_count, "finite": bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all())}
        if ref is None:
            res[name] = {"layer": got, "facts": facts}
        else:
            diffs = {}
            for t1, t2, part in zip(ref[name]["layer"], got, PARTS):
                assert t1.shape == t2.shape and t1.dtype == t2.dtype, (name, part)
                v1, v2 = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (t1, t2))
                diffs[part] = int((v1 != v2).sum())
            res[name] = {"diffs": diffs, "facts": facts}
    if os.environ.get("ISG_LC_GROUP") is None and os.environ.get("ISG_LC_TABLES") is None:
        cfg = dataclasses.replace(synthetic.CFG2, num_graphs=512)
        wl = synthetic.make_workload(cfg).to(dev)
        net = synthetic.build_answer_model(cfg).to(dev).eval()
        with torch.no_grad():
            res["model"] = tuple(t.cpu() for t in net(wl, seed=1000))
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    d = tmp_path_factory.mktemp("live_agg")
    out, ref = {}, None
    for tag, extra in RUNS:
        env = dict(os.environ)
        for k in SWITCHES:
            env.pop(k, None)
        env.update(extra)
        path = str(d / f"{tag}.pt")
        subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.abspath(__file__), path, ref or ""],
                       env=env, cwd=ROOT, check=True, timeout=600)
        out[tag] = torch.load(path)
        ref = ref or path
    return out


@pytest.mark.gpu
def test_the_default_runs_the_grouped_kernel_on_every_case(runs):
    for name, (batch_name, H, _) in CASES.items():
        f = runs["default"][name]["facts"]
        assert f["group"] > 1 and f["group"] == group_rule(f["N"], f["E"], H, f["cap"], f["cus"]), (name, f)
        assert f["T"] == TILES, (name, f)
        assert f["tile_mode"] == ("mixed" if batch_name == "holes" else "tiles"), (name, f)
        assert f["finite"], name
        assert runs["g1"][name]["facts"]["group"] == 1 and runs["g2"][name]["facts"]["group"] == 2, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(CASES))
def test_no_switch_changes_a_bit(runs, name):
    for tag, _ in RUNS[1:]:
        diffs = runs[tag][name]["diffs"]
        assert all(n == 0 for n in diffs.values()), f"{name}: default vs {tag}: values whose bit patterns differ: {diffs}"


@pytest.mark.gpu
def test_model_is_the_same_with_the_fill_and_without(runs):
    for t1, t2, part in zip(runs["default"]["model"], runs["agg_all"]["model"], ("logits", "mask", "gate")):
        assert t1.dtype == t2.dtype and torch.equal(t1, t2), f"configs[1] at 512 graphs, {part}: default vs ISG_LC_AGG_ALL_ROWS=1"
        if t1.dtype == torch.float32:
            assert torch.equal(t1.view(torch.int32), t2.view(torch.int32)), part


if __name__ == "__main__":
    run_cases(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else None)
