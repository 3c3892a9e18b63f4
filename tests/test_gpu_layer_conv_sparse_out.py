"""A sparse launch of the grouped, masked isg_gatv2_layer_conv writes `out` and `rowmax` only where they are read:
per tile the fill writes ONE row, the tile's first row without a live in-slot; the tile's other such rows keep their row_dead
flags and their alpha entries and are not written otherwise.  isg_mgat_dense_tail's live-row form reads only listed rows, and
ops.dense_conv_out fills the others in for every other reader.  `alpha` may be left out altogether.  No bit that is read may move.

Child processes run one after another (the library reads its switches once per process).  The first runs every case through the
sparse entry point under ISG_LC_DENSE_OUT=1 -- the A/B switch: every row is written -- and saves out, alpha, the row maxima, the
dead-row flags and every output of ops.mgat_dense_tail fed with that `out`.  The others run the sparse launch on NaN-FILLED
buffers (ops.CFG.poison_sparse_out): the default, ISG_LC_GROUP=1 (the per-tile kernel: dense by construction), ISG_LC_GROUP=2,
ISG_LC_GROUP=6 and ISG_LC_TABLES=0 (the kernel scans its tiles itself: the fill is the same code).  Each loads the first one's
tensors and counts, per case and tensor, the values whose BIT PATTERNS differ (int32 views): alpha and the flags in full; out
and the maxima on every row that is not flagged dead in all four heads and on each tile's first all-dead row; the tail's h',
gated rows, planes and scales in full; ops.dense_conv_out(sparse) against the dense out and maxima in full.  Every count must be zero: a NaN that reaches a result is a row that was read and not written.

Batches as in tests/test_gpu_layer_conv_live_agg.py (400 tiles, one graph each, so that groups of more than one tile exist), its
own where the case is there already.  Heads are 4: the tail's flag word is an H = 4 contract."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_layer_conv_live_agg as LA

ROOT = LA.ROOT
NCAP, ECAP, C, K, H, TILES = LA.NCAP, LA.ECAP, LA.C, LA.K, 4, LA.TILES
RUNS = (("dense", {"ISG_LC_DENSE_OUT": "1"}), ("sparse", {}), ("g1", {"ISG_LC_GROUP": "1"}), ("g2", {"ISG_LC_GROUP": "2"}),
        ("g6", {"ISG_LC_GROUP": "6"}), ("tables0", {"ISG_LC_TABLES": "0"}))
SWITCHES = LA.SWITCHES + ("ISG_LC_DENSE_OUT", "ISG_DT_DENSE_ROWS")
TAIL_GROUP = 3                       # the product's at configs[1] (ops.dense_tail_group)
# case -> (batch, bias: "random" / None / "negzero", lin_l zeroed, the tail's tiles per workgroup)
CASES = {"none_picked": ("none_picked", "random", False, TAIL_GROUP), "all_picked": ("all_picked", "random", False, TAIL_GROUP),
         "last_row_fill": ("last_row_fill", "random", False, TAIL_GROUP), "first_row_fill": ("first_row_fill", "random", False, TAIL_GROUP),
         "zero_lin_l": ("picked", "random", True, TAIL_GROUP), "hub": ("hub", "random", False, TAIL_GROUP),
         "source_only": ("source_only", "random", False, TAIL_GROUP), "edge_mask": ("edge_mask", "random", False, TAIL_GROUP),
         "no_bias": ("picked", None, False, TAIL_GROUP), "negzero_bias": ("picked", "negzero", False, TAIL_GROUP),
         "holes": ("holes", "random", False, TAIL_GROUP), "tail_over_64": ("all_but_one", "random", False, 4),
         "tail_over_64_sparse_rows": ("four_busy_tiles", "random", False, 4)}
CONV_PARTS = ("out", "alpha", "row maxima", "dead rows")
TAIL_PARTS = ("h'", "gated rows", "planes", "plane scales")
BUSY_LIVE = tuple(range(0, 2)) + tuple(range(6, 20))        # 16 live rows of a busy tile: its first fill row is row 2


# ----------------------------------------------------------------------------------------------------------------- batches
def loops_graph(n, m, gen):
    return n, [(i, i) for i in range(n)] + [tuple(p) for p in torch.randint(0, n, (2, m), generator=gen).t().tolist()]


def case_inputs(batch_name):
    """{batch, ei, B, spans, nm, em}: the live-aggregation test's batch of that name, or one of this file's."""
    if batch_name not in ("last_row_fill", "first_row_fill", "all_but_one", "four_busy_tiles"):
        return LA.case_inputs(batch_name)
    gen = torch.Generator().manual_seed(sum(map(ord, batch_name)) + 20)
    if batch_name in ("last_row_fill", "first_row_fill"):
        special = [loops_graph(30, 60, gen)]              # (30 + 36 nodes pass a tile: it stays alone in its tile)
    elif batch_name == "four_busy_tiles":
        special = [loops_graph(40, 60, gen) for _ in range(4)]
    else:
        special = []
    graphs = special + [LA.plain_graph(gen) for _ in range(TILES - len(special))]
    batch, ei, spans = LA.assemble(graphs, gen)
    N, E = batch.numel(), ei.size(1)
    nm = em = None
    if batch_name == "all_but_one":                       # every node picked but one per tile: lists of 35 rows and more per tile
        nm = torch.ones(N)
        for r0, n in spans:
            nm[r0 + int(torch.randint(0, n, (1,), generator=gen))] = 0.0
    else:                                                 # live slots are self-loops: a row is live-destination iff its loop is live
        loop_of = {int(s): e for e, (s, t) in enumerate(ei.t().tolist()) if s == t}
        em = torch.zeros(E)
        for t, (r0, n) in enumerate(spans):
            if t < len(special):
                if batch_name == "last_row_fill":
                    rows = range(n - 1)
                elif batch_name == "first_row_fill":
                    rows = range(1, n)
                else:
                    rows = BUSY_LIVE
            else:
                rows = [int(torch.randint(0, n, (1,), generator=gen))]        # one live row per plain tile
            for r in rows:
                em[loop_of[r0 + r]] = 1.0
    return {"batch": batch, "ei": ei, "B": len(graphs), "spans": spans, "nm": nm, "em": em}


def read_rows(dead, spans):
    """The rows of `out` / `rowmax` that a reader may look at: every row that is not flagged dead in every head, and each tile's
    first all-dead row (the rows of a graph beyond a tile are never flagged).  -> bool [N]"""
    alldead = (dead != 0).all(dim=1)
    keep = ~alldead
    for r0, n in spans:
        idx = torch.nonzero(alldead[r0:r0 + n])
        if n <= NCAP and idx.numel():
            keep[r0 + int(idx[0])] = True
    return keep


def test_case_batches_hold_what_they_are_named_for():
    sets = {name: (case_inputs(name), None) for name in sorted({b for b, _, _, _ in CASES.values()})}
    sets = {name: (c, LA.tile_sets(c)) for name, (c, _) in sets.items()}
    for name, (batch_name, _, _, _) in CASES.items():
        c, s = sets[batch_name]
        assert c["B"] == TILES and LA.group_rule(c["batch"].numel(), c["ei"].size(1), H, TILES) > 1, name
    fills = lambda t: [r for r in range(len(t[2])) if r not in t[0]]
    c, s = sets["none_picked"]
    assert all(fills(t) == list(range(len(t[2]))) for t in s)                       # every row is a fill row: row 0 represents
    c, s = sets["all_picked"]
    assert all(not fills(t) for t in s)                                             # no dead row anywhere: no representative
    c, s = sets["last_row_fill"]
    assert fills(s[0]) == [len(s[0][2]) - 1] and len(s[0][2]) == 30
    c, s = sets["first_row_fill"]
    assert fills(s[0]) == [0]
    for name in ("last_row_fill", "first_row_fill"):                                # any group with that tile stays within 64 rows
        assert all(len(t[1]) == 1 for t in sets[name][1][1:]) and len(sets[name][1][0][1]) == 29
    c, s = sets["hub"]
    assert s[0][0] == {7} and s[0][2][7] == ECAP
    c, s = sets["source_only"]
    assert all(len(tc - ld) >= 1 for ld, tc, _, _ in s)                             # named rows that are fill rows
    c, s = sets["edge_mask"]
    assert {v.item() for v in c["em"].view(torch.int32)} == {v.item() for v in torch.tensor(LA.MASK_VALUES).view(torch.int32)}
    c, s = sets["picked"]
    assert any(t[0] and fills(t) for t in s) and any(not t[0] for t in s)
    c, s = sets["holes"]
    assert s[TILES // 2] is None and sum(x is None for x in s) == 1
    c, s = sets["all_but_one"]                                                      # four consecutive tiles: far more than 64 live rows
    assert all(len(fills(t)) == 1 and len(t[0]) >= 35 for t in s)
    c, s = sets["four_busy_tiles"]                                                  # 4 x 16 live rows + a dead one = 65 > 64 for the
    assert all(s[t][0] == set(BUSY_LIVE) and fills(s[t])[0] == 2 for t in range(4))  # tail; 16 named rows per tile for the conv
    assert all(len(t[1]) == 1 for t in s[4:]) and 4 * len(BUSY_LIVE) + 1 > NCAP and 3 * len(BUSY_LIVE) + 3 <= NCAP


# ------------------------------------------------------------------------------------------------------------ child process
def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.float16 else t


def count_diffs(t1, t2, rows=None):
    assert t1.shape == t2.shape and t1.dtype == t2.dtype
    v1, v2 = bits(t1), bits(t2)
    if rows is not None:
        v1, v2 = v1[rows], v2[rows]
    return int((v1 != v2).sum())


def run_cases(out_path, ref_path):
    """Child: every case on cuda:0 under this process's switches.  Without ref_path (ISG_LC_DENSE_OUT=1) the tensors are saved; with
    it the sparse launch runs on NaN-filled buffers, is compared with the saved ones, and the counts are saved."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import _lib_masked, ops, synthetic
    from isubgvqa_amd.models.layers import GlorotLinear, GraphNorm
    dev = torch.device("cuda:0")
    ref = torch.load(ref_path) if ref_path else None
    mlib = _lib_masked.load()
    d = lambda t: None if t is None else t.to(dev)
    res, batches = {}, {}
    for ci, (name, (batch_name, bias_mode, zero_l, tail_group)) in enumerate(CASES.items()):
        if batch_name not in batches:
            batches[batch_name] = case_inputs(batch_name)
        c = batches[batch_name]
        batch, ei, B, nm, em, spans = c["batch"], c["ei"], c["B"], c["nm"], c["em"], c["spans"]
        gen = torch.Generator().manual_seed(1200 + ci)
        N, E = batch.numel(), ei.size(1)
        x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-3, 4, (B,), generator=gen).float())[batch][:, None]
        ea = torch.randn(E, K, generator=gen)
        w = torch.randn(H * C, K, generator=gen) * 0.1
        att, bias = torch.randn(1, H, C, generator=gen), LA.make_bias(bias_mode, H, gen)
        ins, ins_next, h = torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen), torch.randn(N, C, generator=gen)
        tail_mask = LA.straight_through(gen, N, 0.13)
        torch.manual_seed(ci)
        lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
        x_proj = torch.nn.Sequential(torch.nn.Linear(H * C, 2 * C), torch.nn.GELU(), torch.nn.Linear(2 * C, C), torch.nn.GELU()).to(dev)
        bn = GraphNorm(C).to(dev)
        with torch.no_grad():
            bn.weight.normal_(1.0, 0.1), bn.bias.normal_(0.0, 0.1), bn.mean_scale.normal_(1.0, 0.1)
            if zero_l:                 # x_l = +0 everywhere: every aggregated row keeps all-zero accumulators and is flagged
                lin_l.weight.zero_(), lin_l.bias.zero_()
        # a batch with one graph beyond a tile is dispatched as mixed only with that dispatch's floors lowered
        with torch.no_grad(), ops.configured(mixed_max_fraction=0.9, mixed_min_nodes=0, poison_sparse_out=ref is not None):
            plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
            o, a = ops.gatv2_layer_conv(d(x), lin_l, lin_r, d(ea), d(w), d(att), plan, H, bias=d(bias), node_mask=d(nm),
                                        edge_mask=d(em), want_rowmax=True, sparse_out=True)
            dead = ops.dead_rows(o)
            conv = (o.cpu(), a.cpu(), ops.row_maxima(o).cpu(), dead.cpu())
            assert ops.dense_tail_supported(plan, x_proj, H * C, C)
            h_out, xg, xp = ops.mgat_dense_tail(o, x_proj, d(ins), d(h), plan, bn.weight, bn.bias, bn.mean_scale, bn.eps,
                                                node_mask=d(tail_mask), ins_next=d(ins_next), want_rows=True, want_planes=True,
                                                group=tail_group)
            tail = (h_out.cpu(), xg.cpu(), xp.planes[:N].cpu(), xp.inv[:N].cpu())
            full = ops.dense_conv_out(o)
            filled = (full.cpu(), ops.row_maxima(full).cpu())
            _, ntiles, cap, _ = plan.tiles(NCAP, ECAP)
            facts = {"group": int(mlib.isg_gatv2_layer_conv_group(N, E, H, cap)), "tile_mode": plan.tile_mode(NCAP, ECAP),
                     "T": int(ntiles.item()), "marked": ops.is_sparse_conv_out(o), "filled_is_out": full is o,
                     "finite": all(bool(torch.isfinite(t.float()).all()) for t in (filled[0], filled[1], conv[1]) + tail),
                     "rows_with_nan": int(torch.isnan(conv[0]).any(dim=1).sum()),
                     "busy_rows_with_nan": [int(torch.isnan(conv[0][r0:r0 + n]).any(dim=1).sum()) for r0, n in spans[:4]]}
        if ref is None:
            res[name] = {"conv": conv, "tail": tail, "facts": facts}
        else:
            rconv, rtail = ref[name]["conv"], ref[name]["tail"]
            rows = read_rows(rconv[3], spans)
            diffs = {"alpha": count_diffs(rconv[1], conv[1]), "dead rows": count_diffs(rconv[3], conv[3]),
                     "out, rows that are read": count_diffs(rconv[0], conv[0], rows),
                     "row maxima, rows that are read": count_diffs(rconv[2], conv[2], rows),
                     "dense_conv_out": count_diffs(rconv[0], filled[0]), "dense_conv_out's maxima": count_diffs(rconv[2], filled[1])}
            diffs.update({part: count_diffs(t1, t2) for t1, t2, part in zip(rtail, tail, TAIL_PARTS)})
            res[name] = {"diffs": diffs, "facts": facts, "read_rows": int(rows.sum())}
    if ref is not None and os.environ.get("ISG_LC_GROUP") is None and os.environ.get("ISG_LC_TABLES") is None:
        res["alpha_none"] = alpha_none(ops, batches["picked"], dev)
        res["model"] = model_runs(ops, synthetic, dev)
    torch.save(res, out_path)


def alpha_none(ops, c, dev):
    """out / row maxima / flags with and without the attention weights, a masked launch and an unmasked one -> differing values."""
    from isubgvqa_amd.models.layers import GlorotLinear
    gen = torch.Generator().manual_seed(77)
    N, E = c["batch"].numel(), c["ei"].size(1)
    x, ea, w = torch.randn(N, 128, generator=gen), torch.randn(E, K, generator=gen), torch.randn(H * C, K, generator=gen) * 0.1
    att, bias = torch.randn(1, H, C, generator=gen), LA.make_bias("random", H, gen)
    torch.manual_seed(5)
    lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
    out = {}
    with torch.no_grad():
        plan = ops.GraphPlan.build(c["batch"].to(dev), c["ei"].to(dev), num_graphs=c["B"])
        for tag, nm in (("masked", c["nm"].to(dev)), ("unmasked", None)):
            runs = [ops.gatv2_layer_conv(x.to(dev), lin_l, lin_r, ea.to(dev), w.to(dev), att.to(dev), plan, H, bias=bias.to(dev),
                                         node_mask=nm, want_rowmax=True, want_alpha=wa) for wa in (True, False)]
            (o1, a1), (o2, a2) = runs
            parts = [(o1, o2), (ops.row_maxima(o1), ops.row_maxima(o2))] + ([(ops.dead_rows(o1), ops.dead_rows(o2))] if nm is not None else [])
            out[tag] = {"alpha_is_none": a2 is None, "alpha_finite": bool(torch.isfinite(a1).all()),
                        "diffs": [count_diffs(p.cpu(), q.cpu()) for p, q in parts]}
    return out


def model_runs(ops, synthetic, dev):
    """BASELINE configs[1]'s model at 512 graphs: the default, both switches off, the default on NaN-filled buffers; and MGAT alone
    with return_attention."""
    cfg = dataclasses.replace(synthetic.CFG2, num_graphs=512)
    wl = synthetic.make_workload(cfg).to(dev)
    net = synthetic.build_answer_model(cfg).to(dev).eval()
    out = {}
    with torch.no_grad():
        out["default"] = tuple(t.cpu() for t in net(wl, seed=1000))
        with ops.configured(sparse_conv_out=False, skip_unread_alpha=False):
            out["off"] = tuple(t.cpu() for t in net(wl, seed=1000))
        with ops.configured(poison_sparse_out=True):
            out["poison"] = tuple(t.cpu() for t in net(wl, seed=1000))
        plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=wl.glf.size(0))
        kw = dict(x=wl.x, edge_index=wl.edge_index, edge_attr=wl.edge_attr, instr_vectors=wl.instr[:4], global_language_feats=wl.glf,
                  batch=wl.batch, return_masks=True, plan=plan, seed=1000)
        h0, m0, _, _ = net.gat_seq(**kw)
        h1, m1, _, _, attn = net.gat_seq(return_attention=True, **kw)
        out["attention"] = {"h_diffs": count_diffs(h0.cpu(), h1.cpu()), "mask_equal": bool(torch.equal(m0, m1)), "layers": len(attn),
                            "shapes": [tuple(a[1].shape) for a in attn], "E": wl.edge_index.size(1),
                            "finite": all(bool(torch.isfinite(a[1]).all()) for a in attn)}
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    d = tmp_path_factory.mktemp("sparse_out")
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
def test_every_case_runs_the_launch_it_is_meant_for(runs):
    for name, (batch_name, _, _, _) in CASES.items():
        for tag, _ in RUNS:
            f = runs[tag][name]["facts"]
            assert f["T"] == TILES and f["finite"], (name, tag, f)
            assert f["tile_mode"] == ("mixed" if batch_name == "holes" else "tiles"), (name, tag, f)
            assert f["marked"] == (tag != "g1") and f["filled_is_out"] == (tag == "g1"), (name, tag, f)
        assert runs["dense"][name]["facts"]["group"] > 1 and runs["dense"][name]["facts"]["rows_with_nan"] == 0, name
        assert runs["g1"][name]["facts"]["group"] == 1 and runs["g1"][name]["facts"]["rows_with_nan"] == 0, name
        assert runs["g2"][name]["facts"]["group"] == 2 and runs["g6"][name]["facts"]["group"] == 6, name
    for tag in ("sparse", "g2", "g6", "tables0"):
        # no row has a live in-slot: every tile's row 0 is written and nothing else (a group's list is empty: never the fall-back)
        c = case_inputs("none_picked")
        assert runs[tag]["none_picked"]["facts"]["rows_with_nan"] == c["batch"].numel() - TILES, tag
        assert runs[tag]["all_picked"]["facts"]["rows_with_nan"] == 0, tag                # no fill row: nothing is left out
    # the tiles whose rows the tail's over-64 fall-back reads through the redirection were written sparsely: 40 rows, 16 of them
    # live, the first fill row written, 23 left as they were
    assert runs["sparse"]["tail_over_64_sparse_rows"]["facts"]["busy_rows_with_nan"] == [23] * 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(CASES))
def test_no_bit_that_is_read_moves(runs, name):
    for tag, _ in RUNS[1:]:
        diffs = runs[tag][name]["diffs"]
        assert runs[tag][name]["read_rows"] > 0
        assert all(n == 0 for n in diffs.values()), f"{name}: ISG_LC_DENSE_OUT=1 vs {tag}: values whose bit patterns differ: {diffs}"


@pytest.mark.gpu
def test_alpha_is_optional(runs):
    for tag, r in runs["sparse"]["alpha_none"].items():
        assert r["alpha_is_none"] and r["alpha_finite"] and all(n == 0 for n in r["diffs"]), (tag, r)
    a = runs["sparse"]["model"]["attention"]
    assert a["h_diffs"] == 0 and a["mask_equal"] and a["finite"] and a["layers"] == 3 and a["shapes"] == [(a["E"], H)] * 3, a


@pytest.mark.gpu
def test_model_is_the_same_with_both_switches_off_and_on_poisoned_buffers(runs):
    m = runs["sparse"]["model"]
    for other in ("off", "poison"):
        for t1, t2, part in zip(m["default"], m[other], ("logits", "mask", "gate")):
            assert t1.dtype == t2.dtype and count_diffs(t1, t2) == 0, f"configs[1] at 512 graphs, {part}: default vs {other}"
    assert bool(torch.isfinite(m["poison"][0]).all())


if __name__ == "__main__":
    run_cases(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else None)
