"""isg_subgraph_cut / ops.subgraph_cut / isubgvqa_amd.explain on the GPU.  Every output of the cut is an integer: it is compared
EXACTLY with the plain-torch restatement of tests/subgraph_restated.py (itself pinned to a hand-written answer by
tests/test_subgraph_cpu.py), for the keep-cut and the complement-cut.  Sizes sit on the boundaries of a wave (64) and of the block
of T = ops.SUBGRAPH_BLOCK elements one workgroup ranks."""
import math

import pytest
import torch

from subgraph_restated import ptr_of, restate

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def _T():
    from isubgvqa_amd import ops
    return ops.SUBGRAPH_BLOCK


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _batch_of(sizes):
    sizes = torch.tensor(sizes, dtype=torch.long)
    return torch.repeat_interleave(torch.arange(sizes.numel()), sizes), sizes.numel()


def _sizes_about_7(N, gen):
    """Graphs of 5..9 nodes adding up to N, an empty graph after every fourth, two empty graphs at the end."""
    sizes, left = [], N
    while left > 0:
        n = min(left, int(torch.randint(5, 10, (1,), generator=gen)))
        sizes.append(n)
        left -= n
        if len(sizes) % 5 == 4:
            sizes.append(0)
    return sizes + [0, 0]


def _edges(N, E, gen):
    """E random edges over N nodes, every seventh a self-loop, every fifth a duplicate of the one before; random order."""
    if N == 0 or E == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    ei = torch.randint(0, N, (2, E), generator=gen)
    ei[1, ::7] = ei[0, ::7]
    dup = ei[:, 4::5]
    dup.copy_(ei[:, 3::5][:, :dup.size(1)])
    return ei[:, torch.randperm(E, generator=gen)].contiguous()


def _plan(batch, B, E, dev):
    """A GraphPlan with what the cut reads (ptr, batch): built by hand, since graphs here may exceed what the model kernels take."""
    from isubgvqa_amd import ops
    return ops.GraphPlan(N=batch.numel(), E=E, B=B, ptr=ptr_of(batch, B).to(torch.int32).to(dev),
                         nmax_dev=torch.zeros(1, dtype=torch.int32, device=dev), nmax=0, batch=batch.to(dev))


def _same(cut, r, what=""):
    """Every output of a SubgraphCut against the restatement, exactly."""
    assert cut.sizes() == r.counts, (what, cut.sizes(), r.counts)
    assert tuple(cut.counts.tolist()) == r.counts
    for name in ("node_new", "edge_new", "node_id", "edge_id", "edge_index", "batch", "ptr"):
        got, want = getattr(cut, name).cpu(), getattr(r, name)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, tuple(got.shape), tuple(want.shape))
        assert torch.equal(got, want), (what, name, int((got != want).sum()))
    if r.sel.size(1) == 0:
        assert cut.sel is None
    else:
        assert cut.sel.dtype == torch.int32 and torch.equal(cut.sel.cpu(), r.sel), (what, "sel")


def _cut_both(mask, ei, batch, B, dev, threshold=0.0, table_k=3, what=""):
    from isubgvqa_amd import ops
    plan = _plan(batch, B, ei.size(1), dev)
    m, e = mask.to(dev), ei.to(dev)
    cuts = []
    for complement in (False, True):
        cut = ops.subgraph_cut(m, e, plan, threshold=threshold, complement=complement, table_k=table_k)
        _same(cut, restate(mask, ei, batch, B, threshold, complement, table_k), f"{what} complement={complement}")
        cuts.append(cut)
    return cuts


def _random_case(N, dev, seed, keep=0.3, edges_per_node=2.5):
    gen = torch.Generator().manual_seed(seed)
    batch, B = _batch_of(_sizes_about_7(N, gen))
    ei = _edges(N, int(edges_per_node * N), gen)
    mask = (torch.rand(N, generator=gen) < keep).float() * (0.5 + torch.rand(N, generator=gen))
    return mask, ei, batch, B


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["0", "1", "63", "64", "65", "T-1", "T", "T+1", "2T+1"])
def test_sizes_on_the_boundaries(dev, where):
    N = eval(where.replace("2T", "2*T"), {"T": _T()})
    mask, ei, batch, B = _random_case(N, dev, seed=100 + N)
    assert batch.numel() == N and ei.size(1) == int(2.5 * N)
    _cut_both(mask, ei, batch, B, dev, what=f"N={N}")


@pytest.mark.parametrize("value", [1.0, 0.0])
def test_all_kept_and_none_kept(dev, value):
    T = _T()
    mask, ei, batch, B = _random_case(T + 70, dev, seed=7)
    keep, comp = _cut_both(torch.full_like(mask, value), ei, batch, B, dev)
    full, empty = (keep, comp) if value else (comp, keep)
    assert full.sizes() == (T + 70, ei.size(1)) and empty.sizes() == (0, 0)
    assert torch.equal(full.edge_index.cpu(), ei) and torch.equal(full.batch.cpu(), batch)


def test_no_edges(dev):
    mask, _, batch, B = _random_case(_T() + 9, dev, seed=8)
    keep, comp = _cut_both(mask, torch.zeros(2, 0, dtype=torch.long), batch, B, dev)
    assert keep.sizes()[1] == 0 and tuple(keep.edge_index.shape) == (2, 0) and keep.edge_new.numel() == 0


def test_out_of_range_endpoints_are_dropped(dev):
    N = 200
    mask, ei, batch, B = _random_case(N, dev, seed=9, keep=0.7)
    bad = torch.tensor([-1, N, N + 7])
    ei[0, 3:90:9] = bad.repeat(4)[:ei[0, 3:90:9].numel()]
    ei[1, 5:95:9] = bad.repeat(4)[:ei[1, 5:95:9].numel()]
    ei[:, 100] = torch.tensor([N + 7, -1])
    keep, comp = _cut_both(torch.ones(N), ei, batch, B, dev)
    inside = ((ei >= 0) & (ei < N)).all(0)
    assert 0 < int((~inside).sum()) and keep.sizes() == (N, int(inside.sum()))
    _cut_both(mask, ei, batch, B, dev)


@pytest.mark.parametrize("sizes", ["2T+5", "T-2,5,T+3", "3,0,0,5,0"])
def test_graphs_across_a_workgroup_boundary(dev, sizes):
    sizes = [eval(s.replace("2T", "2*T"), {"T": _T()}) for s in sizes.split(",")]
    gen = torch.Generator().manual_seed(len(sizes))
    batch, B = _batch_of(sizes)
    N = batch.numel()
    assert B == len(sizes)
    ei = _edges(N, int(2.5 * N), gen)
    mask = (torch.rand(N, generator=gen) < 0.3).float()
    _cut_both(mask, ei, batch, B, dev, table_k=4)


def test_many_workgroups(dev):
    """600 blocks of nodes, 1500 of edges: the sum over the blocks before a workgroup's own loops (256 counts per pass)."""
    N = 600 * _T() + 3
    mask, ei, batch, B = _random_case(N, dev, seed=11)
    keep, comp = _cut_both(mask, ei, batch, B, dev, table_k=2)
    assert keep.sizes()[0] + comp.sizes()[0] == N


@pytest.mark.parametrize("threshold", [0.0, 0.5])
@pytest.mark.parametrize("column", [False, True])
def test_threshold_is_strict_and_a_nan_compares_false(dev, threshold, column):
    from isubgvqa_amd import ops
    special = torch.tensor([threshold, -0.0, 0.0, -1.0, INF, -INF, NAN, 0.5, torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)).item(), 2.0, 1.0, threshold])
    mask = special.repeat(9)                                   # 108 nodes: more than a wave
    N = mask.numel()
    gen = torch.Generator().manual_seed(12)
    batch, B = _batch_of(_sizes_about_7(N, gen))
    ei = _edges(N, 300, gen)
    plan = _plan(batch, B, 300, dev)
    given = mask.view(N, 1) if column else mask
    for complement in (False, True):
        cut = ops.subgraph_cut(given.to(dev), ei.to(dev), plan, threshold=threshold, complement=complement, table_k=3)
        _same(cut, restate(mask, ei, batch, B, threshold, complement, 3))
        kept = set((cut.node_id.cpu() % special.numel()).tolist())
        above = {i for i, v in enumerate(special.tolist()) if v > threshold}          # python's comparison: NaN > t is False
        assert kept == (set(range(special.numel())) - above if complement else above)


def test_sel_lists_the_first_table_k_kept_nodes_of_every_graph(dev):
    from isubgvqa_amd import ops
    kept = [0, 1, 5, 6, 40]
    sizes = [6, 3, 9, 11, 50]
    gen = torch.Generator().manual_seed(13)
    batch, B = _batch_of(sizes)
    ptr = ptr_of(batch, B)
    mask = torch.zeros(batch.numel())
    for g, k in enumerate(kept):
        mask[ptr[g] + torch.randperm(sizes[g], generator=gen)[:k]] = 1.0
    ei = _edges(batch.numel(), 150, gen)
    keep, _ = _cut_both(mask, ei, batch, B, dev, table_k=5)
    sel = keep.sel.cpu()
    assert (sel >= 0).sum(1).tolist() == [0, 1, 5, 5, 5]
    for g in range(B):
        want = torch.nonzero(mask[ptr[g]:ptr[g + 1]]).view(-1)[:5].tolist()
        assert sel[g].tolist() == want + [-1] * (5 - len(want))
    plan = _plan(batch, B, 150, dev)
    assert ops.subgraph_cut(mask.to(dev), ei.to(dev), plan, table_k=0).sel is None
    _cut_both(mask, ei, batch, B, dev, table_k=0)


def _bits(cut):
    n, e = cut.sizes()
    return [t.clone() for t in (cut.node_new, cut.edge_new, cut.node_id, cut.edge_id, cut.edge_index, cut.batch, cut.ptr, cut.sel,
                                cut.counts)]


def test_the_same_call_gives_the_same_bits_whatever_ran_before(dev):
    from isubgvqa_amd import ops
    T = _T()
    mask, ei, batch, B = _random_case(3 * T + 17, dev, seed=14)
    plan = _plan(batch, B, ei.size(1), dev)
    m, e = mask.to(dev), ei.to(dev)
    first = _bits(ops.subgraph_cut(m, e, plan, table_k=3))
    second = _bits(ops.subgraph_cut(m, e, plan, table_k=3))
    other = _random_case(T - 5, dev, seed=15)
    _cut_both(*other, dev)
    third = _bits(ops.subgraph_cut(m, e, plan, table_k=3))
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_plan_of_a_cut_is_the_plan_of_the_restated_sub_batch(dev):
    from isubgvqa_amd import ops, synthetic
    wl = synthetic.make_workload(synthetic.WorkloadConfig(num_graphs=70, channels=8, seed=21))
    mask = (torch.rand(wl.batch.numel(), generator=torch.Generator().manual_seed(22)) < 0.4).float()
    d = wl.to(dev)
    parent = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=70, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
    cut = ops.subgraph_cut(mask.to(dev), d.edge_index, parent)
    r = restate(mask, wl.edge_index, wl.batch, 70)
    _same(cut, r)
    got = cut.plan()
    want = ops.GraphPlan.build(r.batch.to(dev), r.edge_index.to(dev), num_graphs=70, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
    assert (got.N, got.E, got.B, got.nmax, got.emax) == (want.N, want.E, want.B, wl.max_nodes, wl.max_edges) == \
        (r.counts[0], r.counts[1], 70, want.nmax, want.emax)
    for name in ("ptr", "nmax_dev", "rowptr", "eid", "src", "dst", "eptr", "batch", "edge_index"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert torch.equal(got.ptr.cpu(), r.ptr)
    ops.check_plans()


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def _hand_built(wl, r, dev):
    """The sub-batch of a Workload (on the host) by plain indexing with the restatement's lists."""
    from isubgvqa_amd import synthetic
    return synthetic.Workload(wl.x[r.node_id], r.edge_index, wl.edge_attr[r.edge_id], r.batch, wl.instr, wl.glf, wl.num_graphs,
                              wl.max_nodes, wl.max_edges, None).to(dev)


def _model_case(which):
    from isubgvqa_amd import synthetic
    if which == "A":      # the default tile kernels; nodes_min above k: removal empties no graph
        return synthetic.WorkloadConfig(num_graphs=12, channels=128, sampler="gumbel", sample_k=5, nodes_mean=14.0, nodes_min=8,
                                        nodes_max=30, edges_per_graph=30.0, seed=31), {}
    return synthetic.WorkloadConfig(num_graphs=12, channels=8, sampler="imle", sample_k=5, nodes_mean=14.0, nodes_min=8,
                                    nodes_max=30, edges_per_graph=30.0, seed=32), dict(
        fuse_logits=False, fuse_tile_conv=False, fuse_layer_conv=False, fuse_gate=False, fuse_dense_tail=False, fuse_readout=False)


def _equal_or_both_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _whole_graph_flags(flat, batch, B):
    """(kept_none, emptied) of a mask, and the two masks faithfulness() cuts by: a graph that a cut would leave without nodes keeps
    all of them (+inf under the keep-cut, -inf under the complement-cut)."""
    keep = flat > 0
    n = torch.bincount(batch, minlength=B)
    k = torch.bincount(batch[keep], minlength=B)
    kept_none, emptied = (n > 0) & (k == 0), (n > 0) & (k == n)
    return kept_none, emptied, torch.where(kept_none[batch], torch.tensor(INF), flat), torch.where(emptied[batch], torch.tensor(-INF), flat)


@pytest.mark.parametrize("which", ["A", "B"])
def test_cut_batches_and_faithfulness_equal_the_hand_built_ones(dev, which):
    """The zero pads of the sampler's padded rows compete with a graph's nodes (masking.py:162), so a top-k mask may pick fewer
    than k nodes of a graph, or none: the forwards below run on the masks faithfulness() cuts by, which leave no graph empty (they
    ARE the returned mask wherever it keeps and leaves a node of every graph)."""
    from isubgvqa_amd import explain, ops, synthetic
    cfg, switches = _model_case(which)
    B = cfg.num_graphs
    wl = synthetic.make_workload(cfg)
    d = wl.to(dev)
    model = synthetic.build_answer_model(cfg).to(dev).eval()
    seed = 5
    with ops.configured(**switches), torch.no_grad():
        logits, mask, _ = model(d, seed=seed)
        flat = mask.cpu().view(-1)
        assert 0 < int((flat > 0).sum()) <= B * cfg.sample_k
        plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=B, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
        kept_none, emptied, m_keep, m_removed = _whole_graph_flags(flat, wl.batch, B)
        assert not emptied.any()                                 # every graph has more than k nodes
        by_hand = []
        for complement, m in ((False, m_keep), (True, m_removed)):
            # the cut of the mask as the forward returned it ([N, 1]) ...
            cut = ops.subgraph_cut(mask, d.edge_index, plan, complement=complement, table_k=cfg.sample_k)
            r = restate(mask, wl.edge_index, wl.batch, B, 0.0, complement, cfg.sample_k)
            _same(cut, r, f"model {which} complement={complement}")
            got, want = explain.cut_workload(d, cut), _hand_built(wl, r, dev)
            for name in ("x", "edge_index", "edge_attr", "batch", "instr", "glf"):
                assert torch.equal(getattr(got, name), getattr(want, name)), name
            assert (got.num_graphs, got.max_nodes, got.max_edges, got.graph_sizes) == (wl.num_graphs, wl.max_nodes, wl.max_edges, None)
            # ... and the forward on the cut that leaves no graph empty
            cut = ops.subgraph_cut(m.to(dev), d.edge_index, plan, complement=complement)
            r = restate(m, wl.edge_index, wl.batch, B, 0.0, complement)
            _same(cut, r)
            assert (r.ptr[1:] > r.ptr[:-1]).all()
            got, want = explain.cut_workload(d, cut), _hand_built(wl, r, dev)
            out_got, out_want = model(got, seed=seed), model(want, seed=seed)
            for a, b in zip(out_got, out_want):
                assert torch.equal(a, b)
            by_hand.append(out_want[0])
        f = explain.faithfulness(model, d, seed=seed)
        ops.check_plans()
    assert torch.equal(f.logits, logits) and torch.equal(f.mask, mask)
    assert torch.equal(f.logits_keep, by_hand[0]) and torch.equal(f.logits_removed, by_hand[1])
    assert torch.equal(f.scores.emptied.cpu(), emptied) and torch.equal(f.kept_none.cpu(), kept_none)
    want = explain.fidelity_scores(logits, by_hand[0], by_hand[1], emptied)
    some = ~kept_none.to(dev)
    for name, a, b in zip(want._fields, f.scores, want):
        assert torch.equal(a, b) if name != "fid_minus" else torch.equal(a[some], b[some]), name
    assert torch.isnan(f.scores.fid_minus[~some]).all() and not torch.isnan(f.scores.fid_minus[some]).any()
    prob = torch.softmax(logits.double(), 1)
    pred = prob.argmax(1)
    assert torch.equal(f.scores.pred, pred)
    pk = torch.softmax(by_hand[0].double(), 1).gather(1, pred[:, None]).squeeze(1)
    pr = torch.softmax(by_hand[1].double(), 1).gather(1, pred[:, None]).squeeze(1)
    p = prob.gather(1, pred[:, None]).squeeze(1)
    # fp32 softmax over 1842 classes against fp64: a few ulp of values below 1
    assert ((f.scores.fid_minus.double() - (p - pk)).abs()[some].max() < 1e-6 and
            (f.scores.fid_plus.double() - (p - pr)).abs().max() < 1e-6)


def test_a_graph_that_removal_would_empty_goes_through_unchanged(dev):
    """Graph 0 has 4 nodes and k = 5; its explicit Gumbel noise puts the four real slots far above the pads, so all four are
    selected: removal would leave nothing.  The graph reaches the removal forward whole, is flagged and gets fid_plus = NaN."""
    from isubgvqa_amd import explain, ops, synthetic
    sizes = (4, 9, 12, 7)
    cfg = synthetic.WorkloadConfig(num_graphs=4, sizes=sizes, channels=128, sampler="gumbel", sample_k=5, edges_per_graph=30.0, seed=41)
    wl = synthetic.make_workload(cfg)
    d = wl.to(dev)
    model = synthetic.build_answer_model(cfg).to(dev).eval()
    noise = synthetic.gumbel_noise((4, wl.max_nodes), "cpu")
    noise[0, :4] = 50.0
    for g, n in enumerate(sizes):
        noise[g, n:] = -50.0                                   # no pad outranks a node (the zero pads compete: masking.py:162)
    noises = {2: noise.to(dev)}
    with torch.no_grad():
        f = explain.faithfulness(model, d, noises=noises)
        mask = f.mask.cpu().view(-1)
        assert (mask[:4] > 0).all()
        assert f.scores.emptied.tolist() == [True, False, False, False] and not f.kept_none.any()
        # what the removal forward saw: graph 0 whole, the others without their selected nodes
        flags = mask.clone()
        flags[:4] = 0.0
        r = restate(flags, wl.edge_index, wl.batch, 4, 0.0, True)
        _same(f.removed, r)
        assert f.removed.ptr.cpu().tolist()[:2] == [0, 4]
        by_hand = model(_hand_built(wl, r, dev), noises=noises)[0]
    assert torch.equal(f.logits_removed, by_hand)
    assert math.isnan(f.scores.fid_plus[0].item()) and not torch.isnan(f.scores.fid_plus[1:]).any()
    assert not torch.isnan(f.scores.fid_minus).any()
    assert _equal_or_both_nan(f.scores.fid_plus[1:], (f.scores.p - f.scores.p_removed)[1:])


def test_full_model_through_cut_scene_graphs(dev):
    from isubgvqa_amd import explain, ops, synthetic
    from isubgvqa_amd.models import build_model
    vocab = 2048
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(text_vocab_size=vocab), None).to(dev).eval()
    wl = synthetic.make_full_workload(6, tokens=8, seed=51, text_vocab=vocab)
    E = wl.edge_index.size(1)
    wl.added_sym_edge = torch.tensor([0, 3, 3, 7, E - 1, 11])
    d = wl.to(dev)

    def forward(x, ei, ea, batch, sg):
        return model(x, ei, ea, batch, d.questions, d.att_mask, return_masks=True, scene_graphs=sg)

    with torch.no_grad():
        logits, mask = forward(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs())[:2]
        plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=6, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
        cut = ops.subgraph_cut(mask, d.edge_index, plan, complement=True)
        r = restate(mask, wl.edge_index, wl.batch, 6, 0.0, True)
        _same(cut, r)
        x2, ei2, ea2, b2, sg2 = explain.cut_scene_graphs(d.x, d.edge_attr, d.scene_graphs(), cut)
        sym = r.edge_new.long()[wl.added_sym_edge]
        sym = sym[sym >= 0]
        assert 0 < sym.numel() and torch.equal(sg2.added_sym_edge.cpu(), sym)
        assert torch.equal(x2.cpu(), wl.x[r.node_id]) and torch.equal(ea2.cpu(), wl.edge_attr[r.edge_id])
        assert torch.equal(sg2.x_bbox.cpu(), wl.x_bbox[r.node_id]) and (sg2.max_nodes, sg2.max_edges) == (wl.max_nodes, wl.max_edges)
        import argparse
        hand = argparse.Namespace(x_bbox=wl.x_bbox[r.node_id].to(dev), added_sym_edge=sym.to(dev), max_nodes=wl.max_nodes,
                                  max_edges=wl.max_edges)
        got = forward(x2, ei2, ea2, b2, sg2)
        want = forward(wl.x[r.node_id].to(dev), r.edge_index.to(dev), wl.edge_attr[r.edge_id].to(dev), r.batch.to(dev), hand)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        f = explain.faithfulness(model, d)
        ops.check_plans()
    assert torch.equal(f.logits, logits) and f.scores.pred.shape == (6,)
    if not f.scores.emptied.any():
        assert torch.equal(f.logits_removed, want[0])
