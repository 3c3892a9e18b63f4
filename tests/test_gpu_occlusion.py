"""explain.occlusion, explain.faithfulness_of_mask and explain.compare on the GPU.  occlusion() forwards the batch of
leave-one-out instances that ops.induced_instances makes in one pass; here the same model is called on the batch that the CHAIN
builds from the same inputs (ops.graph_instances, a float mask from the bits, ops.subgraph_cut) and the results are compared as
bits: equal inputs take equal kernels, so there is no tolerance.  Chunked against unchunked is NOT compared as floats -- which GEMM
a row meets depends on the batch size -- only the chunks' instance lists are, as integers."""
import argparse
import math

import pytest
import torch

from test_gpu_models import LOGIT_TOL

pytestmark = pytest.mark.gpu

SIZES = (1, 9, 4, 2, 6)          # 5 graphs of 1 to 9 nodes: one that gets no instance, one whose instances have one node
K = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        f"{what}: bits differ, max |d| = {(a - b).abs().max().item():.3e}"


def _answer_case(dev, seed=5):
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=len(SIZES), channels=128, layers=3, masks=(1.0, 1.0, 0.15), sampler="imle",
                                   sample_k=K, edges_per_graph=0.0, seed=seed, sizes=SIZES)
    model = synthetic.build_answer_model(cfg).eval().to(dev)
    return model, synthetic.make_workload(cfg).to(dev)


@pytest.fixture(scope="module")
def answer_case(dev):
    return _answer_case(dev)


def chain_instances(ops, plan, edge_index, index, keep):
    """The two steps: every graph of `index` copied out whole, a float mask from the bits, the cut -> (whole, cut)."""
    whole = ops.graph_instances(plan, edge_index, index)
    local = whole.node_src - plan.ptr.long()[index.long()][whole.batch]
    mask = ((keep.long()[whole.batch, local >> 5] >> (local & 31)) & 1).float()
    return whole, ops.subgraph_cut(mask, whole.edge_index, whole.plan())


def chain_probabilities(ops, model, d, plan, index, keep, pred):
    """The AnswerModel on the chain-built batch of the instances (index, keep): the predicted class's probability per instance."""
    from isubgvqa_amd import synthetic
    whole, cut = chain_instances(ops, plan, d.edge_index, index, keep)
    rows = index.long()
    wl = synthetic.Workload(d.x.index_select(0, whole.node_src[cut.node_id]), cut.edge_index,
                            d.edge_attr.index_select(0, whole.edge_src[cut.edge_id]), cut.batch,
                            d.instr.index_select(1, rows).contiguous(), d.glf.index_select(0, rows), rows.numel(), d.max_nodes,
                            d.max_edges, None)
    logits = model(wl, plan=cut.plan())[0]
    return torch.softmax(logits.float(), dim=1).gather(1, pred.index_select(0, rows).unsqueeze(1)).squeeze(1), whole, cut


def _plan(ops, d, B):
    return ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=B, max_nodes=d.max_nodes or None, max_edges=d.max_edges or None,
                               graph_sizes=d.graph_sizes)


def test_occlusion_in_one_chunk_equals_the_model_on_the_chain_built_batch(answer_case, dev):
    from isubgvqa_amd import explain, ops
    model, d = answer_case
    B, N = len(SIZES), sum(SIZES)
    occ = explain.occlusion(model, d)
    with torch.no_grad():
        plan = _plan(ops, d, B)
        logits = model(d, plan=plan)[0]
        prob = torch.softmax(logits.float(), dim=1)
        pred = prob.argmax(dim=1)
        p = prob.gather(1, pred.unsqueeze(1)).squeeze(1)
        index, keep, inst_node = ops.keep_bits_leave_one_out(plan)
        assert index.tolist() == [g for g, n in enumerate(SIZES) if n >= 2 for _ in range(n)]
        p_without, whole, cut = chain_probabilities(ops, model, d, plan, index, keep, pred)
    assert torch.equal(occ.pred, pred) and torch.equal(occ.index, index) and torch.equal(occ.inst_node, inst_node)
    _same_bits(occ.logits, logits, "logits")
    _same_bits(occ.p, p, "p")
    _same_bits(occ.p_without, p_without, "p without each node")
    want = torch.zeros(N, device=dev)
    want[inst_node] = p[index.long()] - p_without
    _same_bits(occ.attribution, want, "attribution")
    assert occ.single.tolist() == [n < 2 for n in SIZES] and float(occ.attribution[0]) == 0.0      # the one-node graph
    assert int((occ.attribution != 0).sum()) > N // 2
    assert len(occ.chunks) == 1 and isinstance(occ.chunks[0], ops.InducedInstances)
    inst = occ.chunks[0]
    assert torch.equal(inst.node_src, whole.node_src[cut.node_id]) and torch.equal(inst.edge_index, cut.edge_index)
    # the k-hot mask: k nodes per graph (fewer where the graph is smaller), no NaN, the layout of the forward's mask
    m = occ.mask(K)
    assert tuple(m.shape) == (N, 1) and m.dtype == torch.float32
    per_graph = torch.zeros(B, device=dev).index_add_(0, d.batch, m.squeeze(1))
    distinct = all(len(set(occ.attribution[s:e].tolist())) == e - s for s, e in zip(plan.ptr.tolist()[:-1], plan.ptr.tolist()[1:]))
    if distinct:
        assert per_graph.tolist() == [float(min(K, n)) for n in SIZES]
    top = [int(occ.attribution[s:e].argmax()) + s for s, e in zip(plan.ptr.tolist()[:-1], plan.ptr.tolist()[1:])]
    assert bool((m[top] == 1).all()), "a graph's largest attribution is not in its mask"
    ops.check_plans()


def test_occlusion_in_chunks_of_seven(answer_case, dev):
    from isubgvqa_amd import explain, ops
    model, d = answer_case
    B = len(SIZES)
    occ, occ7 = explain.occlusion(model, d), explain.occlusion(model, d, max_instances=7)
    Q = occ.index.numel()
    assert Q == 21 and [c.Q for c in occ7.chunks] == [7, 7, 7] and torch.equal(occ7.index, occ.index)
    whole = occ.chunks[0]
    n_off = e_off = q_off = 0
    parts = {k: [] for k in ("batch", "node_src", "edge_src", "edge_index", "ptr", "eptr")}
    for c in occ7.chunks:                                         # the chunks' lists, renumbered into one batch
        parts["batch"].append(c.batch + q_off)
        parts["node_src"].append(c.node_src)
        parts["edge_src"].append(c.edge_src)
        parts["edge_index"].append(c.edge_index + n_off)
        parts["ptr"].append(c.ptr[:-1] + n_off)
        parts["eptr"].append(c.eptr[:-1] + e_off)
        n_off, e_off, q_off = n_off + c.batch.numel(), e_off + c.edge_src.numel(), q_off + c.Q
    for k, v in parts.items():
        got = torch.cat(v, dim=1 if k == "edge_index" else 0)
        want = getattr(whole, k) if k not in ("ptr", "eptr") else getattr(whole, k)[:-1]
        assert torch.equal(got, want), f"the chunks' {k} do not concatenate to the unchunked list"
    assert (n_off, e_off) == (whole.batch.numel(), whole.edge_src.numel())
    with torch.no_grad():
        plan = _plan(ops, d, B)
        index, keep, _ = ops.keep_bits_leave_one_out(plan)
        for lo in range(0, Q, 7):
            got = occ7.p_without[lo:lo + 7]
            want, _, _ = chain_probabilities(ops, model, d, plan, index[lo:lo + 7].contiguous(), keep[lo:lo + 7].contiguous(), occ.pred)
            _same_bits(got, want, f"instances {lo} to {lo + 7}")
    with pytest.raises(ValueError, match="max_instances"):
        explain.occlusion(model, d, max_instances=0)


def test_occlusion_through_the_full_model_with_added_sym_edges(dev):
    """The small ISubGVQA of tests/test_gpu_instances.py on 3 graphs with a non-empty added_sym_edge: the same comparison through
    forward(), including the added_sym_edge list carried onto the instances."""
    from isubgvqa_amd import explain, ops, synthetic
    from test_gpu_instances import _model
    model = _model().to(dev)
    sizes = (3, 7, 5)
    wl = synthetic.make_full_workload(3, tokens=9, seed=3, text_vocab=512, sizes=sizes)
    E = wl.edge_index.size(1)
    wl.added_sym_edge = torch.tensor([0, 2, 2, 5, E - 1])                 # with a repeat: the encoder flips that edge once
    d = wl.to(dev)
    occ = explain.occlusion(model, d)
    with torch.no_grad():
        plan = _plan(ops, d, 3)
        sg = d.scene_graphs()
        logits = model(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, return_masks=True, scene_graphs=sg, plan=plan)[0]
        prob = torch.softmax(logits.float(), dim=1)
        pred = prob.argmax(dim=1)
        p = prob.gather(1, pred.unsqueeze(1)).squeeze(1)
        index, keep, inst_node = ops.keep_bits_leave_one_out(plan)
        assert index.numel() == sum(sizes)
        whole, cut = chain_instances(ops, plan, d.edge_index, index, keep)
        named = torch.isin(whole.edge_src, d.added_sym_edge)           # every copied edge that the old list names
        sym = cut.remap_edge_positions(torch.nonzero(named).reshape(-1))
        assert sym.numel() > 4
        src_n, src_e = whole.node_src[cut.node_id], whole.edge_src[cut.edge_id]
        sg2 = argparse.Namespace(x_bbox=d.x_bbox.index_select(0, src_n), added_sym_edge=sym, max_nodes=d.max_nodes, max_edges=d.max_edges)
        rows = index.long()
        out = model(d.x.index_select(0, src_n), cut.edge_index, d.edge_attr.index_select(0, src_e), cut.batch,
                    d.questions.index_select(0, rows), d.att_mask.index_select(0, rows), return_masks=True, scene_graphs=sg2,
                    plan=cut.plan())[0]
        p_without = torch.softmax(out.float(), dim=1).gather(1, pred.index_select(0, rows).unsqueeze(1)).squeeze(1)
    used = explain.instance_inputs(d, occ.chunks[0], True)[4]
    assert torch.equal(used.added_sym_edge, sym) and torch.equal(used.x_bbox, sg2.x_bbox)
    assert torch.equal(occ.pred, pred)
    _same_bits(occ.p, p, "p")
    _same_bits(occ.p_without, p_without, "p without each node")
    want = torch.zeros(sum(sizes), device=dev)
    want[inst_node] = p[rows] - p_without
    _same_bits(occ.attribution, want, "attribution")
    assert not bool(occ.single.any())
    ops.check_plans()


def test_faithfulness_of_the_forwards_mask_equals_faithfulness(answer_case):
    from isubgvqa_amd import explain
    model, d = answer_case
    f = explain.faithfulness(model, d)
    g = explain.faithfulness_of_mask(model, d, f.mask)
    for name in explain.Fidelity._fields:
        a, b = getattr(f.scores, name), getattr(g.scores, name)
        if a.dtype == torch.float32:
            _same_bits(a, b, name)
        else:
            assert torch.equal(a, b), name
    for name in ("logits", "logits_keep", "logits_removed", "mask"):
        _same_bits(getattr(f, name), getattr(g, name), name)
    assert torch.equal(f.kept_none, g.kept_none)
    for cut_f, cut_g in ((f.keep, g.keep), (f.removed, g.removed)):
        assert torch.equal(cut_f.node_id, cut_g.node_id) and torch.equal(cut_f.edge_index, cut_g.edge_index)
    # another mask than the model's own: the fidelity of keeping everything is 0 where removal would have emptied the graph
    ones = torch.ones_like(f.mask)
    h = explain.faithfulness_of_mask(model, d, ones)
    assert bool(h.scores.emptied.all()) and bool(torch.isnan(h.scores.fid_plus).all())
    # (the keep forward runs under the cut's plan, built without the host's graph sizes: the bound between kernel paths holds)
    assert float((h.logits_keep - h.logits).abs().max()) < LOGIT_TOL and not bool(torch.isnan(h.scores.fid_minus).any())


def test_compare_totals_equal_the_explainers_called_one_by_one(dev):
    from isubgvqa_amd import explain, ops, synthetic
    V, A = 200, 1842
    tables = explain.TokenTables({f"w{i}": i for i in range(V)}, [f"w{(11 * a) % V}" if a % 3 == 0 else f"answer {a}" for a in range(A)])
    model, _ = _answer_case(dev)
    gen = torch.Generator().manual_seed(13)
    batches = []
    with torch.no_grad():
        for seed in (5, 6):
            d = _answer_case(dev, seed)[1]
            B, N = len(SIZES), sum(SIZES)
            names = torch.randint(0, V, (N,), generator=gen)
            label = model(d)[0].argmax(1).cpu()
            label[1::2] = (label[1::2] + 1) % A
            qtok = torch.full((B, 4), -1, dtype=torch.int32)
            qtok[:, :3] = torch.randint(0, V, (B, 3), generator=gen).int()
            qtok[:, 0] = names[torch.tensor([0, 1, 10, 14, 16])].int()
            gold = synthetic.make_gold(SIZES, facets=2, entries=3, seed=seed)
            batches.append(explain.EvalBatch(d, label.to(dev), qtok.to(dev), (torch.arange(B) % 2).int().to(dev), names.to(dev),
                                             gold=gold.to(dev)))
    report = explain.compare(model, batches, tables, k=K, seed=40)
    assert tuple(report) == explain.EXPLAINERS
    with pytest.raises(ValueError, match="explainers"):
        explain.compare(model, batches, tables, explainers=("gradient",))
    with torch.no_grad():
        for name in explain.EXPLAINERS:
            coo = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
            ground = torch.zeros(ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
            plus, minus, jac = [], [], []
            for number, b in enumerate(batches):
                d = b.inputs
                plan = _plan(ops, d, len(SIZES))
                logits, intrinsic, _ = model(d, plan=plan)
                mask = {"intrinsic": lambda: intrinsic, "occlusion": lambda: explain.occlusion(model, d).mask(K),
                        "random": lambda: explain.random_mask(plan, K, 40 + number)}[name]()
                pred = logits.argmax(1)
                ops.token_coo(b.names, mask, plan, pred, b.label, tables.on("ans_sg", dev), b.qtok, b.qflags, totals=coo)
                ops.grounding(mask, plan, b.gold, pred, b.label, totals=ground)
                f = explain.faithfulness_of_mask(model, d, mask).scores
                plus += [v for v in f.fid_plus.double().tolist() if not math.isnan(v)]
                minus += [v for v in f.fid_minus.double().tolist() if not math.isnan(v)]
                a, c = (mask.reshape(-1) > 0).tolist(), (intrinsic.reshape(-1) > 0).tolist()
                for s, e in zip(plan.ptr.tolist()[:-1], plan.ptr.tolist()[1:]):
                    union = sum(x or y for x, y in zip(a[s:e], c[s:e]))
                    if union:
                        jac.append(sum(x and y for x, y in zip(a[s:e], c[s:e])) / union)
            r = report[name]
            assert r.coo.totals == tuple(coo.tolist()), name
            assert r.grounding.totals == tuple(ground.tolist()), name
            assert (r.sums[1], r.sums[3], r.sums[5]) == (len(plus), len(minus), len(jac)), name
            for got, vals in ((r.fid_plus, plus), (r.fid_minus, minus), (r.jaccard, jac)):
                assert vals and got == pytest.approx(math.fsum(vals) / len(vals), rel=1e-12, abs=1e-15), name
        assert report["intrinsic"].jaccard == 1.0 and report["intrinsic"].coo.totals[0] == 2 * len(SIZES)
        assert report["random"].coo.totals != report["intrinsic"].coo.totals or report["random"].jaccard < 1.0
    ops.check_plans()
