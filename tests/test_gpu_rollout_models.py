"""The attention trace and explain.attention_rollout through the models, on the GPU: a small AnswerModel (C = 128,
3 layers, I-MLE, 12 graphs, one of 70 nodes) and the small ISubGVQA of tests/test_gpu_occlusion.py.  A forward with a trace gives
the bits of the forward without it; the trace's weights are MGAT's own; under ops.run_split the weights merge by edge and every
row is written; the attribution equals the restatement of tests/rollout_restated.py fed the trace's own tensors, at the bound
derived in tests/test_gpu_rollout.py (|got - ref| <= 2 k u ref, k = L (H + d + 6): attention weights, gates and masks are
non-negative); compare() takes "attention" and keeps its default."""
import math

import pytest
import torch

import rollout_restated as RR
from test_gpu_occlusion import _answer_case, _plan
from test_gpu_occlusion import SIZES as SMALL_SIZES

pytestmark = pytest.mark.gpu

SIZES = (5, 9, 70, 3, 12, 1, 20, 33, 2, 64, 7, 16)       # 12 graphs, one beyond a 64-node tile, one that fills one
K = 3
U = 2.0 ** -24
ALPHA_TOL = dict(atol=1e-6, rtol=1e-5)                   # tests/test_gpu_models.py: attention weights between two kernel paths


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def answer(dev):
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=len(SIZES), channels=128, layers=3, masks=(1.0, 1.0, 0.15), sampler="imle",
                                   sample_k=K, edges_per_graph=0.0, seed=9, sizes=SIZES)
    return synthetic.build_answer_model(cfg).eval().to(dev), synthetic.make_workload(cfg).to(dev)


@pytest.fixture(scope="module")
def full(dev):
    from isubgvqa_amd import synthetic
    from test_gpu_instances import _model
    sizes = (3, 7, 5, 66)
    return _model().to(dev), synthetic.make_full_workload(len(sizes), tokens=9, seed=3, text_vocab=512, sizes=sizes).to(dev), sizes


def _mixed(ops, split):
    """The mixed dispatch's profitability gate open (the batches here are far smaller than the ones it pays for), the split
    forward on or off."""
    return ops.configured(mixed_max_fraction=0.9, mixed_min_nodes=0, split_forward=split)


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what}: bits differ"


def _check_trace(trace, N, E, L):
    assert len(trace.alphas) == len(trace.masks) == L
    for a in trace.alphas:
        assert a.dtype == torch.float32 and a.dim() == 2 and a.size(0) == E and bool(torch.isfinite(a).all()) and bool((a >= 0).all())
    for m in trace.masks:
        assert m is None or (tuple(m.shape) == (N, 1) and bool((m >= 0).all()))
    assert trace.gate.numel() == N and bool((trace.gate >= 0).all())


def _restated(trace, plan, ei, start, use_masks, residual):
    N = plan.N
    csr = RR.source_csr(ei.cpu(), N)
    alphas = [a.cpu() for a in trace.alphas]
    masks = [None if (m is None or not use_masks) else m.cpu().reshape(-1) for m in trace.masks]
    rel, flow = RR.rollout(plan.ptr.cpu().tolist(), *csr, alphas, start.cpu(), masks, residual)
    dmax = int((csr[0][1:] - csr[0][:-1]).max())
    return rel, flow, len(alphas) * (alphas[0].size(1) + dmax + 6)


def _assert_bound(got, ref, k, what):
    g = got.cpu().double()
    assert bool((g[ref == 0] == 0).all()), f"{what}: an exact zero came out non-zero"
    err = (g - ref).abs()
    worst = float((err / ref.clamp_min(1e-300)).max())
    print(f"[rollout] {what}: max relative error {worst:.3e} against the bound {2 * k * U:.3e} (k = {k})")
    assert bool(((ref == 0) | (ref >= 1e-30)).all()), f"{what}: an exact non-zero output below 1e-30"
    assert bool((err <= 2 * k * U * ref).all()), f"{what}: max relative error {worst:.3e} beyond 2 k u = {2 * k * U:.3e}"


def _khot_with_ties(explain, r, k):
    """Rollout.mask(k) against the threshold rule on the shifted scores: every node at or above its graph's k-th largest score."""
    s = explain.shifted_attributions(r.attribution, r.plan.batch, r.plan.B).cpu()
    ptr = r.plan.ptr.cpu().tolist()
    want = torch.zeros(r.plan.N)
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        if hi > lo:
            kth = torch.sort(s[lo:hi], descending=True).values[min(k, hi - lo) - 1]
            want[lo:hi] = (s[lo:hi] >= kth).float()
    m = r.mask(k)
    assert tuple(m.shape) == (r.plan.N, 1) and m.dtype == torch.float32 and torch.equal(m.cpu().view(-1), want)
    per_graph = torch.zeros(r.plan.B).index_add_(0, r.plan.batch.cpu(), want)
    assert all(c >= min(k, hi - lo) for c, lo, hi in zip(per_graph.tolist(), ptr[:-1], ptr[1:]))


def test_a_trace_changes_no_bit_and_holds_mgats_own_weights(answer, dev):
    from isubgvqa_amd import explain, ops
    model, d = answer
    B, N, E = len(SIZES), sum(SIZES), d.edge_index.size(1)
    with torch.no_grad(), _mixed(ops, False):
        plan = _plan(ops, d, B)
        plain = model(d, plan=plan)
        trace = explain.AttentionTrace()
        traced = model(d, plan=plan, trace=trace)
        assert len(traced) == 3
        for a, b, name in zip(plain, traced, ("logits", "mask", "gate")):
            _same(a, b, name)
        _check_trace(trace, N, E, 3)
        _same(trace.mask, plain[1], "trace.mask")
        _same(trace.gate, plain[2], "trace.gate")
        assert [m is None for m in trace.masks] == [True, True, False]
        _same(trace.masks[2], plain[1], "the last layer's mask")
        gate_q, _ = model.gat_seq.question_side(d.glf, None, model.graph_global_attention_pooling)
        h, mask, _, _, attn = model.gat_seq(x=d.x, edge_index=d.edge_index, edge_attr=d.edge_attr, instr_vectors=d.instr[:4],
                                            global_language_feats=d.glf, batch=d.batch, return_masks=True, plan=plan, gate_q=gate_q,
                                            return_attention=True)
        assert len(attn) == 3
        for l, (ei, alpha) in enumerate(attn):
            assert torch.equal(trace.alphas[l], alpha), f"layer {l}: trace.alphas differs from MGAT.forward(return_attention=True)"
        # MGAT alone fills the layers' half of a trace
        t2 = explain.AttentionTrace()
        model.gat_seq(x=d.x, edge_index=d.edge_index, edge_attr=d.edge_attr, instr_vectors=d.instr[:4], global_language_feats=d.glf,
                      batch=d.batch, return_masks=True, plan=plan, gate_q=gate_q, trace=t2)
        assert t2.gate is None and t2.mask is None and all(torch.equal(a, b) for a, b in zip(t2.alphas, trace.alphas))
    ops.check_plans()


def test_the_split_forward_merges_the_trace_by_edge_and_writes_every_row(answer, dev, monkeypatch):
    from isubgvqa_amd import explain, ops
    model, d = answer
    B, N, E = len(SIZES), sum(SIZES), d.edge_index.size(1)
    with torch.no_grad():
        with _mixed(ops, False):
            plan = _plan(ops, d, B)
            unsplit, t0 = explain.AttentionTrace(), None
            out0 = model(d, plan=plan, trace=unsplit)
        # a stub around the layer kernel's operator: in the tile pass of run_split (plan.holes) the rows of the holes' edges are
        # filled with NaN behind the launch, so a row the merge does not write shows
        real, seen = ops.gatv2_layer_conv, []

        def stub(x, lin_l, lin_r, edge_attr, w_edge, att, plan_, heads, **kw):
            res = real(x, lin_l, lin_r, edge_attr, w_edge, att, plan_, heads, **kw)
            if res is not None and plan_.holes is not None and res[1] is not None:
                res[1][plan_.holes.edges] = float("nan")
                seen.append(int(plan_.holes.edges.numel()))
            return res
        monkeypatch.setattr(ops, "gatv2_layer_conv", stub)
        with _mixed(ops, True):
            plan = _plan(ops, d, B)
            sub = ops.oversize_split(plan)
            assert sub is not None and sub.gids.tolist() == [2] and sub.edges.numel() > 0
            ops.reset_counters()
            split = explain.AttentionTrace()
            out1 = model(d, plan=plan, trace=split)
            plain = model(d, plan=plan)
        monkeypatch.setattr(ops, "gatv2_layer_conv", real)
    assert len(seen) == 3 and all(n == sub.edges.numel() for n in seen), seen      # 3 layers of the traced forward (the plain one stores no weights)
    _check_trace(split, N, E, 3)                                                  # (finite: every NaN row was overwritten)
    for a, b, name in zip(out1, plain, ("logits", "mask", "gate")):
        _same(a, b, f"split forward with a trace, {name}")
    _same(split.mask, out1[1], "trace.mask")
    _same(split.gate, out1[2], "trace.gate")
    assert torch.equal(out1[1], out0[1])
    for l in range(3):
        assert torch.allclose(split.alphas[l], unsplit.alphas[l], **ALPHA_TOL), \
            f"layer {l}: {(split.alphas[l] - unsplit.alphas[l]).abs().max().item():.3e}"
        assert (split.masks[l] is None) == (unsplit.masks[l] is None)
    assert torch.equal(split.masks[2], unsplit.masks[2]) and tuple(split.masks[2].shape) == (N, 1)
    ops.check_plans()


@pytest.mark.parametrize("use_masks,residual,split", [(True, 0.5, False), (False, 0.5, True), (False, 0.25, False)])
def test_attention_rollout_of_the_answer_model(answer, dev, use_masks, residual, split):
    from isubgvqa_amd import explain, ops
    model, d = answer
    B, N = len(SIZES), sum(SIZES)
    with _mixed(ops, split):
        ops.reset_counters()
        r = explain.attention_rollout(model, d, residual=residual, use_masks=use_masks, want_flow=True)
        assert ops.counters()["attention_rollout"] == 1
        with torch.no_grad():
            logits, mask, gate = model(d, plan=_plan(ops, d, B))
    _same(r.logits, logits, "logits")
    _same(r.trace.gate, gate, "gate")
    assert r.attribution.dtype == torch.float32 and tuple(r.attribution.shape) == (N,) and tuple(r.flow.shape) == (3, d.edge_index.size(1))
    start = (gate * mask).reshape(-1)
    ref, ref_flow, k = _restated(r.trace, r.plan, d.edge_index, start, use_masks, residual)
    _assert_bound(r.attribution, ref, k, f"attribution (masks {use_masks}, residual {residual}, split {split})")
    _assert_bound(r.flow, ref_flow, k, "flow")
    assert float(r.attribution.sum()) > 0
    if not use_masks:
        # conservation: softmax weights into every node (each has its self loop) sum to 1 -- to the rounding of a softmax over
        # d_in terms (the kernels' + 1e-16 in the denominator is far below it), so per layer a graph's sum moves by at most
        # (d_in + 3) u of itself on top of the rollout's own 2 k u
        ptr = r.plan.ptr.cpu().tolist()
        din = int(torch.bincount(d.edge_index[1].cpu(), minlength=N).max())
        tol = (2 * k + 2 * 3 * (din + 3)) * U
        got, want = r.attribution.cpu().double(), start.cpu().double()
        for g, (lo, hi) in enumerate(zip(ptr[:-1], ptr[1:])):
            assert abs(float(got[lo:hi].sum() - want[lo:hi].sum())) <= tol * float(want[lo:hi].sum()), g
    _khot_with_ties(explain, r, K)
    ops.check_plans()


def test_the_full_model_with_a_trace(full, dev):
    from isubgvqa_amd import explain, ops
    model, d, sizes = full
    B, N, E = len(sizes), sum(sizes), d.edge_index.size(1)
    with torch.no_grad():
        plan = _plan(ops, d, B)
        sg = d.scene_graphs()
        args = (d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask)
        plain = model(*args, return_masks=True, scene_graphs=sg, plan=plan)
        trace = explain.AttentionTrace()
        traced = model.forward_traced(trace, *args, return_masks=True, scene_graphs=sg, plan=plan)
    assert len(plain) == len(traced) == 5
    for a, b, name in zip(plain[:3], traced[:3], ("logits", "mask", "gate")):
        _same(a, b, name)
    L = len(model.gat_seq.convs)
    _check_trace(trace, N, E, L)
    _same(trace.mask, plain[1], "trace.mask")
    _same(trace.gate, plain[2], "trace.gate")
    with pytest.raises(ValueError, match="trace together with capture"):
        model.forward_traced(explain.AttentionTrace(), *args, return_masks=True, scene_graphs=sg, capture="language")
    for use_masks in (True, False):
        r = explain.attention_rollout(model, d, use_masks=use_masks)
        _same(r.logits, plain[0], "logits")
        assert r.flow is None
        start = plain[2].reshape(-1) if plain[1] is None else (plain[2] * plain[1]).reshape(-1)
        ref, _, k = _restated(r.trace, r.plan, d.edge_index, start, use_masks, 0.5)
        _assert_bound(r.attribution, ref, k, f"full model, masks {use_masks}")
        _khot_with_ties(explain, r, 2)
    ops.check_plans()


def test_compare_takes_attention_and_keeps_its_default(dev):
    from isubgvqa_amd import explain, ops, synthetic
    V, A, K2 = 200, 1842, 2
    tables = explain.TokenTables({f"w{i}": i for i in range(V)}, [f"w{(11 * a) % V}" if a % 3 == 0 else f"answer {a}" for a in range(A)])
    model, _ = _answer_case(dev)
    gen = torch.Generator().manual_seed(13)
    batches = []
    B, N = len(SMALL_SIZES), sum(SMALL_SIZES)
    with torch.no_grad():
        for seed in (5, 6):
            d = _answer_case(dev, seed)[1]
            names = torch.randint(0, V, (N,), generator=gen)
            label = model(d)[0].argmax(1).cpu()
            label[1::2] = (label[1::2] + 1) % A
            qtok = torch.full((B, 4), -1, dtype=torch.int32)
            qtok[:, :3] = torch.randint(0, V, (B, 3), generator=gen).int()
            gold = synthetic.make_gold(SMALL_SIZES, facets=2, entries=3, seed=seed)
            batches.append(explain.EvalBatch(d, label.to(dev), qtok.to(dev), (torch.arange(B) % 2).int().to(dev), names.to(dev),
                                             gold=gold.to(dev)))
    chosen = ("intrinsic", "attention", "random")
    report = explain.compare(model, batches, tables, explainers=chosen, k=K2, seed=40)
    assert tuple(report) == chosen
    assert tuple(explain.compare(model, batches[:1], tables, k=K2, seed=40)) == explain.EXPLAINERS == ("intrinsic", "occlusion", "random")
    with torch.no_grad():
        for name in chosen:
            coo = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
            ground = torch.zeros(ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
            plus, minus, jac = [], [], []
            for number, b in enumerate(batches):
                d = b.inputs
                plan = _plan(ops, d, B)
                logits, intrinsic, _ = model(d, plan=plan)
                mask = {"intrinsic": lambda: intrinsic, "attention": lambda: explain.attention_rollout(model, d).mask(K2),
                        "random": lambda: explain.random_mask(plan, K2, 40 + number)}[name]()
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
    assert report["intrinsic"].jaccard == 1.0
    ops.check_plans()
