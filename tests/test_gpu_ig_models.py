"""explain.integrated_gradients through the real models on the GPU: the gradient rows against the CPU oracle
differentiated in float64, the device's reduction against the restatement of tests/ig_restated.py, completeness, the one-point
rule against a plain autograd call, the mask, untouched parameters and forwards, the full model on its encoder's rows, compare().

TOLERANCES.  Input gradients of the MGAT stack against the oracle: the project's own, 5e-4 of the largest reference entry through
tests/test_gpu_train.py's `close` (test_training_step_matches_reference_gradients).  The device's reduction of ITS OWN gradient
rows: the bound derived in tests/test_gpu_ig.py, 1.01 (S + C + 8) u sum |x - b| sum |w g|.  Two forwards of the same rows in
batches of different composition: logits within LOGIT_TOL = 1e-4 (tests/test_gpu_models.py), hence a softmax probability within
2e-4 of its value (d ln p = d logit_pred - sum_j p_j d logit_j)."""
import math

import pytest
import torch

import ig_restated as IR
from test_gpu_models import LOGIT_TOL, _noises, _oracle_cfg
from test_gpu_train import close

pytestmark = pytest.mark.gpu

SIZES = (5, 9, 70, 3, 12, 1, 20, 33, 2, 64, 7, 16)       # 12 graphs, one beyond a 64-node tile, one that fills one
K = 3
U = 2.0 ** -24
MASKED_SEED = 1                 # chosen on the CPU oracle (_oracle_gradient): seeds 9, 1, 2, 3, 4, 5 give a smallest top-k gap over the
                                # three points of the path of 4.0e-5, 1.4e-4, 8.1e-5, 8.2e-6, 8.2e-5, 8.7e-7; the gap is asserted on every run
MIN_GAP = 1e-5                  # tests/test_gpu_instances.py: gates of two paths agree within 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def _config(masks, seed):
    from isubgvqa_amd import synthetic
    return synthetic.WorkloadConfig(num_graphs=len(SIZES), channels=128, layers=3, masks=masks, sampler="imle", sample_k=K,
                                    edges_per_graph=0.0, seed=seed, sizes=SIZES)


def _answer(dev, masks, seed):
    from isubgvqa_amd import synthetic
    cfg = _config(masks, seed)
    wl = synthetic.make_workload(cfg)
    return cfg, synthetic.build_answer_model(cfg).eval().to(dev), wl, wl.to(dev)


@pytest.fixture(scope="module")
def unmasked(dev):
    return _answer(dev, (1.0, 1.0, 1.0), 9)


@pytest.fixture(scope="module")
def masked(dev):
    return _answer(dev, (1.0, 1.0, 0.15), MASKED_SEED)


def _pick(logits, pred_rows, target="prob"):
    out = torch.softmax(logits, dim=1) if target == "prob" else logits
    return out.gather(1, pred_rows.unsqueeze(1)).squeeze(1)


def _oracle_gradient(cfg, model, wl, inst_index, batch, edge_index, x_inst, e_inst, pred):
    """The gradient of sum_q softmax(logits)[q, pred[graph q]] with respect to the instance batch's node rows, from the CPU oracle
    in float64 -> (gradient rows, the oracle's node mask, the smallest top-k gap of the masked layer over the instances)."""
    from oracle import model as OM
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    rows = inst_index.long()
    x64 = x_inst.double().requires_grad_(True)
    trace = []
    logits, mask, _ = OM.mgat_pool_classify(sd, x64, edge_index, e_inst.double(), batch, wl.instr[:, rows].double(),
                                            wl.glf[rows].double(), _oracle_cfg(cfg), _noises(cfg, wl, 5), trace)
    _pick(logits, pred[rows]).sum().backward()
    gap = float("inf")
    for layer, thr in enumerate(cfg.masks):
        if thr != 1.0:
            dense = trace[layer]["dense"].detach().squeeze(-1)
            counts = torch.tensor(SIZES)[rows]
            v, idx = dense.sort(dim=1, descending=True)
            involved = (idx[:, K - 1] < counts) | (idx[:, K] < counts)
            gap = min(gap, float(torch.where(involved, v[:, K - 1] - v[:, K], torch.full_like(v[:, 0], float("inf"))).min()))
    return x64.grad, mask, gap


@pytest.mark.parametrize("which", ["unmasked", "masked"])
def test_gradient_rows_and_attributions_against_the_float64_oracle(request, dev, which):
    from isubgvqa_amd import explain, ops, synthetic
    cfg, model, wl, d = request.getfixturevalue(which)
    S, B, C = 3, len(SIZES), 128
    res = explain.integrated_gradients(model, d, steps=S)
    assert len(res.chunks) == 1 and res.edge_attribution is None and res.attribution.shape == (sum(SIZES),)
    inst = res.chunks[0]
    t, w = explain.quadrature(S, "gauss_legendre")
    t_inst, w_inst = t.float().repeat(B).to(dev), w.float().repeat(B).to(dev)
    assert inst.index.tolist() == [q // S for q in range(B * S)]
    with torch.no_grad():
        x_inst, e_inst = ops.ig_path_rows(inst, d.x, d.edge_attr, t_inst)
    rows = inst.index.long()
    # the device's own gradient rows of the same score, by one plain autograd call on the instance batch
    leaf = x_inst.clone().requires_grad_(True)
    out = model(synthetic.Workload(leaf, inst.edge_index, e_inst, inst.batch, d.instr.index_select(1, rows).contiguous(),
                                   d.glf.index_select(0, rows), B * S, d.max_nodes, d.max_edges, None), plan=inst.plan())
    (g_dev,) = torch.autograd.grad(_pick(out[0].float(), res.pred.index_select(0, rows)).sum(), [leaf])
    g_ref, mask_ref, gap = _oracle_gradient(cfg, model, wl, inst.index.cpu(), inst.batch.cpu(), inst.edge_index.cpu(), x_inst.cpu(),
                                            e_inst.cpu(), res.pred.cpu())
    if which == "masked":
        print(f"[ig] masked run: smallest top-k gap over the {B * S} instances = {gap:.3e}")
        assert gap > MIN_GAP, gap
        assert int((out[1].detach().cpu().view(-1) != mask_ref.detach().view(-1).float()).sum()) == 0, "the masks differ along the path"
        assert 0 < int(mask_ref.sum()) < mask_ref.numel()
    else:
        assert out[1] is None or bool((out[1] == 1).all())
    close(g_dev, g_ref, 5e-4, "gradient rows")
    lay = dict(ptr=inst.parent.ptr.cpu().tolist(), inst_ptr=inst.ptr.cpu().tolist())
    gptr, glist = (v.cpu().tolist() for v in inst.by_graph())
    assert (gptr, glist) == IR.by_graph(inst.index.cpu().tolist(), B)
    want = IR.attribution(g_ref, w_inst.cpu(), wl.x, None, lay["ptr"], lay["inst_ptr"], gptr, glist)[0]
    close(res.attribution, want, 5e-4, "attribution")
    # the device's reduction, fed the device's own gradient rows, against the restatement fed the same rows
    with torch.no_grad():
        own = ops.ig_attribution(inst, g_dev.contiguous(), None, w_inst, d.x, d.edge_attr, want_rows=True)
    attr, G, bound, avg_bound, most = IR.attribution(g_dev.cpu(), w_inst.cpu(), wl.x, None, lay["ptr"], lay["inst_ptr"], gptr, glist)
    assert most == S and own.attr_e is None and own.avg_e is None
    err = (own.attr_x.cpu().double() - attr).abs()
    print(f"[ig] {which}: device reduction, largest error / bound = {float((err / (1.01 * (S + C + 8) * U * bound)).max()):.3f}")
    assert bool((err <= 1.01 * (S + C + 8) * U * bound).all())
    assert bool(((own.avg_x.cpu().double() - G).abs() <= 1.01 * (S + 1) * U * avg_bound).all())
    ops.check_plans()


def test_completeness_the_ends_of_the_path_and_the_steps(unmasked, dev):
    from isubgvqa_amd import explain
    cfg, model, wl, d = unmasked
    gaps = {}
    for S in (4, 32):
        res = explain.integrated_gradients(model, d, steps=S, max_instances=96 if S == 32 else None)
        assert len(res.chunks) == (4 if S == 32 else 1)
        p = torch.softmax(res.logits.float(), dim=1).gather(1, res.pred.unsqueeze(1)).squeeze(1)
        assert torch.equal(res.pred, res.logits.argmax(1))
        assert bool(((res.f_input - p).abs() <= 2 * LOGIT_TOL * p).all()), (res.f_input - p).abs().max()
        total = torch.zeros(len(SIZES), dtype=torch.float64).index_add_(0, wl.batch, res.attribution.cpu().double())
        host = total - (res.f_input.cpu().double() - res.f_baseline.cpu().double())
        # the device adds fp32 numbers: n_g additions of attributions and two subtractions
        slack = (max(SIZES) + 2) * U * (torch.zeros(len(SIZES), dtype=torch.float64).index_add_(0, wl.batch, res.attribution.cpu().double().abs())
                                        + res.f_input.cpu().double() + res.f_baseline.cpu().double())
        assert bool(((res.delta.cpu().double() - host).abs() <= slack).all())
        assert bool(torch.isfinite(res.attribution).all()) and float(res.attribution.abs().max()) > 0
        gaps[S] = float(res.delta.abs().mean())
    print(f"[ig] mean |delta|: {gaps[4]:.3e} at 4 steps, {gaps[32]:.3e} at 32")
    assert gaps[32] < gaps[4]


@pytest.mark.parametrize("which", ["unmasked", "masked"])
def test_the_endpoint_rule_is_gradient_times_input(request, dev, which):
    from isubgvqa_amd import explain, ops, synthetic
    cfg, model, wl, d = request.getfixturevalue(which)
    res = explain.integrated_gradients(model, d, steps=1, rule="endpoint")
    leaf = d.x.clone().requires_grad_(True)
    out = model(synthetic.Workload(leaf, d.edge_index, d.edge_attr, d.batch, d.instr, d.glf, len(SIZES), d.max_nodes, d.max_edges,
                                   d.graph_sizes))
    (g,) = torch.autograd.grad(_pick(out[0].float(), res.pred).sum(), [leaf])
    close(res.attribution, (d.x * g).sum(1), 5e-4, "gradient x input")
    base = torch.full((128,), 0.25, device=dev)
    res = explain.integrated_gradients(model, d, steps=1, rule="endpoint", baseline=base, target="logit")
    (g,) = torch.autograd.grad(_pick(model(synthetic.Workload(leaf, d.edge_index, d.edge_attr, d.batch, d.instr, d.glf, len(SIZES),
                                                              d.max_nodes, d.max_edges, d.graph_sizes))[0].float(), res.pred, "logit").sum(),
                               [leaf])
    close(res.attribution, ((d.x - base) * g).sum(1), 5e-4, "gradient x (input - baseline), logit")
    ops.check_plans()


def test_the_mask_is_k_hot_with_ties_kept(masked, dev):
    from isubgvqa_amd import explain
    from test_gpu_rollout_models import _khot_with_ties
    cfg, model, wl, d = masked
    res = explain.integrated_gradients(model, d, steps=2)
    _khot_with_ties(explain, res, K)
    _khot_with_ties(explain, res, 1)


def test_nothing_of_the_model_changes(masked, dev):
    from isubgvqa_amd import explain
    cfg, model, wl, d = masked
    with torch.no_grad():
        before = model(d)
    for kw in ({"steps": 3}, {"steps": 2, "edges": True, "baseline": "mean", "max_instances": 12}):
        res = explain.integrated_gradients(model, d, **kw)
        assert (res.edge_attribution is not None) == bool(kw.get("edges")) and bool(torch.isfinite(res.delta).all())
    with torch.no_grad():
        after = model(d)
    for a, b, name in zip(before, after, ("logits", "mask", "gate")):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    assert all(p.grad is None for p in model.parameters()) and not model.training
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.integrated_gradients(model.train(), d)
    model.eval()


def test_the_full_model_on_its_encoders_rows(dev):
    from isubgvqa_amd import explain, ops, synthetic
    from isubgvqa_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(sg_vocab_size=64, text_vocab_size=64), None).eval().to(dev)
    sizes = (3, 7, 5, 66)
    d = synthetic.make_full_workload(len(sizes), tokens=9, seed=3, sg_vocab=64, text_vocab=64, sizes=sizes).to(dev)
    calls, encode = [], model.encode_scene

    def counted(*a, **kw):
        calls.append(1)
        return encode(*a, **kw)

    model.encode_scene = counted
    try:
        res = explain.integrated_gradients(model, d, steps=3, max_instances=8)
    finally:
        del model.encode_scene
    B, N = len(sizes), sum(sizes)
    assert len(calls) == 1 and len(res.chunks) == 2
    assert res.attribution.shape == (N,) and res.delta.shape == res.f_input.shape == res.f_baseline.shape == res.pred.shape == (B,)
    assert res.logits.shape == (B, 1842) and res.edge_attribution is None
    for v in (res.attribution, res.delta, res.f_input, res.f_baseline):
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all())
    assert float(res.attribution.abs().max()) > 0 and all(p.grad is None for p in model.parameters())
    # by hand: path_attributions on encode_scene's rows, with the score integrated_gradients states
    with torch.no_grad():
        plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=B, max_nodes=d.max_nodes, max_edges=d.max_edges, graph_sizes=d.graph_sizes)
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs(), plan)
        glf, instr = model.language_features(d.questions, d.att_mask)
        logits = model(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, return_masks=True, scene_graphs=d.scene_graphs())[0]
    assert float((res.logits - logits).abs().max()) <= LOGIT_TOL and torch.equal(res.pred, logits.argmax(1))

    def score(x_inst, e_inst, inst):
        rows = inst.index.long()
        out = model.answer_graphs(x_inst, inst.edge_index, e_inst, inst.batch, instr.index_select(1, rows).contiguous(),
                                  glf.index_select(0, rows), inst.plan(), True, None, None)[0]
        return _pick(out.float(), res.pred.index_select(0, rows))

    hand = explain.path_attributions(score, state.x_enc, state.e_enc, plan, d.edge_index, steps=3, max_instances=8)
    for a, b, name in ((res.attribution, hand.attribution, "attribution"), (res.delta, hand.delta, "delta"),
                       (res.f_input, hand.f_input, "f_input"), (res.f_baseline, hand.f_baseline, "f_baseline")):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    ops.check_plans()


def test_compare_takes_the_gradient_explainers_and_keeps_its_default(dev):
    from isubgvqa_amd import explain, ops, synthetic
    from test_gpu_occlusion import SIZES as SMALL_SIZES
    from test_gpu_occlusion import _answer_case, _plan
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
    chosen = ("intrinsic", "integrated_gradients", "grad_x_input")
    report = explain.compare(model, batches, tables, explainers=chosen, k=K2, seed=40, ig_steps=3)
    assert tuple(report) == chosen and torch.is_grad_enabled()
    assert tuple(explain.compare(model, batches[:1], tables, k=K2, seed=40)) == explain.EXPLAINERS == ("intrinsic", "occlusion", "random")
    makers = {"intrinsic": lambda d, intrinsic: intrinsic,
              "integrated_gradients": lambda d, intrinsic: explain.integrated_gradients(model, d, steps=3).mask(K2),
              "grad_x_input": lambda d, intrinsic: explain.integrated_gradients(model, d, steps=1, rule="endpoint").mask(K2)}
    for name in chosen:
        coo = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
        ground = torch.zeros(ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
        plus, minus, jac = [], [], []
        for number, b in enumerate(batches):
            d = b.inputs
            with torch.no_grad():
                plan = _plan(ops, d, B)
                logits, intrinsic, _ = model(d, plan=plan)
            mask = makers[name](d, intrinsic)
            with torch.no_grad():
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
