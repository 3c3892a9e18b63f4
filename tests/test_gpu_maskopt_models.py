"""explain.mask_optimization through the real models on the GPU: the first iteration's d theta against the CPU oracle
differentiated in float64, the recorded scores against a plain forward, the objective's descent, edge logits, untouched parameters
and forwards, the full model on its encoder's rows, compare().

TOLERANCES.  d theta against the oracle: the project's own for gradients, 5e-4 of the largest reference entry through
tests/test_gpu_train.py's `close`.  A recorded score against a plain forward of the same masked rows: logits within LOGIT_TOL = 1e-4
(tests/test_gpu_models.py), hence -log softmax within 2e-4 (d ln p = d logit_pred - sum_j p_j d logit_j)."""
import math

import pytest
import torch

import maskopt_restated as MR
from test_gpu_ig_models import K, MIN_GAP, SIZES, _answer
from test_gpu_models import LOGIT_TOL, _noises, _oracle_cfg
from test_gpu_train import close

pytestmark = pytest.mark.gpu

THETA_SEED = {"unmasked": 2, "masked": 6}       # the seeds of the initial logits; the masked one chosen on the CPU oracle
                                                # (_oracle_objective): seeds 1 to 6 give a smallest top-k gap at the initial mask of 5.0e-4,
                                                # 8.5e-5, 3.5e-5, 5.6e-6, 8.5e-4, 2.1e-3; the gap is asserted on every run
T_DESCENT = 10
SEG = [0]
for _n in SIZES:
    SEG.append(SEG[-1] + _n)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def unmasked(dev):
    return _answer(dev, (1.0, 1.0, 1.0), 9)


@pytest.fixture(scope="module")
def masked(dev):
    return _answer(dev, (1.0, 1.0, 0.15), 1)


def _theta0(which):
    return 0.1 * torch.randn(sum(SIZES), generator=torch.Generator().manual_seed(THETA_SEED[which]))


def _nll(logits, pred):
    return -torch.log_softmax(logits, dim=1).gather(1, pred.unsqueeze(1)).squeeze(1)


def _regularisers(theta):
    """sum over the graphs of a_size mean sigmoid + a_ent mean H, PyG's eps-guarded entropy, differentiable."""
    m = torch.sigmoid(theta)
    ent = MR.pyg_entropy_term(theta)
    return sum(MR.PYG["a_size"] * m[lo:hi].mean() + MR.PYG["a_ent"] * ent[lo:hi].mean() for lo, hi in zip(SEG[:-1], SEG[1:]))


def _oracle_objective(cfg, model, wl, theta, pred):
    """(per-graph score float64 [B], the oracle's node mask, the smallest top-k gap of a masked layer) of the CPU oracle in float64
    on the rows sigmoid(theta) x; differentiable in theta."""
    from oracle import model as OM
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    trace = []
    logits, mask, _ = OM.mgat_pool_classify(sd, torch.sigmoid(theta).unsqueeze(1) * wl.x.double(), wl.edge_index, wl.edge_attr.double(),
                                            wl.batch, wl.instr.double(), wl.glf.double(), _oracle_cfg(cfg), _noises(cfg, wl, 5), trace)
    gap = float("inf")
    for layer, thr in enumerate(cfg.masks):
        if thr != 1.0:
            dense = trace[layer]["dense"].detach().squeeze(-1)
            counts = torch.tensor(SIZES)
            v, idx = dense.sort(dim=1, descending=True)
            involved = (idx[:, K - 1] < counts) | (idx[:, K] < counts)
            gap = min(gap, float(torch.where(involved, v[:, K - 1] - v[:, K], torch.full_like(v[:, 0], float("inf"))).min()))
    return _nll(logits, pred), mask, gap


@pytest.mark.parametrize("which", ["unmasked", "masked"])
def test_first_iteration_against_the_float64_oracle(request, dev, which):
    from isubgvqa_amd import explain, ops, synthetic
    cfg, model, wl, d = request.getfixturevalue(which)
    B, N = len(SIZES), sum(SIZES)
    theta0 = _theta0(which)
    res = explain.mask_optimization(model, d, steps=1, init=theta0.to(dev))
    assert res.theta.shape == res.soft.shape == (N,) and res.nll.shape == (2, B) and res.pred.shape == (B,) and res.edge_theta is None
    assert torch.equal(res.pred, res.logits.argmax(1)) and res.steps == 1 and res.plan.B == B
    # the iteration by hand: the apply-only launch, one forward and backward of the model, the step's launch
    seg = res.plan.ptr
    th, m, v = theta0.to(dev).clone(), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    with torch.no_grad():
        x_m, _ = ops.maskopt_step(d.x, None, seg, th, None, None, step=1)
    leaf = x_m.clone().requires_grad_(True)
    out = model(synthetic.Workload(leaf, d.edge_index, d.edge_attr, d.batch, d.instr, d.glf, B, d.max_nodes, d.max_edges, d.graph_sizes))
    score = _nll(out[0].float(), res.pred)
    (g,) = torch.autograd.grad(score.sum(), [leaf])
    with torch.no_grad():
        _, d_dev = ops.maskopt_step(d.x, g.contiguous(), seg, th, m, v, step=1, want_grad=True)
    # mask_optimization's first step is the step taken by hand (the two forwards differ in how the plan reached them, so the
    # gradient rows may differ in their last bits; at step 1 Adam moves by lr d / (|d| + eps), which hardly sees them)
    assert float((th - res.theta).abs().max()) <= 1e-7
    # the oracle, differentiated in float64: the score and both regularisers with respect to theta
    t64 = theta0.double().requires_grad_(True)
    ref_score, mask_ref, gap = _oracle_objective(cfg, model, wl, t64, res.pred.cpu())
    (d_ref,) = torch.autograd.grad(ref_score.sum() + _regularisers(t64), [t64])
    if which == "masked":
        print(f"[maskopt] masked run: smallest top-k gap at the initial mask = {gap:.3e}")
        assert gap > MIN_GAP, gap
        assert int((out[1].detach().cpu().view(-1) != mask_ref.detach().view(-1).float()).sum()) == 0, "the masks differ"
        assert 0 < int(mask_ref.sum()) < mask_ref.numel()
    else:
        assert out[1] is None or bool((out[1] == 1).all())
    close(d_dev, d_ref, 5e-4, "d theta")
    # the recorded score at the initial mask against the plain forward and the oracle
    assert bool(((res.nll[0] - score.detach()).abs() <= 2 * LOGIT_TOL).all()), float((res.nll[0] - score.detach()).abs().max())
    assert bool(((res.nll[0].cpu().double() - ref_score.detach()).abs() <= 2 * LOGIT_TOL).all())
    ops.check_plans()


def test_the_objective_descends(unmasked, dev):
    """The mean over the graphs of score + regularisers at the final mask lies below the one at the initial mask -- asserted for
    the device after the oracle's float64 loop (torch.optim.Adam on the host) has shown the same for these inputs and T."""
    from isubgvqa_amd import explain
    cfg, model, wl, d = unmasked
    theta0 = _theta0("unmasked")
    with torch.no_grad():
        pred = model(d)[0].argmax(1).cpu()
    t64 = theta0.double().requires_grad_(True)
    opt = torch.optim.Adam([t64], lr=MR.PYG["lr"])
    host = []
    for it in range(T_DESCENT + 1):
        opt.zero_grad()
        score = _oracle_objective(cfg, model, wl, t64, pred)[0]
        host.append(float(MR.objective(score.detach(), t64.detach(), SEG).mean()))
        if it < T_DESCENT:
            (score.sum() + _regularisers(t64)).backward()
            opt.step()
    assert host[-1] < host[0], host
    res = explain.mask_optimization(model, d, steps=T_DESCENT, init=theta0.to(dev))
    first = float(MR.objective(res.nll[0].cpu(), theta0, SEG).mean())
    last = float(MR.objective(res.nll[T_DESCENT].cpu(), res.theta.cpu(), SEG).mean())
    print(f"[maskopt] mean objective over {T_DESCENT} steps: {first:.6f} -> {last:.6f} on the device, {host[0]:.6f} -> {host[-1]:.6f} "
          f"for the float64 oracle")
    assert last < first
    assert abs(first - host[0]) <= 2 * LOGIT_TOL + 1e-6            # the same logits' scores, the same regularisers
    assert bool(torch.isfinite(res.nll).all()) and torch.equal(res.soft, torch.sigmoid(res.theta))
    m = res.mask(K)
    per_graph = torch.zeros(len(SIZES)).index_add_(0, wl.batch, m.cpu().view(-1))
    assert m.shape == (sum(SIZES), 1) and bool((per_graph >= torch.tensor(SIZES).clamp(max=K)).all())


def test_edge_logits_and_nothing_of_the_model_changes(masked, dev):
    from isubgvqa_amd import explain
    cfg, model, wl, d = masked
    with torch.no_grad():
        before = model(d)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    E = d.edge_index.size(1)
    res = explain.mask_optimization(model, d, steps=3, edges=True, init_seed=4)
    again = explain.mask_optimization(model, d, steps=3, edges=True, init_seed=4)
    nodes_only = explain.mask_optimization(model, d, steps=3, init_seed=4)
    assert res.edge_theta.shape == res.edge_soft.shape == (E,) and bool(torch.isfinite(res.edge_theta).all()) and bool(torch.isfinite(res.nll).all())
    assert torch.equal(res.theta, again.theta) and torch.equal(res.edge_theta, again.edge_theta) and torch.equal(res.nll, again.nll)
    gen = torch.Generator(device=dev).manual_seed(4)
    init_x = 0.1 * torch.randn(sum(SIZES), generator=gen, device=dev)
    init_e = 0.1 * torch.randn(E, generator=gen, device=dev)
    moved = (res.edge_theta - init_e).abs()
    # Adam moves a logit by lr at step 1 and, by Cauchy-Schwarz on its two weighted sums, by less than 1.004 lr at steps 2 and 3
    assert float(moved.max()) <= 3 * 0.01 * 1.01 and float(moved.max()) > 0.01
    assert float((res.theta - init_x).abs().max()) > 0.01 and nodes_only.edge_theta is None
    assert not torch.equal(nodes_only.nll[0], res.nll[0])                             # the edge rows were masked as well
    with torch.no_grad():
        after = model(d)
    for a, b, name in zip(before, after, ("logits", "mask", "gate")):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert all(p.grad is None for p in model.parameters()) and not model.training and torch.is_grad_enabled()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.mask_optimization(model.train(), d)
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
        res = explain.mask_optimization(model, d, steps=4, init_seed=2)
    finally:
        del model.encode_scene
    B, N = len(sizes), sum(sizes)
    assert len(calls) == 1
    assert res.theta.shape == (N,) and res.nll.shape == (5, B) and res.pred.shape == (B,) and res.logits.shape == (B, 1842)
    for v in (res.theta, res.soft, res.nll):
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all())
    assert all(p.grad is None for p in model.parameters())
    # by hand: mask_optimize on encode_scene's rows, with the score mask_optimization states
    with torch.no_grad():
        plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=B, max_nodes=d.max_nodes, max_edges=d.max_edges, graph_sizes=d.graph_sizes)
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs(), plan)
        glf, instr = model.language_features(d.questions, d.att_mask)
        logits = model(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, return_masks=True, scene_graphs=d.scene_graphs())[0]
    assert float((res.logits - logits).abs().max()) <= LOGIT_TOL and torch.equal(res.pred, logits.argmax(1))

    def score(x_m, e_m):
        out = model.answer_graphs(x_m, d.edge_index, e_m, d.batch, instr, glf, plan, True, None, None)[0]
        return _nll(out.float(), res.pred)

    hand = explain.mask_optimize(score, state.x_enc, state.e_enc, plan, d.edge_index, steps=4, init_seed=2)
    for a, b, name in ((res.theta, hand.theta, "theta"), (res.soft, hand.soft, "soft"), (res.nll, hand.nll, "nll")):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert hand.pred is None and hand.logits is None
    ops.check_plans()


def test_compare_takes_the_learned_explainer_and_keeps_its_default(dev):
    from isubgvqa_amd import explain, ops, synthetic
    from test_gpu_occlusion import SIZES as SMALL_SIZES
    from test_gpu_occlusion import _answer_case, _plan
    V, A, K2, T = 200, 1842, 2, 10
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
    chosen = ("intrinsic", "mask_optimization")
    report = explain.compare(model, batches, tables, explainers=chosen, k=K2, seed=40, mo_steps=T)
    assert tuple(report) == chosen and torch.is_grad_enabled()
    makers = {"intrinsic": lambda d, intrinsic, number: intrinsic,
              "mask_optimization": lambda d, intrinsic, number: explain.mask_optimization(model, d, steps=T, init_seed=40 + number).mask(K2)}
    for name in chosen:
        coo = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
        ground = torch.zeros(ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
        plus, minus, jac = [], [], []
        for number, b in enumerate(batches):
            d = b.inputs
            with torch.no_grad():
                plan = _plan(ops, d, B)
                logits, intrinsic, _ = model(d, plan=plan)
            mask = makers[name](d, intrinsic, number)
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
