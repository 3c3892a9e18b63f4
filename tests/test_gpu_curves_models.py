"""explain.fidelity_curves through the real models on the GPU: held bit for bit to the same run assembled by hand --
stable torch.argsort ranks, ops._pack_bits rows through ops.induced_instances, the same chunking, the same forward --, untouched
parameters and forwards, and compare(curves=...) against the explainers' .scores() fed to fidelity_curves directly.

Every comparison of probabilities is made inside EQUAL instance batches: a result depends on the composition of its batch (quirks
Q1 / Q3 / Q4), so nothing here is asserted across different chunkings or against subgraph_cut forwards.
TOLERANCES.  Probabilities, ranks, level sizes and counts: exact.  An area against float64 on the device's own probabilities:
L u sum_j |w_j p_j| (u = 2^-24; tests/curves_restated.py).  A double total: R 2^-53 sum |x|."""
import math

import pytest
import torch

import curves_restated as CR
from test_gpu_ig_models import SIZES, _answer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def unmasked(dev):
    return _answer(dev, (1.0, 1.0, 1.0), 9)[1::2]


@pytest.fixture(scope="module")
def masked(dev):
    return _answer(dev, (1.0, 1.0, 0.15), 1)[1::2]


@pytest.fixture(scope="module")
def full(dev):
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(sg_vocab_size=64, text_vocab_size=64), None).eval().to(dev)
    sizes = (3, 7, 5, 66)
    return model, synthetic.make_full_workload(len(sizes), tokens=9, seed=3, sg_vocab=64, text_vocab=64, sizes=sizes).to(dev)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
    assert bool(same.all()), f"{what}: bits differ, max |d| = {(a - b).abs().nan_to_num().max().item():.3e}"


def _tied_scores(N, dev, seed):
    """fp32 [N]: few distinct values, so that ties decide ranks in every graph."""
    return (torch.randint(0, 9, (N,), generator=torch.Generator().manual_seed(seed)).float() / 4 - 1).to(dev)


def _by_hand(model, d, scores, fractions, max_instances):
    """fidelity_curves assembled from torch ops: (pred, p, rank [N], level_k [B, L, 2], p_inst [B, L, 2], the listed graphs)."""
    from isubgvqa_amd import explain, ops
    full, B, forward = explain._forwarder(model, d, None, None)
    with torch.no_grad():
        plan = explain._input_plan(d, B)
        logits = forward(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs() if full else None, plan)[0]
        prob = torch.softmax(logits.float(), dim=1)
        pred = prob.argmax(dim=1)
        p = prob.gather(1, pred.unsqueeze(1)).squeeze(1)
        ptr = plan.ptr.tolist()
        W = ops.keep_words(plan.nmax)
        L = len(fractions)
        rank = torch.zeros(plan.N, dtype=torch.int64, device=scores.device)
        flags, index, level_k = [], [], torch.zeros(B, L, 2, dtype=torch.int32)
        for g in range(B):
            lo, n = ptr[g], ptr[g + 1] - ptr[g]
            order = torch.argsort(scores[lo:lo + n], descending=True, stable=True)
            rank[lo + order] = torch.arange(n, device=scores.device)
            local = torch.zeros(32 * W, dtype=torch.int64, device=scores.device)
            local[:n] = rank[lo:lo + n]
            inside = torch.arange(32 * W, device=scores.device) < n
            for j, t in enumerate(CR.level_sizes(n, fractions)):
                for s, removal in enumerate((False, True)):
                    k = CR.side_k(n, t, removal)
                    level_k[g, j, s] = k
                    flags.append(inside & ((local < k) != removal))
                    index.append(g)
        keep = ops._pack_bits(torch.stack(flags), W)
        index = torch.tensor(index, dtype=torch.int32, device=scores.device)
        Q = index.numel()
        step = Q if max_instances is None else max_instances
        parts = []
        for lo in range(0, Q, step):
            rows = index[lo:lo + step].long()
            inst = ops.induced_instances(plan, d.edge_index, index[lo:lo + step].contiguous(), keep[lo:lo + step].contiguous())
            inst.verify()
            out = forward(*explain.instance_inputs(d, inst, full), inst.plan(), rows, None)[0]
            parts.append(torch.softmax(out.float(), dim=1).gather(1, pred.index_select(0, rows).unsqueeze(1)).squeeze(1))
        return pred, p, rank.int(), level_k, torch.cat(parts).view(B, L, 2), keep


def _check_against_hand(model, d, scores, max_instances, fractions=None):
    from isubgvqa_amd import explain, ops
    fr = explain.CURVE_FRACTIONS if fractions is None else fractions
    ops.reset_counters()
    res = explain.fidelity_curves(model, d, scores, max_instances=max_instances, **({} if fractions is None else {"fractions": fractions}))
    c = ops.counters()
    assert c["curve_keep_bits"] == 1 and c["curve_sums"] == 1
    pred, p, rank, level_k, p_inst, keep = _by_hand(model, d, scores, fr, max_instances)
    B, L = p.numel(), len(fr)
    assert c["induced_instances"] == (1 if max_instances is None else math.ceil(2 * B * L / max_instances)) == len(res.chunks)
    assert torch.equal(res.pred, pred) and torch.equal(res.rank, rank) and torch.equal(res.level_k.cpu(), level_k)
    assert torch.equal(res.bits.keep, keep) and res.bits.graphs.tolist() == list(range(B))
    _same_bits(res.p, p, "p")
    _same_bits(res.p_keep, p_inst[:, :, 0].contiguous(), "p_keep")
    _same_bits(res.p_remove, p_inst[:, :, 1].contiguous(), "p_remove")
    # the areas and the totals from the device's own probabilities
    w = explain.curve_weights(fr)
    assert torch.equal(res.weights, w) and res.totals.shape == (2, L + 3)
    auc, bound, totals, tbound = CR.sums(p_inst.cpu().reshape(-1), w.float(), B, L, 2)
    for s, got in enumerate((res.auc_keep, res.auc_remove)):
        assert got.shape == (B,) and bool(((got.cpu().double() - auc[:, s]).abs() <= bound[:, s]).all())
    assert bool(((res.totals.cpu() - totals).abs() <= tbound).all())
    assert res.totals[:, L + 1].tolist() == [B, B] and res.totals[:, L + 2].tolist() == [0, 0]
    assert bool(torch.isfinite(res.p_keep).all()) and bool(torch.isfinite(res.p_remove).all())
    return res


@pytest.mark.parametrize("which", ["unmasked", "masked"])
def test_fidelity_curves_equal_the_run_assembled_by_hand(request, dev, which):
    from isubgvqa_amd import explain, ops
    model, d = request.getfixturevalue(which)
    B, N = len(SIZES), sum(SIZES)
    scores = _tied_scores(N, dev, 3)
    res = _check_against_hand(model, d, scores, None)
    assert res.p_keep.shape == res.p_remove.shape == (B, 7) and res.level_k.shape == (B, 7, 2)
    # the one-node graph: both sides of every level are the whole graph
    one = SIZES.index(1)
    assert res.level_k[one].tolist() == [[1, 0]] * 7
    # in chunks (47 does not divide the 168 instances), and a second call gives the first one's bits
    chunked = _check_against_hand(model, d, scores, 47)
    again = explain.fidelity_curves(model, d, scores, max_instances=47)
    for a, b, name in ((chunked.p_keep, again.p_keep, "p_keep"), (chunked.p_remove, again.p_remove, "p_remove"),
                       (chunked.auc_keep, again.auc_keep, "auc_keep"), (chunked.auc_remove, again.auc_remove, "auc_remove")):
        _same_bits(a, b, name)
    assert torch.equal(chunked.totals, again.totals)
    # counts, one side, running totals, the caller's logits and plan
    with torch.no_grad():
        plan = explain._input_plan(d, B)
        logits = model(d, plan=plan)[0]
    acc = torch.zeros(1, 5, dtype=torch.float64, device=dev)
    first = explain.fidelity_curves(model, d, scores, counts=(1, 3), sides=("remove",), logits=logits, plan=plan, totals=acc)
    assert first.totals is acc and first.p_keep is None and first.auc_keep is None and first.p_remove.shape == (B, 2)
    assert first.level_k[:, :, 0].tolist() == [[min(n - 1, 1), min(n - 1, 3)] for n in SIZES]
    assert torch.allclose(first.weights, torch.tensor([1 / 3, 1 / 3], dtype=torch.float64), rtol=0, atol=1e-15)   # x = (1/3, 1): both (1 - 1/3) / 2
    once = acc.clone()
    explain.fidelity_curves(model, d, scores, counts=(1, 3), sides=("remove",), logits=logits, plan=plan, totals=acc)
    assert torch.equal(acc, 2 * once) and acc[0, 3].item() == 2 * B
    ops.check_plans()


def test_nothing_of_the_model_changes(masked, dev):
    from isubgvqa_amd import explain
    model, d = masked
    with torch.no_grad():
        before = model(d)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    explain.fidelity_curves(model, d, _tied_scores(sum(SIZES), dev, 4), max_instances=60)
    with torch.no_grad():
        after = model(d)
    for a, b, name in zip(before, after, ("logits", "mask", "gate")):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert all(p.grad is None for p in model.parameters()) and not model.training and torch.is_grad_enabled()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.fidelity_curves(model.train(), d, _tied_scores(sum(SIZES), dev, 4))
    model.eval()


def test_the_full_model(full, dev):
    from isubgvqa_amd import ops
    model, d = full
    N = d.x.size(0)
    res = _check_against_hand(model, d, _tied_scores(N, dev, 5), None, fractions=(0.0, 0.3, 1.0))
    _check_against_hand(model, d, _tied_scores(N, dev, 5), 7, fractions=(0.0, 0.3, 1.0))
    assert res.p_keep.shape == (4, 3) and all(p.grad is None for p in model.parameters())
    ops.check_plans()


def test_compare_with_curves_equals_the_scores_fed_directly(dev):
    from isubgvqa_amd import explain, ops, synthetic
    from test_gpu_occlusion import SIZES as SMALL_SIZES
    from test_gpu_occlusion import _answer_case
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
            qtok = torch.full((B, 4), -1, dtype=torch.int32)
            qtok[:, :3] = torch.randint(0, V, (B, 3), generator=gen).int()
            gold = synthetic.make_gold(SMALL_SIZES, facets=2, entries=3, seed=seed)
            batches.append(explain.EvalBatch(d, label.to(dev), qtok.to(dev), (torch.arange(B) % 2).int().to(dev), names.to(dev),
                                             gold=gold.to(dev)))
    chosen = ("intrinsic", "occlusion", "random", "attention")
    levels = (0.0, 0.25, 0.5, 1.0)
    plain = explain.compare(model, batches, tables, explainers=chosen, k=K2, seed=40)
    report = explain.compare(model, batches, tables, explainers=chosen, k=K2, seed=40, curves=levels)
    assert tuple(report) == chosen and all(r.curves is None for r in plain.values())
    L = len(levels)
    for name in chosen:
        acc = torch.zeros(2, L + 3, dtype=torch.float64, device=dev)
        for number, b in enumerate(batches):
            d = b.inputs
            with torch.no_grad():
                plan = explain._input_plan(d, B)
                logits, intrinsic = explain._forwarder(model, d, None, None)[2](d.x, d.edge_index, d.edge_attr, d.batch, None, plan)
            scores = {"intrinsic": lambda: intrinsic, "occlusion": lambda: explain.occlusion(model, d).scores(),
                      "random": lambda: explain.random_scores(plan, 40 + number),
                      "attention": lambda: explain.attention_rollout(model, d).scores()}[name]()
            explain.fidelity_curves(model, d, scores, fractions=levels, logits=logits, plan=plan, totals=acc)
        c, rows = report[name].curves, acc.cpu().tolist()
        assert c.sums == tuple(tuple(r) for r in rows), name
        assert c.fractions == levels and c.counted == (2 * B, 2 * B) and c.skipped == (0, 0), name
        assert c.p_keep == tuple(rows[0][j] / (2 * B) for j in range(L)) and c.p_remove == tuple(rows[1][j] / (2 * B) for j in range(L))
        assert c.auc_keep == rows[0][L] / (2 * B) and c.auc_remove == rows[1][L] / (2 * B)
        assert 0.0 <= c.auc_keep <= 1.0 and 0.0 <= c.auc_remove <= 1.0
        # everything else of the report is what compare() gives without curves
        r, q = report[name], plain[name]
        assert (r.coo.totals, r.grounding.totals, r.sums) == (q.coo.totals, q.grounding.totals, q.sums), name      # (the reports' means may be NaN)
    # the random explainer's scores are the noise its mask ranks; an explainer's scores are what its mask ranks
    plan = explain._input_plan(batches[0].inputs, B)
    assert torch.equal(explain.random_mask(plan, K2, 40), ops.topk_threshold(explain.random_scores(plan, 40), K2, plan=plan))
    occ = explain.occlusion(model, batches[0].inputs)
    assert occ.scores().shape == (N,) and torch.equal(occ.scores(), occ.attribution)
    ops.check_plans()
