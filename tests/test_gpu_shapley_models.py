"""explain.shapley_values through the real models on the GPU: held bit for bit to the same run assembled by hand --
the restated positions (tests/shapley_restated.py), ops._pack_bits rows through ops.induced_instances, the same chunking, the same
forward, the restated estimator in the header's fp32 order --, untouched parameters and forwards, and compare(explainers=
(..., "shapley")) against .mask(k) and .scores() fed by hand.

Every comparison of probabilities is made inside EQUAL instance batches: a result depends on the composition of its batch (quirks
Q1 / Q3 / Q4), so nothing here is asserted across different chunkings.
TOLERANCES.  Positions, keep rows, probabilities and phi: exact.  gap within (n + 1) u (sum_i |phi_i| + |p - v_empty|) of the
float64 sum of the device's own phi (u = 2^-24: n - 1 additions, the subtraction p - v_empty, the final subtraction)."""
import math

import pytest
import torch

import shapley_restated as SR
from test_gpu_ig_models import SIZES, _answer

pytestmark = pytest.mark.gpu

M = 4                           # permutations: the 70-node graph stays a few hundred instances
PERM_SEED = (1 << 33) + 5


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
    sizes = (3, 7, 1, 34)
    return model, synthetic.make_full_workload(len(sizes), tokens=9, seed=3, sg_vocab=64, text_vocab=64, sizes=sizes).to(dev)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, what
    same = (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
    assert bool(same.all()), f"{what}: bits differ, max |d| = {(a - b).abs().nan_to_num().max().item():.3e}"


def _by_hand(model, d, permutations, antithetic, perm_seed, v_empty, max_instances):
    """shapley_values assembled from the restatement and torch ops: (pred, p, pos [M, N], row_ptr, keep, p_inst, phi, gap, flag)."""
    from isubgvqa_amd import explain, ops
    full, B, forward = explain._forwarder(model, d, None, None)
    dev = d.x.device
    with torch.no_grad():
        plan = explain._input_plan(d, B)
        logits = forward(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs() if full else None, plan)[0]
        prob = torch.softmax(logits.float(), dim=1)
        pred = prob.argmax(dim=1)
        p = prob.gather(1, pred.unsqueeze(1)).squeeze(1)
        ptr = plan.ptr.tolist()
        W = ops.keep_words(plan.nmax)
        pos = torch.zeros(permutations, plan.N, dtype=torch.int64)
        flags, index, row_ptr = [], [], [0]
        for g in range(B):
            lo, n = ptr[g], ptr[g + 1] - ptr[g]
            pm = SR.graph_positions(perm_seed, g, n, permutations, antithetic)
            pos[:, lo:lo + n] = pm
            for m in range(permutations):
                for k in range(1, n):
                    row = torch.zeros(32 * W, dtype=torch.bool)
                    row[:n] = pm[m] < k
                    flags.append(row)
                    index.append(g)
            row_ptr.append(len(index))
        keep = ops._pack_bits(torch.stack(flags).to(dev), W)
        index = torch.tensor(index, dtype=torch.int32, device=dev)
        Q = index.numel()
        step = Q if max_instances is None else max_instances
        parts = []
        for lo in range(0, Q, step):
            rows = index[lo:lo + step].long()
            inst = ops.induced_instances(plan, d.edge_index, index[lo:lo + step].contiguous(), keep[lo:lo + step].contiguous())
            inst.verify()
            out = forward(*explain.instance_inputs(d, inst, full), inst.plan(), rows, None)[0]
            parts.append(torch.softmax(out.float(), dim=1).gather(1, pred.index_select(0, rows).unsqueeze(1)).squeeze(1))
        p_inst = torch.cat(parts)
    phi, m2, gap, flag, _, sq_e = SR.values(p_inst.cpu(), p.cpu(), pos, ptr, list(range(B)), row_ptr, plan.N, permutations, Q, antithetic,
                                            v_empty, W)
    return pred, p, pos.int(), row_ptr, keep, p_inst, phi, gap, flag, sq_e


def _check_against_hand(model, d, max_instances, antithetic=True, v_empty=0.0):
    from isubgvqa_amd import explain, ops
    ops.reset_counters()
    res = explain.shapley_values(model, d, permutations=M, antithetic=antithetic, perm_seed=PERM_SEED, v_empty=v_empty,
                                 max_instances=max_instances)
    c = ops.counters()
    assert c["shapley_keep_bits"] == 1 and c["shapley_values"] == 1
    pred, p, pos, row_ptr, keep, p_inst, phi, gap, flag, sq_e = _by_hand(model, d, M, antithetic, PERM_SEED, v_empty, max_instances)
    B, Q = p.numel(), row_ptr[-1]
    sizes = (res.plan.ptr[1:] - res.plan.ptr[:-1]).tolist()
    assert Q == M * sum(max(n - 1, 0) for n in sizes)
    assert c["induced_instances"] == (1 if max_instances is None else math.ceil(Q / max_instances)) == len(res.chunks)
    res.bits.verify()
    assert torch.equal(res.pred, pred) and torch.equal(res.bits.pos.cpu(), pos) and res.bits.row_ptr.tolist() == row_ptr
    assert torch.equal(res.bits.keep, keep) and res.bits.graphs.tolist() == list(range(B)) and res.bits.status.tolist() == [0, 0, 0, Q]
    assert (res.bits.M, res.bits.antithetic, res.T) == (M, antithetic, M // 2 if antithetic else M)
    _same_bits(res.p, p, "p")
    _same_bits(res.p_inst, p_inst, "p_inst")
    _same_bits(res.attribution.cpu(), phi, "phi")
    _same_bits(res.gap.cpu(), gap, "gap")
    assert res.flag.tolist() == flag.tolist() == [0] * B and bool(torch.isfinite(res.attribution).all())
    T = res.T
    assert bool(((res.m2.cpu().double() - sq_e).abs() <= T * SR.U * sq_e).all())
    # the completeness gap from the device's own phi, inside the derived bound; single graphs get p - v_empty
    ptr = res.plan.ptr.tolist()
    ve = float(torch.tensor(v_empty, dtype=torch.float32))
    for g, n in enumerate(sizes):
        own = res.attribution[ptr[g]:ptr[g + 1]].double().cpu()
        whole = float(res.p[g].double()) - ve
        assert abs(float(res.gap[g]) - (float(own.sum()) - whole)) <= (n + 1) * SR.U * (float(own.abs().sum()) + abs(whole)), g
        assert bool(res.single[g]) == (n < 2)
        if n == 1:                                       # T equal samples d: their mean is d itself for T <= 2 (3 d may round)
            lone = float(res.p[g] - torch.tensor(v_empty, dtype=torch.float32).to(res.p.device))
            assert abs(float(res.attribution[ptr[g]]) - lone) <= (0.0 if T <= 2 else (T + 3) * SR.U * abs(lone))
    se = res.stderr()
    assert se.dtype == torch.float64 and se.shape == (res.plan.N,) and bool((se >= 0).all())
    return res


@pytest.mark.parametrize("which", ["unmasked", "masked"])
def test_shapley_values_equal_the_run_assembled_by_hand(request, dev, which):
    from isubgvqa_amd import explain, ops
    model, d = request.getfixturevalue(which)
    B, N = len(SIZES), sum(SIZES)
    res = _check_against_hand(model, d, None)
    assert res.attribution.shape == (N,) and res.gap.shape == (B,) and res.single.tolist() == [n < 2 for n in SIZES]
    assert res.scores().shape == (N,) and torch.equal(res.scores(), res.attribution)
    # in chunks (211 does not divide the 920 instances): no pos and no keep row changes; a second call gives the first one's bits
    chunked = _check_against_hand(model, d, 211)
    assert torch.equal(chunked.bits.pos, res.bits.pos) and torch.equal(chunked.bits.keep, res.bits.keep)
    again = explain.shapley_values(model, d, permutations=M, perm_seed=PERM_SEED, max_instances=211)
    for a, b, name in ((chunked.attribution, again.attribution, "phi"), (chunked.m2, again.m2, "m2"), (chunked.gap, again.gap, "gap"),
                       (chunked.p_inst, again.p_inst, "p_inst")):
        _same_bits(a, b, name)
    assert torch.equal(chunked.bits.pos, again.bits.pos)
    # another perm_seed gives other permutations; the caller's logits and plan are taken
    with torch.no_grad():
        plan = explain._input_plan(d, B)
        logits = model(d, plan=plan)[0]
    other = explain.shapley_values(model, d, permutations=2, perm_seed=PERM_SEED + 1, logits=logits, plan=plan)
    assert other.plan is plan and other.logits is logits and not torch.equal(other.bits.pos[0], res.bits.pos[0])
    assert other.T == 1 and bool(torch.isnan(other.stderr()).all())
    # the mask by Occlusion.mask's rule
    want = ops.topk_threshold(explain.shifted_attributions(res.attribution, d.batch, B).view(-1, 1).contiguous(), 3, plan=res.plan)
    assert torch.equal(res.mask(3), want)
    ops.check_plans()


def test_without_antithetic_and_with_a_value_for_the_empty_set(masked, dev):
    model, d = masked
    _check_against_hand(model, d, 300, antithetic=False, v_empty=0.03125)


def test_nothing_of_the_model_changes(masked, dev):
    from isubgvqa_amd import explain
    model, d = masked
    with torch.no_grad():
        before = model(d)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    explain.shapley_values(model, d, permutations=2, max_instances=250)
    with torch.no_grad():
        after = model(d)
    for a, b, name in zip(before, after, ("logits", "mask", "gate")):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert all(p.grad is None for p in model.parameters()) and not model.training and torch.is_grad_enabled()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.shapley_values(model.train(), d)
    model.eval()


def test_the_full_model(full, dev):
    from isubgvqa_amd import ops
    model, d = full
    res = _check_against_hand(model, d, None)
    _check_against_hand(model, d, 37)
    assert res.attribution.shape == (45,) and all(p.grad is None for p in model.parameters())
    ops.check_plans()


def test_compare_with_shapley_equals_the_masks_and_scores_fed_by_hand(dev):
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
    levels = (0.0, 0.5, 1.0)
    L = len(levels)
    before = explain.compare(model, batches, tables, explainers=("intrinsic", "random"), k=K2, seed=40)
    ops.reset_counters()
    report = explain.compare(model, batches, tables, explainers=("intrinsic", "shapley"), k=K2, seed=40, sv_permutations=4, curves=levels)
    assert ops.counters()["shapley_keep_bits"] == 2 and ops.counters()["shapley_values"] == 2
    plain = explain.compare(model, batches, tables, explainers=("intrinsic", "shapley"), k=K2, seed=40, sv_permutations=4)
    assert tuple(report) == ("intrinsic", "shapley") and plain["shapley"].curves is None
    # by hand: the masks of shapley_values(permutations=4, perm_seed=seed + batch number) through the same yardsticks
    coo = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    ground = torch.zeros(ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
    sums = torch.zeros(explain.COMPARE_SUMS, dtype=torch.float64, device=dev)
    acc = torch.zeros(2, L + 3, dtype=torch.float64, device=dev)
    for number, b in enumerate(batches):
        d = b.inputs
        with torch.no_grad():
            plan = explain._input_plan(d, B)
            logits, intrinsic = explain._forwarder(model, d, None, None)[2](d.x, d.edge_index, d.edge_attr, d.batch, None, plan)
            res = explain.shapley_values(model, d, permutations=4, perm_seed=40 + number, logits=logits, plan=plan)
            assert res.bits.M == 4 and res.bits.antithetic and res.flag.tolist() == [0] * B
            mask = res.mask(K2)
            pred = logits.argmax(dim=1)
            explain.fidelity_curves(model, d, res.scores(), fractions=levels, logits=logits, plan=plan, totals=acc)
            ops.token_coo(b.names, mask, plan, pred, b.label, tables.on("ans_sg", dev), b.qtok, b.qflags, None, None, threshold=0.0, totals=coo)
            ops.grounding(mask, plan, b.gold, pred, b.label, threshold=0.0, totals=ground)
            f = explain.faithfulness_of_mask(model, d, mask, threshold=0.0, logits=logits, plan=plan).scores
            has_p, has_m = ~torch.isnan(f.fid_plus), ~torch.isnan(f.fid_minus)
            sums += torch.cat([torch.stack([torch.where(has_p, f.fid_plus, torch.zeros_like(f.fid_plus)).double().sum(), has_p.double().sum(),
                                            torch.where(has_m, f.fid_minus, torch.zeros_like(f.fid_minus)).double().sum(), has_m.double().sum()]),
                               explain.jaccard_sums(mask, intrinsic, d.batch, B, 0.0)])
    for r in (report["shapley"], plain["shapley"]):
        assert r.sums == tuple(sums.cpu().tolist()) and r.coo.totals == explain.CooReport.from_totals(coo.cpu().tolist()).totals
        assert r.grounding.totals == explain.GroundingReport.from_totals(ground.cpu()).totals
    c, rows = report["shapley"].curves, acc.cpu().tolist()
    assert c.sums == tuple(tuple(r) for r in rows) and c.fractions == levels and c.counted == (2 * B, 2 * B) and c.skipped == (0, 0)
    # compare() without "shapley" gives the figures it gave before; the intrinsic report beside it is the same too
    after = explain.compare(model, batches, tables, explainers=("intrinsic", "random"), k=K2, seed=40)
    for name in ("intrinsic", "random"):
        assert (after[name].coo.totals, after[name].grounding.totals, after[name].sums) == \
            (before[name].coo.totals, before[name].grounding.totals, before[name].sums), name
    assert (plain["intrinsic"].coo.totals, plain["intrinsic"].sums) == (before["intrinsic"].coo.totals, before["intrinsic"].sums)
    ops.check_plans()
