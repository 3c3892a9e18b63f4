"""explain.compare over all eight explainers at once against compare called with one name at a time: what an
explainer reports does not depend on which others stand beside it.  Every total is an integer count or a float64 sum of values
that the same launches produce in the same order, so the reports are compared as exact tuples.  The smallest inputs that reach
every arm: a graph that gets no instance, chunks of seven instances, both curve sides, both families of EvalBatch totals.

The launch counters are deliberately NOT asserted to satisfy `all eight = the eight single runs - 7 x compare(("intrinsic",))`: a
run with "intrinsic" alone makes the batch forward AND that explainer's yardsticks (token_coo, grounding, the two cuts of
faithfulness_of_mask and their forwards), so seven of them take away more than the seven batch forwards the single runs repeat.
The identity does not hold on the code before the table either; the per-explainer launch counts stay pinned by the suites of the
explainers themselves."""
import pytest
import torch

from test_gpu_occlusion import SIZES, _answer_case

pytestmark = pytest.mark.gpu

NAMES = ("intrinsic", "occlusion", "random", "attention", "integrated_gradients", "grad_x_input", "mask_optimization", "shapley")
K2 = 2
LEVELS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def _totals(r):
    return r.coo.totals, r.grounding.totals, r.sums, r.curves.sums


def test_compare_over_all_eight_equals_compare_one_name_at_a_time(dev):
    from isubgvqa_amd import explain, ops, synthetic
    V, A = 200, 1842
    tables = explain.TokenTables({f"w{i}": i for i in range(V)}, [f"w{(11 * a) % V}" if a % 3 == 0 else f"answer {a}" for a in range(A)])
    model, _ = _answer_case(dev)
    gen = torch.Generator().manual_seed(13)
    batches = []
    B, N = len(SIZES), sum(SIZES)
    with torch.no_grad():
        for seed in (5, 6):
            d = _answer_case(dev, seed)[1]
            names = torch.randint(0, V, (N,), generator=gen)
            label = model(d)[0].argmax(1).cpu()
            qtok = torch.full((B, 4), -1, dtype=torch.int32)
            qtok[:, :3] = torch.randint(0, V, (B, 3), generator=gen).int()
            gold = synthetic.make_gold(SIZES, facets=2, entries=3, seed=seed)
            batches.append(explain.EvalBatch(d, label.to(dev), qtok.to(dev), (torch.arange(B) % 2).int().to(dev), names.to(dev),
                                             gold=gold.to(dev)))
    kw = dict(k=K2, seed=40, ig_steps=2, mo_steps=2, sv_permutations=2, curves=LEVELS, max_instances=7)
    report = explain.compare(model, batches, tables, explainers=NAMES, **kw)
    assert tuple(report) == NAMES
    for name in NAMES:
        alone = explain.compare(model, batches, tables, explainers=(name,), **kw)
        assert tuple(alone) == (name,)
        assert _totals(report[name]) == _totals(alone[name]), name
        assert report[name].curves.fractions == LEVELS and report[name].curves.counted == (2 * B, 2 * B), name
    assert all(p.grad is None for p in model.parameters())
    ops.check_plans()
