"""ops.cross_entropy / isg_xent_fwd / isg_xent_bwd on a real MI355X against F.cross_entropy in float64 on the CPU.

Shapes: B in {1, 2, 65} x A in {1, 2, 63, 64, 65, 257, 1842}, each with ld = A and as a column slice of an [B, A + 3] matrix that
starts at column 1 (rows then sit on 4-byte boundaries only).

TOLERANCE, per quantity and per case: torch's own float32 CPU cross_entropy (forward and backward) is run on the same inputs; its
max abs error against float64 is e32, and the kernels get max(4 * e32, one float32 ulp of the largest expected value).  The
factor covers a different but equally valid summation order and expf.  Measured on the MI355X, the worst over all shapes
(kernel error / torch-float32 error, each the max abs error against float64):
    mean_loss                 1.77e-07 / 6.14e-08  (ties, B = 1, A = 1842, ld=A: 0.72 of the bound)
    loss (fp32)               7.48e-07 / 2.06e-07  (normal, B = 2, A = 1842, slice: 0.78 of the bound)
    row_loss                  1.77e-07 / 6.14e-08  (ties, B = 1, A = 1842, ld=A: 0.72 of the bound)
    d_logits                  4.87e-08 / 1.09e-08  (ties, B = 1, A = 1842, ld=A: 0.82 of the bound)
    d_logits (upstream 0.37)  2.50e-08 / 4.80e-09  (ties, B = 1, A = 65, slice: 0.84 of the bound)
Before the logarithm moved to double, mean_loss of the all-equal row at B = 1, A = 257 missed its bound: 4.81e-07 against one
ulp, 4.77e-07 (torch float32: 4.6e-09).
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import parity_record

pytestmark = pytest.mark.gpu

BS, AS = (1, 2, 65), (1, 2, 63, 64, 65, 257, 1842)
SHAPES = [(B, A, sl) for B, A in itertools.product(BS, AS) for sl in (False, True)]
KINDS = ("normal", "shifted", "equal_row", "ties", "ignored_mixed", "ignored_all", "nan_logit")
WORST = {}       # quantity -> (kernel error, torch float32 error) at the case where kernel error / tolerance was largest


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def accuracy(output, target, topk=(1,)):
    """ISubGVQA/utils/accuracies.py::accuracy, restated."""
    with torch.no_grad():
        maxk = max(topk)
        batch_size = target.size(0)
        _, pred = output.topk(maxk, 1, True, True)
        pred = pred.t()
        correct = pred.eq(target.view(1, -1).expand_as(pred))
        res = []
        for k in topk:
            correct_k = correct[:k].reshape(-1).float().sum(0, keepdim=True)
            res.append(correct_k.mul_(100.0 / batch_size))
        return res


def make_case(kind, B, A, seed):
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(B, A, generator=g)
    y = torch.randint(0, A, (B,), generator=g)
    if kind == "shifted":
        x = x + 1e4
    elif kind == "equal_row":
        x[B // 2] = 1.25
    elif kind == "ties":
        for b in range(B):          # the maximum sits at two or three places of every row; the label is the lowest of them in row 0
            idx = torch.randperm(A, generator=g)[:3]
            x[b, idx] = x[b].max() + 1.0
            if b == 0:
                y[b] = idx.min()
    elif kind == "ignored_mixed":
        y[::2] = -100
    elif kind == "ignored_all":
        y[:] = -100
    elif kind == "nan_logit":
        x[B - 1, A // 2] = float("nan")
    return x, y


def reference(x, y, dtype, upstream):
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    row = F.cross_entropy(xr, y, reduction="none")
    loss = F.cross_entropy(xr, y)
    (loss * upstream).backward()
    return loss.detach().double(), row.detach().double(), xr.grad.double()


def on_device(x, y, dev, sliced, totals=None, upstream=None):
    """The kernels' (result, d_logits): logits as a leaf [B, A], or as columns 1 .. A of a leaf [B, A + 3]."""
    B, A = x.shape
    if sliced:
        wide = torch.full((B, A + 3), 7.0)
        wide[:, 1:A + 1] = x
        leaf = wide.to(dev).requires_grad_(True)
        logits = leaf[:, 1:A + 1]
    else:
        leaf = x.to(dev).requires_grad_(True)
        logits = leaf
    from isubgvqa_amd import ops
    res = ops.cross_entropy(logits, y.to(dev), totals=totals)
    (res.loss if upstream is None else res.loss * upstream).backward()
    grad = leaf.grad
    if sliced:
        assert float(grad[:, 0].abs().max()) == 0.0 and float(grad[:, A + 1:].abs().max()) == 0.0
        grad = grad[:, 1:A + 1]
    return res, grad.detach().cpu().double()


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def hold(what, got, ref64, ref32, case):
    """got within max(4 x torch-float32's error, one float32 ulp of the largest expected value) of float64; NaN where it has NaN."""
    got, ref64, ref32 = got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)
    nan = torch.isnan(ref64)
    assert torch.equal(torch.isnan(got), nan), f"{what} {case}: NaN pattern differs from float64's"
    if bool(nan.all()):
        return
    keep = ~nan
    e32 = float((ref32[keep] - ref64[keep]).abs().max())
    err = float((got[keep] - ref64[keep]).abs().max())
    tol = max(4.0 * e32, ulp32(ref64[keep].abs().max()))
    print(f"[xent] {what} {case}: kernel error {err:.3e}, torch float32 error {e32:.3e}, tolerance {tol:.3e}")
    if what not in WORST or err / tol > WORST[what][2]:
        WORST[what] = (err, e32, err / tol, str(case))
    assert err <= tol, f"{what} {case}: |kernel - float64| = {err:.3e} > {tol:.3e} (torch float32: {e32:.3e})"


@pytest.mark.parametrize("kind", KINDS)
def test_loss_rows_and_gradient_against_float64(dev, kind):
    WORST.clear()
    for i, (B, A, sliced) in enumerate(SHAPES):
        x, y = make_case(kind, B, A, seed=1000 + i)
        case = (kind, B, A, "slice" if sliced else "ld=A")
        for upstream in (None, 0.37):
            l64, r64, g64 = reference(x, y, torch.float64, 1.0 if upstream is None else upstream)
            l32, r32, g32 = reference(x, y, torch.float32, 1.0 if upstream is None else upstream)
            res, grad = on_device(x, y, dev, sliced, upstream=upstream)
            hold("d_logits" + ("" if upstream is None else " (upstream 0.37)"), grad, g64, g32, case)
        hold("mean_loss", res.stats[0].cpu(), l64, l32, case)
        hold("loss (fp32)", res.loss.detach().cpu().double(), l64, l32, case)
        hold("row_loss", res.row_loss.cpu().double(), r64, r32, case)
        stats = res.stats.cpu().tolist()
        counted = int((y != -100).sum())
        assert stats[1] == counted and stats[3] == B
        if kind == "ignored_all":
            assert np.isnan(stats[0]) and stats[2] == 0 and float(grad.abs().max()) == 0.0
        if kind in ("ignored_mixed", "ignored_all"):
            assert float(res.row_loss.cpu()[y == -100].abs().max()) == 0.0 and float(grad[y == -100].abs().max()) == 0.0
        if kind == "nan_logit":
            assert np.isnan(stats[0]) and bool(torch.isnan(res.row_loss[B - 1]))
        if kind in ("ties", "equal_row"):
            first = (x == x.max(1, keepdim=True).values).int().argmax(1)            # the lowest index among a row's maxima
            assert torch.equal(res.pred.cpu().long(), first), case
        assert res.pred.dtype == torch.int32 and res.loss.dim() == 0 and res.loss.dtype == torch.float32
    parity_record(f"xent_{kind}", {k: {"kernel": v[0], "torch_float32": v[1], "over_tolerance": v[2], "case": v[3]} for k, v in WORST.items()})


def test_top1_and_meters_equal_the_references_accuracy(dev):
    """n_correct and Meters' acc@1 against the reference's accuracy() on tie-free inputs.  The count is compared exactly; the
    percentage exactly against 100 * count / B in double, and against accuracy()'s own float32 product (count * float32(100 / B))
    within one float32 ulp of 100, which is what separates the two."""
    from isubgvqa_amd import ops, train
    for i, (B, A, sliced) in enumerate(SHAPES):
        x, y = make_case("normal", B, A, seed=2000 + i)
        assert all(int((r == r.max()).sum()) == 1 for r in x), "tie-free inputs: one maximum per row"
        y[::3] = x.argmax(1)[::3]                    # a third of the rows certainly correct
        ref = float(accuracy(x, y)[0])
        n_ref = int((x.argmax(1) == y).sum())
        assert abs(ref - 100.0 * n_ref / B) <= ulp32(100.0)
        meters = train.Meters(dev)
        xd = (torch.cat([x[:, :1], x, x[:, :2]], 1).to(dev)[:, 1:A + 1]) if sliced else x.to(dev)
        with torch.no_grad():
            res = ops.cross_entropy(xd, y.to(dev), totals=meters.totals)
        assert torch.equal(res.pred.cpu().long(), x.argmax(1))
        assert res.stats.cpu().tolist()[2] == n_ref
        rep = meters.report()
        assert rep["acc1"] == 100.0 * n_ref / B and abs(rep["acc1"] - ref) <= ulp32(100.0), (B, A, rep, ref)
        assert (rep["steps"], rep["rows"], rep["nonfinite_losses"]) == (1, B, 0)
        assert rep["loss"] == float(res.loss), "the meter takes the fp32 loss, as loss.item() is"


def test_totals_skip_a_nan_loss_and_count_it(dev):
    from isubgvqa_amd import ops, train
    meters = train.Meters(dev)
    seq = [("normal", 65, 257), ("nan_logit", 65, 257), ("ignored_mixed", 2, 1842), ("ignored_all", 2, 63)]
    losses, rows, correct = [], [], 0
    for i, (kind, B, A) in enumerate(seq):
        x, y = make_case(kind, B, A, seed=3000 + i)
        before = meters.totals.clone()
        with torch.no_grad():
            res = ops.cross_entropy(x.to(dev), y.to(dev), totals=meters.totals)
        after = meters.totals.cpu()
        if kind in ("nan_logit", "ignored_all"):
            assert torch.equal(after[:2], before.cpu()[:2]), "a nonfinite loss leaves the loss sum and its row count alone"
            assert after[5] == before.cpu()[5] + 1
        else:
            losses.append(float(res.loss))
            rows.append(B)
            assert after[5] == before.cpu()[5]
        correct += int(res.stats[2])
    rep = meters.report()
    assert rep["loss"] == sum(l * n for l, n in zip(losses, rows)) / sum(rows)
    assert (rep["steps"], rep["nonfinite_losses"], rep["rows"]) == (4, 2, 65 + 65 + 2 + 2)
    assert rep["acc1"] == 100.0 * correct / rep["rows"]


def test_an_out_of_range_label_makes_the_row_and_the_step_nonfinite(dev):
    from isubgvqa_amd import ops
    x, y = make_case("normal", 65, 64, seed=5)
    y[7], y[9] = 64, -3
    res, grad = on_device(x, y, dev, False)
    row = res.row_loss.cpu()
    assert bool(torch.isnan(row[[7, 9]]).all()) and int(torch.isnan(row).sum()) == 2 and bool(torch.isnan(res.loss))
    assert bool(torch.isnan(grad[[7, 9]]).all())


def test_two_identical_calls_give_the_same_bits(dev):
    for kind, B, A, sliced in (("normal", 65, 1842, True), ("shifted", 65, 257, False), ("ignored_mixed", 2, 65, True)):
        x, y = make_case(kind, B, A, seed=77)
        (r1, g1), (r2, g2) = on_device(x, y, dev, sliced, upstream=0.37), on_device(x, y, dev, sliced, upstream=0.37)
        for a, b in zip(tuple(r1) + (g1,), tuple(r2) + (g2,)):
            assert a.detach().cpu().contiguous().numpy().tobytes() == b.detach().cpu().contiguous().numpy().tobytes(), (kind, B, A)


def test_classifier_weight_gradient_agrees_with_f_cross_entropy(dev):
    """autograd.linear(512 -> 1842) under ops.cross_entropy against the same Linear under F.cross_entropy, within the tolerance
    tests/test_gpu_train.py holds parameter gradients to (2e-4 of the tensor's largest entry)."""
    from isubgvqa_amd import autograd, ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(65, 512, generator=g).to(dev)
    w = (torch.randn(1842, 512, generator=g) / 512 ** 0.5).to(dev).requires_grad_(True)
    b = (0.1 * torch.randn(1842, generator=g)).to(dev).requires_grad_(True)
    y = torch.randint(0, 1842, (65,), generator=g).to(dev)
    ops.cross_entropy(autograd.linear(x, w, b, False), y).loss.backward()
    ours = (w.grad.clone(), b.grad.clone())
    w.grad = b.grad = None
    F.cross_entropy(autograd.linear(x, w, b, False), y).backward()
    for got, ref, name in zip(ours, (w.grad, b.grad), ("weight", "bias")):
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max()) / scale
        print(f"[xent] classifier {name} gradient: max |diff| / max |ref| = {err:.3e}")
        assert err < 2e-4, (name, err)
