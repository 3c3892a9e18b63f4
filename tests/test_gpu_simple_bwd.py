"""The SIMPLE sampler's backward kernel (csrc/isg_simple_bwd.hip, include/isg_sampler_train.h) on a real MI355X.

The checker is autograd through sampling/methods/simple.py::log_marginals in fp64 on the CPU (tests/simple_bwd_restated.py).  The
bound is measured in the test that applies it: the SAME restatement in fp32 has an error e32 against that fp64 result on the same
inputs, and the kernel may have 4 x e32 (device expf / logf against torch's, another order of summation, about 2 log2(n) chained
logsumexps) plus the absolute floor 5e-6 of the G9 test (tests/test_gpu_train.py::test_simple_sampler_matches_reference).  Both
errors are printed.  Shapes hold a handful of rows: every level layout the kernel has (no level, a level wider than a wave, more
than one leaf per lane, the longest row the LDS rule admits), k clamped to nmax, the impossible-root arm (more zero pads than k),
no -1e10 pads, and B = 5 rows so that the last workgroup is partly empty."""
import pytest
import torch

import simple_bwd_restated as R

pytestmark = pytest.mark.gpu

FLOOR = 5e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def _largest_nmax(k):
    from isubgvqa_amd import _lib_sampler_train
    rule = _lib_sampler_train.load().isg_simple_topk_bwd_row_bytes
    return max(m for m in range(1, 1025) if rule(k, m) > 0)


# name -> (nmax, k, row lengths); nmax None = the longest row the rule admits at that k
SHAPES = {
    "nmax=1": (1, 5, [1, 1, 1, 1, 1]),                    # no level: the gradient is exactly 0
    "nmax=2": (2, 5, [1, 2, 2, 1, 2]),
    "nmax=4": (4, 5, [1, 4, 2, 4, 3]),                    # k clamped to nmax
    "nmax=6 k=2": (6, 2, [1, 2, 3, 6, 6]),                # a length-1 row: more zero pads than k, the impossible-root arm
    "nmax=33 k=3": (33, 3, [1, 3, 4, 33, 20]),            # n = 64: a level wider than a wave
    "nmax=64": (64, 5, [1, 5, 6, 64, 40]),                # n = nmax: no -1e10 pads
    "nmax=65": (65, 5, [1, 5, 6, 65, 33]),                # n = 128: more than one leaf per lane
    "largest nmax at k=5": (None, 5, None),               # B = 2
    "nmax=32 k=16": (32, 16, [1, 16, 17, 32, 20]),
}
GRADS = {"g_out": (True, False), "g_marg": (False, True), "both": (True, True)}
_INPUTS, _REFS = {}, {}


def inputs(name):
    """(dense scores [B, nmax] ~ N(0, 1), lens, k, g_out [B, nmax], g_marg [B, nmax], real [B, nmax]) on the CPU, made once"""
    if name not in _INPUTS:
        nmax, k, lens = SHAPES[name]
        if nmax is None:
            nmax = _largest_nmax(k)
            lens = [nmax, nmax // 2 + k + 1]
        g = torch.Generator().manual_seed(1000 * nmax + k)
        B = len(lens)
        lens = torch.tensor(lens)
        dense, g_out, g_marg = (torch.randn(B, nmax, generator=g) for _ in range(3))
        real = torch.arange(nmax)[None, :] < lens[:, None]
        _INPUTS[name] = (dense * real, lens, k, g_out, g_marg, real)
    return _INPUTS[name]


def reference(name, grads):
    """(fp64 gradient [B, nmax], e32 = max error of the fp32 restatement against it), computed once and shared"""
    if (name, grads) not in _REFS:
        dense, lens, k, g_out, g_marg, _ = inputs(name)
        go, gm = (g_out if GRADS[grads][0] else None), (g_marg if GRADS[grads][1] else None)
        ref = R.grad_autograd(dense, lens, k, go, gm, torch.float64)
        e32 = (R.grad_autograd(dense, lens, k, go, gm, torch.float32).double() - ref).abs().max().item()
        assert torch.isfinite(ref).all()
        _REFS[(name, grads)] = (ref, e32)
    return _REFS[(name, grads)]


def ragged(dev, name):
    """(scores [N, 1] on the device, plan, real) of the shape's rows as MaskingModel hands them over"""
    from isubgvqa_amd import ops
    dense, lens, k, g_out, g_marg, real = inputs(name)
    batch = torch.repeat_interleave(torch.arange(len(lens)), lens)
    plan = ops.GraphPlan.build(batch.to(dev), None, num_graphs=len(lens))
    return dense[real].view(-1, 1).to(dev), plan, real


def kernel_ragged(dev, name, grads):
    from isubgvqa_amd import ops
    dense, lens, k, g_out, g_marg, real = inputs(name)
    sc, plan, _ = ragged(dev, name)
    go = g_out[real].view(-1, 1).to(dev) if GRADS[grads][0] else None
    gm = g_marg.to(dev) if GRADS[grads][1] else None
    d = ops.simple_topk_backward(sc, k, plan, go, gm)
    assert d is not None and d.shape == sc.shape
    return d


@pytest.mark.parametrize("grads", list(GRADS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_gradient_against_fp64(dev, name, grads):
    from isubgvqa_amd import ops
    dense, lens, k, g_out, g_marg, real = inputs(name)
    ref, e32 = reference(name, grads)
    before = ops.COUNTERS["simple_bwd_kernel"]
    d = kernel_ragged(dev, name, grads)
    assert ops.COUNTERS["simple_bwd_kernel"] == before + 1
    err = (d.cpu().view(-1).double() - ref[real]).abs().max().item()
    print(f"[simple bwd] {name} ({tuple(dense.shape)}, k={k}) {grads}: kernel {err:.3e}, fp32 restatement {e32:.3e}, "
          f"max |gradient| {ref.abs().max().item():.3e}")
    assert torch.isfinite(d).all()
    assert err <= 4 * e32 + FLOOR, (name, grads, err, e32)
    if dense.size(1) <= k:
        assert ref.abs().max().item() < 1e-12             # every slot is taken: the marginals are the constant 1
    if dense.size(1) == 1:
        assert not d.any(), "one slot has no level: exactly 0"


@pytest.mark.parametrize("name", ["nmax=6 k=2", "nmax=33 k=3", "nmax=65"])
def test_ragged_and_dense_layouts_give_the_same_bits(dev, name):
    """The dense call sees a ragged row's zero pads as scores 0.0 -- the value the ragged call pads with -- so with g_out = 0 on
    them both calls seed the same circuit; the real slots must agree bit for bit, and on g_marg alone too."""
    from isubgvqa_amd import ops
    dense, lens, k, g_out, g_marg, real = inputs(name)
    for grads, (use_out, use_marg) in GRADS.items():
        r = kernel_ragged(dev, name, grads).view(-1)
        d = ops.simple_topk_backward(dense.to(dev), k, None, (g_out * real).to(dev) if use_out else None,
                                     g_marg.to(dev) if use_marg else None)
        assert d.shape == dense.shape
        assert torch.equal(d.cpu()[real], r.cpu()), (name, grads)


@pytest.mark.parametrize("hint", [64, 100])
def test_hinted_plan_gives_the_unhinted_plans_bits(dev, hint):
    """A plan built with max_nodes= above the longest row (33): the backward follows the forward's row length, the device's true
    longest row, so d scores are the un-hinted plan's bit for bit -- at 64 the circuit has the same n and the hint would only add
    zero pads, at 100 it would double n.  g_marg is [B, true nmax] on both."""
    from isubgvqa_amd import ops
    name = "nmax=33 k=3"
    dense, lens, k, g_out, g_marg, real = inputs(name)
    sc, plain, _ = ragged(dev, name)
    batch = torch.repeat_interleave(torch.arange(len(lens)), lens)
    hinted = ops.GraphPlan.build(batch.to(dev), None, num_graphs=len(lens), max_nodes=hint)
    assert plain.nmax == 33 and hinted.nmax == hint
    go, gm = g_out[real].view(-1, 1).to(dev), g_marg.to(dev)
    for a_out, a_marg in ((go, None), (None, gm), (go, gm)):
        a = ops.simple_topk_backward(sc, k, plain, a_out, a_marg)
        b = ops.simple_topk_backward(sc, k, hinted, a_out, a_marg)
        assert a is not None and b is not None and float(a.abs().max()) > 0
        assert torch.equal(a, b), f"max_nodes={hint}: max difference {float((a - b).abs().max()):.3e}"
    leaves = []
    for plan in (plain, hinted):                         # and through autograd, forward and backward on the same plan
        leaf = sc.clone().requires_grad_(True)
        out, marg = ops.simple_topk(leaf, k, plan=plan, seed=11, return_marginals=True)
        ((out * go).sum() + (marg * gm).sum()).backward()
        leaves.append((out.detach(), marg.detach(), leaf.grad))
    for x, y in zip(*leaves):
        assert torch.equal(x, y)
    ops.check_plans()


def test_every_row_is_its_own(dev):
    from isubgvqa_amd import ops
    dense, lens, k, g_out, g_marg, real = inputs("nmax=65")
    sc, go, gm = dense.to(dev), g_out.to(dev), g_marg.to(dev)
    whole = ops.simple_topk_backward(sc, k, None, go, gm)
    for b in range(sc.size(0)):
        alone = ops.simple_topk_backward(sc[b:b + 1].contiguous(), k, None, go[b:b + 1].contiguous(), gm[b:b + 1].contiguous())
        assert torch.equal(alone[0], whole[b]), b


def test_the_sample_carries_no_gradient(dev):
    """Through autograd: another uniform draw or another seed changes the mask, never d scores; a repeated call repeats its bits."""
    from isubgvqa_amd import autograd, ops
    assert autograd.SIMPLE_BWD_KERNEL
    dense, lens, k, g_out, g_marg, real = inputs("nmax=33 k=3")
    sc, plan, _ = ragged(dev, "nmax=33 k=3")
    w = g_out[real].view(-1, 1).to(dev)
    n = 64
    gen = torch.Generator().manual_seed(5)

    def grad(**kw):
        leaf = sc.clone().requires_grad_(True)
        out = ops.simple_topk(leaf, k, plan=plan, **kw)
        (out * w).sum().backward()
        return out.detach(), leaf.grad

    u1, u2 = (torch.rand(len(lens), n, generator=gen).to(dev) for _ in range(2))
    runs = [grad(uniform=u1), grad(uniform=u2), grad(seed=11), grad(seed=12), grad(seed=11)]
    assert not torch.equal(runs[0][0] > 0.5, runs[1][0] > 0.5) and not torch.equal(runs[2][0] > 0.5, runs[3][0] > 0.5)
    for out, d in runs[1:]:
        assert torch.equal(d, runs[0][1])
    assert torch.equal(runs[2][0], runs[4][0])
    a, b = kernel_ragged(dev, "nmax=65", "both"), kernel_ragged(dev, "nmax=65", "both")
    assert torch.equal(a, b)


def _device_restatement_grad(sc, k, w_out, w_marg):
    """d scores of a dense batch by autograd through log_marginals on the device, written out as simple_topk's backward was
    before the kernel existed"""
    from isubgvqa_amd.sampling.methods.simple import LARGE_NUMBER, log_marginals
    B, nmax = sc.shape
    n = 1 << max(nmax - 1, 0).bit_length()
    leaf = sc.detach().clone().requires_grad_(True)
    flat = torch.cat([leaf.reshape(B, nmax), torch.full((B, n - nmax), -LARGE_NUMBER, dtype=sc.dtype, device=sc.device)], dim=1)
    marg = log_marginals(flat, min(k, nmax)).exp()[:, :nmax]
    outs, gs = [marg.view(sc.shape)], [w_out]
    if w_marg is not None:
        outs, gs = outs + [marg], gs + [w_marg]
    return torch.autograd.grad(outs, [leaf], gs)[0]


def test_fallback_beyond_the_lds_rule_and_the_switch(dev, monkeypatch):
    from isubgvqa_amd import autograd, ops
    k = 5
    nmax = _largest_nmax(k) + 1
    gen = torch.Generator().manual_seed(9)
    sc, w, wm = (torch.randn(2, nmax, generator=gen).to(dev) for _ in range(3))
    before = ops.COUNTERS["simple_bwd_kernel"]
    assert ops.simple_topk_backward(sc, k, None, w, None) is None
    leaf = sc.clone().requires_grad_(True)
    out, marg = ops.simple_topk(leaf, k, seed=1, return_marginals=True)
    ((out * w).sum() + (marg * wm).sum()).backward()
    assert ops.COUNTERS["simple_bwd_kernel"] == before, "a refused shape was counted as a kernel backward"
    assert torch.equal(leaf.grad, _device_restatement_grad(sc, k, w, wm)), "the fallback is not the restatement's gradient"
    # the switch off: the path of before, bit for bit, at a shape the kernel would take
    dense, lens, k, g_out, g_marg, real = inputs("nmax=6 k=2")
    sc, w, wm = dense.to(dev), g_out.to(dev), g_marg.to(dev)
    monkeypatch.setattr(autograd, "SIMPLE_BWD_KERNEL", False)
    before = ops.COUNTERS["simple_bwd_kernel"]
    for w_marg in (None, wm):
        leaf = sc.clone().requires_grad_(True)
        res = ops.simple_topk(leaf, k, seed=1, return_marginals=w_marg is not None)
        ((res * w).sum() if w_marg is None else (res[0] * w).sum() + (res[1] * w_marg).sum()).backward()
        assert torch.equal(leaf.grad, _device_restatement_grad(sc, k, w, w_marg))
    assert ops.COUNTERS["simple_bwd_kernel"] == before


def _bound(scores, lens, k, g_out, g_marg):
    """test_kernel_gradient_against_fp64's bound for these inputs: 4 x the fp32 restatement's error against fp64 + the floor"""
    ref = R.grad_autograd(scores, lens, k, g_out, g_marg, torch.float64)
    e32 = (R.grad_autograd(scores, lens, k, g_out, g_marg, torch.float32).double() - ref).abs().max().item()
    return 4 * e32 + FLOOR, e32


def test_through_the_masking_model(dev, monkeypatch):
    """MaskingModel(sampler_type='simple') on a 4-graph batch: parameter and input gradients with the kernel within the bound of
    those with the restatement, one kernel backward per sampler call."""
    from isubgvqa_amd import autograd, ops
    from isubgvqa_amd.models.masking import MaskingModel
    torch.manual_seed(3)
    C, k, lens = 64, 5, torch.tensor([7, 1, 9, 6])
    model = MaskingModel(C, C, masking_threshold=0.15, use_topk=True, sample_k=k, sampler_type="simple").to(dev).train()
    model.gate_dropout = 0.0
    gen = torch.Generator().manual_seed(4)
    N, B = int(lens.sum()), len(lens)
    batch = torch.repeat_interleave(torch.arange(B), lens).to(dev)
    x0, u0, w = torch.randn(N, C, generator=gen).to(dev), torch.randn(B, C, generator=gen).to(dev), torch.randn(N, 1, generator=gen).to(dev)

    def run(on):
        monkeypatch.setattr(autograd, "SIMPLE_BWD_KERNEL", on)
        model.zero_grad(set_to_none=True)
        x, u = x0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
        before = ops.COUNTERS["simple_bwd_kernel"]
        mask = model(x, u, batch, None, size=B, use_all_instrs=False, seed=21, u_is_per_graph=True)
        (mask * w).sum().backward()
        assert ops.COUNTERS["simple_bwd_kernel"] - before == (1 if on else 0)
        grads = {"x": x.grad, "u": u.grad}
        grads.update({n: p.grad for n, p in model.named_parameters() if p.grad is not None})
        return mask.detach(), grads

    mask_on, on = run(True)
    mask_off, off = run(False)
    assert torch.equal(mask_on, mask_off) and set(on) == set(off) and {"x", "u", "node_nn.0.weight", "ques_nn.0.weight"} <= set(on)
    with torch.no_grad():
        plan = ops.GraphPlan.build(batch, None, num_graphs=B)
        gate = model.gate_scores(x0, u0, batch, True, plan).cpu().view(-1)
    nmax = int(lens.max())
    real = torch.arange(nmax)[None, :] < lens[:, None]
    dense, g_out = torch.zeros(B, nmax), torch.zeros(B, nmax)
    dense[real], g_out[real] = gate, w.cpu().view(-1)
    bound, e32 = _bound(dense, lens, k, g_out, None)
    for name in sorted(on):
        err = (on[name] - off[name]).abs().max().item()
        print(f"[simple bwd] MaskingModel d {name}: |kernel - restatement| {err:.3e} (bound {bound:.3e}, fp32 restatement error {e32:.3e})")
        assert err <= bound, (name, err, bound)
    assert on["x"].abs().max().item() > 0


def test_through_the_text_sampling_call(dev, monkeypatch):
    """EdgeSIMPLEBatched(k=3) on a dense [3, 9] as --text_sampling calls it: both outputs carry a gradient."""
    from isubgvqa_amd import autograd, ops
    from isubgvqa_amd.sampling.methods.simple_scheme import EdgeSIMPLEBatched
    gen = torch.Generator().manual_seed(8)
    B, T, k = 3, 9, 3
    sc, w, wm = (torch.randn(B, T, 1, generator=gen) for _ in range(3))
    sampler = EdgeSIMPLEBatched(k=k, device=dev, policy="edge_candid")

    def run(on):
        monkeypatch.setattr(autograd, "SIMPLE_BWD_KERNEL", on)
        leaf = sc.to(dev).requires_grad_(True)
        before = ops.COUNTERS["simple_bwd_kernel"]
        mask, marg = sampler(leaf, train=True, seed=5)
        ((mask.squeeze(0) * w.to(dev)).sum() + (marg * wm.to(dev)).sum()).backward()
        assert ops.COUNTERS["simple_bwd_kernel"] - before == (1 if on else 0)
        return leaf.grad.cpu().view(B, T)

    on, off = run(True), run(False)
    bound, e32 = _bound(sc.view(B, T), torch.full((B,), T), k, w.view(B, T), wm.view(B, T))
    err = (on - off).abs().max().item()
    ref = R.grad_autograd(sc.view(B, T), torch.full((B,), T), k, w.view(B, T), wm.view(B, T))
    print(f"[simple bwd] EdgeSIMPLEBatched [3, 9] k=3: |kernel - restatement| {err:.3e}, kernel against fp64 "
          f"{(on.double() - ref).abs().max().item():.3e} (bound {bound:.3e}, fp32 restatement error {e32:.3e})")
    assert err <= bound and (on.double() - ref).abs().max().item() <= bound
