"""The top-k samplers with a k per row (include/isg_topk_rows.h, csrc/isg_topk_rows.hip) on a real MI355X.

Every comparison of the kernels is bit for bit.  The reference for row b is the scalar entry point (isg_topk_threshold /
isg_topk_gumbel / isg_topk_gumbel_bwd, which tests/test_gpu_samplers.py pins to the oracle) run on the WHOLE batch at
k = k_rows[b], of which the rows of graph b are taken: once per distinct k, at most 6 per case.  No tolerance: a row's arithmetic is
the scalar kernel's, only its loop count is read per row.

Shapes.  nmax in {1, 33, 64, 65, 130}: SLOTS 1, 2 and 4 and the boundary between 1 and 2.  B in {1, 5, 9}: none a multiple of the 4
rows of a workgroup, so the last workgroup is partly empty and every full one holds rows of different k.  Ragged rows mix the
lengths 1, k_b, k_b + 1 and nmax; the dense layout runs beside them.  k_rows mix 1, 2, 3, nmax (the all-ones branch of the threshold
solve, local_k = nmax of the relaxation) and k_cap = nmax + 2; for the Gumbel backward k_cap is what the LDS rule
k_cap * slots * 64 <= 4096 leaves of that, and one case beyond it is refused.

The model-level cases (AnswerModel, C = 128, two masked layers, 12 graphs) compare a model with a budget against scalar-k models:
bit for bit where every graph gets the same k, and per graph within the project's 1e-4 logit bound on mixed sizes (the masks of
the other graphs differ between the two batches, so tile grouping may).
"""
import ctypes
import functools
import os

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

STRICT = os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc", "libisg_hip_strict.so")
EUNSUPPORTED = -2
TAU = 0.5
NMAXES = (1, 33, 64, 65, 130)
BATCHES = (1, 5, 9)
GUARD = 64                         # words behind every buffer a kernel writes or reads per row
SENTINEL = -12345.0
LOGIT_BOUND = 1e-4                 # the project's bound on logits between two dispatches of one graph


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def slots_of(nmax):
    return 1 if nmax <= 64 else 2 if nmax <= 128 else 4


def bwd_cap(nmax):
    """The largest k_cap the Gumbel backward's LDS history admits on rows of nmax slots, at most nmax + 2."""
    return min(nmax + 2, 4096 // (slots_of(nmax) * 64))


@functools.lru_cache(maxsize=None)
def case(nmax, B, k_cap, ties=False):
    """(sizes, k_rows, scores [N], noise [B, nmax], d_out [N]) on the CPU.  Row 0 has nmax nodes; k cycles through
    1, 2, 3, nmax, k_cap (clipped to k_cap, at most 5 distinct values), so neighbours in a workgroup differ."""
    g = torch.Generator().manual_seed(1000 * nmax + 10 * B + k_cap + ties)
    ks = [min(k, k_cap) for k in (1, 2, 3, nmax, k_cap)]
    k_rows = [ks[(b + (1 if B == 1 else 0)) % len(ks)] for b in range(B)]
    sizes = []
    for b, k in enumerate(k_rows):
        opts = (nmax, 1, k, k + 1)
        sizes.append(nmax if b == 0 else max(1, min(opts[(b + b // 4) % 4], nmax)))
    N = sum(sizes)
    scores = torch.randint(-1, 2, (N,), generator=g).float() if ties else torch.nn.functional.gelu(torch.randn(N, generator=g))
    u = torch.rand(B, nmax, generator=g).clamp(1e-6, 1 - 1e-6)
    return tuple(sizes), tuple(k_rows), scores, -torch.log(-torch.log(u)), torch.randn(N, generator=g)


def on_device(c, dev):
    from isubgvqa_amd import ops
    sizes, k_rows, scores, noise, d_out = c
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    plan = ops.GraphPlan.build(batch, None, num_graphs=len(sizes))
    assert plan.nmax == max(sizes)
    return plan, batch, torch.tensor(k_rows, dtype=torch.int32, device=dev), scores.to(dev), noise.to(dev), d_out.to(dev)


def rows_of(per_k, k_rows, batch=None):
    """The reference: from the scalar call at k = k_rows[b], the rows of graph b.  per_k: {k: tensor}; ragged [N] with `batch`,
    else [B, nmax]."""
    k_t = torch.tensor(k_rows, device=next(iter(per_k.values())).device)
    row_k = k_t if batch is None else k_t[batch]
    out = torch.empty_like(next(iter(per_k.values())))
    for k, v in per_k.items():
        sel = row_k == k
        out[sel] = v[sel]
    return out


def dense_of(scores, sizes, nmax):
    d = torch.zeros(len(sizes), nmax, device=scores.device)
    at = 0
    for b, n in enumerate(sizes):
        d[b, :n] = scores[at:at + n]
        at += n
    return d


def same(got, ref, what):
    """Bit for bit (floats compared as their words: a NaN equals the same NaN)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    a, b = got.contiguous(), ref.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {got.numel()} values differ, max |d| {(got - ref).abs().max().item():.3e}"


# ---- the planning kernel ----------------------------------------------------------------------------------------------------
def test_budget_equals_the_torch_rule(dev):
    from isubgvqa_amd import ops
    import topk_rows_restated as R
    from test_topk_rows_cpu import CEILINGS, NODE_COUNTS
    sizes = list(NODE_COUNTS) + [2, 3, 4, 13, 14, 27, 100, 199] * 40            # 329 graphs: two blocks of the kernel
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    plan = ops.GraphPlan.build(batch, None, num_graphs=len(sizes))
    for ratio, want in CEILINGS.items():
        for k_min, k_cap in ((1, 5), (2, 12), (1, 64), (3, 3)):
            got = ops.topk_budget(plan, ratio, k_min, k_cap)
            assert got.dtype == torch.int32 and got.shape == (len(sizes),) and got.device == batch.device
            assert got[:len(want)].tolist() == [min(k_cap, max(k_min, c)) for c in want]
            same(got.cpu(), R.budget(torch.tensor(sizes), ratio, k_min, k_cap), f"budget {ratio} {k_min} {k_cap}")
            assert ops.topk_budget(plan, ratio, k_min, k_cap) is got, "one tensor per plan and arguments"
    same(ops.topk_budget(plan, 1.0, 1, 1000).cpu(), torch.tensor(sizes, dtype=torch.int32), "ratio 1")
    same(ops.topk_budget(plan, 3e38, 1, 7).cpu(), torch.full((len(sizes),), 7, dtype=torch.int32), "a product beyond the int range")


# ---- the threshold solve -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nmax", NMAXES)
def test_threshold_rows_equal_the_scalar_rows(dev, nmax, B):
    from isubgvqa_amd import ops
    k_cap = nmax + 2
    for ties in (False, True):
        c = case(nmax, B, k_cap, ties)
        sizes, k_rows = c[0], c[1]
        plan, batch, k_t, scores, noise, _ = on_device(c, dev)
        dense = dense_of(scores, sizes, nmax)
        distinct = sorted(set(k_rows))
        assert len(distinct) <= 6
        ops.reset_counters()
        variants = {"plain": {}, "noise": dict(noise=noise, noise_scale=0.37), "seeded": dict(noise_scale=1.0, seed=2 ** 32 + 7)}
        for name, kw in variants.items():
            got, got_d = ops.topk_threshold(scores, k_t, plan=plan, k_cap=k_cap, return_dense=True, **kw)
            ref = {k: ops.topk_threshold(scores, k, plan=plan, return_dense=True, **kw) for k in distinct}
            same(got, rows_of({k: v[0] for k, v in ref.items()}, k_rows, batch), f"threshold {name} ragged, ties={ties}")
            same(got_d, rows_of({k: v[1] for k, v in ref.items()}, k_rows), f"threshold {name} dense_out, ties={ties}")
            same(ops.topk_threshold(scores, k_t, plan=plan, k_cap=k_cap, **kw), got, "two calls")
            got2 = ops.topk_threshold(dense, k_t, k_cap=k_cap, **kw)                         # the dense layout
            same(got2, rows_of({k: ops.topk_threshold(dense, k, **kw) for k in distinct}, k_rows), f"threshold {name} dense")
            if name == "plain":
                for b, k in enumerate(k_rows):                                               # the rule itself, once: pads included
                    row = got_d[b]
                    assert row.sum().item() >= min(k, nmax) and (k < nmax or bool(row.all())), (b, k)
        assert ops.counters()["topk_rows"] == 3 * 3
        if B > 1:                                                                            # a sub-batch keeps its graphs' streams
            plan.graph_ids = torch.arange(B, dtype=torch.int32, device=dev) * 3 + 2
            kw = dict(noise_scale=1.0, seed=11)
            got = ops.topk_threshold(scores, k_t, plan=plan, k_cap=k_cap, **kw)
            same(got, rows_of({k: ops.topk_threshold(scores, k, plan=plan, **kw) for k in distinct}, k_rows, batch), "graph_ids")
            plan.graph_ids = None


# ---- the relaxation and its backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nmax", NMAXES)
def test_gumbel_rows_equal_the_scalar_rows(dev, nmax, B):
    from isubgvqa_amd import ops
    k_cap = nmax + 2
    c = case(nmax, B, k_cap)
    sizes, k_rows = c[0], c[1]
    plan, batch, k_t, scores, noise, _ = on_device(c, dev)
    distinct = sorted(set(k_rows))
    for name, kw in {"noise": dict(noise=noise), "seeded": dict(seed=5)}.items():
        got, khot = ops.topk_gumbel(scores, k_t, TAU, plan=plan, k_cap=k_cap, return_khot=True, **kw)
        ref = {k: ops.topk_gumbel(scores, k, TAU, plan=plan, return_khot=True, **kw) for k in distinct}
        same(got, rows_of({k: v[0] for k, v in ref.items()}, k_rows, batch), f"gumbel {name} ragged")
        same(khot, rows_of({k: v[1] for k, v in ref.items()}, k_rows), f"gumbel {name} khot_out")
        same(ops.topk_gumbel(scores, k_t, TAU, plan=plan, k_cap=k_cap, **kw), got, "two calls")
    dense = dense_of(scores, sizes, nmax)
    got = ops.topk_gumbel(dense, k_t, TAU, noise=noise, k_cap=k_cap)
    same(got, rows_of({k: ops.topk_gumbel(dense, k, TAU, noise=noise) for k in distinct}, k_rows), "gumbel dense")
    for b, k in enumerate(k_rows):
        assert int((got[b] > 0.5).sum()) == min(k, nmax), (b, k)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nmax", NMAXES)
def test_gumbel_rows_backward_equals_the_scalar_rows(dev, nmax, B):
    from isubgvqa_amd import ops
    k_cap = bwd_cap(nmax)
    c = case(nmax, B, k_cap)
    sizes, k_rows = c[0], c[1]
    plan, batch, k_t, scores, noise, d_out = on_device(c, dev)
    distinct = sorted(set(k_rows))
    for name, kw in {"noise": dict(noise=noise), "seeded": dict(seed=5)}.items():
        got = ops.topk_gumbel_backward(scores, d_out, k_t, TAU, plan=plan, k_cap=k_cap, **kw)
        ref = {k: ops.topk_gumbel_backward(scores, d_out, k, TAU, plan=plan, **kw) for k in distinct}
        same(got, rows_of(ref, k_rows, batch), f"gumbel backward {name} ragged")
        same(ops.topk_gumbel_backward(scores, d_out, k_t, TAU, plan=plan, k_cap=k_cap, **kw), got, "two calls")
        assert nmax == 1 or bool(got.any())
    dense, dd = dense_of(scores, sizes, nmax), dense_of(d_out, sizes, nmax)
    got = ops.topk_gumbel_backward(dense, dd, k_t, TAU, noise=noise, k_cap=k_cap)
    same(got, rows_of({k: ops.topk_gumbel_backward(dense, dd, k, TAU, noise=noise) for k in distinct}, k_rows), "gumbel backward dense")


def test_gumbel_rows_backward_refuses_a_cap_beyond_the_lds_history(dev):
    """k_cap * slots * 64 > 4096 is refused whatever the rows hold (here all 1): nmax = 65 is SLOTS 2, so k_cap = 33 is one too many."""
    from isubgvqa_amd import _lib, _lib_topk_rows, ops
    c = case(65, 5, 5)
    plan, batch, _, scores, noise, d_out = on_device(c, dev)
    ones = torch.ones(5, dtype=torch.int32, device=dev)
    out = torch.full_like(scores, SENTINEL)
    args = lambda cap: (scores.data_ptr(), plan.ptr.data_ptr(), 5, 65, 0, noise.data_ptr(), 0, 0, ones.data_ptr(), cap, TAU,
                        d_out.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert _lib_topk_rows.load().isg_topk_gumbel_rows_bwd(*args(33)) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote"
    with pytest.raises(_lib.IsgError):
        ops.topk_gumbel_backward(scores, d_out, ones, TAU, plan=plan, noise=noise, k_cap=33)
    same(ops.topk_gumbel_backward(scores, d_out, ones, TAU, plan=plan, noise=noise, k_cap=32),
         ops.topk_gumbel_backward(scores, d_out, 1, TAU, plan=plan, noise=noise), "k_cap = 32 is admitted")


# ---- autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmax,B", [(33, 9), (65, 5)])
def test_estimators_with_a_k_per_row_give_the_scalar_rows_gradients(dev, nmax, B):
    from isubgvqa_amd import autograd
    k_cap = bwd_cap(nmax)
    c = case(nmax, B, k_cap)
    k_rows = c[1]
    plan, batch, k_t, scores, noise, d_out = on_device(c, dev)
    noise3 = noise * 0.3
    distinct = sorted(set(k_rows))

    def grad(fn):
        s = scores.clone().requires_grad_(True)
        out = fn(s)
        (out * d_out).sum().backward()
        return out.detach(), s.grad

    calls = {
        "gumbel": lambda s, k, cap: autograd.topk_gumbel(s, k, TAU, plan, noise, 0, cap),
        "imle": lambda s, k, cap: autograd.imle_topk(s, k, plan, noise3, 0, 1.0, 10.0, 1.0, 1.0, cap),
        "aimle": lambda s, k, cap: autograd.aimle_topk(s, k, plan, noise3, 0, autograd.AdaptiveTarget(initial_beta=1.0), 1.0, 1.0, cap),
    }
    for name, call in calls.items():
        out, g = grad(lambda s: call(s, k_t, k_cap))
        ref = {k: grad(lambda s: call(s, k, None)) for k in distinct}
        same(out, rows_of({k: v[0] for k, v in ref.items()}, k_rows, batch), f"{name} forward")
        # (AIMLE's perturbation size is a norm over the whole batch's scores and d out: the same in every call, so rows compare)
        same(g, rows_of({k: v[1] for k, v in ref.items()}, k_rows, batch), f"{name} d scores")


# ---- guard words, determinism, the strict twin -------------------------------------------------------------------------------------
def _raw_calls(lib, c, dev, k_cap):
    """The three entry points called on buffers of this test's own, GUARD sentinel words behind each; returns what they wrote."""
    plan, batch, k_t, scores, noise, d_out = on_device(c, dev)
    B, nmax, N = plan.B, plan.nmax, scores.numel()
    k_buf = torch.full((B + GUARD,), 7777, dtype=torch.int32, device=dev)
    k_buf[:B] = k_t
    bufs = {n: torch.full((size + GUARD,), SENTINEL, device=dev) for n, size in
            (("thr", N), ("thr_dense", B * nmax), ("gum", N), ("khot", B * nmax), ("bwd", N))}
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    assert lib.isg_topk_threshold_rows(p(scores), p(plan.ptr), B, nmax, p(plan.nmax_dev), p(noise), 0.37, 0, 0, p(k_buf), k_cap,
                                       p(bufs["thr"]), p(bufs["thr_dense"]), st) == 0
    assert lib.isg_topk_gumbel_rows(p(scores), p(plan.ptr), B, nmax, p(plan.nmax_dev), p(noise), 0, 0, p(k_buf), k_cap, TAU,
                                    p(bufs["gum"]), p(bufs["khot"]), st) == 0
    assert lib.isg_topk_gumbel_rows_bwd(p(scores), p(plan.ptr), B, nmax, p(plan.nmax_dev), p(noise), 0, 0, p(k_buf), k_cap, TAU,
                                        p(d_out), p(bufs["bwd"]), st) == 0
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert bool((t[-GUARD:] == SENTINEL).all()), f"{n}: written behind its end"
        assert not bool((t[:-GUARD] == SENTINEL).any()), f"{n}: an entry was not written"
    assert bool((k_buf[B:] == 7777).all()) and torch.equal(k_buf[:B], k_t), "k_rows was written"
    return {n: t[:-GUARD].clone() for n, t in bufs.items()}


@pytest.mark.parametrize("nmax,B", [(33, 5), (65, 9), (130, 5)])
def test_guard_words_two_calls_and_the_strict_twin(dev, nmax, B):
    from isubgvqa_amd import _lib, _lib_topk_rows, ops
    k_cap = bwd_cap(nmax)
    c = case(nmax, B, k_cap)
    fast = _lib_topk_rows.load()
    first = _raw_calls(fast, c, dev, k_cap)
    again = _raw_calls(fast, c, dev, k_cap)
    assert os.path.exists(STRICT), "csrc/libisg_hip_strict.so is missing: __graft_entry__.build() makes it beside the library"
    strict = _lib.bind(ctypes.CDLL(STRICT), _lib_topk_rows.SIGNATURES)
    assert strict.isg_topk_rows_abi_version() == _lib_topk_rows.ABI_VERSION
    twin = _raw_calls(strict, c, dev, k_cap)
    for n in first:
        same(again[n], first[n], f"{n}: two calls")
        same(twin[n], first[n], f"{n}: the strict twin")
    # and they are what the wrappers return
    plan, batch, k_t, scores, noise, d_out = on_device(c, dev)
    same(first["thr"], ops.topk_threshold(scores, k_t, plan=plan, noise=noise, noise_scale=0.37, k_cap=k_cap), "wrapper")
    same(first["bwd"], ops.topk_gumbel_backward(scores, d_out, k_t, TAU, plan=plan, noise=noise, k_cap=k_cap), "wrapper, backward")


def test_a_bad_entry_is_clamped_to_the_cap(dev):
    """Entries outside [1, k_cap] are the caller's error; the kernels clamp them to [0, k_cap] so that no loop runs past the cap
    and the backward's LDS history is never indexed beyond its k_cap rounds."""
    from isubgvqa_amd import ops
    c = case(33, 5, 4)
    plan, batch, _, scores, noise, d_out = on_device(c, dev)
    big = torch.tensor([1000, 4, 2 ** 31 - 1, 5, 4], dtype=torch.int32, device=dev)
    at_cap = torch.full((5,), 4, dtype=torch.int32, device=dev)
    same(ops.topk_threshold(scores, big, plan=plan, k_cap=4), ops.topk_threshold(scores, at_cap, plan=plan, k_cap=4), "threshold")
    same(ops.topk_gumbel(scores, big, TAU, plan=plan, noise=noise, k_cap=4), ops.topk_gumbel(scores, 4, TAU, plan=plan, noise=noise), "gumbel")
    same(ops.topk_gumbel_backward(scores, d_out, big, TAU, plan=plan, noise=noise, k_cap=4),
         ops.topk_gumbel_backward(scores, d_out, 4, TAU, plan=plan, noise=noise), "gumbel backward")
    neg = torch.tensor([-3, 0, -2 ** 31, 0, -1], dtype=torch.int32, device=dev)
    g = ops.topk_gumbel_backward(scores, d_out, neg, TAU, plan=plan, noise=noise, k_cap=4)
    assert not bool(g.any()), "k = 0: no round, no gradient"
    assert not bool(ops.topk_gumbel(scores, neg, TAU, plan=plan, noise=noise, k_cap=4).any())


# ---- the model ---------------------------------------------------------------------------------------------------------------------
MASKS = (1.0, 0.15, 0.15)          # two masked layers
MIXED = (3, 7, 13, 14, 20, 21, 27, 33, 34, 40, 47, 60)        # ceil(0.15 n) = 1 2 2 3 3 4 5 5 6 6 8 9, capped at 6: six distinct k


def _workload(sizes, dev, seed=5):
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=len(sizes), channels=128, layers=3, masks=MASKS, sampler="imle", sample_k=5,
                                   sizes=tuple(sizes), seed=seed)
    wl = synthetic.make_workload(cfg)
    assert wl.max_nodes <= 64 and wl.max_edges <= 256
    return cfg, wl.to(dev)


@functools.lru_cache(maxsize=None)
def _weights():
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=12, channels=128, layers=3, masks=MASKS, sampler="imle", sample_k=5)
    return {k: v.clone() for k, v in synthetic.build_answer_model(cfg).state_dict().items()}


def _model(dev, sampler, sample_k, **budget):
    from isubgvqa_amd import synthetic
    m = synthetic.AnswerModel(128, 3, MASKS, sampler, sample_k, **budget)
    m.load_state_dict(_weights())
    return m.to(dev).eval()


def test_model_equal_sizes_equal_the_scalar_model_bit_for_bit(dev):
    """(a) every graph has n = 20 nodes: sample_ratio = 0.15 is k = ceil(0.15 * 20) = 3 for every graph."""
    _, wl = _workload((20,) * 12, dev)
    with torch.no_grad():
        for sampler, kw in (("gumbel", dict(seed=3)), ("imle", {}), ("aimle", dict(seed=3))):
            ref = _model(dev, sampler, 3)(wl, **kw)
            got = _model(dev, sampler, 5, sample_ratio=0.15)(wl, **kw)
            for a, b, what in zip(got, ref, ("logits", "mask", "gate")):
                same(a, b, f"{sampler} {what}")
            assert not torch.equal(got[1], _model(dev, sampler, 5)(wl, **kw)[1]), "the budget is not read: the mask is k = 5's"


def test_model_ratio_one_equals_the_scalar_model_bit_for_bit(dev):
    """(b) every graph has at least sample_k nodes and the ratio is 1.0: every budget is the cap."""
    sizes = (5, 6, 9, 12, 17, 20, 24, 31, 38, 40, 52, 64)
    _, wl = _workload(sizes, dev)
    with torch.no_grad():
        for sampler, kw in (("imle", {}), ("gumbel", dict(seed=9))):
            ref = _model(dev, sampler, 5)(wl, **kw)
            got = _model(dev, sampler, 5, sample_ratio=1.0)(wl, **kw)
            for a, b, what in zip(got, ref, ("logits", "mask", "gate")):
                same(a, b, f"{sampler} {what}")


def test_model_mixed_sizes_mask_exact_and_logits_per_graph(dev):
    """(c) sizes 3-60, ratio 0.15, cap 6.  The first masked layer's mask is ops.topk_threshold(gate, k_rows) exactly; the logits of
    graph g agree with the scalar model at k = k_g within the 1e-4 logit bound.  Measured on the MI355X: max |logit diff| 0.0 for
    every k = 1 ... 6 (the test prints the figure per k)."""
    from isubgvqa_amd import ops
    import topk_rows_restated as R
    _, wl = _workload(MIXED, dev)
    plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=12, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
    k_rows = ops.topk_budget(plan, 0.15, 1, 6)
    want = R.budget(torch.tensor(MIXED), 0.15, 1, 6)
    same(k_rows.cpu(), want, "budget")
    assert sorted(set(want.tolist())) == [1, 2, 3, 4, 5, 6]
    model = _model(dev, "imle", 6, sample_ratio=0.15)
    layer = model.gat_seq.convs[1].mask                       # the first masked layer
    seen = {}
    inner = layer.gate_scores
    layer.gate_scores = lambda *a, **kw: seen.setdefault("gate", inner(*a, **kw))
    hook = layer.register_forward_hook(lambda mod, args, out: seen.setdefault("mask", out))
    ops.reset_counters()
    with torch.no_grad():
        logits, mask, _ = model(wl, plan=plan)
        hook.remove()
        del layer.gate_scores
        assert ops.counters()["topk_rows"] == 2, "one per masked layer"
        same(seen["mask"], ops.topk_threshold(seen["gate"], k_rows, plan=plan, k_cap=6), "the first masked layer's mask")
        worst = 0.0
        for k in sorted(set(want.tolist())):
            ref_logits = _model(dev, "imle", k)(wl)[0]
            sel = (want == k).to(dev)
            d = (logits[sel] - ref_logits[sel]).abs().max().item()
            print(f"[topk rows model] graphs with k = {k}: max |logit diff| {d:.3e}")
            worst = max(worst, d)
        assert worst <= LOGIT_BOUND, worst


def test_model_training_step_with_a_budget(dev):
    """(d) one training step with I-MLE and a budget: every parameter the scalar model's step reaches gets a finite gradient."""
    _, wl = _workload(MIXED, dev)
    target = torch.randint(0, 1842, (12,), generator=torch.Generator().manual_seed(1)).to(dev)
    reached = {}
    for name, budget in (("scalar", {}), ("budget", dict(sample_ratio=0.15, sample_k_min=2))):
        model = _model(dev, "imle", 6, **budget).train()
        logits, _, _ = model(wl, seed=7)
        loss = torch.nn.functional.cross_entropy(logits, target)
        assert torch.isfinite(loss)
        loss.backward()
        reached[name] = {n for n, p in model.named_parameters() if p.grad is not None}
        bad = [n for n, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
        assert not bad, bad
    assert reached["budget"] == reached["scalar"] and len(reached["budget"]) > 20


def test_captured_forward_with_a_budget_replays_to_the_eager_bits(dev):
    """ops.topk_budget reads nothing back, so a forward with a budget can be captured: capture and replay give the eager bits."""
    _, wl = _workload(MIXED, dev)
    model = _model(dev, "imle", 6, sample_ratio=0.15, sample_k_min=2)
    with torch.no_grad():
        eager = [t.clone() for t in model(wl)]
        captured = [t.clone() for t in model(wl, capture=True)]
        replayed = [t.clone() for t in model(wl, capture=True)]
        torch.cuda.synchronize()
    for a, b, c, what in zip(eager, captured, replayed, ("logits", "mask", "gate")):
        same(b, a, f"captured {what}")
        same(c, a, f"replayed {what}")
    assert model.__dict__["_step_capture"].replays >= 1
