"""The scene-graph encoder's backward kernels (include/isg_sgenc_train.h) on a real MI355X against the float64 restatements of
tests/sgenc_bwd_restated.py, and the encoder end to end under SPLIT_TRAIN against the float64 oracle.

Operator bound (the project's rule): max(4 x the max abs error of the same restatement in float32 on the CPU, one fp32
ulp of the largest expected value).  The measured errors go to parity_record."""
import argparse
import math

import pytest
import torch
import torch.nn.functional as F

import sgenc_bwd_restated as R
from conftest import parity_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def ulp32(v: float) -> float:
    return 0.0 if v == 0 else 2.0 ** (math.frexp(abs(v))[1] - 24)


def held(name, got, ref64, ref32, record):
    """|got - ref64| <= max(4 x |ref32 - ref64|, one fp32 ulp of max |ref64|); the figures are kept in `record`."""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.detach().double(), ref32.detach().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if ref64.numel() == 0:
        return
    err, e32 = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    bound = max(4.0 * e32, ulp32(float(ref64.abs().max())))
    record[name] = {"err": err, "cpu_fp32_err": e32, "bound": bound}
    print(f"    {name}: err {err:.3e}  cpu fp32 {e32:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e} (fp32 on the CPU: {e32:.3e})"


# ---- isg_segment_rows_sum -----------------------------------------------------------------------------------------------------
def skewed_csr(L, gen):
    """About 6 L entries: an empty first segment, L one-entry segments, a segment of exactly L entries on a piece boundary, one of
    L + 1, a filler that ends mid-piece, one that starts there and crosses three pieces, two empty ones, two short ones, a last
    segment that leaves the last piece partial, an empty last segment."""
    counts = [0] + [1] * L + [L, L + 1, 37, 2 * L + 50, 0, 0, 5, 1, 29, 0]
    M = sum(counts)
    rowptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
    assert int(rowptr[L + 1]) == L and int(rowptr[L + 2]) == 2 * L                       # the L-entry segment sits on a boundary
    crossing = L + 4
    a, b = int(rowptr[crossing]), int(rowptr[crossing + 1])
    assert a % L != 0 and (b - 1) // L - a // L >= 2 and M % L != 0 and 5 * L < M < 6 * L
    perm = torch.randperm(M, generator=gen)
    eid = torch.cat([perm[int(rowptr[s]):int(rowptr[s + 1])].sort().values for s in range(len(counts))])
    return rowptr.to(torch.int32), eid.to(torch.int32), M, crossing


@pytest.mark.parametrize("gdiv", [1, 4])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [4, 300])
def test_segment_rows_sum(dev, C, weighted, gdiv):
    from isubgvqa_amd import ops
    L = ops.segment_rows_chunk()
    gen = torch.Generator().manual_seed(100 * C + 10 * gdiv + weighted)
    rowptr, eid, M, crossing = skewed_csr(L, gen)
    S = rowptr.numel() - 1
    G = torch.randn((M + gdiv - 1) // gdiv, C, generator=gen)
    w = torch.randn(M, generator=gen) if weighted else None
    rp, ed, Gd, wd = rowptr.to(dev), eid.to(dev), G.to(dev), None if w is None else w.to(dev)
    rec = {}
    ref64 = R.segment_rows_sum(rowptr, eid, G, w, gdiv)
    ref32 = R.segment_rows_sum(rowptr, eid, G, w, gdiv, dtype=torch.float32)
    out = ops.segment_rows_sum(rp, ed, Gd, w=wd, gdiv=gdiv)
    held("plain", out, ref64, ref32, rec)
    assert torch.equal(out[0], torch.zeros(C, device=dev)) and torch.equal(out[-1], torch.zeros(C, device=dev))
    assert torch.equal(out, ops.segment_rows_sum(rp, ed, Gd, w=wd, gdiv=gdiv)), "two identical calls differ"
    # skip on a non-empty segment: that row is all zeros, the others keep their bits
    for skip in (crossing, L + 1, 3):
        sk = ops.segment_rows_sum(rp, ed, Gd, w=wd, gdiv=gdiv, skip=skip)
        assert float(out[skip].abs().max()) > 0 and torch.equal(sk[skip], torch.zeros(C, device=dev))
        keep = torch.arange(S, device=dev) != skip
        assert torch.equal(sk[keep], out[keep])
    # out as a column slice of a wider tensor: the neighbour columns stay as they were
    wide = torch.full((S, 3 * C), 7.25, device=dev)
    ops.segment_rows_sum(rp, ed, Gd, w=wd, gdiv=gdiv, out=wide[:, C:2 * C])
    assert torch.equal(wide[:, C:2 * C], out)
    assert bool((wide[:, :C] == 7.25).all()) and bool((wide[:, 2 * C:] == 7.25).all())
    parity_record(f"sgenc_segment_rows_sum_C{C}_w{int(weighted)}_gdiv{gdiv}", rec)


def test_segment_rows_sum_without_entries(dev):
    from isubgvqa_amd import ops
    rowptr = torch.zeros(6, dtype=torch.int32, device=dev)
    out = torch.full((5, 8), 3.0, device=dev)
    ops.segment_rows_sum(rowptr, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 8, device=dev), out=out)
    assert torch.equal(out, torch.zeros(5, 8, device=dev))
    with pytest.raises(Exception):
        ops.segment_rows_sum(rowptr, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 6, device=dev))     # 4 | C


# ---- isg_gather_add_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["edge", "node", "plain"])
@pytest.mark.parametrize("C", [4, 300])
def test_gather_add_backward(dev, C, form):
    """The encoder's two forms (A + B + sign T + bias, GELU; A + D + bias, GELU) with A and B column slices of one [N, 3C] tensor,
    and A alone without activation; gradients of A, B, T, D and bias against float64 autograd of the restatement."""
    from isubgvqa_amd import ops
    L = ops.segment_rows_chunk()
    N, E, V = 37, 3 * L + 7, 11
    gen = torch.Generator().manual_seed(C + len(form))
    ia, ib = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    it = torch.randint(0, V - 1, (E,), generator=gen)
    it[it == 3] = 4                                                     # token 3 (and V - 1) unused
    it[torch.randperm(E, generator=gen)[:int(0.6 * E)]] = 5             # one token owns 60 % of the edges
    sign = torch.where(torch.rand(E, generator=gen) < 0.3, -1.0, 1.0)
    leaves = {"P": torch.randn(N, 3 * C, generator=gen), "T": torch.randn(V, C, generator=gen), "D": torch.randn(E, C, generator=gen),
              "bias": torch.randn(C, generator=gen), "A": torch.randn(N, C, generator=gen)}
    wgt = torch.randn(E, C, generator=gen)

    def run(fn, dtype, device):
        t = {k: v.to(device=device, dtype=dtype).detach().clone().requires_grad_(True) for k, v in leaves.items()}
        i = lambda v: v.to(device)
        if form == "edge":
            out = fn(t["P"][:, :C], i(ia), t["P"][:, C:2 * C], i(ib), t["T"], i(it), i(sign).to(dtype), bias=t["bias"], gelu=True)
            used = ("P", "T", "bias")
        elif form == "node":
            out = fn(t["P"][:, 2 * C:], i(ia), D=t["D"], bias=t["bias"], gelu=True)
            used = ("P", "D", "bias")
        else:
            out = fn(t["A"], i(ia))
            used = ("A",)
        (out * wgt.to(device=device, dtype=dtype)).sum().backward()
        return out.detach(), {k: t[k].grad for k in used}

    o64, g64 = run(R.gather_add, torch.float64, "cpu")
    o32, g32 = run(R.gather_add, torch.float32, "cpu")
    out, got = run(ops.gather_add, torch.float32, dev)
    rec = {}
    held("out", out, o64, o32, rec)
    for k in g64:
        assert got[k] is not None, k
        held("d_" + k, got[k], g64[k], g32[k], rec)
    if form == "edge":
        assert torch.equal(got["T"][3], torch.zeros(C, device=dev)) and torch.equal(got["P"][:, 2 * C:], torch.zeros(N, C, device=dev))
    parity_record(f"sgenc_gather_add_bwd_{form}_C{C}", rec)


def test_gather_add_refuses_planes_under_autograd(dev):
    from isubgvqa_amd import ops
    A = torch.randn(5, 8, device=dev, requires_grad=True)
    ia = torch.tensor([0, 4, 2], device=dev)
    out = ops.gather_add(A, ia)
    assert out.grad_fn is not None, "a recording operand must not be detached silently"
    with pytest.raises(NotImplementedError):
        ops.gather_add(A, ia, planes_out=True)
    with torch.no_grad():
        assert ops.gather_add(A, ia, planes_out=True).rows == 3


# ---- isg_scatter_mean_bwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 300])
def test_scatter_mean_backward(dev, C):
    from isubgvqa_amd import ops
    L = ops.segment_rows_chunk()
    gen = torch.Generator().manual_seed(C)
    N = 23
    dst = torch.cat([torch.full((2 * L,), 4), torch.randint(0, N - 1, (40,), generator=gen)])       # node 4 receives 2 L edges ...
    dst[dst == 9] = 10                                                                                 # ... node 9 and N - 1 none
    dst = dst[torch.randperm(dst.numel(), generator=gen)]
    E = dst.numel()
    ei = torch.stack([torch.randint(0, N, (E,), generator=gen), dst])
    msg, wgt = torch.randn(E, C, generator=gen), torch.randn(N, C, generator=gen)

    def ref(dtype):
        m = msg.to(dtype).detach().clone().requires_grad_(True)
        out = R.scatter_mean(m, dst, N)
        (out * wgt.to(dtype)).sum().backward()
        return out.detach(), m.grad

    o64, g64 = ref(torch.float64)
    o32, g32 = ref(torch.float32)
    plan = ops.GraphPlan.edges_only(ei.to(dev), N)
    m = msg.to(dev).requires_grad_(True)
    out = ops.scatter_mean(m, plan)
    (out * wgt.to(dev)).sum().backward()
    rec = {}
    held("out", out, o64, o32, rec)
    held("d_msg", m.grad, g64, g32, rec)
    assert torch.equal(out[9].detach(), torch.zeros(C, device=dev))
    parity_record(f"sgenc_scatter_mean_bwd_C{C}", rec)


# ---- isg_graph_norm_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("C", [8, 300])
def test_graph_norm_backward(dev, C, fp64):
    from isubgvqa_amd import autograd, ops
    sizes = [5, 1, 70, 17, 3, 0, 9]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    N, B = batch.numel(), len(sizes)
    gen = torch.Generator().manual_seed(C + fp64)
    leaves = {"x": torch.randn(N, C, generator=gen) * 2 + 0.5, "weight": torch.rand(C, generator=gen) + 0.5,
              "bias": torch.randn(C, generator=gen), "mean_scale": torch.rand(C, generator=gen) + 0.5}
    wgt = torch.randn(N, C, generator=gen)

    def ref(dtype, mode):
        t = {k: v.to(dtype).detach().clone().requires_grad_(True) for k, v in leaves.items()}
        out = autograd._graph_norm_t(t["x"], t["weight"], t["bias"], t["mean_scale"], batch, B, 1e-5, mode)
        (out * wgt.to(dtype)).sum().backward()
        return out.detach(), {k: v.grad for k, v in t.items()}

    o64, g64 = ref(torch.float64, False)
    o32, g32 = ref(torch.float32, fp64)
    t = {k: v.to(dev).detach().clone().requires_grad_(True) for k, v in leaves.items()}
    plan = ops.GraphPlan.build(batch.to(dev), num_graphs=B)
    out = ops.graph_norm(t["x"], plan, t["weight"], t["bias"], t["mean_scale"], 1e-5, fp64)
    (out * wgt.to(dev)).sum().backward()
    rec = {}
    held("out", out, o64, o32, rec)
    for k in g64:
        held("d_" + k, t[k].grad, g64[k], g32[k], rec)
    parity_record(f"sgenc_graph_norm_bwd_C{C}_{'fp64' if fp64 else 'fp32'}", rec)


# ---- the node tokens ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 300])
def test_embedding_sum_backward_leaves_the_pad_row_alone(dev, C):
    from isubgvqa_amd import ops
    N, T, V = 50, 4, 11
    gen = torch.Generator().manual_seed(C)
    idx = torch.randint(2, V, (N, T), generator=gen)
    idx[torch.rand(N, T, generator=gen) < 0.5] = R.PAD
    assert 0.35 < float((idx == R.PAD).float().mean()) < 0.65
    weight, wgt = torch.randn(V, C, generator=gen), torch.randn(N, C, generator=gen)

    def ref(dtype):
        w = weight.to(dtype).detach().clone().requires_grad_(True)
        out = F.embedding(idx, w, padding_idx=R.PAD).sum(-2)
        (out * wgt.to(dtype)).sum().backward()
        return out.detach(), w.grad

    o64, g64 = ref(torch.float64)
    o32, g32 = ref(torch.float32)
    w = weight.to(dev).requires_grad_(True)
    out = ops.embedding_sum(w, idx.to(dev), padding_idx=R.PAD)
    (out * wgt.to(dev)).sum().backward()
    rec = {}
    held("out", out, o64, o32, rec)
    held("d_weight", w.grad, g64, g32, rec)
    assert torch.equal(w.grad[R.PAD], torch.zeros(C, device=dev)) and torch.equal(w.grad[0], torch.zeros(C, device=dev))
    assert float(w.grad[2:].abs().min(dim=1).values.max()) > 0
    parity_record(f"sgenc_embedding_sum_bwd_C{C}", rec)


# ---- the encoder end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    enc, inputs = R.make_encoder(), R.make_batch()
    x_ref, e_ref, g_ref = R.oracle_grads(enc, inputs)
    return enc, inputs, x_ref, e_ref, g_ref


def _encoder_step(enc, inputs, dev):
    t = {k: v.to(dev) for k, v in inputs.items()}
    sg = argparse.Namespace(x_bbox=t["x_bbox"], added_sym_edge=t["added_sym_edge"])
    enc.zero_grad(set_to_none=True)
    x_enc, e_enc = enc(t["x"], edge_index=t["edge_index"], edge_attr=t["edge_attr"], batch=t["batch"], gt_scene_graphs=sg)
    wx, we = R.loss_weights(x_enc.size(0), e_enc.size(0), x_enc.size(1))
    ((x_enc * wx.float().to(dev)).sum() + (e_enc * we.float().to(dev)).sum()).backward()
    return x_enc.detach(), e_enc.detach(), {k: v.grad.detach().clone() for k, v in enc.named_parameters()}


def test_encoder_trains_without_its_concatenations(dev, oracle, monkeypatch):
    """train() mode, C = 300, SPLIT_TRAIN on: outputs and EVERY parameter gradient against the float64 oracle within 2e-3 of the
    tensor's largest entry (the project's bound for this comparison); the pad row without gradient; the counter; two runs of the
    whole step bit-equal.  The same batch with the switch off is recorded beside it (no ratio is set)."""
    import copy
    from isubgvqa_amd import ops
    from isubgvqa_amd.models import scene_graph_encoder as M
    enc0, inputs, x_ref, e_ref, g_ref = oracle
    enc = copy.deepcopy(enc0).train().to(dev)

    def rel(a, b):
        return float((a.detach().cpu().double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)

    errs = {}
    for on in (True, False):
        monkeypatch.setattr(M, "SPLIT_TRAIN", on)
        before = ops.COUNTERS["sgenc_train_kernels"]
        x_enc, e_enc, grads = _encoder_step(enc, inputs, dev)
        assert ops.COUNTERS["sgenc_train_kernels"] - before == (1 if on else 0)
        e = {"x_enc": rel(x_enc, x_ref), "e_enc": rel(e_enc, e_ref)}
        assert len(grads) == 28 == len(g_ref)
        for k, g in grads.items():
            assert g_ref[k] is not None and float(g_ref[k].abs().max()) > 1e-6, k
            e["d_" + k] = rel(g, g_ref[k])
        errs["split_train" if on else "concatenated"] = e
        worst = max(e, key=e.get)
        print(f"    SPLIT_TRAIN={on}: worst {worst} {e[worst]:.3e}")
        if on:
            first = grads
    parity_record("sgenc_encoder_train_vs_fp64_oracle", errs)
    for k, v in errs["split_train"].items():
        assert v < 2e-3, f"{k}: {v:.3e}"
    pad = first["sg_vocab_embedding.weight"][R.PAD]
    assert torch.equal(pad, torch.zeros_like(pad))
    monkeypatch.setattr(M, "SPLIT_TRAIN", True)
    _, _, again = _encoder_step(enc, inputs, dev)
    for k in first:
        assert torch.equal(first[k], again[k]), f"{k}: two runs of the same step differ"
