"""Training through shared scene encodings on the GPU (include/ext/isg_instances_train.h): isg_instance_rows_bwd
against a host loop over the copies as BITS, autograd.instance_rows against index_select under autograd in float64, the encoder
with a multiplicity against the float64 oracle on the physically replicated batch, ISubGVQA.forward_shared in train() against
forward() on the replicated batch, and the behaviour around it (eval bits, determinism, train_step, the counter)."""
import argparse
import copy
import ctypes

import pytest
import torch

import instances_restated as IR
import sgenc_bwd_restated as SR
from conftest import parity_record
from test_gpu_instances import CASES, G_MODEL, Q_MODEL, WL_SEED, _same_bits, _workload, index_of, make_graphs, spec_of
from test_gpu_models import LOGIT_TOL

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7.25
MIN_GAP = 1e-4
K = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """(fast, strict): the product library and its strict twin, the extension header bound on both."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_instances_train as X
    from isubgvqa_amd import _lib
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB), X.SIGNATURES)
    assert strict.isg_instances_train_abi_version() == X.ABI_VERSION
    return X.load(), strict


# ---------------------------------------------------------------------------------------------------------------------
# (a) the kernel
# ---------------------------------------------------------------------------------------------------------------------
def host_bwd(g, rng, iptr, gptr, glist, rows_in, Q):
    """isg_instance_rows_bwd restated as a loop on the host, fp32: per graph, its instances in the order of glist; the first copy
    of a row is taken as it is, every further one is added with one rounding.  The same rule for what is skipped as the header's:
    a graph's range in glist clamped to [0, Q], an instance outside [0, Q), a negative or short instance range, a copy's row
    outside [0, rows_in)."""
    G = rng.numel() - 1
    out = torch.zeros(int(rng[-1]), g.size(1), dtype=torch.float32)
    have = torch.zeros(int(rng[-1]), dtype=torch.bool)
    for gr in range(G):
        r0, r1 = int(rng[gr]), int(rng[gr + 1])
        j0 = max(0, min(int(gptr[gr]), Q))
        j1 = max(j0, min(int(gptr[gr + 1]), Q))
        for j in range(j0, j1):
            q = int(glist[j])
            if not 0 <= q < Q:
                continue
            b, e = int(iptr[q]), int(iptr[q + 1])
            if b < 0:
                continue
            n = max(0, min(r1 - r0, e - b, rows_in - b))
            if n == 0:
                continue
            tgt, src = slice(r0, r0 + n), slice(b, b + n)
            out[tgt] = torch.where(have[tgt].unsqueeze(1), out[tgt] + g[src], g[src])
            have[tgt] = True
    return out


def raw_bwd(lib, dev, gx, ge, N, E, C, ptr, erange, iptr, ieptr, gptr, glist, G, Q, xo_rows=None, eo_rows=None):
    """One call through the C ABI: the gradients are column slices of wider tensors, the outputs column slices of wider buffers
    filled with a sentinel and followed by GUARD sentinel words -> (d_x, d_e) on the host.  Asserts that the launch wrote nothing
    but the N x C and E x C words of the two slices."""
    pad = lambda n: torch.full((n * (C + 8) + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    bx, be = pad(N), pad(E)
    rc = lib.isg_instance_rows_bwd(gx.data_ptr(), gx.stride(0), gx.size(0) if xo_rows is None else xo_rows, bx.data_ptr() + 16, C + 8, N, C,
                                   ge.data_ptr(), ge.stride(0), ge.size(0) if eo_rows is None else eo_rows, be.data_ptr() + 16, C + 8, E, C,
                                   ptr.data_ptr(), erange.data_ptr(), iptr.data_ptr(), ieptr.data_ptr(), gptr.data_ptr(),
                                   glist.data_ptr(), G, Q, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    outs = []
    for buf, n in ((bx, N), (be, E)):
        assert bool((buf[n * (C + 8):] == SENTINEL).all()), "a guard word behind an output was written"
        wide = buf[:n * (C + 8)].view(n, C + 8).cpu()
        assert bool((wide[:, :4] == SENTINEL).all()) and bool((wide[:, 4 + C:] == SENTINEL).all()), "a neighbour column was written"
        outs.append(wide[:, 4:4 + C].contiguous())
    return outs


def _case(dev, G, Q, kind, C):
    """The expansion of tests/test_gpu_instances.py's graphs (a graph without nodes, one without edges, one never referenced, the
    longest chain one index 1 025 times) and gradient rows as column slices, with exact zeros of both signs among them."""
    from isubgvqa_amd import ops
    batch, ei = make_graphs(spec_of(G, seed=G, Q=Q), seed=100 + G)
    index = index_of(G, Q, kind, seed=Q)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=G)
    inst = ops.graph_instances(plan, ei.to(dev), index.to(dev))
    r = IR.expand(batch, ei, index, G)
    n, m = r.node_src.numel(), r.edge_src.numel()
    gen = torch.Generator().manual_seed(1000 * G + Q + C)
    wx, we = torch.randn(n, C + 12, generator=gen), torch.randn(m, C + 8, generator=gen)
    for t in (wx, we):
        if t.numel():
            t.view(-1)[::7] = 0.0
            t.view(-1)[3::11] = -0.0
    wx, we = wx.to(dev), we.to(dev)
    return argparse.Namespace(batch=batch, ei=ei, index=index, plan=plan, inst=inst, r=r, gx=wx[:, 8:8 + C], ge=we[:, 4:4 + C],
                              N=batch.numel(), E=ei.size(1), nptr=IR.graph_ptr(batch, G), erange=IR.edge_ranges(batch, ei, G)[0])


@pytest.mark.parametrize("C", [4, 128, 300])
@pytest.mark.parametrize("G,Q,kind", CASES, ids=[f"G{g}-Q{q}-{k}" for g, q, k in CASES])
def test_rows_backward_equals_the_host_loop_as_bits(dev, libs, G, Q, kind, C):
    """(a): G in {1, 3, 70} x Q in {1, 2, 65, 1 025} x C in {4, 128, 300}; every row of d_x and d_e equals the host loop over its
    copies in ascending q as BITS; twice on the fast library and once on the strict one with equal bits; ops.instance_rows_backward
    (contiguous outputs of its own) gives the same."""
    from isubgvqa_amd import ops
    c = _case(dev, G, Q, kind, C)
    inst = c.inst
    gptr, glist = inst.by_graph()
    assert torch.equal(inst.erange.cpu().long(), c.erange) and inst.counts().tolist() == torch.bincount(c.index, minlength=G).tolist()
    assert not c.gx.is_contiguous() or c.gx.size(0) <= 1
    want_x = host_bwd(c.gx.cpu(), c.nptr, c.r.ptr, gptr.cpu(), glist.cpu(), c.gx.size(0), Q)
    want_e = host_bwd(c.ge.cpu(), c.erange, c.r.eptr, gptr.cpu(), glist.cpu(), c.ge.size(0), Q)
    never = [g for g in range(G) if g not in set(c.index.tolist())]
    for g in never:                                             # rows of a graph no instance names: written, +0
        assert not want_x[c.nptr[g]:c.nptr[g + 1]].view(torch.int32).any()
    runs = [raw_bwd(lib, dev, c.gx, c.ge, c.N, c.E, C, c.plan.ptr, inst.erange, inst.ptr, inst.eptr, gptr, glist, G, Q)
            for lib in (libs[0], libs[0], libs[1])]
    for name, (dx, de) in zip(("the first run", "the second run", "the strict library"), runs):
        _same_bits(dx, want_x, f"{name}: d_x against the host loop")
        _same_bits(de, want_e, f"{name}: d_e against the host loop")
    ops.reset_counters()
    dx, de = ops.instance_rows_backward(inst, c.gx, c.ge)
    assert ops.counters()["instance_rows_bwd"] == 1 and dx.is_contiguous() and de.is_contiguous()
    _same_bits(dx.cpu(), want_x, "ops.instance_rows_backward: d_x")
    _same_bits(de.cpu(), want_e, "ops.instance_rows_backward: d_e")


def test_rows_backward_with_an_empty_half_and_without_instances(dev, libs):
    from isubgvqa_amd import ops
    batch, ei = make_graphs([(2, 0), (0, 0), (3, 0)], seed=1)
    plan = ops.GraphPlan.build(batch.to(dev), None, num_graphs=3)
    inst = ops.graph_instances(plan, ei.to(dev), torch.tensor([2, 0, 0, 1, 2]))
    gx = torch.randn(10, 8, generator=torch.Generator().manual_seed(2)).to(dev)
    dx, de = ops.instance_rows_backward(inst, gx, torch.zeros(0, 8, device=dev))
    want = torch.stack([gx[3] + gx[5], gx[4] + gx[6], gx[0] + gx[7], gx[1] + gx[8], gx[2] + gx[9]])
    assert torch.equal(dx, want) and tuple(de.shape) == (0, 8)
    none = ops.graph_instances(plan, ei.to(dev), torch.zeros(0, dtype=torch.int64))
    dx, de = ops.instance_rows_backward(none, torch.zeros(0, 8, device=dev), torch.zeros(0, 8, device=dev))
    assert tuple(dx.shape) == (5, 8) and not dx.view(torch.int32).any()
    with pytest.raises(ValueError):
        ops.instance_rows_backward(inst, gx[:-1], torch.zeros(0, 8, device=dev))


def test_bad_lists_and_short_ranges_are_skipped_and_write_nothing_else(dev, libs):
    """(a), bad inputs: corrupted glist entries, a graph's range in glist beyond [0, Q], an instance range that is negative or too
    short, fewer gradient rows than the ranges name -- every such copy is compared and skipped (the result is the host loop's
    under the same rule), the guard words stay (raw_bwd asserts them), nothing faults."""
    G, Q, C = 70, 65, 128
    c = _case(dev, G, Q, "repeats", C)
    inst = c.inst
    gptr, glist = (t.clone() for t in inst.by_graph())
    big = int(c.index.mode().values)                             # a graph with several instances
    j0, j1 = int(gptr[big]), int(gptr[big + 1])
    assert j1 - j0 >= 2
    bad_list = glist.clone()
    bad_list[j0], bad_list[j1 - 1], bad_list[0 if j0 else j1] = Q, -3, 1 << 20
    bad_gptr = gptr.clone()
    bad_gptr[G] = Q + 1000                                       # the last graph's range runs beyond the list
    bad_gptr[0] = -5
    short_ptr, short_eptr = inst.ptr.clone(), inst.eptr.clone()
    q = int(glist[j0 + 1])
    short_ptr[q + 1] -= 1                                        # instance q lost its last node row (and q + 1 begins earlier)
    short_eptr[q] = -2                                           # a negative range start
    variants = {"glist": (inst.ptr, inst.eptr, gptr, bad_list, None, None), "gptr": (inst.ptr, inst.eptr, bad_gptr, glist, None, None),
                "ranges": (short_ptr, short_eptr, gptr, glist, None, None),
                "rows": (inst.ptr, inst.eptr, gptr, glist, c.gx.size(0) // 2, c.ge.size(0) // 3)}
    good_x = host_bwd(c.gx.cpu(), c.nptr, c.r.ptr, gptr.cpu(), glist.cpu(), c.gx.size(0), Q)
    for name, (iptr, ieptr, gp, gl, xo_rows, eo_rows) in variants.items():
        nx, ne = c.gx.size(0) if xo_rows is None else xo_rows, c.ge.size(0) if eo_rows is None else eo_rows
        want_x = host_bwd(c.gx.cpu(), c.nptr, iptr.cpu(), gp.cpu(), gl.cpu(), nx, Q)
        want_e = host_bwd(c.ge.cpu(), c.erange, ieptr.cpu(), gp.cpu(), gl.cpu(), ne, Q)
        assert not torch.equal(want_x, good_x) or name == "gptr", name
        for lib in libs:
            dx, de = raw_bwd(lib, dev, c.gx, c.ge, c.N, c.E, C, c.plan.ptr, inst.erange, iptr, ieptr, gp, gl, G, Q, xo_rows, eo_rows)
            _same_bits(dx, want_x, f"{name}: d_x")
            _same_bits(de, want_e, f"{name}: d_e")


# ---------------------------------------------------------------------------------------------------------------------
# (b) autograd.instance_rows against index_select in float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,Q,kind", [(70, 65, "repeats"), (3, 1025, "repeats"), (70, 65, "same")])
def test_instance_rows_under_autograd_against_index_select_in_float64(dev, G, Q, kind):
    """(b): the fp32 gradient of a row with m copies lies within one rounding per added copy of the float64 sum: the error of a
    sum of m terms added one after the other is at most gamma(m - 1) = (m - 1) u / (1 - (m - 1) u) times the sum of the terms'
    magnitudes, u = 2^-24 -- computed here per element from the copy count, no constant."""
    from isubgvqa_amd import autograd, ops
    C = 300
    c = _case(dev, G, Q, kind, C)
    gen = torch.Generator().manual_seed(G + Q)
    x, e = torch.randn(c.N, C, generator=gen), torch.randn(c.E, C, generator=gen)
    wx, we = c.gx.contiguous(), c.ge.contiguous()
    xd, ed = x.to(dev).requires_grad_(True), e.to(dev).requires_grad_(True)
    ops.reset_counters()
    xo, eo = autograd.instance_rows(c.inst, xd, ed)
    assert torch.equal(xo, xd.detach()[c.inst.node_src]) and torch.equal(eo, ed.detach()[c.inst.edge_src])
    ((xo * wx).sum() + (eo * we).sum()).backward()
    assert ops.counters()["instance_rows_bwd"] == 1
    x64, e64 = x.double().requires_grad_(True), e.double().requires_grad_(True)
    ((x64.index_select(0, c.r.node_src) * wx.cpu().double()).sum() + (e64.index_select(0, c.r.edge_src) * we.cpu().double()).sum()).backward()
    counts = torch.bincount(c.index, minlength=G)
    u, rec = 2.0 ** -24, {}
    for name, got, ref, w, src, rows in (("d_x", xd.grad, x64.grad, wx, c.r.node_src, c.batch),
                                         ("d_e", ed.grad, e64.grad, we, c.r.edge_src, c.batch[c.ei[1]])):
        m = counts[rows].double().unsqueeze(1)                   # copies per distinct row
        mag = torch.zeros_like(ref).index_add_(0, src, w.cpu().double().abs())
        bound = (m - 1).clamp(min=0) * u / (1 - (m - 1).clamp(min=0) * u) * mag
        err = (got.cpu().double() - ref).abs()
        rec[name] = {"max_err": float(err.max()) if err.numel() else 0.0, "max_bound": float(bound.max()) if bound.numel() else 0.0,
                     "max_copies": int(m.max()) if m.numel() else 0}
        assert bool((err <= bound).all()), f"{name}: {float((err - bound).max()):.3e} beyond one rounding per added copy"
    parity_record(f"instance_rows_bwd_vs_fp64_G{G}_Q{Q}_{kind}", rec)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the encoder with a multiplicity against the float64 oracle on the replicated batch
# ---------------------------------------------------------------------------------------------------------------------
ENC_INDEX = [2, 0, 5, 2, 3, 0, 2, 1]        # six graphs: graph 2 three times, graph 0 twice, graph 4 never


def _grouped_batch():
    """sgenc_bwd_restated.make_batch() with added_sym_edge emptied (quirk Q6) and its shuffled edge list brought into graph
    order by a stable sort (the precondition of the expansion; within a graph the edges keep their order)."""
    inputs = SR.make_batch()
    order = torch.sort(inputs["batch"][inputs["edge_index"][1]], stable=True).indices
    inputs["edge_index"], inputs["edge_attr"] = inputs["edge_index"][:, order].contiguous(), inputs["edge_attr"][order].contiguous()
    inputs["added_sym_edge"] = inputs["added_sym_edge"][:0]
    return inputs


def test_encoder_with_a_multiplicity_against_the_fp64_oracle_on_the_replicated_batch(dev):
    """(c): train(), C = 300.  Reference: the float64 oracle's outputs and 28 parameter gradients on the batch with every asked
    graph physically copied out (instances_restated.expand), the loss weights on the replicated rows.  Ours: the encoder ONCE on
    the six distinct graphs with multiplicity = counts, autograd.instance_rows behind it.  Bound: 2e-3 of the tensor's largest
    entry, the bound tests/test_gpu_sgenc_train.py holds this oracle to.  The GPU encoder on the replicated batch is recorded
    beside it; no ratio is asserted."""
    from isubgvqa_amd import autograd, ops
    inputs, G, index = _grouped_batch(), len(SR.SIZES), torch.tensor(ENC_INDEX)
    r = IR.expand(inputs["batch"], inputs["edge_index"], index, G)
    assert r.status[2:].tolist() == [0, 0] and 4 not in ENC_INDEX
    rep = dict(x=inputs["x"][r.node_src], edge_index=r.edge_index, edge_attr=inputs["edge_attr"][r.edge_src], batch=r.batch,
               x_bbox=inputs["x_bbox"][r.node_src], added_sym_edge=inputs["added_sym_edge"])
    enc0 = SR.make_encoder()
    x_ref, e_ref, g_ref = SR.oracle_grads(enc0, rep)
    wx, we = SR.loss_weights(r.node_src.numel(), r.edge_src.numel(), 300)
    wx, we = wx.float().to(dev), we.float().to(dev)

    def rel(a, b):
        return float((a.detach().cpu().double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)

    def errors(x_enc, e_enc, enc):
        e = {"x_enc": rel(x_enc, x_ref), "e_enc": rel(e_enc, e_ref)}
        grads = {k: v.grad for k, v in enc.named_parameters()}
        assert len(grads) == 28 == len(g_ref)
        for k, g in grads.items():
            assert g is not None and g_ref[k] is not None and float(g_ref[k].abs().max()) > 1e-6, k
            e["d_" + k] = rel(g, g_ref[k])
        return e

    # ours: the distinct batch, weighted statistics, the expansion under autograd
    enc = copy.deepcopy(enc0).train().to(dev)
    t = {k: v.to(dev) for k, v in inputs.items()}
    plan = ops.GraphPlan.build(t["batch"], t["edge_index"], num_graphs=G)
    inst = ops.graph_instances(plan, t["edge_index"], index)
    inst.verify()
    sg = argparse.Namespace(x_bbox=t["x_bbox"], added_sym_edge=t["added_sym_edge"])
    x_enc, e_enc = enc(t["x"], edge_index=t["edge_index"], edge_attr=t["edge_attr"], batch=t["batch"], gt_scene_graphs=sg, plan=plan,
                       multiplicity=inst.counts())
    xo, eo = autograd.instance_rows(inst, x_enc, e_enc)
    ((xo * wx).sum() + (eo * we).sum()).backward()
    errs = {"shared": errors(xo, eo, enc)}
    # beside it: the GPU encoder on the physically replicated batch
    enc_r = copy.deepcopy(enc0).train().to(dev)
    tr = {k: v.to(dev) for k, v in rep.items()}
    sgr = argparse.Namespace(x_bbox=tr["x_bbox"], added_sym_edge=tr["added_sym_edge"])
    xr, er = enc_r(tr["x"], edge_index=tr["edge_index"], edge_attr=tr["edge_attr"], batch=tr["batch"], gt_scene_graphs=sgr)
    ((xr * wx).sum() + (er * we).sum()).backward()
    errs["replicated"] = errors(xr, er, enc_r)
    for name, e in errs.items():
        worst = max(e, key=e.get)
        print(f"    {name}: worst {worst} {e[worst]:.3e}")
    parity_record("instances_train_encoder_vs_fp64_oracle", errs)
    for k, v in errs["shared"].items():
        assert v < 2e-3, f"{k}: {v:.3e}"
    # the graph nobody asked takes no part: no gradient reaches its rows' tokens alone, and the running statistics are those of
    # the replicated batch
    for (k, a), (_, b) in zip(enc.named_buffers(), enc_r.named_buffers()):
        assert float((a.double() - b.double()).abs().max()) <= 1e-6 * max(float(b.double().abs().max()), 1.0), k


# ---------------------------------------------------------------------------------------------------------------------
# (d) the full model: forward_shared in train() against forward() on the replicated batch
# ---------------------------------------------------------------------------------------------------------------------
def _train_model(sampler):
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(text_vocab_size=512, sampler_type=sampler), None).train()
    for m in model.modules():               # dropout is not what is tested: the two paths must be comparable
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
        if hasattr(m, "gate_dropout"):
            m.gate_dropout = 0.0
    gen = torch.Generator().manual_seed(21)
    with torch.no_grad():                   # non-trivial BatchNorm running statistics
        for n_, p_ in model.named_parameters():
            if n_.endswith("mean_scale"):   # at mean_scale = 1 the gradient of a bias in front of a GraphNorm vanishes: only noise
                p_.copy_(torch.rand(p_.shape, generator=gen) + 0.5)     # would be left to compare (sgenc_bwd_restated.make_encoder)
        for n_, b_ in model.named_buffers():
            if n_.endswith("running_mean"):
                b_.copy_(torch.randn(b_.shape, generator=gen) * 0.5)
            if n_.endswith("running_var"):
                b_.copy_(torch.rand(b_.shape, generator=gen) + 0.5)
    return model


def _shared_inputs(d, wl, noises, seed=None):
    kw = dict(node_embeddings=d.x, edge_index=d.edge_index, edge_embeddings=d.edge_attr, batch=d.batch, questions=d.questions,
              qsts_att_mask=d.att_mask, graph_index=wl.graph_index, scene_graphs=d.scene_graphs(), noises=noises)
    return kw if seed is None else dict(kw, seed=seed)


def _perturbed_gaps(scores, noise, batch, Q, nmax):
    """Per question, the gap between the K-th and the (K + 1)-th largest entry of the masked layer's padded row of scores +
    noise (pads score 0.0 and take part, quirk Q1), where at least one of the two is a real node."""
    counts = torch.bincount(batch, minlength=Q)
    ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    dense = torch.zeros(Q, nmax, dtype=torch.float64)
    for q in range(Q):
        dense[q, :counts[q]] = scores[ptr[q]:ptr[q + 1]].double()
    v, idx = (dense + noise.double()).sort(dim=1, descending=True)
    real = idx < counts.view(-1, 1)
    gap = v[:, K - 1] - v[:, K]
    return torch.where(real[:, K - 1] | real[:, K], gap, torch.full_like(gap, float("inf")))


@pytest.fixture(scope="module")
def train_case(dev):
    """(d)'s case: tests/test_gpu_instances.py's workload (G = 5 graphs of 3 to 40 nodes, Q = 12 questions, WL_SEED = 108,
    added_sym_edge empty), the Gumbel sampler with explicit noise, train() with every dropout probability 0; two copies of one
    model, one stepped through forward_shared on the distinct batch, one through forward() on the replicated batch.
    PRECONDITION, asserted on every run: the replicated forward's own masked-layer scores (read through a hook on its gate) plus
    the noise have a K-th / (K + 1)-th gap above MIN_GAP = 1e-4 on every question -- a mask may differ only at a tie.  The seed
    was kept after running that forward alone: smallest gap over the 12 questions 1.795e-02 (printed on every run)."""
    from oracle import samplers as OS
    wl = _workload(WL_SEED, sym=False)
    rep = wl.replicated()
    gen = torch.Generator().manual_seed(5)
    noises = {3: OS.uniform_to_gumbel(torch.rand(Q_MODEL, wl.max_nodes, generator=gen))}
    w = torch.randn(Q_MODEL, 1842, generator=gen).to(dev)
    base = _train_model("gumbel")
    shared, plain = copy.deepcopy(base).to(dev), copy.deepcopy(base).to(dev)
    d, dr = wl.to(dev), rep.to(dev)
    nz = {k: v.to(dev) for k, v in noises.items()}
    seen = []
    mask_mod = plain.gat_seq.convs[3].mask
    keep = mask_mod.gate_scores
    mask_mod.gate_scores = lambda *a, **kw: (seen.append(keep(*a, **kw)), seen[-1])[1]
    try:
        ref = plain(dr.x, dr.edge_index, dr.edge_attr, dr.batch, dr.questions, dr.att_mask, return_masks=True,
                    scene_graphs=dr.scene_graphs(), noises=nz)
    finally:
        del mask_mod.gate_scores
    assert len(seen) == 1
    gaps = _perturbed_gaps(seen[0].detach().cpu().view(-1), noises[3], rep.batch, Q_MODEL, wl.max_nodes)
    print(f"train_case: smallest top-k gap of scores + noise over {Q_MODEL} questions = {float(gaps.min()):.3e}")
    assert float(gaps.min()) > MIN_GAP, gaps
    (ref[0] * w).sum().backward()
    out, inst = shared.forward_shared(**_shared_inputs(d, wl, nz))
    (out[0] * w).sum().backward()
    return argparse.Namespace(base=base, shared=shared, plain=plain, wl=wl, rep=rep, d=d, dr=dr, nz=nz, w=w, out=out, ref=ref, inst=inst)


def test_forward_shared_in_train_against_forward_on_the_replicated_batch(train_case):
    """(d): masks equal; logits within LOGIT_TOL = 1e-4 and gates within 1e-5 (the bounds of tests/test_gpu_instances.py's case
    (e)); every parameter gradient within 2e-3 of the replicated one's largest entry; the running BatchNorm buffers within 1e-6
    of the replicated ones' largest entry."""
    c = train_case
    (logits, mask, gate, _, _), (rl, rm, rg, _, _) = c.out, c.ref
    assert logits.shape == rl.shape == (Q_MODEL, 1842) and mask.shape == rm.shape and gate.shape == rg.shape
    err, gerr = float((logits - rl).detach().abs().max()), float((gate - rg).detach().abs().max())
    print(f"forward_shared vs replicated, train(): max |logit diff| = {err:.3e}, max |gate diff| = {gerr:.3e}")
    assert torch.equal(mask, rm), "a top-k mask differs"
    assert err < LOGIT_TOL and gerr < 1e-5
    rec, checked = {"logits": err, "gate": gerr}, 0
    for (k, a), (_, b) in zip(c.shared.named_parameters(), c.plain.named_parameters()):
        assert (a.grad is None) == (b.grad is None), k
        if b.grad is None:
            continue
        scale = float(b.grad.abs().max())
        rec["d_" + k] = float((a.grad - b.grad).abs().max()) / max(scale, 1e-30)
        checked += 1
    parity_record("instances_train_full_model_vs_replicated", rec)
    for k, v in rec.items():
        if k.startswith("d_"):
            assert v < 2e-3, f"{k}: {v:.3e}"
    assert checked > 100
    for (k, a), (_, b) in zip(c.shared.named_buffers(), c.plain.named_buffers()):
        if k.endswith(("running_mean", "running_var")):
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), k
            assert not torch.equal(b, dict(c.base.named_buffers())[k].to(b.device)), f"{k} did not move"
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 1, k


def test_forward_shared_forward_only_with_imle(dev):
    """(d), the I-MLE sampler forward only (train(), no_grad, explicit noise): masks equal, logits within LOGIT_TOL."""
    from oracle import samplers as OS
    wl = _workload(WL_SEED, sym=False)
    rep = wl.replicated()
    gen = torch.Generator().manual_seed(7)
    nz = {3: OS.uniform_to_gumbel(torch.rand(Q_MODEL, 1, wl.max_nodes, 1, generator=gen), 0.0, 0.3).to(dev)}
    base = _train_model("imle")
    shared, plain = copy.deepcopy(base).to(dev), copy.deepcopy(base).to(dev)
    d, dr = wl.to(dev), rep.to(dev)
    with torch.no_grad():
        out, _ = shared.forward_shared(**_shared_inputs(d, wl, nz))
        ref = plain(dr.x, dr.edge_index, dr.edge_attr, dr.batch, dr.questions, dr.att_mask, return_masks=True,
                    scene_graphs=dr.scene_graphs(), noises=nz)
    err = float((out[0] - ref[0]).abs().max())
    print(f"forward_shared vs replicated, imle forward: max |logit diff| = {err:.3e}")
    assert torch.equal(out[1], ref[1]) and int(out[1].sum()) > 0 and err < LOGIT_TOL


# ---------------------------------------------------------------------------------------------------------------------
# (e) behaviour
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_shared_in_eval_gives_the_bits_of_encode_scene_and_ask(train_case):
    c = train_case
    model = copy.deepcopy(c.shared).eval()
    with torch.no_grad():
        out, inst = model.forward_shared(**_shared_inputs(c.d, c.wl, c.nz))
        state = model.encode_scene(c.d.x, c.d.edge_index, c.d.edge_attr, c.d.batch, c.d.scene_graphs())
        want, winst = model.ask(state, c.d.questions, c.d.att_mask, c.wl.graph_index, noises=c.nz)
    for name, a, b in zip(("logits", "mask", "gate"), out, want):
        _same_bits(a, b, name)
    assert torch.equal(inst.node_src, winst.node_src) and out[3] == want[3] and out[4] is None


def test_two_identical_training_steps_give_equal_bits_and_the_counter_counts(train_case):
    from isubgvqa_amd import ops
    c = train_case
    grads = []
    for _ in range(2):
        model = copy.deepcopy(c.base).to(c.w.device)
        before = ops.COUNTERS["instance_rows_bwd"]
        out, _ = model.forward_shared(**_shared_inputs(c.d, c.wl, c.nz))
        assert ops.COUNTERS["instance_rows_bwd"] == before, "the backward kernel ran in the forward"
        (out[0] * c.w).sum().backward()
        assert ops.COUNTERS["instance_rows_bwd"] == before + 1, "one launch per backward"
        grads.append({k: v.grad for k, v in model.named_parameters() if v.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 100
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), f"{k}: two identical steps differ"
    for k, v in c.shared.named_parameters():                    # and they are the fixture's step
        if v.grad is not None:
            assert torch.equal(v.grad, grads[0][k]), k


def test_train_step_and_validate_drive_shared_scenes(train_case, dev):
    from isubgvqa_amd import optim, train
    c = train_case
    model = copy.deepcopy(c.base).to(dev)
    shared = train.SharedScenes(model)
    opt = optim.Adam(model.parameters(), lr=1e-4)
    meters = train.Meters(dev)
    labels = torch.randint(0, 1842, (Q_MODEL,), generator=torch.Generator().manual_seed(3)).to(dev)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    res = train.train_step(shared, opt, _shared_inputs(c.d, c.wl, c.nz), labels, meters, seed=11)
    assert model.n_train_steps == Q_MODEL == shared.n_train_steps and bool(torch.isfinite(res.loss))
    moved = sum(int(not torch.equal(v, before[k])) for k, v in model.named_parameters())
    assert moved > 100, "the optimizer did not step"
    train.validate(shared, [(_shared_inputs(c.d, c.wl, c.nz), labels)], meters)
    assert model.n_valid_steps == Q_MODEL and model.training and shared.training
