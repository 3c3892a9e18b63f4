"""isg_instances_size / isg_instances_fill / isg_instance_rows, ops.graph_instances, ISubGVQA.encode_scene / ask and
explain.evaluate with a graph index, on the GPU (include/isg_instances.h).  Every output of the expansion is an
integer: it is compared EXACTLY with the loop of tests/instances_restated.py.  Sizes sit on the boundaries of a wave (64 instance
rows per pass of the fill), of a workgroup (256) and of the size pass's scan block (ops.INSTANCES_SCAN_BLOCK = 1024 instances)."""
import argparse
import ctypes

import pytest
import torch

import instances_restated as R
from test_gpu_models import LOGIT_TOL

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7
BIG = (200, 1100)               # an instance longer than a wave's (64) and a workgroup's (256) single pass
SPECIAL = [(0, 0), (4, 0), (1, 1)]      # no nodes; nodes without edges; one node with a self loop (its only possible edge)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """(fast, strict): the product library and its strict twin, both bound from include/isg_instances.h."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib, _lib_instances
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB), _lib_instances.SIGNATURES)
    assert strict.isg_instances_abi_version() == _lib_instances.ABI_VERSION
    return _lib_instances.load(), strict


def make_graphs(spec, seed):
    """spec: (nodes, edges) per graph -> (batch int64 [N], edge_index int64 [2, E]); a graph's edges are random pairs of its own
    nodes and contiguous, the graphs in order."""
    gen = torch.Generator().manual_seed(seed)
    batch, src, dst, lo = [], [], [], 0
    for g, (n, e) in enumerate(spec):
        batch += [g] * n
        assert n > 0 or e == 0
        if e:
            src.append(lo + torch.randint(0, n, (e,), generator=gen))
            dst.append(lo + torch.randint(0, n, (e,), generator=gen))
        lo += n
    ei = torch.stack([torch.cat(src), torch.cat(dst)]) if src else torch.zeros(2, 0, dtype=torch.int64)
    return torch.tensor(batch, dtype=torch.int64), ei


def spec_of(G, seed, Q=1):
    if G == 1:
        return [BIG] if Q <= 2 else [(5, 7)]
    if G == 3:
        return list(SPECIAL)
    gen = torch.Generator().manual_seed(seed)
    n = torch.randint(1, 31, (G,), generator=gen).tolist()
    e = torch.randint(0, 61, (G,), generator=gen).tolist()
    spec = [(a, b) for a, b in zip(n, e)]
    spec[5], spec[17], spec[40], spec[69] = SPECIAL[0], SPECIAL[1], SPECIAL[2], BIG
    return spec


def index_of(G, Q, kind, seed):
    """same: every instance the same graph (the largest); arange; repeats: random with repeats, graph G // 2 never referenced."""
    if kind == "arange":
        assert Q == G
        return torch.arange(G)
    if kind == "same":
        return torch.full((Q,), G - 1, dtype=torch.int64)
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, G - 1, (Q,), generator=gen)
    return idx + (idx >= G // 2)


SCAN = 1024 + 1                 # one more than ops.INSTANCES_SCAN_BLOCK
CASES = [(1, 1, "arange"), (1, 2, "same"), (1, 65, "same"), (1, SCAN, "same"),
         (3, 1, "same"), (3, 2, "repeats"), (3, 65, "repeats"), (3, SCAN, "repeats"), (3, 3, "arange"),
         (70, 1, "same"), (70, 2, "same"), (70, 65, "same"), (70, 65, "repeats"), (70, SCAN, "repeats"), (70, 70, "arange")]


def raw_expand(lib, dev, ptr, batch, ei, index, G, cap_nodes=None, cap_edges=None):
    """Both passes through the C ABI on buffers of the caller, every output followed by GUARD sentinel words -> (outputs trimmed
    to their sizes, status).  Asserts that no guard word was touched.  Capacities default to the sizes the size pass reports."""
    N, E, Q = batch.numel(), ei.size(1), index.numel()
    full = lambda n, dt: torch.full((n + GUARD,), SENTINEL, dtype=dt, device=dev)
    wsb = lib.isg_instances_workspace_bytes(G)
    assert wsb == 4 * (G + 1)
    iptr, ieptr, status, ws = full(Q + 1, torch.int32), full(Q + 1, torch.int32), full(4, torch.int32), full(G + 1, torch.int32)
    rc = lib.isg_instances_size(ptr.data_ptr(), batch.data_ptr(), ei.data_ptr(), index.data_ptr(), N, E, G, Q, iptr.data_ptr(),
                                ieptr.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = status[:4].tolist()
    cn, ce = st[0] if cap_nodes is None else cap_nodes, st[1] if cap_edges is None else cap_edges
    bo, ns, es, eo = full(cn, torch.int64), full(cn, torch.int64), full(ce, torch.int64), full(2 * ce, torch.int64)
    rc = lib.isg_instances_fill(ptr.data_ptr(), ei.data_ptr(), index.data_ptr(), N, E, G, Q, iptr.data_ptr(), ieptr.data_ptr(),
                                ws.data_ptr(), wsb, cn, ce, bo.data_ptr(), eo.data_ptr(), ns.data_ptr(), es.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    sizes = {"ptr": Q + 1, "eptr": Q + 1, "status": 4, "ws": G + 1, "batch": cn, "node_src": cn, "edge_src": ce, "edge_index": 2 * ce}
    bufs = {"ptr": iptr, "eptr": ieptr, "status": status, "ws": ws, "batch": bo, "node_src": ns, "edge_src": es, "edge_index": eo}
    for k, b in bufs.items():
        assert b.numel() == sizes[k] + GUARD and bool((b[sizes[k]:] == SENTINEL).all()), f"{k}: a guard word was written"
    out = {k: b[:sizes[k]].cpu() for k, b in bufs.items()}
    out["edge_index"] = out["edge_index"].view(2, ce)
    return out


def assert_equals_restatement(out, r, what):
    for k in ("ptr", "eptr", "batch", "node_src", "edge_src", "edge_index", "status"):
        got, want = out[k] if isinstance(out, dict) else getattr(out, k).cpu(), getattr(r, k)
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), f"{what}: {k} differs"


@pytest.mark.parametrize("G,Q,kind", CASES, ids=[f"G{g}-Q{q}-{k}" for g, q, k in CASES])
def test_expansion_equals_the_restatement(dev, libs, G, Q, kind):
    """(a): every output as integers, guard words behind every output, twice on the fast library and once on the strict one with
    equal bits; then ops.graph_instances with host sizes (no device-to-host copy) and without (the 8-byte copy)."""
    from isubgvqa_amd import ops
    batch, ei = make_graphs(spec_of(G, seed=G, Q=Q), seed=100 + G)
    index = index_of(G, Q, kind, seed=Q)
    r = R.expand(batch, ei, index, G)
    assert r.status[2:].tolist() == [0, 0]
    if kind == "repeats":
        assert G // 2 not in index.tolist() and (Q <= G or len(set(index.tolist())) < Q)
    d_batch, d_ei, d_idx = batch.to(dev), ei.to(dev), index.int().to(dev)
    plan = ops.GraphPlan.build(d_batch, d_ei, num_graphs=G)
    assert torch.equal(plan.ptr.cpu().long(), R.graph_ptr(batch, G))
    runs = [raw_expand(lib, dev, plan.ptr, d_batch, d_ei, d_idx, G) for lib in (libs[0], libs[0], libs[1])]
    assert_equals_restatement(runs[0], r, "isg_instances_*")
    assert torch.equal(runs[0]["ws"].long(), R.edge_ranges(batch, ei, G)[0])
    for other, name in ((runs[1], "the second run"), (runs[2], "the strict library")):
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), f"{name} differs in {k}"
    sizes = torch.stack([torch.bincount(batch, minlength=G), torch.bincount(batch[ei[1]], minlength=G)])
    ops.reset_counters()
    for inst in (ops.graph_instances(plan, d_ei, index, sizes=sizes), ops.graph_instances(plan, d_ei, d_idx),
                 ops.graph_instances(plan, d_ei, index.to(dev))):
        assert_equals_restatement(inst, r, "ops.graph_instances")
        inst.verify()
        assert inst.Q == Q and torch.equal(inst.index.cpu().long(), index)
    assert ops.counters()["graph_instances"] == 3
    assert torch.equal(inst.gather_nodes(d_batch).cpu(), batch[r.node_src])
    assert torch.equal(inst.gather_edges(d_ei[0]).cpu(), ei[0][r.edge_src])
    if r.batch.numel() and r.edge_src.numel():
        ip = ops.graph_instances(plan, d_ei, index, sizes=sizes).plan()
        assert ip.B == Q and ip.N == r.batch.numel() and ip.E == r.edge_src.numel() and torch.equal(ip.ptr.cpu(), r.ptr)
    ops.check_plans()


def test_expansion_of_a_batch_without_edges(dev, libs):
    from isubgvqa_amd import ops
    G = 3
    batch, ei = make_graphs([(2, 0), (0, 0), (3, 0)], seed=1)
    index = torch.tensor([2, 0, 0, 1, 2])
    r = R.expand(batch, ei, index, G)
    assert r.status.tolist() == [10, 0, 0, 0]
    d_batch, d_ei = batch.to(dev), ei.to(dev)
    plan = ops.GraphPlan.build(d_batch, None, num_graphs=G)
    for lib in libs:
        assert_equals_restatement(raw_expand(lib, dev, plan.ptr, d_batch, d_ei, index.int().to(dev), G), r, "E == 0")
    inst = ops.graph_instances(plan, d_ei, index)
    assert_equals_restatement(inst, r, "ops.graph_instances, E == 0")
    inst.verify()
    none = ops.graph_instances(plan, d_ei, index[:0])
    assert none.Q == 0 and none.ptr.tolist() == [0] and none.status.tolist() == [0, 0, 0, 0] and none.batch.numel() == 0
    none.verify()


def test_bad_inputs_set_their_flag_and_never_write_beyond_the_capacities(dev, libs):
    """(b): an index outside [0, G), a shuffled edge list, an edge across two graphs -- each sets its own flag and no other,
    verify() raises naming it, the guard words behind every output stay (also with capacities smaller than the sizes)."""
    from isubgvqa_amd import _lib, ops
    G = 70
    batch, ei = make_graphs(spec_of(G, seed=G), seed=100 + G)
    index = index_of(G, 65, "repeats", seed=3)
    d_batch = batch.to(dev)
    plan = ops.GraphPlan.build(d_batch, ei.to(dev), num_graphs=G)
    ok = ops.graph_instances(plan, ei.to(dev), index.to(dev))
    assert ok.status.tolist()[2:] == [0, 0]
    ok.verify()
    # an index out of range: those instances are empty, the rest is what the restatement says
    bad_idx = index.clone()
    bad_idx[3], bad_idx[40], bad_idx[64] = G, -1, 1 << 20
    r = R.expand(batch, ei, bad_idx, G)
    assert r.status[2:].tolist() == [1, 0]
    for lib in libs:
        assert_equals_restatement(raw_expand(lib, dev, plan.ptr, d_batch, ei.to(dev), bad_idx.int().to(dev), G), r, "bad index")
    inst = ops.graph_instances(plan, ei.to(dev), bad_idx.to(dev))
    assert_equals_restatement(inst, r, "ops.graph_instances, bad index")
    with pytest.raises(_lib.IsgError, match="bad_index"):
        inst.verify()
    with pytest.raises(ValueError, match="index"):            # a host index is looked at on the host
        ops.graph_instances(plan, ei.to(dev), bad_idx, sizes=torch.stack([torch.bincount(batch, minlength=G),
                                                                           torch.bincount(batch[ei[1]], minlength=G)]))
    # a shuffled edge list / an edge across two graphs
    shuffled = ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(5))].contiguous()
    across = ei.clone()
    e_mid = ei.size(1) // 2
    across[0, e_mid] = (across[0, e_mid] + 31) % batch.numel()
    assert batch[across[0, e_mid]] != batch[across[1, e_mid]]
    for name, bad_ei in (("shuffled", shuffled), ("across", across)):
        assert R.edge_ranges(batch, bad_ei, G)[1] == 1
        d_bad = bad_ei.to(dev)
        for lib in libs:
            out = raw_expand(lib, dev, plan.ptr, d_batch, d_bad, index.int().to(dev), G)
            assert out["status"].tolist()[2:] == [0, 1], name
            assert out["ptr"].tolist() == R.expand(batch, ei, index, G).ptr.tolist()        # the node side does not depend on the edges
            assert bool((out["eptr"][1:] >= out["eptr"][:-1]).all()) and out["eptr"][-1] == out["status"][1]
            assert bool((out["edge_src"] >= 0).all()) and bool((out["edge_src"] < ei.size(1)).all())
            # capacities below the sizes: raw_expand asserts the guard words.  (Where graph ids decrease along the list an entry of
            # the edge ranges has several writers: the ranges of two calls on such a list may differ, their flag does not.)
            small = raw_expand(lib, dev, plan.ptr, d_batch, d_bad, index.int().to(dev), G, cap_nodes=int(out["status"][0]) // 2,
                               cap_edges=int(out["status"][1]) // 3)
            assert small["status"].tolist()[2:] == [0, 1] and small["status"][0] == out["status"][0]
        inst = ops.graph_instances(plan, d_bad, index.to(dev))
        with pytest.raises(_lib.IsgError, match="bad_grouping"):
            inst.verify()
    # capacities below the sizes on a good input: what fits is written, right
    good = R.expand(batch, ei, index, G)
    cn, ce = int(good.status[0]) - 70, int(good.status[1]) - 300
    small = raw_expand(libs[0], dev, plan.ptr, d_batch, ei.to(dev), index.int().to(dev), G, cap_nodes=cn, cap_edges=ce)
    assert torch.equal(small["batch"], good.batch[:cn]) and torch.equal(small["node_src"], good.node_src[:cn])
    assert torch.equal(small["edge_src"], good.edge_src[:ce]) and torch.equal(small["edge_index"], good.edge_index[:, :ce])
    # a host size that disagrees with the device's
    wrong = torch.stack([torch.bincount(batch, minlength=G), torch.bincount(batch[ei[1]], minlength=G)])
    wrong[0, int(index[0])] -= 1
    with pytest.raises(_lib.IsgError, match="sizes"):
        ops.graph_instances(plan, ei.to(dev), index, sizes=wrong).verify()


@pytest.mark.parametrize("Cx,Ce", [(4, 4), (128, 128), (300, 300), (300, 4)])
def test_instance_rows_equal_index_select_as_words(dev, Cx, Ce):
    """(c): the one-launch gather on strided inputs (column slices of wider tensors) against index_select, as words."""
    from isubgvqa_amd import ops
    G = 70
    batch, ei = make_graphs(spec_of(G, seed=G), seed=100 + G)
    index = index_of(G, 65, "repeats", seed=9)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=G)
    inst = ops.graph_instances(plan, ei.to(dev), index)
    assert inst.node_src.numel() > 256 and inst.edge_src.numel() > 256
    g = torch.Generator().manual_seed(Cx + Ce)
    # bit patterns, NaNs and denormals included: the gather moves words
    xw = torch.randint(-2 ** 31, 2 ** 31, (batch.numel(), Cx + 12), generator=g, dtype=torch.int64).int().to(dev)
    ew = torch.randint(-2 ** 31, 2 ** 31, (ei.size(1), Ce + 8), generator=g, dtype=torch.int64).int().to(dev)
    x, e = xw.view(torch.float32)[:, 8:8 + Cx], ew.view(torch.float32)[:, 4:4 + Ce]
    assert not x.is_contiguous() and not e.is_contiguous()
    xo, eo = inst.gather_rows(x, e)
    assert xo.is_contiguous() and eo.is_contiguous() and xo.dtype == eo.dtype == torch.float32
    assert torch.equal(xo.view(torch.int32), xw[:, 8:8 + Cx].index_select(0, inst.node_src))
    assert torch.equal(eo.view(torch.int32), ew[:, 4:4 + Ce].index_select(0, inst.edge_src))
    # contiguous inputs as well, and shapes the kernel does not take are refused on the host
    xc, ec = x.contiguous(), e.contiguous()
    xo2, eo2 = inst.gather_rows(xc, ec)
    assert torch.equal(xo2.view(torch.int32), xo.view(torch.int32)) and torch.equal(eo2.view(torch.int32), eo.view(torch.int32))
    with pytest.raises(ValueError):
        inst.gather_rows(xc[:-1], ec)
    with pytest.raises(ValueError):
        inst.gather_rows(xw.view(torch.float32)[:, 1:1 + Cx], ec)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
G_MODEL, Q_MODEL, K = 5, 12, 5
SIZES = (3, 40, 17, 9, 26)      # nodes per graph: 3 to 40
WL_SEED = 108                   # chosen on the CPU oracle: see shared_case
MIN_GAP = 1e-4


def _model():
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(text_vocab_size=512), None).eval()
    gen = torch.Generator().manual_seed(21)
    with torch.no_grad():   # non-trivial BatchNorm running statistics
        for n_, b_ in model.named_buffers():
            if n_.endswith("running_mean"):
                b_.copy_(torch.randn(b_.shape, generator=gen) * 0.5)
            if n_.endswith("running_var"):
                b_.copy_(torch.rand(b_.shape, generator=gen) + 0.5)
    return model


def _workload(seed, sym: bool):
    """G = 5 graphs of 3 to 40 nodes, Q = 12 questions in a shuffled order that asks every graph at least once."""
    from isubgvqa_amd import synthetic
    wl = synthetic.make_shared_workload(G_MODEL, 3, tokens=9, seed=seed, text_vocab=512, sizes=SIZES)
    first = [int((wl.graph_index == g).nonzero()[0]) for g in range(G_MODEL)]
    rest = [i for i in range(wl.graph_index.numel()) if i not in first]
    keep = torch.tensor(sorted(first + rest[:Q_MODEL - G_MODEL]))
    wl.questions, wl.att_mask, wl.graph_index = wl.questions[keep], wl.att_mask[keep], wl.graph_index[keep]
    assert wl.graph_index.numel() == Q_MODEL and set(wl.graph_index.tolist()) == set(range(G_MODEL))
    assert wl.added_sym_edge.numel() > 0
    if not sym:
        wl.added_sym_edge = wl.added_sym_edge[:0]
    return wl


def topk_gaps(model, rep):
    """On the CPU oracle, for the replicated batch: per question, the gap between the K-th and the (K + 1)-th largest score of
    the masked layer's padded row (pads score 0.0 and take part, quirk Q1), where at least one of the two is a real node."""
    from oracle import model as OM
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ocfg = OM.PathConfig(heads=4, masking_thresholds=[1.0, 1.0, 1.0, 0.15], sampler_type="imle", sample_k=K)
    trace = []
    with torch.no_grad():
        OM.isubgvqa_forward(sd, rep.x, rep.edge_index, rep.edge_attr, rep.batch, rep.questions, rep.att_mask, rep.x_bbox,
                            rep.added_sym_edge, ocfg, None, trace=trace)
    dense = trace[3]["dense"].squeeze(-1).double()
    counts = rep.graph_sizes[0]
    v, idx = dense.sort(dim=1, descending=True)
    real = idx < counts.view(-1, 1)
    gap = v[:, K - 1] - v[:, K]
    involved = real[:, K - 1] | real[:, K]
    return torch.where(involved, gap, torch.full_like(gap, float("inf")))


@pytest.fixture(scope="module")
def shared_case(dev):
    """(e)'s case: added_sym_edge empty.  The workload seed WL_SEED was chosen on the CPU oracle so that for EVERY question the
    gap between the 5-th and the 6-th largest gate of the masked layer exceeds 1e-4 (asserted here on every run): the encoder's
    Linears may take another kernel at G rows than at Q rows, and a mask may flip only at a tie.  Seeds 0 .. 108 were tried in order for a smallest gap beyond
    2e-4 (twice the demand; the scores of this untrained model are of the order 1e-3, most seeds have a question near 6e-5);
    at WL_SEED = 108 the smallest gap over the 12 questions is 2.07e-4, the next ones 5.0e-4 and 6.5e-4."""
    model = _model()
    wl = _workload(WL_SEED, sym=False)
    rep = wl.replicated()
    gaps = topk_gaps(model, rep)
    print(f"shared_case: smallest top-k gap over {Q_MODEL} questions = {float(gaps.min()):.3e}")
    assert float(gaps.min()) > MIN_GAP, gaps
    model = model.to(dev)
    with torch.no_grad():
        d, dr = wl.to(dev), rep.to(dev)
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs())
        out, inst = model.ask(state, d.questions, d.att_mask, wl.graph_index)
        ref = model(dr.x, dr.edge_index, dr.edge_attr, dr.batch, dr.questions, dr.att_mask, return_masks=True,
                    scene_graphs=dr.scene_graphs())
    return argparse.Namespace(model=model, wl=wl, rep=rep, d=d, dr=dr, state=state, out=out, inst=inst, ref=ref)


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        f"{what}: bits differ, max |d| = {(a - b).abs().max().item():.3e}"


def test_ask_returns_the_bits_of_answer_graphs_on_the_restated_instances(dev):
    """(d), first half: with a non-empty added_sym_edge, ask() equals answer_graphs called on tensors gathered with the
    restatement's maps -- logits, mask and gate as bits.  This pins the kernels inside the model."""
    from isubgvqa_amd import ops
    model = _model().to(dev)
    wl = _workload(3, sym=True)
    d = wl.to(dev)
    r = R.expand(wl.batch, wl.edge_index, wl.graph_index, G_MODEL)
    with torch.no_grad():
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs())
        (logits, mask, gate, extra, mask_text), inst = model.ask(state, d.questions, d.att_mask, wl.graph_index)
        assert_equals_restatement(inst, r, "ask's instances")
        glf, instr = model.language_features(d.questions, d.att_mask, None, None)
        b, ei = r.batch.to(dev), r.edge_index.to(dev)
        plan = ops.GraphPlan.build(b, ei, num_graphs=Q_MODEL, max_nodes=state.plan.nmax, max_edges=state.plan.emax)
        want = model.answer_graphs(state.x_enc[r.node_src.to(dev)].contiguous(), ei, state.e_enc[r.edge_src.to(dev)].contiguous(), b,
                                   instr, glf, plan, True, None, None)
    assert extra == [] and mask_text is None and logits.shape == (Q_MODEL, 1842)
    assert mask.shape == gate.shape == (r.batch.numel(), 1) and int(mask.sum()) > 0
    _same_bits(logits, want[0], "logits")
    _same_bits(mask, want[1], "mask")
    _same_bits(gate, want[2], "gate")
    ops.check_plans()


def test_ask_with_the_identity_index_returns_the_bits_of_forward(dev):
    """(d), second half: graph_index = arange(G) and G questions -- logits, mask and gate of forward(), as bits."""
    model = _model().to(dev)
    wl = _workload(3, sym=True)
    first = torch.tensor([int((wl.graph_index == g).nonzero()[0]) for g in range(G_MODEL)])
    d = wl.to(dev)
    q, m = d.questions[first.to(dev)].contiguous(), d.att_mask[first.to(dev)].contiguous()
    with torch.no_grad():
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, d.scene_graphs())
        got, inst = model.ask(state, q, m, torch.arange(G_MODEL))
        want = model(d.x, d.edge_index, d.edge_attr, d.batch, q, m, return_masks=True, scene_graphs=d.scene_graphs())
    assert torch.equal(inst.node_src.cpu(), torch.arange(wl.x.size(0))) and torch.equal(inst.edge_index, d.edge_index)
    for name, a, b in zip(("logits", "mask", "gate"), got, want):
        _same_bits(a, b, name)
    assert got[3] == want[3] == [] and got[4] is None and want[4] is None


def test_shared_encoding_against_the_replicated_forward(shared_case):
    """(e): logits within LOGIT_TOL = 1e-4 (the bound of tests/test_gpu_models.py), gates within 1e-5, masks equal on every
    question.  The seed's smallest top-k gap is asserted by the fixture (2.07e-4 at WL_SEED = 108)."""
    c = shared_case
    (logits, mask, gate, _, _), (rl, rm, rg, _, _) = c.out, c.ref
    assert logits.shape == rl.shape == (Q_MODEL, 1842) and mask.shape == rm.shape and gate.shape == rg.shape
    err, gerr = (logits - rl).abs().max().item(), (gate - rg).abs().max().item()
    print(f"shared vs replicated: max |logit diff| = {err:.3e}, max |gate diff| = {gerr:.3e}")
    assert torch.equal(mask, rm), "a top-k mask differs"
    per_q = torch.zeros(Q_MODEL, device=mask.device).index_add_(0, c.inst.batch, (mask != rm).float().squeeze(1))
    assert int((per_q > 0).sum()) == 0
    assert err < LOGIT_TOL
    assert gerr < 1e-5


def test_the_encoder_runs_on_the_distinct_graphs_and_the_counter_counts(shared_case, dev):
    """(f): x_enc has N rows, not N'; ops.COUNTERS["graph_instances"] advances by one per ask."""
    from isubgvqa_amd import ops
    c = shared_case
    N, E = c.wl.x.size(0), c.wl.edge_index.size(1)
    assert tuple(c.state.x_enc.shape) == (N, 300) and tuple(c.state.e_enc.shape) == (E, 300)
    assert c.inst.node_src.numel() == c.rep.x.size(0) > N and c.state.plan.B == G_MODEL
    assert torch.equal(c.state.sizes, c.wl.graph_sizes)
    before = ops.COUNTERS["graph_instances"]
    with torch.no_grad():
        for i in range(2):
            out, inst = c.model.ask(c.state, c.d.questions, c.d.att_mask, c.wl.graph_index)
            assert ops.COUNTERS["graph_instances"] == before + i + 1
    _same_bits(out[0], c.out[0], "a second ask on the same state")
    # a device index: the sizes come from the 8-byte copy, the result is the same
    with torch.no_grad():
        out_d, _ = c.model.ask(c.state, c.d.questions, c.d.att_mask, c.wl.graph_index.to(dev))
    _same_bits(out_d[0], c.out[0], "ask with a device index")
    ops.check_plans()


def test_evaluate_with_a_graph_index_gives_the_totals_of_the_replicated_evaluation(shared_case, dev):
    """(g): explain.evaluate through encode_scene / ask scores names[node_src]: the integer totals of the replicated run."""
    from isubgvqa_amd import explain
    c = shared_case
    V = 2578
    stoi = {f"w{i}": i for i in range(V)}
    answers = [f"w{(11 * a) % V}" if a % 3 == 0 else f"answer {a}" for a in range(1842)]
    tables = explain.TokenTables(stoi, answers)
    gen = torch.Generator().manual_seed(13)
    label = c.ref[0].argmax(1).cpu()
    label[2::3] = (label[2::3] + 1) % 1842
    names_rep = c.rep.x[:, 0]
    ptr = R.graph_ptr(c.rep.batch, Q_MODEL)
    qtok = torch.full((Q_MODEL, 6), -1, dtype=torch.int32)
    for q in range(Q_MODEL):             # question words: some name nodes of the question's graph, some name nothing
        own = names_rep[ptr[q]:ptr[q + 1]]
        qtok[q, :3] = own[torch.randint(0, own.numel(), (3,), generator=gen)].int()
        qtok[q, 3] = int(torch.randint(0, V, (1,), generator=gen))
    qflags = (torch.arange(Q_MODEL) % 4 == 0).int()
    shared = explain.evaluate(c.model, [explain.EvalBatch(c.d, label.to(dev), qtok.to(dev), qflags.to(dev),
                                                          graph_index=c.wl.graph_index)], tables)
    plain = explain.evaluate(c.model, [explain.EvalBatch(c.dr, label.to(dev), qtok.to(dev), qflags.to(dev))], tables)
    assert shared.totals == plain.totals
    assert shared.totals[0] == Q_MODEL and 0 < shared.totals[1] < Q_MODEL
