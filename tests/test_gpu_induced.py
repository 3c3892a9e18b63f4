"""isg_induced_size / isg_induced_fill and ops.induced_instances on the GPU (include/ext/isg_induced.h).  Every output
is an integer and is compared with torch.equal against three references: the loop of tests/induced_restated.py, the on-device
chain ops.graph_instances -> ops.subgraph_cut that the operator replaces, and a second call (equal bits) -- on the product
library and on its strict twin.  Sizes sit on the boundaries of a keep word (32 nodes), of a wave (64 nodes = two words, 64
edges per ballot, 64 instances), and of the size pass's scan block (1024 instances)."""
import ctypes

import pytest
import torch

import induced_cases as C
import induced_restated as IR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7
FIELDS = ("ptr", "eptr", "status", "batch", "node_src", "edge_src", "edge_index")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """(fast, strict): the product library and its strict twin, both bound from include/ext/isg_induced.h."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_induced, _lib
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB), _ext_induced.SIGNATURES)
    assert strict.isg_induced_abi_version() == _ext_induced.ABI_VERSION
    return _ext_induced.load(), strict


def raw_induce(lib, dev, ptr, batch, ei, index, keep, G, cap_nodes=None, cap_edges=None):
    """Both passes through the C ABI on buffers of the caller, every output followed by GUARD sentinel words -> the outputs
    trimmed to their sizes.  Asserts that no guard word was touched.  Capacities default to the sizes the size pass reports."""
    N, E, Q = batch.numel(), ei.size(1), index.numel()
    full = lambda n, dt: torch.full((n + GUARD,), SENTINEL, dtype=dt, device=dev)
    wsb = lib.isg_induced_workspace_bytes(G, Q)
    assert wsb == 4 * (G + 1 + 2 * Q)
    iptr, ieptr, status, ws = full(Q + 1, torch.int32), full(Q + 1, torch.int32), full(4, torch.int32), full(G + 1 + 2 * Q, torch.int32)
    p_keep, W = (None, 0) if keep is None else (keep.data_ptr(), keep.size(1))
    rc = lib.isg_induced_size(ptr.data_ptr(), batch.data_ptr(), ei.data_ptr(), index.data_ptr(), p_keep, W, N, E, G, Q,
                              iptr.data_ptr(), ieptr.data_ptr(), status.data_ptr(), ws.data_ptr(), wsb, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = status[:4].tolist()
    cn, ce = st[0] if cap_nodes is None else cap_nodes, st[1] if cap_edges is None else cap_edges
    bo, ns, es, eo = full(cn, torch.int64), full(cn, torch.int64), full(ce, torch.int64), full(2 * ce, torch.int64)
    rc = lib.isg_induced_fill(ptr.data_ptr(), ei.data_ptr(), index.data_ptr(), p_keep, W, N, E, G, Q, iptr.data_ptr(),
                              ieptr.data_ptr(), ws.data_ptr(), wsb, cn, ce, bo.data_ptr(), eo.data_ptr(), ns.data_ptr(),
                              es.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    sizes = {"ptr": Q + 1, "eptr": Q + 1, "status": 4, "ws": G + 1 + 2 * Q, "batch": cn, "node_src": cn, "edge_src": ce,
             "edge_index": 2 * ce}
    bufs = {"ptr": iptr, "eptr": ieptr, "status": status, "ws": ws, "batch": bo, "node_src": ns, "edge_src": es, "edge_index": eo}
    for k, b in bufs.items():
        assert b.numel() == sizes[k] + GUARD and bool((b[sizes[k]:] == SENTINEL).all()), f"{k}: a guard word was written"
    out = {k: b[:sizes[k]].cpu() for k, b in bufs.items()}
    out["edge_index"] = out["edge_index"].view(2, ce)
    return out


def device_chain(ops, plan, d_ei, d_index, d_keep):
    """The two steps on the device: every graph copied out whole, a float mask built from the bits with torch ops, the cut."""
    whole = ops.graph_instances(plan, d_ei, d_index)
    if whole.batch.numel() == 0:
        return None
    local = whole.node_src - plan.ptr.long()[d_index.long()][whole.batch]
    if d_keep is None:
        mask = torch.ones(whole.batch.numel(), device=d_ei.device)
    else:
        W = d_keep.size(1)
        word = d_keep.long()[whole.batch, (local >> 5).clamp(max=W - 1)] & 0xFFFFFFFF
        mask = (((word >> (local & 31)) & 1).bool() & (local < 32 * W)).float()
    cut = ops.subgraph_cut(mask, whole.edge_index, whole.plan())
    n, e = cut.sizes()
    return {"ptr": cut.ptr.cpu(), "status2": (n, e), "batch": cut.batch.cpu(), "edge_index": cut.edge_index.cpu(),
            "node_src": whole.node_src[cut.node_id].cpu(), "edge_src": whole.edge_src[cut.edge_id].cpu()}


CASES = [(G, Q) for G in (1, 3, 70) for Q in (1, 2, 65, 1025)]


@pytest.mark.parametrize("G,Q", CASES, ids=[f"G{g}-Q{q}" for g, q in CASES])
def test_induced_instances_equal_the_restatement_the_chain_and_a_second_call(dev, libs, G, Q):
    """Every kind of bits at the minimal W; random bits also with W + 1 and with one word too few (the nodes beyond 32 W are
    dropped).  All set and keep=None equal ops.graph_instances field for field."""
    from isubgvqa_amd import ops
    batch, ei, sizes = C.make_graphs(C.spec_of(G, Q), seed=100 + G)
    index = C.index_of(G, Q, seed=Q)
    d_batch, d_ei, d_idx = batch.to(dev), ei.to(dev), index.int().to(dev)
    plan = ops.GraphPlan.build(d_batch, d_ei, num_graphs=G)
    W = C.words_min(sizes)
    assert ops.keep_words(plan.nmax) == W
    runs = [(kind, W) for kind in C.BITS] + [("random", W + 1)] + ([("random", W - 1), ("all", W - 1)] if W > 1 else [])
    ops.reset_counters()
    for n_run, (kind, w) in enumerate(runs):
        what = f"{kind}, W = {w}"
        keep = C.bits_of(kind, index, sizes, w, seed=7 * Q + w)
        d_keep = None if keep is None else keep.to(dev)
        r = IR.induce(batch, ei, index, keep, G)
        assert r.status[2:].tolist() == [0, 0]
        outs = [raw_induce(lib, dev, plan.ptr, d_batch, d_ei, d_idx, d_keep, G) for lib in (libs[0], libs[0], libs[1])]
        C.assert_same(outs[0], r, f"isg_induced_* ({what})")
        for other, name in ((outs[1], "the second call"), (outs[2], "the strict library")):
            for k, v in outs[0].items():
                assert torch.equal(v, other[k]), f"{what}: {name} differs in {k}"
        inst = ops.induced_instances(plan, d_ei, index if n_run % 2 else d_idx, d_keep)
        assert isinstance(inst, ops.InducedInstances) and inst.Q == Q
        C.assert_same(inst, r, f"ops.induced_instances ({what})")
        inst.verify()
        ch = device_chain(ops, plan, d_ei, d_idx, d_keep)
        if ch is None:
            assert r.batch.numel() == 0
        else:
            assert ch["status2"] == tuple(r.status[:2].tolist())
            for k in ("ptr", "batch", "edge_index", "node_src", "edge_src"):
                assert torch.equal(ch[k], getattr(inst, k).cpu()), f"{what}: the on-device chain differs in {k}"
        if kind in ("all", "none") and w == W:
            whole = ops.graph_instances(plan, d_ei, d_idx)
            for k in FIELDS:
                assert torch.equal(getattr(inst, k), getattr(whole, k)), f"{what}: {k} differs from ops.graph_instances"
        if kind == "zero":
            assert inst.status.tolist() == [0, 0, 0, 0] and inst.batch.numel() == 0 and inst.edge_index.shape == (2, 0)
        if kind == "random" and w == W and r.batch.numel() and r.edge_src.numel():
            assert torch.equal(inst.gather_nodes(d_batch).cpu(), batch[r.node_src])
            assert torch.equal(inst.gather_edges(d_ei[0]).cpu(), ei[0][r.edge_src])
            ip = inst.plan()
            assert ip.B == Q and ip.N == r.batch.numel() and ip.E == r.edge_src.numel() and torch.equal(ip.ptr.cpu(), r.ptr)
    assert ops.counters()["induced_instances"] == len(runs)
    ops.check_plans()


def test_leave_one_out_batch_of_the_helper_equals_the_restatement(dev, libs):
    """ops.keep_bits_leave_one_out on the device, through ops.induced_instances: instance j of graph g lacks node j."""
    from isubgvqa_amd import ops
    G = 70
    batch, ei, sizes = C.make_graphs(C.spec_of(G, 2), seed=100 + G)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=G)
    index, keep, inst_node = ops.keep_bits_leave_one_out(plan)
    want_index = [g for g, n in enumerate(sizes) if n >= 2 for _ in range(n)]
    assert index.tolist() == want_index and keep.size(1) == C.words_min(sizes) and len(want_index) > 1024
    r = IR.induce(batch, ei, index.cpu(), keep.cpu(), G)
    inst = ops.induced_instances(plan, ei.to(dev), index, keep)
    C.assert_same(inst, r, "leave-one-out")
    # every instance has its graph's nodes but one, and the one is inst_node
    n = torch.tensor(sizes)[index.cpu().long()]
    assert torch.equal((inst.ptr[1:] - inst.ptr[:-1]).cpu().long(), n - 1)
    present = torch.zeros(len(want_index), batch.numel(), dtype=torch.bool)
    present[r.batch, r.node_src] = True
    assert not bool(present[torch.arange(len(want_index)), inst_node.cpu()].any())
    out = raw_induce(libs[1], dev, plan.ptr, batch.to(dev), ei.to(dev), index, keep, G)
    C.assert_same(out, r, "leave-one-out, strict library")


def test_bad_inputs_set_their_flag_and_never_write_beyond_the_capacities(dev, libs):
    """An index outside [0, G) sets bad_index and that instance is empty; graph ids decreasing along the edge list set
    bad_grouping and the outputs stay in bounds; capacities that are too short leave the guard words behind every output."""
    from isubgvqa_amd import _lib, ops
    G, Q = 70, 65
    batch, ei, sizes = C.make_graphs(C.spec_of(G, Q), seed=100 + G)
    index = C.index_of(G, Q, seed=3)
    d_batch, d_ei = batch.to(dev), ei.to(dev)
    plan = ops.GraphPlan.build(d_batch, d_ei, num_graphs=G)
    W = C.words_min(sizes)
    keep = C.bits_of("beyond", index, sizes, W, seed=11)
    d_keep = keep.to(dev)
    bad_idx = index.clone()
    bad_idx[3], bad_idx[40], bad_idx[64] = G, -1, 1 << 20
    r = IR.induce(batch, ei, bad_idx, keep, G)
    assert r.status[2:].tolist() == [1, 0] and r.ptr[3] == r.ptr[4] and r.ptr[64] == r.ptr[65]
    for lib in libs:
        C.assert_same(raw_induce(lib, dev, plan.ptr, d_batch, d_ei, bad_idx.int().to(dev), d_keep, G), r, "bad index")
    inst = ops.induced_instances(plan, d_ei, bad_idx.to(dev), d_keep)
    C.assert_same(inst, r, "ops.induced_instances, bad index")
    with pytest.raises(_lib.IsgError, match="bad_index"):
        inst.verify()
    # a shuffled edge list: graph ids decrease along it
    shuffled = ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(5))].contiguous()
    good = IR.induce(batch, ei, index, keep, G)
    for lib in libs:
        out = raw_induce(lib, dev, plan.ptr, d_batch, shuffled.to(dev), index.int().to(dev), d_keep, G)
        assert out["status"].tolist()[2:] == [0, 1]
        assert out["ptr"].tolist() == good.ptr.tolist() and torch.equal(out["node_src"], good.node_src)     # the node side does not depend on the edges
        assert bool((out["eptr"][1:] >= out["eptr"][:-1]).all()) and out["eptr"][-1] == out["status"][1]
        assert bool((out["edge_src"] >= 0).all()) and bool((out["edge_src"] < ei.size(1)).all())
        assert bool((out["edge_index"] >= 0).all()) and bool((out["edge_index"] < int(out["status"][0])).all())
        small = raw_induce(lib, dev, plan.ptr, d_batch, shuffled.to(dev), index.int().to(dev), d_keep, G,
                           cap_nodes=int(out["status"][0]) // 2, cap_edges=int(out["status"][1]) // 3)
        assert small["status"].tolist()[2:] == [0, 1] and small["status"][0] == out["status"][0]
    with pytest.raises(_lib.IsgError, match="bad_grouping"):
        ops.induced_instances(plan, shuffled.to(dev), index.to(dev), d_keep).verify()
    # capacities below the sizes on a good input: what fits is written, right; raw_induce asserts the guard words
    for lib in libs:
        for cn, ce in ((int(good.status[0]) - 70, int(good.status[1]) - 300), (0, int(good.status[1])), (int(good.status[0]), 0), (1, 1)):
            small = raw_induce(lib, dev, plan.ptr, d_batch, d_ei, index.int().to(dev), d_keep, G, cap_nodes=cn, cap_edges=ce)
            assert torch.equal(small["batch"], good.batch[:cn]) and torch.equal(small["node_src"], good.node_src[:cn])
            assert torch.equal(small["edge_src"], good.edge_src[:ce]) and torch.equal(small["edge_index"], good.edge_index[:, :ce])
    # refusals of the operator
    with pytest.raises(_lib.IsgError, match="words per instance"):
        ops.induced_instances(plan, d_ei, index.to(dev), torch.zeros(Q, 65, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="keep"):
        ops.induced_instances(plan, d_ei, index.to(dev), d_keep[:-1])
    none = ops.induced_instances(plan, d_ei, index[:0], d_keep[:0])
    assert none.Q == 0 and none.ptr.tolist() == [0] and none.status.tolist() == [0, 0, 0, 0] and none.batch.numel() == 0
