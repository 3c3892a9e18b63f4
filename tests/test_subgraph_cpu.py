"""Host-side checks of the induced-subgraph cut: the torch restatement the GPU tests compare with (against a known answer written
out by hand), the two C-ABI entry points as far as they go without a GPU, and explain.fidelity_scores."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from subgraph_restated import restate

NAN = float("nan")


def _known():
    batch = torch.tensor([0, 0, 0, 2, 2, 2, 2])
    mask = torch.tensor([1, 0, 1, 0, 1, NAN, 1])
    ei = torch.tensor([[0, 2, 1, 2, 4, 6, 6, 3, 6, 7], [2, 0, 2, 2, 6, 4, 6, 4, 5, 0]])
    return mask, ei, batch


def test_restatement_gives_the_known_answer_written_out_by_hand():
    mask, ei, batch = _known()
    r = restate(mask, ei, batch, 4, threshold=0.0, complement=False, table_k=2)
    assert r.node_new.tolist() == [0, -1, 1, -1, 2, -1, 3]
    assert r.edge_new.tolist() == [0, 1, -1, 2, 3, 4, 5, -1, -1, -1]
    assert r.node_id.tolist() == [0, 2, 4, 6] and r.edge_id.tolist() == [0, 1, 3, 4, 5, 6]
    assert r.edge_index.tolist() == [[0, 1, 1, 2, 3, 3], [1, 0, 1, 3, 2, 3]]
    assert r.batch.tolist() == [0, 0, 2, 2]
    assert r.ptr.tolist() == [0, 2, 2, 4, 4]
    assert r.sel.tolist() == [[0, 2], [-1, -1], [1, 3], [-1, -1]]
    assert r.counts == (4, 6)
    assert r.node_new.dtype == r.edge_new.dtype == r.ptr.dtype == r.sel.dtype == torch.int32
    c = restate(mask.view(-1, 1), ei, batch, 4, threshold=0.0, complement=True, table_k=2)      # the NaN is kept here
    assert c.node_id.tolist() == [1, 3, 5]
    assert c.edge_id.tolist() == [] and tuple(c.edge_index.shape) == (2, 0) and set(c.edge_new.tolist()) == {-1}
    assert c.ptr.tolist() == [0, 1, 1, 3, 3]
    assert c.sel.tolist() == [[1, -1], [-1, -1], [0, 2], [-1, -1]]
    assert c.counts == (3, 0)
    assert tuple(restate(mask, ei, batch, 4).sel.shape) == (4, 0)


def test_header_declares_the_cut_and_the_binding_follows_it():
    from isubgvqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "isg.h")).read()
    body = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"\bsize_t\s+isg_subgraph_workspace_bytes\s*\(", body) and re.search(r"\bint\s+isg_subgraph_cut\s*\(", body)
    assert int(re.search(r"#define ISG_ABI_VERSION (\d+)", header).group(1)) == 23 == _lib.ABI_VERSION
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert _lib.SIGNATURES["isg_subgraph_workspace_bytes"] == (ctypes.c_size_t, [I64, I64])
    assert _lib.SIGNATURES["isg_subgraph_cut"] == (ctypes.c_int, [P, ctypes.c_float, I32, P, P, P, I64, I64, I64, P, P, P, P, P, P, P,
                                                                 P, I32, P, P, ctypes.c_size_t, P])


def _ws_formula(N, E, T):
    return 4 * (-(-N // T) + -(-E // T) + (N + 1) + 1)


def test_workspace_bytes_equal_the_documented_formula():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, ops
    lib = _lib.load()
    T = ops.SUBGRAPH_BLOCK
    assert T == 1024 and "SG_BLOCK = SG_THREADS * SG_PER" in open(os.path.join(
        ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc", "isg_subgraph.hip")).read()
    for N, E in ((0, 0), (1, 0), (0, 1), (T, T), (T + 1, 2 * T + 1), (82000, 205000), (2 ** 31 - 2, 2 ** 31 - 2)):
        assert lib.isg_subgraph_workspace_bytes(N, E) == _ws_formula(N, E, T), (N, E)
    assert lib.isg_subgraph_workspace_bytes(0, 0) == 8
    # one more node behind a full block opens a block: the block size the tests place their sizes on is the kernel's
    assert lib.isg_subgraph_workspace_bytes(T + 1, 0) - lib.isg_subgraph_workspace_bytes(T, 0) == 8
    assert lib.isg_subgraph_workspace_bytes(T, 0) - lib.isg_subgraph_workspace_bytes(T - 1, 0) == 4
    assert lib.isg_subgraph_workspace_bytes(-1, 0) == 0 and lib.isg_subgraph_workspace_bytes(0, -1) == 0


def test_cut_refuses_bad_arguments_before_any_hip_call():
    """No GPU is needed: every refusal below happens on the host, before the library touches HIP."""
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib
    lib = _lib.load()
    N, E, B, k = 5, 3, 2, 2
    keep = [ctypes.create_string_buffer(8 * 64) for _ in range(14)]       # host memory: never dereferenced by a refused call
    p = [ctypes.addressof(b) for b in keep]
    ws_bytes = lib.isg_subgraph_workspace_bytes(N, E)

    def call(**over):
        a = dict(node_mask=p[0], threshold=0.0, complement=0, edge_index=p[1], batch=p[2], ptr=p[3], N=N, E=E, B=B, node_new=p[4],
                 edge_new=p[5], node_id=p[6], edge_id=p[7], edge_index_out=p[8], batch_out=p[9], ptr_out=p[10], sel=p[11], table_k=k,
                 counts=p[12], workspace=p[13], workspace_bytes=ws_bytes, stream=None)
        a.update(over)
        return lib.isg_subgraph_cut(*a.values())

    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
    for name in ("node_mask", "edge_index", "batch", "ptr", "node_new", "edge_new", "node_id", "edge_id", "edge_index_out",
                 "batch_out", "ptr_out", "sel", "counts"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("N", "E", "B", "table_k"):
        assert call(**{name: -1}) == EINVAL, name
    assert call(N=2 ** 31) == EUNSUPPORTED and call(E=2 ** 31) == EUNSUPPORTED and call(B=2 ** 31) == EUNSUPPORTED
    assert call(B=2 ** 30, table_k=4) == EUNSUPPORTED
    assert call(workspace=None) == EWORKSPACE and call(workspace_bytes=ws_bytes - 1) == EWORKSPACE


def test_subgraph_cut_fails_loudly_on_cpu_tensors():
    from isubgvqa_amd import _lib, ops
    mask, ei, batch = _known()
    ptr = torch.tensor([0, 3, 3, 7, 7], dtype=torch.int32)
    plan = ops.GraphPlan(N=7, E=10, B=4, ptr=ptr, nmax_dev=torch.zeros(1, dtype=torch.int32), nmax=4, emax=6, batch=batch,
                         edge_index=ei)
    with pytest.raises(_lib.IsgError, match="no CPU fallback"):
        ops.subgraph_cut(mask, ei, plan)
    with pytest.raises(_lib.IsgError, match="no CPU fallback"):
        ops.subgraph_cut(mask.view(-1, 1), ei, plan, complement=True, table_k=2)


def test_fidelity_scores_on_a_known_answer():
    from isubgvqa_amd import explain
    l2, l3, l4 = math.log(2.0), math.log(3.0), math.log(4.0)
    logits = torch.tensor([[l2, 0.0, 0.0], [0.0, l3, 0.0], [0.0, 0.0, l2]])           # p of the prediction: 1/2, 3/5, 1/2
    keep = torch.tensor([[l2, 0.0, 0.0], [0.0, 0.0, l3], [l4, 0.0, l4 + l2]])         # of that class: 1/2, 1/5, 8/13
    removed = torch.tensor([[0.0, l3, 0.0], [0.0, l3, 0.0], [0.0, 0.0, 0.0]])         # 1/5, 3/5, 1/3
    emptied = torch.tensor([False, True, False])
    f = explain.fidelity_scores(logits, keep, removed, emptied)
    assert f.pred.tolist() == [0, 1, 2]
    close = lambda t, v: torch.allclose(t, torch.tensor(v), rtol=0, atol=1e-6)
    assert close(f.p, [0.5, 0.6, 0.5]) and close(f.p_keep, [0.5, 0.2, 8 / 13]) and close(f.p_removed, [0.2, 0.6, 1 / 3])
    assert close(f.fid_minus, [0.0, 0.4, 0.5 - 8 / 13])
    assert f.emptied.tolist() == [False, True, False]
    assert math.isnan(f.fid_plus[1].item()) and close(f.fid_plus[[0, 2]], [0.3, 0.5 - 1 / 3])


def test_subgraph_cut_views_and_the_explain_helpers_on_host_tensors():
    """SubgraphCut's trimmed views, gathers and position remap, and explain.cut_workload / cut_scene_graphs, are plain indexing: on a
    SubgraphCut filled from the restatement they can be held to the known answer without a GPU."""
    import argparse
    from isubgvqa_amd import explain, ops, synthetic
    mask, ei, batch = _known()
    r = restate(mask, ei, batch, 4, table_k=2)
    N, E = 7, 10
    pad = lambda t, n: torch.cat([t, torch.full((n - t.size(-1),), -5, dtype=t.dtype)])
    parent = ops.GraphPlan(N=N, E=E, B=4, ptr=torch.tensor([0, 3, 3, 7, 7], dtype=torch.int32),
                           nmax_dev=torch.zeros(1, dtype=torch.int32), nmax=4, emax=6, batch=batch, edge_index=ei)
    cut = ops.SubgraphCut(parent, r.node_new, r.edge_new, pad(r.node_id, N), pad(r.edge_id, E),
                          torch.stack([pad(r.edge_index[0], E), pad(r.edge_index[1], E)]), pad(r.batch, N), r.ptr, r.sel,
                          torch.tensor(r.counts, dtype=torch.int32))
    assert cut.sizes() == (4, 6)
    assert cut.node_id.tolist() == [0, 2, 4, 6] and cut.edge_id.tolist() == [0, 1, 3, 4, 5, 6] and cut.batch.tolist() == [0, 0, 2, 2]
    assert cut.edge_index.tolist() == [[0, 1, 1, 2, 3, 3], [1, 0, 1, 3, 2, 3]] and cut.edge_index.is_contiguous()
    rows = torch.arange(N * 2.0).view(N, 2)
    assert cut.gather_nodes(rows).tolist() == rows[[0, 2, 4, 6]].tolist()
    assert cut.gather_edges(torch.arange(E)).tolist() == [0, 1, 3, 4, 5, 6]
    # global edge positions (duplicates stay, cut edges and positions beyond the list go)
    assert cut.remap_edge_positions(torch.tensor([6, 2, 0, 0, 9, 12, 3])).tolist() == [5, 0, 0, 2]
    wl = synthetic.Workload(rows, ei, torch.arange(E * 3.0).view(E, 3), batch, torch.zeros(3, 4, 2), torch.ones(4, 2), 4, 4, 6,
                            torch.zeros(2, 4, dtype=torch.long))
    sub = explain.cut_workload(wl, cut)
    assert torch.equal(sub.x, rows[[0, 2, 4, 6]]) and torch.equal(sub.edge_attr, wl.edge_attr[[0, 1, 3, 4, 5, 6]])
    assert torch.equal(sub.edge_index, cut.edge_index) and torch.equal(sub.batch, cut.batch)
    assert sub.instr is wl.instr and sub.glf is wl.glf and (sub.num_graphs, sub.max_nodes, sub.max_edges) == (4, 4, 6)
    assert sub.graph_sizes is None
    sg = argparse.Namespace(x_bbox=torch.arange(N * 4).view(N, 4), added_sym_edge=torch.tensor([3, 2, 6]), max_nodes=4, max_edges=6,
                            graph_sizes=wl.graph_sizes)
    x2, ei2, ea2, b2, sg2 = explain.cut_scene_graphs(rows, torch.arange(E), sg, cut)
    assert torch.equal(x2, sub.x) and torch.equal(ei2, cut.edge_index) and ea2.tolist() == [0, 1, 3, 4, 5, 6] and torch.equal(b2, cut.batch)
    assert torch.equal(sg2.x_bbox, sg.x_bbox[[0, 2, 4, 6]]) and sg2.added_sym_edge.tolist() == [2, 5]
    assert (sg2.max_nodes, sg2.max_edges) == (4, 6) and not hasattr(sg2, "graph_sizes")
