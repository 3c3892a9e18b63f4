"""Host-side checks of the graph-instance expansion (include/isg_instances.h) that need no GPU: the header declares
exactly the new entry points and shares none with another header; header, library, strict twin and binding agree on the version;
the entry points refuse bad arguments before anything is dereferenced; the restatement of tests/instances_restated.py on a case
written out by hand; SceneGraphStore.collate(distinct=True); the refusals of ISubGVQA.encode_scene / ask; the shared workload."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT, load_golden

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_instances_abi_version", "isg_instances_workspace_bytes", "isg_instances_size", "isg_instances_fill",
         "isg_instance_rows"}


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_instances_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_concat, _lib_dist, _lib_fused, _lib_instances, _lib_linear_train, _lib_masked,
                              _lib_mp_f16_train, _lib_mp_train, _lib_optim, _lib_sampler_train, _lib_sgenc_train, _lib_sparse_out,
                              _lib_topk_rows, _lib_train, ops)
    header = open(os.path.join(ROOT, "include", "isg_instances.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", _strip(header)))
    assert declared == set(_lib_instances.SIGNATURES) == NAMES
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked,
              _lib_sampler_train, _lib_topk_rows, _lib_mp_train, _lib_sparse_out, _lib_mp_f16_train, _lib_concat]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_instances.load()
    abi = int(re.search(r"#define ISG_INSTANCES_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_instances_abi_version() == _lib_instances.ABI_VERSION == abi == 1
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_instances_abi_version.restype = ctypes.c_int
        assert raw.isg_instances_abi_version() == 1, other
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 13
    i32, i64, ptr, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    assert _lib_instances.SIGNATURES["isg_instances_workspace_bytes"] == (sz, [i64])
    # (ptr, batch, edge_index, index, N, E, G, Q, inst_ptr, inst_eptr, status, workspace, workspace_bytes, stream)
    assert _lib_instances.SIGNATURES["isg_instances_size"] == (
        ctypes.c_int, [ptr, ptr, ptr, ptr, i64, i64, i64, i64, ptr, ptr, ptr, ptr, sz, ptr])
    # (ptr, edge_index, index, N, E, G, Q, inst_ptr, inst_eptr, workspace, workspace_bytes, cap_nodes, cap_edges, batch_out,
    #  edge_index_out, node_src, edge_src, stream)
    assert _lib_instances.SIGNATURES["isg_instances_fill"] == (
        ctypes.c_int, [ptr, ptr, ptr, i64, i64, i64, i64, ptr, ptr, ptr, sz, i64, i64, ptr, ptr, ptr, ptr, ptr])
    # (x, ldx, x_rows, node_src, n_out, x_out, ldxo, Cx, e, lde, e_rows, edge_src, m_out, e_out, ldeo, Ce, stream)
    assert _lib_instances.SIGNATURES["isg_instance_rows"] == (
        ctypes.c_int, [ptr, i32, i64, ptr, i64, ptr, i32, i32, ptr, i32, i64, ptr, i64, ptr, i32, i32, ptr])
    build_checks("isg_instances.h")
    assert "_smoke_graph_instances(dev)" in inspect.getsource(ge.smoke)
    smoke = inspect.getsource(ge._smoke_graph_instances)
    assert "isg_instances_abi_version()" in smoke and "graph_instances(" in smoke
    assert "graph_instances" in ops.COUNTERS
    assert ops.INSTANCES_SCAN_BLOCK == 1024
    text = open(os.path.join(ge.CSRC, "isg_instances.hip")).read()
    assert re.search(r"INST_THREADS = 256, INST_PER = 4, INST_SCAN_BLOCK = INST_THREADS \* INST_PER", text)
    assert "atomic" not in re.sub(r"//[^\n]*", "", text).lower(), "the expansion uses no atomic"


def test_size_and_fill_refuse_bad_arguments_before_anything_is_dereferenced():
    from isubgvqa_amd import _lib_instances
    lib = _lib_instances.load()
    assert lib.isg_instances_workspace_bytes(3) == 16 and lib.isg_instances_workspace_bytes(0) == 4
    assert lib.isg_instances_workspace_bytes(-1) == 0

    def size(ptr=P, batch=P, ei=P, index=P, N=10, E=20, G=3, Q=5, iptr=P, ieptr=P, status=P, ws=P, wsb=16):
        return lib.isg_instances_size(ptr, batch, ei, index, N, E, G, Q, iptr, ieptr, status, ws, wsb, None)

    for k in ("ptr", "batch", "ei", "index", "iptr", "ieptr", "status"):
        assert size(**{k: None}) == EINVAL, k
    for k in ("N", "E", "G", "Q"):
        assert size(**{k: -1}) == EINVAL, k
        assert size(**{k: 1 << 31}) == EUNSUPPORTED, k
    assert size(G=0) == EINVAL                                  # questions about no graph
    assert size(ws=None) == EWORKSPACE and size(wsb=15) == EWORKSPACE
    assert size(Q=0) == 0 and size(Q=0, G=0) == 0
    assert size(Q=0, ptr=None, batch=None, ei=None, index=None, iptr=None, ieptr=None, status=None, ws=None, wsb=0) == 0
    assert size(Q=0, N=-1) == EINVAL

    def fill(ptr=P, ei=P, index=P, N=10, E=20, G=3, Q=5, iptr=P, ieptr=P, ws=P, wsb=16, cn=7, ce=9, bo=P, eo=P, ns=P, es=P):
        return lib.isg_instances_fill(ptr, ei, index, N, E, G, Q, iptr, ieptr, ws, wsb, cn, ce, bo, eo, ns, es, None)

    for k in ("ptr", "ei", "index", "iptr", "ieptr", "bo", "eo", "ns", "es"):
        assert fill(**{k: None}) == EINVAL, k
    for k in ("N", "E", "G", "Q", "cn", "ce"):
        assert fill(**{k: -1}) == EINVAL, k
        assert fill(**{k: 1 << 31}) == EUNSUPPORTED, k
    assert fill(G=0) == EINVAL
    assert fill(ws=None) == EWORKSPACE and fill(wsb=15) == EWORKSPACE
    assert fill(Q=0) == 0 and fill(Q=0, ptr=None, ei=None, index=None, iptr=None, ieptr=None, ws=None, bo=None, eo=None, ns=None,
                                   es=None) == 0
    assert fill(cn=0, ce=0, bo=None, eo=None, ns=None, es=None, ei=None) == 0       # nothing to write: nothing is launched


def test_instance_rows_refuses_bad_arguments_before_anything_is_dereferenced():
    from isubgvqa_amd import _lib_instances
    fn = _lib_instances.load().isg_instance_rows

    def call(x=P, ldx=300, xr=10, ns=P, n=7, xo=P, ldxo=300, Cx=300, e=P, lde=300, er=20, es=P, m=9, eo=P, ldeo=300, Ce=300):
        return fn(x, ldx, xr, ns, n, xo, ldxo, Cx, e, lde, er, es, m, eo, ldeo, Ce, None)

    for k in ("x", "ns", "xo", "e", "es", "eo"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("xr", "n", "er", "m"):
        assert call(**{k: -1}) == EINVAL, k
    assert call(Cx=0) == EINVAL and call(Ce=0) == EINVAL and call(ldx=296) == EINVAL and call(ldxo=296) == EINVAL
    assert call(lde=296) == EINVAL and call(ldeo=296) == EINVAL
    assert call(Cx=298, ldx=302) == EUNSUPPORTED and call(ldx=302) == EUNSUPPORTED and call(ldeo=302) == EUNSUPPORTED
    assert call(x=P + 4) == EUNSUPPORTED and call(eo=P + 8) == EUNSUPPORTED and call(n=1 << 31) == EUNSUPPORTED
    # nothing to do: nothing is looked at beyond the numbers; a half without rows may come without pointers
    assert call(n=0, m=0) == 0 and call(n=0, m=0, x=None, ns=None, xo=None, e=None, es=None, eo=None, Cx=0, Ce=0) == 0
    assert call(n=0, m=0, xr=-1) == EINVAL


def test_restatement_on_a_case_written_out_by_hand():
    """Three graphs -- 2 nodes / 2 edges, 0 nodes, 3 nodes / 1 self loop -- and five instances (2, 0, 1, 2, 0)."""
    import instances_restated as R
    batch = torch.tensor([0, 0, 2, 2, 2])
    ei = torch.tensor([[0, 1, 3], [1, 0, 3]])
    r = R.expand(batch, ei, torch.tensor([2, 0, 1, 2, 0]), 3)
    assert r.ptr.tolist() == [0, 3, 5, 5, 8, 10] and r.eptr.tolist() == [0, 1, 3, 3, 4, 6]
    assert r.batch.tolist() == [0, 0, 0, 1, 1, 3, 3, 3, 4, 4]
    assert r.node_src.tolist() == [2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    assert r.edge_src.tolist() == [2, 0, 1, 2, 0, 1]
    assert r.edge_index.tolist() == [[1, 3, 4, 6, 8, 9], [1, 4, 3, 6, 9, 8]]
    assert r.status.tolist() == [10, 6, 0, 0]
    assert r.ptr.dtype == r.eptr.dtype == r.status.dtype == torch.int32 and r.batch.dtype == r.edge_index.dtype == torch.int64
    # the flags
    assert R.expand(batch, ei, torch.tensor([2, 3, -1]), 3).status.tolist() == [3, 1, 1, 0]
    assert R.expand(batch, ei[:, [2, 0, 1]], torch.tensor([0]), 3).status[3] == 1
    assert R.expand(batch, torch.tensor([[0, 1, 3], [1, 2, 3]]), torch.tensor([0]), 3).status[3] == 1
    empty = R.expand(batch, ei, torch.zeros(0, dtype=torch.int64), 3)
    assert empty.ptr.tolist() == [0] and empty.status.tolist() == [0, 0, 0, 0] and tuple(empty.edge_index.shape) == (2, 0)


def test_collate_distinct_holds_every_graph_once_in_first_occurrence_order():
    from isubgvqa_amd import loader
    from isubgvqa_amd.datasets.gqa import gqa_collate
    g8 = load_golden("g8_loader.pt")
    keys = list(json.loads(g8["json"]))
    assert len(keys) >= 3
    a, b, c = keys[:3]
    ids = [b, "no-such-image", a, b, b, "another-unknown", c, a]
    distinct = [b, "no-such-image", a, c]                # both unknown ids share the one dummy graph
    store = loader.SceneGraphStore(loader.SceneGraphVocab(g8["token_lists"])).add_json(g8["json"])
    got, want = store.collate(ids, pin_memory=False, distinct=True), store.collate(distinct, pin_memory=False)
    for name in ("x", "edge_index", "edge_attr", "x_bbox", "added_sym_edge", "batch", "ptr"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert (got.num_graphs, got.max_nodes, got.max_edges) == (4, want.max_nodes, want.max_edges)
    assert got.graph_index.dtype == torch.int64 and got.graph_index.tolist() == [0, 1, 2, 0, 0, 1, 3, 2]
    assert [distinct[g] if distinct[g] in store else None for g in got.graph_index.tolist()] == [i if i in store else None for i in ids]
    # graph_sizes is always filled, and describes the batch
    assert got.graph_sizes is not None and got.graph_sizes.dtype == torch.int64 and tuple(got.graph_sizes.shape) == (2, 4)
    assert torch.equal(got.graph_sizes[0], torch.bincount(got.batch, minlength=4))
    assert torch.equal(got.graph_sizes[1], torch.bincount(got.batch[got.edge_index[1]], minlength=4))
    # by slots as by strings; the default is what it was
    by_slot = store.collate(store.slots(ids), pin_memory=False, distinct=True)
    assert torch.equal(by_slot.x, got.x) and torch.equal(by_slot.graph_index, got.graph_index)
    plain = store.collate(ids, pin_memory=False)
    assert plain.graph_index is None and plain.num_graphs == len(ids)
    moved = got.to("cpu")
    assert moved.graph_index is got.graph_index and moved.graph_sizes is got.graph_sizes
    assert inspect.signature(store.collate).parameters["distinct"].default is False
    # gqa_collate passes the flag through; the tuple keeps its arity
    data = [(f"q{i}", k, "what is it", "t", 0, k) for i, k in enumerate(ids)]
    out = gqa_collate(data, store, None, False, distinct=True)
    assert len(out) == 7 == len(gqa_collate(data, store, None, False))
    assert torch.equal(out[1].graph_index, got.graph_index) and torch.equal(out[1].x, got.x)
    assert gqa_collate(data, store, None, False)[1].graph_index is None


def test_encode_scene_and_ask_refuse_what_a_shared_encoding_cannot_do():
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.models import build_model
    from isubgvqa_amd.models.isubgvqa import SceneState
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(sg_vocab_size=64, text_vocab_size=64), None)
    wl = synthetic.make_shared_workload(2, 2, tokens=4, sg_vocab=64, text_vocab=64)
    state = SceneState(torch.zeros(wl.x.size(0), 300), torch.zeros(wl.edge_index.size(1), 300), wl.edge_index, None, wl.graph_sizes)
    model.train()
    with pytest.raises(ValueError, match="BatchNorm"):
        model.encode_scene(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.scene_graphs())
    with pytest.raises(ValueError, match="inference form"):
        model.ask(state, wl.questions, wl.att_mask, wl.graph_index)
    model.eval()
    with pytest.raises(ValueError, match="capture"):
        model.ask(state, wl.questions, wl.att_mask, wl.graph_index, capture=True)
    for kw in ({"explainer": True}, {"explainer_stage": 1}, {"expl_bypass_x": torch.zeros(1)}):
        with pytest.raises(ValueError, match="explainer"):
            model.ask(state, wl.questions, wl.att_mask, wl.graph_index, **kw)
    with pytest.raises(ValueError, match="questions"):
        model.ask(state, wl.questions[:3], wl.att_mask[:3], wl.graph_index)
    # forward stays as it is: none of the new names in its signature
    assert list(inspect.signature(model.forward).parameters) == [
        "node_embeddings", "edge_index", "edge_embeddings", "batch", "questions", "qsts_att_mask", "return_masks", "explainer",
        "explainer_stage", "expl_bypass_x", "scene_graphs", "noises", "seed", "plan", "text_uniform", "capture"]


def test_shared_workload_and_its_replicated_form():
    import instances_restated as R
    from isubgvqa_amd import explain, synthetic
    wl = synthetic.make_shared_workload(5, 3, tokens=6, seed=11, sizes=[3, 1, 17, 40, 8])
    G, Q = 5, 15
    assert wl.graph_index.dtype == torch.int64 and sorted(wl.graph_index.tolist()) == sorted(list(range(G)) * 3)
    assert wl.graph_index.tolist() != sorted(wl.graph_index.tolist())                  # the questions are not grouped by graph
    assert wl.questions.size(0) == wl.att_mask.size(0) == Q and tuple(wl.graph_sizes.shape) == (2, G)
    assert torch.bincount(wl.batch, minlength=G).tolist() == [3, 1, 17, 40, 8]
    assert wl.to("cpu").graph_index is wl.graph_index
    with pytest.raises(ValueError, match="Q6"):
        wl.replicated()
    wl.added_sym_edge = wl.added_sym_edge[:0]
    rep, r = wl.replicated(), R.expand(wl.batch, wl.edge_index, wl.graph_index, G)
    assert torch.equal(rep.batch, r.batch) and torch.equal(rep.edge_index, r.edge_index)
    assert torch.equal(rep.x, wl.x[r.node_src]) and torch.equal(rep.edge_attr, wl.edge_attr[r.edge_src])
    assert torch.equal(rep.x_bbox, wl.x_bbox[r.node_src]) and rep.graph_index is None and rep.questions is wl.questions
    assert torch.equal(rep.graph_sizes[0], (r.ptr[1:] - r.ptr[:-1]).long()) and torch.equal(rep.graph_sizes[1], (r.eptr[1:] - r.eptr[:-1]).long())
    assert explain.EvalBatch._field_defaults["graph_index"] is None and explain.EvalBatch._fields[-1] == "graph_index"
