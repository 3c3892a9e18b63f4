"""Host-side checks of training through shared scene encodings (include/ext/isg_instances_train.h) that need no GPU:
the extension header, its binding and the two libraries agree, and the table of device headers did not move; the entry point
refuses bad arguments before any launch; GraphInstances.by_graph / counts on indices written out by hand; the weighted BatchNorm
against torch's module on the rows physically repeated, in float64; the SyncBatchNorm refusal; GroupedBatchSampler; the refusals
of encode_scene / ask in train() stand."""
import argparse
import ctypes
import glob
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_instances_train_abi_version", "isg_instance_rows_bwd"}
HEADERS = ["isg.h", "isg_train.h", "isg_optim.h", "isg_fused.h", "isg_sgenc_train.h", "isg_dist.h", "isg_linear_train.h", "isg_masked.h",
           "isg_sampler_train.h", "isg_topk_rows.h", "isg_mp_train.h", "isg_sparse_out.h", "isg_mp_f16_train.h", "isg_concat.h",
           "isg_instances.h", "isg_eval.h", "isg_grounding.h"]


def test_extension_header_binding_and_libraries_agree_and_the_table_did_not_move():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_instances_train as X
    from isubgvqa_amd import _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_instances_train.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_INSTANCES_TRAIN_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_instances_train_abi_version() == X.ABI_VERSION == abi == 1
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    # (g_xo, ldgx, xo_rows, d_x, lddx, x_rows, Cx, g_eo, ldge, eo_rows, d_e, ldde, e_rows, Ce, ptr, erange, inst_ptr, inst_eptr,
    #  gptr, glist, G, Q, stream)
    sig = (ctypes.c_int, [ptr, i32, i64, ptr, i32, i64, i32, ptr, i32, i64, ptr, i32, i64, i32, ptr, ptr, ptr, ptr, ptr, ptr, i64, i64, ptr])
    assert X.SIGNATURES["isg_instance_rows_bwd"] == sig
    fn = lib.isg_instance_rows_bwd
    assert (fn.restype, list(fn.argtypes)) == sig
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export both symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_instances_train_abi_version.restype = ctypes.c_int
        assert raw.isg_instances_train_abi_version() == 1, other
    # a handle swapped in through _lib._lib is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_instance_rows_bwd.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_instance_rows_bwd.argtypes) == sig[1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="instance-training ABI version 2, binding expects 1"):
            X.load()
    # the table of device headers, the pinned directory and the _lib_<name> modules are what they were
    assert list(_lib.HEADERS) == HEADERS and _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "isg*.h")))
    assert on_disk == sorted(HEADERS + ["isg_loader.h", "isg_loader_objects.h"])
    mods = sorted(os.path.basename(p) for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_lib_*.py")))
    assert mods == sorted("_lib" + h[len("isg"):-2] + ".py" for h in HEADERS[1:])
    assert not NAMES & set(_lib._declared_in)
    # the build checks the version, the smoke run has its case, the counter exists, the kernel uses no atomic
    build_checks("isg_instances_train.h")
    assert "isg_instances_train_abi_version()" in inspect.getsource(ge._smoke_graph_instances)
    assert ops.COUNTERS["instance_rows_bwd"] >= 0 and "instance_rows_bwd" not in {f.name for f in __import__("dataclasses").fields(ops.Switches)}
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_instances_bwd.hip")).read())
    assert "atomic" not in text.lower() and "add_rn(" in text


def test_instance_rows_bwd_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_instances_train as X
    fn = X.load().isg_instance_rows_bwd

    def call(gx=P, ldgx=300, xor_=50, dx=P, lddx=300, xr=10, Cx=300, ge_=P, ldge=300, eor=90, de=P, ldde=300, er=20, Ce=300,
             ptr=P, erange=P, iptr=P, ieptr=P, gptr=P, glist=P, G=3, Q=5):
        return fn(gx, ldgx, xor_, dx, lddx, xr, Cx, ge_, ldge, eor, de, ldde, er, Ce, ptr, erange, iptr, ieptr, gptr, glist, G, Q, None)

    for k in ("gx", "dx", "ge_", "de", "ptr", "erange", "iptr", "ieptr", "gptr", "glist"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("xor_", "xr", "eor", "er", "G", "Q"):
        assert call(**{k: -1}) == EINVAL, k
        assert call(**{k: 1 << 31}) == EUNSUPPORTED, k
        assert call(**{k: (1 << 31) - 1024}) == EUNSUPPORTED, k
    assert call(G=0) == EINVAL                                  # rows of no graph
    for k in ("Cx", "Ce"):
        assert call(**{k: 0}) == EINVAL and call(**{k: -4}) == EINVAL, k
    for k in ("ldgx", "lddx", "ldge", "ldde"):
        assert call(**{k: 296}) == EINVAL, k                    # a stride below the width
        assert call(**{k: 302}) == EUNSUPPORTED, k              # no multiple of 4
    assert call(Cx=298, ldgx=304, lddx=304) == EUNSUPPORTED and call(Ce=2, ldge=4, ldde=4) == EUNSUPPORTED
    for k in ("gx", "dx", "ge_", "de"):
        assert call(**{k: P + 4}) == EUNSUPPORTED and call(**{k: P + 8}) == EUNSUPPORTED, k
    # nothing to do: nothing is looked at beyond the numbers; a half without rows comes without its pointers
    none = dict(gx=None, dx=None, ge_=None, de=None, ptr=None, erange=None, iptr=None, ieptr=None, gptr=None, glist=None)
    assert call(xr=0, er=0) == 0 and call(xr=0, er=0, Cx=0, Ce=0, G=0, Q=0, **none) == 0
    assert call(xr=0, er=0, xor_=-1) == EINVAL
    assert call(xr=0, gx=None, dx=None, ptr=None, iptr=None, Cx=0, er=0) == 0
    assert call(xr=0, gx=None, dx=None, ptr=None, iptr=None, Cx=0, de=None) == EINVAL       # the other half still has rows


def _instances(index, G, host=True):
    from isubgvqa_amd import ops
    index = torch.as_tensor(index, dtype=torch.int64)
    Q = index.numel()
    z = torch.zeros(0, dtype=torch.int64)
    return ops.GraphInstances(argparse.Namespace(B=G, N=0, E=0), index.int(), torch.zeros(Q + 1, dtype=torch.int32),
                              torch.zeros(Q + 1, dtype=torch.int32), z, z.view(2, 0), z, z, torch.zeros(4, dtype=torch.int32),
                              index_host=index if host else None)


@pytest.mark.parametrize("host", [True, False], ids=["host-index", "sorted-index"])
def test_by_graph_and_counts_on_indices_written_out_by_hand(host):
    inst = _instances([2, 0, 3, 2, 0, 2], 5, host)              # graphs 1 and 4 are never asked
    gptr, glist = inst.by_graph()
    assert gptr.dtype == glist.dtype == torch.int32 and inst.counts().dtype == torch.int32
    assert gptr.tolist() == [0, 2, 2, 5, 6, 6] and glist.tolist() == [1, 4, 0, 3, 5, 2]
    assert inst.counts().tolist() == [2, 0, 3, 1, 0]
    assert inst.by_graph()[0] is gptr and inst.by_graph()[1] is glist, "by_graph() is cached on the object"
    same = _instances([1] * 7, 3, host)                         # every question asks the same graph
    assert [t.tolist() for t in same.by_graph()] == [[0, 0, 7, 7], list(range(7))] and same.counts().tolist() == [0, 7, 0]
    one = _instances([0], 1, host)
    assert [t.tolist() for t in one.by_graph()] == [[0, 1], [0]]
    none = _instances([], 2, host)
    assert [t.tolist() for t in none.by_graph()] == [[0, 0, 0], []] and none.counts().tolist() == [0, 0]
    bad = _instances([1, 7, 0, -1, 1], 2, False)                # an index outside [0, G) belongs to no graph
    assert bad.by_graph()[0].tolist() == [0, 1, 3] and bad.by_graph()[1].tolist()[:3] == [2, 0, 4] and bad.counts().tolist() == [1, 2]


# ---- the weighted BatchNorm -----------------------------------------------------------------------------------------------------
def _bn_pair(C, momentum, seed):
    torch.manual_seed(seed)
    a = torch.nn.BatchNorm1d(C, momentum=momentum).double().train()
    with torch.no_grad():
        a.weight.uniform_(0.5, 1.5)
        a.bias.uniform_(-0.5, 0.5)
        a.running_mean.normal_()
        a.running_var.uniform_(0.5, 1.5)
    b = torch.nn.BatchNorm1d(C, momentum=momentum).double().train()
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("momentum", [0.1, None], ids=["momentum0.1", "cumulative"])
@pytest.mark.parametrize("C", [4, 16, 332])
def test_weighted_batch_norm_equals_the_module_on_the_rows_repeated(C, momentum):
    """Outputs, input gradients, weight / bias gradients and both running buffers against torch.nn.BatchNorm1d applied to the rows
    physically repeated, float64, within 1e-12; weights 0, 1 and 5 mixed; two steps, so that the cumulative average (momentum=None)
    is used at 1 / 1 and 1 / 2."""
    from isubgvqa_amd.models.scene_graph_encoder import weighted_batch_norm
    gen = torch.Generator().manual_seed(C)
    w = torch.tensor([1, 5, 0, 1, 0, 5, 5, 1, 1, 0, 5, 1, 1], dtype=torch.int32)
    N = w.numel()
    rows = torch.repeat_interleave(torch.arange(N), w.long())   # the repeated batch: row n w[n] times
    assert rows.numel() == 26 and set(w.tolist()) == {0, 1, 5}
    ours, ref = _bn_pair(C, momentum, seed=C)
    for step in range(2):
        x0 = torch.randn(N, C, generator=gen, dtype=torch.float64) * 2 + 0.5
        coef = torch.randn(rows.numel(), C, generator=gen, dtype=torch.float64)
        x, xr = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        y = weighted_batch_norm(ours, x, w)
        yr = ref(xr[rows])
        (y[rows] * coef).sum().backward()
        (yr * coef).sum().backward()
        worst = lambda a, b: float((a.detach() - b.detach()).abs().max())
        assert worst(y[rows], yr) < 1e-12
        assert worst(x.grad, xr.grad) < 1e-12
        assert float(x.grad[w == 0].abs().max()) == 0.0, "a row of weight 0 takes no part in the statistics"
        assert worst(ours.weight.grad, ref.weight.grad) < 1e-12 and worst(ours.bias.grad, ref.bias.grad) < 1e-12
        assert worst(ours.running_mean, ref.running_mean) < 1e-12 and worst(ours.running_var, ref.running_var) < 1e-12
        assert int(ours.num_batches_tracked) == int(ref.num_batches_tracked) == step + 1
        ours.zero_grad(), ref.zero_grad()
    # equal weights: the plain module on the rows as they are
    ours, ref = _bn_pair(C, momentum, seed=C + 1)
    x0 = torch.randn(N, C, generator=gen, dtype=torch.float64)
    assert float((weighted_batch_norm(ours, x0, torch.full((N,), 3, dtype=torch.int32)) - ref(x0)).abs().max()) < 1e-12
    assert float((ours.running_mean - ref.running_mean).abs().max()) < 1e-12


def _small_batch():
    batch = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2])
    return argparse.Namespace(batch=batch, x_bbox=torch.randint(0, 640, (9, 4), generator=torch.Generator().manual_seed(1)),
                              added_sym_edge=torch.zeros(0, dtype=torch.long))


def test_encoder_takes_a_multiplicity_by_keyword_only_and_refuses_it_with_sync_batch_norm():
    from isubgvqa_amd.models.scene_graph_encoder import SceneGraphEncoder
    params = inspect.signature(SceneGraphEncoder.forward).parameters
    assert list(params) == ["self", "x", "edge_index", "edge_attr", "batch", "explainer", "explainer_stage", "gt_scene_graphs", "plan",
                            "multiplicity"]
    assert params["multiplicity"].kind is inspect.Parameter.KEYWORD_ONLY and params["multiplicity"].default is None
    enc = SceneGraphEncoder(300, dist=True, vocab_size=23)
    assert isinstance(enc.bbox_encoding[0], torch.nn.SyncBatchNorm)
    b = _small_batch()
    for mode in (True, False):
        enc.train(mode)
        with pytest.raises(ValueError, match="SyncBatchNorm"):
            enc(torch.zeros(9, 300), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, dtype=torch.long), b.batch, explainer=True,
                explainer_stage=0, gt_scene_graphs=b, multiplicity=torch.tensor([2, 0, 1], dtype=torch.int32))


# ---- GroupedBatchSampler --------------------------------------------------------------------------------------------------------
def _image_ids(seed=0, images=37):
    gen = torch.Generator().manual_seed(seed)
    counts = torch.randint(1, 9, (images,), generator=gen).tolist()
    counts[3], counts[20] = 31, 12                              # 31 = 12 + 12 + 7: two full groups and a leftover; exactly one full group
    ids = [f"img{i}" for i, c in enumerate(counts) for _ in range(c)]
    return [ids[j] for j in torch.randperm(len(ids), generator=gen).tolist()], counts


@pytest.mark.parametrize("drop_last", [False, True])
def test_grouped_batch_sampler_partitions_the_questions_and_keeps_the_cap(drop_last):
    from isubgvqa_amd.datasets import GroupedBatchSampler
    ids, counts = _image_ids()
    sampler = GroupedBatchSampler(ids, images_per_batch=5, questions_per_image=12, seed=3, drop_last=drop_last)
    epochs = []
    for epoch in range(3):
        sampler.set_epoch(epoch)
        batches = list(sampler)
        assert len(batches) == len(sampler) and batches == list(sampler), "an epoch is the same list every time it is asked for"
        seen = sorted(i for b in batches for i in b)
        groups = 0
        for b in batches:
            per_image = {}
            for i in b:
                per_image[ids[i]] = per_image.get(ids[i], 0) + 1
            assert 1 <= len(per_image) <= 5 and max(per_image.values()) <= 12, per_image
            assert not drop_last or len(per_image) == 5
            groups += len(per_image)
        if drop_last:
            assert len(set(seen)) == len(seen) and len(seen) <= len(ids)
        else:
            assert seen == list(range(len(ids))), "every question exactly once per epoch"
            assert groups == sum(-(-c // 12) for c in counts)   # the leftover groups are groups of their own: image 3 comes thrice
            assert sum(1 for b in batches if any(ids[i] == "img3" for i in b)) == 3
        epochs.append(batches)
    assert epochs[0] != epochs[1] and epochs[1] != epochs[2]
    again = GroupedBatchSampler(ids, 5, 12, seed=3, drop_last=drop_last)
    again.set_epoch(1)
    assert list(again) == epochs[1], "the same (seed, epoch) gives the same batches"
    assert list(GroupedBatchSampler(ids, 5, 12, seed=4, drop_last=drop_last)) != epochs[0]
    # a cap of one question per image: no batch repeats a graph; one image per batch: every batch is one group
    single = list(GroupedBatchSampler(ids, 4, 1, seed=0))
    assert all(len({ids[i] for i in b}) == len(b) for b in single) and sorted(i for b in single for i in b) == list(range(len(ids)))
    alone = list(GroupedBatchSampler(ids, 1, 12, seed=0))
    assert all(len({ids[i] for i in b}) == 1 and len(b) <= 12 for b in alone) and len(alone) == sum(-(-c // 12) for c in counts)
    with pytest.raises(ValueError):
        GroupedBatchSampler(ids, 0, 12, seed=0)


def test_shared_scenes_passes_the_step_counters_through():
    from isubgvqa_amd import train

    class Inner(torch.nn.Module):
        n_train_steps, n_valid_steps = 3, 4

        def forward_shared(self, **inputs):
            return (inputs["a"] + 1, "mask", "gate", [], None), "instances"

    inner = Inner()
    shared = train.SharedScenes(inner)
    shared.n_train_steps += 5
    shared.n_valid_steps = 9
    assert (inner.n_train_steps, inner.n_valid_steps, shared.n_train_steps) == (8, 9, 8)
    assert shared(a=1) == (2, "mask", "gate", [], None)
    assert shared.eval() is shared and not inner.training


def test_encode_scene_and_ask_still_refuse_train_and_forward_shared_has_its_signature():
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.models import build_model
    from isubgvqa_amd.models.isubgvqa import SceneState
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(sg_vocab_size=64, text_vocab_size=64), None).train()
    wl = synthetic.make_shared_workload(2, 2, tokens=4, sg_vocab=64, text_vocab=64)
    state = SceneState(torch.zeros(wl.x.size(0), 300), torch.zeros(wl.edge_index.size(1), 300), wl.edge_index, None, wl.graph_sizes)
    with pytest.raises(ValueError, match="BatchNorm"):
        model.encode_scene(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.scene_graphs())
    with pytest.raises(ValueError, match="inference form"):
        model.ask(state, wl.questions, wl.att_mask, wl.graph_index)
    assert list(inspect.signature(model.forward_shared).parameters) == [
        "node_embeddings", "edge_index", "edge_embeddings", "batch", "questions", "qsts_att_mask", "graph_index", "scene_graphs",
        "noises", "seed", "plan", "text_uniform"]
    assert list(inspect.signature(model.forward).parameters) == [
        "node_embeddings", "edge_index", "edge_embeddings", "batch", "questions", "qsts_att_mask", "return_masks", "explainer",
        "explainer_stage", "expl_bypass_x", "scene_graphs", "noises", "seed", "plan", "text_uniform", "capture"]
