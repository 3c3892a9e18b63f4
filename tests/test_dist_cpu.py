"""Host-side checks of data-parallel training (include/isg_dist.h, distributed.GradSync's layout and mask agreement,
train.Meters.report(group)) that need no GPU: the header binds and both libraries export it, isg_mt_pack refuses what its
comment says before it touches a device, the bucket's slots are aligned and disjoint, and on a gloo group of two ranks the
parameter masks are united and the meters summed slot by slot."""
import ctypes
import inspect
import os
import re
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from binding_checks import build_checks
from conftest import ROOT


def test_dist_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_dist, _lib_fused, _lib_optim, _lib_sgenc_train, _lib_train
    header = open(os.path.join(ROOT, "include", "isg_dist.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_dist.SIGNATURES) == {"isg_dist_abi_version", "isg_mt_pack"}
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_dist.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_DIST_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_dist_abi_version() == _lib_dist.ABI_VERSION == abi == 1
    assert (_lib.ABI_VERSION, _lib_optim.ABI_VERSION) == (23, 1) and len(_lib.SIGNATURES) == 74      # the other headers did not move
    res, args = _lib_dist.SIGNATURES["isg_mt_pack"]
    P = ctypes.c_void_p
    assert res is ctypes.c_int and args == [P, P, P, P, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_int32, P]
    build_checks("isg_dist.h")
    assert os.path.exists(os.path.join(ge.CSRC, "isg_dist.hip"))


def test_pack_refuses_bad_arguments_before_any_launch():
    """The refusals and the empty table return before the device is touched, so they hold here as on the GPU."""
    from isubgvqa_amd import _lib_dist
    lib = _lib_dist.load()
    EINVAL, p = -1, 4096                                   # p: any non-null address; nothing dereferences it on these paths
    assert lib.isg_mt_pack(None, None, None, None, 0, 0, 1.0, 0, None) == 0              # T = 0: nothing to do
    assert lib.isg_mt_pack(p, p, p, p, 3, 0, 1.0, 1, None) == 0                           # three empty tensors: no chunk, no launch
    assert lib.isg_mt_pack(p, p, p, p, -1, 0, 1.0, 0, None) == EINVAL
    assert lib.isg_mt_pack(p, p, p, p, 1, -1, 1.0, 0, None) == EINVAL
    assert lib.isg_mt_pack(p, p, p, p, 0, 2, 1.0, 0, None) == EINVAL                      # chunks without tensors
    for hole in range(4):
        arrays = [None if i == hole else p for i in range(4)]
        assert lib.isg_mt_pack(*arrays, 1, 1, 1.0, 0, None) == EINVAL, f"null array {hole} with T = 1"
        assert lib.isg_mt_pack(*arrays, 1, 0, 1.0, 0, None) == EINVAL


def test_bucket_layout_aligns_every_slot_and_overlaps_nothing():
    from isubgvqa_amd.distributed import bucket_layout
    numels = [0, 1, 63, 64, 65, 4096, 4097]
    offsets, total = bucket_layout(numels)
    assert offsets == [0, 0, 64, 128, 192, 320, 4416] and total == 4416 + 4160
    assert all(o % 64 == 0 for o in offsets) and total % 64 == 0
    end = 0
    for o, n in zip(offsets, numels):                       # in order, disjoint, inside the bucket
        assert o >= end
        end = o + n
    assert end <= total and total - end < 64
    assert bucket_layout([]) == ([], 0) and bucket_layout([0, 0]) == ([0, 0], 0)
    assert bucket_layout([5, 3], align=4) == ([0, 8], 12) and bucket_layout([5, 3], align=1) == ([0, 5], 8)
    for sizes in ([64] * 3, [1] * 5, [127, 129]):
        offs, tot = bucket_layout(sizes)
        assert offs == [sum((s + 63) // 64 * 64 for s in sizes[:i]) for i in range(len(sizes))]
        assert tot == sum((s + 63) // 64 * 64 for s in sizes)
    with pytest.raises(ValueError):
        bucket_layout([3, -1])


def test_grad_sync_and_train_step_signatures():
    from isubgvqa_amd import distributed, optim, train
    sig = inspect.signature(distributed.GradSync.__init__)
    assert list(sig.parameters)[1:6] == ["params", "group", "world", "all_reduce", "force"]
    assert [sig.parameters[k].default for k in ("group", "world", "all_reduce", "force")] == [None, None, None, False]
    assert inspect.signature(optim.Adam.__init__).parameters["grad_sync"].default is None
    sig = inspect.signature(train.train_step)
    assert [(k, sig.parameters[k].default) for k in ("sync", "accumulate", "micro")] == [("sync", None), ("accumulate", 1), ("micro", 0)]
    assert inspect.signature(train.validate).parameters["group"].default is None
    assert inspect.signature(train.Meters.report).parameters["group"].default is None
    with pytest.raises(ValueError, match="accumulate > 1"):          # refused before the model is touched
        train.train_step(None, None, None, torch.zeros(2), None, accumulate=2, micro=1)
    with pytest.raises(ValueError, match="micro-batch 2 of 2"):
        train.train_step(None, None, None, torch.zeros(2), None, accumulate=2, micro=2)
    w = torch.nn.Parameter(torch.zeros(5, 3))
    from isubgvqa_amd import _lib
    with pytest.raises(_lib.IsgError, match=r"GradSync: parameter 'head.weight' lives on cpu"):
        distributed.GradSync([("head.weight", w)])


def test_shard_workload_cuts_the_full_models_workload_by_graph():
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.distributed import shard_workload
    wl = synthetic.make_full_workload(10, tokens=6, text_vocab=500, sg_vocab=100)
    parts = [shard_workload(wl, r, 3) for r in range(3)]
    assert [p.questions.size(0) for p in parts] == [4, 4, 2]
    for name in ("x", "x_bbox", "edge_attr", "questions", "att_mask", "added_sym_edge"):
        assert torch.equal(torch.cat([getattr(p, name) for p in parts]), getattr(wl, name)), name
    assert torch.equal(torch.cat([p.graph_sizes for p in parts], dim=1), wl.graph_sizes)
    node0 = 0
    for p in parts:
        assert p.batch.min() == 0 and int(p.batch.max()) == p.questions.size(0) - 1
        assert p.edge_index.min() >= 0 and p.edge_index.max() < p.x.size(0)
        assert p.max_nodes == int(p.graph_sizes[0].max()) and p.max_edges == int(p.graph_sizes[1].max())
        assert torch.equal(p.graph_sizes[0], torch.bincount(p.batch)) and p.graph_sizes.device.type == "cpu"
        node0 += p.x.size(0)
    assert node0 == wl.x.size(0)
    assert torch.equal(torch.cat([p.edge_index + o for p, o in zip(parts, [0, parts[0].x.size(0), parts[0].x.size(0) + parts[1].x.size(0)])],
                                 dim=1), wl.edge_index)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


MASKS = ([True, False, False, True, False, True, False], [False, False, True, True, False, False, False])
TOTALS = ([10.5, 4.0, 3.0, 4.0, 2.0, 1.0, 1.0, 0.0], [7.25, 8.0, 5.0, 12.0, 2.0, 0.0, 1.0, 0.0])


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from isubgvqa_amd import train
    from isubgvqa_amd.distributed import union_mask
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    union = union_mask(MASKS[rank], dist.group.WORLD)
    sub = union_mask(MASKS[rank], dist.new_group([0, 1]))
    empty = union_mask([], dist.group.WORLD)
    m = train.Meters("cpu")
    m.totals.copy_(torch.tensor(TOTALS[rank], dtype=torch.float64))
    local, summed = m.report(), m.report(dist.group.WORLD)
    kept = m.totals.tolist()
    q.put((rank, union, sub, empty, local, summed, kept))
    dist.barrier()
    dist.destroy_process_group()


def test_masks_are_united_and_meters_summed_over_a_gloo_group_of_two():
    from isubgvqa_amd import train
    from isubgvqa_amd.distributed import union_mask
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want_union = [a or b for a, b in zip(*MASKS)]
    assert want_union == [True, False, True, True, False, True, False]
    a, b = TOTALS
    mixed = [[a[i] + b[i] if i in (0, 1, 2, 3, 5) else t[i] for i in range(8)] for t in TOTALS]     # slots 4 and 6 stay local
    for rank, union, sub, empty, local, summed, kept in got:
        assert union == want_union and sub == want_union and empty == []
        assert local == train.Meters.summarize(TOTALS[rank])
        assert summed == train.Meters.summarize(mixed[rank])
        assert kept == TOTALS[rank], "report(group) changed the rank's own totals"
    s0 = got[0][5]
    assert s0["loss"] == (10.5 + 7.25) / 12.0 and s0["acc1"] == 100.0 * 8.0 / 16.0 and s0["rows"] == 16
    assert (s0["steps"], s0["skipped_steps"], s0["nonfinite_losses"]) == (2, 1, 1)
    assert union_mask(MASKS[0]) == list(MASKS[0])            # no process group: the mask as it is
