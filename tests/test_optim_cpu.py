"""Host-side checks of the step's tail (include/isg_optim.h, optim.py, train.py) that need no GPU: the third device header binds
and both libraries export it, build() names it, the other two headers did not move, optim.Adam is torch's Adam with torch's state
layout and refuses what its kernels do not take, Meters weighs like the reference's AverageMeter, and the host's chunk prefix
agrees with the chunk size the library reports."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT


def test_optim_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_optim, _lib_train
    header = open(os.path.join(ROOT, "include", "isg_optim.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_optim.SIGNATURES), declared ^ set(_lib_optim.SIGNATURES)
    assert declared == {"isg_optim_abi_version", "isg_xent_fwd", "isg_xent_bwd", "isg_mt_chunk_elems", "isg_mt_sqnorm_parts",
                        "isg_mt_sqnorm", "isg_mt_adam"}
    assert not declared & (set(_lib.SIGNATURES) | set(_lib_train.SIGNATURES)), "a symbol is declared in two headers"
    lib = _lib_optim.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_OPTIM_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_optim_abi_version() == _lib_optim.ABI_VERSION == abi == 1
    assert (_lib.ABI_VERSION, _lib_train.ABI_VERSION) == (23, 1)          # the other two headers did not move
    # argument marshalling of the longest declaration: pointers, the counts, then the host scalars in double
    res, args = _lib_optim.SIGNATURES["isg_mt_adam"]
    assert res is ctypes.c_int and len(args) == 17
    assert args[3:5] == [ctypes.c_int32, ctypes.c_int64] and args[9] is ctypes.c_int32 and args[10:15] == [ctypes.c_double] * 5
    res, args = _lib_optim.SIGNATURES["isg_xent_fwd"]
    assert len(args) == 13 and args[3] is ctypes.c_int64 and args[-3:] == [ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    # the totals' slots as train.Meters reads them
    slots = dict(re.findall(r"#define (ISG_TOT_\w+) (\d)", header))
    assert [int(slots[k]) for k in ("ISG_TOT_LOSS_SUM", "ISG_TOT_LOSS_ROWS", "ISG_TOT_CORRECT", "ISG_TOT_ROWS", "ISG_TOT_CALLS",
                                    "ISG_TOT_NONFINITE", "ISG_TOT_SKIPPED")] == list(range(7))


def test_build_names_the_header_in_its_staleness_list_and_its_check():
    import __graft_entry__ as ge
    build_checks("isg_optim.h")
    assert os.path.exists(os.path.join(ge.CSRC, "isg_optim.hip"))


def test_host_only_entry_points_and_the_chunk_prefix():
    from isubgvqa_amd import _lib_optim, optim
    lib = _lib_optim.load()
    c = lib.isg_mt_chunk_elems()
    assert c > 0 and c % 1024 == 0          # whole float4 per lane of a 256-thread workgroup; a chunk never splits a 16-byte line
    assert [lib.isg_mt_sqnorm_parts(n) for n in (0, 1, 2, 7000)] == [1, 1, 2, 7000]
    numels = [0, 1, c - 1, c, c + 1]
    assert optim.chunk_prefix(numels, c) == [0, 0, 1, 2, 3, 5]
    assert optim.chunk_prefix([], c) == [0] and optim.chunk_prefix([2 * c + 5, 0, 3], c) == [0, 3, 3, 4]
    # every chunk lies inside its tensor and the chunks of a tensor cover it exactly once
    prefix = optim.chunk_prefix(numels, c)
    for t, n in enumerate(numels):
        spans = [(k * c, min(n, (k + 1) * c)) for k in range(prefix[t + 1] - prefix[t])]
        assert all(a < b for a, b in spans) and sum(b - a for a, b in spans) == n


def test_adam_is_torch_adam_and_refuses_what_the_kernels_do_not_take():
    from isubgvqa_amd import _lib, optim
    assert issubclass(optim.Adam, torch.optim.Adam)
    sig = inspect.signature(optim.Adam.__init__)
    assert list(sig.parameters)[1:9] == ["params", "lr", "betas", "eps", "weight_decay", "decoupled", "max_grad_norm", "skip_nonfinite"]
    assert sig.parameters["decoupled"].default is False and sig.parameters["max_grad_norm"].default is None
    assert sig.parameters["skip_nonfinite"].default is True
    w = torch.nn.Parameter(torch.zeros(5, 3))
    with pytest.raises(_lib.IsgError, match=r"parameter 0 of group 0 \(shape \(5, 3\)\) lives on cpu"):
        optim.Adam([w], lr=1e-3)
    # the dtype and layout refusals come before any kernel could see the tensor; the device check is taken out to reach them here
    real = optim._check_param
    try:
        optim._check_param = lambda p, name: real(_Cuda(p), name)
        with pytest.raises(TypeError, match=r"parameter 1 of group 0 \(shape \(7,\)\) is torch.float16"):
            optim.Adam([w, torch.nn.Parameter(torch.zeros(7, dtype=torch.float16))], lr=1e-3)
        with pytest.raises(ValueError, match=r"parameter 0 of group 1 \(shape \(3, 5\)\) is not contiguous"):
            optim.Adam([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(5, 3).t())]}], lr=1e-3)
        with pytest.raises(TypeError, match=r"parameter 'head.bias' is torch.float64"):
            optim.Adam([("body.weight", w), ("head.bias", torch.nn.Parameter(torch.zeros(2, dtype=torch.float64)))], lr=1e-3)
        with pytest.raises(NotImplementedError, match="amsgrad"):
            optim.Adam([w], lr=1e-3, amsgrad=True)
        with pytest.raises(TypeError, match="tensor lr"):
            optim.Adam([w], lr=torch.tensor(1e-3))
    finally:
        optim._check_param = real


class _Cuda:
    """A parameter as _check_param sees it, reporting that it lives on the GPU: the other refusals are reachable without one."""

    def __init__(self, p):
        self._p = p

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._p, name)


def test_state_dict_round_trips_through_torch_adam_with_the_step_preserved(monkeypatch):
    """optim.Adam's state is torch's layout: it loads into a plain torch.optim.Adam, which steps on, and comes back; the counter
    is one tensor shared by every entry before and after.  (No kernel runs here: the device refusal is taken out, the state is
    filled by the optimizer's own initialiser and torch does the stepping.)"""
    from isubgvqa_amd import optim
    monkeypatch.setattr(optim, "_check_param", lambda p, name: None)
    torch.manual_seed(0)
    make = lambda: [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    ours_p, theirs_p = make(), make()
    ours = optim.Adam([{"params": ours_p[:1]}, {"params": ours_p[1:], "lr": 3e-3}], lr=1e-2, betas=(0.8, 0.99), eps=1e-7,
                      weight_decay=0.01, max_grad_norm=2.0)
    for p in ours_p:
        st = ours._init_state(p)
        st["exp_avg"].normal_()
        st["exp_avg_sq"].uniform_()
    ours._step.fill_(3)
    assert all(ours.state[p]["step"] is ours._step for p in ours_p)
    sd = ours.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and [g["lr"] for g in sd["param_groups"]] == [1e-2, 3e-3]
    assert sd["state"][0]["step"] is not sd["state"][1]["step"] and sd["state"][0]["step"] is not ours._step      # a copy per entry
    theirs = torch.optim.Adam([{"params": theirs_p[:1]}, {"params": theirs_p[1:]}], lr=1.0)
    theirs.load_state_dict(sd)
    assert [float(theirs.state[p]["step"]) for p in theirs_p] == [3.0, 3.0]
    assert theirs.param_groups[1]["lr"] == 3e-3 and theirs.param_groups[0]["betas"] == (0.8, 0.99)
    for a, b in zip(ours_p, theirs_p):
        assert torch.equal(ours.state[a]["exp_avg"], theirs.state[b]["exp_avg"])
        b.grad = torch.randn_like(b)
    theirs.step()                                              # torch's own step: 3 -> 4
    assert float(ours._step) == 3.0 and all(ours.state[p]["step"] is ours._step for p in ours_p)      # not ours that torch stepped
    back = theirs.state_dict()
    assert [float(back["state"][i]["step"]) for i in (0, 1)] == [4.0, 4.0]
    ours.load_state_dict(back)
    assert float(ours._step) == 4.0 and ours._step.dtype == torch.float64 and ours._step.dim() == 0
    assert all(ours.state[p]["step"] is ours._step for p in ours_p), "the counter is shared again after load_state_dict"
    for a, b in zip(ours_p, theirs_p):
        assert torch.equal(ours.state[a]["exp_avg_sq"], theirs.state[b]["exp_avg_sq"])
    assert ours._table_key is None                              # the address table is rebuilt at the next step
    # a checkpoint as the reference writes it ({"optimizer": optimizer.state_dict()} of a torch.optim.Adam) resumes
    ours.load_state_dict(torch.optim.Adam([{"params": theirs_p[:1]}, {"params": theirs_p[1:]}], lr=1e-4).state_dict())   # no state yet
    assert ours.param_groups[0]["lr"] == 1e-4


def test_meters_report_is_the_references_average_meter():
    """Meters.summarize on hand-filled totals against a restated AverageMeter sequence (ISubGVQA/utils/avg_meter.py), one NaN loss
    skipped as train_epoch.py does it."""
    from isubgvqa_amd import train

    class AverageMeter:
        def __init__(self):
            self.val = self.avg = self.sum = self.count = 0

        def update(self, val, n=1):
            self.val = val
            self.sum += val * n
            self.count += n
            self.avg = self.sum / self.count

    steps = [(0.75, 48, 64), (float("nan"), 10, 64), (1.5, 7, 19), (0.3125, 64, 64)]       # (loss, correct, batch size)
    losses, acc = AverageMeter(), AverageMeter()
    totals = [0.0] * 8
    for loss, correct, n in steps:
        acc.update(100.0 * correct / n, n)
        if not math.isnan(loss):
            losses.update(loss, n)
            totals[0] += loss * n
            totals[1] += n
        else:
            totals[5] += 1
        totals[2] += correct
        totals[3] += n
        totals[4] += 1
    totals[6] = 1.0
    r = train.Meters.summarize(totals)
    assert r["loss"] == losses.avg and abs(r["acc1"] - acc.avg) <= 1e-12 * acc.avg
    assert (r["steps"], r["skipped_steps"], r["nonfinite_losses"], r["rows"]) == (4, 1, 1, 211)
    assert train.Meters.summarize([0.0] * 8)["loss"] == 0.0 and train.Meters.summarize([0.0] * 8)["acc1"] == 0.0
    m = train.Meters("cpu")
    assert m.totals.dtype == torch.float64 and tuple(m.totals.shape) == (8,)
    m.totals.copy_(torch.tensor(totals, dtype=torch.float64))
    assert m.report() == r
    m.reset()
    assert m.report()["steps"] == 0


def test_cross_entropy_refuses_cpu_tensors():
    from isubgvqa_amd import _lib, ops
    with pytest.raises(_lib.IsgError, match="must live on the GPU"):
        ops.cross_entropy(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(_lib.IsgError, match="must live on the GPU"):
        ops.cross_entropy(torch.zeros(2, 5, requires_grad=True), torch.zeros(2, dtype=torch.int64))
    assert "GradScaler" in inspect.getdoc(__import__("isubgvqa_amd.train", fromlist=["train"]))
