"""Data-parallel training on a real MI355X: isg_mt_pack through the C ABI, and distributed.GradSync + optim.Adam(grad_sync=...) +
train.train_step(sync=...) on two replicas inside one process, on micro-batches, and on a one-rank RCCL group.

TOLERANCES.  accumulate = 0 is one fp32 multiply: bit-equal to torch's `src * scale`.  accumulate = 1 is one fmaf per call: after
the overwrite and three accumulations an element went through 4 roundings of at most half an ulp of the partial sum each, 2 ulps
of the largest partial sum in all; the bound is 3.  Two micro-batches at scale 0.5: the first product is exact, the fmaf rounds
once, half an ulp; the bound is 2.  Everything else (the two replicas, the third copy stepped by a plain optim.Adam) is the same
kernels on the same values in the same order and is held to equal bits.
"""
import copy
import os
import subprocess
import sys
import textwrap
import threading
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ulp32(x64):
    """one float32 ulp at the magnitude of each float64 element"""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


class Table:
    """A tensor table of isg_mt_pack over a guarded bucket: slots from bucket_layout, `shift[t]` elements into their slot."""

    def __init__(self, numels, shift, dev):
        from isubgvqa_amd import _lib_optim, optim
        from isubgvqa_amd.distributed import bucket_layout
        self.numels, self.dev = list(numels), dev
        offsets, self.total = bucket_layout([n + s for n, s in zip(numels, shift)])
        self.offsets = [o + s for o, s in zip(offsets, shift)]
        self.flat = torch.full((GUARD + self.total + GUARD,), SENTINEL, device=dev)
        self.bucket = self.flat[GUARD:GUARD + self.total]
        self.bucket.zero_()
        assert self.bucket.data_ptr() % 256 == 0
        self.prefix = optim.chunk_prefix(numels, int(_lib_optim.load().isg_mt_chunk_elems()))
        self.inside = torch.zeros(self.total, dtype=torch.bool, device=dev)
        for o, n in zip(self.offsets, numels):
            self.inside[o:o + n] = True

    def slot(self, t):
        return self.bucket[self.offsets[t]:self.offsets[t] + self.numels[t]]

    def pack(self, sources, scale, accumulate):
        from isubgvqa_amd import _lib, _lib_dist, ops
        T = len(self.numels)
        src = [0 if s is None else s.data_ptr() for s in sources]
        dst = [self.bucket.data_ptr() + 4 * o for o in self.offsets]
        table = torch.tensor(src + dst + self.numels + self.prefix, dtype=torch.int64).to(self.dev)
        base = table.data_ptr()
        _lib.check(_lib_dist.load().isg_mt_pack(base, base + 8 * T, base + 16 * T, base + 24 * T, T, self.prefix[-1], scale,
                                                accumulate, ops._stream()), "isg_mt_pack")
        torch.cuda.synchronize()
        return table

    def check_outside(self):
        assert float(self.bucket[~self.inside].abs().max()) == 0.0, "the padding between two slots was written"
        assert bool((self.flat[:GUARD] == SENTINEL).all()) and bool((self.flat[-GUARD:] == SENTINEL).all()), \
            "a guard word beside the bucket was written"


NUMELS = [0, 1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 7, 1000, 4099, 300]
# 1000: a source one element behind a 16-byte boundary, its slot on one -- scalars.  4099: source AND slot one element behind a
# boundary -- the float4 body behind a three-element scalar head.  300: no source.
SHIFT = [0] * 12 + [0, 1, 0]
MISALIGNED, SHIFTED, NULL = 12, 13, 14


def make_sources(dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for t, n in enumerate(NUMELS):
        if t == NULL:
            out.append(None)
        elif t in (MISALIGNED, SHIFTED):
            big = torch.randn(n + 1, device=dev, generator=g)
            assert big.data_ptr() % 16 == 0
            out.append(big[1:])
        else:
            out.append(torch.randn(n, device=dev, generator=g))
    return out


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
def test_pack_through_the_c_abi(dev, scale):
    s32 = torch.tensor(scale, dtype=torch.float32, device=dev)
    runs = []
    for _ in range(2):                                   # two identical sequences: equal bits
        tab = Table(NUMELS, SHIFT, dev)
        src0 = make_sources(dev, 1)
        assert src0[MISALIGNED].data_ptr() % 16 == 4 and tab.slot(MISALIGNED).data_ptr() % 16 == 0
        assert src0[SHIFTED].data_ptr() % 16 == 4 and tab.slot(SHIFTED).data_ptr() % 16 == 4
        tab.slot(NULL).fill_(7.0)                        # the overwrite of a tensor without a source packs zeros
        tab.pack(src0, scale, 0)
        for t, s in enumerate(src0):
            want = torch.zeros(NUMELS[t], device=dev) if s is None else s * s32
            assert same_bits(tab.slot(t), want), f"accumulate = 0, scale {scale}: tensor {t} of {NUMELS[t]} elements"
        tab.check_outside()
        first = tab.bucket.clone()
        # three accumulations with fresh sources, beside the same recurrence in float64
        tab.slot(NULL).copy_(torch.arange(NUMELS[NULL], device=dev, dtype=torch.float32))
        ref = [None if s is None else s.double() * s32.double() for s in src0]
        largest = [None if r is None else r.abs() for r in ref]
        for k in range(3):
            srck = make_sources(dev, 10 + k)
            tab.pack(srck, scale, 1)
            for t, s in enumerate(srck):
                if s is not None:
                    ref[t] = ref[t] + s.double() * s32.double()
                    largest[t] = torch.maximum(largest[t], ref[t].abs())
        worst = 0.0
        for t in range(len(NUMELS)):
            if t == NULL:
                assert same_bits(tab.slot(t), torch.arange(NUMELS[t], device=dev, dtype=torch.float32)), \
                    "accumulate = 1 changed the slot of a tensor without a source"
                continue
            if NUMELS[t] == 0:
                continue
            err = (tab.slot(t).double() - ref[t]).abs() / ulp32(largest[t])
            worst = max(worst, float(err.max()))
            assert float(err.max()) <= 3.0, f"accumulate = 1, scale {scale}: tensor {t} is {float(err.max()):.2f} ulps off"
        print(f"[grad_sync] isg_mt_pack scale {scale:.4f}: three accumulations within {worst:.2f} ulps of float64")
        tab.check_outside()
        runs.append((first, tab.bucket.clone()))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "two identical calls gave different bits"


def test_pack_beyond_the_grid_cap(dev):
    """2049 full chunks and a tail of 5: more chunks than the grid has workgroups, so the first workgroup strides to a second one."""
    n = 2049 * 4096 + 5
    tab = Table([n], [0], dev)
    src = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    tab.pack([src], 0.5, 0)
    assert same_bits(tab.slot(0), src * 0.5)
    tab.check_outside()


# ---- GradSync on the 64-graph Gumbel model of tests/test_gpu_optim.py ------------------------------------------------------------
def small_model(dev):
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=64, channels=64, layers=3, masks=(1.0, 0.15, 0.15), sampler="gumbel", sample_k=5, seed=123)
    wl = synthetic.make_workload(cfg).to(dev)
    torch.manual_seed(0)
    model = synthetic.build_answer_model(cfg).to(dev).train()
    target = torch.randint(0, 1842, (cfg.num_graphs,), generator=torch.Generator().manual_seed(1)).to(dev)
    return model, wl, target


def halves(wl, target):
    from isubgvqa_amd.distributed import shard_workload
    parts = [shard_workload(wl, r, 2) for r in range(2)]
    assert [p.num_graphs for p in parts] == [32, 32]
    return parts, [target[:32].contiguous(), target[32:].contiguous()]


class Pair:
    """The transport of two replicas that live in one process: all_reduce(t) of rank r waits for the other rank's call, then both
    tensors hold the sum.  Each replica runs in a thread of its own, and holds `cv` for as long as it runs: the two never run at
    the same time, a replica hands over only while it waits in its hook."""

    def __init__(self):
        self.cv = threading.Condition()
        self.waiting, self.round, self.failed = {}, 0, None

    def hook(self, rank):
        def all_reduce(t):
            with self.cv:
                self.waiting[rank] = t
                if len(self.waiting) == 2:
                    a, b = self.waiting[0], self.waiting[1]
                    total = a + b
                    a.copy_(total)
                    b.copy_(total)
                    self.waiting, self.round = {}, self.round + 1
                    self.cv.notify_all()
                    return
                mine = self.round
                if not self.cv.wait_for(lambda: self.round != mine or self.failed is not None, timeout=120):
                    raise TimeoutError("the other replica never reached its all-reduce")
                if self.round == mine:
                    raise RuntimeError("the other replica failed")
        return all_reduce

    def run(self, bodies):
        def guarded(body):
            with self.cv:
                try:
                    body()
                except BaseException as e:             # noqa: BLE001 -- handed to the test's thread below
                    self.failed = self.failed or e
                    self.cv.notify_all()
        threads = [threading.Thread(target=guarded, args=(b,)) for b in bodies]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
            assert not t.is_alive()
        if self.failed is not None:
            raise self.failed


def test_two_replicas_in_one_process(dev):
    from isubgvqa_amd import optim, train
    from isubgvqa_amd.distributed import GradSync
    model, wl, target = small_model(dev)
    parts, targets = halves(wl, target)
    reps = [copy.deepcopy(model) for _ in range(2)]
    third = copy.deepcopy(model)
    frozen = "logit_fc.bias"                               # no gradient on replica B: it still steps there, with 0.5 * gA
    dict(reps[1].named_parameters())[frozen].requires_grad_(False)
    pair = Pair()
    syncs = [GradSync(reps[r].named_parameters(), world=2, force=True, all_reduce=pair.hook(r), rank=r) for r in range(2)]
    opts = [optim.Adam(reps[r].parameters(), lr=2e-3, max_grad_norm=2.0, grad_sync=syncs[r]) for r in range(2)]
    meters = [train.Meters(dev) for _ in range(2)]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    pair.run([lambda r=r: train.train_step(reps[r], opts[r], parts[r], targets[r], meters[r], seed=7, sync=syncs[r]) for r in range(2)])
    torch.cuda.synchronize()
    named = [dict(m.named_parameters()) for m in reps]
    members = [n for n, p in named[0].items() if syncs[0].has(p)]
    assert members == [n for n, p in named[1].items() if syncs[1].has(p)], "the replicas agreed on different sets"
    assert frozen in members and named[1][frozen].grad is None and named[0][frozen].grad is not None
    unused = [n for n in named[0] if n not in members]
    assert unused and all(named[r][n].grad is None for r in range(2) for n in unused)      # e.g. node_logits: in no rank's graph
    # (a) every slot is the average of the two local gradients, in one rounding
    for n in members:
        ga, gb = named[0][n].grad, named[1][n].grad
        want = ga * 0.5 + (torch.zeros_like(ga) if gb is None else gb * 0.5)
        assert same_bits(syncs[0].grad(named[0][n]), want), f"bucket slot of {n}"
    assert same_bits(syncs[0].bucket, syncs[1].bucket)
    # (b) the replicas stay equal, bit for bit
    for n in named[0]:
        assert same_bits(named[0][n], named[1][n]), f"parameter {n} differs between the replicas"
        if n not in members:
            assert same_bits(named[0][n], before[n]), f"{n} is outside the set and was stepped"
        elif float(syncs[0].grad(named[0][n]).abs().max()) > 0.0:
            assert not same_bits(named[0][n], before[n]), f"{n} is in the set and was not stepped"
    assert not same_bits(named[1][frozen], before[frozen]), "the parameter without a local gradient did not step on replica B"
    for n in members:
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(opts[0].state[named[0][n]][k], opts[1].state[named[1][n]][k]), f"{k} of {n}"
    assert all(named[r][n] not in opts[r].state for r in range(2) for n in unused)
    assert same_bits(opts[0].last_grad_norm, opts[1].last_grad_norm) and float(opts[0]._step) == float(opts[1]._step) == 1.0
    # (c) a third copy, stepped by a plain optim.Adam whose p.grad are the averaged tensors
    n3 = dict(third.named_parameters())
    for n in members:
        n3[n].grad = syncs[0].grad(named[0][n]).clone()
    plain = optim.Adam(third.parameters(), lr=2e-3, max_grad_norm=2.0)
    plain.step()
    torch.cuda.synchronize()
    assert same_bits(plain.last_grad_norm, opts[0].last_grad_norm), (float(plain.last_grad_norm), float(opts[0].last_grad_norm))
    for n in named[0]:
        assert same_bits(n3[n], named[0][n]), f"parameter {n}: the sync's step differs from a plain step on the averaged gradients"
    for n in members:
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(plain.state[n3[n]][k], opts[0].state[named[0][n]][k]), f"{k} of {n}"
    # a parameter outside the set that receives a gradient later is refused by name
    stray = unused[0]
    named[0][stray].grad = torch.zeros_like(named[0][stray])
    with pytest.raises(RuntimeError, match=stray.replace(".", r"\.")):
        syncs[0].pack()
    named[0][stray].grad = None
    for r in range(2):
        rep = meters[r].report()
        assert rep["steps"] == 1 and rep["rows"] == 32 and rep["skipped_steps"] == 0


def test_two_micro_batches_accumulate_into_one_step(dev):
    from isubgvqa_amd import distributed, optim, train
    model, wl, target = small_model(dev)
    parts, targets = halves(wl, target)
    seen = []
    sync = distributed.GradSync(model.named_parameters(), world=1, force=True, all_reduce=lambda t: seen.append(t.clone()))
    opt = optim.Adam(model.parameters(), lr=2e-3, max_grad_norm=2.0, grad_sync=sync)
    meters = train.Meters(dev)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    launches, ours = dict(optim.LAUNCHES), dict(distributed.LAUNCHES)
    grads = []
    for micro in range(2):
        train.train_step(model, opt, parts[micro], targets[micro], meters, seed=11 + micro, sync=sync, accumulate=2, micro=micro)
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        if micro == 0:
            assert float(opt._step) == 0.0 and optim.LAUNCHES["adam"] == launches["adam"], "the optimizer stepped on the first micro-batch"
            assert all(same_bits(p, before[n]) for n, p in model.named_parameters())
    torch.cuda.synchronize()
    assert float(opt._step) == 1.0 and optim.LAUNCHES["adam"] == launches["adam"] + 1 and optim.LAUNCHES["sqnorm"] == launches["sqnorm"] + 1
    assert distributed.LAUNCHES["pack"] == ours["pack"] + 2 and distributed.LAUNCHES["reduce"] == ours["reduce"] + 1
    assert len(seen) == 2 and seen[1].numel() == sync.bucket.numel()      # the mask once, then the bucket before the step
    snapshot, worst = seen[1], 0.0
    for n, p in model.named_parameters():
        if not sync.has(p):
            continue
        o, cnt = sync._slot[id(p)]
        ref = 0.5 * grads[0][n].double() + 0.5 * grads[1][n].double()
        err = (snapshot[o:o + cnt].view(p.shape).double() - ref).abs() / ulp32(ref)
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= 2.0, f"{n}: {float(err.max()):.2f} ulps from 0.5 * g1 + 0.5 * g2"
        assert not same_bits(p, before[n]) or float(ref.abs().max()) == 0.0
    print(f"[grad_sync] two micro-batches: the bucket is within {worst:.2f} ulps of the float64 mean")
    with pytest.raises(ValueError, match="accumulate > 1"):
        train.train_step(model, optim.Adam(model.parameters(), lr=1e-3), parts[0], targets[0], meters, accumulate=2, micro=0)


def test_five_steps_send_one_table_and_read_nothing_on_the_host(dev):
    from isubgvqa_amd import distributed, optim, train
    model, wl, target = small_model(dev)
    sync = distributed.GradSync(model.named_parameters(), world=1, force=True, all_reduce=lambda t: None)
    opt = optim.Adam(model.parameters(), lr=2e-3, max_grad_norm=2.0, grad_sync=sync)
    meters = train.Meters(dev)
    sent = optim.LAUNCHES["table_copies"]
    with warnings.catch_warnings(record=True) as control:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            float(meters.totals[0])                                     # the detector does see a host read
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert any("synchroniz" in str(w.message) for w in control), "torch's sync debug mode did not report a .item()"
    train.train_step(model, opt, wl, target, meters, seed=7, sync=sync)            # lazy initialisation, the set and the tables
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            for step in range(1, 5):
                opt.zero_grad(set_to_none=True)
                train.train_step(model, opt, wl, target, meters, seed=7 + step, sync=sync)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    assert not syncs, f"a training step with a GradSync read the device on the host: {syncs[:3]}"
    assert optim.LAUNCHES["table_copies"] == sent + 1, "the bucket's slots never move: Adam's table is sent once per run"
    rep = meters.report()
    assert rep["steps"] == 5 and rep["skipped_steps"] == 0 and float(opt._step) == 5.0


SCRIPT = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %r)
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from isubgvqa_amd import distributed, optim
    g = torch.Generator(device=dev).manual_seed(0)
    sizes = (1000, 4097, 64, 5)
    params = [torch.nn.Parameter(torch.randn(n, device=dev, generator=g)) for n in sizes]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    sync = distributed.GradSync(params, force=True)
    assert sync.active and sync.world == 1 and sync.rank == 0
    sync.broadcast_params()
    opt = optim.Adam(params, lr=1e-2, max_grad_norm=2.0, grad_sync=sync)
    ref = optim.Adam(twins, lr=1e-2, max_grad_norm=2.0)
    for step in range(2):
        for p, q in zip(params[:3], twins[:3]):                    # the fourth never has a gradient: outside the set
            p.grad = torch.randn(p.shape, device=dev, generator=g)
            q.grad = p.grad.clone()
        before = distributed.LAUNCHES["reduce"]
        sync.pack()
        sync.reduce()
        opt.step()
        ref.step()
        assert distributed.LAUNCHES["reduce"] == before + 1
    torch.cuda.synchronize()
    assert not sync.has(params[3]) and sync.bucket.numel() == 1024 + 4160 + 64
    for p, q in zip(params, twins):
        if sync.has(p):
            assert torch.equal(sync.grad(p), p.grad), "RCCL's one-rank sum changed the packed gradients"
        assert torch.equal(p, q), "the step from the bucket differs from the step from p.grad"
    flag = sync.params_in_sync()
    assert flag.is_cuda and int(flag) == 1
    dist.barrier()
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("GradSync on RCCL ok")
""") % ROOT


def test_grad_sync_on_a_one_rank_rccl_group():
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    res = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    err = [l for l in res.stderr.splitlines() if l.strip() and "amdgpu.ids" not in l]
    assert res.returncode == 0 and "GradSync on RCCL ok" in res.stdout, "\n".join(err[-25:])
