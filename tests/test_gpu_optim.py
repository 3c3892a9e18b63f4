"""optim.Adam / isg_mt_sqnorm / isg_mt_adam on a real MI355X against torch.optim.Adam (AdamW, clip_grad_norm_) run in float64 on
the CPU, and train.train_step end to end.

Tensor sets, with c = isg_mt_chunk_elems(): every numel of {0, 1, 3, 255, 256, 257, c-1, c, c+1, 2c+5} alone, and all of them plus
27 random sizes as 37 tensors; each set once as separate allocations and once as views at odd element offsets of one flat buffer
(4-byte aligned only: where a vectorised body goes wrong).  In the 37-tensor set every fifth parameter never gets a gradient.

TOLERANCE: torch's float32 CPU Adam runs the same sequence; the kernels get max(4 x its max abs error against float64, one
float32 ulp of the largest parameter) on params, exp_avg and exp_avg_sq after every one of five steps, and last_grad_norm the same
relative to clip_grad_norm_'s float32 norm.  Measured on the MI355X, the worst over all sets, forms and steps (kernel error /
torch-float32 error, each the max abs error against float64):
    param        2.28e-07 / 2.22e-07  (clipping active, one tensor of 4097, step 2: 0.26 of the bound)
    exp_avg      6.95e-08 / 5.61e-08  (L2 weight decay, one view of 4095, step 5: 0.29 of the bound)
    exp_avg_sq   4.08e-09 / 2.30e-09  (one tensor of 255, step 5: 0.02 of the bound)
    grad norm    5.20e-08 / 5.20e-08  (one tensor of 3: 0.25 of the bound)
With the 256 lane totals of a chunk added in fp32 the norm of the 4096-element tensor missed its bound (3.93e-06 against one ulp,
3.81e-06; torch float32: 1.2e-07): they are added in double since.
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import parity_record

pytestmark = pytest.mark.gpu

STEPS = 5
CONFIGS = ("default", "l2", "decoupled", "two_groups", "clip_active", "clip_inactive", "lr_changes")
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def chunk():
    from isubgvqa_amd import _lib_optim
    return int(_lib_optim.load().isg_mt_chunk_elems())


def tensor_sets():
    c = chunk()
    base = [0, 1, 3, 255, 256, 257, c - 1, c, c + 1, 2 * c + 5]
    g = torch.Generator().manual_seed(5)
    extra = [int(v) for v in torch.randint(1, 3000, (27,), generator=g)]
    return [[n] for n in base] + [base + extra]


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def build_params(numels, dev, views, seed):
    """(device parameters, their CPU float32 values).  views: slices of ONE flat buffer, each starting at an odd element offset."""
    g = torch.Generator().manual_seed(seed)
    values = [torch.randn(n, generator=g) for n in numels]
    if not views:
        return [v.to(dev).requires_grad_(True) for v in values], values
    offs, off = [], 1
    for n in numels:
        offs.append(off)
        off += n + (1 if (off + n) % 2 == 0 else 2)          # the next start is odd again
    flat = torch.zeros(off + 1, device=dev)
    assert flat.data_ptr() % 16 == 0
    params = []
    for n, o, v in zip(numels, offs, values):
        assert o % 2 == 1
        p = flat[o:o + n]
        p.copy_(v)
        params.append(p.detach().requires_grad_(True))
    return params, values


def make_grads(numels, step, seed, with_grad):
    g = torch.Generator().manual_seed(seed * 100 + step)
    return [torch.randn(n, generator=g) if w else None for n, w in zip(numels, with_grad)]


def set_grads(params, grads, dev, views):
    """Fresh gradient tensors every step; in the views form they are odd-offset slices of a fresh flat buffer too."""
    if views:
        total = sum(g.numel() + 2 for g in grads if g is not None) + 2
        flat, off = torch.zeros(total, device=dev), 1
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif views:
            p.grad = flat[off:off + g.numel()]
            p.grad.copy_(g)
            off += g.numel() + (1 if (off + g.numel()) % 2 == 0 else 2)
        else:
            p.grad = g.to(dev)


def ref_optimizer(config, params, dtype):
    kw = dict(lr=1e-2)
    cls = torch.optim.Adam
    if config == "l2":
        kw["weight_decay"] = 1e-2
    if config == "decoupled":
        kw["weight_decay"] = 1e-2
        cls = torch.optim.AdamW
    if config == "two_groups" and len(params) > 1:
        h = len(params) // 2
        return cls([{"params": params[:h]}, {"params": params[h:], "lr": 3e-3}], **kw)
    return cls(params, **kw)


def our_optimizer(config, params):
    from isubgvqa_amd import optim
    kw = dict(lr=1e-2)
    if config in ("l2", "decoupled"):
        kw["weight_decay"] = 1e-2
        kw["decoupled"] = config == "decoupled"
    if config == "clip_active":
        kw["max_grad_norm"] = 0.05
    if config == "clip_inactive":
        kw["max_grad_norm"] = 1e6
    if config == "two_groups" and len(params) > 1:
        h = len(params) // 2
        return optim.Adam([{"params": params[:h]}, {"params": params[h:], "lr": 3e-3}], **kw)
    return optim.Adam(params, **kw)


def max_norm_of(config):
    return {"clip_active": 0.05, "clip_inactive": 1e6}.get(config, float("inf"))


def cat(ts):
    ts = [t.detach().reshape(-1) for t in ts]
    return torch.cat(ts).cpu().double() if ts else torch.zeros(0, dtype=torch.float64)


def hold(what, got, r64, r32, floor, case):
    if got.numel() == 0:
        return
    e32 = float((r32 - r64).abs().max())
    err = float((got - r64).abs().max())
    tol = max(4.0 * e32, floor)
    if what not in WORST or err / tol > WORST[what][2]:
        WORST[what] = (err, e32, err / tol, str(case))
    assert err <= tol, f"{what} {case}: |kernel - float64| = {err:.3e} > {tol:.3e} (torch float32: {e32:.3e})"


class Run:
    """One tensor set under one configuration: the device optimizer beside torch's in float64 and in float32 on the CPU."""

    def __init__(self, config, numels, dev, views, seed=3, ours_kw=None):
        self.config, self.numels, self.dev, self.views, self.seed = config, numels, dev, views, seed
        self.params, values = build_params(numels, dev, views, seed)
        self.with_grad = [len(numels) == 1 or i % 5 != 4 for i in range(len(numels))]
        self.p64 = [v.double().requires_grad_(True) for v in values]
        self.p32 = [v.clone().requires_grad_(True) for v in values]
        self.o64, self.o32 = ref_optimizer(config, self.p64, torch.float64), ref_optimizer(config, self.p32, torch.float32)
        self.ours = our_optimizer(config, self.params) if ours_kw is None else ours_kw(self.params)
        self.step_no = 0

    def reference_step(self, grads):
        norms = []
        for ps, opt, dt in ((self.p64, self.o64, torch.float64), (self.p32, self.o32, torch.float32)):
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(dt).clone()
            norms.append(float(torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], max_norm_of(self.config))))
            opt.step()
        return norms

    def step(self, check=True, totals=None):
        self.step_no += 1
        if self.config == "lr_changes" and self.step_no in (2, 4):
            for opt in (self.ours, self.o64, self.o32):
                opt.param_groups[0]["lr"] = 1e-2 / self.step_no
        grads = make_grads(self.numels, self.step_no, self.seed, self.with_grad)
        set_grads(self.params, grads, self.dev, self.views)
        n64, n32 = self.reference_step(grads)
        self.ours.step(totals=totals)
        if check:
            self.check(n64, n32)

    def state_of(self, opt, ps, key):
        return cat([opt.state[p][key] for p, w in zip(ps, self.with_grad) if w])

    def check(self, n64=None, n32=None):
        case = (self.config, self.numels if len(self.numels) == 1 else f"{len(self.numels)} tensors", "views" if self.views else "separate",
                f"step {self.step_no}")
        r64, r32 = cat(self.p64), cat(self.p32)
        floor = ulp32(r64.abs().max()) if r64.numel() else 0.0
        hold("param", cat(self.params), r64, r32, floor, case)
        for key in ("exp_avg", "exp_avg_sq"):
            hold(key, self.state_of(self.ours, self.params, key), self.state_of(self.o64, self.p64, key),
                 self.state_of(self.o32, self.p32, key), floor, case)
        if n64 is not None:
            got = float(self.ours.last_grad_norm)
            e32 = abs(n32 - n64)
            tol = max(4.0 * e32, ulp32(n64))
            err = abs(got - n64)
            if "grad_norm" not in WORST or err / max(tol, 1e-300) > WORST["grad_norm"][2]:
                WORST["grad_norm"] = (err, e32, err / max(tol, 1e-300), str(case))
            assert err <= tol, f"last_grad_norm {case}: {got} vs {n64} (torch float32: {n32})"
            if self.config == "clip_active" and n64 > 0.06:
                assert float(self.ours.last_clip) < 1.0
            if self.config != "clip_active":
                assert float(self.ours.last_clip) == 1.0

    def bits(self):
        ts = list(self.params) + [self.ours.state[p][k] for p, w in zip(self.params, self.with_grad) if w and p in self.ours.state
                                  for k in ("exp_avg", "exp_avg_sq")] + [self.ours._step]
        return [t.detach().cpu().contiguous().numpy().tobytes() for t in ts]


@pytest.mark.parametrize("config", CONFIGS)
def test_five_steps_against_float64(dev, config):
    WORST.clear()
    for numels in tensor_sets():
        for views in (False, True):
            run = Run(config, numels, dev, views)
            for _ in range(STEPS):
                run.step()
            assert float(run.ours._step) == STEPS and all(run.ours.state[p]["step"] is run.ours._step for p in run.ours.state)
            absent = [p for p, w in zip(run.params, run.with_grad) if not w]
            assert all(p not in run.ours.state for p in absent), "a parameter without a gradient is left out, as torch leaves it"
    for k, v in WORST.items():
        print(f"[optim] {config} {k}: kernel error {v[0]:.3e}, torch float32 error {v[1]:.3e}, error / tolerance {v[2]:.3f} at {v[3]}")
    parity_record(f"optim_{config}", {k: {"kernel": v[0], "torch_float32": v[1], "over_tolerance": v[2], "case": v[3]} for k, v in WORST.items()})


@pytest.mark.parametrize("views", (False, True))
def test_a_nonfinite_gradient_skips_the_step_bit_for_bit(dev, views):
    """One NaN, then one Inf among the gradients: params, moments and the counter keep their bits, the skipped counter rises, and
    the next clean step equals the float64 run that never saw the bad ones (bias correction from the unskipped count)."""
    from isubgvqa_amd import optim, train
    numels = tensor_sets()[-1]
    run = Run("default", numels, dev, views, ours_kw=lambda ps: optim.Adam(ps, lr=1e-2, max_grad_norm=1e6))
    meters = train.Meters(dev)
    run.step()
    run.step()
    for n_bad, (bad, totals) in enumerate(((float("nan"), None), (float("inf"), meters.totals)), 1):
        before = run.bits()
        grads = make_grads(numels, 50 + n_bad, 9, run.with_grad)
        grads[7][3] = bad
        set_grads(run.params, grads, dev, views)
        run.ours.step(totals=totals)
        assert run.bits() == before, f"a step with {bad} among its gradients changed a parameter, a moment or the counter"
        assert float(run.ours._clip[2]) == 0.0
    assert float(run.ours.skipped_steps) == 1.0 and meters.report()["skipped_steps"] == 1
    assert float(run.ours._step) == 2.0
    run.step()
    assert float(run.ours._step) == 3.0 and float(run.ours._clip[2]) == 1.0
    assert float(run.ours.skipped_steps) == 1.0


def test_no_norm_launch_without_clipping_or_the_skip(dev):
    from isubgvqa_amd import optim
    run = Run("two_groups", tensor_sets()[-1], dev, False,
              ours_kw=lambda ps: optim.Adam([{"params": ps[:18]}, {"params": ps[18:], "lr": 3e-3}], lr=1e-2, skip_nonfinite=False))
    before = dict(optim.LAUNCHES)
    for _ in range(3):
        run.step(check=False)
    run.check()
    assert optim.LAUNCHES["sqnorm"] == before["sqnorm"] and optim.LAUNCHES["adam"] == before["adam"] + 3 * 2
    assert run.ours.last_grad_norm is None and run.ours.last_clip is None
    run2 = Run("default", [257], dev, False)
    before = dict(optim.LAUNCHES)
    run2.step()
    assert optim.LAUNCHES["sqnorm"] == before["sqnorm"] + 1 and optim.LAUNCHES["adam"] == before["adam"] + 1
    assert isinstance(run2.ours.last_grad_norm, torch.Tensor) and run2.ours.last_grad_norm.is_cuda and run2.ours.last_clip.is_cuda


def test_gradient_addresses_that_change_between_steps(dev):
    """zero_grad(set_to_none=True) and an allocation in between move the gradients: the table is sent again and the right tensors
    are updated; gradients rewritten in place send nothing."""
    from isubgvqa_amd import optim
    run = Run("default", tensor_sets()[-1], dev, False)
    run.step()
    sent = optim.LAUNCHES["table_copies"]
    old = {p.grad.data_ptr() for p in run.params if p.grad is not None and p.numel()}
    keep = [p.grad for p in run.params]                       # the old blocks stay taken: the new gradients must land elsewhere
    run.ours.zero_grad(set_to_none=True)
    junk = torch.empty(12345, device=dev)
    run.step()
    assert not old & {p.grad.data_ptr() for p in run.params if p.grad is not None and p.numel()}
    assert optim.LAUNCHES["table_copies"] == sent + 1
    del keep, junk
    grads = make_grads(run.numels, 3, run.seed, run.with_grad)
    for p, g in zip(run.params, grads):                       # in place: same addresses
        if g is not None:
            p.grad.copy_(g)
    run.step_no = 3
    run.reference_step(grads)
    run.ours.step()
    run.check()
    assert optim.LAUNCHES["table_copies"] == sent + 1


def test_float4_body_behind_a_scalar_head(dev):
    """Param, gradient and both moments at the SAME odd element offset of four flat buffers: the one layout in which the update
    takes its float4 body behind a one- or three-element scalar head (moments that torch allocates are 16-byte aligned, and beside
    an odd-offset parameter they send the chunk down the scalar path)."""
    c = chunk()
    run = Run("l2", [c + 1, 257, 2 * c + 5, 3], dev, True)
    end = max(p.storage_offset() + p.numel() for p in run.params) + 4
    flats = {k: torch.zeros(end, device=dev) for k in ("exp_avg", "exp_avg_sq")}
    for p in run.params:
        st = run.ours._init_state(p)
        for k, flat in flats.items():
            st[k] = flat[p.storage_offset():p.storage_offset() + p.numel()]
    for _ in range(STEPS):
        run.step()
        for p in run.params:
            assert len({t.data_ptr() % 16 for t in (p, p.grad, run.ours.state[p]["exp_avg"], run.ours.state[p]["exp_avg_sq"])}) == 1
            assert p.data_ptr() % 16 in (4, 12)
    inside = torch.zeros(end, dtype=torch.bool, device=dev)
    for p in run.params:
        inside[p.storage_offset():p.storage_offset() + p.numel()] = True
    for flat in flats.values():
        assert float(flat[~inside].abs().max()) == 0.0, "an element between two views was written"


def test_two_runs_from_the_same_state_give_equal_bits(dev):
    for views in (False, True):
        outs = []
        for _ in range(2):
            run = Run("clip_active", tensor_sets()[-1], dev, views)
            for _ in range(3):
                run.step(check=False)
            outs.append(run.bits() + [run.ours._clip.cpu().numpy().tobytes()])
        assert outs[0] == outs[1]


def test_train_step_reduces_the_loss_and_only_report_reads_the_device(dev):
    """tests/test_gpu_train.py::test_a_few_optimizer_steps_reduce_the_loss's 64-graph model (Gumbel sampler) driven by
    train.train_step with optim.Adam(lr=2e-3, max_grad_norm=2.0) for 25 steps.  The loss is read from Meters: snapshots of the
    totals are taken ON the device after steps 5 and 20 and copied once the loop is over.  Every step but the first (lazy
    initialisation) runs under torch's sync debug mode: a host read of a device value inside it would be recorded."""
    from isubgvqa_amd import optim, synthetic, train
    cfg = synthetic.WorkloadConfig(num_graphs=64, channels=64, layers=3, masks=(1.0, 0.15, 0.15), sampler="gumbel", sample_k=5, seed=123)
    wl = synthetic.make_workload(cfg).to(dev)
    torch.manual_seed(0)
    model = synthetic.build_answer_model(cfg).to(dev).train()
    target = torch.randint(0, 1842, (cfg.num_graphs,), generator=torch.Generator().manual_seed(1)).to(dev)
    opt = optim.Adam(model.parameters(), lr=2e-3, max_grad_norm=2.0)
    meters = train.Meters(dev)
    snaps = {}
    with warnings.catch_warnings(record=True) as control:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            float(meters.totals[0])                                     # the detector does see a host read
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert any("synchroniz" in str(w.message) for w in control), "torch's sync debug mode did not report a .item()"
    train.train_step(model, opt, wl, target, meters, seed=7)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            for step in range(1, 25):
                train.train_step(model, opt, wl, target, meters, seed=7 + step)
                if step + 1 in (5, 20):
                    snaps[step + 1] = meters.totals.clone()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    assert not syncs, f"a training step read the device on the host: {syncs[:3]}"
    rep = meters.report()
    assert rep["steps"] == 25 and rep["skipped_steps"] == 0 and rep["nonfinite_losses"] == 0 and rep["rows"] == 25 * 64
    assert model.n_train_steps == 25 * 64
    t5, t20, t25 = snaps[5].cpu(), snaps[20].cpu(), meters.totals.cpu()
    first, last = train.Meters.summarize(t5.tolist())["loss"], train.Meters.summarize((t25 - t20).tolist())["loss"]
    print(f"[optim] train_step: mean loss of steps 1-5 {first:.4f}, of steps 21-25 {last:.4f}")
    assert last < 0.6 * first, (first, last)
    vm = train.Meters(dev)
    train.validate(model, [(wl, target)] * 2, vm, seed=3)
    assert model.training and vm.report()["steps"] == 2 and vm.report()["rows"] == 128
