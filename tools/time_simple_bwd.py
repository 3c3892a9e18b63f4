#!/usr/bin/env python3
"""Forward + backward of ops.simple_topk under autograd with autograd.SIMPLE_BWD_KERNEL on (isg_simple_topk_bwd, one launch)
against off (autograd through the torch restatement of the circuit), alternating in one process, HIP events.

  python tools/time_simple_bwd.py [--rounds 12] [--out profiles/<name>.json]

Shapes: the masked layer of BASELINE configs[1] -- 4096 ragged rows with synthetic.CFG2's node counts (nmax <= 48, n = 64), k = 5 --
and the text-sampling call, dense [4096, 20] with k = 4.  One sample = one call (restatement) or 20 calls (kernel), forward and
backward, median over the rounds behind two discarded ones.  Launches per call: the torch profiler's device kernels of one call,
beside the aten operator calls of the same call (views excluded, as the host sees them).  The two arms' gradients are compared."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import autograd, ops, synthetic

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
ROUNDS, SKIP, KERNEL_REPS = int(opt.get("--rounds", 12)), 2, 20
VIEWS = {"aten::view", "aten::reshape", "aten::select", "aten::slice", "aten::as_strided", "aten::unsqueeze", "aten::squeeze",
         "aten::expand", "aten::permute", "aten::t", "aten::transpose", "aten::alias", "aten::detach", "aten::_unsafe_view",
         "aten::view_as", "aten::unbind", "aten::split", "aten::narrow", "aten::_reshape_alias"}


def shapes():
    gen = torch.Generator().manual_seed(synthetic.CFG2.seed)
    sizes = synthetic.graph_sizes(synthetic.CFG2, gen)
    batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes).to(dev)
    plan = ops.GraphPlan.build(batch, None, num_graphs=sizes.numel())
    g = torch.Generator(device=dev).manual_seed(1)
    N = int(sizes.sum())
    yield (f"configs[1] masked layer: {sizes.numel()} ragged rows, nmax {plan.nmax}, k 5", torch.randn(N, 1, device=dev, generator=g),
           torch.randn(N, 1, device=dev, generator=g), 5, plan)
    yield ("text sampling: dense [4096, 20], k 4", torch.randn(4096, 20, device=dev, generator=g),
           torch.randn(4096, 20, device=dev, generator=g), 4, None)


def call(scores, w, k, plan, on):
    autograd.SIMPLE_BWD_KERNEL = on
    leaf = scores.detach().requires_grad_(True)
    ops.simple_topk(leaf, k, plan=plan, seed=3).backward(w)
    return leaf.grad


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def launches(fn):
    """(device kernels or None, aten operator calls without views) of one call"""
    acts = [torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]
    try:
        with torch.profiler.profile(activities=acts) as prof:
            fn()
            torch.cuda.synchronize()
    except RuntimeError:                                  # no device tracing in this build: the host's view alone
        with torch.profiler.profile(activities=acts[:1]) as prof:
            fn()
            torch.cuda.synchronize()
    kernels = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower()
                  and "memset" not in ev.name.lower())
    aten = sum(e.count for e in prof.key_averages() if e.key.startswith("aten::") and e.key not in VIEWS)
    return (kernels or None), aten


def median(v):
    return sorted(v)[len(v) // 2]


keep = autograd.SIMPLE_BWD_KERNEL
out = {"device": torch.cuda.get_device_name(0),
       "method": f"HIP events around forward + backward of ops.simple_topk under autograd; {ROUNDS} rounds ({SKIP} discarded), the two arms "
                 f"alternating inside a round; a sample is 1 call (restatement) or {KERNEL_REPS} calls (kernel); median us per call",
       "shapes": []}
try:
    for name, scores, w, k, plan in shapes():
        arms = {"kernel": (True, KERNEL_REPS), "restatement": (False, 1)}
        grads = {a: call(scores, w, k, plan, on) for a, (on, _) in arms.items()}           # warm-up of both arms, and their results
        before = ops.COUNTERS["simple_bwd_kernel"]
        call(scores, w, k, plan, True)
        assert ops.COUNTERS["simple_bwd_kernel"] == before + 1, "the kernel arm did not run the kernel"
        diff = (grads["kernel"] - grads["restatement"]).abs().max().item()
        us = {a: [] for a in arms}
        for r in range(ROUNDS):
            for a, (on, reps) in arms.items():
                t = timed(lambda: call(scores, w, k, plan, on), reps)
                if r >= SKIP:
                    us[a].append(t)
        count = {a: launches(lambda: call(scores, w, k, plan, on)) for a, (on, _) in arms.items()}
        row = {"shape": name, "us": {a: round(median(v), 1) for a, v in us.items()}, "min_us": {a: round(min(v), 1) for a, v in us.items()},
               "max_us": {a: round(max(v), 1) for a, v in us.items()},
               "device_kernels_per_call": {a: c[0] for a, c in count.items()}, "aten_ops_per_call": {a: c[1] for a, c in count.items()},
               "max_abs_gradient_difference": diff, "max_abs_gradient": grads["restatement"].abs().max().item()}
        row["restatement_over_kernel"] = round(row["us"]["restatement"] / row["us"]["kernel"], 1)
        out["shapes"].append(row)
        print(f"{name}: kernel {row['us']['kernel']:.1f} us ({row['min_us']['kernel']:.1f}-{row['max_us']['kernel']:.1f}), restatement "
              f"{row['us']['restatement']:.1f} us ({row['min_us']['restatement']:.1f}-{row['max_us']['restatement']:.1f}) = "
              f"{row['restatement_over_kernel']} x; device kernels per call {count['kernel'][0]} / {count['restatement'][0]}, aten operator "
              f"calls {count['kernel'][1]} / {count['restatement'][1]}; max |d kernel - d restatement| {diff:.2e}", flush=True)
finally:
    autograd.SIMPLE_BWD_KERNEL = keep
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
