#!/usr/bin/env python3
"""Mask optimisation (include/ext/isg_maskopt.h) on DESIGN.md 34's batch: 256 graphs drawn as BASELINE configs[1]
draws them, the AnswerModel of configs[1].  A host clock around explain.mask_optimization at T = 100 (and around the no_grad
forward, for scale) between two device synchronises; and -- between HIP events, the two arms alternating in one process --
ops.maskopt_step beside its torch formulation: a sigmoid, a row dot, the two regularisers' gradient, torch.optim.Adam on theta, a
sigmoid and a row scale.

  python tools/time_maskopt.py [--graphs 256] [--steps 100] [--rounds 10] [--out profiles/<name>.json]

Before anything is timed the launch is compared with the torch formulation.  A record, not a gate."""
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import explain, ops, synthetic

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
GRAPHS, STEPS, ROUNDS, WARMUP = int(opt.get("--graphs", 256)), int(opt.get("--steps", 100)), int(opt.get("--rounds", 10)), 2
SEED = 3                                                   # the Gumbel sampler's: the same noise in every iteration
A_SIZE, A_ENT, LR = 1.0, 0.1, 0.01

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS)
wl = synthetic.make_workload(cfg)
d = wl.to(dev)
model = synthetic.build_answer_model(cfg).eval().to(dev)
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=GRAPHS, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                           graph_sizes=wl.graph_sizes)
N, C = d.x.shape
gen = torch.Generator(device=dev).manual_seed(5)
g_rows = torch.randn(N, C, device=dev, generator=gen)
theta0 = 0.1 * torch.randn(N, device=dev, generator=gen)
n_rows = (plan.ptr[1:] - plan.ptr[:-1]).float().index_select(0, d.batch)      # every row's graph size

# the launch's state, and the torch formulation's: a parameter under torch.optim.Adam (its foreach implementation on the device)
state = [theta0.clone(), torch.zeros(N, device=dev), torch.zeros(N, device=dev)]
out_rows = torch.empty(N, C, device=dev)
param = theta0.clone().requires_grad_(True)
adam = torch.optim.Adam([param], lr=LR)
step_no = [0]


def step_launch():
    step_no[0] += 1
    return ops.maskopt_step(d.x, g_rows, plan.ptr, state[0], state[1], state[2], step=step_no[0], a_size=A_SIZE, a_ent=A_ENT, lr=LR,
                            out=out_rows)[0]


def step_torch():
    with torch.no_grad():
        m = torch.sigmoid(param)
        s = (g_rows * d.x).sum(1)
        param.grad = (s + (A_SIZE - A_ENT * param) / n_rows) * m * (1 - m)
    adam.step()
    with torch.no_grad():
        return torch.sigmoid(param).unsqueeze(1) * d.x


a, b = step_launch(), step_torch()
torch.cuda.synchronize()
assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), "the launch differs from its torch formulation"
assert float((state[0] - param.detach()).abs().max()) <= 1e-6


def forward():
    with torch.no_grad():
        return model(d, seed=SEED, plan=plan)


def mask_optimization():
    return explain.mask_optimization(model, d, seed=SEED, steps=STEPS)


def sample_events(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def sample_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def summary(v):
    v = sorted(v)
    at = lambda p: round(v[min(len(v) - 1, int(p * len(v)))], 1)
    return {"median_us": at(0.5), "p10_us": at(0.1), "p90_us": at(0.9)}


whole = {"forward_no_grad": forward, "mask_optimization": mask_optimization}
kernels = {"maskopt_step_launch": step_launch, "maskopt_step_torch": step_torch}
host = {a: [] for a in whole}
events = {a: [] for a in kernels}
for r in range(ROUNDS + WARMUP):
    for a, fn in whole.items():
        v = sample_host(fn)
        if r >= WARMUP:
            host[a].append(v)
    for _ in range(20):                                    # short launches: twenty samples per round
        for a, fn in kernels.items():
            v = sample_events(fn)
            if r >= WARMUP:
                events[a].append(v)
ops.check_plans()

res = mask_optimization()
out = {"device": torch.cuda.get_device_name(0),
       "workload": f"{GRAPHS} graphs of configs[1] (2 to 16 nodes, seed {cfg.seed}): N = {N}, E = {wl.edge_index.size(1)}; AnswerModel of "
                   f"configs[1] (C = {cfg.channels}, {cfg.layers} layers, sampler {cfg.sampler} with seed {SEED}); T = {STEPS} Adam steps",
       "method": f"mask_optimization and the forward: a host clock around the call between two device synchronises; the step's launch "
                 f"and its torch formulation (sigmoid, row dot, regularisers, torch.optim.Adam, sigmoid, row scale): one call between "
                 f"two HIP events, which includes the host's time to queue the call's launches; {ROUNDS} rounds behind {WARMUP} "
                 f"discarded ones, the arms alternating inside a round",
       "host": {a: summary(v) for a, v in host.items()}, "events": {a: summary(v) for a, v in events.items()},
       "bytes_moved_per_step": int(3 * N * C * 4),
       "mean_nll_first": float(res.nll[0].mean()), "mean_nll_last": float(res.nll[-1].mean())}
out["mask_optimization_per_iteration_us"] = round(out["host"]["mask_optimization"]["median_us"] / max(STEPS, 1), 1)
out["mask_optimization_over_forward"] = round(out["host"]["mask_optimization"]["median_us"] / out["host"]["forward_no_grad"]["median_us"], 2)
out["torch_over_launch"] = round(out["events"]["maskopt_step_torch"]["median_us"] / out["events"]["maskopt_step_launch"]["median_us"], 2)
out["launch_share_of_iteration"] = round(out["events"]["maskopt_step_launch"]["median_us"] / out["mask_optimization_per_iteration_us"], 4)
for k in ("host", "events"):
    for a, v in out[k].items():
        print(f"{a}: {v}", flush=True)
for k in ("mask_optimization_per_iteration_us", "mask_optimization_over_forward", "torch_over_launch", "launch_share_of_iteration",
          "mean_nll_first", "mean_nll_last"):
    print(f"{k} = {out[k]}", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
