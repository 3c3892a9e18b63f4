#!/usr/bin/env python3
"""Integrated gradients (include/ext/isg_ig.h) on DESIGN.md 34's batch: 256 graphs drawn as BASELINE configs[1]
draws them, the AnswerModel of configs[1].  Four arms alternate in one process, a host clock around each call and a device
synchronise, median and p10 - p90 after warm-up: the no_grad forward, explain.integrated_gradients at S = 16,
explain.occlusion, and -- between HIP events -- ops.ig_attribution on the S = 16 instance batch beside its torch formulation
(index_select of every row's copies, a weighted sum, an einsum with x).

  python tools/time_ig.py [--graphs 256] [--steps 16] [--rounds 30] [--out profiles/<name>.json]

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
GRAPHS, STEPS, ROUNDS, WARMUP = int(opt.get("--graphs", 256)), int(opt.get("--steps", 16)), int(opt.get("--rounds", 30)), 5
SEED = 3                                                   # the Gumbel sampler's: the same noise in every arm

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS)
wl = synthetic.make_workload(cfg)
d = wl.to(dev)
model = synthetic.build_answer_model(cfg).eval().to(dev)
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=GRAPHS, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                           graph_sizes=wl.graph_sizes)
N, C = d.x.shape

# the attribution launch and its torch formulation on the same gradient rows: S copies of every graph, next to each other
with torch.no_grad():
    inst = ops.graph_instances(plan, d.edge_index, torch.arange(GRAPHS * STEPS) // STEPS, sizes=plan.sizes_host)
    gen = torch.Generator(device=dev).manual_seed(5)
    g_rows = torch.randn(inst.node_src.numel(), C, device=dev, generator=gen)
    w = torch.rand(GRAPHS * STEPS, device=dev, generator=gen)
    # copy s of node n sits at inst.ptr[graph * S + s] + (n - ptr[graph])
    graph = d.batch
    local = torch.arange(N, device=dev) - plan.ptr.long()[graph]
    q = graph.unsqueeze(1) * STEPS + torch.arange(STEPS, device=dev).unsqueeze(0)                   # [N, S]
    copies = (inst.ptr.long()[q] + local.unsqueeze(1)).reshape(-1)
    w_rows = w[q]                                                                                    # [N, S]


def attribution_launch():
    return ops.ig_attribution(inst, g_rows, None, w, d.x, d.edge_attr).attr_x


def attribution_torch():
    G = (g_rows.index_select(0, copies).view(N, STEPS, C) * w_rows.unsqueeze(2)).sum(1)
    return torch.einsum("nc,nc->n", d.x, G)


with torch.no_grad():
    a, b = attribution_launch(), attribution_torch()
    torch.cuda.synchronize()
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= 1e-5 * scale, "the launch differs from its torch formulation"


def forward():
    return model(d, seed=SEED, plan=plan)


def integrated_gradients():
    return explain.integrated_gradients(model, d, seed=SEED, steps=STEPS)


def occlusion():
    return explain.occlusion(model, d, seed=SEED)


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


whole = {"forward_no_grad": forward, "integrated_gradients": integrated_gradients, "occlusion": occlusion}
kernels = {"ig_attribution_launch": attribution_launch, "ig_attribution_torch": attribution_torch}
host = {a: [] for a in whole}
events = {a: [] for a in kernels}
for r in range(ROUNDS + WARMUP):
    for a, fn in whole.items():
        if a == "integrated_gradients":                    # (it enters torch.enable_grad() itself, around the score only)
            v = sample_host(fn)
        else:
            with torch.no_grad():
                v = sample_host(fn)
        if r >= WARMUP:
            host[a].append(v)
    with torch.no_grad():
        for _ in range(10):                                # short launches: ten samples per round
            for a, fn in kernels.items():
                v = sample_events(fn)
                if r >= WARMUP:
                    events[a].append(v)
ops.check_plans()

res = integrated_gradients()
out = {"device": torch.cuda.get_device_name(0),
       "workload": f"{GRAPHS} graphs of configs[1] (2 to 16 nodes, seed {cfg.seed}): N = {N}, E = {wl.edge_index.size(1)}; AnswerModel of "
                   f"configs[1] (C = {cfg.channels}, {cfg.layers} layers, sampler {cfg.sampler} with seed {SEED}); S = {STEPS} steps: "
                   f"{GRAPHS * STEPS} instances, N' = {inst.node_src.numel()} rows",
       "method": f"whole explainers: a host clock around the call between two device synchronises; the attribution launch and its torch "
                 f"formulation: one call between two HIP events; {ROUNDS} rounds behind {WARMUP} discarded ones, the arms alternating "
                 f"inside a round",
       "host": {a: summary(v) for a, v in host.items()}, "events": {a: summary(v) for a, v in events.items()},
       "bytes_read_once": int(inst.node_src.numel() * C * 4),
       "mean_abs_delta": float(res.delta.abs().mean()), "mean_abs_f_input_minus_f_baseline": float((res.f_input - res.f_baseline).abs().mean())}
fw = out["host"]["forward_no_grad"]["median_us"]
out["integrated_gradients_over_forward"] = round(out["host"]["integrated_gradients"]["median_us"] / fw, 2)
out["occlusion_over_integrated_gradients"] = round(out["host"]["occlusion"]["median_us"] / out["host"]["integrated_gradients"]["median_us"], 2)
out["torch_over_launch"] = round(out["events"]["ig_attribution_torch"]["median_us"] / out["events"]["ig_attribution_launch"]["median_us"], 2)
out["launch_gbytes_per_s"] = round(out["bytes_read_once"] / out["events"]["ig_attribution_launch"]["median_us"] / 1e3, 1)
for k in ("host", "events"):
    for a, v in out[k].items():
        print(f"{a}: {v}", flush=True)
for k in ("integrated_gradients_over_forward", "occlusion_over_integrated_gradients", "torch_over_launch", "launch_gbytes_per_s",
          "mean_abs_delta", "mean_abs_f_input_minus_f_baseline"):
    print(f"{k} = {out[k]}", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
