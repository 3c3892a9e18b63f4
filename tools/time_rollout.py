#!/usr/bin/env python3
"""Attention rollout (include/ext/isg_rollout.h) on DESIGN.md 34's batch: 256 graphs drawn as BASELINE configs[1]
draws them, the AnswerModel of configs[1].  Three arms alternate in one process, HIP events around each call, median and
p10 - p90 after warm-up: the forward alone, the forward with a trace (every layer stores its attention weights), and the rollout
launch on that trace (ops.attention_rollout: the table, one launch).  Then explain.attention_rollout as a whole and
explain.occlusion on the same batch in the same run, for the ratio.

  python tools/time_rollout.py [--graphs 256] [--rounds 200] [--out profiles/<name>.json]

Before anything is timed the traced forward is compared with the plain one as bits.  A record, not a gate."""
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
GRAPHS, ROUNDS, WARMUP = int(opt.get("--graphs", 256)), int(opt.get("--rounds", 200)), 20
SEED = 3                                                   # the Gumbel sampler's: the same mask in every arm

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS)
wl = synthetic.make_workload(cfg)
d = wl.to(dev)
model = synthetic.build_answer_model(cfg).eval().to(dev)
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=GRAPHS, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                           graph_sizes=wl.graph_sizes)
trace = explain.AttentionTrace()


def forward():
    return model(d, seed=SEED, plan=plan)


def forward_traced():
    return model(d, seed=SEED, plan=plan, trace=trace)


with torch.no_grad():
    plain, traced = forward(), forward_traced()
    torch.cuda.synchronize()
    for a, b in zip(plain, traced):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a forward with a trace differs from the forward without it"
    start = (trace.gate.float().reshape(-1) * trace.mask.float().reshape(-1)).contiguous()
    plan.source_csr()                                      # built once per plan, on first use: not part of a launch
    alphas, masks = trace.alphas, trace.masks


def rollout():
    return ops.attention_rollout(plan, alphas, start, masks, residual=0.5)


def sample(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3, (time.perf_counter() - t0) * 1e6


def summary(v):
    v = sorted(v)
    at = lambda q: round(v[min(len(v) - 1, int(q * len(v)))], 1)
    return {"median_us": at(0.5), "p10_us": at(0.1), "p90_us": at(0.9)}


arms = {"forward": forward, "forward_with_trace": forward_traced, "rollout_launch": rollout}
events, host = {a: [] for a in arms}, {a: [] for a in arms}
with torch.no_grad():
    for r in range(ROUNDS + WARMUP):
        for a, fn in arms.items():
            ev, ho = sample(fn)
            if r >= WARMUP:
                events[a].append(ev)
                host[a].append(ho)
    ops.check_plans()

H = alphas[0].size(1)
out = {"device": torch.cuda.get_device_name(0),
       "workload": f"{GRAPHS} graphs of configs[1] (2 to 16 nodes, seed {cfg.seed}): N = {wl.x.size(0)}, E = {wl.edge_index.size(1)}; "
                   f"AnswerModel of configs[1] (C = {cfg.channels}, {cfg.layers} layers, H = {H}, sampler {cfg.sampler} with seed {SEED})",
       "method": f"one call between two HIP events, and a host clock around the call and a synchronise; {ROUNDS} rounds behind "
                 f"{WARMUP} discarded ones, the arms alternating inside a round; the plan and its CSR by source are built before",
       "events": {a: summary(v) for a, v in events.items()}, "host": {a: summary(v) for a, v in host.items()}}
for a in arms:
    print(f"{a}: events {out['events'][a]}, host {out['host'][a]}", flush=True)

whole = {"attention_rollout": lambda: explain.attention_rollout(model, d, seed=SEED),
         "occlusion": lambda: explain.occlusion(model, d, seed=SEED)}
wall = {a: [] for a in whole}
with torch.no_grad():
    for r in range(3 + 10):
        for a, fn in whole.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 3:
                wall[a].append((time.perf_counter() - t0) * 1e6)
    ops.check_plans()
out["explainers_host_clock"] = {a: summary(v) for a, v in wall.items()}
ratio = out["explainers_host_clock"]["occlusion"]["median_us"] / out["explainers_host_clock"]["attention_rollout"]["median_us"]
out["occlusion_over_attention_rollout"] = round(ratio, 2)
for a in whole:
    print(f"explain.{a}: {out['explainers_host_clock'][a]}", flush=True)
print(f"occlusion / attention_rollout = {ratio:.2f}", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
