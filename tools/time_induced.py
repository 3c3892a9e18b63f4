#!/usr/bin/env python3
"""Induced-subgraph instances (include/ext/isg_induced.h): the leave-one-out batch of 256 graphs drawn as BASELINE
configs[1] draws them, made by ops.induced_instances in one pass (through its size copy) against the chain it replaces --
ops.graph_instances, a float mask built from the bits with torch ops, ops.subgraph_cut, .sizes().  The arms alternate in one
process, HIP events around each call; median and p10 - p90 after warm-up.  Then explain.occlusion for that batch on the
AnswerModel of configs[1], in questions per second.

  python tools/time_induced.py [--graphs 256] [--rounds 200] [--out profiles/<name>.json]

Before anything is timed the two arms' outputs are compared as integers.  A record, not a gate."""
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

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS)
wl = synthetic.make_workload(cfg)
d = wl.to(dev)
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=GRAPHS, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                           graph_sizes=wl.graph_sizes)
index, keep, inst_node = ops.keep_bits_leave_one_out(plan)
Q = index.numel()


def induced():
    return ops.induced_instances(plan, d.edge_index, index, keep)          # a 16-byte clear, 4 launches, 1 device-to-host copy


def chain():
    whole = ops.graph_instances(plan, d.edge_index, index)                  # a 16-byte clear, 3 launches, 1 device-to-host copy
    local = whole.node_src - plan.ptr.long()[index.long()][whole.batch]     # the float mask: torch ops
    mask = ((keep.long()[whole.batch, local >> 5] >> (local & 31)) & 1).float()
    cut = ops.subgraph_cut(mask, whole.edge_index, whole.plan())            # the instance batch's plan, then 3 launches
    cut.sizes()                                                             # the second device-to-host copy
    return whole, cut


def chain_without_the_plan(whole_plan):
    """The chain when the instance batch's GraphPlan is counted as needed anyway (a forward on the cut needs the CUT's plan, not
    this one): the same calls with the plan handed in."""
    whole = ops.graph_instances(plan, d.edge_index, index)
    whole._plan = whole_plan
    local = whole.node_src - plan.ptr.long()[index.long()][whole.batch]
    mask = ((keep.long()[whole.batch, local >> 5] >> (local & 31)) & 1).float()
    cut = ops.subgraph_cut(mask, whole.edge_index, whole_plan)
    cut.sizes()
    return whole, cut


with torch.no_grad():
    inst = induced()
    whole, cut = chain()
    torch.cuda.synchronize()
    assert torch.equal(inst.node_src, whole.node_src[cut.node_id]) and torch.equal(inst.edge_src, whole.edge_src[cut.edge_id])
    assert torch.equal(inst.edge_index, cut.edge_index) and torch.equal(inst.batch, cut.batch) and torch.equal(inst.ptr, cut.ptr)
    inst.verify()
    ops.check_plans()
    whole_plan = whole.plan()


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


arms = {"induced_instances": induced, "chain": chain, "chain_with_the_plan_handed_in": lambda: chain_without_the_plan(whole_plan)}
events, host = {a: [] for a in arms}, {a: [] for a in arms}
with torch.no_grad():
    for r in range(ROUNDS + WARMUP):
        for a, fn in arms.items():
            ev, ho = sample(fn)
            if r >= WARMUP:
                events[a].append(ev)
                host[a].append(ho)
    ops.check_plans()

out = {"device": torch.cuda.get_device_name(0),
       "workload": f"{GRAPHS} graphs of configs[1] (2 to 16 nodes, seed {cfg.seed}): N = {wl.x.size(0)}, E = {wl.edge_index.size(1)}; "
                   f"leave-one-out: Q = {Q} instances, N' = {inst.node_src.numel()}, E' = {inst.edge_src.numel()}; the whole copies "
                   f"of the chain: {whole.node_src.numel()} nodes, {whole.edge_src.numel()} edges",
       "method": f"one call between two HIP events (the call ends in its own device-to-host copy), and a host clock around the call "
                 f"and a synchronise; {ROUNDS} rounds behind {WARMUP} discarded ones, the arms alternating inside a round",
       "per_call": {"induced_instances": "a 16-byte clear, 4 launches (edge ranges, count, scan, fill), 1 device-to-host copy (16 bytes)",
                    "chain": "graph_instances: a 16-byte clear, 3 launches, 1 copy (8 bytes); the mask: torch ops (gathers, shifts, a cast); the "
                             "plan of the whole copies; subgraph_cut: 3 launches; sizes(): 1 copy (8 bytes)"},
       "events": {a: summary(v) for a, v in events.items()}, "host": {a: summary(v) for a, v in host.items()}}
for a in arms:
    print(f"{a}: events {out['events'][a]}, host {out['host'][a]}", flush=True)
ratio = out["events"]["induced_instances"]["median_us"] / out["events"]["chain"]["median_us"]
out["induced_over_chain"] = round(ratio, 4)
print(f"induced / chain = {ratio:.3f}", flush=True)

# explain.occlusion on the AnswerModel of configs[1]: one forward on the batch, the instance batch, one forward on it
model = synthetic.build_answer_model(cfg).eval().to(dev)
occ_us = []
with torch.no_grad():
    for r in range(3 + 10):
        t0 = time.perf_counter()
        occ = explain.occlusion(model, d, seed=3)
        torch.cuda.synchronize()
        if r >= 3:
            occ_us.append((time.perf_counter() - t0) * 1e6)
    ops.check_plans()
s = summary(occ_us)
out["occlusion"] = {"model": f"AnswerModel of configs[1] (C = {cfg.channels}, {cfg.layers} layers, sampler {cfg.sampler}, seed given: the "
                             f"attribution carries sampling noise)", "instances": Q, **s,
                    "questions_per_second": round(GRAPHS / (s["median_us"] * 1e-6), 1),
                    "instances_per_second": round(Q / (s["median_us"] * 1e-6), 1)}
print(f"occlusion: {out['occlusion']}", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
