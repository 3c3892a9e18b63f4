#!/usr/bin/env python3
"""Fidelity curves (include/ext/isg_curves.h) on 256 graphs drawn as BASELINE configs[1] draws them:
ops.curve_keep_bits (one launch) against its torch formulation -- a padded [B, nmax] stable argsort for the ranks, the level sizes
by torch.ceil, ops._pack_bits over the [2 B L, 32 W] flags --, and ops.curve_sums (one launch) against torch (the weighted sums,
the finiteness mask, the float64 totals).  The arms alternate in one process, HIP events around each call; median and p10 - p90
after warm-up.  Then explain.fidelity_curves for that batch on the AnswerModel of configs[1], by the host clock.

  python tools/time_curves.py [--graphs 256] [--rounds 200] [--out profiles/<name>.json]

Before anything is timed the two arms' outputs are compared (the bits as integers, the sums within fp32 rounding).  A record against
the torch formulation in the same process, not a gate."""
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
FRACTIONS = explain.CURVE_FRACTIONS
L = len(FRACTIONS)

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS, sampler="imle")
wl = synthetic.make_workload(cfg)
d = wl.to(dev)
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=GRAPHS, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                           graph_sizes=wl.graph_sizes)
scores = torch.randn(plan.N, generator=torch.Generator().manual_seed(1)).to(dev)
graphs = torch.arange(GRAPHS, dtype=torch.int32, device=dev)          # every graph of configs[1] has nodes: no copy for R
W = ops.keep_words(plan.nmax)
frac = torch.tensor(FRACTIONS, dtype=torch.float32, device=dev)
weights = explain.curve_weights(FRACTIONS).float().to(dev)


def kernel_bits():
    return ops.curve_keep_bits(scores, plan, graphs=graphs, fractions=FRACTIONS)


def torch_bits():
    """The same rows with torch ops: ranks from a stable descending argsort of the padded scores (the pads -inf, behind every
    node), k per (graph, level, side), flags, ops._pack_bits."""
    ptr = plan.ptr.long()
    n = ptr[1:] - ptr[:-1]
    local = torch.arange(plan.N, device=dev) - ptr.index_select(0, plan.batch)
    dense = torch.full((GRAPHS, 32 * W), float("-inf"), device=dev)
    dense[plan.batch, local] = scores
    order = torch.argsort(dense, dim=1, descending=True, stable=True)
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(32 * W, device=dev).expand(GRAPHS, -1))
    t = torch.ceil(frac.view(1, -1) * n.float().view(-1, 1)).long()
    k = torch.stack([torch.minimum(n.view(-1, 1), t.clamp_min(1)), torch.minimum(n.view(-1, 1) - 1, t.clamp_min(0))], dim=2)     # [B, L, 2]
    inside = (torch.arange(32 * W, device=dev).view(1, -1) < n.view(-1, 1)).view(GRAPHS, 1, 1, -1)
    below = rank.view(GRAPHS, 1, 1, -1) < k.unsqueeze(-1)
    flags = inside & torch.stack([below[:, :, 0], ~below[:, :, 1]], dim=2)
    return ops._pack_bits(flags.view(GRAPHS * L * 2, 32 * W), W), k.int(), rank


def kernel_sums(p, bits):
    return ops.curve_sums(p, bits, weights)


def torch_sums(p):
    v = p.view(GRAPHS, L, 2)
    fin = torch.isfinite(v).all(dim=1)
    auc = (v * weights.view(1, -1, 1)).sum(dim=1)
    safe = torch.where(fin.unsqueeze(1), v, torch.zeros_like(v)).double()
    area = torch.where(fin, auc, torch.zeros_like(auc)).double()
    totals = torch.cat([safe.sum(dim=0).t(), area.sum(dim=0).view(2, 1), fin.double().sum(dim=0).view(2, 1),
                        (~fin).double().sum(dim=0).view(2, 1)], dim=1)
    return torch.where(fin, auc, torch.full_like(auc, float("nan"))), totals


with torch.no_grad():
    bits = kernel_bits().verify()
    keep_t, k_t, rank_t = torch_bits()
    p = torch.rand(GRAPHS * L * 2, generator=torch.Generator().manual_seed(2)).to(dev)
    auc_k, tot_k = kernel_sums(p, bits)
    auc_t, tot_t = torch_sums(p)
    torch.cuda.synchronize()
    assert torch.equal(bits.keep, keep_t) and torch.equal(bits.level_k, k_t)
    local = torch.arange(plan.N, device=dev) - plan.ptr.long().index_select(0, plan.batch)
    assert torch.equal(bits.rank.long(), rank_t[plan.batch, local])
    assert float((auc_k - auc_t).abs().max()) <= 1e-6 and float((tot_k - tot_t).abs().max()) <= 1e-4
    ops.check_plans()


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


arms = {"curve_keep_bits": kernel_bits, "torch_keep_bits": torch_bits, "curve_sums": lambda: kernel_sums(p, bits),
        "torch_sums": lambda: torch_sums(p)}
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
       "workload": f"{GRAPHS} graphs of configs[1] (2 to 16 nodes, seed {cfg.seed}): N = {plan.N}; {L} fractions, both sides: "
                   f"{GRAPHS * L * 2} rows of {W} word(s)",
       "method": f"one call between two HIP events, and a host clock around the call and a synchronise; {ROUNDS} rounds behind "
                 f"{WARMUP} discarded ones, the arms alternating inside a round; a call includes its output allocations",
       "per_call": {"curve_keep_bits": "two allocations (one filled with -1 for the ranks), 1 launch",
                    "torch_keep_bits": "a padded scatter, a stable argsort, a scatter for the ranks, ceil / clamp / minimum for the "
                                       "level sizes, the flags, ops._pack_bits",
                    "curve_sums": "two allocations (the totals zeroed), 1 launch",
                    "torch_sums": "isfinite / all, a weighted sum, where, three float64 reductions, a concatenation"},
       "events": {a: summary(v) for a, v in events.items()}, "host": {a: summary(v) for a, v in host.items()}}
for a in arms:
    print(f"{a}: events {out['events'][a]}, host {out['host'][a]}", flush=True)
for kern, ref in (("curve_keep_bits", "torch_keep_bits"), ("curve_sums", "torch_sums")):
    out[f"{kern}_over_torch"] = round(out["events"][kern]["median_us"] / out["events"][ref]["median_us"], 4)
    print(f"{kern} / torch = {out[f'{kern}_over_torch']:.3f}", flush=True)

# explain.fidelity_curves on the AnswerModel of configs[1]: one forward on the batch, the ranking, the instance batch, one forward
model = synthetic.build_answer_model(cfg).eval().to(dev)
fc_us = []
with torch.no_grad():
    for r in range(3 + 10):
        t0 = time.perf_counter()
        res = explain.fidelity_curves(model, d, scores)
        torch.cuda.synchronize()
        if r >= 3:
            fc_us.append((time.perf_counter() - t0) * 1e6)
    ops.check_plans()
s = summary(fc_us)
out["fidelity_curves"] = {"model": f"AnswerModel of configs[1] (C = {cfg.channels}, {cfg.layers} layers, sampler {cfg.sampler})",
                          "instances": GRAPHS * L * 2, **s, "questions_per_second": round(GRAPHS / (s["median_us"] * 1e-6), 1),
                          "instances_per_second": round(GRAPHS * L * 2 / (s["median_us"] * 1e-6), 1)}
print(f"fidelity_curves: {out['fidelity_curves']}", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
