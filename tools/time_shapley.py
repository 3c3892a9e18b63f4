#!/usr/bin/env python3
"""Shapley sampling (include/ext/isg_shapley.h) on 256 graphs drawn as BASELINE configs[1] draws them:
ops.shapley_keep_bits (one launch) against its torch formulation -- the same Philox keys (made once on the host with
oracle/philox.py and uploaded: torch has no counter-based draw to time) padded to [B, T, nmax], a stable argsort for the positions,
the antithetic twins, the prefix flags and ops._pack_bits --, and ops.shapley_values (one launch) against torch (gathers from the
instance probabilities, the pair means, the sums).  The arms alternate in one process, HIP events around each call; median and
p10 - p90 after warm-up.  Then explain.shapley_values and explain.occlusion for that batch on the AnswerModel of configs[1], by the
host clock.

  python tools/time_shapley.py [--graphs 256] [--rounds 200] [--permutations 16] [--out profiles/<name>.json]

Before anything is timed the two arms' outputs are compared (positions and bits as integers, the estimates within fp32 rounding).
A record against the torch formulation in the same process, not a gate."""
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isubgvqa_amd import explain, ops, synthetic
from oracle import philox

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
GRAPHS, ROUNDS, WARMUP = int(opt.get("--graphs", 256)), int(opt.get("--rounds", 200)), 20
M, SEED = int(opt.get("--permutations", 16)), 0x5EED
T = M // 2

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS, sampler="imle")
wl = synthetic.make_workload(cfg)
d = wl.to(dev)
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=GRAPHS, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                           graph_sizes=wl.graph_sizes)
graphs = torch.arange(GRAPHS, dtype=torch.int32, device=dev)
W = ops.keep_words(plan.nmax)
CAP = 32 * W
ptr = plan.ptr.long()
n = ptr[1:] - ptr[:-1]
local = torch.arange(plan.N, device=dev) - ptr.index_select(0, plan.batch)
g_, t_, i_ = np.meshgrid(np.arange(GRAPHS, dtype=np.uint64), np.arange(T, dtype=np.uint64), np.arange(CAP, dtype=np.uint64), indexing="ij")
keys = torch.from_numpy(philox.draw(SEED, g_, np.uint64(0x80000000) | (t_ << np.uint64(11)) | i_).astype(np.int64)).to(dev)    # [B, T, CAP]
inside = (torch.arange(CAP, device=dev).view(1, -1) < n.view(-1, 1))                                  # [B, CAP]
rows = (M * (n - 1).clamp_min(0))
row_ptr = torch.cat([rows.new_zeros(1), torch.cumsum(rows, 0)])
Q = int(row_ptr[-1])
# row q of the torch arm: (graph, permutation, k) of every row, made once (the kernel's caller forms row_ptr per call; it is cheap)
row_g = torch.repeat_interleave(torch.arange(GRAPHS, device=dev), rows)
within = torch.arange(Q, device=dev) - row_ptr[:-1].index_select(0, row_g)
per = (n - 1).index_select(0, row_g)
row_m, row_k = within // per, within % per + 1


def kernel_bits():
    return ops.shapley_keep_bits(plan, graphs=graphs, permutations=M, antithetic=True, seed=SEED)


def torch_bits():
    """The same positions and rows with torch ops: the pads get the largest key (behind every node), a stable ascending argsort
    gives the order, a scatter the positions, the odd permutations are the reversals, the flags go through ops._pack_bits."""
    padded = torch.where(inside.view(GRAPHS, 1, CAP), keys, torch.full_like(keys, 1 << 32))
    order = torch.argsort(padded, dim=2, stable=True)
    pos = torch.empty_like(order).scatter_(2, order, torch.arange(CAP, device=dev).expand(GRAPHS, T, -1))
    both = torch.stack([pos, n.view(-1, 1, 1) - 1 - pos], dim=2).view(GRAPHS, M, CAP)                 # [B, M, CAP]
    flags = inside.index_select(0, row_g) & (both[row_g, row_m] < row_k.view(-1, 1))
    return ops._pack_bits(flags, W), both


def kernel_values(p_inst, p, bits):
    return ops.shapley_values(p_inst, p, bits, plan)


def torch_values(p_inst, p, pos_nodes):
    """pos_nodes int64 [M, N].  Two gathers per (permutation, node), the ends from p and 0, pair means, sums."""
    first = row_ptr[:-1].index_select(0, plan.batch).view(1, -1)
    nn = n.index_select(0, plan.batch).view(1, -1)
    base = first + torch.arange(M, device=dev).view(-1, 1) * (nn - 1)
    padded = torch.cat([p_inst, p_inst.new_zeros(1)])
    hi = torch.where(pos_nodes + 1 >= nn, p.index_select(0, plan.batch).view(1, -1), padded[(base + pos_nodes).clamp(max=Q)])
    lo = torch.where(pos_nodes == 0, torch.zeros_like(hi), padded[(base + pos_nodes - 1).clamp(0, Q)])
    e = 0.5 * ((hi - lo)[0::2] + (hi - lo)[1::2])
    phi = e.sum(dim=0) / T
    total = torch.zeros(GRAPHS, device=dev).index_add_(0, plan.batch, phi)
    return phi, (e * e).sum(dim=0), total - p


with torch.no_grad():
    bits = kernel_bits().verify()
    keep_t, pos_t = torch_bits()
    pos_nodes = pos_t[plan.batch, :, local].t().contiguous()
    p_inst = torch.rand(Q, generator=torch.Generator().manual_seed(2)).to(dev)
    p = torch.rand(GRAPHS, generator=torch.Generator().manual_seed(3)).to(dev)
    phi_k, m2_k, gap_k, flag_k = kernel_values(p_inst, p, bits)
    phi_t, m2_t, gap_t = torch_values(p_inst, p, pos_nodes)
    torch.cuda.synchronize()
    assert bits.Q == Q and torch.equal(bits.row_ptr.long(), row_ptr) and torch.equal(bits.keep, keep_t)
    assert torch.equal(bits.pos.long(), pos_nodes) and torch.equal(bits.index.long(), row_g)
    assert float((phi_k - phi_t).abs().max()) <= 1e-6 and float((m2_k - m2_t).abs().max()) <= 1e-5 and int(flag_k.abs().sum()) == 0
    assert float((gap_k - gap_t).abs().max()) <= 1e-5
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


arms = {"shapley_keep_bits": kernel_bits, "torch_keep_bits": torch_bits, "shapley_values": lambda: kernel_values(p_inst, p, bits),
        "torch_values": lambda: torch_values(p_inst, p, pos_nodes)}
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
       "workload": f"{GRAPHS} graphs of configs[1] (2 to 16 nodes, seed {cfg.seed}): N = {plan.N}; {M} antithetic permutations: "
                   f"{Q} rows of {W} word(s)",
       "method": f"one call between two HIP events, and a host clock around the call and a synchronise; {ROUNDS} rounds behind "
                 f"{WARMUP} discarded ones, the arms alternating inside a round; a call includes its output allocations",
       "per_call": {"shapley_keep_bits": "row_ptr with torch ops (clamp, index_select, cumsum), the 4-byte copy of Q, two allocations "
                                         "(pos filled with -1), 1 launch that draws the keys itself",
                    "torch_keep_bits": "keys uploaded beforehand and the (graph, permutation, k) of every row made beforehand; the "
                                       "padding, a stable argsort, a scatter for the positions, the reversals, the flags, ops._pack_bits",
                    "shapley_values": "two allocations (zeroed), 1 launch",
                    "torch_values": "two padded gathers per (permutation, node), where for the ends, the pair means, two sums over the "
                                    "samples, an index_add for the gap"},
       "events": {a: summary(v) for a, v in events.items()}, "host": {a: summary(v) for a, v in host.items()}}
for a in arms:
    print(f"{a}: events {out['events'][a]}, host {out['host'][a]}", flush=True)
for kern, ref in (("shapley_keep_bits", "torch_keep_bits"), ("shapley_values", "torch_values")):
    out[f"{kern}_over_torch"] = round(out["events"][kern]["median_us"] / out["events"][ref]["median_us"], 4)
    print(f"{kern} / torch = {out[f'{kern}_over_torch']:.3f}", flush=True)

# explain.shapley_values beside explain.occlusion on the AnswerModel of configs[1], by the host clock
model = synthetic.build_answer_model(cfg).eval().to(dev)
whole = {"shapley_values": [], "occlusion": []}
with torch.no_grad():
    for r in range(3 + 10):
        for name, fn in (("shapley_values", lambda: explain.shapley_values(model, d, permutations=M, perm_seed=SEED)),
                         ("occlusion", lambda: explain.occlusion(model, d))):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if r >= 3:
                whole[name].append((time.perf_counter() - t0) * 1e6)
    ops.check_plans()
for name, instances in (("shapley_values", Q), ("occlusion", int(plan.N))):
    s = summary(whole[name])
    out[f"explain_{name}"] = {"model": f"AnswerModel of configs[1] (C = {cfg.channels}, {cfg.layers} layers, sampler {cfg.sampler})",
                              "instances": instances, **s, "questions_per_second": round(GRAPHS / (s["median_us"] * 1e-6), 1),
                              "instances_per_second": round(instances / (s["median_us"] * 1e-6), 1)}
    print(f"explain.{name}: {out[f'explain_{name}']}", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
