#!/usr/bin/env python3
"""The sampler entry points with a k per row (include/isg_topk_rows.h), every k_rows[b] = 5, against the scalar entry points at
k = 5, alternating in one process, HIP events.

  python tools/time_topk_rows.py [--rounds 10] [--out profiles/<name>.json]

Shape: the masked layer of BASELINE configs[1] -- 4096 ragged rows with synthetic.CFG2's node counts, k = 5.  Three operators:
the threshold solve (seeded noise), the Gumbel relaxation and its backward.  One sample = REPS calls between two events; per round
the scalar arm and the rows arm run one after the other; median, minimum and maximum over the rounds (two more are run first and
discarded).  The two arms' results are compared bit for bit before anything is timed.  A record, not a gate."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import ops, synthetic

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
ROUNDS, SKIP, REPS, K, TAU = int(opt.get("--rounds", 10)), 2, 50, 5, 1.0

gen = torch.Generator().manual_seed(synthetic.CFG2.seed)
sizes = synthetic.graph_sizes(synthetic.CFG2, gen)
batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes).to(dev)
plan = ops.GraphPlan.build(batch, None, num_graphs=sizes.numel())
g = torch.Generator(device=dev).manual_seed(1)
N = int(sizes.sum())
scores = torch.nn.functional.gelu(torch.randn(N, 1, device=dev, generator=g))
d_out = torch.randn(N, 1, device=dev, generator=g)
k_rows = torch.full((plan.B,), K, dtype=torch.int32, device=dev)

OPERATORS = {
    "topk_threshold": lambda k, cap: ops.topk_threshold(scores, k, plan=plan, noise_scale=1.0, seed=3, k_cap=cap),
    "topk_gumbel": lambda k, cap: ops.topk_gumbel(scores, k, TAU, plan=plan, seed=3, k_cap=cap),
    "topk_gumbel_backward": lambda k, cap: ops.topk_gumbel_backward(scores, d_out, k, TAU, plan=plan, seed=3, k_cap=cap),
}
ARMS = {"scalar": (K, None), "rows": (k_rows, K)}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / REPS


def median(v):
    return sorted(v)[len(v) // 2]


out = {"device": torch.cuda.get_device_name(0),
       "shape": f"configs[1] masked layer: {plan.B} ragged rows, {N} nodes, nmax {plan.nmax}, k {K} (rows arm: every k_rows[b] = {K}, k_cap {K})",
       "method": f"HIP events around {REPS} calls of the ops wrapper; {ROUNDS} rounds behind {SKIP} discarded ones, the two arms alternating "
                 f"inside a round; median (min-max) us per call, host launch cost included in both arms",
       "operators": {}}
with torch.no_grad():
    for name, fn in OPERATORS.items():
        res = {a: fn(*kc) for a, kc in ARMS.items()}
        assert torch.equal(res["scalar"].view(-1).view(torch.int32), res["rows"].view(-1).view(torch.int32)), f"{name}: the arms differ"
        us = {a: [] for a in ARMS}
        for r in range(ROUNDS + SKIP):
            for a, kc in ARMS.items():
                t = timed(lambda: fn(*kc))
                if r >= SKIP:
                    us[a].append(t)
        row = {a: {"median_us": round(median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for a, v in us.items()}
        spread = max(r["max_us"] - r["min_us"] for r in row.values())
        row["rows_minus_scalar_us"] = round(row["rows"]["median_us"] - row["scalar"]["median_us"], 2)
        row["larger_round_spread_us"] = round(spread, 2)
        row["rows_slower_beyond_spread"] = row["rows_minus_scalar_us"] > spread
        out["operators"][name] = row
        print(f"{name}: scalar {row['scalar']['median_us']:.2f} us ({row['scalar']['min_us']:.2f}-{row['scalar']['max_us']:.2f}), rows "
              f"{row['rows']['median_us']:.2f} us ({row['rows']['min_us']:.2f}-{row['rows']['max_us']:.2f}); rows - scalar "
              f"{row['rows_minus_scalar_us']:+.2f} us, larger spread {spread:.2f} us; bits equal", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
