#!/usr/bin/env python3
"""concat_instr layers: the row-biased Linear (models.mgat_v2_conv.CONCAT_SPLIT on; include/isg_concat.h) against the literal
torch.cat((x, instruction[batch]), 1) in front of the existing Linears (off); the arms alternate in one process, HIP events.

  python tools/time_concat_instr.py [--rounds 7] [--out profiles/<name>.json]

Batch: synthetic.CFG2's (BASELINE configs[1]: 4096 graphs, N = 82 286 nodes), C = 128, H = 4.
  (a) the x_l | x_r projection alone: the concatenation and ops.linear_fused at K = 2C, against P = instruction . W[:, C:]^T + b on
      the B instruction rows and ops.linear_rowbias at K = C;
  (b) one un-masked MaskingGATv2Conv(2C, C, heads=H, concat_instr=True): the forward in eval under no_grad, and forward + backward
      of sum(out * w) in train().
The arms' results are compared before anything is timed.  One sample = REPS calls between two events; per round the arms run one
after the other; median, minimum and maximum over the rounds (two more are run first and discarded).  The switch ships on iff
median(off) - median(on) exceeds the larger round spread and every round of on is below every round of off."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import isubgvqa_amd.models.mgat_v2_conv as MC
from isubgvqa_amd import ops, synthetic

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
ROUNDS, SKIP, REPS, H, C = int(opt.get("--rounds", 7)), 2, 10, 4, 128
HC = H * C


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / REPS


def rounds(arms):
    us = {a: [] for a in arms}
    for r in range(ROUNDS + SKIP):
        for a, fn in arms.items():
            t = timed(fn)
            if r >= SKIP:
                us[a].append(t)
    row = {a: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
           for a, v in us.items()}
    spread = max(row[a]["max_us"] - row[a]["min_us"] for a in ("off", "on"))
    gain = row["off"]["median_us"] - row["on"]["median_us"]
    row["on_vs_off"] = {"ratio": round(row["on"]["median_us"] / row["off"]["median_us"], 4), "gain_us": round(gain, 1),
                        "larger_round_spread_us": round(spread, 1),
                        "every_round_of_on_below_every_round_of_off": row["on"]["max_us"] < row["off"]["min_us"],
                        "ships_on": bool(gain > spread and row["on"]["max_us"] < row["off"]["min_us"])}
    return row


def show(name, row):
    for a in ("off", "on"):
        print(f"{name}, CONCAT_SPLIT {a}: {row[a]['median_us']:.1f} us ({row[a]['min_us']:.1f}-{row[a]['max_us']:.1f})", flush=True)
    v = row["on_vs_off"]
    print(f"{name}: on / off {v['ratio']:.3f}, gain {v['gain_us']:.1f} us against a round spread of {v['larger_round_spread_us']:.1f} us"
          f" -> ships {'on' if v['ships_on'] else 'off'}", flush=True)


wl = synthetic.make_workload(synthetic.CFG2).to(dev)
plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=wl.glf.size(0))
N, E, B = plan.N, plan.E, plan.B
torch.manual_seed(0)
layer = MC.MaskingGATv2Conv(2 * C, C, heads=H, edge_dim=C, add_self_loops=False, masking_threshold=1.0, use_instr=True,
                            concat_instr=True).to(dev)
ins = wl.instr[0].contiguous()
seg = wl.batch.int()
w = torch.randn(N, HC, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
out = {"device": torch.cuda.get_device_name(0), "batch": f"CFG2: N={N} E={E} B={B} H={H} C={C}",
       "method": f"HIP events around {REPS} calls; {ROUNDS} rounds behind {SKIP} discarded ones, the arms alternating inside a round; "
                 f"median (min-max) us per call"}


# ---- (a) the projection alone ----
def proj_off():
    return ops.linear_fused(torch.cat((wl.x, ins[wl.batch]), 1), (layer.lin_l, layer.lin_r))


def proj_on():
    return layer._project_split(wl.x, (ins, seg, plan.ptr), torch.float32)


with torch.no_grad():
    a, b = proj_off(), proj_on()
    torch.cuda.synchronize()
    err = max(float((p - q).abs().max()) for p, q in zip(a, b)) / float(a[0].abs().max())
    assert err < 1e-5, err
    out["projection_max_rel_diff"] = err
    del a, b
    out["projection"] = rounds({"off": proj_off, "on": proj_on})
show("x_l | x_r projection", out["projection"])


# ---- (b) one layer ----
def forward():
    with torch.no_grad():
        return layer(wl.x, wl.edge_index, wl.batch, edge_attr=wl.edge_attr, instruction=ins, imle_att=wl.glf, plan=plan)[0]


def step():
    for p in layer.parameters():
        p.grad = None
    o, _ = layer(wl.x, wl.edge_index, wl.batch, edge_attr=wl.edge_attr, instruction=ins, imle_att=wl.glf, plan=plan)
    (o * w).sum().backward()


def arm(fn, split):
    def run():
        MC.CONCAT_SPLIT = split
        return fn()
    return run


shipped = MC.CONCAT_SPLIT
layer.eval()
fa, fb = arm(forward, False)(), arm(forward, True)()
torch.cuda.synchronize()
err = float((fa - fb).abs().max()) / float(fa.abs().max())
assert err < 1e-5, err
out["layer_forward_max_rel_diff"] = err
del fa, fb
out["layer_forward"] = rounds({"off": arm(forward, False), "on": arm(forward, True)})
show("layer forward", out["layer_forward"])
layer.train()
out["layer_forward_backward"] = rounds({"off": arm(step, False), "on": arm(step, True)})
show("layer forward + backward", out["layer_forward_backward"])
MC.CONCAT_SPLIT = shipped
out["shipped"] = bool(shipped)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
