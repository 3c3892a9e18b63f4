#!/usr/bin/env python3
"""Training on fp16 feature rows (include/isg_mp_f16_train.h) against fp32 rows: the message-passing backward's two launches
through the C entry points, one layer's forward + backward through the module, and the peak memory of that layer; the arms
alternate in one process, HIP events.

  python tools/time_mp_f16_train.py [--rounds 10] [--out profiles/<name>.json]

Kernel pair: isg_gatv2_mp_bwd on fp32 rows against isg_gatv2_mp_bwd_f16 on the same rows rounded to half (dense, and as inference
lays them out: x_l | x_r the column halves of one [N, 2 H C] buffer, d_x_l | d_x_r written into one), H = 4, C = 128, on the batch of
synthetic.CFG2 (BASELINE configs[1]) and of synthetic.CFG5 (Pareto sizes, power-law in-degree).  The results of the arms are
compared bit for bit before anything is timed.
Layer: MaskingGATv2Conv(128, 128, heads=4, edge_dim=128).train(), un-masked, feature_dtype fp32 against half, forward + backward
of sum(out * w) on CFG2's batch; torch.cuda.max_memory_allocated over one forward + backward and the bytes the forward leaves
allocated for the backward.
One sample = REPS calls between two events; per round the arms run one after the other; median, minimum and maximum over the
rounds (two more are run first and discarded).  A record, not a gate."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import _lib, _lib_mp_f16_train, ops, synthetic
from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
ROUNDS, SKIP, REPS, H, C, SLOPE = int(opt.get("--rounds", 10)), 2, 10, 4, 128, 0.2
HC = H * C
lib0, lib = _lib.load(), _lib_mp_f16_train.load()


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


def rounds(arms):
    us = {a: [] for a in arms}
    for r in range(ROUNDS + SKIP):
        for a, fn in arms.items():
            t = timed(fn)
            if r >= SKIP:
                us[a].append(t)
    return {a: {"median_us": round(median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for a, v in us.items()}


def verdict(row, base, arm):
    """`arm` against `base`: the ratio of the medians, and whether the difference exceeds the larger round spread."""
    spread = max(row[a]["max_us"] - row[a]["min_us"] for a in (base, arm))
    diff = row[arm]["median_us"] - row[base]["median_us"]
    return {"ratio": round(row[arm]["median_us"] / row[base]["median_us"], 4), "diff_us": round(diff, 1),
            "larger_round_spread_us": round(spread, 1),
            "verdict": "faster" if diff < -spread else "slower" if diff > spread else "within the round spread"}


out = {"device": torch.cuda.get_device_name(0),
       "method": f"HIP events around {REPS} calls; {ROUNDS} rounds behind {SKIP} discarded ones, the arms alternating inside a "
                 f"round; median (min-max) us per call", "kernel_pair": {}, "layer": {}}
p_ = lambda t: t.data_ptr()
for name, cfg in (("CFG2", synthetic.CFG2), ("CFG5", synthetic.CFG5)):
    wl = synthetic.make_workload(cfg).to(dev)
    plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=wl.glf.size(0))
    rowptr_s, eid_s, dst_s = plan.source_csr()
    N, E = plan.N, plan.E
    g = torch.Generator(device=dev).manual_seed(C)
    xlr_h = torch.randn(N, 2 * HC, device=dev, generator=g).half()
    e_h = torch.randn(E, HC, device=dev, generator=g).half()
    grad = torch.randn(N, HC, device=dev, generator=g)
    att = torch.randn(HC, device=dev, generator=g) / C ** 0.5
    xl_h, xr_h = xlr_h[:, :HC].contiguous(), xlr_h[:, HC:].contiguous()
    xl_f, xr_f, e_f = xl_h.float(), xr_h.float(), e_h.float()
    with torch.no_grad():
        _, alpha = ops.gatv2_mp(xl_f, xr_f, e_f, att.view(1, H, C), plan, H)
    res = {a: [torch.empty(N, 2 * HC, device=dev), torch.empty(E, HC, device=dev), torch.empty((N + 15) // 16, HC, device=dev)]
           for a in ("fp32", "half", "half_strided")}
    st = torch.cuda.current_stream().cuda_stream
    csr = (p_(plan.rowptr), p_(plan.eid), p_(plan.src), p_(rowptr_s), p_(eid_s), p_(dst_s), 0, 0)

    def fp32():
        lr, de, part = res["fp32"]
        rc = lib0.isg_gatv2_mp_bwd(p_(xl_f), p_(xr_f), p_(e_f), p_(att), p_(alpha), p_(grad), *csr, p_(lr), p_(lr) + 4 * N * HC, p_(de),
                                   p_(part), 0, N, E, H, C, SLOPE, st)
        assert rc == 0, rc

    def half():
        lr, de, part = res["half"]
        rc = lib.isg_gatv2_mp_bwd_f16(p_(xl_h), p_(xr_h), p_(e_h), p_(att), p_(alpha), p_(grad), *csr, p_(lr), p_(lr) + 4 * N * HC,
                                      p_(de), p_(part), 0, N, E, H, C, SLOPE, 0, 0, 0, 0, 0, st)
        assert rc == 0, rc

    def half_strided():
        lr, de, part = res["half_strided"]
        rc = lib.isg_gatv2_mp_bwd_f16(p_(xlr_h), p_(xlr_h) + 2 * HC, p_(e_h), p_(att), p_(alpha), p_(grad), *csr, p_(lr),
                                      p_(lr) + 4 * HC, p_(de), p_(part), 0, N, E, H, C, SLOPE, 2 * HC, 2 * HC, 0, 2 * HC, 2 * HC, st)
        assert rc == 0, rc

    arms = {"fp32": fp32, "half": half, "half_strided": half_strided}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ref = res["fp32"]
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(res["half"][0], ref[0]) and same(res["half"][1], ref[1]) and same(res["half"][2], ref[2]), "half rows: other bits"
    dl, dr = ref[0].view(2, N, HC)
    assert same(res["half_strided"][0], torch.cat([dl, dr], dim=1)) and same(res["half_strided"][1], ref[1]), "strided: other bits"
    row = rounds(arms)
    row["half_vs_fp32"] = verdict(row, "fp32", "half")
    row["half_strided_vs_fp32"] = verdict(row, "fp32", "half_strided")
    out["kernel_pair"][f"{name}: N={N} E={E} H={H} C={C}"] = row
    for a in arms:
        print(f"{name} K1 + K2, {a}: {row[a]['median_us']:.1f} us ({row[a]['min_us']:.1f}-{row[a]['max_us']:.1f})", flush=True)
    print(f"{name}: half / fp32 {row['half_vs_fp32']['ratio']:.3f} ({row['half_vs_fp32']['verdict']}), strided "
          f"{row['half_strided_vs_fp32']['ratio']:.3f} ({row['half_strided_vs_fp32']['verdict']}); bits equal", flush=True)
    if name == "CFG2":
        keep = (wl, plan, N, E)
    del xlr_h, e_h, xl_h, xr_h, xl_f, xr_f, e_f, res, grad, alpha

# ---- one layer through the module ----
wl, plan, N, E = keep
torch.manual_seed(0)
layers = {}
for mode, dt in (("fp32", torch.float32), ("half", torch.float16)):
    torch.manual_seed(0)
    m = MaskingGATv2Conv(C, C, heads=H, edge_dim=C, add_self_loops=False, masking_threshold=1.0, use_instr=True).to(dev).train()
    m.feature_dtype = dt
    layers[mode] = m
w = torch.randn(N, HC, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
ins = wl.instr[0].contiguous()


def step(m):
    def run():
        for p in m.parameters():
            p.grad = None
        out, _ = m(wl.x, wl.edge_index, wl.batch, edge_attr=wl.edge_attr, instruction=ins, imle_att=wl.glf, plan=plan)
        (out * w).sum().backward()
    return run


mem = {}
for mode, m in layers.items():
    step(m)()                                                  # warm: plans, caches
    torch.cuda.synchronize()
    for p in m.parameters():
        p.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out_, _ = m(wl.x, wl.edge_index, wl.batch, edge_attr=wl.edge_attr, instruction=ins, imle_att=wl.glf, plan=plan)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    (out_ * w).sum().backward()
    torch.cuda.synchronize()
    mem[mode] = {"held_after_forward_MB": round(held / 1e6, 1), "peak_over_step_MB": round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)}
    del out_
ops.reset_counters()
row = rounds({mode: step(m) for mode, m in layers.items()})
assert ops.counters()["mp_f16_train"] == (ROUNDS + SKIP) * REPS, "the half layer did not run the half-row backward"
row["half_vs_fp32"] = verdict(row, "fp32", "half")
row["memory"] = mem
out["layer"][f"CFG2: N={N} E={E} H={H} C={C} K={C}, forward + backward"] = row
for mode in layers:
    print(f"layer forward + backward, {mode}: {row[mode]['median_us']:.1f} us ({row[mode]['min_us']:.1f}-{row[mode]['max_us']:.1f}); held after "
          f"the forward {mem[mode]['held_after_forward_MB']} MB, peak over the step {mem[mode]['peak_over_step_MB']} MB", flush=True)
print(f"layer: half / fp32 {row['half_vs_fp32']['ratio']:.3f} ({row['half_vs_fp32']['verdict']})", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
