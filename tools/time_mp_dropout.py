#!/usr/bin/env python3
"""The message-passing forward + backward pair with attention dropout (include/isg_mp_train.h) at p = 0.1 against the same pair at
p = 0, alternating in one process, HIP events.

  python tools/time_mp_dropout.py [--rounds 10] [--out profiles/<name>.json]

Shapes: the layer of BASELINE configs[1] (synthetic.CFG2's batch: N = 82 286, E = 205 024, H = 4, C = 128; the grouped per-graph
forward kernel) and the reference's C = 300 layer on the same batch (the flat per-graph kernel; five channel passes in the
backward).  Both arms go through isg_gatv2_mp_fwd_dropout / isg_gatv2_mp_bwd_dropout: at p = 0 those are the launches of
isg_gatv2_mp_fwd / isg_gatv2_mp_bwd, the kernels without dropout; a third arm calls those two themselves, as the noise floor of
the comparison.  One sample = REPS pairs between two events; per round the arms run one after the other; median, minimum and
maximum over the rounds (two more are run first and discarded).  alpha of the arms is compared bit for bit before anything is
timed.  A record, not a gate."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import _lib, _lib_mp_train, ops, synthetic

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
ROUNDS, SKIP, REPS, H, SEED, SLOPE = int(opt.get("--rounds", 10)), 2, 10, 4, 0x5EED, 0.2
ARMS = {"existing": None, "p0": 0.0, "p0.1": 0.1}      # None: isg_gatv2_mp_fwd / isg_gatv2_mp_bwd themselves, the same launches as p0

wl = synthetic.make_workload(synthetic.CFG2).to(dev)
plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=wl.glf.size(0))
rowptr_s, eid_s, dst_s = plan.source_csr()
lib, lib0 = _lib_mp_train.load(), _lib.load()
N, E = plan.N, plan.E


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
       "method": f"HIP events around {REPS} forward + backward pairs of the C entry points; {ROUNDS} rounds behind {SKIP} discarded "
                 f"ones, the arms alternating inside a round; median (min-max) us per pair",
       "shapes": {}}
for C in (128, 300):
    HC = H * C
    g = torch.Generator(device=dev).manual_seed(C)
    x_l, x_r, grad = (torch.randn(N, HC, device=dev, generator=g) for _ in range(3))
    e_proj = torch.randn(E, HC, device=dev, generator=g)
    att = torch.randn(HC, device=dev, generator=g) / C ** 0.5
    bias = torch.randn(HC, device=dev, generator=g)
    res, alpha = torch.empty(N, HC, device=dev), torch.empty(E, H, device=dev)
    d_xl, d_xr, d_e = torch.empty(N, HC, device=dev), torch.empty(N, HC, device=dev), torch.empty(E, HC, device=dev)
    part = torch.empty((N + 15) // 16, HC, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: t.data_ptr()

    def pair(p):
        fwd, bwd, extra = (lib0.isg_gatv2_mp_fwd, lib0.isg_gatv2_mp_bwd, ()) if p is None else (
            lib.isg_gatv2_mp_fwd_dropout, lib.isg_gatv2_mp_bwd_dropout, (p, SEED))
        rc = fwd(p_(x_l), p_(x_r), p_(e_proj), p_(att), p_(bias), p_(plan.rowptr), p_(plan.eid), p_(plan.src),
                 0, 0, p_(res), p_(alpha), N, E, H, C, SLOPE, p_(plan.ptr), p_(plan.eptr), p_(plan.dst),
                 plan.B, plan.nmax, plan.emax, HC, HC, HC, *extra, st)
        assert rc == 0, rc
        rc = bwd(p_(x_l), p_(x_r), p_(e_proj), p_(att), p_(alpha), p_(grad), p_(plan.rowptr), p_(plan.eid),
                 p_(plan.src), p_(rowptr_s), p_(eid_s), p_(dst_s), 0, 0, p_(d_xl), p_(d_xr), p_(d_e),
                 p_(part), 0, N, E, H, C, SLOPE, *extra, st)
        assert rc == 0, rc

    alphas = {}
    for a, p in ARMS.items():
        pair(p)
        torch.cuda.synchronize()
        alphas[a] = alpha.clone()
        assert bool(torch.isfinite(res).all()) and bool(torch.isfinite(d_xl).all())
    assert torch.equal(alphas["p0"], alphas["p0.1"]) and torch.equal(alphas["p0"], alphas["existing"]), "dropout touched the softmax"
    us = {a: [] for a in ARMS}
    for r in range(ROUNDS + SKIP):
        for a, p in ARMS.items():
            t = timed(lambda: pair(p))
            if r >= SKIP:
                us[a].append(t)
    row = {a: {"median_us": round(median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for a, v in us.items()}
    row["ratio"] = round(row["p0.1"]["median_us"] / row["p0"]["median_us"], 4)
    row["p0_over_existing"] = round(row["p0"]["median_us"] / row["existing"]["median_us"], 4)
    row["p0_round_spread"] = round((row["p0"]["max_us"] - row["p0"]["min_us"]) / row["p0"]["median_us"], 4)
    out["shapes"][f"N={N} E={E} H={H} C={C}"] = row
    print(f"C={C}: existing entry points {row['existing']['median_us']:.1f} us ({row['existing']['min_us']:.1f}-{row['existing']['max_us']:.1f}); "
          f"p = 0 / existing {row['p0_over_existing']:.3f}", flush=True)
    print(f"C={C}: p = 0 {row['p0']['median_us']:.1f} us ({row['p0']['min_us']:.1f}-{row['p0']['max_us']:.1f}), p = 0.1 "
          f"{row['p0.1']['median_us']:.1f} us ({row['p0.1']['min_us']:.1f}-{row['p0.1']['max_us']:.1f}); ratio {row['ratio']:.3f}, "
          f"spread of the p = 0 rounds {100 * row['p0_round_spread']:.1f} %; alpha bits equal", flush=True)
    del x_l, x_r, grad, e_proj, res, alpha, d_xl, d_xr, d_e, part
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
