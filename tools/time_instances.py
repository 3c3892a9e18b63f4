#!/usr/bin/env python3
"""Many questions per scene graph (include/isg_instances.h): the full model in eval() at ~4 096 questions, the
replicated forward (every question brings a copy of its graph) against ISubGVQA.encode_scene + ask (the encoder runs on the
distinct graphs, the instances are expanded on the device) at 1, 4 and 12 questions per graph; the arms alternate in one process,
HIP events.

  python tools/time_instances.py [--questions 4096] [--rounds 6] [--out profiles/<name>.json]

Per setting, besides the two whole forwards: the scene-graph encoder alone on the replicated batch (its share of the replicated
forward) and on the distinct batch, the expansion (ops.graph_instances with host sizes: a 16-byte clear and three launches), the row
gather (isg_instance_rows) and a device-to-device copy of the same rows (the copy rate the gather is held against).
Before anything is timed the two forwards are compared: questions whose top-k mask differs are counted (an untrained model's gate
scores lie within 1e-4 of each other for a few questions in a thousand, and the encoder's Linears take other kernels at G rows than
at Q rows), and on all other questions the logits must agree within 1e-4 and the gates within 1e-5.
One sample = REPS calls between two events; per round the arms run one after the other; median, minimum and maximum over the
rounds (two more are run first and discarded).  A record, not a gate.

  python tools/time_instances.py --train [--questions 4096] [--rounds 6] [--out profiles/<name>.json]

Training through shared encodings (include/ext/isg_instances_train.h), the same method in train(): forward +
backward of the replicated step (forward() on the batch with every graph copied out) against the shared one
(ISubGVQA.forward_shared: the encoder once per distinct graph with weighted BatchNorm statistics, the instance rows' backward as
one launch) at 1, 4 and 12 questions per graph.  Besides the two steps: the new launch alone (isg_instance_rows_bwd), a device
copy_ of the same rows (the rate it is held against) and the generic route it replaces, ops.token_csr over the N' + E' row numbers
+ isg_segment_rows_sum (two stable device sorts per step)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import ops, synthetic
from isubgvqa_amd.models import build_model

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
QUESTIONS, ROUNDS, SKIP, REPS = int(opt.get("--questions", 4096)), int(opt.get("--rounds", 6)), 2, 3


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


def train_main():
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(sampler_type="gumbel"), None).to(dev).train()
    out = {"device": torch.cuda.get_device_name(0), "mode": "train(): forward + backward, Gumbel sampler, dropout as configured",
           "method": f"HIP events around {REPS} calls; {ROUNDS} rounds behind {SKIP} discarded ones, the arms alternating inside a "
                     f"round; median (min-max) us per call", "settings": {}}
    for qpg in (1, 4, 12):
        G = QUESTIONS // qpg
        wl = synthetic.make_shared_workload(G, qpg, seed=7)
        wl.added_sym_edge = wl.added_sym_edge[:0]          # the two forms are equal only without the un-offset flips (quirk Q6)
        rep = wl.replicated()
        Q = wl.graph_index.numel()
        d, dr, index = wl.to(dev), rep.to(dev), wl.graph_index
        sg, sgr = d.scene_graphs(), dr.scene_graphs()
        w = torch.randn(Q, 1842, generator=torch.Generator().manual_seed(1)).to(dev)

        def replicated_step():
            model.zero_grad(set_to_none=True)
            res = model(dr.x, dr.edge_index, dr.edge_attr, dr.batch, dr.questions, dr.att_mask, return_masks=True, scene_graphs=sgr, seed=3)
            (res[0] * w).sum().backward()

        def shared_step():
            model.zero_grad(set_to_none=True)
            res, _ = model.forward_shared(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, index, scene_graphs=sg, seed=3)
            (res[0] * w).sum().backward()

        plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=G, max_nodes=wl.max_nodes, max_edges=wl.max_edges,
                                   graph_sizes=wl.graph_sizes)
        inst = ops.graph_instances(plan, d.edge_index, index, sizes=wl.graph_sizes)
        inst.by_graph()
        N, E, Np, Ep, C = wl.x.size(0), wl.edge_index.size(1), inst.node_src.numel(), inst.edge_src.numel(), 300
        gx, ge = torch.randn(Np, C, device=dev), torch.randn(Ep, C, device=dev)
        x_dst, e_dst = torch.empty_like(gx), torch.empty_like(ge)

        def generic():
            rp, eid = ops.token_csr(inst.node_src, N)
            dx = ops.segment_rows_sum(rp, eid, gx)
            rp, eid = ops.token_csr(inst.edge_src, E)
            return dx, ops.segment_rows_sum(rp, eid, ge)

        with torch.no_grad():
            dx, de = ops.instance_rows_backward(inst, gx, ge)
            gdx, gde = generic()
            torch.cuda.synchronize()
            err = max(float((dx - gdx).abs().max()), float((de - gde).abs().max()))
            assert err < 1e-4, err                              # the same sums, in another order
        arms = {"replicated_step": replicated_step, "shared_step": shared_step}
        row = rounds(arms)
        with torch.no_grad():
            row.update(rounds({"rows_backward": lambda: ops.instance_rows_backward(inst, gx, ge),
                               "inverse_lists": lambda: (setattr(inst, "_by_graph", None), inst.by_graph()),
                               "row_copy": lambda: (x_dst.copy_(gx), e_dst.copy_(ge)),
                               "token_csr_and_segment_rows_sum": generic}))
        ops.check_plans()
        bwd_bytes = (Np + Ep + N + E) * C * 4                  # every gradient row read once, every distinct row written once
        copy_bytes = (Np + Ep) * 2 * C * 4
        rf, sh = row["replicated_step"]["median_us"], row["shared_step"]["median_us"]
        spread = max(row[a]["max_us"] - row[a]["min_us"] for a in ("replicated_step", "shared_step"))
        row.update({"graphs": G, "questions": Q, "N": N, "E": E, "N_instances": Np, "E_instances": Ep,
                    "shared_over_replicated": round(sh / rf, 4), "diff_us": round(sh - rf, 1), "larger_round_spread_us": round(spread, 1),
                    "verdict": "faster" if sh - rf < -spread else "slower" if sh - rf > spread else "within the round spread",
                    "rows_backward_GB_per_s": round(bwd_bytes / row["rows_backward"]["median_us"] / 1e3, 1),
                    "copy_GB_per_s": round(copy_bytes / row["row_copy"]["median_us"] / 1e3, 1),
                    "max_abs_diff_to_the_generic_route": err})
        out["settings"][f"{qpg} questions per graph"] = row
        print(f"train, {qpg} per graph (G={G}, Q={Q}, N'={Np}, E'={Ep}): replicated step {rf:.0f} us, shared step {sh:.0f} us "
              f"({row['shared_over_replicated']:.3f}, {row['verdict']}); rows backward {row['rows_backward']['median_us']:.0f} us "
              f"({row['rows_backward_GB_per_s']} GB/s; copy of the rows {row['row_copy']['median_us']:.0f} us, {row['copy_GB_per_s']} GB/s; "
              f"token_csr + segment_rows_sum {row['token_csr_and_segment_rows_sum']['median_us']:.0f} us; inverse lists "
              f"{row['inverse_lists']['median_us']:.0f} us)", flush=True)
        del d, dr, inst, gx, ge, x_dst, e_dst, plan
    if "--out" in opt:
        with open(opt["--out"], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if "--train" in argv:
    train_main()
    sys.exit(0)

torch.manual_seed(0)
model = build_model(synthetic.full_model_args(), None).to(dev).eval()
out = {"device": torch.cuda.get_device_name(0),
       "method": f"HIP events around {REPS} calls; {ROUNDS} rounds behind {SKIP} discarded ones, the arms alternating inside a "
                 f"round; median (min-max) us per call", "settings": {}}
for qpg in (1, 4, 12):
    G = QUESTIONS // qpg
    wl = synthetic.make_shared_workload(G, qpg, seed=7)
    wl.added_sym_edge = wl.added_sym_edge[:0]              # the two forms are equal only without the un-offset flips (quirk Q6)
    rep = wl.replicated()
    Q = wl.graph_index.numel()
    d, dr, index = wl.to(dev), rep.to(dev), wl.graph_index
    sg, sgr = d.scene_graphs(), dr.scene_graphs()

    def replicated():
        return model(dr.x, dr.edge_index, dr.edge_attr, dr.batch, dr.questions, dr.att_mask, return_masks=True, scene_graphs=sgr)

    def shared():
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, sg)
        return model.ask(state, d.questions, d.att_mask, index)

    with torch.no_grad():
        ref, (got, inst) = replicated(), shared()
        torch.cuda.synchronize()
        ops.check_plans()
        flipped = torch.zeros(Q, device=dev).index_add_(0, inst.batch, (got[1] != ref[1]).float().squeeze(1)) > 0
        same_q = ~flipped
        same_n = same_q[inst.batch]
        lerr = float((got[0] - ref[0])[same_q].abs().max())
        gerr = float((got[2] - ref[2])[same_n].abs().max())
        assert lerr < 1e-4 and gerr < 1e-5, (lerr, gerr)
        state = model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, sg)
        plan_r = ops.GraphPlan.build(dr.batch, dr.edge_index, num_graphs=Q, max_nodes=rep.max_nodes, max_edges=rep.max_edges,
                                     graph_sizes=rep.graph_sizes)
        x_rows, e_rows = inst.gather_rows(state.x_enc, state.e_enc)
        x_dst, e_dst = torch.empty_like(x_rows), torch.empty_like(e_rows)
        arms = {"replicated_forward": replicated, "shared_encode_and_ask": shared,
                "encoder_on_replicated": lambda: model.scene_graph_encoder(dr.x, edge_index=dr.edge_index, edge_attr=dr.edge_attr,
                                                                           batch=dr.batch, gt_scene_graphs=sgr, plan=plan_r),
                "encoder_on_distinct": lambda: model.encode_scene(d.x, d.edge_index, d.edge_attr, d.batch, sg, plan=state.plan),
                "expansion": lambda: ops.graph_instances(state.plan, state.edge_index, index, sizes=state.sizes),
                "row_gather": lambda: inst.gather_rows(state.x_enc, state.e_enc),
                "row_copy": lambda: (x_dst.copy_(x_rows), e_dst.copy_(e_rows))}
        row = rounds(arms)
    Np, Ep, C = x_rows.size(0), e_rows.size(0), x_rows.size(1)
    gather_bytes = (Np + Ep) * (2 * C * 4 + 8)             # rows read and written, one int64 row number each
    copy_bytes = (Np + Ep) * 2 * C * 4
    rf, sh = row["replicated_forward"]["median_us"], row["shared_encode_and_ask"]["median_us"]
    spread = max(row[a]["max_us"] - row[a]["min_us"] for a in ("replicated_forward", "shared_encode_and_ask"))
    row.update({"graphs": G, "questions": Q, "N": wl.x.size(0), "E": wl.edge_index.size(1), "N_instances": Np, "E_instances": Ep,
                "questions_with_another_mask": int(flipped.sum()), "max_abs_logit_diff_elsewhere": lerr,
                "max_abs_gate_diff_elsewhere": gerr,
                "encoder_share_of_replicated_forward": round(row["encoder_on_replicated"]["median_us"] / rf, 4),
                "shared_over_replicated": round(sh / rf, 4), "diff_us": round(sh - rf, 1), "larger_round_spread_us": round(spread, 1),
                "verdict": "faster" if sh - rf < -spread else "slower" if sh - rf > spread else "within the round spread",
                "gather_GB_per_s": round(gather_bytes / row["row_gather"]["median_us"] / 1e3, 1),
                "copy_GB_per_s": round(copy_bytes / row["row_copy"]["median_us"] / 1e3, 1)})
    out["settings"][f"{qpg} questions per graph"] = row
    print(f"{qpg} per graph (G={G}, Q={Q}, N'={Np}, E'={Ep}): replicated {rf:.0f} us, shared {sh:.0f} us "
          f"({row['shared_over_replicated']:.3f}, {row['verdict']}); encoder on the replicated batch "
          f"{row['encoder_on_replicated']['median_us']:.0f} us ({100 * row['encoder_share_of_replicated_forward']:.1f} % of the forward), on "
          f"the distinct batch {row['encoder_on_distinct']['median_us']:.0f} us; expansion {row['expansion']['median_us']:.0f} us, gather "
          f"{row['row_gather']['median_us']:.0f} us ({row['gather_GB_per_s']} GB/s; copy {row['copy_GB_per_s']} GB/s); "
          f"{row['questions_with_another_mask']} questions with another mask, elsewhere |dlogit| <= {lerr:.1e}", flush=True)
    del d, dr, state, inst, x_rows, e_rows, x_dst, e_dst, ref, got, plan_r
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
