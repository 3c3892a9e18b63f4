#!/usr/bin/env python3
"""ops.subgraph_cut (keep-cut, table_k = 5, through .sizes()) against the same cut written with torch ops on the device, on the
configs[1] batch (4 096 graphs) with the model's own Gumbel k = 5 mask.  The two alternate in one process; each repetition is
timed with HIP events after a warm-up (the interval covers the call's own device-to-host waits), and a profiler pass counts the
launches and device-to-host copies of one call of each.   python3 tools/time_subgraph_cut.py [--reps 200] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import ops, synthetic

K = 5


def torch_cut(mask, edge_index, batch, ptr, B):
    """The restatement of tests/subgraph_restated.py on the device, trusting the endpoints to be in range: flags, cumsum, two
    nonzero (each a device-to-host sync), gathers, one scatter for the table."""
    keep = mask.view(-1) > 0
    rank = keep.cumsum(0) - 1
    node_new = torch.where(keep, rank, -1).to(torch.int32)
    node_id = torch.nonzero(keep).view(-1)
    ekeep = keep[edge_index[0]] & keep[edge_index[1]]
    edge_new = torch.where(ekeep, ekeep.cumsum(0) - 1, -1).to(torch.int32)
    edge_id = torch.nonzero(ekeep).view(-1)
    sub_ei = rank[edge_index[:, edge_id]]
    sub_batch = batch[node_id]
    excl = torch.cat([rank.new_zeros(1), rank + 1])
    sub_ptr = excl[ptr]
    j = torch.arange(node_id.numel(), device=mask.device) - sub_ptr[sub_batch]
    sel = torch.full((B * K + 1,), -1, dtype=torch.int32, device=mask.device)
    sel.scatter_(0, torch.where(j < K, sub_batch * K + j, B * K), (node_id - ptr[sub_batch]).to(torch.int32))
    return node_new, edge_new, node_id, edge_id, sub_ei, sub_batch, sub_ptr.to(torch.int32), sel[:B * K].view(B, K)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3, (time.perf_counter() - t0) * 1e6


def stats(ts):
    ts = sorted(ts)
    n = len(ts)
    return {"median_us": round(ts[n // 2], 2), "p10_us": round(ts[n // 10], 2), "p90_us": round(ts[(9 * n) // 10], 2),
            "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2), "mean_us": round(sum(ts) / n, 2), "repetitions": n}


def count_device_work(fn):
    """(kernel launches, device-to-host copies) of one call, from the profiler's device events; None where it gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")]
    except Exception as exc:      # noqa: BLE001 -- a profiler that is not available is reported, not fatal
        return {"error": f"{type(exc).__name__}: {exc}"}
    if not names:
        return {"error": "the profiler recorded no device events"}
    copies = [n for n in names if "memcpy" in n.lower() or "copy" in n.lower() and "kernel" not in n.lower()]
    d2h = [n for n in copies if "dtoh" in n.lower() or "devicetohost" in n.lower().replace(" ", "")]
    return {"launches": len(names) - len(copies), "copies": len(copies), "device_to_host_copies": len(d2h)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synthetic.WorkloadConfig(**{**synthetic.CFG2.__dict__, "num_graphs": a.graphs})
    wl = synthetic.make_workload(cfg).to(dev)
    model = synthetic.build_answer_model(cfg).to(dev).eval()
    with torch.no_grad():
        mask = model(wl, seed=1)[1].contiguous()
    plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=a.graphs, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
    ptr = plan.ptr.long()
    torch.cuda.synchronize()

    def ours():
        cut = ops.subgraph_cut(mask, wl.edge_index, plan, table_k=K)
        cut.sizes()
        return cut

    def theirs():
        return torch_cut(mask, wl.edge_index, wl.batch, ptr, a.graphs)

    cut, ref = ours(), theirs()
    got = (cut.node_new, cut.edge_new, cut.node_id, cut.edge_id, cut.edge_index, cut.batch, cut.ptr, cut.sel)
    for name, g, r in zip(("node_new", "edge_new", "node_id", "edge_id", "edge_index", "batch", "ptr", "sel"), got, ref):
        assert torch.equal(g, r), f"the two cuts disagree on {name}"
    t = {"isg_subgraph_cut": ([], []), "torch_ops": ([], [])}
    for r in range(a.warmup + a.reps):
        for name, fn in (("isg_subgraph_cut", ours), ("torch_ops", theirs)):
            dev_us, wall_us = timed(fn)
            if r >= a.warmup:
                t[name][0].append(dev_us)
                t[name][1].append(wall_us)
    res = {"tool": "tools/time_subgraph_cut.py", "device": torch.cuda.get_device_name(0), "graphs": a.graphs, "N": plan.N,
           "E": plan.E, "kept_nodes": cut.sizes()[0], "kept_edges": cut.sizes()[1], "table_k": K,
           "what": "keep-cut of the model's Gumbel k = 5 mask through .sizes(); the two alternate in one process; HIP-event interval "
                   "around each call (its device-to-host waits included) and host wall time",
           "isg_subgraph_cut": {"events": stats(t["isg_subgraph_cut"][0]), "wall": stats(t["isg_subgraph_cut"][1]),
                                "device_work": count_device_work(ours)},
           "torch_ops": {"events": stats(t["torch_ops"][0]), "wall": stats(t["torch_ops"][1]),
                         "device_work": count_device_work(theirs)}}
    res["speedup_median_events"] = round(res["torch_ops"]["events"]["median_us"] / res["isg_subgraph_cut"]["events"]["median_us"], 2)
    res["speedup_median_wall"] = round(res["torch_ops"]["wall"]["median_us"] / res["isg_subgraph_cut"]["wall"]["median_us"], 2)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
