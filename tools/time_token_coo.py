#!/usr/bin/env python3
"""ops.token_coo (table + running totals) against the same scoring written with torch ops on the device -- dense pad, broadcast
compare, reductions, index_add for the histograms, no device-to-host sync either -- on the configs[1] batch (4 096 graphs) with the
model's own Gumbel k = 5 mask, made-up name ids over a vocabulary of 2 578 and T = 16 question words per question (half of them
names of the question's own graph).  The two alternate in one process; each repetition is timed with HIP events after a warm-up;
ops.token_coo without totals is timed in the same loop (what the one-workgroup totals pass costs), and a profiler pass counts the
launches of one call of each.   python3 tools/time_token_coo.py [--graphs 4096] [--reps 200] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import ops, synthetic

T, VOCAB, CLASSES = 16, 2578, 1842


def torch_coo(names, mask, slots, B, nmax, pred, label, ans_sg, qtok, qflags, totals):
    """include/isg.h's semantics of isg_token_coo without a text explanation, batched."""
    kept = mask.view(-1) > 0
    dense = torch.full((B * nmax,), -1, dtype=torch.int64, device=names.device)
    dense_kept = dense.clone()
    dense[slots] = names
    dense_kept[slots] = torch.where(kept, names, -1)
    dense, dense_kept = dense.view(B, 1, nmax), dense_kept.view(B, 1, nmax)
    A = ans_sg.numel()
    answer = lambda cls: torch.where((cls >= 0) & (cls < A), ans_sg[cls.clamp(0, A - 1)], -1)
    vals = torch.cat([answer(pred)[:, None], answer(label)[:, None], qtok], 1).long()[:, :, None]      # [B, 2 + T, 1]
    in_graph = ((vals == dense) & (vals >= 0)).any(2)
    in_kept = ((vals == dense_kept) & (vals >= 0)).any(2)
    correct = pred == label
    words, words_kept = in_graph[:, 2:].sum(1), in_kept[:, 2:].sum(1)
    zero = torch.zeros_like(words)
    table = torch.stack([correct.long(), in_graph[:, 0].long(), in_graph[:, 1].long(), in_kept[:, 0].long(), words, words_kept, zero,
                         zero], 1).to(torch.int32)
    ans_valid = correct & in_graph[:, 1] & ((qflags & 1) == 0)
    qst_valid = correct & (words > 0)
    add = torch.zeros_like(totals)
    add[:9] = torch.stack([f.long() for f in (torch.ones_like(correct), correct, in_graph[:, 0], correct & in_graph[:, 0], ans_valid,
                                              ans_valid & in_kept[:, 0], qst_valid, words * qst_valid, words_kept * qst_valid)], 1).sum(0)
    H = ops.COO_TOKENS_MAX + 1
    add[16:16 + H].index_add_(0, words, qst_valid.long())
    add[16 + H:16 + 2 * H].index_add_(0, words, words_kept * qst_valid)
    totals += add
    return table


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
    """(kernel launches, copies) of one call, from the profiler's device events; an error text where it gives none."""
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
    B = a.graphs
    cfg = synthetic.WorkloadConfig(**{**synthetic.CFG2.__dict__, "num_graphs": B})
    wl = synthetic.make_workload(cfg).to(dev)
    model = synthetic.build_answer_model(cfg).to(dev).eval()
    with torch.no_grad():
        logits, mask = model(wl, seed=1)[:2]
        mask = mask.contiguous()
    plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=B, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
    gen = torch.Generator().manual_seed(5)
    N = plan.N
    x = torch.randint(0, VOCAB, (N, 4), generator=gen).to(dev)
    names = x[:, 0]                                            # the strided column, as a caller has it
    ptr = plan.ptr.long()
    sizes = (ptr[1:] - ptr[:-1]).clamp(min=1)
    own = names[(ptr[:-1, None] + (torch.randint(0, 1 << 30, (B, T), generator=gen).to(dev) % sizes[:, None])).clamp(max=N - 1)]
    qtok = torch.where(torch.rand(B, T, generator=gen).to(dev) < 0.5, own, torch.randint(-1, VOCAB, (B, T), generator=gen).to(dev))
    qtok = qtok.to(torch.int32).contiguous()
    qflags = (torch.rand(B, generator=gen) < 0.1).to(torch.int32).to(dev)
    ans_sg = torch.where(torch.rand(CLASSES, generator=gen) < 0.6, torch.randint(0, VOCAB, (CLASSES,), generator=gen), -1).to(torch.int32).to(dev)
    pred = logits.argmax(1) % CLASSES
    label = torch.where(torch.rand(B, generator=gen).to(dev) < 0.6, pred, (pred + 1) % CLASSES)
    slots = plan.dense_slots()
    nmax = plan.nmax
    t_ours = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    t_theirs = torch.zeros_like(t_ours)
    torch.cuda.synchronize()

    def ours():
        return ops.token_coo(names, mask, plan, pred, label, ans_sg, qtok, qflags, totals=t_ours).table

    def rows_only():
        return ops.token_coo(names, mask, plan, pred, label, ans_sg, qtok, qflags).table

    def theirs():
        return torch_coo(names, mask, slots, B, nmax, pred, label, ans_sg, qtok, qflags, t_theirs)

    assert torch.equal(ours(), theirs()) and torch.equal(t_ours, t_theirs), "the two scorings disagree"
    assert torch.equal(rows_only(), ours()) and torch.equal(2 * t_theirs, t_ours)
    once = t_theirs.tolist()
    fns = (("isg_token_coo", ours), ("isg_token_coo_without_totals", rows_only), ("torch_ops", theirs))
    t = {name: ([], []) for name, _ in fns}
    for r in range(a.warmup + a.reps):
        for name, fn in fns:
            dev_us, wall_us = timed(fn)
            if r >= a.warmup:
                t[name][0].append(dev_us)
                t[name][1].append(wall_us)
    res = {"tool": "tools/time_token_coo.py", "device": torch.cuda.get_device_name(0), "graphs": B, "N": N, "nmax": nmax, "T": T,
           "kept_nodes": int((mask > 0).sum()), "totals_first_12": once[:12],
           "what": "table + running totals of one batch; the three alternate in one process; HIP-event interval around each call and "
                   "host wall time; the torch-op form pads to [B, nmax], compares by broadcast and makes no device-to-host copy"}
    for name, fn in fns:
        res[name] = {"events": stats(t[name][0]), "wall": stats(t[name][1]), "device_work": count_device_work(fn)}
    res["speedup_median_events"] = round(res["torch_ops"]["events"]["median_us"] / res["isg_token_coo"]["events"]["median_us"], 2)
    res["speedup_median_wall"] = round(res["torch_ops"]["wall"]["median_us"] / res["isg_token_coo"]["wall"]["median_us"], 2)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
