"""Time a FULL training step with its tail on the device (train.train_step with optim.Adam(max_grad_norm=2.0)) against the same
step with the tail as the reference writes it (accuracy().item(), F.cross_entropy, clip_grad_norm_(2.0), torch.optim.Adam, two
loss.item()), in one process, the two alternating round by round; then the Adam update alone.

  python tools/time_train_tail.py [--graphs 4096] [--rounds 7] [--steps 5] [--out profiles/<name>.json]

Shape and method are tools/time_train_full.py's: bench.py --full's `full_model` leg (4096 questions of 12 tokens), the model in
train() mode; each figure is the median over the rounds of a round's mean step (host clock around steps that end in a device
synchronise); `spread` is (max - min) / median over the rounds of one variant -- a difference between the variants inside it is
no difference.  Both variants step the same parameters, each with an optimizer (and moments) of its own.

`adam_alone`: HIP-event time of one isg_mt_adam pair (no norm launch) over gradients of the full model's parameter shapes, of
optim.Adam.step() with the norm, and of torch.optim.Adam.step() on the same tensors; `fraction_of_copy` is the update's 28 B per
element (16 read, 12 written) per second over the bandwidth that a torch copy_ (float4 loads and stores) of the same number of
bytes reaches on this device in this process."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import isubgvqa_amd  # noqa: E402,F401
from isubgvqa_amd import optim, synthetic, train  # noqa: E402
from isubgvqa_amd.models import build_model  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ab(variants, rounds, steps, warmup=2):
    """{variant: [ms per step, one per round]}: the variants alternate inside every round."""
    names = list(variants)
    out = {n: [] for n in names}
    for r in range(-1, rounds):
        for name in names if r % 2 == 0 else names[::-1]:
            if r < 0:
                timed(variants[name], warmup)
            else:
                out[name].append(timed(variants[name], steps))
    return out


def summary(runs):
    res = {}
    for name, v in runs.items():
        med = statistics.median(v)
        res[name] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "spread": round((max(v) - min(v)) / med, 4), "rounds": [round(x, 3) for x in v]}
    return res


def accuracy(output, target, topk=(1,)):
    """ISubGVQA/utils/accuracies.py::accuracy, restated."""
    with torch.no_grad():
        maxk = max(topk)
        batch_size = target.size(0)
        _, pred = output.topk(maxk, 1, True, True)
        pred = pred.t()
        correct = pred.eq(target.view(1, -1).expand_as(pred))
        return [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / batch_size) for k in topk]


def events(fn, n=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3        # microseconds


def adam_alone(model, dev):
    shapes = [tuple(p.shape) for p in model.parameters()]
    g = torch.Generator(device=dev).manual_seed(2)
    params = [torch.randn(s, device=dev, generator=g).requires_grad_(True) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g)
    n = sum(p.numel() for p in params)
    update = optim.Adam(params, lr=1e-3, skip_nonfinite=False)
    clipped = optim.Adam(params, lr=1e-3, max_grad_norm=2.0)
    stock = torch.optim.Adam(params, lr=1e-3)
    src = torch.empty(int(3.5 * n), device=dev)
    dst = torch.empty_like(src)
    t_copy = events(lambda: dst.copy_(src))
    t_update, t_clipped, t_stock = events(update.step), events(clipped.step), events(stock.step)
    copy_bw, adam_bw = 8 * src.numel() / t_copy * 1e-6, 28 * n / t_update * 1e-6          # TB/s
    return {"parameters": n, "tensors": len(params), "isg_mt_adam_pair_us": round(t_update, 1),
            "optim_adam_step_with_norm_us": round(t_clipped, 1), "torch_adam_step_us": round(t_stock, 1),
            "copy_same_bytes_us": round(t_copy, 1), "copy_TBps": round(copy_bw, 3), "adam_TBps_at_28B_per_element": round(adam_bw, 3),
            "fraction_of_copy": round(adam_bw / copy_bw, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(), None).to(dev).train()
    wl = synthetic.make_full_workload(a.graphs).to(dev)
    sg = wl.scene_graphs()
    target = torch.randint(0, 1842, (a.graphs,), device=dev)
    inputs = dict(node_embeddings=wl.x, edge_index=wl.edge_index, edge_embeddings=wl.edge_attr, batch=wl.batch, questions=wl.questions,
                  qsts_att_mask=wl.att_mask, return_masks=True, scene_graphs=sg)
    ours, stock = optim.Adam(model.parameters(), lr=1e-4, max_grad_norm=2.0), torch.optim.Adam(model.parameters(), lr=1e-4)
    meters = train.Meters(dev)
    host = {"loss_sum": 0.0, "rows": 0, "acc_sum": 0.0}

    def device_tail(i):
        train.train_step(model, ours, inputs, target, meters, seed=1000 + i)

    def reference_tail(i):
        model.n_train_steps += a.graphs
        logits = model(**inputs, seed=1000 + i)[0]
        with torch.no_grad():
            host["acc_sum"] += accuracy(logits, target)[0].item() * a.graphs
        loss = torch.nn.functional.cross_entropy(logits, target)
        stock.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=2.0)
        stock.step()
        if not math.isnan(loss.item()):
            host["loss_sum"] += loss.item() * a.graphs
            host["rows"] += a.graphs

    res = {"workload": f"full ISubGVQA model, {a.graphs} questions of {wl.questions.size(1)} tokens, train() mode, a whole step: "
                       "forward, loss, accuracy, backward, clip at 2.0, Adam",
           "method": f"{a.rounds} rounds x {a.steps} steps per variant, variants alternating inside a round; host clock around "
                     "synchronised steps",
           "device": torch.cuda.get_device_name(0)}
    s = summary(ab({"device_tail": device_tail, "reference_tail": reference_tail}, a.rounds, a.steps))
    s["device_over_reference"] = round(s["device_tail"]["median_ms"] / s["reference_tail"]["median_ms"], 4)
    res["full_step"] = s
    res["meters"] = meters.report()
    res["table_copies"] = optim.LAUNCHES["table_copies"]
    res["adam_alone"] = adam_alone(model, dev)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
