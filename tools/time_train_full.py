"""Time forward + backward of the FULL model and of its question side alone, with the question side on this library's kernels
(models/text_encoder.FUSED_TEXT_TRAIN = True) and on torch's modules (False: nn.TransformerEncoder / Decoder, hipBLASLt), in one
process, the two alternating round by round.

  python tools/time_train_full.py [--graphs 4096] [--rounds 7] [--steps 5] [--out profiles/<name>.json] [--kernels]
  python tools/time_train_full.py --sgenc [--out profiles/<name>.json]
  python tools/time_train_full.py --linear-bwd [--out profiles/<name>.json]

--sgenc is the same A/B for the scene-graph encoder's switch (models/scene_graph_encoder.SPLIT_TRAIN: on = the walk without the
[E, 900] / [E, 600] concatenations on csrc/isg_sgenc_bwd.hip, off = the reference's form): the full step, the encoder alone
(forward + backward), torch.cuda.max_memory_allocated of one full step per variant, and HIP-event times of isg_segment_rows_sum
over the workload's CSRs (by source, by destination, by edge token; the node tokens with gdiv = 4) beside a torch copy_ of the
rows it reads, the token CSRs once as the workload has them (evenly loaded) and once skewed the way GQA is (one relation on 40 % of
the edges, the pad id in half of the attribute slots).

--linear-bwd is the A/B of autograd.LINEAR_BWD_KERNELS (on = every Linear's backward through csrc/isg_linear_bwd.hip: dz and db in
one pass, dW on the bf16 matrix cores; off = the torch passes and the fp32 split-M kernel) on the full step and on the question
side, with section 22's rule for the default: on iff the median gain exceeds the larger round spread and every round of one
variant lies below every round of the other.

Shape: bench.py --full's `full_model` leg (synthetic.make_full_workload: 4096 questions of 12 tokens, C = 300, I-MLE k = 5), the
model in train() mode with the constructors' dropouts (0.1 on the question side).  Each figure is the median over the rounds of
a round's mean step (host clock around steps that end in a device synchronise); `spread` is (max - min) / median over the rounds
of one variant -- a difference between the variants inside it is no difference.  --kernels adds HIP-event times of the question
side's operators (forward and backward separately) for the report of where a variant loses."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import isubgvqa_amd  # noqa: E402,F401
from isubgvqa_amd import ops, synthetic  # noqa: E402
from isubgvqa_amd.models import build_model, scene_graph_encoder, text_encoder  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ab(fn, rounds, steps, warmup=2, switch=(text_encoder, "FUSED_TEXT_TRAIN"), names=("kernels", "torch")):
    """{variant: [ms per step, one per round]}: the switch's two settings (names[0] = on) alternate inside every round."""
    out = {names[0]: [], names[1]: []}
    keep = getattr(*switch)
    for r in range(-1, rounds):
        for name, on in ((names[0], True), (names[1], False)) if r % 2 == 0 else ((names[1], False), (names[0], True)):
            setattr(*switch, on)
            if r < 0:
                timed(fn, warmup)                 # every shape of the timed window, both variants
            else:
                out[name].append(timed(fn, steps))
    setattr(*switch, keep)
    return out


def summary(runs):
    res = {}
    for name, v in runs.items():
        med = statistics.median(v)
        res[name] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "spread": round((max(v) - min(v)) / med, 4), "rounds": [round(x, 3) for x in v]}
    a, b = list(runs)
    res[f"{a}_over_{b}"] = round(res[a]["median_ms"] / res[b]["median_ms"], 4)
    return res


def segment_sum_times(wl, dev, C=300, vocab=2578, pad=1):
    """HIP-event time of isg_segment_rows_sum over the workload's CSRs, and of a copy_ of the rows it reads (same process)."""
    N, E = wl.x.size(0), wl.edge_attr.numel()
    g = torch.Generator(device=dev).manual_seed(2)
    dz, dn = torch.randn(E, C, device=dev, generator=g), torch.randn(N, C, device=dev, generator=g)

    def ev(fn, n=10):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / n * 1e3, 1)

    plan = ops.GraphPlan.build(wl.batch, wl.edge_index)
    skew_e = wl.edge_attr.clone()
    skew_e[torch.randperm(E, device=dev)[:int(0.4 * E)]] = 7
    skew_x = wl.x.clone()
    skew_x[:, 1:][torch.rand(N, 3, device=dev) < 0.5] = pad
    sign = torch.where(torch.rand(E, device=dev, generator=g) < 0.1, -1.0, 1.0)
    cases = {
        "by source (d A)": (plan.source_csr()[:2], dz, dict(M=E)),
        "by destination (d B)": ((plan.rowptr, plan.eid), dz, dict(M=E)),
        "edge tokens, as the workload has them: evenly loaded (d T, w = sign)": (ops.token_csr(wl.edge_attr, vocab), dz, dict(w=sign)),
        "edge tokens, one relation on 40 % of the edges (d T, w = sign)": (ops.token_csr(skew_e, vocab), dz, dict(w=sign)),
        "node tokens, evenly loaded (gdiv = 4, skip = pad)": (ops.token_csr(wl.x, vocab), dn, dict(gdiv=4, skip=pad)),
        "node tokens, pad in half of the attribute slots (gdiv = 4, skip = pad)": (ops.token_csr(skew_x, vocab), dn, dict(gdiv=4, skip=pad)),
        "node tokens, pad in half of the attribute slots, pad row summed (gdiv = 4)": (ops.token_csr(skew_x, vocab), dn, dict(gdiv=4)),
    }
    out = {"chunk": ops.segment_rows_chunk()}
    for name, ((rowptr, eid), G, kw) in cases.items():
        counts = (rowptr[1:] - rowptr[:-1]).float()
        out[name] = {"us": ev(lambda: ops.segment_rows_sum(rowptr, eid, G, **kw)), "segments": rowptr.numel() - 1,
                     "entries": int(rowptr[-1]), "longest_segment": int(counts.max()), "median_segment": int(counts.median())}
    for name, G in (("copy_ of the [E, 300] rows", dz), ("copy_ of the [N, 300] rows", dn)):
        dst = torch.empty_like(G)
        out[name] = {"us": ev(lambda: dst.copy_(G)), "bytes_read": G.numel() * 4}
    return out


def sgenc_main(a, model, wl, sg, target, dev):
    switch, names = (scene_graph_encoder, "SPLIT_TRAIN"), ("split_train", "concatenated")
    enc = model.scene_graph_encoder
    plan = ops.GraphPlan.build(wl.batch, wl.edge_index)
    w_enc = None

    def full_step(i):
        model.zero_grad(set_to_none=True)
        logits = model(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.questions, wl.att_mask, return_masks=True, scene_graphs=sg,
                       seed=1000 + i)[0]
        torch.nn.functional.cross_entropy(logits, target).backward()

    def encoder_step(i):
        nonlocal w_enc
        enc.zero_grad(set_to_none=True)
        x_enc, e_enc = enc(wl.x, edge_index=wl.edge_index, edge_attr=wl.edge_attr, batch=wl.batch, gt_scene_graphs=sg, plan=plan)
        if w_enc is None:
            w_enc = (torch.randn_like(x_enc), torch.randn_like(e_enc))
        ((x_enc * w_enc[0]).sum() + (e_enc * w_enc[1]).sum()).backward()

    res = {"workload": f"full ISubGVQA model, {a.graphs} questions, N = {wl.x.size(0)} nodes, E = {wl.edge_attr.numel()} edges, train() mode",
           "method": f"{a.rounds} rounds x {a.steps} steps per variant, variants alternating inside a round; host clock around synchronised steps",
           "device": torch.cuda.get_device_name(0), "shipped_default_SPLIT_TRAIN": scene_graph_encoder.SPLIT_TRAIN}
    ops.reset_counters()
    res["scene_graph_encoder_fwd_bwd"] = summary(ab(encoder_step, a.rounds, a.steps, switch=switch, names=names))
    res["full_model_fwd_bwd"] = summary(ab(full_step, a.rounds, a.steps, switch=switch, names=names))
    res["counters"] = {k: v for k, v in ops.counters().items() if k in ("sgenc_train_kernels", "text_train_kernels", "torch_linear")}
    e, f = res["scene_graph_encoder_fwd_bwd"], res["full_model_fwd_bwd"]
    res["encoder_share_of_full_step"] = {n: round(e[n]["median_ms"] / f[n]["median_ms"], 3) for n in names}
    on, off = f[names[0]], f[names[1]]
    gain = off["median_ms"] - on["median_ms"]
    noise = max(on["max_ms"] - on["min_ms"], off["max_ms"] - off["min_ms"])
    res["decision"] = {"full_step_gain_ms": round(gain, 3), "larger_round_spread_ms": round(noise, 3),
                       "ships_on": bool(gain > noise), "rule": "on iff median(off) - median(on) > the larger of the two variants' (max - min) over the rounds"}
    keep, mem = scene_graph_encoder.SPLIT_TRAIN, {}
    for name, setting in zip(names, (True, False)):
        scene_graph_encoder.SPLIT_TRAIN = setting
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        full_step(0)
        torch.cuda.synchronize()
        mem[name] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    scene_graph_encoder.SPLIT_TRAIN = keep
    res["full_step_max_memory_allocated_MiB"] = mem
    res["isg_segment_rows_sum"] = segment_sum_times(wl, dev)
    return res


def linear_bwd_main(a, model, wl, sg, target):
    from isubgvqa_amd import autograd
    switch, names = (autograd, "LINEAR_BWD_KERNELS"), ("linear_bwd_kernels", "torch_passes")
    w_lang = None

    def full_step(i):
        model.zero_grad(set_to_none=True)
        logits = model(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.questions, wl.att_mask, return_masks=True, scene_graphs=sg,
                       seed=1000 + i)[0]
        torch.nn.functional.cross_entropy(logits, target).backward()

    def language_step(i):
        nonlocal w_lang
        model.zero_grad(set_to_none=True)
        glf, instr = model.language_features(wl.questions, wl.att_mask, None, 1000 + i)
        if w_lang is None:
            w_lang = (torch.randn_like(glf), torch.randn_like(instr))
        ((glf * w_lang[0]).sum() + (instr * w_lang[1]).sum()).backward()

    res = {"workload": f"full ISubGVQA model, {a.graphs} questions, N = {wl.x.size(0)} nodes, E = {wl.edge_attr.numel()} edges, train() mode",
           "method": f"{a.rounds} rounds x {a.steps} steps per variant, variants alternating inside a round; host clock around synchronised steps",
           "device": torch.cuda.get_device_name(0), "shipped_default_LINEAR_BWD_KERNELS": autograd.LINEAR_BWD_KERNELS}
    ops.reset_counters()
    res["question_side_fwd_bwd"] = summary(ab(language_step, a.rounds, a.steps, switch=switch, names=names))
    res["full_model_fwd_bwd"] = summary(ab(full_step, a.rounds, a.steps, switch=switch, names=names))
    res["counters"] = {k: v for k, v in ops.counters().items() if k in ("linear_bwd_kernels", "text_train_kernels", "torch_linear")}
    on, off = (res["full_model_fwd_bwd"][n] for n in names)
    gain = off["median_ms"] - on["median_ms"]
    noise = max(on["max_ms"] - on["min_ms"], off["max_ms"] - off["min_ms"])
    separated = on["max_ms"] < off["min_ms"]
    res["decision"] = {"full_step_gain_ms": round(gain, 3), "larger_round_spread_ms": round(noise, 3),
                       "every_round_on_below_every_round_off": bool(separated), "ships_on": bool(gain > noise and separated),
                       "rule": "on iff median(off) - median(on) > the larger of the two variants' (max - min) over the rounds and every "
                               "round of `on` is below every round of `off`"}
    return res


def operator_times(model, wl, dev):
    """HIP-event time of the question side's forward and of its backward, per variant, and of the autograd operators one by one
    (each timed alone on the shapes of encoder layer 0: forward, then backward)."""
    from isubgvqa_amd import autograd
    B, T = wl.questions.shape
    D, H = 512, 8
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    layer = model.question_encoder.transformer_encoder.layers[0]

    def ev(fn, n=5):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / n * 1e3, 1)

    def fwd_bwd(make):
        """(forward us, backward us) of y = make(leaves)"""
        y = make()
        go = torch.randn_like(y)
        return ev(lambda: make()), ev(lambda: torch.autograd.grad(make(), leaves, go, allow_unused=True)) - ev(lambda: make())

    out = {}
    x = r(T * B, D).requires_grad_(True)
    qkv = r(T * B, 3 * D).requires_grad_(True)
    kb = wl.att_mask.float().contiguous()
    h = r(T * B, 4 * D).requires_grad_(True)
    res = r(T * B, D).requires_grad_(True)

    def packed_attention():
        base = qkv * 1.0                            # a non-leaf [T*B, 3D] tensor, as the fused in_proj's result is
        return autograd.mha_small(base[:, :D], base[:, D:2 * D], base[:, 2 * D:], B, H, kb, 0.1, 5)

    cases = {
        "attention (probabilities dropout 0.1)": ([qkv], packed_attention),
        "attention, torch's ops": ([qkv], lambda: autograd._mha_torch(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, H, kb, 0.1)),
        "dropout + add + LayerNorm": ([x, res], lambda: autograd.add_layernorm(x, res, layer.norm1, 0.1, 6)),
        "dropout + add + LayerNorm, torch": ([x, res], lambda: torch.nn.functional.layer_norm(res + torch.nn.functional.dropout(x, 0.1), (D,), layer.norm1.weight, layer.norm1.bias)),
        "in_proj 512 -> 1536": ([x], lambda: autograd.linear(x, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias, False)),
        "in_proj, torch": ([x], lambda: torch.nn.functional.linear(x, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias)),
        "linear1 + ReLU 512 -> 2048": ([x], lambda: autograd.linear(x, layer.linear1.weight, layer.linear1.bias, False, relu=True)),
        "linear1 + ReLU, torch": ([x], lambda: torch.relu(torch.nn.functional.linear(x, layer.linear1.weight, layer.linear1.bias))),
        "FFN dropout on [M, 2048]": ([h], lambda: autograd.dropout(h, 0.1, 7)),
        "FFN dropout, torch": ([h], lambda: torch.nn.functional.dropout(h, 0.1)),
        "linear2 2048 -> 512": ([h], lambda: autograd.linear(h, layer.linear2.weight, layer.linear2.bias, False)),
        "linear2, torch": ([h], lambda: torch.nn.functional.linear(h, layer.linear2.weight, layer.linear2.bias)),
    }
    for name, (leaves_, make) in cases.items():
        leaves = leaves_ + [p for p in layer.parameters()]
        f, b = fwd_bwd(make)
        out[name] = {"forward_us": f, "backward_us": round(b, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--sgenc", action="store_true", help="A/B of the scene-graph encoder's SPLIT_TRAIN instead of the question side's switch")
    ap.add_argument("--linear-bwd", action="store_true", help="A/B of autograd.LINEAR_BWD_KERNELS instead of the question side's switch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(), None).to(dev).train()
    wl = synthetic.make_full_workload(a.graphs).to(dev)
    sg = wl.scene_graphs()
    target = torch.randint(0, 1842, (a.graphs,), device=dev)
    w_lang = None
    if a.sgenc or a.linear_bwd:
        res = sgenc_main(a, model, wl, sg, target, dev) if a.sgenc else linear_bwd_main(a, model, wl, sg, target)
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")
        return

    def full_step(i):
        model.zero_grad(set_to_none=True)
        logits = model(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.questions, wl.att_mask, return_masks=True, scene_graphs=sg,
                       seed=1000 + i)[0]
        torch.nn.functional.cross_entropy(logits, target).backward()

    def language_step(i):
        nonlocal w_lang
        model.zero_grad(set_to_none=True)
        glf, instr = model.language_features(wl.questions, wl.att_mask, None, 1000 + i)
        if w_lang is None:
            w_lang = (torch.randn_like(glf), torch.randn_like(instr))
        ((glf * w_lang[0]).sum() + (instr * w_lang[1]).sum()).backward()

    res = {"workload": f"full ISubGVQA model, {a.graphs} questions of {wl.questions.size(1)} tokens, train() mode, dropout 0.1 on the question side",
           "method": f"{a.rounds} rounds x {a.steps} steps per variant, variants alternating inside a round; host clock around synchronised steps",
           "device": torch.cuda.get_device_name(0)}
    ops.reset_counters()
    res["question_side_fwd_bwd"] = summary(ab(language_step, a.rounds, a.steps))
    res["full_model_fwd_bwd"] = summary(ab(full_step, a.rounds, a.steps))
    res["counters"] = {k: v for k, v in ops.counters().items() if k in ("text_train_kernels", "torch_attention_train", "torch_linear")}
    q, f = res["question_side_fwd_bwd"], res["full_model_fwd_bwd"]
    res["question_side_share_of_full_step"] = {n: round(q[n]["median_ms"] / f[n]["median_ms"], 3) for n in ("kernels", "torch")}
    if a.kernels:
        res["operators_encoder_layer0"] = operator_times(model, wl, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
