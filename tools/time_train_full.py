"""Time forward + backward of the FULL model and of its question side alone, with the question side on this library's kernels
(models/text_encoder.FUSED_TEXT_TRAIN = True) and on torch's modules (False: nn.TransformerEncoder / Decoder, hipBLASLt), in one
process, the two alternating round by round.

  python tools/time_train_full.py [--graphs 4096] [--rounds 7] [--steps 5] [--out profiles/<name>.json] [--kernels]

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
from isubgvqa_amd.models import build_model, text_encoder  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ab(fn, rounds, steps, warmup=2):
    """{variant: [ms per step, one per round]}: kernels / torch alternate inside every round."""
    out = {"kernels": [], "torch": []}
    for r in range(-1, rounds):
        for name, on in (("kernels", True), ("torch", False)) if r % 2 == 0 else (("torch", False), ("kernels", True)):
            text_encoder.FUSED_TEXT_TRAIN = on
            if r < 0:
                timed(fn, warmup)                 # every shape of the timed window, both variants
            else:
                out[name].append(timed(fn, steps))
    text_encoder.FUSED_TEXT_TRAIN = True
    return out


def summary(runs):
    res = {}
    for name, v in runs.items():
        med = statistics.median(v)
        res[name] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "spread": round((max(v) - min(v)) / med, 4), "rounds": [round(x, 3) for x in v]}
    res["kernels_over_torch"] = round(res["kernels"]["median_ms"] / res["torch"]["median_ms"], 4)
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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(), None).to(dev).train()
    wl = synthetic.make_full_workload(a.graphs).to(dev)
    sg = wl.scene_graphs()
    target = torch.randint(0, 1842, (a.graphs,), device=dev)
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
