#!/usr/bin/env python3
"""Evaluation by question type (include/isg_eval.h): a validation pass of the full model in eval() over a synthetic
workload with random question types, with train.Meters against train.TypedMeters; the arms alternate in one process, HIP events.

  python tools/eval_by_type.py [--questions 4096] [--batches 2] [--rounds 6] [--out profiles/<name>.json]

The report of the typed pass is printed first (overall loss, acc1, acc@5 and the same per structural and semantic type; an
untrained model answers at chance).  Then train.validate over the same batches is timed with plain Meters and with TypedMeters, and
the added launches alone on one batch's logits: ops.answer_rank (without and with the 5 best classes) and ops.group_meters.
One sample = one pass between two events; per round the arms run one after the other; median, minimum and maximum over the rounds
(two more are run first and discarded).  A record, not a gate."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import ops, synthetic, train
from isubgvqa_amd.datasets import QuestionTypes
from isubgvqa_amd.models import build_model

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
QUESTIONS, BATCHES, ROUNDS, SKIP = int(opt.get("--questions", 4096)), int(opt.get("--batches", 2)), int(opt.get("--rounds", 6)), 2
STRUCTURAL = ["query", "verify", "choose", "logical", "compare"]
SEMANTIC = ["attr", "rel", "obj", "cat", "global"]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


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


torch.manual_seed(0)
model = build_model(synthetic.full_model_args(), None).to(dev).eval()
gen = torch.Generator().manual_seed(5)
qt = QuestionTypes(names={"structural": STRUCTURAL, "semantic": SEMANTIC})
batches = []
for i in range(BATCHES):
    d = synthetic.make_full_workload(QUESTIONS, seed=7 + i).to(dev)
    types = [{"structural": STRUCTURAL[int(a)], "semantic": SEMANTIC[int(b)]}
             for a, b in zip(torch.randint(0, 5, (QUESTIONS,), generator=gen), torch.randint(0, 5, (QUESTIONS,), generator=gen))]
    inputs = dict(node_embeddings=d.x, edge_index=d.edge_index, edge_embeddings=d.edge_attr, batch=d.batch, questions=d.questions,
                  qsts_att_mask=d.att_mask, return_masks=True, scene_graphs=d.scene_graphs())
    labels = torch.randint(0, 1842, (QUESTIONS,), generator=gen).to(dev)
    batches.append((inputs, labels, qt.encode(types).to(dev)))

plain, typed = train.Meters(dev), train.TypedMeters(dev, qt, k=5)
train.validate(model, batches, typed, seed=3)
torch.cuda.synchronize()
ops.check_plans()
report = typed.report()
print(json.dumps(report, indent=1), flush=True)
assert report["rows"] == QUESTIONS * BATCHES and typed.status.tolist() == [0, 0]
assert sum(v["rows"] for v in report["by_type"]["structural"].values()) == report["rows"]

with torch.no_grad():
    logits = train._logits(model, batches[0][0], 3)
    labels, groups = batches[0][1], batches[0][2]
    ce = ops.cross_entropy(logits, labels)
    rank = ops.answer_rank(logits, labels).rank
    scratch = torch.zeros(qt.num_groups, 8, dtype=torch.float64, device=dev)
    arms = {"validate_meters": lambda: train.validate(model, batches, plain, seed=3),
            "validate_typed_meters": lambda: train.validate(model, batches, typed, seed=3),
            "cross_entropy": lambda: ops.cross_entropy(logits, labels),
            "answer_rank": lambda: ops.answer_rank(logits, labels),
            "answer_rank_top5": lambda: ops.answer_rank(logits, labels, k=5, lse=ce.lse, want_top=True),
            "group_meters": lambda: ops.group_meters(ce.row_loss, rank, groups, scratch, k=5)}
    row = rounds(arms)
vm, vt = row["validate_meters"]["median_us"], row["validate_typed_meters"]["median_us"]
spread = max(row[a]["max_us"] - row[a]["min_us"] for a in ("validate_meters", "validate_typed_meters"))
logit_bytes = logits.numel() * 4
out = {"device": torch.cuda.get_device_name(0),
       "method": f"HIP events around one call; {ROUNDS} rounds behind {SKIP} discarded ones, the arms alternating inside a round; "
                 f"median (min-max) us per call",
       "questions_per_batch": QUESTIONS, "batches": BATCHES, "classes": logits.size(1), "groups": qt.num_groups, "timings": row,
       "typed_over_plain": round(vt / vm, 4), "diff_us_per_pass": round(vt - vm, 1), "larger_round_spread_us": round(spread, 1),
       "verdict": "slower" if vt - vm > spread else "faster" if vt - vm < -spread else "within the round spread",
       "answer_rank_GB_per_s": round(logit_bytes / row["answer_rank"]["median_us"] / 1e3, 1),
       "cross_entropy_GB_per_s": round(logit_bytes / row["cross_entropy"]["median_us"] / 1e3, 1),
       "report": report}
print(f"validate over {BATCHES} x {QUESTIONS} questions: Meters {vm:.0f} us, TypedMeters {vt:.0f} us ({out['typed_over_plain']:.4f}, "
      f"{out['verdict']}; round spread {spread:.0f} us); on one batch's logits: cross_entropy {row['cross_entropy']['median_us']:.0f} us "
      f"({out['cross_entropy_GB_per_s']} GB/s of logits), answer_rank {row['answer_rank']['median_us']:.0f} us "
      f"({out['answer_rank_GB_per_s']} GB/s), with the 5 best classes {row['answer_rank_top5']['median_us']:.0f} us, group_meters "
      f"{row['group_meters']['median_us']:.0f} us", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
