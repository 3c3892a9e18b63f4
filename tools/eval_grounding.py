#!/usr/bin/env python3
"""Grounding of the sampled subgraph in object annotations (include/isg_grounding.h): a validation pass of the full
model in eval() over a synthetic workload with seeded gold tables (synthetic.make_gold) and random question types, through
explain.evaluate(grounding=True); the report is printed, then the pass is timed with and without the grounding score, and beside
it the two launches of ops.grounding on one batch and the host's construction of the reports from the totals (once per pass).

  python tools/eval_grounding.py [--questions 1024] [--batches 2] [--rounds 6] [--out profiles/<name>.json]

There is no GQA question file here: the gold tables are random, so an untrained model's recall sits at `chance` (the share of a
graph's nodes the mask keeps).  One sample = one pass between two HIP events; per round the arms run one after the other; median,
minimum and maximum over the rounds (two more are run first and discarded).  A record, not a gate."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import explain, ops, synthetic
from isubgvqa_amd.datasets import QuestionTypes
from isubgvqa_amd.models import build_model

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
QUESTIONS, BATCHES, ROUNDS, SKIP = int(opt.get("--questions", 1024)), int(opt.get("--batches", 2)), int(opt.get("--rounds", 6)), 2
STRUCTURAL = ["query", "verify", "choose", "logical", "compare"]
SEMANTIC = ["attr", "rel", "obj", "cat", "global"]
VOCAB = 2578


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def figures(f):
    return {k: (None if v != v else round(v, 4)) if isinstance(v, float) else v for k, v in vars(f).items()}


torch.manual_seed(0)
model = build_model(synthetic.full_model_args(), None).to(dev).eval()
tables = explain.TokenTables({f"w{i}": i for i in range(VOCAB)}, [f"w{(11 * a) % VOCAB}" if a % 3 == 0 else f"answer {a}" for a in range(1842)])
qt = QuestionTypes(names={"structural": STRUCTURAL, "semantic": SEMANTIC})
gen = torch.Generator().manual_seed(5)
batches = []
with torch.no_grad():
    for i in range(BATCHES):
        wl = synthetic.make_full_workload(QUESTIONS, seed=7 + i)
        d = wl.to(dev)
        logits, mask = model(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, return_masks=True, scene_graphs=d.scene_graphs())[:2]
        label = logits.argmax(1)
        label[::2] = torch.randint(0, 1842, (label[::2].numel(),), generator=gen).to(dev)      # half of the answers are right
        types = [{"structural": STRUCTURAL[int(a)], "semantic": SEMANTIC[int(b)]}
                 for a, b in zip(torch.randint(0, 5, (QUESTIONS,), generator=gen), torch.randint(0, 5, (QUESTIONS,), generator=gen))]
        gold = synthetic.make_gold(wl.graph_sizes[0], facets=3, entries=6, seed=11 + i).pin_memory()      # as ObjectAnnotations.encode hands it over
        batches.append(explain.EvalBatch(d, label, groups=qt.encode(types), gold=gold))

ops.reset_counters()
report = explain.evaluate(model, batches, tables, types=qt, grounding=True)
torch.cuda.synchronize()
ops.check_plans()
g = report.grounding
assert ops.counters()["grounding"] == BATCHES and g.questions == QUESTIONS * BATCHES and g.bad == 0
assert sum(r.questions for r in g.by_type["structural"].values()) == g.questions
printed = {"questions": g.questions, "correct": g.correct, "unresolved": g.unresolved, "bad": g.bad,
           "sets": {name: {pop: figures(f) for pop, f in pops.items()} for name, pops in g.sets.items()},
           "any_recall_by_structural_type": {n: figures(r.sets["any"]["all"])["recall"] for n, r in g.by_type["structural"].items()}}
print(json.dumps(printed, indent=1), flush=True)

# the two launches alone, on the last batch's mask: table + totals over all groups
plan = ops.GraphPlan.build(d.batch, d.edge_index, num_graphs=QUESTIONS, max_nodes=d.max_nodes, max_edges=d.max_edges, graph_sizes=d.graph_sizes)
one = batches[-1]
gold_d, groups_d, pred_d = one.gold.to(dev), one.groups.to(dev), logits.argmax(1)
scratch = torch.zeros(1 + qt.num_groups, ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
arms = {"evaluate": lambda: explain.evaluate(model, batches, tables, types=qt),
        "evaluate_grounding": lambda: explain.evaluate(model, batches, tables, types=qt, grounding=True),
        "grounding_launches": lambda: ops.grounding(mask, plan, gold_d, pred_d, one.label, groups_d, qt.num_groups, totals=scratch),
        "report_from_totals": lambda: [explain.GroundingReport.from_totals(r) for r in scratch.cpu()]}
us = {a: [] for a in arms}
for r in range(ROUNDS + SKIP):
    for a, fn in arms.items():
        t = timed(fn)
        if r >= SKIP:
            us[a].append(t)
row = {a: {"median_us": round(sorted(v)[len(v) // 2], 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for a, v in us.items()}
plain, with_g = row["evaluate"]["median_us"], row["evaluate_grounding"]["median_us"]
spread = max(row[a]["max_us"] - row[a]["min_us"] for a in ("evaluate", "evaluate_grounding"))
out = {"device": torch.cuda.get_device_name(0),
       "method": f"HIP events around one evaluation; {ROUNDS} rounds behind {SKIP} discarded ones, the arms alternating inside a round; "
                 f"median (min-max) us per pass",
       "questions_per_batch": QUESTIONS, "batches": BATCHES, "groups": qt.num_groups, "timings": row,
       "grounding_over_plain": round(with_g / plain, 4), "diff_us_per_pass": round(with_g - plain, 1),
       "larger_round_spread_us": round(spread, 1),
       "verdict": "slower" if with_g - plain > spread else "faster" if with_g - plain < -spread else "within the round spread",
       "report": printed}
print(f"evaluate over {BATCHES} x {QUESTIONS} questions: {plain:.0f} us, with grounding {with_g:.0f} us ({out['grounding_over_plain']:.4f}, "
      f"{out['verdict']}; round spread {spread:.0f} us); the two launches on one batch {row['grounding_launches']['median_us']:.0f} us, "
      f"the reports of {1 + qt.num_groups} rows on the host {row['report_from_totals']['median_us']:.0f} us", flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
