#!/usr/bin/env python3
"""The intrinsic mask beside post-hoc baselines (explain.compare) on synthetic workloads: the AnswerModel of
BASELINE configs[1] with the I-MLE sampler (its eval solve is noise-free), seeded batches, seeded names, question words, labels
and annotated objects.  An untrained model on random graphs: the figures show that the yardsticks run and how the explainers
differ on them, not how good an explanation is.

  python tools/compare_explainers.py [--graphs 64] [--batches 2] [--k 5] [--max-instances 2048]
                                     [--explainers intrinsic,occlusion,random,attention,integrated_gradients,grad_x_input,mask_optimization,shapley]
                                     [--ig-steps 16] [--mo-steps 100] [--sv-permutations 16] [--curves 0,0.1,0.2,0.3,0.5,0.7,1]
                                     [--out profiles/<name>.json]
--explainers: a comma-separated list from explain.EXPLAINERS_ALL + explain.EXPLAINERS_GRADIENT + explain.EXPLAINERS_LEARNED +
explain.EXPLAINERS_SAMPLED (default: explain.EXPLAINERS); --ig-steps: the points of integrated_gradients' path;
--mo-steps: the Adam steps of mask_optimization; --sv-permutations: the antithetic permutations of shapley_values
(DESIGN.md 39); --curves: the fractions of every explainer's fidelity curves (without it no
curve is computed)."""
import dataclasses
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import explain, synthetic

dev = torch.device("cuda:0")
argv = sys.argv[1:]
opt = {a: b for a, b in zip(argv, argv[1:]) if a.startswith("--")}
GRAPHS, BATCHES, K = int(opt.get("--graphs", 64)), int(opt.get("--batches", 2)), int(opt.get("--k", 5))
MAX_INSTANCES = int(opt["--max-instances"]) if "--max-instances" in opt else None
EXPLAINERS = tuple(n for n in opt["--explainers"].split(",") if n) if "--explainers" in opt else explain.EXPLAINERS
IG_STEPS = int(opt.get("--ig-steps", 16))
MO_STEPS = int(opt.get("--mo-steps", 100))
SV_PERMUTATIONS = int(opt.get("--sv-permutations", 16))
CURVES = tuple(float(f) for f in opt["--curves"].split(",") if f) if "--curves" in opt else None
V, A = 2578, 1842

cfg = dataclasses.replace(synthetic.CFG1, num_graphs=GRAPHS, sampler="imle", sample_k=K)
model = synthetic.build_answer_model(cfg).eval().to(dev)
tables = explain.TokenTables({f"w{i}": i for i in range(V)}, [f"w{(11 * a) % V}" if a % 3 == 0 else f"answer {a}" for a in range(A)])
gen = torch.Generator().manual_seed(17)
batches = []
with torch.no_grad():
    for b in range(BATCHES):
        wl = synthetic.make_workload(dataclasses.replace(cfg, seed=cfg.seed + b))
        d = wl.to(dev)
        names = torch.randint(0, V, (wl.x.size(0),), generator=gen)
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), wl.graph_sizes[0].cumsum(0)])
        label = model(d)[0].argmax(1).cpu()
        label[2::3] = (label[2::3] + 1) % A                      # a third of the answers wrong
        qtok = torch.full((GRAPHS, 6), -1, dtype=torch.int32)
        for g in range(GRAPHS):                                  # question words: three name nodes of the graph, one names nothing
            own = names[ptr[g]:ptr[g + 1]]
            qtok[g, :3] = own[torch.randint(0, own.numel(), (3,), generator=gen)].int()
            qtok[g, 3] = int(torch.randint(0, V, (1,), generator=gen))
        gold = synthetic.make_gold(wl.graph_sizes[0], seed=b)
        batches.append(explain.EvalBatch(d, label.to(dev), qtok.to(dev), (torch.arange(GRAPHS) % 4 == 0).int().to(dev), names.to(dev),
                                         gold=gold.to(dev)))
report = explain.compare(model, batches, tables, explainers=EXPLAINERS, k=K, max_instances=MAX_INSTANCES, ig_steps=IG_STEPS,
                         mo_steps=MO_STEPS, sv_permutations=SV_PERMUTATIONS, curves=CURVES)
out = {"device": torch.cuda.get_device_name(0), "graphs_per_batch": GRAPHS, "batches": BATCHES, "k": K, "explainers": {}}
for name, r in report.items():
    g = r.grounding.sets["any"]["all"]
    out["explainers"][name] = {"fid_plus": r.fid_plus, "fid_minus": r.fid_minus, "jaccard_with_intrinsic": r.jaccard,
                               "accuracy": r.coo.accuracy, "ans_tok_coo": r.coo.ans_tok_coo, "qst_tok_coo": r.coo.qst_tok_coo,
                               "grounding_precision": g.precision, "grounding_recall": g.recall, "grounding_chance": g.chance}
    print(f"{name:10s} fid+ {r.fid_plus:.4f}  fid- {r.fid_minus:.4f}  jaccard {r.jaccard:.3f}  qst coo {r.coo.qst_tok_coo:.3f}  "
          f"grounding p {g.precision:.3f} r {g.recall:.3f} (chance {g.chance:.3f})", flush=True)
    if r.curves is not None:
        c = r.curves
        out["explainers"][name]["curves"] = {"fractions": c.fractions, "p_keep": c.p_keep, "p_remove": c.p_remove, "auc_keep": c.auc_keep,
                                             "auc_remove": c.auc_remove, "counted": c.counted, "skipped": c.skipped}
        print(f"{'':10s} area kept {c.auc_keep:.4f}  area removed {c.auc_remove:.4f}  kept " + " ".join(f"{v:.3f}" for v in c.p_keep)
              + "  removed " + " ".join(f"{v:.3f}" for v in c.p_remove), flush=True)
if "--out" in opt:
    with open(opt["--out"], "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
