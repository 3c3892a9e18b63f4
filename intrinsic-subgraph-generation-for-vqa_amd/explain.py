"""The generated subgraph as a graph, and what it is worth to the answer.

A forward returns the sampled subgraph as a float node mask (`imle_mask`, [N, 1]).  `ops.subgraph_cut` turns that mask into the
induced subgraph of the whole batch on the device; this module carries a batch across such a cut and asks the model the two
questions an intrinsic explanation has to answer (the reference evaluates them one question per forward, on the host:
run_token_coo.py:65-173): does the subgraph ALONE still give the answer (fid_minus: sufficiency), and does the answer go away
when the subgraph is REMOVED (fid_plus: necessity).
"""
from __future__ import annotations

import argparse
from typing import Dict, NamedTuple, Optional

import torch
from torch import Tensor

from . import ops, synthetic


class Fidelity(NamedTuple):
    pred: Tensor           # int64 [B]: the class predicted on the whole graph
    p: Tensor              # [B]: its softmax probability on the whole graph
    p_keep: Tensor         # [B]: ... on the subgraph alone
    p_removed: Tensor      # [B]: ... with the subgraph removed
    fid_minus: Tensor      # [B]: p - p_keep (small: the subgraph is sufficient)
    fid_plus: Tensor       # [B]: p - p_removed (large: the subgraph is necessary); NaN where `emptied`
    emptied: Tensor        # bool [B]: removal would have left the graph without nodes; it went through the removal forward unchanged


class Faithfulness(NamedTuple):
    scores: Fidelity
    logits: Tensor
    logits_keep: Tensor
    logits_removed: Tensor
    mask: Tensor                   # the forward's node mask [N, 1]
    kept_none: Tensor              # bool [B]: the mask kept no node of a graph that has some; it went through the keep forward
                                   # unchanged and its fid_minus is NaN (no top-k sampler produces such a mask)
    keep: "ops.SubgraphCut"
    removed: "ops.SubgraphCut"


def fidelity_scores(logits: Tensor, logits_keep: Tensor, logits_removed: Tensor, emptied: Tensor) -> Fidelity:
    """The arithmetic of faithfulness() on three [B, classes] logit tensors (any device)."""
    prob = torch.softmax(logits.float(), dim=1)
    pred = prob.argmax(dim=1)
    pick = pred.unsqueeze(1)
    p = prob.gather(1, pick).squeeze(1)
    p_keep = torch.softmax(logits_keep.float(), dim=1).gather(1, pick).squeeze(1)
    p_removed = torch.softmax(logits_removed.float(), dim=1).gather(1, pick).squeeze(1)
    emptied = emptied.to(device=p.device, dtype=torch.bool)
    fid_plus = torch.where(emptied, torch.full_like(p, float("nan")), p - p_removed)
    return Fidelity(pred, p, p_keep, p_removed, p - p_keep, fid_plus, emptied)


def cut_workload(wl: "synthetic.Workload", cut: "ops.SubgraphCut") -> "synthetic.Workload":
    """The batch of an AnswerModel across a cut: node and edge rows gathered, the questions' tensors and the per-graph bounds
    (which hold for any subgraph) carried over; graph_sizes no longer describes the batch and is dropped."""
    return synthetic.Workload(cut.gather_nodes(wl.x), cut.edge_index, cut.gather_edges(wl.edge_attr), cut.batch, wl.instr, wl.glf,
                              wl.num_graphs, wl.max_nodes, wl.max_edges, None)


def cut_scene_graphs(node_embeddings: Tensor, edge_embeddings: Tensor, scene_graphs, cut: "ops.SubgraphCut"):
    """(node_embeddings', edge_index', edge_embeddings', batch', scene_graphs') of ISubGVQA.forward across a cut.  added_sym_edge
    holds positions in the GLOBAL edge list as the encoder applies them (quirk Q6): they follow their edges."""
    sym = getattr(scene_graphs, "added_sym_edge", None)
    sg = argparse.Namespace(x_bbox=cut.gather_nodes(scene_graphs.x_bbox),
                            added_sym_edge=None if sym is None else cut.remap_edge_positions(sym),
                            max_nodes=getattr(scene_graphs, "max_nodes", None), max_edges=getattr(scene_graphs, "max_edges", None))
    return cut.gather_nodes(node_embeddings), cut.edge_index, cut.gather_edges(edge_embeddings), cut.batch, sg


def _per_graph_any(flags: Tensor, batch: Tensor, B: int) -> Tensor:
    return torch.zeros(B, dtype=torch.int64, device=flags.device).index_add_(0, batch, flags.long()) > 0


def faithfulness(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                 threshold: float = 0.0) -> Faithfulness:
    """One forward, the keep-cut and the removal-cut of its node mask, one forward on each.  `inputs`: a synthetic.Workload for
    an AnswerModel, a synthetic.FullWorkload (or any object with its fields and scene_graphs()) for ISubGVQA.  A graph that a cut
    would leave without nodes goes through that forward whole (the flags are adjusted before the cut): the model never sees an
    empty graph it was not given."""
    full = not isinstance(model, synthetic.AnswerModel)
    B = int(inputs.questions.size(0) if full else inputs.glf.size(0))
    with torch.no_grad():
        plan = ops.GraphPlan.build(inputs.batch, inputs.edge_index, num_graphs=B, max_nodes=inputs.max_nodes or None,
                                   max_edges=inputs.max_edges or None, graph_sizes=inputs.graph_sizes)

        def forward(x, edge_index, edge_attr, batch, sg, p):
            if full:
                out = model(x, edge_index, edge_attr, batch, inputs.questions, inputs.att_mask, return_masks=True,
                            scene_graphs=sg, noises=noises, seed=seed, plan=p)
            else:
                out = model(synthetic.Workload(x, edge_index, edge_attr, batch, inputs.instr, inputs.glf, B, inputs.max_nodes,
                                               inputs.max_edges, None), noises=noises, seed=seed, plan=p)
            return out[0], out[1]

        sg = inputs.scene_graphs() if full else None
        logits, mask = forward(inputs.x, inputs.edge_index, inputs.edge_attr, inputs.batch, sg, plan)
        flat = mask.reshape(-1)
        keep = flat > threshold
        has_nodes = (plan.ptr[1:] > plan.ptr[:-1])
        kept_none = has_nodes & ~_per_graph_any(keep, inputs.batch, B)
        emptied = has_nodes & ~_per_graph_any(~keep, inputs.batch, B)
        inf = torch.full_like(flat, float("inf"))
        cuts, outs = [], []
        for whole, fill, complement in ((kept_none, inf, False), (emptied, -inf, True)):
            m = torch.where(whole[inputs.batch], fill, flat).contiguous()
            cut = ops.subgraph_cut(m, inputs.edge_index, plan, threshold=threshold, complement=complement)
            if full:
                args = cut_scene_graphs(inputs.x, inputs.edge_attr, sg, cut)
            else:
                w = cut_workload(inputs, cut)
                args = (w.x, w.edge_index, w.edge_attr, w.batch, None)
            cuts.append(cut)
            outs.append(forward(*args, cut.plan())[0])
        scores = fidelity_scores(logits, outs[0], outs[1], emptied)
        scores = scores._replace(fid_minus=torch.where(kept_none, torch.full_like(scores.p, float("nan")), scores.fid_minus))
    return Faithfulness(scores, logits, outs[0], outs[1], mask, kept_none, cuts[0], cuts[1])
