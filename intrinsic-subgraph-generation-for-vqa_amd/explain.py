"""The generated subgraph as a graph, and what it is worth to the answer.

A forward returns the sampled subgraph as a float node mask (`imle_mask`, [N, 1]).  `ops.subgraph_cut` turns that mask into the
induced subgraph of the whole batch on the device; this module carries a batch across such a cut and asks the model the two
questions an intrinsic explanation has to answer (the reference evaluates them one question per forward, on the host:
run_token_coo.py:65-173): does the subgraph ALONE still give the answer (fid_minus: sufficiency), and does the answer go away
when the subgraph is REMOVED (fid_plus: necessity).

The reference's third question is lexical (run_token_coo.py:145-185, utils/token_coo_fns.py): is the answer's name among the picked
nodes, and how many of the question's words that name an object of the graph were picked.  `TokenTables` turns the strings into
vocabulary ids once, `ops.token_coo` scores whole batches on the device into running totals, `CooReport` reads them -- the one
device-to-host copy of an evaluation (`evaluate`).

Something to hold the intrinsic mask against: `occlusion` gives leave-one-out attributions -- a forward-only post-hoc baseline on
the batch of instances `ops.induced_instances` makes in one pass --, `faithfulness_of_mask` asks the two fidelity questions of ANY
node mask, and `compare` reports the model's own mask, the occlusion mask and a random one by the same yardsticks.
`attention_rollout` is the one-forward baseline, `integrated_gradients` (with gradient x input as its one-point case) the gradient
one: the points of a straight path as one batch of instances, their gradient rows reduced to attributions on the device.
`mask_optimization` is the learned one (GNNExplainer): a soft node mask optimised by Adam, an iteration's arithmetic in one launch.
`shapley_values` is the sampled one: permutation sampling, the prefixes of all permutations as one batch of instances.
`fidelity_curves` scores ANY node ranking along its whole length -- the top-ranked nodes kept alone or removed, level by level --
and `compare(curves=...)` does so for every explainer.

The frame they share: an explainer starts from `_whole_batch` (the model's answer on the whole batch) or, in row
space, from `_encoded_rows`; its result owes `scores()` and `mask(k)` (`_Ranked`); it joins `compare` by one entry of `_COMPARE`.
"""
from __future__ import annotations

import argparse
import functools
import math
import operator
from dataclasses import dataclass, field, replace
from typing import Dict, Iterable, List, Mapping, NamedTuple, Optional, Sequence, Tuple

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
    pred, p = _predicted(logits)
    pick = pred.unsqueeze(1)
    p_keep = torch.softmax(logits_keep.float(), dim=1).gather(1, pick).squeeze(1)
    p_removed = torch.softmax(logits_removed.float(), dim=1).gather(1, pick).squeeze(1)
    emptied = emptied.to(device=p.device, dtype=torch.bool)
    fid_plus = torch.where(emptied, torch.full_like(p, float("nan")), p - p_removed)
    return Fidelity(pred, p, p_keep, p_removed, p - p_keep, fid_plus, emptied)


def cut_workload(wl: "synthetic.Workload", cut: "ops.SubgraphCut") -> "synthetic.Workload":
    """The batch of an AnswerModel across a cut: node and edge rows gathered, the questions' tensors and the per-graph bounds
    (which hold for any subgraph) carried over; graph_sizes no longer describes the batch and is dropped.  A cut is driven by the
    mask, not by k: with a node budget per graph (sample_ratio) a caller who wants SubgraphCut.sel passes the cap
    (sample_k) as ops.subgraph_cut's table_k, and the rows of graphs with a smaller budget end in -1 earlier."""
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


def _forwarder(model, inputs, noises, seed):
    """(full, B, forward) of a model and its batch: forward(x, edge_index, edge_attr, batch, sg, plan, rows=None, noises=...) ->
    (logits, mask) on a batch cut at the model's input.  rows: int64 [B'] -- row r of the question side is question rows[r] of
    `inputs` (a batch of instances); None: the questions as they are."""
    full = not isinstance(model, synthetic.AnswerModel)
    B = int(inputs.questions.size(0) if full else inputs.glf.size(0))

    def forward(x, edge_index, edge_attr, batch, sg, p, rows=None, nz=noises, trace=None):
        extra = {} if trace is None else {"trace": trace}
        if full:
            q, am = (inputs.questions, inputs.att_mask) if rows is None else (inputs.questions.index_select(0, rows),
                                                                            inputs.att_mask.index_select(0, rows))
            # (ISubGVQA.forward keeps its signature: a trace goes through forward_traced)
            call = model if trace is None else functools.partial(model.forward_traced, trace)
            out = call(x, edge_index, edge_attr, batch, q, am, return_masks=True, scene_graphs=sg, noises=nz, seed=seed, plan=p)
        else:
            instr, glf = (inputs.instr, inputs.glf) if rows is None else (inputs.instr.index_select(1, rows).contiguous(),
                                                                          inputs.glf.index_select(0, rows))
            out = model(synthetic.Workload(x, edge_index, edge_attr, batch, instr, glf, glf.size(0), inputs.max_nodes,
                                           inputs.max_edges, None), noises=nz, seed=seed, plan=p, **extra)
        return out[0], out[1]

    return full, B, forward


def _input_plan(inputs, B: int) -> "ops.GraphPlan":
    return ops.GraphPlan.build(inputs.batch, inputs.edge_index, num_graphs=B, max_nodes=inputs.max_nodes or None,
                               max_edges=inputs.max_edges or None, graph_sizes=inputs.graph_sizes)


def _predicted(logits: Tensor, want_p: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """(pred int64 [B]: the predicted class, p fp32 [B]: its softmax probability -- None unless wanted) of [B, classes] logits."""
    prob = torch.softmax(logits.float(), dim=1)
    pred = prob.argmax(dim=1)
    return pred, (prob.gather(1, pred.unsqueeze(1)).squeeze(1) if want_p else None)


class _WholeBatch(NamedTuple):
    """What an explainer starts from: the model's answer on the whole batch (_whole_batch)."""
    full: bool                     # ISubGVQA (else an AnswerModel)
    B: int
    forward: object                # _forwarder's
    plan: "ops.GraphPlan"
    sg: object                     # inputs.scene_graphs() for the full model, else None
    logits: Tensor                 # [B, classes]
    mask: Optional[Tensor]         # the forward's node mask; None when the caller gave the logits

    def predicted(self) -> Tuple[Tensor, Tensor]:
        """(pred, p): device work of its own, so only the callers that need them ask."""
        return _predicted(self.logits)


def _whole_batch(model, inputs, noises, seed, logits: Optional[Tensor] = None, plan: Optional["ops.GraphPlan"] = None,
                 trace=None) -> _WholeBatch:
    """The plan is built only when not given, the batch is forwarded (under torch.no_grad()) only when the logits are not given."""
    full, B, forward = _forwarder(model, inputs, noises, seed)
    with torch.no_grad():
        if plan is None:
            plan = _input_plan(inputs, B)
        sg, mask = inputs.scene_graphs() if full else None, None
        if logits is None:
            logits, mask = forward(inputs.x, inputs.edge_index, inputs.edge_attr, inputs.batch, sg, plan, trace=trace)
    return _WholeBatch(full, B, forward, plan, sg, logits, mask)


def _refuse_training(model, who: str, what_changes: str) -> None:
    if model.training:
        raise ValueError(f"{who} the model in eval(): in train() dropout and the training samplers would change {what_changes} -- "
                         f"call model.eval()")


def _refuse_max_instances(max_instances: Optional[int]) -> None:
    if max_instances is not None and int(max_instances) < 1:
        raise ValueError(f"max_instances must be at least 1, got {max_instances}")


def _noise_rows(noises: Optional[Dict[int, Tensor]], B: int, rows: Tensor) -> Optional[Dict[int, Tensor]]:
    """The noises' rows handed to a batch of instances by their graphs (rows: int64 [Q], the graph of every instance)."""
    return None if noises is None else {i: n.reshape(B, -1).index_select(0, rows).contiguous() for i, n in noises.items()}


def faithfulness_of_mask(model, inputs, mask: Tensor, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                         threshold: float = 0.0, logits: Optional[Tensor] = None, plan: Optional["ops.GraphPlan"] = None) -> Faithfulness:
    """faithfulness() for ANY node mask (fp32 [N] or [N, 1]; kept where > threshold): the keep-cut and the removal-cut of the
    mask, one forward on each, scored against the model's answer on the whole batch -- `logits` when the caller has them (with
    the `plan` of that forward), else one forward more.  This is how an explainer other than the model's own sampler (occlusion,
    a random baseline) is measured with the intrinsic mask's yardstick."""
    full, B, forward, plan, sg, logits, _ = _whole_batch(model, inputs, noises, seed, logits, plan)
    with torch.no_grad():
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


def faithfulness(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                 threshold: float = 0.0) -> Faithfulness:
    """One forward, the keep-cut and the removal-cut of its node mask, one forward on each.  `inputs`: a synthetic.Workload for
    an AnswerModel, a synthetic.FullWorkload (or any object with its fields and scene_graphs()) for ISubGVQA.  A graph that a cut
    would leave without nodes goes through that forward whole (the flags are adjusted before the cut): the model never sees an
    empty graph it was not given.  (The forward, then faithfulness_of_mask on its mask.)"""
    whole = _whole_batch(model, inputs, noises, seed)
    return faithfulness_of_mask(model, inputs, whole.mask, noises=noises, seed=seed, threshold=threshold, logits=whole.logits,
                                plan=whole.plan)


# ---------------------------------------------------------------------------------------------------------------------
# A post-hoc baseline: leave-one-out (occlusion) attributions
# ---------------------------------------------------------------------------------------------------------------------
def shifted_attributions(attribution: Tensor, batch: Tensor, B: int) -> Tensor:
    """fp32 [N]: the attributions moved per graph so that the smallest of a graph is 1 (a - min_g + 1) -- scores for
    ops.topk_threshold, in whose padded rows the pads hold 0 and compete: after the shift no pad beats a node, however negative
    its attribution.  The order inside a graph is kept; two attributions closer than the fp32 spacing near their shifted value
    (1.2e-7 to 2.4e-7 for probabilities) become a tie, and a threshold top-k keeps both."""
    a = attribution.float().reshape(-1)
    low = torch.full((B,), float("inf"), dtype=torch.float32, device=a.device).scatter_reduce(0, batch, a, "amin")
    return a - low.index_select(0, batch) + 1.0


def instance_sym_edges(sym: Optional[Tensor], edge_src: Tensor, E: int) -> Optional[Tensor]:
    """added_sym_edge across a batch of instances: the positions (ascending) of every instance edge whose parent edge the old list
    names.  The old list holds positions in the parent's GLOBAL edge list (quirk Q6); those beyond it name nothing, and an edge
    named several times is flipped once by the encoder, so one entry per instance edge is the same flip."""
    if sym is None:
        return None
    p = sym.long()
    p = p[(p >= 0) & (p < E)]
    named = torch.zeros(E, dtype=torch.bool, device=edge_src.device)
    named[p] = True
    return torch.nonzero(named.index_select(0, edge_src)).reshape(-1)


def instance_inputs(inputs, inst: "ops.GraphInstances", full: bool):
    """(x, edge_index, edge_attr, batch, scene_graphs or None) of a batch of instances of `inputs`' graphs, cut at the model's
    input as faithfulness() cuts it: node and edge rows through node_src / edge_src, x_bbox gathered, added_sym_edge following
    its edges (instance_sym_edges).  The question side is gathered by the caller through inst.index."""
    x, ea = inst.gather_nodes(inputs.x), inst.gather_edges(inputs.edge_attr)
    sg = None
    if full:
        src = inputs.scene_graphs()
        sg = argparse.Namespace(x_bbox=inst.gather_nodes(src.x_bbox),
                                added_sym_edge=instance_sym_edges(getattr(src, "added_sym_edge", None), inst.edge_src,
                                                                  inputs.edge_index.size(1)),
                                max_nodes=getattr(src, "max_nodes", None), max_edges=getattr(src, "max_edges", None))
    return x, inst.edge_index, ea, inst.batch, sg


def _instance_probabilities(whole: _WholeBatch, inputs, index: Tensor, keep: Tensor, pred: Tensor, p: Tensor, noises,
                            max_instances: Optional[int]):
    """(fp32 [Q]: the class pred[index[q]]'s probability on instance q, the instance batches in order) of the Q induced-subgraph
    instances that rows of keep bits name (ops.induced_instances), cut at the model's input (instance_inputs), the question rows
    gathered through index, the noises' rows handed to an instance by its graph, forwarded in chunks of at most max_instances
    instances (None: all at once).  The loop that occlusion(), fidelity_curves() and shapley_values() share; the caller holds
    torch.no_grad()."""
    Q = index.numel()
    step = Q if max_instances is None else int(max_instances)
    chunks, parts = [], []
    for lo in range(0, Q, max(step, 1)):
        rows = index[lo:lo + step].long()
        inst = ops.induced_instances(whole.plan, inputs.edge_index, index[lo:lo + step].contiguous(), keep[lo:lo + step].contiguous())
        out = whole.forward(*instance_inputs(inputs, inst, whole.full), inst.plan(), rows, _noise_rows(noises, whole.B, rows))[0]
        parts.append(torch.softmax(out.float(), dim=1).gather(1, pred.index_select(0, rows).unsqueeze(1)).squeeze(1))
        chunks.append(inst)
    return (torch.cat(parts) if parts else p.new_zeros(0)), chunks


class _Ranked:
    """What a result class owes compare() and fidelity_curves(): scores() and mask(k), over the field that `ranked` names (with
    a `plan` beside it).  Methods and one class attribute, no dataclass field."""
    ranked = "attribution"

    def scores(self) -> Tensor:
        """fp32 [N]: what mask(k) ranks, before the shift -- the scores of a fidelity curve (fidelity_curves()).  The two rules
        differ at ties: mask(k) keeps its threshold rule, under which ties at the k-th value keep MORE than k nodes; a curve's
        rank prefixes (ops.curve_keep_bits) keep exactly k, ties going to the lower node."""
        return getattr(self, self.ranked).float().reshape(-1)

    def mask(self, k) -> Tensor:
        """fp32 [N, 1], k-hot per graph, in imle_mask's layout: the k top-ranked nodes of every graph -- ops.topk_threshold on
        shifted_attributions (the samplers' zero pads compete and lose).  A graph with fewer than k nodes keeps them all; ties
        at the k-th value are all kept, as the samplers' threshold keeps them."""
        scores = shifted_attributions(getattr(self, self.ranked), self.plan.batch, self.plan.B).view(-1, 1).contiguous()
        return ops.topk_threshold(scores, k, plan=self.plan)


@dataclass
class Occlusion(_Ranked):
    """Leave-one-out attributions of one batch (occlusion()): mask(k) keeps the nodes whose removal costs the answer most."""
    pred: Tensor                   # int64 [B]: the class predicted on the whole graph
    p: Tensor                      # fp32 [B]: its softmax probability on the whole graph
    attribution: Tensor            # fp32 [N]: p[g] - (that class's probability with node n removed); 0 on the nodes of `single` graphs
    single: Tensor                 # bool [B]: fewer than 2 nodes -- no node can be removed, the graph got no instance
    index: Tensor                  # int32 [Q]: the graph of every leave-one-out instance
    inst_node: Tensor              # int64 [Q]: the node (row of the batch) every instance lacks
    p_without: Tensor              # fp32 [Q]: the predicted class's probability on every instance
    logits: Tensor                 # [B, classes] of the whole batch
    plan: "ops.GraphPlan"
    chunks: List["ops.InducedInstances"] = field(default_factory=list)      # the instance batches that were forwarded, in order


def occlusion(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
              max_instances: Optional[int] = None) -> Occlusion:
    """Leave-one-out (occlusion) attribution of every node: the change of the predicted answer's probability when that node is
    removed from its scene graph -- a forward-only post-hoc baseline for the intrinsic mask.  One forward on the batch for `pred`
    and `p`; then the batch of leave-one-out instances (ops.keep_bits_leave_one_out, ops.induced_instances: graph g gives n_g
    instances, each without one node and its edges), cut at the model's input as faithfulness() cuts it, forwarded in chunks of
    at most `max_instances` instances (None: all at once).  `inputs` as for faithfulness().  The removed node is removed BEFORE
    the encoder (the full model encodes every instance).

    A graph with fewer than 2 nodes has no instance: its attribution is 0 and it is flagged in `single`.  With a noisy sampler
    (gumbel, simple; `noises` rows are handed to an instance by its graph, where the columns behind the removed node name the next
    node) the attribution carries sampling noise: the difference of two draws, not of two expectations.  The eval solve of the
    imle / aimle samplers is noise-free."""
    _refuse_max_instances(max_instances)
    whole = _whole_batch(model, inputs, noises, seed)
    plan = whole.plan
    with torch.no_grad():
        pred, p = whole.predicted()
        index, keep, inst_node = ops.keep_bits_leave_one_out(plan)
        p_without, chunks = _instance_probabilities(whole, inputs, index, keep, pred, p, noises, max_instances)
        attribution = torch.zeros(plan.N, dtype=torch.float32, device=p.device)
        attribution[inst_node] = p.index_select(0, index.long()) - p_without
        single = (plan.ptr[1:] - plan.ptr[:-1]) < 2
    return Occlusion(pred, p, attribution, single, index, inst_node, p_without, whole.logits, plan, chunks)


# ---------------------------------------------------------------------------------------------------------------------
# A one-forward baseline: attention rollout
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class AttentionTrace:
    """What a forward with `trace=` leaves behind (MGAT.forward, AnswerModel.forward, ISubGVQA.answer_graphs / forward_traced): mutable,
    filled by the call, once."""
    alphas: Optional[List[Tensor]] = None           # L tensors fp32 [E, H]: every layer's attention weights, in the caller's edge order
    masks: Optional[List[Optional[Tensor]]] = None  # L entries: a layer's node mask fp32 [N, 1], or None where the layer has none
    mask: Optional[Tensor] = None                   # the forward's node mask (its second result)
    gate: Optional[Tensor] = None                   # the read-out's pooling weights (its third result)


@dataclass
class Rollout(_Ranked):
    """Attention-rollout attributions of one batch (attention_rollout()): mask(k) keeps the most relevant nodes."""
    attribution: Tensor            # fp32 [N]: the relevance of every node (include/ext/isg_rollout.h)
    flow: Optional[Tensor]         # fp32 [L, E]: what every edge carried at every layer; None unless asked for
    trace: AttentionTrace          # the forward's attention weights, layer masks, mask and gate
    logits: Tensor                 # [B, classes] of the batch
    plan: "ops.GraphPlan"


def attention_rollout(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                      residual: float = 0.5, use_masks: bool = True, want_flow: bool = False) -> Rollout:
    """Attention rollout (Abnar & Zuidema 2020) of every node: the read-out's pooling weights walked back through the layers'
    head-averaged attention weights, a share `residual` of a node's relevance staying on it at every layer.  ONE forward with a
    trace, under torch.no_grad(), and one launch (ops.attention_rollout); `inputs` as for faithfulness().
    The walk starts from gate * mask (a masked node's pooled term is exactly zero, att_pooling.py), or from the gate alone when
    the forward has no mask.  use_masks=False hands the kernel no layer masks: the attention weights alone decide."""
    trace = AttentionTrace()
    whole = _whole_batch(model, inputs, noises, seed, trace=trace)
    with torch.no_grad():
        start = trace.gate.float().reshape(-1)
        if trace.mask is not None:
            start = start * trace.mask.float().reshape(-1)
        relevance, flow = ops.attention_rollout(whole.plan, trace.alphas, start.contiguous(), trace.masks if use_masks else None,
                                                residual=residual, want_flow=want_flow)
    return Rollout(relevance, flow, trace, whole.logits, whole.plan)


# ---------------------------------------------------------------------------------------------------------------------
# A gradient baseline: integrated gradients, with gradient x input as its one-point case
# ---------------------------------------------------------------------------------------------------------------------
QUADRATURE_RULES = ("gauss_legendre", "midpoint", "trapezoid", "endpoint")


def quadrature(steps: int, rule: str = "gauss_legendre") -> Tuple[Tensor, Tensor]:
    """(t, w): the nodes in [0, 1] and the weights of a rule for the path integral, HOST float64 [S]; the weights sum to 1.
    midpoint: t_s = (s + 1/2) / S, w = 1 / S.  trapezoid (S >= 2): t_s = s / (S - 1), the two end points weigh half.
    gauss_legendre: numpy.polynomial.legendre.leggauss mapped from [-1, 1]; exact for polynomials up to degree 2 S - 1.
    endpoint (S = 1): t = 1, w = 1 -- gradient x (input - baseline)."""
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"quadrature: steps must be an integer >= 1, got {steps!r}")
    S = int(steps)
    if rule == "midpoint":
        t = (torch.arange(S, dtype=torch.float64) + 0.5) / S
        w = torch.full((S,), 1.0 / S, dtype=torch.float64)
    elif rule == "trapezoid":
        if S < 2:
            raise ValueError("quadrature: the trapezoid rule needs steps >= 2")
        t = torch.arange(S, dtype=torch.float64) / (S - 1)
        w = torch.full((S,), 1.0 / (S - 1), dtype=torch.float64)
        w[0] = w[-1] = 0.5 / (S - 1)
    elif rule == "gauss_legendre":
        import numpy as np
        nodes, weights = np.polynomial.legendre.leggauss(S)
        t = torch.from_numpy((nodes + 1.0) * 0.5).to(torch.float64)
        w = torch.from_numpy(weights * 0.5).to(torch.float64)
    elif rule == "endpoint":
        if S != 1:
            raise ValueError("quadrature: the endpoint rule is one step (gradient x input), got steps = %d" % S)
        t, w = torch.ones(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    else:
        raise ValueError(f"quadrature: rule from {QUADRATURE_RULES}, got {rule!r}")
    return t, w


@dataclass
class PathAttributions(_Ranked):
    """Path (integrated-gradients) attributions of one batch (path_attributions(), integrated_gradients()): mask(k) keeps the nodes
    with the largest attribution."""
    attribution: Tensor                    # fp32 [N]: sum over the channels of (x - baseline) * the path's weighted gradient
    edge_attribution: Optional[Tensor]     # fp32 [E], when the edge rows were on the path
    avg_grad: Optional[Tuple[Tensor, Optional[Tensor]]]    # (fp32 [N, Cx], fp32 [E, Ce] or None): the weighted gradient rows, when asked for
    f_input: Tensor                        # fp32 [B]: the score at the input (t = 1)
    f_baseline: Tensor                     # fp32 [B]: the score at the baseline (t = 0)
    delta: Tensor                          # fp32 [B]: the graph's attributions summed - (f_input - f_baseline), the completeness gap
    plan: "ops.GraphPlan"
    steps: int
    rule: str
    chunks: List["ops.GraphInstances"] = field(default_factory=list)      # the instance batches that were forwarded, in order
    pred: Optional[Tensor] = None          # int64 [B]: the class that was explained (integrated_gradients)
    logits: Optional[Tensor] = None        # [B, classes] of the whole batch (integrated_gradients)


def _step_instances(plan: "ops.GraphPlan", edge_index: Tensor, steps: int) -> "ops.GraphInstances":
    """`steps` instances of every graph, the copies of one graph next to each other: index[q] = q // steps."""
    index = torch.arange(plan.B * steps, dtype=torch.int64) // max(steps, 1)
    return ops.graph_instances(plan, edge_index, index, sizes=plan.sizes_host)


def path_attributions(score, x: Tensor, e: Tensor, plan: "ops.GraphPlan", edge_index: Tensor, *, steps: int = 16,
                      rule: str = "gauss_legendre", baseline_x: Optional[Tensor] = None, baseline_e: Optional[Tensor] = None,
                      edges: bool = False, rows: bool = False, max_instances: Optional[int] = None) -> PathAttributions:
    """Integrated gradients of `score` along the straight path from a baseline to the rows (x, e) of a batch -- the model-free
    core.  score(x_inst, e_inst, inst) -> fp32 [Q']: any differentiable function of an instance batch (inst: its
    ops.GraphInstances) whose instances do not interact.  x fp32 [N, Cx], e fp32 [E, Ce] of the batch `plan` describes (built
    from its batch vector); a baseline is None (zeros), one row [C] or rows [rows, C].

    The S points of the rule (quadrature) become instances: per chunk of whole steps -- all B graphs x a run of steps, at most
    `max_instances` instances but at least one step -- ops.graph_instances expands the batch, ops.ig_path_rows writes the
    points' rows in one launch, the rows become leaves, ONE torch.autograd.grad call under torch.enable_grad() takes the gradient
    of score(...).sum() with respect to them (no parameter's .grad is touched), and ops.ig_attribution reduces the gradient
    rows to attributions in one launch, adding to the running result.  edges=True puts the edge rows on the path as well;
    otherwise they stay at the input.  rows=True also returns the weighted gradient rows.  The score at t = 1 and t = 0 comes
    from one two-step instance batch without a gradient; `delta` is computed on the device."""
    t_host, w_host = quadrature(steps, rule)
    S, B = int(steps), plan.B
    if plan.batch is None:
        raise ValueError("path_attributions needs a GraphPlan built from the batch vector")
    _refuse_max_instances(max_instances)
    per = S if max_instances is None else max(1, min(S, int(max_instances) // max(B, 1)))
    with torch.no_grad():
        x, e = x.detach(), e.detach()
        dev = x.device
        bx = None if baseline_x is None else baseline_x.detach()
        be = None if baseline_e is None or not edges else baseline_e.detach()
        res, chunks = None, []
        for lo in range(0, S, per):
            sc = min(per, S - lo)
            inst = _step_instances(plan, edge_index, sc)
            t = t_host[lo:lo + sc].float().repeat(B).to(dev)
            w = w_host[lo:lo + sc].float().repeat(B).to(dev)
            x_inst, e_inst = ops.ig_path_rows(inst, x, e, t, bx, be, path_edges=edges)
            leaves = [x_inst.requires_grad_(True)] + ([e_inst.requires_grad_(True)] if edges else [])
            with torch.enable_grad():
                total = score(x_inst, e_inst, inst).sum()
                grads = torch.autograd.grad(total, leaves)
            res = ops.ig_attribution(inst, grads[0].contiguous(), grads[1].contiguous() if edges else None, w, x, e, bx, be,
                                     want_rows=rows, out=res)
            chunks.append(inst)
        ends = _step_instances(plan, edge_index, 2)
        x_end, e_end = ops.ig_path_rows(ends, x, e, torch.tensor([1.0, 0.0]).repeat(B).to(dev), bx, be, path_edges=edges)
        f = score(x_end, e_end, ends).float().reshape(B, 2)
        f_input, f_baseline = f[:, 0].contiguous(), f[:, 1].contiguous()
        total = torch.zeros(B, dtype=torch.float32, device=dev).index_add_(0, plan.batch, res.attr_x)
        if edges:
            total.index_add_(0, plan.batch.index_select(0, edge_index[1]), res.attr_e)
        delta = total - (f_input - f_baseline)
    return PathAttributions(res.attr_x, res.attr_e, (res.avg_x, res.avg_e) if rows else None, f_input, f_baseline, delta, plan, S,
                            rule, chunks)


def _graph_mean_rows(rows: Tensor, graph: Tensor, B: int) -> Tensor:
    """fp32 [rows, C]: every row replaced by the mean row of its graph."""
    sums = torch.zeros(B, rows.size(1), dtype=torch.float32, device=rows.device).index_add_(0, graph, rows.float())
    count = torch.zeros(B, dtype=torch.float32, device=rows.device).index_add_(0, graph, torch.ones_like(graph, dtype=torch.float32))
    return (sums / count.clamp_min(1.0).unsqueeze(1)).index_select(0, graph).contiguous()


def _row_answer(model, inputs, full: bool, seed):
    """answer(x, e, edge_index, batch, instr, glf, plan, noises) -> [B', classes]: the model on rows the MGAT reads, for the row-space
    explainers -- ISubGVQA.answer_graphs behind the encoder, an AnswerModel as it is."""
    def answer(x, e, edge_index, batch, instr, glf, plan, noises):
        if full:
            return model.answer_graphs(x, edge_index, e, batch, instr, glf, plan, True, noises, seed)[0]
        return model(synthetic.Workload(x, edge_index, e, batch, instr, glf, glf.size(0), inputs.max_nodes, inputs.max_edges, None),
                     noises=noises, seed=seed, plan=plan)[0]

    return answer


def _encoded_rows(model, inputs, noises, seed, full: bool, plan: "ops.GraphPlan", answer):
    """(x, e, glf, instr, logits, pred): the fp32 rows the MGAT reads and the question side beside them -- for ISubGVQA the
    scene-graph encoder's OUTPUT (encode_scene and language_features run once, here), for an AnswerModel the inputs' own rows --
    with the model's answer on them, under torch.no_grad().  Where integrated_gradients and mask_optimization start."""
    with torch.no_grad():
        if full:
            state = model.encode_scene(inputs.x, inputs.edge_index, inputs.edge_attr, inputs.batch, inputs.scene_graphs(), plan)
            glf, instr = model.language_features(inputs.questions, inputs.att_mask, None, None if seed is None else seed + 7919)
            x, e = state.x_enc.float().contiguous(), state.e_enc.float().contiguous()
            logits = answer(x, e, inputs.edge_index, inputs.batch, instr, glf, plan, noises)
        else:
            glf, instr = inputs.glf, inputs.instr
            x, e = inputs.x.float().contiguous(), inputs.edge_attr.float().contiguous()
            logits = answer(inputs.x, inputs.edge_attr, inputs.edge_index, inputs.batch, instr, glf, plan, noises)
        return x, e, glf, instr, logits, _predicted(logits, want_p=False)[0]


def integrated_gradients(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                         steps: int = 16, rule: str = "gauss_legendre", baseline="zero", target: str = "prob",
                         edges: bool = False, max_instances: Optional[int] = None) -> PathAttributions:
    """Integrated gradients (Sundararajan et al. 2017) of every node: the gradient of the predicted answer's score along the
    straight path from a baseline to the rows the MGAT reads, integrated by `rule` over `steps` points and multiplied by
    (row - baseline) -- a gradient post-hoc baseline for the intrinsic mask (path_attributions does the work).  steps=1 with
    rule="endpoint" is gradient x input.  `inputs` as for occlusion().  One forward under no_grad gives `pred` and `logits`; the
    score is the softmax probability (target="prob", occlusion's yardstick) or the logit (target="logit") of class pred[graph]
    on every instance, the question side gathered by the instance's graph.

    For an AnswerModel the path lies in inputs.x / inputs.edge_attr.  For ISubGVQA it lies in the scene-graph encoder's OUTPUT:
    encode_scene and language_features run once, every chunk runs answer_graphs on the path's rows -- the token ids have no
    straight path, so the attribution is that of the rows the MGAT reads, not of the tokens.
    baseline: "zero", "mean" (every graph's mean row) or a tensor ([C] or [N, C]; a pair (x, e) with edges=True).

    The model must be in eval().  The samplers along the path behave as the model's autograd defines there: imle / aimle give a
    constant threshold mask (no gradient through the selection), gumbel is straight-through, simple differentiates its marginals.
    The mask may CHANGE along the path (the score is then not smooth in t); `delta`, the completeness gap, reports what that and
    the quadrature cost.  No parameter's .grad is touched."""
    _refuse_training(model, "integrated_gradients explains", "the score from point to point")
    if target not in ("prob", "logit"):
        raise ValueError(f"target: 'prob' or 'logit', got {target!r}")
    full, B, _ = _forwarder(model, inputs, noises, seed)
    answer = _row_answer(model, inputs, full, seed)
    with torch.no_grad():
        plan = _input_plan(inputs, B)
        x, e, glf, instr, logits, pred = _encoded_rows(model, inputs, noises, seed, full, plan, answer)
        graph_e = inputs.batch.index_select(0, inputs.edge_index[1])
        if isinstance(baseline, str):
            if baseline not in ("zero", "mean"):
                raise ValueError(f"baseline: 'zero', 'mean' or a tensor, got {baseline!r}")
            bx = None if baseline == "zero" else _graph_mean_rows(x, inputs.batch, B)
            be = None if baseline == "zero" or not edges else _graph_mean_rows(e, graph_e, B)
        elif isinstance(baseline, (tuple, list)):
            bx, be = baseline
        else:
            bx, be = baseline, None

    def score(x_inst, e_inst, inst):
        rows = inst.index.long()
        nz = _noise_rows(noises, B, rows)
        ins, g = instr.index_select(1, rows).contiguous(), glf.index_select(0, rows)
        out = answer(x_inst, e_inst, inst.edge_index, inst.batch, ins, g, inst.plan(), nz).float()
        pick = pred.index_select(0, rows).unsqueeze(1)
        return (torch.softmax(out, dim=1) if target == "prob" else out).gather(1, pick).squeeze(1)

    res = path_attributions(score, x, e, plan, inputs.edge_index, steps=steps, rule=rule, baseline_x=bx, baseline_e=be, edges=edges,
                            max_instances=max_instances)
    return replace(res, pred=pred, logits=logits)


# ---------------------------------------------------------------------------------------------------------------------
# A learned baseline: mask optimisation (GNNExplainer)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class MaskOptimization(_Ranked):
    """The learned soft node mask of one batch (mask_optimize(), mask_optimization()): B independent GNNExplainer runs.  mask(k)
    keeps the nodes with the largest soft mask."""
    theta: Tensor                          # fp32 [N]: the logit of every node after the last step
    soft: Tensor                           # fp32 [N]: sigmoid(theta), the soft mask
    nll: Tensor                            # fp32 [steps + 1, B] on the device: the score at the mask BEFORE step i (row 0: the initial
                                           # mask) and, in the last row, at the final mask
    plan: "ops.GraphPlan"
    steps: int
    edge_theta: Optional[Tensor] = None    # fp32 [E], when the edge rows had logits of their own (edges=True)
    edge_soft: Optional[Tensor] = None
    pred: Optional[Tensor] = None          # int64 [B]: the class that was explained
    logits: Optional[Tensor] = None        # [B, classes] of the whole, unmasked batch (mask_optimization)
    ranked = "soft"                        # (no annotation: not a field)


def _edge_ranges(plan: "ops.GraphPlan", edge_index: Tensor) -> Tensor:
    """int32 [B + 1] on the device: the range of every graph's rows in the caller's edge order (a graph's edges lie next to each
    other, as a collated batch has them); counted on the device, nothing is copied to the host."""
    count = torch.bincount(plan.batch.index_select(0, edge_index[1]), minlength=plan.B)
    return torch.cat([count.new_zeros(1), count.cumsum(0)]).to(torch.int32).contiguous()


def _initial_logits(init, rows: int, gen, dev, name: str) -> Tensor:
    if torch.is_tensor(init):
        if init.numel() != rows:
            raise ValueError(f"mask_optimize: init for the {name} rows holds {init.numel()} logits, the batch has {rows}")
        return init.detach().to(device=dev, dtype=torch.float32).reshape(-1).clone()
    return float(init) * torch.randn(rows, generator=gen, device=dev, dtype=torch.float32)


def mask_optimize(score, x: Tensor, e: Tensor, plan: "ops.GraphPlan", edge_index: Tensor, *, pred_rows: Optional[Tensor] = None,
                  steps: int = 100, lr: float = 0.01, a_size: float = 1.0, a_ent: float = 0.1, init=0.1, init_seed: int = 0,
                  edges: bool = False) -> MaskOptimization:
    """GNNExplainer's optimisation (Ying et al. 2019, PyG's GNNExplainer with an object-level node mask) of `score` over the rows
    (x, e) of a batch -- the model-free core.  score(x_m, e_m) -> fp32 [B]: any differentiable per-graph loss of the MASKED rows
    whose graphs do not interact.  One logit theta[n] per node, the score reads sigmoid(theta[n]) * x[n]; per graph
        score + a_size * mean_n sigmoid(theta) + a_ent * mean_n H(sigmoid(theta))
    is minimised by `steps` Adam steps of rate `lr`; the batch loss is the sum over the graphs and Adam is elementwise, so the B
    graphs are B independent runs.  edges=True learns a second logit per edge row, with the means over each graph's edge rows.

    Per iteration: the masked rows become leaves, ONE torch.autograd.grad call under torch.enable_grad() takes the gradient of
    score(...).sum() with respect to them (no parameter's .grad is touched), and ONE ops.maskopt_step per half turns the gradient
    rows into d theta, takes the Adam step and writes the next masked rows (include/ext/isg_maskopt.h).  Nothing is copied to the
    host inside the loop.  init: the std of seeded normal logits drawn on the device (init_seed), or a tensor of logits ([N]; a
    pair ([N], [E]) with edges=True).  pred_rows (int64 [B]): the classes the score explains, kept in the result."""
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 0:
        raise ValueError(f"mask_optimize: steps must be an integer >= 0, got {steps!r}")
    if plan.batch is None:
        raise ValueError("mask_optimize needs a GraphPlan built from the batch vector")
    T, B = int(steps), plan.B
    kw = dict(a_size=a_size, a_ent=a_ent, lr=lr)
    with torch.no_grad():
        x, e = x.detach(), e.detach()
        dev = x.device
        gen = torch.Generator(device=dev).manual_seed(int(init_seed))
        init_x, init_e = init if isinstance(init, (tuple, list)) else (init, init)
        halves = [(x, plan.ptr, _initial_logits(init_x, x.size(0), gen, dev, "node"))]
        if edges:
            halves.append((e, _edge_ranges(plan, edge_index), _initial_logits(init_e, e.size(0), gen, dev, "edge")))
        moments = [(torch.zeros_like(th), torch.zeros_like(th)) for _, _, th in halves]
        masked = [ops.maskopt_step(rows, None, seg, th, None, None, step=1, **kw)[0] for rows, seg, th in halves]
        nll = torch.empty(T + 1, B, dtype=torch.float32, device=dev)
        for it in range(1, T + 1):
            leaves = [m.requires_grad_(True) for m in masked]
            with torch.enable_grad():
                f = score(leaves[0], leaves[1] if edges else e)
                grads = torch.autograd.grad(f.sum(), leaves)
            nll[it - 1] = f.detach().float().reshape(B)
            masked = [ops.maskopt_step(rows, g.contiguous(), seg, th, mv[0], mv[1], step=it, **kw)[0]
                      for (rows, seg, th), mv, g in zip(halves, moments, grads)]
        nll[T] = score(masked[0], masked[1] if edges else e).float().reshape(B)
        theta = halves[0][2]
        edge_theta = halves[1][2] if edges else None
    return MaskOptimization(theta, torch.sigmoid(theta), nll, plan, T, edge_theta, None if edge_theta is None else torch.sigmoid(edge_theta),
                            pred_rows)


def mask_optimization(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None, steps: int = 100,
                      lr: float = 0.01, a_size: float = 1.0, a_ent: float = 0.1, init=0.1, init_seed: int = 0,
                      edges: bool = False) -> MaskOptimization:
    """GNNExplainer (Ying et al. 2019) of every node: a soft mask on the rows the MGAT reads, learned so that the masked graph
    still gives the model's answer -- the learned post-hoc baseline for the intrinsic mask (mask_optimize does the work; PyG's
    defaults).  `inputs` as for occlusion().  One forward under no_grad gives `pred` and `logits`; the score is
    -log softmax(logits)[pred[graph]] of the masked batch.

    For an AnswerModel the mask scales inputs.x (and inputs.edge_attr with edges=True).  For ISubGVQA it scales the scene-graph
    encoder's OUTPUT rows, as integrated_gradients' path lies there: encode_scene and language_features run once, every iteration
    runs answer_graphs.  The model must be in eval(); the samplers behave as integrated_gradients states for eval() under
    autograd, and the model's own mask may change from one iteration to the next.  No parameter's .grad is touched."""
    _refuse_training(model, "mask_optimization explains", "the score from iteration to iteration")
    full, B, _ = _forwarder(model, inputs, noises, seed)
    answer = _row_answer(model, inputs, full, seed)
    with torch.no_grad():
        plan = _input_plan(inputs, B)
        x, e, glf, instr, logits, pred = _encoded_rows(model, inputs, noises, seed, full, plan, answer)
        pick = pred.unsqueeze(1)

    def score(x_m, e_m):
        out = answer(x_m, e_m, inputs.edge_index, inputs.batch, instr, glf, plan, noises)
        return -torch.log_softmax(out.float(), dim=1).gather(1, pick).squeeze(1)

    res = mask_optimize(score, x, e, plan, inputs.edge_index, pred_rows=pred, steps=steps, lr=lr, a_size=a_size, a_ent=a_ent,
                        init=init, init_seed=init_seed, edges=edges)
    return replace(res, logits=logits)


# ---------------------------------------------------------------------------------------------------------------------
# Token co-occurrence
# ---------------------------------------------------------------------------------------------------------------------
class TokenTables:
    """The strings of the reference's scoring as scene-graph vocabulary ids.  `stoi`: loader.SceneGraphVocab.get_stoi();
    `answers`: the answer strings by class (label2ans); `clip_itos`: the question tokenizer's tokens by id, for the text
    explanation (their `</w>` is stripped as at run_token_coo.py:83-85).  A string that is no vocabulary token maps to -1."""

    def __init__(self, stoi: Mapping[str, int], answers: Sequence[str], clip_itos: Optional[Sequence[str]] = None):
        self.stoi = dict(stoi)
        ids = lambda strings: torch.tensor([self.stoi.get(s, -1) for s in strings], dtype=torch.int32)
        self.ans_sg = ids(answers)
        self.clip_sg = None if clip_itos is None else ids([clip_itos[i].replace("</w>", "") for i in range(len(clip_itos))])
        self._on: Dict[Tuple[str, torch.device], Tensor] = {}

    def on(self, name: str, device) -> Tensor:
        """ans_sg / clip_sg on `device` (copied there once)."""
        key = (name, torch.device(device))
        if key not in self._on:
            self._on[key] = getattr(self, name).to(device)
        return self._on[key]

    def question_words(self, questions: Sequence[str], device=None) -> Tuple[Tensor, Tensor]:
        """(qtok int32 [B, T], qflags int32 [B]) of raw question strings: the words of `q.split("?")[0].lower().split(" ")`
        (token_coo_fns.py:15 -- an empty word between two spaces is a word) as vocabulary ids, padded with -1 to the longest
        question; bit 0 of qflags is `"color" in q` (token_coo_fns.py:8, on the raw string)."""
        words = [[self.stoi.get(w, -1) for w in q.split("?")[0].lower().split(" ")] for q in questions]
        T = max((len(w) for w in words), default=0)
        qtok = torch.tensor([w + [-1] * (T - len(w)) for w in words], dtype=torch.int32).view(len(words), T)
        qflags = torch.tensor([int("color" in q) for q in questions], dtype=torch.int32)
        return (qtok, qflags) if device is None else (qtok.to(device), qflags.to(device))

    def text_tokens(self, input_ids: Tensor) -> Tensor:
        """clip_sg[input_ids]: the question's tokens as vocabulary ids (int32, on input_ids' device)."""
        if self.clip_sg is None:
            raise ValueError("TokenTables was built without clip_itos")
        return self.on("clip_sg", input_ids.device)[input_ids.long()].contiguous()


def _mean(num: float, den: float) -> float:
    return num / den if den else float("nan")


@dataclass(frozen=True)
class CooReport:
    """The figures of run_token_coo.py:181-185 from isg_token_coo's running totals.  The fields are plain means over the
    questions that have the quantity (NaN when none has); as_printed_by_reference() gives what the script prints."""
    totals: Tuple[int, ...]
    accuracy: float            # correct / questions
    accuracy_at: float         # ... among the questions whose predicted answer names a node of the graph
    ans_tok_coo: float         # the answer's name is among the picked nodes; over correct, non-"color" questions whose answer names a node
    qst_tok_coo: float         # mean over correct questions of (question words naming a picked node / naming a node)
    text_tok_coo: float        # the same over the kept tokens of the text explanation
    by_type: Optional[Dict[str, Dict[str, "CooReport"]]] = field(default=None, compare=False)   # evaluate(types=...): {facet: {name: report}}
    grounding: Optional["GroundingReport"] = field(default=None, compare=False)                 # evaluate(grounding=True)

    @staticmethod
    def _ratio_sum(totals: Sequence[int], which: int) -> float:
        """Sum of the per-question ratios hits / m from the histogram pair `which` (0 question words, 1 text tokens)."""
        H = ops.COO_TOKENS_MAX + 1
        hits = totals[16 + (2 * which + 1) * H:16 + (2 * which + 2) * H]
        return math.fsum(h / m for m, h in enumerate(hits) if m > 0 and h)

    @classmethod
    def from_totals(cls, totals) -> "CooReport":
        t = tuple(int(v) for v in (totals.tolist() if torch.is_tensor(totals) else totals))   # an evaluation's one device-to-host copy
        if len(t) != ops.COO_TOTALS:
            raise ValueError(f"totals: expected {ops.COO_TOTALS} entries, got {len(t)}")
        return cls(t, _mean(t[1], t[0]), _mean(t[3], t[2]), _mean(t[5], t[4]), _mean(cls._ratio_sum(t, 0), t[6]),
                   _mean(cls._ratio_sum(t, 1), t[9]))

    def as_printed_by_reference(self) -> Dict[str, float]:
        """The five printed figures.  The script's np.nanmean runs over lists of (value, count) TUPLES for the answer and the
        question words, so both columns enter the mean: a hit contributes 1 + 1 over two entries, a miss 0 + 0 over two, a NaN
        question its count 0 over one; the text figure is a list of scalars and stays the plain mean."""
        t = self.totals
        return {"Accuracy": self.accuracy, "Accuracy AT": self.accuracy_at, "Ans. Tok. Coo": _mean(2 * t[5], t[4] + t[1]),
                "Qst. Tok. Coo": _mean(self._ratio_sum(t, 0) + t[7], t[6] + t[1]), "Qst. Text Tok. Coo": self.text_tok_coo}


class EvalBatch(NamedTuple):
    inputs: object                     # synthetic.FullWorkload (or any object with its fields and scene_graphs()), or a Workload
    label: Tensor                      # int64 [B], on the device
    qtok: Optional[Tensor] = None      # TokenTables.question_words(...) on the device
    qflags: Optional[Tensor] = None
    names: Optional[Tensor] = None     # int64 [N] name ids; default inputs.x[:, 0]
    graph_index: Optional[Tensor] = None   # int64 [Q]: `inputs` holds G DISTINCT graphs and Q question rows; question q asks about
                                           # graph graph_index[q] (ISubGVQA.encode_scene / ask; the full model only)


_EvalBatchFields = EvalBatch


class EvalBatch(_EvalBatchFields):         # noqa: F811 -- the tuple above, with two keywords beside its fields
    """The batch of evaluate().  `groups` (int32 [B, F]: QuestionTypes.encode(...) of the questions, for evaluate(types=...)) and
    `gold` (int32 [B, F, M]: ObjectAnnotations.encode(...), for evaluate(grounding=True)) are keywords and attributes, not further
    tuple fields: the tuple's fields, their order and `_fields` stay what callers unpack."""
    groups: Optional[Tensor] = None
    gold: Optional[Tensor] = None

    def __new__(cls, *args, groups: Optional[Tensor] = None, gold: Optional[Tensor] = None, **kw):
        self = super().__new__(cls, *args, **kw)
        self.groups = groups
        self.gold = gold
        return self

    def _replace(self, **kw):
        groups = kw.pop("groups", self.groups)
        gold = kw.pop("gold", self.gold)
        out = super()._replace(**kw)
        out.groups = groups
        out.gold = gold
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Grounding in GQA's object annotations
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GroundingFigures:
    """One set of annotated objects (a facet, or the union `any`) over one population of questions; NaN where the denominator is 0."""
    questions: int             # questions whose set holds at least one object of the graph
    precision: float           # picked nodes that are annotated objects: sum hits / sum |P|  (micro)
    recall: float              # annotated objects that were picked: sum hits / sum |G|  (micro)
    macro_recall: float        # mean over the questions of hits / |G|
    f1: float                  # of the two micro figures
    pointing: float            # questions with at least one annotated object picked
    full_recall: float         # questions with every annotated object picked
    chance: float              # sum |P| / sum n_g: the recall of a random subset of the same size


@dataclass(frozen=True)
class GroundingReport:
    """isg_grounding's running totals (one row of them) as figures: sets[name][population], name in `question`, `answer`,
    `fullAnswer` (the facets given) and `any` (their union), population `all` or `correct`."""
    totals: Tuple[int, ...]
    questions: int
    correct: int
    unresolved: int            # annotated objects that are no node of their graph (entries -2)
    bad: int                   # entries that are neither a pad, nor unresolved, nor a node index of the graph
    sets: Dict[str, Dict[str, GroundingFigures]] = field(default_factory=dict, compare=False)
    by_type: Optional[Dict[str, Dict[str, "GroundingReport"]]] = field(default=None, compare=False)

    @staticmethod
    def _figures(blk: Sequence[int]) -> GroundingFigures:
        H = ops.GROUND_HIST
        q, kept, nodes, gold, hits, some, every = blk[:7]
        macro = math.fsum(map(operator.truediv, blk[9 + H:8 + 2 * H], range(1, H)))      # sum over m >= 1 of hits[m] / m: exact terms, exact sum
        p, r = _mean(hits, kept), _mean(hits, gold)
        f1 = float("nan") if p != p or r != r else (2 * p * r / (p + r) if p + r else 0.0)
        return GroundingFigures(q, p, r, _mean(macro, q), f1, _mean(some, q), _mean(every, q), _mean(kept, nodes))

    @classmethod
    def from_totals(cls, totals, facets: Sequence[str] = ("question", "answer", "fullAnswer")) -> "GroundingReport":
        t = tuple(totals.tolist()) if torch.is_tensor(totals) else tuple(int(v) for v in totals)
        if len(t) != ops.GROUND_TOTALS:
            raise ValueError(f"totals: expected {ops.GROUND_TOTALS} entries, got {len(t)}")
        if not 1 <= len(facets) <= ops.GROUND_FACETS:
            raise ValueError(f"facets: 1 to {ops.GROUND_FACETS}, got {len(facets)}")
        names = {s: f for s, f in enumerate(facets)}
        names[ops.GROUND_SETS - 1] = "any"
        sets = {}
        for s, name in names.items():
            at = lambda c: t[ops.GROUND_HEAD + (2 * s + c) * ops.GROUND_BLOCK:ops.GROUND_HEAD + (2 * s + c + 1) * ops.GROUND_BLOCK]
            sets[name] = {"all": cls._figures(at(0)), "correct": cls._figures(at(1))}
        return cls(t, t[0], t[1], t[2], t[3], sets)


def evaluate(model, batches: Iterable[EvalBatch], tables: TokenTables, threshold: float = 0.0, types=None,
             grounding: bool = False) -> CooReport:
    """run_token_coo.py's experiment over whole batches: forward, argmax, ops.token_coo into ONE running totals tensor; nothing is
    copied to the host before the last batch has been queued.  With --text_sampling the forward's token mask is scored against
    tables.clip_sg.
    types (a datasets.gqa.QuestionTypes; every batch then carries `groups`): the report also has by_type, {facet: {name: CooReport}}
    of the questions of every group (ops.token_coo_groups, one launch more per batch).  The overall totals and the [G, COO_TOTALS]
    table are ONE tensor: the evaluation stays one device-to-host copy.
    grounding (every batch then carries `gold`, ObjectAnnotations.encode of its questions): the report also has .grounding, a
    GroundingReport of ops.grounding over the same masks and predictions (two launches more per batch), with by_type when types
    is given.  Its totals lie behind the co-occurrence totals in the SAME int64 buffer: still one device-to-host copy."""
    full = not isinstance(model, synthetic.AnswerModel)
    G = 0 if types is None else int(types.num_groups)
    if types is not None and not 1 <= G <= ops.EVAL_GROUPS_MAX:
        raise ValueError(f"evaluate: {G} groups (1 to {ops.EVAL_GROUPS_MAX})")
    n_coo = (1 + G) * ops.COO_TOTALS
    words = n_coo + ((1 + G) * ops.GROUND_TOTALS if grounding else 0)
    flat = both = ground = None
    with torch.no_grad():
        for b in batches:
            inp = b.inputs
            B = int(inp.questions.size(0) if full else inp.glf.size(0))
            names = inp.x[:, 0] if b.names is None else b.names
            if b.graph_index is not None:           # many questions per graph: encode once, score the instances' names
                if not full:
                    raise ValueError("EvalBatch.graph_index: the full model only (an AnswerModel has no encoder to share)")
                state = model.encode_scene(inp.x, inp.edge_index, inp.edge_attr, inp.batch, inp.scene_graphs())
                out, inst = model.ask(state, inp.questions, inp.att_mask, b.graph_index)
                plan, names = inst.plan(), inst.gather_nodes(names).contiguous()
            else:
                plan = _input_plan(inp, B)
                if full:
                    out = model(inp.x, inp.edge_index, inp.edge_attr, inp.batch, inp.questions, inp.att_mask, return_masks=True,
                                scene_graphs=inp.scene_graphs(), plan=plan)
                else:
                    out = model(inp, plan=plan)
            logits, mask = out[0], out[1]
            mask_text = out[4] if full and len(out) > 4 else None
            if flat is None:                        # one buffer, one copy: [1 + G, COO_TOTALS], with grounding then [1 + G, GROUND_TOTALS]
                flat = torch.zeros(words, dtype=torch.int64, device=logits.device)
                both = flat[:n_coo].view(1 + G, ops.COO_TOTALS)
                ground = flat[n_coo:].view(1 + G, ops.GROUND_TOTALS) if grounding else None
            ttok = tkeep = None
            if mask_text is not None:
                ttok = tables.text_tokens(inp.questions)
                tkeep = mask_text.reshape(B, -1).float().contiguous()
            pred = logits.argmax(dim=1)
            coo = ops.token_coo(names, mask, plan, pred, b.label,
                                tables.on("ans_sg", logits.device), b.qtok, b.qflags, ttok, tkeep, threshold=threshold, totals=both[0])
            groups = None
            if types is not None:
                groups = getattr(b, "groups", None)
                if groups is None:
                    raise ValueError("evaluate(types=...): every EvalBatch carries groups (QuestionTypes.encode)")
                groups = groups.to(logits.device, non_blocking=True)
                ops.token_coo_groups(coo.table, b.qflags, groups, both[1:])
            if grounding:
                gold = getattr(b, "gold", None)
                if gold is None:
                    raise ValueError("evaluate(grounding=True): every EvalBatch carries gold (ObjectAnnotations.encode)")
                ops.grounding(mask, plan, gold.to(logits.device, non_blocking=True), pred, b.label, groups, G, threshold=threshold,
                              totals=ground)
    if flat is None:                                         # no batch: the same report from zeros on the host
        flat = torch.zeros(words, dtype=torch.int64)
    host = flat.cpu()                                        # every table, overall and every group: the one device-to-host copy
    tables_h = [(CooReport, host[:n_coo].view(1 + G, ops.COO_TOTALS).tolist())]
    if grounding:                                            # (rows stay tensors: from_totals turns each into ints in one call)
        tables_h.append((GroundingReport, host[n_coo:].view(1 + G, ops.GROUND_TOTALS)))
    reports = []
    for cls, rows in tables_h:                               # row 0: overall; row 1 + g: group g
        report = cls.from_totals(rows[0])
        if types is not None:
            by_type = {f: {} for f in types.facets}
            for g, (facet, name) in enumerate(types.group_names):
                by_type[facet][name] = cls.from_totals(rows[1 + g])
            report = replace(report, by_type=by_type)
        reports.append(report)
    return replace(reports[0], grounding=reports[1]) if grounding else reports[0]


# ---------------------------------------------------------------------------------------------------------------------
# Fidelity curves: the answer's probability along a node ranking, kept or removed
# ---------------------------------------------------------------------------------------------------------------------
CURVE_FRACTIONS = (0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0)
CURVE_RULES = ("trapezoid", "mean")


def curve_weights(x: Sequence[float], rule: str = "trapezoid") -> Tensor:
    """float64 [L]: quadrature weights over the level axis x (non-decreasing; for fractions the fractions, for counts the counts
    divided by their largest).  trapezoid: w_0 = (x_1 - x_0) / 2, w_j = (x_{j+1} - x_{j-1}) / 2, w_{L-1} = (x_{L-1} - x_{L-2}) / 2
    -- the area under the polygon through the curve's points, x_{L-1} - x_0 for a curve that is 1 everywhere; a single level has
    the weight 1 (the curve's one value).  mean: 1 / L each.  Formed in double; ops.curve_sums takes them rounded to fp32 once."""
    xs = torch.tensor([float(v) for v in x], dtype=torch.float64)
    L = xs.numel()
    if L == 0 or bool(torch.isnan(xs).any()) or bool((xs[1:] < xs[:-1]).any()):
        raise ValueError(f"curve_weights: a non-empty, non-decreasing level axis, got {list(x)}")
    if rule == "mean":
        return torch.full((L,), 1.0 / L, dtype=torch.float64)
    if rule != "trapezoid":
        raise ValueError(f"curve_weights: rule from {CURVE_RULES}, got {rule!r}")
    if L == 1:
        return torch.ones(1, dtype=torch.float64)
    w = torch.zeros(L, dtype=torch.float64)
    w[0], w[-1] = (xs[1] - xs[0]) / 2, (xs[-1] - xs[-2]) / 2
    w[1:-1] = (xs[2:] - xs[:-2]) / 2
    return w


def _curve_levels(fractions, counts):
    """(fractions or None, counts or None, the level axis x) of fidelity_curves' two keywords."""
    if counts is None:
        if fractions is None:
            raise ValueError("fidelity_curves: fractions or counts")
        fr = tuple(float(f) for f in fractions)
        return fr, None, fr
    if fractions is not None and tuple(fractions) != CURVE_FRACTIONS:
        raise ValueError("fidelity_curves: fractions or counts, not both")
    cn = tuple(operator.index(c) for c in counts)
    top = max(cn) if cn else 0
    return None, cn, tuple(c / top if top else 0.0 for c in cn)


@dataclass
class FidelityCurves:
    """Deletion and insertion curves of one batch along one node ranking (fidelity_curves())."""
    pred: Tensor                   # int64 [B]: the class predicted on the whole graph
    p: Tensor                      # fp32 [B]: its softmax probability on the whole graph
    rank: Tensor                   # int32 [N]: every node's rank inside its graph, 0 = the most important (ops.curve_keep_bits)
    level_k: Tensor                # int32 [B, L, S]: the nodes ranked into (keep) or out of (remove) every instance; 0 for graphs without nodes
    p_keep: Optional[Tensor]       # fp32 [B, L]: that class's probability on the level's top-ranked nodes ALONE; NaN for graphs without nodes
    p_remove: Optional[Tensor]     # fp32 [B, L]: ... with the level's top-ranked nodes REMOVED
    auc_keep: Optional[Tensor]     # fp32 [B]: the area under p_keep over the level axis (the weights of curve_weights); NaN where skipped
    auc_remove: Optional[Tensor]   # fp32 [B]
    totals: Tensor                 # float64 [S, L + 3] on the device: per side the L level sums, the sum of the areas, graphs counted, skipped
    weights: Optional[Tensor] = None           # float64 [L] on the host: the quadrature weights
    bits: Optional["ops.CurveBits"] = None     # the ranking's keep rows
    chunks: List["ops.InducedInstances"] = field(default_factory=list)      # the instance batches that were forwarded, in order


def fidelity_curves(model, inputs, scores: Tensor, *, fractions=CURVE_FRACTIONS, counts=None, sides=ops.CURVE_SIDES,
                    noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None, max_instances: Optional[int] = None,
                    logits: Optional[Tensor] = None, plan: Optional["ops.GraphPlan"] = None, totals: Optional[Tensor] = None,
                    rule: str = "trapezoid") -> FidelityCurves:
    """The predicted answer's probability as the top-ranked nodes of `scores` (fp32 [N] or [N, 1], higher = more important; any
    explainer's .scores()) are kept alone (p_keep: an insertion curve) or removed (p_remove: a deletion curve), at every level of
    `fractions` (shares of a graph's nodes, ceil(fp32(f) * fp32(n))) or `counts` (numbers of nodes), with the area under each
    curve.  One forward on the batch for `pred` and `p` (or `logits`, with the `plan` of that forward); ONE launch for the
    ranking and all keep rows (ops.curve_keep_bits); the batch of 2 B L instances cut and forwarded exactly as occlusion() does it
    (ops.induced_instances, instance_inputs, question rows through the index, noises by graph, chunks of at most max_instances);
    ONE launch for the areas and the running totals (ops.curve_sums; `totals` float64 [S, L + 3] is accumulated into).

    Ties go to the lower node and a level holds EXACTLY its k nodes (an explainer's .mask(k) keeps every tie at the k-th value).
    The keep side never has fewer than 1 node and the remove side never removes the last one, so the model sees no empty graph:
    at fraction 0 the keep curve is the best single node, at fraction 1 the remove curve leaves the worst single node.  Graphs
    without nodes have NaN rows and are not counted.  The model must be in eval(); the call runs under torch.no_grad().  A result
    depends on the composition of its instance batch (quirks Q1 / Q3 / Q4): curves from different max_instances may differ in
    the last bits."""
    _refuse_training(model, "fidelity_curves scores", "the answer from instance to instance")
    _refuse_max_instances(max_instances)
    fr, cn, x = _curve_levels(fractions, counts)
    weights = curve_weights(x, rule)
    whole = _whole_batch(model, inputs, noises, seed, logits, plan)
    with torch.no_grad():
        pred, p = whole.predicted()
        bits = ops.curve_keep_bits(scores.detach().float().reshape(-1).contiguous(), whole.plan, fractions=fr, counts=cn, sides=sides)
        p_inst, chunks = _instance_probabilities(whole, inputs, bits.index, bits.keep, pred, p, noises, max_instances)
        auc, totals = ops.curve_sums(p_inst, bits, weights.float().to(p.device), totals)
        B, R, L, S = whole.B, bits.R, bits.L, bits.S
        listed = bits.graphs.long()
        nan = float("nan")
        per_side = p_inst.view(R, L, S)
        level_k = torch.zeros(B, L, S, dtype=torch.int32, device=p.device).index_copy_(0, listed, bits.level_k)
        curves, areas = {}, {}
        for s, name in enumerate(n for b, n in enumerate(ops.CURVE_SIDES) if bits.sides >> b & 1):
            curves[name] = torch.full((B, L), nan, dtype=torch.float32, device=p.device).index_copy_(0, listed, per_side[:, :, s].contiguous())
            areas[name] = torch.full((B,), nan, dtype=torch.float32, device=p.device).index_copy_(0, listed, auc[:, s].contiguous())
    return FidelityCurves(pred, p, bits.rank, level_k, curves.get("keep"), curves.get("remove"), areas.get("keep"),
                          areas.get("remove"), totals, weights, bits, chunks)


@dataclass(frozen=True)
class CurveReport:
    """One explainer's fidelity curves over an evaluation (compare(curves=...)): means over the graphs that were counted (those
    with nodes and finite probabilities at every level of the side); NaN where none was."""
    fractions: Tuple[float, ...]             # the level axis
    p_keep: Tuple[float, ...]                # per level: the mean probability of the predicted answer on the top-ranked nodes alone
    p_remove: Tuple[float, ...]              # per level: ... with the top-ranked nodes removed
    auc_keep: float                          # the mean area under a graph's keep curve (curve_weights' trapezoid rule)
    auc_remove: float
    counted: Tuple[int, int]                 # graphs counted on the keep side, on the remove side
    skipped: Tuple[int, int]                 # graphs skipped for a non-finite probability
    sums: Tuple[Tuple[float, ...], ...] = ()         # the two rows of L + 3 totals behind the means

    @classmethod
    def from_totals(cls, fractions, rows) -> "CurveReport":
        L = len(fractions)
        keep, remove = (tuple(float(v) for v in r) for r in rows)
        return cls(tuple(float(f) for f in fractions), tuple(_mean(v, keep[L + 1]) for v in keep[:L]),
                   tuple(_mean(v, remove[L + 1]) for v in remove[:L]), _mean(keep[L], keep[L + 1]), _mean(remove[L], remove[L + 1]),
                   (int(keep[L + 1]), int(remove[L + 1])), (int(keep[L + 2]), int(remove[L + 2])), (keep, remove))


# ---------------------------------------------------------------------------------------------------------------------
# A sampled baseline: Shapley values by permutation sampling
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class ShapleyValues(_Ranked):
    """Shapley estimates of one batch by permutation sampling (shapley_values())."""
    pred: Tensor                   # int64 [B]: the class predicted on the whole graph
    p: Tensor                      # fp32 [B]: its softmax probability on the whole graph
    attribution: Tensor            # fp32 [N]: the mean marginal contribution of every node over the permutations (phi); NaN in flagged graphs
    m2: Tensor                     # fp32 [N]: the sum of the squared samples (for stderr())
    gap: Tensor                    # fp32 [B]: sum of a graph's attributions - (p - v_empty), the completeness gap; NaN in flagged graphs
    flag: Tensor                   # int32 [B]: 0 fine, 1 a non-finite probability among the graph's instances or its p
    single: Tensor                 # bool [B]: fewer than 2 nodes -- no instance; a lone node's attribution is p - v_empty
    bits: "ops.ShapleyBits"        # the permutations (pos) and their prefixes' keep rows
    p_inst: Tensor                 # fp32 [Q]: the predicted class's probability on every instance
    logits: Tensor                 # [B, classes] of the whole batch
    plan: "ops.GraphPlan"
    chunks: List["ops.InducedInstances"] = field(default_factory=list)      # the instance batches that were forwarded, in order

    @property
    def T(self) -> int:
        """Samples behind every estimate: the permutations, or their antithetic pairs."""
        return self.bits.T

    def stderr(self) -> Tensor:
        """float64 [N]: the standard error of every estimate, sqrt(max(m2 - T phi^2, 0) / (T (T - 1))); NaN for T = 1."""
        T = self.T
        if T < 2:
            return torch.full_like(self.attribution, float("nan"), dtype=torch.float64)
        phi, m2 = self.attribution.double(), self.m2.double()
        return torch.sqrt((m2 - T * phi * phi).clamp_min(0.0) / (T * (T - 1)))


def shapley_values(model, inputs, *, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None, permutations: int = 16,
                   antithetic: bool = True, perm_seed: int = 0, v_empty: float = 0.0, max_instances: Optional[int] = None,
                   logits: Optional[Tensor] = None, plan: Optional["ops.GraphPlan"] = None) -> ShapleyValues:
    """Shapley values of every node by permutation sampling (Castro et al. 2009; Strumbelj and Kononenko 2014): the mean, over
    `permutations` random orders of a graph's nodes, of the change of the predicted answer's probability when the node joins the
    nodes before it -- the axiomatic reference point of the post-hoc baselines, of which occlusion() is the one-term truncation
    (the marginal contribution at the full set alone).  One forward on the batch for `pred` and `p` (or `logits`, with the `plan`
    of that forward); ONE launch for the seeded permutations and the keep rows of all their prefixes (ops.shapley_keep_bits:
    permutations * (n - 1) instances per graph of n nodes); the instances cut and forwarded exactly as occlusion() does it
    (ops.induced_instances, instance_inputs, question rows through the index, noises by graph, chunks of at most max_instances);
    ONE launch for the estimates (ops.shapley_values).

    The value of the full set is p (not forwarded again), the value of the empty set is `v_empty` (the model never sees an empty
    graph); with v_empty = 0 a graph's attributions sum to p, and `gap` says how nearly.  antithetic: every other permutation is
    the one before it reversed (variance reduction; permutations is even).  perm_seed seeds the permutations alone (a graph's
    depend on it and on the graph's number in the batch); `seed` and `noises` are the sampler's, as in occlusion().  The model
    must be in eval(); the call runs under torch.no_grad().  A result depends on the composition of its instance batch (quirks
    Q1 / Q3 / Q4): estimates from different max_instances may differ in the last bits, the permutations never do."""
    _refuse_training(model, "shapley_values scores", "the answer from instance to instance")
    _refuse_max_instances(max_instances)
    whole = _whole_batch(model, inputs, noises, seed, logits, plan)
    plan = whole.plan
    with torch.no_grad():
        pred, p = whole.predicted()
        bits = ops.shapley_keep_bits(plan, permutations=permutations, antithetic=antithetic, seed=perm_seed)
        p_inst, chunks = _instance_probabilities(whole, inputs, bits.index, bits.keep, pred, p, noises, max_instances)
        phi, m2, gap, flag = ops.shapley_values(p_inst, p.contiguous(), bits, plan, v_empty=v_empty)
        single = (plan.ptr[1:] - plan.ptr[:-1]) < 2
    return ShapleyValues(pred, p, phi, m2, gap, flag, single, bits, p_inst, whole.logits, plan, chunks)


# ---------------------------------------------------------------------------------------------------------------------
# The intrinsic mask beside post-hoc baselines
# ---------------------------------------------------------------------------------------------------------------------
EXPLAINERS = ("intrinsic", "occlusion", "random")
EXPLAINERS_ALL = EXPLAINERS + ("attention",)       # what compare() accepts beside the gradient explainers; EXPLAINERS stays its default
EXPLAINERS_GRADIENT = ("integrated_gradients", "grad_x_input")      # compare() accepts these too (integrated_gradients())
EXPLAINERS_LEARNED = ("mask_optimization",)                         # ... and this one (mask_optimization(): GNNExplainer)
EXPLAINERS_SAMPLED = ("shapley",)                                   # ... and this one (shapley_values(): permutation sampling)
COMPARE_SUMS = 6       # float64 per explainer: sum fid_plus, questions that have one, sum fid_minus, questions that have one,
                       # sum of the Jaccard overlaps with the intrinsic mask, graphs that have one


@dataclass(frozen=True)
class ExplainerReport:
    """One explainer's masks over an evaluation (compare()); NaN where no question has the quantity."""
    coo: CooReport                           # token co-occurrence of its masks (the model's predictions are the same for all)
    grounding: Optional[GroundingReport]     # against the annotated objects, when every batch carried `gold`
    fid_plus: float                          # mean over the questions that have one (faithfulness_of_mask)
    fid_minus: float
    jaccard: float                           # mean over the graphs of |mask & intrinsic| / |mask | intrinsic| (graphs where both are empty: none)
    sums: Tuple[float, ...]                  # the COMPARE_SUMS totals behind the three means
    curves: Optional[CurveReport] = None     # its fidelity curves, when compare() was given `curves`


def random_scores(plan: "ops.GraphPlan", seed: int) -> Tensor:
    """fp32 [N, 1]: the seeded noise random_mask ranks (uniform in [1, 2), so no zero pad is picked) -- the random explainer's
    scores for a fidelity curve."""
    gen = torch.Generator(device=plan.ptr.device).manual_seed(int(seed))
    return 1.0 + torch.rand(plan.N, 1, generator=gen, device=plan.ptr.device)


def random_mask(plan: "ops.GraphPlan", k, seed: int) -> Tensor:
    """fp32 [N, 1], k-hot per graph: ops.topk_threshold on seeded noise alone (random_scores)."""
    return ops.topk_threshold(random_scores(plan, seed), k, plan=plan)


def jaccard_sums(mask: Tensor, other: Tensor, batch: Tensor, B: int, threshold: float = 0.0) -> Tensor:
    """float64 [2] on the device: (sum over the graphs of |a & b| / |a | b|, graphs where a | b is not empty)."""
    a, b = mask.reshape(-1) > threshold, other.reshape(-1) > threshold
    z = torch.zeros(B, dtype=torch.float64, device=batch.device)
    inter, union = z.index_add(0, batch, (a & b).double()), z.index_add(0, batch, (a | b).double())
    some = union > 0
    return torch.stack([torch.where(some, inter / union.clamp_min(1.0), torch.zeros_like(z)).sum(), some.double().sum()])


def fidelity_sums(f: Fidelity) -> Tensor:
    """float64 [4] on the device: (sum of fid_plus, questions that have one, sum of fid_minus, questions that have one)."""
    has_p, has_m = ~torch.isnan(f.fid_plus), ~torch.isnan(f.fid_minus)
    return torch.stack([torch.where(has_p, f.fid_plus, torch.zeros_like(f.fid_plus)).double().sum(), has_p.double().sum(),
                        torch.where(has_m, f.fid_minus, torch.zeros_like(f.fid_minus)).double().sum(), has_m.double().sum()])


# name -> (model, inp, ctx) -> a result object (a _Ranked: compare() asks it for mask(k) and, for a curve, scores()), in the order
# compare() names them when it refuses one.  ctx, per batch: compare()'s k, max_instances, ig_steps, mo_steps and sv_permutations,
# seed (its seed + the batch's number), and logits, plan and intrinsic (the node mask) of the batch forward it makes once.
# intrinsic and random have no result object: they give the pair (mask, a function that returns the scores -- random's cost a
# launch, which only a curve pays).  A new explainer joins compare() by one entry.  Only shapley takes compare()'s batch forward;
# the others forward the batch themselves (the follow-up).
_COMPARE = {
    "intrinsic": lambda model, inp, c: (c.intrinsic, lambda: c.intrinsic),
    "occlusion": lambda model, inp, c: occlusion(model, inp, max_instances=c.max_instances),
    "random": lambda model, inp, c: (random_mask(c.plan, c.k, c.seed), lambda: random_scores(c.plan, c.seed)),
    "attention": lambda model, inp, c: attention_rollout(model, inp),
    "integrated_gradients": lambda model, inp, c: integrated_gradients(model, inp, steps=c.ig_steps, max_instances=c.max_instances),
    "grad_x_input": lambda model, inp, c: integrated_gradients(model, inp, steps=1, rule="endpoint", max_instances=c.max_instances),
    "mask_optimization": lambda model, inp, c: mask_optimization(model, inp, steps=c.mo_steps, init_seed=c.seed),
    "shapley": lambda model, inp, c: shapley_values(model, inp, permutations=c.sv_permutations, perm_seed=c.seed,
                                                    max_instances=c.max_instances, logits=c.logits, plan=c.plan),
}
assert tuple(_COMPARE) == EXPLAINERS_ALL + EXPLAINERS_GRADIENT + EXPLAINERS_LEARNED + EXPLAINERS_SAMPLED      # the public name tuples


def _compare_totals(flat: Tensor, X: int, L: int):
    """The four views of compare()'s totals buffer (int64 [X * (COO_TOTALS + GROUND_TOTALS + COMPARE_SUMS + 2 (L + 3))], with no
    curve words when L = 0), on the device and on the host alike: coo int64 [X, COO_TOTALS], ground int64 [X, GROUND_TOTALS], sums
    float64 [X, COMPARE_SUMS] in int64 words, curves float64 [X, 2, L + 3] (both sides' ops.curve_sums totals) or None."""
    a = X * ops.COO_TOTALS
    b = a + X * ops.GROUND_TOTALS
    c = b + X * COMPARE_SUMS
    return (flat[:a].view(X, ops.COO_TOTALS), flat[a:b].view(X, ops.GROUND_TOTALS), flat[b:c].view(torch.float64).view(X, COMPARE_SUMS),
            flat[c:].view(torch.float64).view(X, 2, L + 3) if L else None)


def compare(model, batches: Iterable[EvalBatch], tables: TokenTables, explainers: Sequence[str] = EXPLAINERS, k: int = 5,
            threshold: float = 0.0, seed: int = 0, max_instances: Optional[int] = None, ig_steps: int = 16,
            mo_steps: int = 100, sv_permutations: int = 16, curves: Optional[Sequence[float]] = None) -> Dict[str, ExplainerReport]:
    """The model's intrinsic mask beside post-hoc baselines, each measured by the same yardsticks over whole batches: per
    explainer the CooReport figures (ops.token_coo), the GroundingReport where every batch carries `gold` (ops.grounding), the
    mean fid_plus / fid_minus (faithfulness_of_mask) and the mean Jaccard overlap with the intrinsic mask.
    intrinsic: the forward's own mask; occlusion: occlusion().mask(k); random: random_mask(plan, k, seed + batch number);
    attention (not among the default): attention_rollout().mask(k); integrated_gradients and grad_x_input (EXPLAINERS_GRADIENT,
    not among the default): integrated_gradients(steps=ig_steps).mask(k) and its one-point case (steps=1, rule="endpoint") --
    autograd records inside those calls only; mask_optimization (EXPLAINERS_LEARNED, not among the default):
    mask_optimization(steps=mo_steps, init_seed=seed + batch number).mask(k), GNNExplainer with PyG's defaults; shapley
    (EXPLAINERS_SAMPLED, not among the default): shapley_values(permutations=sv_permutations, perm_seed=seed + batch
    number).mask(k), antithetic permutation sampling with v_empty = 0.
    Every total stays on the device, in ONE buffer: the evaluation is one device-to-host copy at the end, as in evaluate().
    curves: a tuple of fractions (CURVE_FRACTIONS, say) -- every explainer's ranking is also scored along the whole curve
    (fidelity_curves on its .scores(); random: its seeded noise; intrinsic: the k-hot mask itself, so the picked nodes come first
    and the rest fall to node order -- its curve says something at the level of k nodes only) and every report carries a
    CurveReport; the curve totals ride in the same buffer.  None: no curve is computed and `curves` of every report is None."""
    names_x = tuple(explainers)
    levels = None if curves is None else tuple(float(f) for f in curves)
    if levels is not None:
        curve_weights(levels)                                # (refuses an empty or decreasing axis before any forward)
    L = 0 if levels is None else len(levels)
    known = tuple(_COMPARE)
    unknown = [x for x in names_x if x not in known]
    if unknown or not names_x:
        raise ValueError(f"compare: explainers from {known}, got {names_x}")
    X = len(names_x)
    words = X * (ops.COO_TOTALS + ops.GROUND_TOTALS + COMPARE_SUMS + (2 * (L + 3) if L else 0))   # int64; the sums are float64 in theirs
    flat = with_gold = None
    with torch.no_grad():
        for number, b in enumerate(batches):
            inp = b.inputs
            if b.graph_index is not None:
                raise ValueError("compare: one graph per question (occlusion on shared encodings would leave the removed node "
                                 "seen by the encoder)")
            _, B, _, plan, _, logits, intrinsic = _whole_batch(model, inp, None, None)
            gold = getattr(b, "gold", None)
            if with_gold is None:
                with_gold = gold is not None
                flat = torch.zeros(words, dtype=torch.int64, device=logits.device)
                coo, ground, sums, ctot = _compare_totals(flat, X, L)
            elif with_gold != (gold is not None):
                raise ValueError("compare: every EvalBatch carries gold, or none does")
            names = inp.x[:, 0] if b.names is None else b.names
            pred = logits.argmax(dim=1)
            ctx = argparse.Namespace(k=k, seed=seed + number, max_instances=max_instances, ig_steps=ig_steps, mo_steps=mo_steps,
                                     sv_permutations=sv_permutations, logits=logits, plan=plan, intrinsic=intrinsic)
            for x, name in enumerate(names_x):
                res = _COMPARE[name](model, inp, ctx)
                mask, ranked = res if isinstance(res, tuple) else (res.mask(k), res.scores)
                if L:
                    fidelity_curves(model, inp, ranked(), fractions=levels, max_instances=max_instances, logits=logits, plan=plan,
                                    totals=ctot[x])
                ops.token_coo(names, mask, plan, pred, b.label, tables.on("ans_sg", logits.device), b.qtok, b.qflags, None, None,
                              threshold=threshold, totals=coo[x])
                if with_gold:
                    ops.grounding(mask, plan, gold.to(logits.device, non_blocking=True), pred, b.label, threshold=threshold,
                                  totals=ground[x])
                f = faithfulness_of_mask(model, inp, mask, threshold=threshold, logits=logits, plan=plan).scores
                sums[x] += torch.cat([fidelity_sums(f), jaccard_sums(mask, intrinsic, inp.batch, B, threshold)])
    if flat is None:
        flat, with_gold = torch.zeros(words, dtype=torch.int64), False
    coo, ground, sums, ctot = _compare_totals(flat.cpu(), X, L)          # every explainer's totals: the one device-to-host copy
    coo, sums = coo.tolist(), sums.tolist()
    out = {}
    for x, name in enumerate(names_x):
        s = tuple(float(v) for v in sums[x])
        out[name] = ExplainerReport(CooReport.from_totals(coo[x]), GroundingReport.from_totals(ground[x]) if with_gold else None,
                                    _mean(s[0], s[1]), _mean(s[2], s[3]), _mean(s[4], s[5]), s,
                                    CurveReport.from_totals(levels, ctot[x].tolist()) if L else None)
    return out
