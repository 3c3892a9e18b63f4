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
"""
from __future__ import annotations

import argparse
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
    totals = flat = ground = None
    G = 0 if types is None else int(types.num_groups)
    if types is not None and not 1 <= G <= ops.EVAL_GROUPS_MAX:
        raise ValueError(f"evaluate: {G} groups (1 to {ops.EVAL_GROUPS_MAX})")
    both = None
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
                plan = ops.GraphPlan.build(inp.batch, inp.edge_index, num_graphs=B, max_nodes=inp.max_nodes or None,
                                           max_edges=inp.max_edges or None, graph_sizes=inp.graph_sizes)
                if full:
                    out = model(inp.x, inp.edge_index, inp.edge_attr, inp.batch, inp.questions, inp.att_mask, return_masks=True,
                                scene_graphs=inp.scene_graphs(), plan=plan)
                else:
                    out = model(inp, plan=plan)
            logits, mask = out[0], out[1]
            mask_text = out[4] if full and len(out) > 4 else None
            if totals is None:
                if grounding:                       # one buffer, one copy: [1 + G, COO_TOTALS] then [1 + G, GROUND_TOTALS]
                    flat = torch.zeros((1 + G) * (ops.COO_TOTALS + ops.GROUND_TOTALS), dtype=torch.int64, device=logits.device)
                    both = flat[:(1 + G) * ops.COO_TOTALS].view(1 + G, ops.COO_TOTALS)
                    ground = flat[(1 + G) * ops.COO_TOTALS:].view(1 + G, ops.GROUND_TOTALS)
                else:
                    both = torch.zeros(1 + G, ops.COO_TOTALS, dtype=torch.int64, device=logits.device)
                totals = both[0]
            ttok = tkeep = None
            if mask_text is not None:
                ttok = tables.text_tokens(inp.questions)
                tkeep = mask_text.reshape(B, -1).float().contiguous()
            pred = logits.argmax(dim=1)
            coo = ops.token_coo(names, mask, plan, pred, b.label,
                                tables.on("ans_sg", logits.device), b.qtok, b.qflags, ttok, tkeep, threshold=threshold, totals=totals)
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
    if both is None:
        flat = torch.zeros((1 + G) * (ops.COO_TOTALS + (ops.GROUND_TOTALS if grounding else 0)), dtype=torch.int64)
        both = flat[:(1 + G) * ops.COO_TOTALS].view(1 + G, ops.COO_TOTALS)
    if types is None and not grounding:
        return CooReport.from_totals(both[0])
    if not grounding:
        rows = both.tolist()                                 # overall and every group: the evaluation's one device-to-host copy
        by_type = {f: {} for f in types.facets}
        for g, (facet, name) in enumerate(types.group_names):
            by_type[facet][name] = CooReport.from_totals(rows[1 + g])
        return replace(CooReport.from_totals(rows[0]), by_type=by_type)
    host = flat.cpu()                                        # both tables, overall and every group: the one device-to-host copy
    n_coo = (1 + G) * ops.COO_TOTALS
    rows = host[:n_coo].view(1 + G, ops.COO_TOTALS).tolist()
    grows = host[n_coo:].view(1 + G, ops.GROUND_TOTALS)     # rows stay tensors: from_totals turns each into ints in one call
    report, ground_report = CooReport.from_totals(rows[0]), GroundingReport.from_totals(grows[0])
    if types is not None:
        by_type, ground_by_type = {f: {} for f in types.facets}, {f: {} for f in types.facets}
        for g, (facet, name) in enumerate(types.group_names):
            by_type[facet][name] = CooReport.from_totals(rows[1 + g])
            ground_by_type[facet][name] = GroundingReport.from_totals(grows[1 + g])
        report = replace(report, by_type=by_type)
        ground_report = replace(ground_report, by_type=ground_by_type)
    return replace(report, grounding=ground_report)
