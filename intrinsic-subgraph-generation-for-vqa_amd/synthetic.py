"""Synthetic GQA-shaped scene-graph batches and the BASELINE.json workload configurations.

There is no GQA data in either container, so every measurement and most parity tests
run on seeded synthetic batches with the layout `gqa_collate` produces (datasets/gqa.py:237-272;
datasets/scene_graph.py:309-343): per graph one self-loop per node first, then directed relation
edges, graphs concatenated PyG-style (edge ids of a graph are contiguous, `batch` sorted).

`AnswerModel` = MGAT -> GlobalAttention -> classifier with ISubGVQA's own state_dict keys: the part of
ISubGVQA.forward (isubgvqa.py:267-292) that BASELINE config 2 drives directly, because the full model
only runs at C=300 (GraphNorm(300) in the scene-graph encoder).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor


@dataclass
class WorkloadConfig:
    num_graphs: int = 4096
    channels: int = 128
    heads: int = 4
    layers: int = 3
    masks: Tuple[float, ...] = (1.0, 1.0, 0.15)
    sampler: str = "gumbel"
    sample_k: int = 5
    nodes_dist: str = "normal"          # normal | uniform | pareto
    nodes_mean: float = 20.0
    nodes_std: float = 4.0
    nodes_min: int = 4
    nodes_max: int = 48
    edges_per_graph: float = 50.0       # self-loops included
    degree: str = "uniform"             # uniform | powerlaw (in-degree, cfg5)
    interpretable_mode: bool = False
    feature_dtype: str = "fp32"         # "fp16": projected rows / aggregated output stored as half (configs[4])
    seed: int = 2345
    sizes: Optional[Tuple[int, ...]] = None    # explicit node count per graph (tests: one oversize graph in a batch of small ones)


# BASELINE.json configs
CFG1 = WorkloadConfig(num_graphs=32, channels=300, layers=4, masks=(1.0, 1.0, 1.0, 0.15), sampler="gumbel", sample_k=5,
                      nodes_dist="uniform", nodes_min=2, nodes_max=16, edges_per_graph=0.0, seed=1234)
CFG2 = WorkloadConfig()
CFG4_PER_RANK = WorkloadConfig(seed=3456)
CFG5 = WorkloadConfig(sampler="aimle", nodes_dist="pareto", nodes_min=8, nodes_max=200, edges_per_graph=0.0,
                      degree="powerlaw", seed=4567)


@dataclass
class Workload:
    x: Tensor            # [N, C] node features entering MGAT
    edge_index: Tensor   # [2, E] int64, row 0 source, row 1 target
    edge_attr: Tensor    # [E, C]
    batch: Tensor        # [N] int64 sorted
    instr: Tensor        # [L, B, C]
    glf: Tensor          # [B, C]
    num_graphs: int = 0
    max_nodes: int = 0
    max_edges: int = 0
    graph_sizes: Optional[Tensor] = None      # HOST int64 [2, B]: nodes / in-edges per graph (what a collate knows anyway); stays on the host

    def to(self, device) -> "Workload":
        return Workload(self.x.to(device), self.edge_index.to(device), self.edge_attr.to(device), self.batch.to(device),
                        self.instr.to(device), self.glf.to(device), self.num_graphs, self.max_nodes, self.max_edges,
                        self.graph_sizes)


def graph_sizes(cfg: WorkloadConfig, gen: torch.Generator) -> Tensor:
    B = cfg.num_graphs
    if cfg.sizes is not None:
        if len(cfg.sizes) != B:
            raise ValueError("sizes: one entry per graph")
        return torch.tensor(cfg.sizes, dtype=torch.long)
    if cfg.nodes_dist == "uniform":
        n = torch.randint(cfg.nodes_min, cfg.nodes_max + 1, (B,), generator=gen)
    elif cfg.nodes_dist == "pareto":      # 8 + Pareto(alpha=1.5) clipped (cfg5)
        u = torch.rand(B, generator=gen).clamp_min(1e-6)
        n = (cfg.nodes_min + (u.pow(-1.0 / 1.5) - 1.0) * 8.0).round().long()
    else:
        n = (cfg.nodes_mean + cfg.nodes_std * torch.randn(B, generator=gen)).round().long()
    return n.clamp(cfg.nodes_min, cfg.nodes_max)


def make_topology(cfg: WorkloadConfig, gen: torch.Generator):
    """batch[N], edge_index[2,E]: per graph its self-loops, then random directed pairs."""
    n = graph_sizes(cfg, gen)
    B = cfg.num_graphs
    ptr = torch.zeros(B + 1, dtype=torch.long)
    ptr[1:] = n.cumsum(0)
    N = int(ptr[-1])
    batch = torch.repeat_interleave(torch.arange(B), n)
    if cfg.edges_per_graph > 0:
        extra = (cfg.edges_per_graph - cfg.nodes_mean + 5.0 * torch.randn(B, generator=gen)).round().long().clamp_min(1)
    elif cfg.degree == "powerlaw":
        extra = (2.0 * n.float()).round().long()
    else:                                 # cfg1: U{1..(32-n)} random pairs, <= 32 edges in total
        hi = (32 - n).clamp_min(1)
        extra = (torch.rand(B, generator=gen) * hi.float()).floor().long() + 1
    M = int(extra.sum())
    eg = torch.repeat_interleave(torch.arange(B), extra)          # graph of every extra edge
    ng = n[eg].float()
    src_loc = (torch.rand(M, generator=gen) * ng).floor().long()
    if cfg.degree == "powerlaw":          # in-degree ~ power law (alpha = 2): a few hub targets per graph
        u = torch.rand(M, generator=gen).clamp_min(1e-6)
        dst_loc = ((u.pow(-1.0) - 1.0)).floor().long()
        dst_loc = torch.minimum(dst_loc, (n[eg] - 1))
    else:
        dst_loc = (torch.rand(M, generator=gen) * ng).floor().long()
    # interleave per graph: [self loops of g][extras of g]
    loops = torch.arange(N)
    key_loop = batch * 2
    key_extra = eg * 2 + 1
    src_all = torch.cat([loops, ptr[eg] + src_loc])
    dst_all = torch.cat([loops, ptr[eg] + dst_loc])
    order = torch.sort(torch.cat([key_loop, key_extra]), stable=True).indices
    edge_index = torch.stack([src_all[order], dst_all[order]]).contiguous()
    return batch, edge_index, int(n.max())


def make_workload(cfg: WorkloadConfig) -> Workload:
    gen = torch.Generator().manual_seed(cfg.seed)
    batch, edge_index, nmax = make_topology(cfg, gen)
    N, E, B, C, L = batch.numel(), edge_index.size(1), cfg.num_graphs, cfg.channels, cfg.layers
    x = torch.randn(N, C, generator=gen)
    edge_attr = torch.randn(E, C, generator=gen)
    instr = torch.randn(L, B, C, generator=gen)
    glf = torch.randn(B, C, generator=gen)
    epg = torch.bincount(batch[edge_index[1]], minlength=B)
    emax = int(epg.max())
    return Workload(x, edge_index, edge_attr, batch, instr, glf, B, nmax, emax,
                    torch.stack([torch.bincount(batch, minlength=B), epg]))


def gumbel_noise(shape, device) -> Tensor:
    """Standard Gumbel noise as the reference's sampler draws it (gumbel_scheme.py:65-69: torch.distributions.Gumbel(0, 1)
    = TransformedDistribution(Uniform(tiny, 1 - eps), ...)): -log(-log(u)), u = tiny + rand * (1 - eps - tiny), from torch's
    generator -- which, unlike a kernel-argument seed, advances on every replay of a captured hipGraph."""
    tiny, eps = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).eps
    u = tiny + torch.rand(shape, device=device) * ((1.0 - eps) - tiny)
    return -torch.log(-torch.log(u))


class AnswerModel(torch.nn.Module):
    """gat_seq + graph_global_attention_pooling + embedding + logit_fc, keyed like ISubGVQA."""

    def __init__(self, channels: int, layers: int, masks, sampler: str, sample_k: int, heads: int = 4,
                 interpretable_mode: bool = False, tau: float = 1.0, num_answers: int = 1842,
                 concat_instr: bool = False, attn_dropout: float = 0.0, sample_ratio: Optional[float] = None,
                 sample_k_min: int = 1):
        super().__init__()
        from .models.att_pooling import GlobalAttention
        from .models.mgat import MGAT
        self.gat_seq = MGAT(channels=channels, num_ins=layers, heads=heads, use_instr=True,
                            masking_thresholds=list(masks), use_topk=True, interpretable_mode=interpretable_mode,
                            sampler_type=sampler, sample_k=sample_k, nb_samples=1, alpha=1.0, beta=10.0, tau=tau,
                            attn_dropout=attn_dropout, sample_ratio=sample_ratio, sample_k_min=sample_k_min,
                            concat_instr=bool(concat_instr))
        self.graph_global_attention_pooling = GlobalAttention(channels, channels)
        self.embedding = torch.nn.Sequential(torch.nn.Linear(channels * 3, 512), torch.nn.GELU(),
                                             torch.nn.Dropout(p=0.2))
        self.logit_fc = torch.nn.Linear(512, num_answers)

    def forward(self, wl: Workload, noises: Optional[Dict[int, Tensor]] = None, seed: Optional[int] = None,
                plan=None, use_hints: bool = True, capture: bool = False, trace=None):
        # trace: an explain.AttentionTrace; it receives the layers' attention weights and node masks, the mask and the gate of this
        # call.  The return tuple and its bits do not change
        from . import ops
        if trace is not None and capture:
            raise ValueError("trace together with capture=True: a replayed step keeps no attention weights; run it eagerly")
        if capture:
            return self._captured(wl, noises, seed, plan)
        if plan is None:
            plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=wl.glf.size(0),
                                       max_nodes=(wl.max_nodes or None) if use_hints else None,
                                       max_edges=(wl.max_edges or None) if use_hints else None,
                                       graph_sizes=wl.graph_sizes if use_hints else None)
        sub = ops.oversize_split(plan) if self.gat_seq.on_tiles(plan, wl.x.size(1), wl.edge_attr) else None
        if sub is None:
            return self._answer(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf, plan, noises, seed, None, trace)
        # a few graphs beyond a graph tile: they run as a batch of their own, the rest stays on the tile kernels
        if trace is not None:
            # each pass fills a trace of its own; the weights merge by edge, the layer masks by node, and the caller's trace is
            # filled once, behind the merge
            from .explain import AttentionTrace

            def traced(*args):
                t = AttentionTrace()
                logits, mask, gate = self._answer(*args, t)
                return logits, mask, gate, t.alphas, t.masks

            logits, mask, gate, alphas, masks = ops.run_split(plan, sub, traced, wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr,
                                                              wl.glf, noises, seed, kinds="gnnen")
            trace.alphas, trace.masks, trace.mask, trace.gate = alphas, masks, mask, gate
            return logits, mask, gate
        return ops.run_split(plan, sub, self._answer, wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf, noises, seed,
                             kinds="gnn")

    def _captured(self, wl: Workload, noises, seed, plan):
        """forward() as a replayed hipGraph (ops.StepCapture), one capture per batch SHAPE: for evaluation loops whose batches are
        launch-bound (the reference evaluates 4 x --batch-size graphs per step, datasets/build.py:59-62).  The plan is built inside
        the graph from the collate's bounds (wl.max_nodes / wl.max_edges, required); sampler noise comes from `noises` (copied into
        the graph's static tensors) or, when none is given, from torch's generator inside the graph -- fresh on every replay, like
        the reference's own draw; a kernel-argument `seed` would be frozen into the graph and is refused."""
        from . import ops
        if seed is not None:
            raise ValueError("capture=True: a seed is a kernel argument and would repeat in every replay; pass `noises` or neither")
        if plan is not None:
            raise ValueError("capture=True builds its plan inside the captured step")
        if not wl.max_nodes or not wl.max_edges:
            raise ValueError("capture=True needs the batch's per-graph bounds (Workload.max_nodes / max_edges): a captured step cannot "
                             "read them back from the device")
        cap = self.__dict__.get("_step_capture")
        if cap is None:
            cap = self.__dict__["_step_capture"] = ops.StepCapture()
        watch = self.__dict__.get("_weights_watch")
        if watch is None:
            watch = self.__dict__["_weights_watch"] = ops.WeightsWatch(self)
        keys = sorted(noises) if noises else []
        hints = (int(wl.max_nodes), int(wl.max_edges))

        def fn(x, edge_index, edge_attr, batch, instr, glf, *nz):
            p = ops.GraphPlan.build(batch, edge_index, num_graphs=glf.size(0), max_nodes=hints[0], max_edges=hints[1])
            out = self._answer(x, edge_index, edge_attr, batch, instr, glf, p, dict(zip(keys, nz)) if keys else None, None, None)
            return out, p

        tensors = [wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf] + [noises[k] for k in keys]
        return cap.run(fn, tensors, key_extra=("answer", hints, tuple(keys), self.training), stamp=watch.stamp())

    def _answer(self, x, edge_index, edge_attr, batch, instr, glf, plan, noises, seed, gate_feats, trace=None):
        from . import ops as _ops
        gate_q, pool_q = self.gat_seq.question_side(glf, gate_feats, self.graph_global_attention_pooling)
        h, mask, _, _ = self.gat_seq(x=x, edge_index=edge_index, edge_attr=edge_attr, instr_vectors=instr[:4],
                                     global_language_feats=glf, batch=batch, return_masks=True, plan=plan, noises=noises, seed=seed,
                                     gate_feats=gate_feats, gate_q=gate_q, trace=trace)
        embed, gate = self.graph_global_attention_pooling(x=h, u=glf, batch=batch, size=None, return_mask=True,
                                                          node_mask=mask, plan=plan, q=pool_q)
        if trace is not None:
            trace.mask, trace.gate = mask, gate
        feats = _ops.cat_mul_mlp(self.embedding, embed, glf, want_rowmax=True)
        return _ops.linear(feats, self.logit_fc.weight, self.logit_fc.bias), mask, gate


def build_answer_model(cfg: WorkloadConfig, weight_seed: int = 0) -> AnswerModel:
    torch.manual_seed(weight_seed)
    m = AnswerModel(cfg.channels, cfg.layers, cfg.masks, cfg.sampler, cfg.sample_k, cfg.heads, cfg.interpretable_mode)
    if cfg.feature_dtype == "fp16":
        for conv in m.gat_seq.convs:
            conv.feature_dtype = torch.float16
    # GraphNorm / bias parameters start at their trivial values; perturb them so parity covers them
    g = torch.Generator().manual_seed(weight_seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "bns" in name or name.endswith(".bias"):
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m


# ----------------------------------------------------------------------------------------------------------------
# BASELINE configs[2] stand-in: the FULL model (question encoder / decoder, scene-graph encoder, MGAT, pooling, classifier)
# at the reference's default width on GQA-shaped synthetic A0 tensors (no GQA data in either container)
# ----------------------------------------------------------------------------------------------------------------
def full_model_args(**overrides):
    """The argparse namespace `build_model` reads (ISubGVQA/utils/arg_parser.py defaults that reach the path)."""
    import argparse
    d = dict(text_sampling=False, general_hidden_dim=300, distributed=False, mgat_layers=4, use_all_instrs=False,
             use_global_mask=False, node_classification=False, sampler_type="imle", sample_k=5, nb_samples=1, alpha=1.0,
             beta=10.0, tau=1.0, use_masking=True, use_instruction=1, use_mgat=True, mgat_masks=[1.0, 1.0, 1.0, 0.15],
             use_topk=True, interpretable_mode=False, concat_instr=0, embed_cat=0, device="cpu", text_vocab_size=49408,
             sg_vocab_size=2578)
    d.update(overrides)
    return argparse.Namespace(**d)


@dataclass
class FullWorkload:
    x: Tensor                 # [N, 4] token ids (name + <= 3 attributes, pad id 1)
    edge_index: Tensor
    edge_attr: Tensor         # [E] relation token ids
    batch: Tensor
    x_bbox: Tensor            # [N, 4] ints
    added_sym_edge: Tensor    # per-graph LOCAL edge positions, concatenated without offset (quirk Q6)
    questions: Tensor         # [B, T] CLIP token ids
    att_mask: Tensor          # [B, T] 1 = real token
    max_nodes: int
    max_edges: int
    graph_sizes: Optional[Tensor] = None      # HOST int64 [2, B] (nodes, in-edges per graph), as loader.collate hands them over
    graph_index: Optional[Tensor] = None      # HOST int64 [Q] (make_shared_workload): the graph every question row asks; the
                                              # graph tensors then hold G distinct graphs, for ISubGVQA.encode_scene / ask

    def to(self, device) -> "FullWorkload":
        mv = lambda t: t.to(device)
        return FullWorkload(mv(self.x), mv(self.edge_index), mv(self.edge_attr), mv(self.batch), mv(self.x_bbox),
                            mv(self.added_sym_edge), mv(self.questions), mv(self.att_mask), self.max_nodes, self.max_edges,
                            self.graph_sizes, self.graph_index)

    def scene_graphs(self):
        import argparse
        return argparse.Namespace(x_bbox=self.x_bbox, added_sym_edge=self.added_sym_edge, max_nodes=self.max_nodes,
                                  max_edges=self.max_edges, graph_sizes=self.graph_sizes)

    def replicated(self) -> "FullWorkload":
        """A shared workload (graph_index set) with every question's graph copied out: the batch forward() takes for the same
        questions.  Host tensors, plain torch indexing.  added_sym_edge holds positions in the global edge list (quirk Q6) and
        cannot follow the copies: it has to be empty."""
        if self.graph_index is None or self.graph_sizes is None or self.x.is_cuda:
            raise ValueError("replicated(): a shared workload on the host (graph_index and graph_sizes set)")
        if self.added_sym_edge.numel():
            raise ValueError("replicated(): added_sym_edge positions are not offset per graph (quirk Q6) and cannot be replicated")
        idx = self.graph_index
        n, e = self.graph_sizes[0], self.graph_sizes[1]
        nptr, eptr = torch.cat([n.new_zeros(1), n.cumsum(0)]), torch.cat([e.new_zeros(1), e.cumsum(0)])
        nq, eq = n[idx], e[idx]
        iptr = torch.cat([nq.new_zeros(1), nq.cumsum(0)])
        batch = torch.repeat_interleave(torch.arange(idx.numel()), nq)
        node_src = torch.arange(int(nq.sum())) - iptr[:-1][batch] + nptr[idx][batch]
        ebatch = torch.repeat_interleave(torch.arange(idx.numel()), eq)
        eoff = torch.cat([eq.new_zeros(1), eq.cumsum(0)])
        edge_src = torch.arange(int(eq.sum())) - eoff[:-1][ebatch] + eptr[idx][ebatch]
        ei = self.edge_index[:, edge_src] + (iptr[:-1] - nptr[idx])[ebatch]
        return FullWorkload(self.x[node_src], ei, self.edge_attr[edge_src], batch, self.x_bbox[node_src], self.added_sym_edge,
                            self.questions, self.att_mask, self.max_nodes, self.max_edges, torch.stack([nq, eq]), None)


def make_full_workload(num_graphs: int, tokens: int = 12, seed: int = 7, sg_vocab: int = 2578,
                       text_vocab: int = 49408, sizes=None) -> FullWorkload:
    gen = torch.Generator().manual_seed(seed + 1)
    cfg = WorkloadConfig(num_graphs=num_graphs, seed=seed, sizes=None if sizes is None else tuple(sizes))
    batch, ei, nmax = make_topology(cfg, gen)
    N, E = batch.numel(), ei.size(1)
    x = torch.randint(0, sg_vocab, (N, 4), generator=gen)
    x[:, 1:][torch.rand(N, 3, generator=gen) < 0.5] = 1
    edge_attr = torch.randint(0, sg_vocab, (E,), generator=gen)
    x_bbox = torch.randint(0, 640, (N, 4), generator=gen)
    sym = torch.randint(0, 10, (num_graphs,), generator=gen)
    q = torch.randint(0, text_vocab, (num_graphs, tokens), generator=gen)
    lens = torch.randint(max(1, tokens // 2), tokens + 1, (num_graphs,), generator=gen)
    qmask = (torch.arange(tokens)[None] < lens[:, None]).long()
    epg = torch.bincount(batch[ei[1]], minlength=num_graphs)
    return FullWorkload(x, ei, edge_attr, batch, x_bbox, sym, q, qmask, nmax, int(epg.max()),
                        torch.stack([torch.bincount(batch, minlength=num_graphs), epg]))


def make_shared_workload(num_graphs: int, questions_per_graph: int, tokens: int = 12, seed: int = 7, sg_vocab: int = 2578,
                         text_vocab: int = 49408, sizes=None, shuffle: bool = True) -> FullWorkload:
    """G distinct graphs, Q = G x questions_per_graph question rows and the host index that names every question's graph
    (FullWorkload.graph_index): what an evaluation loop grouped by image hands to ISubGVQA.encode_scene / ask.  The graph side is
    make_full_workload(num_graphs)'s; shuffle: the questions come in a seeded random order, not grouped by graph."""
    wl = make_full_workload(num_graphs, tokens, seed, sg_vocab, text_vocab, sizes)
    gen = torch.Generator().manual_seed(seed + 2)
    Q = num_graphs * int(questions_per_graph)
    index = torch.arange(num_graphs).repeat_interleave(int(questions_per_graph))
    if shuffle:
        index = index[torch.randperm(Q, generator=gen)]
    q = torch.randint(0, text_vocab, (Q, tokens), generator=gen)
    lens = torch.randint(max(1, tokens // 2), tokens + 1, (Q,), generator=gen)
    wl.questions, wl.att_mask, wl.graph_index = q, (torch.arange(tokens)[None] < lens[:, None]).long(), index
    return wl


def make_gold(nodes_per_question, facets: int = 3, entries: int = 6, seed: int = 0, repeat: float = 0.2,
              unresolved: float = 0.1) -> Tensor:
    """A seeded gold table int32 [B, facets, entries] for ops.grounding / explain.evaluate(grounding=True), shaped like
    datasets.gqa.ObjectAnnotations.encode's: LOCAL node indices in [0, n_q), every facet list of a random length padded with -1,
    a share `repeat` of the entries repeating the question's first index (duplicates inside a facet and across facets), a share
    `unresolved` equal to -2 (annotated, not in the graph).  A question without nodes has -2 and -1 only.
    nodes_per_question: the node count of every question's graph (Workload.graph_sizes[0]; graph_sizes[0][graph_index] for a
    shared workload)."""
    gen = torch.Generator().manual_seed(seed)
    n = torch.as_tensor(nodes_per_question, dtype=torch.long).view(-1, 1, 1)
    B, F, M = n.size(0), int(facets), int(entries)
    idx = (torch.rand(B, F, M, generator=gen) * n.float()).floor().long()
    idx = torch.minimum(idx, (n - 1).clamp_min(0).expand(B, F, M))
    idx = torch.where(torch.rand(B, F, M, generator=gen) < repeat, idx[:, :1, :1].expand(B, F, M), idx)
    idx[(torch.rand(B, F, M, generator=gen) < unresolved) | (n == 0).expand(B, F, M)] = -2
    count = torch.randint(0, M + 1, (B, F), generator=gen)
    idx[torch.arange(M).view(1, 1, M) >= count.view(B, F, 1)] = -1
    return idx.to(torch.int32)
