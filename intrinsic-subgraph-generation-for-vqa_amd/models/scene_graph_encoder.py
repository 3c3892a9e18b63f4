"""Scene-graph encoder: token-embedding sum + bbox MLP -> one MetaLayer round -> fp64 GraphNorm.

Reference behaviour: SceneGraphEncoder.forward, ISubGVQA/models/scene_graph_encoder.py:53-104 with the
EdgeModel / NodeModel of :108-143 (PyG MetaLayer: edge model first, node model on the NEW edge features).
The reference constructor loads the GQA vocabulary and GloVe vectors from disk (:11-22); here the
vocabulary size is a constructor argument and weights come from the checkpoint.

Device work: embedding gathers are torch ops, every Linear(+GELU) runs on isg_linear_bf16x6 (ops.mlp; the E x 900 x C
edge MLP is the model's largest GEMM), BatchNorm stays a torch module; the per-destination mean of edge
messages is isg_scatter_mean over the batch's CSR plan (:141), and the float64 GraphNorm of :99-102 is
isg_graph_norm(accumulate_fp64=1) -- same fp64 arithmetic, without the reference's device->host->device
round trip through torch.DoubleTensor.
`added_sym_edge` holds per-graph LOCAL edge indices that PyG concatenates without offset; they are
applied to the global edge list as-is, exactly like the reference.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import autograd, ops
from .layers import GraphNorm

SPLIT_LINEARS = True    # inference path without the [E, 900] / [E, 600] concatenations (A/B switch for tests and tools)
SPLIT_TRAIN = True      # the same walk under autograd (forward_split_train, csrc/isg_sgenc_bwd.hip); off: training takes the reference's
                        # form, with the concatenations.  On by measurement: the full step at 4096 questions 127.8 against 131.8 ms,
                        # round spreads 0.3 ms (tools/time_train_full.py --sgenc, profiles/r09_a_sgenc_train_ab.json)
SG_VOCAB_SIZE = 2578   # reconstruction of the reference's torchtext vocab over meta_info/* 


class _EdgeModel(torch.nn.Module):
    def __init__(self, nf, ef, hidden_dim):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.edge_mlp = torch.nn.Sequential(torch.nn.Linear(2 * nf + ef, hidden_dim), torch.nn.GELU(),
                                            torch.nn.Linear(hidden_dim, hidden_dim))

    def forward(self, src, dest, edge_attr, u=None, batch=None):
        return ops.mlp(self.edge_mlp, torch.cat([src, dest, edge_attr], 1))              # :119-120 (E x 900 x C: bf16x6 kernel)


class _NodeModel(torch.nn.Module):
    def __init__(self, nf, hidden_dim):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.node_mlp_1 = torch.nn.Sequential(torch.nn.Linear(nf + hidden_dim, hidden_dim), torch.nn.GELU(),
                                              torch.nn.Linear(hidden_dim, hidden_dim))
        self.node_mlp_2 = torch.nn.Sequential(torch.nn.Linear(nf + hidden_dim, hidden_dim), torch.nn.GELU(),
                                              torch.nn.Linear(hidden_dim, hidden_dim))

    def forward(self, x, edge_index, edge_attr, plan: ops.GraphPlan):
        row = edge_index[0]
        out = ops.mlp(self.node_mlp_1, torch.cat([x[row], edge_attr], dim=1))            # :139-140
        out = ops.scatter_mean(out.contiguous(), plan)                                   # :141
        return ops.mlp(self.node_mlp_2, torch.cat([x, out], dim=1))                      # :142-143


class _MetaLayer(torch.nn.Module):
    def __init__(self, edge_model, node_model):
        super().__init__()
        self.edge_model, self.node_model = edge_model, node_model

    def forward(self, x, edge_index, edge_attr, plan):
        row, col = edge_index[0], edge_index[1]
        edge_attr = self.edge_model(x[row], x[col], edge_attr)
        return self.node_model(x, edge_index, edge_attr, plan), edge_attr

    def forward_split(self, x, edge_index, edge_tokens, edge_sign, embedding, plan):
        """The same MetaLayer round without the [E, 900] / [E, 600] concatenations (inference; csrc/isg_sgenc.hip):
        a Linear over cat([x[row], x[col], e]) is W_a x[row] + W_b x[col] + W_c e, so the node parts are projected once
        per NODE, W_c emb[token] is a row of a [vocabulary, C] table (the added_sym_edge sign commutes), and what is left
        per edge is a gather-add + GELU.  Same for node_mlp_1 over cat([x[row], e']).  1.67x fewer flops."""
        em, nm = self.edge_model.edge_mlp, self.node_model.node_mlp_1
        nf, C = x.size(1), em[0].weight.size(0)
        w_nodes = ops.derived_weight("sg_nodes", (em[0].weight, nm[0].weight), lambda: torch.cat(
            [em[0].weight[:, :nf], em[0].weight[:, nf:2 * nf], nm[0].weight[:, :nf]], dim=0).contiguous())
        w_tok = ops.derived_weight("sg_tok", (em[0].weight,), lambda: em[0].weight[:, 2 * nf:].contiguous())
        w_e = ops.derived_weight("sg_e", (nm[0].weight,), lambda: nm[0].weight[:, nf:].contiguous())
        row, col = edge_index[0].contiguous(), edge_index[1].contiguous()
        P = ops.linear(x, w_nodes, None)                                   # [N, 3C]: W_a x | W_b x | W_x x
        # [V, C]: W_c emb -- a function of the parameters and of the kernel its Linear runs on alone: made once per (weights,
        # route), not once per forward (it was a 20 us launch of every forward: 2.5 % of a single question's GPU time)
        route = ops.linear_route(embedding.weight.size(0), *w_tok.shape)
        table = ops.derived_weight(("sg_table", route), (embedding.weight, em[0].weight),
                                   lambda: ops.linear(embedding.weight.detach(), w_tok, None))
        E = row.numel()
        po = ops.GATHER_ADD_PLANES and ops.reads_planes32(E, em[2].weight.size(0), C)   # the Linear behind a gather-add runs on the planes32
        h = ops.gather_add(P[:, :C], row, P[:, C:2 * C], col, table, edge_tokens, edge_sign, bias=em[0].bias, gelu=True,
                           planes_out=po)                                  # engine: its operand leaves the gather-add as planes
        e_new = ops.linear(h, em[2].weight, em[2].bias)                    # :119-120 second layer
        g = ops.linear(e_new, w_e, None)                                   # W_e e'
        po = ops.GATHER_ADD_PLANES and ops.reads_planes32(E, *nm[2].weight.shape)
        h = ops.gather_add(P[:, 2 * C:], row, D=g, bias=nm[0].bias, gelu=True, planes_out=po)
        m = ops.linear(h, nm[2].weight, nm[2].bias)                        # :139-140
        agg = ops.scatter_mean(m, plan)                                    # :141
        return ops.mlp(self.node_model.node_mlp_2, torch.cat([x, agg], dim=1)), e_new   # :142-143

    def forward_split_train(self, x, edge_index, edge_tokens, edge_sign, embedding, plan, edge_sign_grad=None):
        """forward_split under autograd (SPLIT_TRAIN).  The slices and the concatenation of the parameters are torch ops, so that
        their gradients flow back into edge_mlp.0 / node_mlp_1.0 (ops.derived_weight builds under no_grad); the token table is made
        every step from the embedding matrix, behind an identity that keeps its padding_idx row without gradient (zeroing that row
        of d table instead would also drop the pad row's share of d w_tok); every Linear is autograd.linear; both gather-adds
        write fp32 rows and differentiate through isg_gather_add_bwd + isg_segment_rows_sum over the plan's two CSRs and the edge
        tokens' CSR.  Nothing of size [E, 900] or [E, 600] is made or kept.
        edge_sign_grad: `e[sym] = e[sym] * -1` (:80) flips an edge named m times in added_sym_edge ONCE, but autograd differentiates
        the indexed read by an index_add: the embedding receives -m times that edge's gradient, while the gradient of edge_mlp.0's
        weight is formed with the row's forward value, flipped once.  The reference trains with that and so does this walk: with
        a sign of the backward's own, the table is made twice with equal values -- one differentiated into the weight slice under
        edge_sign, one into the embedding under edge_sign_grad (a [V, C] Linear and one more segment sum over dz)."""
        em, nm = self.edge_model.edge_mlp, self.node_model.node_mlp_1
        nf, C = x.size(1), em[0].weight.size(0)
        w_nodes = torch.cat([em[0].weight[:, :nf], em[0].weight[:, nf:2 * nf], nm[0].weight[:, :nf]], dim=0)
        w_tok = em[0].weight[:, 2 * nf:].contiguous()
        w_e = nm[0].weight[:, nf:].contiguous()
        row, col = edge_index[0].contiguous(), edge_index[1].contiguous()
        by_src, by_dst = plan.source_csr()[:2], (plan.rowptr, plan.eid)
        by_tok = ops.token_csr(edge_tokens, embedding.weight.size(0))
        P = autograd.linear(x, w_nodes, None, False)                       # [N, 3C]: W_a x | W_b x | W_x x
        emb = autograd.zero_row_grad(embedding.weight, embedding.padding_idx)
        if edge_sign_grad is None:
            table, table_e = autograd.linear(emb, w_tok, None, False), None                # [V, C]: W_c emb
        else:
            table = autograd.linear(embedding.weight.detach(), w_tok, None, False)
            table_e = autograd.linear(emb, w_tok.detach(), None, False)
        h = ops.gather_add(P[:, :C], row, P[:, C:2 * C], col, table, edge_tokens, edge_sign, bias=em[0].bias, gelu=True,
                           csr_a=by_src, csr_b=by_dst, csr_t=by_tok, T2=table_e, sign2=edge_sign_grad)
        e_new = autograd.linear(h, em[2].weight, em[2].bias, False)        # :119-120 second layer
        g = autograd.linear(e_new, w_e, None, False)                       # W_e e'
        h = ops.gather_add(P[:, 2 * C:], row, D=g, bias=nm[0].bias, gelu=True, csr_a=by_src)
        m = autograd.linear(h, nm[2].weight, nm[2].bias, False)            # :139-140
        agg = ops.scatter_mean(m, plan)                                    # :141
        return ops.mlp(self.node_model.node_mlp_2, torch.cat([x, agg], dim=1)), e_new   # :142-143


def weighted_batch_norm(bn: torch.nn.BatchNorm1d, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """A BatchNorm1d in train() over rows [N, C] of which row n stands for w[n] >= 0 equal rows: W = sum w, mean = sum w x / W,
    biased var = sum w (x - mean)^2 / W -- the statistics, the result and (under autograd) the gradients of the module applied
    to the rows physically repeated, up to rounding; a row of weight 0 takes no part.  The running statistics move as torch
    moves them at W rows (unbiased factor W / (W - 1), `momentum` or the cumulative average, num_batches_tracked).  Torch ops:
    these are reductions over [N, 4], [N, 16] and [N, 332], not a hot path.  Nothing here waits for the device (so W <= 1,
    which torch refuses, is not looked for)."""
    wc = w.to(x.dtype).unsqueeze(1)
    W = wc.sum()
    mean = (wc * x).sum(0) / W
    xc = x - mean
    var = (wc * xc * xc).sum(0) / W
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            bn.num_batches_tracked += 1
            f = 1.0 / bn.num_batches_tracked.to(x.dtype) if bn.momentum is None else bn.momentum
            bn.running_mean.mul_(1.0 - f).add_(f * mean.detach().to(bn.running_mean.dtype))
            bn.running_var.mul_(1.0 - f).add_(f * (var.detach() * (W / (W - 1.0))).to(bn.running_var.dtype))
    y = xc * torch.rsqrt(var + bn.eps)
    return y * bn.weight + bn.bias if bn.affine else y


class _WeightedBatchNorm:
    """What stands in for a BatchNorm1d of a Sequential handed to ops.mlp while a multiplicity is in force (no `weight` of its
    own: ops.mlp calls it like any module that is no Linear)."""

    def __init__(self, bn, w):
        self.bn, self.w = bn, w

    def __call__(self, x):
        return weighted_batch_norm(self.bn, x, self.w)


class SceneGraphEncoder(torch.nn.Module):
    def __init__(self, hidden_dim, dist=False, vocab_size: int = SG_VOCAB_SIZE, pad_idx: Optional[int] = 1):
        super().__init__()
        self.hidden_dim, self.dist = hidden_dim, dist
        self.sg_emb_dim = 300
        self.sg_vocab_embedding = torch.nn.Embedding(vocab_size, self.sg_emb_dim, padding_idx=pad_idx)
        self.scene_graph_encoding_layer = _MetaLayer(_EdgeModel(self.sg_emb_dim, self.sg_emb_dim, hidden_dim),
                                                     _NodeModel(self.sg_emb_dim, hidden_dim))
        self.graph_layer_norm = GraphNorm(self.sg_emb_dim)
        bn = torch.nn.SyncBatchNorm if dist else torch.nn.BatchNorm1d
        self.bbox_encoding = torch.nn.Sequential(bn(4), torch.nn.Linear(4, 16), torch.nn.GELU(),
                                                 bn(16), torch.nn.Linear(16, 32), torch.nn.GELU())
        self.feat_reduc = torch.nn.Sequential(bn(self.sg_emb_dim + 32),
                                              torch.nn.Linear(self.sg_emb_dim + 32, self.sg_emb_dim), torch.nn.GELU())

    def forward(self, x, edge_index, edge_attr, batch, explainer=False, explainer_stage=False, gt_scene_graphs=None,
                plan: Optional[ops.GraphPlan] = None, *, multiplicity: Optional[torch.Tensor] = None):
        # train(): the BatchNorm layers use batch statistics like the reference's (torch modules); the HIP operators of this
        # encoder (embedding sum, gather-add, scatter_mean, fp64 GraphNorm) differentiate through autograd.py
        # multiplicity: int32 [G], how often every graph of this DISTINCT batch is asked (ops.GraphInstances.counts()).  In train()
        # the three BatchNorm layers then weigh a node's row by its graph's count, which gives the statistics of the batch with
        # every graph copied out (weighted_batch_norm); in eval() the layers run as they are.  None: nothing changes.
        bbox_encoding, feat_reduc = self.bbox_encoding, self.feat_reduc
        if multiplicity is not None and self.dist:
            raise ValueError("SceneGraphEncoder: a multiplicity with SyncBatchNorm (dist=True) is not supported -- the weighted "
                             "statistics would need a weighted all-reduce")
        if multiplicity is not None and self.training:
            w = multiplicity.index_select(0, batch)
            weighted = lambda seq: [_WeightedBatchNorm(m, w) if isinstance(m, torch.nn.BatchNorm1d) else m for m in seq]
            bbox_encoding, feat_reduc = weighted(bbox_encoding), weighted(feat_reduc)
        first = explainer and (explainer_stage == 0)
        x_embed_sum = x if first else ops.embedding_sum(self.sg_vocab_embedding.weight, x,     # :63-70 (sum of the token rows)
                                                        self.sg_vocab_embedding.padding_idx)
        x_bbox = ops.mlp(bbox_encoding, gt_scene_graphs.x_bbox.to(dtype=x_embed_sum.dtype))   # :72
        x_embed_sum = ops.mlp(feat_reduc, torch.cat((x_embed_sum, x_bbox), dim=1))  # :73-74
        sym = gt_scene_graphs.added_sym_edge
        if plan is None:
            plan = ops.GraphPlan.build(batch, edge_index)
        rec = torch.is_grad_enabled() and (x_embed_sum.requires_grad or any(p.requires_grad for p in self.parameters()))
        shapes = self.hidden_dim % 4 == 0 and self.sg_emb_dim % 4 == 0                       # isg_gather_add: float4 rows
        split = shapes and (SPLIT_TRAIN if rec else SPLIT_LINEARS)
        if split:   # no [E, 900] concatenation (forward_split / forward_split_train); the sign of :80 rides along as a vector
            sign = torch.ones(edge_attr.numel(), dtype=torch.float32, device=edge_attr.device)
            if sym is not None and sym.numel() > 0:
                sign.index_fill_(0, sym, -1.0)        # :80 (duplicates: flipped once); index_fill_, not sign[sym] = ...: the indexed
                                                      # assignment synchronises on this stack and cannot sit in a captured step
            operands = (x_embed_sum.contiguous(), edge_index, edge_attr.contiguous(), sign, self.sg_vocab_embedding, plan)
            if rec:
                ops.COUNTERS["sgenc_train_kernels"] += 1
                sign_grad = None
                if sym is not None and sym.numel() > 0:       # an edge named m times: -m in the backward (forward_split_train)
                    named = torch.zeros_like(sign).index_add_(0, sym, torch.ones(sym.numel(), dtype=sign.dtype, device=sign.device))
                    sign_grad = torch.where(named > 0, -named, sign)
                x_enc, e_enc = self.scene_graph_encoding_layer.forward_split_train(*operands, edge_sign_grad=sign_grad)
            else:
                x_enc, e_enc = self.scene_graph_encoding_layer.forward_split(*operands)
        else:
            edge_embed = self.sg_vocab_embedding(edge_attr)                              # :76
            if sym is not None and sym.numel() > 0:
                edge_embed[sym, :] = edge_embed[sym, :] * -1                             # :80
            x_enc, e_enc = self.scene_graph_encoding_layer(x_embed_sum, edge_index, edge_embed, plan)   # :91-97
        gn = self.graph_layer_norm
        if x_enc.size(1) != gn.in_channels:
            raise RuntimeError(f"GraphNorm({gn.in_channels}) applied to {x_enc.size(1)} channels: the full model only "
                               "works at general_hidden_dim=300 (scene_graph_encoder.py:33,101)")
        x_enc = gn(x_enc, plan=plan, fp64=True)                                          # :99-102
        return x_enc, e_enc
