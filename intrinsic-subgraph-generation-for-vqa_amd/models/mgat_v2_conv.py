"""GATv2 convolution with edge features, instruction gating and node->edge masking.

Reference behaviour: MaskingGATv2Conv, ISubGVQA/models/mgat_v2_conv.py:18-285 (constructor keywords,
forward signature and return tuples are kept; ``plan``/``noise``/``seed`` are optional extras).

Device work per call:
  isg_instr_gate                 x = gelu(x * instruction[batch])                       (:156-157)
  isg_linear_bf16x6_rowbias      concat_instr: the layer reads cat(x, instruction[batch]), 2C wide (:153-154), and the
                                 concatenation is never formed: cat(x, u[batch]) W^T + b = x W[:, :C]^T + (u W[:, C:]^T + b)[batch],
                                 the N-row GEMM at K = C with one bias row per graph (CONCAT_SPLIT; include/isg_concat.h)
  MaskingModel (masked layers)   node gate + top-k sampler -> node mask [N,1]           (:161-168)
  three dense projections        lin_l, lin_r (C -> H*C, +bias), lin_edge (no bias)     (:177,181,259)
  isg_gatv2_mp_fwd               message + segment softmax + aggregate + bias, with the node->edge
                                 mask product of NodeMaskToEdgeMask fused in            (:169-171,215-232,243-279)
  autograd.conv_half_rows        feature_dtype = half under autograd: both projections, isg_gatv2_mp_fwd_f16 and the rounding of
                                 `out` as one autograd node with fp32 ends; its backward reads the saved half rows
                                 (isg_gatv2_mp_bwd_f16, include/isg_mp_f16_train.h)
  isg_gatv2_mp_fwd_dropout       the same in train() with dropout > 0: alpha = F.dropout(alpha, p, training) between the
                                 softmax and the aggregation, keep or drop drawn from (seed, edge id, head)  (:274-279)
Which of these launches a layer makes on a batch -- message passing as one persistent launch on graph tiles, with lin_l | lin_r
inside or before it, as the edge-logits pair, or un-fused; what the gate writes -- is decided by ops.conv_route, nowhere else:
route() asks it once per forward, forward() follows the answer.
The reference stashes alpha on the module between message() and forward() (:223-224,274); here it
is a local, so the module is re-entrant.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import Parameter

from .. import ops
from ..sampling.node_edge_masks import NodeMaskToEdgeMask
from .layers import GlorotLinear, glorot_
from .masking import MaskingModel

# The attention dropout of a layer draws from the stream of (layer seed + this): the sampler of the same layer draws from the
# layer seed itself (MaskingModel), so an edge's keep decision never shares a Philox stream with a node's noise.
ATTN_DROPOUT_SEED_OFFSET = 8192
# concat_instr layers: lin_l | lin_r and the node gate's node_nn on the row-biased Linear (ops.linear_rowbias) instead of the
# literal torch.cat((x, instruction[batch]), 1) in front of the existing Linears.  Off is the parity twin and the measured
# baseline (tools/time_concat_instr.py).  An input width that is no multiple of 4 takes the literal form either way.
CONCAT_SPLIT = True


def _seg32(plan, batch: Tensor) -> Tensor:
    """batch as the int32 segment vector the row-biased Linear reads, kept on the plan (one cast per batch, not per layer)."""
    memo = plan.memo()
    seg = memo.get("seg32")
    if seg is None or seg.numel() != batch.numel():
        seg = memo["seg32"] = batch.int().contiguous()
    return seg


class MaskingGATv2Conv(torch.nn.Module):
    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1,
                 concat: bool = True, negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim: Optional[int] = None, fill_value="mean", bias: bool = True, share_weights: bool = False,
                 masking_threshold=None, use_instr: bool = False, use_topk: bool = False, concat_instr: bool = False,
                 use_all_instrs: bool = False, sampler_type: str = None, sample_k: int = None, nb_samples: int = 1,
                 alpha=1.0, beta=10.0, tau=1.0, sample_ratio: Optional[float] = None, sample_k_min: int = 1, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("bipartite in_channels=(src, dst) is never used by ISubGVQA (mgat.py:58)")
        if add_self_loops:
            raise NotImplementedError("add_self_loops=True: MGAT passes False (mgat.py:63); scene graphs carry their "
                                      "self-loops already (datasets/scene_graph.py:309-343)")
        if not concat:
            raise NotImplementedError("concat=False (head averaging) is never used by ISubGVQA")
        if use_all_instrs:
            raise NotImplementedError("use_all_instrs is off by default (arg_parser.py:108) and outside this path: under use_topk "
                                      "it hands the samplers a 2-D tensor they cannot unpack (deterministic_scheme.py:37)")
        if concat_instr and use_instr and in_channels % 2 != 0:
            raise ValueError(f"concat_instr: in_channels = {in_channels} is the width of cat(x, instruction[batch]), twice the node "
                             "rows' (mgat_v2_conv.py:152-154)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.add_self_loops, self.edge_dim, self.fill_value = add_self_loops, edge_dim, fill_value
        self.share_weights, self.use_instr = share_weights, use_instr
        self.concat_instr, self.use_all_instrs = concat_instr, use_all_instrs
        self._cat = bool(concat_instr and use_instr)     # the flag acts under use_instr only (mgat_v2_conv.py:152-153)

        self.lin_l = GlorotLinear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else GlorotLinear(in_channels, heads * out_channels, bias=bias)
        self.att = Parameter(torch.empty(1, heads, out_channels))
        self.lin_edge = GlorotLinear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
        if bias:
            self.bias = Parameter(torch.empty(heads * out_channels))
        else:
            self.register_parameter("bias", None)
        self.mask = MaskingModel(in_channels, out_channels, masking_threshold, use_topk=use_topk,
                                 sampler_type=sampler_type, sample_k=sample_k, nb_samples=nb_samples, alpha=alpha,
                                 beta=beta, tau=tau, sample_ratio=sample_ratio, sample_k_min=sample_k_min)
        self.masking = NodeMaskToEdgeMask.apply
        # storage type of the projected rows x_l / x_r / e_proj and of the aggregated output (fp32 arithmetic either way):
        # torch.float16 is BASELINE configs[4] ("fp16 features / fp32 accumulate").  Inference reads and writes half rows in every
        # kernel that has the form; under autograd the un-fused route keeps them as the layer's saved tensors and differentiates
        # the fp32 function at the rounded rows (trains_on_half_rows, autograd.conv_half_rows).  Attention dropout needs fp32 rows
        self.feature_dtype = torch.float32
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout={dropout}: the attention dropout needs 0 <= dropout < 1")
        self.reset_parameters()

    def attn_dropout_active(self) -> bool:
        """Does this call drop attention weights?  train() with dropout > 0, whether or not autograd records."""
        return bool(self.training and self.dropout > 0.0)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()
        if self.lin_edge is not None:
            self.lin_edge.reset_parameters()
        glorot_(self.att)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def rows_dtype(self, plan) -> torch.dtype:
        """The storage type of x_l / x_r / e_proj / out for THIS batch: feature_dtype -- unless it is half and a graph of the batch lies
        beyond the per-graph kernel's 256-node / 1 024-slot tables (GK_NCAP_L / GK_ECAP_L, csrc/isg_mp_graph.hip), the only kernels
        that read half rows: such a batch keeps fp32 rows (more precise than the half rows it was asked for, never less; within the
        1e-3 the fp16 mode is held to) instead of raising ISG_EUNSUPPORTED from the message-passing launch."""
        fdt = self.feature_dtype
        if fdt == torch.float16 and plan is not None and (plan.nmax > ops.GK_NCAP_L or plan.emax > ops.GK_ECAP_L):
            return torch.float32
        return fdt

    def trains_on_half_rows(self, plan, conv: str, recording: bool, e_proj_given: bool) -> bool:
        """Does this call run as autograd.conv_half_rows -- projections, message passing and the rounding of `out` as ONE autograd
        node that saves half rows?  The un-fused route, half rows on this batch (rows_dtype: an oversize graph keeps fp32 rows),
        autograd recording through an operand of the layer, e_proj not handed in (it would be a half tensor on the autograd
        graph's edge), no attention dropout (fp32 rows only).  Otherwise every line of forward() runs as it did."""
        return bool(conv == "unfused" and self.rows_dtype(plan) == torch.float16 and recording and not e_proj_given
                    and not self.attn_dropout_active())

    def route(self, plan, in_channels: int, edge_attr, e_proj=None, imle_att=None) -> "ops.ConvRoute":
        """ops.conv_route for this layer on this batch, kept on the plan.  GraphPlan.tile_mode can cost a device-to-host sync: it is
        asked only when the route depends on it."""
        masked = self.mask.masking_threshold != 1.0
        if self._cat:
            in_channels = self.in_channels          # the true input width, whatever the caller read off the node rows
        facts = dict(heads=self.heads, channels=self.out_channels, in_channels=in_channels,
                     edge_dim=edge_attr.size(1) if edge_attr is not None and edge_attr.dim() == 2 else None,
                     rows_dtype=self.rows_dtype(plan), share_weights=self.share_weights, use_instr=self.use_instr, masked=masked,
                     gate_on_planes=masked and self.mask.planes_ready(imle_att), grad=torch.is_grad_enabled(),
                     e_proj_given=e_proj is not None, has_edge_lin=self.lin_edge is not None,
                     attn_dropout=self.attn_dropout_active())
        if self._cat:
            facts["concat_instr"] = True
        if plan is None:
            return ops.conv_route(N=0, B=0, E=0, nmax=0, has_csr=False, tile_mode="none", **facts)
        memo, key = plan.memo(), ("route", id(self), *facts.values())
        hit = memo.get(key)
        if hit is None or hit[0] is not ops.CFG:
            facts.update(N=plan.N, B=plan.B, E=plan.E, nmax=plan.nmax, has_csr=plan.rowptr is not None)
            route = ops.conv_route(tile_mode="tiles", **facts)
            if route.conv in ("layer_conv", "tile_conv"):
                mode = plan.tile_mode(ops.TILE_CONV_NODES, ops.TILE_CONV_EDGES)
                if mode != "tiles":
                    route = ops.conv_route(tile_mode=mode, **facts)
            hit = memo[key] = (ops.CFG, route)
        return hit[1]

    def dispatch(self, plan, in_channels: int, edge_attr, e_proj=None) -> str:
        """Which kernels run this layer's message passing: ops.ConvRoute.conv."""
        return self.route(plan, in_channels, edge_attr, e_proj).conv

    def forward(self, x: Tensor, edge_index: Tensor, batch: Tensor, edge_attr: Optional[Tensor] = None,
                instruction: Optional[Tensor] = None, imle_att: Optional[Tensor] = None,
                return_attention_weights: bool = None, return_masks: bool = None, all_instrs=None,
                plan: Optional[ops.GraphPlan] = None, noise: Optional[Tensor] = None, seed: Optional[int] = None,
                e_proj: Optional[Tensor] = None, x_gated: Optional[Tensor] = None,
                x_planes: Optional["ops.NodePlanes"] = None, out_planes: bool = False, gate_rows_given: bool = False,
                route: Optional["ops.ConvRoute"] = None, gate_q: Optional[Tensor] = None, want_alpha: bool = True,
                sparse_out: bool = False):
        # want_alpha / sparse_out (the layer_conv route alone; ops.gatv2_layer_conv): False = the attention weights are not stored and
        # None is returned for them; True = the result may lack the rows without a live in-slot (the caller reads it through
        # ops.mgat_dense_tail or ops.dense_conv_out)
        # route: self.route(...) of this call, from a caller that has asked already (MGAT)
        # gate_q: mask.ques_nn(imle_att), from a caller that ran it ahead of the layers (ops.small_mlps)
        # gate_rows_given: imle_att[g] already IS the row the node gate of graph g reads (ops.run_split's sub-batch: the reference's
        # double index batch[batch[n]], quirk Q3, refers to positions in the batch the graphs were taken from)
        # out_planes (inference): the caller feeds the result to a Linear + GELU on the planes32 engine (MGAT's x_proj.0) and
        # takes it as a segmented ops.Planes32 where the message-passing kernel can write that (H = 4, the flat kernel)
        H, C = self.heads, self.out_channels
        if x.dim() != 2:
            raise ValueError("x must be [N, C]")
        if plan is None:
            plan = ops.GraphPlan.build(batch, edge_index,
                                       num_graphs=None if instruction is None else instruction.size(0))
        if route is None:
            route = self.route(plan, x.size(1), edge_attr, e_proj, imle_att)
        how, masked = route.conv, self.mask.masking_threshold != 1.0
        planes = None          # gelu(x * instruction[batch]) as the planes isg_gatv2_layer_conv reads (fp32 rows only where needed)
        split = None           # concat_instr on the row-biased Linear: (instruction [B, C], seg int32 [N], ptr int32 [B + 1])
        if self._cat:                                                            # :153-154
            if route.gate != "none" or how not in ("pair", "unfused"):
                raise RuntimeError(f"a concat_instr layer runs un-gated on the pair or the un-fused kernels, not as {route}: a "
                                   "route handed in must come from self.route() of this call")
            x = x.float().contiguous()
            if 2 * x.size(1) != self.in_channels or instruction is None or instruction.size(1) != x.size(1):
                raise ValueError(f"concat_instr: x {tuple(x.shape)} and instruction must both be {self.in_channels // 2} wide")
            if CONCAT_SPLIT and x.size(1) % 4 == 0:
                split = (instruction.float().contiguous(), _seg32(plan, batch), plan.ptr)
            else:
                x = torch.cat((x, instruction.float()[batch]), dim=1)
        elif (x_gated is not None or x_planes is not None) and self.use_instr:
            # gelu(x * instruction[batch]) was already written by the previous layer's fused tail (isg_mgat_dense_tail)
            x, planes = x_gated, x_planes
            if x is None and route.gate_rows:
                raise RuntimeError("the previous layer's tail left no fp32 rows of the gated input, and this layer needs them")
        else:
            x = x.float().contiguous()
            if route.gate == "planes":
                x, planes = ops.instr_gate_planes(x, instruction.contiguous(), batch, want_rows=route.gate_rows)   # :156-157
            elif route.gate == "planes32":
                # the projection runs on the planes32 engine: the gate writes its operand (and fp32 rows only for a node gate)
                rows, xp = ops.instr_gate_planes32(x, instruction.contiguous(), batch, want_rows=masked)   # :156-157
                x = rows if masked else xp
            elif route.gate == "rows":
                x = ops.instr_gate(x, instruction.contiguous(), batch, plan=plan)        # :156-157

        mask = None
        if masked:                                                                       # :161
            mask = self.mask(x, imle_att, batch, edge_index, use_all_instrs=False, plan=plan, noise=noise,
                             seed=seed, u_is_per_graph=not gate_rows_given, x_planes=planes, q=gate_q, concat=split)   # :166-168

        def done(out, alpha):
            if isinstance(return_attention_weights, bool):
                return out, mask, (None if alpha is None else (edge_index, alpha))       # :237 (None: want_alpha=False)
            return out, mask                                                             # :241

        fdt = self.rows_dtype(plan)
        kw = dict(bias=self.bias, node_mask=mask, negative_slope=self.negative_slope)
        drop = self.attn_dropout_active()
        if drop and (how != "unfused" or fdt != torch.float32):
            raise RuntimeError(f"attention dropout runs on the un-fused route with fp32 rows only, not on {how!r} / {fdt}: a "
                               "route handed in must come from self.route() of this call")
        if how == "layer_conv":
            # lin_l | lin_r, lin_edge, logits, softmax and aggregation as ONE persistent launch on graph-aligned tiles
            # (csrc/isg_layer_conv.hip): x_l / x_r live in LDS only                       # :177-181, :215-232, :243-279
            res = ops.gatv2_layer_conv(planes if planes is not None else x, self.lin_l, self.lin_r, edge_attr.float().contiguous(),
                                       self.lin_edge.weight, self.att, plan, H, want_rowmax=True, want_alpha=want_alpha,
                                       sparse_out=sparse_out, **kw)
            if res is not None:
                return done(*res)
            if x is None:
                raise RuntimeError("isg_gatv2_layer_conv refused a shape ops.conv_route accepted, and the gated input "
                                   "exists only as planes")
            how = "tile_conv"
        if self._cat and fdt != torch.float32 and ops._rec(x, instruction, mask, *self.lin_l.parameters(),
                                                                   *self.lin_r.parameters()):
            raise ops._lib.IsgError("training a concat_instr layer on half rows (feature_dtype = torch.float16) is not supported: "
                                    "the row-biased Linear differentiates fp32 rows only; train it with fp32 rows")
        if (edge_attr is not None and self.lin_edge is not None and
                self.trains_on_half_rows(plan, how, ops._rec(x, edge_attr, mask, self.att, self.bias, *self.lin_l.parameters(),
                                                             *self.lin_r.parameters(), *self.lin_edge.parameters()),
                                         e_proj is not None)):
            from .. import autograd
            if edge_attr.dim() == 1:
                edge_attr = edge_attr.view(-1, 1)
            return done(*autograd.conv_half_rows(x, edge_attr.float().contiguous(), self.lin_l, self.lin_r, self.lin_edge.weight,
                                                 self.att, self.bias, mask, None, plan, H, self.negative_slope))
        if split is not None:
            x_l, x_r = self._project_split(x, split, fdt)                                # :177-181 without the concatenation
        elif self.share_weights:
            x_l = x_r = ops.linear(x, self.lin_l.weight, self.lin_l.bias, out_dtype=fdt)  # :177-179
        else:   # lin_l and lin_r share their input: one [N, 2*H*C] projection, x_l / x_r are its column halves
            x_l, x_r = ops.linear_fused(x, (self.lin_l, self.lin_r), out_dtype=fdt)      # :177,181
        if how == "tile_conv" and ops.tile_conv_supported(plan, H, C, edge_attr.size(1)):
            # edge GEMM + logits + softmax + aggregation as one launch on graph-aligned tiles (csrc/isg_layer_tile.hip)
            res = ops.gatv2_tile_conv(x_l, x_r, edge_attr.float().contiguous(), self.lin_edge.weight, self.att, plan, H,
                                      want_rowmax=True, **kw)                            # :215-232, :243-279
            if res is not None:
                return done(*res)
            how = "pair"
        if how in ("tile_conv", "pair"):
            # lin_edge folded into the logits (csrc/isg_mp_logits.hip): e_proj [E, H*C] is neither written nor read
            res = ops.gatv2_mp_edge_logits(x_l, x_r, edge_attr.float().contiguous(), self.lin_edge.weight, self.att, plan, H,
                                           want_rowmax=True, want_planes=out_planes, **kw)          # :215-232, :243-279
            if res is not None:
                return done(*res)
        if e_proj is None:
            if edge_attr is None or self.lin_edge is None:
                raise NotImplementedError("edge_attr=None: MGAT always passes edge features (mgat.py:147)")
            if edge_attr.dim() == 1:
                edge_attr = edge_attr.view(-1, 1)
            e_proj = ops.linear(edge_attr.float().contiguous(), self.lin_edge.weight, None, out_dtype=fdt)   # :259
        if drop:                                                                         # :274-279
            # seed: the layer's, as for its sampler; without one a draw from torch's CPU generator (no device sync, and
            # torch.manual_seed reproduces a run), as models/text_encoder._base_seed
            if seed is None and x_l.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("attention dropout inside a captured step needs an explicit seed per replay: a base drawn "
                                   "here is a kernel argument and would repeat in every replay")
            base = int(seed) if seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            return done(*ops.gatv2_mp(x_l, x_r, e_proj, self.att, plan, H, dropout_p=float(self.dropout),
                                      dropout_seed=base + ATTN_DROPOUT_SEED_OFFSET, **kw))
        return done(*ops.gatv2_mp(x_l, x_r, e_proj, self.att, plan, H, want_rowmax=not torch.is_grad_enabled(),
                                  want_planes=out_planes and not torch.is_grad_enabled(), **kw))          # :215-232

    def _project_split(self, x: Tensor, split, fdt):
        """x_l, x_r of cat(x, instruction[batch]) as ONE launch over the fused [N, 2 H C] projection (one [N, H C] projection with
        share_weights): P = instruction . [W_l[:, C:]; W_r[:, C:]]^T + [b_l; b_r] is [B, 2 H C], one bias row per graph, and the
        N-row GEMM runs at K = C.  Training: the parameters stay ONE tensor each in the reference's layout -- the fused weight is
        their stack, sliced by column, and torch's slicing carries the gradients of both halves back."""
        ins, seg, ptr = split
        C, lins = x.size(1), ([self.lin_l] if self.share_weights else [self.lin_l, self.lin_r])
        has_bias = lins[0].bias is not None

        def fused():
            w = lins[0].weight if len(lins) == 1 else torch.stack([m.weight for m in lins]).flatten(0, 1)
            b = None if not has_bias else (lins[0].bias if len(lins) == 1 else torch.stack([m.bias for m in lins]).flatten())
            return w, b

        srcs = [m.weight for m in lins] + ([m.bias for m in lins] if has_bias else [])
        if torch.is_grad_enabled() and ops._rec(x, ins, *srcs):
            w, b = fused()
            w_x, w_u = w[:, :C], w[:, C:].contiguous()
        else:
            def build():
                w, b = fused()
                return w[:, :C].contiguous(), w[:, C:].contiguous(), None if b is None else b.detach().contiguous()
            w_x, w_u, b = ops.derived_weight("concat_split", srcs, build)
        y = ops.linear_rowbias(x, w_x, ops.linear(ins, w_u, b), seg, out_dtype=fdt, rowptr=ptr)
        HC = self.heads * self.out_channels
        return (y, y) if self.share_weights else (y[:, :HC], y[:, HC:])

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"
