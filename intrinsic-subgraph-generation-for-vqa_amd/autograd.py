"""Training of the hot path: autograd wiring around the HIP kernels.

`ops.*` dispatch here when autograd is recording and an input requires grad; inside a Function's forward autograd is
off, so the same `ops.*` call runs the plain forward kernel.  Three kinds of backward:

  * hand-written HIP kernels for the operators the reference differentiates by hand or that dominate the step:
      GatV2MP            isg_gatv2_mp_bwd            (PyG propagate autograd behind mgat_v2_conv.py:215-279)
      NodeToEdgeMask     isg_node_to_edge_mask_bwd   (NodeMaskToEdgeMask.backward, sampling/node_edge_masks.py:13-19)
      GumbelTopK         isg_topk_gumbel_bwd         (straight-through, gumbel_scheme.py:83-90)
      ImleTopK/AimleTopK isg_topk_threshold again    (second MAP solve, wrapper.py:124-172; aimle.py:141-243;
                                                      adaptive beta, target_aimle.py:88-162 -- state kept ON THE DEVICE)
      SimpleTopK         isg_simple_topk_bwd         (the exact marginals' reverse pass over the circuit's two trees, one launch;
                                                      autograd through simple.py:203-236 in the reference)
  * Linear: forward and dX on the bf16x6 matrix-core kernel, dW (a reduction over the rows) as a split-M GEMM on the
    fp32 matrix-core instruction (csrc/isg_wgrad.hip);
  * the per-graph operators around the message passing -- layer tail (instruction attention + GraphNorm + residual),
    pooling, instruction gate, node gate: per-graph HIP backward kernels (csrc/isg_tail_bwd.hip);
  * the scene-graph encoder's operators -- gather-add, the node tokens' embedding sum, scatter_mean, GraphNorm alone (both modes):
    HIP backward kernels of their own (csrc/isg_sgenc_bwd.hip); every scatter among them is one segment sum without atomics;
  * what only stand-alone utilities use (scatter attention alone, gates without a plan), and a SIMPLE sampler row too long for the
    backward kernel's LDS rule: forward = fused kernel, backward re-evaluates a torch-op restatement ON THE DEVICE under autograd
    (`_Recomputed`).

Nothing here runs on the CPU and nothing imports `oracle/`.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from . import ops


# ------------------------------------------------------------------------------------------------
# Generic: fused forward, recomputed torch backward
# ------------------------------------------------------------------------------------------------
def _restated_grads(restate, tensors, need, gouts):
    """One gradient (or None) per tensor: autograd through restate(*tensors), a torch-op restatement of a fused forward,
    evaluated again on detached copies.  need: which tensors want a gradient; gouts: the upstream gradient of each of the
    restatement's outputs, None where there is none."""
    with torch.enable_grad():
        ins = [None if t is None else (t.detach().requires_grad_(True) if n else t.detach())
               for t, n in zip(tensors, need)]
        outs = restate(*ins)
        outs = outs if isinstance(outs, tuple) else (outs,)
        pairs = [(o, g) for o, g in zip(outs, gouts) if g is not None and o.requires_grad]
        wanted = [i for i, n in zip(ins, need) if n]
        grads = torch.autograd.grad([o for o, _ in pairs], wanted, [g for _, g in pairs], allow_unused=True)
    it = iter(grads)
    return tuple(next(it) if n else None for n in need)


class _Recomputed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fused, restate, consts, *tensors):
        ctx.restate, ctx.consts = restate, consts
        ctx.save_for_backward(*tensors)
        out = fused(*tensors, *consts)
        return out

    @staticmethod
    def backward(ctx, *gouts):
        restate, consts = ctx.restate, ctx.consts
        return (None, None, None) + _restated_grads(lambda *ins: restate(*ins, *consts), ctx.saved_tensors,
                                                    ctx.needs_input_grad[3:], gouts)


def _seg_sum(v: Tensor, batch: Tensor, B: int) -> Tensor:
    return torch.zeros((B,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device).index_add_(0, batch, v)


def _seg_softmax(logits: Tensor, batch: Tensor, B: int, eps: float = 0.0) -> Tensor:
    m = torch.full((B,), -math.inf, dtype=logits.dtype, device=logits.device)
    m = m.scatter_reduce(0, batch, logits.detach(), "amax", include_self=True)
    e = (logits - m[batch]).exp()
    return e / (_seg_sum(e, batch, B)[batch] + eps)


def _instr_gate_t(x, instr, batch):
    return F.gelu(x * instr[batch])


class _InstrGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, instr, batch, plan):
        ctx.save_for_backward(x, instr)
        ctx.plan = plan
        return ops.instr_gate(x, instr, batch)

    @staticmethod
    def backward(ctx, g):
        x, instr = ctx.saved_tensors
        d_x, d_instr = ops.instr_gate_backward(x, instr, ctx.plan, g.contiguous())
        return d_x, d_instr, None, None


def instr_gate(x, instr, batch, plan=None):
    if plan is not None and instr.size(0) == plan.B:
        return _InstrGate.apply(x, instr, batch, plan)
    return _Recomputed.apply(ops.instr_gate, _instr_gate_t, (batch,), x, instr)


def _node_gate_t(xn, q, batch, double_index):
    idx = batch[batch] if double_index else batch
    return F.gelu((xn * q[idx]).sum(-1, keepdim=True) / math.sqrt(xn.size(1)))


class _NodeGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xn, q, batch, double_index, plan):
        ctx.save_for_backward(xn, q, batch)
        ctx.cfg = (double_index, plan)
        return ops.node_gate(xn, q, batch, double_index)

    @staticmethod
    def backward(ctx, g):
        xn, q, batch = ctx.saved_tensors
        double_index, plan = ctx.cfg
        d_xn, d_q = ops.node_gate_backward(xn, q, batch, double_index, plan, g.contiguous())
        return d_xn, d_q, None, None, None


def node_gate(xn, q, batch, double_index, plan=None):
    if plan is not None:
        return _NodeGate.apply(xn, q, batch, double_index, plan)
    return _Recomputed.apply(ops.node_gate, _node_gate_t, (batch, double_index), xn, q)


def _graph_norm_t(v, weight, bias, mean_scale, batch, B, eps, fp64):
    dt = v.dtype
    if fp64:
        v, weight, bias, mean_scale = v.double(), weight.double(), bias.double(), mean_scale.double()
    cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(v.dtype).unsqueeze(1)
    mean = _seg_sum(v, batch, B) / cnt
    out = v - mean[batch] * mean_scale
    var = _seg_sum(out * out, batch, B) / cnt
    return (weight * out / (var + eps).sqrt()[batch] + bias).to(dt)


def _layer_tail_t(ins, c, h, weight, bias, mean_scale, node_mask, batch, B, eps):
    att = _seg_softmax((ins[batch] * c).sum(-1) / math.sqrt(c.size(1)), batch, B)
    y = _graph_norm_t(att.unsqueeze(1) * c, weight, bias, mean_scale, batch, B, eps, False) + h
    return y if node_mask is None else node_mask.view(-1, 1) * y


class _LayerTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ins, c, h, weight, bias, mean_scale, node_mask, plan, eps):
        ctx.save_for_backward(ins, c, h, weight, bias, mean_scale, node_mask)
        ctx.cfg = (plan, eps)
        return ops.mgat_layer_tail(ins, c, h, plan, weight, bias, mean_scale, eps, node_mask=node_mask)

    @staticmethod
    def backward(ctx, g):
        ins, c, h, weight, bias, mean_scale, node_mask = ctx.saved_tensors
        plan, eps = ctx.cfg
        want_mask = node_mask is not None and ctx.needs_input_grad[6]
        d_ins, d_c, d_h, d_w, d_b, d_ms, d_m = ops.layer_tail_backward(
            ins, c, h, plan, weight, bias, mean_scale, eps, node_mask, g.contiguous(), want_mask)
        return d_ins, d_c, d_h, d_w, d_b, d_ms, (d_m.view_as(node_mask) if want_mask else None), None, None


def mgat_layer_tail(ins, c, h, plan, weight, bias, mean_scale, eps, node_mask):
    return _LayerTail.apply(ins, c, h, weight, bias, mean_scale, node_mask, plan, eps)


def _pool_t(xn, q, node_mask, batch, B):
    x = xn if node_mask is None else xn * node_mask.view(-1, 1)
    gate = _seg_softmax((x * q[batch]).sum(-1) / math.sqrt(x.size(1)), batch, B, 1e-16).unsqueeze(1)
    return _seg_sum(gate * x, batch, B), gate


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xn, q, node_mask, plan):
        ctx.save_for_backward(xn, q, node_mask)
        ctx.plan = plan
        ctx.set_materialize_grads(False)          # the gate output is usually unused: its gradient arrives as None
        return ops.global_attn_pool(xn, q, plan, node_mask)

    @staticmethod
    def backward(ctx, g_out, g_gate):
        xn, q, node_mask = ctx.saved_tensors
        if g_out is None:
            g_out = torch.zeros(ctx.plan.B, xn.size(1), dtype=xn.dtype, device=xn.device)
        want_mask = node_mask is not None and ctx.needs_input_grad[2]
        d_xn, d_q, d_m = ops.global_attn_pool_backward(xn, q, ctx.plan, node_mask, g_out.contiguous(),
                                                       None if g_gate is None else g_gate.contiguous(), want_mask)
        return d_xn, d_q, (d_m.view_as(node_mask) if want_mask else None), None


def global_attn_pool(xn, q, plan, node_mask):
    return _Pool.apply(xn, q, node_mask, plan)


class _GraphNorm(torch.autograd.Function):
    """ops.graph_norm with isg_graph_norm_bwd behind it, in the forward's mode (fp64: every intermediate a double).  Saved: the
    inputs; the statistics are recomputed per graph.  `_graph_norm_t` above stays as the restatement the tests compare against."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean_scale, plan, eps, fp64):
        ctx.save_for_backward(x, weight, mean_scale)
        ctx.cfg = (plan, eps, fp64)
        return ops.graph_norm(x, plan, weight, bias, mean_scale, eps, fp64)

    @staticmethod
    def backward(ctx, g):
        x, weight, mean_scale = ctx.saved_tensors
        plan, eps, fp64 = ctx.cfg
        d_x, d_w, d_b, d_ms = ops.graph_norm_bwd(x, plan, weight, mean_scale, eps, fp64, g.contiguous())
        return d_x, d_w, d_b, d_ms, None, None, None


def graph_norm(x, plan, weight, bias, mean_scale, eps, fp64):
    return _GraphNorm.apply(x.contiguous(), weight, bias, mean_scale, plan, eps, fp64)


def scatter_attention(query, key, plan, value):
    batch, B = plan.batch, plan.B

    def restate(qr, k, v, _p):
        att = _seg_softmax((qr[batch] * k).sum(-1) / math.sqrt(k.size(1)), batch, B)
        return att.unsqueeze(1) * v
    return _Recomputed.apply(lambda qr, k, v, p: ops.scatter_attention(qr, k, p, v), restate, (plan,), query, key, value)


class _ScatterMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, plan):
        ctx.plan = plan
        return ops.scatter_mean(msg, plan)

    @staticmethod
    def backward(ctx, g):
        return ops.scatter_mean_bwd(g.contiguous(), ctx.plan), None


def scatter_mean(msg, plan):
    return _ScatterMean.apply(msg, plan)


# ------------------------------------------------------------------------------------------------
# Training through shared scene encodings (include/ext/isg_instances_train.h)
# ------------------------------------------------------------------------------------------------
class _InstanceRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inst, x, e):
        ctx.inst = inst
        return inst.gather_rows(x, e)

    @staticmethod
    def backward(ctx, g_x, g_e):
        d_x, d_e = ops.instance_rows_backward(ctx.inst, g_x.contiguous(), g_e.contiguous())
        return None, d_x, d_e


def instance_rows(inst, x, e):
    """(x[inst.node_src], e[inst.edge_src]) of an ops.GraphInstances, one launch each way: forward isg_instance_rows, backward
    isg_instance_rows_bwd -- per distinct row the sum of its copies' gradient rows in ascending instance number, no atomics."""
    return _InstanceRows.apply(inst, x, e)


# ------------------------------------------------------------------------------------------------
# Scene-graph encoder without its concatenations (include/isg_sgenc_train.h)
# ------------------------------------------------------------------------------------------------
def _column_slice(t):
    """(base, first column) when `t` is a column slice t = base[:, c0:c0 + C] of a contiguous 2-D tensor, else None."""
    base = None if t is None else t._base
    if base is None or base.dim() != 2 or t.dim() != 2 or not base.is_contiguous() or t.stride() != base.stride() \
            or t.size(0) != base.size(0):
        return None
    c0 = t.storage_offset() - base.storage_offset()
    return (base, c0) if 0 <= c0 and c0 + t.size(1) <= base.size(1) else None


class _GatherAdd(torch.autograd.Function):
    """ops.gather_add with isg_gather_add_bwd and isg_segment_rows_sum behind it.  Saved: the inputs only; the pre-activation is
    evaluated again.  cols = (column of A, column of B or None): `a` is then the tensor A and B are column slices of, and ONE
    gradient goes back to it (its other columns zero) -- no zero-filled slice gradients for autograd to add up, as _MhaSmall has it
    for q, k, v.  T2 / sign2 (optional): a second tensor with T's VALUES that is only differentiated, its gradient the segment sum
    of dz weighted by sign2 instead of sign (the encoder's duplicate-sym rule, scene_graph_encoder.py)."""

    @staticmethod
    def forward(ctx, a, b, T, D, bias, T2, ia, ib, it, sign, sign2, gelu, cols, csrs):
        if cols is not None:
            A = a[:, cols[0]:cols[0] + cols[2]]
            B = None if cols[1] is None else a[:, cols[1]:cols[1] + cols[2]]
        else:
            A, B = a, b
        ctx.save_for_backward(a, b, T, D, bias, ia, ib, it, sign, sign2)
        ctx.cfg = (gelu, cols, csrs)
        return ops.gather_add(A, ia, B, ib, T, it, sign, D, bias, gelu=gelu)

    @staticmethod
    def backward(ctx, g):
        a, b, T, D, bias, ia, ib, it, sign, sign2 = ctx.saved_tensors
        gelu, cols, (csr_a, csr_b, csr_t) = ctx.cfg
        need = ctx.needs_input_grad
        if cols is not None:
            A = a[:, cols[0]:cols[0] + cols[2]]
            B = None if cols[1] is None else a[:, cols[1]:cols[1] + cols[2]]
        else:
            A, B = a, b
        E = ia.numel()
        dz, d_bias = ops.gather_add_bwd(A, ia, B, ib, T, it, sign, D, bias, gelu, g.contiguous(),
                                        want_bias=bias is not None and need[4])
        csr = lambda given, index, rows: given if given is not None else ops.token_csr(index, rows)
        d_a = d_b = d_T = d_T2 = None
        if cols is not None:
            if need[0]:
                covered = cols[2] * (1 if cols[1] is None else 2) == a.size(1)
                d_a = torch.empty_like(a) if covered else torch.zeros_like(a)
                ops.segment_rows_sum(*csr(csr_a, ia, a.size(0)), dz, out=d_a[:, cols[0]:cols[0] + cols[2]], M=E)
                if cols[1] is not None:
                    ops.segment_rows_sum(*csr(csr_b, ib, a.size(0)), dz, out=d_a[:, cols[1]:cols[1] + cols[2]], M=E)
        else:
            if need[0]:
                d_a = ops.segment_rows_sum(*csr(csr_a, ia, a.size(0)), dz, M=E)
            if b is not None and need[1]:
                d_b = ops.segment_rows_sum(*csr(csr_b, ib, b.size(0)), dz, M=E)
        if T is not None and (need[2] or need[5]):
            csr_t = csr(csr_t, it, T.size(0))
            if need[2]:
                d_T = ops.segment_rows_sum(*csr_t, dz, w=sign, M=E)
            if need[5]:
                d_T2 = ops.segment_rows_sum(*csr_t, dz, w=sign2, M=E)
        return (d_a, d_b, d_T, (dz if D is not None and need[3] else None), d_bias, d_T2, None, None, None, None, None, None,
                None, None)


def gather_add(A, ia, B=None, ib=None, T=None, it=None, sign=None, D=None, bias=None, gelu=False, csr_a=None, csr_b=None,
               csr_t=None, T2=None, sign2=None):
    """act(A[ia] + B[ib] + sign * T[it] + D + bias), differentiable in A, B, T, D and bias (sign and the indices get no gradient).
    csr_*: (rowptr int32, eid int32) of the index tensors where the caller has them; ops.token_csr builds the others.
    T2, sign2: see _GatherAdd."""
    if (T2 is None) != (sign2 is None) or (T2 is not None and (T is None or T2.shape != T.shape)):
        raise ValueError("gather_add: T2 and sign2 come together, beside a T of T2's shape")
    sa, sb = _column_slice(A), _column_slice(B)
    cols = None
    if sa is not None and (B is None or (sb is not None and sb[0] is sa[0])):
        cols = (sa[1], None if B is None else sb[1], A.size(1))
        if cols[1] is not None and abs(cols[1] - cols[0]) < cols[2]:
            cols = None                                   # overlapping slices: two gradients for autograd to add
    if cols is not None:
        return _GatherAdd.apply(sa[0], None, T, D, bias, T2, ia, ib, it, sign, sign2, gelu, cols, (csr_a, csr_b, csr_t))
    return _GatherAdd.apply(A, B, T, D, bias, T2, ia, ib, it, sign, sign2, gelu, None, (csr_a, csr_b, csr_t))


class _EmbeddingSum(torch.autograd.Function):
    """sum_t weight[idx[:, t]]: forward on the inference kernels (ops.embedding_sum), backward one segment sum over the tokens'
    CSR -- entry n * T + t reads row n of the gradient (gdiv = T), and row padding_idx is written as zeros."""

    @staticmethod
    def forward(ctx, weight, idx, padding_idx):
        ctx.save_for_backward(idx)
        ctx.cfg = (weight.size(0), padding_idx)
        return ops.embedding_sum(weight, idx, padding_idx)

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        V, padding_idx = ctx.cfg
        rowptr, eid = ops.token_csr(idx, V)
        return ops.segment_rows_sum(rowptr, eid, g.contiguous(), gdiv=idx.size(1), skip=padding_idx), None, None


def embedding_sum(weight, idx, padding_idx=None):
    if padding_idx is not None and padding_idx < 0:
        padding_idx += weight.size(0)
    return _EmbeddingSum.apply(weight, idx, padding_idx)


class _ZeroRowGrad(torch.autograd.Function):
    """The identity whose backward zeroes one row: an embedding matrix read as a whole (projected into a table) keeps its
    padding_idx row without gradient, as nn.Embedding's own lookup does."""

    @staticmethod
    def forward(ctx, weight, row):
        ctx.row = row
        return weight.view_as(weight)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[ctx.row].zero_()
        return g, None


def zero_row_grad(weight, row):
    return weight if row is None else _ZeroRowGrad.apply(weight, row)


# ------------------------------------------------------------------------------------------------
# Dense projection
# ------------------------------------------------------------------------------------------------
# g^T x through torch sums the rows of one output in a single fp32 chain: its error against float64 grows like
# sqrt(M) * 3.7e-8 of the largest entry (measured: 1.1e-6 at M = 2047, 2.3e-6 at 4095, 3.6e-6 at 16383 -- six to ten times the
# blocked fp32 sum of a CPU BLAS) and passes 2e-6 near M = 3000.  The split-M kernel sums M / splits rows per chain (32 at a time on the
# matrix core) and stays at 3e-7 to 6e-7 at every M.  Its time against hipBLASLt between 2 k and 16 k rows is NOT measured yet
# (`tools/time_wgrad.py --mid` times that range; at 4096 x 1842 x 512 it is 26 us slower, profiles/r01_o_wgrad_vs_hipblaslt.txt): the
# switch sits here for the error, not for the time.
WGRAD_MIN_ROWS = 2048
# The backward on csrc/isg_linear_bwd.hip (include/isg_linear_train.h): dz and db in one pass (ops.linear_bwd_prep) instead of
# aten.gelu_backward / g * (z > 0), g.sum(0) and g.contiguous(); dW on the bf16 matrix cores (ops.linear_wgrad_bf16x6) at
# M >= WGRAD_MIN_ROWS.  Off: every line runs as before.  On by DESIGN.md section 24's rule: the full training step at 4096
# questions takes 98.4 ms with it and 125.4 ms without (7 rounds each, spreads 0.3 ms, every round of one below every round of the
# other; profiles/r14_b_linear_bwd_ab.json).
LINEAR_BWD_KERNELS = True


def _linear_backward(g, x, weight, saved, mode, want_dx, want_dw, want_db, kernels):
    """(dz, dx, dW, db) of y = act(x W^T + b) from its upstream gradient g, whose rows may be strided (a column slice): the one
    place that knows a Linear's backward.  mode: ops.LINEAR_BWD_MODES -- 0 identity, 1 GELU (saved = the pre-activation), 2 ReLU
    (saved = its result).  kernels: dz and db in one pass of ops.linear_bwd_prep and dW on the bf16 matrix cores
    (csrc/isg_linear_bwd.hip); False: the torch passes and the fp32 split-M kernel of before.  The CALLER reads
    LINEAR_BWD_KERNELS and counts in ops.COUNTERS["linear_bwd_kernels"], so what each node does with the switch stands at its call."""
    db = None
    if kernels:
        if g.dim() != 2 or g.stride(1) != 1 or g.stride(0) < g.size(1):
            g = g.contiguous()
        if mode == 0:                   # identity: the bias gradient alone, g is not copied
            if want_db:
                db = ops.linear_bwd_prep(g, None, 0, want_dz=False, want_db=True)[1]
            if not g.is_contiguous():
                g = g.contiguous()
        else:
            g, db = ops.linear_bwd_prep(g, saved, mode, want_dz=True, want_db=want_db)
    else:
        g = g.contiguous()
        if mode == 1:
            g = torch.ops.aten.gelu_backward(g, saved)
        elif mode == 2:
            g = g * (saved > 0)
    dx = None
    if want_dx:                         # dX = g W: the same matrix-core kernel on the transposed weight
        dx = (ops.linear(g, weight.detach().t().contiguous(), None, cache_planes=False)
              if (g.size(1) & 3) == 0 else g @ weight)
    dw = None
    if want_dw:                         # long-and-thin reductions on a split-M kernel; short ones are hipBLASLt's home turf
        if g.size(0) < WGRAD_MIN_ROWS:
            dw = g.t() @ x
        else:
            dw = ops.linear_wgrad_bf16x6(g, x.contiguous()) if kernels else ops.linear_wgrad(g, x.contiguous())
    if want_db and not kernels:
        db = g.sum(0)
    return g, dx, dw, db


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b): forward on isg_linear_bf16x6 (pre-activation kept when act = GELU; ReLU fused into the kernel's epilogue
    and its RESULT kept: y > 0 is all the backward needs of it); backward on csrc/isg_linear_bwd.hip (LINEAR_BWD_KERNELS), or as
    fp32 GEMMs and torch passes with the switch off."""

    @staticmethod
    def forward(ctx, x, weight, bias, gelu, relu=False):
        z = ops.linear(x, weight, bias, gelu=False, cache_planes=False, relu=relu)
        ctx.mode = 1 if gelu else 2 if relu else 0
        ctx.save_for_backward(x, weight, z if gelu or relu else None)
        ctx.has_bias = bias is not None
        return F.gelu(z) if gelu else z

    @staticmethod
    def backward(ctx, g):
        x, weight, z = ctx.saved_tensors
        need = ctx.needs_input_grad
        if LINEAR_BWD_KERNELS:
            ops.COUNTERS["linear_bwd_kernels"] += 1
        _, dx, dw, db = _linear_backward(g, x, weight, z, ctx.mode, need[0], need[1], ctx.has_bias and need[2],
                                         kernels=LINEAR_BWD_KERNELS)
        return dx, dw, db, None, None


def linear(x, weight, bias, gelu, relu=False):
    if relu and gelu:
        raise ValueError("relu excludes gelu")
    return _Linear.apply(x, weight, bias, gelu, relu)


class _LinearRowBias(torch.autograd.Function):
    """y = act(x W^T + P[seg]) (ops.linear_rowbias, include/isg_concat.h), in the mould of _Linear: the forward keeps the
    pre-activation when an activation follows; the backward is _linear_backward's without a bias sum, and dP[s] = the sum of dz
    over segment s's rows -- contiguous ranges, summed in row order by ops.segment_range_sum without atomics, so two calls agree
    bit for bit.  It runs the kernel path whatever LINEAR_BWD_KERNELS says and does not count in "linear_bwd_kernels"."""

    @staticmethod
    def forward(ctx, x, weight, P, seg, gelu, relu, rowptr):
        z = ops.linear_rowbias(x, weight, P, seg, relu=relu, cache_planes=False)
        ctx.mode, ctx.S = 1 if gelu else 2 if relu else 0, P.size(0)
        ctx.save_for_backward(x, weight, z if gelu or relu else None, seg, rowptr)
        return F.gelu(z) if gelu else z

    @staticmethod
    def backward(ctx, g):
        x, weight, z, seg, rowptr = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz, dx, dw, _ = _linear_backward(g, x, weight, z, ctx.mode, need[0], need[1], False, kernels=True)
        dp = None
        if need[2]:
            if rowptr is None:
                rowptr = ops.segment_rowptr(seg, ctx.S)
            dp = ops.segment_range_sum(rowptr, dz)
        return dx, dw, dp, None, None, None, None


def linear_rowbias(x, weight, P, seg, gelu=False, relu=False, rowptr=None):
    """ops.linear_rowbias under autograd; that entry has checked the operands (relu excludes gelu among them)."""
    return _LinearRowBias.apply(x, weight, P, seg, gelu, relu, rowptr)


# ------------------------------------------------------------------------------------------------
# The loss (include/isg_optim.h)
# ------------------------------------------------------------------------------------------------
class _CrossEntropy(torch.autograd.Function):
    """ops.cross_entropy with isg_xent_bwd behind it.  Saved: the logits, the labels, the rows' log-sum-exp and the counts; the
    probabilities are recomputed.  The upstream gradient reaches the kernel as the device scalar it is."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, totals):
        r = ops.cross_entropy(logits, labels, ignore_index, totals)
        ctx.ignore_index = ignore_index
        ctx.save_for_backward(logits, labels, r.lse, r.stats)
        ctx.mark_non_differentiable(r.pred, r.row_loss, r.stats, r.lse)
        return tuple(r)

    @staticmethod
    def backward(ctx, g, *_):
        logits, labels, lse, stats = ctx.saved_tensors
        return ops.cross_entropy_backward(logits, labels, lse, stats, g.float().contiguous(), ctx.ignore_index), None, None, None


def cross_entropy(logits, labels, ignore_index=-100, totals=None):
    return ops.CrossEntropy(*_CrossEntropy.apply(logits, labels, ignore_index, totals))


# ------------------------------------------------------------------------------------------------
# Question side: short-sequence attention, add + LayerNorm, dropout (include/isg_train.h)
# ------------------------------------------------------------------------------------------------
# No dropout mask is stored: a Function keeps its inputs and the seed, and its backward kernel draws the mask again from
# (seed, position) -- the keep rule of include/isg_train.h.
class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.cfg = (p, seed)
        return ops.dropout(x, p, seed)

    @staticmethod
    def backward(ctx, g):
        p, seed = ctx.cfg
        return ops.dropout(g.contiguous(), p, seed), None, None


def dropout(x, p, seed):
    """x * keep / (1 - p), the mask a function of (seed, position); the identity at p == 0."""
    return x if p == 0 else _Dropout.apply(x, p, seed)


def _packed(parts):
    """The tensor that `parts` are the consecutive equal column slices of (q | k | v of a fused in_proj, k | v of the memory's),
    or None.  The Function then takes THAT tensor and returns ONE gradient for it: no zero-filled slice gradients to add up."""
    base = parts[0]._base
    if base is None or base.dim() != 2 or not base.is_contiguous() or any(t._base is not base for t in parts):
        return None
    D = parts[0].size(1)
    if base.size(1) != D * len(parts):
        return None
    for i, t in enumerate(parts):
        if tuple(t.shape) != (base.size(0), D) or t.stride() != base.stride() or t.storage_offset() != base.storage_offset() + i * D:
            return None
    return base


class _MhaSmall(torch.autograd.Function):
    """layout "qkv": one [T*B, 3D] tensor; "q_kv": q and one [S*B, 2D] tensor; "sep": q, k, v."""

    @staticmethod
    def forward(ctx, a, b, c, layout, B, H, key_bias, p, seed):
        D = a.size(1) // 3 if layout == "qkv" else a.size(1)
        if layout == "qkv":
            q, k, v = a[:, :D], a[:, D:2 * D], a[:, 2 * D:]
        elif layout == "q_kv":
            q, k, v = a, b[:, :D], b[:, D:]
        else:
            q, k, v = a, b, c
        ctx.save_for_backward(a, b, c, key_bias)
        ctx.cfg = (layout, B, H, D, p, seed)
        return ops.mha_small(q, k, v, B, H, key_bias) if p == 0 else ops.mha_small_train(q, k, v, B, H, key_bias, p, seed)

    @staticmethod
    def backward(ctx, g):
        a, b, c, key_bias = ctx.saved_tensors
        layout, B, H, D, p, seed = ctx.cfg
        g = g.contiguous()
        if layout == "qkv":
            da, db, dc = torch.empty_like(a), None, None
            q, k, v, dq, dk, dv = a[:, :D], a[:, D:2 * D], a[:, 2 * D:], da[:, :D], da[:, D:2 * D], da[:, 2 * D:]
        elif layout == "q_kv":
            da, db, dc = torch.empty_like(a), torch.empty_like(b), None
            q, k, v, dq, dk, dv = a, b[:, :D], b[:, D:], da, db[:, :D], db[:, D:]
        else:
            da, db, dc = (torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in (a, b, c))
            q, k, v, dq, dk, dv = a, b, c, da, db, dc
        if not ops.mha_small_backward(q, k, v, B, H, key_bias, g, dq, dk, dv, p, seed):
            raise ops._lib.IsgError("isg_mha_small_bwd refused a shape autograd.mha_small had asked ops.mha_small_train_supported about")
        return da, db, dc, None, None, None, None, None, None


def _mha_torch(q, k, v, B, H, key_bias, p):
    """Beyond the kernels' limits: the same formula on torch's ops (its own dropout stream), counted."""
    ops.COUNTERS["torch_attention_train"] += 1
    D = q.size(1)
    hd = D // H
    Tq, Tk = q.size(0) // B, k.size(0) // B
    heads = lambda t, T: t.reshape(T, B, H, hd).permute(1, 2, 0, 3)          # [B, H, T, hd]
    s = heads(q, Tq) @ heads(k, Tk).transpose(-1, -2) / math.sqrt(hd)
    if key_bias is not None:
        s = s + key_bias[:, None, None, :]
    pr = F.dropout(torch.softmax(s, dim=-1), p, training=p > 0)
    return (pr @ heads(v, Tk)).permute(2, 0, 1, 3).reshape(Tq * B, D)


def mha_small(q, k, v, B, H, key_bias=None, p=0.0, seed=0):
    """softmax(Q K^T / sqrt(hd) + key_bias) V with dropout p on the probabilities, differentiable in q, k, v (ops.mha_small's
    operands; key_bias gets no gradient and must not require one).  Saves q, k, v and the seed."""
    if key_bias is not None and key_bias.requires_grad:
        raise NotImplementedError("autograd.mha_small: key_bias has no gradient here; detach it")
    D = q.size(1)
    if not ops.mha_small_train_supported(q.size(0) // B, k.size(0) // B, D // H) or D % H:
        return _mha_torch(q, k, v, B, H, key_bias, p)
    base = _packed((q, k, v))
    if base is not None:
        return _MhaSmall.apply(base, None, None, "qkv", B, H, key_bias, p, seed)
    base = _packed((k, v))
    if base is not None:
        return _MhaSmall.apply(q, base, None, "q_kv", B, H, key_bias, p, seed)
    return _MhaSmall.apply(q, k, v, "sep", B, H, key_bias, p, seed)


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, norm, p, seed):
        ctx.save_for_backward(x, residual)
        ctx.cfg = (norm, p, seed)
        if p == 0:
            return ops.add_layernorm(x, residual, norm, want_rowmax=False)
        return ops.dropout_add_layernorm(x, residual, norm, p, seed)

    @staticmethod
    def backward(ctx, g):
        x, residual = ctx.saved_tensors
        norm, p, seed = ctx.cfg
        d_x, d_r, d_g, d_b = ops.add_layernorm_backward(x, residual, norm, g.contiguous(), p, seed,
                                                        want_residual=residual is not None and ctx.needs_input_grad[1])
        return d_x, d_r, d_g, d_b, None, None, None


def add_layernorm_supported(D: int) -> bool:
    return D % 4 == 0 and D <= 2048


def add_layernorm(x, residual, norm, p=0.0, seed=0):
    """LayerNorm(residual + dropout(x)), differentiable in x, residual and the norm's weight / bias (which the Function receives
    as inputs so that autograd hands them their gradients; the kernels read them from `norm`)."""
    if not add_layernorm_supported(x.size(1)):
        ops.COUNTERS["torch_layer_norm"] += 1
        y = F.dropout(x, p, training=p > 0)
        return F.layer_norm(y if residual is None else y + residual, norm.normalized_shape, norm.weight, norm.bias, norm.eps)
    return _AddLayerNorm.apply(x.contiguous(), None if residual is None else residual.contiguous(), norm.weight, norm.bias, norm, p, seed)


# ------------------------------------------------------------------------------------------------
# Message passing and the node -> edge mask
# ------------------------------------------------------------------------------------------------
def _mask_grad_wanted(node_mask, edge_mask, need_node, need_edge):
    return (node_mask is not None and need_node) or (edge_mask is not None and need_edge)


def _mask_grads(d_m, node_mask, edge_mask, plan, need_node, need_edge):
    """(d_node_mask, d_edge_mask) from the message passing's d_m [E], the gradient of the mask each edge was scaled by."""
    if not _mask_grad_wanted(node_mask, edge_mask, need_node, need_edge):
        return None, None
    if node_mask is not None:                         # the fused mask[src]*mask[dst] product keeps the reference's rule
        return ops.node_to_edge_mask_backward(d_m, plan).view_as(node_mask), None
    return None, d_m.view_as(edge_mask)


class _GatV2MP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_l, x_r, e_proj, att, bias, node_mask, edge_mask, plan, heads, slope, kernel, drop_p=0.0, drop_seed=0):
        out, alpha = ops.gatv2_mp(x_l, x_r, e_proj, att, plan, heads, bias=bias, node_mask=node_mask,
                                  edge_mask=edge_mask, negative_slope=slope, kernel=kernel, dropout_p=drop_p,
                                  dropout_seed=drop_seed)
        ctx.save_for_backward(x_l, x_r, e_proj, att, alpha, node_mask, edge_mask)
        ctx.cfg = (plan, heads, slope, bias is not None)
        ctx.drop = (drop_p, drop_seed)        # no mask is kept: the backward draws it again from (seed, edge id, head)
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, g_out, _g_alpha):
        x_l, x_r, e_proj, att, alpha, node_mask, edge_mask = ctx.saved_tensors
        plan, heads, slope, has_bias = ctx.cfg
        need = ctx.needs_input_grad
        d_xl, d_xr, d_e, d_att, d_bias, d_m = ops.gatv2_mp_backward(
            x_l, x_r, e_proj, att, alpha, g_out, plan, heads, node_mask=node_mask, edge_mask=edge_mask,
            negative_slope=slope, want_mask_grad=_mask_grad_wanted(node_mask, edge_mask, need[5], need[6]),
            dropout_p=ctx.drop[0], dropout_seed=ctx.drop[1])
        d_node, d_edge = _mask_grads(d_m, node_mask, edge_mask, plan, need[5], need[6])
        return (d_xl, d_xr, d_e, d_att.view_as(att), d_bias if has_bias else None, d_node, d_edge,
                None, None, None, None, None, None)


def gatv2_mp(x_l, x_r, e_proj, att, plan, heads, bias, node_mask, edge_mask, negative_slope, kernel, dropout_p=0.0, dropout_seed=0):
    return _GatV2MP.apply(x_l, x_r, e_proj, att, bias, node_mask, edge_mask, plan, heads, negative_slope, kernel, dropout_p,
                          dropout_seed)


class _ConvHalfRows(torch.autograd.Function):
    """One GATv2 layer's projections, message passing and output rounding on fp16 feature rows (MaskingGATv2Conv.feature_dtype =
    torch.float16, BASELINE configs[4]) as ONE node of the autograd graph, fp32 at every differentiable input and output.

    A half tensor must never be an edge of the graph: the engine casts a gradient to the dtype of the tensor it belongs to, and a
    gradient rounded to half flushes below 6e-8.  So x_l | x_r, e_proj and the half `out` live inside this Function only.
    Rule: each of the four roundings (x_l, x_r, e_proj, out) has derivative 1 -- what is differentiated is the fp32 function
    evaluated AT the rounded rows, the rows the forward kernels read.
    Forward: ops.linear(out_dtype=half) twice (lin_l | lin_r as one [N, 2 H C] projection; lin_edge), isg_gatv2_mp_fwd_f16 on the
    half slices, out.float().  Backward: isg_gatv2_mp_bwd_f16 on the saved half rows, d_x_l | d_x_r written into one [N, 2 H C]
    buffer that IS the fused projection's upstream gradient, then the Linear backwards as _Linear makes them."""

    @staticmethod
    def forward(ctx, x, edge_attr, w_l, b_l, w_r, b_r, w_e, att, bias, node_mask, edge_mask, plan, heads, slope):
        shared = w_r is None
        w, b = (w_l, b_l) if shared else ops.fused_weight((w_l, w_r), (b_l, b_r))
        x_lr = ops.linear(x, w, b, out_dtype=torch.float16, cache_planes=False)
        e_half = ops.linear(edge_attr, w_e, None, out_dtype=torch.float16, cache_planes=False)
        HC = w_l.size(0)
        x_l, x_r = (x_lr, x_lr) if shared else (x_lr[:, :HC], x_lr[:, HC:])
        out, alpha = ops.gatv2_mp(x_l, x_r, e_half, att, plan, heads, bias=bias, node_mask=node_mask, edge_mask=edge_mask,
                                  negative_slope=slope)
        ctx.save_for_backward(x, edge_attr, w_l, b_l, w_r, b_r, w_e, att, x_lr, e_half, alpha, node_mask, edge_mask)
        ctx.cfg = (plan, heads, slope, bias is not None)
        ctx.mark_non_differentiable(alpha)
        return out.float(), alpha

    @staticmethod
    def backward(ctx, g_out, _g_alpha):
        x, edge_attr, w_l, b_l, w_r, b_r, w_e, att, x_lr, e_half, alpha, node_mask, edge_mask = ctx.saved_tensors
        plan, heads, slope, has_bias = ctx.cfg
        need = ctx.needs_input_grad
        shared = w_r is None
        HC = w_l.size(0)
        N = x.size(0)
        x_l, x_r = (x_lr, x_lr) if shared else (x_lr[:, :HC], x_lr[:, HC:])
        buf = None if shared else torch.empty(N, 2 * HC, dtype=torch.float32, device=x.device)
        d_xl, d_xr, d_e, d_att, d_bias, d_m = ops.gatv2_mp_backward_f16(
            x_l, x_r, e_half, att, alpha, g_out, plan, heads, node_mask=node_mask, edge_mask=edge_mask, negative_slope=slope,
            want_mask_grad=_mask_grad_wanted(node_mask, edge_mask, need[9], need[10]), d_x_lr=buf)
        g = d_xl + d_xr if shared else buf
        w = w_l.detach() if shared else ops.fused_weight((w_l.detach(), w_r.detach()), (None, None))[0]
        want_b = (b_l is not None and need[3]) or (b_r is not None and need[5])
        kernels = LINEAR_BWD_KERNELS                    # two Linears without an activation, each counted as _Linear counts one
        ops.COUNTERS["linear_bwd_kernels"] += int(kernels)
        _, dx, dw, db = _linear_backward(g, x, w, None, 0, need[0], need[2] or need[4], want_b, kernels=kernels)
        ops.COUNTERS["linear_bwd_kernels"] += int(kernels)
        _, d_ea, d_we, _ = _linear_backward(d_e, edge_attr, w_e.detach(), None, 0, need[1], need[6], False, kernels=kernels)
        half = lambda t, lo: None if t is None else t[lo:lo + HC]
        d_node, d_edge = _mask_grads(d_m, node_mask, edge_mask, plan, need[9], need[10])
        return (dx, d_ea, half(dw, 0) if need[2] else None, half(db, 0) if b_l is not None and need[3] else None,
                half(dw, HC) if not shared and need[4] else None, half(db, HC) if b_r is not None and need[5] else None,
                d_we, d_att.view_as(att) if need[7] else None, d_bias if has_bias and need[8] else None, d_node, d_edge,
                None, None, None)


def conv_half_rows(x, edge_attr, lin_l, lin_r, w_edge, att, bias, node_mask, edge_mask, plan, heads, negative_slope):
    """(out fp32 [N, H*C] holding half-rounded values, alpha [E, H]) of a GATv2 layer trained on fp16 feature rows.  lin_l / lin_r:
    modules with .weight and .bias; lin_r None or lin_l itself: the layer shares its weights (g = d_x_l + d_x_r)."""
    shared = lin_r is None or lin_r is lin_l
    return _ConvHalfRows.apply(x, edge_attr, lin_l.weight, lin_l.bias, None if shared else lin_r.weight,
                               None if shared else lin_r.bias, w_edge, att, bias, node_mask, edge_mask, plan, heads,
                               negative_slope)


class _NodeToEdgeMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask, edge_index, plan):
        ctx.plan = plan
        ctx.shape = mask.shape
        return ops.node_to_edge_mask(mask, edge_index)

    @staticmethod
    def backward(ctx, g):
        return ops.node_to_edge_mask_backward(g.contiguous(), ctx.plan).view(ctx.shape), None, None


def node_to_edge_mask(mask, edge_index, plan):
    return _NodeToEdgeMask.apply(mask, edge_index, plan)


# ------------------------------------------------------------------------------------------------
# Samplers
# ------------------------------------------------------------------------------------------------
class _GumbelTopK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, k, tau, plan, noise, seed, k_cap):
        ctx.save_for_backward(scores, noise)
        ctx.cfg = (k, tau, plan, seed, k_cap)          # k: an int, or the int32 [B] budget (no gradient, not written after)
        return ops.topk_gumbel(scores, k, tau, plan=plan, noise=noise, seed=seed, k_cap=k_cap)

    @staticmethod
    def backward(ctx, g):
        scores, noise = ctx.saved_tensors
        k, tau, plan, seed, k_cap = ctx.cfg
        return (ops.topk_gumbel_backward(scores, g, k, tau, plan=plan, noise=noise, seed=seed, k_cap=k_cap),) + (None,) * 6


def topk_gumbel(scores, k, tau, plan, noise, seed, k_cap=None):
    """``k``: an int, or a k per row (int32 [B] device tensor) with ``k_cap`` the bound of its entries."""
    return _GumbelTopK.apply(scores, k, tau, plan, noise, seed, k_cap)


# The SIMPLE marginals' backward on csrc/isg_simple_bwd.hip (one launch).  False: autograd through the torch restatement of the
# circuit (`_Recomputed`, a few thousand launches per call), which also takes the rows the kernel's LDS rule refuses.  A/B:
# tools/time_simple_bwd.py, DESIGN.md 25.
SIMPLE_BWD_KERNEL = True


def _simple_restatement(scores, k, plan, return_marginals):
    """The differentiable part of simple_topk written with torch ops: (out [, marginals]) = the marginals in both layouts."""
    from .sampling.methods.simple import LARGE_NUMBER, log_marginals
    if plan is not None:                               # the forward's row length: the true longest row under a max_nodes hint too
        B, nmax, slots = plan.B, plan.true_nmax("the SIMPLE sampler"), plan.dense_slots()
        if nmax != plan.nmax:
            slots = slots - plan.batch * (plan.nmax - nmax)
    else:
        B, nmax, slots = scores.shape[0], scores.shape[1], None
    n = 1 << max(nmax - 1, 0).bit_length()
    kk = min(int(k), nmax)

    def restate(sc, *_c):
        if slots is not None:
            dense = torch.zeros(B * nmax, dtype=sc.dtype, device=sc.device).index_put((slots,), sc.reshape(-1)).view(B, nmax)
        else:
            dense = sc.reshape(B, nmax)
        flat = torch.cat([dense, torch.full((B, n - nmax), -LARGE_NUMBER, dtype=sc.dtype, device=sc.device)], dim=1)
        marg = log_marginals(flat, kk).exp()[:, :nmax]
        out = marg.reshape(-1)[slots].view(sc.shape) if slots is not None else marg.view(sc.shape)
        return (out, marg) if return_marginals else out

    return restate


class _SimpleTopK(torch.autograd.Function):
    """out = (sample - marginals).detach() + marginals: only the marginals are differentiable and the sample carries no gradient,
    so the backward needs the scores alone."""

    @staticmethod
    def forward(ctx, scores, k, plan, uniform, seed, return_marginals):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(scores)
        ctx.cfg = (k, plan, return_marginals)
        return ops.simple_topk(scores, k, plan, uniform, seed, return_marginals)

    @staticmethod
    def backward(ctx, g_out, g_marg=None):
        scores, = ctx.saved_tensors
        k, plan, return_marginals = ctx.cfg
        if g_out is None and g_marg is None:
            return (None,) * 6
        d = ops.simple_topk_backward(scores, k, plan, None if g_out is None else g_out.contiguous(),
                                     None if g_marg is None else g_marg.contiguous())
        if d is None:                                   # a row beyond the kernel's LDS rule: the restatement, as with the switch off
            d, = _restated_grads(_simple_restatement(scores, k, plan, return_marginals), (scores,), (True,), (g_out, g_marg))
        return (d,) + (None,) * 5


def simple_topk(scores, k, plan, uniform, seed, return_marginals):
    """forward = isg_simple_topk; backward = isg_simple_topk_bwd, the reverse pass over the circuit's trees as one launch, or --
    SIMPLE_BWD_KERNEL off, or a row the kernel refuses -- autograd over the torch restatement of the circuit's marginals (the only
    differentiable part: out = (sample - marginals).detach() + marginals)."""
    if SIMPLE_BWD_KERNEL:
        return _SimpleTopK.apply(scores, k, plan, uniform, seed, return_marginals)

    def fused(sc, *_c):
        return ops.simple_topk(sc, k, plan, uniform, seed, return_marginals)

    return _Recomputed.apply(fused, _simple_restatement(scores, k, plan, return_marginals), (), scores)


class _ImleTopK(torch.autograd.Function):
    """z = MAP(theta + tau_in * eps);  d theta = z - MAP(alpha * theta - beta * dy + tau_t * eps)."""

    @staticmethod
    def forward(ctx, scores, k, plan, noise, seed, alpha, beta, tau_in, tau_target, k_cap):
        z = ops.topk_threshold(scores, k, plan=plan, noise=noise, noise_scale=tau_in, seed=seed, k_cap=k_cap)
        ctx.save_for_backward(scores, noise, z)
        ctx.cfg = (k, plan, seed, alpha, beta, tau_target, k_cap)
        return z

    @staticmethod
    def backward(ctx, dy):
        scores, noise, z = ctx.saved_tensors
        k, plan, seed, alpha, beta, tau_target, k_cap = ctx.cfg
        target = alpha * scores - beta * dy                                              # target.py:43
        z_t = ops.topk_threshold(target.contiguous(), k, plan=plan, noise=noise, noise_scale=tau_target, seed=seed, k_cap=k_cap)
        return (z - z_t,) + (None,) * 9                                                  # wrapper.py:170-172 (S = 1)


class AdaptiveTarget:
    """AdaptiveTargetDistribution (target_aimle.py:88-162) with beta / grad_norm as 0-dim DEVICE tensors, so the
    backward never synchronises (the reference calls .item() three times per backward)."""

    def __init__(self, initial_alpha: float = 1.0, initial_beta: float = 1.0, initial_grad_norm: float = 1.0,
                 beta_update_step: float = 0.0001, beta_update_momentum: float = 0.0, grad_norm_decay_rate: float = 0.9,
                 target_norm: float = 1.0):
        self.alpha = initial_alpha
        self._beta0, self._gn0 = float(initial_beta), float(initial_grad_norm)
        self.beta_t: Optional[Tensor] = None        # float64, like the reference's Python float
        self.grad_norm_t: Optional[Tensor] = None   # float32
        self.prev_update_t: Optional[Tensor] = None
        self.beta_update_step, self.beta_update_momentum = beta_update_step, beta_update_momentum
        self.grad_norm_decay_rate, self.target_norm = grad_norm_decay_rate, target_norm

    def _init(self, device):
        if self.beta_t is None or self.beta_t.device != device:
            self.beta_t = torch.tensor(self._beta0, dtype=torch.float64, device=device)
            self.grad_norm_t = torch.tensor(self._gn0, dtype=torch.float32, device=device)
            self.prev_update_t = torch.zeros((), dtype=torch.float64, device=device)

    @property
    def beta(self) -> float:
        return self._beta0 if self.beta_t is None else float(self.beta_t)

    @property
    def grad_norm(self) -> float:
        return self._gn0 if self.grad_norm_t is None else float(self.grad_norm_t)

    def magnitude(self, theta: Tensor, dy: Tensor) -> Tensor:
        self._init(theta.device)
        norm_dy = torch.linalg.norm(dy)
        pm = self.beta_t.float() * (torch.linalg.norm(theta) / norm_dy)                  # :114-116
        return torch.where(norm_dy > 0, pm, torch.zeros_like(pm))

    def update(self, grad_dense: Tensor, n_gradients: int) -> None:
        nnz = torch.count_nonzero(grad_dense).float()                                    # :137
        d = self.grad_norm_decay_rate
        self.grad_norm_t = d * self.grad_norm_t + (1.0 - d) * (nnz / n_gradients)        # :144-146
        step = torch.where(self.grad_norm_t < self.target_norm, self.beta_update_step, -self.beta_update_step)
        upd = self.beta_update_momentum * self.prev_update_t + step.double()             # :149-154
        self.beta_t = torch.clamp(self.beta_t + upd, min=0.0)                            # :157
        self.prev_update_t = upd


class _AimleTopK(torch.autograd.Function):
    """z = MAP(theta + tau * eps);  d theta = (MAP(theta'_L + eps') - MAP(theta'_R + eps')) / 2 / lambda with
    theta'_{R,L} = alpha * theta -/+ lambda * dy (symmetric perturbation).  The two target solves also return their
    selection over the padded rows: the adaptive rule counts the flipped slots INCLUDING the pads."""

    @staticmethod
    def forward(ctx, scores, k, plan, noise, seed, state, tau_theta, tau_target, k_cap):
        z = ops.topk_threshold(scores, k, plan=plan, noise=noise, noise_scale=tau_theta, seed=seed, k_cap=k_cap)
        ctx.save_for_backward(scores, noise)
        ctx.cfg = (k, plan, seed, state, tau_target, k_cap)
        return z

    @staticmethod
    def backward(ctx, dy):
        scores, noise = ctx.saved_tensors
        k, plan, seed, state, tau_target, k_cap = ctx.cfg
        pm = state.magnitude(scores, dy)
        t_r = (state.alpha * scores - pm * dy).contiguous()                              # aimle.py:173-176
        t_l = (state.alpha * scores + pm * dy).contiguous()                              # :178-182 (params(theta, -dy))
        z_r, dense_r = ops.topk_threshold(t_r, k, plan=plan, noise=noise, noise_scale=tau_target, seed=seed,
                                          return_dense=True, k_cap=k_cap)
        z_l, dense_l = ops.topk_threshold(t_l, k, plan=plan, noise=noise, noise_scale=tau_target, seed=seed,
                                          return_dense=True, k_cap=k_cap)
        state.update((dense_l - dense_r) / 2.0, dense_l.size(0))                         # target_aimle.py:131-159
        g = (z_l - z_r) / 2.0 / torch.where(pm > 0, pm, torch.ones_like(pm))             # aimle.py:231-237, :161
        return (g,) + (None,) * 8


def imle_topk(scores, k, plan, noise, seed, alpha, beta, tau_in, tau_target, k_cap=None):
    """``k``: an int, or a k per row (int32 [B] device tensor) with ``k_cap``; the backward's target solve uses the same k."""
    return _ImleTopK.apply(scores, k, plan, noise, seed, alpha, beta, tau_in, tau_target, k_cap)


def aimle_topk(scores, k, plan, noise, seed, state, tau_theta, tau_target, k_cap=None):
    """``k``: an int, or a k per row (int32 [B] device tensor) with ``k_cap``; both target solves of the backward use the same k."""
    return _AimleTopK.apply(scores, k, plan, noise, seed, state, tau_theta, tau_target, k_cap)
