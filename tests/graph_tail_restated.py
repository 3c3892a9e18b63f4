"""The layer tail and the read-out restated in plain torch on the CPU, generic in the dtype: every function takes `dt` and evaluates
the formula in it from the same float32 inputs -- torch.float64 is the reference, torch.float32 the yardstick of
tests/test_gpu_graph_tail_fp64.py.  Nothing here knows a kernel's summation order; segment sums are index_add.  Not a test module:
tests/test_graph_tail_cases_cpu.py runs it in both dtypes on every case, tests/test_gpu_graph_tail_fp64.py judges the kernels by it.

Formulas (the reference model's, by file):
  scatter_attention   softmax_g(<q_g, k_n> / sqrt(C)) * v_n, no epsilon in the denominator  (utils/scatter_scaled_dot_product.py)
  graph_norm          o = x - mean_g(x) * mean_scale;  weight * o / sqrt(mean_g(o^2) + eps) + bias                 (PyG GraphNorm)
  layer_tail          graph_norm(scatter_attention(ins, c, c)) + h, then * node_mask                            (mgat.py:168-177)
  attn_pool           x * mask;  gate = softmax_g(<x_n, q_g> / sqrt_fp32(C)) with + 1e-16;  out_g = sum gate_n x_n  (att_pooling.py)
  dense_tail          x_proj.0 -> GELU -> x_proj.2 -> GELU -> layer_tail -> gelu(h' * ins_next[batch])
  readout             node_nn (Linear, GELU, Linear) -> attn_pool with q, or q = ques_nn(u)
"""
import math

import torch


def cast(dt, *ts):
    return tuple(None if t is None else t.detach().to(dt) for t in ts)


def seg_sum(src, batch, B):
    return torch.zeros((B,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, batch, src)


def seg_count(batch, B, dt):
    return torch.bincount(batch, minlength=B).to(dt)


def seg_softmax(logits, batch, B, add):
    """exp(l - max_g) / (sum_g + add) per graph; graphs without nodes take no part."""
    mx = torch.full((B,), -math.inf, dtype=logits.dtype).scatter_reduce_(0, batch, logits, "amax", include_self=True)
    ex = (logits - mx[batch]).exp()
    return ex / (seg_sum(ex, batch, B)[batch] + add)


def attention_logits(dt, query, key, batch):
    query, key = cast(dt, query, key)
    return (query[batch] * key).sum(1) / math.sqrt(key.size(1))


def scatter_attention(dt, query, key, value, batch, B):
    """(alpha[:, None] * value, alpha)"""
    alpha = seg_softmax(attention_logits(dt, query, key, batch), batch, B, 0.0)
    return alpha[:, None] * cast(dt, value)[0], alpha


def graph_norm(dt, x, batch, B, weight, bias, mean_scale, eps):
    x, weight, bias, mean_scale = cast(dt, x, weight, bias, mean_scale)
    cnt = seg_count(batch, B, dt).clamp(min=1)[:, None]
    o = x - (seg_sum(x, batch, B) / cnt)[batch] * mean_scale
    var = seg_sum(o * o, batch, B) / cnt
    return weight * o / (var + eps).sqrt()[batch] + bias


def layer_tail(dt, ins, c, h, batch, B, weight, bias, mean_scale, eps, node_mask=None):
    v, _ = scatter_attention(dt, ins, c, c, batch, B)
    y = graph_norm(dt, v, batch, B, weight, bias, mean_scale, eps) + cast(dt, h)[0]
    if node_mask is not None:
        y = cast(dt, node_mask)[0].reshape(-1, 1) * y
    return y


def pool_logits(dt, x, q, batch, node_mask=None):
    """(<x_n * mask_n, q_g> / sqrt(C) with the float32 square root att_pooling.py takes, the masked rows)"""
    x, q = cast(dt, x, q)
    if node_mask is not None:
        x = x * cast(dt, node_mask)[0].reshape(-1, 1)
    denom = float(torch.sqrt(torch.tensor(float(x.size(1)), dtype=torch.float32)))
    return (x * q[batch]).sum(1) / denom, x


def attn_pool(dt, x, q, batch, B, node_mask=None):
    """(out [B, C] with zero rows for graphs without nodes, gate [N])"""
    logits, x = pool_logits(dt, x, q, batch, node_mask)
    gate = seg_softmax(logits, batch, B, 1e-16)
    return seg_sum(gate[:, None] * x, batch, B), gate


def gelu(x):
    return torch.nn.functional.gelu(x)


def linear(dt, x, weight, bias):
    weight, bias = cast(dt, weight, bias)
    return x.to(dt) @ weight.t() + bias


def x_proj(dt, conv_out, w0, b0, w2, b2):
    return gelu(linear(dt, gelu(linear(dt, conv_out, w0, b0)), w2, b2))


def dense_tail(dt, c, ins, h, batch, B, weight, bias, mean_scale, eps, node_mask=None, ins_next=None):
    """From c = x_proj(conv_out) (its own function: one evaluation serves every run form): (h', gated rows or None)."""
    y = layer_tail(dt, ins, c, h, batch, B, weight, bias, mean_scale, eps, node_mask)
    return y, None if ins_next is None else gelu(y * cast(dt, ins_next)[0][batch])


def mlp3(dt, x, w0, b0, w2, b2):
    """Linear, GELU, Linear: node_nn and ques_nn of the read-out."""
    return linear(dt, gelu(linear(dt, x, w0, b0)), w2, b2)


def readout(dt, xn, q, batch, B, node_mask=None):
    """From xn = mlp3(x, node_nn) and q (given, or mlp3(u, ques_nn)): attn_pool."""
    return attn_pool(dt, xn, q, batch, B, node_mask)
