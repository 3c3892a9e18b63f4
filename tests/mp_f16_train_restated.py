"""The GATv2 layer on fp16 feature rows as the training path differentiates it, in plain torch (no kernel, no GPU).

BASELINE configs[4] rounds four tensors to IEEE half once each: x_l, x_r, e_proj and the aggregated output (+ bias).  Training
treats every one of those roundings as a straight-through step,

    ste(t) = t + (t.half().float() - t).detach()

whose value is the rounded tensor and whose derivative is the identity: what autograd differentiates is the fp32 function
evaluated at the rounded rows.  `conv` is `oracle.model.gatv2_conv_forward` (unmasked, or with an edge mask handed in) with
`ste` at the four places where the oracle writes `.half().float()`; in the forward the two are the same operations.
"""
import torch
import torch.nn.functional as F


def ste(t):
    return t + (t.half().float() - t).detach()


def conv(sd, p, x, edge_index, batch, edge_attr, instruction, heads, negative_slope=0.2, edge_mask=None, half=True):
    """(out [N, H*C], alpha [E, H]) of one layer from a state dict `sd` under prefix `p`; half=False: no rounding at all."""
    from oracle import model as OM
    from oracle import primitives as P
    r = ste if half else (lambda t: t)
    HC = sd[p + ".lin_l.weight"].shape[0]
    C = HC // heads
    x = P.gelu(x * instruction[batch])
    x_l = r(F.linear(x, sd[p + ".lin_l.weight"], sd.get(p + ".lin_l.bias")).view(-1, heads, C))
    x_r = r(F.linear(x, sd[p + ".lin_r.weight"], sd.get(p + ".lin_r.bias")).view(-1, heads, C))
    e_proj = r(F.linear(edge_attr, sd[p + ".lin_edge.weight"]).view(-1, heads, C))
    out, alpha = OM.gatv2_message_passing(x_l, x_r, e_proj, sd[p + ".att"], edge_index, edge_mask, negative_slope)
    return r(out.view(-1, HC) + sd[p + ".bias"]), alpha
