"""The --concat_instr model variant restated literally in torch, for the tests of DESIGN.md 29 (no test in this file).

The reference's MaskingGATv2Conv under concat_instr reads `torch.cat((x, instruction[batch]), dim=1)`, 2C wide, where the default
variant reads gelu(x * instruction[batch]) (mgat_v2_conv.py:153-157); everything behind that line is the same.  So the layer here
is that one line followed by the oracle's own pieces -- oracle.model.linear, masking_model_forward, node_mask_to_edge_mask,
gatv2_message_passing -- and the stack is oracle.model.mgat_forward's loop around it.  Every function takes the dtype of its
inputs: float32 is the yardstick, float64 the reference.

`separated()` is the fixture rule for a masked layer: an input is rejected when, in the float64 restatement, the k-th and the
(k+1)-th largest sampler score of a graph's padded row (noise included) lie closer than 1e-3 of the row's largest magnitude and
at least one of the two belongs to a real node -- a top-k that near a tie may legitimately fall either way in fp32.  `reseeded()`
draws inputs from seeds 0, 1, 2, ... on the CPU until none of a fixture's masked rows is that close; on such inputs the masks of
two implementations must be EQUAL.
"""
import torch
import torch.nn.functional as F

from oracle import model as OM

P = OM.P
TIE_GAP = 1e-3


def cat_input(x, instruction, batch):
    return torch.cat((x, instruction[batch]), 1)                                         # mgat_v2_conv.py:154


def conv(sd, p, x, edge_index, batch, edge_attr, instruction, imle_att, masking_threshold, cfg, noise=None, aux=None):
    """oracle.model.gatv2_conv_forward with the concatenation in place of the gate -> (out [N, H C], mask | None, alpha)."""
    H = cfg.heads
    HC = sd[p + ".lin_l.weight"].shape[0]
    C = HC // H
    x = cat_input(x, instruction, batch)
    mask = edge_mask = None
    thr = int(masking_threshold) if masking_threshold > 1 else masking_threshold
    if thr != 1.0:
        mask, a = OM.masking_model_forward(sd, p + ".mask", x, imle_att[batch], batch, cfg, noise, return_aux=True)
        if aux is not None:
            aux.update(a)
        edge_mask = OM.node_mask_to_edge_mask(mask, edge_index)
    x_l = OM.linear(sd, p + ".lin_l", x).view(-1, H, C)
    x_r = OM.linear(sd, p + ".lin_r", x).view(-1, H, C)
    e_proj = F.linear(edge_attr, sd[p + ".lin_edge.weight"]).view(-1, H, C)
    if cfg.fp16_features:
        x_l, x_r, e_proj = x_l.half().float(), x_r.half().float(), e_proj.half().float()
    out, alpha = OM.gatv2_message_passing(x_l, x_r, e_proj, sd[p + ".att"], edge_index, edge_mask, cfg.negative_slope)
    out = out.view(-1, HC) + sd[p + ".bias"]
    if cfg.fp16_features:
        out = out.half().float()
    return out, mask, alpha


def mgat(sd, p, x, edge_index, instr_vectors, glf, edge_attr, batch, cfg, noises=None, trace=None):
    """oracle.model.mgat_forward's loop around conv() -> (h, mask)."""
    h, mask = x, None
    for i in range(len(cfg.masking_thresholds)):
        ins = instr_vectors[i]
        aux = {}
        c, mask, _ = conv(sd, f"{p}.convs.{i}", h, edge_index, batch, edge_attr, ins, glf, cfg.masking_thresholds[i], cfg,
                          None if noises is None else noises.get(i), aux)
        c = P.gelu(OM.linear(sd, f"{p}.x_proj.{i}.0", c))
        c = P.gelu(OM.linear(sd, f"{p}.x_proj.{i}.2", c))
        c = OM.scatter_scaled_dot_product_attention(ins, c, c, batch)
        c = P.graph_norm(c, batch, sd[f"{p}.bns.{i}.weight"], sd[f"{p}.bns.{i}.bias"], sd[f"{p}.bns.{i}.mean_scale"],
                         cfg.graphnorm_eps, num_graphs=instr_vectors.size(1))
        h = c + h
        if cfg.interpretable_mode and mask is not None:
            h = mask * h
        if trace is not None:
            trace.append(aux)
    return h, mask


def answer(sd, x, edge_index, edge_attr, batch, instr, glf, cfg, noises=None, trace=None):
    """oracle.model.mgat_pool_classify around mgat() -> (logits, mask, gate)."""
    h, mask = mgat(sd, "gat_seq", x, edge_index, instr[:4], glf, edge_attr, batch, cfg, noises, trace)
    embed, gate = OM.global_attention_forward(sd, "graph_global_attention_pooling", h, glf, batch, node_mask=mask,
                                              size=glf.size(0))
    return OM.classifier_head(sd, embed, glf), mask, gate


def cast(tree, dtype):
    """Every floating tensor of a dict / list / tuple / tensor as `dtype` (detached copies); everything else as it is."""
    if isinstance(tree, torch.Tensor):
        return tree.detach().to(dtype).clone() if tree.is_floating_point() else tree
    if isinstance(tree, dict):
        return {k: cast(v, dtype) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(cast(v, dtype) for v in tree)
    return tree


def separated(dense, k, counts, noise=None, noise_scale=0.0):
    """The fixture rule on one masked layer's padded scores `dense` [B, nmax] (float64; counts[g] real nodes lead row g)."""
    s = dense.double() if noise is None else dense.double() + noise_scale * noise.reshape(dense.shape).double()
    if s.size(1) <= k:
        return True
    v, idx = s.sort(dim=1, descending=True)
    real = idx < counts.view(-1, 1)
    gap = v[:, k - 1] - v[:, k]
    close = gap < TIE_GAP * s.abs().amax(dim=1)
    return not bool((close & (real[:, k - 1] | real[:, k])).any())


def reseeded(make, scores, tries=64):
    """make(seed) -> a fixture; scores(fixture) -> [(dense, k, counts, noise, noise_scale), ...] from the float64 restatement.
    The first fixture of seeds 0 .. tries - 1 whose masked rows are all separated."""
    for seed in range(tries):
        fx = make(seed)
        if all(separated(*s) for s in scores(fx)):
            return fx
    raise AssertionError(f"no fixture with separated top-k scores among {tries} seeds")
