"""Same-box A/B at BASELINE configs[1] shapes: isg_mgat_dense_tail (x_proj + layer tail + next instruction gate on graph-aligned
tiles) against the un-fused chain it replaces (2 x isg_linear_f16x3_tile, isg_instr_attn_graphnorm_residual, isg_instr_gate).
HIP events, interleaved rounds, a 512 MiB write between launches (cold caches, as between the kernels of a step).
Then the masked layer's launch: the conv output of a masked isg_gatv2_layer_conv launch (three nodes picked per
graph: 15 % of the rows live, the step's masked layer has 13 %) through the live-row form at 1-4 tiles per workgroup against the same rows without their flags (the existing form)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isubgvqa_amd import ops, synthetic  # noqa: E402

dev = torch.device("cuda:0")
graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
cfg = synthetic.WorkloadConfig(**{**synthetic.CFG2.__dict__, "num_graphs": graphs})
wl = synthetic.make_workload(cfg).to(dev)
net = synthetic.build_answer_model(cfg).to(dev).eval()
m = net.gat_seq
N, H, C = wl.x.size(0), cfg.heads, cfg.channels
plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=graphs, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
g = torch.Generator(device=dev).manual_seed(1)
conv_out = torch.randn(N, H * C, device=dev, generator=g)
rm = conv_out.view(N, H, C).abs().amax(dim=2).contiguous()
h = torch.randn(N, C, device=dev, generator=g)
ins, ins_next = wl.instr[0].contiguous(), wl.instr[1].contiguous()
bn = m.bns[0]
flush = torch.empty(1 << 27, device=dev)
tile_ptr, ntiles, cap, _ = plan.tiles(64)
print(f"N={N} graphs={graphs} tiles={int(ntiles.item())} (capacity {cap}), rows/tile={N / max(int(ntiles.item()), 1):.1f}")


def fused():
    ops.attach_row_maxima(conv_out, rm)
    return ops.mgat_dense_tail(conv_out, m.x_proj[0], ins, h, plan, bn.weight, bn.bias, bn.mean_scale, bn.eps, ins_next=ins_next)[:2]


def chain():
    ops.attach_row_maxima(conv_out, rm)
    c = ops.mlp(m.x_proj[0], conv_out)
    hh = ops.mgat_layer_tail(ins, c, h, plan, bn.weight, bn.bias, bn.mean_scale, bn.eps)
    return hh, ops.instr_gate(hh, ins_next, wl.batch, plan=plan)


def timed(fn, r):
    flush.fill_(float(r))
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


with torch.no_grad():
    a, b = fused(), chain()
    print("max |h fused - h chain| =", (a[0] - b[0]).abs().max().item(), " max |xg diff| =", (a[1] - b[1]).abs().max().item())
    tf, tc = [], []
    for r in range(23):
        x, y = timed(fused, r), timed(chain, r)
        if r >= 3:
            tf.append(x)
            tc.append(y)
flops = 2.0 * N * (512 * 256 + 256 * 128) * 3
print(f"fused dense tail : {sum(tf) / len(tf):8.1f} us  (min {min(tf):.1f})  {flops / (sum(tf) / len(tf)) / 1e6:.0f} TF/s of fp16 products")
print(f"un-fused chain   : {sum(tc) / len(tc):8.1f} us  (min {min(tc):.1f})")


# ---- the masked layer's tail: live-row form per group size against the existing form on the same conv output -------------------
def masked_conv_out(conv, picks=3):
    """The output of `conv`'s masked isg_gatv2_layer_conv launch with `picks` nodes picked per graph (row maxima and dead-row flags
    attached), and the share of dead rows."""
    score = torch.rand(N, device=dev, generator=g)
    order = torch.argsort(wl.batch.double() + (1.0 - score.double()) * 0.5)
    rank = torch.empty(N, dtype=torch.long, device=dev)
    rank[order] = torch.arange(N, device=dev) - plan.ptr.long()[wl.batch[order]]
    nm = (rank < picks).float()
    x = torch.randn(N, 128, device=dev, generator=g)
    out, _ = ops.gatv2_layer_conv(x, conv.lin_l, conv.lin_r, wl.edge_attr.float().contiguous(), conv.lin_edge.weight, conv.att, plan, H,
                                  bias=conv.bias, node_mask=nm, negative_slope=conv.negative_slope, want_rowmax=True)
    return out, ops.dead_rows(out).all(dim=1).float().mean().item()


with torch.no_grad():
    last = len(m.bns) - 1
    conv_m, share = masked_conv_out(m.convs[last])
    plain = conv_m.clone()                      # the same rows without flags: the existing form
    ops.attach_row_maxima(plain, ops.row_maxima(conv_m))
    bn = m.bns[last]
    ins_l = wl.instr[last].contiguous()
    run = lambda c, grp: ops.mgat_dense_tail(c, m.x_proj[last], ins_l, h, plan, bn.weight, bn.bias, bn.mean_scale, bn.eps, group=grp)[0]
    forms = [("existing form", plain, None)] + [(f"live rows, group {k}", conv_m, k) for k in (1, 2, 3, 4)]
    ref = run(plain, None)
    times = {n: [] for n, _, _ in forms}
    for r in range(23):
        for n, c, k in forms:
            t_us = timed(lambda: run(c, k), r)
            if r >= 3:
                times[n].append(t_us)
    print(f"masked layer: {100 * share:.1f} % of the rows dead; the rule picks group {ops.dense_tail_group(N, plan.E, dev)}")
    for n, c, k in forms:
        same = torch.equal(run(c, k).view(torch.int32), ref.view(torch.int32))
        print(f"  {n:22s}: {sum(times[n]) / len(times[n]):8.1f} us  (min {min(times[n]):.1f})  bits {'equal' if same else 'DIFFER'}")
