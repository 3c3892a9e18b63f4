#!/usr/bin/env python3
"""Where does a wave of isg_gatv2_layer_conv spend its cycles?  Uses tools/_build/libisg_dt_stamp.so (tools/stamp_dense_tail.py
--build makes it with -DISG_DIAG).

--masked: the masked launch, with the node mask the model's masked layer (BASELINE configs[1]'s third, Gumbel top-k) gives on this
batch -- taken from one forward of the model -- and, first, how many of each tile's CSR slots that mask leaves live (nonzero).
The masked launch is the grouped form unless ISG_LC_GROUP=1 is set: its phases carry their own labels.
--tables (with --masked): the tiles' live tables come from isg_layer_conv_live_tables, whose launch the stamps
do not cover: the first phase is then the fetch of the images, and compaction builds no live lists.
The grouped form ends in the constant fill and the list pass, each with a line of its own; with
ISG_LC_AGG_ALL_ROWS=1 it ends in the per-tile aggregation over all rows instead, as before.
--sparse (with --masked): the launch goes through isg_gatv2_layer_conv_sparse with ISG_LC_SPARSE_OUT and a flag buffer, without
attention weights, as MGAT.forward issues it: the fill stores one row per tile."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tools", "_build", "libisg_dt_stamp.so")

import torch

from isubgvqa_amd import _lib, _lib_masked, _lib_sparse_out, ops, synthetic

stamp = ctypes.CDLL(OUT)
stamp.isg_gatv2_layer_conv.restype, stamp.isg_gatv2_layer_conv.argtypes = _lib.SIGNATURES["isg_gatv2_layer_conv"]
stamp.isg_lc_set_stamp_buffer.argtypes = [ctypes.c_void_p]
stamp.isg_gatv2_layer_conv_sparse.restype, stamp.isg_gatv2_layer_conv_sparse.argtypes = _lib_sparse_out.SIGNATURES["isg_gatv2_layer_conv_sparse"]
for sym in ("isg_gatv2_layer_conv_tables", "isg_layer_conv_live_tables", "isg_layer_conv_live_tables_bytes"):
    getattr(stamp, sym).restype, getattr(stamp, sym).argtypes = _lib_masked.SIGNATURES[sym]
dev = torch.device("cuda:0")
cfg = synthetic.CFG2
wl = synthetic.make_workload(cfg).to(dev)
net = synthetic.build_answer_model(cfg).to(dev).eval()
conv = net.gat_seq.convs[0]
N, E, H, C = wl.x.size(0), wl.edge_index.size(1), cfg.heads, cfg.channels
plan = ops.GraphPlan.build(wl.batch, wl.edge_index, num_graphs=cfg.num_graphs, max_nodes=wl.max_nodes, max_edges=wl.max_edges)
x = wl.x.contiguous()
cat_w = torch.cat([conv.lin_l.weight.detach(), conv.lin_r.weight.detach()], 0).contiguous()
cat_b = torch.cat([conv.lin_l.bias.detach(), conv.lin_r.bias.detach()]).contiguous()
wn, wn_inv = ops._weight_planes(cat_w, False, "f16x3")
we, we_inv = ops._weight_planes(conv.lin_edge.weight, True, "f16x3")
ep, ep_inv = plan.edge_planes(wl.edge_attr)
_, ntiles, cap, tile_info = plan.tiles(64, 256)
T = int(ntiles.item())
out = torch.empty(N, H * C, device=dev)
alpha = torch.empty(E, H, device=dev)
rowmax = torch.empty(N, H, device=dev)
xp = ops.node_planes(x)
nm_arg = 0
if "--masked" in sys.argv:
    seen = []
    real = ops.gatv2_layer_conv

    def spy(*args, **kw):
        if kw.get("node_mask") is not None:
            seen.append(kw["node_mask"].reshape(-1).float().contiguous().clone())
        return real(*args, **kw)

    ops.gatv2_layer_conv = spy
    with torch.no_grad():
        net(wl, seed=1000)
    ops.gatv2_layer_conv = real
    assert len(seen) == 1, f"{len(seen)} masked layer_conv launches in one forward"
    node_mask = seen[0]
    nm_arg = node_mask.data_ptr()
    tinfo = tile_info[:int(ntiles.item())].long().cpu()
    live_slot = ((node_mask[plan.src.long()] * node_mask[plan.dst.long()]) != 0).cpu()
    cs = torch.cat([torch.zeros(1, dtype=torch.long), live_slot.long().cumsum(0)])
    ne = tinfo[:, 3].clamp(max=256)
    live = cs[tinfo[:, 2] + ne] - cs[tinfo[:, 2]]
    picked = (node_mask != 0).float().sum().item()
    print(f"masked layer: {picked:.0f} of {N} nodes picked; {int(live.sum())} of {int(ne.sum())} tile slots live "
          f"({100 * live.sum().item() / max(ne.sum().item(), 1):.2f} %); per tile: slots {ne.float().mean():.1f}, live {live.float().mean():.2f} "
          f"(max {int(live.max())}); 64-slot chunks per tile: every slot {((ne + 63) // 64).float().mean():.2f}, live slots "
          f"{((live + 63) // 64).float().mean():.2f}; tiles without a live slot {int((live == 0).sum())} of {len(ne)}")
buf = torch.zeros(4096 * 8, 16, dtype=torch.int64, device=dev)
assert stamp.isg_lc_set_stamp_buffer(buf.data_ptr()) == 0
att = conv.att.detach().reshape(-1).contiguous()
use_tables = bool(nm_arg) and "--tables" in sys.argv
tables = torch.empty(stamp.isg_layer_conv_live_tables_bytes(cap) if use_tables else 0, dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream().cuda_stream
sparse = bool(nm_arg) and "--sparse" in sys.argv
row_dead = torch.empty(N, H, dtype=torch.uint8, device=dev)
for rep in range(2):
    buf.zero_()
    front = (xp.planes.data_ptr(), xp.inv.data_ptr(), wn.data_ptr(), wn_inv.data_ptr(), cat_b.data_ptr(), ep.data_ptr(),
             ep_inv.data_ptr(), we.data_ptr(), we_inv.data_ptr(), att.data_ptr(), conv.bias.data_ptr(),
             plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(), plan.dst.data_ptr(),
             tile_info.data_ptr(), ntiles.data_ptr(), cap, nm_arg, 0, out.data_ptr(), H * C, 0 if sparse else alpha.data_ptr(),
             rowmax.data_ptr(), row_dead.data_ptr() if sparse else 0)
    if use_tables:
        assert stamp.isg_layer_conv_live_tables(plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(), plan.dst.data_ptr(),
                                                ep_inv.data_ptr(), tile_info.data_ptr(), ntiles.data_ptr(), cap, nm_arg, 0,
                                                tables.data_ptr(), N, E, st) == 0
        if sparse:
            rc = stamp.isg_gatv2_layer_conv_sparse(*front, tables.data_ptr(), ops.ISG_LC_SPARSE_OUT, N, E, H, C, 128, 128, 0.2, st)
        else:
            rc = stamp.isg_gatv2_layer_conv_tables(*front, tables.data_ptr(), N, E, H, C, 128, 128, 0.2, st)
    elif sparse:
        rc = stamp.isg_gatv2_layer_conv_sparse(*front, 0, ops.ISG_LC_SPARSE_OUT, N, E, H, C, 128, 128, 0.2, st)
    else:
        rc = stamp.isg_gatv2_layer_conv(*front, N, E, H, C, 128, 128, 0.2, st)
    assert rc == 0
    torch.cuda.synchronize()
s = buf.double().cpu()
s = s[s[:, 12] > 0]
names = ["first tile's inputs (once)", "node GEMM: barrier", "chunks: staging barrier", "chunks: k loops",
         "chunks: epilogue + barrier", "next tile: rows -> planes, tables", "softmax + aggregation per node, stores",
         "hand-over barrier", "node GEMM: k loop", "node GEMM: epilogue (LDS writes)", "chunks: wait for the planes, LDS writes", "last logit sums + barrier", "(total)", "(probe) other", "(probe) exposed latency of a chunk request"]
if nm_arg and os.environ.get("ISG_LC_GROUP") != "1" and os.environ.get("ISG_LC_DENSE_MASK", "0") == "0":
    # gatv2_layer_conv_groups_kernel's stamps (per group of tiles; 3, 4, 10 per chunk; 6 covers the group's tiles)
    # 5 and 7: the constant fill and the list pass; 6 only with ISG_LC_AGG_ALL_ROWS=1, which runs neither
    names = ["fetch: the group's table images (per group)" if use_tables else "scan: requests, tables, ballots (per group)",
             "compaction: node list, maps" if use_tables else "compaction: node list, maps, live lists", "gather: node planes, first edge planes (wait)",
             "group chunks: k loops", "group chunks: epilogue + barrier", "fill: rows without a live in-slot, as constants (per sub-group)",
             "per tile: softmax + aggregation, stores (all tiles of the group)",
             "list pass: softmax + aggregation of live-destination rows (per sub-group)", "group node product: k loop",
             "group node product: barrier + epilogue (LDS writes)", "panel staging + barrier", "last logit sums + barrier", "(total)"]
tot = s[:, 12].mean().item()
nwg = s.size(0) // 8
print(f"{T} tiles x {H} heads on {nwg} persistent workgroups of 8 waves; a wave lives {tot:.0f} cycles = {tot * nwg / max(T * H, 1):.0f} per (tile, head)")
for i, n in enumerate(names):
    print(f"  {n:55s} {s[:, i].mean().item():10.0f}  ({100 * s[:, i].mean().item() / tot:5.1f} %)   max {s[:, i].max().item():10.0f}")
