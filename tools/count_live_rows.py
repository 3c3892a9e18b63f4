#!/usr/bin/env python3
"""DESIGN.md 17.10's count, on the CPU: the rows of x_proj per group of G tiles in the dense tail's live-row form at BASELINE
configs[1] -- live rows of the masked layer (a destination with an in-slot whose two ends are both picked) plus one for the group's
dead rows -- from synthetic.make_workload, the model's CPU path (its mask indices are bit-exact with the GPU's) and isg_tile_plan's
packing rule (64 nodes / 256 slots, consecutive graphs, 1024-graph chunks).       python3 tools/count_live_rows.py [graphs]
Then DESIGN.md 17.12's count: per group of G tiles of the masked layer kernel's grouped form, the nodes that a live slot names and
the live slots, in the order the kernel walks (heavy-first list, a workgroup takes every 64th entry: 256 CUs, 4 heads).
Then DESIGN.md 17.15's count: the live-destination rows (the rows the grouped kernel's one aggregation pass lists; every other row
of a tile is a constant fill) per tile and per group of G tiles in the same walk, and the fill rows' in-slots (one alpha store each)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isubgvqa_amd import synthetic  # noqa: E402
from oracle import model as OM  # noqa: E402
from oracle import samplers as OS  # noqa: E402

graphs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
cfg = synthetic.WorkloadConfig(**{**synthetic.CFG2.__dict__, "num_graphs": graphs})
wl = synthetic.make_workload(cfg)
model = synthetic.build_answer_model(cfg).eval()
sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
ocfg = OM.PathConfig(heads=cfg.heads, masking_thresholds=list(cfg.masks), use_topk=True, sampler_type=cfg.sampler, sample_k=cfg.sample_k)
gen = torch.Generator().manual_seed(1)
noises = {i: OS.uniform_to_gumbel(torch.rand(graphs, wl.max_nodes, generator=gen)) for i, t in enumerate(cfg.masks) if t != 1.0}
torch.set_num_threads(min(16, os.cpu_count() or 1))
with torch.no_grad():
    mask = OM.mgat_pool_classify(sd, wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf, ocfg, noises)[1].reshape(-1)
picked = mask != 0
src, dst = wl.edge_index
N, B = wl.x.size(0), graphs
live = torch.bincount(dst, weights=(picked[src] & picked[dst]).double(), minlength=N) > 0
sizes = torch.bincount(wl.batch, minlength=B).tolist()
slots = torch.bincount(wl.batch[dst], minlength=B).tolist()
tiles, g, r = [], 0, 0
while g < B:
    end = min((g // 1024 + 1) * 1024, B)
    n, s, k = sizes[g], slots[g], g + 1
    while k < end and n + sizes[k] <= 64 and s + slots[k] <= 256:
        n += sizes[k]; s += slots[k]; k += 1
    tiles.append((r, n, s))
    r += n
    g = k
print(f"{N} nodes, {int(picked.sum())} picked, {int(live.sum())} live rows ({100 * live.double().mean().item():.1f} %), {len(tiles)} tiles")
print("| G | groups | mean | <= 8 | 9-16 | 17-32 | 33-64 | > 64 | max |")
print("|---|---|---|---|---|---|---|---|---|")
for G in (1, 2, 3, 4):
    rows = []
    for t0 in range(0, len(tiles), G):
        a, b = tiles[t0][0], tiles[min(t0 + G, len(tiles)) - 1][:2]
        seg = live[a:b[0] + b[1]]
        rows.append(int(seg.sum()) + int((~seg).any()))
    v = torch.tensor(rows)
    share = lambda lo, hi: f"{100 * ((v >= lo) & (v <= hi)).double().mean().item():.1f} %"
    print(f"| {G} | {len(rows)} | {v.double().mean().item():.1f} | {share(0, 8)} | {share(9, 16)} | {share(17, 32)} | {share(33, 64)} | "
          f"{share(65, 10 ** 9)} | {int(v.max())} |")

# ---- 17.12: the layer kernel's groups.  A slot (in-edge) is live when both ends are picked; the nodes it names are its ends.
live_slot = picked[src] & picked[dst]
named = torch.zeros(N, dtype=torch.bool)
named[src[live_slot]] = True
named[dst[live_slot]] = True
slots_at = torch.bincount(dst[live_slot], minlength=N)
cs_named = torch.cat([torch.zeros(1, dtype=torch.long), named.long().cumsum(0)])
cs_slots = torch.cat([torch.zeros(1, dtype=torch.long), slots_at.cumsum(0)])
heavy = sorted(range(len(tiles)), key=lambda t: -min((tiles[t][2] + 31) // 32, 8))      # stable: ties keep the tile order
NGRP = 64
print(f"\n{int(named.sum())} of {N} nodes are named by a live slot; {int(live_slot.sum())} of {src.numel()} slots are live")
print("| tiles per group G | groups | named nodes mean / max | groups > 32 nodes | groups > 64 nodes | live slots mean / max | groups > 64 slots |")
print("|---|---|---|---|---|---|---|")
for G in (1, 2, 3, 4, 5, 6):
    nn, ns = [], []
    for w in range(min(NGRP, len(heavy))):
        seq = heavy[w::NGRP]
        for i in range(0, len(seq), G):
            grp = [tiles[t] for t in seq[i:i + G]]
            nn.append(sum(int(cs_named[a + n] - cs_named[a]) for a, n, _ in grp))
            ns.append(sum(int(cs_slots[a + n] - cs_slots[a]) for a, n, _ in grp))
    nn, ns = torch.tensor(nn), torch.tensor(ns)
    pc = lambda m: f"{100 * m.double().mean().item():.1f} %"
    print(f"| {G} | {len(nn)} | {nn.double().mean().item():.1f} / {int(nn.max())} | {pc(nn > 32)} | {pc(nn > 64)} | "
          f"{ns.double().mean().item():.1f} / {int(ns.max())} | {pc(ns > 64)} |")

# ---- 17.15: the rows the grouped kernel aggregates.  A row is listed when a live slot has it as destination (`live` above); the
# list of a sub-group is one pass of at most 64 rows (a subset of the named nodes: a group beyond 64 named nodes runs tile by tile).
cs_live = torch.cat([torch.zeros(1, dtype=torch.long), live.long().cumsum(0)])
indeg = torch.bincount(dst, minlength=N)
per_tile = torch.tensor([int(cs_live[a + n] - cs_live[a]) for a, n, _ in tiles])
rows_tile = torch.tensor([n for _, n, _ in tiles])
print(f"\n{int(live.sum())} of {N} rows are the destination of a live slot ({100 * live.double().mean().item():.1f} %): listed; the other "
      f"{int((~live).sum())} are fills, holding {int(indeg[~live].sum())} of {src.numel()} in-slots (one alpha store each) and "
      f"{int((indeg[~live] == 0).sum())} rows without an in-slot")
print(f"per tile: rows {rows_tile.double().mean().item():.1f}, listed mean {per_tile.double().mean().item():.2f} / max {int(per_tile.max())}, "
      f"tiles without a listed row {int((per_tile == 0).sum())} of {len(tiles)}")
print("| tiles per group G | groups | listed rows mean / max | groups > 8 rows (a wave with two) | groups > 64 rows | 64-row passes before (one per tile) | after (one per sub-group) |")
print("|---|---|---|---|---|---|---|")
for G in (1, 2, 4, 6):
    nl, passes = [], 0
    for w in range(min(NGRP, len(heavy))):
        seq = heavy[w::NGRP]
        for i in range(0, len(seq), G):
            grp = [tiles[t] for t in seq[i:i + G]]
            named_rows = sum(int(cs_named[a + n] - cs_named[a]) for a, n, _ in grp)
            listed = [int(cs_live[a + n] - cs_live[a]) for a, n, _ in grp]
            if named_rows <= 64:
                nl.append(sum(listed)); passes += 1
            else:                          # the fall-back: the group's tiles one by one
                nl += listed; passes += len(grp)
    nl = torch.tensor(nl)
    pc = lambda m: f"{100 * m.double().mean().item():.1f} %"
    print(f"| {G} | {len(nl)} | {nl.double().mean().item():.1f} / {int(nl.max())} | {pc(nl > 8)} | {pc(nl > 64)} | {len(tiles)} | {passes} |")
