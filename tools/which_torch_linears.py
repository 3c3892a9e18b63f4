import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isubgvqa_amd import ops, synthetic
from isubgvqa_amd.models import build_model
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = build_model(synthetic.full_model_args(), None).to(dev).eval()
wl = synthetic.make_full_workload(1).to(dev)
sg = wl.scene_graphs()
orig = ops._linear_torch
def spy(x, w, b, gelu, relu):
    print("torch linear:", tuple(x.shape), tuple(w.shape), "x.stride", x.stride(), "ptr%16", x.data_ptr() % 16)
    return orig(x, w, b, gelu, relu)
ops._linear_torch = spy
import torch.nn.functional as F
of = F.linear
def spy2(x, w, b=None):
    print("F.linear:", tuple(x.shape), tuple(w.shape))
    return of(x, w, b)
F.linear = spy2
with torch.no_grad():
    model(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.questions, wl.att_mask, return_masks=True, scene_graphs=sg)
    ops.reset_counters()
    model(wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.questions, wl.att_mask, return_masks=True, scene_graphs=sg)
print(ops.counters())
