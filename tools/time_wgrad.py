#!/usr/bin/env python3
"""dW = g^T x: isg_linear_wgrad (fp32 MFMA, split over rows) vs isg_linear_wgrad_bf16x6 (six bf16 products, transposed LDS reads)
vs torch (hipBLASLt fp32), interleaved in one process, HIP events.

  python tools/time_wgrad.py [--mid | --step] [--prep] [--wgs 256,1024] [--out profiles/<name>.json]

`--mid`: reductions of 2 k to 16 k rows, between autograd.WGRAD_MIN_ROWS and where the split-M kernels win on time, instead of
the flagship's long-thin shapes.  `--step`: the training step's own Linears (question side at 49 152 rows, MGAT at H C = 1200, the
classifier).  `--prep`: isg_linear_bwd_prep at (49152, 2048) in each mode beside a torch copy_ of the bytes it reads and writes.
TF/s are of fp32-equivalent work (2 M N K)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from isubgvqa_amd import ops

dev = torch.device("cuda:0")
argv = sys.argv[1:]
SHAPES = [("lin_edge", 205024, 512, 128), ("lin_l|lin_r", 82286, 1024, 128), ("x_proj.0", 82286, 256, 512),
          ("x_proj.2", 82286, 128, 256), ("node_nn", 82286, 128, 128), ("logit_fc", 4096, 1842, 512)]
if "--mid" in argv:
    SHAPES = [(f"{w}@{M}", M, N, K) for w, N, K in [("narrow", 128, 128), ("mid", 512, 128), ("wide", 1200, 300), ("logit_fc", 1842, 512)]
              for M in (2048, 4096, 8192, 16383)]
if "--step" in argv:
    SHAPES = [("in_proj", 49152, 1536, 512), ("linear1", 49152, 2048, 512), ("linear2", 49152, 512, 2048),
              ("mgat edge", 204753, 1200, 300), ("mgat node", 82189, 1200, 300), ("mgat 1200->600", 82189, 600, 1200),
              ("logit_fc", 4096, 1842, 512)]
KERNELS = {"torch": lambda g, x: g.t() @ x, "isg": ops.linear_wgrad, "bf16x6": ops.linear_wgrad_bf16x6}


def _with_wgs(target):
    def run(g, x):
        os.environ["ISG_WGRAD_BF16_WGS"] = str(target)          # isg_linear_wgrad_bf16x6_splits reads it on every call
        try:
            return ops.linear_wgrad_bf16x6(g, x)
        finally:
            del os.environ["ISG_WGRAD_BF16_WGS"]
    return run


for a, b in zip(argv, argv[1:]):                                # --wgs 256,1024: the bf16 kernel at other workgroup targets, as further columns
    if a == "--wgs":
        KERNELS.update({f"bf16x6@{t}": _with_wgs(int(t)) for t in b.split(",")})


def median(v):
    return sorted(v)[len(v) // 2]


def interleaved(fns, rounds=10, skip=2):
    """{name: median us} of the callables, one call of each per round"""
    res = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r >= skip:
                res[k].append(s.elapsed_time(e) * 1e3)
    return {k: round(median(v), 1) for k, v in res.items()}, {k: round(min(v), 1) for k, v in res.items()}


out = {"device": torch.cuda.get_device_name(0), "method": "HIP events, 10 rounds (2 discarded), the kernels interleaved inside a round; median us",
       "wgrad": [], "prep": []}
for name, M, N, K in SHAPES:
    g, x = torch.randn(M, N, device=dev), torch.randn(M, K, device=dev)
    med, low = interleaved({k: (lambda f=f: f(g, x)) for k, f in KERNELS.items()})
    fl = 2.0 * M * N * K
    tf = {k: round(fl / v / 1e6, 1) for k, v in med.items()}
    out["wgrad"].append({"name": name, "M": M, "N": N, "K": K, "us": med, "min_us": low, "TF": tf,
                         "bf16x6_over_isg": round(med["bf16x6"] / med["isg"], 3), "bf16x6_over_torch": round(med["bf16x6"] / med["torch"], 3)})
    print(f"{name:14s} [{M},{N}]^T x [{M},{K}]: torch {med['torch']:7.1f} us ({tf['torch']:5.1f} TF)  isg {med['isg']:7.1f} us "
          f"({tf['isg']:5.1f} TF)  bf16x6 {med['bf16x6']:7.1f} us ({tf['bf16x6']:5.1f} TF)  bf16x6 / isg {med['bf16x6'] / med['isg']:.2f}"
          + "".join(f"  {k} {v:7.1f} us" for k, v in med.items() if "@" in k), flush=True)
    del g, x
if "--prep" in argv:
    M, N = 49152, 2048
    g, z = torch.randn(M, N, device=dev), torch.randn(M, N, device=dev)
    y = torch.relu(z)
    two, three = torch.empty(2, M, N, device=dev), torch.empty(3, M, N, device=dev)      # copy_ of as many bytes as a mode moves
    fns = {"mode 0, db alone (reads 1x)": lambda: ops.linear_bwd_prep(g, None, 0, want_dz=False),
           "mode 1 GELU' (reads 2x, writes 1x)": lambda: ops.linear_bwd_prep(g, z, 1),
           "mode 2 ReLU' (reads 2x, writes 1x)": lambda: ops.linear_bwd_prep(g, y, 2),
           "torch: aten.gelu_backward + sum(0)": lambda: torch.ops.aten.gelu_backward(g, z).sum(0),
           "torch: g * (y > 0) + sum(0)": lambda: (g * (y > 0)).sum(0),
           "torch: g.sum(0)": lambda: g.sum(0),
           "copy_ of [M, N] (reads 1x, writes 1x)": lambda: two[0].copy_(g),
           "copy_ of 1.5 x [M, N] (reads 1.5x, writes 1.5x: the bytes of modes 1 and 2)": lambda: three.view(-1)[:M * N * 3 // 2].copy_(two.view(-1)[:M * N * 3 // 2])}
    med, low = interleaved(fns)
    for k in fns:
        out["prep"].append({"what": k, "M": M, "N": N, "us": med[k], "min_us": low[k]})
        print(f"prep [{M},{N}] {k}: {med[k]:.1f} us", flush=True)
for a, b in zip(argv, argv[1:]):
    if a == "--out":
        with open(b, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
