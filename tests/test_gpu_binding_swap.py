"""A swap of `_lib._lib` reaches the entry points of every device header (isubgvqa_amd/_lib.py): one masked ops.gatv2_layer_conv on
groups of tiles -- the pre-pass and the layer entry of include/isg_masked.h -- under a recording proxy around the product library
and around its strict twin (tests/test_gpu_strict.py).  Both recordings name the two entry points, and the two builds give equal
bits.  With a handle per header the recordings held neither name: the masked layer ran on the product library whatever was
swapped in."""
import ctypes

import pytest
import torch

from test_gpu_ops import _rand_graphs

pytestmark = pytest.mark.gpu


class Recorder:
    """Not a CDLL, only __getattr__: the calls that reach it, by name, passed on to a handle."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def wrapped(*a):
            self.calls.append(name)
            return fn(*a)
        return wrapped


def test_a_swapped_library_runs_the_masked_layer():
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib, _lib_masked, ops
    from isubgvqa_amd.models.layers import GlorotLinear
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    dev = torch.device("cuda:0")
    H, C, K = 4, 128, 128
    gen = torch.Generator().manual_seed(43)
    sizes = torch.randint(8, 34, (300,), generator=gen).tolist()
    batch, ei = _rand_graphs(gen, sizes, extra_per_node=1.5, hub=(7, 60))
    N, E = batch.numel(), ei.size(1)
    torch.manual_seed(47)
    lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
    x = (torch.randn(N, 128, generator=gen) * torch.rand(N, 1, generator=gen).mul(3).exp()).to(dev)
    ea = torch.randn(E, K, generator=gen).to(dev)
    w = (torch.randn(H * C, K, generator=gen) * 0.1).to(dev)
    att, bias = torch.randn(1, H, C, generator=gen).to(dev), torch.randn(H * C, generator=gen).to(dev)
    nm = (torch.rand(N, generator=gen) < 0.6).float().to(dev)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=len(sizes))

    fast = _lib.load()
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    # the library's own rule for this shape: on the per-tile kernel the launch needs no tables, and the test would test nothing
    cap = plan.tiles_and_edge_planes(ea, ops.TILE_CONV_NODES, ops.TILE_CONV_EDGES)[0][2]
    assert _lib_masked.load().isg_gatv2_layer_conv_group(N, E, H, cap) > 1
    assert _lib_masked.load().isg_layer_conv_live_tables_enabled()

    runs = []
    for lib in (fast, strict):
        rec = Recorder(lib)
        _lib._lib = rec
        try:
            with torch.no_grad():
                out, alpha = ops.gatv2_layer_conv(x, lin_l, lin_r, ea, w, att, plan, H, bias=bias, node_mask=nm, want_rowmax=True)
            torch.cuda.synchronize()
        finally:
            _lib._lib = fast
        runs.append((rec.calls, out, alpha, ops.row_maxima(out)))
    for calls, out, alpha, rowmax in runs:
        assert "isg_layer_conv_live_tables" in calls and "isg_gatv2_layer_conv_tables" in calls, calls
        assert torch.isfinite(out).all() and rowmax is not None
    (_, out, alpha, rowmax), (_, s_out, s_alpha, s_rowmax) = runs
    for what, a, b in (("out", out, s_out), ("alpha", alpha, s_alpha), ("row maxima", rowmax, s_rowmax)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"{what}: the strict and the fast build differ in {int((a != b).sum())} values"
