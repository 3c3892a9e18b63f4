"""Host-side checks of the SIMPLE sampler's backward (include/isg_sampler_train.h, csrc/isg_simple_bwd.hip) that
need no GPU: the header declares exactly the new entry points and shares none with another header, header, library and binding
agree on the version, the LDS rule is the one restated here, the entry point refuses what its comment says before it touches a
device, and -- the algorithm before any kernel -- the explicit two-sweep reverse pass of tests/simple_bwd_restated.py equals
autograd through sampling/methods/simple.py::log_marginals in fp64."""
import ctypes
import os
import re

import torch

from binding_checks import build_checks
from conftest import ROOT, load_golden

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null address; nothing dereferences it on the paths tested here

# ---- the LDS rule of csrc/isg_simple_bwd.hip, restated -----------------------------------------------------------------
ROW_LIMIT = 150 * 1024          # bytes of one row's four trees beyond which isg_simple_topk_bwd refuses
MAX_N, MAX_K = 1024, 16


def bwd_row_bytes(k, nmax):
    """Four trees (W, M, dW, dM) of (2n - 1)(kk + 1) floats, n = nmax rounded up to a power of two, kk = min(k, nmax)."""
    if k <= 0 or nmax < 0:
        return EINVAL
    if nmax == 0:
        return 0
    n = 1 << (nmax - 1).bit_length()
    kk = min(k, nmax)
    row = 4 * (2 * n - 1) * (kk + 1) * 4
    return EUNSUPPORTED if nmax > MAX_N or kk > MAX_K or row > ROW_LIMIT else row


def test_sampler_train_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_optim, _lib_sampler_train,
                              _lib_sgenc_train, _lib_train)
    header = open(os.path.join(ROOT, "include", "isg_sampler_train.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_sampler_train.SIGNATURES) == {
        "isg_sampler_train_abi_version", "isg_simple_topk_bwd_row_bytes", "isg_simple_topk_bwd"}
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_sampler_train.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_SAMPLER_TRAIN_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_sampler_train_abi_version() == _lib_sampler_train.ABI_VERSION == abi == 1
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert (_lib_optim.ABI_VERSION, _lib_fused.ABI_VERSION, _lib_sgenc_train.ABI_VERSION, _lib_dist.ABI_VERSION,
            _lib_linear_train.ABI_VERSION, _lib_masked.ABI_VERSION) == (1, 1, 1, 1, 1, 1)
    V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sig = _lib_sampler_train.SIGNATURES
    assert sig["isg_simple_topk_bwd_row_bytes"] == (I64, [I32, I32])
    #                                                     scores ptr B  nmax k   g_out g_marg d_scores stream
    assert sig["isg_simple_topk_bwd"] == (ctypes.c_int, [V, V, I64, I32, I32, V, V, V, V])
    build_checks("isg_sampler_train.h")
    assert os.path.exists(os.path.join(ge.CSRC, "isg_simple_bwd.hip")) and os.path.exists(os.path.join(ge.CSRC, "isg_simple.hpp"))
    # the backward rebuilds the trees with the forward's code: both sources take it from the one shared header
    for f in ("isg_simple.hip", "isg_simple_bwd.hip"):
        text = open(os.path.join(ge.CSRC, f)).read()
        assert '#include "isg_simple.hpp"' in text and "sm_build_trees(W, M, c, lane, flat)" in text, f
        assert "atomicAdd" not in text, f
    from isubgvqa_amd import autograd, ops
    assert "simple_bwd_kernel" in ops.COUNTERS and autograd.SIMPLE_BWD_KERNEL in (True, False)


def test_lds_rule_is_the_one_restated_here():
    from isubgvqa_amd import _lib_sampler_train
    rule = _lib_sampler_train.load().isg_simple_topk_bwd_row_bytes
    for k in (1, 5, 16):
        for nmax in (1, 2, 64, 65, 512, 513, 1024):
            assert rule(k, nmax) == bwd_row_bytes(k, nmax), (k, nmax)
    # k = 5: a row of 512 slots (n = 512, 98 208 bytes) is the longest admitted; 513 rounds up to n = 1024, 196 512 bytes
    assert rule(5, 512) == 4 * 1023 * 6 * 4 == 98208 and rule(5, 513) == EUNSUPPORTED
    assert max(m for m in range(1, 1025) if rule(5, m) > 0) == 512
    assert rule(1, 1024) == 4 * 2047 * 2 * 4 and rule(16, 1024) == EUNSUPPORTED and rule(16, 64) == 4 * 127 * 17 * 4
    assert rule(7, 3) == rule(3, 3) == 4 * 7 * 4 * 4                          # k is clamped to nmax
    assert rule(17, 64) == EUNSUPPORTED and rule(17, 16) == bwd_row_bytes(16, 16) and rule(5, 1025) == EUNSUPPORTED
    assert rule(0, 8) == EINVAL and rule(5, -1) == EINVAL and rule(5, 0) == 0


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _lib_sampler_train
    bwd = _lib_sampler_train.load().isg_simple_topk_bwd
    #          scores ptr B nmax k g_out g_marg d_scores stream
    assert bwd(P, None, 0, 8, 5, P, None, P, None) == 0                      # no row: nothing to do, no launch
    assert bwd(P, None, 4, 0, 5, P, None, P, None) == 0                      # no slot
    assert bwd(None, None, 0, 0, 5, None, None, None, None) == 0
    assert bwd(None, None, 4, 8, 5, P, None, P, None) == EINVAL              # null scores
    assert bwd(P, None, 4, 8, 5, P, None, None, None) == EINVAL              # null d_scores
    assert bwd(P, None, 4, 8, 0, P, None, P, None) == EINVAL                 # k <= 0
    assert bwd(P, None, -1, 8, 5, P, None, P, None) == EINVAL
    assert bwd(P, None, 4, -8, 5, P, None, P, None) == EINVAL
    assert bwd(P, None, 4, 513, 5, P, None, P, None) == EUNSUPPORTED         # one slot beyond the LDS rule at k = 5
    assert bwd(P, None, 4, 1025, 1, P, None, P, None) == EUNSUPPORTED
    assert bwd(P, None, 4, 64, 17, P, None, P, None) == EUNSUPPORTED
    assert bwd(P, None, 1 << 31, 8, 5, P, None, P, None) == EUNSUPPORTED


# ---- the reverse sweep itself, in fp64 on the CPU -----------------------------------------------------------------------
def _rows(nmax, k, lens, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    return (torch.randn(B, nmax, generator=g, dtype=torch.float64), torch.tensor(lens), k,
            torch.randn(B, nmax, generator=g, dtype=torch.float64), torch.randn(B, nmax, generator=g, dtype=torch.float64))


def _cases():
    out = []
    for c in load_golden("g9_simple.pt"):
        if c["train"] and not torch.isnan(c["marginals"]).any():
            B, nmax = c["scores"].shape[:2]
            out.append((f"g9 [{B}, {nmax}] k={c['k']}", c["scores"].view(B, nmax).double(), torch.full((B,), nmax), c["k"],
                        c["w"].view(B, nmax).double(), None))
    # seeded rows of lengths {1, 2, k, k+1, nmax}: with nmax > 2k + 1 the shortest rows hold more zero pads than k
    for nmax, k in ((1, 5), (2, 5), (4, 5), (6, 2), (13, 5), (33, 3), (64, 5), (65, 4)):
        lens = sorted({min(v, nmax) for v in (1, 2, k, k + 1, nmax)})
        dense, lens, k, g_out, g_marg = _rows(nmax, k, lens, 100 * nmax + k)
        out.append((f"seeded nmax={nmax} k={k} lens={lens.tolist()}", dense, lens, k, g_out, g_marg))
    return out


def test_two_sweep_reverse_pass_equals_autograd_in_fp64():
    import simple_bwd_restated as R
    cases = _cases()
    assert sum(name.startswith("g9") for name, *_ in cases) == 7
    for name, dense, lens, k, g_out, g_marg in cases:
        for what, go, gm in (("g_out", g_out, None), ("g_marg", None, g_marg), ("both", g_out, g_marg)):
            if go is None and gm is None:
                continue
            ref = R.grad_autograd(dense, lens, k, go, gm)
            got = R.grad_two_sweeps(dense, lens, k, go, gm)
            assert torch.isfinite(ref).all(), name
            err = (got - ref).abs().max().item()
            scale = max(ref.abs().max().item(), 1.0)
            print(f"[simple bwd restated] {name} {what}: max |d| {err:.2e} of {scale:.2e}")
            # fp64 with sums in another order: a few hundred roundings of 1.1e-16 on values of size `scale`
            assert err <= 1e-12 * scale, (name, what, err)
        if dense.size(1) == 1:
            assert not got.any(), "one slot: the marginal is the constant 1"
