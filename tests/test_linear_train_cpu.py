"""Host-side checks of a Linear's backward (include/isg_linear_train.h, csrc/isg_linear_bwd.hip, autograd.LINEAR_BWD_KERNELS) that
need no GPU: the header binds and both libraries export it, the entry points refuse what their comments say before they touch a
device, the host-only sizes stay inside their ranges, and with the switch off _Linear.backward reaches neither new operator."""
import ctypes
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null address; nothing dereferences it on the paths tested here


def test_status_codes_match_isg_h():
    header = open(os.path.join(ROOT, "include", "isg.h")).read()
    assert int(re.search(r"#define\s+ISG_EINVAL\s+\(?(-?\d+)", header).group(1)) == EINVAL
    assert int(re.search(r"#define\s+ISG_EUNSUPPORTED\s+\(?(-?\d+)", header).group(1)) == EUNSUPPORTED


def test_linear_train_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_optim, _lib_sgenc_train, _lib_train
    header = open(os.path.join(ROOT, "include", "isg_linear_train.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_linear_train.SIGNATURES) == {
        "isg_linear_train_abi_version", "isg_linear_bwd_prep_parts", "isg_linear_bwd_prep", "isg_linear_wgrad_bf16x6_splits",
        "isg_linear_wgrad_bf16x6"}
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_linear_train.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_LINEAR_TRAIN_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_linear_train_abi_version() == _lib_linear_train.ABI_VERSION == abi == 1
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74      # include/isg.h did not move
    assert (_lib_train.ABI_VERSION, _lib_optim.ABI_VERSION, _lib_dist.ABI_VERSION) == (
        int(re.search(r"ABI_VERSION (\d+)", open(_lib_train.HEADER_PATH).read()).group(1)), 1, 1)
    V, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sig = _lib_linear_train.SIGNATURES
    assert sig["isg_linear_bwd_prep_parts"] == (I64, [I64, I32])
    assert sig["isg_linear_bwd_prep"] == (ctypes.c_int, [V, I32, V, I32, I32, V, I32, V, I64, I32, V])
    assert sig["isg_linear_wgrad_bf16x6_splits"] == (I64, [I64, I32, I32])
    assert sig["isg_linear_wgrad_bf16x6"] == (ctypes.c_int, [V, V, V, I64, I32, I32, I32, I32, I64, V])
    build_checks("isg_linear_train.h")
    assert os.path.exists(os.path.join(ge.CSRC, "isg_linear_bwd.hip"))
    # the strict twin is a second build of the new source, not the fast object linked twice
    assert any(m in open(os.path.join(ge.CSRC, "isg_linear_bwd.hip")).read() for m in ("ISG_WAIT(", "ISG_BARRIER("))


def test_prep_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _lib_linear_train
    prep = _lib_linear_train.load().isg_linear_bwd_prep
    #          g  ldg saved lds mode dz lddz db_part M  N  stream
    assert prep(P, 8, P, 8, 1, P, 8, P, 0, 8, None) == 0                       # M == 0: nothing to do, no launch
    assert prep(P, 8, None, 0, 0, None, 0, P, 0, 8, None) == 0
    assert prep(None, 8, P, 8, 1, P, 8, P, 5, 8, None) == EINVAL               # null g
    assert prep(None, 8, P, 8, 1, P, 8, P, 0, 8, None) == EINVAL               # ... refused even with nothing to do
    for mode in (1, 2):
        assert prep(P, 8, None, 8, mode, P, 8, P, 5, 8, None) == EINVAL        # null saved with an activation
    assert prep(P, 8, None, 0, 0, None, 0, None, 5, 8, None) == EINVAL         # both outputs null
    assert prep(P, 8, P, 8, 1, None, 8, None, 5, 8, None) == EINVAL
    assert prep(P, 7, P, 8, 1, P, 8, P, 5, 8, None) == EINVAL                  # ldg < N
    assert prep(P, 8, P, 7, 2, P, 8, P, 5, 8, None) == EINVAL                  # lds < N
    assert prep(P, 8, P, 8, 1, P, 7, P, 5, 8, None) == EINVAL                  # lddz < N
    for mode in (-1, 3, 17):
        assert prep(P, 8, P, 8, mode, P, 8, P, 5, 8, None) == EINVAL
    assert prep(P, 8, P, 8, 1, P, 8, P, -1, 8, None) == EINVAL                 # M < 0
    assert prep(P, 8, P, 8, 1, P, 8, P, 5, 0, None) == EINVAL                  # N <= 0
    assert prep(P, 8, P, 8, 1, P, 8, P, 1 << 31, 8, None) == EUNSUPPORTED


def test_wgrad_bf16x6_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _lib_linear_train
    wg = _lib_linear_train.load().isg_linear_wgrad_bf16x6
    #        g  x  partial M   N   K  ldg ldx splits stream
    for hole in range(3):
        ptrs = [None if i == hole else P for i in range(3)]
        assert wg(*ptrs, 64, 16, 8, 16, 8, 1, None) == EINVAL, f"null pointer {hole}"
    assert wg(P, P, P, 64, 16, 8, 15, 8, 1, None) == EINVAL                   # ldg < N
    assert wg(P, P, P, 64, 16, 8, 16, 7, 1, None) == EINVAL                   # ldx < K
    assert wg(P, P, P, 64, 16, 8, 16, 8, 0, None) == EINVAL                   # splits <= 0
    assert wg(P, P, P, 64, 16, 8, 16, 8, -3, None) == EINVAL
    assert wg(P, P, P, -1, 16, 8, 16, 8, 1, None) == EINVAL
    assert wg(P, P, P, 64, 0, 8, 16, 8, 1, None) == EINVAL
    assert wg(P, P, P, 64, 16, 0, 16, 8, 1, None) == EINVAL
    assert wg(P, P, P, 1 << 31, 16, 8, 16, 8, 1, None) == EUNSUPPORTED        # M >= 2^31
    assert wg(P, P, P, 64, 16, 8, 16, 8, 65536, None) == EUNSUPPORTED         # splits > 65535
    wide = 65535 * 128 + 1                                                    # 65 536 column tiles
    assert wg(P, P, P, 64, wide, 8, wide, 8, 1, None) == EUNSUPPORTED
    assert wg(P, P, P, 64, 16, wide, 16, wide, 1, None) == EUNSUPPORTED


def test_host_only_sizes_stay_inside_their_ranges():
    from isubgvqa_amd import _lib_linear_train
    lib = _lib_linear_train.load()
    for M in (0, 1, 2, 31, 32, 33, 1000, 4097, 49152, 204753, 1024 * 257 + 3, (1 << 31) - 1):
        for N in (1, 5, 8, 64, 300, 1842, 2048):
            parts = lib.isg_linear_bwd_prep_parts(M, N)
            assert 1 <= parts <= 1024 and parts <= max(M, 1), (M, N, parts)
    assert lib.isg_linear_bwd_prep_parts(1024 * 257 + 3, 8) == 1024              # the GPU test's "more than one block of rows" shape:
    assert -(-(1024 * 257 + 3) // 1024) > 256                                    # a workgroup takes at most 256 rows at a time
    for M in (1, 2, 255, 256, 257, 2049, 4096, 49152, 82189, 204753, (1 << 31) - 1):
        for N, K in ((1, 1), (5, 7), (128, 128), (130, 300), (1200, 300), (1842, 512), (2048, 512), (512, 2048)):
            s = lib.isg_linear_wgrad_bf16x6_splits(M, N, K)
            assert 1 <= s <= 65535 and s <= -(-M // 256), (M, N, K, s)
    assert lib.isg_linear_wgrad_bf16x6_splits(0, 8, 8) == 0


def test_switch_off_reaches_neither_new_operator(monkeypatch):
    """With LINEAR_BWD_KERNELS off _Linear.backward runs the lines it ran before: the new operators are not called.  (Forward and the
    old backward's own kernels need the GPU, so they are stood in for by torch here; the routing is what is under test.)"""
    from isubgvqa_amd import autograd, ops

    def boom(*a, **k):
        raise AssertionError("a new Linear-backward operator was reached with the switch off")

    monkeypatch.setattr(autograd, "LINEAR_BWD_KERNELS", False)
    monkeypatch.setattr(ops, "linear_bwd_prep", boom)
    monkeypatch.setattr(ops, "linear_wgrad_bf16x6", boom)
    monkeypatch.setattr(ops, "linear", lambda x, w, b, gelu=False, cache_planes=True, relu=False:
                        torch.relu(torch.nn.functional.linear(x, w, b)) if relu else torch.nn.functional.linear(x, w, b))
    monkeypatch.setattr(ops, "linear_wgrad", lambda g, x: g.t() @ x)
    monkeypatch.setattr(autograd, "WGRAD_MIN_ROWS", 4)
    before = ops.counters()["linear_bwd_kernels"]
    gen = torch.Generator().manual_seed(0)
    for M, gelu, relu in ((3, True, False), (9, False, True), (9, False, False)):
        x = torch.randn(M, 8, generator=gen, requires_grad=True)
        w = torch.randn(12, 8, generator=gen, requires_grad=True)
        b = torch.randn(12, generator=gen, requires_grad=True)
        go = torch.randn(M, 12, generator=gen)
        autograd.linear(x, w, b, gelu, relu=relu).backward(go)
        x2, w2, b2 = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
        z = torch.nn.functional.linear(x2, w2, b2)
        (torch.nn.functional.gelu(z) if gelu else torch.relu(z) if relu else z).backward(go)
        for got, ref in ((x.grad, x2.grad), (w.grad, w2.grad), (b.grad, b2.grad)):      # the old lines, still computing the gradient
            assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)
    assert ops.counters()["linear_bwd_kernels"] == before
    # and with it on, the same call reaches the new path (the operator raises: that is the proof)
    monkeypatch.setattr(autograd, "LINEAR_BWD_KERNELS", True)
    x = torch.randn(9, 8, generator=gen, requires_grad=True)
    w = torch.randn(12, 8, generator=gen, requires_grad=True)
    b = torch.randn(12, generator=gen, requires_grad=True)
    with pytest.raises(AssertionError, match="a new Linear-backward operator was reached"):
        autograd.linear(x, w, b, True).backward(torch.ones(9, 12))
    assert ops.counters()["linear_bwd_kernels"] == before + 1
