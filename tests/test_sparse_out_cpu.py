"""Host-side checks of the sparse convolution output that need no GPU: the rule by which MGAT.forward asks for
it, ops.dense_conv_out against a construction in plain torch, the marker's tie to the tensor's version, and what the new entry
point refuses before it touches a device."""
import inspect
import itertools

import torch

from binding_checks import build_checks

P = 4096                        # any non-null 16-byte aligned address; nothing dereferences it on the paths tested here
EINVAL = -1


def test_rule_needs_every_condition():
    from isubgvqa_amd import ops
    rule = ops.sparse_conv_out_rule
    yes = dict(masked=True, tail_supported=True, explainer=False, dense_rows=False, conv="layer_conv")
    assert rule(**yes) is True
    # each condition on its own turns it off ...
    for key, other in (("masked", False), ("tail_supported", False), ("explainer", True), ("dense_rows", True), ("conv", "tile_conv"),
                       ("conv", "pair"), ("conv", "unfused")):
        assert rule(**{**yes, key: other}) is False, key
    # ... and no combination with one of them off turns it on
    for m, t, e, dr, conv in itertools.product((False, True), (False, True), (False, True), (False, True), ("layer_conv", "tile_conv")):
        assert rule(m, t, e, dr, conv) == (m and t and not e and not dr and conv == "layer_conv")


def test_mgat_forward_asks_the_rule_and_the_wrappers_guard_the_other_readers():
    from isubgvqa_amd import ops
    from isubgvqa_amd.models.mgat import MGAT
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    src = inspect.getsource(MGAT.forward)
    assert "ops.sparse_conv_out_rule(" in src and "ops.dense_tail_dense_rows()" in src and "routes[i].conv" in src
    assert "want_alpha=bool(return_attention)" in src and "sparse_out=sparse" in src
    assert src.index("ops.dense_conv_out(conv_res)") < src.index("ops.mlp(self.x_proj[i], conv_res)")      # the un-fused path
    conv = inspect.getsource(MaskingGATv2Conv.forward)
    assert "want_alpha=want_alpha" in conv and "sparse_out=sparse_out" in conv
    sig = inspect.signature(ops.gatv2_layer_conv).parameters
    assert sig["want_alpha"].default is True and sig["sparse_out"].default is False
    tail = inspect.getsource(ops.mgat_dense_tail)
    assert "dense_tail_dense_rows()" in tail and "dense_conv_out(conv_out).index_select(0, sub.nodes)" in tail
    assert ops.Switches().poison_sparse_out is False and ops.Switches().sparse_conv_out is True


def conv_result(H=4, C=8, N=23, bias="random", seed=0):
    """(dense out, sparse out with NaN in the rows a sparse launch leaves out, maxima of both, flags): tiles of 5 rows."""
    g = torch.Generator().manual_seed(seed)
    b = None if bias is None else torch.randn(H * C, generator=g)
    if bias == "negzero":
        b[::2] = -0.0
    dead = (torch.rand(N, H, generator=g) < 0.7).to(torch.uint8)
    dead[3], dead[4], dead[11], dead[12], dead[13], dead[22] = 1, 1, 1, 1, 1, 1
    alldead = dead.bool().all(dim=1)
    const = torch.zeros(H * C) + (0 if b is None else b)
    out = torch.randn(N, H * C, generator=g)
    out[alldead] = const
    rowmax = out.view(N, H, C).abs().amax(dim=2)
    sparse, srm = out.clone(), rowmax.clone()
    for r0 in range(0, N, 5):                       # every all-dead row of a tile but its first is left out
        rows = [r for r in range(r0, min(r0 + 5, N)) if alldead[r]]
        sparse[rows[1:]] = float("nan")
        srm[rows[1:]] = float("nan")
    return out, sparse, rowmax, srm, dead, b


def test_dense_conv_out_fills_the_flagged_rows():
    from isubgvqa_amd import ops
    for bias in ("random", None, "negzero"):
        out, sparse, rowmax, srm, dead, b = conv_result(bias=bias)
        assert torch.isnan(sparse).any()
        ops.attach_row_maxima(sparse, srm)
        ops.attach_dead_rows(sparse, dead)
        assert ops.dense_conv_out(sparse) is sparse and not ops.is_sparse_conv_out(sparse)        # no marker: the identity
        ops._attach(sparse, "_isg_sparse_out", b)
        assert ops.is_sparse_conv_out(sparse)
        full = ops.dense_conv_out(sparse)
        assert full is not sparse and not ops.is_sparse_conv_out(full)
        assert torch.equal(full.view(torch.int32), out.view(torch.int32)), bias                  # signed zeros included
        assert torch.equal(ops.row_maxima(full).view(torch.int32), rowmax.view(torch.int32)), bias
        assert ops.dead_rows(full) is dead
        assert torch.isnan(sparse).any()                                                         # the input is left as it was
        assert ops.dense_conv_out(full) is full
    # -0 in the bias becomes +0 (an addition, as in the kernel); the maxima are +0 where the bias is all zeros
    out, sparse, rowmax, srm, dead, b = conv_result(bias="negzero")
    assert (out[3].view(torch.int32)[::2] == 0).all()


def test_marker_is_tied_to_the_tensors_version():
    from isubgvqa_amd import ops
    out, sparse, rowmax, srm, dead, b = conv_result()
    ops.attach_row_maxima(sparse, srm)
    ops.attach_dead_rows(sparse, dead)
    ops._attach(sparse, "_isg_sparse_out", b)
    sparse[0, 0] = 1.0                                # an in-place write: maxima, flags and marker are all stale together
    assert not ops.is_sparse_conv_out(sparse) and ops.dead_rows(sparse) is None and ops.dense_conv_out(sparse) is sparse


def test_sparse_out_header_parses_binds_and_is_exported():
    """include/isg_sparse_out.h declares exactly the new entry point and its version function; header, binding and both libraries
    agree; the signature is isg_gatv2_layer_conv_tables's with a flag word behind live_tables; the other headers did not move."""
    import ctypes
    import os
    import re
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_mp_train, _lib_optim,
                              _lib_sampler_train, _lib_sgenc_train, _lib_sparse_out, _lib_topk_rows, _lib_train)
    header = open(os.path.join(ge.ROOT, "include", "isg_sparse_out.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_sparse_out.SIGNATURES) == {"isg_sparse_out_abi_version", "isg_gatv2_layer_conv_sparse"}
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked,
              _lib_sampler_train, _lib_topk_rows, _lib_mp_train]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_sparse_out.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_SPARSE_OUT_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_sparse_out_abi_version() == _lib_sparse_out.ABI_VERSION == abi == 1
    assert int(re.search(r"#define ISG_LC_SPARSE_OUT (\d+)", header).group(1)) == 1
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74 and _lib_masked.ABI_VERSION == 1 and len(_lib_masked.SIGNATURES) == 6
    res, args = _lib_masked.SIGNATURES["isg_gatv2_layer_conv_tables"]
    assert _lib_sparse_out.SIGNATURES["isg_gatv2_layer_conv_sparse"] == (res, args[:26] + [ctypes.c_int32] + args[26:])
    import inspect
    build_checks("isg_sparse_out.h")


def test_sparse_entry_point_refuses_bad_flags_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib_sparse_out, ops
    lib = _lib_sparse_out.load()
    assert ops.ISG_LC_SPARSE_OUT == 1
    conv = lib.isg_gatv2_layer_conv_sparse
    #       17 operands      max_tiles nm  em    out ldo  alpha rowmax dead tables flags N   E  H  C    K_in K_e slope stream
    args = [P] * 17 + [8, P, None, P, 512, None, P, P, P, 1, 10, 20, 4, 128, 128, 128, 0.2, None]
    args[17] = 0
    assert conv(*args) == 0                               # no tile: nothing to do, no launch
    args[26] = 2
    assert conv(*args) == EINVAL                          # an unknown flag
    args[26], args[24] = 1, None
    assert conv(*args) == EINVAL                          # sparse output without flags for its readers
    args[24], args[18] = P, None
    assert conv(*args) == EINVAL                          # ... or without a mask
    args[26] = 0
    assert conv(*args) == 0                               # flags = 0: isg_gatv2_layer_conv_tables itself
