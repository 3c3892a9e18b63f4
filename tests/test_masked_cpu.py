"""Host-side checks of the masked layer's live tables (include/isg_masked.h, csrc/isg_live_tables.hip) that need
no GPU: the header declares exactly the new entry points, header, library and binding agree on the version, the other headers
did not move, the image layout the header documents is the one both sources share, and the entry points refuse what their
comments say before they touch a device."""
import ctypes
import os
import re

from binding_checks import build_checks
from conftest import ROOT

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null 16-byte aligned address; nothing dereferences it on the paths tested here
TILE_BYTES = 4176


def test_masked_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_optim, _lib_sgenc_train, _lib_train
    header = open(os.path.join(ROOT, "include", "isg_masked.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_masked.SIGNATURES) == {
        "isg_masked_abi_version", "isg_layer_conv_live_tables_bytes", "isg_layer_conv_live_tables", "isg_gatv2_layer_conv_group",
        "isg_layer_conv_live_tables_enabled", "isg_gatv2_layer_conv_tables"}
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_masked.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_MASKED_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_masked_abi_version() == _lib_masked.ABI_VERSION == abi == 1
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert _lib_fused.ABI_VERSION == 1 and set(_lib_fused.SIGNATURES) == {"isg_fused_abi_version", "isg_small_mlps",
                                                                           "isg_linear_f16x3_catmul"}
    assert (_lib_optim.ABI_VERSION, _lib_sgenc_train.ABI_VERSION, _lib_dist.ABI_VERSION, _lib_linear_train.ABI_VERSION) == (1, 1, 1, 1)
    assert _lib_train.ABI_VERSION == int(re.search(r"ABI_VERSION (\d+)", open(_lib_train.HEADER_PATH).read()).group(1))
    V, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    sig = _lib_masked.SIGNATURES
    assert sig["isg_layer_conv_live_tables_bytes"] == (I64, [I64])
    assert sig["isg_layer_conv_live_tables"] == (ctypes.c_int, [V] * 7 + [I64, V, V, V, I64, I64, V])
    assert sig["isg_gatv2_layer_conv_group"] == (I32, [I64, I64, I32, I64])
    assert sig["isg_layer_conv_live_tables_enabled"] == (I32, [])
    # isg_gatv2_layer_conv's parameters in its order, with live_tables behind row_dead
    res, args = _lib.SIGNATURES["isg_gatv2_layer_conv"]
    assert args[24] == V and args[25:] == [I64, I64, I32, I32, I32, I32, F, V]
    assert sig["isg_gatv2_layer_conv_tables"] == (res, args[:25] + [V] + args[25:])
    build_checks("isg_masked.h")
    assert os.path.exists(os.path.join(ge.CSRC, "isg_live_tables.hip"))


def test_image_layout_is_declared_once_and_documented():
    """csrc/isg_live_tables.hpp holds the offsets for the pre-pass and the layer kernel; include/isg_masked.h documents them."""
    import __graft_entry__ as ge
    hpp = open(os.path.join(ge.CSRC, "isg_live_tables.hpp")).read()
    header = open(os.path.join(ROOT, "include", "isg_masked.h")).read()
    for src in ("isg_live_tables.hip", "isg_layer_conv.hip"):
        text = open(os.path.join(ge.CSRC, src)).read()
        assert '#include "isg_live_tables.hpp"' in text, src
        assert not re.search(r"constexpr int[^;]*\bLG_T_\w+ =", text), f"{src} declares a table offset of its own"
    assert int(re.search(r"#define ISG_LIVE_TABLES_TILE_BYTES (\d+)", header).group(1)) == TILE_BYTES
    assert f"LG_TILE_BYTES == {TILE_BYTES}" in hpp
    # the documented offsets: {eid, mask} 0, logits 2048, source 3072, destination 3328, live list 3584, row pointers 3840, header 4112
    offs = [int(m) for m in re.findall(r"^ \*\s+(\d+)  (?:int32|float|uint8|uint64)", header, flags=re.M)]
    assert offs == [0, 2048, 3072, 3328, 3584, 3840, 4112, 4128, 4144]
    assert offs[6] + 64 == TILE_BYTES


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from isubgvqa_amd import _lib_masked
    lib = _lib_masked.load()
    assert lib.isg_layer_conv_live_tables_bytes(0) == 0 and lib.isg_layer_conv_live_tables_bytes(-3) == 0
    assert lib.isg_layer_conv_live_tables_bytes(1) == TILE_BYTES and lib.isg_layer_conv_live_tables_bytes(1 << 20) == TILE_BYTES << 20
    pre = lib.isg_layer_conv_live_tables
    #          rowptr eid src dst einv tile_info ntiles cap node_mask edge_mask tables N  E  stream
    assert pre(P, P, P, P, P, P, P, 0, P, None, P, 10, 20, None) == 0                   # no entry: nothing to do, no launch
    assert pre(P, P, P, P, P, P, P, 4, P, None, P, 0, 0, None) == 0                     # no node
    assert pre(P, P, P, P, P, P, P, 4, None, None, P, 10, 20, None) == EINVAL           # neither mask form
    assert pre(None, P, P, P, P, P, P, 4, P, None, P, 10, 20, None) == EINVAL           # null rowptr
    assert pre(P, None, P, P, P, P, P, 4, P, None, P, 10, 20, None) == EINVAL           # null eid with edges
    assert pre(P, P, P, P, None, P, P, 4, None, P, P, 10, 20, None) == EINVAL           # null inverse scales with edges
    assert pre(P, P, P, P, P, None, P, 4, P, None, P, 10, 20, None) == EINVAL           # null tile list
    assert pre(P, P, P, P, P, P, None, 4, P, None, P, 10, 20, None) == EINVAL           # null tile count
    assert pre(P, P, P, P, P, P, P, 4, P, None, None, 10, 20, None) == EINVAL           # null tables
    assert pre(P, P, P, P, P, P, P, -1, P, None, P, 10, 20, None) == EINVAL
    assert pre(P, P, P, P, P, P, P, 4, P, None, P + 8, 10, 20, None) == EUNSUPPORTED    # tables not 16-byte aligned
    assert pre(P, P, P, P, P, P + 4, P, 4, P, None, P, 10, 20, None) == EUNSUPPORTED    # tile list not 16-byte aligned
    assert pre(P, P, P, P, P, P, P, 4, P, None, P, 1 << 31, 20, None) == EUNSUPPORTED
    # the layer entry with tables: a misaligned buffer is refused before anything else is looked at twice
    conv = lib.isg_gatv2_layer_conv_tables
    args = [P] * 17 + [8, P, None, P, 512, P, None, None, P + 4, 10, 20, 4, 128, 128, 128, 0.2, None]
    assert conv(*args) == EUNSUPPORTED
    args[25] = P
    args[17] = 0
    assert conv(*args) == 0                                                                # no tile: nothing to do, no launch
    # the group size of a shape: at least 1, at most the kernel's 6, 1 where there is nothing to group
    g = lib.isg_gatv2_layer_conv_group
    assert g(0, 0, 4, 0) == 1 and g(100, 300, 4, 0) == 1 and g(100, 300, 0, 8) == 1
    assert 1 <= g(82000, 205000, 4, 1400) <= 6
    assert lib.isg_layer_conv_live_tables_enabled() in (0, 1)
