"""ops.small_mlps_supported: the pure rule that decides whether the question-side MLPs of a step run as one
isg_small_mlps launch.  The launch reproduces isg_linear_bf16x6's bits and nothing else's, so the rule says yes only where every
Linear of every chain is one ops.linear_route sends to "bf16x6": both sides of each condition are held here, without a GPU."""
import dataclasses

import pytest
import torch

from binding_checks import build_checks
from isubgvqa_amd import ops

GATE = [(128, 128)]                      # MaskingModel.ques_nn: Linear(+GELU)
POOL = [(128, 128), (128, 128)]          # GlobalAttention.ques_nn: Linear, GELU, Linear
STEP = [GATE, POOL]                      # configs[1]: one masked layer and the read-out


def test_the_step_is_taken_above_the_skinny_regime_only():
    assert ops.small_mlps_supported(4096, STEP)
    assert ops.small_mlps_supported(1025, STEP)
    assert not ops.small_mlps_supported(1024, STEP)          # isg_linear_skinny keeps its place
    assert ops.linear_route(1024, 128, 128) == "skinny" and ops.linear_route(1025, 128, 128) == "bf16x6"
    assert not ops.small_mlps_supported(0, STEP)
    # without the skinny kernel the same rows ARE bf16x6's
    assert ops.small_mlps_supported(1024, STEP, cfg=dataclasses.replace(ops.CFG, skinny=False))


@pytest.mark.parametrize("width, ok", [(32, True), (64, True), (96, True), (128, True), (160, False), (300, False), (100, False),
                                       (16, False)])
def test_widths(width, ok):
    assert ops.small_mlps_supported(4096, [[(width, width)]]) == ok
    assert ops.small_mlps_supported(4096, [[(128, width)]]) == ok
    assert ops.small_mlps_supported(4096, [[(width, 128)]]) == ok
    assert ops.small_mlps_supported(4096, [[(width, 128), (128, width)]]) == ok


def test_chain_shapes():
    assert ops.small_mlps_supported(2048, [[(128, 96), (64, 128)]])                 # 96 -> 128 -> 64
    assert not ops.small_mlps_supported(2048, [[(128, 96), (64, 96)]])              # the second Linear does not read the first's width
    assert not ops.small_mlps_supported(2048, [[(128, 128)] * 3])                   # three Linears
    assert not ops.small_mlps_supported(2048, [[]])
    assert not ops.small_mlps_supported(2048, [])
    assert ops.small_mlps_supported(2048, [GATE] * 4)
    assert not ops.small_mlps_supported(2048, [GATE] * 5)


def test_inference_on_fp32_rows_only():
    assert not ops.small_mlps_supported(4096, STEP, grad=True)
    assert not ops.small_mlps_supported(4096, STEP, x_dtype=torch.float16)
    assert not ops.small_mlps_supported(4096, STEP, x_dtype=torch.float64)


def test_switches():
    assert ops.Switches().fuse_question_mlps is True
    with ops.configured(fuse_question_mlps=False):
        assert not ops.small_mlps_supported(4096, STEP)
    assert ops.small_mlps_supported(4096, STEP)
    # any switch that takes a Linear off isg_linear_bf16x6 takes the launch with it
    for off in (dict(gemm_backend="torch"), dict(gemm_kernel="panel")):
        cfg = dataclasses.replace(ops.CFG, **off)
        assert ops.linear_route(4096, 128, 128, cfg=cfg) != "bf16x6"
        assert not ops.small_mlps_supported(4096, STEP, cfg=cfg)


def test_modules_are_read_as_chains():
    """ops._mlp_steps / _small_mlps_plan on the modules themselves: Linear / exact GELU / eval Dropout, nothing else; CPU tensors,
    training mode and a tanh GELU are refused before any launch."""
    lin = lambda i, o: torch.nn.Linear(i, o)
    seq = torch.nn.Sequential(lin(128, 128), torch.nn.GELU(), lin(128, 64))
    steps = ops._mlp_steps(seq)
    assert [(m.weight.shape, g) for m, g in steps] == [((128, 128), True), ((64, 128), False)]
    assert ops._mlp_steps(torch.nn.Sequential(lin(128, 128), torch.nn.GELU(approximate="tanh"))) is None
    assert ops._mlp_steps(torch.nn.Sequential(lin(128, 128), torch.nn.ReLU())) is None
    assert ops._mlp_steps(torch.nn.Sequential(torch.nn.GELU(), lin(128, 128))) is None
    drop = torch.nn.Sequential(lin(128, 128), torch.nn.GELU(), torch.nn.Dropout(0.2))
    assert ops._mlp_steps(drop.eval()) is not None and ops._mlp_steps(drop.train()) is None
    with torch.no_grad():
        host = [(seq, torch.zeros(4096, 128))]                                       # rows on the host
        assert ops._small_mlps_plan(host) is None and ops.small_mlps(host, strict=False) is None
        assert ops.small_mlps([], strict=False) is None
        with pytest.raises(ValueError):
            ops.small_mlps(host)


def test_the_cheap_refusal_is_the_rule_on_the_rows_own_width():
    """MGAT.question_side first asks small_mlps_supported on a square Linear of the rows' width (what a host-bound forward
    pays).  That must refuse nothing the full rule takes: at every M and width the rule admits, a Linear's route does not depend
    on N."""
    for M in (1, 1024, 1025, 8191, 8192, 40000):
        for K in (32, 64, 96, 128):
            square = ops.small_mlps_supported(M, [[(K, K)]])
            for N in (32, 64, 96, 128):
                assert ops.small_mlps_supported(M, [[(N, K)]]) == square, (M, N, K)


def test_the_fourth_header_binds_and_the_constants_agree():
    """include/isg_fused.h: its declarations are what _lib_fused binds, the built library exports them under the header's ABI
    version, build() depends on the header, and the limits ops quotes are the header's."""
    import ctypes
    import inspect
    import os
    import re
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib, _lib_fused
    header = open(os.path.join(ge.ROOT, "include", "isg_fused.h")).read()
    body = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", body)) == {"isg_fused_abi_version", "isg_small_mlps", "isg_linear_f16x3_catmul"} == set(_lib_fused.SIGNATURES)
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert _lib_fused.SIGNATURES["isg_small_mlps"] == (ctypes.c_int, [P, I32, I64, P])
    assert not set(_lib_fused.SIGNATURES) & set(_lib.SIGNATURES)
    abi = int(re.search(r"#define ISG_FUSED_ABI_VERSION (\d+)", header).group(1))
    assert _lib_fused.ABI_VERSION == abi == 1
    assert int(re.search(r"#define ISG_SMALL_MLPS_MAX_CHAINS (\d+)", header).group(1)) == ops.SMALL_MLPS_MAX_CHAINS
    assert int(re.search(r"#define ISG_SMALL_MLPS_MAX_WIDTH (\d+)", header).group(1)) == ops.SMALL_MLPS_MAX_WIDTH
    assert int(re.search(r"#define ISG_SMALL_MLPS_FIELDS (\d+)", header).group(1)) == 15
    assert int(re.search(r"#define ISG_CATMUL_MAX_C (\d+)", header).group(1)) == ops.CAT_MUL_MAX_C
    F = ctypes.c_float
    assert _lib_fused.SIGNATURES["isg_linear_f16x3_catmul"] == (ctypes.c_int, [P, P, P, P, P, P, P, I64, I32, I32, I32, I32, P])
    build_checks("isg_fused.h")
    if os.path.exists(_lib.LIB_PATH):
        assert _lib_fused.load().isg_fused_abi_version() == abi


# ---- ops.cat_mul_linear_supported: the answer head's Linear over cat(a, b, a * b) reading a and b ---------------------------------
def test_cat_mul_linear_rule():
    ok = ops.cat_mul_linear_supported
    assert ok(4096, 512, 128) and ok(1025, 512, 128) and ok(4127, 160, 128)
    assert not ok(1024, 512, 128)                        # isg_linear_skinny's rows
    assert ops.linear_route(1025, 512, 384, rowmax_slices=True) == "f16x3_tile"
    assert not ok(8192, 512, 128)                        # the planes32 engine takes the un-fused Linear there
    assert ops.linear_route(8192, 512, 384, rowmax_slices=True) == "h3p"
    assert not ok(0, 512, 128)
    # widths: 32 | C <= 128 and the un-fused route "f16x3_tile" (K = 3C > 128), 32 | N
    assert ok(4096, 512, 64) and ok(4096, 512, 96)
    assert not ok(4096, 512, 32)                         # K = 96: the un-fused Linear is not the tile kernel's
    assert ops.linear_route(4096, 512, 96, rowmax_slices=True) != "f16x3_tile"
    assert not ok(4096, 512, 160) and not ok(4096, 512, 300) and not ok(4096, 512, 100)
    assert not ok(4096, 1842, 128) and not ok(4096, 500, 128)
    # inference on fp32 rows
    assert not ok(4096, 512, 128, grad=True)
    assert not ok(4096, 512, 128, x_dtype=torch.float16)
    # switches
    assert ops.Switches().fuse_cat_mul_linear is True
    with ops.configured(fuse_cat_mul_linear=False):
        assert not ok(4096, 512, 128)
    for off in (dict(gemm_backend="torch"), dict(f16x3_tile=False), dict(gemm_f16x3=False), dict(gemm_kernel="tile")):
        cfg = dataclasses.replace(ops.CFG, **off)
        assert ops.linear_route(4096, 512, 384, rowmax_slices=True, cfg=cfg) != "f16x3_tile"
        assert not ok(4096, 512, 128, cfg=cfg)
