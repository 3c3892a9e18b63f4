"""Host-side checks of the --concat_instr variant (include/isg_concat.h) that need no GPU: the header declares
exactly the new entry points and shares none with another header; header, library, strict twin and binding agree on the version;
the signature; the entry point refuses bad arguments before anything is dereferenced; ops.conv_route with the new fact over its
truth table (every existing row at the default unchanged); the constructors, parameter names and shapes; and the restatement of
tests/concat_instr_restated.py against the oracle on a reference-made golden."""
import ctypes
import glob
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_concat_abi_version", "isg_linear_bf16x6_rowbias", "isg_segment_range_sum"}
GOLDEN = os.path.join(ROOT, "tests", "golden")
G5 = sorted(glob.glob(os.path.join(GOLDEN, "g5_mgat_*.pt")))


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_concat_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_concat, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_mp_f16_train,
                              _lib_mp_train, _lib_optim, _lib_sampler_train, _lib_sgenc_train, _lib_sparse_out, _lib_topk_rows,
                              _lib_train)
    header = open(os.path.join(ROOT, "include", "isg_concat.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", _strip(header)))
    assert declared == set(_lib_concat.SIGNATURES) == NAMES
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked,
              _lib_sampler_train, _lib_topk_rows, _lib_mp_train, _lib_sparse_out, _lib_mp_f16_train]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_concat.load()
    abi = int(re.search(r"#define ISG_CONCAT_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_concat_abi_version() == _lib_concat.ABI_VERSION == abi == 1
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_concat_abi_version.restype = ctypes.c_int
        assert raw.isg_concat_abi_version() == 1, other
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 12
    # (a, w_planes, p, ldp, seg, S, d, d_is_f16, M, N, K, lda, ldd, act, stream)
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _lib_concat.SIGNATURES["isg_linear_bf16x6_rowbias"] == (
        ctypes.c_int, [ptr, ptr, ptr, i32, ptr, i32, ptr, i32, i64, i32, i32, i32, i32, i32, ptr])
    body = re.search(r"\bisg_linear_bf16x6_rowbias\s*\(([^)]*)\)", _strip(header)).group(1)
    assert [" ".join(p.split()) for p in body.split(",")] == [
        "const float *a", "const uint16_t *w_planes", "const float *p", "int32_t ldp", "const int32_t *seg", "int32_t S", "void *d",
        "int32_t d_is_f16", "int64_t M", "int32_t N", "int32_t K", "int32_t lda", "int32_t ldd", "int32_t act", "void *stream"]
    # (rowptr, g, ldg, out, ldo, S, M, C, stream)
    assert _lib_concat.SIGNATURES["isg_segment_range_sum"] == (ctypes.c_int, [ptr, ptr, i32, ptr, i32, i32, i64, i32, ptr])
    build_checks("isg_concat.h")
    assert "_smoke_linear_rowbias(dev)" in inspect.getsource(ge.smoke)
    smoke = inspect.getsource(ge._smoke_linear_rowbias)
    assert "isg_concat_abi_version()" in smoke and "linear_rowbias(" in smoke
    from isubgvqa_amd import ops
    assert "linear_rowbias" in ops.COUNTERS
    text = open(os.path.join(ge.CSRC, "isg_gemm.hip")).read()
    assert re.search(r"template <int ACT, int DBG, bool A16, bool D16, bool XCD, bool DUAL = false, bool ROWB = false>", text)
    assert "atomic" not in re.sub(r"//[^\n]*", "", text).lower(), "the GEMM uses no atomic"
    text = open(os.path.join(ge.CSRC, "isg_concat.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", text).lower(), "the range sum uses no atomic"


def test_entry_point_refuses_bad_arguments_before_anything_is_dereferenced():
    from isubgvqa_amd import _lib_concat
    fn = _lib_concat.load().isg_linear_bf16x6_rowbias

    def call(a=P, w=P, p=P, ldp=128, seg=P, S=3, d=P, f16=0, M=100, N=128, K=128, lda=128, ldd=128, act=0):
        return fn(a, w, p, ldp, seg, S, d, f16, M, N, K, lda, ldd, act, None)

    assert call(p=None) == EINVAL and call(seg=None) == EINVAL and call(a=None) == EINVAL and call(w=None) == EINVAL
    assert call(d=None) == EINVAL
    assert call(ldp=127) == EINVAL and call(ldp=0) == EINVAL and call(S=0) == EINVAL and call(S=-1) == EINVAL
    assert call(M=-1) == EINVAL and call(N=0) == EINVAL and call(K=0) == EINVAL and call(lda=124) == EINVAL
    assert call(ldd=127) == EINVAL and call(act=3) == EINVAL and call(act=-1) == EINVAL
    # wherever isg_linear_bf16x6 says so: 4 !| K, 4 !| lda, a misaligned a, more than 65535 row tiles; ReLU on half rows
    assert call(K=126, lda=126) == EUNSUPPORTED and call(lda=130) == EUNSUPPORTED and call(a=P + 4) == EUNSUPPORTED
    assert call(M=65536 * 128) == EUNSUPPORTED and call(f16=1, act=2) == EUNSUPPORTED
    # nothing to do: nothing is looked at beyond the numbers
    assert call(M=0) == 0 and call(M=0, a=None, w=None, p=None, seg=None, d=None) == 0
    assert call(M=0, ldp=127) == EINVAL and call(M=0, S=0) == EINVAL


def test_range_sum_refuses_bad_arguments_before_anything_is_dereferenced():
    from isubgvqa_amd import _lib_concat
    fn = _lib_concat.load().isg_segment_range_sum

    def call(rowptr=P, g=P, ldg=128, out=P, ldo=128, S=3, M=100, C=128):
        return fn(rowptr, g, ldg, out, ldo, S, M, C, None)

    assert call(rowptr=None) == EINVAL and call(g=None) == EINVAL and call(out=None) == EINVAL
    assert call(ldg=127) == EINVAL and call(ldo=127) == EINVAL and call(C=0) == EINVAL and call(S=-1) == EINVAL and call(M=-1) == EINVAL
    assert call(M=1 << 31) == EUNSUPPORTED
    assert call(S=0) == 0 and call(S=0, rowptr=None, g=None, out=None) == 0 and call(S=0, ldg=3) == EINVAL


def test_conv_route_with_the_concat_fact():
    """concat_instr=True: never a gate, never a graph-tile kernel -- "pair" where the fused logits run, "unfused" elsewhere; the
    default leaves every row of the existing truth table where the parent has it."""
    import test_host_cpu as TH
    from isubgvqa_amd import ops
    assert inspect.signature(ops.conv_route).parameters["concat_instr"].default is False
    for facts, switches, route in TH.CONV_ROUTES:
        kw = {**TH._CONV, **facts}
        cfg = ops.Switches(**switches)
        assert ops.conv_route(cfg=cfg, **kw) == route == ops.conv_route(cfg=cfg, concat_instr=False, **kw)
        cat = ops.conv_route(cfg=cfg, concat_instr=True, **kw)
        assert cat.gate == "none" and cat.gate_rows is True and cat.conv in ("pair", "unfused") and cat.e_proj == (cat.conv == "unfused")
        if route[0] == "unfused":
            assert cat.conv == "unfused", (facts, switches)
        elif kw.get("rows_dtype", torch.float32) == torch.float32:
            assert cat.conv == "pair", (facts, switches)
    base = dict(TH._CONV)
    # C = 128: the true input width is 256; C = 64: it is 128 and still no layer_conv shape
    assert ops.conv_route(**{**base, "in_channels": 256}, concat_instr=True) == ("pair", "none", True, False)
    c64 = {**base, "channels": 64, "in_channels": 128, "edge_dim": 64}
    assert ops.conv_route(**c64).conv == "pair" and ops.conv_route(**{**c64, "channels": 128, "edge_dim": 128}).conv == "layer_conv"
    assert ops.conv_route(**c64, concat_instr=True) == ("pair", "none", True, False)
    assert ops.conv_route(**{**base, "in_channels": 128}, concat_instr=True) == ("pair", "none", True, False)
    assert ops.conv_route(**{**base, "in_channels": 256, "grad": True}, concat_instr=True) == ("unfused", "none", True, True)
    assert ops.conv_route(**{**base, "in_channels": 256, "attn_dropout": True}, concat_instr=True) == ("unfused", "none", True, True)
    assert ops.conv_route(**{**base, "in_channels": 256, "rows_dtype": torch.float16}, concat_instr=True).conv == "pair"
    assert ops.conv_route(**{**base, "in_channels": 256, "rows_dtype": torch.float16, "edge_dim": 64}, concat_instr=True).conv == "unfused"
    # the layer asks with its TRUE width, whatever the caller read off the node rows, and the fact is part of its memo key
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    layer = MaskingGATv2Conv(128, 64, heads=4, edge_dim=64, add_self_loops=False, masking_threshold=1.0, use_instr=True,
                             concat_instr=True)
    plain = TH._conv_layer(128, 128)
    with torch.no_grad():
        plan = TH._StubPlan()
        assert layer.route(plan, 64, torch.empty(0, 64)) == ("pair", "none", True, False) and plan.asked == 0
        assert plain.route(plan, 128, torch.empty(0, 128)) == ("layer_conv", "planes", False, False)
        assert any("route" in k and True in k[-1:] for k in plan.memo() if isinstance(k, tuple))


def test_constructors():
    from isubgvqa_amd.models.mgat import MGAT
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    import isubgvqa_amd.models.mgat_v2_conv as MC
    assert MC.CONCAT_SPLIT in (True, False)
    kw = dict(heads=2, edge_dim=8, add_self_loops=False, masking_threshold=0.15, use_instr=True, use_topk=True,
              sampler_type="imle", sample_k=3)
    layer = MaskingGATv2Conv(16, 8, concat_instr=True, **kw)
    assert layer.concat_instr is True and layer.in_channels == 16 and layer.mask.dim_nodes == 16
    with pytest.raises(NotImplementedError, match="use_all_instrs"):
        MaskingGATv2Conv(16, 8, use_all_instrs=True, **kw)
    with pytest.raises(NotImplementedError, match="use_all_instrs"):
        MaskingGATv2Conv(16, 8, concat_instr=True, use_all_instrs=True, **kw)
    with pytest.raises(ValueError, match="concat_instr"):
        MaskingGATv2Conv(15, 8, concat_instr=True, **kw)
    stack = MGAT(channels=8, num_ins=2, heads=2, use_instr=True, masking_thresholds=[1.0, 0.15], use_topk=True,
                 concat_instr=True, sampler_type="imle", sample_k=3)
    assert stack.in_channels == 16 and all(c.concat_instr and c.in_channels == 16 for c in stack.convs)


@pytest.mark.parametrize("C", [8, 64, 300])
def test_parameter_names_and_shapes(C):
    """The state_dict of a concat_instr model has the default model's keys; lin_l / lin_r are [H C, 2 C] and the node gate's
    node_nn.0 is [C, 2 C] (mgat.py:41-44, mgat_v2_conv.py:63-84, masking.py:76), each ONE tensor."""
    from isubgvqa_amd import synthetic
    H = 4
    kw = dict(channels=C, layers=2, masks=(1.0, 0.15), sampler="imle", sample_k=3, heads=H)
    cat, plain = synthetic.AnswerModel(concat_instr=True, **kw), synthetic.AnswerModel(**kw)
    a, b = cat.state_dict(), plain.state_dict()
    assert list(a) == list(b)
    wide = {f"gat_seq.convs.{i}.{n}.weight": (H * C, 2 * C) for i in range(2) for n in ("lin_l", "lin_r")}
    wide.update({f"gat_seq.convs.{i}.mask.node_nn.0.weight": (C, 2 * C) for i in range(2)})
    for k in a:
        assert tuple(a[k].shape) == wide.get(k, tuple(b[k].shape)), k
    assert all(tuple(b[k].shape) == (s[0], C) for k, s in wide.items())


@pytest.mark.parametrize("path", G5[:2], ids=[os.path.basename(p) for p in G5[:2]])
def test_restatement_reproduces_the_oracle_when_the_instruction_half_is_zero(path):
    """cat(x', u[batch]) [W | 0]^T = x' W^T: with the instruction columns of lin_l, lin_r and node_nn.0 zeroed and x' =
    gelu(x * u[batch]) handed in, the restated concat layer is oracle.model.gatv2_conv_forward of the golden."""
    import concat_instr_restated as R
    from oracle import model as OM
    from test_oracle_golden import _cfg
    g = torch.load(path, map_location="cpu", weights_only=False)
    cfg, li = _cfg(g), g["conv_layer"]
    p = f"gat_seq.convs.{li}"
    sd = dict(g["sd"])
    for k in (f"{p}.lin_l.weight", f"{p}.lin_r.weight", f"{p}.mask.node_nn.0.weight"):
        sd[k] = torch.cat((sd[k], torch.zeros_like(sd[k])), 1)
    ins = g["instr"][li]
    want, want_mask, want_alpha = OM.gatv2_conv_forward(g["sd"], p, g["x"], g["edge_index"], g["batch"], g["edge_attr"], ins,
                                                        g["glf"], cfg.masking_thresholds[li], cfg, g["conv_noise"])
    pre = OM.P.gelu(g["x"] * ins[g["batch"]])
    got, mask, alpha = R.conv(sd, p, pre, g["edge_index"], g["batch"], g["edge_attr"], ins, g["glf"], cfg.masking_thresholds[li],
                              cfg, g["conv_noise"])
    assert (mask is None) == (want_mask is None) and (mask is None or torch.equal(mask, want_mask))
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-6) and torch.allclose(alpha, want_alpha, atol=1e-7, rtol=1e-6)
    # and the instruction half is felt when it is not zero
    sd[f"{p}.lin_l.weight"] = sd[f"{p}.lin_l.weight"] + 0.01
    assert not torch.allclose(R.conv(sd, p, pre, g["edge_index"], g["batch"], g["edge_attr"], ins, g["glf"],
                                     cfg.masking_thresholds[li], cfg, g["conv_noise"])[0], want, atol=1e-4)


def test_separated_rejects_near_ties_of_real_nodes_only():
    import concat_instr_restated as R
    counts = torch.tensor([4, 1])
    dense = torch.tensor([[0.9, 0.5, 0.5 - 1e-5, 0.1], [0.7, 0.0, 0.0, 0.0]], dtype=torch.float64)
    assert not R.separated(dense, 2, counts)                  # row 0: 2nd and 3rd score 1e-5 apart
    assert R.separated(dense, 1, counts)                      # k = 1: 0.9 | 0.5 and 0.7 | pad
    assert R.separated(dense[1:], 2, counts[1:])              # two pads tie: no real node is involved
    assert not R.separated(dense[1:] * torch.tensor([1.0, 1.0, 1.0, 1.0]) - torch.tensor([[0.0, -1e-5, 0.0, 0.0]]), 2,
                           torch.tensor([2]))                 # a real node 1e-5 from a pad
