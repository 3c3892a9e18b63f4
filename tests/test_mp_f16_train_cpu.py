"""Host-side checks of training on fp16 feature rows (include/isg_mp_f16_train.h) that need no GPU: the header
declares exactly the new entry points and shares none with another header; header, library, strict twin and binding agree on the
version; the signature is isg_gatv2_mp_bwd's with half row pointers and five strides in front of the stream; the entry point
refuses a bad stride, a missing pointer and a shape without a kernel before any launch; MaskingGATv2Conv.trains_on_half_rows over
its truth table; and the layer restated in plain torch with straight-through roundings (tests/mp_f16_train_restated.py) is the
oracle's fp16_features convolution forward and the identity through each rounding backward."""
import ctypes
import inspect
import os
import re

import torch

from binding_checks import build_checks
from conftest import ROOT

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_mp_f16_train_abi_version", "isg_gatv2_mp_bwd_f16"}


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_mp_f16_train_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_mp_f16_train, _lib_mp_train,
                              _lib_optim, _lib_sampler_train, _lib_sgenc_train, _lib_sparse_out, _lib_topk_rows, _lib_train)
    header = open(os.path.join(ROOT, "include", "isg_mp_f16_train.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", _strip(header)))
    assert declared == set(_lib_mp_f16_train.SIGNATURES) == NAMES
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked,
              _lib_sampler_train, _lib_topk_rows, _lib_mp_train, _lib_sparse_out]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_mp_f16_train.load()
    abi = int(re.search(r"#define ISG_MP_F16_TRAIN_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_mp_f16_train_abi_version() == _lib_mp_f16_train.ABI_VERSION == abi == 1
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_mp_f16_train_abi_version.restype = ctypes.c_int
        assert raw.isg_mp_f16_train_abi_version() == 1, other
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert [m.ABI_VERSION for m in others[1:]] == [1] * 11 and len(others[1:]) == 11
    assert len(_lib_mp_train.SIGNATURES) == 3
    # isg_gatv2_mp_bwd's signature: the three row pointers as `const uint16_t *`, five int32_t strides in front of the stream
    res, args = _lib.SIGNATURES["isg_gatv2_mp_bwd"]
    assert args[-1] is ctypes.c_void_p
    assert _lib_mp_f16_train.SIGNATURES["isg_gatv2_mp_bwd_f16"] == (res, args[:-1] + [ctypes.c_int32] * 5 + args[-1:])

    def params(text, name):
        body = re.search(r"\b%s\s*\(([^)]*)\)" % name, _strip(text)).group(1)
        return [" ".join(p.split()) for p in body.split(",")]

    old = params(open(os.path.join(ROOT, "include", "isg.h")).read(), "isg_gatv2_mp_bwd")
    new = params(header, "isg_gatv2_mp_bwd_f16")
    assert old[:3] == ["const float *x_l", "const float *x_r", "const float *e_proj"]
    assert new[:3] == ["const uint16_t *x_l", "const uint16_t *x_r", "const uint16_t *e_proj"]
    assert new[3:-6] == old[3:-1] and new[-1] == old[-1] == "void *stream"
    assert new[-6:-1] == ["int32_t ld_l", "int32_t ld_r", "int32_t ld_e", "int32_t ld_dl", "int32_t ld_dr"]
    build_checks("isg_mp_f16_train.h")
    assert "_smoke_mp_f16_train(dev)" in inspect.getsource(ge.smoke)
    smoke = inspect.getsource(ge._smoke_mp_f16_train)
    assert "isg_mp_f16_train_abi_version()" in smoke and "gatv2_mp_backward_f16(" in smoke and "gatv2_mp_backward(" in smoke
    from isubgvqa_amd import ops
    assert "mp_f16_train" in ops.COUNTERS
    # K1 is templated on the rows' storage type, the half form has no dropout instantiation, the struct carries the strides
    text = open(os.path.join(ge.CSRC, "isg_mp_bwd.hip")).read()
    assert re.search(r"template <int H, int P, bool F16 = false, bool DROP = false>\s*__global__ [^\n]*void gatv2_mp_bwd_dst_kernel\(", text)
    assert "static_assert(!(F16 && DROP)" in text and "int ld_l4, ld_r4, ld_e4, ld_dl4, ld_dr4;" in text
    assert "atomic" not in re.sub(r"//[^\n]*", "", text).lower(), "the backward kernels use no atomic"


def test_entry_point_refuses_bad_strides_missing_pointers_and_shapes_without_a_kernel():
    from isubgvqa_amd import _lib_mp_f16_train
    bwd = _lib_mp_f16_train.load().isg_gatv2_mp_bwd_f16
    H, C = 4, 8
    HC = H * C

    def b(x_l=P, x_r=P, e=P, d_x_l=P, d_x_r=P, N=8, E=16, H=H, C=C, ld=(0, 0, 0, 0, 0)):
        #          x_l x_r e_proj att alpha g rowptr eid src rowptr_s eid_s dst_s nm em d_x_l d_x_r d_e d_att d_m N E H C slope strides stream
        return bwd(x_l, x_r, e, P, P, P, P, P, P, P, P, P, None, None, d_x_l, d_x_r, P, P, None, N, E, H, C, 0.2, *ld, None)

    for k in range(5):                                    # every stride: 2, HC - 4, HC + 2 and a negative one
        for bad in (2, HC - 4, HC + 2, -HC, 1):
            ld = [0] * 5
            ld[k] = bad
            assert b(ld=ld) == EINVAL, (k, bad)
    assert b(x_l=None) == EINVAL and b(x_r=None) == EINVAL and b(e=None) == EINVAL
    assert b(d_x_l=None) == EINVAL and b(d_x_r=None) == EINVAL
    assert b(x_l=P + 4) == EINVAL and b(e=P + 2) == EINVAL and b(d_x_l=P + 8) == EINVAL          # 8 / 8 / 16 bytes
    assert b(N=-1) == EINVAL
    assert b(H=3) == EUNSUPPORTED and b(C=6) == EUNSUPPORTED and b(H=16, C=4) == EUNSUPPORTED
    assert b(H=8, C=260) == EUNSUPPORTED                                                          # nine channel passes
    assert b(N=0) == 0 and b(N=0, x_l=None, d_x_l=None) == 0                                      # nothing to do, nothing looked at
    assert b(N=0, ld=(2, 0, 0, 0, 0)) == 0 and b(N=0, ld=(-4, 0, 0, 0, 0)) == EINVAL


class _Plan:
    """What rows_dtype reads of a plan."""
    def __init__(self, nmax=40, emax=100):
        self.nmax, self.emax = nmax, emax


def test_trains_on_half_rows_truth_table():
    import test_host_cpu as TH
    from isubgvqa_amd import ops
    half, full, drop = TH._conv_layer(), TH._conv_layer(), TH._conv_layer(dropout=0.1)
    half.feature_dtype = drop.feature_dtype = torch.float16
    for m in (half, full, drop):
        m.train()
    plan = _Plan()
    assert half.trains_on_half_rows(plan, "unfused", True, False) is True
    assert half.trains_on_half_rows(None, "unfused", True, False) is True
    assert full.trains_on_half_rows(plan, "unfused", True, False) is False                      # fp32 rows
    assert half.trains_on_half_rows(plan, "unfused", False, False) is False                     # autograd does not record
    assert drop.trains_on_half_rows(plan, "unfused", True, False) is False                      # attention dropout is active
    assert drop.eval().trains_on_half_rows(plan, "unfused", True, False) is True                # ... and is not in eval()
    assert half.trains_on_half_rows(plan, "unfused", True, True) is False                       # e_proj handed in
    for conv in ("layer_conv", "tile_conv", "pair"):
        assert half.trains_on_half_rows(plan, conv, True, False) is False                       # a fused route
    for big in (_Plan(nmax=ops.GK_NCAP_L + 1), _Plan(emax=ops.GK_ECAP_L + 1)):                  # an oversize plan keeps fp32 rows
        assert half.rows_dtype(big) == torch.float32 and half.trains_on_half_rows(big, "unfused", True, False) is False
    assert half.trains_on_half_rows(_Plan(ops.GK_NCAP_L, ops.GK_ECAP_L), "unfused", True, False) is True
    # autograd sends every layer to the un-fused route (ops.conv_route), so a recording half-row layer always meets the Function
    assert half.route(TH._StubPlan(), 128, torch.empty(0, 128)).conv == "unfused"
    assert "trains_on_half_rows(" in inspect.getsource(type(half).forward)
    assert "inference only" not in inspect.getsource(type(half).__init__)


def _layer(seed, N, E, H, C, Cin, K, B=2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    HC = H * C
    sd = {"c.lin_l.weight": r(HC, Cin) / Cin ** 0.5, "c.lin_l.bias": r(HC), "c.lin_r.weight": r(HC, Cin) / Cin ** 0.5,
          "c.lin_r.bias": r(HC), "c.lin_edge.weight": r(HC, K) / K ** 0.5, "c.att": r(1, H, C) / C ** 0.5, "c.bias": r(HC)}
    batch = torch.arange(N) * B // N
    ei = torch.randint(0, N // B, (2, E), generator=g) + (torch.arange(E) * B // E) * (N // B)
    return sd, r(N, Cin), ei, batch, r(E, K), r(B, Cin)


def test_restated_forward_is_the_oracles_fp16_convolution():
    import mp_f16_train_restated as R
    from oracle import model as OM
    for seed, (N, E, H, C, Cin, K) in enumerate([(10, 40, 2, 4, 8, 4), (16, 90, 4, 8, 12, 8)]):
        sd, x, ei, batch, ea, ins = _layer(seed, N, E, H, C, Cin, K)
        for fp16 in (True, False):
            cfg = OM.PathConfig(heads=H, fp16_features=fp16)
            want, mask, want_alpha = OM.gatv2_conv_forward(sd, "c", x, ei, batch, ea, ins, None, 1.0, cfg)
            got, alpha = R.conv(sd, "c", x, ei, batch, ea, ins, H, cfg.negative_slope, half=fp16)
            assert mask is None and got.dtype == torch.float32
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(alpha, want_alpha), (seed, fp16)
        assert not torch.equal(got, R.conv(sd, "c", x, ei, batch, ea, ins, H)[0])   # the rounding is felt
        half = R.conv(sd, "c", x, ei, batch, ea, ins, H)[0]
        assert torch.equal(half, half.half().float())


def test_restated_gradient_through_a_rounding_is_the_identity():
    import mp_f16_train_restated as R
    g = torch.Generator().manual_seed(3)
    t = (torch.randn(7, 5, generator=g) * 1e-3).requires_grad_(True)          # 1e-3: gradients a half tensor would flush
    w = torch.randn(7, 5, generator=g) * 1e-6
    y = R.ste(t)
    assert torch.equal(y.detach(), t.detach().half().float()) and not torch.equal(y.detach(), t.detach())
    (y * w).sum().backward()
    assert torch.equal(t.grad, w) and float(w.abs().min()) < 6e-8 and bool((w.half() == 0).any())
    # the layer: every gradient equals that of the un-rounded function evaluated at rows it is handed already rounded --
    # checked where that is expressible, on the output rounding: d out / d bias is exactly the upstream gradient's column sums
    sd, x, ei, batch, ea, ins = _layer(5, 10, 40, 2, 4, 8, 4)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out, _ = R.conv(sd, "c", x, ei, batch, ea, ins, 2)
    up = torch.randn(out.shape, generator=g) * 1e-6
    (out * up).sum().backward()
    assert torch.equal(sd["c.bias"].grad, up.sum(0))
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0 for v in sd.values())
