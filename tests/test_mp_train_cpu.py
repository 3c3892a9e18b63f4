"""Host-side checks of the attention dropout of the message passing (include/isg_mp_train.h) that need no GPU: the
header declares exactly the new entry points and shares none with another header; header, library, strict twin and binding agree
on the version; the two signatures are the old ones with (p, seed) in front of the stream; the entry points refuse a bad p and a
null alpha before they look at anything else; the keep rule restated in tests/mp_dropout_restated.py gives the hand-computed
answers of tests/test_text_train_cpu.py; ops.conv_route sends a layer that drops attention weights to the un-fused kernels and
changes nothing else; and the constructors pass the keyword down without touching a model built without it."""
import argparse
import ctypes
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

EINVAL = -1
P = 4096                        # any non-null address; nothing dereferences it on the paths tested here
NAMES = {"isg_mp_train_abi_version", "isg_gatv2_mp_fwd_dropout", "isg_gatv2_mp_bwd_dropout"}


def test_mp_train_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_mp_train, _lib_optim,
                              _lib_sampler_train, _lib_sgenc_train, _lib_topk_rows, _lib_train)
    header = open(os.path.join(ROOT, "include", "isg_mp_train.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_mp_train.SIGNATURES) == NAMES
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked,
              _lib_sampler_train, _lib_topk_rows]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_mp_train.load()
    abi = int(re.search(r"#define ISG_MP_TRAIN_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_mp_train_abi_version() == _lib_mp_train.ABI_VERSION == abi == 1
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_mp_train_abi_version.restype = ctypes.c_int
        assert raw.isg_mp_train_abi_version() == 1, other
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert (_lib_train.ABI_VERSION, _lib_optim.ABI_VERSION, _lib_fused.ABI_VERSION, _lib_sgenc_train.ABI_VERSION, _lib_dist.ABI_VERSION,
            _lib_linear_train.ABI_VERSION, _lib_masked.ABI_VERSION, _lib_sampler_train.ABI_VERSION,
            _lib_topk_rows.ABI_VERSION) == (1,) * 9
    # the old signatures with (float p, uint64_t seed) in front of the stream
    sig, old = _lib_mp_train.SIGNATURES, _lib.SIGNATURES
    for new, was in (("isg_gatv2_mp_fwd_dropout", "isg_gatv2_mp_fwd"), ("isg_gatv2_mp_bwd_dropout", "isg_gatv2_mp_bwd")):
        res, args = old[was]
        assert args[-1] is ctypes.c_void_p
        assert sig[new] == (res, args[:-1] + [ctypes.c_float, ctypes.c_uint64] + args[-1:]), new
    build_checks("isg_mp_train.h")
    assert "_smoke_mp_dropout(dev)" in inspect.getsource(ge.smoke) and "dropout_p=p" in inspect.getsource(ge._smoke_mp_dropout)
    from isubgvqa_amd import ops
    assert "mp_dropout" in ops.COUNTERS
    # dropout is a template parameter of all five kernels, and both argument structs carry its fields
    for f, kernels in (("isg_mp.hip", ("gatv2_mp_kernel",)), ("isg_mp_graph.hip", ("gatv2_mp_graph_kernel", "gatv2_mp_graph_flat_kernel")),
                       ("isg_mp_bwd.hip", ("gatv2_mp_bwd_dst_kernel", "gatv2_mp_bwd_src_kernel"))):
        text = open(os.path.join(ge.CSRC, f)).read()
        for k in kernels:
            assert re.search(r"template <[^>]*bool DROP = false>\s*__global__ [^\n]*void " + k + r"\(", text), (f, k)
    for f in ("isg_mp.hpp", "isg_mp_bwd.hip"):
        text = open(os.path.join(ge.CSRC, f)).read()
        assert "drop_p" in text and "uint64_t drop_seed;" in text, f


def test_entry_points_refuse_a_bad_p_and_a_null_alpha_before_any_launch():
    from isubgvqa_amd import _lib_mp_train
    lib = _lib_mp_train.load()
    fwd, bwd = lib.isg_gatv2_mp_fwd_dropout, lib.isg_gatv2_mp_bwd_dropout

    def f(p, alpha=P, N=8, seed=3):
        #          x_l x_r e_proj att bias rowptr eid src nm em out alpha N E H C slope gptr geptr dst B nmax emax ld_l ld_r ld_e p seed stream
        return fwd(P, P, P, P, None, P, P, P, None, None, P, alpha, N, 16, 4, 8, 0.2, None, None, None, 0, 0, 0, 0, 0, 0, p, seed, None)

    def b(p, N=8, seed=3):
        #          x_l x_r e_proj att alpha g rowptr eid src rowptr_s eid_s dst_s nm em d_x_l d_x_r d_e d_att d_m N E H C slope p seed stream
        return bwd(P, P, P, P, P, P, P, P, P, P, P, P, None, None, P, P, P, P, None, N, 16, 4, 8, 0.2, p, seed, None)

    for bad in (-0.1, -1e-30, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert f(bad) == EINVAL, bad
        assert b(bad) == EINVAL, bad
        assert f(bad, N=0) == EINVAL and b(bad, N=0) == EINVAL, bad        # refused before "nothing to do"
    assert f(0.3, alpha=None) == EINVAL and f(0.0, alpha=None) == EINVAL      # alpha is required here
    assert f(0.3, alpha=None, N=0) == EINVAL
    # a good p and nothing to do: ISG_OK without a launch, at p == 0 and p > 0, whatever the seed
    for p in (0.0, 0.3, 0.999):
        assert f(p, N=0, seed=2 ** 64 - 1) == 0 and b(p, N=0, seed=2 ** 64 - 1) == 0
    # everything else is what the two existing entry points say
    assert fwd(P, P, P, P, None, P, P, P, None, None, P, P, -1, 16, 4, 8, 0.2, None, None, None, 0, 0, 0, 0, 0, 0, 0.3, 0, None) == EINVAL
    assert fwd(P, P, P, P, None, P, P, P, None, None, P, P, 8, 16, 4, 6, 0.2, None, None, None, 0, 0, 0, 0, 0, 0, 0.3, 0, None) == -2   # 4 !| C
    assert fwd(None, P, P, P, None, P, P, P, None, None, P, P, 8, 16, 4, 8, 0.2, None, None, None, 0, 0, 0, 0, 0, 0, 0.3, 0, None) == EINVAL
    assert bwd(P, P, P, P, P, None, P, P, P, P, P, P, None, None, P, P, P, P, None, 8, 16, 4, 8, 0.2, 0.3, 0, None) == EINVAL
    assert bwd(P, P, P, P, P, P, P, P, P, P, P, P, None, None, P, P, P, P, None, 8, 16, 4, 6, 0.2, 0.3, 0, None) == -2


def test_keep_rule_restated_gives_the_hand_computed_blocks():
    """Blocks (0, 0) under seed 0 and (5, 1) under 0x0123456789ABCDEF, the known answers of tests/test_text_train_cpu.py: here the
    first counter word is the edge id and the second is head >> 2."""
    import numpy as np
    import mp_dropout_restated as R
    from oracle import philox
    assert philox.philox4x32_10((0, 0, 0x1571, 0x9E37), (0, 0)) == (0x4343BE88, 0xB4D85013, 0x5FBCD453, 0x3A00EED9)
    # edge 0, head 0, seed 0: word 0, u = 0.2627524137496948
    assert bool(R.keep_mask(0, 1, 4, 0.25)[0, 0]) and not bool(R.keep_mask(0, 1, 4, 0.27)[0, 0])
    u = [w >> 8 for w in (0x4343BE88, 0xB4D85013, 0x5FBCD453, 0x3A00EED9)]
    for h in range(4):                                        # the four heads of edge 0 are the four words of that block
        at = float(np.float32(u[h] / 2 ** 24))
        assert bool(R.keep_mask(0, 1, 4, at)[0, h]), h                              # `>=` in fp32: u == p keeps
        assert not bool(R.keep_mask(0, 1, 4, float(np.nextafter(np.float32(at), np.float32(1))))[0, h]), h
    # edge 5, head 6, seed 0x0123456789ABCDEF: block (5, 6 >> 2 = 1), word 2, u = 0.12496310472488403
    seed = 0x0123456789ABCDEF
    assert philox.philox4x32_10((5, 1, 0x1571, 0x9E37), (0x89ABCDEF, 0x01234567)) == (0xD0922A6A, 0xA943BC15, 0x1FFD95EB, 0xFF71980D)
    m = R.keep_mask(seed, 6, 8, 0.125)
    assert tuple(m.shape) == (6, 8) and not bool(m[5, 6]) and bool(R.keep_mask(seed, 6, 8, 0.1249)[5, 6])
    assert bool(m[5, 4]) and bool(m[5, 7])                    # words 0 and 3 of the same block: 0.8147..., 0.9978...
    assert bool(R.keep_mask(seed, 6, 8, float(np.float32((0x1FFD95EB >> 8) / 2 ** 24)))[5, 6])
    # heads 0..3 of an edge come from block (e, 0): H = 4 is the first half of H = 8
    assert torch.equal(R.keep_mask(seed, 50, 8, 0.5)[:, :4], R.keep_mask(seed, 50, 4, 0.5))
    # edge_ids: the row of an edge follows its id
    perm = torch.randperm(50, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.keep_mask(seed, 50, 8, 0.5, edge_ids=perm.numpy()), R.keep_mask(seed, 50, 8, 0.5)[perm])
    assert bool(R.keep_mask(seed, 3, 5, 0.0).all())
    assert R.inv_keep(0.5) == 2.0 and R.inv_keep(0.1) == float(np.float32(1) / np.float32(0.9)) and R.inv_keep(0.0) == 1.0
    f = R.factor(seed, 6, 8, 0.125, torch.float64)
    assert f.dtype == torch.float64 and float(f[5, 6]) == 0.0 and float(f[5, 4]) == R.inv_keep(0.125)
    # the seed is taken modulo 2^64, both halves used
    assert not torch.equal(R.keep_mask(1, 200, 4, 0.5), R.keep_mask(1 << 32, 200, 4, 0.5))
    assert torch.equal(R.keep_mask(-1, 200, 4, 0.5), R.keep_mask(2 ** 64 - 1, 200, 4, 0.5))


def test_restated_message_passing_without_dropout_is_the_oracle():
    import mp_dropout_restated as R
    from oracle import model as OM
    g = torch.Generator().manual_seed(5)
    N, E, H, C = 9, 30, 2, 4
    ei = torch.randint(0, N, (2, E), generator=g)
    x_l, x_r, e = (torch.randn(n, H, C, generator=g, dtype=torch.float64) for n in (N, N, E))
    att, m = torch.randn(1, H, C, generator=g, dtype=torch.float64), torch.rand(E, 1, generator=g, dtype=torch.float64)
    for mask in (None, m):
        want = OM.gatv2_message_passing(x_l, x_r, e, att, ei, mask, 0.2)
        for r in (None, torch.ones(E, H, dtype=torch.float64)):
            got = R.message_passing(x_l, x_r, e, att, ei, mask, 0.2, r)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a dropped edge leaves the sum, alpha keeps it
    r = R.factor(7, E, H, 0.5, torch.float64)
    assert 0 < int((r == 0).sum()) < E * H
    out, alpha = R.message_passing(x_l, x_r, e, att, ei, None, 0.2, r)
    assert torch.equal(alpha, OM.gatv2_message_passing(x_l, x_r, e, att, ei, None, 0.2)[1]) and not torch.equal(out, want[0])


def test_attn_dropout_selects_the_unfused_route_and_nothing_else():
    """conv_route(attn_dropout=True): "unfused" wherever the layer would run fused (layer_conv, tile_conv, the pair); the whole route
    unchanged where it was un-fused already; attn_dropout=False is the default and the function as it was."""
    import test_host_cpu as TH
    from isubgvqa_amd import ops
    assert inspect.signature(ops.conv_route).parameters["attn_dropout"].default is False
    fused = set()
    for facts, switches, route in TH.CONV_ROUTES:
        cfg = ops.Switches(**switches)
        kw = {**TH._CONV, **facts}
        plain = ops.conv_route(cfg=cfg, **kw)
        assert plain == route == ops.conv_route(cfg=cfg, attn_dropout=False, **kw)
        dropped = ops.conv_route(cfg=cfg, attn_dropout=True, **kw)
        assert dropped.conv == "unfused" and dropped.e_proj and dropped.gate_rows, (facts, switches, dropped)
        if plain.conv == "unfused":
            assert dropped == plain, (facts, switches)
        else:
            fused.add(plain.conv)
            assert dropped.gate != "planes", (facts, switches)          # the planes are what isg_gatv2_layer_conv reads
            assert dropped == ops.conv_route(cfg=cfg, **{**kw, "e_proj_given": True}), (facts, switches)
    assert fused == {"layer_conv", "tile_conv", "pair"}


def test_a_layer_routes_by_its_mode():
    """train() with dropout > 0 is un-fused, with and without autograd; eval() routes as a layer with dropout = 0; so does
    train() at dropout = 0."""
    import test_host_cpu as TH
    from isubgvqa_amd.models import mgat_v2_conv as MC
    assert MC.ATTN_DROPOUT_SEED_OFFSET == 8192
    ea = torch.empty(0, 128)
    plain, drop = TH._conv_layer(), TH._conv_layer(dropout=0.1)
    assert plain.dropout == 0.0 and drop.dropout == 0.1
    with torch.no_grad():
        plan = TH._StubPlan()
        plain.eval(), drop.eval()
        want = plain.route(plan, 128, ea)
        assert want.conv == "layer_conv" and drop.route(plan, 128, ea) == want and not drop.attn_dropout_active()
        drop.train(), plain.train()
        assert drop.attn_dropout_active() and not plain.attn_dropout_active()
        assert drop.route(plan, 128, ea).conv == "unfused" and plain.route(plan, 128, ea) == want      # under no_grad too
        drop.eval()
        assert drop.route(plan, 128, ea) == want                                    # the memo is keyed by the fact
    drop.train()
    assert drop.route(TH._StubPlan(), 128, ea).conv == "unfused"
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="0 <= dropout < 1"):
            TH._conv_layer(dropout=bad)
    from isubgvqa_amd import ops
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            ops.gatv2_mp(*(torch.zeros(1, 4),) * 4, None, 1, dropout_p=bad)
        with pytest.raises(ValueError, match="0 <= p < 1"):
            ops.gatv2_mp_backward(*(torch.zeros(1, 4),) * 6, None, 1, dropout_p=bad)


def test_constructors_pass_attn_dropout_down_and_a_namespace_without_it_builds_todays_model():
    from isubgvqa_amd import checkpoint, synthetic
    from isubgvqa_amd.models import build_model
    from isubgvqa_amd.models.mgat import MGAT
    for cls in (MGAT, synthetic.AnswerModel):
        assert inspect.signature(cls.__init__).parameters["attn_dropout"].default == 0.0, cls
    kw = dict(channels=16, num_ins=2, use_instr=True, masking_thresholds=[1.0, 0.15], use_topk=True, sampler_type="gumbel", sample_k=5)
    torch.manual_seed(0)
    g0 = MGAT(**kw)
    torch.manual_seed(0)
    g1 = MGAT(attn_dropout=0.2, dropout=0.5, **kw)
    assert [c.dropout for c in g0.convs] == [0.0, 0.0] and [c.dropout for c in g1.convs] == [0.2, 0.2]
    assert g1.dropout == 0.5 and g0.dropout == 0.0, "the reference's own `dropout` argument of MGAT is stored and unused"
    assert list(g0.state_dict()) == list(g1.state_dict()), "dropout adds no parameter"
    assert all(torch.equal(a, b) for a, b in zip(g0.state_dict().values(), g1.state_dict().values()))
    a = synthetic.AnswerModel(16, 2, (1.0, 0.15), "imle", 5, attn_dropout=0.1, num_answers=7)
    assert [c.dropout for c in a.gat_seq.convs] == [0.1, 0.1]
    assert [c.dropout for c in synthetic.AnswerModel(16, 2, (1.0, 0.15), "imle", 5, num_answers=7).gat_seq.convs] == [0.0, 0.0]
    d = dict(text_sampling=False, general_hidden_dim=32, distributed=False, mgat_layers=2, use_all_instrs=False,
             use_global_mask=False, node_classification=False, sampler_type="imle", sample_k=5, nb_samples=1,
             alpha=1.0, beta=10.0, tau=1.0, use_masking=True, use_instruction=1, use_mgat=True,
             mgat_masks=[1.0, 0.15], use_topk=True, interpretable_mode=False, concat_instr=0, embed_cat=0,
             device="cpu", text_vocab_size=64, sg_vocab_size=40)
    assert "attn_dropout" not in d
    torch.manual_seed(0)
    m = build_model(argparse.Namespace(**d), None)
    assert all(c.dropout == 0.0 and not c.train().attn_dropout_active() for c in m.gat_seq.convs)
    torch.manual_seed(0)
    b = build_model(argparse.Namespace(**d, attn_dropout=0.1), None)
    assert all(c.dropout == 0.1 for c in b.gat_seq.convs)
    assert list(m.state_dict()) == list(b.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(m.state_dict().values(), b.state_dict().values()))
    assert checkpoint._ARG_DEFAULTS["attn_dropout"] == 0.0
