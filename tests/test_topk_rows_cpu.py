"""Host-side checks of the per-graph node budget (include/isg_topk_rows.h, csrc/isg_topk_rows.hip) that need no
GPU: the header declares exactly the new entry points and shares none with another header; header, library and binding agree on
the version; the entry points refuse what their comments say before they touch a device; the budget rule restated in torch gives
the ceilings worked out by hand; the restated per-row samplers (tests/topk_rows_restated.py) equal the oracle's scalar-k samplers
on the rows that carry each k; and the constructors pass the two new keywords down without touching a model built without them."""
import argparse
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null address; nothing dereferences it on the paths tested here

NODE_COUNTS = (1, 5, 6, 7, 20, 40, 64, 65, 200)
CEILINGS = {0.15: (1, 1, 1, 2, 3, 6, 10, 10, 31), 0.25: (1, 2, 2, 2, 5, 10, 16, 17, 50)}


def test_topk_rows_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import (_lib, _lib_dist, _lib_fused, _lib_linear_train, _lib_masked, _lib_optim, _lib_sampler_train,
                              _lib_sgenc_train, _lib_topk_rows, _lib_train)
    header = open(os.path.join(ROOT, "include", "isg_topk_rows.h")).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_topk_rows.SIGNATURES) == {
        "isg_topk_rows_abi_version", "isg_topk_budget", "isg_topk_threshold_rows", "isg_topk_gumbel_rows", "isg_topk_gumbel_rows_bwd"}
    others = [_lib, _lib_train, _lib_optim, _lib_fused, _lib_sgenc_train, _lib_dist, _lib_linear_train, _lib_masked,
              _lib_sampler_train]
    assert not any(declared & set(m.SIGNATURES) for m in others), "a symbol is declared in two headers"
    lib = _lib_topk_rows.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_TOPK_ROWS_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_topk_rows_abi_version() == _lib_topk_rows.ABI_VERSION == abi == 1
    # the other headers did not move
    assert _lib.ABI_VERSION == 23 and len(_lib.SIGNATURES) == 74
    assert (_lib_optim.ABI_VERSION, _lib_fused.ABI_VERSION, _lib_sgenc_train.ABI_VERSION, _lib_dist.ABI_VERSION,
            _lib_linear_train.ABI_VERSION, _lib_masked.ABI_VERSION, _lib_sampler_train.ABI_VERSION) == (1, 1, 1, 1, 1, 1, 1)
    V, I, I32, I64, U64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
    sig, old = _lib_topk_rows.SIGNATURES, _lib.SIGNATURES
    assert sig["isg_topk_budget"] == (I, [V, I64, F, I32, I32, V, V])

    def with_rows(args, at):                              # the scalar entry point's `int32_t k` becomes `k_rows, k_cap`
        assert args[at] is I32
        return args[:at] + [V, I32] + args[at + 1:]

    #   scores ptr B nmax_host nmax_dev noise [noise_scale] seed graph_ids k ...
    assert sig["isg_topk_threshold_rows"] == (I, with_rows(old["isg_topk_threshold"][1], 9))
    assert sig["isg_topk_gumbel_rows"] == (I, with_rows(old["isg_topk_gumbel"][1], 8))
    assert sig["isg_topk_gumbel_rows_bwd"] == (I, with_rows(old["isg_topk_gumbel_bwd"][1], 8))
    assert old["isg_topk_threshold"][1][6] is F and old["isg_topk_gumbel"][1][6] is U64
    build_checks("isg_topk_rows.h")
    assert "ops.topk_budget(" in inspect.getsource(ge.smoke)
    # the scalar entry points and the per-row ones run the same kernels: both sources take them from the one shared header
    for f in ("isg_sampler.hip", "isg_topk_rows.hip"):
        text = open(os.path.join(ge.CSRC, f)).read()
        assert '#include "isg_topk.hpp"' in text and "__syncthreads" not in text, f
    hpp = open(os.path.join(ge.CSRC, "isg_topk.hpp")).read()
    assert "__syncthreads" not in hpp and "ISG_BARRIER" not in hpp, "waves of one workgroup run different loop counts"
    from isubgvqa_amd import ops
    assert "topk_rows" in ops.COUNTERS


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from isubgvqa_amd import _lib_topk_rows
    lib = _lib_topk_rows.load()
    bud = lib.isg_topk_budget
    #          ptr B ratio k_min k_cap k_rows stream
    assert bud(None, 0, 0.15, 1, 5, None, None) == 0                          # no graph: nothing to do, no launch
    assert bud(P, 4, 0.0, 1, 5, P, None) == EINVAL                            # 0 < ratio
    assert bud(P, 4, -0.5, 1, 5, P, None) == EINVAL
    assert bud(P, 4, float("nan"), 1, 5, P, None) == EINVAL
    assert bud(P, 4, 0.15, 0, 5, P, None) == EINVAL                           # 1 <= k_min
    assert bud(P, 4, 0.15, 6, 5, P, None) == EINVAL                           # k_min <= k_cap
    assert bud(None, 4, 0.15, 1, 5, P, None) == EINVAL
    assert bud(P, 4, 0.15, 1, 5, None, None) == EINVAL
    assert bud(P, -1, 0.15, 1, 5, P, None) == EINVAL
    assert bud(P, 1 << 31, 0.15, 1, 5, P, None) == EUNSUPPORTED
    thr, gum, bwd = lib.isg_topk_threshold_rows, lib.isg_topk_gumbel_rows, lib.isg_topk_gumbel_rows_bwd
    #          scores ptr B nmax nmax_dev noise noise_scale seed gids k_rows k_cap out dense stream
    assert thr(P, None, 0, 8, None, None, 0.0, 0, None, None, 5, P, None, None) == 0
    assert thr(P, None, 4, 0, None, None, 0.0, 0, None, None, 5, P, None, None) == 0
    assert thr(P, None, 4, 8, None, None, 0.0, 0, None, None, 5, P, None, None) == EINVAL      # k_rows is required
    assert thr(None, None, 4, 8, None, None, 0.0, 0, None, P, 5, P, None, None) == EINVAL
    assert thr(P, None, 4, 8, None, None, 0.0, 0, None, P, 5, None, None, None) == EINVAL
    assert thr(P, None, 4, 8, None, None, 0.0, 0, None, P, -1, P, None, None) == EINVAL
    assert thr(P, None, 1 << 31, 8, None, None, 0.0, 0, None, P, 5, P, None, None) == EUNSUPPORTED
    assert thr(P, None, 4, 1025, None, None, 0.0, 0, None, P, 5, P, None, None) == EUNSUPPORTED
    #          scores ptr B nmax nmax_dev noise seed gids k_rows k_cap tau out khot stream
    assert gum(P, None, 0, 8, None, None, 0, None, None, 5, 1.0, P, None, None) == 0
    assert gum(P, None, 4, 8, None, None, 0, None, None, 5, 1.0, P, None, None) == EINVAL
    assert gum(P, None, 4, 8, None, None, 0, None, P, 5, 0.0, P, None, None) == EINVAL          # tau > 0
    assert gum(P, None, 4, 1025, None, None, 0, None, P, 5, 1.0, P, None, None) == EUNSUPPORTED
    #          scores ptr B nmax nmax_dev noise seed gids k_rows k_cap tau d_out d_scores stream
    assert bwd(P, None, 0, 8, None, None, 0, None, None, 5, 1.0, P, P, None) == 0
    assert bwd(P, None, 4, 8, None, None, 0, None, None, 5, 1.0, P, P, None) == EINVAL
    assert bwd(P, None, 4, 8, None, None, 0, None, P, 5, 1.0, None, P, None) == EINVAL
    assert bwd(P, None, 4, 8, None, None, 0, None, P, 5, 1.0, P, None, None) == EINVAL
    # k_cap sizes the LDS history, whatever the rows hold: k_cap * slots * 64 <= 4096
    assert bwd(P, None, 4, 64, None, None, 0, None, P, 65, 1.0, P, P, None) == EUNSUPPORTED     # 65 * 1 * 64
    assert bwd(P, None, 4, 65, None, None, 0, None, P, 33, 1.0, P, P, None) == EUNSUPPORTED     # 33 * 2 * 64
    assert bwd(P, None, 4, 130, None, None, 0, None, P, 17, 1.0, P, P, None) == EUNSUPPORTED    # 17 * 4 * 64
    assert bwd(P, None, 4, 1025, None, None, 0, None, P, 1, 1.0, P, P, None) == EUNSUPPORTED


def test_budget_rule_gives_the_ceilings_worked_out_by_hand():
    import topk_rows_restated as R
    n = torch.tensor(NODE_COUNTS)
    for ratio, want in CEILINGS.items():
        # the formula of the reference's comment (masking.py:113), one fp32 product
        raw = torch.ceil(torch.tensor(ratio, dtype=torch.float32) * n.float()).long()
        assert tuple(raw.tolist()) == want, (ratio, raw.tolist())
        for k_min, k_cap in ((1, 5), (2, 12), (1, 64), (3, 3)):
            got = R.budget(n, ratio, k_min, k_cap)
            assert got.dtype == torch.int32
            assert got.tolist() == [min(k_cap, max(k_min, c)) for c in want], (ratio, k_min, k_cap)
    # float32(0.15) * 20 is 3 + 2^-23 exactly, halfway between 3 and the next float, and float32(0.15) * 40 is 6 + 2^-22, halfway
    # again: rounded to nearest-even the products are 3 and 6.  A product kept wider (fused, or in fp64) would give 4 and 7: the
    # rule is the ceiling of the ROUNDED fp32 product
    assert math.ceil(float(torch.tensor(0.15, dtype=torch.float32)) * 20) == 4
    assert R.budget(torch.tensor([20, 40]), 0.15, 1, 99).tolist() == [3, 6]


def _case(nmax, ks, seed, ties=False):
    """Ragged rows of lengths {1, k, k + 1, nmax} (clipped to nmax) per distinct k, padded with 0.0."""
    g = torch.Generator().manual_seed(seed)
    rows, k_rows = [], []
    for k in ks:
        for n in sorted({min(v, nmax) for v in (1, k, k + 1, nmax)}):
            rows.append(torch.randint(-1, 2, (n,), generator=g).float() if ties else torch.randn(n, generator=g))
            k_rows.append(k)
    return rows, k_rows


@pytest.mark.parametrize("nmax", [1, 7, 33, 65])
def test_restated_rows_equal_the_oracle_at_every_distinct_k(nmax):
    import topk_rows_restated as R
    from oracle import samplers as OS
    k_cap = 12
    ks = [1, 2, 5, k_cap, 70]                              # 70: beyond the cap (clamped to it) and, at nmax <= 12, beyond the row
    for ties in (False, True):
        rows, k_rows = _case(nmax, ks, 10 * nmax + ties, ties)
        dense = R.dense_rows(rows, nmax)
        B = dense.size(0)
        k_t = torch.tensor(k_rows)
        got = R.threshold_rows(dense, k_rows, k_cap)
        g = torch.Generator().manual_seed(nmax)
        noise = OS.uniform_to_gumbel(torch.rand(B, nmax, generator=g))
        got_g, got_khot = R.gumbel_rows(dense, noise, k_rows, k_cap, 1.0)
        for k in sorted(set(k_rows)):
            sel = k_t == k
            kk = min(k, k_cap)
            ref = OS.threshold_topk(dense.view(B, nmax, 1), kk).view(B, nmax)
            assert torch.equal(got[sel], ref[sel]), (nmax, ties, k)
            m, khot, _ = OS.gumbel_relaxed_topk(dense.view(B, nmax, 1), kk, noise, 1.0)
            assert torch.equal(got_khot[sel], khot[sel]), (nmax, ties, k)
            assert torch.equal(got_g[sel], m.view(B, nmax)[sel]), (nmax, ties, k)
        assert len({int(r.sum()) for r in got}) > 1 or nmax == 1, "every row selected the same count: the case tests nothing"


def test_ops_refuse_a_malformed_k_per_row():
    from isubgvqa_amd import ops
    s = torch.zeros(3, 8)
    k = torch.tensor([1, 2, 3], dtype=torch.int32)
    for call in (lambda **kw: ops.topk_threshold(s, **kw), lambda **kw: ops.topk_gumbel(s, tau=1.0, **kw),
                 lambda **kw: ops.topk_gumbel_backward(s, s, tau=1.0, **kw)):
        with pytest.raises(ValueError, match="needs k_cap"):
            call(k=k)
        with pytest.raises(ValueError, match="k_cap goes with a tensor"):
            call(k=2, k_cap=5)
        with pytest.raises(ValueError, match="int32"):
            call(k=k.long(), k_cap=5)                      # dtype
        with pytest.raises(ValueError, match="int32"):
            call(k=k[:2], k_cap=5)                         # length
        with pytest.raises(ValueError, match="int32"):
            call(k=k.to("meta"), k_cap=5)                  # device
        with pytest.raises(ValueError, match="at least 1"):
            call(k=k, k_cap=0)
    with pytest.raises(NotImplementedError, match="SIMPLE"):
        ops.simple_topk(s, k)
    plan = argparse.Namespace(memo=dict)
    for bad in ((0.0, 1, 5), (-1.0, 1, 5), (float("nan"), 1, 5), (0.15, 0, 5), (0.15, 6, 5)):
        with pytest.raises(ValueError, match="topk_budget needs"):
            ops.topk_budget(plan, *bad)


def _masking_args(**kw):
    d = dict(dim_nodes=16, dim_questions=16, masking_threshold=0.15, use_topk=True, sample_k=5, sampler_type="imle")
    d.update(kw)
    return d


def test_constructors_pass_the_budget_down_and_leave_the_default_alone():
    from isubgvqa_amd import synthetic
    from isubgvqa_amd.models.masking import MaskingModel
    from isubgvqa_amd.models.mgat import MGAT
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    for cls in (MaskingModel, MaskingGATv2Conv, MGAT, synthetic.AnswerModel):
        p = inspect.signature(cls.__init__).parameters
        assert p["sample_ratio"].default is None and p["sample_k_min"].default == 1, cls
        names = [n for n, q in p.items() if q.kind is not inspect.Parameter.VAR_KEYWORD]
        assert names[-2:] == ["sample_ratio", "sample_k_min"], (cls, names)        # trailing: the reference's positions stay
    torch.manual_seed(0)
    plain = MaskingModel(**_masking_args())
    torch.manual_seed(0)
    same = MaskingModel(**_masking_args(sample_ratio=None))
    assert plain.sample_ratio is None and same.sample_ratio is None and plain.sample_k_min == 1
    assert list(plain.state_dict()) == list(same.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), same.state_dict().values()))
    for sampler in ("imle", "aimle", "gumbel"):
        torch.manual_seed(0)
        m = MaskingModel(**_masking_args(sampler_type=sampler, sample_ratio=0.15, sample_k_min=2))
        assert (m.sample_ratio, m.sample_k_min, m.sample_k) == (0.15, 2, 5)
        assert list(m.state_dict()) == list(plain.state_dict()), "the budget adds no parameter"
    with pytest.raises(NotImplementedError, match="SIMPLE"):
        MaskingModel(**_masking_args(sampler_type="simple", sample_ratio=0.15))
    MaskingModel(**_masking_args(sampler_type="simple"))                             # without a ratio: as before
    for bad in (dict(sample_ratio=0.0), dict(sample_ratio=-0.1), dict(sample_ratio=0.15, sample_k_min=0),
                dict(sample_ratio=0.15, sample_k_min=6), dict(sample_ratio=0.15, sample_k=None)):
        with pytest.raises(ValueError, match="sample_ratio needs"):
            MaskingModel(**_masking_args(**bad))
    g = MGAT(channels=16, num_ins=2, use_instr=True, masking_thresholds=[1.0, 0.15], use_topk=True, sampler_type="gumbel",
             sample_k=5, sample_ratio=0.25, sample_k_min=2)
    assert [(c.mask.sample_ratio, c.mask.sample_k_min) for c in g.convs] == [(0.25, 2)] * 2
    a = synthetic.AnswerModel(16, 2, (1.0, 0.15), "imle", 5, sample_ratio=0.15, sample_k_min=2, num_answers=7)
    assert [(c.mask.sample_ratio, c.mask.sample_k_min) for c in a.gat_seq.convs] == [(0.15, 2)] * 2
    with pytest.raises(NotImplementedError, match="SIMPLE"):
        synthetic.AnswerModel(16, 2, (1.0, 0.15), "simple", 5, sample_ratio=0.15, num_answers=7)


def test_a_namespace_without_the_fields_builds_and_one_with_them_is_read():
    from isubgvqa_amd import checkpoint
    from isubgvqa_amd.models import build_model
    d = dict(text_sampling=False, general_hidden_dim=32, distributed=False, mgat_layers=2, use_all_instrs=False,
             use_global_mask=False, node_classification=False, sampler_type="imle", sample_k=5, nb_samples=1,
             alpha=1.0, beta=10.0, tau=1.0, use_masking=True, use_instruction=1, use_mgat=True,
             mgat_masks=[1.0, 0.15], use_topk=True, interpretable_mode=False, concat_instr=0, embed_cat=0,
             device="cpu", text_vocab_size=64, sg_vocab_size=40)
    assert "sample_ratio" not in d and "sample_k_min" not in d
    torch.manual_seed(0)
    m = build_model(argparse.Namespace(**d), None)
    assert all(c.mask.sample_ratio is None and c.mask.sample_k_min == 1 for c in m.gat_seq.convs)
    torch.manual_seed(0)
    b = build_model(argparse.Namespace(**d, sample_ratio=0.15, sample_k_min=2), None)
    assert all((c.mask.sample_ratio, c.mask.sample_k_min, c.mask.sample_k) == (0.15, 2, 5) for c in b.gat_seq.convs)
    assert list(m.state_dict()) == list(b.state_dict())
    assert checkpoint._ARG_DEFAULTS["sample_ratio"] is None and checkpoint._ARG_DEFAULTS["sample_k_min"] == 1
