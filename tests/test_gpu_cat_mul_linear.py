"""isg_linear_f16x3_catmul: the answer head's Linear over cat(a, b, a * b), reading a and b on 32-row blocks,
must leave the BITS of ops.linear(ops.cat_mul(a, b), ...) -- isg_cat_mul_rowmax + isg_linear_f16x3_tile -- in the result and in
the row maxima attached to it (int32 views compared).

M = 4096, 4097, 4127 (whole blocks, one row more, a last block of 31 rows); C = 128 and 32 (at C = 32 the un-fused Linear is not
the tile kernel's, so the rule says no and the two launches run: the wrapper's other arm); N = 512 and 160 (a last 128-column tile
that is not full); with and without GELU, with and without bias; rows scaled by exp(U(0, 6)), a zero row.
Model level: synthetic.AnswerModel on 1100 graphs with each new switch off, alone and together, eager and captured."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("M", [4096, 4097, 4127])
@pytest.mark.parametrize("C", [128, 32])
@pytest.mark.parametrize("N", [512, 160])
@pytest.mark.parametrize("gelu", [False, True])
def test_bits_of_cat_mul_then_linear(M, C, N, gelu):
    from isubgvqa_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(M + C + N + gelu)
    a = torch.randn(M, C, generator=gen) * torch.rand(M, 1, generator=gen).mul(6).exp()
    b = torch.randn(M, C, generator=gen)
    a[M // 3] = 0.0
    b[M // 3] = 0.0
    a, b = a.to(dev), b.to(dev)
    w = (torch.randn(N, 3 * C, generator=gen) / (3 * C) ** 0.5).to(dev)
    bias = torch.randn(N, generator=gen).to(dev)
    with torch.no_grad():
        assert ops.cat_mul_linear_supported(M, N, C) == (C == 128)
        for bs in (bias, None):
            ref = ops.linear(ops.cat_mul(a, b), w, bs, gelu=gelu, want_rowmax=True)
            got = ops.cat_mul_linear(a, b, w, bs, gelu=gelu, want_rowmax=True)
            plain = ops.cat_mul_linear(a, b, w, bs, gelu=gelu)
            torch.cuda.synchronize()
            assert torch.isfinite(ref).all() and got.shape == ref.shape
            diff = bits(got) != bits(ref)
            assert not diff.any(), f"{int(diff.sum())} of {ref.numel()} elements differ, first at {diff.nonzero()[0].tolist()}"
            assert torch.equal(bits(plain), bits(ref)) and ops.row_maxima(plain) is None
            rm, rr = ops.row_maxima(got), ops.row_maxima(ref)
            assert (rm is None) == (rr is None)          # C = 32: the un-fused Linear is bf16x6's, which leaves none
            if C == 128:
                assert rm is not None and rm.shape == rr.shape == (M, (N + 31) // 32)
            if rm is not None:
                assert torch.equal(bits(rm), bits(rr)), "the attached row maxima differ"


def test_answer_model_is_bit_identical_with_each_new_switch_off():
    from isubgvqa_amd import ops, synthetic
    import test_gpu_small_mlps as T
    dev = torch.device("cuda:0")
    model, wl = T._model_and_batch(dev)
    noises = {2: synthetic.gumbel_noise((wl.glf.size(0), wl.max_nodes), dev)}
    with torch.no_grad():
        on = [t.clone() for t in model(wl, noises=noises)]
        cap = [t.clone() for t in model(wl, noises=noises, capture=True)]
        T._same(cap, on, "captured")
        for off in (dict(fuse_cat_mul_linear=False), dict(fuse_question_mlps=False),
                    dict(fuse_cat_mul_linear=False, fuse_question_mlps=False)):
            with ops.configured(**off):
                model.__dict__.pop("_step_capture", None)
                T._same(on, [t.clone() for t in model(wl, noises=noises)], f"eager, {off}")
                T._same(on, [t.clone() for t in model(wl, noises=noises, capture=True)], f"captured, {off}")
        model.__dict__.pop("_step_capture", None)
        torch.cuda.synchronize()
