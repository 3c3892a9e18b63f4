"""Host-side checks of the question side's training path (include/isg_train.h, autograd.py, models/text_encoder.py) that need no
GPU: the second device header binds and the built library exports it, include/isg.h did not move, the shape limits and the LDS
formula the GPU cases rely on, the keep rule against hand-computed Philox values, and the CPU behaviour of the Python layer."""
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT


def test_training_header_parses_binds_and_is_exported():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_train
    path = os.path.join(ROOT, "include", "isg_train.h")
    header = open(path).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(_lib_train.SIGNATURES) and len(declared) == 8, declared ^ set(_lib_train.SIGNATURES)
    assert declared >= {"isg_train_abi_version", "isg_dropout", "isg_mha_small_train", "isg_mha_small_bwd", "isg_dropout_add_layernorm",
                        "isg_add_layernorm_bwd", "isg_add_layernorm_bwd_parts"}
    assert not declared & set(_lib.SIGNATURES), "a training symbol is declared in include/isg.h too"
    lib = _lib_train.load()
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
    abi = int(re.search(r"#define ISG_TRAIN_ABI_VERSION (\d+)", header).group(1))
    assert lib.isg_train_abi_version() == _lib_train.ABI_VERSION == abi == 1
    # argument marshalling of the two longest declarations
    res, args = _lib_train.SIGNATURES["isg_mha_small_bwd"]
    assert res is ctypes.c_int and len(args) == 23 and args[-3:] == [ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p]
    res, args = _lib_train.SIGNATURES["isg_add_layernorm_bwd"]
    assert len(args) == 19 and args[5] is ctypes.c_float and args[-5:-3] == [ctypes.c_int64, ctypes.c_int32]
    # host-only entry points answer without a GPU
    assert [lib.isg_add_layernorm_bwd_parts(m) for m in (0, 1, 16, 17, 1030, 10 ** 6)] == [0, 1, 1, 2, 65, 1024]
    assert lib.isg_mha_small_bwd_lds_bytes(64, 77, 77) == 4 * (2 * 77 * 68 + 2 * 77 * 64 + 2 * 77 * 77)
    # the staleness list of build() knows the header
    build_checks("isg_train.h")


def test_inference_header_did_not_move():
    from isubgvqa_amd import _lib
    header = open(os.path.join(ROOT, "include", "isg.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert len(set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", body))) == 74 == len(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 23


def test_cases_reach_the_limits_they_claim():
    """The host restatement of the kernels' limits (ops.mha_small_train_supported, the LDS formulas of the GPU file) against what
    the GPU cases claim: every case fits, the CLIP case is the largest and needs the dynamic-LDS opt-in, the refused case passes
    the forward's bound and fails the backward's; every PARTS form, the second key per lane, a head width off the multiples of 8;
    both sides of every NV template of the LayerNorm kernels."""
    from isubgvqa_amd import ops
    import test_gpu_text_train as G
    parts = lambda hd, Tk: 4 if Tk <= 16 and hd % 16 == 0 else 2 if Tk <= 32 and hd % 8 == 0 else 1
    seen = set()
    for case in G.ATTN_CASES:
        B, H, hd, Tq, Tk = case
        assert hd <= 64 and hd % 4 == 0 and 1 <= Tk <= 128
        assert G.lds_fwd(hd, Tq, Tk) <= G.LDS_FWD and G.lds_bwd(hd, Tq, Tk) <= G.LDS_BWD, case
        assert ops.mha_small_train_supported(Tq, Tk, hd) and ops.mha_small_supported(max(Tq, Tk), hd), case
        assert ops.mha_small_bwd_lds_bytes(hd, Tq, Tk) == G.lds_bwd(hd, Tq, Tk)
        seen.add(parts(hd, Tk))
    assert set(G.ATTN_CASES) >= {(1, 1, 4, 1, 1), (3, 2, 16, 5, 5), (2, 8, 64, 12, 12), (2, 8, 64, 4, 12), (2, 1, 64, 4, 65),
                                 (1, 1, 32, 3, 128), (1, 2, 20, 7, 9), (1, 2, 64, 77, 77)} and len(set(G.ATTN_CASES)) == len(G.ATTN_CASES)
    assert seen == {1, 2, 4}
    big = max(G.ATTN_CASES, key=lambda c: G.lds_bwd(c[2], c[3], c[4]))
    assert big == (1, 2, 64, 77, 77) and 64 * 1024 < G.lds_bwd(64, 77, 77) == 128744 <= ops.MHA_BWD_LDS_MAX == G.LDS_BWD
    assert any(c[4] > 64 for c in G.ATTN_CASES) and any(c[2] % 8 for c in G.ATTN_CASES) and any(c[3] != c[4] for c in G.ATTN_CASES)
    # one key-and-query more than 80 x 80 at hd = 64 leaves the forward's 64 KB; 128 x 128 at hd = 32 only the backward's 160 KB
    assert ops.mha_small_train_supported(80, 80, 64) and not ops.mha_small_train_supported(81, 81, 64)
    assert G.lds_fwd(32, 128, 128) <= G.LDS_FWD < G.LDS_BWD < G.lds_bwd(32, 128, 128) and not ops.mha_small_train_supported(128, 128, 32)
    assert not ops.mha_small_train_supported(100, 100, 64)          # the modules' T = 100 case
    for hd, tq, tk in ((68, 4, 4), (16, 4, 129), (6, 4, 4)):
        assert not ops.mha_small_train_supported(tq, tk, hd)
    nv = lambda D: 1 if D <= 256 else 2 if D <= 512 else 4 if D <= 1024 else 8
    assert [nv(D) for D in G.LN_DS] == [1, 1, 2, 2, 4, 4, 8, 8] and all(D % 4 == 0 and D <= 2048 for D in G.LN_DS)
    assert G.LN_MS == [1, 3, 9, 1030] and (1030 + 15) // 16 > 4 * 4          # several partial rows, several rows per wave
    assert G.MODULE_DIMS == {"g4": (32, 4, 64, 6, 3), "real": (512, 8, 2048, 12, 3)}
    for ninp, heads, _, T, _ in G.MODULE_DIMS.values():
        assert ops.mha_small_train_supported(T, T, ninp // heads) and ops.mha_small_train_supported(4, T, ninp // heads)


def test_keep_rule_on_two_hand_computed_blocks():
    """Element (i, j) is kept iff uniform24(word[j & 3] of philox4x32_10((i, j >> 2, 0x1571, 0x9E37), seed)) >= p.  The two blocks
    below were worked out from the generator's definition (tests/test_philox_cpu.py holds philox4x32_10 to its published answers)."""
    import numpy as np
    from oracle import philox
    import test_gpu_text_train as G
    # (i, j) = (0, 0), seed 0: block (0, 0), word 0
    assert philox.philox4x32_10((0, 0, 0x1571, 0x9E37), (0, 0)) == (0x4343BE88, 0xB4D85013, 0x5FBCD453, 0x3A00EED9)
    u = 0x4343BE88 >> 8
    assert u == 4408254 and float(philox.uniform24(0x4343BE88)) == u / 2 ** 24 == 0.2627524137496948
    assert bool(G.keep_mask(0, 1, 4, 0.25)[0, 0]) and not bool(G.keep_mask(0, 1, 4, 0.27)[0, 0])
    # (i, j) = (5, 6), seed 0x0123456789ABCDEF: block (5, 1), word 2; key = (0x89ABCDEF, 0x01234567)
    seed = 0x0123456789ABCDEF
    assert philox.philox4x32_10((5, 1, 0x1571, 0x9E37), (0x89ABCDEF, 0x01234567)) == (0xD0922A6A, 0xA943BC15, 0x1FFD95EB, 0xFF71980D)
    u = 0x1FFD95EB >> 8
    assert u == 2096533 and float(philox.uniform24(0x1FFD95EB)) == u / 2 ** 24 == 0.12496310472488403
    m = G.keep_mask(seed, 6, 8, 0.125)
    assert not bool(m[5, 6]) and bool(G.keep_mask(seed, 6, 8, 0.1249)[5, 6])
    assert bool(m[5, 4]) and bool(m[5, 7])          # words 0 and 3 of the same block: 0.8147..., 0.9978...
    # the comparison is made in fp32, `>=`: u == p keeps
    assert bool(G.keep_mask(seed, 6, 8, float(np.float32(u / 2 ** 24)))[5, 6])
    assert bool(G.keep_mask(seed, 3, 5, 0.0).all()) and G.inv_keep(0.5) == 2.0 and G.inv_keep(0.1) == float(np.float32(1) / np.float32(0.9))


def test_autograd_linear_accepts_relu_and_ops_need_the_gpu():
    """autograd.linear runs on the GPU only (the product path has no CPU fallback): on the CPU the signature is what can be held --
    `relu` is accepted, excludes gelu, and the call reaches the kernel launch, which refuses CPU tensors loudly."""
    from isubgvqa_amd import _lib, autograd, ops
    sig = inspect.signature(autograd.linear)
    assert list(sig.parameters) == ["x", "weight", "bias", "gelu", "relu"] and sig.parameters["relu"].default is False
    for name in ("mha_small", "add_layernorm", "dropout"):
        assert callable(getattr(autograd, name)), name
    assert list(inspect.signature(autograd.mha_small).parameters) == ["q", "k", "v", "B", "H", "key_bias", "p", "seed"]
    assert list(inspect.signature(autograd.add_layernorm).parameters) == ["x", "residual", "norm", "p", "seed"]
    assert list(inspect.signature(autograd.dropout).parameters) == ["x", "p", "seed"]
    x, w = torch.randn(4, 8, requires_grad=True), torch.randn(8, 8, requires_grad=True)
    with pytest.raises(ValueError):
        autograd.linear(x, w, None, True, relu=True)
    with pytest.raises(_lib.IsgError, match="GPU"):
        autograd.linear(x, w, None, False, relu=True)
    assert autograd.dropout(x, 0.0, 1) is x                      # p == 0: nothing is drawn, nothing is launched
    with pytest.raises(ValueError):
        ops.dropout(x.detach(), 1.0, 0)
    # linear_route keeps its answers: ReLU under autograd is not ops.linear's business
    assert ops.linear_route(12, 2048, 512, relu=True, recording=True) == "torch"
    assert "text_train_kernels" in ops.COUNTERS and "torch_attention_train" in ops.COUNTERS


def test_text_encoder_on_cpu_tensors_runs_the_torch_modules():
    from isubgvqa_amd import ops
    from isubgvqa_amd.models import text_encoder as TE
    assert TE.FUSED_TEXT_TRAIN is True and TE.FUSED_TEXT is True
    torch.manual_seed(3)
    enc = TE.QuestionEncoder(TE.CLIPTextEmbeddings(50, 32, 16), 32, 32, 4, 64, 2, dropout=0.0).train()
    dec = TE.QuestionDecoder(4, 32, 4, 64, 2, dropout=0.0).train()
    ids = torch.randint(0, 50, (3, 6))
    mask = torch.ones(3, 6, dtype=torch.long)
    ops.reset_counters()
    mem = enc(ids, mask=mask, seed=5)
    out = dec(memory=mem, seed=6)
    assert ops.counters()["text_train_kernels"] == 0
    want_mem = enc.transformer_encoder(enc.text_vocab_embedding(ids).permute(1, 0, 2), src_key_padding_mask=mask.float())
    want = dec.coarse_decoder(tgt=dec.query_embed.weight.unsqueeze(1).repeat(1, 3, 1), memory=want_mem, tgt_mask=None)
    assert torch.equal(mem, want_mem) and torch.equal(out, want)
    out.sum().backward()
    assert enc.transformer_encoder.layers[0].linear1.weight.grad is not None
