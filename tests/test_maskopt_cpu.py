"""Host-side checks of mask optimisation (include/ext/isg_maskopt.h) that need no GPU: the extension header, its
binding and the two libraries agree; the entry point refuses bad arguments before any launch; the known answer of the header
through the restatement of tests/maskopt_restated.py; the closed-form entropy gradient against PyG's guarded formula; the explainer
names; a model in train() is refused."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

import maskopt_restated as MR

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
BIG = (1 << 31) - 1024
NAMES = {"isg_maskopt_abi_version", "isg_maskopt_step"}


def test_maskopt_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_maskopt as X
    from isubgvqa_amd import _ext_ig, _ext_induced, _ext_instances_train, _ext_rollout, _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_maskopt.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_MASKOPT_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_maskopt_abi_version() == X.ABI_VERSION == abi == 1
    i32, i64, ptr, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
    sigs = {"isg_maskopt_abi_version": (ctypes.c_int, []),
            # (x, ldx, g, ldg, seg, B, theta, exp_avg, exp_avg_sq, x_out, ldxo, d_theta, N, C) + the eight host scalars + stream
            "isg_maskopt_step": (ctypes.c_int, [ptr, i32, ptr, i32, ptr, i64, ptr, ptr, ptr, ptr, i32, ptr, i64, i32] + [f64] * 8 + [ptr])}
    assert X.SIGNATURES == sigs
    for name, sig in sigs.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export exactly the header's symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_maskopt_abi_version.restype = ctypes.c_int
        assert raw.isg_maskopt_abi_version() == 1, other
        exported = set(m.decode() for m in re.findall(rb"\x00(isg_maskopt_[a-z0-9_]*)(?=\x00)", open(other, "rb").read()))
        assert exported == NAMES, (other, exported)
    # a handle swapped in through _lib.using is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_maskopt_step.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_maskopt_step.argtypes) == sigs["isg_maskopt_step"][1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="mask-optimisation ABI version 2, binding expects 1"):
            X.load()
    # a symbol declared twice is refused; the header lies outside the table of device headers, whose table did not move; each of
    # the four other extension headers is among those this one is held against
    assert not NAMES & set(X.declared_elsewhere()) and "isg_maskopt.h" not in _lib.HEADERS
    with pytest.raises(_lib.IsgError, match="`isg_maskopt_step` is declared in include/isg_x.h and in include/ext/isg_maskopt.h"):
        X.refuse_redeclared(X.SIGNATURES, {"isg_maskopt_step": "isg_x.h"})
    for mod, file in ((_ext_instances_train, "isg_instances_train.h"), (_ext_induced, "isg_induced.h"), (_ext_rollout, "isg_rollout.h"),
                      (_ext_ig, "isg_ig.h")):
        assert set(mod.SIGNATURES) <= set(X.declared_elsewhere())
        name = sorted(mod.SIGNATURES)[-1]
        with pytest.raises(_lib.IsgError, match=f"`{name}` is declared in include/ext/{file} and in include/ext/isg_maskopt.h"):
            X.refuse_redeclared({name: None}, X.declared_elsewhere())
    # the build lists the header and checks the version, the counter exists, the kernel is plain HIP
    build_checks("isg_maskopt.h")
    build_checks("isg_ig.h")
    assert ops.COUNTERS["maskopt_step"] >= 0
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_maskopt.hip")).read()).lower()
    assert "atomic" not in text and "printf" not in text and "assert" not in text and "asm" not in text
    assert "__shared__" not in text and text.count("__launch_bounds__(mo_threads)") == 1 and text.count("<<<") == 1
    assert "fma" not in text                              # the header: the function uses no fma


def test_step_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_maskopt as X
    lib = X.load()

    def call(x=P, ldx=8, g=P, ldg=8, seg=P, B=2, theta=P, exp_avg=P, exp_avg_sq=P, x_out=P, ldxo=8, d_theta=P, N=5, C=8,
             a_size=1.0, a_ent=0.1, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, bc1=0.1, bc2=0.001):
        return lib.isg_maskopt_step(x, ldx, g, ldg, seg, B, theta, exp_avg, exp_avg_sq, x_out, ldxo, d_theta, N, C,
                                    a_size, a_ent, lr, beta1, beta2, eps, bc1, bc2, None)

    # every call below carries at least one fault, or no rows: none launches
    for k in ("N", "B"):
        assert call(**{k: -1}) == EINVAL, k
        assert call(**{k: BIG}, C=6) == EUNSUPPORTED and call(**{k: 1 << 31}, C=6) == EUNSUPPORTED, k
    for k in ("x", "seg", "theta", "x_out", "exp_avg", "exp_avg_sq"):
        assert call(**{k: None}) == EINVAL, k
    assert call(B=0) == EINVAL and call(C=0) == EINVAL and call(C=-4) == EINVAL
    assert call(ldx=4) == EINVAL and call(ldg=4) == EINVAL and call(ldxo=4) == EINVAL
    assert call(bc1=0.0) == EINVAL and call(bc2=-1.0) == EINVAL and call(bc1=float("nan")) == EINVAL
    # what is no multiple of 4, or not aligned
    assert call(C=6) == EUNSUPPORTED and call(ldx=10) == EUNSUPPORTED and call(ldg=9) == EUNSUPPORTED and call(ldxo=10) == EUNSUPPORTED
    for k in ("x", "g", "x_out"):
        assert call(**{k: P + 4}) == EUNSUPPORTED, k
    # EINVAL is found before EUNSUPPORTED, a negative count before everything
    assert call(C=6, ldx=4) == EINVAL and call(N=BIG, x=None) == EINVAL and call(N=-1, C=6) == EINVAL
    # the apply-only form needs neither the moments nor g's stride nor the bias corrections; it is then refused for the width alone
    assert call(g=None, ldg=0, exp_avg=None, exp_avg_sq=None, d_theta=None, bc1=0.0, bc2=0.0, C=6) == EUNSUPPORTED
    assert call(g=None, ldg=0, exp_avg=None, exp_avg_sq=None, bc1=0.0, x=P + 8) == EUNSUPPORTED
    # no rows: ISG_OK whatever the pointers, nothing is launched
    assert call(N=0) == 0
    assert call(N=0, B=0, x=None, g=None, seg=None, theta=None, exp_avg=None, exp_avg_sq=None, x_out=None, d_theta=None, C=0, ldx=0,
                ldg=0, ldxo=0) == 0
    assert call(N=0, B=-1) == EINVAL and call(N=0, B=BIG) == EUNSUPPORTED


def test_the_known_answer_of_the_header():
    x, g, seg, s, m, reg, d, theta_new = MR.known_answer()
    zero = torch.zeros(2)
    got_d, bound, inside = MR.d_theta(x, g, seg, zero)
    assert (g.double() * x.double()).sum(1).tolist() == s and float(MR.sigmoid(zero)[0]) == m
    k = MR.scalars(step=1)
    assert (k["A"] - k["E"] * 0.0) / 2 == reg and abs(k["bc1"] - 0.1) < 1e-15 and abs(k["bc2"] - 0.001) < 1e-15
    assert got_d.tolist() == d and bool(inside.all()) and bool((bound > 0).all()) and float(bound.max()) < 2e-5
    rows, dd, t1, m1, v1 = MR.step(x, g, seg, zero, zero, zero, step=1, **MR.PYG)
    assert dd.tolist() == d and float((t1 - torch.tensor(theta_new).double()).abs().max()) < 1e-9
    # at step 1 Adam moves by lr d / (|d| + eps), but for the scalars' fp32 roundings
    want = -0.01 * torch.tensor(d).double() / (torch.tensor(d).double().abs() + 1e-8)
    assert float((t1 - want).abs().max()) < 1e-9
    assert torch.allclose(rows, MR.sigmoid(t1).unsqueeze(1) * x.double(), rtol=0, atol=0)
    assert float((m1 - 0.1 * torch.tensor(d).double()).abs().max()) < 1e-8 and float((v1 - 0.001 * torch.tensor(d).double() ** 2).abs().max()) < 1e-9
    header = re.sub(r"\s+\*\s+", " ", open(os.path.join(ROOT, "include", "ext", "isg_maskopt.h")).read())
    for text in ("theta = [0, 0]", "x = [[1, 2, 3, 4], [-1, 0, 1, 2]]", "g = [[1, 1, 1, 1], [2, 0, -2, 4]]", "s = [10, 4]", "m = 0.5",
                 "= [2.625, 1.125]", "theta_new = [-0.01, -0.01]", "bc1 = 0.1, bc2 = 0.001"):
        assert text in header, text
    # the apply-only form; a non-finite d skips its row alone; saturation; a row outside every segment
    rows0, none, t0, _, _ = MR.step(x, None, seg, zero, None, None)
    assert none is None and torch.equal(rows0, 0.5 * x.double()) and torch.equal(t0, zero.double())
    bad = g.clone()
    bad[1, 2] = float("inf")
    rows, dd, t1b, m1b, v1b = MR.step(x, bad, seg, zero, zero, zero, step=1, **MR.PYG)
    assert not bool(torch.isfinite(dd[1])) and dd[0] == d[0]
    assert (t1b[1], m1b[1], v1b[1]) == (0.0, 0.0, 0.0) and t1b[0] == t1[0] and torch.equal(rows[1], 0.5 * x[1].double())
    sat = torch.tensor([90.0, -90.0])
    dd = MR.d_theta(x, g, seg, sat)[0]
    assert float(MR.sigmoid(sat)[0]) == 1.0 and float(MR.sigmoid(sat)[1]) < 1e-38      # (fp32's expf overflows there: m = +0)
    assert dd[0] == 0 and dd.abs().max() < 1e-36 and bool(torch.isfinite(dd).all())
    j_of, n_of = MR.segment_of([1, 1, 3, 3, 4], 6)
    assert j_of.tolist() == [-1, 1, 1, 3, -1, -1] and n_of.tolist() == [0, 2, 2, 1, 0, 0]
    rows = MR.step(torch.ones(6, 4), None, [1, 1, 3, 3, 4], torch.zeros(6), None, None)[0]
    assert torch.isnan(rows[:, 0]).tolist() == [True, False, False, False, True, True]
    assert MR.segment_of([0, 5, 3, 9], 9)[0].tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 2]       # a decreasing range: compared, never an address


def test_closed_form_entropy_gradient_equals_pygs_guarded_formula():
    """d/dtheta H(sigmoid(theta)) = -theta sigmoid'(theta), against torch.autograd of PyG's -m log(m + eps) - (1 - m) log(1 - m + eps)
    with eps = 1e-15, in float64 for |theta| <= 20, within 1e-12; and the regulariser of d_theta as a whole against autograd of the
    objective's regularisers over a segment."""
    theta = torch.cat([torch.linspace(-20, 20, 4001, dtype=torch.float64), torch.tensor([0.0, 1e-9, -1e-9], dtype=torch.float64)])
    leaf = theta.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(MR.pyg_entropy_term(leaf).sum(), leaf)
    m = MR.sigmoid(theta)
    closed = -theta * m * (1 - m)
    assert float((grad - closed).abs().max()) <= 1e-12
    # the size and entropy terms together, as means over a segment of 7 rows: (a_size - a_ent theta) / n * sigmoid'
    t = torch.tensor([-3.0, -0.5, 0.0, 0.25, 1.0, 4.0, 20.0], dtype=torch.float64).requires_grad_(True)
    reg = 1.0 * torch.sigmoid(t).mean() + 0.1 * MR.pyg_entropy_term(t).mean()
    (grad,) = torch.autograd.grad(reg, t)
    x, g = torch.ones(7, 4), torch.zeros(7, 4)
    d = MR.d_theta(x, g, [0, 7], t.detach(), a_size=1.0, a_ent=0.1)[0]
    assert float((d - grad).abs().max()) <= 1e-9           # (a_ent is the header's fp32 E = 0.1 (1 + 1.5e-8) here)
    assert torch.allclose(MR.objective(torch.zeros(1), t.detach(), [0, 7])[0], reg.detach(), rtol=0, atol=1e-12)


def test_explainer_names_defaults_and_the_refusals():
    from isubgvqa_amd import explain, ops, synthetic
    assert explain.EXPLAINERS_LEARNED == ("mask_optimization",)
    assert explain.EXPLAINERS_GRADIENT == ("integrated_gradients", "grad_x_input")
    assert explain.EXPLAINERS == ("intrinsic", "occlusion", "random") and explain.EXPLAINERS_ALL == explain.EXPLAINERS + ("attention",)
    p = inspect.signature(explain.compare).parameters
    assert p["explainers"].default is explain.EXPLAINERS and p["ig_steps"].default == 16 and p["mo_steps"].default == 100
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2)
    assert explain.compare(model, [], None, explainers=("mask_optimization",)).keys() == {"mask_optimization"}
    assert list(explain.compare(model, [], None, explainers=("intrinsic", "mask_optimization", "grad_x_input"), mo_steps=3)) == \
        ["intrinsic", "mask_optimization", "grad_x_input"]
    for bad in (("gnnexplainer",), ("mask_optimization", "pgexplainer"), ()):
        with pytest.raises(ValueError, match="explainers"):
            explain.compare(None, [], None, explainers=bad)
    p = inspect.signature(explain.mask_optimization).parameters
    assert [k for k in p][:2] == ["model", "inputs"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[2:])
    assert {k: p[k].default for k in list(p)[2:]} == dict(noises=None, seed=None, steps=100, lr=0.01, a_size=1.0, a_ent=0.1, init=0.1,
                                                          init_seed=0, edges=False)
    p = inspect.signature(explain.mask_optimize).parameters
    assert [k for k in p][:5] == ["score", "x", "e", "plan", "edge_index"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[5:])
    assert {k: p[k].default for k in list(p)[5:]} == dict(pred_rows=None, steps=100, lr=0.01, a_size=1.0, a_ent=0.1, init=0.1, init_seed=0,
                                                          edges=False)
    p = inspect.signature(ops.maskopt_step).parameters
    assert list(p) == ["x", "g", "seg", "theta", "exp_avg", "exp_avg_sq", "step", "a_size", "a_ent", "lr", "betas", "eps", "out", "want_grad"]
    assert all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[6:]) and p["step"].default is p["step"].empty
    assert {k: p[k].default for k in list(p)[7:]} == dict(a_size=1.0, a_ent=0.1, lr=0.01, betas=(0.9, 0.999), eps=1e-8, out=None, want_grad=False)
    assert [f for f in explain.MaskOptimization.__dataclass_fields__][:5] == ["theta", "soft", "nll", "plan", "steps"]
    assert {"pred", "logits", "edge_theta", "edge_soft"} <= set(explain.MaskOptimization.__dataclass_fields__)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="step"):
            ops.adam_bias_corrections(bad)
    assert ops.adam_bias_corrections(1) == (1.0 - 0.9, 1.0 - 0.999) and ops.adam_bias_corrections(7)[0] == 1.0 - 0.9 ** 7
    with pytest.raises(_lib_error(), match="must live on the GPU"):
        ops.maskopt_step(torch.zeros(2, 4), None, torch.zeros(2, dtype=torch.int32), torch.zeros(2), None, None, step=1)


def _lib_error():
    from isubgvqa_amd import _lib
    return _lib.IsgError


def test_a_model_in_train_mode_is_refused():
    from isubgvqa_amd import explain, synthetic
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2).train()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.mask_optimization(model, None)
    with pytest.raises(ValueError, match="steps"):
        explain.mask_optimize(None, None, None, None, None, steps=-1)
