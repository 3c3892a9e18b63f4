"""Host-side checks of integrated gradients (include/ext/isg_ig.h) that need no GPU: the extension header, its
binding and the two libraries agree; the two entry points refuse bad arguments before any launch; the quadrature rules; the known
answer of the header through the restatement of tests/ig_restated.py; the explainer names; a model in train() is refused."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

import ig_restated as IR

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
BIG = (1 << 31) - 1024
NAMES = {"isg_ig_abi_version", "isg_ig_path_rows", "isg_ig_attribution"}


def test_ig_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_ig as X
    from isubgvqa_amd import _ext_rollout, _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_ig.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_IG_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_ig_abi_version() == X.ABI_VERSION == abi == 1
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    sigs = {"isg_ig_abi_version": (ctypes.c_int, []),
            # (x, ldx, x_rows, b_x, ldbx, node_src, inst_of, n_out, x_out, ldxo, Cx) + the same for the edges + (t, Q, path_e, stream)
            "isg_ig_path_rows": (ctypes.c_int, [ptr, i32, i64, ptr, i32, ptr, ptr, i64, ptr, i32, i32] * 2 + [ptr, i64, i32, ptr]),
            # (g, ldg, rows_in, x, ldx, b, ldb, attr, avg, lda, rows, C) twice + (w, ptr, erange, inst_ptr, inst_eptr, gptr, glist,
            # G, Q, accumulate, stream)
            "isg_ig_attribution": (ctypes.c_int, [ptr, i32, i64, ptr, i32, ptr, i32, ptr, ptr, i32, i64, i32] * 2 +
                                   [ptr] * 7 + [i64, i64, i32, ptr])}
    assert X.SIGNATURES == sigs
    for name, sig in sigs.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export exactly the header's symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_ig_abi_version.restype = ctypes.c_int
        assert raw.isg_ig_abi_version() == 1, other
        exported = set(m.decode() for m in re.findall(rb"\x00(isg_ig_[a-z0-9_]*)(?=\x00)", open(other, "rb").read()))
        assert exported == NAMES, (other, exported)
    # a handle swapped in through _lib.using is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_ig_attribution.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_ig_attribution.argtypes) == sigs["isg_ig_attribution"][1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="integrated-gradients ABI version 2, binding expects 1"):
            X.load()
    # a symbol declared twice is refused; the header lies outside the table of device headers, whose table did not move; the
    # rollout's header is among the others this one is held against
    assert not NAMES & set(X.declared_elsewhere()) and "isg_ig.h" not in _lib.HEADERS
    assert set(_ext_rollout.SIGNATURES) <= set(X.declared_elsewhere())
    with pytest.raises(_lib.IsgError, match="`isg_ig_attribution` is declared in include/isg_x.h and in include/ext/isg_ig.h"):
        X.refuse_redeclared(X.SIGNATURES, {"isg_ig_attribution": "isg_x.h"})
    with pytest.raises(_lib.IsgError, match="include/ext/isg_rollout.h and in include/ext/isg_ig.h"):
        X.refuse_redeclared({"isg_attention_rollout": None}, X.declared_elsewhere())
    # the build lists the header and checks the version, the counters exist, the kernels are plain HIP
    build_checks("isg_ig.h")
    build_checks("isg_rollout.h")
    assert ops.COUNTERS["ig_path_rows"] >= 0 and ops.COUNTERS["ig_attribution"] >= 0
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_ig.hip")).read()).lower()
    assert "atomic" not in text and "printf" not in text and "assert" not in text and "asm" not in text
    assert "__shared__" not in text and text.count("__launch_bounds__(ig_threads)") == 2
    assert ge.EXTRA_FLAGS["isg_ig.hip"] == ["-fno-slp-vectorize"]


def test_path_rows_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_ig as X
    lib = X.load()

    def call(x=P, ldx=8, x_rows=5, b_x=P, ldbx=8, node_src=P, inst_of=P, n_out=7, x_out=P, ldxo=8, Cx=8,
             e=P, lde=4, e_rows=3, b_e=P, ldbe=0, edge_src=P, einst_of=P, m_out=6, e_out=P, ldeo=4, Ce=4, t=P, Q=2, path_e=1):
        return lib.isg_ig_path_rows(x, ldx, x_rows, b_x, ldbx, node_src, inst_of, n_out, x_out, ldxo, Cx,
                                    e, lde, e_rows, b_e, ldbe, edge_src, einst_of, m_out, e_out, ldeo, Ce, t, Q, path_e, None)

    for k in ("x_rows", "n_out", "e_rows", "m_out", "Q"):
        assert call(**{k: -1}) == EINVAL, k
    for k in ("n_out", "m_out", "Q"):
        assert call(**{k: BIG}) == EUNSUPPORTED and call(**{k: 1 << 31}) == EUNSUPPORTED, k
    for k in ("x", "node_src", "inst_of", "x_out", "e", "edge_src", "einst_of", "e_out", "t"):
        assert call(**{k: None}) == EINVAL, k
    assert call(Cx=0) == EINVAL and call(Ce=0) == EINVAL and call(Cx=-4) == EINVAL
    assert call(ldx=4) == EINVAL and call(ldxo=4) == EINVAL and call(lde=0) == EINVAL and call(ldeo=0) == EINVAL
    assert call(ldbx=4) == EINVAL and call(ldbx=-8) == EINVAL and call(ldbe=-4) == EINVAL
    # what is no multiple of 4, or not aligned
    assert call(Cx=6) == EUNSUPPORTED and call(ldx=10) == EUNSUPPORTED and call(ldxo=9) == EUNSUPPORTED and call(ldbx=10) == EUNSUPPORTED
    assert call(Ce=2, lde=4) == EUNSUPPORTED and call(lde=6) == EUNSUPPORTED and call(ldbe=6) == EUNSUPPORTED
    for k in ("x", "b_x", "x_out", "e", "b_e", "e_out"):
        assert call(**{k: P + 4}) == EUNSUPPORTED, k
    # a plain copy of the edges looks at neither their baseline nor their instance numbers; without node rows t is not needed either
    assert call(path_e=0, b_e=P + 4, ldbe=-4, einst_of=None, n_out=0, t=None, m_out=0) == 0
    assert call(path_e=0, einst_of=None, b_e=P + 4, ldbe=2, Q=BIG) == EUNSUPPORTED            # (refused for Q alone)
    # a half without rows is not looked at; both empty: ISG_OK, nothing is launched
    assert call(n_out=0, m_out=0, x=None, node_src=None, inst_of=None, x_out=None, e=None, edge_src=None, einst_of=None, e_out=None,
                t=None, Cx=0, Ce=0, ldx=0, lde=0) == 0
    assert call(n_out=0, m_out=0, Q=-1) == EINVAL


def test_attribution_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_ig as X
    lib = X.load()

    def call(g_xo=P, ldgx=8, xo_rows=10, x=P, ldx=8, b_x=P, ldbx=8, attr_x=P, avg_x=P, ldax=8, x_rows=5, Cx=8,
             g_eo=P, ldge=4, eo_rows=6, e=P, lde=4, b_e=P, ldbe=0, attr_e=P, avg_e=None, ldae=0, e_rows=3, Ce=4,
             w=P, ptr=P, erange=P, inst_ptr=P, inst_eptr=P, gptr=P, glist=P, G=2, Q=4, accumulate=0):
        return lib.isg_ig_attribution(g_xo, ldgx, xo_rows, x, ldx, b_x, ldbx, attr_x, avg_x, ldax, x_rows, Cx,
                                      g_eo, ldge, eo_rows, e, lde, b_e, ldbe, attr_e, avg_e, ldae, e_rows, Ce,
                                      w, ptr, erange, inst_ptr, inst_eptr, gptr, glist, G, Q, accumulate, None)

    for k in ("xo_rows", "x_rows", "eo_rows", "e_rows", "G", "Q"):
        assert call(**{k: -1}) == EINVAL, k
    for k in ("xo_rows", "x_rows", "eo_rows", "e_rows", "G", "Q"):
        assert call(**{k: BIG}) == EUNSUPPORTED, k
    for k in ("g_xo", "x", "attr_x", "g_eo", "e", "attr_e", "w", "ptr", "erange", "inst_ptr", "inst_eptr", "gptr", "glist"):
        assert call(**{k: None}) == EINVAL, k
    assert call(G=0) == EINVAL and call(Cx=0) == EINVAL and call(Ce=-4) == EINVAL
    assert call(ldgx=4) == EINVAL and call(ldx=4) == EINVAL and call(ldax=4) == EINVAL and call(ldbx=4) == EINVAL and call(ldbx=-8) == EINVAL
    assert call(ldge=0) == EINVAL and call(lde=0) == EINVAL and call(avg_e=P, ldae=0) == EINVAL and call(ldbe=-4) == EINVAL
    assert call(Cx=6) == EUNSUPPORTED and call(ldgx=10) == EUNSUPPORTED and call(ldx=9) == EUNSUPPORTED
    assert call(ldax=10) == EUNSUPPORTED and call(ldbx=10) == EUNSUPPORTED and call(ldge=6) == EUNSUPPORTED and call(ldbe=6) == EUNSUPPORTED
    for k in ("g_xo", "x", "b_x", "avg_x", "g_eo", "e", "b_e"):
        assert call(**{k: P + 4}) == EUNSUPPORTED, k
    assert call(avg_e=P + 4, ldae=4) == EUNSUPPORTED
    # the optional pointers may be missing; without instances neither the list, the weights nor the gradient rows are needed, but
    # such a call would launch (every row is written), so it is only asked to pass the checks up to a refusal behind them
    assert call(b_x=None, b_e=None, avg_x=None, Q=0, xo_rows=0, eo_rows=0, g_xo=None, g_eo=None, glist=None, w=None, Cx=6) == EUNSUPPORTED
    # a half without rows is not looked at; both empty: ISG_OK, nothing is launched
    assert call(x_rows=0, e_rows=0, g_xo=None, x=None, attr_x=None, g_eo=None, e=None, attr_e=None, w=None, ptr=None, erange=None,
                inst_ptr=None, inst_eptr=None, gptr=None, glist=None, G=0, Q=0, Cx=0, Ce=0) == 0
    assert call(x_rows=0, e_rows=0, G=-1) == EINVAL


def test_quadrature_rules():
    from isubgvqa_amd import explain
    assert inspect.signature(explain.quadrature).parameters["rule"].default == "gauss_legendre"
    for rule, sizes in (("midpoint", (1, 2, 3, 16, 33)), ("trapezoid", (2, 3, 16)), ("gauss_legendre", (1, 2, 5, 16, 32)), ("endpoint", (1,))):
        for S in sizes:
            t, w = explain.quadrature(S, rule)
            assert t.dtype == w.dtype == torch.float64 and t.shape == w.shape == (S,) and t.device.type == "cpu"
            assert abs(float(w.sum()) - 1.0) <= 1e-15, (rule, S)
            assert bool((t >= 0).all()) and bool((t <= 1).all()) and bool((w > 0).all())
    for S in (1, 2, 3, 8, 16):                           # Gauss-Legendre is exact up to degree 2 S - 1
        t, w = explain.quadrature(S, "gauss_legendre")
        assert abs(float((w * t ** (2 * S - 1)).sum()) - 1.0 / (2 * S)) <= 1e-14, S
    t, w = explain.quadrature(4, "midpoint")
    assert t.tolist() == [0.125, 0.375, 0.625, 0.875] and w.tolist() == [0.25] * 4
    t, w = explain.quadrature(3, "trapezoid")
    assert t.tolist() == [0.0, 0.5, 1.0] and w.tolist() == [0.25, 0.5, 0.25]
    t, w = explain.quadrature(5, "trapezoid")
    assert t.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0] and w.tolist() == [0.125, 0.25, 0.25, 0.25, 0.125]
    assert [v.tolist() for v in explain.quadrature(1, "endpoint")] == [[1.0], [1.0]]
    for steps, rule in ((0, "midpoint"), (-3, "gauss_legendre"), (2.5, "midpoint"), (True, "midpoint"), (1, "trapezoid"),
                        (2, "endpoint"), (4, "simpson"), (4, None)):
        with pytest.raises(ValueError, match="quadrature"):
            explain.quadrature(steps, rule)


def test_the_known_answer_of_the_header():
    x, base, t, w, rows, g, G, attr = IR.known_answer()
    src, inst_of = [0, 1, 0, 1], [0, 0, 1, 1]
    assert IR.path_rows(x, base, src, inst_of, t).tolist() == rows
    gptr, glist = IR.by_graph([0, 0], 1)
    assert (gptr, glist) == ([0, 2], [0, 1])
    a, avg, bound, avg_bound, most = IR.attribution(g, w, x, base, [0, 2], [0, 2, 4], gptr, glist)
    assert a.tolist() == attr and avg.tolist() == G and most == 2
    assert bound.tolist() == [2 * 1 + 2 * 1 + 4 * 0.75, 2 * 1 + 2 * 4] and avg_bound[0].tolist() == [2.0, 1.0, 1.0, 0.75]
    header = re.sub(r"\s+\*\s+", " ", open(os.path.join(ROOT, "include", "ext", "isg_ig.h")).read())
    for text in ("t = [0.25, 0.75]", "w = [0.5, 0.5]", "x = [[1, 2, 3, 4], [-1, 0, 1, 2]]", "b = [1, 0, 1, 0]",
                 "[[1, 0.5, 1.5, 1], [0.5, 0, 1, 0.5], [1, 1.5, 2.5, 3], [-0.5, 0, 1, 1.5]]",
                 "g = [[1, 1, 1, 1], [2, 0, -2, 4], [3, -1, 1, 0.5], [0, 2, 2, -4]]", "[[2, 0, 1, 0.75], [1, 1, 0, 0]]", "= [5, -2]"):
        assert text in header, text
    # the two ends of the path, a baseline of zeros, rows of baselines; accumulation adds, and a graph without an instance keeps
    assert torch.equal(IR.path_rows(x, base, src, inst_of, torch.tensor([0.0, 1.0])), torch.stack([base, base, x[0], x[1]]).double())
    assert IR.path_rows(x, None, src, inst_of, t)[2].tolist() == [0.75, 1.5, 2.25, 3.0]
    b2 = torch.stack([base, 2 * base])
    assert IR.path_rows(x, b2, src, inst_of, t)[1].tolist() == [1.25, 0.0, 1.75, 0.5]
    twice = IR.attribution(g, w, x, base, [0, 2], [0, 2, 4], gptr, glist, attr_in=a, avg_in=avg)
    assert twice[0].tolist() == [10.0, -4.0] and twice[1].tolist() == [[4.0, 0.0, 2.0, 1.5], [2.0, 2.0, 0.0, 0.0]]
    kept = IR.attribution(g, w, x, base, [0, 2], [0, 2, 4], [0, 0], glist, attr_in=a)
    assert kept[0].tolist() == attr and kept[4] == 0
    # the skip rules: an instance number outside [0, Q), a short instance range, a copy row beyond the gradient rows, a bad source row
    assert IR.attribution(g, w, x, base, [0, 2], [0, 2, 4], gptr, [0, 7])[0].tolist() == [0.5 * (2 + 2 + 4), 0.5 * (-4 + 8)]
    assert IR.attribution(g, w, x, base, [0, 2], [0, 2, 3], gptr, glist)[1][1].tolist() == [1.0, 0.0, -1.0, 2.0]
    assert IR.attribution(g[:3], w, x, base, [0, 2], [0, 2, 4], gptr, glist)[1][1].tolist() == [1.0, 0.0, -1.0, 2.0]
    out = IR.path_rows(x, base, [0, 2, -1, 1], [0, 0, 1, 5], t)
    assert out[0].tolist() == rows[0] and bool(torch.isnan(out[1:]).all())


def test_explainer_names_and_the_refusals():
    from isubgvqa_amd import explain, synthetic
    from isubgvqa_amd.models.isubgvqa import ISubGVQA
    assert explain.EXPLAINERS_GRADIENT == ("integrated_gradients", "grad_x_input")
    assert explain.EXPLAINERS == ("intrinsic", "occlusion", "random") and explain.EXPLAINERS_ALL == explain.EXPLAINERS + ("attention",)
    p = inspect.signature(explain.compare).parameters
    assert p["explainers"].default is explain.EXPLAINERS and p["ig_steps"].default == 16
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2)
    assert explain.compare(model, [], None, explainers=("integrated_gradients",)).keys() == {"integrated_gradients"}
    assert list(explain.compare(model, [], None, explainers=("intrinsic", "grad_x_input", "attention"))) == ["intrinsic", "grad_x_input", "attention"]
    for bad in (("gradient",), ("integrated_gradients", "ig"), ()):
        with pytest.raises(ValueError, match="explainers"):
            explain.compare(None, [], None, explainers=bad)
    p = inspect.signature(explain.integrated_gradients).parameters
    assert [k for k in p][:2] == ["model", "inputs"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[2:])
    assert (p["steps"].default, p["rule"].default, p["baseline"].default, p["target"].default, p["edges"].default) == \
        (16, "gauss_legendre", "zero", "prob", False)
    p = inspect.signature(explain.path_attributions).parameters
    assert [k for k in p][:5] == ["score", "x", "e", "plan", "edge_index"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[5:])
    assert "trace" not in inspect.signature(ISubGVQA.forward).parameters
    for fn, names in ((__import__("isubgvqa_amd").ops.ig_path_rows, ["inst", "x", "e", "t", "base_x", "base_e", "path_edges"]),
                      (__import__("isubgvqa_amd").ops.ig_attribution, ["inst", "g_x", "g_e", "w", "x", "e", "base_x", "base_e", "want_rows", "out"])):
        assert list(inspect.signature(fn).parameters) == names


def test_a_model_in_train_mode_is_refused():
    from isubgvqa_amd import explain, synthetic
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2).train()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.integrated_gradients(model, None)
    with pytest.raises(ValueError, match="target"):
        explain.integrated_gradients(model.eval(), None, target="loss")
