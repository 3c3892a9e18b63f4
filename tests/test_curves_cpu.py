"""Host-side checks of the fidelity curves (include/ext/isg_curves.h) that need no GPU: the extension header, its
binding and the two libraries agree; both entry points refuse bad arguments before any launch; the header's known answer and the
level rule's discriminating cases on the restatement of tests/curves_restated.py; the quadrature weights by hand; the names and
defaults; a model in train() is refused."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

import curves_restated as CR

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
BIG = (1 << 31) - 1024
NAMES = {"isg_curve_abi_version", "isg_curve_keep_bits", "isg_curve_sums"}


def test_curves_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_curves as X
    from isubgvqa_amd import _ext_ig, _ext_induced, _ext_instances_train, _ext_maskopt, _ext_rollout, _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_curves.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_CURVES_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_curve_abi_version() == X.ABI_VERSION == abi == 1
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    sigs = {"isg_curve_abi_version": (ctypes.c_int, []),
            # (a, ptr, graphs, frac, count, N, G, R, L, sides, W, rank, level_k, index, keep, status, stream)
            "isg_curve_keep_bits": (ctypes.c_int, [ptr] * 5 + [i64] * 4 + [i32, i32] + [ptr] * 6),
            # (p_inst, w, R, L, sides, auc, totals, stream)
            "isg_curve_sums": (ctypes.c_int, [ptr, ptr, i64, i64, i32, ptr, ptr, ptr])}
    assert X.SIGNATURES == sigs
    for name, sig in sigs.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export exactly the header's symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_curve_abi_version.restype = ctypes.c_int
        assert raw.isg_curve_abi_version() == 1, other
        exported = set(m.decode() for m in re.findall(rb"\x00(isg_curve_[a-z0-9_]*)(?=\x00)", open(other, "rb").read()))
        assert exported == NAMES, (other, exported)
    # a handle swapped in through _lib.using is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_curve_sums.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_curve_sums.argtypes) == sigs["isg_curve_sums"][1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="fidelity-curve ABI version 2, binding expects 1"):
            X.load()
    # a symbol declared twice is refused; the header lies outside the table of device headers, whose table did not move; each of
    # the five other extension headers is among those this one is held against
    assert not NAMES & set(X.declared_elsewhere()) and "isg_curves.h" not in _lib.HEADERS and len(_lib.HEADERS) == 17
    with pytest.raises(_lib.IsgError, match="`isg_curve_sums` is declared in include/isg_x.h and in include/ext/isg_curves.h"):
        X.refuse_redeclared(X.SIGNATURES, {"isg_curve_sums": "isg_x.h"})
    for mod, file in ((_ext_instances_train, "isg_instances_train.h"), (_ext_induced, "isg_induced.h"), (_ext_rollout, "isg_rollout.h"),
                      (_ext_ig, "isg_ig.h"), (_ext_maskopt, "isg_maskopt.h")):
        assert set(mod.SIGNATURES) <= set(X.declared_elsewhere())
        name = sorted(mod.SIGNATURES)[-1]
        with pytest.raises(_lib.IsgError, match=f"`{name}` is declared in include/ext/{file} and in include/ext/isg_curves.h"):
            X.refuse_redeclared({name: None}, X.declared_elsewhere())
    # the build lists the header and checks the version, the counters exist, smoke() runs the known answer
    build_checks("isg_curves.h")
    assert ops.COUNTERS["curve_keep_bits"] >= 0 and ops.COUNTERS["curve_sums"] >= 0
    assert "_smoke_curves(dev)" in inspect.getsource(ge.smoke) and "counts=(1, 2)" in inspect.getsource(ge._smoke_curves)


def test_the_source_is_plain_hip_without_atomics():
    import __graft_entry__ as ge
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_curves.hip")).read()).lower()
    assert "atomic" not in text and "printf" not in text and "assert" not in text and "asm" not in text
    assert text.count("__global__") == 2 and text.count("<<<") == 2
    assert "fp contract(off)" in open(os.path.join(ge.CSRC, "isg_common.hpp")).read()       # mul_rn: the level rule's one product
    assert "ceilf(mul_rn(" in text and "__builtin_fmaf(" in text


def test_keep_bits_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_curves as X
    lib = X.load()
    fr = (ctypes.c_float * 64)(*([0.5] * 64))
    cn = (ctypes.c_int32 * 64)(*([3] * 64))
    F, C = ctypes.addressof(fr), ctypes.addressof(cn)

    def call(a=P, ptr=P, graphs=P, frac=F, count=None, N=10, G=2, R=2, L=3, sides=3, W=1, rank=P, level_k=P, index=P, keep=P, status=P):
        return lib.isg_curve_keep_bits(a, ptr, graphs, frac, count, N, G, R, L, sides, W, rank, level_k, index, keep, status, None)

    # every call below carries at least one fault, or no rows: none launches
    for k in ("N", "G", "R", "L"):
        assert call(**{k: -1}) == EINVAL, k
    for k in ("N", "G", "R"):
        assert call(**{k: BIG}, ptr=None) == EUNSUPPORTED and call(**{k: 1 << 31}, ptr=None) == EUNSUPPORTED, k
    assert call(R=BIG // 2, L=2, sides=1, ptr=None) == EUNSUPPORTED and call(R=BIG // 2, L=1, sides=3, ptr=None) == EUNSUPPORTED
    assert call(R=BIG // 2 - 1, L=1, sides=2, ptr=None) == EINVAL                # (inside the limit: the missing pointer is found)
    for bad in (0, 4, -1, 7):
        assert call(sides=bad) == EINVAL, bad
    assert call(W=0) == EINVAL and call(W=-3) == EINVAL and call(W=65) == EUNSUPPORTED and call(W=64, ptr=None) == EINVAL
    assert call(L=65) == EUNSUPPORTED and call(L=64, ptr=None) == EINVAL
    assert call(frac=F, count=C) == EINVAL and call(frac=None, count=None) == EINVAL
    assert call(frac=None, count=C, ptr=None) == EINVAL and call(frac=None, count=C, R=0) == 0
    # EINVAL is found before EUNSUPPORTED
    assert call(W=65, sides=0) == EINVAL and call(L=65, frac=None) == EINVAL and call(N=BIG, R=-1) == EINVAL
    # the levels' values
    for j, bad in ((0, float("nan")), (2, -0.25), (1, float("-inf"))):
        vals = [0.5] * 64
        vals[j] = bad
        arr = (ctypes.c_float * 64)(*vals)
        assert call(frac=ctypes.addressof(arr)) == EINVAL, (j, bad)
    arr = (ctypes.c_float * 64)(*([0.5] * 3 + [float("nan")] * 61))
    assert call(frac=ctypes.addressof(arr), R=0) == 0                             # (only the L values are looked at)
    arr = (ctypes.c_float * 64)(*([0.0, float("inf"), 3.0] + [0.0] * 61))
    assert call(frac=ctypes.addressof(arr), ptr=None) == EINVAL                   # (admitted values: the missing pointer is found)
    arr = (ctypes.c_int32 * 64)(*([3, -1] + [0] * 62))
    assert call(frac=None, count=ctypes.addressof(arr)) == EINVAL
    # a missing pointer where a launch would follow
    for k in ("a", "ptr", "graphs", "rank", "level_k", "index", "keep", "status"):
        assert call(**{k: None}) == EINVAL, k
    # no rows or no levels: ISG_OK whatever the pointers, nothing is launched
    assert call(R=0) == 0 and call(L=0) == 0 and call(L=0, frac=None, count=None) == 0
    assert call(R=0, a=None, ptr=None, graphs=None, rank=None, level_k=None, index=None, keep=None, status=None, N=0, G=0) == 0


def test_sums_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_curves as X
    lib = X.load()

    def call(p_inst=P, w=P, R=4, L=3, sides=3, auc=P, totals=P):
        return lib.isg_curve_sums(p_inst, w, R, L, sides, auc, totals, None)

    assert call(R=-1) == EINVAL and call(L=-1) == EINVAL
    for bad in (0, 4, -1):
        assert call(sides=bad) == EINVAL, bad
    assert call(L=65) == EUNSUPPORTED and call(R=BIG) == EUNSUPPORTED and call(R=BIG // 2, L=1, sides=3) == EUNSUPPORTED
    assert call(L=65, sides=0) == EINVAL
    for k in ("p_inst", "w", "auc", "totals"):
        assert call(**{k: None}) == EINVAL, k
    assert call(R=0) == 0 and call(L=0) == 0 and call(R=0, p_inst=None, w=None, auc=None, totals=None) == 0


def test_the_known_answer_of_the_header():
    a, ptr, counts, rank, rows, level_k = CR.known_answer()
    got_rank, got_k, index, keep, status, sets = CR.keep_bits(a, ptr, [0], counts=counts, sides=3, W=1)
    assert got_rank.tolist() == rank and keep.view(-1).tolist() == rows and got_k.tolist() == [level_k]
    assert index.tolist() == [0, 0, 0, 0] and status == [0, 0, 4, 0] and sets == [[1], [0, 2], [1, 2], [0]]
    header = re.sub(r"\s+\*\s+", " ", open(os.path.join(ROOT, "include", "ext", "isg_curves.h")).read())
    for text in ("a = [0.5, 2, 2]", "count = (1, 2)", "rank = [2, 0, 1]", "keep = [0b010, 0b101, 0b110, 0b001]",
                 "level_k = [[1, 1], [2, 2]]"):
        assert text in re.sub(r" +", " ", header), text
    # each side alone; the relation: NaNs last in node order, -0 = +0, ties to the lower node
    assert CR.keep_bits(a, ptr, [0], counts=counts, sides=1)[3].view(-1).tolist() == [0b010, 0b110]
    assert CR.keep_bits(a, ptr, [0], counts=counts, sides=2)[3].view(-1).tolist() == [0b101, 0b001]
    nan, inf = float("nan"), float("inf")
    assert CR.ranks(torch.tensor([nan, 0.0, -0.0, inf, -inf, nan, 1.0])).tolist() == [5, 2, 3, 0, 4, 6, 1]
    assert CR.ranks(torch.ones(5)).tolist() == [0, 1, 2, 3, 4]
    # no instance is empty: the keep side holds at least one node, the remove side leaves at least one; n = 0 gives zero rows
    _, k, _, keep, status, sets = CR.keep_bits([3.0, 1.0, 2.0, 9.0], [0, 3, 3, 4], [0, 1, 2, 5], counts=(0, 1000), sides=3)
    assert k.tolist() == [[[1, 0], [3, 2]], [[0, 0], [0, 0]], [[1, 0], [1, 0]], [[0, 0], [0, 0]]] and status == [0, 1, 16, 0]
    assert keep.view(-1).tolist() == [0b001, 0b111, 0b111, 0b010, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
    # ptr is clamped to [0, N] and to non-decreasing; a graph beyond 32 W nodes ranks its first 32 W and sets the flag
    assert CR.graph_range([0, 7, 3, 99], 1, 10, 1) == (7, 0, False) and CR.graph_range([-4, 7, 3, 99], 2, 10, 1) == (3, 7, False)
    big = torch.arange(40.0)
    rank, k, _, keep, status, _ = CR.keep_bits(big, [0, 40], [0], counts=(2,), sides=1, W=1)
    assert status[0] == 1 and rank[:32].tolist() == list(range(31, -1, -1)) and rank[32:].tolist() == [-1] * 8
    assert keep.view(-1).tolist() == [0b11 << 30]


def test_the_level_rule_is_one_fp32_product():
    cases = ((0.1, 10), (0.1, 20), (0.2, 5), (0.2, 65), (0.3, 10))
    assert [CR.level_sizes(n, [f])[0] for f, n in cases] == [1, 2, 1, 13, 3]
    assert [CR.level_sizes_double(n, [f])[0] for f, n in cases] == [2, 3, 2, 14, 4]
    assert CR.level_sizes(7, [0.0, 1e-9, 1.0, 3.0, float("inf")]) == [0, 1, 7, 7, 7]
    assert [CR.side_k(7, t, False) for t in (0, 1, 7, 1000)] == [1, 1, 7, 7] and [CR.side_k(7, t, True) for t in (0, 1, 7, 1000)] == [0, 1, 6, 6]
    assert CR.side_k(1, 5, True) == 0 and CR.side_k(1, 0, False) == 1 and CR.side_k(0, 5, False) == 0 and CR.side_k(0, 5, True) == 0


def test_curve_weights_against_the_trapezoid_rule_by_hand():
    from isubgvqa_amd import explain
    w = explain.curve_weights(explain.CURVE_FRACTIONS)
    assert w.dtype == torch.float64 and torch.allclose(w, torch.tensor([0.05, 0.1, 0.1, 0.15, 0.2, 0.25, 0.15], dtype=torch.float64), rtol=0, atol=1e-15)
    assert abs(float(w.sum()) - 1.0) < 1e-15
    x = (0.0, 0.25, 1.0)
    y = torch.tensor([0.5, 1.0, 0.25], dtype=torch.float64)
    by_hand = 0.25 * (0.5 + 1.0) / 2 + 0.75 * (1.0 + 0.25) / 2
    assert abs(float((explain.curve_weights(x) * y).sum()) - by_hand) < 1e-15
    assert explain.curve_weights((0.3,)).tolist() == [1.0] and explain.curve_weights((0.0, 1.0), "mean").tolist() == [0.5, 0.5]
    assert explain.curve_weights((1 / 5, 5 / 5)).tolist() == [0.4, 0.4]                    # counts (1, 5) over their largest
    for bad in ((), (0.5, 0.2), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="level axis"):
            explain.curve_weights(bad)
    with pytest.raises(ValueError, match="rule"):
        explain.curve_weights((0.0, 1.0), "simpson")
    # the restated sums: a skipped graph is counted in the skipped slot alone, its area is NaN
    p = torch.tensor([0.5, 0.25, 0.75, 0.125, float("inf"), 0.5, 0.5, 0.5])
    auc, bound, totals, tb = CR.sums(p, [0.5, 0.5], 2, 2, 2)
    assert auc[0].tolist() == [0.625, 0.1875] and torch.isnan(auc[1, 0]) and float(auc[1, 1]) == 0.5
    assert totals.tolist() == [[0.5, 0.75, 0.625, 1.0, 1.0], [0.75, 0.625, 0.6875, 2.0, 0.0]]
    assert float(bound[0, 0]) == 2 * CR.U * 0.625 and float(tb[1, 0]) == 2 * 2.0 ** -53 * 0.75


def test_names_defaults_and_the_refusals():
    from isubgvqa_amd import _lib, explain, ops, synthetic
    assert explain.CURVE_FRACTIONS == (0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0)
    assert explain.EXPLAINERS == ("intrinsic", "occlusion", "random") and explain.EXPLAINERS_ALL == explain.EXPLAINERS + ("attention",)
    assert explain.COMPARE_SUMS == 6
    p = inspect.signature(explain.compare).parameters
    assert p["explainers"].default is explain.EXPLAINERS and p["curves"].default is None and list(p)[-1] == "curves"
    fields = list(explain.ExplainerReport.__dataclass_fields__)
    assert fields == ["coo", "grounding", "fid_plus", "fid_minus", "jaccard", "sums", "curves"]
    assert explain.ExplainerReport.__dataclass_fields__["curves"].default is None
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2)
    out = explain.compare(model, [], None, explainers=("intrinsic", "random"))
    assert all(r.curves is None for r in out.values())
    out = explain.compare(model, [], None, explainers=("intrinsic", "random"), curves=(0.0, 0.5, 1.0))
    for r in out.values():
        c = r.curves
        assert c.fractions == (0.0, 0.5, 1.0) and c.counted == (0, 0) and c.skipped == (0, 0) and len(c.p_keep) == len(c.p_remove) == 3
        assert c.auc_keep != c.auc_keep and c.auc_remove != c.auc_remove                   # no graph: NaN
    c = explain.CurveReport.from_totals((0.0, 1.0), [[1.0, 3.0, 2.0, 4.0, 1.0], [0.5, 0.25, 0.375, 1.0, 0.0]])
    assert (c.p_keep, c.p_remove, c.auc_keep, c.auc_remove, c.counted, c.skipped) == ((0.25, 0.75), (0.5, 0.25), 0.5, 0.375, (4, 1), (1, 0))
    with pytest.raises(ValueError, match="level axis"):
        explain.compare(model, [], None, curves=(0.5, 0.1))
    p = inspect.signature(explain.fidelity_curves).parameters
    assert list(p)[:3] == ["model", "inputs", "scores"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[3:])
    want = dict(fractions=explain.CURVE_FRACTIONS, counts=None, sides=("keep", "remove"), noises=None, seed=None, max_instances=None,
                logits=None, plan=None, totals=None)
    assert {k: p[k].default for k in want} == want
    assert list(explain.FidelityCurves.__dataclass_fields__)[:9] == ["pred", "p", "rank", "level_k", "p_keep", "p_remove", "auc_keep",
                                                                     "auc_remove", "totals"]
    for cls in (explain.Occlusion, explain.Rollout, explain.PathAttributions, explain.MaskOptimization):
        assert callable(cls.scores) and "before the shift" in cls.scores.__doc__
    p = inspect.signature(ops.curve_keep_bits).parameters
    assert list(p) == ["a", "plan", "graphs", "fractions", "counts", "sides"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[2:])
    assert p["sides"].default == ("keep", "remove") and p["graphs"].default is None
    assert list(inspect.signature(ops.curve_sums).parameters) == ["p_inst", "bits", "w", "totals"]
    assert [f for f in ops.CurveBits.__dataclass_fields__][:8] == ["index", "keep", "rank", "level_k", "status", "graphs", "L", "S"]
    assert callable(ops.CurveBits.verify)
    for bad in ((), ("keep", "keep"), ("both",), "insert"):
        with pytest.raises(ValueError, match="sides"):
            ops._curve_sides(bad)
    assert ops._curve_sides("keep") == 1 and ops._curve_sides(("remove",)) == 2 and ops._curve_sides(("keep", "remove")) == 3
    with pytest.raises(ValueError, match="not both"):
        explain._curve_levels((0.1, 0.2), (1, 2))
    assert explain._curve_levels(explain.CURVE_FRACTIONS, (1, 5)) == (None, (1, 5), (0.2, 1.0))
    with pytest.raises(_lib.IsgError, match="must live on the GPU"):
        ops.curve_sums(torch.zeros(0), ops.CurveBits(None, None, None, None, None, torch.zeros(0, dtype=torch.int32), 2, 2, 3),
                       torch.zeros(2))


def test_a_model_in_train_mode_is_refused():
    from isubgvqa_amd import explain, synthetic
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2).train()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.fidelity_curves(model, None, None)
    with pytest.raises(ValueError, match="max_instances"):
        explain.fidelity_curves(model.eval(), None, None, max_instances=0)
