"""Host-side checks of Shapley sampling (include/ext/isg_shapley.h) that need no GPU: the extension header, its
binding and the two libraries agree; both entry points refuse bad arguments before any launch; the header's known answer on the
restatement of tests/shapley_restated.py; the restatement's own properties on fixed seeds (permutations, the antithetic reversal,
independence of the listing, uniformity); the names and defaults; a model in train() is refused."""
import collections
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

import shapley_restated as SR

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
BIG = (1 << 31) - 1024
NAMES = {"isg_shapley_abi_version", "isg_shapley_keep_bits", "isg_shapley_values"}


def test_shapley_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_shapley as X
    from isubgvqa_amd import _ext_curves, _ext_ig, _ext_induced, _ext_instances_train, _ext_maskopt, _ext_rollout, _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_shapley.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_SHAPLEY_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_shapley_abi_version() == X.ABI_VERSION == abi == 1
    i32, i64, u64, f32, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
    sigs = {"isg_shapley_abi_version": (ctypes.c_int, []),
            # (ptr, graphs, row_ptr, N, G, R, M, Q, antithetic, seed, W, pos, index, keep, status, stream)
            "isg_shapley_keep_bits": (ctypes.c_int, [ptr] * 3 + [i64] * 5 + [i32, u64, i32] + [ptr] * 5),
            # (p_inst, p, pos, ptr, graphs, row_ptr, N, G, R, M, Q, antithetic, v_empty, W, phi, m2, gap, flag, stream)
            "isg_shapley_values": (ctypes.c_int, [ptr] * 6 + [i64] * 5 + [i32, f32, i32] + [ptr] * 5)}
    assert X.SIGNATURES == sigs
    for name, sig in sigs.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export exactly the header's symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_shapley_abi_version.restype = ctypes.c_int
        assert raw.isg_shapley_abi_version() == 1, other
        exported = set(m.decode() for m in re.findall(rb"\x00(isg_shapley_[a-z0-9_]*)(?=\x00)", open(other, "rb").read()))
        assert exported == NAMES, (other, exported)
    # a handle swapped in through _lib.using is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_shapley_values.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_shapley_values.argtypes) == sigs["isg_shapley_values"][1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="Shapley-sampling ABI version 2, binding expects 1"):
            X.load()
    # a symbol declared twice is refused; the header lies outside the table of device headers, whose table did not move; each of
    # the six other extension headers is among those this one is held against
    assert not NAMES & set(X.declared_elsewhere()) and "isg_shapley.h" not in _lib.HEADERS and len(_lib.HEADERS) == 17
    with pytest.raises(_lib.IsgError, match="`isg_shapley_values` is declared in include/isg_x.h and in include/ext/isg_shapley.h"):
        X.refuse_redeclared(X.SIGNATURES, {"isg_shapley_values": "isg_x.h"})
    for mod, file in ((_ext_instances_train, "isg_instances_train.h"), (_ext_induced, "isg_induced.h"), (_ext_rollout, "isg_rollout.h"),
                      (_ext_ig, "isg_ig.h"), (_ext_maskopt, "isg_maskopt.h"), (_ext_curves, "isg_curves.h")):
        assert set(mod.SIGNATURES) <= set(X.declared_elsewhere())
        name = sorted(mod.SIGNATURES)[-1]
        with pytest.raises(_lib.IsgError, match=f"`{name}` is declared in include/ext/{file} and in include/ext/isg_shapley.h"):
            X.refuse_redeclared({name: None}, X.declared_elsewhere())
    # the build lists the header and checks the version, the counters exist, smoke() runs the known answer
    build_checks("isg_shapley.h")
    assert ops.COUNTERS["shapley_keep_bits"] >= 0 and ops.COUNTERS["shapley_values"] >= 0
    assert "_smoke_shapley(dev)" in inspect.getsource(ge.smoke) and "seed=0x100000007" in inspect.getsource(ge._smoke_shapley)


def test_the_source_is_plain_hip_without_atomics():
    import __graft_entry__ as ge
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_shapley.hip")).read()).lower()
    assert "atomic" not in text and "printf" not in text and "assert" not in text and "asm" not in text
    assert text.count("__global__") == 2 and text.count("<<<") == 2
    assert "fp contract(off)" in open(os.path.join(ge.CSRC, "isg_common.hpp")).read()       # sub_rn / add_rn / mul_rn: the estimator's steps
    for step in ("sub_rn(v_hi, v_lo)", "mul_rn(0.5f, add_rn(d0, d1))", "add_rn(acc, e)", "__builtin_fmaf(e, e, sq)", "__fdiv_rn(acc, tf)",
                 "philox::draw(seed, (uint32_t)g, sv_stream |"):
        assert step in text, step


def _keep_call(lib):
    def call(ptr=P, graphs=P, row_ptr=P, N=10, G=2, R=2, M=4, Q=12, antithetic=1, seed=5, W=1, pos=P, index=P, keep=P, status=P):
        return lib.isg_shapley_keep_bits(ptr, graphs, row_ptr, N, G, R, M, Q, antithetic, seed, W, pos, index, keep, status, None)
    return call


def _values_call(lib):
    def call(p_inst=P, p=P, pos=P, ptr=P, graphs=P, row_ptr=P, N=10, G=2, R=2, M=4, Q=12, antithetic=1, v_empty=0.0, W=1, phi=P, m2=P,
             gap=P, flag=P):
        return lib.isg_shapley_values(p_inst, p, pos, ptr, graphs, row_ptr, N, G, R, M, Q, antithetic, v_empty, W, phi, m2, gap, flag, None)
    return call


@pytest.mark.parametrize("entry", ["keep_bits", "values"])
def test_entry_points_refuse_bad_arguments_before_any_launch(entry):
    from isubgvqa_amd import _ext_shapley as X
    lib = X.load()
    call = _keep_call(lib) if entry == "keep_bits" else _values_call(lib)
    # every call below carries at least one fault, or no rows: none launches
    for k in ("N", "G", "R", "M", "Q"):
        assert call(**{k: -1}) == EINVAL, k
    assert call(M=0) == EINVAL and call(M=3) == EINVAL and call(M=3, antithetic=0, ptr=None) == EINVAL
    for bad in (-1, 2, 7):
        assert call(antithetic=bad) == EINVAL, bad
    assert call(W=0) == EINVAL and call(W=-3) == EINVAL and call(W=65) == EUNSUPPORTED and call(W=64, ptr=None) == EINVAL
    assert call(M=1026) == EUNSUPPORTED and call(M=1025, antithetic=0) == EUNSUPPORTED and call(M=1024, ptr=None) == EINVAL
    for k in ("N", "G", "R", "Q"):
        assert call(**{k: BIG}, ptr=None) == EUNSUPPORTED and call(**{k: 1 << 31}, ptr=None) == EUNSUPPORTED, k
        assert call(**{k: BIG - 1}, M=1, antithetic=0, ptr=None) == EINVAL, k        # (inside the limit: the missing pointer is found)
    assert call(N=BIG // 2, M=2, ptr=None) == EUNSUPPORTED and call(N=BIG // 1024 + 1, M=1024, ptr=None) == EUNSUPPORTED
    assert call(N=BIG // 2 - 1, M=2, ptr=None) == EINVAL
    # EINVAL is found before EUNSUPPORTED
    assert call(W=65, antithetic=2) == EINVAL and call(M=1025) == EINVAL and call(N=BIG, R=-1) == EINVAL and call(M=2000, W=0) == EINVAL
    # a missing pointer where a launch would follow
    needed = ("ptr", "graphs", "row_ptr", "pos", "index", "keep", "status") if entry == "keep_bits" else \
        ("p_inst", "p", "pos", "ptr", "graphs", "row_ptr", "phi", "gap", "flag")
    for k in needed:
        assert call(**{k: None}) == EINVAL, k
    # no listed graph: ISG_OK whatever the pointers, nothing is launched
    assert call(R=0) == 0
    if entry == "keep_bits":
        assert call(R=0, ptr=None, graphs=None, row_ptr=None, pos=None, index=None, keep=None, status=None, N=0, G=0, Q=0) == 0
    else:
        assert call(R=0, p_inst=None, p=None, pos=None, ptr=None, graphs=None, row_ptr=None, phi=None, m2=None, gap=None, flag=None) == 0
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert call(v_empty=bad) == EINVAL and call(v_empty=bad, R=0) == EINVAL and call(v_empty=bad, W=65) == EINVAL, bad


def test_the_known_answer_of_the_header():
    seed, key, pos_rows, rows, p_inst, p, phi = SR.known_answer()
    assert SR.keys(seed, 0, 0, 3).tolist() == key and SR.positions(SR.keys(seed, 0, 0, 3)).tolist() == pos_rows[0]
    row_ptr = SR.row_ptr_of([0, 3], [0], 3, 2, 1)
    assert row_ptr == [0, 4]
    pos, index, keep, status, sets, written = SR.keep_bits([0, 3], [0], row_ptr, 3, 2, 4, True, seed, 1)
    assert pos.tolist() == pos_rows and keep.view(-1).tolist() == rows and index.tolist() == [0, 0, 0, 0] and status == [0, 0, 0, 4]
    assert sets == {0: [1], 1: [1, 2], 2: [0], 3: [0, 2]} and bool(written.all())
    for dtype in (torch.float32, torch.float64):
        got_phi, m2, gap, flag, abs_e, sq_e = SR.values(p_inst, [p], pos, [0, 3], [0], row_ptr, 3, 2, 4, True, 0.0, 1, dtype)
        assert got_phi.tolist() == phi and m2.tolist() == [0.09765625, 0.0625, 0.19140625] and gap.tolist() == [0.0] and flag.tolist() == [0]
        assert abs_e.tolist() == phi and sq_e.tolist() == m2.tolist() and sum(phi) == p
    header = re.sub(r" +", " ", re.sub(r"\s+\*\s+", " ", open(os.path.join(ROOT, "include", "ext", "isg_shapley.h")).read()))
    for text in ("g = 0, seed = 0x100000007, M = 2, antithetic, W = 1", "key = [0xB8A65C43, 0x29FF42B2, 0x3C12D07E]",
                 "pos = [[2, 0, 1], [0, 2, 1]]", "keep = [0b010, 0b110, 0b001, 0b101]", "p_inst = [0.25, 0.5, 0.125, 0.75], p = [1], v_empty = 0",
                 "phi = [0.3125, 0.25, 0.4375]", "m2 = [0.09765625, 0.0625, 0.19140625], gap = [0], flag = [0]"):
        assert text in header, text
    # without antithetic the second permutation is draw 1's; v_empty moves the first node of every permutation alone
    pos2 = SR.graph_positions(seed, 0, 3, 2, False)
    assert pos2[0].tolist() == pos_rows[0] and pos2[1].tolist() == SR.positions(SR.keys(seed, 0, 1, 3)).tolist()
    shifted = SR.values(p_inst, [p], pos, [0, 3], [0], row_ptr, 3, 2, 4, True, 0.125, 1)[0]
    assert shifted.tolist() == [0.3125 - 0.0625, 0.25 - 0.0625, 0.4375] and float(shifted.sum()) == p - 0.125


@pytest.mark.parametrize("n", [1, 2, 3, 33, 64, 65])
def test_positions_are_permutations_and_the_twin_is_the_reversal(n):
    for seed in (0x5EED, (1 << 40) + 3):
        pm = SR.graph_positions(seed, 4, n, 6, True)
        for m in range(6):
            assert sorted(pm[m].tolist()) == list(range(n)), (seed, m)
        assert torch.equal(pm[1::2], n - 1 - pm[0::2])
        plain = SR.graph_positions(seed, 4, n, 3, False)
        assert torch.equal(plain, pm[0::2])                                    # draw t is permutation t, or the pair 2 t / 2 t + 1
        if n >= 33:
            assert not torch.equal(pm[0], pm[2]) and not torch.equal(pm[0], SR.graph_positions(seed + 1, 4, n, 2, True)[0])
    # ties go to the lower node
    assert SR.positions([5, 1, 5, 1, 0]).tolist() == [3, 1, 4, 2, 0]


def test_a_graphs_positions_do_not_depend_on_the_listing():
    sizes = [3, 0, 33, 1, 7]
    ptr = [0, 3, 3, 36, 37, 44]
    N, M, W, seed = 44, 4, 2, 0x5EED

    def run(graphs):
        rp = SR.row_ptr_of(ptr, graphs, N, M, W)
        return SR.keep_bits(ptr, graphs, rp, N, M, rp[-1], True, seed, W), rp

    (alone, _, keep_a, st_a, _, _), rp_a = run([2])
    (among, _, keep_b, st_b, _, _), rp_b = run([0, 1, 2, 3, 4])
    (back, _, keep_c, st_c, _, _), rp_c = run([4, 3, 2, 1, 0])
    assert st_a == [0, 0, 0, 4 * 32] and st_b == [0, 0, 0, 4 * (2 + 32 + 6)] and st_c == st_b
    assert torch.equal(alone[:, 3:36], among[:, 3:36]) and torch.equal(among, back) and bool((alone[:, :3] == -1).all())
    assert torch.equal(keep_a, keep_b[rp_b[2]:rp_b[3]]) and torch.equal(keep_a, keep_c[rp_c[2]:rp_c[3]])
    assert rp_b == [0, 8, 8, 136, 136, 160] and rp_c == [0, 24, 24, 152, 152, 160]
    # the faults of the listing: an entry outside the batch, a graph beyond 32 W nodes, a short, a negative and an inconsistent row_ptr
    assert SR.keep_bits(ptr, [5, 0], [0, 0, 8], N, M, 8, True, seed, W)[3] == [0, 1, 0, 8]
    assert SR.keep_bits(ptr, [2], [0, 124], N, M, 124, True, seed, 1)[3] == [1, 0, 0, 124]
    pos, index, keep, status, _, written = SR.keep_bits(ptr, [0, 4], [0, 8, 32], N, M, 31, True, seed, W)
    assert status == [0, 0, 1, 31] and bool(written[:8].all()) and not bool(written[8:].any()) and bool((pos[:, 37:] == -1).all())
    pos, _, _, status, _, written = SR.keep_bits(ptr, [0, 4], [-1, 7, 31], N, M, 31, True, seed, W)
    assert status == [0, 0, 1, 31] and bool((pos[:, :3] == -1).all()) and bool(written[7:].all()) and not bool(written[:7].any())
    assert SR.keep_bits(ptr, [0, 4], [0, 9, 33], N, M, 40, True, seed, W)[3] == [0, 0, 1, 40]


def test_uniformity_of_the_permutations_of_three_nodes():
    """6 000 draws (graphs 0 .. 5999, draw 0, seed 0x5EED): each of the 6 permutations within 5 sigma of 1 000, that is within
    145 (sigma = sqrt(6000 * 1/6 * 5/6) = 28.9).  The bound is a condition, set before the counts were looked at."""
    seen = collections.Counter(tuple(SR.positions(SR.keys(0x5EED, g, 0, 3)).tolist()) for g in range(6000))
    assert len(seen) == 6 and sum(seen.values()) == 6000
    assert all(abs(c - 1000) <= 145 for c in seen.values()), seen


def test_the_estimator_restated_on_games_with_a_known_answer():
    ptr, graphs, N, M, W, seed = [0, 5, 6, 6, 9], [0, 1, 2, 3], 9, 6, 1, 11
    for antithetic in (True, False):
        rp = SR.row_ptr_of(ptr, graphs, N, M, W)
        Q = rp[-1]
        pos, index, keep, status, sets, _ = SR.keep_bits(ptr, graphs, rp, N, M, Q, antithetic, seed, W)
        c = torch.tensor([0.25, 0.0, 0.125, 0.5, 0.0625, 0.75, 0.5, 0.25, 0.0])
        p_inst = torch.tensor([float(sum(c[ptr[int(index[q])] + i] for i in sets[q])) for q in range(Q)])
        p = torch.tensor([float(c[ptr[g]:ptr[g + 1]].sum()) for g in graphs])
        phi, m2, gap, flag, _, _ = SR.values(p_inst, p, pos, ptr, graphs, rp, N, M, Q, antithetic, 0.0, W)
        assert torch.equal(phi, c) and gap.tolist() == [0.0] * 4 and flag.tolist() == [0] * 4        # additive: phi_i = c_i; a dummy gets 0
        T = SR.draws(M, antithetic)
        assert torch.equal(m2, T * c * c)


def test_names_defaults_and_the_refusals():
    from isubgvqa_amd import _lib, explain, ops, synthetic
    assert ops.SHAPLEY_PERMUTATIONS_MAX == SR.PERMUTATIONS_MAX == 1024
    assert explain.EXPLAINERS_SAMPLED == ("shapley",)
    assert explain.EXPLAINERS == ("intrinsic", "occlusion", "random") and explain.EXPLAINERS_ALL == explain.EXPLAINERS + ("attention",)
    assert explain.EXPLAINERS_GRADIENT == ("integrated_gradients", "grad_x_input") and explain.EXPLAINERS_LEARNED == ("mask_optimization",)
    assert explain.COMPARE_SUMS == 6
    p = inspect.signature(explain.compare).parameters
    assert list(p)[-2:] == ["sv_permutations", "curves"] and p["sv_permutations"].default == 16 and p["explainers"].default is explain.EXPLAINERS
    assert list(explain.ExplainerReport.__dataclass_fields__) == ["coo", "grounding", "fid_plus", "fid_minus", "jaccard", "sums", "curves"]
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2)
    out = explain.compare(model, [], None, explainers=("shapley",))
    assert list(out) == ["shapley"] and out["shapley"].curves is None and out["shapley"].sums == (0.0,) * 6
    out = explain.compare(model, [], None, explainers=("intrinsic", "shapley"), sv_permutations=4, curves=(0.0, 1.0))
    assert out["shapley"].curves.counted == (0, 0)
    with pytest.raises(ValueError, match="explainers from"):
        explain.compare(model, [], None, explainers=("shap",))
    p = inspect.signature(explain.shapley_values).parameters
    assert list(p)[:2] == ["model", "inputs"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[2:])
    want = dict(noises=None, seed=None, permutations=16, antithetic=True, perm_seed=0, v_empty=0.0, max_instances=None, logits=None, plan=None)
    assert {k: p[k].default for k in list(p)[2:]} == want and list(p)[2:] == list(want)
    assert list(explain.ShapleyValues.__dataclass_fields__) == ["pred", "p", "attribution", "m2", "gap", "flag", "single", "bits", "p_inst",
                                                                "logits", "plan", "chunks"]
    assert "before the shift" in explain.ShapleyValues.scores.__doc__ and callable(explain.ShapleyValues.mask)
    p = inspect.signature(ops.shapley_keep_bits).parameters
    assert list(p) == ["plan", "graphs", "permutations", "antithetic", "seed"] and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[1:])
    assert [p[k].default for k in list(p)[1:]] == [None, 16, True, 0]
    p = inspect.signature(ops.shapley_values).parameters
    assert list(p) == ["p_inst", "p", "bits", "plan", "v_empty", "want_m2"] and p["v_empty"].default == 0.0 and p["want_m2"].default is True
    assert list(ops.ShapleyBits.__dataclass_fields__) == ["index", "keep", "pos", "row_ptr", "status", "graphs", "M", "antithetic"]
    assert callable(ops.ShapleyBits.verify)
    bits = ops.ShapleyBits(None, None, None, None, None, torch.zeros(0, dtype=torch.int32), 6, True)
    assert bits.T == 3 and bits.R == 0 and dataclasses_replace(bits, antithetic=False).T == 6
    # the standard error: sqrt(max(m2 - T phi^2, 0) / (T (T - 1))) in float64; NaN at T = 1
    res = explain.ShapleyValues(None, None, torch.tensor([0.5, 0.25]), torch.tensor([1.0, 0.1875]), None, None, None, bits, None, None, None)
    assert res.T == 3 and res.stderr().dtype == torch.float64
    assert res.stderr().tolist() == [math.sqrt(0.25 / 6), 0.0]
    one = explain.ShapleyValues(None, None, torch.tensor([0.5]), torch.tensor([0.25]), None, None, None,
                                dataclasses_replace(bits, M=1, antithetic=False), None, None, None)
    assert bool(torch.isnan(one.stderr()).all())

    class NoPlan:
        N, B, nmax = 3, 1, 3
        ptr = torch.tensor([0, 3], dtype=torch.int32)
    with pytest.raises(_lib.IsgError, match="1 to 1024"):
        ops.shapley_keep_bits(NoPlan, permutations=1026)
    with pytest.raises(ValueError, match="pairs"):
        ops.shapley_keep_bits(NoPlan, permutations=3)
    with pytest.raises(ValueError, match="64-bit"):
        ops.shapley_keep_bits(NoPlan, seed=-1)
    with pytest.raises(_lib.IsgError, match="must live on the GPU"):
        ops.shapley_keep_bits(NoPlan)


def dataclasses_replace(obj, **kw):
    import dataclasses
    return dataclasses.replace(obj, **kw)


def test_a_model_in_train_mode_is_refused():
    from isubgvqa_amd import explain, synthetic
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2).train()
    with pytest.raises(ValueError, match=r"eval\(\)"):
        explain.shapley_values(model, None)
    with pytest.raises(ValueError, match="max_instances"):
        explain.shapley_values(model.eval(), None, max_instances=0)
