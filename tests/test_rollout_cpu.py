"""Host-side checks of the attention rollout (include/ext/isg_rollout.h) that need no GPU: the known answer and the
conservation law through the restatement of tests/rollout_restated.py; the extension header, its binding and the two libraries
agree; the entry point refuses bad arguments before any launch; ops.run_split's per-edge merge against index_copy_ with a stub
core; the explainer names; a trace together with a capture is refused."""
import argparse
import ctypes
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

import rollout_restated as RR

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_rollout_abi_version", "isg_rollout_max_layers", "isg_rollout_max_nodes", "isg_attention_rollout"}


def test_the_known_answer_of_the_header():
    ei = torch.tensor([[0, 1, 0], [0, 1, 1]])
    rowptr, eid, dst = RR.source_csr(ei, 2)
    assert (rowptr.tolist(), eid.tolist(), dst.tolist()) == ([0, 2, 3], [0, 2, 1], [0, 1, 1])
    alpha = torch.tensor([[1.0], [0.25], [0.75]])
    start = torch.tensor([0.0, 1.0])
    for fn in (RR.rollout, RR.rollout_fp32):
        rel, flow = fn([0, 2], rowptr, eid, dst, [alpha], start, None, 0.5)
        assert rel.tolist() == [0.375, 0.625] and flow.tolist() == [[0.0, 0.125, 0.375]], fn.__name__
    header = open(os.path.join(ROOT, "include", "ext", "isg_rollout.h")).read()
    assert "relevance = [0.375, 0.625] and flow[0] = [0, 0.125, 0.375]" in header
    # the residual's two ends: everything stays, nothing stays
    assert RR.rollout([0, 2], rowptr, eid, dst, [alpha], start, None, 1.0)[0].tolist() == [0.0, 1.0]
    assert RR.rollout([0, 2], rowptr, eid, dst, [alpha], start, None, 0.0)[0].tolist() == [0.75, 0.25]
    # a layer mask that drops node 0: its self loop and the edge out of it carry nothing
    rel, flow = RR.rollout([0, 2], rowptr, eid, dst, [alpha], start, [torch.tensor([0.0, 1.0])], 0.5)
    assert rel.tolist() == [0.0, 0.625] and flow.tolist() == [[0.0, 0.125, 0.0]]


def test_the_restatements_rules():
    """Out-of-range slots contribute nothing, a graph beyond nmax gets NaN rows, ptr is clamped -- and the two variants agree."""
    ptr, batch, ei, dmax = RR.make_graphs([3, 0, 5, 2], [0, 1, 3], seed=3)
    N, E = batch.numel(), ei.size(1)
    rowptr, eid, dst = RR.source_csr(ei, N)
    gen = torch.Generator().manual_seed(4)
    alphas = [0.25 + 0.75 * torch.rand(E, 3, generator=gen) for _ in range(2)]
    start = 0.25 + 0.75 * torch.rand(N, generator=gen)
    whole, flow = RR.rollout(ptr, rowptr, eid, dst, alphas, start)
    eid2, dst2 = eid.clone(), dst.clone()
    other = int(rowptr[4])                               # a slot of node 4 (graph 2: nodes 3 .. 7), sent to node 0 of graph 0
    bad = [0, 5, 7, other]
    assert len(set(bad)) == 4 and 3 <= _slot_source(rowptr, other) < 8
    eid2[0], eid2[5], dst2[7], dst2[other] = -1, E, N + 3, 0
    rel2, flow2 = RR.rollout(ptr, rowptr, eid2, dst2, alphas, start)
    assert not torch.equal(rel2, whole) and not bool(torch.isnan(rel2).any())
    skipped = torch.zeros(E, dtype=torch.bool)
    skipped[eid[bad].long()] = True
    assert float(flow2[:, skipped].abs().sum()) == 0.0 and torch.equal(flow2[:, ~skipped][1], flow[:, ~skipped][1])
    assert bool((flow[:, skipped] > 0).all()) and bool((rel2 <= whole).all())
    rel3, flow3 = RR.rollout(ptr, rowptr, eid, dst, alphas, start, nmax=4)
    assert torch.isnan(rel3[3:8]).all() and torch.equal(rel3[:3], whole[:3]) and torch.equal(rel3[8:], whole[8:])
    assert float(flow3[:, (batch[ei[0]] == 2)].abs().sum()) == 0.0
    # a ptr that runs beyond N and back: clamped to [0, N], made non-decreasing
    rel4, _ = RR.rollout([0, 3, 3, N + 9, 5], rowptr, eid, dst, alphas, start)
    assert rel4.shape == (N,) and torch.equal(rel4[:3], whole[:3])
    for kw in ({}, {"nmax": 4}, {"masks": [None, (torch.arange(N) % 3 != 0).float()], "residual": 0.25}):
        a, fa = RR.rollout(ptr, rowptr, eid2, dst2, alphas, start, **kw)
        b, fb = RR.rollout_fp32(ptr, rowptr, eid2, dst2, alphas, start, **kw)
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        ok = ~torch.isnan(a)
        assert float((a[ok] - b[ok].double()).abs().max()) <= 1e-5 and float((fa - fb.double()).abs().max()) <= 1e-5


def _slot_source(rowptr, j):
    return int((rowptr.long() <= j).sum()) - 1


@pytest.mark.parametrize("H,L,lam", [(1, 1, 0.5), (4, 3, 0.5), (3, 8, 0.25), (4, 2, 0.0)])
def test_conservation_on_softmax_inputs(H, L, lam):
    """A true softmax per destination, no mask, a self loop on every node: each graph's relevance sums to its start's sum."""
    sizes = [1, 7, 0, 12, 3]
    ptr, batch, ei, _ = RR.make_graphs(sizes, [0, 2, 1, 5], seed=10 + H)
    N, E = batch.numel(), ei.size(1)
    gen = torch.Generator().manual_seed(L)
    alphas = [RR.softmax_by_destination(torch.randn(E, H, generator=gen), ei[1], N) for _ in range(L)]
    start = torch.rand(N, generator=gen)
    rel, flow = RR.rollout(ptr, *RR.source_csr(ei, N), alphas, start, None, lam)
    for g in range(len(sizes)):
        want = float(start[ptr[g]:ptr[g + 1]].double().sum())
        assert abs(float(rel[ptr[g]:ptr[g + 1]].sum()) - want) <= 1e-6 * max(want, 1.0), g
    assert flow.shape == (L, E) and bool((flow >= 0).all())


def test_rollout_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_rollout as X
    from isubgvqa_amd import _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_rollout.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_ROLLOUT_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_rollout_abi_version() == X.ABI_VERSION == abi == 1
    assert lib.isg_rollout_max_layers() == 8 == ops.ROLLOUT_MAX_LAYERS and lib.isg_rollout_max_nodes() >= 2048
    assert lib.isg_rollout_max_nodes() >= ops.MAX_NODES_PER_GRAPH          # every plan's bound can be launched
    i64, ptr = ctypes.c_int64, ctypes.c_void_p
    sigs = {"isg_rollout_abi_version": (ctypes.c_int, []), "isg_rollout_max_layers": (ctypes.c_int, []),
            "isg_rollout_max_nodes": (ctypes.c_int, []),
            # (ptr, rowptr_s, eid_s, dst_s, layers, L, H, residual, start, N, E, B, nmax, relevance, edge_flow, stream)
            "isg_attention_rollout": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, i64, i64, ctypes.c_float, ptr, i64, i64, i64, i64, ptr,
                                                     ptr, ptr])}
    assert X.SIGNATURES == sigs
    for name, sig in sigs.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export exactly the header's symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_rollout_abi_version.restype = ctypes.c_int
        assert raw.isg_rollout_abi_version() == 1, other
        exported = set(m.decode() for m in re.findall(rb"\x00(isg_(?:rollout_|attention_rollout)[a-z0-9_]*)(?=\x00)", open(other, "rb").read()))
        assert exported == NAMES, (other, exported)
    # a handle swapped in through _lib.using is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_attention_rollout.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_attention_rollout.argtypes) == sigs["isg_attention_rollout"][1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="attention-rollout ABI version 2, binding expects 1"):
            X.load()
    # a symbol declared twice is refused; the header lies outside the table of device headers, whose table did not move
    assert not NAMES & set(X.declared_elsewhere()) and "isg_rollout.h" not in _lib.HEADERS
    with pytest.raises(_lib.IsgError, match="`isg_attention_rollout` is declared in include/isg_x.h and in include/ext/isg_rollout.h"):
        X.refuse_redeclared(X.SIGNATURES, {"isg_attention_rollout": "isg_x.h"})
    with pytest.raises(_lib.IsgError, match="include/ext/isg_induced.h and in include/ext/isg_rollout.h"):
        X.refuse_redeclared({"isg_induced_size": None}, X.declared_elsewhere())
    # the build checks the version, the counter exists, the kernel uses no atomic, printf, assert or inline assembly
    build_checks("isg_rollout.h")
    assert ops.COUNTERS["attention_rollout"] >= 0
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_rollout.hip")).read()).lower()
    assert "atomic" not in text and "printf" not in text and "assert" not in text and "asm" not in text
    assert "__launch_bounds__(roll_threads, 8)" in text and "extern __shared__ __align__(16)" in text


def test_rollout_entry_point_refuses_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_rollout as X
    lib = X.load()

    def table(L=2, alpha=P, lda=4, mask=0):
        rows = []
        for _ in range(L):
            rows += [alpha, lda, mask]
        return (ctypes.c_int64 * max(len(rows), 1))(*rows)

    def call(ptr=P, rowptr=P, eid=P, dst=P, layers="table", L=2, H=4, lam=0.5, start=P, N=10, E=20, B=3, nmax=8, rel=P, flow=P, **tk):
        t = table(max(min(L, 8), 1), **tk) if layers == "table" else None
        return lib.isg_attention_rollout(ptr, rowptr, eid, dst, None if t is None else ctypes.addressof(t), L, H, lam, start, N, E,
                                         B, nmax, rel, flow, None)

    for k in ("N", "E", "B", "nmax"):
        assert call(**{k: -1}) == EINVAL, k
    for k in ("N", "E", "B"):
        assert call(**{k: 1 << 31}) == EUNSUPPORTED and call(**{k: (1 << 31) - 1024}) == EUNSUPPORTED, k
    assert call(H=(1 << 31) - 1024, lda=1 << 31) == EUNSUPPORTED
    assert call(L=0) == EINVAL and call(L=-2) == EINVAL and call(H=0) == EINVAL and call(H=-4) == EINVAL
    assert call(L=9) == EUNSUPPORTED and call(nmax=lib.isg_rollout_max_nodes() + 1) == EUNSUPPORTED
    for lam in (-0.125, 1.5, float("nan"), float("inf")):
        assert call(lam=lam) == EINVAL, lam
    assert call(lda=3) == EINVAL and call(lda=0) == EINVAL and call(H=1, lda=0) == EINVAL
    assert call(lda=(1 << 31) - 1024) == EUNSUPPORTED
    for k in ("ptr", "rowptr", "eid", "dst", "start", "rel"):
        assert call(**{k: None}) == EINVAL, k
    assert call(layers=None) == EINVAL and call(alpha=0) == EINVAL
    # B == 0 or N == 0: nothing is looked at beyond the numbers
    for kw in ({"B": 0}, {"N": 0}):
        assert call(ptr=None, rowptr=None, eid=None, dst=None, layers=None, start=None, rel=None, flow=None, **kw) == 0
        assert call(L=0, **kw) == EINVAL and call(lam=2.0, **kw) == EINVAL and call(L=9, **kw) == EUNSUPPORTED


class _Sub(argparse.Namespace):
    pass


def test_run_split_merges_a_row_per_edge_through_the_sub_batchs_edge_ids():
    from isubgvqa_amd import ops
    N, E, B = 9, 14, 4
    gids, nodes, edges = torch.tensor([1, 3]), torch.tensor([2, 3, 7, 8]), torch.tensor([1, 4, 5, 11, 13])
    sub_plan = argparse.Namespace(nmax=3)
    sub = ops.OversizeGraphs(gids, nodes, edges, torch.tensor([0, 0, 1, 1]), torch.zeros(2, 5, dtype=torch.long), sub_plan)

    class Plan(argparse.Namespace):
        def with_holes(self, s):
            return self
    plan = Plan(N=N, E=E, B=B)
    x, ea = torch.arange(N * 2.0).view(N, 2), torch.arange(E * 3.0).view(E, 3)
    batch = torch.tensor([0, 0, 1, 1, 2, 2, 2, 3, 3])
    instr, glf = torch.zeros(1, B, 2), torch.zeros(B, 2)

    def core(x_, ei_, ea_, batch_, instr_, glf_, plan_, noises, seed, gate_feats):
        side = plan_ is sub_plan
        n, e, g = x_.size(0), ea_.size(0), glf_.size(0)
        fill = 100.0 if side else float("nan")            # the main pass leaves NaN: a row that the merge misses shows
        per_edge = [ea_[:, :2] + fill if side else torch.full((e, 2), fill), None, ea_[:, 0] + fill if side else torch.full((e,), fill)]
        return torch.full((g, 1), fill), x_[:, :1] + fill, per_edge, [x_ + fill, None]

    logits, per_node, per_edge, masks = ops.run_split(plan, sub, core, x, torch.zeros(2, E, dtype=torch.long), ea, batch, instr, glf,
                                                      kinds="gnen")
    want0 = torch.full((E, 2), float("nan")).index_copy_(0, edges, ea[edges][:, :2] + 100.0)
    want2 = torch.full((E,), float("nan")).index_copy_(0, edges, ea[edges][:, 0] + 100.0)
    assert per_edge[1] is None and isinstance(per_edge, list) and len(per_edge) == 3
    for got, want in ((per_edge[0], want0), (per_edge[2], want2)):
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    assert int(torch.isnan(per_edge[2]).sum()) == E - edges.numel()
    # "g" and "n" as before, lists element-wise
    assert torch.equal(torch.isnan(logits).view(-1), torch.tensor([True, False, True, False]))
    assert torch.equal(torch.nan_to_num(per_node)[nodes], x[nodes][:, :1] + 100.0) and masks[1] is None
    assert torch.equal(torch.nan_to_num(masks[0])[nodes], x[nodes] + 100.0) and int(torch.isnan(masks[0][:, 0]).sum()) == N - 4
    # the shape checks of "n" hold for "e": rows of the whole batch / of the sub-batch, equal widths
    def bad_rows(*a):
        out = list(core(*a))
        out[2] = out[2][0][:-1]
        return tuple(out)
    with pytest.raises(ValueError, match="run_split: a 'e' result"):
        ops.run_split(plan, sub, bad_rows, x, torch.zeros(2, E, dtype=torch.long), ea, batch, instr, glf, kinds="gnen")

    def bad_width(*a):
        out = list(core(*a))
        out[2] = out[2][0] if a[6] is sub_plan else out[2][0][:, :1]
        return tuple(out)
    with pytest.raises(ValueError, match="per-edge results of different widths"):
        ops.run_split(plan, sub, bad_width, x, torch.zeros(2, E, dtype=torch.long), ea, batch, instr, glf, kinds="gnen")
    with pytest.raises(ValueError, match="one letter"):
        ops.run_split(plan, sub, core, x, torch.zeros(2, E, dtype=torch.long), ea, batch, instr, glf, kinds="gnn")


def test_explainer_names_and_the_refusals():
    from isubgvqa_amd import explain, synthetic
    assert explain.EXPLAINERS == ("intrinsic", "occlusion", "random")
    assert explain.EXPLAINERS_ALL == explain.EXPLAINERS + ("attention",)
    assert inspect.signature(explain.compare).parameters["explainers"].default is explain.EXPLAINERS
    for bad in (("gradient",), ("intrinsic", "attention", "rollout"), ()):
        with pytest.raises(ValueError, match="explainers"):
            explain.compare(None, [], None, explainers=bad)
    assert explain.compare(synthetic.AnswerModel(8, 1, (1.0,), "imle", 2), [], None, explainers=("attention",)).keys() == {"attention"}
    t = explain.AttentionTrace()
    assert (t.alphas, t.masks, t.mask, t.gate) == (None, None, None, None)
    t.alphas = []                                        # mutable: the forward fills it
    r = explain.Rollout(torch.zeros(2), None, t, torch.zeros(1, 3), None)
    assert r.flow is None and r.trace is t
    for fn in (explain.attention_rollout,):
        p = inspect.signature(fn).parameters
        assert [k for k in p][:2] == ["model", "inputs"] and p["residual"].default == 0.5 and p["use_masks"].default is True
        assert p["want_flow"].default is False and all(p[k].kind is p[k].KEYWORD_ONLY for k in list(p)[2:])


def test_a_trace_together_with_a_capture_is_refused():
    from isubgvqa_amd import explain, synthetic
    from isubgvqa_amd.models.isubgvqa import ISubGVQA
    from isubgvqa_amd.models.mgat import MGAT
    model = synthetic.AnswerModel(8, 1, (1.0,), "imle", 2)
    with pytest.raises(ValueError, match="trace together with capture"):
        model(None, capture=True, trace=explain.AttentionTrace())
    from isubgvqa_amd.models import build_model
    torch.manual_seed(0)
    full = build_model(synthetic.full_model_args(sg_vocab_size=64, text_vocab_size=64), None).eval()
    for capture in (True, "language"):
        with pytest.raises(ValueError, match="trace together with capture"):
            full.forward_traced(explain.AttentionTrace(), None, None, None, None, None, None, return_masks=True, capture=capture)
    with pytest.raises(ValueError, match="needs a trace"):
        full.forward_traced(None)
    for fn in (MGAT.forward, synthetic.AnswerModel.forward, ISubGVQA.answer_graphs):
        assert inspect.signature(fn).parameters["trace"].default is None, fn.__qualname__
    # ISubGVQA.forward keeps the signature two existing tests pin; its trace comes through forward_traced(trace, ...)
    assert "trace" not in inspect.signature(ISubGVQA.forward).parameters
    assert list(inspect.signature(ISubGVQA._forward).parameters)[2:] == list(inspect.signature(ISubGVQA.forward).parameters)[1:]
