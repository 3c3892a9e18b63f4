"""Host-side checks of the induced-subgraph instances (include/ext/isg_induced.h) that need no GPU: the extension
header, its binding and the two libraries agree; the entry points refuse bad arguments before any launch; the restatement of
tests/induced_restated.py equals the CHAIN of the two existing restatements (expansion, mask, cut) as integers; the bit helpers
against loops; InducedInstances refuses the training forms; the arithmetic behind Occlusion.mask on attributions written by hand."""
import argparse
import ctypes
import inspect
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT

import induced_cases as C
import induced_restated as IR

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
P = 4096                        # any non-null, aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_induced_abi_version", "isg_induced_workspace_bytes", "isg_induced_size", "isg_induced_fill"}


def test_induced_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _ext_induced as X
    from isubgvqa_amd import _lib, ops
    assert X.HEADER_PATH == os.path.join(ROOT, "include", "ext", "isg_induced.h")
    header = open(X.HEADER_PATH).read()
    declared = set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(X.SIGNATURES) == NAMES
    assert (X.SIGNATURES, X.ABI_VERSION) == _lib.read_header(X.HEADER_PATH)
    abi = int(re.search(r"#define ISG_INDUCED_ABI_VERSION (\d+)", header).group(1))
    lib = X.load()
    assert lib is _lib.load() and lib.isg_induced_abi_version() == X.ABI_VERSION == abi == 1
    i64, ptr, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    sigs = {"isg_induced_abi_version": (ctypes.c_int, []),
            "isg_induced_workspace_bytes": (sz, [i64, i64]),
            # (ptr, batch, edge_index, index, keep, W, N, E, G, Q, inst_ptr, inst_eptr, status, workspace, workspace_bytes, stream)
            "isg_induced_size": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, i64, i64, i64, i64, i64, ptr, ptr, ptr, ptr, sz, ptr]),
            # (ptr, edge_index, index, keep, W, N, E, G, Q, inst_ptr, inst_eptr, workspace, workspace_bytes, cap_nodes, cap_edges,
            #  batch_out, edge_index_out, node_src, edge_src, stream)
            "isg_induced_fill": (ctypes.c_int, [ptr, ptr, ptr, ptr, i64, i64, i64, i64, i64, ptr, ptr, ptr, sz, i64, i64, ptr, ptr,
                                                ptr, ptr, ptr])}
    assert X.SIGNATURES == sigs
    for name, sig in sigs.items():
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    for other in (_lib.LIB_PATH, ge.STRICT_LIB):          # the product library and its strict twin export exactly the header's symbols
        raw = ctypes.CDLL(other)
        for name in declared:
            assert hasattr(raw, name), (other, name)
        raw.isg_induced_abi_version.restype = ctypes.c_int
        assert raw.isg_induced_abi_version() == 1, other
        exported = set(m.decode() for m in re.findall(rb"\x00(isg_induced_[a-z0-9_]+)(?=\x00)", open(other, "rb").read()))
        assert exported == NAMES, (other, exported)
    # a handle swapped in through _lib._lib is bound and checked the first time load() sees it
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB))
    assert strict.isg_induced_fill.argtypes is None
    with _lib.using(strict):
        assert X.load() is strict and list(strict.isg_induced_fill.argtypes) == sigs["isg_induced_fill"][1]
    assert X.load() is lib

    class Stale:                                         # a library of another version is refused, by name
        def __getattr__(self, name):
            return (lambda: 2) if name == X.VERSION_SYMBOL else getattr(lib, name)
    with _lib.using(Stale()):
        with pytest.raises(_lib.IsgError, match="induced-instance ABI version 2, binding expects 1"):
            X.load()
    # a symbol declared twice is refused; the header lies outside the table of device headers
    assert not NAMES & set(_lib._declared_in) and "isg_induced.h" not in _lib.HEADERS
    with pytest.raises(_lib.IsgError, match="`isg_induced_size` is declared in include/isg_x.h and in include/ext/isg_induced.h"):
        X.refuse_redeclared(X.SIGNATURES, {"isg_induced_size": "isg_x.h"})
    # the build checks the version, the smoke run has its case, the counter exists, the kernels use no atomic, printf or assert
    build_checks("isg_induced.h")
    assert "isg_induced_abi_version()" in inspect.getsource(ge._smoke_induced)
    assert ops.COUNTERS["induced_instances"] >= 0
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_induced.hip")).read()).lower()
    assert "atomic" not in text and "printf" not in text and "assert" not in text and "asm" not in text
    assert "__ballot(" in text and "__popc" in text


def test_induced_entry_points_refuse_bad_arguments_before_any_launch():
    from isubgvqa_amd import _ext_induced as X
    lib = X.load()
    assert lib.isg_induced_workspace_bytes(3, 5) == 4 * (3 + 1 + 2 * 5) and lib.isg_induced_workspace_bytes(0, 0) == 4
    assert lib.isg_induced_workspace_bytes(-1, 5) == 0 and lib.isg_induced_workspace_bytes(3, -1) == 0

    def size(ptr=P, batch=P, ei=P, index=P, keep=P, W=2, N=10, E=20, G=3, Q=5, iptr=P, ieptr=P, status=P, ws=P, wsb=1 << 20):
        return lib.isg_induced_size(ptr, batch, ei, index, keep, W, N, E, G, Q, iptr, ieptr, status, ws, wsb, None)

    def fill(ptr=P, ei=P, index=P, keep=P, W=2, N=10, E=20, G=3, Q=5, iptr=P, ieptr=P, ws=P, wsb=1 << 20, cn=7, ce=9, bo=P, eo=P,
             ns=P, es=P):
        return lib.isg_induced_fill(ptr, ei, index, keep, W, N, E, G, Q, iptr, ieptr, ws, wsb, cn, ce, bo, eo, ns, es, None)

    for k in ("ptr", "batch", "ei", "index", "iptr", "ieptr", "status"):
        assert size(**{k: None}) == EINVAL, k
    for k in ("ptr", "ei", "index", "iptr", "ieptr", "bo", "eo", "ns", "es"):
        assert fill(**{k: None}) == EINVAL, k
    for call, sizes in ((size, ("N", "E", "G", "Q")), (fill, ("N", "E", "G", "Q", "cn", "ce"))):
        for k in sizes:
            assert call(**{k: -1}) == EINVAL, k
            assert call(**{k: 1 << 31}) == EUNSUPPORTED and call(**{k: (1 << 31) - 1024}) == EUNSUPPORTED, k
        assert call(G=0) == EINVAL
        assert call(W=0) == EINVAL and call(W=-3) == EINVAL
        assert call(W=65) == EUNSUPPORTED                       # one word of keep per lane of the instance's wave
        assert call(ws=None) == EWORKSPACE and call(wsb=4 * (3 + 1 + 2 * 5) - 1) == EWORKSPACE
        # Q == 0: nothing is looked at beyond the numbers
        assert call(Q=0, ptr=None, index=None, iptr=None, ieptr=None, ws=None, wsb=0, G=0) == 0
        assert call(Q=0, N=-1) == EINVAL
    # without a keep W is not looked at; without edges neither batch nor edge_index
    assert size(keep=None, W=0, batch=None, ei=None, E=0, ws=None) == EWORKSPACE
    assert size(keep=None, W=1000, ws=None) == EWORKSPACE and fill(keep=None, W=-1, ws=None) == EWORKSPACE
    # the fill pass with no capacity at all launches nothing; a half without capacity comes without its pointers
    assert fill(cn=0, ce=0, bo=None, eo=None, ns=None, es=None, ei=None) == 0
    assert fill(cn=0, bo=None, ns=None, ws=None) == EWORKSPACE and fill(ce=0, ei=None, eo=None, es=None, ws=None) == EWORKSPACE


CPU_CASES = [(1, 1), (1, 2), (1, 65), (3, 1), (3, 2), (3, 65), (3, 1025), (70, 2), (70, 65)]


@pytest.mark.parametrize("G,Q", CPU_CASES, ids=[f"G{g}-Q{q}" for g, q in CPU_CASES])
def test_the_restatement_equals_the_chain_of_the_two_existing_restatements(G, Q):
    """As integers, for every kind of bits; for random bits also with one word more than needed and one word too few (the nodes
    beyond 32 W are dropped by both)."""
    batch, ei, sizes = C.make_graphs(C.spec_of(G, Q), seed=100 + G)
    index = C.index_of(G, Q, seed=Q)
    W = C.words_min(sizes)
    runs = [(kind, W) for kind in C.BITS] + [("random", W + 1)] + ([("random", W - 1), ("all", W - 1)] if W > 1 else [])
    whole = None
    for kind, w in runs:
        keep = C.bits_of(kind, index, sizes, w, seed=7 * Q + w)
        r = IR.induce(batch, ei, index, keep, G)
        C.assert_same(r, C.chain(batch, ei, index, keep, G), f"{kind}, W = {w}")
        assert r.status.tolist()[2:] == [0, 0] and r.ptr[-1] == r.batch.numel() == r.node_src.numel()
        if kind in ("all", "none") and w == W:              # every node kept: the plain expansion, field for field
            x = C.R.expand(batch, ei, index, G)
            for k in IR.Restated._fields:
                assert torch.equal(getattr(r, k), getattr(x, k)), (kind, k)
            whole = r
        if kind == "zero":
            assert r.status.tolist() == [0, 0, 0, 0] and r.ptr.tolist() == [0] * (Q + 1)
        if w < W:
            assert r.batch.numel() < whole.batch.numel() or max(sizes[g] for g in index.tolist()) <= 32 * w


def test_the_restatement_flags_a_bad_index_and_a_bad_grouping():
    batch, ei, sizes = C.make_graphs(C.spec_of(3, 2), seed=1)
    index = torch.tensor([2, 3, 0, -1, 1])
    keep = C.bits_of("random", index, sizes, 3, seed=3)
    r = IR.induce(batch, ei, index, keep, 3)
    assert r.status[2:].tolist() == [1, 0] and r.ptr[1] == r.ptr[2] and r.ptr[3] == r.ptr[4] and r.eptr[3] == r.eptr[4]
    good = index.clamp(0, 2)
    C.assert_same(IR.induce(batch, ei, good, keep, 3), C.chain(batch, ei, good, keep, 3), "random")
    assert IR.induce(batch, ei.flip(1), good, keep, 3).status[3] == 1


def _plan_of(sizes):
    n = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([n.new_zeros(1), n.cumsum(0)])
    return argparse.Namespace(ptr=ptr.int(), B=len(sizes), N=int(ptr[-1]), nmax=max(sizes),
                              batch=torch.repeat_interleave(torch.arange(len(sizes)), n))


HELPER_SIZES = [5, 0, 1, 32, 33, 2, 64, 65, 0]


def test_leave_one_out_bits_against_loops():
    from isubgvqa_amd import ops
    plan = _plan_of(HELPER_SIZES)
    index, keep, inst_node = ops.keep_bits_leave_one_out(plan)
    W = 3
    assert ops.keep_words(65) == W == keep.size(1) and ops.keep_words(64) == 2 and ops.keep_words(0) == 1 and ops.keep_words(33) == 2
    assert index.dtype == torch.int32 and keep.dtype == torch.int32 and inst_node.dtype == torch.int64 and keep.is_contiguous()
    want_index, want_node, want_flags = [], [], []
    for g, n in enumerate(HELPER_SIZES):
        if n < 2:
            continue                                            # no nodes, one node: no instance
        for j in range(n):
            want_index.append(g)
            want_node.append(int(plan.ptr[g]) + j)
            want_flags.append([i != j for i in range(n)])
    assert index.tolist() == want_index and inst_node.tolist() == want_node
    assert torch.equal(keep, IR.pack(want_flags, W))
    assert IR.node_flags(keep, index, HELPER_SIZES) == want_flags
    # a list of graphs, in the caller's order
    index2, keep2, node2 = ops.keep_bits_leave_one_out(plan, graphs=torch.tensor([5, 1, 2, 0]))
    assert index2.tolist() == [5, 5] + [0] * 5 and node2.tolist() == [71, 72, 0, 1, 2, 3, 4]
    assert torch.equal(keep2, IR.pack([[False, True], [True, False]] + [[i != j for i in range(5)] for j in range(5)], W))
    # nothing to remove anywhere
    index3, keep3, node3 = ops.keep_bits_leave_one_out(_plan_of([1, 0, 1]))
    assert index3.numel() == node3.numel() == 0 and tuple(keep3.shape) == (0, 1)


@pytest.mark.parametrize("complement", [False, True])
def test_mask_bits_against_loops(complement):
    from isubgvqa_amd import ops
    plan = _plan_of(HELPER_SIZES)
    gen = torch.Generator().manual_seed(5)
    mask = torch.rand(plan.N, generator=gen) - 0.4
    mask[3], mask[40] = float("nan"), 0.25
    for shape, thr in (((plan.N,), 0.0), ((plan.N, 1), 0.25)):
        keep = ops.keep_bits_from_mask(mask.view(shape), plan, threshold=thr, complement=complement)
        flags = [[bool(mask[int(plan.ptr[g]) + i] > thr) != complement for i in range(n)] for g, n in enumerate(HELPER_SIZES)]
        assert tuple(keep.shape) == (len(HELPER_SIZES), 3) and torch.equal(keep, IR.pack(flags, 3))
    with pytest.raises(ValueError):
        ops.keep_bits_from_mask(mask[:-1], plan)


def test_induced_instances_refuse_the_training_forms():
    from isubgvqa_amd import ops
    z = torch.zeros(0, dtype=torch.int64)
    inst = ops.InducedInstances(argparse.Namespace(B=2, N=0, E=0), torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                                torch.zeros(4, dtype=torch.int32), z, z.view(2, 0), z, z, torch.zeros(4, dtype=torch.int32),
                                keep=torch.zeros(3, 1, dtype=torch.int32))
    assert isinstance(inst, ops.GraphInstances) and inst.Q == 3 and inst.keep is not None
    with pytest.raises(NotImplementedError, match="by_graph"):
        inst.by_graph()
    with pytest.raises(NotImplementedError, match="counts"):
        inst.counts()
    x, e = torch.zeros(0, 4, requires_grad=True), torch.zeros(0, 4)
    with pytest.raises(NotImplementedError, match="no backward"):
        inst.gather_rows(x, e)
    with pytest.raises(NotImplementedError, match="no backward"):
        inst.gather_rows(e, x)
    assert inst.gather_nodes(torch.zeros(0, 2)).shape == (0, 2)
    # the parent class keeps its forms
    whole = ops.GraphInstances(argparse.Namespace(B=2, N=0, E=0), torch.tensor([1, 0, 1], dtype=torch.int32),
                               torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), z, z.view(2, 0), z, z,
                               torch.zeros(4, dtype=torch.int32))
    assert whole.counts().tolist() == [1, 2]


def test_occlusion_mask_scores_let_no_pad_win():
    """Occlusion.mask hands ops.topk_threshold the attributions shifted per graph; in the padded rows the pads hold 0.  Three
    graphs written by hand -- all attributions negative; mixed; one node -- and the threshold rule restated on padded rows."""
    from isubgvqa_amd import explain
    att = torch.tensor([-0.5, -0.125, -0.25, -0.75,   0.25, -0.5, 0.0,   -0.375])
    batch = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2])
    s = explain.shifted_attributions(att, batch, 3)
    assert s.dtype == torch.float32
    assert s.tolist() == [1.25, 1.625, 1.5, 1.0,   1.75, 1.0, 1.5,   1.0]
    ptr, nmax = [0, 4, 7, 8], 4
    for k, want in ((1, [0, 1, 0, 0, 1, 0, 0, 1]), (2, [0, 1, 1, 0, 1, 0, 1, 1]), (4, [1, 1, 1, 1, 1, 1, 1, 1])):
        got = []
        for g in range(3):
            row = s[ptr[g]:ptr[g + 1]].tolist()
            padded = row + [0.0] * (nmax - len(row))           # the samplers' pads compete
            kth = sorted(padded, reverse=True)[k - 1]
            sel = [v >= kth for v in padded]
            assert not any(sel[len(row):]) or k > len(row), "a pad was picked while nodes were left"
            got += [int(v) for v in sel[:len(row)]]
        assert got == want, (k, got)
    # unshifted, the pads would have won over the negative attributions of graph 0
    assert float(att[:4].max()) < 0.0 < float(s[:4].min())
    # a graph without nodes between others, and attributions that are all equal
    s2 = explain.shifted_attributions(torch.tensor([0.5, 0.5, -1.0]), torch.tensor([0, 0, 2]), 3)
    assert s2.tolist() == [1.0, 1.0, 1.0]
