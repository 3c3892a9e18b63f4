"""isg_attention_rollout and ops.attention_rollout on the GPU (include/ext/isg_rollout.h) against the float64 loop of
tests/rollout_restated.py -- on the product library and on its strict twin, with guard words behind both outputs and a second
call that must give the first one's bits.

TOLERANCE (derived, not measured).  Every input is non-negative, so every output is a sum of non-negative terms and a relative
bound per term carries over to the sum.  Per layer a term goes through: H - 1 additions of the head sum, the rounded 1 / H and the
multiplication by it (2), two mask multiplications (2), the rounded 1 - lambda and its multiplication (2), the multiplication by
r[dst] (1), and at most d additions of the node's sum behind lambda * r[s] (1) -- H + d + 7 roundings of relative size
u = 2^-24 at the most, composed over L layers: (1 + u)^(L (H + d + 7)) - 1 < 2 k u with k = L (H + d + 6) for every case here
(k u < 1e-4).  So |got - ref| <= 2 k u ref, with d the largest out-degree of the case and ref the float64 restatement.  Inputs are
drawn so that every exact non-zero output is at least 1e-30 (asserted on the host): no output comes near the subnormals, and no
absolute term is needed.  An exact zero (a zero mask, a zero start, lambda at one of its ends) must come out as zero."""
import ctypes
import functools

import pytest
import torch

import rollout_restated as RR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7.0
U = 2.0 ** -24
ALL_SIZES = [0, 1, 2, 63, 64, 65, 130]
ALL_DEGREES = [0, 1, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """(fast, strict): the product library and its strict twin, both bound from include/ext/isg_rollout.h."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_rollout, _lib
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB), _ext_rollout.SIGNATURES)
    assert strict.isg_rollout_abi_version() == _ext_rollout.ABI_VERSION
    return _ext_rollout.load(), strict


def _case(id, sizes, deg, L, H, pad=0, misaligned=False, lam=0.5, masks="none", zero_start=(), flow=True, seed=0):
    return dict(id=id, sizes=tuple(sizes), deg=tuple(deg), L=L, H=H, pad=pad, misaligned=misaligned, lam=lam, masks=masks,
                zero_start=tuple(zero_start), flow=flow, seed=seed)


CASES = [
    _case("B1-n130-every-degree-L8-H4-vector", [130], ALL_DEGREES, 8, 4, masks="some"),
    _case("B1-n1-d129-L1-H1-lam0-no-flow", [1], [129], 1, 1, lam=0.0, flow=False),
    _case("B1-n64-L2-H3-lam1", [64], [1, 64], 2, 3, pad=3, lam=1.0, masks="some"),
    _case("B1-no-nodes", [0], [0], 2, 3, pad=3),
    _case("B3-n64-0-65-L4-H4-misaligned-zero-layer", [64, 0, 65], [1, 64, 0, 65], 4, 4, misaligned=True, masks="zero_layer",
          zero_start=[0]),
    _case("B3-n2-63-1-L2-H3-pad-no-flow", [2, 63, 1], [63, 0, 129], 2, 3, pad=3, masks="some", flow=False),
    _case("B3-n65-2-130-L1-H4-pad", [65, 2, 130], [2, 1, 0], 1, 4, pad=3, masks="all"),
    _case("B3-n63-L4-H1-pad-lam0", [63, 63, 2], [1, 0, 2], 4, 1, pad=3, lam=0.0, masks="some"),
    _case("B70-every-size-L2-H3", ALL_SIZES * 10, [0, 1, 2, 1, 3], 2, 3, masks="some", zero_start=range(0, 70, 5)),
    _case("B70-every-size-L8-H4-vector-no-flow", ALL_SIZES * 10, [1, 0, 2], 8, 4, masks="zero_layer", flow=False),
    _case("B70-every-size-L1-H4-misaligned-lam1", ALL_SIZES * 10, [0, 65, 1, 0, 0, 0, 0, 0, 0], 1, 4, misaligned=True, lam=1.0),
]


@functools.lru_cache(maxsize=None)
def _inputs(id):
    """The case's inputs on the host, drawn once: (ptr, batch, edge_index, dmax, csr, alphas, start, masks)."""
    c = next(c for c in CASES + EXTRA if c["id"] == id)
    ptr, batch, ei, dmax = RR.make_graphs(list(c["sizes"]), list(c["deg"]), seed=100 + c["seed"] + len(c["sizes"]))
    N, E, L, H = batch.numel(), ei.size(1), c["L"], c["H"]
    gen = torch.Generator().manual_seed(7 + c["seed"])
    alphas = [0.25 + 0.75 * torch.rand(E, H, generator=gen) for _ in range(L)]
    start = 0.25 + 0.75 * torch.rand(N, generator=gen)
    for g in c["zero_start"]:
        start[ptr[g]:ptr[g + 1]] = 0.0
    masks = [None] * L
    if c["masks"] != "none":
        for l in range(L):
            if c["masks"] == "some" and l % 2 == 0 and L > 1:
                continue                                                   # on some layers only
            masks[l] = torch.tensor([0.0, 0.5, 1.0, 1.0])[torch.randint(0, 4, (N,), generator=gen)]
        if c["masks"] == "zero_layer":
            masks = [None] * L
            masks[L // 2] = torch.zeros(N)
    for t in alphas + [start] + [m for m in masks if m is not None]:
        assert bool((t >= 0).all()) and t.dtype == torch.float32
    return ptr, batch, ei, dmax, RR.source_csr(ei, N), alphas, start, masks


@functools.lru_cache(maxsize=None)
def _reference(id, nmax=None, bad=False):
    c = next(c for c in CASES + EXTRA if c["id"] == id)
    ptr, batch, ei, dmax, (rowptr, eid, dst), alphas, start, masks = _inputs(id)
    if bad:
        eid, dst = _bad_slots(id)
    rel, flow = RR.rollout(ptr, rowptr, eid, dst, alphas, start, masks, c["lam"], nmax)
    for t in (rel[~torch.isnan(rel)], flow):                               # the tolerance's premise, asserted on the host
        assert bool(((t == 0) | (t >= 1e-30)).all()), "an exact non-zero output below 1e-30"
    return rel, flow


def _bad_slots(id):
    """The case's eid_s / dst_s with a few entries out of range: an edge id of -1 and of E, a destination of -5, of N + 2 and of
    a node in another graph."""
    ptr, batch, ei, dmax, (rowptr, eid, dst), *_ = _inputs(id)
    N, E = batch.numel(), ei.size(1)
    eid, dst = eid.clone(), dst.clone()
    eid[3], eid[E // 2] = -1, E
    dst[5], dst[E // 3] = -5, N + 2
    j = E - 2                                                              # a slot of the last graph, sent to node 0 of the first
    assert batch[ei[0][eid[j].long()]] != batch[0]
    dst[j] = 0
    return eid, dst


def _device_layers(alphas, pad, misaligned, dev):
    """Every alpha on the device with row stride H + pad, behind one float when `misaligned` (the base is then no multiple of 16
    bytes) -> (the views, the buffers that keep them alive)."""
    views, bufs = [], []
    for a in alphas:
        E, H = a.shape
        buf = torch.full((E * (H + pad) + 4,), 1e30, dtype=torch.float32, device=dev)       # (padding that would show in a sum)
        off = 1 if misaligned else 0
        v = buf[off:off + E * (H + pad)].view(E, H + pad)[:, :H]
        v.copy_(a)
        assert (v.data_ptr() % 16 != 0) == bool(misaligned) or E == 0
        views.append(v)
        bufs.append(buf)
    return views, bufs


def raw_rollout(lib, dev, id, nmax=None, bad=False, want_flow=None, pad=None, misaligned=None, expect=0, args=None):
    """One call through the C ABI on buffers of the caller: relevance behind a sentinel fill, edge_flow zeros, GUARD sentinel
    words behind both -> (relevance [N], flow [L, E] or None) on the host.  Asserts the status and that no guard word was touched;
    with a status other than 0, that nothing at all was written."""
    c = next(c for c in CASES + EXTRA if c["id"] == id)
    ptr, batch, ei, dmax, (rowptr, eid, dst), alphas, start, masks = _inputs(id)
    if bad:
        eid, dst = _bad_slots(id)
    N, E, B, L, H = batch.numel(), ei.size(1), len(ptr) - 1, c["L"], c["H"]
    want_flow = c["flow"] if want_flow is None else want_flow
    views, keep = _device_layers(alphas, c["pad"] if pad is None else pad, c["misaligned"] if misaligned is None else misaligned, dev)
    d_masks = [None if m is None else m.to(dev) for m in masks]
    table = []
    for v, m in zip(views, d_masks):
        table += [v.data_ptr() if E else 0, v.stride(0) if E > 1 else H, 0 if m is None else m.data_ptr()]
    d_ptr, d_rowptr = torch.tensor(ptr, dtype=torch.int32, device=dev), rowptr.to(dev)
    d_eid, d_dst, d_start = eid.to(dev), dst.to(dev), start.to(dev)
    rel = torch.full((N + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    flow = torch.cat([torch.zeros(L * E, device=dev), torch.full((GUARD,), SENTINEL, device=dev)]) if want_flow else None
    bound = max(c["sizes"]) if nmax is None else nmax
    a = dict(L=L, H=H, lam=c["lam"], N=N, E=E, B=B, nmax=bound)
    if args:
        a.update(args)
        if "lda" in args:
            table[1::3] = [args["lda"]] * L
    arr = (ctypes.c_int64 * len(table))(*table)
    rc = lib.isg_attention_rollout(d_ptr.data_ptr(), d_rowptr.data_ptr(), d_eid.data_ptr() if E else None, d_dst.data_ptr() if E else None,
                                   ctypes.addressof(arr), a["L"], a["H"], a["lam"], d_start.data_ptr(), a["N"], a["E"], a["B"], a["nmax"],
                                   rel.data_ptr(), None if flow is None else flow.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert bool((rel[N:] == SENTINEL).all()), "relevance: a guard word was written"
    assert flow is None or bool((flow[L * E:] == SENTINEL).all()), "edge_flow: a guard word was written"
    if expect != 0:
        assert bool((rel == SENTINEL).all()) and (flow is None or bool((flow[:L * E] == 0).all())), "a refused call wrote something"
    del keep
    return rel[:N].cpu(), None if flow is None else flow[:L * E].view(L, E).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_close(got, ref, k, what):
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: the NaN rows differ"
    g, r = got.double()[~nan], ref[~nan]
    assert bool((g[r == 0] == 0).all()), f"{what}: an exact zero came out as {float(g[r == 0].abs().max()):.3e}"
    err = (g - r).abs()
    worst = float((err / r.clamp_min(1e-300)).max()) if r.numel() else 0.0
    print(f"[rollout] {what}: max relative error {worst:.3e} against the bound {2 * k * U:.3e} (k = {k})")
    assert bool((err <= 2 * k * U * r).all()), f"{what}: max relative error {worst:.3e} beyond 2 k u = {2 * k * U:.3e}"


@pytest.mark.parametrize("id", [c["id"] for c in CASES])
def test_rollout_equals_the_restatement_on_both_libraries_and_twice(dev, libs, id):
    c = next(c for c in CASES if c["id"] == id)
    ptr, batch, ei, dmax, *_ = _inputs(id)
    N = batch.numel()
    ref_rel, ref_flow = _reference(id)
    k = c["L"] * (c["H"] + dmax + 6)
    assert 2 * k * U < 1e-3
    first = None
    for name, lib in (("fast", libs[0]), ("fast again", libs[0]), ("strict", libs[1])):
        rel, flow = raw_rollout(lib, dev, id)
        if N == 0:
            assert rel.numel() == 0
            continue
        assert_close(rel, ref_rel, k, f"{id}, relevance ({name})")
        if c["flow"]:
            assert_close(flow, ref_flow, k, f"{id}, flow ({name})")
        else:
            assert flow is None
        if first is None:
            first = (rel, flow)
        else:
            assert torch.equal(_bits(rel), _bits(first[0])), f"{name}: relevance differs from the first call's bits"
            assert flow is None or torch.equal(_bits(flow), _bits(first[1])), f"{name}: flow differs from the first call's bits"
    if N and c["lam"] == 1.0:                                              # everything stays: the start, as bits
        assert torch.equal(first[0], _inputs(id)[6])
    if N and not c["flow"]:                                                # with and without edge_flow: the same relevance
        assert torch.equal(_bits(raw_rollout(libs[0], dev, id, want_flow=True)[0]), _bits(first[0]))


def test_the_vector_and_the_scalar_alpha_paths_give_equal_bits(dev, libs):
    """H = 4 on the same values: lda = 4 on an aligned base (one 16-byte load per row), the same behind one float (scalar), and
    lda = 7 (scalar)."""
    id = "B1-n130-every-degree-L8-H4-vector"
    for lib in libs:
        vec = raw_rollout(lib, dev, id, pad=0, misaligned=False)
        for pad, mis in ((0, True), (3, False), (3, True), (4, False)):
            other = raw_rollout(lib, dev, id, pad=pad, misaligned=mis)
            assert torch.equal(_bits(vec[0]), _bits(other[0])) and torch.equal(_bits(vec[1]), _bits(other[1])), (pad, mis)
    # and the kernel's order, restated in fp32 on the host: the bits are a function of the inputs alone
    c = next(c for c in CASES if c["id"] == id)
    ptr, batch, ei, dmax, (rowptr, eid, dst), alphas, start, masks = _inputs(id)
    rel32, flow32 = RR.rollout_fp32(ptr, rowptr, eid, dst, alphas, start, masks, c["lam"])
    assert torch.equal(_bits(vec[0]), _bits(rel32)) and torch.equal(_bits(vec[1]), _bits(flow32))


EXTRA = [_case("B3-bad-slots-and-a-graph-beyond-nmax", [65, 130, 64], [2, 1, 0, 3], 3, 4, masks="some", seed=1),
         _case("B70-bad-slots-and-graphs-beyond-nmax", ALL_SIZES * 10, [1, 2, 0], 2, 3, pad=3, seed=2)]


@pytest.mark.parametrize("id,nmax", [(EXTRA[0]["id"], 65), (EXTRA[1]["id"], 64)])
def test_bad_slots_are_skipped_and_a_graph_beyond_nmax_gets_nan(dev, libs, id, nmax):
    c = next(c for c in EXTRA if c["id"] == id)
    ptr, batch, ei, dmax, *_ = _inputs(id)
    ref_rel, ref_flow = _reference(id, nmax, True)
    whole_rel, _ = _reference(id)
    big = torch.tensor([ptr[g + 1] - ptr[g] > nmax for g in range(len(ptr) - 1)])
    assert bool(big.any()) and torch.equal(torch.isnan(ref_rel), big[batch]) and not torch.equal(torch.nan_to_num(ref_rel), whole_rel)
    k = c["L"] * (c["H"] + dmax + 6)
    first = None
    for name, lib in (("fast", libs[0]), ("fast again", libs[0]), ("strict", libs[1])):
        rel, flow = raw_rollout(lib, dev, id, nmax=nmax, bad=True)
        assert_close(rel, ref_rel, k, f"{id}, relevance ({name})")
        assert_close(flow, ref_flow, k, f"{id}, flow ({name})")          # a skipped slot's edge and a skipped graph's edges: exactly 0
        if first is not None:
            assert torch.equal(_bits(rel), _bits(first[0])) and torch.equal(_bits(flow), _bits(first[1])), name
        first = first or (rel, flow)


def test_refused_calls_write_nothing(dev, libs):
    id = "B3-n65-2-130-L1-H4-pad"
    for lib in libs:
        top = lib.isg_rollout_max_nodes()
        for args, status in (({"lam": 2.0}, -1), ({"lam": float("nan")}, -1), ({"L": 0}, -1), ({"H": 0}, -1), ({"lda": 3}, -1),
                             ({"N": -1}, -1), ({"L": 9}, -2), ({"nmax": top + 1}, -2), ({"E": (1 << 31) - 1024}, -2)):
            raw_rollout(lib, dev, id, expect=status, args=args)
        # B == 0: ISG_OK, and nothing is written either
        rel = torch.full((8,), SENTINEL, device=dev)
        assert lib.isg_attention_rollout(None, None, None, None, None, 1, 4, 0.5, None, 8, 0, 0, 4, rel.data_ptr(), None, None) == 0
        torch.cuda.synchronize()
        assert bool((rel == SENTINEL).all())


def test_ops_attention_rollout_on_a_plan_equals_the_raw_call(dev, libs):
    """The operator: the plan's own CSR by source is the restatement's (out-slots in edge-id order), strided alphas and [N, 1]
    masks pass, the counter counts, and the result is the raw call's, as bits."""
    from isubgvqa_amd import _lib, ops
    id = "B3-n64-0-65-L4-H4-misaligned-zero-layer"
    c = next(c for c in CASES if c["id"] == id)
    ptr, batch, ei, dmax, csr, alphas, start, masks = _inputs(id)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=len(ptr) - 1)
    for got, want in zip(plan.source_csr(), csr):
        assert torch.equal(got[:want.numel()].cpu(), want)
    views, keep = _device_layers(alphas, 4, False, dev)
    d_masks = [None if m is None else m.to(dev).view(-1, 1) for m in masks]
    ops.reset_counters()
    rel, flow = ops.attention_rollout(plan, views, start.to(dev).view(-1, 1), d_masks, residual=c["lam"], want_flow=True)
    rel2, none = ops.attention_rollout(plan, views, start.to(dev), d_masks, residual=c["lam"])
    assert ops.counters()["attention_rollout"] == 2 and none is None
    raw = raw_rollout(libs[0], dev, id)
    assert torch.equal(_bits(rel.cpu()), _bits(raw[0])) and torch.equal(_bits(flow.cpu()), _bits(raw[1]))
    assert torch.equal(_bits(rel2), _bits(rel))
    with pytest.raises(ValueError, match="residual"):
        ops.attention_rollout(plan, views, start.to(dev), None, residual=1.5)
    with pytest.raises(ValueError, match="masks"):
        ops.attention_rollout(plan, views, start.to(dev), d_masks[:2])
    with pytest.raises(ValueError, match=r"alphas\[1\]"):
        ops.attention_rollout(plan, [views[0], views[1][:, :3]], start.to(dev))
    with pytest.raises(_lib.IsgError, match="layers"):
        ops.attention_rollout(plan, views * 3, start.to(dev))
    with pytest.raises(_lib.IsgError, match="GPU"):
        ops.attention_rollout(plan, [v.cpu() for v in views], start.to(dev))
    ops.check_plans()
