"""isg_curve_keep_bits and isg_curve_sums on the GPU (include/ext/isg_curves.h) against the restatement of
tests/curves_restated.py -- on the product library and on its strict twin, with guard words behind every output and a second call
that must give the first one's bits.

The keep bits, ranks, level sizes, index and status are integers: they are held EXACTLY, there is no tolerance.
TOLERANCES of the sums (derived, not measured; u = 2^-24): an area against float64 within L u sum_j |w_j p_j| (an fma chain of L
steps over exact products); a double total against a float64 sum within R 2^-53 sum |x| over the column's terms; the column of
areas is held against the float64 sum of the device's own fp32 areas."""
import ctypes
import functools

import pytest
import torch

import curves_restated as CR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7
NODE_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 129]
FRACTIONS = (0.0, 1e-9, 0.1, 0.2, 0.3, 0.5, 1.0)
COUNTS = (0, 1, 5, 1000)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """{"fast": the product library, "strict": its strict twin}: every header of the table bound, so that ops runs on either."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_curves, _lib
    strict = _lib.bind(_lib.bind(ctypes.CDLL(ge.STRICT_LIB)), _ext_curves.SIGNATURES)
    assert strict.isg_curve_abi_version() == _ext_curves.ABI_VERSION
    return {"fast": _ext_curves.load(), "strict": strict}


def _scores(sizes, kind, seed):
    """fp32 [N] on the host for graphs of the given sizes."""
    gen = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    if kind == "equal":
        return torch.full((N,), 0.25)
    if kind == "pairs":                                  # every value twice or more: ties everywhere
        return torch.randint(0, 6, (N,), generator=gen).float() / 4 - 0.5
    a = torch.randn(N, generator=gen)
    if kind == "planted":                                # +-0, +-inf and NaNs in every graph that has room for them
        lo = 0
        plant = (0.0, -0.0, INF, -INF, NAN, NAN, INF, 0.0, -0.0)
        for n in sizes:
            pos = torch.randperm(n, generator=gen)[:len(plant)].tolist()
            for p, v in zip(pos, plant):
                a[lo + p] = v
            lo += n
    return a


def _ptr(sizes):
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    return ptr


def _guarded(n, dev, dtype=torch.int32):
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[:n]


def _keep_bits(lib, dev, a, ptr, graphs, *, fractions=None, counts=None, sides=3, W=1):
    """One call of the entry point on guarded buffers -> (status code, {name: host tensor}, guards intact?)."""
    N, G, R = a.numel(), len(ptr) - 1, len(graphs)
    S = len(CR.side_list(sides))
    vals = fractions if counts is None else counts
    L = len(vals)
    host = ((ctypes.c_float if counts is None else ctypes.c_int32) * max(L, 1))(*vals)
    Q = R * L * S
    a_d, ptr_d = a.to(dev), torch.tensor(ptr, dtype=torch.int32, device=dev)
    g_d = torch.tensor(graphs, dtype=torch.int32, device=dev)
    bufs = {"rank": _guarded(N, dev), "level_k": _guarded(Q, dev), "index": _guarded(Q, dev), "keep": _guarded(Q * W, dev),
            "status": _guarded(4, dev)}
    code = lib.isg_curve_keep_bits(a_d.data_ptr(), ptr_d.data_ptr(), g_d.data_ptr(), ctypes.addressof(host) if counts is None else None,
                                   None if counts is None else ctypes.addressof(host), N, G, R, L, sides, W,
                                   *(bufs[k][1].data_ptr() for k in ("rank", "level_k", "index", "keep", "status")), None)
    torch.cuda.synchronize()
    intact = all(bool((b[v.numel():] == SENTINEL).all()) for b, v in bufs.values())
    return code, {k: v.cpu().clone() for k, (b, v) in bufs.items()}, intact


def _check_keep_bits(lib, dev, a, ptr, graphs, W, **kw):
    code, got, intact = _keep_bits(lib, dev, a, ptr, graphs, W=W, **kw)
    assert code == 0 and intact
    rank, level_k, index, keep, status, sets = CR.keep_bits(a, ptr, graphs, W=W, **kw)
    assert got["status"].tolist() == status
    assert torch.equal(got["index"], index) and torch.equal(got["level_k"], level_k.view(-1))
    assert torch.equal(CR.as_words(got["keep"]).view(-1, W), keep)
    assert torch.equal(got["rank"], torch.where(rank >= 0, rank, torch.full_like(rank, SENTINEL)))       # unlisted nodes: unwritten
    code, again, intact = _keep_bits(lib, dev, a, ptr, graphs, W=W, **kw)
    assert code == 0 and intact and all(torch.equal(again[k], got[k]) for k in got)
    return got, sets


# sizes of the batch: every size of NODE_SIZES eight times over, an empty graph in front, in the middle and at the end
BATCH = [0] + NODE_SIZES * 4 + [0] + NODE_SIZES * 4 + [0]


@functools.lru_cache(maxsize=None)
def _listed(R):
    """R graphs of BATCH, out of order; beyond one entry also a listed empty graph and an entry outside the batch."""
    gen = torch.Generator().manual_seed(R)
    order = [g for g in torch.randperm(len(BATCH), generator=gen).tolist() if BATCH[g] > 0]
    if R == 1:
        return (order[0],)
    head = [order[0], len(BATCH), 0, -1] if R > 3 else [order[0], len(BATCH), 0]
    return tuple(head + order[1:R - len(head) + 1])


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("R,L,sides,kind", [(1, 1, 1, "planted"), (1, 3, 3, "pairs"), (3, 3, 2, "planted"), (3, 1, 3, "equal"),
                                            (3, 64, 1, "randn"), (70, 3, 3, "planted"), (70, 64, 3, "pairs"), (70, 1, 2, "randn")])
def test_keep_bits_are_exact(libs, dev, which, R, L, sides, kind):
    a = _scores(BATCH, kind, 11 + R + L)
    graphs = _listed(R)
    assert len(graphs) == R
    fractions = {1: (0.3,), 3: (0.0, 0.2, 1.0), 64: tuple(j / 63 for j in range(64))}[L]
    got, _ = _check_keep_bits(libs[which], dev, a, _ptr(BATCH), graphs, W=5, fractions=fractions, sides=sides)
    assert got["status"][1] == (1 if R > 1 else 0) and got["status"][0] == 0
    counts = {1: (5,), 3: (0, 1, 1000), 64: tuple(range(64))}[L]
    _check_keep_bits(libs[which], dev, a, _ptr(BATCH), graphs, W=5, counts=counts, sides=sides)


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_the_level_rule_and_the_counts_on_the_device(libs, dev, which):
    sizes = [5, 10, 20, 65]
    a = _scores(sizes, "randn", 3)
    got, _ = _check_keep_bits(libs[which], dev, a, _ptr(sizes), [0, 1, 2, 3], W=3, fractions=FRACTIONS, sides=3)
    keep_k = got["level_k"].view(4, len(FRACTIONS), 2)[:, :, 0].tolist()
    # ceil of ONE fp32 product: 0.1 * 10 = 1, 0.1 * 20 = 2, 0.2 * 5 = 1, 0.2 * 65 = 13, 0.3 * 10 = 3 (a double evaluation: one more)
    assert keep_k == [[1, 1, 1, 1, 2, 3, 5], [1, 1, 1, 2, 3, 5, 10], [1, 1, 2, 4, 6, 10, 20], [1, 1, 7, 13, 20, 33, 65]]
    remove_k = got["level_k"].view(4, len(FRACTIONS), 2)[:, :, 1].tolist()
    assert remove_k == [[0, 1, 1, 1, 2, 3, 4], [0, 1, 1, 2, 3, 5, 9], [0, 1, 2, 4, 6, 10, 19], [0, 1, 7, 13, 20, 33, 64]]
    for sides in (1, 2, 3):
        got, _ = _check_keep_bits(libs[which], dev, a, _ptr(sizes), [3, 0], W=3, counts=COUNTS, sides=sides)
    assert got["level_k"].view(2, 4, 2).tolist() == [[[1, 0], [1, 1], [5, 5], [65, 64]], [[1, 0], [1, 1], [5, 4], [5, 4]]]


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_a_graph_of_2048_nodes_and_a_graph_beyond_the_words(libs, dev, which):
    sizes = [3, 2048, 0, 7]
    a = _scores(sizes, "pairs", 5)
    a[3 + 100], a[3 + 2047], a[3] = NAN, INF, -0.0
    got, _ = _check_keep_bits(libs[which], dev, a, _ptr(sizes), [1, 3, 2], W=64, fractions=(0.0, 0.3, 1.0), sides=3)
    assert got["status"].tolist() == [0, 0, 18, 0] and sorted(got["rank"][3:3 + 2048].tolist()) == list(range(2048))
    # one graph larger than 32 W: the flag is set, the first 32 W nodes are ranked among themselves, the others take no part
    sizes = [40, 70, 64]
    a = _scores(sizes, "planted", 6)
    got, sets = _check_keep_bits(libs[which], dev, a, _ptr(sizes), [1, 0, 2], W=2, counts=(1, 64, 1000), sides=3)
    assert got["status"].tolist() == [1, 0, 18, 0] and sorted(got["rank"][40:104].tolist()) == list(range(64))
    assert got["rank"][104:110].tolist() == [SENTINEL] * 6 and got["level_k"].view(3, 3, 2)[0].tolist() == [[1, 1], [64, 63], [64, 63]]
    # ptr clamped to [0, N] and to non-decreasing: never an address beyond a
    # (graphs 0 and 2 of this broken ptr overlap: listed in separate calls, so that every rank word keeps its one writer)
    a = _scores([10], "randn", 7)
    _check_keep_bits(libs[which], dev, a, [-4, 7, 3, 99], [0, 1], W=1, counts=(2,), sides=3)
    _check_keep_bits(libs[which], dev, a, [-4, 7, 3, 99], [2, 1], W=1, counts=(2,), sides=3)


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_refusals_write_nothing(libs, dev, which):
    sizes = [5, 3]
    a = _scores(sizes, "randn", 1)
    for kw in (dict(fractions=(0.5, NAN)), dict(fractions=(-0.5,)), dict(counts=(1, -1)), dict(fractions=(0.5,), sides=0),
               dict(fractions=(0.5,), sides=4), dict(fractions=(0.5,), W=65), dict(fractions=tuple([0.5] * 65))):
        W = kw.pop("W", 1)
        code, got, intact = _keep_bits(libs[which], dev, a, _ptr(sizes), [0, 1], W=W, **kw)
        assert code in (-1, -2) and intact, kw
        assert all(bool((v == SENTINEL).all()) for v in got.values()), kw
    code, got, intact = _keep_bits(libs[which], dev, a, _ptr(sizes), [], fractions=(0.5,))
    assert code == 0 and intact and bool((got["status"] == SENTINEL).all()) and bool((got["rank"] == SENTINEL).all())
    code, got, intact = _keep_bits(libs[which], dev, a, _ptr(sizes), [0], fractions=())
    assert code == 0 and intact and bool((got["status"] == SENTINEL).all()) and bool((got["rank"] == SENTINEL).all())


def _dyadic_scores(sizes, seed):
    """Distinct multiples of 2^-8 in [0, 4) inside every graph: no ties, and shifted_attributions is exact on them."""
    gen = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(1024, generator=gen)[:n].float() / 256 for n in sizes])


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_ops_rows_equal_the_threshold_masks_and_feed_induced_instances(libs, dev, which):
    from isubgvqa_amd import _lib, explain, ops
    sizes = [0] + NODE_SIZES + [0, 5, 1]
    a = _dyadic_scores(sizes, 9)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    gen = torch.Generator().manual_seed(4)
    ptr = _ptr(sizes)
    src, dst = [], []
    for g, n in enumerate(sizes):                        # a few edges per graph, self loops among them, the graphs in order
        for _ in range(min(2 * n, 40)):
            s, d = torch.randint(0, n, (2,), generator=gen).tolist()
            src.append(ptr[g] + s)
            dst.append(ptr[g] + d)
    ei = torch.tensor([src, dst], dtype=torch.int64, device=dev)
    with _lib.using(libs[which]):
        plan = ops.GraphPlan.build(batch, ei, num_graphs=len(sizes))
        ops.reset_counters()
        counts = (1, 5, 40)
        bits = ops.curve_keep_bits(a.to(dev), plan, counts=counts).verify()
        assert ops.counters()["curve_keep_bits"] == 1 and (bits.L, bits.S, bits.R) == (3, 2, len(sizes) - 2)
        listed = [g for g, n in enumerate(sizes) if n > 0]
        assert bits.graphs.tolist() == listed and bits.keep.size(1) == ops.keep_words(129) == 5
        rank, level_k, index, keep, status, sets = CR.keep_bits(a, ptr, listed, counts=counts, sides=3, W=5)
        assert torch.equal(bits.rank.cpu(), rank) and torch.equal(bits.level_k.cpu(), level_k) and torch.equal(bits.index.cpu(), index)
        assert torch.equal(CR.as_words(bits.keep), keep) and bits.status.tolist() == status
        # tie-free dyadic scores: the keep row at count k is the threshold top-k mask's row, the remove row its complement
        shifted = explain.shifted_attributions(a.to(dev), batch, len(sizes)).view(-1, 1).contiguous()
        rows = bits.keep.view(bits.R, 3, 2, 5)
        for j, k in enumerate(counts):
            mask = ops.topk_threshold(shifted, k, plan=plan)
            want = ops.keep_bits_from_mask(mask, plan)[listed]
            assert torch.equal(rows[:, j, 0], want), k
            full_graph = torch.tensor([n <= k for n in sizes if n > 0]).to(dev)
            gone = ops.keep_bits_from_mask(mask, plan, complement=True)[listed]
            assert torch.equal(rows[:, j, 1][~full_graph], gone[~full_graph]), k         # (a graph of n <= k nodes keeps its last one)
        # the rows through ops.induced_instances: the node lists are the restatement's sets
        inst = ops.induced_instances(plan, ei, bits.index, bits.keep)
        inst.verify()
        iptr, node_src = inst.ptr.tolist(), inst.node_src.tolist()
        for q, members in enumerate(sets):
            assert node_src[iptr[q]:iptr[q + 1]] == [ptr[int(index[q])] + i for i in members], q
        # graphs= in the caller's order; each side alone; fractions
        some = torch.tensor([10, 3, 1])
        for sides, code in (("keep", 1), (("remove",), 2)):
            b2 = ops.curve_keep_bits(a.to(dev), plan, graphs=some, fractions=(0.0, 0.5), sides=sides).verify()
            want = CR.keep_bits(a, ptr, some.tolist(), fractions=(0.0, 0.5), sides=code, W=5)
            assert torch.equal(CR.as_words(b2.keep), want[3]) and torch.equal(b2.level_k.cpu(), want[1]) and b2.S == 1
            assert torch.equal(b2.rank.cpu(), want[0])                                     # unlisted graphs: -1
        with pytest.raises(ValueError, match="exactly one"):
            ops.curve_keep_bits(a.to(dev), plan)
        with pytest.raises(ValueError, match="fractions"):
            ops.curve_keep_bits(a.to(dev), plan, fractions=(0.1, NAN))


def _sums(lib, dev, p, w, R, L, S, totals0):
    p_d, w_d = p.to(dev), torch.tensor(w, dtype=torch.float32, device=dev)
    auc_b, auc = _guarded(R * S, dev, torch.float32)
    tot_b, tot = _guarded(S * (L + 3), dev, torch.float64)
    tot.copy_(totals0.view(-1))
    code = lib.isg_curve_sums(p_d.data_ptr(), w_d.data_ptr(), R, L, 3 if S == 2 else 1, auc.data_ptr(), tot.data_ptr(), None)
    torch.cuda.synchronize()
    intact = bool((auc_b[R * S:] == SENTINEL).all()) and bool((tot_b[S * (L + 3):] == SENTINEL).all())
    return code, auc.cpu().view(R, S).clone(), tot.cpu().view(S, L + 3).clone(), intact


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("R,L,S", [(1, 1, 1), (3, 7, 2), (70, 64, 2), (256, 7, 2), (70, 3, 1)])
def test_sums_against_float64(libs, dev, which, R, L, S):
    from isubgvqa_amd import explain
    gen = torch.Generator().manual_seed(R + L + S)
    p = torch.rand(R * L * S, generator=gen)
    w = explain.curve_weights([j / max(L - 1, 1) for j in range(L)]).float().tolist()
    planted = R >= 3
    if planted:                                          # an inf in graph 1's keep side, a NaN in the last graph's last side
        p.view(R, L, S)[1, L // 2, 0] = INF
        p.view(R, L, S)[R - 1, L - 1, S - 1] = NAN
    zero = torch.zeros(S, L + 3, dtype=torch.float64)
    code, auc, tot, intact = _sums(libs[which], dev, p, w, R, L, S, zero)
    assert code == 0 and intact
    want_auc, auc_bound, want_tot, tot_bound = CR.sums(p, w, R, L, S)
    skipped = torch.isnan(want_auc)
    assert torch.equal(torch.isnan(auc), skipped) and int(skipped.sum()) == (2 if planted else 0)
    err = torch.where(skipped, torch.zeros_like(want_auc), (auc.double() - want_auc).abs())
    assert bool((err <= auc_bound).all()), float((err / auc_bound.clamp_min(1e-300)).max())
    assert bool(((tot[:, :L] - want_tot[:, :L]).abs() <= tot_bound[:, :L]).all())
    own = torch.where(skipped, torch.zeros_like(want_auc), auc.double())                   # the device's own fp32 areas, summed in float64
    assert bool(((tot[:, L] - own.sum(dim=0)).abs() <= R * 2.0 ** -53 * own.abs().sum(dim=0)).all())
    assert bool(((tot[:, L] - want_tot[:, L]).abs() <= tot_bound[:, L]).all())
    assert torch.equal(tot[:, L + 1:], want_tot[:, L + 1:]) and float(tot[:, L + 1:].sum()) == R * S
    # a second call gives the first one's bits; a call on the first one's totals accumulates
    code, auc2, tot2, intact = _sums(libs[which], dev, p, w, R, L, S, zero)
    assert code == 0 and intact and torch.equal(tot2, tot) and torch.equal(auc2.view(torch.int32), auc.view(torch.int32))
    code, _, tot3, intact = _sums(libs[which], dev, p, w, R, L, S, tot)
    assert code == 0 and intact
    assert bool(((tot3[:, :L + 1] - 2 * want_tot[:, :L + 1]).abs() <= 2 * tot_bound[:, :L + 1] + 2.0 ** -52 * want_tot[:, :L + 1].abs()).all())
    assert torch.equal(tot3[:, L + 1:], 2 * want_tot[:, L + 1:])


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_ops_curve_sums_and_its_refusals(libs, dev, which):
    from isubgvqa_amd import _lib, ops
    with _lib.using(libs[which]):
        plan = ops.GraphPlan.build(torch.tensor([0, 0, 0]).to(dev), torch.zeros(2, 0, dtype=torch.int64, device=dev), num_graphs=1)
        bits = ops.curve_keep_bits(torch.tensor([0.5, 2.0, 2.0]).to(dev), plan, counts=(1, 2)).verify()
        assert bits.rank.tolist() == [2, 0, 1] and bits.keep.tolist() == [[0b010], [0b101], [0b110], [0b001]]
        assert bits.level_k.tolist() == [[[1, 1], [2, 2]]] and bits.index.tolist() == [0, 0, 0, 0]
        ops.reset_counters()
        p = torch.tensor([0.5, 0.25, 0.75, 0.125]).to(dev)
        auc, totals = ops.curve_sums(p, bits, torch.tensor([0.5, 0.5]).to(dev))
        assert auc.tolist() == [[0.625, 0.1875]] and totals.tolist() == [[0.5, 0.75, 0.625, 1.0, 0.0], [0.25, 0.125, 0.1875, 1.0, 0.0]]
        _, again = ops.curve_sums(p, bits, torch.tensor([0.5, 0.5]).to(dev), totals)
        assert again is totals and totals.tolist() == [[1.0, 1.5, 1.25, 2.0, 0.0], [0.5, 0.25, 0.375, 2.0, 0.0]]
        assert ops.counters()["curve_sums"] == 2
        with pytest.raises(ValueError, match="shape"):
            ops.curve_sums(p[:3].contiguous(), bits, torch.tensor([0.5, 0.5]).to(dev))
        with pytest.raises(TypeError):
            ops.curve_sums(p, bits, torch.tensor([0.5, 0.5], dtype=torch.float64).to(dev))
        # no graph listed: nothing is launched into
        none = ops.curve_keep_bits(torch.tensor([0.5, 2.0, 2.0]).to(dev), plan, graphs=torch.zeros(0, dtype=torch.int64),
                                   fractions=(0.0, 1.0)).verify()
        assert none.R == 0 and none.keep.shape == (0, 1) and none.status.tolist() == [0, 0, 0, 0] and none.rank.tolist() == [-1] * 3
        auc, totals = ops.curve_sums(torch.zeros(0, device=dev), none, torch.tensor([0.5, 0.5]).to(dev))
        assert auc.shape == (0, 2) and float(totals.abs().sum()) == 0.0
