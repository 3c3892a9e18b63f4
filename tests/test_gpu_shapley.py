"""isg_shapley_keep_bits and isg_shapley_values on the GPU (include/ext/isg_shapley.h) against the restatement of
tests/shapley_restated.py -- on the product library and on its strict twin, with guard words behind every output and a second
call that must give the first one's bits.

The positions, keep bits, index and status are integers: they are held EXACTLY, there is no tolerance.  phi is held EXACTLY
against the restatement in fp32 operations in the header's order (sub, add, multiply by 0.5 and one division are IEEE single on
the CPU too), and so is the gap, whose order the header states.
TOLERANCES (derived, not measured; u = 2^-24):
phi against the estimator in float64 within (T + 3) u (sum_t |e_t|) / T: T - 1 additions of the recursive sum (Higham, Accuracy
and Stability, 4.2), one division, and per sample one subtraction, one pair addition and one (exact) halving;
m2 within T u sum_t e_t^2 of the float64 sum of the squares of the estimator's samples e_t -- the fp32 numbers the header
defines; their squares are exact in float64 -- an fma chain of T steps, each rounded once (Higham 3.1);
gap within (n + 1) u (sum_i |phi_i| + |p - v_empty|) of the float64 sum of the device's own phi: n - 1 additions, one subtraction
for p - v_empty, one for the gap."""
import ctypes
import functools

import pytest
import torch

import shapley_restated as SR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7
NODE_SIZES = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 129]
BATCH = NODE_SIZES * 7                                   # 77 graphs, every size seven times
SEEDS = (0x5EED, (1 << 40) + 3)                          # one of them beyond 2^32: both key words are used
NAN, INF = float("nan"), float("inf")
U = SR.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """{"fast": the product library, "strict": its strict twin}: every header of the table bound, so that ops runs on either."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_induced, _ext_shapley, _lib
    strict = _lib.bind(_lib.bind(_lib.bind(ctypes.CDLL(ge.STRICT_LIB)), _ext_shapley.SIGNATURES), _ext_induced.SIGNATURES)
    assert strict.isg_shapley_abi_version() == _ext_shapley.ABI_VERSION
    return {"fast": _ext_shapley.load(), "strict": strict}


def _ptr(sizes):
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    return ptr


def _guarded(n, dev, dtype=torch.int32):
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[:n]


def _i32(v, dev):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def _keep_bits(lib, dev, ptr, graphs, row_ptr, N, M, Q, antithetic, seed, W):
    """One call of the entry point on guarded buffers -> (status code, {name: host tensor}, guards intact?)."""
    G, R = len(ptr) - 1, len(graphs)
    ptr_d, g_d, rp_d = _i32(ptr, dev), _i32(graphs, dev), _i32(row_ptr, dev)
    bufs = {"pos": _guarded(M * N, dev), "index": _guarded(Q, dev), "keep": _guarded(Q * W, dev), "status": _guarded(4, dev)}
    code = lib.isg_shapley_keep_bits(ptr_d.data_ptr(), g_d.data_ptr(), rp_d.data_ptr(), N, G, R, M, Q, int(antithetic), seed, W,
                                     *(bufs[k][1].data_ptr() for k in ("pos", "index", "keep", "status")), None)
    torch.cuda.synchronize()
    intact = all(bool((b[v.numel():] == SENTINEL).all()) for b, v in bufs.values())
    return code, {k: v.cpu().clone() for k, (b, v) in bufs.items()}, intact


@functools.lru_cache(maxsize=None)
def _restated_bits(ptr, graphs, row_ptr, N, M, Q, antithetic, seed, W, want_sets=False):
    """The restatement, computed once and shared by the product library's and the strict twin's test."""
    return SR.keep_bits(list(ptr), list(graphs), list(row_ptr), N, M, Q, antithetic, seed, W, sentinel=SENTINEL, want_sets=want_sets)


def _check_keep_bits(lib, dev, ptr, graphs, N, M, antithetic, seed, W, row_ptr=None, Q=None, want_sets=False):
    if row_ptr is None:
        row_ptr = SR.row_ptr_of(ptr, graphs, N, M, W)
    Q = row_ptr[-1] if Q is None else Q
    code, got, intact = _keep_bits(lib, dev, ptr, graphs, row_ptr, N, M, Q, antithetic, seed, W)
    assert code == 0 and intact
    pos, index, keep, status, sets, written = _restated_bits(tuple(ptr), tuple(graphs), tuple(row_ptr), N, M, Q, antithetic, seed, W,
                                                             want_sets)
    assert got["status"].tolist() == status
    assert torch.equal(got["pos"].view(M, N), pos)                                                     # unlisted nodes: unwritten
    assert torch.equal(got["index"], index)                                                            # unwritten rows: sentinels
    assert torch.equal(SR.as_words(got["keep"]).view(Q, W), keep & 0xFFFFFFFF)
    code, again, intact = _keep_bits(lib, dev, ptr, graphs, row_ptr, N, M, Q, antithetic, seed, W)
    assert code == 0 and intact and all(torch.equal(again[k], got[k]) for k in got)
    return got, (pos, index, keep, status, sets, written), row_ptr


@functools.lru_cache(maxsize=None)
def _listed(R):
    """R graphs of BATCH, out of order; beyond one entry also entries outside the batch and a graph listed twice."""
    gen = torch.Generator().manual_seed(R)
    order = torch.randperm(len(BATCH), generator=gen).tolist()
    if R == 1:
        return (BATCH.index(129),)
    head = [order[0], len(BATCH), order[0]] + ([-1] if R > 3 else [])
    return tuple(head[:R] + order[1:R - len(head) + 1])


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("R,M,antithetic,seed", [(1, 1, False, SEEDS[0]), (1, 16, True, SEEDS[1]), (3, 2, True, SEEDS[1]),
                                                 (3, 16, False, SEEDS[0]), (70, 2, False, SEEDS[1]), (70, 16, True, SEEDS[0])])
def test_keep_bits_are_exact(libs, dev, which, R, M, antithetic, seed):
    graphs = _listed(R)
    assert len(graphs) == R
    ptr = _ptr(BATCH)
    got, (pos, _, _, status, _, written), row_ptr = _check_keep_bits(libs[which], dev, ptr, graphs, ptr[-1], M, antithetic, seed, 5)
    assert status[:3] == [0, 1 if R > 1 else 0, 0] and status[3] == row_ptr[-1] and bool(written.all())
    for r, g in enumerate(graphs):                       # every listed graph's rows of pos are permutations of its nodes
        if 0 <= g < len(BATCH) and BATCH[g]:
            assert torch.equal(got["pos"].view(M, -1)[:, ptr[g]:ptr[g + 1]].sort(dim=1).values, torch.arange(BATCH[g], dtype=torch.int32).expand(M, -1))
    if R == 70 and M == 16:                              # the same graph alone: its permutations do not depend on the listing
        g = graphs[5]
        alone, _, _ = _check_keep_bits(libs[which], dev, ptr, (g,), ptr[-1], M, antithetic, seed, 5)
        assert torch.equal(alone["pos"].view(M, -1)[:, ptr[g]:ptr[g + 1]], got["pos"].view(M, -1)[:, ptr[g]:ptr[g + 1]])
        assert torch.equal(alone["keep"].view(-1, 5), got["keep"].view(-1, 5)[row_ptr[5]:row_ptr[6]])


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("antithetic", [True, False])
def test_the_largest_number_of_permutations_on_a_few_small_graphs(libs, dev, which, antithetic):
    sizes = [3, 5, 0, 2, 1, 9]
    got, _, row_ptr = _check_keep_bits(libs[which], dev, _ptr(sizes), (5, 0, 3, 1, 2, 4), 20, 1024, antithetic, SEEDS[1], 1)
    assert row_ptr[-1] == 1024 * (8 + 2 + 1 + 4) and got["status"].tolist() == [0, 0, 0, row_ptr[-1]]
    pos = got["pos"].view(1024, 20)[:, :3]                # graph 0: all 6 orders of 3 nodes occur among 1024 permutations
    assert len(set(map(tuple, pos.tolist()))) == 6
    if antithetic:
        last = torch.repeat_interleave(torch.tensor(sizes, dtype=torch.int32) - 1, torch.tensor(sizes))
        assert torch.equal(got["pos"].view(1024, 20)[1::2], last - got["pos"].view(1024, 20)[0::2])          # n - 1 - pos, graph by graph


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_a_graph_of_2048_nodes_a_graph_beyond_the_words_and_a_broken_ptr(libs, dev, which):
    sizes = [3, 2048, 0, 7]
    got, _, row_ptr = _check_keep_bits(libs[which], dev, _ptr(sizes), (1, 3, 2), 2058, 2, True, SEEDS[0], 64)
    assert got["status"].tolist() == [0, 0, 0, 2 * 2047 + 2 * 6] and sorted(got["pos"][3:3 + 2048].tolist()) == list(range(2048))
    # one graph larger than 32 W: the flag is set, the first 32 W nodes are permuted among themselves, the others take no part
    sizes = [40, 70, 64]
    got, _, row_ptr = _check_keep_bits(libs[which], dev, _ptr(sizes), (1, 0, 2), 174, 2, False, SEEDS[1], 2)
    assert got["status"].tolist() == [1, 0, 0, 2 * (63 + 39 + 63)] and sorted(got["pos"][40:104].tolist()) == list(range(64))
    assert got["pos"][104:110].tolist() == [SENTINEL] * 6
    # ptr clamped to [0, N] and to non-decreasing: never an address beyond pos
    # (graphs 0 and 2 of this broken ptr overlap: listed in separate calls, so that every pos word keeps its one writer)
    _check_keep_bits(libs[which], dev, [-4, 7, 3, 99], (0, 1), 10, 4, True, SEEDS[0], 1)
    _check_keep_bits(libs[which], dev, [-4, 7, 3, 99], (2, 1), 10, 4, True, SEEDS[0], 1)


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_a_row_ptr_that_is_short_negative_or_inconsistent(libs, dev, which):
    sizes = [3, 0, 33, 1, 7]
    ptr, N, M, W = _ptr(sizes), 44, 4, 2
    # short: graph 4's rows would end behind Q -- it writes no rows and no pos; the rows of graph 0 stand
    got, (_, _, _, status, _, written), _ = _check_keep_bits(libs[which], dev, ptr, (0, 4), N, M, True, SEEDS[0], W, row_ptr=[0, 8, 32], Q=31)
    assert status == [0, 0, 1, 31] and bool((got["index"][8:] == SENTINEL).all()) and bool((got["keep"][8 * W:] == SENTINEL).all())
    assert bool((got["pos"].view(M, N)[:, 37:] == SENTINEL).all()) and bool(written[:8].all())
    # negative: graph 0 writes nothing, graph 4 does
    got, (_, _, _, status, _, _), _ = _check_keep_bits(libs[which], dev, ptr, (0, 4), N, M, True, SEEDS[0], W, row_ptr=[-1, 7, 31], Q=31)
    assert status == [0, 0, 1, 31] and bool((got["index"][:7] == SENTINEL).all()) and bool((got["pos"].view(M, N)[:, :3] == SENTINEL).all())
    assert got["index"][7:].tolist() == [4] * 24
    # inconsistent but inside Q: the flag alone; a gap between the graphs' rows stays unwritten
    got, (_, _, _, status, _, _), _ = _check_keep_bits(libs[which], dev, ptr, (0, 4), N, M, False, SEEDS[1], W, row_ptr=[0, 9, 33], Q=40)
    assert status == [0, 0, 1, 40] and got["index"].tolist() == [0] * 8 + [SENTINEL] + [4] * 24 + [SENTINEL] * 7
    # an entry outside the batch between two graphs: no rows, never an address
    got, (_, _, _, status, _, _), _ = _check_keep_bits(libs[which], dev, ptr, (0, 1 << 30, -(1 << 31), 4), N, M, True, SEEDS[0], W)
    assert status == [0, 1, 0, 32]


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_refusals_write_nothing(libs, dev, which):
    sizes = [5, 3]
    for kw in (dict(M=3), dict(M=0), dict(M=1026), dict(antithetic=2), dict(W=65), dict(W=0)):
        args = dict(M=4, antithetic=1, W=1)
        args.update(kw)
        code, got, intact = _keep_bits(libs[which], dev, _ptr(sizes), (0, 1), [0, 16, 24], 8, args["M"], 24, args["antithetic"], 5, args["W"])
        assert code in (-1, -2) and intact, kw
        assert all(bool((v == SENTINEL).all()) for v in got.values()), kw
    code, got, intact = _keep_bits(libs[which], dev, _ptr(sizes), (), [0], 8, 4, 0, True, 5, 1)
    assert code == 0 and intact and bool((got["status"] == SENTINEL).all()) and bool((got["pos"] == SENTINEL).all())


def _edges(sizes, gen, dev):
    ptr = _ptr(sizes)
    src, dst = [], []
    for g, n in enumerate(sizes):                        # a few edges per graph, self loops among them, the graphs in order
        for _ in range(min(2 * n, 40)):
            s, d = torch.randint(0, n, (2,), generator=gen).tolist()
            src.append(ptr[g] + s)
            dst.append(ptr[g] + d)
    return torch.tensor([src, dst], dtype=torch.int64, device=dev)


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_ops_rows_feed_induced_instances(libs, dev, which):
    from isubgvqa_amd import _lib, ops
    sizes = [0, 1, 2, 3, 33, 65, 0, 5]
    ptr, N = _ptr(sizes), sum(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)
    ei = _edges(sizes, torch.Generator().manual_seed(4), dev)
    with _lib.using(libs[which]):
        plan = ops.GraphPlan.build(batch, ei, num_graphs=len(sizes))
        ops.reset_counters()
        bits = ops.shapley_keep_bits(plan, permutations=4, seed=SEEDS[1]).verify()
        assert ops.counters()["shapley_keep_bits"] == 1 and (bits.M, bits.T, bits.R, bits.antithetic) == (4, 2, len(sizes), True)
        assert bits.graphs.tolist() == list(range(len(sizes))) and bits.keep.size(1) == ops.keep_words(65) == 3
        graphs = tuple(range(len(sizes)))
        row_ptr = SR.row_ptr_of(ptr, graphs, N, 4, 3)
        assert bits.row_ptr.tolist() == row_ptr and bits.Q == row_ptr[-1] == 4 * (1 + 2 + 32 + 64 + 4)
        pos, index, keep, status, sets, _ = _restated_bits(tuple(ptr), graphs, tuple(row_ptr), N, 4, row_ptr[-1], True, SEEDS[1], 3, True)
        assert torch.equal(bits.pos.cpu(), torch.where(pos == SENTINEL, torch.full_like(pos, -1), pos))
        assert torch.equal(bits.index.cpu(), index) and torch.equal(SR.as_words(bits.keep), keep) and bits.status.tolist() == status
        # the rows through ops.induced_instances: the node lists are the restatement's prefixes
        inst = ops.induced_instances(plan, ei, bits.index, bits.keep)
        inst.verify()
        iptr, node_src = inst.ptr.tolist(), inst.node_src.tolist()
        for q in range(bits.Q):
            assert node_src[iptr[q]:iptr[q + 1]] == [ptr[int(index[q])] + i for i in sets[q]], q
        # graphs= in the caller's order; without antithetic; a graph's permutations are those it has in the whole listing
        some = torch.tensor([5, 3, 1])
        b2 = ops.shapley_keep_bits(plan, graphs=some, permutations=3, antithetic=False, seed=SEEDS[1]).verify()
        rp2 = SR.row_ptr_of(ptr, some.tolist(), N, 3, 3)
        want = SR.keep_bits(ptr, some.tolist(), rp2, N, 3, rp2[-1], False, SEEDS[1], 3, want_sets=False)
        assert torch.equal(b2.pos.cpu(), want[0]) and torch.equal(SR.as_words(b2.keep), want[2]) and b2.row_ptr.tolist() == rp2
        assert torch.equal(b2.pos[0].cpu()[ptr[5]:ptr[6]], bits.pos[0].cpu()[ptr[5]:ptr[6]])
        none = ops.shapley_keep_bits(plan, graphs=torch.zeros(0, dtype=torch.int64), permutations=2).verify()
        assert none.R == 0 and none.Q == 0 and none.status.tolist() == [0, 0, 0, 0] and bool((none.pos == -1).all())
        with pytest.raises(_lib.IsgError, match="status"):
            ops.shapley_keep_bits(plan, graphs=torch.tensor([2, 99]), permutations=2).verify()


# ---------------------------------------------------------------------------------------------------------------------
# the values
# ---------------------------------------------------------------------------------------------------------------------
def _values(lib, dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, antithetic, v_empty, W, want_m2=True):
    G, R = len(ptr) - 1, len(graphs)
    pi_d, p_d, pos_d = p_inst.float().to(dev), p.float().to(dev), pos.int().contiguous().to(dev)
    ptr_d, g_d, rp_d = _i32(ptr, dev), _i32(graphs, dev), _i32(row_ptr, dev)
    bufs = {"phi": _guarded(N, dev, torch.float32), "m2": _guarded(N, dev, torch.float32), "gap": _guarded(R, dev, torch.float32),
            "flag": _guarded(R, dev)}
    code = lib.isg_shapley_values(pi_d.data_ptr(), p_d.data_ptr(), pos_d.data_ptr(), ptr_d.data_ptr(), g_d.data_ptr(), rp_d.data_ptr(),
                                  N, G, R, M, Q, int(antithetic), v_empty, W, bufs["phi"][1].data_ptr(),
                                  bufs["m2"][1].data_ptr() if want_m2 else None, bufs["gap"][1].data_ptr(), bufs["flag"][1].data_ptr(), None)
    torch.cuda.synchronize()
    intact = all(bool((b[v.numel():] == SENTINEL).all()) for b, v in bufs.values())
    return code, {k: v.cpu().clone() for k, (b, v) in bufs.items()}, intact


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_values(lib, dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, antithetic, v_empty, W, want_m2=True):
    """The device against the fp32-order restatement (phi, gap and flag EXACT) and against float64 within the derived bounds."""
    code, got, intact = _values(lib, dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, antithetic, v_empty, W, want_m2)
    assert code == 0 and intact
    args = (p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, antithetic, v_empty, W)
    phi32, m32, gap32, flag32, _, sq_e = SR.values(*args, dtype=torch.float32, sentinel=float(SENTINEL))
    phi64, _, gap64, flag64, abs_e, _ = SR.values(*args, dtype=torch.float64, sentinel=float(SENTINEL))
    T = SR.draws(M, antithetic)
    assert torch.equal(got["flag"], flag32) and torch.equal(flag32, flag64)
    assert _same_bits(got["phi"], phi32), float((got["phi"] - phi32).abs().max())
    written = (phi64 != SENTINEL) & ~torch.isnan(phi64)
    err = torch.where(written, (got["phi"].double() - phi64).abs(), torch.zeros_like(phi64))
    bound = (T + 3) * U * abs_e / T
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    if want_m2:
        assert torch.equal(torch.isnan(got["m2"]), torch.isnan(m32)) and torch.equal(got["m2"] == SENTINEL, m32 == SENTINEL)
        err = torch.where(written, (got["m2"].double() - sq_e).abs(), torch.zeros_like(sq_e))      # sq_e: float64 over the fp32 samples
        assert bool((err <= T * U * sq_e).all()), float((err / (T * U * sq_e).clamp_min(1e-300)).max())
    else:
        assert bool((got["m2"] == SENTINEL).all())
    assert torch.equal(torch.isnan(got["gap"]), torch.isnan(gap32)) and torch.equal(torch.isnan(gap32), torch.isnan(gap64))
    G = len(ptr) - 1
    ve = float(torch.tensor(v_empty, dtype=torch.float32))
    for r, g in enumerate(graphs):
        if int(flag32[r]) == 0:
            lo, n, _ = SR.graph_range(ptr, g, N, W)
            own = got["phi"][lo:lo + n].double()
            if n == 0:
                assert float(got["gap"][r]) == 0.0 and not torch.signbit(got["gap"][r])
                continue
            full = float(p[g].float().double()) - ve
            want = float(own.sum()) - full
            assert abs(float(got["gap"][r]) - want) <= (n + 1) * U * (float(own.abs().sum()) + abs(full)), (r, g)
    mask = ~torch.isnan(gap32)
    assert _same_bits(got["gap"][mask], gap32[mask])
    code, again, intact = _values(lib, dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, antithetic, v_empty, W, want_m2)
    assert code == 0 and intact and all(_same_bits(again[k], got[k]) for k in got)
    return got


@functools.lru_cache(maxsize=None)
def _value_case(sizes, graphs, M, antithetic, seed, W):
    """Permutations by the restatement and seeded probabilities for a batch -> (ptr, row_ptr, N, Q, pos, p_inst, p)."""
    ptr = _ptr(sizes)
    N = ptr[-1]
    row_ptr = SR.row_ptr_of(ptr, graphs, N, M, W)
    Q = row_ptr[-1]
    pos = SR.keep_bits(ptr, list(graphs), row_ptr, N, M, Q, antithetic, seed, W, sentinel=SENTINEL, want_sets=False)[0]
    gen = torch.Generator().manual_seed(seed & 0xFFFF)
    return ptr, row_ptr, N, Q, pos, torch.rand(Q, generator=gen), torch.rand(len(sizes), generator=gen)


VALUE_SIZES = (0, 1, 2, 3, 31, 33, 64, 65, 129)
VALUE_GRAPHS = (8, 2, 9, 0, 7, 1, -1, 3, 6, 5, 4)        # out of order, two entries outside the batch


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("M,antithetic,v_empty,want_m2", [(1, False, 0.0, True), (2, True, 0.0, True), (16, True, 0.0, False),
                                                          (16, False, 0.0625, True), (6, True, -0.3, True)])
def test_values_are_the_estimator_in_the_stated_order(libs, dev, which, M, antithetic, v_empty, want_m2):
    ptr, row_ptr, N, Q, pos, p_inst, p = _value_case(VALUE_SIZES, VALUE_GRAPHS, M, antithetic, SEEDS[0], 5)
    got = _check_values(libs[which], dev, p_inst, p, pos, ptr, VALUE_GRAPHS, row_ptr, N, M, Q, antithetic, v_empty, 5, want_m2)
    assert got["flag"].tolist() == [0, 0, 2, 0, 0, 0, 2, 0, 0, 0, 0]
    # n = 1: the lone node gets p - v_empty: T equal samples d, whose recursive sum is exact up to 2 d (3 d may round), so the
    # mean is d itself for T <= 2 and within the bound of _check_values beyond
    d = p[1] - torch.tensor(v_empty, dtype=torch.float32)
    T = SR.draws(M, antithetic)
    assert abs(float(got["phi"][0]) - float(d)) <= (0.0 if T <= 2 else (T + 3) * U * abs(float(d)))
    # a pos outside [0, n - 1] is clamped before it forms a row number: the call reads no row of another graph and nothing beyond p_inst
    wild = pos.clone()
    wild[wild != SENTINEL] = torch.where(torch.arange(int((wild != SENTINEL).sum())) % 2 == 0, torch.tensor(1 << 30), torch.tensor(-(1 << 31))).int()
    _check_values(libs[which], dev, p_inst, p, wild, ptr, VALUE_GRAPHS, row_ptr, N, M, Q, antithetic, v_empty, 5, want_m2)


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_values_with_the_largest_number_of_permutations_and_a_graph_of_2048_nodes(libs, dev, which):
    ptr, row_ptr, N, Q, pos, p_inst, p = _value_case((3, 5, 0, 2, 1, 9), (5, 0, 3, 1, 2, 4), 1024, True, SEEDS[1], 1)
    _check_values(libs[which], dev, p_inst, p, pos, ptr, (5, 0, 3, 1, 2, 4), row_ptr, N, 1024, Q, True, 0.0, 1)
    ptr, row_ptr, N, Q, pos, p_inst, p = _value_case((3, 2048, 0, 7), (1, 3, 2), 2, True, SEEDS[0], 64)
    _check_values(libs[which], dev, p_inst, p, pos, ptr, (1, 3, 2), row_ptr, N, 2, Q, True, 0.0, 64)
    # a graph beyond 32 W nodes: phi for its first 32 W nodes only
    ptr, row_ptr, N, Q, pos, p_inst, p = _value_case((40, 70, 64), (1, 0, 2), 2, False, SEEDS[1], 2)
    got = _check_values(libs[which], dev, p_inst, p, pos, ptr, (1, 0, 2), row_ptr, N, 2, Q, False, 0.0, 2)
    assert bool((got["phi"][104:110] == SENTINEL).all()) and bool((got["phi"][40:104] != SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _game_case(sizes, M, antithetic, seed):
    """A batch for the games: (ptr, graphs, row_ptr, N, Q, pos, index, sets)."""
    ptr, graphs = _ptr(sizes), tuple(range(len(sizes)))
    N = ptr[-1]
    row_ptr = SR.row_ptr_of(ptr, graphs, N, M, 1)
    pos, index, _, _, sets, _ = SR.keep_bits(ptr, list(graphs), row_ptr, N, M, row_ptr[-1], antithetic, seed, 1, sentinel=SENTINEL)
    return ptr, graphs, row_ptr, N, row_ptr[-1], pos, index, sets


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("M,antithetic", [(1, False), (2, True), (6, True), (6, False), (16, True)])
def test_games_whose_shapley_values_are_known_without_sampling_error(libs, dev, which, M, antithetic):
    sizes = (5, 1, 0, 3, 8, 16, 2, 4)
    ptr, graphs, row_ptr, N, Q, pos, index, sets = _game_case(sizes, M, antithetic, SEEDS[0])
    T = SR.draws(M, antithetic)
    # additive, with dummies: v(S) = sum_{i in S} c_i, c dyadic (multiples of 2^-6 below 1, every fourth node 0): phi_i = c_i EXACTLY
    gen = torch.Generator().manual_seed(8)
    c = torch.randint(1, 64, (N,), generator=gen).float() / 64
    c[::4] = 0.0
    p_inst = torch.stack([c[[ptr[int(index[q])] + i for i in sets[q]]].sum() for q in range(Q)])
    p = torch.stack([c[ptr[g]:ptr[g + 1]].sum() for g in graphs])
    got = _check_values(libs[which], dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, antithetic, 0.0, 1)
    assert _same_bits(got["phi"], c) and bool((got["phi"][::4] == 0.0).all())
    assert _same_bits(got["m2"], T * c * c) and got["gap"].tolist() == [0.0] * len(sizes) and got["flag"].tolist() == [0] * len(sizes)
    # symmetric: v(S) = |S| / n on the graphs whose n is a power of two: every phi of the graph is 1 / n EXACTLY
    sym = torch.tensor([len(sets[q]) / sizes[int(index[q])] for q in range(Q)])
    got = _check_values(libs[which], dev, sym, torch.ones(len(sizes)), pos, ptr, graphs, row_ptr, N, M, Q, antithetic, 0.0, 1)
    for g, n in enumerate(sizes):
        if n and n & (n - 1) == 0:
            assert got["phi"][ptr[g]:ptr[g + 1]].tolist() == [1.0 / n] * n and float(got["gap"][g]) == 0.0, (g, n)


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_flags_and_the_nan_rule(libs, dev, which):
    sizes = (5, 3, 0, 1, 8, 4, 1)
    graphs = (0, 1, 2, 3, 4, 5, 6, 7)
    M = 4
    ptr, row_ptr, N, Q, pos, p_inst, p = _value_case(sizes, graphs, M, True, SEEDS[1], 1)
    p_inst, p, row_ptr = p_inst.clone(), p.clone(), list(row_ptr)
    p_inst[row_ptr[1] - 1] = INF                         # the last row of graph 0
    p[1] = NAN                                           # graph 1's own probability
    p[3] = -INF                                          # the one-node graph 3 has no rows: its p alone flags it
    p_inst[row_ptr[5]] = NAN                             # graph 5 ...
    row_ptr[5] = Q - M * 3 + 1                           # ... whose rows would end behind Q: the bad row_ptr comes first, nothing is read
    got = _check_values(libs[which], dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, True, 0.0, 1)
    assert got["flag"].tolist() == [1, 1, 0, 1, 0, 2, 0, 2]
    assert bool(torch.isnan(got["phi"][:9]).all()) and bool(torch.isnan(got["m2"][:9]).all()) and bool(torch.isnan(got["gap"][[0, 1, 3, 5, 7]]).all())
    assert bool((got["phi"][ptr[5]:ptr[6]] == SENTINEL).all()) and bool((got["m2"][ptr[5]:ptr[6]] == SENTINEL).all())
    assert float(got["gap"][2]) == 0.0 and bool(torch.isfinite(got["phi"][ptr[4]:ptr[5]]).all()) and float(got["phi"][ptr[6]]) == float(p[6])
    row_ptr[0] = -1                                      # a negative first row
    got = _check_values(libs[which], dev, p_inst, p, pos, ptr, graphs, row_ptr, N, M, Q, True, 0.0, 1)
    assert got["flag"].tolist() == [2, 1, 0, 1, 0, 2, 0, 2] and bool((got["phi"][:5] == SENTINEL).all())
    # refusals write nothing
    for kw in (dict(M=3), dict(M=1026), dict(antithetic=2), dict(W=65), dict(v_empty=NAN), dict(v_empty=INF)):
        args = dict(M=M, antithetic=1, W=1, v_empty=0.0)
        args.update(kw)
        code, out, intact = _values(libs[which], dev, p_inst, p, pos, ptr, graphs, row_ptr, N, args["M"], Q, args["antithetic"],
                                    args["v_empty"], args["W"])
        assert code in (-1, -2) and intact and all(bool((v == SENTINEL).all()) for v in out.values()), kw


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_ops_shapley_values_and_the_known_answer(libs, dev, which):
    from isubgvqa_amd import _lib, ops
    seed, _, pos_rows, rows, p_inst, p, phi = SR.known_answer()
    with _lib.using(libs[which]):
        plan = ops.GraphPlan.build(torch.tensor([0, 0, 0]).to(dev), torch.zeros(2, 0, dtype=torch.int64, device=dev), num_graphs=1)
        ops.reset_counters()
        bits = ops.shapley_keep_bits(plan, permutations=2, seed=seed).verify()
        assert bits.pos.tolist() == pos_rows and bits.keep.view(-1).tolist() == rows and bits.status.tolist() == [0, 0, 0, 4]
        out = ops.shapley_values(torch.tensor(p_inst).to(dev), torch.tensor([p]).to(dev), bits, plan)
        assert ops.counters()["shapley_values"] == 1 and ops.counters()["shapley_keep_bits"] == 1
        assert out[0].tolist() == phi and out[1].tolist() == [0.09765625, 0.0625, 0.19140625] and out[2].tolist() == [0.0] and out[3].tolist() == [0]
        phi2, none, gap, flag = ops.shapley_values(torch.tensor(p_inst).to(dev), torch.tensor([p]).to(dev), bits, plan, v_empty=0.125, want_m2=False)
        assert none is None and phi2.tolist() == [0.25, 0.1875, 0.4375] and gap.tolist() == [0.0]
        with pytest.raises(ValueError, match="shape"):
            ops.shapley_values(torch.zeros(3, device=dev), torch.tensor([p]).to(dev), bits, plan)
        with pytest.raises(ValueError, match="finite"):
            ops.shapley_values(torch.tensor(p_inst).to(dev), torch.tensor([p]).to(dev), bits, plan, v_empty=NAN)
        # graphs that are not listed keep 0
        two = ops.GraphPlan.build(torch.tensor([0, 0, 0, 1, 1]).to(dev), torch.zeros(2, 0, dtype=torch.int64, device=dev), num_graphs=2)
        b1 = ops.shapley_keep_bits(two, graphs=torch.tensor([0]), permutations=2, seed=seed).verify()
        assert b1.pos.tolist() == [r + [-1, -1] for r in pos_rows]
        out = ops.shapley_values(torch.tensor(p_inst).to(dev), torch.tensor([p, 0.5]).to(dev), b1, two)
        assert out[0].tolist() == phi + [0.0, 0.0] and out[2].tolist() == [0.0]
