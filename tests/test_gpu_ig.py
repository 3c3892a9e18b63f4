"""isg_ig_path_rows and isg_ig_attribution on the GPU (include/ext/isg_ig.h) against the float64 loops of
tests/ig_restated.py -- on the product library and on its strict twin, with guard words behind every output and a second call
that must give the first one's bits -- and explain.path_attributions on a score whose integral is known in closed form.

TOLERANCES (derived, not measured; u = 2^-24).
Path rows: rn(1 - t), rn(. * b) and the fma are three roundings, each relative to a quantity no larger than |t x| + |(1 - t) b|:
|got - ref| <= 4 u (|t x| + |(1 - t) b|) (the fourth u pays for the second-order terms).  t = 0 and t = 1 must give the bits of
the baseline and of x, a missing baseline the bits of torch's fp32 x * t.
Attribution: G is a chain of at most S fmas over terms w g (S roundings relative to sum_j |w g|), d = rn(x - b) is one, every
product d G one, and the C products are added in SOME order by C - 1 additions (the bound does not care which): fewer than
S + C + 8 roundings relative to sum_c |x_c - b_c| sum_j |w_j g_jc|, so |got - ref| <= 1.01 (S + C + 8) u times that sum (in
float64), plus u |result| for the one add of an accumulating call.  The rows G themselves: 1.01 (S + 1) u sum_j |w_j g_jc|."""
import ctypes
import functools

import pytest
import torch

import ig_restated as IR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7.0
U = 2.0 ** -24
ALL_SIZES = [0, 1, 2, 15, 16, 17, 65]
WORST = {}                       # largest error / bound seen per check, printed by the last test (a record for DESIGN.md 36)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """{"fast": the product library, "strict": its strict twin}, both bound from include/ext/isg_ig.h."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_ig, _lib
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB), _ext_ig.SIGNATURES)
    assert strict.isg_ig_abi_version() == _ext_ig.ABI_VERSION
    return {"fast": _ext_ig.load(), "strict": strict}


def _case(id, sizes, S, C, pad, base, path_e, edges=True, unnamed=(), avg=True, Ce=None):
    return dict(id=id, sizes=tuple(sizes), S=S, C=C, pad=pad, base=base, path_e=path_e, edges=edges, unnamed=tuple(unnamed), avg=avg,
                Ce=C if Ce is None else Ce)


CASES = [
    _case("B1-n65-S1-C4", [65], 1, 4, 0, None, 0),
    _case("B1-n17-S9-C300-pad-rows", [17], 9, 300, 4, "rows", 1, Ce=68),
    _case("B3-n16-0-15-S2-C60-row-no-edges", [16, 0, 15], 2, 60, 0, "row", 1, edges=False),
    _case("B3-n2-1-65-S3-C64-pad-rows-unnamed", [2, 1, 65], 3, 64, 4, "rows", 0, unnamed=[1], avg=False),
    _case("B3-n1-17-2-S4-C68", [1, 17, 2], 4, 68, 0, None, 1),
    _case("B70-every-size-S5-C68-pad-row-unnamed", ALL_SIZES * 10, 5, 68, 4, "row", 1, unnamed=[3, 4, 69], Ce=4),
    _case("B70-every-size-S2-C4-rows", ALL_SIZES * 10, 2, 4, 0, "rows", 0, Ce=60),
    _case("B70-every-size-S3-C60-no-avg", ALL_SIZES * 10, 3, 60, 4, None, 1, avg=False, Ce=64),
]
IDS = [c["id"] for c in CASES]


def _layout(sizes, ecount, index):
    """The instance batch of `index` over graphs of `sizes` nodes and `ecount` edges, as lists: what ops.graph_instances makes."""
    ptr, erange = [0], [0]
    for n, m in zip(sizes, ecount):
        ptr.append(ptr[-1] + n)
        erange.append(erange[-1] + m)
    inst_ptr, inst_eptr, node_src, inst_of, edge_src, einst_of = [0], [0], [], [], [], []
    for q, g in enumerate(index):
        node_src += list(range(ptr[g], ptr[g + 1]))
        inst_of += [q] * sizes[g]
        edge_src += list(range(erange[g], erange[g + 1]))
        einst_of += [q] * ecount[g]
        inst_ptr.append(len(node_src))
        inst_eptr.append(len(edge_src))
    gptr, glist = IR.by_graph(index, len(sizes))
    return dict(ptr=ptr, erange=erange, inst_ptr=inst_ptr, inst_eptr=inst_eptr, node_src=node_src, inst_of=inst_of, edge_src=edge_src,
                einst_of=einst_of, gptr=gptr, glist=glist, G=len(sizes), Q=len(index))


@functools.lru_cache(maxsize=None)
def _inputs(id):
    """The case's inputs on the host, drawn once (signed): the layout of all S steps (step-major: the instances of step s are
    the graphs in order, so a run of steps is a run of instances AND of rows), x, e, baselines, t, w, gradient rows."""
    c = next(c for c in CASES if c["id"] == id)
    sizes = list(c["sizes"])
    ecount = [(3 * n + g) % 7 if n else 0 for g, n in enumerate(sizes)] if c["edges"] else [0] * len(sizes)
    named = [g for g in range(len(sizes)) if g not in c["unnamed"]]
    index = [g for _ in range(c["S"]) for g in named]
    lay = _layout(sizes, ecount, index)
    gen = torch.Generator().manual_seed(11 + len(sizes) + c["S"])
    N, E, C, Ce = lay["ptr"][-1], lay["erange"][-1], c["C"], c["Ce"]
    x, e = torch.randn(N, C, generator=gen), torch.randn(E, Ce, generator=gen)
    base = {None: (None, None), "row": (torch.randn(C, generator=gen), torch.randn(Ce, generator=gen)),
            "rows": (torch.randn(N, C, generator=gen), torch.randn(E, Ce, generator=gen))}[c["base"]]
    t_steps, w_steps = torch.rand(c["S"], generator=gen), torch.rand(c["S"], generator=gen) - 0.3      # signed weights too
    t = t_steps.repeat_interleave(len(named))
    w = w_steps.repeat_interleave(len(named))
    g_x = torch.randn(len(lay["node_src"]), C, generator=gen)
    g_e = torch.randn(len(lay["edge_src"]), Ce, generator=gen)
    return c, lay, x, e, base, t, w, g_x, g_e


def _rows_buffer(rows, C, pad, dev, values=None):
    """A [rows, C] view with row stride C + pad of a buffer filled with SENTINEL (or holding `values`), GUARD words behind it."""
    buf = torch.full((rows * (C + pad) + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[:rows * (C + pad)].view(rows, C + pad)[:, :C]
    if values is not None:
        view.copy_(values)
    return buf, view


def _untouched(buf, rows, C, pad):
    """The pad columns and the guard words still hold SENTINEL."""
    body = buf[:rows * (C + pad)].view(rows, C + pad)
    return bool((body[:, C:] == SENTINEL).all()) and bool((buf[rows * (C + pad):] == SENTINEL).all())


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _i64(v, dev):
    return torch.tensor(v, dtype=torch.int64, device=dev)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _note(name, err, bound):
    ok = bound > 0
    if bool(ok.any()):
        WORST[name] = max(WORST.get(name, 0.0), float((err[ok] / bound[ok]).max()))


def _run_path(lib, dev, c, lay, x, e, base, t, node_src=None, inst_of=None, x_rows=None):
    """One call of isg_ig_path_rows on fresh sentinel buffers -> (rc, x_out view, e_out view, the buffers)."""
    pad, C, Ce = c["pad"], c["C"], c["Ce"]
    n, m = len(lay["node_src"]), len(lay["edge_src"])
    _, xd = _rows_buffer(x.size(0), C, pad, dev, x)
    _, ed = _rows_buffer(e.size(0), Ce, pad, dev, e)
    bx, be = (None if b is None else (b.to(dev) if b.dim() == 1 else _rows_buffer(b.size(0), b.size(1), pad, dev, b)[1]) for b in base)
    xo_buf, xo = _rows_buffer(n, C, pad, dev)
    eo_buf, eo = _rows_buffer(m, Ce, pad, dev)
    ns = _i64(lay["node_src"] if node_src is None else node_src, dev)
    io = _i64(lay["inst_of"] if inst_of is None else inst_of, dev)
    es, eio, td = _i64(lay["edge_src"], dev), _i64(lay["einst_of"], dev), t.to(dev)
    ldb = lambda b, CC: 0 if b is None or b.dim() == 1 else CC + pad
    rc = lib.isg_ig_path_rows(_p(xd), C + pad, x.size(0) if x_rows is None else x_rows, _p(bx), ldb(base[0], C), _p(ns), _p(io), n,
                              _p(xo), C + pad, C, _p(ed), Ce + pad, e.size(0), _p(be), ldb(base[1], Ce), _p(es), _p(eio), m, _p(eo),
                              Ce + pad, Ce, _p(td), lay["Q"], c["path_e"], None)
    torch.cuda.synchronize()
    return rc, xo, eo, (xo_buf, eo_buf, n, m)


def _check_path(got, x, base, src, inst_of, t, interpolate, name):
    ref = IR.path_rows(x, base, src, inst_of, t, out=torch.full((len(src), x.size(1)), SENTINEL), interpolate=interpolate)
    got = got.cpu()
    if not interpolate:
        assert torch.equal(got.double(), ref), name
        return
    bound = 4 * U * IR.path_rows_bound(x, base, src, inst_of, t)
    err = (got.double() - ref).abs()
    _note("path rows", err, bound)
    assert bool((err <= bound).all()), (name, float((err - bound).max()))


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("id", IDS)
def test_path_rows_against_the_restatement(dev, libs, which, id):
    c, lay, x, e, base, t, w, g_x, g_e = _inputs(id)
    lib = libs[which]
    rc, xo, eo, (xo_buf, eo_buf, n, m) = _run_path(lib, dev, c, lay, x, e, base, t)
    assert rc == 0
    _check_path(xo, x, base[0], lay["node_src"], lay["inst_of"], t, True, "nodes")
    _check_path(eo, e, base[1], lay["edge_src"], lay["einst_of"], t, bool(c["path_e"]), "edges")
    assert _untouched(xo_buf, n, c["C"], c["pad"]) and _untouched(eo_buf, m, c["Ce"], c["pad"])
    again = _run_path(lib, dev, c, lay, x, e, base, t)
    assert again[0] == 0 and torch.equal(again[1], xo) and torch.equal(again[2], eo)
    if base[0] is None and n:                            # a baseline of zeros: ONE multiplication, torch's bits
        assert torch.equal(xo.cpu(), x[lay["node_src"]] * t[lay["inst_of"]].unsqueeze(1))
    # the two ends of the path as bits: the instances alternate between t = 0 and t = 1
    ends = (torch.arange(lay["Q"]) % 2).float()
    rc, xo, eo, _ = _run_path(lib, dev, c, lay, x, e, base, ends)
    assert rc == 0
    for got, rows, b, src, io, on in ((xo.cpu(), x, base[0], lay["node_src"], lay["inst_of"], True),
                                      (eo.cpu(), e, base[1], lay["edge_src"], lay["einst_of"], bool(c["path_e"]))):
        if not len(src):
            continue
        src_t, t_row = torch.tensor(src), ends[torch.tensor(io)].unsqueeze(1)
        full = rows[src_t]
        if not on:
            want = full
        elif b is None:                                  # rn(t x): a zero with x's sign at t = 0
            want = full * t_row
        else:                                            # (no input here is a zero, whose sign a sum may lose)
            want = torch.where(t_row == 1, full, b.expand_as(full) if b.dim() == 1 else b[src_t])
        assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def _run_attr(lib, dev, c, lay, x, e, base, w, g_x, g_e, accumulate=0, into=None, xo_rows=None):
    """One call of isg_ig_attribution; `into`: the buffers of a previous call (accumulate) -> (rc, attr_x, attr_e, avg_x, avg_e, bufs)."""
    pad, C, Ce = c["pad"], c["C"], c["Ce"]
    N, E = x.size(0), e.size(0)
    _, xd = _rows_buffer(N, C, pad, dev, x)
    _, ed = _rows_buffer(E, Ce, pad, dev, e)
    _, gx = _rows_buffer(g_x.size(0), C, pad, dev, g_x)
    _, ge = _rows_buffer(g_e.size(0), Ce, pad, dev, g_e)
    bx, be = (None if b is None else (b.to(dev) if b.dim() == 1 else _rows_buffer(b.size(0), b.size(1), pad, dev, b)[1]) for b in base)
    if into is None:
        ax_buf, ae_buf = (torch.full((k + GUARD,), SENTINEL, dtype=torch.float32, device=dev) for k in (N, E))
        vx_buf, vx = _rows_buffer(N, C, pad, dev) if c["avg"] else (None, None)
        ve_buf, ve = _rows_buffer(E, Ce, pad, dev) if c["avg"] else (None, None)
    else:
        ax_buf, ae_buf, vx_buf, vx, ve_buf, ve = into
    ldb = lambda b, CC: 0 if b is None or b.dim() == 1 else CC + pad
    keep = [_i32(lay[k], dev) for k in ("ptr", "erange", "inst_ptr", "inst_eptr", "gptr", "glist")]
    wd = w.to(dev)
    rc = lib.isg_ig_attribution(_p(gx), C + pad, g_x.size(0) if xo_rows is None else xo_rows, _p(xd), C + pad, _p(bx), ldb(base[0], C),
                                _p(ax_buf), _p(vx), C + pad, N, C,
                                _p(ge), Ce + pad, g_e.size(0), _p(ed), Ce + pad, _p(be), ldb(base[1], Ce), _p(ae_buf), _p(ve), Ce + pad,
                                E, Ce, _p(wd), *[_p(k) for k in keep], lay["G"], lay["Q"], accumulate, None)
    torch.cuda.synchronize()
    return rc, ax_buf[:N], ae_buf[:E], vx, ve, (ax_buf, ae_buf, vx_buf, vx, ve_buf, ve)


def _check_attr(c, out, refs, S, extra_u=False, name=""):
    rc, ax, ae, vx, ve, (ax_buf, ae_buf, vx_buf, _, ve_buf, _) = out
    assert rc == 0
    for got, avg, buf, avg_buf, (attr, G, bound, avg_bound, most), C in ((ax, vx, ax_buf, vx_buf, refs[0], c["C"]),
                                                                         (ae, ve, ae_buf, ve_buf, refs[1], c["Ce"])):
        assert most <= S
        rows = attr.numel()
        tol = 1.01 * (S + C + 8) * U * bound + (U * attr.abs() if extra_u else 0)
        err = (got.cpu().double() - attr).abs()
        _note("attribution" + (" (accumulated)" if extra_u else ""), err, tol)
        assert bool((err <= tol).all()), (name, float((err - tol).max()))
        assert bool((buf[rows:] == SENTINEL).all())
        if avg is not None:
            tol = 1.01 * (S + 1) * U * avg_bound + (U * G.abs() if extra_u else 0)
            err = (avg.cpu().double() - G).abs()
            _note("avg rows", err, tol)
            assert bool((err <= tol).all()), (name, "avg", float((err - tol).max()))
            assert _untouched(avg_buf, rows, C, c["pad"])


def _refs(lay, x, e, base, w, g_x, g_e):
    return (IR.attribution(g_x, w, x, base[0], lay["ptr"], lay["inst_ptr"], lay["gptr"], lay["glist"]),
            IR.attribution(g_e, w, e, base[1], lay["erange"], lay["inst_eptr"], lay["gptr"], lay["glist"]))


@functools.lru_cache(maxsize=None)
def _reference(id):
    """The case's float64 attribution, computed once and shared by the two libraries' tests."""
    c, lay, x, e, base, t, w, g_x, g_e = _inputs(id)
    return _refs(lay, x, e, base, w, g_x, g_e)


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("id", IDS)
def test_attribution_against_the_restatement(dev, libs, which, id):
    c, lay, x, e, base, t, w, g_x, g_e = _inputs(id)
    lib, S = libs[which], c["S"]
    refs = _reference(id)
    one = _run_attr(lib, dev, c, lay, x, e, base, w, g_x, g_e)
    _check_attr(c, one, refs, S, name="one call")
    for g in c["unnamed"]:                               # a graph that no instance names: +0, written
        rows = one[1][lay["ptr"][g]:lay["ptr"][g + 1]]
        assert bool((rows.view(torch.int32) == 0).all())
    again = _run_attr(lib, dev, c, lay, x, e, base, w, g_x, g_e)
    assert torch.equal(again[1], one[1]) and torch.equal(again[2], one[2])
    if c["avg"]:
        assert torch.equal(again[3], one[3]) and torch.equal(again[4], one[4])
    if S < 2:
        return
    # the same path in two chunks of whole steps, the second call accumulating: steps are runs of instances and of rows
    named = lay["Q"] // S
    sizes = [lay["ptr"][g + 1] - lay["ptr"][g] for g in range(lay["G"])]
    ecount = [lay["erange"][g + 1] - lay["erange"][g] for g in range(lay["G"])]
    index = [g for g in range(lay["G"]) if g not in c["unnamed"]]
    s1 = S // 2
    out = None
    for lo, hi in ((0, s1), (s1, S)):
        part = _layout(sizes, ecount, index * (hi - lo))
        q0, q1 = lo * named, hi * named
        r0, r1, e0, e1 = lay["inst_ptr"][q0], lay["inst_ptr"][q1], lay["inst_eptr"][q0], lay["inst_eptr"][q1]
        out = _run_attr(lib, dev, c, part, x, e, base, w[q0:q1], g_x[r0:r1], g_e[e0:e1], accumulate=0 if out is None else 1,
                        into=None if out is None else out[5])
    _check_attr(c, out, refs, S, extra_u=True, name="two chunks")
    for g in c["unnamed"]:                               # left as the first call wrote it
        assert bool((out[1][lay["ptr"][g]:lay["ptr"][g + 1]].view(torch.int32) == 0).all())


@pytest.mark.parametrize("which", ["fast", "strict"])
def test_bad_inputs_write_nothing_beyond_their_own_rows(dev, libs, which):
    c, lay, x, e, base, t, w, g_x, g_e = _inputs("B3-n2-1-65-S3-C64-pad-rows-unnamed")
    lib, Q, N = libs[which], lay["Q"], x.size(0)
    # path rows: a source row of -1 and of N, an instance number of -1 and of Q: those rows stay as they were, the others are right
    node_src, inst_of = list(lay["node_src"]), list(lay["inst_of"])
    node_src[0], node_src[5], inst_of[7], inst_of[-1] = -1, N, -1, Q
    rc, xo, eo, (xo_buf, eo_buf, n, m) = _run_path(lib, dev, c, lay, x, e, base, t, node_src=node_src, inst_of=inst_of)
    assert rc == 0
    _check_path(xo, x, base[0], node_src, inst_of, t, True, "nodes")
    for i in (0, 5, 7, n - 1):
        assert bool((xo[i] == SENTINEL).all())
    assert _untouched(xo_buf, n, c["C"], c["pad"]) and _untouched(eo_buf, m, c["Ce"], c["pad"])
    # fewer source rows than the map names: the rows beyond them are skipped
    rc, xo, _, _ = _run_path(lib, dev, c, lay, x, e, base, t, x_rows=N - 3)
    beyond = torch.tensor(lay["node_src"]) >= N - 3
    assert rc == 0 and int(beyond.sum()) == 9 and bool((xo.cpu()[beyond] == SENTINEL).all()) and bool((xo.cpu()[~beyond] != SENTINEL).all())
    # attribution: an instance number outside [0, Q) in the list, a short instance range, fewer gradient rows than the ranges name
    bad = dict(lay)
    bad["glist"] = list(lay["glist"])
    bad["glist"][1], bad["glist"][-1] = Q + 3, -2
    bad["inst_ptr"] = list(lay["inst_ptr"])
    bad["inst_ptr"][2] -= 1                              # instance 1 (graph 2, 65 nodes) is one row short; instance 2 starts a row early
    bad["gptr"] = list(lay["gptr"])
    bad["gptr"][-1] = Q + 50                             # clamped to Q
    rows_in = g_x.size(0) - 40
    refs = (IR.attribution(g_x[:rows_in], w, x, base[0], bad["ptr"], bad["inst_ptr"], bad["gptr"], bad["glist"]),
            IR.attribution(g_e, w, e, base[1], bad["erange"], bad["inst_eptr"], bad["gptr"], bad["glist"]))
    assert not torch.equal(refs[0][0], _reference(c["id"])[0][0])
    out = _run_attr(lib, dev, c, bad, x, e, base, w, g_x, g_e, xo_rows=rows_in)
    _check_attr(c, out, refs, c["S"], name="bad inputs")


def test_refusals_write_nothing(dev, libs):
    c, lay, x, e, base, t, w, g_x, g_e = _inputs("B3-n1-17-2-S4-C68")
    lib = libs["fast"]
    for change in ({"C": 66}, {"pad": 2}):
        cc = dict(c, **change)
        xs = x[:, :cc["C"]].contiguous()
        rc, xo, eo, (xo_buf, eo_buf, n, m) = _run_path(lib, dev, cc, lay, xs, e, base, t)
        assert rc == -2 and bool((xo_buf == SENTINEL).all()) and bool((eo_buf == SENTINEL).all()), change
        out = _run_attr(lib, dev, cc, lay, xs, e, base, w, g_x[:, :cc["C"]].contiguous(), g_e)
        assert out[0] == -2 and all(bool((b == SENTINEL).all()) for b in (out[5][0], out[5][1], out[5][2], out[5][4])), change


# ---- the model-free core -------------------------------------------------------------------------------------------------------
def _quadratic_problem(dev):
    """Three graphs (17, 1 and 65 nodes), C = 12 / Ce = 8, every number >= 0 and x >= b, e >= b_e."""
    from isubgvqa_amd import ops
    sizes = [17, 1, 65]
    gen = torch.Generator().manual_seed(5)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    src, dst, off = [], [], 0
    for n in sizes:
        k = 2 * n
        src += (off + torch.randint(0, n, (k,), generator=gen)).tolist()
        dst += (off + torch.randint(0, n, (k,), generator=gen)).tolist()
        off += n
    ei = torch.tensor([src, dst])
    N, E, C, Ce = batch.numel(), ei.size(1), 12, 8
    bx, be = torch.rand(N, C, generator=gen), torch.rand(Ce, generator=gen)
    x, e = bx + torch.rand(N, C, generator=gen), be + torch.rand(E, Ce, generator=gen)
    a, cvec = torch.rand(C, generator=gen) + 0.1, torch.rand(Ce, generator=gen) + 0.1
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=3)
    return dict(sizes=sizes, batch=batch, ei=ei, x=x, e=e, bx=bx, be=be, a=a, c=cvec, plan=plan, C=C, Ce=Ce)


@pytest.mark.parametrize("rule,S", [("midpoint", 1), ("midpoint", 3), ("gauss_legendre", 2)])
@pytest.mark.parametrize("edges", [False, True])
def test_path_attributions_are_exact_on_a_quadratic_score(dev, rule, S, edges):
    """score = sum_n (a . x_n)^2 + sum_e (c . e_e)^2 per instance; its gradient is linear along the path, so the midpoint rule and
    two-point Gauss-Legendre integrate it exactly: attribution[n] = (a . x_n)^2 - (a . b_n)^2 and delta = 0.

    THE BOUND.  a, c, b >= 0 and x >= b: every intermediate is a sum of non-negative terms, so relative errors add.  The chain
    behind attribution[n], in roundings of relative size u = 2^-24: t and w rounded to fp32 (the point b + t (x - b) moves by at
    most 2 u of its value since x >= b; w by u): 3; the path row's three operations: 3; the score's a . x as C products and C - 1
    additions: 2 C - 1; autograd's gradient 2 (a . x) a_c: 2; the S fmas behind G: S; rn(x - b): 1; the C products d G and their
    C - 1 additions: 2 C - 1 -- fewer than k = 4 C + S + 8, and (1 + u)^k - 1 <= 1.01 k u.  The same with Ce for an edge.
    delta adds the device's sums over a graph (n_g + e_g additions of non-negative attributions), and f_input, f_baseline, each
    2 C + 1 + n_g + e_g roundings of its own value, and their difference: |delta| <= 1.01 u ((k + n_g + e_g + 1) sum attr
    + (2 C + n_g + e_g + 3) (f_input + f_baseline)).  A chunked path is held to the same bound."""
    from isubgvqa_amd import explain
    p = _quadratic_problem(dev)
    a, cv = p["a"].to(dev).requires_grad_(True), p["c"].to(dev).requires_grad_(True)      # parameter-like leaves of the score
    calls = []

    def score(x_inst, e_inst, inst):
        calls.append((inst.Q, torch.is_grad_enabled()))
        node = ((x_inst * a).sum(1)) ** 2
        edge = ((e_inst * cv).sum(1)) ** 2
        z = torch.zeros(inst.Q, device=x_inst.device)
        return z.index_add(0, inst.batch, node).index_add(0, inst.batch.index_select(0, inst.edge_index[0]), edge)

    x, e = p["x"].to(dev), p["e"].to(dev)
    kw = dict(steps=S, rule=rule, baseline_x=p["bx"].to(dev), baseline_e=p["be"].to(dev), edges=edges)
    whole = explain.path_attributions(score, x, e, p["plan"], p["ei"].to(dev), rows=True, **kw)
    parts = explain.path_attributions(score, x, e, p["plan"], p["ei"].to(dev), max_instances=4, **kw)      # one step per chunk
    assert len(whole.chunks) == 1 and len(parts.chunks) == S and a.grad is None and cv.grad is None
    assert calls[0] == (3 * S, True) and calls[1] == (6, False)
    xd, bd, ed, bed, ad, cd = (t.double() for t in (p["x"], p["bx"], p["e"], p["be"], p["a"], p["c"]))
    want_x = (xd @ ad) ** 2 - (bd @ ad) ** 2
    want_e = (ed @ cd) ** 2 - (bed @ cd) ** 2
    ge = p["batch"][p["ei"][1]]
    nodes, edgs = torch.tensor(p["sizes"]).double(), torch.bincount(ge, minlength=3).double()
    f_in = torch.zeros(3, dtype=torch.float64).index_add_(0, p["batch"], (xd @ ad) ** 2).index_add_(0, ge, (ed @ cd) ** 2)
    f_base = torch.zeros(3, dtype=torch.float64).index_add_(0, p["batch"], (bd @ ad) ** 2)
    f_base.index_add_(0, ge, ((bed @ cd) ** 2).expand(ge.numel()) if edges else (ed @ cd) ** 2)      # off the path the edges stay
    total = torch.zeros(3, dtype=torch.float64).index_add_(0, p["batch"], want_x)
    if edges:
        total.index_add_(0, ge, want_e)
    for res in (whole, parts):
        k = 4 * p["C"] + S + 8
        err = (res.attribution.cpu().double() - want_x).abs()
        _note("quadratic score, nodes", err, 1.01 * k * U * want_x)
        assert bool((err <= 1.01 * k * U * want_x).all()), float((err / want_x).max() / U)
        if edges:
            ke = 4 * p["Ce"] + S + 8
            err = (res.edge_attribution.cpu().double() - want_e).abs()
            assert bool((err <= 1.01 * ke * U * want_e).all()), float((err / want_e).max() / U)
        else:
            assert res.edge_attribution is None
        ne = nodes + edgs
        assert bool(((res.f_input.cpu().double() - f_in).abs() <= 1.01 * (2 * p["C"] + ne + 2) * U * f_in).all())
        assert bool(((res.f_baseline.cpu().double() - f_base).abs() <= 1.01 * (2 * p["C"] + ne + 2) * U * f_base).all())
        bound = 1.01 * U * ((k + ne + 1) * total + (2 * p["C"] + ne + 3) * (f_in + f_base))
        _note("quadratic score, delta", res.delta.cpu().double().abs(), bound)
        assert bool((res.delta.cpu().double().abs() <= bound).all()), (res.delta.tolist(), bound.tolist())
        # delta is what it says, recomputed on the host from the device's own numbers
        again = torch.zeros(3).index_add_(0, p["batch"], res.attribution.cpu())
        if edges:
            again.index_add_(0, ge, res.edge_attribution.cpu())
        assert float((res.delta.cpu() - (again - (res.f_input.cpu() - res.f_baseline.cpu()))).abs().max()) <= \
            4 * U * float((again.abs() + res.f_input.cpu().abs() + res.f_baseline.cpu().abs()).max()) * (float(ne.max()) + 2)
    # the weighted gradient rows, when asked for: 2 (a . (x + b) / 2) a
    G = whole.avg_grad[0].cpu().double()
    want_G = ((xd + bd) @ ad).unsqueeze(1) * ad
    assert float(((G - want_G).abs() / want_G).max()) <= 1.01 * (2 * p["C"] + S + 8) * U
    assert parts.avg_grad is None and (whole.avg_grad[1] is not None) == edges
    m = whole.mask(2)
    per_graph = torch.zeros(3).index_add_(0, p["batch"], m.cpu().view(-1))
    assert m.shape == (p["batch"].numel(), 1) and per_graph.tolist() == [2.0, 1.0, 2.0]


def test_zz_print_the_largest_errors_seen():
    """A record, not a check: the largest error / bound of every kind of comparison above (DESIGN.md 36 quotes them)."""
    for k in sorted(WORST):
        print(f"[ig] {k}: largest error / bound = {WORST[k]:.3f}")
