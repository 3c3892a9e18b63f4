"""isg_maskopt_step on the GPU (include/ext/isg_maskopt.h) against the float64 restatement of
tests/maskopt_restated.py -- on the product library and on its strict twin, with guard words behind every output and a second call
that must give the first one's bits -- and explain.mask_optimize on scores whose optimisation can be followed on the host.

TOLERANCES (derived in tests/maskopt_restated.py, not measured; u = 2^-24).  d theta against float64 by the bound of its operation
chain: the row dot's C + 8 roundings, expf's documented ulp, the divisions.  The Adam update FROM THE KERNEL'S OWN d theta BITS: the
restatement does Adam in float64 on those bits, so that the division by sqrt(v) + eps amplifies nothing of the gradient's rounding
into the tolerance; a skipped row keeps its bits.  The masked rows FROM THE KERNEL'S OWN new logits likewise.  The trajectory: the
device's distance from a float64 run at most 4 x an fp32 torch run's (torch.optim.Adam on the host) plus u |theta|."""
import ctypes
import functools

import pytest
import torch

import maskopt_restated as MR

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -7.0
U = 2.0 ** -24
ALL_SIZES = [0, 1, 2, 15, 16, 17, 65]
STEPS = (1, 2, 7)
WORST = {}                       # largest error / bound seen per check, printed by the last test (a record for DESIGN.md 37)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def libs():
    """{"fast": the product library, "strict": its strict twin}, both bound from include/ext/isg_maskopt.h."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _ext_maskopt, _lib
    strict = _lib.bind(ctypes.CDLL(ge.STRICT_LIB), _ext_maskopt.SIGNATURES)
    assert strict.isg_maskopt_abi_version() == _ext_maskopt.ABI_VERSION
    return {"fast": _ext_maskopt.load(), "strict": strict}


def _case(id, sizes, C, pad, lead=0, trail=0, with_d=True):
    return dict(id=id, sizes=tuple(sizes), C=C, pad=pad, lead=lead, trail=trail, with_d=with_d)


CASES = [
    _case("B1-n65-C4", [65], 4, 0),
    _case("B1-n17-C300-pad", [17], 300, 4, lead=2, trail=3),
    _case("B3-n0-17-0-C60", [0, 17, 0], 60, 0),
    _case("B3-n2-1-65-C64-pad-no-d", [2, 1, 65], 64, 4, with_d=False),
    _case("B3-n15-16-17-C68-outside", [15, 16, 17], 68, 0, lead=1, trail=18),
    _case("B70-every-size-C68-pad-outside", ALL_SIZES * 10, 68, 4, lead=3, trail=2),
    _case("B70-every-size-reversed-C4-no-d", (ALL_SIZES * 10)[::-1], 4, 0, with_d=False),
    _case("B70-every-size-C300-pad", ALL_SIZES * 10, 300, 4),
    _case("B70-every-size-reversed-C60", (ALL_SIZES * 10)[::-1], 60, 0, trail=1),
]
IDS = [c["id"] for c in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(id):
    """The case's inputs on the host, drawn once: the segment starts (the first `lead` and the last `trail` rows lie in no
    segment), x, one gradient tensor per step of STEPS, logits in [-4, 4] with +-20 and +-90 planted, the rows whose gradient holds
    an inf / a NaN at the second step."""
    c = next(c for c in CASES if c["id"] == id)
    seg = [c["lead"]]
    for n in c["sizes"]:
        seg.append(seg[-1] + n)
    N = seg[-1] + c["trail"]
    gen = torch.Generator().manual_seed(7 + len(c["sizes"]) + c["C"])
    x = torch.randn(N, c["C"], generator=gen)
    gs = [torch.randn(N, c["C"], generator=gen) for _ in STEPS]
    theta = torch.rand(N, generator=gen) * 8 - 4
    inner = list(range(seg[0], seg[-1]))
    planted = {}
    if len(inner) >= 12:
        for row, v in zip(inner[1:9:2], (20.0, -20.0, 90.0, -90.0)):
            theta[row] = v
            planted[row] = v
        bad = (inner[2], inner[-2])                      # between planted rows, and next to the end
        gs[1][bad[0], c["C"] // 2] = float("inf")
        gs[1][bad[1], 0] = float("nan")
    else:
        bad = ()
    return c, seg, N, x, gs, theta, planted, bad


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


def _vec(values, dev):
    """An fp32 [N] view holding `values` with GUARD sentinel words behind it -> (buffer, view)."""
    n = values.numel()
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[:n] = values
    return buf, buf[:n]


def _p(t):
    return 0 if t is None else t.data_ptr()


def _note(name, err, bound):
    ok = bound > 0
    if bool(ok.any()):
        WORST[name] = max(WORST.get(name, 0.0), float((err[ok] / bound[ok]).max()))


def _run(lib, dev, c, seg, x, g, theta, exp_avg, exp_avg_sq, step, with_d=True, moments=True, C=None, pad=None):
    """One call of isg_maskopt_step on fresh buffers (state copied in, outputs filled with SENTINEL) ->
    dict(rc, theta, exp_avg, exp_avg_sq, d, x_out, bufs)."""
    C = c["C"] if C is None else C
    pad = c["pad"] if pad is None else pad
    N = x.size(0)
    _, xd = _rows_buffer(N, C, pad, dev, x[:, :C])
    gd = None if g is None else _rows_buffer(N, C, pad, dev, g[:, :C])[1]
    tb, tv = _vec(theta, dev)
    mb, mv = _vec(exp_avg, dev) if moments else (None, None)
    vb, vv = _vec(exp_avg_sq, dev) if moments else (None, None)
    db, dv = _vec(torch.full((N,), SENTINEL), dev) if with_d else (None, None)
    ob, ov = _rows_buffer(N, C, pad, dev)
    segd = torch.tensor(seg, dtype=torch.int32, device=dev)
    k = MR.scalars(step=step, **MR.PYG)
    rc = lib.isg_maskopt_step(_p(xd), C + pad, _p(gd), C + pad, _p(segd), len(seg) - 1, _p(tv), _p(mv), _p(vv), _p(ov), C + pad, _p(dv),
                              N, C, MR.PYG["a_size"], MR.PYG["a_ent"], MR.PYG["lr"], MR.PYG["beta1"], MR.PYG["beta2"], MR.PYG["eps"],
                              k["bc1"], k["bc2"], None)
    torch.cuda.synchronize()
    return dict(rc=rc, theta=tv, exp_avg=mv, exp_avg_sq=vv, d=dv, x_out=ov, bufs=(tb, mb, vb, db, ob), N=N, C=C, pad=pad)


def _guards_intact(out):
    tb, mb, vb, db, ob = out["bufs"]
    N = out["N"]
    return all(b is None or bool((b[N:] == SENTINEL).all()) for b in (tb, mb, vb, db)) and _untouched(ob, N, out["C"], out["pad"])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_step(out, x, g, seg, theta0, m0, v0, step, planted, bad, name):
    """One call's outputs against the restatement: d theta by its chain's bound, Adam from the device's own d, the masked rows from
    the device's own new logits; rows outside every segment unwritten."""
    assert out["rc"] == 0 and _guards_intact(out), name
    N = x.size(0)
    d_ref, d_bound, inside = MR.d_theta(x, g, seg, theta0, MR.PYG["a_size"], MR.PYG["a_ent"])
    d_dev = out["d"].cpu()
    outside = ~inside
    assert bool((d_dev[outside] == SENTINEL).all()), name
    finite = inside & torch.isfinite(d_ref)
    assert bool(torch.isfinite(d_dev[finite]).all()) and not bool(torch.isfinite(d_dev[inside & ~finite]).any()), name
    err = (d_dev.double() - d_ref).abs()
    _note("d theta", err[finite], d_bound[finite])
    assert bool((err[finite] <= d_bound[finite]).all()), (name, float((err[finite] / d_bound[finite]).max()))
    for row, v in planted.items():
        if abs(v) == 90.0 and bool(finite[row]):         # saturation: exactly zero, never a NaN
            assert float(d_dev[row]) == 0.0, (name, row, float(d_dev[row]))
    if step == STEPS[1]:
        for row in bad:
            assert not bool(torch.isfinite(d_dev[row])), (name, row)
    # Adam from the device's own d: rows outside are handed a d of NaN here, which the restatement skips as the kernel leaves them
    d_own = torch.where(inside, d_dev, torch.full_like(d_dev, float("nan")))
    (t1, m1, v1), (bt, bm, bv), applied = MR.adam(d_own, theta0, m0, v0, step=step, **{k: MR.PYG[k] for k in ("lr", "beta1", "beta2", "eps")})
    for what, got, ref, bound in (("theta", out["theta"], t1, bt), ("exp_avg", out["exp_avg"], m1, bm), ("exp_avg_sq", out["exp_avg_sq"], v1, bv)):
        err = (got.cpu().double() - ref).abs()
        _note("adam " + what, err[applied], bound[applied])
        assert bool((err <= bound).all()), (name, what, float((err[applied] / bound[applied]).max()))
    for got, before in ((out["theta"], theta0), (out["exp_avg"], m0), (out["exp_avg_sq"], v0)):      # skipped and outside rows: the same bits
        assert _same_bits(got.cpu()[~applied], before[~applied]), name
    _check_rows(out, x, out["theta"].cpu(), inside, name)
    return d_dev


def _check_rows(out, x, theta_dev, inside, name):
    rows, bound = MR.masked_rows(x, theta_dev)
    got = out["x_out"].cpu()
    assert bool((got[~inside] == SENTINEL).all()), name
    err = (got.double() - rows).abs()
    _note("masked rows", err[inside], bound[inside])
    assert bool((err[inside] <= bound[inside]).all()), (name, float((err[inside] / bound[inside].clamp_min(1e-300)).max()))


@pytest.mark.parametrize("which", ["fast", "strict"])
@pytest.mark.parametrize("id", IDS)
def test_step_against_the_restatement(dev, libs, which, id):
    c, seg, N, x, gs, theta, planted, bad = _inputs(id)
    lib = libs[which]
    inside = MR.segment_of(seg, N)[0] >= 0
    # the apply-only form first, as the first iteration uses it: nothing but x_out is written, moments and d theta are not looked at
    first = _run(lib, dev, c, seg, x, None, theta, theta, theta, 1, with_d=True)
    assert first["rc"] == 0 and _guards_intact(first)
    assert _same_bits(first["theta"].cpu(), theta) and _same_bits(first["exp_avg"].cpu(), theta) and bool((first["d"] == SENTINEL).all())
    _check_rows(first, x, theta, inside, "apply-only")
    bare = _run(lib, dev, c, seg, x, None, theta, None, None, 1, with_d=False, moments=False)
    assert bare["rc"] == 0 and torch.equal(bare["x_out"], first["x_out"])
    for row, v in planted.items():                       # saturation: a mask of exactly 1 or +0
        want = x[row] if v >= 20 else (x[row] * 0.0 if v == -90 else None)
        if want is not None:
            assert _same_bits(first["x_out"][row].cpu(), want), (row, v)
    # steps 1, 2 and 7, each fed the state the one before left on the device
    t0, m0, v0 = theta, torch.zeros(N), torch.zeros(N)
    for step, g in zip(STEPS, gs):
        out = _run(lib, dev, c, seg, x, g, t0, m0, v0, step)
        _check_step(out, x, g, seg, t0, m0, v0, step, planted, bad, f"step {step}")
        again = _run(lib, dev, c, seg, x, g, t0, m0, v0, step, with_d=c["with_d"])
        assert again["rc"] == 0 and _guards_intact(again)
        for k in ("theta", "exp_avg", "exp_avg_sq", "x_out"):            # a second call, with or without d theta: the same bits
            assert _same_bits(again[k], out[k]), (step, k)
        if c["with_d"]:
            assert _same_bits(again["d"], out["d"])
        applied = _run(lib, dev, c, seg, x, None, out["theta"].cpu(), None, None, 1, with_d=False, moments=False)
        assert torch.equal(applied["x_out"], out["x_out"]), "the apply-only form on the new logits gives the step's rows"
        t0, m0, v0 = out["theta"].cpu().clone(), out["exp_avg"].cpu().clone(), out["exp_avg_sq"].cpu().clone()
    assert bool(torch.isfinite(t0[inside]).all())
    if bad:                                              # the skipped rows moved at steps 1 and 7 only: their moments are one update short
        assert float(m0[bad[0]]) != 0.0 and float(m0[bad[1]]) != 0.0


def test_refusals_write_nothing(dev, libs):
    c, seg, N, x, gs, theta, planted, bad = _inputs("B3-n15-16-17-C68-outside")
    lib = libs["fast"]
    zero = torch.zeros(N)
    for change in ({"C": 66}, {"pad": 2}):
        for g in (gs[0], None):
            out = _run(lib, dev, c, seg, x, g, theta, zero, zero, 1, **change)
            assert out["rc"] == -2, change
            tb, mb, vb, db, ob = out["bufs"]
            assert bool((ob == SENTINEL).all()) and bool((db == SENTINEL).all()) and _same_bits(out["theta"].cpu(), theta)
            assert bool((out["exp_avg"] == 0).all()) and bool((out["exp_avg_sq"] == 0).all())
    from isubgvqa_amd import ops
    xd, td = x.to(dev), theta.to(dev)
    segd = torch.tensor(seg, dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.maskopt_step(xd.clone().requires_grad_(True), None, segd, td, None, None, step=1)
    with pytest.raises(ValueError, match="step"):
        ops.maskopt_step(xd, None, segd, td, None, None, step=0)
    with pytest.raises(ValueError, match="exp_avg is required"):
        ops.maskopt_step(xd, gs[0].to(dev), segd, td, None, None, step=1)
    # through ops: strided rows, out=, want_grad; the counter
    ops.reset_counters()
    wide = torch.full((N, 72), SENTINEL, device=dev)
    t1, m1, v1 = td.clone(), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    rows, d = ops.maskopt_step(xd, gs[0].to(dev), segd, t1, m1, v1, step=1, out=wide[:, :68], want_grad=True)
    ref = _run(lib, dev, c, seg, x, gs[0], theta, zero, zero, 1)
    assert rows.data_ptr() == wide.data_ptr() and bool((wide[:, 68:] == SENTINEL).all()) and ops.counters()["maskopt_step"] == 1
    inside = MR.segment_of(seg, N)[0] >= 0
    assert _same_bits(rows[inside], ref["x_out"][inside]) and _same_bits(d[inside], ref["d"][inside]) and _same_bits(t1, ref["theta"])
    assert ops.maskopt_step(xd, None, segd, t1, None, None, step=3, want_grad=True)[1] is None


# ---- the model-free core -------------------------------------------------------------------------------------------------------
def _plan_of(sizes, dev, edges_per_node=2, seed=5):
    from isubgvqa_amd import ops
    gen = torch.Generator().manual_seed(seed)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    src, dst, off = [], [], 0
    for n in sizes:
        k = edges_per_node * n
        src += (off + torch.randint(0, n, (k,), generator=gen)).tolist()
        dst += (off + torch.randint(0, n, (k,), generator=gen)).tolist()
        off += n
    ei = torch.tensor([src, dst])
    return batch, ei, ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=len(sizes))


def _torch_run(score, x, seg, theta0, T, dtype):
    """GNNExplainer's loop as PyG writes it, in torch on the host in `dtype`: the mask's sigmoid, the score, the size term and the
    eps-guarded entropy as per-graph means, torch.optim.Adam on theta -> (theta after T steps, every step's d theta)."""
    theta = theta0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([theta], lr=MR.PYG["lr"])
    xs, grads = x.to(dtype), []
    for _ in range(T):
        opt.zero_grad()
        m = torch.sigmoid(theta)
        loss = score(xs * m.unsqueeze(1)).sum()
        for j in range(len(seg) - 1):
            mj = m[seg[j]:seg[j + 1]]
            ent = -mj * torch.log(mj + 1e-15) - (1 - mj) * torch.log(1 - mj + 1e-15)
            loss = loss + MR.PYG["a_size"] * mj.mean() + MR.PYG["a_ent"] * ent.mean()
        loss.backward()
        grads.append(theta.grad.detach().clone())
        opt.step()
    return theta.detach(), torch.stack(grads)


def test_trajectory_against_float64_and_an_fp32_torch_run(dev):
    """score = sum_n (a . x_n)^2 over the graph's MASKED rows with a, x > 0: s = 2 sigmoid (a . x)^2 > 0 and reg > 0 while
    theta < 10, so every d theta is positive and far from zero (verified below, in float64, before anything runs on the device) and
    Adam's m / sqrt(v) does not turn a rounding into a sign.  T = 20 steps from the same seeded logits, three ways: float64 torch on
    the host (the truth), fp32 torch on the host (the reference: torch.optim.Adam, autograd's sigmoid and row sums), the device."""
    from isubgvqa_amd import explain
    sizes, C, T = [17, 1, 65, 5], 12, 20
    batch, ei, plan = _plan_of(sizes, dev)
    gen = torch.Generator().manual_seed(21)
    N = batch.numel()
    x, a = torch.rand(N, C, generator=gen) + 0.5, torch.rand(C, generator=gen) + 0.1
    e = torch.rand(ei.size(1), 4, generator=gen)
    theta0 = 0.1 * torch.randn(N, generator=gen)
    seg = [0]
    for n in sizes:
        seg.append(seg[-1] + n)

    def score_on(bt, av):
        return lambda xm, em=None: torch.zeros(len(sizes), dtype=xm.dtype, device=xm.device).index_add(0, bt, ((xm * av).sum(1)) ** 2)

    truth, d64 = _torch_run(score_on(batch, a.double()), x, seg, theta0, T, torch.float64)
    assert float(d64.min()) > 1.0, float(d64.min())                       # no d theta comes near zero
    ref, _ = _torch_run(score_on(batch, a), x, seg, theta0, T, torch.float32)
    # the restatement's own loop in float64 (the header's function, its scalars rounded once) stays with PyG's formulation
    t_r, m_r, v_r = theta0.double(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for it in range(1, T + 1):
        xm = (MR.sigmoid(t_r).unsqueeze(1) * x.double()).requires_grad_(True)
        (g,) = torch.autograd.grad(score_on(batch, a.double())(xm).sum(), [xm])
        _, _, t_r, m_r, v_r = MR.step(x, g, seg, t_r, m_r, v_r, step=it, **MR.PYG)
    assert float((t_r - truth).abs().max()) < 1e-7
    ad = a.to(dev).requires_grad_(True)
    res = explain.mask_optimize(score_on(batch.to(dev), ad), x.to(dev), e.to(dev), plan, ei.to(dev), steps=T, init=theta0.to(dev))
    assert ad.grad is None and res.steps == T and res.nll.shape == (T + 1, len(sizes)) and res.edge_theta is None
    got = res.theta.cpu().double()
    dist_dev, dist_ref = float((got - truth).abs().max()), float((ref.double() - truth).abs().max())
    print(f"[maskopt] trajectory, T = {T}: max |theta - float64| = {dist_dev:.3e} on the device, {dist_ref:.3e} for fp32 torch on the host")
    assert dist_dev <= 4 * dist_ref + U * float(truth.abs().max()), (dist_dev, dist_ref)
    assert torch.equal(res.soft, torch.sigmoid(res.theta))
    # the recorded scores: row 0 at the initial mask, the last row at the final one
    for row, t in ((0, theta0.double()), (T, got)):
        want = score_on(batch, a.double())(MR.sigmoid(t).unsqueeze(1) * x.double())
        assert float(((res.nll[row].cpu().double() - want).abs() / want).max()) < 1e-5
    assert bool((res.nll[T] < res.nll[0]).all())
    # a seeded std as init: the same call gives the same bits, another seed other logits
    kw = dict(steps=2, init=0.1)
    one, two, other = (explain.mask_optimize(score_on(batch.to(dev), ad), x.to(dev), e.to(dev), plan, ei.to(dev), init_seed=s, **kw)
                       for s in (3, 3, 4))
    assert torch.equal(one.theta, two.theta) and torch.equal(one.nll, two.nll) and not torch.equal(one.theta, other.theta)


def test_planted_nodes_are_found(dev):
    """A score that rewards k = 3 planted nodes of each graph and ignores the others: score_b = -sum over the planted n of a . x_n
    (masked).  A planted row's d theta is negative (its logit rises by about lr a step), every other row's is the regularisers'
    alone (positive: its logit falls).  12 graphs of 5 to 17 nodes, T = 60; mask(3) must be the planted set in every graph -- on
    the float64 host loop first, then on the device."""
    from isubgvqa_amd import explain
    sizes, C, T, K = [5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17], 8, 60, 3
    batch, ei, plan = _plan_of(sizes, dev, seed=9)
    gen = torch.Generator().manual_seed(33)
    N = batch.numel()
    x, a = torch.rand(N, C, generator=gen) + 0.5, torch.rand(C, generator=gen) + 0.1
    e = torch.rand(ei.size(1), 4, generator=gen)
    theta0 = 0.1 * torch.randn(N, generator=gen)
    seg, planted = [0], torch.zeros(N)
    for n in sizes:
        planted[seg[-1] + torch.randperm(n, generator=gen)[:K]] = 1.0
        seg.append(seg[-1] + n)

    def score_on(bt, av, w):
        return lambda xm, em=None: torch.zeros(len(sizes), dtype=xm.dtype, device=xm.device).index_add(0, bt, -w * (xm * av).sum(1))

    t_r, m_r, v_r = theta0.double(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    g = -planted.double().unsqueeze(1) * a.double()                      # the score is linear: its gradient rows do not move
    for it in range(1, T + 1):
        _, _, t_r, m_r, v_r = MR.step(x, g, seg, t_r, m_r, v_r, step=it, **MR.PYG)
    for j in range(len(sizes)):
        top = t_r[seg[j]:seg[j + 1]].topk(K).indices + seg[j]
        assert bool((planted[top] == 1).all()), ("float64", j)
    assert float(t_r[planted == 1].min() - t_r[planted == 0].max()) > 0.5
    res = explain.mask_optimize(score_on(batch.to(dev), a.to(dev), planted.to(dev)), x.to(dev), e.to(dev), plan, ei.to(dev), steps=T,
                                init=theta0.to(dev))
    assert torch.equal(res.mask(K).cpu().view(-1), planted)
    assert float((res.theta.cpu().double() - t_r).abs().max()) < 1e-4


def test_zz_print_the_largest_errors_seen():
    """A record, not a check: the largest error / bound of every kind of comparison above (DESIGN.md 37 quotes them)."""
    for k in sorted(WORST):
        print(f"[maskopt] {k}: largest error / bound = {WORST[k]:.3f}")
