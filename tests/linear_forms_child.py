"""The helpers of tests/test_gpu_linear_forms_fp64.py -- operands, the launch of a case through the Python launchers with its route
named, the rule each kernel family is judged by -- and, run as a program, the child of its streaming-store test:

    python tests/linear_forms_child.py OUTDIR

runs linear_forms_restated.STREAM_CASES and STREAM_MULTI on the plain operand class in THIS process's environment (the test starts it
with ISG_GEMM_NT_MB=0, which the library reads once, at its first launch), fails unless form() says every one of them streams,
judges each by the same rule as the parent and writes the raw bytes of every result to OUTDIR/<index>.bin.  Not a test module."""
import functools
import os
import sys

import torch

import linear_forms_restated as R

CLASSES = ("plain", "scaled", "exact")
F16, F32 = torch.float16, torch.float32
S_ROWS = 3                       # rows of the row-biased Linear's P


def zero_rows(M, N):
    return M - 2, N - 2          # in the ragged last row tile (its first row) and in the ragged last subtile


def boost_from(K):
    """First column of the block that rows 1, 6, 11, .. of the exact class carry 64 times larger: the second K chunk of
    isg_linear_f16x3_tile where there is one (a chunk scaled by another chunk's row maximum overflows fp16 there), else K / 2."""
    nchunk, step = R.k_chunks(K)
    return step if nchunk > 1 else (K // 2) & ~3


def _act(t, act):
    return torch.nn.functional.gelu(t) if act == 1 else (torch.relu(t) if act == 2 else t)


@functools.lru_cache(maxsize=8)
def operands(M, N, K, cls, a16):
    """CPU operands of a shape and class, the same in every process (seeded), with the fp64 product; nothing writes to them.
    plain: x ~ N(0, 1), w ~ N(0, 1) / sqrt(K); scaled: the rows of x times exp(U(0, 6)) (bench.dense_err_vs_fp32's rows);
    exact: integers in [-4, 4] (bias and P in [-8, 8]), a column block of every fifth row times 64 -- every operand one bf16 plane
    (at most 8 significant bits) and one fp16 plane under a power-of-two row scale, every partial sum below 644 * 4 * 256 < 2^24."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K * 7 + CLASSES.index(cls))
    if cls == "exact":
        x = torch.randint(-4, 5, (M, K), generator=g).float()
        w = torch.randint(-4, 5, (N, K), generator=g).float()
        b = torch.randint(-8, 9, (N,), generator=g).float()
        P = torch.randint(-8, 9, (S_ROWS, N), generator=g).float()
        x[1::5, boost_from(K):] *= 64.0
    else:
        x = torch.randn(M, K, generator=g)
        if cls == "scaled":
            x = x * torch.rand(M, 1, generator=g).mul(6).exp()
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g)
        P = torch.randn(S_ROWS, N, generator=g)
    seg = torch.sort(torch.randint(0, S_ROWS, (M,), generator=g)).values.int()
    zx, zw = zero_rows(M, N)
    x[zx] = 0.0
    w[zw] = 0.0
    if a16:
        x = x.half()
    return dict(x=x, w=w, b=b, P=P, seg=seg, prod64=x.double() @ w.double().t())


def run_case(c, cls, dev, route=None):
    """The case through its Python launcher with the route named (weight splitting and the plane cache on the path); returns the
    result on the device (the f16x3 tile kernel's row maxima ride on it: ops.row_maxima)."""
    from isubgvqa_amd import ops
    o = operands(c.M, c.N, c.K, cls, c.a16)
    route = c.route if route is None else route
    x, w = o["x"].to(dev), o["w"].to(dev)
    b = o["b"].to(dev) if c.bias else None
    gelu, relu = c.act == 1, c.act == 2
    before = ops.COUNTERS["torch_linear"]
    with torch.no_grad():
        if route == "skinny":
            y = ops.linear_skinny(x, w, b, gelu=gelu, relu=relu)
            assert y is not None, "isg_linear_skinny refused a layout it documents"
        elif route == "rowbias":
            y = ops.linear_rowbias(x, w, o["P"].to(dev), o["seg"].to(dev), gelu=gelu, relu=relu, out_dtype=F16 if c.d16 else F32)
        else:
            y = ops._launch(route, x, w, b, gelu, relu, True, F16 if (c.d16 and route != "f16x3") else F32, c.rowmax_out)
    assert y.shape == (c.M, c.N) and y.dtype == (F16 if (c.d16 and route != "f16x3") else F32)
    assert ops.COUNTERS["torch_linear"] == before, "the launcher fell back to hipBLASLt"
    return y


def reference(c, cls):
    """(the fp64 reference, torch's fp32 Linear on the CPU on the same operands, the bias term as fp64 [.., N])."""
    o = operands(c.M, c.N, c.K, cls, c.a16)
    xf = o["x"].float()
    if c.route == "rowbias":
        term = o["P"][o["seg"].long()]
        base = torch.nn.functional.linear(xf, o["w"]) + term
    else:
        term = o["b"] if c.bias else torch.zeros(c.N)
        base = torch.nn.functional.linear(xf, o["w"], o["b"] if c.bias else None)
    return _act(o["prod64"] + term.double(), c.act), _act(base, c.act), term.double()


def bound_factor(c):
    """The factor on the fp32 GEMM's error each kernel's own test holds it to (tests/test_gpu_ops.py)."""
    return 6.0 if c.route == "panel" and c.K > 256 else 2.0


def judge(c, cls, got, twin=None):
    """(passed, figures, why not) of a result by its family's rule.  got: the result on the CPU; twin: for f16x3_f16 the fp32 result
    of the same case on isg_linear_f16x3.
      exact class (no GELU: the activation must be exact too): the int64 product, bit for bit (a half result: rounded once).
      fp32 result of fp32 rows: err <= max(factor * e32, 1e-6); plain: err, e32 = the largest |. - ref64| over the matrix; scaled:
        the largest over the rows of (the row's largest |. - ref64|) / (the row's largest |ref64|) -- a small row counts as a large one.
      fp32 result of half rows (test_linear_bf16x6_fp16_io): err < 2e-6 max(1, max |ref64|); scaled: row by row.
      half result of the bf16 kernels (the same test): |got - half(ref64)| <= max(|.|, 6.1e-5) 2^-10 + 4e-6 elementwise.  The 4e-6
        is that test's allowance for the fp32 summation noise that decides the rounding of entries near zero, stated for rows of
        magnitude ~1; it grows with the row like the noise does, so the scaled class, judged row by row, takes
        4e-6 max(1, the row's largest |ref64|).  (With the constant, torch's own fp32 Linear on the CPU, rounded to half, misses the
        rule on 51 of the 225 scaled half-result cases, by up to 16.3 times the step, each time at an entry below 0.03 of a row whose
        largest is 75 .. 780 -- and on none of the plain class; the kernels: 45 cases, up to 11.9.)
      half result of isg_linear_f16x3_f16 (test_linear_f16x3_half_rows_are_the_fp32_result_rounded_once): the twin rounded to half,
        bit for bit.
    A zero row of x and a zero row of w give act(bias term) exactly (no GELU)."""
    ref, base, term = reference(c, cls)
    fig = {}
    if not torch.isfinite(got.float()).all() and cls != "exact":
        return False, fig, "a non-finite result"
    zx, zw = zero_rows(c.M, c.N)
    if c.act != 1:
        want = _act(term, c.act).float()
        want = want.half() if c.d16 else want
        wz = want.expand(c.M, c.N)
        if not (torch.equal(got[zx], wz[zx]) and torch.equal(got[:, zw], wz[:, zw])):
            return False, fig, "a zero row of x or w does not give act(bias) exactly"
    if cls == "exact":
        assert c.act != 1
        want = ref.float().half() if c.d16 else ref.float()
        assert c.d16 or torch.equal(want.double(), ref), "the exact class left the integers fp32 holds"
        bad = (got != want).sum().item()
        fig["mismatches"] = bad
        return bad == 0, fig, f"{bad} elements differ from the integer product"
    if c.route == "f16x3_f16":
        bad = (got.view(torch.int16) != twin.half().view(torch.int16)).sum().item()
        fig["mismatches"] = bad
        return bad == 0, fig, f"{bad} elements are not the fp32 result rounded once"
    if c.d16:
        r = ref.float().half().float()
        noise = 4e-6 * ref.abs().amax(dim=1, keepdim=True).clamp_min(1.0).float() if cls == "scaled" else 4e-6
        ulp = torch.maximum(r.abs(), torch.tensor(6.1e-5)) * 2.0 ** -10 + noise
        worst = ((got.float() - r).abs() / ulp).max().item()
        fig["half_steps"] = worst
        return worst <= 1.0, fig, f"{worst:.2f} of the allowed half step"
    diff, d32 = (got.double() - ref).abs(), (base.double() - ref).abs()
    if cls == "scaled":
        scale = ref.abs().amax(dim=1).clamp_min(1e-30)
        err, e32 = (diff.amax(dim=1) / scale).max().item(), (d32.amax(dim=1) / scale).max().item()
    else:
        err, e32 = diff.max().item(), d32.max().item()
    fig.update(err=err, e32=e32, ratio=err / max(e32, 1e-30))
    if c.a16:
        if cls == "scaled":
            lim = 2e-6 * ref.abs().amax(dim=1).clamp_min(1.0)
            worst = (diff.amax(dim=1) / lim).max().item()
        else:
            worst = err / (2e-6 * max(1.0, ref.abs().max().item()))
        fig["of_bound"] = worst
        return worst < 1.0, fig, f"{worst:.2f} of 2e-6 max(1, |ref|)"
    f = bound_factor(c)
    return err <= max(f * e32, 1e-6), fig, f"err {err:.3e} > max({f} x {e32:.3e}, 1e-6)"


def run_and_judge(c, cls, dev):
    """Launch, judge, print the figures; returns (the result on the device, passed, figures, why not)."""
    y = run_case(c, cls, dev)
    twin = run_case(c, cls, dev, route="f16x3").cpu() if c.route == "f16x3_f16" and cls != "exact" else None
    ok, fig, why = judge(c, cls, y.cpu(), twin)
    if c.rowmax_out:
        from isubgvqa_amd import ops
        rm = ops.row_maxima(y)
        want = torch.stack([y[:, s:s + 32].abs().amax(1) for s in range(0, c.N, 32)], 1)
        if rm is None or not torch.equal(rm.view(torch.int32), want.view(torch.int32)):
            ok, why = False, "d_rowmax is not the maxima of the stored rows"
    print(f"linear forms {cls} {R.case_id(c)}: " + " ".join(f"{k} {v:.3g}" for k, v in fig.items()) + ("" if ok else f"  FAILS: {why}"))
    return y, ok, fig, why


def multi_switches(route):
    """The switches under which ops.linear_multi takes `route` at a few rows (linear_route's row thresholds are the product's)."""
    return dict(gemm_kernel="panel", gemm_f16x3=route != "panel")


def run_multi(m, dev):
    """A multi-output launch through ops.linear_multi; returns (outputs on the device, [(passed, figures, why not)] per output)."""
    from isubgvqa_amd import ops
    route, M, n, L, K, a16, d16 = m
    o = operands(M, n * L, K, "plain", a16)
    x = o["x"].to(dev)
    ws = [o["w"][i * n:(i + 1) * n].contiguous().to(dev) for i in range(L)]
    with torch.no_grad(), ops.configured(**multi_switches(route)):
        assert ops.linear_route(M, n * L, K, x.dtype, F16 if d16 else F32) == route, m
        outs = ops.linear_multi(x, ws, out_dtype=F16 if d16 else F32)
        assert outs is not None and len(outs) == L, m
        twins = ops.linear_multi(x, ws) if route == "f16x3_f16" else None
    verdicts = []
    whole = R.Case(route, M, n * L, K, 0, a16, d16, False, False)
    got = torch.cat([t.cpu() for t in outs], dim=1)
    twin = torch.cat([t.cpu() for t in twins], dim=1) if twins is not None else None
    ok, fig, why = judge(whole, "plain", got, twin)
    print(f"linear forms multi {route} {M}x{L}*{n}x{K} {'h' if a16 else 'f'}{'h' if d16 else 'f'}: " +
          " ".join(f"{k} {v:.3g}" for k, v in fig.items()) + ("" if ok else f"  FAILS: {why}"))
    verdicts.append((ok, fig, why))
    return outs, verdicts


def stream_results(dev):
    """Every streaming case's result as raw bytes, in a fixed order: (name, bytes, passed, why not)."""
    out = []
    for c in R.STREAM_CASES:
        y, ok, _, why = run_and_judge(c, "plain", dev)
        out.append((R.case_id(c), y.cpu().contiguous().view(torch.uint8).numpy().tobytes(), ok, why))
    for m in R.STREAM_MULTI:
        outs, verdicts = run_multi(m, dev)
        raw = b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in outs)
        out.append(("multi-" + "-".join(map(str, m)), raw, all(v[0] for v in verdicts), "; ".join(v[2] for v in verdicts if not v[0])))
    return out


def main(argv):
    outdir = argv[1]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env = {k: v for k, v in os.environ.items() if k.startswith("ISG_")}
    assert torch.cuda.is_available(), "the child needs the GPU"
    for c in R.STREAM_CASES:
        assert R.case_form(c, env).streaming, f"{R.case_id(c)} does not stream under {env}"
    for r, M, n, L, K, a16, d16 in R.STREAM_MULTI:
        assert R.form(r, M, n * L, K, 0, a16, d16, ldd=n, env=env, out_cols=n).streaming
    from isubgvqa_amd import _lib
    _lib.load()
    failed = []
    for i, (name, raw, ok, why) in enumerate(stream_results(torch.device("cuda:0"))):
        with open(os.path.join(outdir, f"{i}.bin"), "wb") as f:
            f.write(raw)
        if not ok:
            failed.append(f"{name}: {why}")
    torch.cuda.synchronize()
    if failed:
        print("streaming child: " + "\n".join(failed))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
