"""The training graph's recipes, pinned on the CPU: which ops.* functions each autograd node of autograd.py calls, in which order
and with which operands (A), and which arguments ops.gatv2_mp_backward / ops.gatv2_mp_backward_f16 hand to the C entry points,
position by position (B).  Nothing here needs a GPU or the built library: the ops.* functions are stood in for by torch, the C
entry points by recorders.  The tables are literal: a change to a call, its order, an operand's shape, stride or dtype, a keyword or
the linear_bwd_kernels counter shows up as a diff against them."""
import types

import pytest
import torch
import torch.nn.functional as F

from isubgvqa_amd import autograd, ops

DT = {torch.float32: "f32", torch.float16: "f16", torch.int32: "i32", torch.int64: "i64", torch.bool: "b8"}


# ------------------------------------------------------------------------------------------------
# A. Call traces
# ------------------------------------------------------------------------------------------------
def _desc(v):
    """(shape, stride, dtype) of a tensor; a plain value as it is; a plan by name."""
    if isinstance(v, torch.Tensor):
        return tuple(v.shape), tuple(v.stride()), v.dtype
    if isinstance(v, types.SimpleNamespace):
        return "plan"
    return v


def _show(d):
    if isinstance(d, tuple) and len(d) == 3 and isinstance(d[2], torch.dtype):
        return f"{DT[d[2]]}{list(d[0])}/{list(d[1])}".replace(" ", "")
    return repr(d)


def _expand(names):
    """The rendered trace a table row stands for: its words are keys of CALLS (at the end of the file)."""
    return [CALLS[n] for n in names.split()]


def _render(trace):
    """One line per recorded call: name(positional, ...; keyword=value, ...)."""
    return [f"{name}({', '.join(_show(a) for a in args)}{'; ' if kw else ''}{', '.join(f'{k}={_show(v)}' for k, v in kw)})"
            for name, args, kw in trace]


class Plan(types.SimpleNamespace):
    pass


PLAN = Plan(N=5, E=7)
H, C = 2, 4
HC = H * C


def _mp_forward(x_l, x_r, e_proj, att, plan, heads, bias=None, node_mask=None, edge_mask=None, negative_slope=0.2, kernel=None,
                dropout_p=0.0, dropout_seed=0):
    out = (x_l.float() + 2 * x_r.float()).to(x_l.dtype)
    return out, torch.full((plan.E, heads), 0.5)


def _mp_backward(x_l, x_r, e_proj, att, alpha, grad_out, plan, heads, node_mask=None, edge_mask=None, negative_slope=0.2,
                 want_mask_grad=False, dropout_p=0.0, dropout_seed=0, d_x_lr=None):
    n, hc = x_l.shape
    d_xl, d_xr = grad_out * 1.0, grad_out * 2.0
    if d_x_lr is not None:
        d_x_lr[:, :hc], d_x_lr[:, hc:] = d_xl, d_xr
        d_xl, d_xr = d_x_lr[:, :hc], d_x_lr[:, hc:]
    d_e = torch.arange(plan.E * hc, dtype=torch.float32).view(plan.E, hc) / 7
    d_m = torch.arange(plan.E, dtype=torch.float32) if want_mask_grad else None
    return d_xl, d_xr, d_e, torch.full((hc,), 3.0), grad_out.sum(0), d_m


def _prep(g, saved, mode, want_dz=True, want_db=True):
    dz = g if mode == 0 else torch.ops.aten.gelu_backward(g, saved) if mode == 1 else g * (saved > 0)
    return (dz.contiguous() if want_dz else None), (dz.sum(0) if want_db else None)


def _act(z, gelu, relu):
    return F.gelu(z) if gelu else torch.relu(z) if relu else z


STANDINS = {
    "linear": lambda x, w, b=None, gelu=False, cache_planes=True, relu=False, out_dtype=torch.float32:
        _act(F.linear(x.float(), w, b), gelu, relu).to(out_dtype),
    "linear_rowbias": lambda x, w, P, seg, gelu=False, relu=False, cache_planes=True:
        _act(F.linear(x, w) + P[seg.long()], gelu, relu),
    "linear_bwd_prep": _prep,
    "linear_wgrad": lambda g, x: g.t() @ x,
    "linear_wgrad_bf16x6": lambda g, x: g.t() @ x,
    "segment_rowptr": lambda seg, S: torch.searchsorted(seg, torch.arange(S + 1, dtype=seg.dtype)).int(),
    "segment_range_sum": lambda rowptr, G: torch.stack([G[int(rowptr[s]):int(rowptr[s + 1])].sum(0)
                                                        for s in range(rowptr.numel() - 1)]),
    "gatv2_mp": _mp_forward,
    "gatv2_mp_backward_f16": _mp_backward,
    "gatv2_mp_backward": _mp_backward,
    "node_to_edge_mask_backward": lambda d_m, plan: torch.arange(plan.N, dtype=torch.float32) + d_m.sum(),
}


@pytest.fixture
def trace(monkeypatch):
    """The list every stood-in ops.* function appends (name, per-argument description, sorted keywords) to."""
    calls = []

    def recorded(name, fn):
        def call(*a, **k):
            calls.append((name, tuple(_desc(v) for v in a), tuple(sorted((key, _desc(v)) for key, v in k.items()))))
            return fn(*a, **k)
        return call

    for name, fn in STANDINS.items():
        monkeypatch.setattr(ops, name, recorded(name, fn))
    monkeypatch.setattr(autograd, "WGRAD_MIN_ROWS", 4)
    return calls


def _upstream(shape, variant, gen):
    """The upstream gradient: contiguous, a column slice of a wider tensor (rows strided), or a transposed tensor."""
    M, N = shape
    if variant == "slice":
        return torch.randn(M, 2 * N, generator=gen)[:, N:]
    if variant == "t":
        return torch.randn(N, M, generator=gen).t()
    return torch.randn(M, N, generator=gen)


def _close(got, ref):
    assert (got is None) == (ref is None)
    if ref is not None:
        assert got.shape == ref.shape and torch.allclose(got, ref, rtol=1e-5, atol=1e-5)


MODES = {"identity": (False, False), "gelu": (True, False), "relu": (False, True)}

# (mode, switch, M, N, upstream gradient, bias, gradients wanted): every mode under both switch states with every upstream layout;
# then, from those, one step to each of: rows below WGRAD_MIN_ROWS, N % 4 != 0, no bias, x only, weight only.
LINEAR_CASES = ([(m, s, 9, 12, u, True, "all") for m in MODES for s in (True, False) for u in ("contiguous", "slice", "t")] +
                [(m, s, 3, 12, "contiguous", True, "all") for m in ("identity", "gelu") for s in (True, False)] +
                [(m, s, 9, 10, u, True, "all") for m, u in (("identity", "slice"), ("relu", "contiguous")) for s in (True, False)] +
                [(m, s, 9, 12, "slice", False, "all") for m in ("identity", "gelu") for s in (True, False)] +
                [(m, s, 9, 12, "contiguous", True, w) for m in ("identity", "gelu") for s in (True, False) for w in ("x", "w")])


def _id(case):
    return "-".join(str(c) for c in case)


def _run_linear(case, calls, monkeypatch):
    mode, switch, M, N, variant, bias, wants = case
    gelu, relu = MODES[mode]
    monkeypatch.setattr(autograd, "LINEAR_BWD_KERNELS", switch)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(M, 8, generator=gen, requires_grad=wants in ("all", "x"))
    w = torch.randn(N, 8, generator=gen, requires_grad=wants in ("all", "w"))
    b = torch.randn(N, generator=gen, requires_grad=wants == "all") if bias else None
    go = _upstream((M, N), variant, gen)
    before = ops.COUNTERS["linear_bwd_kernels"]
    autograd.linear(x, w, b, gelu, relu=relu).backward(go)
    delta = ops.COUNTERS["linear_bwd_kernels"] - before
    ref = [None if t is None else t.detach().clone().requires_grad_(t.requires_grad) for t in (x, w, b)]
    _act(F.linear(*ref), gelu, relu).backward(go)
    for got, want in zip((x, w, b), ref):
        if got is not None:
            _close(got.grad, want.grad)
    return delta, _render(calls)


@pytest.mark.parametrize("case", LINEAR_CASES, ids=_id)
def test_linear_backward_trace(case, trace, monkeypatch):
    delta, calls = LINEAR_TRACES[_id(case)]
    assert _run_linear(case, trace, monkeypatch) == (delta, _expand(calls))


# (mode, rowptr given, switch): the row-biased Linear runs the kernel path whatever the switch says and never counts.
ROWBIAS_CASES = [(m, r, s) for m in MODES for r in (True, False) for s in (True, False)]


def _run_rowbias(case, calls, monkeypatch):
    mode, given, switch = case
    gelu, relu = MODES[mode]
    monkeypatch.setattr(autograd, "LINEAR_BWD_KERNELS", switch)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(9, 8, generator=gen, requires_grad=True)
    w = torch.randn(12, 8, generator=gen, requires_grad=True)
    P = torch.randn(3, 12, generator=gen, requires_grad=True)
    seg = torch.tensor([0, 0, 0, 0, 1, 2, 2, 2, 2], dtype=torch.int32)
    rowptr = torch.tensor([0, 4, 5, 9], dtype=torch.int32) if given else None
    go = torch.randn(9, 24, generator=gen)[:, :12]
    before = ops.COUNTERS["linear_bwd_kernels"]
    autograd.linear_rowbias(x, w, P, seg, gelu, relu, rowptr).backward(go)
    delta = ops.COUNTERS["linear_bwd_kernels"] - before
    ref = [t.detach().clone().requires_grad_(True) for t in (x, w, P)]
    _act(F.linear(ref[0], ref[1]) + ref[2][seg.long()], gelu, relu).backward(go)
    for got, want in zip((x, w, P), ref):
        _close(got.grad, want.grad)
    return delta, _render(calls)


@pytest.mark.parametrize("case", ROWBIAS_CASES, ids=_id)
def test_linear_rowbias_backward_trace(case, trace, monkeypatch):
    got = _run_rowbias(case, trace, monkeypatch)
    assert got[0] == 0
    assert got[1] == _expand(ROWBIAS_TRACES[_id(case[:2])][1])         # one row for both states of the switch


# (lin_r, biases, mask, switch)
CONV_CASES = ([(r, "both", k, s) for r in ("shared", "distinct") for k in ("none", "node", "edge") for s in (True, False)] +
              [(r, b, "none", s) for r in ("shared", "distinct") for b in ("left", "neither") for s in (True, False)])


def _masks(mask, gen):
    node = torch.rand(PLAN.N, generator=gen, requires_grad=True) if mask == "node" else None
    edge = torch.rand(PLAN.E, generator=gen, requires_grad=True) if mask == "edge" else None
    return node, edge


def _run_conv(case, calls, monkeypatch):
    lin_r, biases, mask, switch = case
    monkeypatch.setattr(autograd, "LINEAR_BWD_KERNELS", switch)
    gen = torch.Generator().manual_seed(2)
    K, KE = 12, 8
    x = torch.randn(PLAN.N, K, generator=gen, requires_grad=True)
    ea = torch.randn(PLAN.E, KE, generator=gen, requires_grad=True)

    def lin(has_bias):
        m = torch.nn.Linear(K, HC, bias=has_bias)
        with torch.no_grad():
            m.weight.copy_(torch.randn(HC, K, generator=gen))
            if has_bias:
                m.bias.copy_(torch.randn(HC, generator=gen))
        return m
    lin_l = lin(biases in ("both", "left"))
    lr = None if lin_r == "shared" else lin(biases == "both")
    w_e = torch.randn(HC, KE, generator=gen, requires_grad=True)
    att = torch.randn(1, H, C, generator=gen, requires_grad=True)
    bias = torch.randn(HC, generator=gen, requires_grad=True)
    node, edge = _masks(mask, gen)
    go = torch.randn(PLAN.N, HC, generator=gen)
    before = ops.COUNTERS["linear_bwd_kernels"]
    out, _alpha = autograd.conv_half_rows(x, ea, lin_l, lr, w_e, att, bias, node, edge, PLAN, H, 0.2)
    out.backward(go)
    delta = ops.COUNTERS["linear_bwd_kernels"] - before
    # what the stood-in message passing hands back, through the two Linears by hand
    g = torch.cat([go, 2 * go], dim=1) if lr is not None else 3 * go
    wcat = lin_l.weight.detach() if lr is None else torch.cat([lin_l.weight.detach(), lr.weight.detach()])
    d_e = torch.arange(PLAN.E * HC, dtype=torch.float32).view(PLAN.E, HC) / 7
    _close(x.grad, g @ wcat)
    _close(ea.grad, d_e @ w_e.detach())
    _close(w_e.grad, d_e.t() @ ea.detach())
    dw, db = g.t() @ x.detach(), g.sum(0)
    _close(lin_l.weight.grad, dw[:HC])
    _close(lin_l.bias.grad if lin_l.bias is not None else None, db[:HC] if lin_l.bias is not None else None)
    if lr is not None:
        _close(lr.weight.grad, dw[HC:])
        _close(lr.bias.grad if lr.bias is not None else None, db[HC:] if lr.bias is not None else None)
    _close(att.grad, torch.full((1, H, C), 3.0))
    _close(bias.grad, go.sum(0))
    d_m = torch.arange(PLAN.E, dtype=torch.float32)
    _close(None if node is None else node.grad, None if node is None else torch.arange(PLAN.N, dtype=torch.float32) + d_m.sum())
    _close(None if edge is None else edge.grad, None if edge is None else d_m)
    return delta, _render(calls)


@pytest.mark.parametrize("case", CONV_CASES, ids=_id)
def test_conv_half_rows_trace(case, trace, monkeypatch):
    got = _run_conv(case, trace, monkeypatch)
    assert got[0] == (2 if case[3] else 0)
    assert got == (CONV_TRACES[_id(case)][0], _expand(CONV_TRACES[_id(case)][1]))


def _run_mp(mask, calls):
    gen = torch.Generator().manual_seed(3)
    x_l = torch.randn(PLAN.N, HC, generator=gen, requires_grad=True)
    x_r = torch.randn(PLAN.N, HC, generator=gen, requires_grad=True)
    e = torch.randn(PLAN.E, HC, generator=gen, requires_grad=True)
    att = torch.randn(1, H, C, generator=gen, requires_grad=True)
    bias = torch.randn(HC, generator=gen, requires_grad=True)
    node, edge = _masks(mask, gen)
    go = torch.randn(PLAN.N, HC, generator=gen)
    out, _alpha = autograd.gatv2_mp(x_l, x_r, e, att, PLAN, H, bias, node, edge, 0.2, None, 0.25, 7)
    out.backward(go)
    d_m = torch.arange(PLAN.E, dtype=torch.float32)
    _close(x_l.grad, go)
    _close(x_r.grad, 2 * go)
    _close(e.grad, torch.arange(PLAN.E * HC, dtype=torch.float32).view(PLAN.E, HC) / 7)
    _close(att.grad, torch.full((1, H, C), 3.0))
    _close(bias.grad, go.sum(0))
    _close(None if node is None else node.grad, None if node is None else torch.arange(PLAN.N, dtype=torch.float32) + d_m.sum())
    _close(None if edge is None else edge.grad, None if edge is None else d_m)
    return _render(calls)


@pytest.mark.parametrize("mask", ["none", "node", "edge"])
def test_gatv2_mp_trace(mask, trace):
    assert _run_mp(mask, trace) == _expand(MP_TRACES[mask])


def test_simple_topk_falls_back_to_the_restatement(monkeypatch):
    """A row the backward kernel refuses (ops.simple_topk_backward returns None): the gradient is autograd's through
    _simple_restatement -- the same torch graph on the CPU, so to 0 ulp."""
    B, Nmax, k = 2, 5, 2
    gen = torch.Generator().manual_seed(4)
    asked = []
    monkeypatch.setattr(autograd, "SIMPLE_BWD_KERNEL", True)
    monkeypatch.setattr(ops, "simple_topk", lambda sc, k, plan, uniform, seed, rm:
                        (torch.zeros_like(sc), torch.zeros_like(sc)) if rm else torch.zeros_like(sc))
    monkeypatch.setattr(ops, "simple_topk_backward", lambda *a: asked.append(tuple(_desc(v) for v in a)))
    for return_marginals, use in ((False, "out"), (True, "both"), (True, "marginals")):
        scores = torch.randn(B, Nmax, generator=gen, requires_grad=True)
        g_out, g_marg = torch.randn(B, Nmax, generator=gen), torch.randn(B, Nmax, generator=gen)
        res = autograd.simple_topk(scores, k, None, None, 0, return_marginals)
        outs = res if return_marginals else (res,)
        pairs = [(o, g) for o, g, name in zip(outs, (g_out, g_marg), ("out", "marginals")) if use in (name, "both")]
        got, = torch.autograd.grad([o for o, _ in pairs], [scores], [g for _, g in pairs])
        sc = scores.detach().clone().requires_grad_(True)
        ref_outs = autograd._simple_restatement(sc, k, None, return_marginals)(sc)
        ref_outs = ref_outs if return_marginals else (ref_outs,)
        pairs = [(o, g) for o, g, name in zip(ref_outs, (g_out, g_marg), ("out", "marginals")) if use in (name, "both")]
        ref, = torch.autograd.grad([o for o, _ in pairs], [sc], [g for _, g in pairs])
        assert torch.equal(got, ref) and bool(got.abs().sum() > 0)
    f = ((B, Nmax), (Nmax, 1), torch.float32)
    assert asked == [(f, k, None, f, None), (f, k, None, f, f), (f, k, None, None, f)]


@pytest.mark.parametrize("has_bias", [(True, False, True), (False, False, False)], ids=["some-biases", "no-bias"])
@pytest.mark.parametrize("training", [True, False])
def test_linear_fused_weight_bias_and_cache_key(training, has_bias, monkeypatch):
    """ops.linear_fused hands ops.linear the weights stacked along the output dim and the biases in a row, zeros for a layer without
    one (None when no layer has one); in inference that pair is a derived weight under the tag "linear_fused", its sources the
    weights and then the biases there are; under autograd nothing is cached."""
    gen = torch.Generator().manual_seed(6)
    layers = []
    for n, hb in zip((4, 3, 5), has_bias):
        m = torch.nn.Linear(6, n, bias=hb).requires_grad_(training)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen))
        layers.append(m)
    seen, cached = [], []
    real_derived = ops.derived_weight
    monkeypatch.setattr(ops, "linear", lambda x, w, b, **k: seen.append((w, b, k)) or F.linear(x, w, b))
    monkeypatch.setattr(ops, "derived_weight", lambda tag, sources, build: cached.append((tag, sources)) or real_derived(tag, sources, build))
    outs = ops.linear_fused(torch.randn(2, 6, generator=gen), layers)
    (w, b, kw), = seen
    assert torch.equal(w, torch.cat([m.weight for m in layers]))
    if any(has_bias):
        assert torch.equal(b, torch.cat([m.bias if m.bias is not None else torch.zeros(m.out_features) for m in layers]))
    else:
        assert b is None
    assert [(tuple(o.shape), o.stride(), o.storage_offset()) for o in outs] == [((2, 4), (12, 1), 0), ((2, 3), (12, 1), 4), ((2, 5), (12, 1), 7)]
    if training:
        assert not cached and kw == {} and w.requires_grad
    else:
        (tag, sources), = cached
        assert tag == "linear_fused" and kw == {"out_dtype": torch.float32} and not w.requires_grad
        assert [id(s) for s in sources] == [id(m.weight) for m in layers] + [id(m.bias) for m in layers if m.bias is not None]


# ------------------------------------------------------------------------------------------------
# B. The C calls of the message-passing backward, argument by argument
# ------------------------------------------------------------------------------------------------
MP_N, MP_E = 4, 6
STREAM = 0x5EA


class _Entries:
    """Stands in for a loaded library: the three backward entry points record their positional arguments and return 0."""

    def __init__(self, calls):
        for name in ("isg_gatv2_mp_bwd", "isg_gatv2_mp_bwd_dropout", "isg_gatv2_mp_bwd_f16"):
            setattr(self, name, lambda *a, _n=name: calls.append((_n, a)) or 0)


@pytest.fixture
def c_calls(monkeypatch):
    from isubgvqa_amd import _lib, _lib_mp_f16_train, _lib_mp_train
    calls = []

    def chk(t, name, dtype, shape=None, optional=False):
        if t is None:
            assert optional, name
            return 0
        assert t.dtype == dtype and t.is_contiguous() and (shape is None or tuple(t.shape) == tuple(shape)), name
        return t.data_ptr()

    def chk_rows(t, name, dtype=torch.float32):
        assert t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1 and not (t.stride(0) & 3), name
        return t.data_ptr()

    monkeypatch.setattr(ops, "_chk", chk)
    monkeypatch.setattr(ops, "_chk_rows", chk_rows)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    for mod in (_lib, _lib_mp_train, _lib_mp_f16_train):
        monkeypatch.setattr(mod, "load", lambda: _Entries(calls))
    return calls


def _c_plan(E):
    i32 = lambda n: torch.zeros(max(n, 1), dtype=torch.int32)
    t = {"rowptr": i32(MP_N + 1), "eid": i32(E), "src": i32(E), "rowptr_s": i32(MP_N + 1), "eid_s": i32(E), "dst_s": i32(E)}
    plan = Plan(N=MP_N, E=E, rowptr=t["rowptr"], eid=t["eid"], src=t["src"], require_csr=lambda: None,
                source_csr=lambda: (t["rowptr_s"], t["eid_s"], t["dst_s"]))
    return plan, t


# The operand list of include/isg.h's isg_gatv2_mp_bwd, shared by all three entry points up to the slope; E_PROJ / ALPHA are null
# without edges, NODE / EDGE without that mask, D_M unless the mask gradient is wanted.
COMMON = ["x_l", "x_r", "E_PROJ", "att", "ALPHA", "grad_out", "rowptr", "eid", "src", "rowptr_s", "eid_s", "dst_s", "NODE", "EDGE",
          "d_x_l", "d_x_r", "d_e", "part", "D_M", MP_N, "E", H, C, 0.125]
TAILS = {"isg_gatv2_mp_bwd": [STREAM],
         "isg_gatv2_mp_bwd_dropout": [0.25, 77, STREAM],
         # pitches of x_l, x_r, e_proj, d_x_l, d_x_r: the inputs are column halves of one [N, 2*H*C] half buffer, ...
         "f16 into d_x_lr": [2 * HC, 2 * HC, "LD_E", 2 * HC, 2 * HC, STREAM],      # ... the outputs those of the caller's fp32 one
         "f16": [2 * HC, 2 * HC, "LD_E", HC, HC, STREAM]}                          # ... the outputs tensors of their own


@pytest.mark.parametrize("E", [MP_E, 0])
@pytest.mark.parametrize("want", [False, True])
@pytest.mark.parametrize("masks", ["none", "node", "edge"])
@pytest.mark.parametrize("form", list(TAILS))
def test_mp_backward_c_arguments(form, masks, want, E, c_calls):
    gen = torch.Generator().manual_seed(5)
    plan, named = _c_plan(E)
    half = form.startswith("f16")
    if half:
        x_lr = torch.randn(MP_N, 2 * HC, generator=gen).half()
        e_wide = torch.randn(max(E, 1), 2 * HC, generator=gen).half()[:E]
        x_l, x_r, e_proj = x_lr[:, :HC], x_lr[:, HC:], e_wide[:, :HC]
    else:
        x_l, x_r = torch.randn(MP_N, HC, generator=gen), torch.randn(MP_N, HC, generator=gen)
        e_proj = torch.randn(max(E, 1), HC, generator=gen)[:E]
    att = torch.randn(1, H, C, generator=gen)
    alpha = torch.rand(max(E, 1), H, generator=gen)[:E]
    grad_out = torch.randn(MP_N, HC, generator=gen)
    node_mask = torch.rand(MP_N, 1, generator=gen) if masks == "node" else None
    edge_mask = torch.rand(max(E, 1), generator=gen)[:E] if masks == "edge" else None
    named.update(x_l=x_l, x_r=x_r, e_proj=e_proj, att=att, alpha=alpha, grad_out=grad_out, node_mask=node_mask, edge_mask=edge_mask)
    kw = dict(node_mask=node_mask, edge_mask=edge_mask, negative_slope=0.125, want_mask_grad=want)
    before = ops.COUNTERS["mp_f16_train"]
    buf = None
    if form == "isg_gatv2_mp_bwd":
        res = ops.gatv2_mp_backward(x_l, x_r, e_proj, att, alpha, grad_out, plan, H, **kw)
    elif form == "isg_gatv2_mp_bwd_dropout":
        res = ops.gatv2_mp_backward(x_l, x_r, e_proj, att, alpha, grad_out, plan, H, dropout_p=0.25, dropout_seed=77, **kw)
    else:
        buf = torch.full((MP_N, 2 * HC), 9.0) if form == "f16 into d_x_lr" else None
        res = ops.gatv2_mp_backward_f16(x_l, x_r, e_proj, att, alpha, grad_out, plan, H, d_x_lr=buf, **kw)
    assert ops.COUNTERS["mp_f16_train"] - before == (1 if half else 0)
    d_x_l, d_x_r, d_e, d_att, d_bias, d_m = res
    assert [tuple(t.shape) for t in (d_x_l, d_x_r, d_e, d_att, d_bias)] == [(MP_N, HC), (MP_N, HC), (E, HC), (HC,), (HC,)]
    assert (d_m is None) == (not want) and (d_m is None or tuple(d_m.shape) == (E,))
    assert torch.equal(d_bias, grad_out.sum(0))
    if buf is not None:      # the two output pointers are the caller's buffer and the buffer plus 4*H*C bytes
        assert d_x_l.data_ptr() == buf.data_ptr() and d_x_r.data_ptr() == buf.data_ptr() + 4 * HC
        assert d_x_l.stride() == d_x_r.stride() == (2 * HC, 1)
    named.update(d_x_l=d_x_l, d_x_r=d_x_r, d_e=d_e, d_m=d_m)
    names = {t.data_ptr(): n for n, t in named.items() if t is not None and t.data_ptr() != 0}
    assert len(names) == sum(t is not None and t.data_ptr() != 0 for t in named.values()), "two operands share an address"
    (entry, args), = c_calls
    assert entry == ("isg_gatv2_mp_bwd_f16" if half else form)
    got = [names.get(a, a) if i < 19 else a for i, a in enumerate(args)]
    assert isinstance(got[17], int) and got[17] != 0, "the partial sums' buffer"        # freed by now: the one unnamed pointer
    got[17] = "part"
    fill = {"E_PROJ": "e_proj" if E else 0, "ALPHA": "alpha" if E else 0, "NODE": "node_mask" if masks == "node" else 0,
            "EDGE": "edge_mask" if masks == "edge" and edge_mask.data_ptr() else 0,
            "d_e": "d_e" if d_e.data_ptr() else 0, "D_M": "d_m" if want and d_m.data_ptr() else 0, "E": E,
            "LD_E": 2 * HC if E > 1 else HC if E else 0}
    assert got == [fill.get(v, v) if isinstance(v, str) else v for v in COMMON + TAILS[form]]


def test_mp_backward_f16_single_edge_pitch(c_calls):
    """A single row has no pitch to speak of: H*C is passed, whatever the tensor's stride says."""
    plan, _ = _c_plan(1)
    x = torch.zeros(MP_N, 2 * HC).half()
    ops.gatv2_mp_backward_f16(x[:, :HC], x[:, HC:], torch.zeros(1, 2 * HC).half()[:, :HC], torch.zeros(HC), torch.zeros(1, H),
                              torch.zeros(MP_N, HC), plan, H)
    assert c_calls[0][1][24:] == (2 * HC, 2 * HC, HC, HC, HC, STREAM)


# ------------------------------------------------------------------------------------------------
# The tables of A: every distinct recorded call under a short name, then per case (counter delta, the calls in order)
# ------------------------------------------------------------------------------------------------
CALLS = {
    'linear.1': 'linear(f32[9,8]/[8,1], f32[12,8]/[8,1], f32[12]/[1]; cache_planes=False, gelu=False, relu=False)',
    'linear_bwd_prep.1': 'linear_bwd_prep(f32[9,12]/[12,1], None, 0; want_db=True, want_dz=False)',
    'linear.2': 'linear(f32[9,12]/[12,1], f32[8,12]/[12,1], None; cache_planes=False)',
    'linear_wgrad_bf16x6.1': 'linear_wgrad_bf16x6(f32[9,12]/[12,1], f32[9,8]/[8,1])',
    'linear_bwd_prep.2': 'linear_bwd_prep(f32[9,12]/[24,1], None, 0; want_db=True, want_dz=False)',
    'linear_wgrad.1': 'linear_wgrad(f32[9,12]/[12,1], f32[9,8]/[8,1])',
    'linear_bwd_prep.3': 'linear_bwd_prep(f32[9,12]/[12,1], f32[9,12]/[12,1], 1; want_db=True, want_dz=True)',
    'linear_bwd_prep.4': 'linear_bwd_prep(f32[9,12]/[24,1], f32[9,12]/[12,1], 1; want_db=True, want_dz=True)',
    'linear.3': 'linear(f32[9,8]/[8,1], f32[12,8]/[8,1], f32[12]/[1]; cache_planes=False, gelu=False, relu=True)',
    'linear_bwd_prep.5': 'linear_bwd_prep(f32[9,12]/[12,1], f32[9,12]/[12,1], 2; want_db=True, want_dz=True)',
    'linear_bwd_prep.6': 'linear_bwd_prep(f32[9,12]/[24,1], f32[9,12]/[12,1], 2; want_db=True, want_dz=True)',
    'linear.4': 'linear(f32[3,8]/[8,1], f32[12,8]/[8,1], f32[12]/[1]; cache_planes=False, gelu=False, relu=False)',
    'linear_bwd_prep.7': 'linear_bwd_prep(f32[3,12]/[12,1], None, 0; want_db=True, want_dz=False)',
    'linear.5': 'linear(f32[3,12]/[12,1], f32[8,12]/[12,1], None; cache_planes=False)',
    'linear_bwd_prep.8': 'linear_bwd_prep(f32[3,12]/[12,1], f32[3,12]/[12,1], 1; want_db=True, want_dz=True)',
    'linear.6': 'linear(f32[9,8]/[8,1], f32[10,8]/[8,1], f32[10]/[1]; cache_planes=False, gelu=False, relu=False)',
    'linear_bwd_prep.9': 'linear_bwd_prep(f32[9,10]/[20,1], None, 0; want_db=True, want_dz=False)',
    'linear_wgrad_bf16x6.2': 'linear_wgrad_bf16x6(f32[9,10]/[10,1], f32[9,8]/[8,1])',
    'linear_wgrad.2': 'linear_wgrad(f32[9,10]/[10,1], f32[9,8]/[8,1])',
    'linear.7': 'linear(f32[9,8]/[8,1], f32[10,8]/[8,1], f32[10]/[1]; cache_planes=False, gelu=False, relu=True)',
    'linear_bwd_prep.10': 'linear_bwd_prep(f32[9,10]/[10,1], f32[9,10]/[10,1], 2; want_db=True, want_dz=True)',
    'linear.8': 'linear(f32[9,8]/[8,1], f32[12,8]/[8,1], None; cache_planes=False, gelu=False, relu=False)',
    'linear_bwd_prep.11': 'linear_bwd_prep(f32[9,12]/[24,1], f32[9,12]/[12,1], 1; want_db=False, want_dz=True)',
    'linear_bwd_prep.12': 'linear_bwd_prep(f32[9,12]/[12,1], f32[9,12]/[12,1], 1; want_db=False, want_dz=True)',
    'linear_rowbias.1': 'linear_rowbias(f32[9,8]/[8,1], f32[12,8]/[8,1], f32[3,12]/[12,1], i32[9]/[1]; cache_planes=False, relu=False)',
    'segment_range_sum.1': 'segment_range_sum(i32[4]/[1], f32[9,12]/[12,1])',
    'segment_rowptr.1': 'segment_rowptr(i32[9]/[1], 3)',
    'linear_rowbias.2': 'linear_rowbias(f32[9,8]/[8,1], f32[12,8]/[8,1], f32[3,12]/[12,1], i32[9]/[1]; cache_planes=False, relu=True)',
    'linear_bwd_prep.13': 'linear_bwd_prep(f32[9,12]/[24,1], f32[9,12]/[12,1], 2; want_db=False, want_dz=True)',
    'linear.9': 'linear(f32[5,12]/[12,1], f32[8,12]/[12,1], f32[8]/[1]; cache_planes=False, out_dtype=torch.float16)',
    'linear.10': 'linear(f32[7,8]/[8,1], f32[8,8]/[8,1], None; cache_planes=False, out_dtype=torch.float16)',
    'gatv2_mp.1': (("gatv2_mp(f16[5,8]/[8,1], f16[5,8]/[8,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], edge_mask=None, negative_slope=0.2, "
         'node_mask=None)')),
    'gatv2_mp_backward_f16.1': (("gatv2_mp_backward_f16(f16[5,8]/[8,1], f16[5,8]/[8,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; d_x_lr=None, "
         'edge_mask=None, negative_slope=0.2, node_mask=None, want_mask_grad=False)')),
    'linear_bwd_prep.14': 'linear_bwd_prep(f32[5,8]/[8,1], None, 0; want_db=True, want_dz=False)',
    'linear.11': 'linear(f32[5,8]/[8,1], f32[12,8]/[8,1], None; cache_planes=False)',
    'linear_wgrad_bf16x6.3': 'linear_wgrad_bf16x6(f32[5,8]/[8,1], f32[5,12]/[12,1])',
    'linear.12': 'linear(f32[7,8]/[8,1], f32[8,8]/[8,1], None; cache_planes=False)',
    'linear_wgrad_bf16x6.4': 'linear_wgrad_bf16x6(f32[7,8]/[8,1], f32[7,8]/[8,1])',
    'linear_wgrad.3': 'linear_wgrad(f32[5,8]/[8,1], f32[5,12]/[12,1])',
    'linear_wgrad.4': 'linear_wgrad(f32[7,8]/[8,1], f32[7,8]/[8,1])',
    'gatv2_mp.2': (("gatv2_mp(f16[5,8]/[8,1], f16[5,8]/[8,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], edge_mask=None, negative_slope=0.2, "
         'node_mask=f32[5]/[1])')),
    'gatv2_mp_backward_f16.2': (("gatv2_mp_backward_f16(f16[5,8]/[8,1], f16[5,8]/[8,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; d_x_lr=None, "
         'edge_mask=None, negative_slope=0.2, node_mask=f32[5]/[1], want_mask_grad=True)')),
    'node_to_edge_mask_backward.1': "node_to_edge_mask_backward(f32[7]/[1], 'plan')",
    'gatv2_mp.3': (("gatv2_mp(f16[5,8]/[8,1], f16[5,8]/[8,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], edge_mask=f32[7]/[1], negative_slope=0.2, "
         'node_mask=None)')),
    'gatv2_mp_backward_f16.3': (("gatv2_mp_backward_f16(f16[5,8]/[8,1], f16[5,8]/[8,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; d_x_lr=None, "
         'edge_mask=f32[7]/[1], negative_slope=0.2, node_mask=None, want_mask_grad=True)')),
    'linear.13': 'linear(f32[5,12]/[12,1], f32[16,12]/[12,1], f32[16]/[1]; cache_planes=False, out_dtype=torch.float16)',
    'gatv2_mp.4': (("gatv2_mp(f16[5,8]/[16,1], f16[5,8]/[16,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], edge_mask=None, negative_slope=0.2, "
         'node_mask=None)')),
    'gatv2_mp_backward_f16.4': (("gatv2_mp_backward_f16(f16[5,8]/[16,1], f16[5,8]/[16,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; "
         'd_x_lr=f32[5,16]/[16,1], edge_mask=None, negative_slope=0.2, node_mask=None, want_mask_grad=False)')),
    'linear_bwd_prep.15': 'linear_bwd_prep(f32[5,16]/[16,1], None, 0; want_db=True, want_dz=False)',
    'linear.14': 'linear(f32[5,16]/[16,1], f32[12,16]/[16,1], None; cache_planes=False)',
    'linear_wgrad_bf16x6.5': 'linear_wgrad_bf16x6(f32[5,16]/[16,1], f32[5,12]/[12,1])',
    'linear_wgrad.5': 'linear_wgrad(f32[5,16]/[16,1], f32[5,12]/[12,1])',
    'gatv2_mp.5': (("gatv2_mp(f16[5,8]/[16,1], f16[5,8]/[16,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], edge_mask=None, negative_slope=0.2, "
         'node_mask=f32[5]/[1])')),
    'gatv2_mp_backward_f16.5': (("gatv2_mp_backward_f16(f16[5,8]/[16,1], f16[5,8]/[16,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; "
         'd_x_lr=f32[5,16]/[16,1], edge_mask=None, negative_slope=0.2, node_mask=f32[5]/[1], want_mask_grad=True)')),
    'gatv2_mp.6': (("gatv2_mp(f16[5,8]/[16,1], f16[5,8]/[16,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], edge_mask=f32[7]/[1], "
         'negative_slope=0.2, node_mask=None)')),
    'gatv2_mp_backward_f16.6': (("gatv2_mp_backward_f16(f16[5,8]/[16,1], f16[5,8]/[16,1], f16[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; "
         'd_x_lr=f32[5,16]/[16,1], edge_mask=f32[7]/[1], negative_slope=0.2, node_mask=None, want_mask_grad=True)')),
    'linear.15': 'linear(f32[5,12]/[12,1], f32[8,12]/[12,1], None; cache_planes=False, out_dtype=torch.float16)',
    'linear.16': 'linear(f32[5,12]/[12,1], f32[16,12]/[12,1], None; cache_planes=False, out_dtype=torch.float16)',
    'gatv2_mp.7': (("gatv2_mp(f32[5,8]/[8,1], f32[5,8]/[8,1], f32[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], dropout_p=0.25, dropout_seed=7, "
         'edge_mask=None, kernel=None, negative_slope=0.2, node_mask=None)')),
    'gatv2_mp_backward.1': (("gatv2_mp_backward(f32[5,8]/[8,1], f32[5,8]/[8,1], f32[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; dropout_p=0.25, "
         'dropout_seed=7, edge_mask=None, negative_slope=0.2, node_mask=None, want_mask_grad=False)')),
    'gatv2_mp.8': (("gatv2_mp(f32[5,8]/[8,1], f32[5,8]/[8,1], f32[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], dropout_p=0.25, dropout_seed=7, "
         'edge_mask=None, kernel=None, negative_slope=0.2, node_mask=f32[5]/[1])')),
    'gatv2_mp_backward.2': (("gatv2_mp_backward(f32[5,8]/[8,1], f32[5,8]/[8,1], f32[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; dropout_p=0.25, "
         'dropout_seed=7, edge_mask=None, negative_slope=0.2, node_mask=f32[5]/[1], want_mask_grad=True)')),
    'gatv2_mp.9': (("gatv2_mp(f32[5,8]/[8,1], f32[5,8]/[8,1], f32[7,8]/[8,1], f32[1,2,4]/[8,4,1], 'plan', 2; bias=f32[8]/[1], dropout_p=0.25, dropout_seed=7, "
         'edge_mask=f32[7]/[1], kernel=None, negative_slope=0.2, node_mask=None)')),
    'gatv2_mp_backward.3': (("gatv2_mp_backward(f32[5,8]/[8,1], f32[5,8]/[8,1], f32[7,8]/[8,1], f32[1,2,4]/[8,4,1], f32[7,2]/[2,1], f32[5,8]/[8,1], 'plan', 2; dropout_p=0.25, "
         'dropout_seed=7, edge_mask=f32[7]/[1], negative_slope=0.2, node_mask=None, want_mask_grad=True)')),
}

LINEAR_TRACES = {
    'identity-True-9-12-contiguous-True-all': (1, 'linear.1 linear_bwd_prep.1 linear.2 linear_wgrad_bf16x6.1'),
    'identity-True-9-12-slice-True-all': (1, 'linear.1 linear_bwd_prep.2 linear.2 linear_wgrad_bf16x6.1'),
    'identity-True-9-12-t-True-all': (1, 'linear.1 linear_bwd_prep.1 linear.2 linear_wgrad_bf16x6.1'),
    'identity-False-9-12-contiguous-True-all': (0, 'linear.1 linear.2 linear_wgrad.1'),
    'identity-False-9-12-slice-True-all': (0, 'linear.1 linear.2 linear_wgrad.1'),
    'identity-False-9-12-t-True-all': (0, 'linear.1 linear.2 linear_wgrad.1'),
    'gelu-True-9-12-contiguous-True-all': (1, 'linear.1 linear_bwd_prep.3 linear.2 linear_wgrad_bf16x6.1'),
    'gelu-True-9-12-slice-True-all': (1, 'linear.1 linear_bwd_prep.4 linear.2 linear_wgrad_bf16x6.1'),
    'gelu-True-9-12-t-True-all': (1, 'linear.1 linear_bwd_prep.3 linear.2 linear_wgrad_bf16x6.1'),
    'gelu-False-9-12-contiguous-True-all': (0, 'linear.1 linear.2 linear_wgrad.1'),
    'gelu-False-9-12-slice-True-all': (0, 'linear.1 linear.2 linear_wgrad.1'),
    'gelu-False-9-12-t-True-all': (0, 'linear.1 linear.2 linear_wgrad.1'),
    'relu-True-9-12-contiguous-True-all': (1, 'linear.3 linear_bwd_prep.5 linear.2 linear_wgrad_bf16x6.1'),
    'relu-True-9-12-slice-True-all': (1, 'linear.3 linear_bwd_prep.6 linear.2 linear_wgrad_bf16x6.1'),
    'relu-True-9-12-t-True-all': (1, 'linear.3 linear_bwd_prep.5 linear.2 linear_wgrad_bf16x6.1'),
    'relu-False-9-12-contiguous-True-all': (0, 'linear.3 linear.2 linear_wgrad.1'),
    'relu-False-9-12-slice-True-all': (0, 'linear.3 linear.2 linear_wgrad.1'),
    'relu-False-9-12-t-True-all': (0, 'linear.3 linear.2 linear_wgrad.1'),
    'identity-True-3-12-contiguous-True-all': (1, 'linear.4 linear_bwd_prep.7 linear.5'),
    'identity-False-3-12-contiguous-True-all': (0, 'linear.4 linear.5'),
    'gelu-True-3-12-contiguous-True-all': (1, 'linear.4 linear_bwd_prep.8 linear.5'),
    'gelu-False-3-12-contiguous-True-all': (0, 'linear.4 linear.5'),
    'identity-True-9-10-slice-True-all': (1, 'linear.6 linear_bwd_prep.9 linear_wgrad_bf16x6.2'),
    'identity-False-9-10-slice-True-all': (0, 'linear.6 linear_wgrad.2'),
    'relu-True-9-10-contiguous-True-all': (1, 'linear.7 linear_bwd_prep.10 linear_wgrad_bf16x6.2'),
    'relu-False-9-10-contiguous-True-all': (0, 'linear.7 linear_wgrad.2'),
    'identity-True-9-12-slice-False-all': (1, 'linear.8 linear.2 linear_wgrad_bf16x6.1'),
    'identity-False-9-12-slice-False-all': (0, 'linear.8 linear.2 linear_wgrad.1'),
    'gelu-True-9-12-slice-False-all': (1, 'linear.8 linear_bwd_prep.11 linear.2 linear_wgrad_bf16x6.1'),
    'gelu-False-9-12-slice-False-all': (0, 'linear.8 linear.2 linear_wgrad.1'),
    'identity-True-9-12-contiguous-True-x': (1, 'linear.1 linear.2'),
    'identity-True-9-12-contiguous-True-w': (1, 'linear.1 linear_wgrad_bf16x6.1'),
    'identity-False-9-12-contiguous-True-x': (0, 'linear.1 linear.2'),
    'identity-False-9-12-contiguous-True-w': (0, 'linear.1 linear_wgrad.1'),
    'gelu-True-9-12-contiguous-True-x': (1, 'linear.1 linear_bwd_prep.12 linear.2'),
    'gelu-True-9-12-contiguous-True-w': (1, 'linear.1 linear_bwd_prep.12 linear_wgrad_bf16x6.1'),
    'gelu-False-9-12-contiguous-True-x': (0, 'linear.1 linear.2'),
    'gelu-False-9-12-contiguous-True-w': (0, 'linear.1 linear_wgrad.1'),
}

ROWBIAS_TRACES = {
    'identity-True': (0, 'linear_rowbias.1 linear.2 linear_wgrad_bf16x6.1 segment_range_sum.1'),
    'identity-False': (0, 'linear_rowbias.1 linear.2 linear_wgrad_bf16x6.1 segment_rowptr.1 segment_range_sum.1'),
    'gelu-True': (0, 'linear_rowbias.1 linear_bwd_prep.11 linear.2 linear_wgrad_bf16x6.1 segment_range_sum.1'),
    'gelu-False': (0, 'linear_rowbias.1 linear_bwd_prep.11 linear.2 linear_wgrad_bf16x6.1 segment_rowptr.1 segment_range_sum.1'),
    'relu-True': (0, 'linear_rowbias.2 linear_bwd_prep.13 linear.2 linear_wgrad_bf16x6.1 segment_range_sum.1'),
    'relu-False': (0, 'linear_rowbias.2 linear_bwd_prep.13 linear.2 linear_wgrad_bf16x6.1 segment_rowptr.1 segment_range_sum.1'),
}

CONV_TRACES = {
    'shared-both-none-True': (2, 'linear.9 linear.10 gatv2_mp.1 gatv2_mp_backward_f16.1 linear_bwd_prep.14 linear.11 linear_wgrad_bf16x6.3 linear.12 linear_wgrad_bf16x6.4'),
    'shared-both-none-False': (0, 'linear.9 linear.10 gatv2_mp.1 gatv2_mp_backward_f16.1 linear.11 linear_wgrad.3 linear.12 linear_wgrad.4'),
    'shared-both-node-True': (2, 'linear.9 linear.10 gatv2_mp.2 gatv2_mp_backward_f16.2 linear_bwd_prep.14 linear.11 linear_wgrad_bf16x6.3 linear.12 linear_wgrad_bf16x6.4 node_to_edge_mask_backward.1'),
    'shared-both-node-False': (0, 'linear.9 linear.10 gatv2_mp.2 gatv2_mp_backward_f16.2 linear.11 linear_wgrad.3 linear.12 linear_wgrad.4 node_to_edge_mask_backward.1'),
    'shared-both-edge-True': (2, 'linear.9 linear.10 gatv2_mp.3 gatv2_mp_backward_f16.3 linear_bwd_prep.14 linear.11 linear_wgrad_bf16x6.3 linear.12 linear_wgrad_bf16x6.4'),
    'shared-both-edge-False': (0, 'linear.9 linear.10 gatv2_mp.3 gatv2_mp_backward_f16.3 linear.11 linear_wgrad.3 linear.12 linear_wgrad.4'),
    'distinct-both-none-True': (2, 'linear.13 linear.10 gatv2_mp.4 gatv2_mp_backward_f16.4 linear_bwd_prep.15 linear.14 linear_wgrad_bf16x6.5 linear.12 linear_wgrad_bf16x6.4'),
    'distinct-both-none-False': (0, 'linear.13 linear.10 gatv2_mp.4 gatv2_mp_backward_f16.4 linear.14 linear_wgrad.5 linear.12 linear_wgrad.4'),
    'distinct-both-node-True': (2, 'linear.13 linear.10 gatv2_mp.5 gatv2_mp_backward_f16.5 linear_bwd_prep.15 linear.14 linear_wgrad_bf16x6.5 linear.12 linear_wgrad_bf16x6.4 node_to_edge_mask_backward.1'),
    'distinct-both-node-False': (0, 'linear.13 linear.10 gatv2_mp.5 gatv2_mp_backward_f16.5 linear.14 linear_wgrad.5 linear.12 linear_wgrad.4 node_to_edge_mask_backward.1'),
    'distinct-both-edge-True': (2, 'linear.13 linear.10 gatv2_mp.6 gatv2_mp_backward_f16.6 linear_bwd_prep.15 linear.14 linear_wgrad_bf16x6.5 linear.12 linear_wgrad_bf16x6.4'),
    'distinct-both-edge-False': (0, 'linear.13 linear.10 gatv2_mp.6 gatv2_mp_backward_f16.6 linear.14 linear_wgrad.5 linear.12 linear_wgrad.4'),
    'shared-left-none-True': (2, 'linear.9 linear.10 gatv2_mp.1 gatv2_mp_backward_f16.1 linear_bwd_prep.14 linear.11 linear_wgrad_bf16x6.3 linear.12 linear_wgrad_bf16x6.4'),
    'shared-left-none-False': (0, 'linear.9 linear.10 gatv2_mp.1 gatv2_mp_backward_f16.1 linear.11 linear_wgrad.3 linear.12 linear_wgrad.4'),
    'shared-neither-none-True': (2, 'linear.15 linear.10 gatv2_mp.1 gatv2_mp_backward_f16.1 linear.11 linear_wgrad_bf16x6.3 linear.12 linear_wgrad_bf16x6.4'),
    'shared-neither-none-False': (0, 'linear.15 linear.10 gatv2_mp.1 gatv2_mp_backward_f16.1 linear.11 linear_wgrad.3 linear.12 linear_wgrad.4'),
    'distinct-left-none-True': (2, 'linear.13 linear.10 gatv2_mp.4 gatv2_mp_backward_f16.4 linear_bwd_prep.15 linear.14 linear_wgrad_bf16x6.5 linear.12 linear_wgrad_bf16x6.4'),
    'distinct-left-none-False': (0, 'linear.13 linear.10 gatv2_mp.4 gatv2_mp_backward_f16.4 linear.14 linear_wgrad.5 linear.12 linear_wgrad.4'),
    'distinct-neither-none-True': (2, 'linear.16 linear.10 gatv2_mp.4 gatv2_mp_backward_f16.4 linear.14 linear_wgrad_bf16x6.5 linear.12 linear_wgrad_bf16x6.4'),
    'distinct-neither-none-False': (0, 'linear.16 linear.10 gatv2_mp.4 gatv2_mp_backward_f16.4 linear.14 linear_wgrad.5 linear.12 linear_wgrad.4'),
}

MP_TRACES = {
    'none': 'gatv2_mp.7 gatv2_mp_backward.1',
    'node': 'gatv2_mp.8 gatv2_mp_backward.2 node_to_edge_mask_backward.1',
    'edge': 'gatv2_mp.9 gatv2_mp_backward.3',
}
