"""The --concat_instr variant on the MI355X (include/isg_concat.h): the row-biased Linear exactly on integers and
bit for bit against the composed form, ops / autograd against float64, the layer and the model against the literal restatement of
tests/concat_instr_restated.py, a reference-layout checkpoint, and half rows.

Rule against float64 (tests/test_gpu_backward_fp64.py, its Judge): e_k <= max(4 e_32, 2e-6), e_32 the literal torch.cat form in
float32 on the CPU.
"""
import argparse
import ctypes
import itertools

import pytest
import torch

gpu = pytest.mark.gpu
GM_BM = GM_BN = 128          # csrc/isg_gemm.hip: rows / columns of a workgroup's tile
DUAL_K = 256                 # linear_launch: K > 256 takes the two-accumulator form
MS, NS, KS = (1, 31, 127, 128, 129, 300), (4, 100, 128, 132), (32, 128, 132, 300)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def launch_form(N, K):
    """(XCD tile order, DUAL) of linear_launch for a shape: more than one column tile; K > 256."""
    return ((N + GM_BN - 1) // GM_BN > 1, K > DUAL_K)


def test_the_exact_shapes_reach_every_launch_form():
    forms = {launch_form(N, K) for N in NS for K in KS}
    assert forms == set(itertools.product((False, True), repeat=2))
    assert launch_form(132, 300) == (True, True) and launch_form(128, 128) == (False, False)
    assert launch_form(132, 32) == (True, False) and launch_form(4, 300) == (False, True)
    assert any(M % GM_BM for M in MS) and any(M > GM_BM for M in MS) and 128 in MS          # partial, several and whole row tiles


def _segments(M, S):
    """seg [M] for the exact test.  S = 1: one segment; S = M: single-row segments; S = 3: rows [0, b) | no row | [b, M) with b on
    the 128-row tile edge when there is one, else inside the first wave's 32-row patch."""
    if S == 1:
        return torch.zeros(M, dtype=torch.int32)
    if S == M:
        return torch.arange(M, dtype=torch.int32)
    b = 128 if M > 128 else M // 3
    return torch.cat((torch.zeros(b, dtype=torch.int32), torch.full((M - b,), 2, dtype=torch.int32)))


def _rowbias(lib, a, planes, p, seg, d, N, K, act=0):
    from isubgvqa_amd import _lib
    M = a.size(0)
    _lib.check(lib.isg_linear_bf16x6_rowbias(a.data_ptr(), planes.data_ptr(), p.data_ptr(), p.stride(0) if p.size(0) > 1 else max(p.stride(0), N),
                                             seg.data_ptr(), p.size(0), d.data_ptr(), 1 if d.dtype == torch.float16 else 0, M, N, K,
                                             a.stride(0) if M > 1 else K, d.stride(0) if M > 1 else max(d.stride(0), N), act, None),
               "isg_linear_bf16x6_rowbias")


def _planes(w):
    from isubgvqa_amd import ops
    return ops._split_weight(w, "tile")


def _strict():
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib, _lib_concat
    return _lib.bind(ctypes.CDLL(ge.STRICT_LIB), _lib_concat.SIGNATURES)


# ---- 1: exact on integers ---------------------------------------------------------------------------------------------------
@gpu
def test_kernel_is_exact_on_small_integers(dev):
    """A, W in [-7, 7], P integers: every product and every partial sum is an integer below 2^24, so every entry of D must equal
    the integer result -- over every M x N x K x S of the lists, on both libraries, twice."""
    from isubgvqa_amd import _lib_concat
    lib, strict = _lib_concat.load(), _strict()
    g = torch.Generator().manual_seed(1)
    checked = 0
    for N, K in itertools.product(NS, KS):
        w = torch.randint(-7, 8, (N, K), generator=g).float().to(dev)
        planes = _planes(w)
        for M in MS:
            a = torch.randint(-7, 8, (M, K), generator=g).float().to(dev)
            for S in sorted({1, 3, M}):
                seg = _segments(M, S).to(dev)
                p = torch.randint(-1000, 1001, (S, N), generator=g).float().to(dev)
                want = a.double() @ w.double().t() + p.double()[seg.long()]
                outs = []
                for which in (lib, lib, strict):
                    d = torch.full((M, N), float("nan"), device=dev)
                    _rowbias(which, a, planes, p, seg, d, N, K)
                    outs.append(d)
                assert torch.equal(outs[0].double(), want), (M, N, K, S)
                assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), (M, N, K, S, "two calls")
                assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32)), (M, N, K, S, "strict library")
                checked += 1
    assert checked == len(NS) * len(KS) * (len(MS) * 3 - 1)          # M = 1: S = 1 and S = M coincide


@gpu
@pytest.mark.parametrize("N,K", [(132, 300), (100, 128), (4, 32), (128, 132)])
def test_kernel_segment_edges_slices_and_guards(dev, N, K):
    """300 rows in six segments -- 13 | 115 | none | 1 | 1 | 170: a boundary inside a wave's 32-row patch, one on the 128-row tile
    edge, an empty segment, single-row segments -- with P and D column slices of wider tensors (ldp > N, ldd > N), D one float past
    a 16-byte boundary, and guard words around and between D's rows."""
    from isubgvqa_amd import _lib_concat
    lib = _lib_concat.load()
    g = torch.Generator().manual_seed(2)
    M, counts = 300, torch.tensor([13, 115, 0, 1, 1, 170])
    seg = torch.repeat_interleave(torch.arange(6), counts).int().to(dev)
    a = torch.randint(-7, 8, (M, K), generator=g).float().to(dev)
    w = torch.randint(-7, 8, (N, K), generator=g).float().to(dev)
    pw = torch.randint(-1000, 1001, (6, N + 7), generator=g).float().to(dev)
    p = pw[:, 3:3 + N]
    ldd, GUARD = N + 5, -12345.0
    buf = torch.full((M * ldd + 64,), GUARD, device=dev)
    d = buf[17:17 + M * ldd].view(M, ldd)[:, :N]                       # 17 floats in: one float past a 16-byte boundary
    assert d.data_ptr() % 16 == 4 and p.stride(0) == N + 7
    want = a.double() @ w.double().t() + p.double()[seg.long()]
    for act in (0, 2):
        buf.fill_(GUARD)
        _rowbias(lib, a, _planes(w), p, seg, d, N, K, act)
        assert torch.equal(d.double(), want.clamp_min(0) if act == 2 else want), act
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[17:17 + M * ldd].view(M, ldd)[:, :N] = False
        assert bool((buf[mask] == GUARD).all()), "a word outside D was written"
    # half rows: the same integers (|D| < 2048 would be exact in half; here: one rounding of the exact value)
    h = torch.full((M, ldd), GUARD, device=dev).half()
    _rowbias(lib, a, _planes(w), p, seg, h[:, :N], N, K)
    assert torch.equal(h[:, :N], want.float().half()) and bool((h[:, N:] == torch.tensor(GUARD).half()).all())


# ---- 2: bits on random fp32 -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,N,K", [(300, 132, 300), (129, 100, 128), (31, 4, 32), (300, 128, 132)])
def test_kernel_bits_against_the_composed_form(dev, M, N, K):
    from isubgvqa_amd import _lib, _lib_concat
    lib, base = _lib_concat.load(), _lib.load()
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    planes = _planes(w)
    S = 5
    seg = (torch.arange(M) * S // M).int().to(dev)
    p = torch.randn(S, N, generator=g).to(dev)

    def plain(bias, act):
        d = torch.empty(M, N, device=dev)
        _lib.check(base.isg_linear_bf16x6(a.data_ptr(), planes.data_ptr(), 0 if bias is None else bias.data_ptr(), d.data_ptr(), M, N, K,
                                          K, N, act, None), "isg_linear_bf16x6")
        return d

    def rowb(pp, sg, act, dtype=torch.float32):
        d = torch.empty(M, N, device=dev, dtype=dtype)
        _rowbias(lib, a, planes, pp, sg, d, N, K, act)
        return d

    got = rowb(p, seg, 0)
    assert torch.equal(got.view(torch.int32), (plain(None, 0) + p[seg.long()]).view(torch.int32))
    zero = torch.zeros(M, dtype=torch.int32, device=dev)
    for act in (0, 1, 2):
        one = rowb(p[:1], zero, act)
        assert torch.equal(one.view(torch.int32), plain(p[0].contiguous(), act).view(torch.int32)), act
    for act in (0, 1):
        assert torch.equal(rowb(p, seg, act, torch.float16), rowb(p, seg, act).half()), act


@gpu
def test_range_sum_is_exact_on_integers_and_touches_nothing_else(dev):
    """ops.segment_range_sum on integer rows: every sum equals the integer result -- segments of 0, 1, 3, 4, 5 and 700 rows, widths
    on the vector path (4 | C, aligned) and the scalar one (C = 6; a column slice one float in), G and out as column slices of wider
    tensors with guard columns, two calls equal."""
    from isubgvqa_amd import ops
    g = torch.Generator().manual_seed(5)
    counts = torch.tensor([3, 0, 700, 1, 4, 0, 5])
    ptr = torch.cat((torch.zeros(1, dtype=torch.long), counts.cumsum(0))).int().to(dev)
    M, S = int(counts.sum()), counts.numel()
    seg = torch.repeat_interleave(torch.arange(S), counts).to(dev)
    for C, off in ((1024, 0), (128, 4), (300, 8), (6, 0), (128, 1), (1028, 0)):
        wide = torch.randint(-50, 51, (M, C + 12), generator=g).float().to(dev)
        G = wide[:, off:off + C]
        buf = torch.full((S, C + 12), -7.0, device=dev)
        out = buf[:, off:off + C]
        ops.segment_range_sum(ptr, G, out=out)
        want = torch.zeros(S, C, dtype=torch.float64, device=dev).index_add_(0, seg, G.double())
        assert torch.equal(out.double(), want), (C, off)
        assert bool((buf[:, :off] == -7.0).all()) and bool((buf[:, off + C:] == -7.0).all()), (C, off)
        again = ops.segment_range_sum(ptr, G)
        assert again.is_contiguous() and torch.equal(again.view(torch.int32), out.contiguous().view(torch.int32)), (C, off)
    assert ops.segment_range_sum(ptr[:1], wide[:, :8]).shape == (0, 8)
    assert torch.equal(ops.segment_rowptr(seg.int(), S), ptr)


# ---- 3: ops and autograd against float64 ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gelu", [False, True], ids=["none", "gelu"])
@pytest.mark.parametrize("M,K", [(95, 128), (2050, 128), (95, 300), (2050, 300)])
def test_linear_rowbias_and_its_gradients_against_float64(dev, M, K, gelu):
    """y = act(cat(x, u[seg]) W^T + b) with W [N, 2K] ONE parameter: forward, dx, dW (both column halves), db, du against the
    literal form in float64, and dP against the segment sums of dz there.  M: both sides of autograd.WGRAD_MIN_ROWS."""
    import torch.nn.functional as F
    from isubgvqa_amd import autograd, ops
    from test_gpu_backward_fp64 import LINEAR_CAP, Judge
    assert 95 < autograd.WGRAD_MIN_ROWS <= 2050
    N, S = 132, 5
    g = torch.Generator().manual_seed(4)
    x, u = torch.randn(M, K, generator=g), torch.randn(S, K, generator=g)
    W, b = torch.randn(N, 2 * K, generator=g) / (2 * K) ** 0.5, torch.randn(N, generator=g)
    up = torch.randn(M, N, generator=g)
    counts = torch.tensor([M // 3, M // 5, 0, 1, M - M // 3 - M // 5 - 1])
    seg = torch.repeat_interleave(torch.arange(S), counts)

    def literal(dtype):
        lv = [t.to(dtype).clone().requires_grad_(True) for t in (x, u, W, b)]
        z = F.linear(torch.cat((lv[0], lv[1][seg]), 1), lv[2], lv[3])
        z.retain_grad()
        y = F.gelu(z) if gelu else z
        (y * up.to(dtype)).sum().backward()
        dP = torch.zeros(S, N, dtype=dtype).index_add(0, seg, z.grad)
        return [y.detach()] + [t.grad for t in lv] + [dP]

    ref64, ref32 = literal(torch.float64), literal(torch.float32)
    lv = [t.to(dev).requires_grad_(True) for t in (x, u, W, b)]
    segd = seg.int().to(dev)
    ops.reset_counters()
    Pd = autograd.linear(lv[1], lv[2][:, K:].contiguous(), lv[3], False)
    Pd.retain_grad()
    y = ops.linear_rowbias(lv[0], lv[2][:, :K], Pd, segd, gelu=gelu)
    (y * up.to(dev)).sum().backward()
    again = autograd.linear(lv[1].detach(), lv[2].detach()[:, K:].contiguous(), lv[3].detach(), False).requires_grad_(True)
    y2 = ops.linear_rowbias(lv[0].detach(), lv[2].detach()[:, :K], again, segd, gelu=gelu)
    (y2 * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert ops.counters()["linear_rowbias"] == 2
    assert torch.equal(again.grad.view(torch.int32), Pd.grad.view(torch.int32)), "dP: two calls differ"
    with torch.no_grad():
        inf = ops.linear_rowbias(lv[0], lv[2][:, :K], Pd, segd, gelu=gelu)
    j = Judge(f"linear_rowbias M={M} K={K} gelu={gelu}", LINEAR_CAP)
    j("forward (autograd)", y, ref64[0], ref32[0])
    j("forward (inference)", inf, ref64[0], ref32[0])
    for name, got, r64, r32 in zip(("dx", "du", "dW", "db", "dP"), [t.grad for t in lv] + [Pd.grad], ref64[1:], ref32[1:]):
        j(name, got, r64, r32)
    j.done()


# ---- 4: the layer -----------------------------------------------------------------------------------------------------------
def _graphs(sizes, gen):
    """batch, edge_index of graphs with the given node counts: every node's self-loop and 2 n random edges inside each graph."""
    n = torch.tensor(sizes)
    ptr = torch.cat((torch.zeros(1, dtype=torch.long), n.cumsum(0)))
    batch = torch.repeat_interleave(torch.arange(len(sizes)), n)
    src, dst = [torch.arange(int(ptr[-1]))], [torch.arange(int(ptr[-1]))]
    for gi, k in enumerate(sizes):
        src.append(torch.randint(0, k, (2 * k,), generator=gen) + ptr[gi])
        dst.append(torch.randint(0, k, (2 * k,), generator=gen) + ptr[gi])
    return batch, torch.stack((torch.cat(src), torch.cat(dst)))


def _layer_fixture(C, H, masked, share, seed):
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    gen = torch.Generator().manual_seed(100 + seed)
    torch.manual_seed(seed)
    layer = MaskingGATv2Conv(2 * C, C, heads=H, edge_dim=C, add_self_loops=False, masking_threshold=0.15 if masked else 1.0,
                             use_instr=True, use_topk=True, concat_instr=True, share_weights=share, sampler_type="imle",
                             sample_k=3).eval()
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if name.endswith("bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    sizes = [1, 70, 2, 33, 17]
    batch, ei = _graphs(sizes, gen)
    N, E, B = batch.numel(), ei.size(1), len(sizes)
    r = lambda *s: torch.randn(*s, generator=gen)
    return dict(layer=layer, batch=batch, ei=ei, x=r(N, C), ea=r(E, C), ins=r(B, C), glf=r(B, C), up=r(N, H * C),
                counts=torch.tensor(sizes), H=H, C=C, masked=masked)


def _layer_restated(fx, dtype, grad=False):
    import concat_instr_restated as R
    from oracle import model as OM
    sd = {"c." + k: v for k, v in R.cast(dict(fx["layer"].state_dict()), dtype).items()}
    cfg = OM.PathConfig(heads=fx["H"], use_topk=True, sampler_type="imle", sample_k=3)
    x, ea, ins, glf = (R.cast(fx[k], dtype) for k in ("x", "ea", "ins", "glf"))
    if grad:
        x.requires_grad_(True)
    aux = {}
    out, mask, _ = R.conv(sd, "c", x, fx["ei"], fx["batch"], ea, ins, glf, 0.15 if fx["masked"] else 1.0, cfg, None, aux)
    dx = None
    if grad:
        (out * fx["up"].to(dtype)).sum().backward()
        dx = x.grad
    return out.detach(), mask, aux, dx


LAYERS = [(8, 2), (64, 4), (128, 4), (300, 4)]


@gpu
@pytest.mark.parametrize("share", [False, True], ids=["distinct", "shared"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "imle"])
@pytest.mark.parametrize("C,H", LAYERS)
def test_layer_against_the_restatement(dev, monkeypatch, C, H, masked, share):
    import concat_instr_restated as R
    import isubgvqa_amd.models.mgat_v2_conv as MC
    from isubgvqa_amd import ops
    from test_gpu_backward_fp64 import MP_CAP, Judge

    def scores(fx):
        aux = _layer_restated(fx, torch.float64)[2]
        return [(aux["dense"].squeeze(-1), 3, fx["counts"])] if masked else []

    fx = R.reseeded(lambda seed: _layer_fixture(C, H, masked, share, seed), scores)
    out64, mask64, _, dx64 = _layer_restated(fx, torch.float64, grad=True)
    out32, mask32, _, dx32 = _layer_restated(fx, torch.float32, grad=True)
    layer = fx["layer"].to(dev)
    t = {k: fx[k].to(dev) for k in ("x", "ei", "batch", "ea", "ins", "glf", "up")}
    plan = ops.GraphPlan.build(t["batch"], t["ei"], num_graphs=5)
    call = lambda x: layer(x, t["ei"], t["batch"], edge_attr=t["ea"], instruction=t["ins"], imle_att=t["glf"], plan=plan)
    j = Judge(f"concat layer C={C} H={H} masked={masked} share={share}", MP_CAP)
    results = {}
    for split in (True, False):
        monkeypatch.setattr(MC, "CONCAT_SPLIT", split)
        ops.reset_counters()
        with torch.no_grad():
            out, mask = call(t["x"])
        n = ops.counters()["linear_rowbias"]
        assert n == ((2 if masked else 1) if split else 0), (split, n)
        if masked:
            assert torch.equal(mask.cpu(), mask64.to(mask.dtype)) and torch.equal(mask64, mask32.double()), split
        else:
            assert mask is None and mask64 is None
        j(f"out (split={split})", out, out64, out32)
        results[split] = out
    # forward and backward of the split form never call torch.cat
    monkeypatch.setattr(MC, "CONCAT_SPLIT", True)

    def no_cat(*a, **k):
        raise AssertionError("torch.cat was called")

    xg = t["x"].clone().requires_grad_(True)
    with monkeypatch.context() as m:
        m.setattr(torch, "cat", no_cat)
        ops.reset_counters()
        out, _ = call(xg)
        (out * t["up"]).sum().backward()
        torch.cuda.synchronize()
    assert ops.counters()["linear_rowbias"] == (2 if masked else 1)
    j("out (autograd)", out, out64, out32)
    j("dx", xg.grad, dx64, dx32)
    grads = {k: p.grad for k, p in layer.named_parameters()}
    assert grads["lin_l.weight"] is not None and float(grads["lin_l.weight"][:, :C].abs().max()) > 0
    assert float(grads["lin_l.weight"][:, C:].abs().max()) > 0, "the instruction half of lin_l.weight has no gradient"
    if masked:
        # the node gate's scores differentiated on their own (the eval sampler behind them passes no gradient): d node_nn.0.weight,
        # both column halves, and dx against oracle.model.node_gate_scores on the concatenated input
        from oracle import model as OM
        gw = torch.randn(t["x"].size(0), 1, generator=torch.Generator().manual_seed(7))
        refs = []
        for dtype in (torch.float64, torch.float32):
            sd = {"c." + k: v.cpu().requires_grad_(True) for k, v in R.cast(dict(layer.state_dict()), dtype).items()}
            x = fx["x"].to(dtype).requires_grad_(True)
            xc = R.cat_input(x, fx["ins"].to(dtype), fx["batch"])
            sc = OM.node_gate_scores(sd, "c.mask", xc, fx["glf"].to(dtype)[fx["batch"]], fx["batch"])
            (sc * gw.to(dtype)).sum().backward()
            refs.append((sc.detach(), x.grad, sd["c.mask.node_nn.0.weight"].grad))
        layer.zero_grad(set_to_none=True)
        xg = t["x"].clone().requires_grad_(True)
        with monkeypatch.context() as m:
            m.setattr(torch, "cat", no_cat)
            sc = layer.mask.gate_scores(xg, t["glf"], t["batch"], u_is_per_graph=True, plan=plan,
                                        concat=(t["ins"], t["batch"].int(), plan.ptr))
            (sc * gw.to(dev)).sum().backward()
        gwt = layer.mask.node_nn[0].weight.grad
        assert float(gwt[:, :C].abs().max()) > 0 and float(gwt[:, C:].abs().max()) > 0
        for name, got, i in (("gate scores", sc, 0), ("gate: dx", xg.grad, 1), ("gate: d node_nn.0.weight", gwt, 2)):
            j(name, got, refs[0][i], refs[1][i])
    j.done()


# ---- 5: the model -----------------------------------------------------------------------------------------------------------
def _model_fixture(seed):
    from isubgvqa_amd import synthetic
    cfg = synthetic.WorkloadConfig(num_graphs=12, channels=128, layers=2, masks=(1.0, 0.15), sampler="imle", sample_k=3,
                                   nodes_dist="uniform", nodes_min=5, nodes_max=64, edges_per_graph=0.0, seed=500 + seed)
    wl = synthetic.make_workload(cfg)
    torch.manual_seed(seed)
    model = synthetic.AnswerModel(128, 2, (1.0, 0.15), "imle", 3, concat_instr=True).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "bns" in name or name.endswith(".bias"):
                p.add_(0.05 * torch.randn(p.shape, generator=gen))
    from oracle import samplers as OS
    noise = OS.uniform_to_gumbel(torch.rand(12, 1, wl.max_nodes, 1, generator=gen), 0.0, 0.3)
    target = torch.randint(0, 1842, (12,), generator=gen)
    return dict(cfg=cfg, wl=wl, model=model, noise=noise, target=target, seed=seed)


def _model_restated(fx, dtype, training=False, grad=False):
    import concat_instr_restated as R
    from oracle import model as OM
    wl = fx["wl"]
    sd = R.cast({k: v for k, v in fx["model"].state_dict().items() if v.is_floating_point()}, dtype)
    if grad:
        for v in sd.values():
            v.requires_grad_(True)
    cfg = OM.PathConfig(heads=4, masking_thresholds=[1.0, 0.15], use_topk=True, sampler_type="imle", sample_k=3, training=training)
    trace = []
    logits, mask, _ = R.answer(sd, *(R.cast(t, dtype) for t in (wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf)), cfg,
                               {1: R.cast(fx["noise"], dtype)} if training else None, trace)
    return logits, mask, trace, sd


@pytest.fixture(scope="module")
def model_fx():
    import concat_instr_restated as R

    def scores(fx):
        counts = torch.bincount(fx["wl"].batch)
        with torch.no_grad():
            ev = _model_restated(fx, torch.float64)[2][1]["dense"].squeeze(-1)
            tr = _model_restated(fx, torch.float64, training=True)[2][1]["dense"].squeeze(-1)
        return [(ev, 3, counts), (tr, 3, counts, fx["noise"], 1.0)]

    return R.reseeded(_model_fixture, scores)


@gpu
def test_model_eval_against_the_restatement_and_its_captured_replay(dev, model_fx):
    from isubgvqa_amd import ops
    fx = model_fx
    with torch.no_grad():
        ref, ref_mask, _, _ = _model_restated(fx, torch.float32)
        model, d = _model_fixture(fx["seed"])["model"].to(dev).eval(), fx["wl"].to(dev)      # (the fixture's own stays on the CPU)
        ops.reset_counters()
        logits, mask, gate = model(d)
        assert ops.counters()["linear_rowbias"] == 3                 # two projections and the masked layer's node gate
        err = float((logits.cpu() - ref).abs().max())
        print(f"[concat model] max |logit diff| = {err:.3e}")
        assert torch.equal(mask.cpu(), ref_mask)
        assert err < 1e-4
        for _ in range(3):                                           # warm-up calls, the capture, a replay
            cl, cm, cg = model(d, capture=True)
        assert torch.equal(cl.view(torch.int32), logits.view(torch.int32)) and torch.equal(cm, mask)
        assert torch.equal(cg.view(torch.int32), gate.view(torch.int32))


@gpu
def test_model_takes_a_training_step(dev, model_fx):
    from isubgvqa_amd import ops, optim, train
    fx = model_fx
    model = _model_fixture(fx["seed"])["model"].to(dev).train()
    for conv in model.gat_seq.convs:
        conv.mask.gate_dropout = 0.0
    model.embedding[2].p = 0.0
    logits, _, _, sd = _model_restated(fx, torch.float32, training=True, grad=True)
    ref_loss = torch.nn.functional.cross_entropy(logits, fx["target"])
    ref_loss.backward()
    ins = {"wl": fx["wl"].to(dev), "noises": {1: fx["noise"].to(dev)}}
    # the gradients of the step's own forward and backward, read before the optimizer moves the weights
    out = model(**ins)[0]
    torch.nn.functional.cross_entropy(out, fx["target"].to(dev)).backward()
    bad = []
    for k, p in model.named_parameters():
        want = sd[k].grad
        if want is None or float(want.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        e = float((p.grad.cpu() - want).abs().max()) / float(want.abs().max())
        print(f"[concat train] {k}: {e:.3e}")
        if not e < 1e-3:
            bad.append((k, e))
    C = 128
    # both column halves of the wide parameters (the node gate's: where the estimator's two MAP states differ -- the loop above
    # holds it to the restatement's exact zeros where they do not; test_layer_against_the_restatement differentiates the gate)
    for k in ("gat_seq.convs.0.lin_l.weight", "gat_seq.convs.1.lin_l.weight", "gat_seq.convs.1.mask.node_nn.0.weight"):
        g, want = dict(model.named_parameters())[k].grad, sd[k].grad
        for half in (slice(0, C), slice(C, 2 * C)):
            assert (float(g[:, half].abs().max()) > 0) == (want is not None and float(want[:, half].abs().max()) > 0), k
        assert k.endswith("node_nn.0.weight") or float(g.abs().max()) > 0, k
    assert not bad, bad
    model.zero_grad(set_to_none=True)
    ops.reset_counters()
    meters = train.Meters(dev)
    res = train.train_step(model, optim.Adam(model.parameters(), lr=1e-3, max_grad_norm=2.0), ins, fx["target"].to(dev), meters)
    torch.cuda.synchronize()
    assert ops.counters()["linear_rowbias"] == 3
    rep = meters.report()
    assert rep["steps"] == 1 and rep["skipped_steps"] == 0 and rep["nonfinite_losses"] == 0
    loss = float(res.loss.detach())
    print(f"[concat train] loss {loss:.6f}, restatement {float(ref_loss.detach()):.6f}")
    assert abs(loss - float(ref_loss.detach())) < 1e-3


# ---- 6: checkpoint ----------------------------------------------------------------------------------------------------------
@gpu
def test_reference_layout_checkpoint_loads_and_runs(dev, tmp_path):
    from isubgvqa_amd import checkpoint, ops, synthetic
    from isubgvqa_amd.models import build_model
    from test_gpu_models import _full_args
    torch.manual_seed(0)
    args = _full_args(concat_instr=1)
    src = build_model(args, None).eval()
    sd = src.state_dict()
    assert tuple(sd["gat_seq.convs.0.lin_l.weight"].shape) == (1200, 600)
    assert tuple(sd["gat_seq.convs.3.mask.node_nn.0.weight"].shape) == (300, 600)
    path = str(tmp_path / "checkpoint.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}, "optimizer": {}, "lr_scheduler": {}, "epoch": 3,
                "args": argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in ("text_vocab_size", "sg_vocab_size")})},
               path)
    model, largs, rest = checkpoint.load_model(path, device="cpu", strict=True)
    assert largs.concat_instr == 1 and rest["epoch"] == 3 and all(c.concat_instr for c in model.gat_seq.convs)
    gen = torch.Generator().manual_seed(21)
    cfg = synthetic.WorkloadConfig(num_graphs=6, nodes_dist="uniform", nodes_min=2, nodes_max=16, edges_per_graph=0.0, seed=99)
    batch, ei, nmax = synthetic.make_topology(cfg, gen)
    N, E, B, T = batch.numel(), ei.size(1), 6, 9
    x = torch.randint(0, 2578, (N, 4), generator=gen)
    edge_attr = torch.randint(0, 2578, (E,), generator=gen)
    sg = argparse.Namespace(x_bbox=torch.randint(0, 640, (N, 4), generator=gen).to(dev),
                            added_sym_edge=torch.randint(0, 2, (4,), generator=gen).to(dev))
    q = torch.randint(0, 512, (B, T), generator=gen)
    qmask = torch.ones(B, T, dtype=torch.long)
    outs = []
    with torch.no_grad():
        for m in (src, model):
            m = m.to(dev).eval()
            ops.reset_counters()
            outs.append(m(x.to(dev), ei.to(dev), edge_attr.to(dev), batch.to(dev), q.to(dev), qmask.to(dev), return_masks=True,
                          scene_graphs=sg))
            assert ops.counters()["linear_rowbias"] == 5             # four projections and the masked layer's node gate
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[1][0]).all())


# ---- 7: half rows -----------------------------------------------------------------------------------------------------------
@gpu
def test_half_rows_in_inference_and_the_refusal_in_training(dev):
    from isubgvqa_amd import _lib, ops
    fx = _layer_fixture(128, 4, False, False, 0)
    layer = fx["layer"].to(dev)
    t = {k: fx[k].to(dev) for k in ("x", "ei", "batch", "ea", "ins", "glf", "up")}
    plan = ops.GraphPlan.build(t["batch"], t["ei"], num_graphs=5)
    seg = t["batch"].int()
    with torch.no_grad():
        full = layer._project_split(t["x"], (t["ins"], seg, plan.ptr), torch.float32)
        half = layer._project_split(t["x"], (t["ins"], seg, plan.ptr), torch.float16)
        for a, b in zip(half, full):
            assert a.dtype == torch.float16 and torch.equal(a, b.half())
        layer.feature_dtype = torch.float16
        out, _ = layer(t["x"], t["ei"], t["batch"], edge_attr=t["ea"], instruction=t["ins"], imle_att=t["glf"], plan=plan)
        layer.feature_dtype = torch.float32
        ref, _ = layer(t["x"], t["ei"], t["batch"], edge_attr=t["ea"], instruction=t["ins"], imle_att=t["glf"], plan=plan)
    err = float((out.float() - ref).abs().max()) / float(ref.abs().max())
    print(f"[concat half rows] max |out_half - out_fp32| / max |out_fp32| = {err:.3e}")
    assert err < 1e-3                                                # the bound the fp16 mode is held to
    layer.feature_dtype = torch.float16
    with pytest.raises(_lib.IsgError, match="concat_instr layer on half rows"):
        layer(t["x"].clone().requires_grad_(True), t["ei"], t["batch"], edge_attr=t["ea"], instruction=t["ins"], imle_att=t["glf"],
              plan=plan)
