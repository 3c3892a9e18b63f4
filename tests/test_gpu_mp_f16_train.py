"""Training on fp16 feature rows (include/isg_mp_f16_train.h) on the GPU.

  1  kernel bits      isg_gatv2_mp_bwd_f16 against isg_gatv2_mp_bwd on the same rows upcast: every result equal as words, on every
                      case of tests/test_gpu_backward_fp64.py (hub / every (H, P) / edge shapes), dense and strided, guard words
                      and unused columns untouched, two calls and the strict library the same bits
  2  the fp64 rule    the half entry point against oracle.model.gatv2_message_passing in float64 on the rounded rows, fp32 as the
                      yardstick (Judge: F = 4, FLOOR = 2e-6, cap 2e-4)
  3  refusals         bad strides ISG_EINVAL, shapes without a kernel ISG_EUNSUPPORTED, nothing written
  4  the Function     autograd.conv_half_rows: forward bits of the inference calls, every gradient the bits of the chain composed by
                      hand from ops.gatv2_mp_backward and autograd.linear on the upcast rows, half tensors saved
  5  the module       MaskingGATv2Conv(feature_dtype = half).train() runs forward and backward (IsgError before this feature)
  6  the model        one train.train_step of synthetic.AnswerModel on half rows; loss within 1e-3 of the oracle's fp16 mode
"""
import copy
import ctypes
import math

import pytest
import torch

from test_gpu_backward_fp64 import (EDGE_CASES, HUB_CASES, MP_CAP, MP_NAMES, SMALL_CASES, SMALL_PARTIAL, Judge, _grad, _mp_id,
                                    _NodeToEdge, _one_thread, mp_inputs, passes, topology)

gpu = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -2
GUARD = 64                       # words behind every output
SENTINEL = 0x7FC0BEEF            # a NaN pattern no kernel writes
ALL_CASES = HUB_CASES + SMALL_CASES + EDGE_CASES
OUT_NAMES = ("d x_l", "d x_r", "d e_proj", "d att partial", "d edge mask")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def _words(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_words(a), _words(b))


def _guarded(numel, dev):
    """A flat fp32 buffer of numel + GUARD words, every word the sentinel."""
    return torch.full((numel + GUARD,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _untouched(buf):
    return bool((buf.view(torch.int32) == SENTINEL).all())


class Rows:
    """The operands of one case on the device: x_l, x_r, e_proj of mp_inputs(case) rounded to half, alpha of the fp32 forward on
    those rows upcast, the plan and the mask."""

    def __init__(self, case, dev):
        from isubgvqa_amd import ops
        topo, self.H, self.C, self.mk, self.slope = case
        batch, ei, B = topology(topo)
        t = mp_inputs(case)
        self.N, self.E, self.HC = batch.numel(), ei.size(1), self.H * self.C
        self.dev = dev
        self.x_l, self.x_r, self.e = (t[k].half().to(dev) for k in ("x_l", "x_r", "e_proj"))
        self.att, self.w, self.bias = t["att"].to(dev), t["w"].to(dev), t["bias"].to(dev)
        self.plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
        self.mask = None if self.mk == "none" else t["mask"].to(dev)
        self.kw = {} if self.mk == "none" else {("node_mask" if self.mk == "node" else "edge_mask"): self.mask}
        with torch.no_grad():
            _, self.alpha = ops.gatv2_mp(self.x_l.float(), self.x_r.float(), self.e.float(), self.att, self.plan, self.H,
                                         bias=self.bias, negative_slope=self.slope, **self.kw)

    def entry(self, f16, strided=False, lib=None, strides=None, H=None, C=None):
        """One call of isg_gatv2_mp_bwd (f16=False, rows upcast) or isg_gatv2_mp_bwd_f16 through the C ABI into guarded
        buffers.  strided: x_l | x_r the halves of one [N, 2 HC] half buffer, e_proj the SECOND half of an [E, 2 HC] one,
        d_x_l | d_x_r the first columns of one [N, 2 HC + 8] fp32 buffer (8 unused columns per row).  Returns (status, the five
        results or None where the call asked for none, problems)."""
        from isubgvqa_amd import _lib, _lib_mp_f16_train
        N, E, HC, dev = self.N, self.E, self.HC, self.dev
        H, C = self.H if H is None else H, self.C if C is None else C
        lib = lib or (_lib_mp_f16_train.load() if f16 else _lib.load())
        keep = []
        if not f16:
            x_l, x_r, e = self.x_l.float(), self.x_r.float(), self.e.float()
            ld_in = ()
        elif strided:
            xlr = torch.full((N, 2 * HC), 7.0, dtype=torch.float16, device=dev)
            xlr[:, :HC], xlr[:, HC:] = self.x_l, self.x_r
            e2 = torch.full((E, 2 * HC), -3.0, dtype=torch.float16, device=dev)
            e2[:, HC:] = self.e
            x_l, x_r, e = xlr[:, :HC], xlr[:, HC:], e2[:, HC:]
            keep = [(xlr, xlr.clone()), (e2, e2.clone())]
            ld_in = (2 * HC, 2 * HC, 2 * HC)
        else:
            x_l, x_r, e = self.x_l, self.x_r, self.e
            keep = [(t, t.clone()) for t in (x_l, x_r, e)]
            ld_in = (0, 0, 0)
        blocks = (N + 15) // 16
        wide = 2 * HC + 8
        if f16 and strided:
            lr = _guarded(N * wide, dev)
            p_l, p_r, ld_out = lr.data_ptr(), lr.data_ptr() + 4 * HC, (wide, wide)
            bufs = [lr]
        else:
            b_l, b_r = _guarded(N * HC, dev), _guarded(N * HC, dev)
            p_l, p_r, ld_out = b_l.data_ptr(), b_r.data_ptr(), ((0, 0) if f16 else ())
            bufs = [b_l, b_r]
        b_e, b_a = _guarded(E * HC, dev), _guarded(blocks * HC, dev)
        b_m = _guarded(E, dev) if self.mk != "none" else None
        if strides is not None:
            ld_in, ld_out = tuple(strides[:3]), tuple(strides[3:])
        rs, es, ds = self.plan.source_csr()
        nm = self.mask.reshape(-1).data_ptr() if self.mk == "node" else 0
        em = self.mask.reshape(-1).data_ptr() if self.mk == "edge" else 0
        rc = lib.isg_gatv2_mp_bwd_f16 if f16 else lib.isg_gatv2_mp_bwd
        status = rc(x_l.data_ptr(), x_r.data_ptr(), e.data_ptr() if E > 0 else 0, self.att.data_ptr(),
                    self.alpha.data_ptr() if E > 0 else 0, self.w.data_ptr(), self.plan.rowptr.data_ptr(), self.plan.eid.data_ptr(),
                    self.plan.src.data_ptr(), rs.data_ptr(), es.data_ptr(), ds.data_ptr(), nm, em, p_l, p_r, b_e.data_ptr(),
                    b_a.data_ptr(), 0 if b_m is None else b_m.data_ptr(), N, E, H, C, float(self.slope), *ld_in, *ld_out,
                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        bad = []
        for src, was in keep:
            if not torch.equal(src.view(torch.int16), was.view(torch.int16)):
                bad.append("an input buffer changed")
        everything = bufs + [b_e, b_a] + ([b_m] if b_m is not None else [])
        if status != 0 or N == 0:
            if not all(_untouched(b) for b in everything):
                bad.append(f"status {status}, N = {N}: a result buffer was written")
            return status, None, bad
        if f16 and strided:
            rows = lr[:N * wide].view(N, wide)
            d_l, d_r = rows[:, :HC], rows[:, HC:2 * HC]
            if not _untouched(rows[:, 2 * HC:].contiguous()) or not _untouched(lr[N * wide:]):
                bad.append("d_x_l | d_x_r: an unused column or a guard word was written")
        else:
            d_l, d_r = b_l[:N * HC].view(N, HC), b_r[:N * HC].view(N, HC)
            if not _untouched(b_l[N * HC:]) or not _untouched(b_r[N * HC:]):
                bad.append("d_x_l / d_x_r: a guard word was written")
        if not (_untouched(b_e[E * HC:]) and _untouched(b_a[blocks * HC:]) and (b_m is None or _untouched(b_m[E:]))):
            bad.append("d_e_proj / d_att_partial / d_edge_mask: a guard word was written")
        return status, (d_l, d_r, b_e[:E * HC].view(E, HC), b_a[:blocks * HC].view(blocks, HC), None if b_m is None else b_m[:E]), bad


@gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=_mp_id)
def test_half_rows_give_the_bits_of_fp32_rows(dev, case):
    """Every (H, P) instantiation, a 1100-in-edge destination (parking beyond MP_LCAP, slots beyond MP_ECAP), N = 16 / 17, E = 0,
    N = 0, single nodes, node / edge / no mask, slopes 0, 0.2 and 1.5: the half kernels do the fp32 kernels' arithmetic."""
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib_mp_f16_train
    r = Rows(case, dev)
    assert 1 <= passes(r.H, r.C) <= 8
    status, ref, bad = r.entry(False)
    assert status == 0 and not bad, (status, bad)
    strict = _lib_mp_f16_train._lib.bind(ctypes.CDLL(ge.STRICT_LIB), _lib_mp_f16_train.SIGNATURES)
    for what, kw in (("dense", {}), ("strided", {"strided": True}), ("dense again", {}), ("strided again", {"strided": True}),
                     ("strict dense", {"lib": strict}), ("strict strided", {"lib": strict, "strided": True})):
        status, got, problems = r.entry(True, **kw)
        assert status == 0, (what, status)
        bad += [f"{what}: {p}" for p in problems]
        if r.N == 0:
            assert got is None and ref is None
            continue
        for name, a, b in zip(OUT_NAMES, got, ref):
            if b is None:
                assert a is None and r.mk == "none", name
            elif not _same(a, b):
                diff = int((_words(a) != _words(b)).sum())
                bad.append(f"{what}: {name} differs from the fp32-row kernel in {diff} of {b.numel()} words")
    assert not bad, _mp_id(case) + ":\n  " + "\n  ".join(bad)


@gpu
def test_the_wrapper_returns_the_kernels_results_and_fills_a_callers_buffer(dev):
    from isubgvqa_amd import ops
    case = ("small", 4, 300, "edge", 0.2)
    r = Rows(case, dev)
    with torch.no_grad():
        ref = ops.gatv2_mp_backward(r.x_l.float(), r.x_r.float(), r.e.float(), r.att, r.alpha, r.w, r.plan, r.H, negative_slope=r.slope,
                                    want_mask_grad=True, **r.kw)
        ops.reset_counters()
        dense = ops.gatv2_mp_backward_f16(r.x_l, r.x_r, r.e, r.att, r.alpha, r.w, r.plan, r.H, negative_slope=r.slope,
                                          want_mask_grad=True, **r.kw)
        xlr = torch.cat([r.x_l, r.x_r], dim=1)
        buf = torch.full((r.N, 2 * r.HC), float("nan"), device=dev)
        strided = ops.gatv2_mp_backward_f16(xlr[:, :r.HC], xlr[:, r.HC:], r.e, r.att, r.alpha, r.w, r.plan, r.H, negative_slope=r.slope,
                                            want_mask_grad=True, d_x_lr=buf, **r.kw)
        assert ops.counters()["mp_f16_train"] == 2
        with pytest.raises(Exception, match="fp32 feature rows only"):
            ops.gatv2_mp_backward_f16(r.x_l, r.x_r, r.e, r.att, r.alpha, r.w, r.plan, r.H, dropout_p=0.1, **r.kw)
        with pytest.raises(ValueError, match="d_x_lr"):
            ops.gatv2_mp_backward_f16(r.x_l, r.x_r, r.e, r.att, r.alpha, r.w, r.plan, r.H, d_x_lr=buf[:, :r.HC], **r.kw)
    assert strided[0].data_ptr() == buf.data_ptr() and strided[1].data_ptr() == buf.data_ptr() + 4 * r.HC
    assert _same(buf, torch.cat([ref[0], ref[1]], dim=1))
    for got in (dense, strided):
        for name, a, b in zip(MP_NAMES + ("d edge mask",), got, ref):
            assert _same(a, b), name


# ---- 2: the fp64 rule -------------------------------------------------------------------------------------------------------
def _oracle_on_rounded_rows(case, dtype):
    """test_gpu_backward_fp64.mp_oracle with x_l, x_r and e_proj rounded to half first: the function the half entry point is the
    backward of."""
    from oracle import model as OM
    topo, H, C, mk, slope = case
    batch, ei, _ = topology(topo)
    t = mp_inputs(case)
    N, E = batch.numel(), ei.size(1)
    rounded = {k: (t[k].half().float() if k in ("x_l", "x_r", "e_proj") else t[k]) for k in ("x_l", "x_r", "e_proj", "att", "bias")}
    leaves = [rounded[k].to(dtype).clone().requires_grad_(True) for k in ("x_l", "x_r", "e_proj", "att", "bias")]
    m = em = None
    with _one_thread():
        if mk != "none":
            m = t["mask"].to(dtype).clone().requires_grad_(True)
            em = _NodeToEdge.apply(m, ei) if mk == "node" else m
        out, _ = OM.gatv2_message_passing(leaves[0].view(N, H, C), leaves[1].view(N, H, C), leaves[2].view(E, H, C), leaves[3], ei,
                                          em, slope)
        out = out.reshape(N, H * C) + leaves[4]
        (out * t["w"].to(dtype)).sum().backward()
    return [_grad(v) for v in leaves], None if m is None else _grad(m)


@gpu
@pytest.mark.parametrize("case", HUB_CASES + [("small", H, C, "edge", 0.2) for H, C in SMALL_PARTIAL], ids=_mp_id)
def test_half_row_backward_against_fp64(dev, case):
    from isubgvqa_amd import ops
    r = Rows(case, dev)
    g64, m64 = _oracle_on_rounded_rows(case, torch.float64)
    g32, m32 = _oracle_on_rounded_rows(case, torch.float32)
    with torch.no_grad():
        got = ops.gatv2_mp_backward_f16(r.x_l, r.x_r, r.e, r.att, r.alpha, r.w, r.plan, r.H, negative_slope=r.slope,
                                        want_mask_grad=r.mk != "none", **r.kw)
        d_mask = None
        if r.mk == "node":
            d_mask = ops.node_to_edge_mask_backward(got[5], r.plan).view_as(r.mask)
        elif r.mk == "edge":
            d_mask = got[5].view_as(r.mask)
    judge = Judge(_mp_id(case) + " half rows", MP_CAP)
    for name, a, b64, b32 in zip(MP_NAMES, got, g64, g32):
        judge(name, a.view(b64.shape), b64, b32)
    if d_mask is not None:
        judge(f"d {r.mk} mask", d_mask, m64, m32)
    judge.done()


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------
@gpu
def test_bad_strides_and_shapes_without_a_kernel_write_nothing(dev):
    r = Rows(("small", 4, 8, "edge", 0.2), dev)
    HC = r.HC
    for k in range(5):
        for stride in (2, HC - 4, HC + 2):
            ld = [0] * 5
            ld[k] = stride
            status, got, bad = r.entry(True, strides=ld)
            assert status == EINVAL and got is None and not bad, (k, stride, status, bad)
    for H, C in ((3, 8), (4, 6)):
        status, got, bad = r.entry(True, H=H, C=C)
        assert status == EUNSUPPORTED and got is None and not bad, (H, C, status, bad)
    status, got, bad = r.entry(True)
    assert status == 0 and got is not None and not bad


# ---- 4: the Function --------------------------------------------------------------------------------------------------------
FN_SHAPES = [(2, 16, 16, 8), (4, 128, 128, 64), (8, 12, 12, 4)]       # H, C, Cin, K


@gpu
@pytest.mark.parametrize("topo", ["small", "n17"])
@pytest.mark.parametrize("shape", FN_SHAPES, ids=lambda s: "H%d-C%d-Cin%d-K%d" % s)
def test_conv_half_rows_is_the_inference_forward_and_the_hand_composed_backward(dev, topo, shape):
    from isubgvqa_amd import autograd as AG
    from isubgvqa_amd import ops
    H, C, Cin, K = shape
    HC = H * C
    batch, ei, B = topology(topo)
    N, E = batch.numel(), ei.size(1)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
    gen = torch.Generator().manual_seed(100 * H + C + N)
    rn = lambda *s: torch.randn(*s, generator=gen)
    host = {"x": rn(N, Cin), "ea": rn(E, K), "wl": rn(HC, Cin) / math.sqrt(Cin), "bl": rn(HC), "wr": rn(HC, Cin) / math.sqrt(Cin),
            "br": rn(HC), "we": rn(HC, K) / math.sqrt(K), "att": rn(1, H, C) / math.sqrt(C), "bias": rn(HC), "w": rn(N, HC),
            "node": 0.25 + 1.5 * torch.rand(N, 1, generator=gen), "edge": 0.25 + 1.5 * torch.rand(E, 1, generator=gen)}
    host["node"][::3] = 0.0
    host["edge"][::4] = 0.0
    bad = []
    for shared in (False, True):
        for mk in ("none", "node", "edge"):
            leaf = {k: v.to(dev).requires_grad_(True) for k, v in host.items() if k != "w"}
            w = host["w"].to(dev)
            lin_l = torch.nn.Linear(Cin, HC)
            lin_r = lin_l if shared else torch.nn.Linear(Cin, HC)
            lin_l.weight, lin_l.bias = torch.nn.Parameter(leaf["wl"].detach()), torch.nn.Parameter(leaf["bl"].detach())
            if not shared:
                lin_r.weight, lin_r.bias = torch.nn.Parameter(leaf["wr"].detach()), torch.nn.Parameter(leaf["br"].detach())
            nm = leaf["node"] if mk == "node" else None
            em = leaf["edge"] if mk == "edge" else None
            ops.reset_counters()
            out, alpha = AG.conv_half_rows(leaf["x"], leaf["ea"], lin_l, lin_r, leaf["we"], leaf["att"], leaf["bias"], nm, em, plan,
                                           H, 0.2)
            assert out.dtype == torch.float32 and out.requires_grad and not alpha.requires_grad
            saved = [t for t in out.grad_fn.saved_tensors if t is not None]
            rows = [t for t in saved if t.dim() == 2 and t.size(1) in (HC, 2 * HC) and t.size(0) in (N, E)]
            assert sorted(tuple(t.shape) for t in rows) == sorted([(N, HC if shared else 2 * HC), (E, HC)]), [t.shape for t in rows]
            assert all(t.dtype == torch.float16 for t in rows), "a saved feature row is not half"
            (out * w).sum().backward()
            assert ops.counters()["mp_f16_train"] == 1
            # the inference calls and the chain composed by hand
            with torch.no_grad():
                wc = lin_l.weight if shared else torch.cat([lin_l.weight, lin_r.weight])
                bc = lin_l.bias if shared else torch.cat([lin_l.bias, lin_r.bias])
                x_lr = ops.linear(leaf["x"], wc, bc, out_dtype=torch.float16)
                e_h = ops.linear(leaf["ea"], leaf["we"], None, out_dtype=torch.float16)
                x_l, x_r = (x_lr, x_lr) if shared else (x_lr[:, :HC], x_lr[:, HC:])
                mkw = {"node_mask": nm} if mk == "node" else {"edge_mask": em} if mk == "edge" else {}
                ref_out, ref_alpha = ops.gatv2_mp(x_l, x_r, e_h, leaf["att"], plan, H, bias=leaf["bias"], negative_slope=0.2, **mkw)
                assert ref_out.dtype == torch.float16
                d_xl, d_xr, d_e, d_att, d_bias, d_m = ops.gatv2_mp_backward(
                    x_l.float().contiguous(), x_r.float().contiguous(), e_h.float(), leaf["att"], ref_alpha, w, plan, H,
                    negative_slope=0.2, want_mask_grad=mk != "none", **mkw)
                d_mask = None
                if mk == "node":
                    d_mask = ops.node_to_edge_mask_backward(d_m, plan).view_as(nm)
                elif mk == "edge":
                    d_mask = d_m.view_as(em)
            xa, wa, ba = leaf["x"].detach().requires_grad_(True), wc.detach().requires_grad_(True), bc.detach().requires_grad_(True)
            AG.linear(xa, wa, ba, False).backward(d_xl + d_xr if shared else torch.cat([d_xl, d_xr], dim=1))
            ea, we = leaf["ea"].detach().requires_grad_(True), leaf["we"].detach().requires_grad_(True)
            AG.linear(ea, we, None, False).backward(d_e)
            pairs = [("out", out, ref_out.float()), ("alpha", alpha, ref_alpha), ("d x", leaf["x"].grad, xa.grad),
                     ("d edge_attr", leaf["ea"].grad, ea.grad), ("d lin_l.weight", lin_l.weight.grad, wa.grad[:HC]),
                     ("d lin_l.bias", lin_l.bias.grad, ba.grad[:HC]), ("d lin_edge.weight", leaf["we"].grad, we.grad),
                     ("d att", leaf["att"].grad, d_att.view(1, H, C)), ("d bias", leaf["bias"].grad, d_bias)]
            if not shared:
                pairs += [("d lin_r.weight", lin_r.weight.grad, wa.grad[HC:]), ("d lin_r.bias", lin_r.bias.grad, ba.grad[HC:])]
            if mk != "none":
                pairs.append((f"d {mk} mask", (nm if mk == "node" else em).grad, d_mask))
            for name, a, b in pairs:
                if a is None:
                    bad.append(f"shared={shared} {mk}: {name} has no gradient")
                elif not _same(a.detach(), b.detach()):
                    bad.append(f"shared={shared} {mk}: {name} differs in {int((_words(a.detach()) != _words(b.detach())).sum())} "
                               f"of {b.numel()} words")
    assert not bad, "\n  ".join(bad)


# ---- 5: the module ----------------------------------------------------------------------------------------------------------
def _batch_of(sizes, K, seed):
    gen = torch.Generator().manual_seed(seed)
    src, dst, off = [], [], 0
    for n in sizes:
        src += list(range(off, off + n)) + (off + torch.randint(0, n, (2 * n,), generator=gen)).tolist()
        dst += list(range(off, off + n)) + (off + torch.randint(0, n, (2 * n,), generator=gen)).tolist()
        off += n
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ei = torch.tensor([src, dst])
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)]
    return batch, ei, torch.randn(off, 128, generator=gen), torch.randn(ei.size(1), K, generator=gen), \
        torch.randn(len(sizes), 128, generator=gen), torch.randn(len(sizes), 128, generator=gen), torch.randn(off, 512, generator=gen)


SIZES_12 = [5, 64, 9, 17, 33, 48, 12, 25, 60, 7, 40, 21]


def _conv(dev, masked=False, dropout=0.0, dtype=torch.float16):
    from isubgvqa_amd.models.mgat_v2_conv import MaskingGATv2Conv
    torch.manual_seed(4)
    m = MaskingGATv2Conv(128, 128, heads=4, edge_dim=64, add_self_loops=False, dropout=dropout, use_instr=True,
                         masking_threshold=0.15 if masked else 1.0, use_topk=True, sampler_type="imle", sample_k=5)
    m.feature_dtype = dtype
    with torch.no_grad():
        m.bias.add_(0.05 * torch.randn(m.bias.shape))
    return m.to(dev).train()


@gpu
def test_a_half_row_layer_trains(dev):
    """MaskingGATv2Conv(128, 128, heads=4, edge_dim=64), feature_dtype = half, train(): before this feature lin_edge under
    autograd raised IsgError("fp16 feature rows are an inference feature ...")."""
    from isubgvqa_amd import ops
    batch, ei, x, ea, ins, glf, w = (t.to(dev) for t in _batch_of(SIZES_12, 64, 3))
    conv = _conv(dev)
    ops.reset_counters()
    out, mask = conv(x, ei, batch, edge_attr=ea, instruction=ins, imle_att=glf)
    assert mask is None and out.dtype == torch.float32 and out.requires_grad
    (out * w).sum().backward()
    assert ops.counters()["mp_f16_train"] == 1
    for k, p in conv.named_parameters():
        if k.startswith("mask."):
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    with torch.no_grad():
        ref, _ = conv(x, ei, batch, edge_attr=ea, instruction=ins, imle_att=glf)
    assert ref.dtype == torch.float16 and _same(out.detach(), ref.float())
    assert ops.counters()["mp_f16_train"] == 1                                      # inference did not come through here


@gpu
def test_a_masked_half_row_layer_trains_its_gate(dev):
    from isubgvqa_amd import ops
    batch, ei, x, ea, ins, glf, w = (t.to(dev) for t in _batch_of(SIZES_12, 64, 5))
    conv = _conv(dev, masked=True)
    ops.reset_counters()
    out, mask = conv(x, ei, batch, edge_attr=ea, instruction=ins, imle_att=glf, seed=11)
    assert mask is not None and out.dtype == torch.float32
    (out * w).sum().backward()
    assert ops.counters()["mp_f16_train"] == 1
    for k, p in conv.named_parameters():                 # (mask.gate_nn and mask.gate_top are not on this path)
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), k
        assert p.grad is not None or k.startswith(("mask.gate_nn", "mask.gate_top")), k
    for part in ("mask.node_nn", "mask.ques_nn"):
        grads = [p.grad for k, p in conv.named_parameters() if k.startswith(part)]
        assert grads and all(float(g.abs().max()) > 0 for g in grads), part


@gpu
def test_attention_dropout_on_half_rows_keeps_its_error(dev):
    batch, ei, x, ea, ins, glf, w = (t.to(dev) for t in _batch_of(SIZES_12, 64, 3))
    conv = _conv(dev, dropout=0.1)
    with pytest.raises(RuntimeError, match="attention dropout"):
        conv(x, ei, batch, edge_attr=ea, instruction=ins, imle_att=glf, seed=3)


@gpu
def test_a_batch_with_an_oversize_graph_trains_on_fp32_rows(dev):
    from isubgvqa_amd import ops
    batch, ei, x, ea, ins, glf, w = (t.to(dev) for t in _batch_of([257, 10, 20], 64, 7))
    half = _conv(dev)
    full = copy.deepcopy(half)
    full.feature_dtype = torch.float32
    ops.reset_counters()
    outs = []
    for conv in (half, full):
        out, _ = conv(x, ei, batch, edge_attr=ea, instruction=ins, imle_att=glf)
        (out * w).sum().backward()
        outs.append(out.detach())
    assert ops.counters()["mp_f16_train"] == 0
    assert _same(outs[0], outs[1])
    for (k, a), (_, b) in zip(half.named_parameters(), full.named_parameters()):
        if k.startswith("mask."):
            continue
        assert a.grad is not None and _same(a.grad, b.grad), k


# ---- 6: the model -----------------------------------------------------------------------------------------------------------
@gpu
def test_the_answer_model_takes_a_training_step_on_half_rows(dev):
    """Forward loss against oracle.model with fp16_features=True: within 1e-3, the bound the fp16 mode is held to."""
    import dataclasses
    from isubgvqa_amd import ops, optim, synthetic, train
    from oracle import model as OM
    from oracle import samplers as OS
    cfg = synthetic.WorkloadConfig(num_graphs=12, channels=128, layers=2, masks=(1.0, 0.15), sampler="imle", sample_k=5,
                                   nodes_dist="uniform", nodes_min=8, nodes_max=200, edges_per_graph=0.0, degree="powerlaw",
                                   feature_dtype="fp16", seed=31)
    wl = synthetic.make_workload(cfg)
    assert 8 <= int(wl.graph_sizes[0].min()) and 64 < int(wl.graph_sizes[0].max()) <= 200
    gen = torch.Generator().manual_seed(9)
    noises = {1: OS.uniform_to_gumbel(torch.rand(cfg.num_graphs, 1, wl.max_nodes, 1, generator=gen), 0.0, 0.3)}
    target = torch.randint(0, 1842, (cfg.num_graphs,), generator=gen)

    def build(c):
        m = synthetic.build_answer_model(c).to(dev).train()
        for conv in m.gat_seq.convs:
            conv.mask.gate_dropout = 0.0
        m.embedding[2].p = 0.0
        return m

    model, twin = build(cfg), build(dataclasses.replace(cfg, feature_dtype="fp32"))
    assert all(c.feature_dtype == torch.float16 for c in model.gat_seq.convs)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if v.is_floating_point()}
    ins = {"wl": wl.to(dev), "noises": {i: n.to(dev) for i, n in noises.items()}}
    grads = []
    for m in (model, twin):
        logits = m(**ins)[0]
        torch.nn.functional.cross_entropy(logits, target.to(dev)).backward()
        grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
        m.zero_grad(set_to_none=True)
    missing = [k for k in grads[1] if k not in grads[0]]
    assert not missing, f"no gradient on half rows: {missing}"
    for k, g in grads[0].items():
        assert bool(torch.isfinite(g).all()), k
    for k, g in grads[1].items():
        scale = float(g.abs().max())
        dev_k = float((grads[0][k] - g).abs().max()) / scale if scale > 0 else 0.0
        print(f"[f16 train] {k}: max |g_half - g_fp32| / max |g_fp32| = {dev_k:.3e}")
    ops.reset_counters()
    opt = optim.Adam(model.parameters(), lr=1e-3, max_grad_norm=2.0)
    meters = train.Meters(dev)
    res = train.train_step(model, opt, ins, target.to(dev), meters)
    torch.cuda.synchronize()
    assert ops.counters()["mp_f16_train"] == cfg.layers
    rep = meters.report()
    assert rep["steps"] == 1 and rep["skipped_steps"] == 0 and rep["nonfinite_losses"] == 0
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(p.detach().cpu(), sd[k]) for k, p in model.named_parameters())
    ocfg = OM.PathConfig(heads=cfg.heads, masking_thresholds=list(cfg.masks), use_topk=True, sampler_type="imle", sample_k=5,
                         fp16_features=True, training=True)
    with torch.no_grad():
        ref_logits = OM.mgat_pool_classify(sd, wl.x, wl.edge_index, wl.edge_attr, wl.batch, wl.instr, wl.glf, ocfg, noises)[0]
        ref_loss = float(torch.nn.functional.cross_entropy(ref_logits, target))
    loss = float(res.loss.detach())
    print(f"[f16 train] loss {loss:.6f}, oracle (fp16_features) {ref_loss:.6f}, |diff| = {abs(loss - ref_loss):.3e}")
    assert abs(loss - ref_loss) < 1e-3
