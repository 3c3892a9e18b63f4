"""Training of the question side on the library's kernels (include/isg_train.h, csrc/isg_text_bwd.hip, autograd.py,
models/text_encoder.py): the backward of the short-sequence attention and of add + LayerNorm, the dropout a backward
regenerates, ReLU in autograd.linear, and the question encoder / program decoder under autograd.

The rule is tests/test_gpu_text_kernels_fp64.py's.  Reference: the formula in plain torch on the CPU in float64, differentiated by
torch autograd.  Yardstick: the SAME formula in float32 on the CPU.  For every result

    e_k  = max |kernel - ref64| / max |ref64|          e_32 = max |formula32 - ref64| / max |ref64|

and the test asserts  e_k <= max(F * e_32, FLOOR),  FLOOR = 2e-6; where the float64 reference is identically zero the kernel's
result must be exact zeros.  Every figure is printed before anything is asserted and goes through conftest.parity_record.

Dropout: no mask is stored anywhere, so the references take the keep masks as EXPLICIT tensors made on the host from
oracle/philox.py by the keep rule of include/isg_train.h (`keep_mask` below), multiplied by float32(1) / (float32(1) - float32(p)).

Measured on the MI355X, from this tree (e_k / e_32 per comparison; "above the floor" = the comparisons with e_k > FLOOR, where F
decides, with the largest ratio among them):

    part                                     comparisons   max e_k    e_32 range          max ratio   above the floor
    attention "plain"   out                  18            3.9e-7     0 .. 3.9e-7         1.3         --
    attention "plain"   d_q / d_k / d_v      74            7.6e-7     0 .. 7.1e-7         3.4         --
    attention "sharp"   out                  26            1.7e-6     0 .. 1.7e-6         6.4         --
    attention "sharp"   d_q / d_k / d_v      74            2.9e-6     0 .. 3.5e-6         8.5         1.04  (3 comparisons)
    attention "shift"   out                  26            2.8e-6     0 .. 2.8e-6         1.1         1.13  (18)
    attention "shift"   d_q / d_k / d_v      74            2.9e-6     0 .. 3.0e-6         1.3         1.09  (22)
    attention "neginf"  out                  26            8.1e-7     0 .. 8.1e-7         1.3         --
    attention "neginf"  d_q / d_k / d_v      74            6.8e-7     0 .. 6.8e-7         2.2         --
    attention, exact zeros demanded          32            all exact (one key: d_q, d_k; a single key dropped at p = 0.5: out, d_v)
    attention through torch (fallback)       3 + 1         5.4e-7     3.3e-7 .. 5.3e-7    1.6         --
    LayerNorm N(0, 1)        out             248           2.0e-7     3.7e-8 .. 4.9e-7    3.5         --
    LayerNorm N(0, 1)        gradients       768           3.0e-7     0 .. 1.4e-6         4.5         --
    LayerNorm 1000 + N(0, 1) out             256           2.5e-4     5.5e-8 .. 4.3e-4    1.3         1.20  (80)
    LayerNorm 1000 + N(0, 1) gradients       768           7.2e-4     0 .. 2.4e-3         1.9         1.11  (124)
    autograd.linear with ReLU                8 + 2 masks   5.4e-7     9.8e-8 .. 3.2e-7    1.9         --
    modules: p = 0, eval(), switch off       228           4.3e-7     7.1e-8 .. 6.2e-7    2.1         --
    modules at T = 100                       4             5.9e-7     2.5e-7 .. 4.1e-7    1.4         --

(The large ratios all lie below the floor, where e_32 is a few 1e-8 and F does not decide.  The 1000 + N(0, 1) rows with a
dropout mask on them are rows of 0 and 1111: the float32 formula itself is off by 1e-4 .. 1e-3 there and the kernels stay below
it.)  F = 4: the smallest of 2, 4, 8 that leaves a factor of 2 over the largest ratio among the comparisons it decides (1.20).
Every bit-for-bit check (second calls, p = 0 against the inference kernels, packed against separate tensors, the kept sets and
kept values against the host rule for three seeds, same seed twice through the modules and through the full model) held on the
first run.

Two things the first run showed were mistakes of this file, not of the kernels, and are mended here: the float64 references of
the modules now call nn.TransformerEncoder / nn.TransformerDecoder directly with the float mask in float64 (see _run_modules:
torch's CPU attention misreads a float32 mask beside float64 activations from about 33 keys on), and "T = 100 falls back to torch"
is asserted where it is true -- at head width 64; at G4's head width 8 a hundred keys fit both attention kernels (13 KB / 94 KB of
LDS), the call stays on them, and its result is held to the same rule.  One case was added to the attention shapes, (2, 2, 8, 6,
20): none of the others reaches the PARTS = 2 instantiation of the kernels.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from conftest import parity_record

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
F = 4
ISG_EUNSUPPORTED = -2       # include/isg.h
LDS_FWD, LDS_BWD = 64 * 1024, 160 * 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


class Judge:
    """Collects every comparison of one test; prints each figure before anything is asserted, and puts them on record."""

    def __init__(self, case):
        self.case, self.bad, self.rows = case, [], {}

    def __call__(self, name, got, ref64, ref32):
        got = got.detach().cpu()
        if tuple(got.shape) != tuple(ref64.shape):
            self.bad.append(f"{name}: shape {tuple(got.shape)}, reference {tuple(ref64.shape)}")
            return
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f"{name}: not finite")
            return
        scale = float(ref64.abs().max()) if ref64.numel() else 0.0
        if scale == 0.0:
            worst = float(got.abs().max()) if got.numel() else 0.0
            print(f"[fp64] {self.case} | {name} | exact zero expected, max |kernel| = {worst:.3e}")
            self.rows[name] = {"exact_zero_expected": True, "max_abs_kernel": worst}
            if worst != 0.0:
                self.bad.append(f"{name}: reference is identically zero, kernel has {worst:.3e}")
            return
        e_k = float((got.double() - ref64).abs().max()) / scale
        e_32 = float((ref32.double() - ref64).abs().max()) / scale
        bound = max(F * e_32, FLOOR)
        ratio = e_k / max(e_32, 1e-30)
        print(f"[fp64] {self.case} | {name} | e_k={e_k:.3e} e_32={e_32:.3e} ratio={ratio:.2f}" + ("  ABOVE-FLOOR" if e_k > FLOOR else ""))
        self.rows[name] = {"e_k": e_k, "e_32": e_32, "ratio": ratio if e_32 > 0 else None}
        if not e_k <= bound:
            self.bad.append(f"{name}: e_k = {e_k:.3e} > max({F} * e_32, floor) = {bound:.3e}  (e_32 = {e_32:.3e})")

    def same_bits(self, name, a, b):
        if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape) or not torch.equal(a, b):
            self.bad.append(f"{name}: not the same bits")

    def check(self, ok, text):
        if not ok:
            self.bad.append(text)

    def done(self):
        parity_record(f"text_train {self.case}", self.rows)
        assert not self.bad, f"{self.case}:\n  " + "\n  ".join(self.bad)


class _one_thread:
    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


# ---- the keep rule on the host ------------------------------------------------------------------------------------------------
def keep_mask(seed: int, M: int, D: int, p: float) -> torch.Tensor:
    """bool [M, D]: element (i, j) is kept iff uniform24(word[j & 3] of philox4x32_10((i, j >> 2, 0x1571, 0x9E37), seed)) >= p."""
    from oracle import philox
    if p == 0:
        return torch.ones(M, D, dtype=torch.bool)
    seed &= 2 ** 64 - 1
    nq = (D + 3) // 4
    words = philox.philox4x32_10((np.arange(M, dtype=np.uint64)[:, None], np.arange(nq, dtype=np.uint64)[None, :], philox.C2, philox.C3),
                                 (seed & 0xFFFFFFFF, seed >> 32))
    u = philox.uniform24(np.stack(words, axis=2).reshape(M, nq * 4)[:, :D])
    return torch.from_numpy(np.ascontiguousarray(u >= np.float32(p)))


def inv_keep(p: float) -> float:
    """float32(1) / (float32(1) - float32(p)), as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ==========================================================================================================================
# Part 1: attention
# ==========================================================================================================================
# (B, H, hd, Tq, Tk)
ATTN_CASES = [(1, 1, 4, 1, 1), (3, 2, 16, 5, 5), (2, 8, 64, 12, 12), (2, 8, 64, 4, 12), (2, 1, 64, 4, 65), (1, 1, 32, 3, 128),
              (1, 2, 20, 7, 9), (1, 2, 64, 77, 77),
              (2, 2, 8, 6, 20)]       # PARTS = 2 (17 .. 32 keys, 8 | hd), which none of the above reaches
ATTN_CLASSES = ("plain", "sharp", "shift", "neginf")
ATTN_PS = (0.0, 0.1, 0.5)
ATTN_SEED = 0x1234_5678_9ABC


def _attn_id(case):
    return "B%d-H%d-hd%d-Tq%d-Tk%d" % case


@functools.lru_cache(maxsize=None)
def attn_inputs(case, cls):
    B, H, hd, Tq, Tk = case
    D = H * hd
    gen = torch.Generator().manual_seed(7000 + 10 * ATTN_CASES.index(case) + ATTN_CLASSES.index(cls))
    if Tq == Tk:
        src = (torch.randn(Tq * B, 3 * D, generator=gen),)
    else:
        src = (torch.randn(Tq * B, D, generator=gen), torch.randn(Tk * B, 2 * D, generator=gen))
    q, k, v = attn_operands(case, src)
    bias, dead = None, None
    if cls == "sharp":
        q.mul_(12.0)
    elif cls == "shift":
        bias = 100.0 + torch.rand(B, Tk, generator=gen)
    elif cls == "neginf":
        dead = torch.rand(B, Tk, generator=gen) < 0.4
        dead[:, 0] = False
        bias = torch.zeros(B, Tk).masked_fill_(dead, -math.inf)
        v[dead.t().reshape(-1).nonzero().squeeze(1)] = 1e30          # row s * B + b
    w = torch.randn(Tq * B, D, generator=gen)                        # d_out
    return {"src": src, "bias": bias, "dead": dead, "w": w}


def attn_operands(case, src):
    B, H, hd, Tq, Tk = case
    D = H * hd
    if len(src) == 1:
        return src[0][:, :D], src[0][:, D:2 * D], src[0][:, 2 * D:]
    return src[0], src[1][:, :D], src[1][:, D:]


@functools.lru_cache(maxsize=None)
def attn_keep(case, p):
    B, H, hd, Tq, Tk = case
    return keep_mask(ATTN_SEED, B * H * Tq, Tk, p).view(B, H, Tq, Tk)       # i = (b * H + h) * Tq + t, j = s


@functools.lru_cache(maxsize=None)
def attn_ref(case, cls, p, dtype):
    """(out, d_q, d_k, d_v) of out = (softmax(Q K^T / sqrt(hd) + bias) * keep / (1 - p)) V under d_out = w, in `dtype` on the CPU."""
    B, H, hd, Tq, Tk = case
    t = attn_inputs(case, cls)
    q, k, v = (x.to(dtype).clone().requires_grad_(True) for x in attn_operands(case, t["src"]))
    with _one_thread():
        heads = lambda x, T: x.view(T, B, H, hd).permute(1, 2, 0, 3)
        sc = heads(q, Tq) @ heads(k, Tk).transpose(-1, -2) / math.sqrt(hd)
        if t["bias"] is not None:
            sc = sc + t["bias"].to(dtype)[:, None, None, :]
        pr = torch.softmax(sc, -1) * (attn_keep(case, p).to(dtype) * inv_keep(p))
        out = (pr @ heads(v, Tk)).permute(2, 0, 1, 3).reshape(Tq * B, H * hd)
        (out * t["w"].to(dtype)).sum().backward()
    return out.detach(), q.grad, k.grad, v.grad


def _attn_on_device(case, cls, dev, packed=True):
    t = attn_inputs(case, cls)
    src = tuple(s.to(dev) for s in t["src"])
    q, k, v = attn_operands(case, src)
    if not packed:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return src, q, k, v, None if t["bias"] is None else t["bias"].to(dev), t["w"].to(dev)


def _attn_grads(case, src, packed=True):
    """Gradient storage laid out like the operands: (owners, d_q, d_k, d_v), NaN-filled so that an unwritten element shows."""
    B, H, hd, Tq, Tk = case
    D = H * hd
    if packed:
        own = tuple(torch.full_like(s, math.nan) for s in src)
        return (own,) + attn_operands(case, own)
    dev = src[0].device
    own = (torch.full((Tq * B, D), math.nan, device=dev), torch.full((Tk * B, D), math.nan, device=dev),
           torch.full((Tk * B, D), math.nan, device=dev))
    return (own,) + own


def lds_fwd(hd, Tq, Tk):
    return 4 * (Tk * (2 * hd + 4) + Tq * hd + 4 * 128)


def lds_bwd(hd, Tq, Tk):
    return 4 * (2 * Tk * (hd + 4) + 2 * Tq * hd + 2 * Tq * Tk)


@pytest.mark.parametrize("case", ATTN_CASES, ids=_attn_id)
def test_mha_small_train_and_backward(dev, case):
    """isg_mha_small_train and isg_mha_small_bwd on four input classes and p in {0, 0.1, 0.5}, q / k / v and their gradients
    column slices of one tensor; once on separate tensors; second calls; p = 0 against isg_mha_small."""
    from isubgvqa_amd import ops
    B, H, hd, Tq, Tk = case
    judge = Judge(f"mha_bwd {_attn_id(case)}")
    assert ops.mha_small_train_supported(Tq, Tk, hd) and lds_fwd(hd, Tq, Tk) <= LDS_FWD and lds_bwd(hd, Tq, Tk) <= LDS_BWD
    for cls in ATTN_CLASSES:
        src, q, k, v, kb, w = _attn_on_device(case, cls, dev)
        dead = attn_inputs(case, cls)["dead"]
        for p in ATTN_PS:
            tag = f"{cls} p={p}"
            r64, r32 = attn_ref(case, cls, p, torch.float64), attn_ref(case, cls, p, torch.float32)
            out = ops.mha_small_train(q, k, v, B, H, kb, p, ATTN_SEED)
            judge(f"{tag}: out", out, r64[0], r32[0])
            if p == 0:
                judge.same_bits(f"{tag}: isg_mha_small_train against isg_mha_small", out, ops.mha_small(q, k, v, B, H, kb))
            own, dq, dk, dv = _attn_grads(case, src)
            judge.check(ops.mha_small_backward(q, k, v, B, H, kb, w, dq, dk, dv, p, ATTN_SEED), f"{tag}: backward refused")
            for name, got, i in (("d_q", dq, 1), ("d_k", dk, 2), ("d_v", dv, 3)):
                judge(f"{tag}: {name}", got.contiguous(), r64[i], r32[i])
            if dead is not None:                      # masked keys: no weight, so no gradient -- exact zeros
                rows = dead.t().reshape(-1).nonzero().squeeze(1).to(dev)
                judge.check(rows.numel() == 0 or (float(dk[rows].abs().max()) == 0.0 and float(dv[rows].abs().max()) == 0.0),
                            f"{tag}: d_k / d_v of the masked keys are not exact zeros")
            own2, dq2, dk2, dv2 = _attn_grads(case, src)
            ops.mha_small_backward(q, k, v, B, H, kb, w, dq2, dk2, dv2, p, ATTN_SEED)
            for a, b_ in zip(own, own2):
                judge.same_bits(f"{tag}: second backward call", a, b_)
            judge.same_bits(f"{tag}: second forward call", ops.mha_small_train(q, k, v, B, H, kb, p, ATTN_SEED), out)
            if cls == "plain" and p == 0.1:           # the same on separate contiguous tensors
                _, qs, ks, vs, _, _ = _attn_on_device(case, cls, dev, packed=False)
                _, dqs, dks, dvs = _attn_grads(case, src, packed=False)
                ops.mha_small_backward(qs, ks, vs, B, H, kb, w, dqs, dks, dvs, p, ATTN_SEED)
                for name, a, b_ in (("d_q", dqs, dq), ("d_k", dks, dk), ("d_v", dvs, dv)):
                    judge.same_bits(f"{tag}: {name} on separate tensors", a, b_.contiguous())
    judge.done()


def test_autograd_mha_small_packs_the_gradient_and_falls_back_beyond_the_limits(dev):
    """autograd.mha_small on slices of a fused projection hands ONE gradient to it (the kernel's bits); a key_bias that requires
    grad is refused; a shape beyond the backward's LDS is ISG_EUNSUPPORTED at the ABI, and the operator runs torch's ops, counted."""
    from isubgvqa_amd import _lib_train, autograd, ops
    judge = Judge("mha autograd")
    case, cls, p = (2, 8, 64, 12, 12), "plain", 0.1
    B, H, hd, Tq, Tk = case
    src, q, k, v, kb, w = _attn_on_device(case, cls, dev)
    own, dq, dk, dv = _attn_grads(case, src)
    ops.mha_small_backward(q, k, v, B, H, kb, w, dq, dk, dv, p, ATTN_SEED)
    leaf = src[0].clone().requires_grad_(True)
    proj = leaf * 1.0                                  # a non-leaf [T*B, 3D] tensor, as a fused in_proj's result is
    D = H * hd
    out = autograd.mha_small(proj[:, :D], proj[:, D:2 * D], proj[:, 2 * D:], B, H, None, p, ATTN_SEED)
    judge.check(out.grad_fn is not None and "MhaSmall" in type(out.grad_fn).__name__, "autograd.mha_small did not record its Function")
    (out * w).sum().backward()
    judge.same_bits("packed gradient", leaf.grad, own[0])
    with pytest.raises(NotImplementedError):
        autograd.mha_small(q, k, v, B, H, torch.zeros(B, Tk, device=dev, requires_grad=True), 0.0, 0)
    # beyond the limits: the forward's 64 KB hold, the backward's 160 KB do not
    big = (1, 1, 32, 128, 128)
    B, H, hd, Tq, Tk = big
    assert lds_fwd(hd, Tq, Tk) <= LDS_FWD and lds_bwd(hd, Tq, Tk) > LDS_BWD and not ops.mha_small_train_supported(Tq, Tk, hd)
    gen = torch.Generator().manual_seed(5)
    q0, k0, v0, w0 = (torch.randn(128, 32, generator=gen) for _ in range(4))
    qd, kd, vd, wd = (t.to(dev) for t in (q0, k0, v0, w0))
    g = [torch.full((128, 32), -7.25, device=dev) for _ in range(3)]
    lib = _lib_train.load()
    rc = lib.isg_mha_small_bwd(qd.data_ptr(), 32, kd.data_ptr(), 32, vd.data_ptr(), 32, 0, wd.data_ptr(), 32, g[0].data_ptr(), 32,
                               g[1].data_ptr(), 32, g[2].data_ptr(), 32, B, H, hd, Tq, Tk, 0.0, 0, ops._stream())
    torch.cuda.synchronize()
    judge.check(rc == ISG_EUNSUPPORTED, f"isg_mha_small_bwd beyond 160 KB of LDS returned {rc}")
    judge.check(all(bool((t == -7.25).all()) for t in g), "a refused call wrote something")
    judge.check(int(lib.isg_mha_small_bwd_lds_bytes(hd, Tq, Tk)) == lds_bwd(hd, Tq, Tk), "isg_mha_small_bwd_lds_bytes")
    for hd_, tq_, tk_ in ((68, 4, 4), (16, 4, 129), (6, 4, 4)):
        z = torch.zeros(max(tq_, tk_), 2 * hd_ + 2, device=dev)
        rc = lib.isg_mha_small_bwd(z.data_ptr(), hd_, z.data_ptr(), hd_, z.data_ptr(), hd_, 0, z.data_ptr(), hd_, g[0].data_ptr(), hd_,
                                   g[1].data_ptr(), hd_, g[2].data_ptr(), hd_, 1, 1, hd_, tq_, tk_, 0.0, 0, ops._stream())
        judge.check(rc == ISG_EUNSUPPORTED, f"isg_mha_small_bwd(hd={hd_}, Tq={tq_}, Tk={tk_}) returned {rc}")
    for bad_p in (1.0, -0.1):
        rc = lib.isg_dropout(qd.data_ptr(), 32, g[0].data_ptr(), 32, 128, 32, bad_p, 0, ops._stream())
        judge.check(rc == -1, f"isg_dropout(p={bad_p}) returned {rc}")
    refs = []
    for dt in (torch.float64, torch.float32):
        a, b_, c = (t.to(dt).clone().requires_grad_(True) for t in (q0, k0, v0))
        with _one_thread():
            o = torch.softmax(a @ b_.t() / math.sqrt(32), -1) @ c
            (o * w0.to(dt)).sum().backward()
        refs.append((o.detach(), a.grad, b_.grad, c.grad))
    ops.reset_counters()
    a, b_, c = (t.clone().requires_grad_(True) for t in (qd, kd, vd))
    o = autograd.mha_small(a, b_, c, B, H, None, 0.0, 0)
    (o * wd).sum().backward()
    judge.check(ops.counters()["torch_attention_train"] == 1, f"the fallback was not counted: {ops.counters()}")
    for name, got, i in (("out", o, 0), ("d_q", a.grad, 1), ("d_k", b_.grad, 2), ("d_v", c.grad, 3)):
        judge(f"fallback: {name}", got, refs[0][i], refs[1][i])
    judge.done()


# ==========================================================================================================================
# Part 2: add + LayerNorm
# ==========================================================================================================================
LN_DS = [4, 256, 300, 512, 516, 1024, 1056, 2048]      # both sides of every NV template (256 / 512 / 1024 columns)
LN_MS = [1, 3, 9, 1030]
LN_SEED = 0xFEED_F00D_0001
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_inputs(M, D, shifted):
    gen = torch.Generator().manual_seed(100 * D + M + (50000 if shifted else 0))
    x, r = torch.randn(M, D, generator=gen), torch.randn(M, D, generator=gen)
    if shifted:
        x = 1000.0 + x
    return {"x": x, "r": r, "gamma": 1.0 + 0.5 * torch.randn(D, generator=gen), "beta": torch.randn(D, generator=gen),
            "w": torch.randn(M, D, generator=gen)}


@functools.lru_cache(maxsize=None)
def ln_keep(M, D, p):
    return keep_mask(LN_SEED, M, D, p)


def ln_ref(M, D, shifted, with_r, with_beta, p, dtype):
    """(out, d_x, d_r, d_gamma, d_beta) of LayerNorm(r + x * keep / (1 - p)) under d_out = w."""
    t = ln_inputs(M, D, shifted)
    x, r, gamma, beta = (t[n].to(dtype).clone().requires_grad_(True) for n in ("x", "r", "gamma", "beta"))
    with _one_thread():
        v = x * (ln_keep(M, D, p).to(dtype) * inv_keep(p))
        if with_r:
            v = v + r
        out = torch.nn.functional.layer_norm(v, (D,), gamma, beta if with_beta else None, LN_EPS)
        (out * t["w"].to(dtype)).sum().backward()
    return out.detach(), x.grad, r.grad if with_r else None, gamma.grad, beta.grad if with_beta else None


@pytest.mark.parametrize("D", LN_DS)
def test_add_layernorm_backward(dev, D):
    from isubgvqa_amd import _lib_train, ops
    judge = Judge(f"ln_bwd D={D}")
    lib = _lib_train.load()
    for M in LN_MS:
        parts = int(lib.isg_add_layernorm_bwd_parts(M))
        judge.check(parts == min((M + 15) // 16, 1024) and (M != 1030 or parts > 4), f"isg_add_layernorm_bwd_parts({M}) = {parts}")
        for shifted in (False, True):
            t = {n: v.to(dev) for n, v in ln_inputs(M, D, shifted).items()}
            for with_beta in (True, False):
                norm = torch.nn.LayerNorm(D, eps=LN_EPS, bias=with_beta).to(dev)
                with torch.no_grad():
                    norm.weight.copy_(t["gamma"])
                    if with_beta:
                        norm.bias.copy_(t["beta"])
                for with_r in (True, False):
                    r = t["r"] if with_r else None
                    for p in (0.0, 0.1):
                        tag = f"M={M} {'1000+N' if shifted else 'N'} r={int(with_r)} beta={int(with_beta)} p={p}"
                        r64 = ln_ref(M, D, shifted, with_r, with_beta, p, torch.float64)
                        r32 = ln_ref(M, D, shifted, with_r, with_beta, p, torch.float32)
                        out = ops.dropout_add_layernorm(t["x"], r, norm, p, LN_SEED)
                        judge(f"{tag}: out", out, r64[0], r32[0])
                        if p == 0:
                            judge.same_bits(f"{tag}: isg_dropout_add_layernorm against isg_add_layernorm", out,
                                            ops.add_layernorm(t["x"], r, norm, want_rowmax=False))
                        got = ops.add_layernorm_backward(t["x"], r, norm, t["w"], p, LN_SEED)
                        for name, g, i in (("d_x", got[0], 1), ("d_r", got[1], 2), ("d_gamma", got[2], 3), ("d_beta", got[3], 4)):
                            judge.check((g is None) == (r64[i] is None), f"{tag}: {name} is {'missing' if g is None else 'unexpected'}")
                            if g is not None and r64[i] is not None:
                                judge(f"{tag}: {name}", g, r64[i], r32[i])
                        again = ops.add_layernorm_backward(t["x"], r, norm, t["w"], p, LN_SEED)
                        for name, a, b_ in zip(("d_x", "d_r", "d_gamma", "d_beta"), got, again):
                            if a is not None:
                                judge.same_bits(f"{tag}: second call, {name}", a, b_)
                        judge.same_bits(f"{tag}: second forward call", ops.dropout_add_layernorm(t["x"], r, norm, p, LN_SEED), out)
    judge.done()


# ==========================================================================================================================
# Part 3: dropout
# ==========================================================================================================================
def test_dropout_keeps_what_the_host_rule_keeps(dev):
    """isg_dropout's kept set against the host rule, exactly, and kept values x * (1.0f / (1.0f - p)) bit for bit; the attention
    kernel's mask read back through isg_mha_small_train with q = 0 (P = 1 / Tk exactly) and one-hot V rows."""
    from isubgvqa_amd import ops
    judge = Judge("dropout")
    for seed in (0, 0x9E3779B97F4A7C15, 2 ** 64 - 1):
        for M, D in ((1, 4), (7, 300), (33, 2048)):
            for p in (0.1, 0.5):
                x = torch.randn(M, D, generator=torch.Generator().manual_seed(M + D)) + 3.0       # no zeros among the inputs
                got = ops.dropout(x.to(dev), p, seed).cpu()
                keep = keep_mask(seed, M, D, p)
                want = torch.where(keep, x * torch.tensor(inv_keep(p), dtype=torch.float32), torch.zeros(()))
                judge.check(torch.equal(got != 0, keep), f"seed {seed:#x} {M} x {D} p={p}: kept set differs from the host rule")
                judge.same_bits(f"seed {seed:#x} {M} x {D} p={p}: values", got, want)
                frac = float(keep.float().mean())
                judge.check(M * D < 1000 or abs(frac - (1 - p)) < 0.05, f"kept fraction {frac} at p={p}")
        x = torch.randn(7, 300).to(dev)
        judge.same_bits(f"seed {seed:#x}: p = 0 is the identity", ops.dropout(x, 0.0, seed), x)
        # attention: i = (b * H + h) * Tq + t, j = s
        for (B, H, hd, Tq, Tk), p in (((2, 2, 16, 5, 12), 0.1), ((1, 1, 64, 3, 100), 0.5)):
            D = H * hd
            keep = keep_mask(seed, B * H * Tq, Tk, p).view(B, H, Tq, Tk)
            val = (torch.tensor(1.0) / torch.tensor(float(Tk))) * torch.tensor(inv_keep(p), dtype=torch.float32)
            q = torch.zeros(Tq * B, D, device=dev)
            k = torch.randn(Tk * B, D, device=dev)
            seen = torch.zeros(B, H, Tq, Tk)
            for s0 in range(0, Tk, hd):                # keys s0 .. s0 + hd - 1 show in channels 0 .. hd - 1
                v = torch.zeros(Tk, B, H, hd)
                for s in range(s0, min(s0 + hd, Tk)):
                    v[s, :, :, s - s0] = 1.0
                out = ops.mha_small_train(q, k, v.view(Tk * B, D).to(dev), B, H, None, p, seed).cpu()
                n = min(hd, Tk - s0)
                seen[..., s0:s0 + n] = out.view(Tq, B, H, hd).permute(1, 2, 0, 3)[..., :n]
            judge.check(torch.equal(seen != 0, keep), f"seed {seed:#x} attention {Tq} x {Tk} p={p}: kept set differs from the host rule")
            judge.same_bits(f"seed {seed:#x} attention {Tq} x {Tk} p={p}: values", seen, torch.where(keep, val, torch.zeros(())))
    judge.done()


# ==========================================================================================================================
# Part 4: autograd.linear with ReLU
# ==========================================================================================================================
# The inputs keep every pre-activation away from 0 (asserted on the float64 reference: min |z| > 1e-4 against a GEMM error of
# ~1e-6), so that the ReLU's mask is the same in every arithmetic and the gradients are comparable: the bias is +-amp per column,
# which leaves 79 % / 85 % of the columns with both signs among their rows.
@pytest.mark.parametrize("M,N,K,amp,seed", [(12, 2048, 512, 1.0, 3), (2100, 512, 2048, 3.0, 3)])
def test_autograd_linear_relu(dev, M, N, K, amp, seed):
    from isubgvqa_amd import autograd
    judge = Judge(f"linear_relu {M}x{N}x{K}")
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    sign = (torch.rand(N, generator=g) < 0.5).float() * 2 - 1
    b = amp * sign * (1 + 0.1 * torch.rand(N, generator=g))
    go = torch.randn(M, N, generator=torch.Generator().manual_seed(seed + 1))
    refs = []
    for dt in (torch.float64, torch.float32):
        xx, ww, bb = (t.to(dt).clone().requires_grad_(True) for t in (x, w, b))
        z = xx @ ww.t() + bb
        y = torch.relu(z)
        (y * go.to(dt)).sum().backward()
        refs.append((y.detach(), xx.grad, ww.grad, bb.grad, z.detach()))
    assert float(refs[0][4].abs().min()) > 1e-4 and 0.3 < float((refs[0][4] > 0).double().mean()) < 0.7
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    y = autograd.linear(xd, wd, bd, False, relu=True)
    (y * go.to(dev)).sum().backward()
    for name, got, i in (("y", y, 0), ("d_x", xd.grad, 1), ("d_w", wd.grad, 2), ("d_b", bd.grad, 3)):
        judge(name, got, refs[0][i], refs[1][i])
    judge.check(bool(((y.detach().cpu() > 0) == (refs[0][0] > 0)).all()), "the ReLU's mask differs from the reference's")
    with pytest.raises(ValueError):
        autograd.linear(xd, wd, bd, True, relu=True)
    judge.done()


# ==========================================================================================================================
# Part 5: the modules
# ==========================================================================================================================
MODULE_DIMS = {"g4": (32, 4, 64, 6, 3), "real": (512, 8, 2048, 12, 3)}       # ninp, heads, nhid, T, B


def _build_modules(ninp, nhead, nhid, dropout):
    from isubgvqa_amd.models.text_encoder import CLIPTextEmbeddings, QuestionDecoder, QuestionEncoder
    torch.manual_seed(11)
    enc = QuestionEncoder(CLIPTextEmbeddings(200, ninp, 128), ninp, ninp, nhead, nhid, 4, dropout=dropout)
    dec = QuestionDecoder(4, ninp, nhead, nhid, 3, dropout=dropout)
    return enc, dec


def _zero_dropouts(*modules):
    for mod in modules:
        for m in mod.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if isinstance(m, torch.nn.MultiheadAttention):
                m.dropout = 0.0


def _module_inputs(T, B, ninp):
    gen = torch.Generator().manual_seed(T * 100 + B)
    ids = torch.randint(0, 200, (B, T), generator=gen)
    mask = (torch.arange(T)[None] < torch.randint(max(T // 2, 1), T + 1, (B,), generator=gen)[:, None]).long()
    return ids, mask, torch.randn(4, B, ninp, generator=gen)


def _run_modules(enc, dec, ids, mask, w, seed=None, reference=False):
    """(output, d enc_out, parameter gradients by name) of one forward + backward of decoder(encoder(ids)).  reference: torch's own
    nn.TransformerEncoder / nn.TransformerDecoder called directly, the float mask in the modules' dtype (QuestionEncoder.forward
    hands torch a float32 mask, which torch's CPU attention misreads beside float64 activations from about 33 keys on: measured
    here, max |difference| 1.4 at 40 keys, 0 at 12)."""
    for m in (enc, dec):
        m.zero_grad(set_to_none=True)
    if reference:
        dt = enc.transformer_encoder.norm.weight.dtype
        mem = enc.transformer_encoder(enc.text_vocab_embedding(ids).permute(1, 0, 2), src_key_padding_mask=mask.to(dt))
        mem.retain_grad()
        out = dec.coarse_decoder(tgt=dec.query_embed.weight.unsqueeze(1).repeat(1, ids.size(0), 1), memory=mem, tgt_mask=None)
    else:
        mem = enc(ids, mask=mask, **({} if seed is None else {"seed": seed}))
        mem.retain_grad()
        out = dec(memory=mem, **({} if seed is None else {"seed": seed + 4096}))
    (out * w).sum().backward()
    grads = {f"{n0}.{n}": p.grad for n0, m in (("enc", enc), ("dec", dec)) for n, p in m.named_parameters() if p.grad is not None}
    return out.detach(), mem.grad, grads


@pytest.mark.parametrize("dims", list(MODULE_DIMS))
def test_question_modules_train_on_the_kernels(dev, dims):
    from isubgvqa_amd import ops
    from isubgvqa_amd.models import text_encoder as TE
    ninp, nhead, nhid, T, B = MODULE_DIMS[dims]
    judge = Judge(f"modules {dims}")
    ids, mask, w = _module_inputs(T, B, ninp)
    enc, dec = _build_modules(ninp, nhead, nhid, 0.1)
    enc.train(), dec.train()
    # ---- all p = 0, set after construction: against torch's own modules on the CPU ----
    e0, d0 = copy.deepcopy(enc), copy.deepcopy(dec)
    _zero_dropouts(e0, d0)
    with _one_thread():
        r32 = _run_modules(copy.deepcopy(e0), copy.deepcopy(d0), ids, mask, w, reference=True)
        r64 = _run_modules(copy.deepcopy(e0).double(), copy.deepcopy(d0).double(), ids, mask, w.double(), reference=True)
    eg, dg = copy.deepcopy(e0).to(dev), copy.deepcopy(d0).to(dev)
    ops.reset_counters()
    got = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev))
    judge.check(ops.counters()["text_train_kernels"] == 2, f"text_train_kernels = {ops.counters()['text_train_kernels']} after two forwards")
    judge.check(ops.counters()["torch_attention_train"] == 0, "an attention call left the kernels")
    judge("p=0: output", got[0], r64[0], r32[0])
    judge("p=0: d memory", got[1], r64[1], r32[1])
    judge.check(set(got[2]) == set(r64[2]), f"parameters with a gradient differ: {sorted(set(got[2]) ^ set(r64[2]))}")
    for name in sorted(r64[2]):
        if name in got[2]:
            judge(f"p=0: d {name}", got[2][name], r64[2][name], r32[2][name])
    TE.FUSED_TEXT_TRAIN = False
    try:
        ops.reset_counters()
        off = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev))
        judge.check(ops.counters()["text_train_kernels"] == 0, "FUSED_TEXT_TRAIN = False still took the kernels")
        judge("switch off: output", off[0], r64[0], r32[0])
    finally:
        TE.FUSED_TEXT_TRAIN = True
    # ---- the constructors' dropout 0.1 ----
    eg, dg = copy.deepcopy(enc).to(dev), copy.deepcopy(dec).to(dev)
    ops.reset_counters()
    a = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev), seed=77)
    b_ = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev), seed=77)
    c = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev), seed=78)
    judge.check(ops.counters()["text_train_kernels"] == 6, "dropout 0.1: the forwards did not all take the kernels")
    judge.same_bits("dropout 0.1, same seed: output", a[0], b_[0])
    judge.same_bits("dropout 0.1, same seed: d memory", a[1], b_[1])
    for name in a[2]:
        judge.same_bits(f"dropout 0.1, same seed: d {name}", a[2][name], b_[2][name])
    judge.check(not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]), "another seed gave the same bits")
    judge.check(not torch.equal(a[0], got[0]), "dropout 0.1 gave the bits of p = 0")
    torch.manual_seed(5)
    u1 = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev))
    torch.manual_seed(5)
    u2 = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev))
    judge.same_bits("no seed: torch.manual_seed reproduces the run", u1[0], u2[0])
    judge.check(not torch.equal(u1[0], a[0]), "no seed: the bits of seed 77")
    # ---- eval() with autograd recording: every p is 0, the inference walk's result ----
    eg.eval(), dg.eval()
    ops.reset_counters()
    ev = _run_modules(eg, dg, ids.to(dev), mask.to(dev), w.to(dev))
    judge.check(ops.counters()["text_train_kernels"] == 2, "eval() under autograd left the kernels")
    with torch.no_grad():
        inf = dg(memory=eg(ids.to(dev), mask=mask.to(dev)))
    judge("eval() under autograd: output", ev[0], r64[0], r32[0])
    judge("inference walk: output", inf, r64[0], r32[0])
    judge("eval() under autograd: d memory", ev[1], r64[1], r32[1])
    # ---- T = 100: at head width 64 beyond the attention kernels' LDS (the forward's 64 KB hold 80 keys): torch's modules.  At G4's
    # head width 8 a hundred keys fit both kernels (13 KB / 94 KB), so there the same call stays on them; both are held to the rule.
    fits = ops.mha_small_train_supported(100, 100, ninp // nhead)
    judge.check(fits == (dims == "g4"), f"T = 100 at head width {ninp // nhead}: mha_small_train_supported says {fits}")
    ids100, mask100, w100 = _module_inputs(100, 2, ninp)
    with _one_thread():
        q32 = _run_modules(copy.deepcopy(e0).eval(), copy.deepcopy(d0).eval(), ids100, mask100, w100, reference=True)
        q64 = _run_modules(copy.deepcopy(e0).double().eval(), copy.deepcopy(d0).double().eval(), ids100, mask100, w100.double(),
                           reference=True)
    ops.reset_counters()
    far = _run_modules(eg, dg, ids100.to(dev), mask100.to(dev), w100.to(dev))
    judge.check(ops.counters()["text_train_kernels"] == (2 if fits else 0),
                f"T = 100: text_train_kernels = {ops.counters()['text_train_kernels']}" + ("" if fits else ": did not fall back to torch"))
    judge("T=100: output", far[0], q64[0], q32[0])
    judge("T=100: d memory", far[1], q64[1], q32[1])
    judge.done()


def test_full_model_training_step_with_dropout_is_reproducible(dev):
    """One ISubGVQA training step with every dropout left on and a seed: finite loss, a gradient for every parameter, the
    question side on the kernels, and the same bits from a second run."""
    import argparse
    from isubgvqa_amd import ops, synthetic
    from isubgvqa_amd.models import build_model
    from test_gpu_models import _full_args
    torch.manual_seed(0)
    model = build_model(_full_args(sampler_type="imle", mgat_masks=[1.0, 0.15, 1.0, 0.15]), None).train().to(dev)
    gen = torch.Generator().manual_seed(29)
    cfg = synthetic.WorkloadConfig(num_graphs=10, nodes_dist="uniform", nodes_min=2, nodes_max=16, edges_per_graph=0.0, seed=97)
    batch, ei, nmax = synthetic.make_topology(cfg, gen)
    N, E, B, T = batch.numel(), ei.size(1), 10, 9
    x = torch.randint(0, 2578, (N, 4), generator=gen)
    edge_attr = torch.randint(0, 2578, (E,), generator=gen)
    sgd = argparse.Namespace(x_bbox=torch.randint(0, 640, (N, 4), generator=gen).to(dev),
                             added_sym_edge=torch.randint(0, 10, (12,), generator=gen).to(dev))
    q = torch.randint(0, 512, (B, T), generator=gen)
    qmask = (torch.arange(T)[None] < torch.randint(5, T + 1, (B,), generator=gen)[:, None]).long()
    target = torch.randint(0, 1842, (B,), generator=gen).to(dev)

    def step():
        torch.manual_seed(3)                      # the torch dropouts outside the question side (gates, the classifier's)
        model.zero_grad(set_to_none=True)
        ops.reset_counters()
        logits = model(x.to(dev), ei.to(dev), edge_attr.to(dev), batch.to(dev), q.to(dev), qmask.to(dev), return_masks=True,
                       scene_graphs=sgd, seed=41)[0]
        loss = torch.nn.functional.cross_entropy(logits, target)
        loss.backward()
        return loss.detach(), {n: p.grad for n, p in model.named_parameters()}, ops.counters()

    l1, g1, c1 = step()
    l2, g2, _ = step()
    assert bool(torch.isfinite(l1)), l1
    assert c1["text_train_kernels"] == 2 and c1["torch_attention_train"] == 0, c1
    # every parameter that takes part has a gradient: the set torch's modules give (switch off), which lacks only what the model
    # constructs and does not apply -- emb_proj (question_encoder.py:33-34), the mask heads of the layers whose threshold is 1.0
    from isubgvqa_amd.models import text_encoder as TE
    TE.FUSED_TEXT_TRAIN = False
    try:
        _, g0, c0 = step()
    finally:
        TE.FUSED_TEXT_TRAIN = True
    assert c0["text_train_kernels"] == 0, c0
    have = {n for n, g in g1.items() if g is not None}
    assert have == {n for n, g in g0.items() if g is not None}, sorted(have ^ {n for n, g in g0.items() if g is not None})
    side = [n for n in g1 if n.startswith(("question_encoder.", "program_decoder.", "text_vocab_embedding."))
            and not n.startswith("question_encoder.emb_proj.") and "position_ids" not in n]
    assert len(side) > 100 and not [n for n in side if n not in have], [n for n in side if n not in have]
    assert all(bool(torch.isfinite(g).all()) for g in g1.values() if g is not None)
    assert torch.equal(l1, l2)
    differing = [n for n in g1 if g1[n] is not None and not torch.equal(g1[n], g2[n])]
    assert not differing, differing
