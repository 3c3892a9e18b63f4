"""A Linear's backward on its own kernels (include/isg_linear_train.h, csrc/isg_linear_bwd.hip): the weight gradient on the bf16
matrix cores, the one-pass dz / bias-gradient kernel, autograd.linear with LINEAR_BWD_KERNELS on, and the strict twin's bits.

The error rule is tests/test_gpu_backward_fp64.py's, with its constants: e_k = max |kernel - float64| / max |float64|, e_32 the
same for torch float32 on the CPU, and e_k <= max(F * e_32, FLOOR) with F = 4, FLOOR = 2e-6.  An fp32 restatement of the kernels'
arithmetic on the CPU stays inside it: the six-product dW (16-row blocks, fp32 accumulation, splits) at 0.09 - 0.37 of the bound
over the shapes below (rows scaled by 2^+-20 and all-positive entries included), the erf form of GELU' at 0.04 - 0.06, a plain
chain over 1024 bias partials at 0.38.

Exact cases use small integers: every operand is then one bf16 plane and every partial sum stays below 2^24, so the result must
equal the int64 product whatever the order of the sums -- a wrong address in a transposed LDS read shows on every row and column.
"""
import ctypes
import math
import os

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
F = 4
GUARD = 64                       # floats on either side of a buffer a kernel writes
SENTINEL = -12345.0
STRICT = os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc", "libisg_hip_strict.so")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from isubgvqa_amd import _lib_linear_train
    return _lib_linear_train.load()


def rule(name, got, ref64, ref32, bad):
    """Print e_k and e_32, then note a miss of e_k <= max(F * e_32, FLOOR) in `bad`."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    if not bool(torch.isfinite(got).all()):
        bad.append(f"{name}: not finite")
        return float("nan")
    scale = float(ref64.abs().max())
    if scale == 0.0:
        if float(got.abs().max()) != 0.0:
            bad.append(f"{name}: the reference is identically zero, the kernel is not")
        return 0.0
    e_k = float((got.double() - ref64).abs().max()) / scale
    e_32 = float((ref32.double() - ref64).abs().max()) / scale
    bound = max(F * e_32, FLOOR)
    print(f"[linear-train] {name} | e_k={e_k:.3e} e_32={e_32:.3e} share of the bound={e_k / bound:.2f}")
    if not e_k <= bound:
        bad.append(f"{name}: e_k = {e_k:.3e} > max({F} * e_32, floor) = {bound:.3e}  (e_32 = {e_32:.3e})")
    return e_k


def guarded(numel, dev):
    """(whole buffer, the view of `numel` floats between its guard words)"""
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def guards_intact(buf, numel):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + numel:] == SENTINEL).all())


def pitch(t):
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def raw_wgrad(lib, g, x, splits, dev):
    """isg_linear_wgrad_bf16x6 on caller-made views (rows may be strided): partial [splits, N, K] between guard words."""
    from isubgvqa_amd import _lib, ops
    (M, N), K = g.shape, x.size(1)
    buf, part = guarded(splits * N * K, dev)
    _lib.check(lib.isg_linear_wgrad_bf16x6(g.data_ptr(), x.data_ptr(), part.data_ptr(), M, N, K, max(pitch(g), N), max(pitch(x), K),
                                           splits, ops._stream()), "isg_linear_wgrad_bf16x6")
    torch.cuda.synchronize()
    assert guards_intact(buf, splits * N * K), "isg_linear_wgrad_bf16x6 wrote outside partial[splits][N][K]"
    return part.view(splits, N, K).clone()


def sliced(t, dev, pad=None):
    """`t` as a column slice of a wider device tensor whose base lies one float past a 16-byte boundary."""
    M, N = t.shape
    pad = 4 + (-N) % 4 if pad is None else pad            # the pitch stays a multiple of 4: float4 bodies remain possible
    wide = torch.full((M, N + pad), SENTINEL, dtype=torch.float32, device=dev)
    view = wide[:, 1:N + 1]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return wide, view


# ==========================================================================================================================
# 1. dW, exact
# ==========================================================================================================================
EXACT = [((1, 1, 1), None, False), ((31, 5, 7), None, False), ((32, 128, 128), None, False), ((33, 129, 131), None, False),
         ((95, 130, 300), None, False), ((2049, 64, 132), 3, False), ((40, 20, 12), 8, False), ((64, 128, 128), None, True)]


@pytest.mark.parametrize("shape,splits,slices", EXACT, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wgrad_bf16x6_is_exact_on_small_integers(dev, lib, shape, splits, slices):
    from isubgvqa_amd import ops
    M, N, K = shape
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    g = torch.randint(-7, 8, (M, N), generator=gen)
    x = torch.randint(-7, 8, (M, K), generator=gen)
    want = g.t() @ x                                                   # int64
    assert int((g.abs().t() @ x.abs()).max()) < 2 ** 24
    if slices:
        gw, gd = sliced(g.float(), dev, pad=9)                         # ldg = 137 > N, ldx = 133 > K, both bases misaligned
        xw, xd = sliced(x.float(), dev, pad=5)
        assert gd.stride(0) > N and xd.stride(0) > K
    else:
        gd, xd = g.float().to(dev), x.float().to(dev)
    s = splits if splits is not None else int(lib.isg_linear_wgrad_bf16x6_splits(M, N, K))
    part = raw_wgrad(lib, gd, xd, s, dev)
    again = raw_wgrad(lib, gd, xd, s, dev)
    assert torch.equal(part, again), "two calls differ"
    got = part.cpu().double().sum(0)
    wrong = (got != want.double())
    assert not bool(wrong.any()), f"{int(wrong.sum())} of {N * K} entries differ from the integer product; first at {wrong.nonzero()[0].tolist()}"
    if splits is not None:                                             # every split holds exactly its own rows' product
        rows = -(-M // s)
        rows = -(-rows // 16) * 16
        for z in range(s):
            lo, hi = min(M, z * rows), min(M, (z + 1) * rows)
            assert torch.equal(part[z].cpu().double(), (g[lo:hi].t() @ x[lo:hi]).double()), f"split {z} (rows {lo}..{hi})"
        if shape == (40, 20, 12):
            assert not bool(part[3:].any()), "a split with no rows must write a zero tile"
    out = ops.linear_wgrad_bf16x6(gd, xd, splits=splits)
    assert out.shape == (N, K) and torch.equal(out.cpu().double(), want.double())
    if slices:
        assert bool((gw[:, 0] == SENTINEL).all()) and bool((xw[:, 0] == SENTINEL).all())


def test_wgrad_bf16x6_of_no_rows_is_zero(dev):
    from isubgvqa_amd import ops
    out = ops.linear_wgrad_bf16x6(torch.empty(0, 5, device=dev), torch.empty(0, 7, device=dev))
    assert out.shape == (5, 7) and not bool(out.any())


# ==========================================================================================================================
# 2. dW against float64
# ==========================================================================================================================
FP64_SHAPES = [((95, 130, 300), None), ((2049, 64, 132), 3), ((4096, 32, 32), 4)]


def _wgrad_inputs(shape, kind):
    M, N, K = shape
    gen = torch.Generator().manual_seed(M + N + K + len(kind))
    g, x = torch.randn(M, N, generator=gen), torch.randn(M, K, generator=gen)
    if kind == "scaled":
        g = g * torch.exp2(torch.randint(-20, 21, (M, 1), generator=gen).float())
        x = x * torch.exp2(torch.randint(-10, 11, (M, 1), generator=gen).float())
    elif kind == "positive":
        g, x = g.abs() + 0.1, x.abs() + 0.1
    return g, x


@pytest.mark.parametrize("shape,splits", FP64_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("kind", ["normal", "scaled", "positive"])
def test_wgrad_bf16x6_against_float64(dev, shape, splits, kind):
    from isubgvqa_amd import ops
    g, x = _wgrad_inputs(shape, kind)
    ref64, ref32 = g.double().t() @ x.double(), g.t() @ x
    bad = []
    rule(f"dW {shape} splits={splits} {kind}", ops.linear_wgrad_bf16x6(g.to(dev), x.to(dev), splits=splits), ref64, ref32, bad)
    rule(f"   (ops.linear_wgrad, the fp32 kernel, beside it)", ops.linear_wgrad(g.to(dev), x.to(dev)), ref64, ref32, [])
    assert not bad, "\n".join(bad)


def test_wgrad_bf16x6_one_inf_poisons_one_row(dev):
    from isubgvqa_amd import ops
    shape, (m0, n0) = (95, 130, 300), (41, 77)
    g, x = _wgrad_inputs(shape, "normal")
    g[m0, n0] = float("inf")
    got = ops.linear_wgrad_bf16x6(g.to(dev), x.to(dev)).cpu()
    assert not bool(torch.isfinite(got[n0]).any()), "row n0 of dW keeps a finite entry beside an Inf in g[:, n0]"
    keep = [n for n in range(shape[1]) if n != n0]
    ref64, ref32 = g[:, keep].double().t() @ x.double(), g[:, keep].t() @ x
    bad = []
    rule("dW beside a poisoned row", got[keep], ref64, ref32, bad)
    assert not bad, "\n".join(bad)


# ==========================================================================================================================
# 3. prep
# ==========================================================================================================================
BIG_M = 1024 * 257 + 3          # isg_linear_bwd_prep_parts gives 1024: 258 rows per workgroup, more than the 256 it takes at a time
PREP_SHAPES = [(1, 1), (17, 5), (33, 300), (4097, 64), (BIG_M, 8)]
SPECIAL_Z = [0.0, -0.0, 10.0, -10.0, 40.0, -40.0, 1e-30]


def raw_prep(lib, g, saved, mode, dz, want_db, dev):
    """isg_linear_bwd_prep on caller-made views; db_part [P, N] between guard words (or None)."""
    from isubgvqa_amd import _lib, ops
    M, N = g.shape
    P = int(lib.isg_linear_bwd_prep_parts(M, N))
    buf, part = guarded(P * N, dev) if want_db else (None, None)
    _lib.check(lib.isg_linear_bwd_prep(g.data_ptr(), max(pitch(g), N), 0 if saved is None else saved.data_ptr(),
                                       0 if saved is None else max(pitch(saved), N), mode, 0 if dz is None else dz.data_ptr(),
                                       0 if dz is None else max(pitch(dz), N), 0 if part is None else part.data_ptr(), M, N,
                                       ops._stream()), "isg_linear_bwd_prep")
    torch.cuda.synchronize()
    if want_db:
        assert guards_intact(buf, P * N), "isg_linear_bwd_prep wrote outside db_part[P][N]"
        return part.view(P, N).clone()
    return None


@pytest.fixture(scope="module")
def prep_data():
    """shape -> (g, z with the special values, y = a ReLU's result), made once on the CPU"""
    out = {}
    for M, N in PREP_SHAPES:
        gen = torch.Generator().manual_seed(M * 31 + N)
        g, z = torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen) * 2.0
        k = min(len(SPECIAL_Z), M * N)
        z.view(-1)[:k] = torch.tensor(SPECIAL_Z[:k])
        out[(M, N)] = (g, z, torch.relu(torch.randn(M, N, generator=gen)))
    return out


def _owned_parts(M, P):
    rows = -(-M // P)
    return [p for p in range(P) if p * rows < M]


@pytest.mark.parametrize("shape", PREP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", ["contiguous", "slices", "mixed"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prep_dz_and_bias_partials(dev, lib, prep_data, shape, layout, mode):
    """contiguous: float4 throughout where N allows.  slices: g, saved and dz are column slices that share a base one float past a
    16-byte boundary (scalar head, float4 body, scalar tail).  mixed: only g is such a slice (scalars throughout)."""
    M, N = shape
    g, z, y = prep_data[shape]
    saved = None if mode == 0 else z if mode == 1 else y
    if mode == 0:
        ref64, ref32 = g.double(), g
    elif mode == 1:
        ref64, ref32 = torch.ops.aten.gelu_backward(g.double(), z.double()), torch.ops.aten.gelu_backward(g, z)
    else:
        ref32 = g * (y > 0)
        ref64 = ref32.double()
    gw, gd = sliced(g, dev) if layout != "contiguous" else (None, g.to(dev))
    sw, sd = (None, None) if saved is None else sliced(saved, dev) if layout == "slices" else (None, saved.to(dev))
    if layout == "slices":
        dw_, dz = sliced(torch.zeros(M, N), dev)
    else:
        dw_, dz = guarded(M * N, dev)
        dz = dz.view(M, N)
    part = raw_prep(lib, gd, sd, mode, dz, True, dev)
    bad = []
    # ---- dz
    if layout == "slices":
        assert bool((dw_[:, 0] == SENTINEL).all()) and bool((dw_[:, N + 1:] == SENTINEL).all()), "dz written outside its columns"
    else:
        assert guards_intact(dw_, M * N), "dz written outside [M, N]"
    got = dz.cpu()
    if mode == 1:
        assert bool(torch.isfinite(got).all()), "GELU': a nonfinite entry"
        rule(f"prep {shape} {layout} GELU' dz", got, ref64, ref32, bad)
    else:
        assert torch.equal(got, ref32), f"mode {mode}: dz differs from " + ("g" if mode == 0 else "g * (y > 0)")
    # ---- db: the partial rows, summed by the caller
    P = part.size(0)
    owned = _owned_parts(M, P)
    rows = -(-M // P)
    if len(owned) < P:
        assert not bool(part[len(owned):].any()), "a workgroup that owns no rows must write zeros"
    if shape == (BIG_M, 8):
        assert rows > 256 and len(owned) < P
    rule(f"prep {shape} {layout} mode {mode} db", part.sum(0), ref64.sum(0), ref32.sum(0), bad)
    p_mid = owned[len(owned) // 2]                                      # one workgroup's own row, against its own rows
    lo, hi = p_mid * rows, min(M, (p_mid + 1) * rows)
    rule(f"prep {shape} {layout} mode {mode} db_part[{p_mid}]", part[p_mid], ref64[lo:hi].sum(0), ref32[lo:hi].sum(0), bad)
    assert torch.equal(part, raw_prep(lib, gd, sd, mode, dz, True, dev)), "two calls differ"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", [(17, 5), (4097, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_prep_identity_with_no_dz_writes_the_bias_partials_alone(dev, lib, prep_data, shape):
    from isubgvqa_amd import ops
    g, _, _ = prep_data[shape]
    gd = g.to(dev)
    part = raw_prep(lib, gd, None, 0, None, True, dev)
    bad = []
    rule(f"prep {shape} identity, db alone", part.sum(0), g.double().sum(0), g.sum(0), bad)
    dz, db = ops.linear_bwd_prep(gd, None, 0, want_dz=False, want_db=True)
    assert dz is None and torch.equal(db, part.sum(0) if part.size(0) > 1 else part[0])
    dz, db = ops.linear_bwd_prep(gd, None, 0, want_dz=True, want_db=False)
    assert db is None and torch.equal(dz, gd)
    assert not bad, "\n".join(bad)


def test_prep_relu_gives_nan_for_a_nonfinite_gradient_at_a_masked_position(dev, prep_data):
    from isubgvqa_amd import ops
    g, _, y = prep_data[(33, 300)]
    g = g.clone()
    dead = (y <= 0).nonzero()
    live = (y > 0).nonzero()
    (m0, n0), (m1, n1), (m2, n2) = dead[3].tolist(), dead[len(dead) // 2].tolist(), live[5].tolist()
    g[m0, n0], g[m1, n1], g[m2, n2] = float("inf"), float("nan"), float("-inf")
    want = g * (y > 0)                                                  # torch's own product: NaN, NaN, -inf
    assert math.isnan(float(want[m0, n0])) and math.isnan(float(want[m1, n1])) and float(want[m2, n2]) == float("-inf")
    dz, db = ops.linear_bwd_prep(g.to(dev), y.to(dev), 2)
    dz, db = dz.cpu(), db.cpu()
    assert torch.equal(torch.isnan(dz), torch.isnan(want)) and torch.equal(dz.nan_to_num(nan=7.0), want.nan_to_num(nan=7.0))
    assert math.isnan(float(db[n0])) and math.isnan(float(db[n1])) and float(db[n2]) == float("-inf")


# ==========================================================================================================================
# 4. autograd.linear with the switch on
# ==========================================================================================================================
AUTOGRAD_CASES = [(7, 300, 1200, "gelu"), (2050, 300, 1200, "gelu"), (2050, 512, 2048, "relu"), (2050, 64, 1842, "none")]


def _autograd_inputs(case):
    """x, W, b and the upstream gradient.  The ReLU case is made of small dyadic numbers with a bias of k + 1/16: every
    pre-activation is then exact in every precision and never zero, so the kernels and the float64 reference mask the same
    entries (a pre-activation within rounding of zero would flip a whole term of the gradient on one side only)."""
    M, K, N, act = case
    gen = torch.Generator().manual_seed(M + K + N)
    if act == "relu":
        x = torch.randint(-3, 4, (M, K), generator=gen).float()
        w = torch.randint(-3, 4, (N, K), generator=gen).float() / 8
        b = torch.randint(-2, 3, (N,), generator=gen).float() + 1.0 / 16
    else:
        x, w, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / math.sqrt(K), torch.randn(N, generator=gen)
    return x, w, b, torch.randn(M, N, generator=gen)


def _oracle(case, dtype):
    x, w, b, go = _autograd_inputs(case)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, w, b)]
    z = torch.nn.functional.linear(*leaves)
    y = torch.nn.functional.gelu(z) if case[3] == "gelu" else torch.relu(z) if case[3] == "relu" else z
    y.backward(go.to(dtype))
    return [t.grad for t in leaves]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=lambda c: f"M{c[0]}-K{c[1]}-N{c[2]}-{c[3]}")
def test_autograd_linear_on_the_backward_kernels(dev, case, monkeypatch):
    from isubgvqa_amd import autograd, ops
    M, K, N, act = case
    x, w, b, go = _autograd_inputs(case)
    g64, g32 = _oracle(case, torch.float64), _oracle(case, torch.float32)
    if act == "relu":
        z = torch.nn.functional.linear(x.double(), w.double(), b.double())
        assert float(z.abs().min()) >= 1.0 / 16
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(autograd, "LINEAR_BWD_KERNELS", on)
        leaves = [t.to(dev).requires_grad_(True) for t in (x, w, b)]
        before = ops.counters()["linear_bwd_kernels"]
        calls = {"prep": 0, "wgrad": 0}
        prep, wgrad = ops.linear_bwd_prep, ops.linear_wgrad_bf16x6
        monkeypatch.setattr(ops, "linear_bwd_prep", lambda *a, **k: (calls.__setitem__("prep", calls["prep"] + 1), prep(*a, **k))[1])
        monkeypatch.setattr(ops, "linear_wgrad_bf16x6", lambda *a, **k: (calls.__setitem__("wgrad", calls["wgrad"] + 1), wgrad(*a, **k))[1])
        autograd.linear(leaves[0], leaves[1], leaves[2], act == "gelu", relu=act == "relu").backward(go.to(dev))
        monkeypatch.setattr(ops, "linear_bwd_prep", prep)
        monkeypatch.setattr(ops, "linear_wgrad_bf16x6", wgrad)
        rose = ops.counters()["linear_bwd_kernels"] - before
        if on:
            assert rose == 1 and calls["prep"] == 1, (rose, calls)
            assert calls["wgrad"] == (1 if M >= autograd.WGRAD_MIN_ROWS else 0), calls
        else:
            assert rose == 0 and calls == {"prep": 0, "wgrad": 0}, (rose, calls)
        grads[on] = [t.grad for t in leaves]
    bad = []
    for name, got, off, a, b_ in zip(("dX", "dW", "db"), grads[True], grads[False], g64, g32):
        assert got is not None, name
        rule(f"autograd.linear {case} {name}", got, a, b_, bad)
        rule(f"   (switch off, beside it) {name}", off, a, b_, [])
    assert not bad, "\n".join(bad)


# ==========================================================================================================================
# 5. the strict twin
# ==========================================================================================================================
def test_strict_twin_gives_the_fast_librarys_bits(dev, lib):
    from isubgvqa_amd import _lib, _lib_linear_train
    assert os.path.exists(STRICT), "csrc/libisg_hip_strict.so is missing: __graft_entry__.build() makes it beside the library"
    strict = _lib.bind(ctypes.CDLL(STRICT), _lib_linear_train.SIGNATURES)
    assert strict.isg_linear_train_abi_version() == _lib_linear_train.ABI_VERSION
    gen = torch.Generator().manual_seed(5)
    g, x = torch.randn(95, 130, generator=gen).to(dev), torch.randn(95, 300, generator=gen).to(dev)
    a, b = raw_wgrad(lib, g, x, 1, dev), raw_wgrad(strict, g, x, 1, dev)
    assert torch.equal(a, b), f"dW: the strict and the fast build differ in {int((a != b).sum())} values"
    g, z = torch.randn(33, 300, generator=gen).to(dev), torch.randn(33, 300, generator=gen).to(dev)
    for mode in (1, 2):
        outs = []
        for which in (lib, strict):
            dz = torch.empty(33, 300, device=dev)
            outs.append((raw_prep(which, g, z, mode, dz, True, dev), dz))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"prep mode {mode}: the builds differ"
