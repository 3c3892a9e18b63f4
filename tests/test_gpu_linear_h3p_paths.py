"""isg_linear_h3p (csrc/isg_gemm_h3p.hip) against fp64 on every non-segmented instantiation and every tile-walk regime of its
persistent form, and a proof that it writes nothing outside its result.

Which shape reaches which instantiation and regime is worked out by tests/h3p_walk_restated.py (the wrapper's dispatch and the
kernel's tile order restated in Python; tests/test_h3p_walk_cpu.py proves the claims for 256 CUs on the host).  Every test here
repeats the proof with the device's own CU count before it launches: on a device where a case does not reach its regime the test
fails, it does not pass on something else.

Parts (the numbers are the issue's):
  2  every instantiation at its smallest shape: M = 300 (two row tiles, the second 44 rows; three fp32-result shapes more, see the
     end of this text), N = 132 (160 for a planes32 result of the 256 x 256 form), K in {36, 224 | 256, 260, 480 | 512, 516, 576}, x {none, gelu, relu} x {bias, none}; one all-zero row of x
     and one of w.
  3  W1 16540 x 516 x 260 GELU: HEAD 8 with 69 workgroups walking two tiles (the two-pieces-per-k-tile path stores real results),
     ragged column tiles in flight and by epilogue; W2 26500 x 1028 x {256, 288, 320, 512, 544, 576}: every workgroup walks 3 or 4
     tiles, the three-slot rings wrap, KT mod 3 = 0, 1, 2 in both HEAD forms; W3 700 x 4100 x 256: 160 of 256 workgroups start on a
     padding entry of the tile order, and workgroup 2 stores a ragged row tile in flight.  (Not reachable on 256 CUs: a workgroup
     that starts on a padding entry and finds a valid tile later -- its entries are G = 256 apart, so they share L & 7.  In W1 and W2
     the one ragged row tile is the last of the order and leaves by epilogues only; W3 brings it in flight.)
     Row position: a 300-row block under in-flight tiles only and the last 300 rows, each run alone, give the bits they had in
     the batch.
  4  direct C-ABI calls: an fp32 result written into a column slice of a sentinel-filled tensor (ldd = N + 12), a planes32 result
     with guard words behind it; what the wrapper refuses.

Bounds, all the project's own (test_linear_h3p_matches_fp64_within_fp32_gemm_error, test_linear_h3p_planes_out_feeds_the_next_linear):
fp32 result: max |got - ref64| <= 1.5 e32 (e32 = the error of torch.nn.functional.linear in fp32 on the same inputs) and every row
within 2e-6 of its own largest magnitude; planes32 result: |rows - h32| <= inv * 16384 * 2^-23 elementwise and a second Linear over
the planes within 2.0 x the fp32 chain's error.

Measured err / e32 (MI355X, 256 CUs; part 2: the largest over the group's K, activations and bias; chain = the planes32 result
through a second Linear, against 2.0):
    part 2, per K (smallest .. largest of the six activation / bias cases)
    K     KT  instantiations   fp32 result: M, err / e32     planes32 result (M = 300): chain err / e32
    36     2  256 x 256         556   0.57 .. 0.92            0.49 .. 1.09
    224    7  256 x 256         300   0.55 .. 0.72            0.49 .. 0.85
    256    8  HEAD 8            300   0.62 .. 0.81            0.64 .. 1.02
    260    9  HEAD 8            300   0.50 .. 0.51            0.47 .. 0.90
    480   15  HEAD 8            300   0.49 .. 0.50            0.46 .. 0.85
    512   16  HEAD 16           300   0.55 .. 0.61            0.63 .. 0.77
    516   17  HEAD 16          1068   0.67 .. 0.78            0.78 .. 0.98
    576   18  HEAD 16          1068   0.45 .. 0.57            0.70 .. 1.09
    part 3 (fp32 result err / e32; planes32 result chain err / e32)
    W1 16540 x 516 x 260 gelu          0.60   0.93
    W2 26500 x 1028 x 256 / 288 / 320  0.51 / 0.65 / 0.77   0.54 / 0.50 / 0.53
    W2 26500 x 1028 x 512 / 544 / 576  0.61 / 0.80 / 0.59   0.67 / 0.71 / 0.63
    W2 relu, no bias, K = 288 / 544    0.64 / 0.83          1.03 / 0.99
    W3 700 x 4100 x 256                0.62   1.56
    row position: all six cases bit-equal (the in-flight piece path and the epilogue compute the same bits; no kernel change).

Three fp32-result shapes of part 2 run at more than 300 rows (tests/h3p_walk_restated.py::SMALL_M_FP32; M = 300 + 256 k keeps the last
row tile at 44 rows and every workgroup at one tile).  At M = 300 they exceeded 1.5 e32 and the kernel is not what differs:
  * K = 36: 1.34 .. 1.81 at M = 300, one element of one of the few rows scaled near e^5 (both sides' maxima come from those rows).
    Over all elements the engine's error is 0.84-0.89 x the fp32 GEMM's in rms and 0.71-0.80 x at the 99.9 % quantile at every M measured
    (300 .. 16684), and its largest error relative to the row's magnitude is 2.4e-7 against 3.7e-7: no outliers, a maximum over too
    few rows.  M = 556: 0.57 .. 0.92.
  * K = 516, 576: 1.50 .. 2.18 at M = 300, 1.40 .. 2.37 at 556, 1.21 .. 1.89 at 812 -- and 0.45 .. 0.78 at 1068, 0.49 .. 0.56 at 1324.
    What steps between 812 and 1068 rows is the yardstick: torch's fp32 GEMM is about 3 x more accurate below (its largest row-relative
    error 4.2e-7 .. 7.1e-7 there, 1.1e-6 .. 2.1e-6 from 1068 rows on and at K = 512 for every M; rms ratio 1.2 below, 0.63 above),
    presumably a different hipBLASLt algorithm for few rows and K > 512.  The engine's own error does not move with M (row-relative
    6.7e-7 .. 1.4e-6 throughout).  1068 is the first 300 + 256 k on the side of the step where e32 is what it is for the shapes
    the engine serves.
The ratio stays 1.5.
"""
import functools

import pytest
import torch

import h3p_walk_restated as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
SENT32 = 0x5A5AA5A5             # sentinel words: as fp32 1.5e16, as fp16 pairs 179.25 / -0.0201
SENT16 = 0x5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    from isubgvqa_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _act64(t, act):
    return torch.nn.functional.gelu(t) if act == "gelu" else (torch.relu(t) if act == "relu" else t)


@functools.lru_cache(maxsize=4)
def _operands(M, N, K, zx, zw):
    """The recipe of test_linear_h3p_matches_fp64_within_fp32_gemm_error (rows of x spanning seven binades, w ~ N(0, 1 / K)) with
    row zx of x and row zw of w all zero; the fp64 product is computed once per shape and shared (nothing writes to it)."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    x = torch.randn(M, K, device=dev, generator=g) * torch.rand(M, 1, device=dev, generator=g).mul(5).exp()
    w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    b = torch.randn(N, device=dev, generator=g)
    x[zx] = 0.0
    w[zw] = 0.0
    return x, w, b, x.double() @ w.double().t()


def _zero_rows(M, N):
    return M - 30, N - 2         # in the ragged row tile and in the ragged column tile


def _check_fp32(got, x, w, b, prod64, act, zx, zw, tag):
    """The fp32 result against fp64 on every element; returns err / e32."""
    M, N = prod64.shape
    ref = _act64(prod64 if b is None else prod64 + b.double(), act)
    base = _act64(torch.nn.functional.linear(x, w, b), act)
    e32 = (base.double() - ref).abs().max().item()
    assert got.shape == (M, N) and torch.isfinite(got).all(), tag
    diff = (got.double() - ref).abs()
    err = diff.max().item()
    print(f"h3p paths {tag}: err {err:.3e} fp32 gemm {e32:.3e} ratio {err / e32:.2f}")
    assert err <= 1.5 * e32 + 1e-30, (tag, err, e32)
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    assert (diff / scale).max().item() < 2e-6, tag
    if act != "gelu":           # a zero row of either operand: act(bias) exactly (the scales are powers of two, the product is 0)
        want = _act64(b if b is not None else torch.zeros(N, device=got.device), act)
        assert torch.equal(got[zx], want), (tag, "zero row of x")
        assert torch.equal(got[:, zw], want[zw].expand(M)), (tag, "zero row of w")
    return err / e32


def _planes_raw(hp, M, N):
    KT = (N + 31) // 32
    return hp.planes.view(torch.float16).view(M, KT, 2, 32).permute(0, 2, 1, 3).reshape(M, 2, KT * 32)


def _check_planes(hp, h32, x, w, b, prod64, act, zx, zw, tag):
    """The planes32 result against the fp32 result of the same instantiation family, and through a second Linear into 64 columns
    against the fp64 chain; returns the chain's err / e32."""
    from isubgvqa_amd import ops
    M, N = prod64.shape
    assert hp.rows == M and hp.cols == N and hp.inv.shape == (M,), tag
    assert (torch.log2(hp.inv) == torch.log2(hp.inv).round()).all(), (tag, "inv: powers of two")
    rows = ops.planes32_to_rows(hp)
    assert torch.isfinite(rows).all(), tag
    raw = _planes_raw(hp, M, N)
    assert (raw[:, :, N:] == 0).all(), (tag, "columns [N, roundup32(N)) of both planes are the next Linear's k padding: zeros")
    bound = hp.inv[:, None] * 16384.0
    assert ((rows - h32).abs() <= bound * 2.0 ** -23 + 1e-30).all(), (tag, ((rows - h32).abs() / bound).max().item() * 2.0 ** 23)
    want = _act64(b.double() if b is not None else torch.zeros(N, device=rows.device, dtype=torch.float64), act)
    slack = 2e-6 * want.abs().max().item() if act == "gelu" else 0.0       # an exact GELU in fp32: the per-row bound of the fp32 result
    assert ((rows[zx].double() - want).abs() <= bound[zx].double() * 2.0 ** -23 + slack).all(), (tag, "zero row of x")
    assert ((rows[:, zw].double() - want[zw]).abs() <= bound[:, 0].double() * 2.0 ** -23 + slack).all(), (tag, "zero row of w")
    g = torch.Generator(device=rows.device).manual_seed(N)
    w2 = torch.randn(64, N, device=rows.device, generator=g) / N ** 0.5
    b2 = torch.randn(64, device=rows.device, generator=g)
    y = ops.linear_h3p(hp, w2, b2, cache_planes=False)
    ref = _act64(prod64 if b is None else prod64 + b.double(), act) @ w2.double().t() + b2.double()
    base = torch.nn.functional.linear(_act64(torch.nn.functional.linear(x, w, b), act), w2, b2)
    e32 = (base.double() - ref).abs().max().item()
    err = (y.double() - ref).abs().max().item()
    print(f"h3p paths {tag}: chain err {err:.3e} fp32 chain {e32:.3e} ratio {err / e32:.2f}")
    assert err <= 2.0 * e32, (tag, err, e32)
    return err / e32


def _run_case(case, tag):
    from isubgvqa_amd import ops
    M, N, K, act, planes_out, bias = case
    zx, zw = _zero_rows(M, N)
    x, w, b, prod64 = _operands(M, N, K, zx, zw)
    b = b if bias else None
    kw = dict(gelu=act == "gelu", relu=act == "relu", cache_planes=False)
    h32 = ops.linear_h3p(x, w, b, **kw)
    if not planes_out:
        return _check_fp32(h32, x, w, b, prod64, act, zx, zw, tag)
    hp = ops.linear_h3p(x, w, b, planes_out=True, **kw)
    return _check_planes(hp, h32, x, w, b, prod64, act, zx, zw, tag)


def _tag(case):
    M, N, K, act, po, bias = case
    return f"{M}x{N}x{K} {act or 'none'} {'planes32' if po else 'fp32'} {'bias' if bias else 'nobias'}"


# ---- part 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes_out", [False, True], ids=["fp32", "planes32"])
@pytest.mark.parametrize("group", ["p256", "q8", "q16"])
def test_every_instantiation_at_its_smallest_shape_matches_fp64(dev, ncu, group, planes_out):
    cases = R.small_cases(group, planes_out)
    form, head = {"p256": ("p256", 0), "q8": ("q", 8), "q16": ("q", 16)}[group]
    assert R.regimes(cases, ncu)["instantiations"] == {R.Inst(form, a, planes_out, head, False) for a in R.ACTS}
    for case in cases:
        r = R.report(*case[:5], ncu)
        assert (case[0] - 300) % 256 == 0 and r.tiles_m >= 2 and r.ragged_row_epilogue and r.ragged_col_epilogue and r.depth == 1, case
    worst = max(_run_case(case, _tag(case)) for case in cases)
    print(f"h3p paths part 2 {group} {'planes32' if planes_out else 'fp32'}: worst ratio {worst:.2f}")


# ---- part 3 -----------------------------------------------------------------------------------------------------------------------
def _assert_regime(case, ncu):
    """What the case is in the list for, proved for THIS device's CU count."""
    M, N, K, act, po, _ = case
    r = R.report(M, N, K, act, po, ncu)
    if case in R.W1:
        assert r.inst == R.Inst("q", "gelu", po, 8, False) and r.depth >= 2 and r.depth_counts.get(2, 0) >= 1, r[:-1]
        assert r.ragged_col_inflight and r.ragged_col_epilogue and r.ragged_row_epilogue, r[:-1]
    elif case in R.W2:
        assert r.inst == R.Inst("q", act, po, 16 if K >= 512 else 8, False), r[:-1]
        assert min(r.depth_counts) >= 3 and r.depth >= 4, r[:-1]               # the three-slot parameter ring wraps in every workgroup
        assert r.kt_mod3 == {256: 2, 288: 0, 320: 1, 512: 1, 544: 2, 576: 0}[K], r[:-1]
        assert r.ragged_col_inflight and r.ragged_col_epilogue and r.ragged_row_epilogue, r[:-1]
    else:
        assert case in R.W3
        assert r.inst == R.Inst("q", None, po, 8, False) and r.padding_first and r.depth_counts.get(0, 0) >= 1, r[:-1]
        assert r.ragged_row_inflight and r.ragged_row_epilogue and r.ragged_col_epilogue, r[:-1]
    return r


@pytest.mark.parametrize("case", R.WALK_CASES, ids=[_tag(c).replace(" ", "-") for c in R.WALK_CASES])
def test_tile_walk_regimes_match_fp64_on_every_element(dev, ncu, case):
    _assert_regime(case, ncu)
    _run_case(case, _tag(case))


def test_walk_cases_together_reach_every_regime_on_this_device(ncu):
    walk = R.regimes(R.WALK_CASES, ncu)
    assert walk["max_depth"] >= 4 and walk["head8_max_depth"] >= 2
    assert walk["kt_mod3_at_depth3"] == {8: {0, 1, 2}, 16: {0, 1, 2}}
    assert walk["padding_first"]
    assert walk["ragged_row_inflight"] and walk["ragged_row_epilogue"] and walk["ragged_col_inflight"] and walk["ragged_col_epilogue"]
    assert R.regimes(R.small_cases(), ncu)["instantiations"] == R.all_instantiations()


@pytest.mark.parametrize("case", R.ROW_POSITION_CASES, ids=[_tag(c).replace(" ", "-") for c in R.ROW_POSITION_CASES])
def test_a_rows_result_does_not_depend_on_its_position_in_the_walk(dev, ncu, case):
    """The engine's row of test_a_rows_projection_does_not_depend_on_its_position_in_the_batch: rows stored piece by piece during the
    workgroup's next tile (a block in the middle, 100 rows into a row tile) and rows stored by the epilogue (the last 300) have,
    bit for bit, the result of the same rows run alone -- where one tile per workgroup leaves by the epilogue."""
    from isubgvqa_amd import ops
    M, N, K, act, po, bias = case
    _assert_regime(case, ncu)
    r0 = R.inflight_block(M, N, K, ncu)
    paths = R.store_paths(M, N, K, ncu)
    assert r0 is not None and r0 + 300 <= M - 300
    assert all(p == "inflight" for (m0, _), p in paths.items() if m0 in (r0 // 256 * 256, r0 // 256 * 256 + 256))
    assert all(p == "epilogue" for (m0, _), p in paths.items() if m0 + 256 >= M)
    assert R.report(300, N, K, act, po, ncu).depth == 1
    x, w, b, _ = _operands(M, N, K, *_zero_rows(M, N))
    b = b if bias else None
    kw = dict(gelu=act == "gelu", relu=act == "relu", planes_out=po, cache_planes=False)
    full = ops.linear_h3p(x, w, b, **kw)
    for start, where in ((r0, "in flight"), (M - 300, "epilogue")):
        alone = ops.linear_h3p(x[start:start + 300].contiguous(), w, b, **kw)
        if po:
            per = full.planes.numel() // M
            a, f = alone.planes.view(300, per), full.planes.view(M, per)[start:start + 300]
            assert torch.equal(alone.inv.view(torch.int32), full.inv[start:start + 300].view(torch.int32)), (where, "inv")
        else:
            a, f = alone.view(torch.int32), full[start:start + 300].view(torch.int32)
        bad = (a != f).any(dim=1).sum().item()
        assert bad == 0, f"{_tag(case)}: {bad} of the 300 rows at {start} ({where}) differ from the rows run alone"


# ---- part 4 -----------------------------------------------------------------------------------------------------------------------
def _call(lib, xp, wp, winv, bias, d, d_planes, d_inv, d_bound, M, N, K, ldd, act, a_inv_first=0, k_split=0):
    s = torch.cuda.current_stream().cuda_stream
    return lib.isg_linear_h3p(xp.planes.data_ptr(), xp.inv.data_ptr(), wp.data_ptr(), winv.data_ptr(), bias, d, d_planes, d_inv,
                              d_bound, M, N, K, ldd, act, a_inv_first, k_split, s)


def _guarded(lib, case):
    """One case through the C ABI twice: into exactly its result, and into a result with sentinel words around it."""
    from isubgvqa_amd import ops
    M, N, K, act, po, bias = case
    dev = torch.device("cuda:0")
    x, w, b, _ = _operands(M, N, K, *_zero_rows(M, N))
    b = b if bias else None
    xp = ops.split_planes32(x)
    wp, winv, bound = ops._h3p_weight(w, b, cache=False)
    bptr = b.data_ptr() if bias else 0
    code = {None: 0, "gelu": 1, "relu": 2}[act]
    tag = _tag(case)
    if not po:
        plain = torch.empty(M, N, dtype=torch.float32, device=dev)
        assert _call(lib, xp, wp, winv, bptr, plain.data_ptr(), 0, 0, 0, M, N, K, N, code) == 0, tag
        big = torch.full((M + 8, N + 12), SENT32, dtype=torch.int32, device=dev)
        d = big[:, 4:4 + N]
        assert d.data_ptr() % 16 == 0 and d.stride(0) == N + 12
        assert _call(lib, xp, wp, winv, bptr, d.data_ptr(), 0, 0, 0, M, N, K, N + 12, code) == 0, tag
        torch.cuda.synchronize()
        assert torch.equal(big[:M, 4:4 + N], plain.view(torch.int32)), (tag, "ldd = N + 12 changes the result")
        outside = big.clone()
        outside[:M, 4:4 + N] = SENT32
        hit = (outside != SENT32).nonzero()
        assert hit.numel() == 0, (tag, "written outside the result at (row, column)", hit[:8].tolist())
        return
    elems = int(lib.isg_planes32_elems(M, N))
    plain_p = torch.empty(elems, dtype=torch.int16, device=dev)
    plain_i = torch.empty(M, dtype=torch.float32, device=dev)
    assert _call(lib, xp, wp, winv, bptr, 0, plain_p.data_ptr(), plain_i.data_ptr(), bound.data_ptr(), M, N, K, 0, code) == 0, tag
    dp = torch.full((elems + 4096,), SENT16, dtype=torch.int16, device=dev)
    di = torch.full((M + 64,), SENT32, dtype=torch.int32, device=dev)
    assert _call(lib, xp, wp, winv, bptr, 0, dp.data_ptr(), di.data_ptr(), bound.data_ptr(), M, N, K, 0, code) == 0, tag
    torch.cuda.synchronize()
    assert torch.equal(dp[:elems], plain_p) and torch.equal(di[:M], plain_i.view(torch.int32)), (tag, "guard words change the result")
    assert (dp[elems:] == SENT16).all() and (di[M:] == SENT32).all(), (tag, "written behind the planes32 result")


@pytest.mark.parametrize("planes_out", [False, True], ids=["fp32", "planes32"])
@pytest.mark.parametrize("group", ["p256", "q8", "q16", "W1"])
def test_nothing_is_written_outside_the_result(dev, ncu, group, planes_out):
    """A store that should have been dropped (a lane right of column N in a ragged column tile, a row below M) lands, with ldd == N
    and a result of exactly M rows, inside the same tensor: here it would land on a sentinel."""
    from isubgvqa_amd import _lib
    lib = _lib.load()
    cases = [c for c in R.W1 if c[4] == planes_out] if group == "W1" else R.small_cases(group, planes_out)
    for case in cases:
        if group == "W1":
            _assert_regime(case, ncu)
        _guarded(lib, case)


def test_the_wrapper_refuses_what_its_header_says(dev):
    """Every refusal returns before a launch: the result buffers keep their sentinel."""
    from isubgvqa_amd import _lib, ops
    lib = _lib.load()
    M, K = 300, 512
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(132, K, device=dev, generator=g) / K ** 0.5
    xp = ops.split_planes32(x)
    wp, winv, bound = ops._h3p_weight(w, None, cache=False)
    x224 = ops.split_planes32(x[:, :224].contiguous())
    w224 = ops._h3p_weight(w[:, :224].contiguous(), None, cache=False)
    d = torch.full((M + 8, 144), SENT32, dtype=torch.int32, device=dev)
    dp = torch.full((int(lib.isg_planes32_elems(M, 160)) + 64,), SENT16, dtype=torch.int16, device=dev)
    di = torch.full((M + 8,), SENT32, dtype=torch.int32, device=dev)
    D, DP, DI, B = d.data_ptr(), dp.data_ptr(), di.data_ptr(), bound.data_ptr()
    call = functools.partial(_call, lib, xp, wp, winv, 0)
    #           d  d_planes d_inv d_bound  M  N    K  ldd act a_inv_first k_split
    assert call(D, 0, 0, 0, M, 132, K, 132, 0) == 0                                     # the call the refusals below vary
    torch.cuda.synchronize()
    d.fill_(SENT32)
    assert call(D, 0, 0, 0, M, 132, K, 128, 0) == EINVAL                                # ldd < N
    assert call(D, 0, 0, 0, M, 132, K, 134, 0) == EUNSUPPORTED                          # ldd % 4
    assert call(D, 0, 0, 0, M, 130, K, 132, 0) == EUNSUPPORTED                          # N % 4
    assert call(D, DP, DI, B, M, 132, K, 132, 0) == EINVAL                              # both result forms
    assert call(D, DP, 0, 0, M, 132, K, 132, 0) == EINVAL
    assert call(0, DP, DI, 0, M, 132, K, 0, 0) == EINVAL                                # a planes32 result without its bound
    assert call(D, 0, 0, 0, M, 132, K, 132, 3) == EINVAL                                # act
    assert call(D, 0, 0, 0, M, 132, K, 132, 1, xp.inv.data_ptr(), 48) == EINVAL         # k_split % 32
    assert call(D, 0, 0, 0, M, 132, K, 132, 1, 0, 256) == EINVAL                        # k_split without a_inv_first
    assert call(D, 0, 0, 0, M, 132, K, 132, 1, xp.inv.data_ptr(), 0) == EINVAL          # a_inv_first without k_split
    # a planes32 result of the 256 x 256 form (KT < 8) pads no columns: N % 32; the persistent form takes the same N
    assert _call(lib, x224, w224[0], w224[1], 0, 0, DP, DI, w224[2].data_ptr(), M, 132, 224, 0, 0) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (d == SENT32).all() and (dp == SENT16).all() and (di == SENT32).all(), "a refused call wrote to its result"
    assert _call(lib, xp, wp, winv, 0, 0, DP, DI, B, M, 132, K, 0, 0) == 0
    torch.cuda.synchronize()
    assert (di[:M] != SENT32).all() and (di[M:] == SENT32).all()
