"""What tests/test_gpu_simple_fwd.py rests on, held on the CPU: the restated forward of the SIMPLE sampler
(tests/simple_fwd_restated.py) in float32 IS the oracle (oracle/simple.py::simple_forward) on the G9 goldens and on every shape the
GPU test runs; in float64 a full row's marginals sum to min(k, nmax); every shape reaches the rows per workgroup, the LDS regime or
the refusal it is there for, by the restated host rule row_bytes = 2 (2n - 1)(min(k, nmax) + 1) 4; and the reference alone says the
chosen inputs are well conditioned -- no row left out."""
import pytest
import torch

import simple_fwd_restated as S
from conftest import load_golden
from oracle import simple as OS

ALL = list(S.CASES) + ["hint"]


def _oracle(dense, k, uniform):
    mask, marg = OS.simple_forward(dense.unsqueeze(-1), k, uniform.unsqueeze(0))
    return mask[0, :, :, 0], marg[:, :, 0]


def _same_as_oracle(dense, lens, k, uniform, real, what):
    out, marg, hot, _ = S.forward(dense, lens, k, uniform, torch.float32)
    o_mask, o_marg = _oracle(dense, k, uniform)
    assert torch.equal(torch.isnan(marg), torch.isnan(o_marg)), what
    torch.testing.assert_close(marg, o_marg, rtol=1e-5, atol=1e-6, equal_nan=True, msg=lambda m: f"{what}: {m}")
    torch.testing.assert_close(out[real], o_mask[real], rtol=0, atol=1e-6, equal_nan=True, msg=lambda m: f"{what}: {m}")
    return marg, out


def test_float32_restatement_is_the_oracle_on_the_g9_goldens():
    for i, c in enumerate(load_golden("g9_simple.pt")):
        dense, uniform = c["scores"][:, :, 0], c["uniform"][0]
        B, nmax = dense.shape
        lens, real = torch.full((B,), nmax), torch.ones(B, nmax, dtype=torch.bool)
        marg, out = _same_as_oracle(dense, lens, c["k"], uniform, real, f"G9 case {i}")
        assert torch.equal(torch.isnan(marg), torch.isnan(c["marginals"][:, :, 0]))
        torch.testing.assert_close(marg, c["marginals"][:, :, 0], rtol=1e-5, atol=1e-6, equal_nan=True)
        torch.testing.assert_close(out, c["mask"][0, :, :, 0], rtol=0, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize("name", ALL)
def test_float32_restatement_is_the_oracle_on_the_new_shapes(name):
    dense, lens, k, uniform, real = S.inputs(name)
    _same_as_oracle(dense, lens, k, uniform, real, name)


@pytest.mark.parametrize("name", ALL)
def test_full_rows_sum_to_k_in_float64(name):
    dense, lens, k, uniform, real = S.inputs(name)
    nmax = dense.size(1)
    full = lens == nmax
    assert bool(full.any()), "every shape holds a full row"
    total = S.reference(name)["marg64"][full].sum(1)
    assert float((total - min(k, nmax)).abs().max()) <= 1e-9, (name, total.tolist())
    if k >= nmax:
        assert bool((S.reference(name)["marg64"][full] == 1.0).all())


@pytest.mark.parametrize("name", ALL)
def test_the_reference_alone_says_the_input_is_well_conditioned(name):
    """float32 and float64 agree on the NaN pattern and on every row's set, every row's float64 key gap at the k-th place exceeds
    1e-3 (a 1-ulp logf cannot flip the set), and e32 < 2.5e-4 so that 4 e32 stays a meaningful bound.  Every row of every shape."""
    r = S.reference(name)
    B = S.inputs(name)[0].size(0)
    assert r["gap"].numel() == B and r["hot64"].size(0) == B and r["marg64"].size(0) == B
    assert S.well_conditioned(name) == []


def test_every_shape_reaches_what_it_claims():
    rb = S.row_bytes
    # rows per workgroup, with a batch that leaves the last workgroup partly empty
    for k, rows in ((5, 4), (6, 3), (8, 2), (16, 1)):
        assert S.rows_per_block(k, 128) == rows and S.regime(k, 128) == "48K"
        for B in (5, 7):
            nmax, kk, lens, _, _ = S.CASES[f"rows n128 k{k} B{B}"]
            assert (nmax, kk, len(lens)) == (128, k, B) and max(lens) == 128
            assert B % rows != 0 or rows == 1, (k, B)
    # the three LDS regimes and the largest admitted row
    # (257, 5) is 49 104 B: 48 B below 48 KB = 49 152 B, so it is the largest single row of the first regime and not yet in the
    # second; (257, 6) and (200, 15) are in the second, the latter 128 B below 64 KB
    assert rb(5, 257) == 49104 and S.regime(5, 257) == "48K" and S.rows_per_block(5, 257) == 1
    assert rb(6, 257) == 57288 and S.regime(6, 257) == "64K" and S.rows_per_block(6, 257) == 1
    assert rb(15, 200) == 65408 and S.regime(15, 200) == "64K" and S.OPT_IN - rb(15, 200) == 128
    assert rb(16, 130) == 69496 and S.regime(16, 130) == "opt-in"
    assert rb(8, 1024) == 147384 and S.regime(8, 1024) == "opt-in" and S.largest_k(1024) == 8
    assert rb(7, 700) == 131008 and S.regime(7, 700) == "opt-in"
    assert rb(16, 128) == 34680 and rb(8, 128) == 18360 and rb(6, 128) == 14280 and rb(5, 128) == 12240
    for name in ("lds n257 k5", "lds n257 k6", "lds n200 k15", "lds n130 k16", "lds n1024 k8", "lds n700 k7"):
        nmax, k, lens, _, _ = S.CASES[name]
        assert max(lens) == nmax and f"n{nmax} k{k}" in name
    # refusals: beyond 1024 slots, beyond 16 picks, beyond 150 KB; their nearest admitted neighbours run
    assert rb(9, 1024) == 163760 > S.ROW_LIMIT
    assert all(S.refused(k, nmax) for nmax, k in S.REFUSED.values())
    assert not S.refused(5, 1024) and not S.refused(16, 32) and not S.refused(17, 16) and not S.refused(8, 1024)
    # the table sweep: every level count 0..10, at each 1, 2, 5 and the largest admitted k; every k at nmax 32 and 40; all regimes
    sweep = {(v[0], v[1]) for v in S.CASES.values() if v[4] == "table sweep"}
    assert {S.n_of(nmax).bit_length() - 1 for nmax, _ in sweep} == set(range(11))
    for nmax in S.LEVELS:
        assert {(nmax, 1), (nmax, 2), (nmax, 5), (nmax, S.largest_k(nmax))} <= sweep
        assert S.refused(S.largest_k(nmax) + 1, nmax) or S.largest_k(nmax) == S.MAXK
    assert {(n, k) for n in (32, 40) for k in range(1, 17)} <= sweep
    assert {S.regime(k, nmax) for nmax, k in sweep} == {"48K", "opt-in"}             # (the regime between them: 'LDS regimes')
    assert {S.regime(v[1], v[0]) for v in S.CASES.values()} == {"48K", "64K", "opt-in"}
    assert {S.rows_per_block(k, nmax) for nmax, k in sweep} == {1, 2, 3, 4}
    for name, (nmax, k, lens, kind, cls) in S.CASES.items():
        assert not S.refused(k, nmax) and max(lens) == nmax and min(lens) >= 0, name
        if cls == "table sweep":
            assert lens == [nmax, min(min(k, nmax) + 1, nmax), 1], name
    # power of two (no -1e10 pad) and one more than a power of two
    assert all(S.n_of(p) == p and S.n_of(p + 1) == 2 * p for p in (2, 8, 32, 64, 128, 256, 512))
    # the arms
    assert S.CASES["arm empty graph"][2][1] == 0 and 0 not in (S.CASES["arm empty graph"][2][0], S.CASES["arm empty graph"][2][-1])
    assert S.CASES["arm zero pads > k"][:3] == (6, 2, [1, 2, 6]) and S.CASES["arm k=1 NaN rows"][:3] == (129, 1, [129, 1, 60])
    assert S.CASES["arm k>=nmax n4"][:2] == (4, 5) and S.CASES["arm k>=nmax n2"][:2] == (2, 5) and S.CASES["arm nmax=1"][0] == 1
    # the hinted plans: the same n with more zero pads, and a larger n
    true = max(S.HINT_LENS)
    assert [S.n_of(h) for h in S.HINTS] == [S.n_of(true), 2 * S.n_of(true)] and all(h > true for h in S.HINTS)


def test_the_named_arms_hold_what_they_are_named_for():
    r = S.reference("arm k=1 NaN rows")
    # a k = 1 row with zero pads is NaN in float64 too, on most of its slots; the full row is not
    assert not r["nan64"][0].any() and int(r["nan64"][1].sum()) > 64 and int(r["nan64"][2].sum()) > 32
    for name in ("arm k>=nmax n4", "arm k>=nmax n2", "arm nmax=1"):
        assert bool((S.reference(name)["marg64"] == 1.0).all()) and bool((S.reference(name)["marg32"] == 1.0).all()), name
    dense = S.inputs("arm ln2")[0]
    assert dense[0, :6].tolist() == torch.tensor(S.LN2_VALUES).tolist()
    x = -dense[0, :6].abs()
    assert (x > -0.6931471805599453094).tolist() == [True, True, False, False, False, False]     # both branches of log1mexp are taken
    assert S.inputs("arm 30")[0][0, :2].tolist() == [30.0, -30.0]
    # more zero pads than k (rows 0 and 1: 5 and 4 forced slots, k = 2): the impossible-root arm, finite by the two paddings alone
    dense, lens, k, _, _ = S.inputs("arm zero pads > k")
    m = S.reference("arm zero pads > k")["marg64"]
    assert bool(torch.isfinite(m).all()) and int((dense[0] == 0).sum()) > k and int((dense[1] == 0).sum()) > k
    # the pad count decides the result: 40 real slots padded to 40 sum to k, padded to 64 (a hint's zero pads) they do not
    dense, lens, k, _, _ = S.inputs("hint")
    row = dense[:1]
    wide = torch.cat([row, torch.zeros(1, 24)], 1)
    a = S.marginals(row, torch.tensor([40]), k, torch.float64)
    b = S.marginals(wide, torch.tensor([40]), k, torch.float64)
    assert abs(float(a.sum()) - k) <= 1e-9 and abs(float(b.sum()) - k) > 1e-3


def test_true_nmax_of_a_hinted_plan_on_the_host(monkeypatch):
    """GraphPlan.true_nmax, the row length the SIMPLE sampler goes by, on plans made from CPU tensors (nothing touches the library):
    nmax itself without a hint; nmax_dev read back once under a hint and kept in the cache the plan's views share; IsgError where
    the copy is impossible (a capture in progress, a plan built inside one) and where the hint understates the batch."""
    from isubgvqa_amd import _lib, ops
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # (without a GPU the predicate itself raises)

    def plan(true, nmax, hinted):
        return ops.GraphPlan(N=7, E=0, B=2, ptr=torch.tensor([0, 3, 7], dtype=torch.int32), nmax_dev=torch.tensor([true], dtype=torch.int32),
                             nmax=nmax, batch=torch.tensor([0, 0, 0, 1, 1, 1, 1]), nmax_hinted=hinted)

    assert plan(4, 4, False).true_nmax("x") == 4
    assert plan(9, 4, False).true_nmax("x") == 4                      # no hint: nmax_dev is not read
    p = plan(4, 64, True)
    view = p.with_holes(None)
    assert p.true_nmax("x") == 4 and p._cache.nmax_true == 4
    p.nmax_dev.fill_(5)
    assert p.true_nmax("x") == 4 and view.true_nmax("x") == 4         # read once, shared with the views
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert p.true_nmax("x") == 4                                      # known before the capture
    with pytest.raises(_lib.IsgError, match="true longest row"):
        plan(4, 64, True).true_nmax("the SIMPLE sampler")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    q = plan(4, 64, True)
    q._bounds_dev = torch.tensor([4, 0], dtype=torch.int32)           # built inside a capture: every replay rewrites nmax_dev
    with pytest.raises(_lib.IsgError, match="true longest row"):
        q.true_nmax("the SIMPLE sampler")
    with pytest.raises(_lib.IsgError, match="understate"):
        plan(65, 64, True).true_nmax("the SIMPLE sampler")
    assert ops._simple_n(0) == 0 and [ops._simple_n(v) for v in (1, 2, 3, 40, 64, 65, 1024)] == [1, 2, 4, 64, 64, 128, 1024]
    assert [S.n_of(v) for v in (1, 2, 3, 40, 64, 65, 1024)] == [1, 2, 4, 64, 64, 128, 1024]


def test_the_tie_rule_restated():
    dense, uniform, expect = S.tie_rows()
    lens = torch.full((dense.size(0),), S.TIE_N)
    for dtype in (torch.float32, torch.float64):
        key = S.keys(dense, lens, uniform, dtype)
        for row, pair in enumerate(S.TIE_PAIRS):
            assert key[row, pair[0]] == key[row, pair[1]]                       # the same key, bit for bit
            top = key[row].sort(descending=True).values
            assert top[1] > top[2] == top[3] > top[4]                           # the pair straddles the k-th place
        hot = S.select(key, S.TIE_K)
        assert [torch.nonzero(h).view(-1).tolist() for h in hot] == expect
    assert expect == [[3, 7, 10], [3, 7, 10], [3, 7, 11]]
