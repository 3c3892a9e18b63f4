"""Host-side proof that the case lists of tests/test_gpu_linear_h3p_paths.py reach what they claim on a 256-CU device: the walk of
isg_linear_h3p's persistent form restated in tests/h3p_walk_restated.py, checked against tile counts worked out by hand, and the
instantiations and walk regimes the case lists cover together.  The two segmented instantiations stay with
test_linear_h3p_segmented_operand.  Also here, because it needs no GPU: both Linear entry points refuse relu together with gelu."""
import os
import re

import pytest

import h3p_walk_restated as R
from conftest import ROOT

NCU = 256
HIP = os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc", "isg_gemm_h3p.hip")


def test_the_restated_constants_are_the_kernels():
    src = open(HIP).read()
    assert int(re.search(r"constexpr int P3_T = (\d+)", src).group(1)) == R.P3_T
    bm, bn = re.search(r"constexpr int Q3_BM = (\d+), Q3_BN = (\d+);", src).groups()
    assert (int(bm), int(bn)) == (R.Q3_BM, R.Q3_BN)
    assert int(re.search(r"constexpr int Q3_HEAD = (\d+);", src).group(1)) == R.Q3_HEAD
    assert "if (KT >= 16) ISG_Q3H(ACT_, PO_, 16); else ISG_Q3H(ACT_, PO_, 8);" in src
    assert "if (version != 1 && KT >= Q3_HEAD) {" in src
    assert "m0 = ((L & 7) + 8 * (slot / a.tiles_n)) * Q3_BM;" in src and "n0 = (slot % a.tiles_n) * Q3_BN;" in src
    assert "const unsigned grid = (unsigned)(total < ncu ? total : ncu);" in src


def test_instantiation_and_k_tiles_by_hand():
    assert [R.kt_of(K) for K in R.SMALL_KS] == [2, 7, 8, 9, 15, 16, 17, 18]
    assert [R.instantiation(K, None, False)[::3] for K in R.SMALL_KS] == (
        [("p256", 0)] * 2 + [("q", 8)] * 3 + [("q", 16)] * 3)
    assert len(R.all_instantiations()) == 18 and len(R.all_instantiations(seg=True)) == 2
    assert R.instantiation(1200, "gelu", True, seg=True) == R.Inst("q", "gelu", True, 16, True)
    assert [R.kt_of(K) % 3 for K in R.W2_KS] == [2, 0, 1, 1, 2, 0]
    assert sorted(K for ks in R.SMALL_GROUPS.values() for K in ks) == sorted(R.SMALL_KS)
    assert R.small_n(224, True) == 160 and R.small_n(224, False) == 132 and R.small_n(256, True) == 132


def test_walks_by_hand():
    # W1: 65 row tiles in 72 slots x 5 column tiles; entries 256..319 are row tiles 48..63 (all valid), of 320..359 (row tiles 64..71)
    # only the five of row tile 64: 69 workgroups walk two tiles
    r = R.report(*R.W1[0][:5], NCU)
    assert (r.tiles_m, r.slots_m, r.tiles_n, r.total_l, r.grid, r.valid) == (65, 72, 5, 360, 256, 325)
    assert r.depth_counts == {2: 69, 1: 187} and r.inst == R.Inst("q", "gelu", False, 8, False) and r.kt == 9
    # entry 256 = slot 32 = row group 6 (row tile 48), column tile 2; entry 64 = slot 8 = row group 1, column tile 3; 320 = slot 40
    assert r.walks[0][1] == [(0, 0), (48 * 256, 2 * 128)] and r.walks[64][1] == [(8 * 256, 3 * 128), (64 * 256, 0)]
    assert r.walks[65][1] == [(9 * 256, 3 * 128)]                   # entry 321 is row tile 65: padding
    # the only ragged row tile (64) sits at the end of the order: stored by epilogues alone
    assert (r.ragged_row_inflight, r.ragged_row_epilogue, r.ragged_col_inflight, r.ragged_col_epilogue) == (False, True, True, True)
    # W2: 104 row tiles (no padding slot) x 9 column tiles = 936 entries on 256 workgroups: 168 walk four tiles, 88 three
    r = R.report(*R.W2[0][:5], NCU)
    assert (r.tiles_m, r.slots_m, r.tiles_n, r.total_l, r.grid, r.valid) == (104, 104, 9, 936, 256, 936)
    assert r.depth_counts == {4: 168, 3: 88} and not r.padding_first
    # W3: 3 row tiles in 8 slots x 33 column tiles: 264 entries, 99 valid.  Workgroups 2 (entries 2, 258: row tile 2, ragged, first
    # column tile and last) and 0, 1 walk two tiles; 160 start on a padding entry
    r = R.report(*R.W3[0][:5], NCU)
    assert (r.tiles_m, r.slots_m, r.tiles_n, r.total_l, r.grid, r.valid) == (3, 8, 33, 264, 256, 99)
    assert r.depth_counts == {2: 3, 1: 93, 0: 160} and r.padding_first
    assert r.walks[2][1] == [(512, 0), (512, 32 * 128)] and r.walks[3] == (True, [])
    assert (r.ragged_row_inflight, r.ragged_row_epilogue, r.ragged_col_inflight, r.ragged_col_epilogue) == (True, True, False, True)
    # a workgroup's entries are G apart and G = 256 is a multiple of 8, so they all share L & 7: one that starts on a padding entry
    # meets padding entries only.  next_tile() finding a valid tile behind a padding first entry needs a CU count that is no multiple
    # of 8
    assert not r.padding_first_then_valid
    assert R.report(700, 4100, 256, None, False, 250).padding_first_then_valid
    # the 256 x 256 form: one workgroup per entry
    r = R.report(300, 132, 224, "relu", False, NCU)
    assert (r.tiles_m, r.tiles_n, r.total_l, r.grid, r.valid, r.depth) == (2, 1, 8, 8, 2, 1)
    assert r.ragged_row_epilogue and r.ragged_col_epilogue and not r.ragged_row_inflight


def test_case_lists_reach_the_instantiations_and_regimes_they_claim():
    small = R.regimes(R.small_cases(), NCU)
    assert small["instantiations"] == R.all_instantiations(), "part 2 reaches all 18 non-segmented instantiations"
    assert small["max_depth"] == 1
    # 300 rows, or 300 + 256 k where the fp32 yardstick needs more rows: the last row tile has 44 rows either way
    assert {M for M, *_ in R.small_cases()} == {300, 556, 1068} and all((M - 300) % 256 == 0 for M, *_ in R.small_cases())
    assert all(M == 300 for M, _, _, _, po, _ in R.small_cases() if po)
    for group, form, head in (("p256", "p256", 0), ("q8", "q", 8), ("q16", "q", 16)):
        for po in (False, True):
            got = R.regimes(R.small_cases(group, po), NCU)["instantiations"]
            assert got == {R.Inst(form, a, po, head, False) for a in R.ACTS}, (group, po)
    walk = R.regimes(R.WALK_CASES, NCU)
    assert walk["max_depth"] >= 4
    assert walk["head8_max_depth"] >= 2
    assert walk["kt_mod3_at_depth3"] == {8: {0, 1, 2}, 16: {0, 1, 2}}
    assert walk["padding_first"]
    assert walk["ragged_row_inflight"] and walk["ragged_row_epilogue"] and walk["ragged_col_inflight"] and walk["ragged_col_epilogue"]
    # per regime: which case brings it
    w1, w2, w3 = (R.regimes(c, NCU) for c in (R.W1, R.W2, R.W3))
    assert w1["head8_max_depth"] == 2 and w1["ragged_col_inflight"] and w1["ragged_row_epilogue"] and not w1["padding_first"]
    assert w2["max_depth"] == 4 and w2["kt_mod3_at_depth3"] == {8: {0, 1, 2}, 16: {0, 1, 2}}
    assert w3["padding_first"] and w3["ragged_row_inflight"]
    # both result forms of every walk case; the W2 extras are ReLU without a bias at one K per HEAD form
    assert all((M, N, K, act, not po, bias) in R.WALK_CASES for M, N, K, act, po, bias in R.WALK_CASES)
    assert {(R.instantiation(K, act, po).head, act, bias) for _, _, K, act, po, bias in R.W2 if act} == {(8, "relu", False), (16, "relu", False)}
    # every result stays below the 128 MB where the store policy and its one-time measurement come in
    assert all(M * N * 4 < 128_000_000 for M, N, *_ in R.WALK_CASES + R.small_cases())
    # the row-position cases have a 300-row block in the middle under in-flight tiles only, and their last rows leave by epilogues
    for M, N, K, act, po, _ in R.ROW_POSITION_CASES:
        r0 = R.inflight_block(M, N, K, NCU)
        paths = R.store_paths(M, N, K, NCU)
        assert r0 is not None and r0 % 256 == 100 and r0 + 300 < M - 300
        assert all(p == "inflight" for (m0, _), p in paths.items() if m0 in (r0 // 256 * 256, r0 // 256 * 256 + 256))
        assert all(p == "epilogue" for (m0, _), p in paths.items() if m0 + 256 >= M)
        alone = R.report(300, N, K, act, po, NCU)
        assert alone.depth == 1 and alone.inst == R.instantiation(K, act, po)
    assert {R.instantiation(c[2], c[3], c[4]).head for c in R.ROW_POSITION_CASES} == {8, 16}


def test_both_linear_entry_points_refuse_relu_with_gelu():
    """ops.linear refused the pair; ops.linear_h3p and ops.linear_skinny used to let ReLU win silently.  All raise before they look
    at a tensor's device or load the library."""
    import torch
    from isubgvqa_amd import ops
    x, w = torch.zeros(4, 256), torch.zeros(8, 256)
    for fn in (ops.linear, ops.linear_h3p, ops.linear_skinny):
        with pytest.raises(ValueError, match="relu excludes gelu"):
            fn(x, w, None, gelu=True, relu=True)
