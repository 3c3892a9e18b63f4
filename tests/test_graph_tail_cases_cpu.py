"""Without a GPU: the cases of tests/test_gpu_graph_tail_fp64.py reach the branches they are there for, and the reference alone is
well-posed on every case and class -- the restatement in float32 against itself in float64 stays below the cap of the rule."""
import torch

import test_gpu_graph_tail_fp64 as T



def test_named_batches_have_the_fills_they_claim():
    tiles = {name: T.fused_tiles(name) for name in T.FUSED_NAMES}
    per = {name: [w[1] for w in tiles[name]] for name in T.FUSED_NAMES}
    for name in T.FUSED_NAMES:
        sizes, batch, ei = T.fused_batch(name)
        assert torch.bincount(batch, minlength=len(sizes)).tolist() == sizes, name
        assert torch.bincount(batch[ei[1]], minlength=len(sizes)).tolist() == sizes, name           # one slot per node: the node cap decides
        assert max(sizes) <= 64 and all(w[2] <= 64 for w in tiles[name]), name
        print(f"{name}: {len(sizes)} graphs, {batch.numel()} nodes, {len(tiles[name])} tiles, up to {max(per[name])} graphs a tile")
    # nine: every tile nine graphs and 64 nodes -- one graph past DT_GST
    assert per["nine"] == [9, 9, 9] and all(w[2] == 64 for w in tiles["nine"]) and T.DT_GST + 1 == 9
    # ones64: 64 one-node graphs a tile: two statistics rounds of 32
    assert per["ones64"] == [64, 64, 64] and 2 * T.STAT_ROUND == 64
    # pairs33: 33 graphs, the second round holds one graph, of one node
    assert per["pairs33"] == [33, 33, 33] and T.fused_sizes("pairs33")[T.STAT_ROUND] == 1
    # empties: a tile beyond DT_GPC / RO_GPC graphs with nodes BEHIND graph 128 of it; the last tile 70 graphs without a node,
    # alone behind the chunk edge at graph 1024
    s = T.fused_sizes("empties")
    assert tiles["empties"][0][:2] == (0, 166) and 166 > T.DT_GPC and sum(s[T.DT_GPC:166]) > 0 and s[165] == 40
    assert tiles["empties"][-1] == (1024, 70, 0) and s[1023] > 0
    # chunk_edge: the tile ending at graph 1024 is cut short; full tiles of 21 before it, the rest behind it
    ce = tiles["chunk_edge"]
    short = [w for w in ce if w[0] + w[1] == 1024]
    assert short == [(1008, 16, 48)] and ce[ce.index(short[0]) - 1] == (987, 21, 63) and ce[-1] == (1024, 6, 18)
    assert all(w[1] == 21 for w in ce[:-2])
    # mixed_small: a few hundred graphs of 1-6 nodes, tiles between 9 and 32 graphs
    ms = T.fused_sizes("mixed_small")
    assert len(ms) == 300 and set(ms) == {1, 2, 3, 4, 5, 6} and min(per["mixed_small"][:-1]) > T.DT_GST
    # the three thresholds, over all batches
    every = [n for name in T.FUSED_NAMES for n in per[name]]
    assert any(T.DT_GST < n <= T.STAT_ROUND for n in every) and any(T.STAT_ROUND < n <= T.DT_GPC for n in every)
    assert any(n > T.DT_GPC for n in every)
    # the constant class runs where sums of equal rows are exact whatever the row: graphs of one and two nodes
    for name in T.EXACT_BATCHES:
        assert set(T.fused_sizes(name)) <= {1, 2}
    # the unpicked graph's instruction row is not among the DT_GST staged ones, in `empties` its offsets not among the DT_GPC
    for name in T.FUSED_NAMES:
        g = T.fused_inputs(name, "unpicked")["unpicked"]
        tile = next(w for w in tiles[name] if w[0] <= g < w[0] + w[1])
        assert g - tile[0] >= T.DT_GST and T.fused_sizes(name)[g] > 0, name
    g = T.fused_inputs("empties", "unpicked")["unpicked"]
    assert g >= T.DT_GPC and g < 166


def test_per_graph_cases_hold_the_boundary_values():
    assert set(T.PG_C) >= {4, 8, 100, 128, 300, 324, 512, 516, 1024} and all(C % 4 == 0 for C in T.PG_C)
    assert T.GN_CMAX in T.PG_C and T.GN_CMAX + 4 in T.PG_C and max(T.PG_C) >= 2 * T.GN_CMAX          # the strips boundary; two channels a thread
    block = lambda C: 64 if C <= 64 else 128 if C <= 128 else 256 if C <= 256 else 320 if C <= 320 else 384 if C <= 384 else 512
    assert {block(C) for C in T.PG_C} == {64, 128, 256, 320, 384, 512} and block(300) == 320 and block(324) == 384
    assert any(block(C) % C for C in T.PG_C if C <= T.GN_CMAX)                                          # idle threads in the last pass
    want = {1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024}
    assert set(T.PG_SHORT) | set(T.PG_LONG) == want and set(T.PG_LONG_C) == {8, 128, 516}
    for C in T.PG_C:
        s = T.pg_sizes(C)
        assert set(T.PG_SHORT) <= set(s) and s[0] == 0 and s[-1] == 0 and 0 in s[1:-1], C
        assert (set(T.PG_LONG) <= set(s)) == (C in T.PG_LONG_C), C
        assert max(s) <= T.GN_NCAP
        t = T.pg_inputs(C, "unpicked")
        assert s[t["unpicked"]] >= 2 and bool((t["mask"][t["batch"] == t["unpicked"]] == 0).all())
        assert bool((T.pg_inputs(C, "st")["mask"] == T.ST).any()) and T.ST < 1.0
    # phase_softmax's two summation forms, phase_logits' and the column passes' partly filled last rounds, the full strip
    long = T.pg_sizes(128)
    assert {128, 129} <= set(long) and T.GN_NCAP in long and any(n % T.PL_U for n in long) and any(n % T.GT_U for n in long)
    assert set(T.pg_sizes(8, "const_exact")) - {0} == set(T.PG_CONST) == {1, 2, 4, 16, 64}
    key = T.pg_inputs(128, "const_exact")["key"]
    assert bool((key * 256 == (key * 256).round()).all()) and float(key.abs().max()) < 8.0          # 12 mantissa bits


def _well_posed(what, ref64, ref32, per_row=False):
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32, what
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all()), what
    e_k, e_32, _ = T.errors(ref32, ref64, ref32, per_row)
    if e_32 is not None:
        assert T.F * e_32 <= T.CAP, f"{what}: the float32 formula alone is {e_32:.3e} off: ill-posed"
    return e_32 or 0.0


def test_the_reference_alone_is_well_posed_on_every_case_and_class():
    worst = {}
    for C in T.PG_C:
        for cls in T.PG_CLASSES:
            r64, r32 = T.pg_ref(C, cls, torch.float64), T.pg_ref(C, cls, torch.float32)
            for k in ("scatter_attention", "graph_norm", "layer_tail", "attn_pool", "gate"):
                if cls in T.PG_APPLIES.get(k, T.PG_CLASSES):
                    e = _well_posed(f"C{C} {cls} {k}", r64[k], r32[k])
                    worst[cls] = max(worst.get(cls, 0.0), e)
            if cls == "const_exact":          # exact in float32: the formula gives the bias, bit for bit
                t = T.pg_inputs(C, cls)
                assert torch.equal(r32["graph_norm"], t["b"].expand(t["N"], C)), C
                assert torch.equal(r32["layer_tail"], t["b"].expand(t["N"], C) + t["h"]), C
    for name in T.FUSED_NAMES:
        for cls in T.fused_classes(name):
            per_row = cls == "outlier"
            d64, d32 = T.dense_tail_ref(name, cls, torch.float64), T.dense_tail_ref(name, cls, torch.float32)
            for form in ("inner", "last"):
                for i, part in enumerate(("h'", "gated rows")):
                    if d64[form][i] is not None:
                        e = _well_posed(f"{name} {cls} dense tail {form} {part}", d64[form][i], d32[form][i], per_row)
                        worst["fused " + cls] = max(worst.get("fused " + cls, 0.0), e)
            if cls == "const_exact":
                continue
            r64, r32 = T.readout_ref(name, cls, torch.float64), T.readout_ref(name, cls, torch.float32)
            for form in r64:
                e = _well_posed(f"{name} {cls} readout {form} pooled", r64[form]["out"], r32[form]["out"], per_row)
                worst["fused " + cls] = max(worst.get("fused " + cls, 0.0), e)
                _well_posed(f"{name} {cls} readout {form} gate", r64[form]["gate"], r32[form]["gate"])
            t = T.fused_inputs(name, cls)
            empty = torch.tensor([n == 0 for n in t["sizes"]])
            assert bool((r64["masked"]["out"][empty] == 0).all())
            if cls == "shift":          # the logits do sit near +100: exp overflows in float32 without the maximum
                assert float(r64["unmasked"]["logits"].median()) > 89.0, name
    for k in sorted(worst):
        print(f"float32 formula against float64, worst of {k}: {worst[k]:.2e}")
    for C in T.PG_C:
        lg = T.pg_ref(C, "shift", torch.float64)["logits"]
        assert float(lg.median()) > 89.0, C
