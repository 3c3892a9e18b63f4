"""Without a GPU: the dispatch of the message-passing forward as tests/mp_forward_restated.py restates it, the cases of
tests/test_gpu_mp_forward_fp64.py against it -- every case reaches the branch it names, by route() and by its own CSR; together they
cover every instantiation any supported input reaches; the rest is listed in UNREACHABLE -- and the float32 formula alone against
float64 on every case and class: 8 * e_32 stays under the cap of the rule."""
import torch

import mp_forward_restated as R

CAP = 1e-3
F32, F16 = torch.float32, torch.float16


def _masked(cls):
    return R.MASK_OF[cls] is not None


def test_route_on_values_worked_out_by_hand():
    r = lambda H, C, nmax, emax, form="rows", dt=F32, kernel="graph", B=3: R.route(H, C, nmax, emax, B, dt, form, kernel, False)
    # the table choice and the 40 KiB window: static = ECAP * 16 + ECAP * HS * 4 + (NCAP + 4) * 4
    assert r(4, 128, 64, 256) == ("grouped", 2, 1, True, "S", 33) and (40960 - (4096 + 2048 + 272)) // 1024 == 33
    assert r(4, 128, 20, 256) == ("grouped", 2, 1, True, "S", 20)
    assert r(4, 128, 65, 256) == r(4, 128, 64, 257)[:5] + (14,) == ("grouped", 2, 1, True, "L", 14)
    assert r(4, 128, 256, 1024) == ("grouped", 2, 1, True, "L", 14)
    assert r(4, 128, 257, 1024) == r(4, 128, 256, 1025) == ("chunk", 4, 2)
    # heads per workgroup: the largest hs | H with hs * C * 4 <= 1280
    assert [R.heads_per_workgroup(H, C) for H, C in [(8, 40), (8, 44), (4, 80), (4, 84), (2, 160), (2, 164), (6, 40), (16, 8), (3, 8)]] \
        == [8, 4, 4, 2, 2, 1, 2, 8, 1]
    assert r(2, 132, 30, 100) == ("grouped", 2, 2, False, "S", 30) and r(4, 68, 30, 100)[:4] == ("grouped", 4, 2, False)
    assert r(8, 36, 30, 100)[:4] == ("grouped", 8, 2, False) and r(8, 32, 30, 100)[:4] == ("grouped", 8, 1, True)
    # the 8-row floor on the large tables: HS = 8 never, HS = 4 up to C = 52
    assert r(8, 16, 65, 100) == ("chunk", 8, 1) and r(4, 52, 65, 100)[:5] == ("grouped", 4, 1, False, "L") and r(4, 56, 65, 100) == ("chunk", 4, 1)
    # 2 < P
    assert r(1, 512, 30, 100)[:4] == ("grouped", 1, 2, True) and r(1, 516, 30, 100) == ("chunk", 1, 3)
    # the flat rule: HS = 1, H > 1, P = 2, Q * 10 < 896
    assert r(4, 300, 64, 256) == ("flat", 3, 14) and r(4, 260, 10, 40) == ("flat", 3, 10) and r(4, 356, 64, 256) == ("flat", 3, 12)
    assert r(4, 256, 10, 40)[:4] == ("grouped", 1, 1, True) and r(4, 360, 10, 40)[:4] == ("grouped", 1, 2, False)
    assert r(1, 300, 10, 40)[:4] == ("grouped", 1, 2, False)
    assert r(4, 300, 65, 256) == r(4, 300, 64, 257) == ("chunk", 4, 5) and r(3, 300, 10, 40) == "unsupported"
    # which form exists where
    for form in ("rowmax", "logits_rowmax"):
        assert r(4, 128, 64, 256, form)[0] == "grouped" and r(4, 300, 64, 256, form) == "unsupported"
        assert r(4, 128, 257, 100, form) == "unsupported"
    for form in ("planes", "logits_planes"):
        assert r(4, 300, 64, 256, form) == ("flat", 3, 14) and r(4, 128, 64, 256, form) == "unsupported"
        assert r(2, 300, 64, 256, form) == r(8, 300, 64, 256, form) == "unsupported"
    assert r(2, 300, 64, 256, "logits") == ("flat", 3, 14) and r(4, 300, 64, 0, "logits") == "unsupported"
    assert r(4, 128, 64, 256, dt=F16) == r(4, 128, 64, 256, "logits", dt=F16) == ("grouped", 2, 1, True, "S", 33)
    assert r(4, 300, 64, 256, dt=F16) == r(4, 128, 257, 100, dt=F16) == r(4, 128, 64, 256, "rowmax", dt=F16) == "unsupported"
    # the node-chunk kernel
    assert r(4, 128, 64, 256, kernel="chunk") == ("chunk", 4, 2) and r(4, 128, 64, 256, dt=F16, kernel="chunk") == "unsupported"
    assert r(3, 8, 64, 256, kernel="chunk") == "unsupported" and r(3, 8, 64, 256) == ("grouped", 1, 1, False, "S", 64)
    assert r(8, 256, 9, 9, kernel="chunk") == ("chunk", 8, 8) and r(8, 260, 9, 9, kernel="chunk") == r(8, 516, 9, 9) == "unsupported"
    assert r(1, 2048, 9, 9) == ("chunk", 1, 8) and r(1, 2052, 9, 9) == "unsupported" and r(4, 6, 9, 9) == "unsupported"
    assert r(4, 128, 0, 0, B=0) == ("chunk", 4, 2) and r(4, 128, 0, 0, "rowmax", B=0) == "unsupported"


def _reachable():
    """Every instantiation route() returns over a grid that holds both sides of every threshold of the dispatch."""
    seen = {}
    tables = [(1, 0), (64, 256), (65, 256), (64, 257), (256, 1024), (257, 1024), (256, 1025)]
    for H in (1, 2, 3, 4, 5, 6, 8, 12, 16):
        for C in range(4, 2060, 4):
            for nmax, emax in tables:
                for dt in (F32, F16):
                    for form in R.FORMS:
                        for kernel in ("graph", "chunk"):
                            rt = R.route(H, C, nmax, emax, 2, dt, form, kernel, False)
                            for m in (False, True):
                                inst = R.instantiation(rt, m, dt == F16)
                                if inst is not None:
                                    seen.setdefault(inst, (H, C, nmax, emax))
    return seen


def test_unreachable_lists_exactly_what_no_input_reaches():
    seen = _reachable()
    every, dead = R.all_instantiations(), R.unreachable_instantiations()
    assert len(every) == 32 + 6 + 128 and dead <= every
    assert set(seen) == every - dead, (sorted(set(seen) & dead), sorted(every - dead - set(seen)))
    assert {k for k in seen if k[0] == "chunk"} == {("chunk", H, P) for H in (1, 2, 4, 8) for P in range(1, 9)}
    assert {k for k in seen if k[0] == "flat"} == {("flat", 3, False), ("flat", 3, True)}
    print(f"{len(every)} instantiations without dropout: {len(seen)} reachable, {len(dead)} unreachable "
          f"({len(R.UNREACHABLE['grouped'])} grouped (HS, P, exact, tables) x MASKED x F16, flat P = {R.UNREACHABLE['flat']} x MASKED)")


def _covered():
    """instantiation -> the cases and classes that launch it (fp32 rows; half rows where the grouped kernel takes them)."""
    cov = {}
    for case in R.CASES:
        for cls in R.classes_of(case.topo):
            for dt in (F32, F16):
                rt = R.case_route(case, "rows", dt, _masked(cls))
                inst = R.instantiation(rt, _masked(cls), dt == F16)
                if inst is not None:
                    cov.setdefault(inst, []).append(f"{case.id}/{cls}")
    return cov


def test_the_cases_cover_every_reachable_instantiation():
    cov, seen = _covered(), _reachable()
    missing = sorted(set(seen) - set(cov))
    assert not missing, f"no case launches {missing}"
    assert set(cov) <= set(seen)
    print("coverage (instantiation: cases x classes that launch it, the first of them)")
    for inst in sorted(cov, key=str):
        print(f"  {inst}: {len(cov[inst])}, e.g. {cov[inst][0]}")


def test_every_case_reaches_the_branch_it_names():
    for case in R.CASES:
        c = R.csr(case.topo)
        for masked in (False, True):
            rt = R.case_route(case, "rows", F32, masked)
            assert rt != "unsupported" and rt[0] == case.family and rt[:len(case.want)] == case.want, (case, rt)
        if case.family != "chunk":          # by the CSR: every graph inside the tables the route names, the window as the kernel sizes it
            small = c["nmax"] <= R.GK_NCAP_S and c["emax"] <= R.GK_ECAP_S
            assert small == (rt[0] == "flat" or rt[4] == "S") and c["nmax"] <= R.GK_NCAP_L and c["emax"] <= R.GK_ECAP_L, case
            assert 8 <= rt[-1] or rt[-1] == c["nmax"], case
        if case.kernel == "graph" and case.family == "chunk":      # ... or one graph outside them, or a width without an instantiation
            outside = c["nmax"] > R.GK_NCAP_L or c["emax"] > R.GK_ECAP_L
            assert outside or R._graph_route(case.H, case.C, c["nmax"], c["emax"], False, "rows") is None, case
    fams = {f: sum(1 for c in R.CASES if c.family == f) for f in ("chunk", "grouped", "flat")}
    print(f"{len(R.CASES)} cases: {fams}")
    # all 32 node-chunk (H, P) on the "small" topology with kernel="chunk", the last pass full and partly filled
    assert {c.want for c in R.CHUNK_CASES if c.topo == "small" and c.kernel == "chunk"} >= {("chunk", H, P) for H in (1, 2, 4, 8) for P in range(1, 9)}
    for H, P, C in R.CHUNK_HP:
        G, Q = 64 // H, C // 4
        assert (P - 1) * G < Q <= P * G and (Q == P * G) == (P % 2 == 1), (H, P, C)
    # the P = 2 instantiations the older cases never launched: C in (128, 160], (64, 80], (32, 40]
    for HS, lo, hi in ((2, 128, 160), (4, 64, 80), (8, 32, 40)):
        assert any(c.want[:3] == ("grouped", HS, 2) and lo < c.C <= hi for c in R.GROUPED_CASES), HS


def _graphs(topo):
    c = R.csr(topo)
    sizes = R.TOPOLOGIES[topo].sizes
    return [(g, sizes[g], int(c["eptr"][g + 1] - c["eptr"][g])) for g in range(c["B"])]


def test_topologies_hold_what_they_are_there_for():
    every = {t: _graphs(t) for t in R.TOPOLOGIES}
    for topo, graphs in every.items():
        batch, ei, sizes = R.topology(topo)
        c = R.csr(topo)
        assert bool((batch[ei[0]] == batch[ei[1]]).all()), topo                      # edges stay inside their graph
        assert c["nmax"] == max(sizes) and c["emax"] == max(ne for _, _, ne in graphs)
        for g, want in R.TOPOLOGIES[topo].slots.items():
            assert graphs[g][2] == want, (topo, g)
        if c["E"]:
            pairs = ei.t().tolist()
            assert len(set(map(tuple, pairs))) < len(pairs), topo                    # duplicate edges
            assert not torch.equal(ei[1], ei[1].sort().values), topo                 # shuffled order
        print(f"{topo}: graphs (nodes, slots) {[(n, ne) for _, n, ne in graphs]}")
        for g, n, ne in graphs:                                                       # the chosen nodes of every graph of >= 5 nodes
            if n >= 5 and c["E"]:
                p = int(c["ptr"][g])
                assert int(c["deg"][p + R.NO_IN]) == 0 and not bool((ei[0] == p + R.NO_OUT).any()), (topo, g)
                assert int(c["deg"][p + R.SINGLE]) == 1 and bool((ei[0] == p + R.NO_IN).any()) and int(c["deg"][p + R.NO_OUT]) > 0
                assert not bool(((ei[0] == ei[1]) & (ei[0] >= p) & (ei[0] < p + 4) & (ei[0] > p)).any()), (topo, g)   # no self loop on them
    small = every["small"]
    assert [n for _, n, _ in small] == [1, 1, 5, 0, 9, 17, 3, 0, 0]                  # an empty graph in the middle, trailing ones
    assert small[0][2] == 1 and small[1][2] == 2                                      # a one-node graph with only its self loop
    sizes = {n for g in every.values() for _, n, _ in g}
    assert {1, 0, 64, 65, 256, 257, 16, 17, 14, 15, 33, 34} <= sizes
    assert R.csr("n16")["N"] == R.MP_NPB and R.csr("n17")["N"] == R.MP_NPB + 1 and R.csr("e0")["E"] == 0
    slots = {ne for g in every.values() for _, _, ne in g}
    assert {256, 257, 1024, 1025} <= slots and {ne % 4 for ne in slots if ne} >= {0, 1, 3}
    assert every["t64"][0][1:] == (64, 256) and every["e257"][0][1:] == (64, 257)
    assert every["t256"][0][1:] == (256, 1024) and every["t257"][0][1] == 257 and every["e1025"][0][2] == 1025
    # a hub with in-degree above MP_LCAP inside the small tables; the big one: the first 16-node block holds more than MP_ECAP slots
    # and the hub's segment straddles slot 1024
    c = R.csr("small")
    hub = int(c["ptr"][5])
    assert R.MP_LCAP < int(c["deg"][hub]) and c["emax"] <= R.GK_ECAP_S
    c = R.csr("hub")
    assert int(c["deg"][0]) > 1100 and int(c["rowptr"][R.MP_NPB]) > R.MP_ECAP and int(c["rowptr"][0]) < R.MP_ECAP < int(c["rowptr"][1])
    assert int(c["rowptr"][R.MP_NPB]) - int(c["rowptr"][1]) > 0                        # destinations whose every slot lies beyond the staged ones
    # the windows: a graph of exactly lrows nodes, one of lrows + 1 with sources on both sides of the window
    for topo, H, C, lrows in R.WINDOWS:
        c = R.csr(topo)
        rt = R.route(H, C, c["nmax"], c["emax"], c["B"], F32, "rows", "graph", False)
        assert rt[-1] == lrows, (topo, H, C, rt)
        _, ei, _ = R.topology(topo)
        at = {n: g for g, n, _ in every[topo]}
        assert lrows in at and lrows + 1 in at, (topo, lrows)
        p = int(c["ptr"][at[lrows + 1]])
        local = ei[0][(ei[0] >= p) & (ei[0] < p + lrows + 1)] - p
        assert bool((local == lrows).any()) and bool((local < lrows).any()), (topo, lrows)
    assert len({(w[1], w[2], w[3]) for w in R.WINDOWS}) >= 2
    # the "dead" class: a destination with in-edges, all masked, and a graph masked completely
    for topo in R.TOPOLOGIES:
        if "dead" in R.classes_of(topo):
            node, graph = R.dead_parts(topo)
            t = R.inputs(topo, 4, 8, "dead")
            _, ei, _ = R.topology(topo)
            assert int(R.csr(topo)["deg"][node]) >= 2 and float(t["edge_mask"][ei[1] == node].abs().max()) == 0.0, topo
            assert (graph is None) == (sum(1 for _, n, ne in every[topo] if n >= 2 and ne) < 2), topo
    t = R.inputs("small", 4, 8, "mask01")
    assert bool((t["node_mask"] == R.ST).any()) and bool((t["node_mask"] == 0).any()) and R.ST < 1.0
    t = R.inputs("small", 4, 8, "frac")["edge_mask"]
    assert bool((t == 0).any()) and bool(((t > 0) & (t < 1)).any()) and bool((t > 1).any())


def _e32(ref64, ref32):
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    return 0.0 if scale == 0.0 else float((ref32.double() - ref64).abs().max()) / scale


def test_the_float32_formula_alone_is_well_posed_on_every_case_and_class():
    worst, seen = {}, set()
    for case in R.CASES:
        key = (case.topo, case.H, case.C)
        if key in seen:
            continue
        seen.add(key)
        line = []
        for cls in R.classes_of(case.topo):
            figs = []
            for half in (False, True):
                r64, r32 = R.reference(*key, cls, torch.float64, half), R.reference(*key, cls, torch.float32, half)
                _, l64 = R.reference_from_logits(*key, cls, torch.float64, half)
                _, l32 = R.reference_from_logits(*key, cls, torch.float32, half)
                for a, b in ((r64, r32), (l64, l32)):
                    for k in ("out", "alpha"):
                        assert a[k].dtype == torch.float64 and b[k].dtype == torch.float32
                        assert bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), (key, cls, k)
                        figs.append(_e32(a[k], b[k]))
                assert torch.equal(l64["logits"], l32["logits"].double())          # both start from the same float32 logits
            e = max(figs)
            assert 8 * e <= CAP, f"{key} {cls}: the float32 formula alone is {e:.3e} off: ill-posed"
            worst[cls] = max(worst.get(cls, 0.0), e)
            line.append(f"{cls} {e:.1e}")
            lg = R.reference(*key, cls, torch.float64)["logits"]
            if cls == "shift" and lg.numel():
                assert 25.0 < float(lg.median()) < 40.0 and float(lg.min()) > 15.0, (key, float(lg.median()), float(lg.min()))
            if cls == "far" and lg.numel():       # exp overflows in float32 without the maximum
                assert float(lg.min()) > 89.0 and float(lg.max()) < 115.0, (key, float(lg.min()), float(lg.max()))
            if cls == "dead":
                _, ei, _ = R.topology(case.topo)
                node, graph = R.dead_parts(case.topo)
                r64 = R.reference(*key, cls, torch.float64)
                bias = R.inputs(*key, cls)["bias"].double()
                assert torch.equal(r64["out"][node], bias) and bool((r64["alpha"][ei[1] == node] == 1.0 / int((ei[1] == node).sum())).all())
        print(f"e_32 {case.topo} H{case.H} C{case.C}: " + ", ".join(line))
    for cls, e in worst.items():
        print(f"float32 formula against float64, worst of {cls}: {e:.2e}  ({CAP / (8 * max(e, 1e-30)):.0f} x under the cap at F = 8)")
    sharp = max(float(R.reference(c.topo, c.H, c.C, "sharp", torch.float64)["logits"].abs().max()) for c in R.CASES if R.csr(c.topo)["E"])
    assert sharp > 30.0, sharp
    print(f"largest |logit| of the sharp class: {sharp:.1f}")
