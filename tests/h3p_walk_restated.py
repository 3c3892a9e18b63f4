"""Which kernel isg_linear_h3p launches for a shape and how its workgroups walk the tiles (csrc/isg_gemm_h3p.hip: the wrapper's
dispatch and linear_h3q_kernel's origin / next_tile), restated in plain Python, plus the case lists of
tests/test_gpu_linear_h3p_paths.py.  No torch, no GPU: tests/test_h3p_walk_cpu.py proves on the host, for 256 CUs, that the case
lists reach every instantiation and walk regime they claim; the GPU tests repeat the proof with the device's CU count before they
launch anything."""
from collections import namedtuple

P3_T = 256                      # the 256 x 256 form's tile
Q3_BM, Q3_BN = 256, 128         # the persistent form's tile
Q3_HEAD = 8                     # fewest k-tiles of the persistent form

Inst = namedtuple("Inst", "form act planes_out head seg")        # form: "p256" (linear_h3p_kernel) / "q" (linear_h3q_kernel)
Report = namedtuple("Report", "inst kt kt_mod3 tiles_m slots_m tiles_n total_l grid valid depth depth_counts padding_first "
                              "padding_first_then_valid ragged_row_inflight ragged_row_epilogue ragged_col_inflight "
                              "ragged_col_epilogue walks")

ACTS = (None, "gelu", "relu")


def kt_of(K):
    return (K + 31) // 32


def roundup8(v):
    return (v + 7) // 8 * 8


def instantiation(K, act, planes_out, seg=False):
    """The template arguments the wrapper picks: the 256 x 256 form below 8 k-tiles, else the persistent form with HEAD 8 below 16
    k-tiles and HEAD 16 from there; a segmented A operand has the two HEAD 16 GELU instantiations of its own."""
    assert act in ACTS
    KT = kt_of(K)
    if KT < Q3_HEAD:
        assert not seg
        return Inst("p256", act, bool(planes_out), 0, False)
    if seg:
        assert KT >= 16 and act == "gelu"
        return Inst("q", act, bool(planes_out), 16, True)
    return Inst("q", act, bool(planes_out), 16 if KT >= 16 else 8, False)


def all_instantiations(seg=False):
    """The 18 non-segmented instantiations (6 of the 256 x 256 form, 6 each at HEAD 8 and HEAD 16), or the 2 segmented ones."""
    if seg:
        return {Inst("q", "gelu", po, 16, True) for po in (False, True)}
    return ({Inst("p256", a, po, 0, False) for a in ACTS for po in (False, True)} |
            {Inst("q", a, po, h, False) for a in ACTS for po in (False, True) for h in (8, 16)})


def origin(L, M, tiles_n, bm, bn):
    """Entry L of the XCD-aware order -> (m0, n0), or None for a padding entry (a row tile beyond M)."""
    slot = L >> 3
    m0 = ((L & 7) + 8 * (slot // tiles_n)) * bm
    n0 = (slot % tiles_n) * bn
    return (m0, n0) if m0 < M else None


def walks(M, N, K, ncu):
    """Per workgroup: (is its first entry a padding entry, [the (m0, n0) of the valid tiles it visits, in order]).  The 256 x 256
    form launches one workgroup per entry and each does its own tile or returns."""
    KT = kt_of(K)
    tiles_m = (M + 255) // 256
    if KT < Q3_HEAD:
        tiles_n = (N + P3_T - 1) // P3_T
        total_l = tiles_n * roundup8(tiles_m)
        out = []
        for L in range(total_l):
            o = origin(L, M, tiles_n, P3_T, P3_T)
            out.append((o is None, [] if o is None else [o]))
        return tiles_m, tiles_n, total_l, total_l, out
    tiles_n = (N + Q3_BN - 1) // Q3_BN
    total_l = tiles_n * roundup8(tiles_m)
    G = min(total_l, ncu)
    out = []
    for b in range(G):
        tiles = [o for o in (origin(L, M, tiles_n, Q3_BM, Q3_BN) for L in range(b, total_l, G)) if o is not None]
        out.append((origin(b, M, tiles_n, Q3_BM, Q3_BN) is None, tiles))
    return tiles_m, tiles_n, total_l, G, out


def store_paths(M, N, K, ncu):
    """(m0, n0) of every valid tile -> "inflight" (stored piece by piece during the workgroup's next tile) or "epilogue" (the last
    tile of its workgroup's walk; every tile of the 256 x 256 form)."""
    paths = {}
    for _, tiles in walks(M, N, K, ncu)[4]:
        for i, t in enumerate(tiles):
            assert t not in paths, "a tile visited twice"
            paths[t] = "epilogue" if i == len(tiles) - 1 else "inflight"
    return paths


def report(M, N, K, act, planes_out, ncu):
    inst = instantiation(K, act, planes_out)
    tiles_m, tiles_n, total_l, G, w = walks(M, N, K, ncu)
    bm, bn = (P3_T, P3_T) if inst.form == "p256" else (Q3_BM, Q3_BN)
    paths = store_paths(M, N, K, ncu)
    assert len(paths) == tiles_m * tiles_n, "the walk misses a tile"
    rag = {(kind, p) for (m0, n0), p in paths.items() for kind, r in (("row", m0 + bm > M), ("col", n0 + bn > N)) if r}
    counts = {}
    for _, tiles in w:
        counts[len(tiles)] = counts.get(len(tiles), 0) + 1
    return Report(inst, kt_of(K), kt_of(K) % 3, tiles_m, roundup8(tiles_m), tiles_n, total_l, G, len(paths),
                  max(len(t) for _, t in w), counts, any(p for p, _ in w), any(p and t for p, t in w),
                  ("row", "inflight") in rag, ("row", "epilogue") in rag, ("col", "inflight") in rag, ("col", "epilogue") in rag, w)


def inflight_row_tiles(M, N, K, ncu):
    """Row tiles (index m0 / 256) ALL of whose column tiles are stored in flight."""
    paths = store_paths(M, N, K, ncu)
    rows = sorted({m0 for m0, _ in paths})
    return [m0 // 256 for m0 in rows if all(p == "inflight" for (m, _), p in paths.items() if m == m0)]


def inflight_block(M, N, K, ncu, rows=300, lead=100):
    """First row of a `rows`-row block in the middle of the batch, `lead` rows into a row tile, every tile under which is stored in
    flight (the block spans two row tiles); None when the walk has no such pair."""
    ok = inflight_row_tiles(M, N, K, ncu)
    assert lead + rows <= 512
    pairs = [t for t in ok if t + 1 in ok and t > 0]
    if not pairs:
        return None
    return pairs[len(pairs) // 2] * 256 + lead


# ---- the case lists of tests/test_gpu_linear_h3p_paths.py -----------------------------------------------------------------------
# part 2: every instantiation at its smallest shape.  M = 300: two row tiles, the second with 44 rows (SMALL_M_FP32: more full
# ones before it).  KT = 2, 7 | 8, 9, 15 | 16, 17, 18: both sides of both HEAD steps, a K tail in each form, body loops of 0, 1, 7
# (HEAD 8) and 0, 1, 2 (HEAD 16) k-tiles.
SMALL_M = 300
SMALL_KS = (36, 224, 256, 260, 480, 512, 516, 576)
SMALL_GROUPS = {"p256": (36, 224), "q8": (256, 260, 480), "q16": (512, 516, 576)}
# fp32 results whose 1.5 e32 bound is undecidable at 300 rows, raised to the next 300 + 256 k (the same last row tile of 44 rows)
# at which it decides; the measurements and the reasons are in the docstring of tests/test_gpu_linear_h3p_paths.py
SMALL_M_FP32 = {36: 556, 516: 1068, 576: 1068}


def small_m(K, planes_out):
    return SMALL_M if planes_out else SMALL_M_FP32.get(K, SMALL_M)


def small_n(K, planes_out):
    """132 = 128 + 4 columns (one ragged 256-column tile in the 256 x 256 form); that form's planes32 result refuses N % 32."""
    return 160 if planes_out and kt_of(K) < Q3_HEAD else 132


def small_cases(group=None, planes_out=None):
    """(M, N, K, act, planes_out, bias) of part 2."""
    ks = SMALL_KS if group is None else SMALL_GROUPS[group]
    pos = (False, True) if planes_out is None else (planes_out,)
    return [(small_m(K, po), small_n(K, po), K, act, po, bias) for K in ks for po in pos for act in ACTS for bias in (True, False)]


# part 3: the tile-walk regimes at the smallest size that reaches them on 256 CUs; each with an fp32 and a planes32 result
W1 = [(16540, 516, 260, "gelu", po, True) for po in (False, True)]
W2_KS = (256, 288, 320, 512, 544, 576)
W2_EXTRA_KS = (288, 544)                       # one K per HEAD form also with ReLU and no bias
W2 = ([(26500, 1028, K, None, po, True) for K in W2_KS for po in (False, True)] +
      [(26500, 1028, K, "relu", po, False) for K in W2_EXTRA_KS for po in (False, True)])
W3 = [(700, 4100, 256, None, po, True) for po in (False, True)]
WALK_CASES = W1 + W2 + W3
ROW_POSITION_CASES = W1 + [c for c in W2 if c[2] in (288, 576) and c[3] is None]


def regimes(cases, ncu):
    """What a case list reaches on `ncu` CUs: the facts the CPU test and the GPU tests assert."""
    reps = [report(M, N, K, act, po, ncu) for M, N, K, act, po, _ in cases]
    q = [r for r in reps if r.inst.form == "q"]
    return {
        "instantiations": {r.inst for r in reps},
        "max_depth": max(r.depth for r in reps),
        "head8_max_depth": max([r.depth for r in q if r.inst.head == 8], default=0),
        "kt_mod3_at_depth3": {h: {r.kt_mod3 for r in q if r.inst.head == h and min(len(t) for _, t in r.walks) >= 3} for h in (8, 16)},
        "padding_first": any(r.padding_first for r in q),
        "padding_first_then_valid": any(r.padding_first_then_valid for r in q),
        "ragged_row_inflight": any(r.ragged_row_inflight for r in q),
        "ragged_row_epilogue": any(r.ragged_row_epilogue for r in q),
        "ragged_col_inflight": any(r.ragged_col_inflight for r in q),
        "ragged_col_epilogue": any(r.ragged_col_epilogue for r in q),
    }
