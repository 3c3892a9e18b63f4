"""Which kernel instantiation each Linear launcher but isg_linear_h3p's picks for a call, and what that launch does at its edges
(csrc/isg_gemm.hip linear_launch, csrc/isg_gemm_panel.hip panel_launch, csrc/isg_gemm_f16x3.hip linear_f16x3_launch and
isg_linear_f16x3_tile, csrc/isg_gemm_skinny.hip isg_linear_skinny, ops._k_chunks), restated in plain Python, plus the case lists of
tests/test_gpu_linear_forms_fp64.py.  No torch, no GPU: tests/test_linear_forms_cpu.py proves on the host that the case lists reach
every instantiation a supported input reaches, each with every store form it has; the GPU tests ask form() again before each launch.

Routes: the seven of ops.linear_route that are not the engine's -- "bf16x6", "bf16x6_f16", "panel", "f16x3", "f16x3_f16",
"f16x3_tile", "skinny" -- and "rowbias" (isg_linear_bf16x6_rowbias: linear_launch with a segment vector)."""
from collections import namedtuple

# ---- constants, named after the ones in csrc/ they restate ------------------------------------------------------------------------
GM_BM, GM_BN, GM_BK = 128, 128, 32          # isg_gemm.hip: the tile kernel's tile
DUAL_K = 256                                # linear_launch: dual = K > dual_k (ISG_GEMM_DUAL_K)
PN_BM, PN_KC = 64, 128                      # isg_gemm_panel.hip: rows per panel, k per LDS chunk (SINGLE: KS <= 8 = PN_KC / 16)
H3_BM, H3_KC = 64, 128                      # isg_gemm_f16x3.hip: the panel form, K <= H3_KC
HT_BM, HT_BN, HT_BK = 128, 128, 32          # isg_gemm_f16x3.hip: the tile form
SK_T, SK_WAVES = 16, 8                      # isg_gemm_skinny.hip
NT_MB = 128                                 # ISG_GEMM_NT_MB's default in all four matrix-core launchers (MB = 10^6 bytes)
K_CHUNK = 640                               # ops._k_chunks: the longest chain of isg_linear_f16x3_tile
F16X3_MFMA = 16                             # isg_linear_f16x3_tile: mf, unless ISG_F16X3_MFMA=32

ACTS = (0, 1, 2)                            # 0 none, 1 exact GELU, 2 ReLU
ACT_NAMES = {0: "none", 1: "gelu", 2: "relu"}
ROUTES = ("bf16x6", "bf16x6_f16", "rowbias", "panel", "f16x3", "f16x3_f16", "f16x3_tile", "skinny")

Bf16x6 = namedtuple("Bf16x6", "kernel act a16 d16 xcd dual rowb")          # linear_bf16x6_kernel<ACT, 0, A16, D16, XCD, DUAL, ROWB>
Panel = namedtuple("Panel", "kernel act wtn a16 d16 single")               # linear_panel_kernel<ACT, WTN, A16, D16, SINGLE>
F16x3 = namedtuple("F16x3", "kernel act wtn f16d")                         # linear_f16x3_kernel<ACT, WTN, F16D>
F16x3Tile = namedtuple("F16x3Tile", "kernel act xcd rmax accum mf")        # linear_f16x3_tile_kernel<ACT, XCD, RMAX, ACCUM, MF>
Skinny = namedtuple("Skinny", "kernel act")                                # linear_skinny_kernel<ACT>
Chunk = namedtuple("Chunk", "k0 kc accum inst")
Form = namedtuple("Form", "inst streaming stores padding chunks")


class Refused(Exception):
    """The launcher returns ISG_EINVAL / ISG_EUNSUPPORTED for this call."""


def roundup(v, m):
    return (v + m - 1) // m * m


def k_chunks(K):
    """ops._k_chunks: (number of chunks, columns per chunk)."""
    nchunk = (K + K_CHUNK - 1) // K_CHUNK
    return nchunk, roundup((K + nchunk - 1) // nchunk, 32)


def wtn_of(N):
    """panel_launch / linear_f16x3_launch: subtiles per wave and pass -- the wider tile unless it idles much more of the last pass."""
    NT = (N + 31) // 32
    waste = lambda w: roundup(NT, 4 * w) - NT
    return 2 if waste(2) <= waste(1) + 1 else 1


def streams(M, N, out_bytes, env):
    """Bit 0 of the launchers' nt flag: the result is at least ISG_GEMM_NT_MB (10^6-byte) megabytes."""
    nt_mb = int(env.get("ISG_GEMM_NT_MB", NT_MB))
    return nt_mb >= 0 and M * N * out_bytes >= nt_mb * 1000000


def _tile_stores(M, N, ldd, d_align, nt, half, has_nt):
    """The store forms of the 32-column subtiles of the two 128 x 128 tile kernels: vec_ok = 4 | ldd, the whole subtile inside N, D
    16-byte aligned; the streaming branch exists for fp32 results only (linear_bf16x6_kernel's D16 branch has none)."""
    out = set()
    for colb in range(0, N, 32):
        vec = ldd % 4 == 0 and colb + 32 <= N and d_align % 16 == 0
        out.add(("vector_nt" if nt and has_nt and not half else "vector") if vec else "scalar")
    return out


def _panel_stores(M, N, bm, nt, has_nt):
    """The row-panel kernels store lane by lane: whole panels of whole subtiles without a condition, the rest guarded."""
    out = set()
    if M >= bm and N >= 32:                    # a whole panel under a whole subtile
        out.add("full")
    if M % bm != 0 or N % 32 != 0:             # a ragged last panel or a ragged last subtile
        out.add("guarded")
    return {s + ("_nt" if nt and has_nt else "") for s in out}


def form(route, M, N, K, act, a16=False, d16=False, ldd=None, d_align=0, rowmax_out=False, env=None, out_cols=None):
    """What the launcher of `route` does with act(x[M, K] @ w[N, K]^T + b): Form(instantiation, streaming flag, store forms of its
    column subtiles, padding workgroups of the rounded grid, [Chunk] for f16x3_tile else None).  d_align: the result pointer modulo
    16; env: the environment the library read at its first launch ({} = defaults).  Raises Refused where the launcher refuses."""
    env = {} if env is None else env
    ldd = N if ldd is None else ldd
    out_cols = N if out_cols is None else out_cols
    assert route in ROUTES and act in ACTS and M > 0
    if K % 4:
        raise Refused("4 | K")
    if route in ("bf16x6", "bf16x6_f16", "rowbias"):
        if route == "bf16x6" and (a16 or d16):
            raise Refused("isg_linear_bf16x6 is fp32 in, fp32 out")
        if route == "rowbias" and a16:
            raise Refused("the row-biased Linear reads fp32 rows")
        if act == 2 and (a16 or d16):
            raise Refused("ReLU has no half-row form")
        if ldd < N:
            raise Refused("ldd < N")
        tiles_n, mt = (N + GM_BN - 1) // GM_BN, (M + GM_BM - 1) // GM_BM
        xcd = tiles_n > 1 and "ISG_GEMM_NO_XCD" not in env
        dual = K > int(env.get("ISG_GEMM_DUAL_K", DUAL_K))
        nt = streams(M, N, 2 if d16 else 4, env)
        inst = Bf16x6("linear_bf16x6_kernel", act, bool(a16), bool(d16), xcd, dual, route == "rowbias")
        return Form(inst, nt, _tile_stores(M, N, ldd, d_align, nt, d16, True), tiles_n * (roundup(mt, 8) - mt) if xcd else 0, None)
    if route == "panel":
        if act == 2:
            raise Refused("the panel kernel has no ReLU")
        if (out_cols < N and out_cols % 32) or N % out_cols or ldd < out_cols:
            raise Refused("out_cols")
        forced = int(env.get("ISG_PANEL_WTN", 0))
        wtn = forced if forced in (1, 2) else wtn_of(N)
        nt = streams(M, N, 2 if d16 else 4, env)
        inst = Panel("linear_panel_kernel", act, wtn, bool(a16), bool(d16), (K + 15) // 16 <= PN_KC // 16)
        return Form(inst, nt, _panel_stores(M, N, PN_BM, nt, not d16), 0, None)          # PN_EPI streams fp32 results only
    if route in ("f16x3", "f16x3_f16"):
        if act == 2:
            raise Refused("the f16x3 panel kernel has no ReLU")
        if K > H3_KC:
            raise Refused("K > 128")
        if a16:
            raise Refused("fp32 rows in")
        if (out_cols < N and out_cols % 32) or N % out_cols or ldd < out_cols:
            raise Refused("out_cols")
        half = route == "f16x3_f16"
        nt = streams(M, N, 2 if half else 4, env)
        inst = F16x3("linear_f16x3_kernel", act, wtn_of(N), half)
        return Form(inst, nt, _panel_stores(M, N, H3_BM, nt, True), 0, None)               # H3_EPI streams both result types
    if route == "f16x3_tile":
        if a16 or d16:
            raise Refused("fp32 in, fp32 out")
        if ldd < N:
            raise Refused("ldd < N")
        tiles_n, mt = (N + HT_BN - 1) // HT_BN, (M + HT_BM - 1) // HT_BM
        xcd = tiles_n > 1
        mf = 32 if env.get("ISG_F16X3_MFMA") == "32" else F16X3_MFMA
        nt = streams(M, N, 4, env)
        nchunk, step = k_chunks(K)
        chunks, k0 = [], 0
        while k0 < K:              # ops._linear_f16x3_tile: bias, activation and the row maxima with the last chunk only
            kc = min(step, K - k0)
            last = k0 + kc >= K
            chunks.append(Chunk(k0, kc, k0 > 0, F16x3Tile("linear_f16x3_tile_kernel", act if last else 0, xcd,
                                                           bool(rowmax_out) and last, k0 > 0, mf)))
            k0 += kc
        assert len(chunks) == nchunk
        return Form(chunks[-1].inst, nt, _tile_stores(M, N, ldd, d_align, nt, False, True),
                    tiles_n * (roundup(mt, 8) - mt) if xcd else 0, chunks)
    if a16 or d16:
        raise Refused("isg_linear_skinny is fp32 in, fp32 out")
    if ldd < N:
        raise Refused("ldd < N")
    return Form(Skinny("linear_skinny_kernel", act), False, {"guarded"}, 0, None)


def instantiations(f):
    """Every kernel instantiation a call launches (f16x3_tile: one per K chunk)."""
    return {c.inst for c in f.chunks} if f.chunks else {f.inst}


def store_forms(inst):
    """The store forms an instantiation has under the default environment (results below ISG_GEMM_NT_MB)."""
    if isinstance(inst, (Bf16x6, F16x3Tile)):
        return {"vector", "scalar"}
    if isinstance(inst, Skinny):
        return {"guarded"}
    return {"full", "guarded"}


def reachable():
    """Every instantiation a supported input reaches under the default environment: 56 + 32 + 8 + 24 + 3 = 123."""
    out = set()
    for xcd in (False, True):
        for dual in (False, True):
            for a16, d16 in ((False, False), (True, False), (False, True), (True, True)):
                for act in (ACTS if not (a16 or d16) else (0, 1)):
                    out.add(Bf16x6("linear_bf16x6_kernel", act, a16, d16, xcd, dual, False))
            for d16 in (False, True):
                for act in (ACTS if not d16 else (0, 1)):
                    out.add(Bf16x6("linear_bf16x6_kernel", act, False, d16, xcd, dual, True))
    for act in (0, 1):
        for wtn in (1, 2):
            for a16 in (False, True):
                for d16 in (False, True):
                    for single in (False, True):
                        out.add(Panel("linear_panel_kernel", act, wtn, a16, d16, single))
            for half in (False, True):
                out.add(F16x3("linear_f16x3_kernel", act, wtn, half))
    for act in ACTS:
        for xcd in (False, True):
            for rmax in (False, True):
                for accum in (False, True):
                    out.add(F16x3Tile("linear_f16x3_tile_kernel", act, xcd, rmax, accum, 16))
        out.add(Skinny("linear_skinny_kernel", act))
    return out


UNREACHABLE = {
    "linear_bf16x6_kernel<ACT, DBG != 0, ...>": "the ablation forms exist in builds with -DISG_GEMM_ABLATION only (tools/build_ablation.sh)",
    "linear_bf16x6_kernel<2, 0, A16 or D16, ...>": "ReLU with half rows: linear_launch returns ISG_EUNSUPPORTED (ReLU is the fp32 text encoder's)",
    "linear_bf16x6_kernel<..., A16 = true, ..., ROWB = true>": "isg_linear_bf16x6_rowbias takes fp32 rows only; the template is never instantiated",
    "linear_bf16x6_kernel<..., XCD = false> at N > 128": "only with ISG_GEMM_NO_XCD set; the same instantiations run at N <= 128",
    "linear_panel_kernel<..., DBG != 0>": "the ablation forms exist in builds with -DISG_PANEL_ABLATION only (tools/ablate_panel.py)",
    "linear_panel_kernel<2, ...> / linear_f16x3_kernel<2, ...>": "the row-panel kernels have no ReLU: act > 1 is ISG_EINVAL",
    "linear_panel_kernel<ACT, WTN other than waste()'s, ...>": "only with ISG_PANEL_WTN set",
    "linear_f16x3_tile_kernel<..., MF = 32>": "only with ISG_F16X3_MFMA=32 (24 instantiations); the default is the 16 x 16 x 32 MFMA",
    "linear_f16x3_tile_kernel<ACT != 0 or RMAX, ..., ACCUM> before the last K chunk": "ops._linear_f16x3_tile passes bias, "
        "activation and d_rowmax with the last chunk only (every <ACT, RMAX, ACCUM> exists, on the last chunk)",
    "linear_f16x3_tile_kernel under ISG_F16X3_APLANES": "a timing diagnostic build (tools/time_f16x3_tile.py); its results are garbage by design",
}

# ---- the case lists of tests/test_gpu_linear_forms_fp64.py --------------------------------------------------------------------------
Case = namedtuple("Case", "route M N K act a16 d16 bias rowmax_out")
KS = (36, 128, 132, 256, 260, 644)          # two k-tiles with zero padding | both sides of SINGLE | both sides of DUAL | two K chunks
TILE_M, PANEL_M, WIDE_M = 130, 66, 1026     # two row tiles / panels, the second of 2 rows; nine row tiles
TILE_NS = (100, 132)                        # one column tile, its last subtile ragged (non-XCD, both store forms) | two column tiles,
#                                             the last subtile 4 columns wide (XCD, both store forms)
PANEL_NS = (96, 132)                        # WTN 1 (three whole subtiles) | WTN 2 (NT = 5: four whole subtiles and a 4-column one)
EXTRA_NS = (96, 128, 260, 130)              # whole / ragged one tile, three column tiles, 4 does not divide N (scalar stores everywhere)
PANEL_EXTRA_NS = (128, 260, 130)            # (96 and 132 are PANEL_NS)
SKINNY_MS, SKINNY_NS = (17, 33), (96, 130)
IO = ((False, False), (True, False), (False, True), (True, True))


def _acts(a16, d16):
    return ACTS if not (a16 or d16) else (0, 1)


def cases_bf16x6():
    out = [Case("bf16x6" if not (a16 or d16) else "bf16x6_f16", TILE_M, N, K, act, a16, d16, bias, False)
           for a16, d16 in IO for act in _acts(a16, d16) for K in KS for N in TILE_NS for bias in (True, False)]
    out += [Case("bf16x6", TILE_M, N, 132, 1, False, False, True, False) for N in EXTRA_NS]
    out += [Case("bf16x6_f16", TILE_M, N, 132, 0, True, True, True, False) for N in EXTRA_NS]
    out += [Case("bf16x6", WIDE_M, 260, 260, 2, False, False, True, False), Case("bf16x6_f16", WIDE_M, 260, 260, 1, True, True, True, False),
            Case("bf16x6_f16", WIDE_M, 100, 644, 1, True, False, True, False)]
    return out


def cases_rowbias():
    out = [Case("rowbias", TILE_M, N, K, act, False, d16, True, False)
           for d16 in (False, True) for act in _acts(False, d16) for K in KS for N in TILE_NS]
    out += [Case("rowbias", TILE_M, N, 132, 1, False, False, True, False) for N in EXTRA_NS]
    out += [Case("rowbias", WIDE_M, 260, 260, 2, False, False, True, False), Case("rowbias", WIDE_M, 260, 260, 1, False, True, True, False)]
    return out


def cases_panel():
    out = [Case("panel", PANEL_M, N, K, act, a16, d16, bias, False)
           for a16, d16 in IO for act in (0, 1) for K in KS for N in PANEL_NS for bias in (True, False)]
    out += [Case("panel", PANEL_M, N, 132, 1, a16, d16, True, False) for N in PANEL_EXTRA_NS for a16, d16 in ((False, False), (True, True))]
    return out


def cases_f16x3():
    out = [Case("f16x3_f16" if half else "f16x3", PANEL_M, N, K, act, False, half, bias, False)
           for half in (False, True) for act in (0, 1) for K in (36, 128) for N in PANEL_NS for bias in (True, False)]
    out += [Case("f16x3_f16" if half else "f16x3", PANEL_M, N, 36, 1, False, half, True, False) for N in PANEL_EXTRA_NS for half in (False, True)]
    return out


def cases_f16x3_tile():
    out = [Case("f16x3_tile", TILE_M, N, K, act, False, False, bias, rmax)
           for act in ACTS for rmax in (False, True) for K in KS for N in TILE_NS for bias in (True, False)]
    out += [Case("f16x3_tile", TILE_M, N, 132, 1, False, False, True, True) for N in EXTRA_NS]
    out += [Case("f16x3_tile", WIDE_M, 260, 644, 1, False, False, True, True)]
    return out


def cases_skinny():
    return [Case("skinny", M, N, K, act, False, False, bias, False)
            for M in SKINNY_MS for N in SKINNY_NS for K in KS for act in ACTS for bias in (True, False)]


FAMILIES = {"bf16x6": cases_bf16x6, "rowbias": cases_rowbias, "panel": cases_panel, "f16x3": cases_f16x3,
            "f16x3_tile": cases_f16x3_tile, "skinny": cases_skinny}


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]


def case_form(c, env=None):
    """form() of a case as the Python launchers call the kernels: a dense result (ldd = N) from torch's allocator (16-byte aligned)."""
    return form(c.route, c.M, c.N, c.K, c.act, c.a16, c.d16, c.N, 0, c.rowmax_out, env)


def case_id(c):
    return (f"{c.route}-{c.M}x{c.N}x{c.K}-{ACT_NAMES[c.act]}-{'h' if c.a16 else 'f'}{'h' if c.d16 else 'f'}-"
            f"{'bias' if c.bias else 'nobias'}{'-rowmax' if c.rowmax_out else ''}")


def covered(cases, env=None):
    """instantiation -> the store forms the cases bring to it."""
    out = {}
    for c in cases:
        f = case_form(c, env)
        for inst in instantiations(f):
            out.setdefault(inst, set()).update(f.stores)
    return out


# the multi-output launches (ops.linear_multi: L bias-free Linears of n columns over the same rows; out_cols = n, out_stride = M n):
# (route, M, n, L, K, a16, d16).  n = 96, L = 2: NT = 6, WTN 2 -- the wave that owns subtiles 2 and 3 writes into both outputs;
# n = 32, L = 3: WTN 1, an output per subtile; K = 132 with fp32 rows goes to the panel kernel's chunked form
MULTI_CASES = [(r, PANEL_M, n, L, K, a16, d16)
               for n, L in ((96, 2), (32, 3))
               for r, K, a16, d16 in (("f16x3", 36, False, False), ("f16x3", 128, False, False), ("f16x3_f16", 128, False, True),
                                      ("panel", 132, False, False), ("panel", 128, True, False), ("panel", 260, True, True),
                                      ("panel", 36, False, False))]

# the streaming-store cases (ISG_GEMM_NT_MB=0 in a fresh child): one per instantiation family of the four matrix-core kernels --
# fp32 and half results, vector and scalar store forms -- and the out_cols forms of MULTI_CASES
STREAM_CASES = [
    Case("bf16x6", TILE_M, 132, 260, 1, False, False, True, False),          # XCD, DUAL: vector_nt and scalar subtiles
    Case("bf16x6", TILE_M, 100, 132, 2, False, False, True, False),          # one column tile
    Case("bf16x6", TILE_M, 130, 132, 0, False, False, False, False),         # scalar stores everywhere
    Case("bf16x6_f16", TILE_M, 132, 132, 1, True, True, True, False),        # half result: the flag is set, the store has no streaming form
    Case("bf16x6_f16", WIDE_M, 260, 260, 1, True, False, True, False),
    Case("rowbias", TILE_M, 132, 644, 1, False, False, True, False),
    Case("rowbias", TILE_M, 100, 36, 0, False, True, True, False),
    Case("panel", PANEL_M, 132, 128, 1, False, False, True, False),          # SINGLE, WTN 2: full_nt and guarded_nt
    Case("panel", PANEL_M, 96, 260, 0, True, False, False, False),           # chunked, WTN 1
    Case("panel", PANEL_M, 132, 132, 1, True, True, True, False),            # half result: plain stores
    Case("f16x3", PANEL_M, 132, 128, 1, False, False, True, False),
    Case("f16x3", PANEL_M, 96, 36, 0, False, False, False, False),
    Case("f16x3_f16", PANEL_M, 132, 36, 1, False, True, True, False),        # streams half results too
    Case("f16x3_f16", PANEL_M, 96, 128, 0, False, True, True, False),
    Case("f16x3_tile", TILE_M, 132, 644, 1, False, False, True, True),       # two K chunks: the second reads what the first streamed
    Case("f16x3_tile", TILE_M, 100, 260, 2, False, False, True, False),
    Case("f16x3_tile", TILE_M, 130, 132, 0, False, False, False, True),      # scalar stores everywhere
    Case("f16x3_tile", WIDE_M, 260, 644, 1, False, False, True, True),
]
STREAM_MULTI = [m for m in MULTI_CASES if m[4] in (128, 132)]
