"""The forward of the SIMPLE sampler restated in torch on the CPU, in a dtype of the caller's choice: the marginals of the exactly-k
circuit (the two tree passes of tests/simple_bwd_restated.py::trees, i.e. oracle/simple.py::log_marginals written level by level),
the Gumbel keys flat + (-log(-log(u))), the selected set under the kernel's tie rule (equal keys go to the lower slot,
csrc/isg_simple.hip) and the straight-through value (hot - marg) + marg.  With torch.float64 it is the yardstick of
tests/test_gpu_simple_fwd.py; with torch.float32 it is oracle/simple.py::simple_forward again (tests/test_simple_fwd_cpu.py holds
the two together) and measures e32, the error a float32 evaluation of the same formulas has on the same input.

The file also holds what the GPU test and the host test share: the host rule of isg_simple_topk restated (row bytes, rows per
workgroup, LDS regime, refusal), the table of shapes, their inputs and their references, each computed once.

Not a test module: tests/test_simple_fwd_cpu.py and tests/test_gpu_simple_fwd.py import it.  Nothing of the package is imported
except the circuit tables simple_bwd_restated.trees already reads.
"""
import functools

import torch

import simple_bwd_restated as R

MAXK, MAXN = 16, 1024                 # SM_MAXK, 1 << SM_MAXL of csrc/isg_simple.hpp
ROW_LIMIT = 150 * 1024                # bytes of one row's two trees beyond which isg_simple_topk refuses
BLOCK_LDS = 48 * 1024                 # rows per workgroup = min(4, BLOCK_LDS // row_bytes), at least 1
OPT_IN = 64 * 1024                    # dynamic LDS beyond which the launch needs hipFuncSetAttribute
FLOOR, F = 5e-6, 4                    # the rule of tests/test_gpu_simple_bwd.py: err <= F * e32 + FLOOR
E32_MAX = 2.5e-4                      # the float32 restatement's own error stays below this on every input used
MIN_GAP = 1e-3                        # float64 gap between the k-th and the (k+1)-th key of every row


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def n_of(nmax):
    """Variables of the circuit: nmax rounded up to a power of two (simple_scheme.py:88)."""
    return 1 << max(nmax - 1, 0).bit_length()


def marginals(dense, lens, k, dtype):
    """[B, nmax] marginals of rows dense[b, :lens[b]] padded with zeros to nmax and -1e10 to n, evaluated in `dtype`."""
    B, nmax = dense.shape
    flat, _ = R._padded(dense.to(dtype), lens, n_of(nmax))
    _, M = R.trees(flat, min(k, nmax))
    return M[0][:, :nmax, 1].exp()


def keys(dense, lens, uniform, dtype):
    """[B, n] Gumbel keys of the padded rows: flat + (-log(-log(u))) (simple.py:99-104), evaluated in `dtype`."""
    flat, _ = R._padded(dense.to(dtype), lens, n_of(dense.size(1)))
    return flat + (-torch.log(-torch.log(uniform.to(dtype))))


def select(key, kk):
    """bool [B, n]: the kk largest keys of every row, equal keys to the lower slot (a stable descending sort keeps the lower slot
    of a tie in front) -- the kernel's kk rounds of 'largest unpicked key, lowest slot among equals'."""
    order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :kk]
    return torch.zeros(key.shape, dtype=torch.bool).scatter_(1, order, True)


def key_gap(key, kk):
    """[B]: k-th largest key minus the (k+1)-th of every row; inf where all n slots are taken."""
    s = torch.sort(key.double(), dim=1, descending=True).values
    if kk >= key.size(1):
        return torch.full((key.size(0),), float("inf"), dtype=torch.float64)
    return s[:, kk - 1] - s[:, kk]


def forward(dense, lens, k, uniform, dtype):
    """(out [B, nmax] = (hot - marg) + marg, marginals [B, nmax], hot bool [B, n], keys [B, n]) in `dtype`; `out` is meant on the
    real slots (column < lens[b])."""
    nmax = dense.size(1)
    marg = marginals(dense, lens, k, dtype)
    key = keys(dense, lens, uniform, dtype)
    hot = select(key, min(k, nmax))
    return (hot[:, :nmax].to(dtype) - marg) + marg, marg, hot, key


# ---- the host rule of isg_simple_topk, restated -----------------------------------------------------------------------------------
def row_bytes(k, nmax):
    return 2 * (2 * n_of(nmax) - 1) * (min(k, nmax) + 1) * 4


def refused(k, nmax):
    return nmax > MAXN or min(k, nmax) > MAXK or row_bytes(k, nmax) > ROW_LIMIT


def rows_per_block(k, nmax):
    return max(1, min(4, BLOCK_LDS // row_bytes(k, nmax)))


def regime(k, nmax):
    """'48K' (the workgroup's rows fit the default), '64K' (one row above 48 KB, no opt-in), 'opt-in' (hipFuncSetAttribute), 'refused'"""
    if refused(k, nmax):
        return "refused"
    lds = rows_per_block(k, nmax) * row_bytes(k, nmax)
    return "48K" if lds <= BLOCK_LDS else "64K" if lds <= OPT_IN else "opt-in"


def largest_k(nmax):
    """The largest k <= 16 the 150 KB rule admits on rows of nmax slots."""
    return max(k for k in range(1, MAXK + 1) if not refused(k, nmax))


# ---- the shapes of tests/test_gpu_simple_fwd.py ---------------------------------------------------------------------------------
# name -> (nmax, k, row lengths, input kind, class).  Kinds: "gelu" = gelu(randn), the node gate's scores (negative ones lose to the
# 0.0 pads); "randn"; "ln2" / "30" = gelu(randn) with the named values written over the head of row 0.
LEVELS = (1, 2, 3, 4, 8, 9, 16, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
LN2_VALUES = (0.6931, -0.6931, 0.6932, -0.6932, 0.6931471805599453, -0.6931471805599453)    # around log1mexp's branch point
BIG_VALUES = (30.0, -30.0)                                                                # expm1f / log1pf saturate


def _sweep_lens(nmax, k):
    """one full row, one short row (k + 1 slots) and a one-slot row"""
    return [nmax, min(min(k, nmax) + 1, nmax), 1]


def _make_cases():
    cases = {}
    for nmax in LEVELS:
        for k in sorted({1, 2, 5, largest_k(nmax)}):
            cases[f"sweep n{nmax} k{k}"] = (nmax, k, _sweep_lens(nmax, k), "gelu", "table sweep")
    for nmax in (32, 40):
        for k in range(1, 17):
            cases.setdefault(f"sweep n{nmax} k{k}", (nmax, k, _sweep_lens(nmax, k), "gelu", "table sweep"))
    for k in (5, 6, 8, 16):                                # 4, 3, 2, 1 rows per workgroup; B = 5 and 7 leave the last one partial
        cases[f"rows n128 k{k} B5"] = (128, k, [128, k + 1, 1, 77, 128], "gelu", "rows per block")
        cases[f"rows n128 k{k} B7"] = (128, k, [100, 128, 1, k + 1, 128, 64, 9], "randn", "rows per block")
    cases["lds n257 k5"] = (257, 5, [257, 6, 130], "gelu", "LDS regimes")            # 49 104 B: 48 B BELOW 48 KB = 49 152, one row
    cases["lds n257 k6"] = (257, 6, [257, 7, 130], "gelu", "LDS regimes")            # 57 288 B: between 48 and 64 KB, no opt-in
    cases["lds n200 k15"] = (200, 15, [200, 16, 1], "randn", "LDS regimes")          # 65 408 B: the largest launch without opt-in
    cases["lds n130 k16"] = (130, 16, [130, 17, 1, 64], "randn", "LDS regimes")      # 69 496 B
    cases["lds n1024 k8"] = (1024, 8, [1024, 9, 600], "gelu", "LDS regimes")         # 147 384 B
    cases["lds n700 k7"] = (700, 7, [700, 8, 1, 333], "randn", "LDS regimes")
    cases["arm k>=nmax n4"] = (4, 5, [4, 4, 4], "randn", "arms")
    cases["arm k>=nmax n2"] = (2, 5, [2, 2, 2], "randn", "arms")
    cases["arm nmax=1"] = (1, 5, [1, 1, 1, 1, 1], "randn", "arms")
    cases["arm empty graph"] = (7, 3, [7, 0, 5, 4, 7], "gelu", "arms")
    cases["arm zero pads > k"] = (6, 2, [1, 2, 6], "gelu", "arms")
    cases["arm k=1 NaN rows"] = (129, 1, [129, 1, 60], "gelu", "arms")
    cases["arm ln2"] = (16, 5, [16, 9, 16], "ln2", "arms")
    cases["arm 30"] = (16, 5, [16, 9, 16], "30", "arms")
    return cases


CASES = _make_cases()
REFUSED = {"nmax=1025": (1025, 5), "min(k, nmax)=17": (32, 17), "(1024, 9)": (1024, 9)}
HINT_LENS, HINTS, HINT_K = [40, 7, 33], (64, 100), 5       # a max_nodes hint with the same n (more zero pads) and with a larger n

# Seeds of inputs(): per shape the first of 0, 1, 2, ... under which the reference ALONE says the input is well conditioned -- float32
# and float64 restatement agree on the NaN pattern and on every row's selected set, every row's float64 key gap at the k-th place
# exceeds MIN_GAP and e32 < E32_MAX.  tests/test_simple_fwd_cpu.py asserts all of it for every shape, no row left out.
# Seed 0 wherever the shape is not named; the five named ones had a key gap below MIN_GAP in some row under the earlier seeds.
SEED = {"sweep n32 k5": 1, "sweep n512 k16": 1, "sweep n32 k11": 1, "rows n128 k16 B7": 3, "lds n257 k6": 1}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(dense [B, nmax] float32 with zeros behind a row's length, lens int64 [B], k, uniform [B, n] float32, real bool [B, nmax])"""
    if name in CASES:
        nmax, k, lens, kind, _ = CASES[name]
    else:
        nmax, k, lens, kind = max(HINT_LENS), HINT_K, HINT_LENS, "gelu"
    gen = torch.Generator().manual_seed(1000 * nmax + k + 1000003 * SEED.get(name, 0))
    B, lens = len(lens), torch.tensor(lens)
    dense = torch.randn(B, nmax, generator=gen)
    if kind != "randn":
        dense = torch.nn.functional.gelu(dense)
    values = {"ln2": LN2_VALUES, "30": BIG_VALUES}.get(kind)
    if values is not None:
        dense[0, :len(values)] = torch.tensor(values)
    uniform = torch.rand(B, n_of(nmax), generator=gen)
    real = torch.arange(nmax)[None, :] < lens[:, None]
    return dense * real, lens, k, uniform, real


TIE_K, TIE_N = 3, 128
TIE_PAIRS = ((10, 11), (10, 74), (11, 74))      # neighbouring lanes; one lane's two slots (i, i + 64); the lower slot in the higher lane
TIE_WINNERS = (3, 7)


def tie_rows():
    """(dense [3, 128], uniform [3, 128], expected selected slots per row) for k = 3: slots 3 and 7 win the first two places, and
    the third is a tie of two slots with the same (score, u), hence the same key bit for bit; every other slot lies far below.  The
    documented rule gives the place to the lower slot of the pair."""
    dense = (-3.0 - 0.01 * torch.arange(TIE_N, dtype=torch.float32)).repeat(len(TIE_PAIRS), 1)
    uniform = torch.full((len(TIE_PAIRS), TIE_N), 0.5)
    dense[:, TIE_WINNERS[0]], dense[:, TIE_WINNERS[1]] = 4.0, 3.0
    for row, pair in enumerate(TIE_PAIRS):
        dense[row, list(pair)] = 2.0
        uniform[row, list(pair)] = 0.25
    return dense, uniform, [sorted(TIE_WINNERS + (min(pair),)) for pair in TIE_PAIRS]


@functools.lru_cache(maxsize=None)
def reference(name):
    """{'marg64', 'marg32', 'hot64', 'hot32', 'out64', 'gap', 'e32', 'nan64', 'nan32'} of a shape, computed once and left unchanged"""
    dense, lens, k, uniform, real = inputs(name)
    out64, marg64, hot64, key64 = forward(dense, lens, k, uniform, torch.float64)
    _, marg32, hot32, _ = forward(dense, lens, k, uniform, torch.float32)
    nan64, nan32 = torch.isnan(marg64), torch.isnan(marg32)
    diff = (marg32.double() - marg64).abs()[~(nan64 | nan32)]
    return {"marg64": marg64, "marg32": marg32, "hot64": hot64, "hot32": hot32, "out64": out64, "nan64": nan64, "nan32": nan32,
            "gap": key_gap(key64, min(k, dense.size(1))), "e32": diff.max().item() if diff.numel() else 0.0}


def well_conditioned(name):
    """The conditions a seed is chosen by, as a list of the ones that fail (empty: the input is fit for the comparison)."""
    r = reference(name)
    bad = []
    if not torch.equal(r["nan64"], r["nan32"]):
        bad.append("float32 and float64 disagree on the NaN pattern")
    if not torch.equal(r["hot64"], r["hot32"]):
        bad.append("float32 and float64 select different sets")
    if not bool((r["gap"] > MIN_GAP).all()):
        bad.append(f"key gap {r['gap'].min().item():.3e} <= {MIN_GAP}")
    if not r["e32"] < E32_MAX:
        bad.append(f"e32 {r['e32']:.3e} >= {E32_MAX}")
    return bad
