"""The cases of tests/test_gpu_sgenc_fp64.py -- the scene-graph encoder's kernels (csrc/isg_sgenc.hip, csrc/isg_sgenc_bwd.hip,
scatter_mean_kernel in csrc/isg_mp.hip) at the shapes where they branch -- with the kernels' dispatch restated in plain Python and
the float64 / float32 references every case is judged against.  Not a test module: tests/test_sgenc_cases_cpu.py proves without a
GPU that every case reaches the branch it is there for and that the float32 formula alone stays under the cap of the rule, and
tests/test_gpu_sgenc_fp64.py runs the kernels on the very same inputs.  The references are the restatements of
tests/sgenc_bwd_restated.py and autograd._graph_norm_t, gradients by torch autograd of those."""
import torch
import torch.nn.functional as F

import sgenc_bwd_restated as R
from test_gpu_sgenc_train import skewed_csr

FLOOR = 2e-6                 # the project's floor
CAP = 1e-3                   # no comparison may be decided by a bound above this
F_CAP = 8                    # the largest factor the rule may take: the well-posedness of a case is proven for it
EPS = 1e-5

# ---- the dispatch of the kernels, restated -------------------------------------------------------------------------------------
SEG_CHUNK, SEG_PASSES, SEG_U = 256, 5, 4            # csrc/isg_sgenc_bwd.hip
GAB_PARTS_MAX = 1024


def planes_passes(C):
    """The instantiation of gather_add_planes32_kernel isg_gather_add launches: 5, 8, or 0 (the row evaluated twice)."""
    passes = ((C // 4 + 7) // 8 * 8 + 15) // 16
    return 5 if passes <= 5 else (8 if passes <= 8 else 0)


def gab_parts(E):
    return 0 if E <= 0 else min((E + 15) // 16, GAB_PARTS_MAX)


def gab_rows(E):
    """rows_per_block of gather_add_bwd_kernel."""
    return 0 if E <= 0 else (E + gab_parts(E) - 1) // gab_parts(E)


def gab_idle_from(E):
    """The first workgroup of gather_add_bwd_kernel whose row range is empty (== gab_parts(E): none is)."""
    return 0 if E <= 0 else min((E + gab_rows(E) - 1) // gab_rows(E), gab_parts(E))


def gn_block(C):
    return 64 if C <= 64 else (128 if C <= 128 else (256 if C <= 256 else (320 if C <= 320 else (384 if C <= 384 else 512))))


def gn_strided(C):
    """Does a thread of graph_norm_bwd_kernel own more than one channel?"""
    return C > gn_block(C)


def pieces_crossed(rowptr, s, L=SEG_CHUNK):
    """The pieces of L slots segment s has entries in (0: an empty segment; 1: pass 1 stores it; more: the finish kernel adds
    the partial rows of pieces k0 + 1 .. k1 to the one of piece k0)."""
    rb, re = int(rowptr[s]), int(rowptr[s + 1])
    return 0 if re <= rb else (re - 1) // L - rb // L + 1


def finish_trips(rowptr, s, L=SEG_CHUNK):
    """The rows each trip of segment_rows_finish_kernel's SEG_U loop adds for segment s: [4, 1] = a second trip that is not full."""
    n = max(pieces_crossed(rowptr, s, L) - 1, 0)
    return [min(SEG_U, n - i) for i in range(0, n, SEG_U)]


def column_walks(C):
    """Trips of `for (cb = 0; cb < Q; cb += 16 * SEG_PASSES)` in segment_rows_chunk_kernel and gather_add_bwd_kernel."""
    return -(-(C // 4) // (16 * SEG_PASSES))


def scatter_q_trips(C):
    """Trips of the lane-strided q loop of scatter_mean_kernel (64 lanes a node)."""
    return -(-(C // 4) // 64)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def errors(got, ref64, ref32):
    """(e_k, e_32, None) relative to max |ref64|, or (None, None, max |got|) where the reference is identically zero."""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.detach().double(), ref32.detach().double()
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    if scale == 0.0:
        return None, None, (float(got.abs().max()) if got.numel() else 0.0)
    return float((got - ref64).abs().max()) / scale, float((ref32 - ref64).abs().max()) / scale, None


def _gen(*key):
    h = 17
    for k in key:
        for ch in str(k):
            h = (h * 131 + ord(ch)) % 2147483647
    return torch.Generator().manual_seed(h)


# ---- isg_gather_add and isg_gather_add_bwd -------------------------------------------------------------------------------------
GA_C = (4, 28, 32, 36, 300, 320, 324, 512, 516)
GA_E = (1, 16, 17, 257)                # one row, a full workgroup of the planes kernel, one row past it, E * Q across 256 threads
GA_C_EVERY_E = (4, 300, 516)
GA_FORMS = {                           # operand forms: which of B, T, sign, D, bias are given
    "a": (), "ab": ("B",), "at": ("T",), "edge": ("B", "T", "sign", "bias"), "node": ("D", "bias"),
    "all": ("B", "T", "sign", "D", "bias")}
GA_CLASSES = ("plain", "wide", "tail", "cancel", "zero_row")
GA_LAYOUTS = ("contig", "t_slice", "d_slice")       # A and B are ALWAYS column slices of one [N, 3C] tensor


def ga_cases(C):
    """(E, form, gelu, class, layout) of every forward comparison at width C."""
    out = []
    for E in (GA_E if C in GA_C_EVERY_E else (17,)):
        out += [(E, form, gelu, "plain", "contig") for form in GA_FORMS for gelu in (False, True)]
    for gelu in (False, True):
        out += [(17, "all", gelu, "wide", "contig"), (17, "ab", gelu, "cancel", "contig"), (17, "edge", gelu, "cancel", "contig"),
                (17, "all", gelu, "cancel", "contig"), (17, "ab", gelu, "zero_row", "contig")]
    out += [(17, "all", True, "tail", "contig"), (17, "node", True, "tail", "contig"),
            (17, "all", True, "plain", "t_slice"), (17, "all", True, "plain", "d_slice")]
    return out


def ga_inputs(C, E, form, cls, seed=0, N=None, V=7):
    """Float32 CPU tensors of one case.  P [N, 3C] holds A | B | (a third slice); Tw [V, 2C] and Dw [E, 2C] hold T and D in their
    second halves.  wide: node rows x exp(U(0, 6)).  cancel: B[ib[e]] = -A[ia[e]] + 1e-3 N(0, 1) (N = E rows, ia and ib
    permutations).  zero_row: B[ib[0]] = -A[ia[0]] exactly.  tail: D such that the pre-activation lies in [-6, -3] or [3, 6].
    heavy: one token owns 60 % of `it`, one node 60 % of `ia`."""
    gen = _gen("ga", C, E, form, cls, seed)
    N = (E if cls == "cancel" else 13) if N is None else N
    P = torch.randn(N, 3 * C, generator=gen)
    if cls == "wide":
        P = P * torch.exp(6 * torch.rand(N, 1, generator=gen))
    ia, ib = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    it = torch.randint(0, V - 1, (E,), generator=gen)
    it[it == 3] = 4                                                       # token 3 and token V - 1 are unused
    if cls == "heavy":
        it[torch.randperm(E, generator=gen)[:int(0.6 * E)]] = 5
        ia[torch.randperm(E, generator=gen)[:int(0.6 * E)]] = 2
    if cls == "cancel":
        assert N == E
        ia, ib = torch.randperm(N, generator=gen), torch.randperm(N, generator=gen)
        P[ib, C:2 * C] = -P[ia, :C] + 1e-3 * torch.randn(E, C, generator=gen)
    if cls == "zero_row":
        ib[0] = N - 1
        P[N - 1, C:2 * C] = -P[ia[0], :C]
    t = {"P": P, "Tw": torch.randn(V, 2 * C, generator=gen), "Dw": 3 * torch.randn(E, 2 * C, generator=gen),
         "bias": torch.randn(C, generator=gen), "ia": ia, "ib": ib, "it": it,
         "sign": torch.where(torch.rand(E, generator=gen) < 0.4, -1.0, 1.0), "wgt": torch.randn(E, C, generator=gen)}
    if cls == "tail":
        assert "D" in GA_FORMS[form]
        z = (3 + 3 * torch.rand(E, C, generator=gen)) * torch.where(torch.rand(E, C, generator=gen) < 0.5, -1.0, 1.0)
        t["Dw"][:, C:] = 0
        _, (A, i), kw = ga_operands(t, C, form, False, "contig")
        t["Dw"][:, C:] = z - R.gather_add(A, i, **kw)
    return t


def ga_operands(t, C, form, gelu, layout, dtype=torch.float32, device="cpu", grad=False):
    """(leaves, (A, ia), keywords) for R.gather_add / ops.gather_add: the same call on either side."""
    cv = lambda v: v.to(device=device, dtype=dtype).detach().clone().requires_grad_(grad)
    leaves = {k: cv(t[k]) for k in ("P", "Tw", "Dw", "bias")}
    has = GA_FORMS[form]
    T, D = leaves["Tw"][:, C:], leaves["Dw"][:, C:]
    kw = dict(B=leaves["P"][:, C:2 * C] if "B" in has else None, ib=t["ib"].to(device) if "B" in has else None,
              T=(T if layout == "t_slice" else T.contiguous()) if "T" in has else None, it=t["it"].to(device) if "T" in has else None,
              sign=t["sign"].to(device=device, dtype=dtype) if "sign" in has else None,
              D=(D if layout == "d_slice" else D.contiguous()) if "D" in has else None,
              bias=leaves["bias"] if "bias" in has else None, gelu=gelu)
    return leaves, (leaves["P"][:, :C], t["ia"].to(device)), kw


def ga_forward_ref(t, C, form, gelu, layout, dtype):
    _, (A, ia), kw = ga_operands(t, C, form, gelu, layout, dtype)
    return R.gather_add(A, ia, **kw)


GA_GRADS = {"P": "d_AB", "Tw": "d_T", "Dw": "d_D", "bias": "d_bias"}


def ga_backward(fn, t, C, form, gelu, layout="contig", dtype=torch.float64, device="cpu"):
    """(out, {d_AB, d_T, d_D, d_bias} of the leaves in use) of sum(out * wgt) through `fn` (R.gather_add or ops.gather_add)."""
    leaves, (A, ia), kw = ga_operands(t, C, form, gelu, layout, dtype, device, grad=True)
    out = fn(A, ia, **kw)
    (out * t["wgt"].to(device=device, dtype=dtype)).sum().backward()
    used = ("P",) + tuple(k for k, o in (("Tw", "T"), ("Dw", "D"), ("bias", "bias")) if o in GA_FORMS[form])
    return out.detach(), {GA_GRADS[k]: leaves[k].grad for k in used}


def ga_dz_ref(t, C, form, gelu, dtype):
    """(dz, column sums of dz) of the restatement: the gradient of the pre-activation."""
    _, (A, ia), kw = ga_operands(t, C, form, False, "contig", dtype)
    z = R.gather_add(A, ia, **kw).detach().requires_grad_(True)
    ((F.gelu(z) if gelu else z) * t["wgt"].to(dtype)).sum().backward()
    return z.grad, z.grad.sum(0)


GAB_SHAPES = ((16384, 4), (16385, 4), (17409, 4), (775, 324), (775, 644))
GAB_CLASSES = ("plain", "tail", "heavy")
GAB_NODES, GAB_VOCAB = 37, 11


def gab_cases(E, C):
    """(form, gelu, class) at one shape; tail needs D and the GELU: the node form."""
    out = [(form, gelu, "plain") for form in ("edge", "node") for gelu in (False, True)]
    out += [(form, gelu, "heavy") for form in ("edge", "node") for gelu in (False, True)]
    return out + [("node", True, "tail"), ("all", True, "tail")]


def gab_inputs(E, C, form, cls):
    return ga_inputs(C, E, form, cls, seed=1, N=GAB_NODES, V=GAB_VOCAB)


# ---- ops.embedding_sum ---------------------------------------------------------------------------------------------------------
ES_T = (2, 3, 4, 5, 6, 7)
ES_CHAINS = {2: (2,), 3: (3,), 4: (3, 1), 5: (3, 2), 6: (3, 2, 1), 7: (3, 2, 2)}
ES_C = (4, 300, 324)
ES_ROWS, ES_VOCAB = 50, 13


def es_chain(T):
    """Tokens each isg_gather_add launch of ops.embedding_sum adds: three into an empty sum, then two beside the running one."""
    out, t = [], 0
    while t < T:
        take = min(3 if not out else 2, T - t)
        out.append(take)
        t += take
    return tuple(out)


def es_inputs(C, T):
    gen = _gen("es", C, T)
    idx = torch.randint(2, ES_VOCAB - 1, (ES_ROWS, T), generator=gen)              # rows 0 and V - 1 unused, row 1 the pad token
    idx[torch.rand(ES_ROWS, T, generator=gen) < 0.5] = R.PAD
    return {"idx": idx, "weight": torch.randn(ES_VOCAB, C, generator=gen), "wgt": torch.randn(ES_ROWS, C, generator=gen)}


def es_ref(t, dtype):
    w = t["weight"].to(dtype).detach().clone().requires_grad_(True)
    out = F.embedding(t["idx"], w, padding_idx=R.PAD).sum(-2)
    (out * t["wgt"].to(dtype)).sum().backward()
    return out.detach(), w.grad


# ---- isg_segment_rows_sum ------------------------------------------------------------------------------------------------------
SEG_C = (4, 300, 320, 324, 644)
SEG_LAYOUTS = ("skewed", "mid5", "aligned8", "aligned8p1", "single", "multiple")


def seg_layout(name, L=SEG_CHUNK):
    """(rowptr int32, eid int32, M, crossing) -- crossing: the segment `skip` is tried on (the longest one).
    mid5: one segment of 5L + 3 entries that begins mid-piece (k1 - k0 = 5: a second trip of the finish loop with ONE row).
    aligned8: exactly 8L entries from a piece boundary: pieces k0 .. k0 + 7, so the finish loop adds 7 rows, trips of 4 and 3.
    aligned8p1: 8L + 1 entries from a boundary: 8 rows, two FULL trips (aligned8 alone would leave that form out).
    single: M = 1.  multiple: M = 4L exactly, the last piece full."""
    gen = _gen("seg", name, L)
    if name == "skewed":
        return skewed_csr(L, gen)
    counts = {"mid5": [37, 5 * L + 3, 4, 0], "aligned8": [0, L, 8 * L, 3], "aligned8p1": [L // 2, L // 2, 8 * L + 1, 0, 2],
              "single": [0, 1, 0], "multiple": [3, L - 3, 0, L, 2 * L - 5, 5]}[name]
    M = sum(counts)
    rowptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
    perm = torch.randperm(M, generator=gen)
    eid = torch.cat([perm[int(rowptr[s]):int(rowptr[s + 1])].sort().values for s in range(len(counts))])
    return rowptr.to(torch.int32), eid.to(torch.int32), M, max(range(len(counts)), key=lambda s: counts[s])


def seg_inputs(name, C, weighted, gdiv, L=SEG_CHUNK):
    rowptr, eid, M, crossing = seg_layout(name, L)
    gen = _gen("segv", name, C, weighted, gdiv)
    return {"rowptr": rowptr, "eid": eid, "M": M, "crossing": crossing, "G": torch.randn((M + gdiv - 1) // gdiv, C, generator=gen),
            "w": torch.randn(M, generator=gen) if weighted else None}


def seg_ref(t, gdiv, dtype, skip=None):
    return R.segment_rows_sum(t["rowptr"], t["eid"], t["G"], t["w"], gdiv, skip=skip, dtype=dtype)


# ---- isg_scatter_mean / isg_scatter_mean_bwd -----------------------------------------------------------------------------------
SM_C = (4, 256, 260, 516)
SM_N = (1, 5, 23)


def sm_inputs(C, N, L=SEG_CHUNK):
    """2L + 41 edges (E * Q is no multiple of 256 at any of the widths); one node with more than 2L in-edges, nodes with none, the
    last node with none.  N = 1 cannot have both: its only node takes every edge."""
    gen = _gen("sm", C, N)
    if N == 1:
        dst = torch.zeros(2 * L + 41, dtype=torch.int64)
    elif N == 5:
        dst = torch.cat([torch.full((2 * L,), 1), torch.tensor([0, 2])[torch.randint(0, 2, (41,), generator=gen)]])      # 3, 4: none
    else:
        dst = torch.cat([torch.full((2 * L,), 4), torch.randint(0, N - 1, (41,), generator=gen)])
        dst[dst == 9] = 10
    dst = dst[torch.randperm(dst.numel(), generator=gen)]
    E = dst.numel()
    return {"dst": dst, "src": torch.randint(0, N, (E,), generator=gen), "msg": torch.randn(E, C, generator=gen),
            "wgt": torch.randn(N, C, generator=gen), "empty": [i for i in range(N) if int((dst == i).sum()) == 0]}


def sm_ref(t, N, dtype):
    m = t["msg"].to(dtype).detach().clone().requires_grad_(True)
    out = R.scatter_mean(m, t["dst"], N)
    (out * t["wgt"].to(dtype)).sum().backward()
    return out.detach(), m.grad


# ---- isg_graph_norm_bwd --------------------------------------------------------------------------------------------------------
GN_C = (4, 64, 68, 128, 132, 256, 260, 320, 324, 384, 388, 512, 516, 1028)
GN_SIZES = {"mixed": [1, 0, 2, 64, 17, 0], "limit": [1024, 1, 0]}
GN_SHAPES = tuple((C, "mixed") for C in GN_C) + ((8, "limit"), (516, "limit"))
GN_CLASSES = ("plain", "offset", "const", "ms1")
GN_CONST_SIZES = (2, 64)             # const: the graphs of these sizes have identical rows (the others stay random)
# Identical rows leave o = x (1 - mean_scale) the same in every node, so var = o^2 and the sum of d_o over the graph is
# w rstd sum(g) (1 - var / (var + eps)): at eps = 1e-5 under var ~ 0.04 that difference keeps 2.5e-4 of its terms, and d_mean_scale,
# which is -mean times it, came out 2.9e-4 off in the float32 formula ALONE (C = 68; 8 x that is beyond the cap of the rule).  eps is
# an argument of the kernel: the const class passes 0.1, as the layer tail's cases do for the same reason, and one-node graphs --
# identical rows by nature -- are covered at eps = 1e-5 by the plain class, where the larger graphs carry the sums.
# The offset class (x + 100, as asked) takes 0.1 too: in a ONE-node graph o = x - x * mean_scale is a difference of two numbers
# near 100 (3e-6 off in float32) under rstd = 1 / sqrt(o^2 + eps), 316 where mean_scale is near 1 -- with -mean = -100 in front,
# d_mean_scale of the float32 formula ALONE was 4.9e-4 off on the mixed sizes and 1.3e-3 on a one-node graph by itself; at
# eps = 0.1 it is 4e-5 at most.  The offset stays 100.
# ms1 (mean_scale == 1) as well: its one-node graph has o = 0 and var = 0 exactly, d_x = g w rstd - g w rstd = 0 in exact
# arithmetic, and autograd of the float32 formula leaves the rounding of two products of size 316 |g w| there: 2.0e-4 of max |d_x|
# at eps = 1e-5 (C = 388), 100 times less at 0.1.  var == 0 is var == 0 under either eps.
EPS_BIG = 0.1


def gn_eps(cls):
    return EPS if cls == "plain" else EPS_BIG


def gn_inputs(C, sizes_name, cls):
    sizes = GN_SIZES[sizes_name]
    gen = _gen("gn", C, sizes_name, cls)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    N = batch.numel()
    x = torch.randn(N, C, generator=gen) * 2 + 0.5
    if cls == "offset":
        x = x + 100
    if cls == "const":
        first = torch.tensor([0] + sizes[:-1]).cumsum(0)
        for g, n in enumerate(sizes):
            if n in GN_CONST_SIZES:
                x[batch == g] = x[int(first[g])].clone()
    w = torch.rand(C, generator=gen) + 0.5
    w[::7] = -w[::7]
    ms = torch.ones(C) if cls == "ms1" else 1.0 + 0.1 * torch.randn(C, generator=gen)
    return {"sizes": sizes, "batch": batch, "B": len(sizes), "x": x, "weight": w, "bias": torch.randn(C, generator=gen),
            "mean_scale": ms, "wgt": torch.randn(N, C, generator=gen), "eps": gn_eps(cls)}


GN_LEAVES = ("x", "weight", "bias", "mean_scale")


def gn_ref(t, dtype, mode):
    """(out, {d_x, d_weight, d_bias, d_mean_scale}) of autograd._graph_norm_t in `dtype`, intermediates in double when `mode`."""
    from isubgvqa_amd import autograd
    lv = {k: t[k].to(dtype).detach().clone().requires_grad_(True) for k in GN_LEAVES}
    out = autograd._graph_norm_t(lv["x"], lv["weight"], lv["bias"], lv["mean_scale"], t["batch"], t["B"], t["eps"], mode)
    (out * t["wgt"].to(dtype)).sum().backward()
    return out.detach(), {"d_" + k: lv[k].grad for k in GN_LEAVES}
