"""The two functions of include/ext/isg_curves.h restated in plain torch on the CPU, for the tests: the rank by the stated relation
(a double loop's worth of comparisons, no sort), the level rule through torch.ceil(fp32 * fp32), the keep bits, and the sums in
float64 with their derived error bounds beside the values."""
import torch

U = 2.0 ** -24                  # fp32's unit roundoff
LEVELS_MAX, WORDS_MAX = 64, 64


def side_list(sides: int):
    """[removal?] per side of the header's bits, the keep side first."""
    return [False] * (sides & 1) + [True] * ((sides >> 1) & 1)


def graph_range(ptr, g: int, N: int, W: int):
    """(lo, n, over) of graph g: ptr clamped to [0, N] and to non-decreasing, n cut at 32 W nodes."""
    lo = min(max(int(ptr[g]), 0), N)
    hi = max(min(max(int(ptr[g + 1]), 0), N), lo)
    return lo, min(hi - lo, 32 * W), hi - lo > 32 * W


def ranks(a: torch.Tensor) -> torch.Tensor:
    """int64 [n]: rank[i] = #{m : a[m] before a[i]} by the header's relation -- IEEE > with every NaN below -inf, NaNs equal
    among themselves, -0 = +0, ties to the lower index."""
    a = a.float()
    n = a.numel()
    nan = torch.isnan(a)
    v = torch.where(nan, torch.zeros_like(a), a)
    gt = (v.view(-1, 1) > v.view(1, -1)) & ~nan.view(-1, 1) & ~nan.view(1, -1)     # [m, i]: a[m] > a[i], both numbers
    gt |= ~nan.view(-1, 1) & nan.view(1, -1)                                        # any number beats a NaN
    eq = ((v.view(-1, 1) == v.view(1, -1)) & ~nan.view(-1, 1) & ~nan.view(1, -1)) | (nan.view(-1, 1) & nan.view(1, -1))
    m = torch.arange(n)
    return (gt | (eq & (m.view(-1, 1) < m.view(1, -1)))).sum(dim=0)


def level_sizes(n: int, fractions=None, counts=None):
    """t_j per level: counts as they are, or ceil of ONE fp32 product -- torch.ceil(fp32 * fp32), cut at n."""
    if counts is not None:
        return [int(c) for c in counts]
    out = []
    for f in fractions:
        c = torch.ceil(torch.tensor(float(f), dtype=torch.float32) * torch.tensor(float(n), dtype=torch.float32))
        out.append(n if float(c) >= float(n) else int(c))
    return out


def level_sizes_double(n: int, fractions):
    """What a double evaluation of the same rule gives (the fp32 fraction times n in float64): the rule the header does NOT use."""
    import math
    return [int(math.ceil(float(torch.tensor(float(f), dtype=torch.float32).double()) * n)) for f in fractions]


def side_k(n: int, t: int, removal: bool) -> int:
    if n == 0:
        return 0
    return min(n - 1, max(0, t)) if removal else min(n, max(1, t))


def keep_bits(a, ptr, graphs, *, fractions=None, counts=None, sides: int = 3, W: int = 1):
    """(rank int32 [N] (-1 where unwritten), level_k int32 [R, L, S], index int32 [Q], keep int64 [Q, W] of unsigned words,
    status [4], sets: a list of Q lists of local node numbers) of isg_curve_keep_bits."""
    a = torch.as_tensor(a, dtype=torch.float32)
    N, G = a.numel(), len(ptr) - 1
    rm = side_list(sides)
    L, S, R = len(fractions if counts is None else counts), len(rm), len(graphs)
    rank = torch.full((N,), -1, dtype=torch.int32)
    level_k = torch.zeros(R, L, S, dtype=torch.int32)
    index = torch.zeros(R * L * S, dtype=torch.int32)
    keep = torch.zeros(R * L * S, W, dtype=torch.int64)
    sets = []
    over = outside = 0
    for r, g in enumerate(graphs):
        g = int(g)
        lo = n = 0
        rk = torch.zeros(0, dtype=torch.int64)
        if 0 <= g < G:
            lo, n, o = graph_range(ptr, g, N, W)
            over |= int(o)
            rk = ranks(a[lo:lo + n])
            rank[lo:lo + n] = rk.int()
        else:
            outside = 1
        t = level_sizes(n, fractions, counts)
        rk = rk.tolist()
        for j in range(L):
            for s, removal in enumerate(rm):
                k = side_k(n, t[j], removal)
                q = (r * L + j) * S + s
                index[q], level_k[r, j, s] = g, k
                members = [i for i in range(n) if (rk[i] < k) != removal]
                words = [0] * W
                for i in members:
                    words[i >> 5] |= 1 << (i & 31)
                keep[q] = torch.tensor(words, dtype=torch.int64)
                sets.append(members)
    return rank, level_k, index, keep, [over, outside, R * L * S, 0], sets


def as_words(keep_int32: torch.Tensor) -> torch.Tensor:
    """The device's int32 words as unsigned numbers in int64."""
    return keep_int32.cpu().long() & 0xFFFFFFFF


def sums(p_inst, w, R: int, L: int, S: int, totals=None):
    """(auc float64 [R, S] (NaN where skipped), auc_bound [R, S], totals float64 [S, L + 3], totals_bound [S, L + 3]) of
    isg_curve_sums in float64.  auc_bound = L u sum_j |w_j p_j| (an fma chain of L steps, each rounded once: the first-order bound
    of a recursive sum of L exact products, Higham, Accuracy and Stability, 3.1); totals_bound = R 2^-53 sum |x| over the column's
    terms, for the recursive double sums (the auc column sums the device's fp32 areas, so it also carries the sum of their
    bounds when it is held against exact areas)."""
    p = torch.as_tensor(p_inst, dtype=torch.float32).double().view(R, L, S)
    w64 = torch.as_tensor(w, dtype=torch.float32).double().view(1, L, 1)
    fin = torch.isfinite(p).all(dim=1)                                           # [R, S]
    safe = torch.where(fin.unsqueeze(1), p, torch.zeros_like(p))
    auc = (w64 * safe).sum(dim=1)
    auc_bound = L * U * (w64 * safe).abs().sum(dim=1)
    out = torch.zeros(S, L + 3, dtype=torch.float64) if totals is None else totals.clone().double()
    bound = torch.zeros(S, L + 3, dtype=torch.float64)
    for s in range(S):
        out[s, :L] += safe[:, :, s].sum(dim=0)
        bound[s, :L] = R * 2.0 ** -53 * safe[:, :, s].abs().sum(dim=0)
        out[s, L] += auc[:, s].sum()
        bound[s, L] = R * 2.0 ** -53 * auc[:, s].abs().sum() + auc_bound[:, s].sum()
        out[s, L + 1] += float(fin[:, s].sum())
        out[s, L + 2] += float((~fin[:, s]).sum())
    auc = torch.where(fin, auc, torch.full_like(auc, float("nan")))
    return auc, auc_bound, out, bound


def known_answer():
    """The header's: (a, ptr, counts, rank, keep rows, level_k)."""
    return [0.5, 2.0, 2.0], [0, 3], (1, 2), [2, 0, 1], [0b010, 0b101, 0b110, 0b001], [[1, 1], [2, 2]]
