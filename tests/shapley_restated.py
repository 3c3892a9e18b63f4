"""The two functions of include/ext/isg_shapley.h restated in plain torch and numpy on the CPU, for the tests: the keys through
oracle.philox.draw, the positions by the stated relation as an n x n comparison (no sort), the keep rows through explicit bit
packing, the estimator in fp32 torch operations in the stated order (sub, add, multiply by 0.5 and divide are IEEE single on the
CPU) and, separately, in float64 with the sums its error bounds need."""
import numpy as np
import torch

from oracle import philox

U = 2.0 ** -24                  # fp32's unit roundoff
WORDS_MAX, PERMUTATIONS_MAX = 64, 1024
STREAM = 0x80000000             # the top bit of a key's slot word: disjoint from the samplers' (g, slot) draws


def graph_range(ptr, g: int, N: int, W: int):
    """(lo, n, over) of graph g: ptr clamped to [0, N] and to non-decreasing, n cut at 32 W nodes (isg_curve_keep_bits's rule)."""
    lo = min(max(int(ptr[g]), 0), N)
    hi = max(min(max(int(ptr[g + 1]), 0), N), lo)
    return lo, min(hi - lo, 32 * W), hi - lo > 32 * W


def draws(M: int, antithetic: bool) -> int:
    return M // 2 if antithetic else M


def keys(seed: int, g: int, t: int, n: int) -> np.ndarray:
    """uint32 [n]: key_i = Philox::draw(seed, (uint32) g, 0x80000000 | (t << 11) | i)."""
    i = np.arange(n, dtype=np.uint64)
    return np.asarray(philox.draw(seed, np.uint64(g & 0xFFFFFFFF), np.uint64(STREAM | (t << 11)) | i), dtype=np.uint32).reshape(n)


def positions(key: np.ndarray) -> torch.Tensor:
    """int64 [n]: pos[i] = #{j : key_j < key_i, or key_j = key_i and j < i}."""
    k = torch.from_numpy(np.asarray(key, dtype=np.int64))
    j = torch.arange(k.numel())
    before = (k.view(-1, 1) < k.view(1, -1)) | ((k.view(-1, 1) == k.view(1, -1)) & (j.view(-1, 1) < j.view(1, -1)))       # [j, i]
    return before.sum(dim=0)


def graph_positions(seed: int, g: int, n: int, M: int, antithetic: bool) -> torch.Tensor:
    """int64 [M, n]: the M permutations of a graph of n nodes; an odd m under antithetic is the reversal of m - 1."""
    out = torch.zeros(M, n, dtype=torch.int64)
    for m in range(M):
        if antithetic and m & 1:
            out[m] = n - 1 - out[m - 1]
        else:
            out[m] = positions(keys(seed, g, m >> 1 if antithetic else m, n))
    return out


def need_rows(n: int, M: int) -> int:
    return M * max(n - 1, 0)


def row_ptr_of(ptr, graphs, N: int, M: int, W: int):
    """The consistent row_ptr of the listed graphs (an entry outside the batch has no rows)."""
    G = len(ptr) - 1
    out = [0]
    for g in graphs:
        n = graph_range(ptr, int(g), N, W)[1] if 0 <= int(g) < G else 0
        out.append(out[-1] + need_rows(n, M))
    return out


def pack_rows(flags: torch.Tensor, W: int) -> torch.Tensor:
    """bool [rows, n] -> int64 [rows, W] of unsigned words: bit i & 31 of word i >> 5, by explicit shifts."""
    rows, n = flags.shape
    wide = torch.zeros(rows, 32 * W, dtype=torch.int64)
    wide[:, :n] = flags.long()
    return (wide.view(rows, W, 32) << torch.arange(32, dtype=torch.int64)).sum(dim=2)


def keep_bits(ptr, graphs, row_ptr, N: int, M: int, Q: int, antithetic: bool, seed: int, W: int, sentinel: int = -1, want_sets: bool = True):
    """(pos int32 [M, N], index int32 [Q], keep int64 [Q, W] of unsigned words (sentinel where unwritten: every word of an
    unwritten row), status [4], sets: {q: the local nodes of row q} (None unless wanted), written: bool [Q]) of
    isg_shapley_keep_bits."""
    G, R = len(ptr) - 1, len(graphs)
    pos = torch.full((M, N), sentinel, dtype=torch.int32)
    index = torch.full((Q,), sentinel, dtype=torch.int32)
    keep = torch.full((Q, W), sentinel, dtype=torch.int64)
    written = torch.zeros(Q, dtype=torch.bool)
    sets = {}
    over = outside = bad = 0
    for r, g in enumerate(graphs):
        g = int(g)
        listed = 0 <= g < G
        lo = n = 0
        if listed:
            lo, n, o = graph_range(ptr, g, N, W)
            over |= int(o)
        else:
            outside = 1
        need, first = need_rows(n, M), int(row_ptr[r])
        fits = first >= 0 and first + need <= Q
        if not fits or int(row_ptr[r + 1]) != first + need:
            bad = 1
        if not (listed and fits):
            continue
        pm = graph_positions(seed, g, n, M, antithetic)
        pos[:, lo:lo + n] = pm.int()
        if n < 2:
            continue
        ks = torch.arange(1, n).view(-1, 1)
        for m in range(M):
            q0 = first + m * (n - 1)
            flags = pm[m].view(1, n) < ks                                      # [k - 1, i]: pos_m[i] < k
            index[q0:q0 + n - 1] = g
            keep[q0:q0 + n - 1] = pack_rows(flags, W)
            written[q0:q0 + n - 1] = True
            if want_sets:
                for k in range(1, n):
                    sets[q0 + k - 1] = torch.nonzero(flags[k - 1]).view(-1).tolist()
    return pos, index, keep, [over, outside, bad, Q], (sets if want_sets else None), written


def as_words(keep_int32: torch.Tensor) -> torch.Tensor:
    """The device's int32 words as unsigned numbers in int64."""
    return keep_int32.cpu().long() & 0xFFFFFFFF


def _marginals(p_inst, pg, v_empty, pos_m, first: int, m: int, n: int):
    """(v_hi, v_lo) [n] of draw m: every pos clamped to [0, n - 1] before it forms a row number."""
    ps = pos_m.long().clamp(0, n - 1)
    base = first + m * (n - 1)
    if n > 1:
        hi = torch.where(ps + 1 >= n, pg.expand(n), p_inst[(base + ps).clamp(max=base + n - 2)])
        lo = torch.where(ps == 0, v_empty.expand(n), p_inst[(base + ps - 1).clamp(min=base)])
    else:
        hi, lo = pg.expand(n), v_empty.expand(n)
    return hi, lo


def butterfly_sum(phi: torch.Tensor) -> torch.Tensor:
    """The header's order in fp32: lane l sums its nodes l, l + 64, ... ascending from +0, then xor butterflies at 32 .. 1."""
    n = phi.numel()
    lanes = torch.zeros(64, dtype=torch.float32)
    for i0 in range(0, n, 64):
        part = torch.zeros(64, dtype=torch.float32)
        part[:min(64, n - i0)] = phi[i0:i0 + 64]
        lanes = torch.where(torch.arange(64) < n - i0, lanes + part, lanes)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[lane ^ off]
    return lanes[0]


def values(p_inst, p, pos, ptr, graphs, row_ptr, N: int, M: int, Q: int, antithetic: bool, v_empty: float, W: int, dtype=torch.float32,
           sentinel: float = -7.0):
    """(phi [N], m2 [N], gap [R], flag [R], abs_e [N]: sum_t |e_t|, sq_e [N]: sum_t e_t^2) of isg_shapley_values in `dtype`:
    torch.float32 is the header's arithmetic order operation for operation (m2 by a product and a sum: it is not held exactly);
    torch.float64 is the same estimator in double.  Unwritten words hold the sentinel."""
    G, R = len(ptr) - 1, len(graphs)
    p_inst = torch.as_tensor(p_inst, dtype=torch.float32).to(dtype)
    p = torch.as_tensor(p, dtype=torch.float32).to(dtype)
    pos = torch.as_tensor(pos).view(M, N)
    ve = torch.tensor(float(np.float32(v_empty)), dtype=dtype)
    T = draws(M, antithetic)
    phi = torch.full((N,), sentinel, dtype=dtype)
    m2, abs_e, sq_e = phi.clone(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    gap = torch.full((R,), float("nan"), dtype=dtype)
    flag = torch.zeros(R, dtype=torch.int32)
    half = torch.tensor(0.5, dtype=dtype)
    for r, g in enumerate(graphs):
        g = int(g)
        if not 0 <= g < G:
            flag[r] = 2
            continue
        lo, n, _ = graph_range(ptr, g, N, W)
        need, first = need_rows(n, M), int(row_ptr[r])
        if first < 0 or first + need > Q:
            flag[r] = 2
            continue
        if n == 0:
            gap[r] = 0.0
            continue
        pg = p[g]
        if not (bool(torch.isfinite(pg)) and bool(torch.isfinite(p_inst[first:first + need]).all())):
            flag[r] = 1
            phi[lo:lo + n] = float("nan")
            m2[lo:lo + n] = float("nan")
            continue
        acc, sq = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
        for t in range(T):
            if antithetic:
                h0, l0 = _marginals(p_inst, pg, ve, pos[2 * t, lo:lo + n], first, 2 * t, n)
                h1, l1 = _marginals(p_inst, pg, ve, pos[2 * t + 1, lo:lo + n], first, 2 * t + 1, n)
                e = half * ((h0 - l0) + (h1 - l1))
            else:
                h0, l0 = _marginals(p_inst, pg, ve, pos[t, lo:lo + n], first, t, n)
                e = h0 - l0
            acc = acc + e
            sq = sq + e * e
            abs_e[lo:lo + n] += e.double().abs()
            sq_e[lo:lo + n] += e.double() ** 2
        phi[lo:lo + n] = acc / torch.tensor(float(T), dtype=dtype)
        m2[lo:lo + n] = sq
        total = butterfly_sum(phi[lo:lo + n]) if dtype == torch.float32 else phi[lo:lo + n].sum()
        gap[r] = total - (pg - ve)
    return phi, m2, gap, flag, abs_e, sq_e


def known_answer():
    """The header's: one graph of 3 nodes, g = 0, seed, M = 2, antithetic, W = 1 -> (seed, keys, pos rows, keep rows, p_inst, p,
    phi)."""
    return ((1 << 32) + 7, [0xB8A65C43, 0x29FF42B2, 0x3C12D07E], [[2, 0, 1], [0, 2, 1]], [0b010, 0b110, 0b001, 0b101],
            [0.25, 0.5, 0.125, 0.75], 1.0, [0.3125, 0.25, 0.4375])
