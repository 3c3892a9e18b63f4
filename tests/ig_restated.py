"""The two functions of include/ext/isg_ig.h restated as float64 loops on the host, with the header's skip rules, for the tests of
integrated gradients (tests/test_ig_cpu.py, tests/test_gpu_ig.py, tests/test_gpu_ig_models.py).  Plain Python over small inputs;
nothing here is fast, and nothing here rounds to fp32: the tests hold the device to bounds derived from fp32's roundings."""
import torch


def _base_row(base, r):
    """Row r of a baseline: None -> None (zeros), [C] -> that row for every r, [rows, C] -> its row r."""
    if base is None:
        return None
    return base if base.dim() == 1 else base[r]


def path_rows(x, base, src, inst_of, t, out=None, interpolate=True):
    """float64 [n_out, C]: row i = t[q] x[r] + (1 - t[q]) base[r], r = src[i], q = inst_of[i]; rows whose r lies outside
    [0, rows) or (when interpolating) whose q lies outside [0, Q) keep what `out` holds (NaN when none is given).
    interpolate=False: the plain copy x[r]."""
    n, C = len(src), x.size(1)
    res = torch.full((n, C), float("nan"), dtype=torch.float64) if out is None else out.double().clone()
    for i in range(n):
        r = int(src[i])
        if not 0 <= r < x.size(0):
            continue
        if not interpolate:
            res[i] = x[r].double()
            continue
        q = int(inst_of[i])
        if not 0 <= q < t.numel():
            continue
        tq = float(t[q])
        b = _base_row(base, r)
        res[i] = tq * x[r].double() if b is None else tq * x[r].double() + (1.0 - tq) * b.double()
    return res


def path_rows_bound(x, base, src, inst_of, t):
    """float64 [n_out, C]: |t x| + |(1 - t) b| of every output entry (0 on skipped rows) -- what the header's three roundings
    are relative to."""
    n, C = len(src), x.size(1)
    res = torch.zeros(n, C, dtype=torch.float64)
    for i in range(n):
        r, q = int(src[i]), int(inst_of[i])
        if 0 <= r < x.size(0) and 0 <= q < t.numel():
            tq = float(t[q])
            b = _base_row(base, r)
            res[i] = (tq * x[r].double()).abs() + (0 if b is None else ((1.0 - tq) * b.double()).abs())
    return res


def copies(r, rng, iptr, gptr, glist, Q, rows_in):
    """The (instance, row of the instance batch) pairs of parent row r that pass the header's rules, in the order of glist; the
    graph is the first whose range ends behind r (graphs without rows are passed over), as the kernel's binary search finds it."""
    G = len(rng) - 1
    g = next((k for k in range(G) if int(rng[k + 1]) > r), G - 1)
    if G < 1 or not int(rng[g]) <= r < int(rng[g + 1]) or rows_in <= 0:
        return []
    j0 = max(0, min(int(gptr[g]), Q))
    j1 = max(j0, min(int(gptr[g + 1]), Q))
    out = []
    for j in range(j0, j1):
        q = int(glist[j])
        if not 0 <= q < Q:
            continue
        b, e = int(iptr[q]), int(iptr[q + 1])
        row = b + (r - int(rng[g]))
        if b >= 0 and row < e and row < rows_in:
            out.append((q, row))
    return out


def attribution(g_rows, w, x, base, rng, iptr, gptr, glist, attr_in=None, avg_in=None):
    """(attr float64 [rows], avg float64 [rows, C], bound float64 [rows], avg_bound float64 [rows, C], most copies of a row):
    avg[n] = sum_j w[q_j] g[copy_j], attr[n] = sum_c (x - base)[n, c] avg[n, c]; with attr_in / avg_in the result is added onto
    them (accumulate), and a row without a valid copy keeps them.  bound[n] = sum_c |x - b| * sum_j |w g| and avg_bound = sum_j |w g|:
    the magnitudes the header's roundings are relative to."""
    rows, C, Q = x.size(0), x.size(1), w.numel()
    attr = torch.zeros(rows, dtype=torch.float64) if attr_in is None else attr_in.double().clone()
    avg = torch.zeros(rows, C, dtype=torch.float64) if avg_in is None else avg_in.double().clone()
    bound, avg_bound, most = torch.zeros(rows, dtype=torch.float64), torch.zeros(rows, C, dtype=torch.float64), 0
    for n in range(rows):
        cs = copies(n, rng, iptr, gptr, glist, Q, g_rows.size(0))
        if not cs:
            continue
        most = max(most, len(cs))
        G = torch.zeros(C, dtype=torch.float64)
        A = torch.zeros(C, dtype=torch.float64)
        for q, row in cs:
            G += float(w[q]) * g_rows[row].double()
            A += (float(w[q]) * g_rows[row].double()).abs()
        b = _base_row(base, n)
        d = x[n].double() if b is None else x[n].double() - b.double()
        attr[n] += float((d * G).sum())
        avg[n] += G
        bound[n] = float((d.abs() * A).sum())
        avg_bound[n] = A
    return attr, avg, bound, avg_bound, most


def by_graph(index, G):
    """(gptr [G + 1], glist [Q]): the instances of every graph in ascending q; an index outside [0, G) belongs to no graph."""
    lists = [[] for _ in range(G)]
    for q, g in enumerate(index):
        if 0 <= int(g) < G:
            lists[int(g)].append(q)
    gptr, glist = [0], []
    for l in lists:
        glist += l
        gptr.append(len(glist))
    glist += [q for q, g in enumerate(index) if not 0 <= int(g) < G]
    return gptr, glist


def known_answer():
    """The header's known answer: (x, base, t, w, path rows, gradient rows, G, attribution)."""
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0], [-1.0, 0.0, 1.0, 2.0]])
    base = torch.tensor([1.0, 0.0, 1.0, 0.0])
    t, w = torch.tensor([0.25, 0.75]), torch.tensor([0.5, 0.5])
    rows = [[1.0, 0.5, 1.5, 1.0], [0.5, 0.0, 1.0, 0.5], [1.0, 1.5, 2.5, 3.0], [-0.5, 0.0, 1.0, 1.5]]
    g = torch.tensor([[1.0, 1.0, 1.0, 1.0], [2.0, 0.0, -2.0, 4.0], [3.0, -1.0, 1.0, 0.5], [0.0, 2.0, 2.0, -4.0]])
    return x, base, t, w, rows, g, [[2.0, 0.0, 1.0, 0.75], [1.0, 1.0, 0.0, 0.0]], [5.0, -2.0]
