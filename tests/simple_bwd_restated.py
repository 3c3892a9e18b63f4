"""The backward of the SIMPLE sampler's marginals restated: the explicit two-sweep reverse pass over the (level, count) tables
of the exactly-k circuit, in torch without autograd.  It is the algorithm csrc/isg_simple_bwd.hip implements,
written so that a CPU test can hold it against autograd through sampling/methods/simple.py::log_marginals before any GPU runs.

Not a test module: tests/test_sampler_train_cpu.py and tests/test_gpu_simple_bwd.py import it.
"""
import torch

LARGE_NUMBER = 1.0e10
PAD_ELEMENT, PAD_PARENT = -2000.0, -1000.0


def _log1mexp(x):
    x = -x.abs()
    return torch.where(x > -0.6931471805599453094, torch.log(-torch.expm1(x)), torch.log1p(-torch.exp(x)))


def _elements(cap, l, j):
    return range(max(0, j - cap[l - 1]), min(j, cap[l - 1]) + 1)


def trees(flat, k):
    """(W, M): per level l a [R, n >> l, k + 1] tensor of bottom-up log-weights / top-down log-marginals of flat [R, n]."""
    from isubgvqa_amd.sampling.methods.simple import circuit_tables
    R, n = flat.shape
    L, cap, reach, max_el, max_par = circuit_tables(n, k)
    new = lambda blocks: torch.full((R, blocks, k + 1), float("-inf"), dtype=flat.dtype)
    pad = lambda blocks, v: torch.full((R, blocks), v, dtype=flat.dtype)
    W = [new(n >> l) for l in range(L + 1)]
    W[0][:, :, 0] = _log1mexp(-flat)
    W[0][:, :, 1] = flat
    for l in range(1, L + 1):
        left, right = W[l - 1][:, 0::2], W[l - 1][:, 1::2]
        for j in range(cap[l] + 1):
            if reach[l][j]:
                terms = [left[:, :, jj] + right[:, :, j - jj] for jj in _elements(cap, l, j)]
                W[l][:, :, j] = torch.logsumexp(torch.stack(terms + [pad(n >> l, PAD_ELEMENT)] * (max_el - len(terms)), -1), -1)
    M = [new(n >> l) for l in range(L + 1)]
    M[L][:, 0, k] = 0.0
    for l in range(L - 1, -1, -1):
        left, right = W[l][:, 0::2], W[l][:, 1::2]
        for j in range(cap[l] + 1):
            if not reach[l][j]:
                continue
            terms = []
            for jp in range(j, min(cap[l + 1], j + cap[l]) + 1):
                if reach[l + 1][jp]:
                    as_left = ((left[:, :, j] + right[:, :, jp - j]) - W[l + 1][:, :, jp]) + M[l + 1][:, :, jp]
                    as_right = ((left[:, :, jp - j] + right[:, :, j]) - W[l + 1][:, :, jp]) + M[l + 1][:, :, jp]
                    terms.append(torch.stack((as_left, as_right), -1).reshape(R, n >> l))
            M[l][:, :, j] = torch.logsumexp(torch.stack(terms + [pad(n >> l, PAD_PARENT)] * (max_par - len(terms)), -1), -1)
    return W, M


def marginals_backward(flat, k, g):
    """d flat [R, n] of sum(g * exp(M(0, :, 1))): sweep A reverses the top-down pass, sweep B the bottom-up pass."""
    from isubgvqa_amd.sampling.methods.simple import circuit_tables
    R, n = flat.shape
    L, cap, reach, _, _ = circuit_tables(n, k)
    W, M = trees(flat, k)
    dW = [torch.zeros_like(w) for w in W]
    dM = [torch.zeros_like(w) for w in W]
    dM[0][:, :, 1] = g * M[0][:, :, 1].exp()
    for l in range(L):                                   # sweep A
        Wl, Wr, Ml, Mr, dMl, dMr = W[l][:, 0::2], W[l][:, 1::2], M[l][:, 0::2], M[l][:, 1::2], dM[l][:, 0::2], dM[l][:, 1::2]
        for jp in range(cap[l + 1] + 1):
            if not reach[l + 1][jp]:
                continue
            total = torch.zeros(R, n >> (l + 1), dtype=flat.dtype)
            for jj in _elements(cap, l + 1, jp):
                x = ((Wl[:, :, jj] + Wr[:, :, jp - jj]) - W[l + 1][:, :, jp]) + M[l + 1][:, :, jp]
                E = dMl[:, :, jj] * (x - Ml[:, :, jj]).exp() + dMr[:, :, jp - jj] * (x - Mr[:, :, jp - jj]).exp()
                total = total + E
                dW[l][:, 0::2, jj] += E
                dW[l][:, 1::2, jp - jj] += E
            dM[l + 1][:, :, jp] = total
            dW[l + 1][:, :, jp] = -total
    for l in range(L, 0, -1):                            # sweep B
        Wl, Wr = W[l - 1][:, 0::2], W[l - 1][:, 1::2]
        for j in range(cap[l] + 1):
            if not reach[l][j]:
                continue
            for jj in _elements(cap, l, j):
                c = dW[l][:, :, j] * ((Wl[:, :, jj] + Wr[:, :, j - jj]) - W[l][:, :, j]).exp()
                dW[l - 1][:, 0::2, jj] += c
                dW[l - 1][:, 1::2, j - jj] += c
    return dW[0][:, :, 1]                                # W(0, i, 0) = log1mexp(-w) is detached


def _padded(dense, lens, n):
    """[B, n]: the row's scores, zeros up to nmax (to_dense_batch), -LARGE_NUMBER up to n (simple_scheme.py:86-92); the real slots"""
    B, nmax = dense.shape
    real = torch.arange(nmax)[None, :] < lens[:, None]
    flat = torch.cat([torch.where(real, dense, torch.zeros_like(dense)),
                      torch.full((B, n - nmax), -LARGE_NUMBER, dtype=dense.dtype)], 1)
    return flat, real


def _seed(real, g_out, g_marg, dtype):
    g = torch.zeros(real.shape, dtype=dtype)
    if g_out is not None:
        g = g + torch.where(real, g_out.to(dtype), torch.zeros_like(g))
    if g_marg is not None:
        g = g + g_marg.to(dtype)
    return g


def grad_two_sweeps(dense, lens, k, g_out=None, g_marg=None, dtype=torch.float64):
    """d scores [B, nmax] (zeros at and behind a row's length) by the explicit reverse pass."""
    B, nmax = dense.shape
    n = 1 << max(nmax - 1, 0).bit_length()
    flat, real = _padded(dense.to(dtype), lens, n)
    g = torch.cat([_seed(real, g_out, g_marg, dtype), torch.zeros(B, n - nmax, dtype=dtype)], 1)
    d = marginals_backward(flat, min(k, nmax), g)[:, :nmax]
    return torch.where(real, d, torch.zeros_like(d))


def grad_autograd(dense, lens, k, g_out=None, g_marg=None, dtype=torch.float64):
    """The same gradient by autograd through log_marginals, the restatement the product differentiates when the kernel is off."""
    from isubgvqa_amd.sampling.methods.simple import log_marginals
    B, nmax = dense.shape
    n = 1 << max(nmax - 1, 0).bit_length()
    leaf = dense.to(dtype).clone().requires_grad_(True)
    flat, real = _padded(leaf, lens, n)
    marg = log_marginals(flat, min(k, nmax)).exp()[:, :nmax]
    if not marg.requires_grad:                           # nmax == 1: no level, the marginal is the constant 1
        return torch.zeros_like(dense, dtype=dtype)
    d, = torch.autograd.grad((marg * _seed(real, g_out, g_marg, dtype)).sum(), leaf, allow_unused=True)
    d = torch.zeros_like(leaf) if d is None else d
    return torch.where(real, d, torch.zeros_like(d))
