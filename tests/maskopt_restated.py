"""isg_maskopt_step (include/ext/isg_maskopt.h) restated in float64 on the host, with the header's skip rules, for the tests of mask
optimisation (tests/test_maskopt_cpu.py, tests/test_gpu_maskopt.py, tests/test_gpu_maskopt_models.py).  Nothing here rounds to
fp32 but the host scalars, which the header rounds once (A, E, w1, b2, w2, step_size, r2, e): every function returns, beside its
float64 values, the bound that fp32's roundings allow the device.

THE BOUNDS (u = 2^-24; TINY = 2^-120 pays for an operation whose result leaves fp32's normal range; 1.01 for second-order terms).
d theta.  s: every term g_c x_c is rounded once as a product and passes through at most 3 + ceil(C / 64) + 4 additions, fewer than
    C + 8 roundings in all: |ds| <= 1.01 (C + 8) u sum_c |g_c x_c|.
    m = 1 / (1 + expf(-t)): expf's documented 1 ulp is 2 u of e = exp(-t), which is 2 u e / (1 + e) <= 2 u of the sum; the sum and
    the division round once each: |dm| <= 4.04 u m + TINY.     1 - m: |d(1 - m)| <= u (1 - m) + |dm|.
    p = m (1 - m): |dp| <= |dm| (1 - m) + m |d(1 - m)| + u p.
    reg = (A - E t) / n: three roundings, each relative to no more than (|A| + |E t|) / n.
    d = (s + reg) p: |dd| <= 1.01 (|s + reg| |dp| + p (|ds| + |dreg| + u |s + reg|) + u |d|) + TINY.
Adam, FROM THE DEVICE'S OWN d (fp32 values, so exact inputs): exp_avg is three roundings, |dm1| <= 1.01 u (2 |(d - m0) w1| + |m1|) +
    TINY; exp_avg_sq is a sum of non-negative terms, three roundings on one and two on the other: |dv1| <= 4.04 u v1 + TINY;
    |sqrt(a) - sqrt(b)| <= min(|a - b| / (2 sqrt(b)), sqrt(|a - b|)) and sqrt rounds once; / r2 and + e round once each:
    |ddenom| <= 1.01 ((dsqrt + u sqrt(v1)) / r2 + u sqrt(v1) / r2 + u denom); q = m1 / denom: |dq| <= 1.01 (|dm1| + |q| |ddenom|) /
    denom + u |q|; theta1 = theta0 - step_size q: |dtheta1| <= 1.01 (step_size (|dq| + u |q|) + u |theta1|).
Masked rows, FROM THE DEVICE'S OWN theta1: |dx_out| <= 1.01 (4.04 u + u) |m x| + TINY |x|."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -120
PYG = dict(a_size=1.0, a_ent=0.1, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)


def f32(v: float) -> float:
    """The fp32 value nearest to the double v, as a double: the header's `(float)`."""
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def scalars(a_size=1.0, a_ent=0.1, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """The header's A, E, w1, b2, w2, step_size, r2, e of a call: double arithmetic, ONE rounding each."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return dict(A=f32(a_size), E=f32(a_ent), w1=f32(1.0 - beta1), b2=f32(beta2), w2=f32(1.0 - beta2), step_size=f32(lr / bc1),
                r2=f32(math.sqrt(bc2)), e=f32(eps), bc1=bc1, bc2=bc2)


def segment_of(seg, N):
    """(j int64 [N], n_j int64 [N]): the segment the kernel's binary search finds for every row -- the first whose range ends behind
    the row, segments without rows passed over -- or -1 where no segment holds the row."""
    seg = [int(v) for v in seg]
    B = len(seg) - 1
    j_of, n_of = torch.full((N,), -1, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    for n in range(N):
        lo, hi = 0, B - 1
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            if seg[mid + 1] > n:
                hi = mid
            else:
                lo = mid + 1
        if B >= 1 and seg[lo] <= n < seg[lo + 1]:
            j_of[n], n_of[n] = lo, seg[lo + 1] - seg[lo]
    return j_of, n_of


def sigmoid(t):
    """float64 1 / (1 + exp(-t)); exp's overflow gives +0, as the header says."""
    return 1.0 / (1.0 + torch.exp(-t.double()))


def d_theta(x, g, seg, theta, a_size=1.0, a_ent=0.1):
    """(d float64 [N], bound float64 [N], inside bool [N]): the header's d[n] and what fp32 allows the device around it; rows
    outside every segment hold NaN and a bound of 0."""
    N, C = x.shape
    k = scalars(a_size=a_size, a_ent=a_ent)
    j_of, n_of = segment_of(seg, N)
    inside = j_of >= 0
    t, n = theta.double(), n_of.clamp_min(1).double()
    terms = g.double() * x.double()
    s, s_abs = terms.sum(1), terms.abs().sum(1)
    m = sigmoid(t)
    reg = (k["A"] - k["E"] * t) / n
    p = m * (1.0 - m)
    d = (s + reg) * p
    ds = 1.01 * (C + 8) * U * s_abs
    dm = 4.04 * U * m + TINY
    d1m = U * (1.0 - m) + dm
    dp = dm * (1.0 - m) + m * d1m + U * p
    dreg = 1.01 * 3 * U * (abs(k["A"]) + (k["E"] * t).abs()) / n
    bound = 1.01 * ((s + reg).abs() * dp + p * (ds + dreg + U * (s + reg).abs()) + U * d.abs()) + TINY
    nan = torch.full_like(d, float("nan"))
    return torch.where(inside, d, nan), torch.where(inside, bound, torch.zeros_like(bound)), inside


def adam(d, theta, exp_avg, exp_avg_sq, *, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """((theta1, m1, v1), (their bounds), applied bool [N]) of the header's Adam lines in float64 on the given d (the device's own
    values, or a float64 d): a row whose d is not finite keeps its three values, with bounds of 0."""
    k = scalars(lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step)
    d, t0, m0, v0 = d.double(), theta.double(), exp_avg.double(), exp_avg_sq.double()
    ok = torch.isfinite(d)
    dz = torch.where(ok, d, torch.zeros_like(d))
    lerp = (dz - m0) * k["w1"]
    m1 = m0 + lerp
    v1 = v0 * k["b2"] + dz * dz * k["w2"]
    root = v1.sqrt()
    denom = root / k["r2"] + k["e"]
    q = m1 / denom
    t1 = t0 - k["step_size"] * q
    dm1 = 1.01 * U * (2 * lerp.abs() + m1.abs()) + TINY
    dv1 = 4.04 * U * v1 + TINY
    droot = torch.minimum(dv1 / (2 * root).clamp_min(1e-300), dv1.sqrt())
    ddenom = 1.01 * ((droot + U * root) / k["r2"] + U * root / k["r2"] + U * denom)
    dq = 1.01 * (dm1 + q.abs() * ddenom) / denom + U * q.abs()
    dt1 = 1.01 * (k["step_size"] * (dq + U * q.abs()) + U * t1.abs())
    zero = torch.zeros_like(d)
    vals = tuple(torch.where(ok, a, b) for a, b in ((t1, t0), (m1, m0), (v1, v0)))
    bounds = tuple(torch.where(ok, b, zero) for b in (dt1, dm1, dv1))
    return vals, bounds, ok


def masked_rows(x, theta):
    """(rows float64 [N, C], bound float64 [N, C]): sigmoid(theta[n]) x[n, c] and what fp32 allows the device around it."""
    m = sigmoid(theta).unsqueeze(1)
    rows = m * x.double()
    return rows, 1.01 * 5.04 * U * rows.abs() + TINY * x.double().abs()


def step(x, g, seg, theta, exp_avg, exp_avg_sq, *, a_size=1.0, a_ent=0.1, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    """The whole call in float64 (inputs of any float type): (x_out, d, theta1, m1, v1); g None is the apply-only form (d None,
    the three unchanged).  Rows outside every segment keep their logit and moments and hold NaN in x_out and d."""
    N = x.size(0)
    inside = segment_of(seg, N)[0] >= 0
    if g is None:
        rows = masked_rows(x, theta)[0]
        rows[~inside] = float("nan")
        return rows, None, theta.double(), None if exp_avg is None else exp_avg.double(), None if exp_avg_sq is None else exp_avg_sq.double()
    d, _, _ = d_theta(x, g, seg, theta, a_size, a_ent)
    (t1, m1, v1), _, _ = adam(d, theta, exp_avg, exp_avg_sq, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step)
    rows = masked_rows(x, t1)[0]
    rows[~inside] = float("nan")
    return rows, d, t1, m1, v1


def pyg_entropy_term(theta, eps=1e-15):
    """PyG's GNNExplainer entropy of a soft mask, elementwise: -m log(m + eps) - (1 - m) log(1 - m + eps), m = sigmoid(theta)."""
    m = torch.sigmoid(theta)
    return -m * torch.log(m + eps) - (1 - m) * torch.log(1 - m + eps)


def objective(nll, theta, seg, a_size=1.0, a_ent=0.1):
    """float64 [B]: nll + a_size * mean sigmoid(theta) + a_ent * mean H(sigmoid(theta)) per segment (an empty one: the nll alone)."""
    t = theta.double()
    m = sigmoid(t)
    h = torch.log1p(torch.exp(-t.abs())) + t.abs() * torch.where(t >= 0, 1.0 - m, m)       # H(sigmoid(t)) in nats, stable
    out = nll.double().clone()
    for j in range(len(seg) - 1):
        lo, hi = int(seg[j]), int(seg[j + 1])
        if hi > lo:
            out[j] += a_size * m[lo:hi].mean() + a_ent * h[lo:hi].mean()
    return out


def known_answer():
    """The header's known answer: (x, g, seg, s, m, reg, d, theta_new)."""
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0], [-1.0, 0.0, 1.0, 2.0]])
    g = torch.tensor([[1.0, 1.0, 1.0, 1.0], [2.0, 0.0, -2.0, 4.0]])
    return x, g, [0, 2], [10.0, 4.0], 0.5, 0.5, [2.625, 1.125], [-0.01, -0.01]
