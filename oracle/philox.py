"""The samplers' in-kernel noise, restated on the host: Philox4x32-10 and the draw convention of csrc/isg_common.hpp.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Philox4x32-10 is the counter-based generator of Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as 1, 2, 3"
(SC'11): ten rounds, each multiplying counter words 0 and 2 by 0xD2511F53 / 0xCD9E8D57 into 64-bit products, and bumping the
two key words by 0x9E3779B9 / 0xBB67AE85 between rounds.  tests/test_philox_cpu.py holds it to the published known answers.

The kernels' convention (Philox::draw): slot j of graph g under a 64-bit seed is word 0 of
    philox4x32_10((g, j, 0x1571, 0x9E37), (seed & 0xffffffff, seed >> 32))
one block per slot; the upper 24 bits make a uniform in [0, 1) (uniform24), and gumbel() is gumbel_from_bits: the
reference's Uniform(tiny, 1 - eps) -> log -> log chain with both logarithms in float64, rounded once to float32.
"""
from __future__ import annotations

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57        # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85        # key increments (Weyl sequence)
ROUNDS = 10
C2, C3 = 0x1571, 0x9E37                # counter words 2 and 3 of every draw of the kernels
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox4x32_10(counter4, key2, rounds: int = ROUNDS):
    """(c0, c1, c2, c3), (k0, k1) -> the four output words.  Every word is an int or an integer array (broadcast against each
    other); arrays come back as uint32 arrays, plain ints as a tuple of ints."""
    scalar = all(np.ndim(v) == 0 for v in tuple(counter4) + tuple(key2))
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter4]
    k = [np.asarray(v, dtype=np.uint64) & _MASK for v in key2]
    m0, m1 = np.uint64(M0), np.uint64(M1)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _SH, p0 & _MASK, p1 >> _SH, p1 & _MASK
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    if scalar:
        return tuple(int(v) for v in c)
    return tuple(v.astype(np.uint32) for v in np.broadcast_arrays(*c))


def draw(seed: int, g, j):
    """Philox::draw(seed, g, j): the 32 random bits of slot j of graph g.  g, j: ints or integer arrays."""
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10((g, j, C2, C3), (seed & 0xFFFFFFFF, seed >> 32))[0]


def uniform24(bits):
    """(bits >> 8) / 2**24 as float32: exact, in [0, 1)."""
    b = np.asarray(bits, dtype=np.uint64) >> np.uint64(8)
    return b.astype(np.float32) * np.float32(1.0 / 16777216.0)


def gumbel(bits, loc: float = 0.0, scale: float = 1.0):
    """gumbel_from_bits as the kernel states it: every product and sum rounded to float32 on its own, the two logarithms
    taken in float64 and rounded once."""
    f32 = np.float32
    tiny, hi = f32(np.finfo(np.float32).tiny), f32(1.0) - f32(np.finfo(np.float32).eps)
    u = (tiny + (uniform24(bits) * f32(hi - tiny)).astype(f32)).astype(f32)
    l1 = np.log(u.astype(np.float64)).astype(f32)
    l2 = np.log((-l1).astype(np.float64)).astype(f32)
    return (f32(loc) - (f32(scale) * l2).astype(f32)).astype(f32)


def _bits(seed: int, B: int, n: int, graph_ids=None):
    g = np.arange(B, dtype=np.uint64) if graph_ids is None else np.asarray(graph_ids, dtype=np.int64).astype(np.uint64)
    assert g.shape == (B,), "one graph number per row"
    return draw(seed, g[:, None], np.arange(n, dtype=np.uint64)[None, :])


def gumbel_noise(seed: int, B: int, nmax: int, loc: float = 0.0, scale: float = 1.0, graph_ids=None) -> torch.Tensor:
    """The [B, nmax] noise isg_topk_gumbel (loc 0, scale 1) / isg_topk_threshold (loc 0, scale 0.3) draw under `seed`; row b
    is the stream of graph b, or of graph graph_ids[b]."""
    return torch.from_numpy(np.ascontiguousarray(gumbel(_bits(seed, B, nmax, graph_ids), loc, scale)))


def uniform_noise(seed: int, B: int, n: int, graph_ids=None) -> torch.Tensor:
    """The [B, n] raw uniform isg_simple_topk draws under `seed` (n = the row length rounded up to a power of two)."""
    return torch.from_numpy(np.ascontiguousarray(uniform24(_bits(seed, B, n, graph_ids))))
