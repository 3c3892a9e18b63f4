"""oracle/philox.py against things that are not this project's code: the published Philox4x32-10 known answers, and the oracle's
torch.distributions restatement of the Gumbel transform.  The GPU tests (test_gpu_samplers.py) then hold the kernels' in-kernel
noise to oracle/philox.py."""
import numpy as np
import torch

from oracle import philox as PH
from oracle import samplers as OS

# counter, key -> output: the known-answer vectors published with the generator (Random123, kat_vectors, philox4x32 10)
KNOWN_ANSWERS = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        got = PH.philox4x32_10(counter, key)
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # the vectorised path gives the same words as the scalar one
    ctr = [np.array([c[i] for c, _, _ in KNOWN_ANSWERS], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[i] for _, k, _ in KNOWN_ANSWERS], dtype=np.uint64) for i in range(2)]
    got = PH.philox4x32_10(ctr, key)
    for i in range(4):
        assert got[i].dtype == np.uint32 and got[i].tolist() == [w[i] for _, _, w in KNOWN_ANSWERS]
    # nine rounds are another generator
    assert PH.philox4x32_10(KNOWN_ANSWERS[0][0], KNOWN_ANSWERS[0][1], rounds=9) != KNOWN_ANSWERS[0][2]


def test_draw_is_word_0_of_the_documented_block():
    for seed, g, j in [(0, 0, 0), (1, 3, 70), (2 ** 32, 9, 1023), (2 ** 63 + 5, 2, 64)]:
        want = PH.philox4x32_10((g, j, 0x1571, 0x9E37), (seed & 0xffffffff, seed >> 32))[0]
        assert PH.draw(seed, g, j) == want
    grid = PH.draw(7, np.arange(3)[:, None], np.arange(130)[None, :])
    assert grid.shape == (3, 130) and int(grid[2, 129]) == PH.draw(7, 2, 129)


def test_draw_sees_the_high_word_of_the_seed_and_the_order_of_graph_and_slot():
    j = np.arange(1024)
    assert not np.array_equal(PH.draw(1, 0, j), PH.draw(2 ** 32 + 1, 0, j))
    assert all(PH.draw(1, 0, int(i)) != PH.draw(2 ** 32 + 1, 0, int(i)) for i in (0, 1, 64, 1023))
    a = PH.draw(5, np.arange(8)[:, None], np.arange(8)[None, :])
    off = ~np.eye(8, dtype=bool)
    assert np.all(a[off] != a.T[off]), "draw(seed, g, j) == draw(seed, j, g)"
    # no two slots of a graph, and no two graphs at a slot, share a stream
    assert len(set(PH.draw(5, 3, j).tolist())) == 1024 and len(set(PH.draw(5, j, 3).tolist())) == 1024


def test_uniform24_is_the_upper_24_bits():
    bits = np.array([0, 0xff, 0x100, 0xffffffff, 0x80000000], dtype=np.uint64)
    u = PH.uniform24(bits)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]


def test_gumbel_matches_the_oracles_transform_to_an_ulp_of_each_logarithm():
    """gumbel() and oracle.samplers.uniform_to_gumbel differ only in how the two logarithms are rounded: float64 rounded once
    (within half an ulp) against torch's float32 log (within one ulp).  l1 = log(u) then differs by at most one ulp of l1,
    which log(-l1) turns into ulp(l1) / |l1| <= 2^-23; the second log adds its own ulp, the product and the difference one
    rounding each.  Bound per draw: scale * (2^-23 + 2 ulp(l2)) + ulp(scale * l2) + ulp(result)."""
    bits = PH.draw(11, np.arange(4)[:, None], np.arange(1024)[None, :]).reshape(-1)
    assert bits.size == 4096
    u01 = torch.from_numpy(PH.uniform24(bits))
    worst = 0.0
    for loc, scale in [(0.0, 1.0), (0.0, 0.3), (0.5, 2.0)]:
        got = PH.gumbel(bits, loc, scale)
        ref = OS.uniform_to_gumbel(u01, loc, scale).numpy()
        assert got.dtype == np.float32 and ref.dtype == np.float32
        l2 = (np.float64(loc) - ref.astype(np.float64)) / scale
        ulp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
        bound = scale * (2.0 ** -23 + 2 * ulp(l2)) + ulp(scale * l2) + ulp(ref)
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        worst = max(worst, float((err / bound).max()))
        print(f"[philox] loc={loc} scale={scale}: max |gumbel - oracle| = {err.max():.3e}, worst err / bound = {(err / bound).max():.2f}, "
              f"bit-equal {float((got == ref).mean()):.3f}")
        assert np.all(err <= bound)
    assert worst <= 1.0
    # the ends of the uniform: u01 = 0 gives Uniform's lower end `tiny`, the largest u01 stays below 1
    ends = PH.gumbel(np.array([0, 0xffffffff], dtype=np.uint64))
    assert np.all(np.isfinite(ends)) and ends[0] < -4.0 and ends[1] > 15.0


def test_noise_helpers_lay_rows_out_by_graph():
    n = PH.gumbel_noise(3, 4, 70)
    assert n.dtype == torch.float32 and tuple(n.shape) == (4, 70)
    assert float(n[2, 69]) == float(PH.gumbel(PH.draw(3, 2, 69)))
    cut = PH.gumbel_noise(3, 3, 70, graph_ids=[9, 2, 7])
    assert torch.equal(cut[1], n[2]) and not torch.equal(cut[0], n[0])
    assert float(cut[0, 5]) == float(PH.gumbel(PH.draw(3, 9, 5)))
    a = PH.gumbel_noise(3, 4, 70, 0.0, 0.3)
    assert torch.allclose(a, 0.3 * n, atol=1e-6) and not torch.equal(a, n)
    u = PH.uniform_noise(3, 4, 128)
    assert tuple(u.shape) == (4, 128) and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert float(u[1, 100]) == float(PH.uniform24(PH.draw(3, 1, 100)))
