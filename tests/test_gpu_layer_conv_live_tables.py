"""The masked layer kernel's live tables are built once per launch by a pre-pass and read from memory (DESIGN.md 17.14,
include/isg_masked.h).  The same table values reach the same code, so no bit of the layer may change.

(a) isg_layer_conv_live_tables against a restatement of the grouped kernel's scan written here in numpy, field by field as bit
    patterns: hand-made CSR arrays and tile lists (the pre-pass reads nothing else), 1 / 7 / 11 / 12 entries of a 14-entry list
    (the entries behind *ntiles keep the bytes they had), holding an entry beyond both caps (300 slots, 70 rows: clamped to
    256 / 64, more slots than 64 rows' worth), an entry without slots, an empty entry as a mixed plan has them, sources outside
    their tile (most: they are drawn from the whole batch), destinations without in-edges, tiles without a live slot and with
    every slot live, both mask forms, masks holding -0.0, +0.0, 0.5, 1 - 2^-24, 1 + 2^-23 and 1.  One more case takes its CSR
    and heavy-first tile list from a GraphPlan with an oversize graph.
(b) ops.gatv2_layer_conv in child processes (the switches are read once per process): the default (tables on), ISG_LC_TABLES=0,
    ISG_LC_GROUP=1 and every forced group size from 2 to 6 with tables on give EQUAL bit patterns of out, alpha, the row maxima
    and the dead-row flags, on the case batches of tests/test_gpu_layer_conv_live_groups.py and
    tests/test_gpu_layer_conv_mask_skip.py (loaded by path; the former asserts that they reach the shapes at which the grouped
    kernel branches: 32 / 33 / 64 / 65 named rows, 64 / 65 live slots).
(c) BASELINE configs[1]'s model at 256 graphs, eager and as a captured step (the pre-pass inside the hipGraph): logits, mask and
    gate equal between tables on and off."""
import dataclasses
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCAP, ECAP, H = 64, 256, 4
TILE_BYTES = 4176
FIELDS = (("eid, mask bits", 0, 2048), ("logit / inverse scale", 2048, 3072), ("source row", 3072, 3328),
          ("destination row", 3328, 3584), ("live list", 3584, 3840), ("row pointers", 3840, 4112), ("descriptor", 4112, 4128),
          ("named rows", 4128, 4144), ("live words", 4144, 4176))
MASK_VALUES = np.array([0.0, -0.0, 0.5, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0], dtype=np.float32)
RUNS = (("default", {}), ("tables0", {"ISG_LC_TABLES": "0"}), ("g1", {"ISG_LC_GROUP": "1"})) + \
    tuple((f"g{g}", {"ISG_LC_GROUP": str(g)}) for g in (2, 3, 4, 5, 6))


def _load(name):
    spec = importlib.util.spec_from_file_location("_lt_" + name, os.path.join(ROOT, "tests", f"test_gpu_layer_conv_{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------- (a) the scan, restated
def restate_image(d, rowptr, eid, src, dst, einv, nm, em):
    """One tile's table set as gatv2_layer_conv_groups_kernel's scan and compaction leave it (csrc/isg_layer_conv.hip), as bytes."""
    r0, nrows, e0, ne = (int(v) for v in d)
    nr, n = min(nrows, NCAP), min(ne, ECAP)
    s = np.arange(e0, e0 + n)
    eidv, srcv, dstv = (np.zeros(ECAP, np.int64) for _ in range(3))
    eidv[:n], srcv[:n], dstv[:n] = eid[s], src[s], dst[s]
    mask = np.ones(ECAP, np.float32)
    mask[:n] = em[eid[s]] if em is not None else nm[src[s]] * nm[dst[s]]          # one fp32 product
    bits = mask.view(np.int32)
    live = (np.arange(ECAP) < n) & ((bits & 0x7fffffff) != 0)
    inv = np.zeros(ECAP, np.float32)
    inv[:n] = einv[s]
    hi = max(nr - 1, 0)
    sx, dz = np.clip(srcv - r0, 0, hi), np.clip(dstv - r0, 0, hi)
    img = np.zeros(TILE_BYTES, np.uint8)
    img[0:2048] = np.stack([eidv.astype(np.int32), bits], 1).reshape(-1).view(np.uint8)
    img[2048:3072] = np.where(live, inv, np.float32(0.0)).astype(np.float32).view(np.uint8)
    img[3072:3328], img[3328:3584] = sx.astype(np.uint8), dz.astype(np.uint8)
    lv = np.nonzero(live)[0]
    img[3584:3584 + lv.size] = lv.astype(np.uint8)
    rp = np.zeros(68, np.int32)
    rp[:nr + 1] = rowptr[r0:r0 + nr + 1] - e0
    img[3840:4112] = rp.view(np.uint8)
    img[4112:4128] = np.array([r0, nr, e0, n], np.int32).view(np.uint8)
    touch = 0
    for r in np.concatenate([sx[live], dz[live]]):
        touch |= 1 << int(r)
    words = [sum(1 << int(b - 64 * w) for b in lv if 64 * w <= b < 64 * w + 64) for w in range(4)]
    img[4128:4136] = np.array([touch], np.uint64).view(np.uint8)
    img[4144:4176] = np.array(words, np.uint64).view(np.uint8)
    return img, int(lv.size), n


def crafted(seed):
    """A CSR over 760 rows with 0-8 in-edges each, sources drawn from ALL rows, and a 12-entry tile list: an entry beyond both
    caps, one without slots, an empty one, then rows packed greedily into <= 64 rows / <= 256 slots."""
    rng = np.random.default_rng(seed)
    N = 760
    deg = rng.integers(0, 9, N)
    deg[rng.random(N) < 0.15] = 0
    deg[:80] = np.maximum(deg[:80], 4)                   # the first entry's 64 rows hold more than 256 slots
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    E = int(rowptr[-1])
    dst = np.repeat(np.arange(N), deg).astype(np.int32)
    src = rng.integers(0, N, E).astype(np.int32)
    eid = rng.permutation(E).astype(np.int32)
    einv = (2.0 ** rng.integers(-6, 7, E)).astype(np.float32)
    lone = int(np.nonzero(deg == 0)[0][5])
    tiles = [(0, 70, 0, 300), (lone, 1, int(rowptr[lone]), 0), (17, 0, int(rowptr[17]), 0)]
    r = 80
    while r < N and len(tiles) < 12:
        k = r
        while k < N and k - r < NCAP and rowptr[k + 1] - rowptr[r] <= ECAP:
            k += 1
        tiles.append((r, k - r, int(rowptr[r]), int(rowptr[k] - rowptr[r])))
        r = k
    assert len(tiles) == 12
    return N, E, rowptr, eid, src, dst, einv, tiles, rng


def crafted_masks(N, E, rowptr, eid, tiles, rng):
    """(node mask, edge mask): every value of MASK_VALUES; tile 3 without a live slot in both forms, tiles 0 and 4 with every slot
    live in the edge form."""
    nm = MASK_VALUES[rng.integers(0, len(MASK_VALUES), N)]
    em = MASK_VALUES[rng.integers(0, len(MASK_VALUES), E)]
    r0, nr, e0, ne = tiles[3]
    nm[r0:r0 + nr] = np.where(rng.random(nr) < 0.5, np.float32(0.0), np.float32(-0.0))
    em[eid[e0:e0 + ne]] = np.where(rng.random(ne) < 0.5, np.float32(0.0), np.float32(-0.0))
    for t in (0, 4):
        r0, nr, e0, ne = tiles[t]
        em[eid[e0:e0 + min(ne, ECAP)]] = MASK_VALUES[rng.integers(2, len(MASK_VALUES), min(ne, ECAP))]
    return nm.astype(np.float32), em.astype(np.float32)


def run_prepass(dev, rowptr, eid, src, dst, einv, tile_list, T, cap, nm, em, N, E):
    from isubgvqa_amd import _lib, _lib_masked
    lib = _lib_masked.load()
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    info = np.zeros((cap, 4), np.int32)
    info[:len(tile_list)] = np.array(tile_list, np.int32).reshape(-1, 4)
    t_rowptr, t_eid, t_src, t_dst = (d(a, torch.int32) for a in (rowptr, eid, src, dst))
    t_einv, t_info, t_nt = d(einv, torch.float32), d(info, torch.int32), torch.tensor([T], dtype=torch.int32, device=dev)
    t_nm = None if nm is None else d(nm, torch.float32)
    t_em = None if em is None else d(em, torch.float32)
    assert lib.isg_layer_conv_live_tables_bytes(cap) == cap * TILE_BYTES
    tables = torch.full((cap * TILE_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    rc = lib.isg_layer_conv_live_tables(t_rowptr.data_ptr(), t_eid.data_ptr(), t_src.data_ptr(), t_dst.data_ptr(), t_einv.data_ptr(),
                                        t_info.data_ptr(), t_nt.data_ptr(), cap, 0 if t_nm is None else t_nm.data_ptr(),
                                        0 if t_em is None else t_em.data_ptr(), tables.data_ptr(), N, E,
                                        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "isg_layer_conv_live_tables")
    torch.cuda.synchronize()
    return tables.cpu().numpy().reshape(cap, TILE_BYTES)


def compare_images(got, tile_list, T, rowptr, eid, src, dst, einv, nm, em, what):
    stats = []
    for t in range(got.shape[0]):
        if t >= T:
            assert (got[t] == 0xAB).all(), f"{what}: entry {t} behind *ntiles = {T} was written"
            continue
        want, nlive, n = restate_image(tile_list[t], rowptr, eid, src, dst, einv, nm, em)
        for name, a, b in FIELDS:
            bad = np.nonzero(got[t, a:b] != want[a:b])[0]
            assert bad.size == 0, f"{what}: tile {t} {tile_list[t]}: {name}: {bad.size} bytes differ, first at byte {a + int(bad[0])}"
        assert (got[t, 4136:4144] == 0).all()
        stats.append((nlive, n))
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("node_mask", "edge_mask"))
def test_prepass_writes_the_scans_tables(form):
    dev = torch.device("cuda:0")
    N, E, rowptr, eid, src, dst, einv, tiles, rng = crafted(5)
    nm, em = crafted_masks(N, E, rowptr, eid, tiles, rng)
    nm, em = (nm, None) if form == "node_mask" else (None, em)
    # what the list holds: the entry beyond the caps, no slots, empty, clamped sources, destinations without in-edges
    assert tiles[0][1] > NCAP and tiles[0][3] > ECAP and rowptr[NCAP] - rowptr[0] > ECAP
    assert tiles[1][1] == 1 and tiles[1][3] == 0 and tiles[2][1] == 0 and tiles[2][3] == 0
    outside = sum(int(((src[e0:e0 + ne] < r0) | (src[e0:e0 + ne] >= r0 + nr)).sum()) for r0, nr, e0, ne in tiles[3:])
    assert outside > 100 and int((rowptr[1:] == rowptr[:-1]).sum()) > 20
    values = nm if nm is not None else em
    assert {v.tobytes() for v in values} == {v.tobytes() for v in MASK_VALUES}
    for T in (1, 7, 11, 12):
        got = run_prepass(dev, rowptr, eid, src, dst, einv, tiles, T, 14, nm, em, N, E)
        stats = compare_images(got, tiles, T, rowptr, eid, src, dst, einv, nm, em, f"{form}, {T} tiles")
        if T == 12:
            assert stats[0][1] == ECAP and stats[1] == (0, 0) and stats[2] == (0, 0)
            assert stats[3][0] == 0 and stats[3][1] > 0, "tile 3 was to have no live slot"
            assert any(0 < nl < n for nl, n in stats)
            if form == "edge_mask":
                assert stats[0] == (ECAP, ECAP) and stats[4][0] == stats[4][1] > 0, "tiles 0 and 4 were to have every slot live"


@pytest.mark.gpu
def test_prepass_on_a_mixed_plans_heavy_first_list():
    """CSR and tile list of a GraphPlan: two dozen graphs, one beyond a tile (an empty entry), the list in heavy-first order."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import ops
    ms = _load("mask_skip")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(21)
    graphs = ms.full_tiles(gen, 2) + ms.dense_graphs(gen, 8) + [(90, 300, True)] + ms.sparse_graphs(gen, 8)
    batch, ei = ms.topology(graphs, gen)
    plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=len(graphs))
    plan.require_csr()
    _, ntiles, cap, _ = plan.tiles(NCAP, ECAP)
    T = int(ntiles.item())
    heavy = plan.tiles_heavy_first(NCAP, ECAP).cpu().numpy()
    tiles = [tuple(int(v) for v in row) for row in heavy[:T]]
    assert 1 < T <= 12 and any(nr == 0 and ne == 0 for _, nr, _, ne in tiles) and max(ne for _, _, _, ne in tiles) == ECAP
    rowptr, eid, src, dst = (t.cpu().numpy() for t in (plan.rowptr, plan.eid, plan.src, plan.dst))
    N, E = batch.numel(), ei.size(1)
    rng = np.random.default_rng(3)
    einv = (2.0 ** rng.integers(-6, 7, E)).astype(np.float32)
    nm = np.where(rng.random(N) < 0.3, MASK_VALUES[rng.integers(2, 6, N)], np.float32(0.0)).astype(np.float32)
    got = run_prepass(dev, rowptr, eid, src, dst, einv, tiles, T, cap, nm, None, N, E)
    stats = compare_images(got, tiles, T, rowptr, eid, src, dst, einv, nm, None, "mixed plan")
    assert any(0 < nl < n for nl, n in stats)


# ------------------------------------------------------------------------------------- (b), (c) the layer, in child processes
EXTRA = ("one_per_tile", "last_chunk", "chunk_edges")        # mask_skip's cases that live_groups does not borrow


def run_child(out_path):
    """Child: every case batch of both files through ops.gatv2_layer_conv under this process's switches; the default and
    ISG_LC_TABLES=0 also run configs[1]'s model at 256 graphs, eager and captured."""
    sys.path.insert(0, ROOT)
    from isubgvqa_amd import ops, synthetic
    from isubgvqa_amd.models.layers import GlorotLinear
    lg, ms = _load("live_groups"), _load("mask_skip")
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    C, K = 128, 128
    res = {}
    for ci, name in enumerate(lg.CASES + EXTRA):
        with ops.configured(mixed_min_nodes=0):
            if name in EXTRA:
                batch, ei, B, nm, em = ms.case_inputs(name)
                plan = ops.GraphPlan.build(batch.to(dev), ei.to(dev), num_graphs=B)
            else:
                batch, ei, B, nm, em, plan, _ = lg.build_case(name, ms, ops, dev, cus, False)
            gen = torch.Generator().manual_seed(700 + ci)
            N, E = batch.numel(), ei.size(1)
            x = torch.randn(N, 128, generator=gen) * (2.0 ** torch.randint(-3, 4, (B,), generator=gen).float())[batch][:, None]
            ea = torch.randn(E, K, generator=gen)
            w = torch.randn(H * C, K, generator=gen) * 0.1
            att, bias = torch.randn(1, H, C, generator=gen), torch.randn(H * C, generator=gen) * 2.0 ** -6
            torch.manual_seed(ci)
            lin_l, lin_r = GlorotLinear(128, H * C, bias=True).to(dev), GlorotLinear(128, H * C, bias=True).to(dev)
            d = lambda t: None if t is None else t.to(dev)
            with torch.no_grad():
                o, a = ops.gatv2_layer_conv(d(x), lin_l, lin_r, d(ea), d(w), d(att), plan, H, bias=d(bias), node_mask=d(nm),
                                            edge_mask=d(em), want_rowmax=True)
                dead = ops.dead_rows(o)
                res[name] = {"layer": (o.cpu(), a.cpu(), ops.row_maxima(o).cpu(), None if dead is None else dead.cpu()),
                             "mask": (nm, em)}
    if os.environ.get("ISG_LC_GROUP") is None:
        cfg = dataclasses.replace(synthetic.CFG2, num_graphs=256)
        wl = synthetic.make_workload(cfg).to(dev)
        net = synthetic.build_answer_model(cfg).to(dev).eval()
        u = torch.rand(cfg.num_graphs, wl.max_nodes, generator=torch.Generator().manual_seed(9)).clamp(1e-6, 1.0 - 1e-6)
        noises = {i: (-torch.log(-torch.log(u))).to(dev) for i, t in enumerate(cfg.masks) if t != 1.0}
        from isubgvqa_amd import _lib_masked
        lib = _lib_masked.load()
        N, E = wl.x.size(0), wl.edge_index.size(1)
        with torch.no_grad():
            res["model"] = tuple(t.clone().cpu() for t in net(wl, noises=noises))
            res["captured"] = tuple(t.clone().cpu() for t in net(wl, noises=noises, capture=True))
            res["replayed"] = tuple(t.clone().cpu() for t in net(wl, noises=noises, capture=True))
        res["model_group"] = int(lib.isg_gatv2_layer_conv_group(N, E, H, (N + NCAP - 1) // NCAP))
        res["tables_enabled"] = int(lib.isg_layer_conv_live_tables_enabled())
    torch.save(res, out_path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    d = tmp_path_factory.mktemp("live_tables")
    out = {}
    for tag, extra in RUNS:
        env = dict(os.environ)
        for k in ("ISG_LC_GROUP", "ISG_LC_DENSE_MASK", "ISG_LC_TABLES"):
            env.pop(k, None)
        env.update(extra)
        path = str(d / f"{tag}.pt")
        subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.abspath(__file__), path], env=env,
                       cwd=ROOT, check=True, timeout=900)
        out[tag] = torch.load(path)
    return out


def _equal(what, r1, r2, parts):
    for t1, t2, part in zip(r1, r2, parts):
        if t1 is None or t2 is None:
            assert t1 is None and t2 is None, f"{what}: {part} missing on one side"
            continue
        assert t1.shape == t2.shape and t1.dtype == t2.dtype, f"{what}: {part} shape"
        if t1.dtype == torch.float32:        # bit patterns: signed zeros and NaN payloads count
            diff = (t1.view(torch.int32) != t2.view(torch.int32))
            assert not diff.any(), f"{what}: {part}: {int(diff.sum())} values differ, by up to {(t1 - t2).abs().nan_to_num(1e30).max().item():.3e}"
        else:
            assert torch.equal(t1, t2), f"{what}: {part} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("name", _load("live_groups").CASES + EXTRA)
def test_tables_change_no_bit_of_the_layer(runs, name):
    base = runs["g1"][name]                              # the per-tile kernel: no tables, no groups
    for tag, _ in RUNS:
        if tag == "g1":
            continue
        other = runs[tag][name]
        for m1, m2 in zip(base["mask"], other["mask"]):
            assert (m1 is None and m2 is None) or torch.equal(m1, m2), f"{name}: the case's mask is not the same in every process"
        _equal(f"{name}: ISG_LC_GROUP=1 vs {tag}", base["layer"], other["layer"], ("out", "alpha", "row maxima", "dead rows"))
    assert torch.isfinite(base["layer"][0]).all() and torch.isfinite(base["layer"][1]).all(), name


@pytest.mark.gpu
def test_model_is_the_same_with_tables_on_and_off(runs):
    on, off = runs["default"], runs["tables0"]
    assert on["tables_enabled"] == 1 and off["tables_enabled"] == 0
    assert on["model_group"] > 1, "256 graphs were to take the grouped kernel (and with it the tables)"
    parts = ("logits", "mask", "gate")
    _equal("configs[1] at 256 graphs, eager: tables on vs off", on["model"], off["model"], parts)
    for side, r in (("on", on), ("off", off)):
        _equal(f"tables {side}: captured vs eager", r["captured"], r["model"], parts)
        _equal(f"tables {side}: replayed vs eager", r["replayed"], r["model"], parts)
    _equal("captured: tables on vs off", on["captured"], off["captured"], parts)
    assert int(on["model"][1].sum()) > 0


if __name__ == "__main__":
    run_child(sys.argv[1])
