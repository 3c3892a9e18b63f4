"""isg_grounding / ops.grounding / explain.evaluate(grounding=True) on the GPU (include/isg_grounding.h).  Every output
is an integer: the table and the totals are compared EXACTLY with the loops over sets of tests/grounding_restated.py.  Every call of
the C ABI here runs on buffers with guard words behind them.  Sizes sit on the boundaries of a wave (graphs of 1, 64, 65 and 300
nodes: lanes stride a graph up to five times), of the first launch's workgroup (4 questions: B = 1, 5, 9) and of a facet (M = 1, 7,
64)."""
import itertools

import pytest
import torch

from grounding_restated import add_totals, bad_group_ids, restate_table

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
SIZES = {1: [65], 5: [1, 64, 65, 300, 0], 9: [1, 64, 65, 300, 0, 7, 12, 3, 33]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def C():
    from isubgvqa_amd import _lib_grounding
    return _lib_grounding.CONSTANTS


def _ptr(sizes):
    return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int32)


def _plan(sizes, dev):
    """A GraphPlan with what the scoring reads (ptr): built by hand, since graphs here may exceed what the model kernels take."""
    from isubgvqa_amd import ops
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))
    return ops.GraphPlan(N=int(sum(sizes)), E=0, B=len(sizes), ptr=_ptr(sizes).to(dev),
                         nmax_dev=torch.zeros(1, dtype=torch.int32, device=dev), nmax=0, batch=batch.to(dev))


def _gold(sizes, F, M, seed):
    """Random lists of random lengths over each graph's nodes (small graphs repeat indices by themselves), then the rows the
    header names: all pads; unresolved entries; one index repeated inside a facet and across the facets; 64 distinct indices (M =
    64, the graph of 300 nodes); entries equal to n_g, to 2^30 and to -3."""
    gen = torch.Generator().manual_seed(seed)
    B = len(sizes)
    gold = torch.full((B, F, M), -1, dtype=torch.int32)
    for q, n in enumerate(sizes):
        for f in range(F):
            cnt = int(torch.randint(0, M + 1, (1,), generator=gen))
            gold[q, f, :cnt] = torch.randint(0, max(n, 1), (cnt,), generator=gen).int()
    if B >= 5:
        gold[0] = -1                                            # all pads (a graph of one node)
        gold[1, :, 0] = -2                                      # unresolved, one per facet ...
        gold[1, 0, M // 2] = -2                                 # ... and one more where M allows
        gold[2] = 17                                            # one index in every entry of every facet
        gold[2, F - 1, M - 1] = 64                              # ... and the last node of the graph of 65
        if M == 64:
            gold[3, 0] = torch.randperm(300, generator=gen)[:64].int()          # a full row of 64 distinct indices
            if F > 1:
                gold[3, 1, :32] = gold[3, 0, 16:48]             # half of it again in the next facet
    for q in {1: [0], 5: [4], 9: [4, 7]}[B]:                    # entries equal to n_g, to 2^30 and to -3 (graphs of 65, 0 and 3 nodes)
        gold[q, 0, M - 1] = sizes[q]
        gold[q, F - 1, 0] = 1 << 30
        gold[q, F // 2, M // 3] = -3
    return gold


def _masks(sizes, seed):
    """All kept, none kept, a mix with NaNs, negative and fractional values, and a top-5 mask of random scores."""
    gen = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    values = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.3, -1.0, NAN])
    mixed = values[torch.randint(0, values.numel(), (N,), generator=gen)]
    mixed[0] = NAN
    top = torch.zeros(N)
    scores, lo = torch.rand(N, generator=gen), 0
    for n in sizes:
        if n:
            top[lo + scores[lo:lo + n].topk(min(5, n)).indices] = 1.0
        lo += n
    return {"all": torch.ones(N), "none": torch.zeros(N), "mixed": mixed, "topk": top}


def _call(dev, C, mask, sizes, gold, pred=None, label=None, groups=None, G=0, totals=None, status=None, threshold=0.0,
          want_totals=True):
    """One call of the C ABI on guarded buffers.  Returns (rc, table rows, totals rows or None, status list or None); the totals and
    the status continue from `totals` / `status` (lists) when given."""
    from isubgvqa_amd import _lib_grounding
    lib = _lib_grounding.load()
    B, T, COLS = len(sizes), C["ISG_GROUND_TOTALS"], C["ISG_GROUND_COLS"]
    F, M = gold.size(1), gold.size(2)
    d = lambda t: None if t is None else t.to(dev).contiguous()
    p = lambda t: None if t is None else t.data_ptr()
    mask_d, ptr_d, gold_d, pred_d, label_d, groups_d = d(mask), d(_ptr(sizes)), d(gold), d(pred), d(label), d(groups)
    table = torch.full((B * COLS + GUARD,), -7, dtype=torch.int32, device=dev)
    tot = torch.full(((1 + G) * T + GUARD,), 1000, dtype=torch.int64, device=dev)
    if totals is not None:
        tot[:(1 + G) * T] = torch.tensor(totals, dtype=torch.int64).view(-1).to(dev)
    st = torch.full((2 + GUARD,), -9, dtype=torch.int32, device=dev)
    st[:2] = torch.tensor(status if status is not None else [0, 0], dtype=torch.int32).to(dev)
    torch.cuda.synchronize()
    rc = lib.isg_grounding(p(mask_d) if mask_d is not None and mask_d.numel() else None, float(threshold), p(ptr_d), p(gold_d), F, M,
                           p(pred_d), p(label_d), p(groups_d), 0 if groups is None else groups.size(1), G, table.data_ptr(),
                           tot.data_ptr() if want_totals else None, st.data_ptr(), sum(sizes), B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (table[B * COLS:] == -7).all() and (tot[(1 + G) * T:] == 1000).all() and (st[2:] == -9).all(), "a guard word was written"
    if not want_totals:
        assert totals is not None or (tot == 1000).all(), "totals == NULL: the second launch does not run"
    return rc, table[:B * COLS].view(B, COLS).tolist(), tot[:(1 + G) * T].view(1 + G, T).tolist(), st[:2].tolist()


def _reserved(C):
    H, BL = C["ISG_GROUND_HEAD"], C["ISG_GROUND_BLOCK"]
    return [4, 5, 6, 7] + [H + b * BL + 7 for b in range(8)]


def _groups(B, G, seed):
    gen = torch.Generator().manual_seed(seed)
    groups = torch.randint(-1, G, (B, 2), generator=gen).to(torch.int32)
    groups[0, 0] = -1
    if B > 1:
        groups[B - 1, 1] = G                                    # a bad id, in the last row
        groups[1, 0] = groups[1, 1] = 0                         # one group named by both facets: added twice
    return groups


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("M", [1, 7, 64])
@pytest.mark.parametrize("B", [1, 5, 9])
def test_table_and_totals_equal_the_restatement(dev, C, B, M, F):
    sizes = SIZES[B]
    gold = _gold(sizes, F, M, seed=100 * B + 10 * F + M)
    gen = torch.Generator().manual_seed(B + M + F)
    pred = torch.randint(0, 3, (B,), generator=gen)
    label = torch.where(torch.rand(B, generator=gen) < 0.6, pred, pred + 1)
    zeros = lambda G: [[0] * C["ISG_GROUND_TOTALS"] for _ in range(1 + G)]
    for name, mask in _masks(sizes, seed=B).items():
        want = restate_table(mask, _ptr(sizes), gold)
        rc, table, totals, status = _call(dev, C, mask, sizes, gold, totals=zeros(0))      # no pred, no groups
        assert rc == 0 and table == want, (name, [(q, a, b) for q, (a, b) in enumerate(zip(table, want)) if a != b][:4])
        assert totals == add_totals(None, want, C) and totals[0][1] == 0 and status == [0, 0], name
        for G in (1, 5):
            groups = _groups(B, G, seed=G + B)
            rc, table, totals, status = _call(dev, C, mask, sizes, gold, pred, label, groups, G, totals=zeros(G))
            assert rc == 0 and table == want, (name, G)
            ref = add_totals(None, want, C, pred.tolist(), label.tolist(), groups, G)
            assert totals == ref, (name, G, [(r, i, a, b) for r in range(1 + G) for i, (a, b) in enumerate(zip(totals[r], ref[r])) if a != b][:6])
            n_bad, first = bad_group_ids(groups, G)
            assert status == ([n_bad, first] if n_bad else [0, 0]), (name, G)
    if B >= 5:                                                  # the rows _gold wrote by hand are what it says they are
        assert want[0][2:] == [0] * 10 and want[1][2] == F + (1 if M >= 2 else 0) and want[2][10] == (2 if F * M > 1 else 1)
        assert want[4][:2] == [0, 0] and want[4][3] >= 1 and want[4][4:] == [0] * 8
        if M == 64:
            assert want[3][4] == 64 and want[3][10] >= 64 and (F == 1 or want[3][6] >= 32)
    assert sum(r[3] for r in want) >= 1


def test_bad_entries_are_counted_and_change_nothing_else(dev, C):
    sizes = SIZES[9]
    gold = _gold(sizes, 3, 7, seed=5)
    for q, n in enumerate(sizes):                               # every kind in every question, beside what _gold placed
        gold[q, 1, 2], gold[q, 2, 6], gold[q, 0, 3] = n, 1 << 30, -3
    gold[8, 1, 5] = -(1 << 31)
    mask = _masks(sizes, seed=2)["mixed"]
    clean = gold.clone()
    bad = (clean < -2) | (clean >= torch.tensor(sizes).view(-1, 1, 1))
    clean[bad] = -1
    _, with_bad, _, _ = _call(dev, C, mask, sizes, gold, want_totals=False)
    _, without, _, _ = _call(dev, C, mask, sizes, clean, want_totals=False)
    assert with_bad == restate_table(mask, _ptr(sizes), gold)
    assert [r[3] for r in with_bad] == bad.sum((1, 2)).tolist() and all(r[3] >= 3 for r in with_bad) and all(r[3] == 0 for r in without)
    assert [r[:3] + r[4:] for r in with_bad] == [r[:3] + r[4:] for r in without]


def test_threshold_is_strict_and_a_nan_is_never_kept(dev, C):
    sizes = [3, 70]
    mask = torch.cat([torch.tensor([0.5, NAN, 0.6]), torch.full((70,), 0.5)])
    mask[3 + 69] = 0.75
    gold = torch.tensor([[[0, 1, 2]], [[69, 0, 68]]], dtype=torch.int32)
    for thr, rows in ((0.0, [[2, 3, 0, 0, 3, 2], [70, 70, 0, 0, 3, 3]]), (0.5, [[1, 3, 0, 0, 3, 1], [1, 70, 0, 0, 3, 1]]),
                      (-1.0, [[2, 3, 0, 0, 3, 2], [70, 70, 0, 0, 3, 3]]), (float("-inf"), [[2, 3, 0, 0, 3, 2], [70, 70, 0, 0, 3, 3]])):
        _, table, _, _ = _call(dev, C, mask, sizes, gold, threshold=thr, want_totals=False)
        assert [r[:6] for r in table] == rows and table == restate_table(mask, _ptr(sizes), gold, thr), thr


def test_totals_accumulate_and_two_identical_calls_give_identical_bits(dev, C):
    sizes = SIZES[9]
    gold, masks = _gold(sizes, 3, 7, seed=11), _masks(sizes, seed=3)
    pred = torch.arange(9) % 2
    label = torch.zeros(9, dtype=torch.int64)
    groups = _groups(9, 5, seed=1)
    args = (pred, label, groups, 5)
    _, t1, one, s1 = _call(dev, C, masks["mixed"], sizes, gold, *args, totals=[[0] * C["ISG_GROUND_TOTALS"]] * 6)
    _, t2, two, s2 = _call(dev, C, masks["mixed"], sizes, gold, *args, totals=[[0] * C["ISG_GROUND_TOTALS"]] * 6)
    assert t1 == t2 and one == two and s1 == s2 == [1, 8]
    # a second batch on top of the first; the status' count runs on and its first bad row stays
    _, t3, both, s3 = _call(dev, C, masks["topk"], sizes, gold, *args, totals=one, status=s1)
    want = add_totals(add_totals(None, t1, C, pred.tolist(), label.tolist(), groups, 5), t3, C, pred.tolist(), label.tolist(), groups, 5)
    assert both == want and s3 == [2, 8]
    groups[2, 0] = -5
    _, _, _, s4 = _call(dev, C, masks["topk"], sizes, gold, *args, totals=one, status=[0, 0])
    assert s4 == [2, 2]
    # whatever the buffers held: every entry has the batch added, the reserved ones are never written
    _, _, dirty, _ = _call(dev, C, masks["mixed"], sizes, gold, pred, label)
    fresh = add_totals(None, t1, C, pred.tolist(), label.tolist())
    res = set(_reserved(C))
    assert dirty[0] == [1000 + (0 if i in res else v) for i, v in enumerate(fresh[0])] and all(fresh[0][i] == 0 for i in res)


def test_without_totals_one_launch_runs_and_without_questions_none(dev, C):
    sizes = SIZES[5]
    gold, mask = _gold(sizes, 3, 7, seed=4), _masks(sizes, seed=4)["mixed"]
    groups = _groups(5, 5, seed=2)
    assert bad_group_ids(groups, 5)[0] == 1
    rc, table, totals, status = _call(dev, C, mask, sizes, gold, None, None, groups, 5, want_totals=False)
    assert rc == 0 and table == restate_table(mask, _ptr(sizes), gold)
    assert status == [0, 0], "the status is the second launch's: without totals nothing advances it"
    rc, table, totals, status = _call(dev, C, torch.zeros(0), [], torch.zeros(0, 3, 7, dtype=torch.int32), None, None,
                                      torch.zeros(0, 2, dtype=torch.int32), 5)
    assert rc == 0 and table == [] and all(v == 1000 for r in totals for v in r) and status == [0, 0]
    # graphs without a node in a batch without a node: the mask may be NULL
    rc, table, _, _ = _call(dev, C, torch.zeros(0), [0, 0], torch.tensor([[[0, -2]], [[-1, -1]]], dtype=torch.int32), want_totals=False)
    assert rc == 0 and table == [[0, 0, 1, 1] + [0] * 8, [0] * 12]


def test_a_ptr_beyond_the_mask_is_clamped(dev, C):
    """ptr is the caller's; the kernel clamps it to [0, N] as isg_token_coo does, so no index derived from it leaves the mask."""
    from isubgvqa_amd import _lib_grounding
    lib = _lib_grounding.load()
    mask = torch.ones(8, device=dev)
    ptr = torch.tensor([-3, 5, 1 << 20], dtype=torch.int32, device=dev)
    gold = torch.tensor([[[0, 4, 5]], [[2, 3, 7]]], dtype=torch.int32, device=dev)
    table = torch.full((2 * 12 + GUARD,), -7, dtype=torch.int32, device=dev)
    assert lib.isg_grounding(mask.data_ptr(), 0.0, ptr.data_ptr(), gold.data_ptr(), 1, 3, None, None, None, 0, 0, table.data_ptr(), None,
                             None, 8, 2, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert table[:24].view(2, 12).tolist() == [[5, 5, 0, 1, 2, 2, 0, 0, 0, 0, 2, 2], [3, 3, 0, 2, 1, 1, 0, 0, 0, 0, 1, 1]]
    assert (table[24:] == -7).all()


def test_ops_grounding_takes_a_forward_mask_and_counts(dev, C):
    from isubgvqa_amd import ops
    sizes = SIZES[9]
    gold, mask = _gold(sizes, 3, 7, seed=21), _masks(sizes, seed=21)["topk"]
    plan = _plan(sizes, dev)
    want = restate_table(mask, _ptr(sizes), gold)
    ops.reset_counters()
    res = ops.grounding(mask.view(-1, 1).to(dev), plan, gold.to(dev))
    assert isinstance(res, ops.Grounding) and res.totals is None and res.table.dtype == torch.int32
    assert tuple(res.table.shape) == (9, ops.GROUND_COLS) and res.table.tolist() == want
    pred, label = torch.arange(9) % 3, torch.zeros(9, dtype=torch.int64)
    flat = torch.zeros(ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
    out = ops.grounding(mask.to(dev), plan, gold.to(dev), pred.to(dev), label.to(dev), totals=flat)
    assert out.totals is flat and flat.tolist() == add_totals(None, want, C, pred.tolist(), label.tolist())[0]
    groups = _groups(9, 5, seed=3)
    totals = torch.zeros(6, ops.GROUND_TOTALS, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    for _ in range(2):
        ops.grounding(mask.to(dev), plan, gold.to(dev), pred.to(dev), label.to(dev), groups.to(dev), 5, totals=totals, status=status)
    once = add_totals(None, want, C, pred.tolist(), label.tolist(), groups, 5)
    assert totals.tolist() == add_totals(once, want, C, pred.tolist(), label.tolist(), groups, 5) and status.tolist() == [2, 8]
    assert ops.counters()["grounding"] == 4
    half = ops.grounding(mask.to(dev), plan, gold.to(dev), threshold=1.0)
    assert [r[0] for r in half.table.tolist()] == [0] * 9
    assert ops.grounding(torch.zeros(0, device=dev), _plan([], dev), torch.zeros(0, 3, 4, dtype=torch.int32, device=dev)).table.shape == (0, 12)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def _sync_warnings(fn):
    import warnings
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, [str(w.message) for w in seen if "synchroniz" in str(w.message)]


def _tables(classes, vocab):
    from isubgvqa_amd import explain
    return explain.TokenTables({f"w{i}": i for i in range(vocab)}, [f"w{(11 * a) % vocab}" if a % 3 == 0 else f"answer {a}" for a in range(classes)])


def test_evaluate_with_grounding_equals_the_restatement_on_the_same_forwards(dev, C):
    from isubgvqa_amd import explain, ops, synthetic
    from isubgvqa_amd.datasets import QuestionTypes
    cfgs = [synthetic.WorkloadConfig(num_graphs=B, channels=128, layers=3, masks=(1.0, 1.0, 0.15), sampler="imle", sample_k=5,
                                     nodes_mean=14.0, nodes_std=6.0, nodes_min=2, nodes_max=40, edges_per_graph=30.0, seed=40 + B)
            for B in (6, 9)]
    model = synthetic.build_answer_model(cfgs[0]).to(dev).eval()
    seen = []
    model.register_forward_hook(lambda m, args, out: seen.append(tuple(t.detach() for t in out[:2])))
    tables = _tables(1842, 300)
    qt = QuestionTypes(names={"structural": ["query", "verify", "choose"], "semantic": ["attr", "rel"]})
    gen = torch.Generator().manual_seed(9)
    host, batches = [], []
    for i, cfg in enumerate(cfgs):
        wl = synthetic.make_workload(cfg)
        d = wl.to(dev)
        with torch.no_grad():
            first = model(d)
        label = first[0].argmax(1).cpu()
        label[2::3] = (label[2::3] + 1) % 1842                  # two answers of three are right
        gold = synthetic.make_gold(wl.graph_sizes[0], facets=3, entries=6, seed=50 + i)
        names = torch.randint(0, 300, (wl.x.size(0),), generator=gen)
        types = [{"structural": ["query", "verify", "choose"][q % 3], "semantic": ["attr", "rel"][q % 2]} for q in range(cfg.num_graphs)]
        del types[1]["semantic"]
        batches.append(explain.EvalBatch(d, label.to(dev), names=names.to(dev), groups=qt.encode(types), gold=gold))
        host.append((wl, label, gold, qt.encode(types), first[1].cpu()))
        assert int((gold == -2).sum()) > 0 and int((gold == -1).sum()) > 0 and int((gold >= 0).sum()) > 0
    run = lambda **kw: _sync_warnings(lambda: explain.evaluate(model, batches, tables, **kw))
    run(types=qt, grounding=True)                                # warm: plans, the tables' device copies
    ops.check_plans()
    seen.clear()
    ops.reset_counters()
    plain, waits_plain = run()
    assert ops.counters()["grounding"] == 0 and plain.grounding is None and plain.by_type is None
    typed, waits_typed = run(types=qt)
    assert ops.counters()["grounding"] == 0 and typed.grounding is None
    seen.clear()
    report, waits = run(grounding=True)
    both, waits_both = run(types=qt, grounding=True)
    assert ops.counters()["grounding"] == 4
    assert len(waits) == len(waits_plain) == len(waits_both) == len(waits_typed), f"grounding costs a device-to-host copy more: {waits}"
    # grounding=False is today's evaluation, and grounding=True leaves the co-occurrence totals their bits
    assert report.totals == plain.totals == both.totals == typed.totals and report.by_type is None
    assert {f: {n: r.totals for n, r in d_.items()} for f, d_ in both.by_type.items()} == \
           {f: {n: r.totals for n, r in d_.items()} for f, d_ in typed.by_type.items()}
    # the restatement, fed with the same forwards' masks and predictions
    assert len(seen) == 4
    want = want_typed = None
    for (logits, mask), (wl, label, gold, groups, first_mask) in zip(seen[:2], host):
        assert torch.equal(mask.cpu(), first_mask), "the imle sampler in eval() is deterministic"
        table = restate_table(mask.cpu(), _ptr(wl.graph_sizes[0].tolist()), gold)
        pred = logits.argmax(1).cpu().tolist()
        want = add_totals(want, table, C, pred, label.tolist())
        want_typed = add_totals(want_typed, table, C, pred, label.tolist(), groups, qt.num_groups)
        assert all(0 < r[0] <= min(5, r[1]) for r in table), "a top-5 mask"
    g = report.grounding
    assert isinstance(g, explain.GroundingReport) and list(g.totals) == want[0] and g.by_type is None
    assert g.questions == 15 and 0 < g.correct < 15 and g.unresolved > 0 and g.bad == 0
    any_all = g.sets["any"]["all"]
    assert 0 < any_all.questions <= 15 and 0.0 <= any_all.recall <= 1.0 and 0.0 < any_all.chance < 1.0
    assert g.sets["any"]["correct"].questions <= any_all.questions
    gb = both.grounding
    assert list(gb.totals) == want_typed[0] == want[0] and set(gb.by_type) == {"structural", "semantic"}
    for i, (facet, name) in enumerate(qt.group_names):
        assert list(gb.by_type[facet][name].totals) == want_typed[1 + i], (facet, name)
    assert sum(r.questions for r in gb.by_type["structural"].values()) == 15
    assert sum(r.questions for r in gb.by_type["semantic"].values()) == 13          # one question of each batch has no semantic type
    with pytest.raises(ValueError):
        explain.evaluate(model, [b._replace(gold=None) for b in batches], tables, grounding=True)


def test_grounding_through_a_graph_index_equals_the_expanded_batch(dev, C):
    """One full-model batch asked through encode_scene / ask (many questions per graph) and the same questions through forward()
    on the expanded batch: the masks agree (asserted), so the grounding reports are equal."""
    from isubgvqa_amd import explain, ops, synthetic
    from test_gpu_instances import G_MODEL, Q_MODEL, WL_SEED, _model, _workload
    model = _model().to(dev)
    wl = _workload(WL_SEED, sym=False)
    rep = wl.replicated()
    d, dr = wl.to(dev), rep.to(dev)
    seen = []

    class Recorder:
        def __init__(self, inner):
            self.inner = inner

        def encode_scene(self, *a, **k):
            return self.inner.encode_scene(*a, **k)

        def ask(self, *a, **k):
            out, inst = self.inner.ask(*a, **k)
            seen.append((out[0].detach(), out[1].detach()))
            return out, inst

        def __call__(self, *a, **k):
            out = self.inner(*a, **k)
            seen.append((out[0].detach(), out[1].detach()))
            return out

    tables = _tables(1842, 2578)
    nodes_q = wl.graph_sizes[0][wl.graph_index]
    gold = synthetic.make_gold(nodes_q, facets=3, entries=5, seed=77)
    with torch.no_grad():
        label = model(dr.x, dr.edge_index, dr.edge_attr, dr.batch, dr.questions, dr.att_mask, return_masks=True,
                      scene_graphs=dr.scene_graphs())[0].argmax(1)
    label[1::2] = (label[1::2] + 1) % 1842
    rec = Recorder(model)
    shared = explain.evaluate(rec, [explain.EvalBatch(d, label, graph_index=wl.graph_index, gold=gold)], tables, grounding=True)
    plain = explain.evaluate(rec, [explain.EvalBatch(dr, label, gold=gold)], tables, grounding=True)
    ops.check_plans()
    (logits_s, mask_s), (logits_p, mask_p) = seen
    assert mask_s.shape == mask_p.shape and torch.equal(mask_s, mask_p), "a top-k mask differs between the two routes"
    assert torch.equal(logits_s.argmax(1), logits_p.argmax(1))
    assert shared.grounding.totals == plain.grounding.totals and shared.totals == plain.totals
    want = add_totals(None, restate_table(mask_p.cpu(), _ptr(nodes_q.tolist()), gold), C, logits_p.argmax(1).tolist(), label.tolist())
    assert list(shared.grounding.totals) == want[0]
    assert shared.grounding.questions == Q_MODEL and 0 < shared.grounding.correct < Q_MODEL and G_MODEL < Q_MODEL
    assert shared.grounding.sets["any"]["all"].questions > 0
