"""isg_answer_rank / isg_group_meters / isg_token_coo_groups, ops.answer_rank / group_meters / token_coo_groups, train.validate with
TypedMeters and explain.evaluate(types=...) on the GPU (include/isg_eval.h).  Ranks, ids and counts are compared
EXACTLY with the restatement of tests/eval_restated.py; probabilities and loss sums within bounds derived from the number formats.
Sizes sit on the boundaries of a wave (64 classes per trip), of the rank kernel's workgroup (4 rows) and of the grouped meters'
partial tables (64 rows)."""
import warnings

import pytest
import torch

from eval_restated import add_coo_groups, add_group_meters, bad_ids, restate_rank, restate_top
from test_gpu_token_coo import _made_up_tables, _pick, _questions, _random_case, _run, _sizes

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# rank and the K best classes
# ---------------------------------------------------------------------------------------------------------------------
def _rank_case(A, seed):
    """Twelve rows of every class the header names: random, ties at the label with equal values below and above its index, a
    constant row, infinities, a NaN row, an ignored row, labels -1 and A, and rows of few distinct values (ties everywhere)."""
    gen = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(12, A, generator=gen)
    lab = torch.randint(0, A, (12,), generator=gen)
    mid = A // 2
    x[1] = torch.randint(0, 3, (A,), generator=gen).float()
    x[1, [0, mid, A - 1]] = 2.0                                 # the label's value below and above its index
    lab[1] = mid
    x[2] = 1.5                                                  # constant: the rank is the label's index
    x[3, ::3] = -INF
    x[3, A - 1] = INF
    if A > 2:
        x[3, 1] = INF
    lab[3] = A - 1
    x[4, A // 3] = NAN
    lab[5] = -100
    lab[6] = -1
    lab[7] = A
    x[8:] = torch.randint(0, 4, (4, A), generator=gen).float()
    return x, lab


_REF = {}


def _rank_ref(A):
    """The restatement of one A, computed once and shared by the cases that read it (never modified)."""
    if A not in _REF:
        x, lab = _rank_case(A, seed=1000 + A)
        _REF[A] = (x, lab, restate_rank(x, lab))
    return _REF[A]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("A", [1, 2, 63, 64, 65, 129, 1842])
def test_rank_and_top_k_equal_the_restatement(dev, A, pad):
    from isubgvqa_amd import ops
    x, lab, want_rank = _rank_ref(A)
    wide = torch.full((12, A + pad), 77.0)                      # ld = A + 3: rows only 4-byte aligned, padding that would win
    wide[:, :A] = x
    xd, labd = wide.to(dev)[:, :A], lab.to(dev)
    assert xd.stride(0) == A + pad
    for B in (0, 1, 5, 12):                                     # 5: one row more than a workgroup of the rank kernel takes
        ce = ops.cross_entropy(xd[:B], labd[:B])
        for K in (1, 5, 8):
            res = ops.answer_rank(xd[:B], labd[:B], k=K, lse=ce.lse, want_top=True)
            assert res.rank.dtype == torch.int32 and res.top_ids.dtype == torch.int64 and res.top_prob.dtype == torch.float32
            assert tuple(res.top_ids.shape) == tuple(res.top_prob.shape) == (B, K)
            assert res.rank.tolist() == want_rank[:B].tolist(), (A, B, K)
            lse = ce.lse.cpu()
            want_ids, want_prob = restate_top(x[:B], K, lse)
            assert res.top_ids.tolist() == want_ids.tolist(), (A, B, K)
            if K > A:
                assert (res.top_ids[:, A:] == -1).all() and (res.top_prob[:, A:] == 0).all()
            got = res.top_prob.cpu().double()
            for b in range(B):
                for r in range(K):
                    g, w, a = float(got[b, r]), float(want_prob[b, r]), int(want_ids[b, r])
                    if a < 0 or w == 0.0:
                        assert g == 0.0, (A, b, r, g)
                    elif w != w:
                        assert g != g, (A, b, r, g)
                    else:       # the fp32 argument's rounding, |x - lse| * 2^-24 relative, plus two ulp of expf: derived, not measured
                        tol = (abs(float(x[b, a]) - float(lse[b])) + 4.0) * 2.0 ** -23
                        assert abs(g - w) <= tol * w, (A, b, r, g, w, tol)
        alone = ops.answer_rank(xd[:B], labd[:B])               # the rank alone: no K, no lse
        assert alone.top_ids is None and alone.top_prob is None and alone.rank.tolist() == want_rank[:B].tolist()
        ids_only = ops.answer_rank(xd[:B], labd[:B], k=5, want_top=True)
        assert ids_only.top_prob is None and ids_only.top_ids.tolist() == restate_top(x[:B], 5)[0].tolist()
        if B:
            # rank == 0 is isg_xent_fwd's pred == label on every row without a NaN
            clean = ~torch.isnan(x[:B]).any(1)
            hit = (ce.pred.cpu().long() == lab[:B])
            assert ((alone.rank.cpu() == 0) == hit)[clean].all()
    with pytest.raises(ValueError):
        ops.answer_rank(xd, labd, k=9, want_top=True)


def test_ignore_index_inside_the_classes_and_a_nan_at_the_label(dev):
    from isubgvqa_amd import ops
    x = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [NAN, 2.0, 3.0], [3.0, NAN, 1.0]])
    lab = torch.tensor([1, 2, 0, 0])
    res = ops.answer_rank(x.to(dev), lab.to(dev), ignore_index=1)
    assert res.rank.tolist() == restate_rank(x, lab, ignore_index=1).tolist() == [-1, 0, 3, 3]


def test_hits_at_1_and_5_equal_the_reference_accuracy_counts(dev):
    """accuracy(output, target, topk=(1, 5)) of the reference: a row is a hit at k iff its label is among torch.topk's first k
    indices.  On rows without a tie at positions 1 and 5 that is 0 <= rank < k."""
    from isubgvqa_amd import ops
    gen = torch.Generator().manual_seed(17)
    B, A = 300, 1842
    x = torch.randn(B, A, generator=gen)
    lab = torch.randint(0, A, (B,), generator=gen)
    lab[::3] = x[::3].topk(7, 1).indices[torch.arange(len(lab[::3])), torch.randint(0, 7, (len(lab[::3]),), generator=gen)]
    top = x.topk(6, 1, True, True)                               # on the CPU
    assert (top.values[:, 0] != top.values[:, 1]).all() and (top.values[:, 4] != top.values[:, 5]).all(), \
        "seeded inputs with a tie at position 1 or 5: the test's inputs are wrong"
    want = {k: int((top.indices[:, :k] == lab[:, None]).any(1).sum()) for k in (1, 5)}
    rank = ops.answer_rank(x.to(dev), lab.to(dev)).rank.cpu()
    assert {k: int(((rank >= 0) & (rank < k)).sum()) for k in (1, 5)} == want
    assert 0 < want[1] < want[5] < B


# ---------------------------------------------------------------------------------------------------------------------
# grouped meters
# ---------------------------------------------------------------------------------------------------------------------
def _meters_case(B, F, G, seed, empty=(3,)):
    gen = torch.Generator().manual_seed(seed)
    loss = 5.0 * torch.rand(B, generator=gen)
    loss[torch.randint(0, B, (max(1, B // 40),), generator=gen)] = NAN
    loss[torch.randint(0, B, (max(1, B // 60),), generator=gen)] = INF
    rank = torch.randint(-1, 9, (B,), generator=gen).to(torch.int32)
    groups = torch.randint(-1, G, (B, F), generator=gen).to(torch.int32)
    for g in empty:
        if G > g + 1:
            groups[groups == g] = g + 1                        # a group without rows
    return loss, rank, groups


def _check_meters(totals, want, loss, B_total, what):
    got = totals.cpu()
    for slot in (0, 2, 3, 4):
        assert got[:, slot].tolist() == want[:, slot].tolist(), (what, "slot", slot)
    fin = loss[torch.isfinite(loss)].double().abs().sum()
    bound = B_total * 2.0 ** -52 * float(fin)                   # B terms, each rounded once in double
    assert float((got[:, 1] - want[:, 1]).abs().max()) <= bound, (what, float((got[:, 1] - want[:, 1]).abs().max()), bound)
    assert float(got[:, 5:].abs().sum()) == 0.0, "the reserved slots are never written"


@pytest.mark.parametrize("G", [1, 7, 256])
@pytest.mark.parametrize("F", [1, 2, 4])
def test_group_meters_equal_the_restatement_over_two_batches(dev, F, G):
    from isubgvqa_amd import ops
    k = 5
    first, second = _meters_case(600, F, G, seed=10 * F + G), _meters_case(257, F, G, seed=10 * F + G + 1)    # 10 and 5 partial tables
    totals = torch.zeros(G, 8, dtype=torch.float64, device=dev)
    overall = torch.zeros(8, dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    want = None
    for loss, rank, groups in (first, second):
        out = ops.group_meters(loss.to(dev), rank.to(dev), groups.to(dev), totals, k=k, status=status, overall=overall)
        assert out is totals
        want = add_group_meters(want, loss, rank, groups, G, k)
    both = torch.cat([first[0], second[0]])
    _check_meters(totals, want, both, 857, f"F={F} G={G}")
    assert status.tolist() == [0, 0]
    if G == 7:
        assert float(want[3].abs().sum()) == 0.0 and float(totals[3].abs().sum()) == 0.0       # the empty group
    if G == 1:
        assert want[0, 0] > 0                                   # every row that has a group has this one
    # overall: the same slots with every counted row once
    ranks = torch.cat([first[1], second[1]])
    ones = torch.zeros(857, 1, dtype=torch.int32)
    _check_meters(overall.view(1, 8), add_group_meters(None, both, ranks, ones, 1, k), both, 857, "overall")


def test_group_meters_give_the_same_bits_whatever_ran_before(dev):
    from isubgvqa_amd import ops
    loss, rank, groups = _meters_case(1500, 2, 7, seed=3)
    d = [t.to(dev) for t in (loss, rank, groups)]
    one = ops.group_meters(*d, torch.zeros(7, 8, dtype=torch.float64, device=dev), k=3).clone()
    other = _meters_case(700, 4, 256, seed=4)
    ops.group_meters(*[t.to(dev) for t in other], torch.zeros(256, 8, dtype=torch.float64, device=dev), k=5)
    two = ops.group_meters(*d, torch.zeros(7, 8, dtype=torch.float64, device=dev), k=3)
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))
    assert float(one[:, 1].sum()) > 0


def test_a_facet_that_names_every_row_once_sums_to_the_meters(dev):
    from isubgvqa_amd import ops, train
    gen = torch.Generator().manual_seed(23)
    B, A, G = 300, 65, 7
    x = torch.randn(B, A, generator=gen).to(dev)
    lab = torch.randint(0, A, (B,), generator=gen)
    lab[::2] = x[::2].argmax(1).cpu()
    lab = lab.to(dev)
    groups = torch.stack([torch.randint(0, 4, (B,), generator=gen), torch.randint(4, 8, (B,), generator=gen)], 1).to(torch.int32)
    groups[groups == 7] = -1                                    # the second facet leaves rows out, the first names every row once
    meters = train.Meters(dev)
    ce = ops.cross_entropy(x, lab, totals=meters.totals)
    rank = ops.answer_rank(x, lab).rank
    totals = ops.group_meters(ce.row_loss, rank, groups.to(dev), torch.zeros(G, 8, dtype=torch.float64, device=dev), k=5).cpu()
    t = meters.totals.cpu()
    assert float(totals[:4, 0].sum()) == float(t[3]) == B and float(totals[:4, 3].sum()) == float(t[2]) >= B // 2
    assert float(totals[4:, 0].sum()) < B


def test_a_bad_id_sets_status_and_skips_the_row(dev):
    from isubgvqa_amd import ops
    loss, rank, groups = _meters_case(600, 2, 7, seed=5)
    rank[:] = rank.clamp(min=0)
    groups[300, 1], groups[299, 0], groups[580, 0] = 7, 0, -2   # G itself and an id below -1; row 300 is the first bad one
    assert bad_ids(groups, 7) == (2, 300)
    totals = torch.zeros(7, 8, dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.group_meters(loss.to(dev), rank.to(dev), groups.to(dev), totals, k=5, status=status)
    _check_meters(totals, add_group_meters(None, loss, rank, groups, 7, 5), loss, 600, "bad ids")
    assert status.tolist() == [2, 300]
    groups[5, 0] = 1 << 20
    ops.group_meters(loss.to(dev), rank.to(dev), groups.to(dev), totals, k=5, status=status)
    assert status.tolist() == [5, 300], "the count runs on, the first bad row of the evaluation stays"
    torch.cuda.synchronize()                                    # the pass ends clean
    # the grouped co-occurrence totals keep the same rule
    c = _random_case(_sizes(5, seed=5), 6, 4, seed=105)
    table = _run(c, dev).table
    g = torch.tensor([[0, 3], [9, 1], [-1, -7], [2, 2], [0, 1]], dtype=torch.int32)
    coo = torch.zeros(4, ops.COO_TOTALS, dtype=torch.int64, device=dev)
    status.zero_()
    ops.token_coo_groups(table, c["qflags"].to(dev), g.to(dev), coo, status=status)
    assert status.tolist() == [2, 1] and coo.tolist() == add_coo_groups(None, table.cpu(), c["qflags"], g, 4)


# ---------------------------------------------------------------------------------------------------------------------
# grouped co-occurrence totals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,G", [(3, 1, 1), (4, 2, 7), (5, 4, 7), (257, 2, 256)])
def test_grouped_coo_totals_equal_the_fold_over_every_subset(dev, B, F, G):
    from isubgvqa_amd import ops
    c = _random_case(_sizes(B, seed=B), 6, 4, seed=100 + B)     # the workloads of tests/test_gpu_token_coo.py
    whole = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    table = _run(c, dev, totals=whole).table
    gen = torch.Generator().manual_seed(B)
    groups = torch.randint(-1, G, (B, F), generator=gen).to(torch.int32)
    per = max(1, G // F)
    groups[:, 0] = torch.randint(0, per, (B,), generator=gen)   # facet 0 names every question once, with ids no other facet uses
    for f in range(1, F):
        groups[:, f][(groups[:, f] >= 0) & (groups[:, f] < per)] = -1
    totals = torch.zeros(G, ops.COO_TOTALS, dtype=torch.int64, device=dev)
    want = None
    for _ in range(2):                                          # two calls add up
        assert ops.token_coo_groups(table, c["qflags"].to(dev), groups.to(dev), totals) is totals
        want = add_coo_groups(want, table.cpu(), c["qflags"], groups, G)
    got = totals.tolist()
    assert got == want, [(g, i, a, b) for g in range(G) for i, (a, b) in enumerate(zip(got[g], want[g])) if a != b][:8]
    assert [sum(col) for col in zip(*got[:per])] == [2 * v for v in whole.tolist()], "the groups of one facet sum to the totals"
    assert all(row[12:16] == [0, 0, 0, 0] for row in got)
    no_flags = ops.token_coo_groups(table, None, groups.to(dev), torch.zeros(G, ops.COO_TOTALS, dtype=torch.int64, device=dev))
    assert no_flags.tolist() == add_coo_groups(None, table.cpu(), None, groups, G)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _types(B, seed, drop=()):
    gen = torch.Generator().manual_seed(seed)
    st, se = ["query", "verify", "choose", "logical"], ["attr", "rel", "obj"]
    out = [{"structural": st[int(torch.randint(0, 4, (1,), generator=gen))], "semantic": se[int(torch.randint(0, 3, (1,), generator=gen))],
            "detailed": f"d{q}"} for q in range(B)]
    for q in drop:
        del out[q]["semantic"]
    return out


def _sync_warnings(fn):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return out, [str(w.message) for w in seen if "synchroniz" in str(w.message)]


def test_validate_with_typed_meters_reports_the_restatement_in_one_copy(dev):
    from isubgvqa_amd import ops, synthetic, train
    from isubgvqa_amd.datasets import QuestionTypes
    from isubgvqa_amd.models import build_model
    vocab = 2048
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(text_vocab_size=vocab), None).to(dev).eval()
    host = [synthetic.make_full_workload(6, tokens=8, seed=61, text_vocab=vocab, sg_vocab=300),
            synthetic.make_full_workload(9, tokens=8, seed=62, text_vocab=vocab, sg_vocab=300)]
    types = [_types(6, 1, drop=(2,)), _types(9, 2)]
    qt = QuestionTypes(names={"structural": ["query", "verify", "choose", "logical", "compare"], "semantic": ["attr", "rel", "obj"]})
    seen = []

    class Recorder(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, **kw):
            out = self.inner(**kw)
            seen.append(out[0].detach().clone())                # stays on the device: no copy inside the pass
            return out

    batches = []
    for i, wl in enumerate(host):
        d = wl.to(dev)
        with torch.no_grad():
            logits = model(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, return_masks=True,
                           scene_graphs=d.scene_graphs(), seed=3)[0]
        label = logits.argmax(1)
        label[1::3] = logits.topk(4, 1).indices[1::3, 3]        # a third of the answers sit at rank 3: hits at 5, not at 1
        label[2::3] = logits.argmin(1)[2::3]
        label[0] = -100 if i == 0 else label[0]                 # one ignored row
        inputs = dict(node_embeddings=d.x, edge_index=d.edge_index, edge_embeddings=d.edge_attr, batch=d.batch, questions=d.questions,
                      qsts_att_mask=d.att_mask, return_masks=True, scene_graphs=d.scene_graphs())
        batches.append((inputs, label, qt.encode(types[i])))
    rec = Recorder(model)
    train.validate(rec, batches, train.TypedMeters(dev, qt, k=5), seed=3)          # warm: plans, derived weights
    seen.clear()
    ops.check_plans()
    _, control = _sync_warnings(lambda: float(torch.zeros(1, device=dev)[0]))
    assert control, "torch's sync debug mode did not report a .item()"
    plain, typed = train.Meters(dev), train.TypedMeters(dev, qt, k=5)
    _, syncs_plain = _sync_warnings(lambda: train.validate(rec, [b[:2] for b in batches], plain, seed=3))
    seen.clear()
    ops.reset_counters()
    _, syncs_typed = _sync_warnings(lambda: train.validate(rec, batches, typed, seed=3))
    assert len(syncs_typed) == len(syncs_plain), f"the typed pass waits for the device where the plain one does not: {syncs_typed[:3]}"
    assert ops.counters()["eval_groups"] == 2
    rep, copies = _sync_warnings(typed.report)
    assert len(copies) == 1, f"report() is one device-to-host copy: {copies}"
    # the restatement, fed with the forward's logits
    want, want_all, n_rows, hits = None, None, 0, {1: 0, 5: 0}
    for logits, (_, label, groups) in zip(seen, batches):
        x, lab = logits.cpu(), label.cpu()
        assert x.size(1) == 1842 and float((x.max(1).values - x.min(1).values).max()) <= 32.0
        row_loss = torch.nn.functional.cross_entropy(x.double(), lab, reduction="none").float()
        rank = restate_rank(x, lab)
        want = add_group_meters(want, row_loss, rank, groups, qt.num_groups, 5)
        n_rows += len(lab)
        for k in hits:
            hits[k] += int(((rank >= 0) & (rank < k)).sum())
    plain_rep = plain.report()
    assert {k: rep[k] for k in plain_rep} == plain_rep and rep["rows"] == n_rows == 15
    assert rep["acc1"] == 100.0 * hits[1] / 15 and rep["acc@5"] == 100.0 * hits[5] / 15 and hits[1] < hits[5] < 15
    for g, (facet, name) in enumerate(qt.group_names):
        got = rep["by_type"][facet][name]
        rows, loss, bad, hit1, hitk = want[g, :5].tolist()
        assert (got["rows"], got["acc1"], got["acc@5"]) == (int(rows), 100.0 * hit1 / rows if rows else 0.0,
                                                            100.0 * hitk / rows if rows else 0.0), (facet, name)
        # a row's loss on the device: 29 fp32 terms per lane, each exp within 2 ulp of an argument rounded once (|x - max| <= 32
        # here), so the sum is within (29 + 2 + 16) * 2^-23 relative and its logarithm within that absolutely; then one rounding to
        # fp32.  The mean of a group's rows is no further from the float64 mean than one row is.
        mean = loss / rows if rows else 0.0
        assert abs(got["loss"] - mean) <= 47 * 2.0 ** -23 + mean * 2.0 ** -23, (facet, name, got["loss"], mean)
    assert rep["by_type"]["structural"]["compare"] == {"loss": 0.0, "acc1": 0.0, "acc@5": 0.0, "rows": 0}
    assert sum(v["rows"] for v in rep["by_type"]["structural"].values()) == 14          # every counted row once; one is ignored
    assert sum(v["rows"] for v in rep["by_type"]["semantic"].values()) == 13            # ... and one has no semantic type
    assert typed.status.tolist() == [0, 0]


def _subset(wl, rows):
    """The graphs `rows` of a host FullWorkload, renumbered: what a batch of those questions alone would hold."""
    from isubgvqa_amd import synthetic
    rows = torch.tensor(rows, dtype=torch.long)
    new_id = torch.full((wl.questions.size(0),), -1, dtype=torch.long)
    new_id[rows] = torch.arange(len(rows))
    keep = new_id[wl.batch] >= 0
    node_new = torch.cumsum(keep.long(), 0) - 1
    ekeep = keep[wl.edge_index[0]] & keep[wl.edge_index[1]]
    return synthetic.FullWorkload(wl.x[keep], node_new[wl.edge_index[:, ekeep]], wl.edge_attr[ekeep], new_id[wl.batch[keep]],
                                  wl.x_bbox[keep], wl.added_sym_edge[:0], wl.questions[rows], wl.att_mask[rows], 0, 0), keep


def _same_figures(a, b):
    same = lambda u, v: u == v or (u != u and v != v)
    pa, pb = a.as_printed_by_reference(), b.as_printed_by_reference()
    return a.totals == b.totals and all(same(pa[k], pb[k]) for k in pa) and all(
        same(getattr(a, f), getattr(b, f)) for f in ("accuracy", "accuracy_at", "ans_tok_coo", "qst_tok_coo", "text_tok_coo"))


def test_evaluate_by_type_equals_evaluate_on_every_subset(dev):
    """A stand-in for a --text_sampling model (fixed logits, node masks and token masks), so that a subset of the questions can be
    evaluated alone on the same outputs."""
    from isubgvqa_amd import explain, synthetic
    from isubgvqa_amd.datasets import QuestionTypes
    vocab, classes = 64, 10
    host = [synthetic.make_full_workload(5, tokens=8, seed=81, text_vocab=vocab, sg_vocab=120),
            synthetic.make_full_workload(8, tokens=8, seed=82, text_vocab=vocab, sg_vocab=120)]
    tables = _made_up_tables(classes, 120, vocab)
    types = [_types(5, 3), _types(8, 4, drop=(1,))]
    qt = QuestionTypes(names={"structural": ["query", "verify", "choose", "logical", "compare"], "semantic": ["attr", "rel", "obj"]})
    gen = torch.Generator().manual_seed(83)
    outs, batches, parts = [], [], []
    for i, wl in enumerate(host):
        B, N = wl.questions.size(0), wl.x.size(0)
        wl.x[:, 0] = 5 * torch.randint(0, 24, (N,), generator=gen)            # names the CLIP words can hit
        wl.questions = torch.randint(0, 24, wl.questions.shape, generator=gen)
        logits = torch.randn(B, classes, generator=gen)
        mask = _pick([0.0, 1.0], (N, 1), gen)
        mask_text = _pick([1.0, 1.0, 0.0], (1, B, 8, 1), gen)
        label = torch.where(torch.rand(B, generator=gen) < 0.7, logits.argmax(1), torch.zeros(B, dtype=torch.long))
        qtok, qflags = tables.question_words(_questions(wl, seed=90 + i), dev)
        outs.append(tuple(t.to(dev) for t in (logits, mask)) + (None, None, mask_text.to(dev)))
        batches.append(explain.EvalBatch(wl.to(dev), label.to(dev), qtok, qflags, groups=qt.encode(types[i])))
        parts.append((wl, logits, mask, mask_text, label, qtok, qflags))

    def run(**kw):
        it = iter(outs)
        return _sync_warnings(lambda: explain.evaluate(lambda *a, **k: next(it), batches, tables, **kw))

    run(types=qt)                                               # warm: the tables' device copies
    report, waits = run(types=qt)
    plain, waits_plain = run()
    assert len(waits) == len(waits_plain), f"by_type costs a second device-to-host copy: {waits}"
    assert plain.by_type is None and _same_figures(plain, report), "types=... does not change the overall report"
    assert report.totals[0] == 13 and set(report.by_type) == {"structural", "semantic"}
    for g, (facet, name) in enumerate(qt.group_names):
        sub_outs, sub_batches = [], []
        for i, (wl, logits, mask, mask_text, label, qtok, qflags) in enumerate(parts):
            rows = [q for q, t in enumerate(types[i]) if t.get(facet) == name]
            if not rows:
                continue
            sub, keep = _subset(wl, rows)
            sub_outs.append((logits[rows].to(dev), mask[keep].to(dev), None, None, mask_text[:, rows].to(dev)))
            sub_batches.append(explain.EvalBatch(sub.to(dev), label[rows].to(dev), qtok[rows].contiguous(), qflags[rows].contiguous()))
        it = iter(sub_outs)
        alone = explain.evaluate(lambda *a, **k: next(it), sub_batches, tables)
        assert _same_figures(report.by_type[facet][name], alone), (facet, name, report.by_type[facet][name].totals[:12], alone.totals[:12])
    assert report.by_type["structural"]["compare"].totals == (0,) * len(report.totals)
    assert sum(r.totals[0] for r in report.by_type["structural"].values()) == 13
    assert sum(r.totals[0] for r in report.by_type["semantic"].values()) == 12
    with pytest.raises(ValueError):
        it2 = iter(outs)
        explain.evaluate(lambda *a, **k: next(it2), [b._replace(groups=None) for b in batches], tables, types=qt)
