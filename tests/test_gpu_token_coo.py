"""isg_token_coo / ops.token_coo / explain.evaluate on the GPU.  Every output is an integer: the table and the totals are compared
EXACTLY with the plain-Python restatement of tests/token_coo_restated.py (itself held to the reference's functions on strings by
tests/test_token_coo_cpu.py).  Sizes sit on the boundaries of a wave (64), of the chunk of C = ops.COO_NODE_CHUNK nodes the kernel
stages per pass, of the totals workgroup (256 rows per pass) and of the token tables (two tokens per lane: 64, 128)."""
import itertools

import pytest
import torch

from token_coo_restated import add_totals, restate_table

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
VOCAB, A = 40, 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _ptr(sizes):
    return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int32)


def _plan(sizes, dev):
    """A GraphPlan with what the scoring reads (ptr): built by hand, since graphs here may exceed what the model kernels take."""
    from isubgvqa_amd import ops
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long))
    return ops.GraphPlan(N=int(sum(sizes)), E=0, B=len(sizes), ptr=_ptr(sizes).to(dev),
                         nmax_dev=torch.zeros(1, dtype=torch.int32, device=dev), nmax=0, batch=batch.to(dev))


def _pick(values, shape, gen):
    values = torch.tensor(values)
    return values[torch.randint(0, values.numel(), shape, generator=gen)]


def _random_case(sizes, T, T2, seed):
    """A batch on the host: names from a vocabulary of 40 (so words repeat and several nodes share a name), masks with un-kept,
    negative and NaN entries, answers in and out of [0, A), tokens with -1 and ids no node has, token masks of 1, 0, 0.999, NaN."""
    gen = torch.Generator().manual_seed(seed)
    N, B = int(sum(sizes)), len(sizes)
    x = torch.randint(0, VOCAB, (N, 4), generator=gen)
    pred = torch.randint(-1, A + 2, (B,), generator=gen)
    label = torch.where(torch.rand(B, generator=gen) < 0.6, pred, torch.randint(-1, A + 2, (B,), generator=gen))
    return dict(sizes=list(sizes), x=x, mask=_pick([0.0, 0.0, 1.0, 1.0, 0.3, -1.0, NAN], (N,), gen), pred=pred, label=label,
                ans_sg=torch.randint(-1, VOCAB, (A,), generator=gen).to(torch.int32),
                qtok=torch.randint(-1, VOCAB + 5, (B, T), generator=gen).to(torch.int32),
                qflags=torch.randint(0, 4, (B,), generator=gen).to(torch.int32),
                ttok=torch.randint(-1, VOCAB + 5, (B, T2), generator=gen).to(torch.int32),
                tkeep=_pick([1.0, 1.0, 0.0, 0.999, NAN], (B, T2), gen))


def _restated(c, threshold=0.0, text=True):
    table = restate_table(c["x"][:, 0], c["mask"], _ptr(c["sizes"]), c["pred"], c["label"], c["ans_sg"], c["qtok"],
                          c["ttok"] if text else None, c["tkeep"] if text else None, threshold)
    return table, add_totals(None, table, c["qflags"])


def _run(c, dev, threshold=0.0, totals=None, text=True, names=None, qflags=True):
    from isubgvqa_amd import ops
    x = c["x"].to(dev)
    give = lambda t: t.to(dev) if t.size(1) else None          # an EMPTY table is not given
    return ops.token_coo(x[:, 0] if names is None else names, c["mask"].to(dev), _plan(c["sizes"], dev), c["pred"].to(dev),
                         c["label"].to(dev), c["ans_sg"].to(dev), give(c["qtok"]), c["qflags"].to(dev) if qflags else None,
                         give(c["ttok"]) if text else None, give(c["tkeep"]) if text else None, threshold=threshold, totals=totals)


def _check(c, dev, threshold=0.0, what=""):
    """Table and totals of one call against the restatement, exactly; the table also without totals."""
    from isubgvqa_amd import ops
    want_table, want_totals = _restated(c, threshold)
    totals = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    out = _run(c, dev, threshold, totals)
    assert out.totals is totals and out.table.dtype == torch.int32 and tuple(out.table.shape) == (len(c["sizes"]), 8)
    bad = (out.table.cpu() != want_table).any(1).nonzero().view(-1).tolist()
    assert not bad, (what, "rows", bad[:5], out.table.cpu()[bad[:5]].tolist(), want_table[bad[:5]].tolist())
    got = totals.tolist()
    assert got == want_totals, (what, [(i, g, w) for i, (g, w) in enumerate(zip(got, want_totals)) if g != w][:8])
    assert got[12:16] == [0, 0, 0, 0]
    alone = _run(c, dev, threshold, None)
    assert alone.totals is None and torch.equal(alone.table, out.table)
    return out.table.cpu(), got


def _sizes(B, seed, top=12):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, top + 1, (B,), generator=gen).tolist()
    sizes[B // 2] = 0
    return sizes


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last_kept", [True, False])
def test_graph_sizes_on_the_chunk_boundaries_with_the_only_match_in_the_last_node(dev, last_kept):
    from isubgvqa_amd import ops
    C = ops.COO_NODE_CHUNK
    assert C % 64 == 0
    sizes = [0, 1, 63, 64, 65, C - 1, C, C + 1, 0, 2 * C + 1, 3 * C]
    B, N = len(sizes), sum(sizes)
    ptr = _ptr(sizes).tolist()
    x = torch.full((N, 4), 7)                                  # a name no token has
    mask = torch.ones(N)
    for g in range(B):
        if sizes[g]:
            x[ptr[g + 1] - 1, 0] = 100 + g                     # the only match: the last node of the last chunk
            mask[ptr[g + 1] - 1] = 1.0 if last_kept else 0.0
    c = dict(sizes=sizes, x=x, mask=mask, pred=torch.arange(B), label=torch.arange(B), ans_sg=(100 + torch.arange(B)).to(torch.int32),
             qtok=torch.stack([100 + torch.arange(B), torch.full((B,), 5)], 1).to(torch.int32), qflags=torch.zeros(B, dtype=torch.int32),
             ttok=torch.stack([torch.full((B,), 5), 100 + torch.arange(B), 100 + torch.arange(B)], 1).to(torch.int32),
             tkeep=torch.ones(B, 3))
    table, totals = _check(c, dev)
    k = int(last_kept)
    for g in range(B):
        assert table[g].tolist() == ([1, 1, 1, k, 1, k, 2, 2 * k] if sizes[g] else [1, 0, 0, 0, 0, 0, 0, 0]), (g, sizes[g])
    some = sum(1 for s in sizes if s)
    assert totals[:12] == [B, B, some, some, some, some * k, some, some, some * k, some, 2 * some, 2 * some * k]
    # the same graphs with random names, masks and tokens
    r = _random_case(sizes, 9, 7, seed=3)
    _check(r, dev, what="random names on the chunk boundaries")


@pytest.mark.parametrize("B", [3, 4, 5, 255, 256, 257, 1025])
def test_batch_sizes_around_the_totals_workgroup(dev, B):
    c = _random_case(_sizes(B, seed=B), 6, 4, seed=100 + B)
    table, totals = _check(c, dev, what=f"B={B}")
    assert totals[0] == B and (B < 255 or (0 < totals[1] < B and totals[4] > 0 and totals[8] > 0 and totals[11] > 0))


@pytest.mark.parametrize("T,T2", [(0, 65), (1, 127), (63, 128), (64, 0), (65, 1), (127, 63), (128, 64), (128, 128), (0, 0)])
def test_token_counts_on_the_lane_boundaries(dev, T, T2):
    c = _random_case(_sizes(7, seed=T + T2, top=30), T, T2, seed=200 + 3 * T + T2)
    table, totals = _check(c, dev, what=f"T={T} T2={T2}")
    assert table[:, 4].max() <= T and table[:, 6].max() <= T2
    if T >= 63:
        assert table[:, 4].max() > 2                           # words repeat over a vocabulary of 40: each occurrence counts


def test_more_tokens_than_the_tables_hold_are_refused(dev):
    from isubgvqa_amd import _lib, ops
    c = _random_case([3, 4], ops.COO_TOKENS_MAX + 1, 2, seed=5)
    with pytest.raises(_lib.IsgError, match="status -2"):
        _run(c, dev)
    c = _random_case([3, 4], 2, ops.COO_TOKENS_MAX + 1, seed=6)
    with pytest.raises(_lib.IsgError, match="status -2"):
        _run(c, dev)


def test_duplicates_unkept_names_shared_names_and_negative_ids(dev):
    """Graph 0: name 5 on three nodes of which one is kept (counts as kept), name 9 only on an un-kept node, a NEGATIVE name
    against a -1 token, a name beyond int32 whose low 32 bits equal a token.  Graph 1 has nodes but none matches; graph 2: answers
    out of [0, A) on both sides are equal, and name nothing."""
    big = (1 << 32) + 3
    sizes = [7, 2, 1]
    x = torch.zeros(10, 4, dtype=torch.long)
    x[:, 0] = torch.tensor([5, 5, 5, 9, -1, big, -2, 30, 31, 3])
    mask = torch.tensor([0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    qtok = torch.tensor([[5, 5, 9, -1, 3, -2, 5, 8], [5, 9, 3, -1, -1, -1, -1, -1], [3, 3, -1, 5, -1, -1, -1, -1]], dtype=torch.int32)
    ans_sg = torch.tensor([9, 5, -1, 3], dtype=torch.int32)
    c = dict(sizes=sizes, x=x, mask=mask, pred=torch.tensor([0, 2, -5]), label=torch.tensor([1, 2, 4]), ans_sg=ans_sg, qtok=qtok,
             qflags=torch.tensor([0, 1, 2], dtype=torch.int32), ttok=qtok[:, :3].contiguous(),
             tkeep=torch.tensor([[1.0, 0.999, 1.0], [1.0, 1.0, 1.0], [NAN, 1.0, 0.0]]))
    table, totals = _check(c, dev)
    assert table.tolist() == [[0, 1, 1, 0, 4, 3, 2, 1],          # pred 9 (un-kept only), label 5; words 5, 5, 9, 5 / 5, 5, 5; text 5, 9 / 5
                              [1, 0, 0, 0, 0, 0, 0, 0],          # ans_sg[2] = -1 names nothing
                              [0, 0, 0, 0, 2, 2, 1, 1]]          # -5 != 4 although both are out of range; text: only the middle 3
    assert totals[:12] == [3, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("threshold", [0.0, 0.5, -1.0])
def test_threshold_is_strict_and_a_nan_is_not_kept(dev, threshold):
    special = [threshold, -0.0, 0.0, -1.0, INF, -INF, NAN, 0.5, torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)).item(), 2.0,
               torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0)).item()]
    n = len(special)
    x = torch.zeros(n, 4, dtype=torch.long)
    x[:, 0] = torch.arange(n)                                  # every node its own name, every name a question word
    c = dict(sizes=[n], x=x, mask=torch.tensor(special), pred=torch.tensor([0]), label=torch.tensor([0]),
             ans_sg=torch.tensor([0], dtype=torch.int32), qtok=torch.arange(n, dtype=torch.int32).view(1, n),
             qflags=torch.zeros(1, dtype=torch.int32), ttok=torch.zeros(1, 0, dtype=torch.int32), tkeep=torch.zeros(1, 0))
    table, _ = _check(c, dev, threshold)
    above = sum(1 for v in special if v > threshold)           # python's comparison: NaN > t is False
    assert table[0].tolist() == [1, 1, 1, 0, n, above, 0, 0] and 0 < above < n      # node 0 sits ON the threshold: not kept


def test_names_as_a_strided_column_and_as_a_contiguous_copy(dev):
    c = _random_case(_sizes(40, seed=8), 10, 5, seed=9)
    column = c["x"].to(dev)[:, 0]
    assert column.stride(0) == 4 and not column.is_contiguous()
    a, b = _run(c, dev, names=column), _run(c, dev, names=column.contiguous())
    assert torch.equal(a.table, b.table) and torch.equal(a.table.cpu(), _restated(c)[0])
    wide = torch.cat([torch.full((c["x"].size(0), 3), 3), c["x"][:, :1], torch.full((c["x"].size(0), 5), 3)], 1).to(dev)      # stride 9
    assert torch.equal(_run(c, dev, names=wide[:, 3]).table, a.table)


def test_two_calls_on_two_halves_add_up_to_one_call_on_the_whole(dev):
    from isubgvqa_amd import ops
    B, cut = 300, 137
    c = _random_case(_sizes(B, seed=10), 6, 4, seed=11)
    whole = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    full = _run(c, dev, totals=whole)
    n = sum(c["sizes"][:cut])
    halves = []
    for rows, nodes in ((slice(0, cut), slice(0, n)), (slice(cut, B), slice(n, None))):
        halves.append({k: (c[k][nodes] if k in ("x", "mask") else c[k] if k == "ans_sg" else c[k][rows]) for k in c})
    parts = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    tables = [_run(h, dev, totals=parts).table for h in halves]
    assert torch.equal(torch.cat(tables), full.table)
    assert torch.equal(parts, whole) and whole.tolist() == _restated(c)[1]
    again = _run(c, dev, totals=whole)                         # the call ADDS
    assert torch.equal(whole, 2 * parts) and torch.equal(again.table, full.table)


def test_optional_tables_may_be_left_out(dev):
    from isubgvqa_amd import ops
    c = _random_case(_sizes(20, seed=12), 5, 4, seed=13)
    want_table, _ = _restated(c, text=False)
    totals = torch.zeros(ops.COO_TOTALS, dtype=torch.int64, device=dev)
    out = _run(c, dev, totals=totals, text=False, qflags=False)
    assert torch.equal(out.table.cpu(), want_table) and (want_table[:, 6:] == 0).all()
    assert totals.tolist() == add_totals(None, want_table, None)
    none = dict(c, qtok=c["qtok"][:, :0], ttok=c["ttok"][:, :0], tkeep=c["tkeep"][:, :0])
    table, got = _check(none, dev)
    assert (table[:, 4:] == 0).all() and got[6:12] == [0] * 6 and sum(got[16:]) == 0


def test_nothing_is_written_beyond_the_table_and_the_totals(dev):
    """The C ABI on buffers with a guard behind them: without totals only the table changes; with totals every entry but the
    reserved four has the batch added (to whatever it held), and neither guard is touched."""
    from isubgvqa_amd import _lib, ops
    lib = _lib.load()
    c = _random_case(_sizes(70, seed=14), 5, 4, seed=15)
    B, N, G = 70, sum(c["sizes"]), 64
    d = {k: v.to(dev) for k, v in c.items() if k != "sizes"}
    names = d["x"][:, 0].contiguous()
    ptr = _ptr(c["sizes"]).to(dev)
    table = torch.full((B * 8 + G,), -7, dtype=torch.int32, device=dev)
    totals = torch.full((ops.COO_TOTALS + G,), 1000, dtype=torch.int64, device=dev)

    def call(with_totals):
        torch.cuda.synchronize()
        rc = lib.isg_token_coo(names.data_ptr(), 1, d["mask"].data_ptr(), 0.0, ptr.data_ptr(), d["pred"].data_ptr(), d["label"].data_ptr(),
                               d["ans_sg"].data_ptr(), d["qtok"].data_ptr(), d["qflags"].data_ptr(), d["ttok"].data_ptr(),
                               d["tkeep"].data_ptr(), N, B, A, 5, 4, table.data_ptr(), totals.data_ptr() if with_totals else None,
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    want_table, want_totals = _restated(c)
    assert call(False) == 0
    assert torch.equal(table[:B * 8].view(B, 8).cpu(), want_table) and (table[B * 8:] == -7).all() and (totals == 1000).all()
    table.fill_(-7)
    assert call(True) == 0
    assert torch.equal(table[:B * 8].view(B, 8).cpu(), want_table) and (table[B * 8:] == -7).all()
    assert totals[:ops.COO_TOTALS].tolist() == [1000 + w for w in want_totals] and (totals[ops.COO_TOTALS:] == 1000).all()
    assert want_totals[12:16] == [0, 0, 0, 0]                  # the reserved four: never written, so still what they held


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """A model as explain.evaluate calls it, keeping what every forward returned."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __call__(self, *args, **kwargs):
        out = self.model(*args, **kwargs)
        self.seen.append(tuple(None if t is None or not torch.is_tensor(t) else t.detach().cpu().clone() for t in out))
        return out


def _made_up_tables(classes, sg_vocab, text_vocab=None):
    """A vocabulary over the synthetic ids: name id i is the word `w<i>`; every third answer class is a word, the others are not
    vocabulary tokens; CLIP token t is the word of name id 5 t (where there is one)."""
    from isubgvqa_amd import explain
    stoi = {f"w{i}": i for i in range(sg_vocab)}
    answers = [f"w{(11 * a) % sg_vocab}" if a % 3 == 0 else f"answer {a}" for a in range(classes)]
    clip = None if text_vocab is None else [f"w{5 * t}</w>" for t in range(text_vocab)]
    return explain.TokenTables(stoi, answers, clip)


def _questions(wl, seed):
    """A question per graph that names two of its nodes (one twice), a word no graph has and, in every third, `color`."""
    gen = torch.Generator().manual_seed(seed)
    ptr = _ptr(torch.bincount(wl.batch, minlength=wl.questions.size(0)).tolist()).tolist()
    out = []
    for g in range(len(ptr) - 1):
        pick = lambda: int(wl.x[torch.randint(ptr[g], ptr[g + 1], (1,), generator=gen), 0])
        a, b = pick(), pick()
        out.append(f"Is the w{a} near the  w{b} or the W{a}{' in color' if g % 3 == 0 else ''}? w{b} GT")
    return out


def _restate_evaluation(seen, batches, host, tables, ttoks=None):
    totals = None
    for i, (out, b, wl) in enumerate(zip(seen, batches, host)):
        B = b.label.numel()
        ptr = _ptr(torch.bincount(wl.batch, minlength=B).tolist())
        text = (None, None) if out[4] is None else (ttoks[i], out[4].reshape(B, -1))
        table = restate_table(wl.x[:, 0], out[1], ptr, out[0].argmax(1), b.label.cpu(), tables.ans_sg, b.qtok.cpu(), *text)
        totals = add_totals(totals, table, b.qflags.cpu())
    return totals


def test_evaluate_equals_the_restatement_on_the_same_forwards(dev):
    from isubgvqa_amd import explain, ops, synthetic
    from isubgvqa_amd.models import build_model
    vocab = 2048
    torch.manual_seed(0)
    model = build_model(synthetic.full_model_args(text_vocab_size=vocab), None).to(dev).eval()
    host = [synthetic.make_full_workload(6, tokens=8, seed=61, text_vocab=vocab, sg_vocab=300),
            synthetic.make_full_workload(9, tokens=8, seed=62, text_vocab=vocab, sg_vocab=300)]
    batches = []
    with torch.no_grad():
        for i, wl in enumerate(host):
            d = wl.to(dev)
            logits = model(d.x, d.edge_index, d.edge_attr, d.batch, d.questions, d.att_mask, return_masks=True, scene_graphs=d.scene_graphs())[0]
            classes = logits.size(1)
            tables = _made_up_tables(classes, 300)
            # the true answer: the prediction for two questions of three, and a class whose name is a node of the graph for some
            label = logits.argmax(1).cpu()
            label[2::3] = (label[2::3] + 1) % classes
            qtok, qflags = tables.question_words(_questions(wl, seed=70 + i), dev)
            batches.append(explain.EvalBatch(d, label.to(dev), qtok, qflags))
    rec = _Recorder(model)
    report = explain.evaluate(rec, batches, tables)
    ops.check_plans()
    assert len(rec.seen) == 2 and rec.seen[0][4] is None
    want = _restate_evaluation(rec.seen, batches, host, tables)
    assert list(report.totals) == want
    assert want[0] == 15 and 0 < want[1] < 15 and want[6] > 0 and want[7] >= 3 * want[6]      # three matching words per question
    assert report.accuracy == want[1] / 15 and 0.0 <= report.qst_tok_coo <= 1.0 and report.text_tok_coo != report.text_tok_coo


def test_evaluate_scores_the_text_explanation_of_a_forward_that_returns_one(dev):
    """A stand-in for a --text_sampling model: fixed logits, node masks and token masks of the right shapes."""
    from isubgvqa_amd import explain, synthetic
    vocab, classes = 64, 10
    host = [synthetic.make_full_workload(5, tokens=8, seed=81, text_vocab=vocab, sg_vocab=120),
            synthetic.make_full_workload(8, tokens=8, seed=82, text_vocab=vocab, sg_vocab=120)]
    tables = _made_up_tables(classes, 120, vocab)
    gen = torch.Generator().manual_seed(83)
    outs, batches, ttoks = [], [], []
    for i, wl in enumerate(host):
        B, N = wl.questions.size(0), wl.x.size(0)
        wl.x[:, 0] = 5 * torch.randint(0, 24, (N,), generator=gen)            # names the CLIP words can hit
        wl.questions = torch.randint(0, 24, wl.questions.shape, generator=gen)
        logits = torch.randn(B, classes, generator=gen)
        mask = _pick([0.0, 1.0], (N, 1), gen)
        mask_text = _pick([1.0, 1.0, 0.0], (1, B, 8, 1), gen)
        outs.append(tuple(t.to(dev) for t in (logits, mask)) + (None, None, mask_text.to(dev)))
        label = torch.where(torch.rand(B, generator=gen) < 0.7, logits.argmax(1), torch.zeros(B, dtype=torch.long))
        qtok, qflags = tables.question_words(_questions(wl, seed=90 + i), dev)
        batches.append(explain.EvalBatch(wl.to(dev), label.to(dev), qtok, qflags))
        ttoks.append(tables.clip_sg[wl.questions])
    replay = iter(outs)
    rec = _Recorder(lambda *args, **kwargs: next(replay))
    report = explain.evaluate(rec, batches, tables)
    want = _restate_evaluation(rec.seen, batches, host, tables, ttoks)
    assert list(report.totals) == want and want[9] > 0 and 0 < want[11] < want[10]
    assert 0.0 < report.text_tok_coo < 1.0 and report.as_printed_by_reference()["Qst. Text Tok. Coo"] == report.text_tok_coo
