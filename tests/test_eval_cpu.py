"""Host-side checks of the evaluation by question type (include/isg_eval.h) that need no GPU: the header declares
exactly the new entry points and the library exports them; the entry points refuse bad arguments before any HIP call;
datasets.gqa.QuestionTypes; train.TypedMeters.summarize; explain.EvalBatch without groups; train.validate with plain Meters; and
the restatement of tests/eval_restated.py on cases written out by hand."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT
from eval_restated import add_coo_groups, add_group_meters, bad_ids, restate_rank, restate_top
from token_coo_restated import HIST, TOTALS, add_totals

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
NAMES = {"isg_eval_abi_version", "isg_answer_rank", "isg_group_meters_parts", "isg_group_meters", "isg_token_coo_groups"}
NAN, INF = float("nan"), float("inf")


def test_eval_header_parses_binds_and_is_exported():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib, _lib_eval, _lib_instances, _lib_optim, loader, ops
    path = os.path.join(ROOT, "include", "isg_eval.h")
    declared = set(loader.declared_symbols(path))
    assert declared == set(_lib_eval.SIGNATURES) == NAMES
    for other in (_lib, _lib_optim, _lib_instances):
        assert not declared & set(other.SIGNATURES), "a symbol is declared in two headers"
    abi = int(re.search(r"#define ISG_EVAL_ABI_VERSION (\d+)", open(path).read()).group(1))
    assert _lib_eval.load().isg_eval_abi_version() == _lib_eval.ABI_VERSION == abi == 1
    for lib_path in (_lib.LIB_PATH, ge.STRICT_LIB):           # the product library and its strict twin export every one
        raw = ctypes.CDLL(lib_path)
        for name in declared:
            assert hasattr(raw, name), (lib_path, name)
        raw.isg_eval_abi_version.restype = ctypes.c_int
        assert raw.isg_eval_abi_version() == 1, lib_path
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    # (logits, ld, labels, ignore_index, row_lse, rank, top_ids, top_prob, K, B, A, stream)
    assert _lib_eval.SIGNATURES["isg_answer_rank"] == (ctypes.c_int, [ptr, i32, ptr, i64, ptr, ptr, ptr, ptr, i32, i64, i32, ptr])
    assert _lib_eval.SIGNATURES["isg_group_meters_parts"] == (i64, [i64, i32])
    # (row_loss, rank, groups, F, G, k, totals, overall, parts, parts_len, status, B, stream)
    assert _lib_eval.SIGNATURES["isg_group_meters"] == (ctypes.c_int, [ptr, ptr, ptr, i32, i32, i32, ptr, ptr, ptr, i64, ptr, i64, ptr])
    # (table, qflags, groups, F, G, totals, status, B, stream)
    assert _lib_eval.SIGNATURES["isg_token_coo_groups"] == (ctypes.c_int, [ptr, ptr, ptr, i32, i32, ptr, ptr, i64, ptr])
    build_checks("isg_eval.h")
    assert "_smoke_eval(dev)" in inspect.getsource(ge.smoke)
    assert "eval_groups" in ops.COUNTERS
    assert (ops.EVAL_TOPK_MAX, ops.EVAL_FACETS_MAX, ops.EVAL_GROUPS_MAX, ops.GROUP_SLOTS) == (8, 4, 256, 8)
    # the rules of include/isg_optim.h: integer LDS atomics only -- no atomic takes a floating-point operand, none a global address
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_eval.hip")).read())
    atomics = re.findall(r"atomic\w+\(([^;]*);", text)
    assert atomics and all(re.match(r"\s*(&?s_|&hist\[|s_bad|s_first)", a) for a in atomics), atomics
    assert "isg_xent_fwd" not in text and "token_coo_totals_kernel" not in text


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from isubgvqa_amd import _lib_eval
    lib = _lib_eval.load()

    def rank(x=P, ld=10, lab=P, lse=P, rk=P, ids=P, prob=P, K=5, B=3, A=10):
        return lib.isg_answer_rank(x, ld, lab, -100, lse, rk, ids, prob, K, B, A, None)

    for k in ("x", "lab", "rk"):
        assert rank(**{k: None}) == EINVAL, k
    assert rank(lse=None) == EINVAL                            # probabilities without the log-sum-exp
    assert rank(B=-1) == EINVAL and rank(A=0) == EINVAL and rank(ld=9) == EINVAL
    assert rank(K=0) == EINVAL and rank(K=9) == EINVAL and rank(K=-1) == EINVAL
    assert rank(B=1 << 31) == EUNSUPPORTED
    assert rank(B=0) == 0 and rank(B=0, x=None, lab=None, rk=None, ids=None, prob=None, lse=None, K=0) == 0
    assert rank(B=0, A=0) == EINVAL

    assert lib.isg_group_meters_parts(0, 7) == 7 * 5 + 7 == lib.isg_group_meters_parts(64, 7) and lib.isg_group_meters_parts(65, 7) == 84
    assert lib.isg_group_meters_parts(257, 256) == 5 * (256 * 5 + 7)                # a partial table per 64 rows
    assert lib.isg_group_meters_parts(-1, 7) == 0 and lib.isg_group_meters_parts(5, 0) == 0 and lib.isg_group_meters_parts(5, 257) == 0

    def meters(loss=P, rk=P, groups=P, F=2, G=7, k=5, totals=P, overall=P, parts=P, n=210, status=P, B=300):
        return lib.isg_group_meters(loss, rk, groups, F, G, k, totals, overall, parts, n, status, B, None)

    for k in ("loss", "rk", "groups", "totals", "parts"):
        assert meters(**{k: None}) == EINVAL, k
    assert meters(F=0) == EINVAL and meters(F=5) == EINVAL and meters(G=0) == EINVAL and meters(G=257) == EINVAL
    assert meters(k=0) == EINVAL and meters(B=-1) == EINVAL
    assert meters(n=209) == EWORKSPACE and meters(B=1 << 31) == EUNSUPPORTED
    assert meters(B=0) == 0 and meters(B=0, loss=None, rk=None, groups=None, totals=None, parts=None, n=0, status=None, overall=None) == 0

    def coo(table=P, qflags=P, groups=P, F=2, G=7, totals=P, status=P, B=300):
        return lib.isg_token_coo_groups(table, qflags, groups, F, G, totals, status, B, None)

    for k in ("table", "groups", "totals"):
        assert coo(**{k: None}) == EINVAL, k
    assert coo(F=0) == EINVAL and coo(F=5) == EINVAL and coo(G=0) == EINVAL and coo(G=257) == EINVAL and coo(B=-1) == EINVAL
    assert coo(B=(1 << 31) - 1) == EUNSUPPORTED
    assert coo(B=0) == 0 and coo(B=0, table=None, qflags=None, groups=None, totals=None, status=None) == 0


def test_ops_refuse_host_tensors_and_bad_shapes():
    from isubgvqa_amd import _lib, ops
    x, lab = torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.IsgError):
        ops.answer_rank(x, lab)                               # no CPU fallback
    with pytest.raises(ValueError):
        ops.group_meters(torch.zeros(3), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 5, dtype=torch.int32),
                         torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.token_coo_groups(torch.zeros(3, 8, dtype=torch.int32), None, torch.zeros(3, 1, dtype=torch.int32),
                             torch.zeros(2, 9, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# QuestionTypes
# ---------------------------------------------------------------------------------------------------------------------
TYPES = [{"structural": "query", "semantic": "attr", "detailed": "d1"}, {"structural": "verify", "semantic": "rel", "detailed": "d2"},
         {"structural": "query", "semantic": "obj", "detailed": "d1"}, {"structural": "choose", "semantic": "attr", "detailed": "d3"}]


def test_question_types_number_names_in_order_of_first_occurrence():
    from isubgvqa_amd.datasets import QuestionTypes
    from isubgvqa_amd.datasets.gqa import QuestionTypes as same
    assert QuestionTypes is same
    qt = QuestionTypes().fit(TYPES)
    assert qt.facets == ("structural", "semantic") and qt.num_groups == 6
    assert qt.group_names == [("structural", "query"), ("structural", "verify"), ("structural", "choose"), ("semantic", "attr"),
                              ("semantic", "rel"), ("semantic", "obj")]
    enc = qt.encode(TYPES)
    assert enc.dtype == torch.int32 and enc.tolist() == [[0, 3], [1, 4], [0, 5], [2, 3]]
    assert enc.is_pinned() == torch.cuda.is_available()
    empty = qt.encode([])
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.int32


def test_question_types_given_names_unknown_strings_and_missing_keys():
    from isubgvqa_amd.datasets import QuestionTypes
    qt = QuestionTypes(names={"structural": ["verify", "query"], "semantic": ["rel"]})
    assert qt.num_groups == 3 and qt.group_names == [("structural", "verify"), ("structural", "query"), ("semantic", "rel")]
    enc = qt.encode(TYPES + [{"semantic": "rel"}, {}, {"structural": "never seen", "semantic": None}, None])
    assert enc.tolist() == [[1, -1], [0, 2], [1, -1], [-1, -1], [-1, 2], [-1, -1], [-1, -1], [-1, -1]]
    three = QuestionTypes(facets=("structural", "semantic", "detailed")).fit(TYPES)
    ids = three.encode(TYPES)
    assert three.num_groups == 9 and ids[:, 2].tolist() == [6, 7, 6, 8]
    per_facet = [set(ids[:, f].tolist()) for f in range(3)]
    assert not (per_facet[0] & per_facet[1] or per_facet[0] & per_facet[2] or per_facet[1] & per_facet[2]), "two facets share an id"
    with pytest.raises(ValueError):
        QuestionTypes(facets=("a", "b", "c", "d", "e"))
    with pytest.raises(ValueError):
        QuestionTypes(facets=("detailed",)).fit([{"detailed": f"d{i}"} for i in range(257)])


def test_gqa_collate_hands_on_what_encode_takes():
    from isubgvqa_amd.datasets import QuestionTypes, gqa_collate

    class Graphs:
        def collate(self, ids, pin_memory, distinct=False):
            return list(ids)

    data = [(f"q{i}", 10 + i, "what", t, i, 10 + i) for i, t in enumerate(TYPES)]
    out = gqa_collate(data, Graphs())
    assert len(out) == 7 and out[6] == tuple(TYPES)
    assert QuestionTypes().fit(TYPES).encode(out[6]).tolist() == [[0, 3], [1, 4], [0, 5], [2, 3]]


# ---------------------------------------------------------------------------------------------------------------------
# TypedMeters, EvalBatch, validate
# ---------------------------------------------------------------------------------------------------------------------
def test_typed_meters_summarize_from_a_table_made_by_hand():
    from isubgvqa_amd import train
    from isubgvqa_amd.datasets import QuestionTypes
    qt = QuestionTypes(names={"structural": ["query", "verify"], "semantic": ["attr"]})
    m = train.TypedMeters(torch.device("cpu"), qt, k=5)
    assert isinstance(m, train.Meters) and tuple(m.totals.shape) == (8,) and tuple(m.groups.shape) == (3, 8)
    assert m.totals.dtype == m.groups.dtype == torch.float64 and m.totals.is_contiguous() and m.groups.is_contiguous()
    assert m.totals.data_ptr() + 16 * 8 == m.groups.data_ptr(), "one allocation: one copy at report()"
    m.totals.copy_(torch.tensor([30.0, 20.0, 5.0, 20.0, 2.0, 0.0, 0.0, 0.0]))
    m.overall.copy_(torch.tensor([18.0, 27.0, 0.0, 5.0, 9.0, 0.0, 0.0, 0.0]))
    m.groups[0].copy_(torch.tensor([8.0, 12.0, 2.0, 2.0, 4.0, 0.0, 0.0, 0.0]))          # two of the eight losses were not finite
    m.groups[2].copy_(torch.tensor([10.0, 15.0, 0.0, 3.0, 5.0, 0.0, 0.0, 0.0]))
    rep = m.report()
    plain = train.Meters.summarize(m.totals.tolist())
    assert {k: rep[k] for k in plain} == plain and set(rep) == set(plain) | {"acc@5", "by_type"}
    assert rep["loss"] == 1.5 and rep["acc1"] == 25.0 and rep["acc@5"] == 45.0 and rep["rows"] == 20
    assert rep["by_type"] == {"structural": {"query": {"loss": 2.0, "acc1": 25.0, "acc@5": 50.0, "rows": 8},
                                             "verify": {"loss": 0.0, "acc1": 0.0, "acc@5": 0.0, "rows": 0}},      # an empty group
                              "semantic": {"attr": {"loss": 1.5, "acc1": 30.0, "acc@5": 50.0, "rows": 10}}}
    assert m.summarize(m._all.tolist()) == rep
    m.reset()
    assert float(m._all.abs().sum()) == 0.0 and m.report()["acc@5"] == 0.0
    assert "acc@3" in train.TypedMeters(torch.device("cpu"), qt, k=3).report()
    with pytest.raises(ValueError):
        train.TypedMeters(torch.device("cpu"), QuestionTypes(), k=5)          # no groups yet


def test_typed_meters_report_over_a_process_group_is_one_all_reduce(tmp_path, monkeypatch):
    import torch.distributed as dist
    from isubgvqa_amd import train
    from isubgvqa_amd.datasets import QuestionTypes
    qt = QuestionTypes(names={"structural": ["query", "verify"], "semantic": ["attr"]})
    m = train.TypedMeters(torch.device("cpu"), qt, k=5)
    m._all.copy_(torch.arange(1, 41, dtype=torch.float64))
    alone = m.report()
    mine = not dist.is_initialized()
    if mine:
        dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        reduced = []
        real = dist.all_reduce
        monkeypatch.setattr(dist, "all_reduce", lambda t, group=None: (reduced.append(t.numel()), real(t, group=group))[1])
        assert m.report(dist.group.WORLD) == alone             # a world of one: the sums are this rank's
        assert reduced == [5 + 8 + 3 * 8], "slots 0-3 and 5, the overall block and the table travel together"
    finally:
        if mine:
            dist.destroy_process_group()


def test_eval_batch_built_without_groups_stays_valid():
    from isubgvqa_amd import explain
    b = explain.EvalBatch("inputs", torch.zeros(2, dtype=torch.int64))
    assert b.groups is None and b.graph_index is None and len(b) == 6 and explain.EvalBatch._fields[-1] == "graph_index"
    old = explain.EvalBatch("inputs", 1, 2, 3, 4, 5)                              # the six positional fields of before
    assert old.graph_index == 5 and old.groups is None and tuple(old) == ("inputs", 1, 2, 3, 4, 5)
    new = explain.EvalBatch("inputs", 1, qflags=3, groups="g")                    # groups: a keyword beside the tuple's fields
    assert new.groups == "g" and new.qflags == 3 and len(new) == 6
    assert new._replace(label=2).groups == "g" and new._replace(groups=None).groups is None and new._replace(groups=None).label == 1
    assert explain.EvalBatch._make(range(6)).groups is None
    assert "types" in inspect.signature(explain.evaluate).parameters
    r = explain.CooReport.from_totals(torch.zeros(TOTALS, dtype=torch.int64))
    assert r.by_type is None and explain.CooReport.from_totals([0] * TOTALS).totals == r.totals == (0,) * TOTALS


def test_validate_with_plain_meters_calls_nothing_new(monkeypatch):
    from isubgvqa_amd import ops, train
    calls = []

    def fake_xent(logits, labels, ignore_index=-100, totals=None):
        calls.append("cross_entropy")
        return ops.CrossEntropy(None, None, torch.zeros(labels.numel()), None, None)

    monkeypatch.setattr(ops, "cross_entropy", fake_xent)
    monkeypatch.setattr(ops, "answer_rank", lambda *a, **k: calls.append("answer_rank"))
    monkeypatch.setattr(ops, "group_meters", lambda *a, **k: calls.append("group_meters"))
    model = torch.nn.Linear(4, 3)
    labels = torch.zeros(2, dtype=torch.int64)
    groups = torch.zeros(2, 2, dtype=torch.int32)
    plain = train.Meters(torch.device("cpu"))
    assert train.validate(model, [(torch.zeros(2, 4), labels), (torch.zeros(2, 4), labels, groups)], plain) is None
    assert calls == ["cross_entropy", "cross_entropy"] and model.n_valid_steps == 4 and model.training
    # with a TypedMeters the two new operators follow every loss, and a batch without groups is refused
    from isubgvqa_amd.datasets import QuestionTypes
    typed = train.TypedMeters(torch.device("cpu"), QuestionTypes(names={"structural": ["a"], "semantic": ["b"]}))
    calls.clear()
    monkeypatch.setattr(ops, "answer_rank", lambda *a, **k: calls.append("answer_rank") or ops.AnswerRank(None, None, None))
    train.validate(model, [(torch.zeros(2, 4), labels, groups)], typed)
    assert calls == ["cross_entropy", "answer_rank", "group_meters"]
    with pytest.raises(ValueError):
        train.validate(model, [(torch.zeros(2, 4), labels)], typed)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement on cases written out by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_rank_and_top_on_rows_written_out_by_hand():
    x = torch.tensor([[0., 3., 1., 2., -1.], [2., 2., 0., 1., 2.], [4., 3., 2., 1., 0.], [1., 0., 0., 0., 0.], [0., 1., 2., 3., 4.],
                      [0., NAN, 0., 0., 9.], [-INF, INF, 0., INF, -INF]])
    labels = torch.tensor([1, 1, 3, -100, 5, 4, 3])
    assert restate_rank(x, labels).tolist() == [0, 1, 3, -1, 5, 5, 1]
    assert restate_rank(x, torch.tensor([4, 4, 0, 0, -1, 0, 4])).tolist() == [4, 2, 0, 0, 5, 5, 4]
    ids, prob = restate_top(x, 3, lse=torch.logsumexp(x.double(), 1))
    assert ids.tolist() == [[1, 3, 2], [0, 1, 4], [0, 1, 2], [0, 1, 2], [4, 3, 2], [-1, -1, -1], [1, 3, 2]]
    assert abs(float(prob[0, 0]) - math.exp(3) / sum(math.exp(v) for v in (0, 3, 1, 2, -1))) < 1e-15
    assert prob[5].tolist() == [0.0, 0.0, 0.0] and math.isnan(float(prob[6, 0])) and float(prob[6, 2]) == 0.0
    wide, none = restate_top(x[:, :2], 4)
    assert none is None and wide[0].tolist() == [1, 0, -1, -1] and wide[1].tolist() == [0, 1, -1, -1]
    # the reference's accuracy(): a hit at k iff the label is among torch.topk's k indices, where no tie decides
    y = torch.randn(50, 30, generator=torch.Generator().manual_seed(5))
    lab = torch.randint(0, 30, (50,), generator=torch.Generator().manual_seed(6))
    rk = restate_rank(y, lab)
    for k in (1, 5):
        assert ((rk >= 0) & (rk < k)).tolist() == (y.topk(k, 1).indices == lab[:, None]).any(1).tolist()


def test_restated_group_meters_and_coo_fold_on_cases_written_out_by_hand():
    loss = torch.tensor([1.0, 2.0, NAN, 4.0, 0.0, INF])
    rank = torch.tensor([0, 3, 9, 4, -1, 0], dtype=torch.int32)
    groups = torch.tensor([[0, 2], [0, -1], [1, 2], [1, 2], [0, 2], [7, -5]], dtype=torch.int32)
    t = add_group_meters(None, loss, rank, groups, 3, 4)
    assert t[:, :5].tolist() == [[2, 3, 0, 1, 2], [2, 4, 1, 0, 0], [3, 5, 1, 1, 1]] and float(t[:, 5:].abs().sum()) == 0
    assert bad_ids(groups, 3) == (2, 5) and bad_ids(groups[:5], 3) == (0, None)
    twice = add_group_meters(t, loss, rank, groups, 3, 4)
    assert torch.equal(twice, 2 * t)
    same = add_group_meters(None, loss[:2], rank[:2], torch.tensor([[1, 1], [1, -1]]), 2, 1)      # one group named by two facets
    assert same[1, :5].tolist() == [3, 4, 0, 2, 2]
    table = torch.tensor([[1, 1, 1, 1, 2, 1, 0, 0], [0, 1, 0, 0, 3, 3, 1, 1], [1, 0, 1, 0, 1, 0, 2, 1], [1, 1, 1, 1, 0, 0, 0, 0]],
                         dtype=torch.int32)
    qflags = [0, 0, 1, 0]
    g = [[0, 2], [0, -1], [1, 2], [-1, 2]]
    got = add_coo_groups(None, table, qflags, g, 3)
    assert got[0] == add_totals(None, table[[0, 1]], [0, 0]) and got[1] == add_totals(None, table[[2]], [1])
    assert got[2] == add_totals(None, table[[0, 2, 3]], [0, 1, 0])
    assert got[2][:12] == [3, 3, 2, 2, 2, 2, 2, 3, 1, 1, 2, 1] and got[2][16 + 2] == 1 and got[2][16 + HIST + 2] == 1
    whole = add_totals(None, table[[0, 2, 3]], [0, 1, 0])
    facet1 = add_coo_groups(None, table, qflags, [[r[1]] for r in g], 3)
    assert [sum(v) for v in zip(*facet1)] == whole                   # the groups of one facet sum to the totals of their questions
    again = add_coo_groups(got, table, qflags, g, 3)
    assert again == [[2 * v for v in row] for row in got]
