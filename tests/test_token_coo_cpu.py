"""Host-side checks of the token co-occurrence scoring: explain.TokenTables + the restatement the GPU tests compare with reproduce,
from STRINGS, what the reference's three functions returned for every case of tests/golden/g11_token_coo.pt
(tools/make_token_coo_golden.py), explain.CooReport reproduces the figures its script prints over lists of cases, and the C-ABI
entry point as far as it goes without a GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from token_coo_restated import HIST, TOKENS_MAX, TOTALS, add_totals, restate_table

NAN = float("nan")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("g11_token_coo.pt")
    masks, tkeeps = g["masks"].tolist(), g["tkeeps"].tolist()
    for c in g["cases"]:                       # the two float32 columns are stored once for all cases
        c["mask"], masks = masks[:c["mask"]], masks[c["mask"]:]
        c["tkeep"], tkeeps = tkeeps[:c["tkeep"]], tkeeps[c["tkeep"]:]
    assert not masks and not tkeeps
    return g


@pytest.fixture(scope="module")
def scored(golden):
    """(tables, [(table row, qflag, table row without the text explanation)] per case): every case as a batch of one graph."""
    from isubgvqa_amd import explain
    tables = explain.TokenTables(golden["stoi"], golden["answers"], golden["clip_itos"])
    rows = []
    for c in golden["cases"]:
        names = [golden["stoi"][o] for o in c["objects"]]
        qtok, qflags = tables.question_words([c["question"]])
        pred, label = [golden["answers"].index(c["answer"])], [golden["answers"].index(c["label"])]
        ttok = tables.text_tokens(torch.tensor([c["input_ids"]]))
        assert ttok.dtype == torch.int32 and tuple(ttok.shape) == (1, len(c["input_ids"]))
        args = (names, c["mask"], [0, len(names)], pred, label, tables.ans_sg, qtok)
        rows.append((restate_table(*args, ttok, [c["tkeep"]], threshold=c["threshold"])[0].tolist(), int(qflags[0]),
                     restate_table(*args, threshold=c["threshold"])[0].tolist()))
    return tables, rows


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_generator_covers_every_class_of_case(golden):
    cases = golden["cases"]
    assert len(cases) >= 200
    words = lambda c: c["question"].split("?")[0].lower().split(" ")
    nan = math.isnan
    classes = {
        "answer hit": lambda c: c["ans"] == (1.0, 1),
        "answer miss": lambda c: c["ans"] == (0.0, 0),
        "NaN by color": lambda c: nan(c["ans"][0]) and c["label"] in c["objects"] and "color" in c["question"],
        "NaN by absent label": lambda c: nan(c["ans"][0]) and c["label"] not in c["objects"],
        "partial question ratio with a repeated word": lambda c: 0.0 < c["qst"][0] < 1.0 and any(
            words(c).count(w) > 1 for w in words(c) if w in c["objects"]),
        "question NaN": lambda c: nan(c["qst"][0]) and c["qst"][1] == 0,
        "text NaN": lambda c: nan(c["text"]),
        "text not NaN": lambda c: not nan(c["text"]),
        "multi-word object name": lambda c: any(" " in o for o in c["objects"]),
        "empty word from a double space": lambda c: "" in words(c),
        "NaN mask entry": lambda c: any(nan(m) for m in c["mask"]),
        "mask value equal to the threshold, on a node the scoring looks up": lambda c: any(
            m == c["threshold"] and o in words(c) + [c["answer"]] for o, m in zip(c["objects"], c["mask"])),
        "wrong prediction": lambda c: c["answer"] != c["label"],
        "graph without nodes": lambda c: not c["objects"],
    }
    for name, is_one in classes.items():
        n = sum(1 for c in cases if is_one(c))
        assert n >= 10, f"{name}: {n} cases"
    assert {c["threshold"] for c in cases} >= {0.0, 0.5}


def test_tables_and_restatement_reproduce_every_case_from_the_strings(golden, scored):
    for c, (row, color, _) in zip(golden["cases"], scored[1]):
        correct, pred_in, label_in, ans_kept, words, words_kept, text, text_kept = row
        what = (c["kind"], c["question"], c["objects"], c["mask"], c["answer"], c["label"])
        assert correct == int(c["answer"] == c["label"]) and pred_in == int(c["answer"] in c["objects"]), what
        assert color == int("color" in c["question"])
        ans = ((1.0, 1) if ans_kept else (0.0, 0)) if label_in and not color else (NAN, 0)
        # the reference looks the PREDICTED answer up among the picked nodes and the true one among all: rows with a wrong
        # prediction are held to it as well
        assert _same(ans[0], c["ans"][0]) and ans[1] == c["ans"][1], (what, row, c["ans"])
        qst = (words_kept / words, words) if words else (NAN, 0)
        assert _same(qst[0], c["qst"][0]) and qst[1] == c["qst"][1], (what, row, c["qst"])
        assert _same(text_kept / text if text else NAN, c["text"]), (what, row, c["text"], c["input_ids"], c["tkeep"])


def test_report_prints_what_the_reference_prints(golden, scored):
    from isubgvqa_amd import explain
    assert len(golden["aggregates"]) >= 5
    for name, agg in golden["aggregates"].items():
        totals = None
        for i in agg["cases"]:                               # one call per question: totals accumulate over calls
            row, color, row_without_text = scored[1][i]
            totals = add_totals(totals, [row if agg["with_text"] else row_without_text], [color])
        totals = [0] * TOTALS if totals is None else totals
        assert totals[12:16] == [0, 0, 0, 0]
        report = explain.CooReport.from_totals(torch.tensor(totals, dtype=torch.int64))
        got = report.as_printed_by_reference()
        assert list(got) == ["Accuracy", "Accuracy AT", "Ans. Tok. Coo", "Qst. Tok. Coo", "Qst. Text Tok. Coo"]
        for key, want in agg["printed"].items():
            assert (math.isnan(want) and math.isnan(got[key])) or abs(got[key] - want) <= 1e-12 * abs(want), (name, key, got[key], want)
        assert _same(report.accuracy, got["Accuracy"]) and _same(report.accuracy_at, got["Accuracy AT"])
        assert _same(report.text_tok_coo, got["Qst. Text Tok. Coo"])


def test_report_on_a_known_answer():
    """np.nanmean([(0.5, 2), (nan, 0), (1.0, 3)]) = (0.5 + 2 + 0 + 1.0 + 3) / 5 = 1.3: three correct questions, two with matches
    (1 of 2, 3 of 3); the plain mean of the two ratios is 0.75."""
    import numpy as np
    from isubgvqa_amd import explain
    assert abs(float(np.nanmean([(0.5, 2), (NAN, 0), (1.0, 3)])) - 1.3) < 1e-15
    table = [[1, 0, 1, 1, 2, 1, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 3, 3, 4, 1], [0, 1, 1, 1, 5, 5, 2, 2]]
    totals = add_totals(None, table, [0, 0, 1, 0])
    assert totals[:12] == [4, 3, 3, 2, 1, 1, 2, 5, 4, 1, 4, 1]
    assert totals[16 + 2] == 1 and totals[16 + 3] == 1 and totals[16 + HIST + 2] == 1 and totals[16 + HIST + 3] == 3
    assert totals[16 + 2 * HIST + 4] == 1 and totals[16 + 3 * HIST + 4] == 1 and sum(totals) == sum(totals[:12]) + 8
    r = explain.CooReport.from_totals(torch.tensor(totals))
    assert (r.accuracy, r.accuracy_at, r.ans_tok_coo, r.qst_tok_coo, r.text_tok_coo) == (0.75, 2 / 3, 1.0, 0.75, 0.25)
    p = r.as_printed_by_reference()
    assert abs(p["Qst. Tok. Coo"] - 1.3) < 1e-15 and p["Ans. Tok. Coo"] == 2 * 1 / (1 + 3) and p["Qst. Text Tok. Coo"] == 0.25
    empty = explain.CooReport.from_totals(torch.zeros(TOTALS, dtype=torch.int64))
    assert all(math.isnan(v) for v in empty.as_printed_by_reference().values()) and math.isnan(empty.qst_tok_coo)
    with pytest.raises(ValueError):
        explain.CooReport.from_totals(torch.zeros(TOTALS - 1, dtype=torch.int64))


def test_question_words_split_as_the_reference_splits():
    from isubgvqa_amd import explain
    t = explain.TokenTables({"cat": 3, "dog": 5, "traffic light": 7, "light": 8}, ["cat", "yes", "traffic light"], ["cat</w>", "do", "light</w>"])
    assert t.ans_sg.tolist() == [3, -1, 7] and t.clip_sg.tolist() == [3, -1, 8] and t.ans_sg.dtype == t.clip_sg.dtype == torch.int32
    qtok, qflags = t.question_words(["Is the  CAT near the traffic light? dog", "what colors?", ""])
    assert qtok.tolist() == [[-1, -1, -1, 3, -1, -1, -1, 8], [-1, -1] + [-1] * 6, [-1] * 8]       # upper case folds, `dog` is cut off
    assert qflags.tolist() == [0, 1, 0] and qtok.dtype == qflags.dtype == torch.int32
    assert tuple(t.question_words([])[0].shape) == (0, 0)
    with pytest.raises(ValueError):
        explain.TokenTables({}, []).text_tokens(torch.zeros(1, 2, dtype=torch.long))


def test_header_declares_the_entry_point_and_the_constants_agree():
    from isubgvqa_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "isg.h")).read()
    body = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"\bint\s+isg_token_coo\s*\(", body)
    assert int(re.search(r"#define ISG_ABI_VERSION (\d+)", header).group(1)) == 23 == _lib.ABI_VERSION
    P, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    assert _lib.SIGNATURES["isg_token_coo"] == (ctypes.c_int, [P, I64, P, F, P, P, P, P, P, P, P, P, I64, I64, I64, I32, I32, P, P, P])
    assert len(_lib.SIGNATURES) == 74
    assert int(re.search(r"#define ISG_COO_TOKENS_MAX (\d+)", header).group(1)) == ops.COO_TOKENS_MAX == TOKENS_MAX == 128
    assert re.search(r"#define ISG_COO_TOTALS \(16 \+ 4 \* \(ISG_COO_TOKENS_MAX \+ 1\)\)", header)
    assert ops.COO_TOTALS == TOTALS == 16 + 4 * 129
    kernel = open(os.path.join(ROOT, "intrinsic-subgraph-generation-for-vqa_amd", "csrc", "isg_token_coo.hip")).read()
    assert int(re.search(r"constexpr int COO_NODE_CHUNK = (\d+);", kernel).group(1)) == ops.COO_NODE_CHUNK
    assert "ISG_WAIT(" not in kernel and "ISG_BARRIER(" not in kernel          # plain HIP: the strict library shares the object
    assert not re.search(r"\batomic\w*\s*\(\s*&?\s*a\.", kernel)                 # nothing is accumulated atomically in global memory


def test_token_coo_refuses_bad_arguments_before_any_hip_call():
    """No GPU is needed: every refusal below happens on the host, before the library touches HIP."""
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import _lib
    lib = _lib.load()
    keep = [ctypes.create_string_buffer(8 * 64) for _ in range(12)]       # host memory: never dereferenced by a refused call
    p = [ctypes.addressof(b) for b in keep]

    def call(**over):
        a = dict(names=p[0], name_stride=4, node_mask=p[1], threshold=0.0, ptr=p[2], pred=p[3], label=p[4], ans_sg=p[5], qtok=p[6],
                 qflags=p[7], ttok=p[8], tkeep=p[9], N=5, B=2, A=3, T=4, T2=6, table=p[10], totals=p[11], stream=None)
        a.update(over)
        return lib.isg_token_coo(*a.values())

    EINVAL, EUNSUPPORTED = -1, -2
    for name in ("names", "node_mask", "ptr", "pred", "label", "ans_sg", "qtok", "ttok", "tkeep", "table"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("N", "B", "A", "T", "T2"):
        assert call(**{name: -1}) == EINVAL, name
    assert call(name_stride=0) == EINVAL and call(name_stride=-4) == EINVAL
    assert call(T=129) == EUNSUPPORTED and call(T2=129) == EUNSUPPORTED
    assert call(N=2 ** 31) == EUNSUPPORTED and call(B=2 ** 31) == EUNSUPPORTED and call(A=2 ** 31) == EUNSUPPORTED
    assert call(name_stride=2 ** 31) == EUNSUPPORTED
    # tables that are not given may be null, and a batch without questions is complete before any launch
    assert call(B=0, pred=None, label=None, table=None, qtok=None, T=0, ttok=None, tkeep=None, T2=0, qflags=None, totals=None) == 0
    assert call(B=0, ptr=None) == EINVAL


def test_token_coo_fails_loudly_on_cpu_tensors():
    from isubgvqa_amd import _lib, ops
    ptr = torch.tensor([0, 3, 5], dtype=torch.int32)
    plan = ops.GraphPlan(N=5, E=0, B=2, ptr=ptr, nmax_dev=torch.zeros(1, dtype=torch.int32), nmax=3, batch=torch.tensor([0, 0, 0, 1, 1]))
    x = torch.arange(20).view(5, 4)
    pred = torch.zeros(2, dtype=torch.long)
    with pytest.raises(_lib.IsgError, match="no CPU fallback"):
        ops.token_coo(x[:, 0], torch.ones(5), plan, pred, pred, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="come together"):
        ops.token_coo(x[:, 0], torch.ones(5), plan, pred, pred, torch.zeros(3, dtype=torch.int32), ttok=torch.zeros(2, 1, dtype=torch.int32))
