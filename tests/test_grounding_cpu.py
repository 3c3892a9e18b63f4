"""Host-side checks of the grounding score (include/isg_grounding.h, include/isg_loader_objects.h) that need no GPU:
the loader's object id -> node index on the graphs of the golden G8; headers, bindings and exported symbols; the entry point's
refusals before any HIP call; datasets.gqa.ObjectAnnotations and gqa_collate; explain.GroundingReport.from_totals on a row written
by hand; explain.EvalBatch with gold; the restatement of tests/grounding_restated.py on cases written out by hand."""
import ctypes
import inspect
import json
import math
import os
import re

import pytest
import torch

from binding_checks import build_checks
from conftest import ROOT, load_golden
from grounding_restated import add_totals, bad_group_ids, macro_recall, restate_table

EINVAL, EUNSUPPORTED = -1, -2
P = 4096                        # any non-null, 16-byte aligned address; nothing dereferences it on the paths tested here
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from isubgvqa_amd import loader
    return loader


@pytest.fixture(scope="module")
def g8():
    return load_golden("g8_loader.pt")


@pytest.fixture(scope="module")
def store(L, g8):
    return L.SceneGraphStore(L.SceneGraphVocab(g8["token_lists"])).add_json(g8["json"])


@pytest.fixture(scope="module")
def C():
    from isubgvqa_amd import _lib_grounding
    return _lib_grounding.CONSTANTS


# ---------------------------------------------------------------------------------------------------------------------
# loader: object id -> node index
# ---------------------------------------------------------------------------------------------------------------------
def _dummy_at_collate(objects):
    """An image the collate replaces by a dummy graph: no objects, or one object without relations (a single self loop)."""
    return len(objects) == 0 or (len(objects) == 1 and not next(iter(objects.values()))["relations"])


def test_every_object_id_of_every_image_resolves_to_its_place_in_the_sorted_ids(L, g8, store):
    graphs = json.loads(g8["json"])
    seen_real = 0
    for key, graph in graphs.items():
        ids = list(graph["objects"])
        nodes, ptr = store.object_nodes([key], [ids])
        assert nodes.dtype == torch.int32 and ptr.dtype == torch.int64 and ptr.tolist() == [0, len(ids)]
        if _dummy_at_collate(graph["objects"]):
            assert nodes.tolist() == [L.NO_NODE] * len(ids), key
            continue
        order = sorted(graph["objects"].keys())
        assert nodes.tolist() == [order.index(i) for i in ids], key
        # the index is the row of the collated batch: the node carries the object's name token
        x = store.collate([key], pin_memory=False).x
        assert x.size(0) == len(ids)
        for i, n in zip(ids, nodes.tolist()):
            assert int(x[n, 0]) == g8["stoi"].get(graph["objects"][i]["name"], 1), (key, i)
        seen_real += 1
    assert seen_real >= 14


def test_dummies_absent_images_and_absent_ids_resolve_nothing(L, g8, store):
    graphs = json.loads(g8["json"])
    assert graphs["empty"]["objects"] == {} and len(graphs["single"]["objects"]) == 1
    some = sorted(graphs["img3"]["objects"])[0]
    only = next(iter(graphs["single"]["objects"]))
    nodes, ptr = store.object_nodes(["empty", "not-in-the-file", "img3", "single"], [["0", "1", some], [some, "0"], ["no such id", some, ""], [only]])
    assert ptr.tolist() == [0, 3, 5, 8, 9]
    # `single` is one self loop: every collate hands out the 6-node dummy for it, so its object is no node of that graph
    assert nodes.tolist() == [-2, -2, -2, -2, -2, -2, 0, -2, -2]
    assert store.collate(["single"], pin_memory=False).x.size(0) == 6 and store.collate(["empty"], pin_memory=False).x.size(0) == 2


def test_node_order_is_string_order(L, g8):
    obj = lambda name, rels: {"name": name, "attributes": [], "relations": [{"object": r, "name": "on"} for r in rels]}
    graph = {"pic": {"objects": {"9": obj("cat", ["10"]), "10": obj("dog", []), "100": obj("man", ["9"])}}}
    st = L.SceneGraphStore(L.SceneGraphVocab(g8["token_lists"])).add_json(json.dumps(graph))
    assert sorted(["9", "10", "100"]) == ["10", "100", "9"]
    nodes, _ = st.object_nodes(["pic"], [["9", "10", "100", "1", "1000", "99"]])
    assert nodes.tolist() == [2, 0, 1, -2, -2, -2]
    # a later file replaces the image: the ids follow
    st.add_json(json.dumps({"pic": {"objects": {"7": obj("cat", ["8"]), "8": obj("dog", [])}}}))
    assert st.object_nodes(["pic"], [["9", "7", "8"]])[0].tolist() == [-2, 0, 1]
    assert st.object_bytes() == len("910100") + len("78") + 8 * (4 + 3)


def test_a_mixed_batch_with_an_empty_list_in_the_middle_and_slots(L, g8, store):
    graphs = json.loads(g8["json"])
    keys = ["img5", "empty", "img0", "nope", "img5", "selfrel"]
    lists = [list(graphs["img5"]["objects"])[::-1], ["1"], [], ["2"], ["x", None, sorted(graphs["img5"]["objects"])[-1]],
             list(graphs["selfrel"]["objects"])]
    nodes, ptr = store.object_nodes(keys, lists)
    want = []
    for k, ids in zip(keys, lists):
        objects = graphs.get(k, {"objects": {}})["objects"]
        order = [] if _dummy_at_collate(objects) else sorted(objects)
        want += [order.index(i) if i in order else -2 for i in ids]
    assert ptr.tolist() == [0, 8, 9, 9, 10, 13, 16] and nodes.tolist() == want
    assert nodes[10:13].tolist() == [-2, -2, len(graphs["img5"]["objects"]) - 1]           # None is a NULL string
    by_slot, ptr2 = store.object_nodes(store.slots(keys), lists)
    assert torch.equal(by_slot, nodes) and torch.equal(ptr2, ptr)
    none, p0 = store.object_nodes([], [])
    assert none.numel() == 0 and p0.tolist() == [0]
    with pytest.raises(ValueError):
        store.object_nodes(["img0"], [])
    per_object = store.object_bytes() / sum(len(g["objects"]) for g in graphs.values() if g["objects"])
    assert 8.0 < per_object < 24.0                              # its characters, one offset, and its share of one offset per image


def test_object_nodes_refuses_bad_arguments(L, store):
    lib = L.load()
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    ids = (ctypes.c_char_p * 2)(b"1", b"2")
    out = (ctypes.c_int32 * 2)()
    call = lambda s, slots, B, ptr, strings, nodes: lib.isg_sg_store_object_nodes(s, slots, B, ptr, strings, nodes)
    assert call(store._h, i64([0]), 1, i64([0, 2]), ids, out) == 0
    assert call(None, i64([0]), 1, i64([0, 2]), ids, out) == EINVAL
    assert call(store._h, None, 1, i64([0, 2]), ids, out) == EINVAL and call(store._h, i64([0]), 1, None, ids, out) == EINVAL
    assert call(store._h, i64([0]), -1, i64([0, 2]), ids, out) == EINVAL
    assert call(store._h, i64([0]), 1, i64([1, 2]), ids, out) == EINVAL and b"id_ptr[0]" in lib.isg_sg_last_error()
    assert call(store._h, i64([0, 0]), 2, i64([0, 2, 1]), ids, out) == EINVAL and b"descends" in lib.isg_sg_last_error()
    assert call(store._h, i64([0]), 1, i64([0, 2]), None, out) == EINVAL and call(store._h, i64([0]), 1, i64([0, 2]), ids, None) == EINVAL
    assert call(store._h, None, 0, None, None, None) == 0 and call(store._h, i64([5]), 1, i64([0, 0]), None, None) == 0
    assert lib.isg_sg_store_object_bytes(None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# headers, bindings, exported symbols
# ---------------------------------------------------------------------------------------------------------------------
def test_both_headers_parse_bind_and_are_exported(L, C):
    import __graft_entry__ as ge
    from isubgvqa_amd import _lib, _lib_eval, _lib_grounding, ops
    path = os.path.join(ROOT, "include", "isg_grounding.h")
    declared = set(L.declared_symbols(path))
    assert declared == set(_lib_grounding.SIGNATURES) == {"isg_grounding_abi_version", "isg_grounding"}
    for other in (_lib, _lib_eval):
        assert not declared & set(other.SIGNATURES), "a symbol is declared in two headers"
    abi = int(re.search(r"#define ISG_GROUNDING_ABI_VERSION (\d+)", open(path).read()).group(1))
    assert _lib_grounding.load().isg_grounding_abi_version() == _lib_grounding.ABI_VERSION == abi == 1
    for lib_path in (_lib.LIB_PATH, ge.STRICT_LIB):
        raw = ctypes.CDLL(lib_path)
        raw.isg_grounding_abi_version.restype = ctypes.c_int
        assert hasattr(raw, "isg_grounding") and raw.isg_grounding_abi_version() == 1, lib_path
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    # (node_mask, threshold, ptr, gold, F, M, pred, label, groups, Fg, G, table, totals, status, N, B, stream)
    assert _lib_grounding.SIGNATURES["isg_grounding"] == (ctypes.c_int, [ptr, ctypes.c_float, ptr, ptr, i32, i32, ptr, ptr, ptr, i32, i32,
                                                                         ptr, ptr, ptr, i64, i64, ptr])
    # the loader's second header: a table of its own; the first header's equality is untouched
    opath = os.path.join(ROOT, "include", "isg_loader_objects.h")
    odecl = L.declared_symbols(opath)
    assert odecl == sorted(L.OBJECT_SIGNATURES) == ["isg_loader_objects_abi_version", "isg_sg_store_object_bytes", "isg_sg_store_object_nodes"]
    assert L.declared_symbols(os.path.join(ROOT, "include", "isg_loader.h")) == sorted(L.SIGNATURES)
    assert not set(odecl) & set(L.SIGNATURES)
    oabi = int(re.search(r"#define ISG_LOADER_OBJECTS_ABI_VERSION (\d+)", open(opath).read()).group(1))
    assert L.load().isg_loader_objects_abi_version() == L.OBJECT_ABI_VERSION == oabi == 1
    raw = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(raw, n) for n in odecl)
    assert L.OBJECT_SIGNATURES["isg_sg_store_object_nodes"] == (ctypes.c_int, [ptr, ptr, i64, ptr, ptr, ptr])
    assert L.NO_NODE == int(re.search(r"#define ISG_LD_NO_NODE \((-\d+)\)", open(opath).read()).group(1)) == C["ISG_GROUND_UNRESOLVED"]
    # build() and smoke()
    build_checks("isg_grounding.h")
    build_checks("isg_loader_objects.h")
    assert "_smoke_grounding(dev)" in inspect.getsource(ge.smoke)
    # the constants come from the header
    assert (ops.GROUND_COLS, ops.GROUND_TOTALS, ops.GROUND_GOLD_MAX) == (C["ISG_GROUND_COLS"], C["ISG_GROUND_TOTALS"], C["ISG_GROUND_GOLD_MAX"])
    assert (C["ISG_GROUND_COLS"], C["ISG_GROUND_GOLD_MAX"], C["ISG_GROUND_FACETS"], C["ISG_GROUND_SETS"], C["ISG_GROUND_HEAD"]) == (12, 64, 3, 4, 8)
    assert C["ISG_GROUND_HIST"] == 3 * 64 + 1 and C["ISG_GROUND_BLOCK"] == 8 + 2 * C["ISG_GROUND_HIST"]
    assert C["ISG_GROUND_TOTALS"] == 8 + 8 * C["ISG_GROUND_BLOCK"] and (C["ISG_GROUND_PAD"], C["ISG_GROUND_UNRESOLVED"]) == (-1, -2)
    assert "grounding" in ops.COUNTERS
    # the rules of include/isg_eval.h: integer LDS atomics only
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ge.CSRC, "isg_grounding.hip")).read())
    atomics = re.findall(r"atomic\w+\(([^;]*);", text)
    assert atomics and all(re.match(r"\s*&(s_tot|hist|s_bad|s_first)\b", a) for a in atomics), atomics
    assert "double" not in text, "no floating-point sum runs on the device"


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    from isubgvqa_amd import _lib_grounding
    lib = _lib_grounding.load()

    def call(mask=P, ptr=P, gold=P, F=3, M=7, pred=P, label=P, groups=P, Fg=2, G=5, table=P, totals=P, status=P, N=100, B=9):
        return lib.isg_grounding(mask, 0.0, ptr, gold, F, M, pred, label, groups, Fg, G, table, totals, status, N, B, None)

    for k in ("mask", "ptr", "gold", "table"):
        assert call(**{k: None}) == EINVAL, k
    assert call(F=0) == EINVAL and call(F=4) == EINVAL and call(M=0) == EINVAL and call(M=65) == EINVAL and call(M=-1) == EINVAL
    assert call(N=-1) == EINVAL and call(B=-1) == EINVAL
    assert call(pred=None) == EINVAL and call(label=None) == EINVAL
    assert call(G=0) == EINVAL and call(G=257) == EINVAL and call(Fg=0) == EINVAL and call(Fg=5) == EINVAL
    assert call(B=(1 << 31) - 1) == EUNSUPPORTED and call(N=(1 << 31) - 1) == EUNSUPPORTED and call(B=1 << 40) == EUNSUPPORTED
    assert call(B=0) == 0
    assert call(B=0, mask=None, ptr=None, gold=None, pred=None, label=None, groups=None, table=None, totals=None, status=None) == 0
    assert call(B=0, groups=None, G=999, Fg=-3) == 0              # without groups, G and Fg are not looked at
    assert call(B=0, F=0) == EINVAL and call(B=0, G=0) == EINVAL


def test_ops_grounding_refuses_host_tensors_and_bad_shapes():
    from isubgvqa_amd import _lib, ops

    class Plan:
        N, B, ptr = 4, 2, torch.tensor([0, 2, 4], dtype=torch.int32)

    mask, gold = torch.ones(4), torch.zeros(2, 3, 5, dtype=torch.int32)
    with pytest.raises(_lib.IsgError):
        ops.grounding(mask, Plan, gold)                          # no CPU fallback
    for bad in (torch.zeros(2, 4, 5, dtype=torch.int32), torch.zeros(2, 3, 65, dtype=torch.int32), torch.zeros(3, 3, 5, dtype=torch.int32),
                torch.zeros(2, 5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.grounding(mask, Plan, bad)
    with pytest.raises(ValueError):
        ops.grounding(mask, Plan, gold, pred=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.grounding(mask, Plan, gold, num_groups=3)
    with pytest.raises(ValueError):
        ops.grounding(mask, Plan, gold, groups=torch.zeros(2, 2, dtype=torch.int32), num_groups=0)
    with pytest.raises(ValueError):
        ops.grounding(mask, Plan, gold, totals=torch.zeros(2, ops.GROUND_TOTALS, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# ObjectAnnotations, gqa_collate, EvalBatch
# ---------------------------------------------------------------------------------------------------------------------
class _Store:
    """object_nodes on made-up graphs: image `a` has objects 10 < 11 < 9 (string order), image `b` object 5."""
    graphs = {"a": ["10", "11", "9"], "b": ["5"]}

    def __init__(self):
        self.calls = 0

    def object_nodes(self, image_ids, object_ids):
        self.calls += 1
        flat = [self.graphs[k].index(i) if i in self.graphs.get(k, []) else -2 for k, ids in zip(image_ids, object_ids) for i in ids]
        ptr = [0]
        for ids in object_ids:
            ptr.append(ptr[-1] + len(ids))
        return torch.tensor(flat, dtype=torch.int32), torch.tensor(ptr, dtype=torch.int64)

    def collate(self, ids, pin_memory, distinct=False):
        return ("batch", list(ids), distinct)


ANNOS = [{"question": {"4": "9", "1:3": "10,11"}, "answer": {"0": ["11", "77"]}, "fullAnswer": {"2": "9", "5": "9"}},
         {"question": {}, "answer": {"0": "5"}},                                     # no fullAnswer
         {"question": {"7": "10", "0": "9"}, "answer": None, "fullAnswer": "not a dict"},
         None]


def test_object_annotations_encode_value_forms_order_and_missing_facets():
    from isubgvqa_amd.datasets import ObjectAnnotations
    from isubgvqa_amd.datasets.gqa import ObjectAnnotations as same
    assert ObjectAnnotations is same
    oa = ObjectAnnotations()
    assert oa.facets == ("question", "answer", "fullAnswer") and oa.max_gold == 64
    st = _Store()
    enc = oa.encode(ANNOS, ["a", "b", "a", "a"], st)
    assert st.calls == 1, "one batched call to the loader"
    assert enc.dtype == torch.int32 and tuple(enc.shape) == (4, 3, 3) and enc.is_pinned() == torch.cuda.is_available()
    assert enc.tolist() == [[[2, 0, 1], [1, -2, -1], [2, 2, -1]],       # dict order: "4" before "1:3"; a comma list; a list; an absent id
                            [[-1, -1, -1], [0, -1, -1], [-1, -1, -1]],
                            [[0, 2, -1], [-1, -1, -1], [-1, -1, -1]],   # the dict's order, not the word positions'
                            [[-1, -1, -1]] * 3]
    assert oa.object_ids(ANNOS[:1]) == [[["9", "10", "11"], ["11", "77"], ["9", "9"]]]
    two = ObjectAnnotations(facets=("answer", "question"))
    assert two.encode(ANNOS[:2], ["a", "zzz"], st).tolist() == [[[1, -2, -1], [2, 0, 1]], [[-2, -1, -1], [-1, -1, -1]]]
    empty = oa.encode([], [], st)
    assert tuple(empty.shape) == (0, 3, 1) and empty.dtype == torch.int32
    assert oa.encode([{}, None], ["a", "b"], st).tolist() == [[[-1]] * 3] * 2      # M is at least 1
    with pytest.raises(ValueError):
        ObjectAnnotations(facets=())
    with pytest.raises(ValueError):
        ObjectAnnotations(facets=("a", "b", "c", "d"))
    with pytest.raises(ValueError):
        ObjectAnnotations(max_gold=65)
    with pytest.raises(ValueError):
        oa.encode(ANNOS, ["a"], st)


def test_object_annotations_refuse_more_ids_than_max_gold_naming_the_question():
    from isubgvqa_amd.datasets import ObjectAnnotations
    small = ObjectAnnotations(max_gold=2)
    with pytest.raises(ValueError, match=r"question 0 .*`question`"):
        small.encode(ANNOS, ["a", "b", "a", "a"], _Store())
    assert small.encode(ANNOS[1:], ["b", "a", "a"], _Store()).size(2) == 2
    wide = [{}, {"answer": {str(i): str(i) for i in range(65)}}]
    with pytest.raises(ValueError, match=r"question 1 .*65 .*`answer`"):
        ObjectAnnotations().encode(wide, ["a", "a"], _Store())
    wide[1]["answer"].pop("64")
    assert tuple(ObjectAnnotations().encode(wide, ["a", "a"], _Store()).shape) == (2, 3, 64)


def test_gqa_collate_with_and_without_annotations(L, g8, store):
    from isubgvqa_amd.datasets import ObjectAnnotations, gqa_collate
    graphs = json.loads(g8["json"])
    keys = ["img1", "img2", "img1", "nope"]
    annos = [{"question": {"0": sorted(graphs[k]["objects"])[-1]} if k in graphs else {"0": "1"}, "answer": {}} for k in keys]
    six = [(f"q{i}", k, "what", {"structural": "query"}, i, k) for i, k in enumerate(keys)]
    seven = [item + (a,) for item, a in zip(six, annos)]

    class Graphs:                                                # a GQASceneGraphs as far as the collate looks
        def __init__(self, st):
            self.store = st

        def collate(self, ids, pin_memory, distinct=False):
            return self.store.collate(ids, pin_memory, distinct=distinct)

    plain = gqa_collate(six, Graphs(store), pin_memory=False)
    assert len(plain) == 7 and plain[6] == tuple(t[3] for t in six)
    with pytest.raises(ValueError):
        gqa_collate(seven, Graphs(store), pin_memory=False)      # without the keyword, the accepted item is exactly today's
    out = gqa_collate(seven, Graphs(store), pin_memory=False, annotations=ObjectAnnotations())
    assert len(out) == 8 and out[0] == plain[0] and out[5:7] == plain[5:7] and torch.equal(out[4], plain[4]) and out[1].num_graphs == 4
    assert torch.equal(out[1].x, plain[1].x) and out[2] is None and out[3] is None
    want = [[[len(graphs[k]["objects"]) - 1] if k in graphs else [-2], [-1], [-1]] for k in keys]
    assert out[7].tolist() == want and out[7].dtype == torch.int32
    shared = gqa_collate(seven, Graphs(store), pin_memory=False, distinct=True, annotations=ObjectAnnotations())
    assert shared[1].num_graphs == 3 and shared[1].graph_index.tolist() == [0, 1, 0, 2]
    assert torch.equal(shared[7], out[7]), "indices are local to a graph: the same for every instance of it"
    assert gqa_collate(seven, store, pin_memory=False, annotations=ObjectAnnotations())[7].tolist() == want      # a bare store


def test_eval_batch_carries_gold_beside_its_fields():
    from isubgvqa_amd import explain
    b = explain.EvalBatch("inputs", torch.zeros(2, dtype=torch.int64))
    assert b.gold is None and b.groups is None and len(b) == 6 and explain.EvalBatch._fields[-1] == "graph_index"
    new = explain.EvalBatch("inputs", 1, qflags=3, groups="g", gold="au")
    assert (new.gold, new.groups, new.qflags) == ("au", "g", 3) and len(new) == 6 and tuple(new) == ("inputs", 1, None, 3, None, None)
    assert new._replace(label=2).gold == "au" and new._replace(label=2).groups == "g"
    assert new._replace(gold=None).gold is None and new._replace(gold=None).groups == "g" and new._replace(groups=None).gold == "au"
    assert explain.EvalBatch._make(range(6)).gold is None
    sig = inspect.signature(explain.evaluate).parameters
    assert sig["grounding"].default is False and list(sig)[-1] == "grounding"
    from token_coo_restated import TOTALS
    r = explain.CooReport.from_totals([0] * TOTALS)
    assert r.grounding is None and r.by_type is None and r.totals == (0,) * TOTALS
    fields = {f.name: f for f in __import__("dataclasses").fields(explain.CooReport)}
    assert fields["grounding"].default is None and fields["grounding"].compare is False


# ---------------------------------------------------------------------------------------------------------------------
# the restatement and the report on cases written out by hand
# ---------------------------------------------------------------------------------------------------------------------
MASK = [1.0, 0.0, 1.0, NAN, 1.0, 0.5, 0.5]
PTR = [0, 3, 3, 5, 7]
GOLD = [[[0, 0, 1], [2, -2, -1]], [[0, -2, -1], [-1, -1, -1]], [[1, 2, -1], [0, 1, -3]], [[-1, -1, -1], [-1, -1, -1]]]


def test_restated_table_on_rows_written_out_by_hand():
    assert restate_table(MASK, PTR, GOLD) == [[2, 3, 1, 0, 2, 1, 1, 1, 0, 0, 3, 2],
                                              [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0],
                                              [1, 2, 0, 2, 1, 1, 2, 1, 0, 0, 2, 1],
                                              [2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    strict = restate_table(MASK, PTR, GOLD, threshold=0.5)       # the comparison is strict
    assert [r[0] for r in strict] == [2, 0, 1, 0] and strict[0][4:] == [2, 1, 1, 1, 0, 0, 3, 2]
    assert restate_table(torch.tensor(MASK).view(-1, 1), torch.tensor(PTR), torch.tensor(GOLD)) == restate_table(MASK, PTR, GOLD)


def test_restated_totals_and_the_report_on_rows_written_out_by_hand(C):
    from isubgvqa_amd import explain
    table = restate_table(MASK, PTR, GOLD)
    groups = [[0, 1], [0, -1], [1, 1], [5, -2]]
    assert bad_group_ids(groups, 2) == (2, 3) and bad_group_ids(groups[:3], 2) == (0, None)
    tot = add_totals(None, table, C, pred=[4, 1, 2, 0], label=[4, 0, 2, 0], groups=groups, G=2)
    assert len(tot) == 3 and all(len(r) == C["ISG_GROUND_TOTALS"] for r in tot)
    H, BL, HI = C["ISG_GROUND_HEAD"], C["ISG_GROUND_BLOCK"], C["ISG_GROUND_HIST"]
    all_rows = tot[0]
    assert all_rows[:8] == [4, 3, 2, 3, 0, 0, 0, 0]
    union = H + 6 * BL
    assert all_rows[union:union + 8] == [2, 3, 5, 5, 3, 2, 0, 0] and all_rows[union + BL:union + BL + 8] == [2, 3, 5, 5, 3, 2, 0, 0]
    assert all_rows[union + 8 + 2] == 1 and all_rows[union + 8 + 3] == 1 and all_rows[union + 8 + HI + 3] == 2 and all_rows[union + 8 + HI + 2] == 1
    assert all_rows[H:H + 7] == [2, 3, 5, 3, 2, 2, 1]             # the question facet: |G| = 2 and 1, hits 1 and 1
    assert tot[1][:4] == [2, 1, 2, 1] and tot[2][:4] == [3, 3, 1, 4]        # group 1: question 0 once, question 2 twice
    assert tot[2][H:H + 7] == [3, 4, 7, 4, 3, 3, 2]
    twice = add_totals(tot, table, C, pred=[4, 1, 2, 0], label=[4, 0, 2, 0], groups=groups, G=2)
    assert twice == [[2 * v for v in r] for r in tot]
    none = add_totals(None, table, C)
    assert none[0][1] == 0 and sum(none[0][H + BL:H + 2 * BL]) == 0 and none[0][H:H + BL] == all_rows[H:H + BL]

    rep = explain.GroundingReport.from_totals(all_rows)
    assert (rep.questions, rep.correct, rep.unresolved, rep.bad) == (4, 3, 2, 3) and rep.by_type is None
    assert set(rep.sets) == {"question", "answer", "fullAnswer", "any"} and set(rep.sets["any"]) == {"all", "correct"}
    q = rep.sets["question"]["all"]
    assert (q.questions, q.precision, q.recall, q.chance, q.pointing, q.full_recall) == (2, 2 / 3, 2 / 3, 3 / 5, 1.0, 0.5)
    assert q.macro_recall == (1 / 2 + 1 / 1) / 2 == macro_recall(table, 0) and abs(q.f1 - 2 / 3) < 1e-15
    u = rep.sets["any"]["all"]
    assert u.macro_recall == (2 / 3 + 1 / 2) / 2 == macro_recall(table, 3) and u.recall == 3 / 5 and u.full_recall == 0.0
    third = rep.sets["fullAnswer"]["all"]                        # no question annotates it: every figure is NaN
    assert third.questions == 0 and all(math.isnan(v) for v in (third.precision, third.recall, third.macro_recall, third.f1,
                                                                  third.pointing, third.full_recall, third.chance))
    zero = explain.GroundingReport.from_totals([0] * C["ISG_GROUND_TOTALS"])
    assert zero.questions == 0 and math.isnan(zero.sets["any"]["correct"].chance) and zero == explain.GroundingReport.from_totals(
        torch.zeros(C["ISG_GROUND_TOTALS"], dtype=torch.int64))
    # hits 0 of 0 kept nodes: precision NaN, recall 0, F1 NaN;  precision 0 and recall 0: F1 0
    row = [0] * C["ISG_GROUND_TOTALS"]
    row[H:H + 7] = [1, 0, 4, 2, 0, 0, 0]
    row[H + 8 + 2] = 1
    f = explain.GroundingReport.from_totals(row).sets["question"]["all"]
    assert math.isnan(f.precision) and f.recall == 0.0 and math.isnan(f.f1) and f.macro_recall == 0.0 and f.chance == 0.0
    row[H + 1] = 3
    assert explain.GroundingReport.from_totals(row).sets["question"]["all"].f1 == 0.0
    two = explain.GroundingReport.from_totals(all_rows, facets=("answer", "question"))
    assert set(two.sets) == {"answer", "question", "any"} and two.sets["answer"]["all"] == q
    with pytest.raises(ValueError):
        explain.GroundingReport.from_totals(all_rows[:-1])
