"""ctypes binding of libisg_loader.so (include/isg_loader.h) and the batch object it fills.

Host side of SURVEY §8f row 2: GQA scene-graph JSON -> token tensors (once per image, while parsing) -> collated PyG-style
batch written straight into pinned host memory -> one async copy per tensor -> `ops.GraphPlan` without a device sync
(the collate also returns the max nodes / edges per graph).  Reference: ISubGVQA/datasets/scene_graph.py:145-389,
ISubGVQA/datasets/gqa.py:170-175,237-272.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_int64, c_void_p
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from ._lib import bind, read_header

_HERE = os.path.dirname(os.path.abspath(__file__))
# ISG_LOADER_LIB: an alternative build of the same library (the sanitizer build of tools/asan_loader.sh)
LIB_PATH = os.environ.get("ISG_LOADER_LIB") or os.path.join(_HERE, "csrc", "libisg_loader.so")


class LoaderError(RuntimeError):
    pass


# name -> (restype, argtypes) of every symbol include/isg_loader.h declares; ISG_LOADER_ABI_VERSION
SIGNATURES, ABI_VERSION = read_header(os.path.join(os.path.dirname(_HERE), "include", "isg_loader.h"), LoaderError)

# the same of include/isg_loader_objects.h (object id -> node index), a table and an ABI version of its own: SIGNATURES stays
# exactly what isg_loader.h declares
OBJECT_SIGNATURES, OBJECT_ABI_VERSION = read_header(os.path.join(os.path.dirname(_HERE), "include", "isg_loader_objects.h"), LoaderError)
NO_NODE = -2               # ISG_LD_NO_NODE: the object is not a node of the graph a collate of that image gives

_lib = None


def load():
    """Load libisg_loader.so (built by __graft_entry__.build()); fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LoaderError(f"{LIB_PATH} is missing: run `python __graft_entry__.py` (build()) first")
    lib = bind(ctypes.CDLL(LIB_PATH), SIGNATURES)
    if lib.isg_loader_abi_version() != ABI_VERSION:
        raise LoaderError(f"libisg_loader.so ABI {lib.isg_loader_abi_version()}, binding expects {ABI_VERSION}")
    try:
        bind(lib, OBJECT_SIGNATURES)
    except AttributeError as e:
        raise LoaderError(f"{LIB_PATH} lacks a symbol of include/isg_loader_objects.h ({e}): rebuild it (build())") from None
    if lib.isg_loader_objects_abi_version() != OBJECT_ABI_VERSION:
        raise LoaderError(f"libisg_loader.so objects ABI {lib.isg_loader_objects_abi_version()}, binding expects {OBJECT_ABI_VERSION}")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise LoaderError(f"{what} failed ({rc}): {load().isg_sg_last_error().decode('utf-8', 'replace')}")


def _c_strings(items: Sequence[str]):
    arr = (c_char_p * len(items))(*[None if s is None else s.encode("utf-8") for s in items])      # None: a NULL string
    return arr


class SceneGraphVocab:
    """The scene-graph token vocabulary (scene_graph.py:145-183): ``token_lists`` are the six lists the reference reads
    from meta_info (name, attr, rel text files; objects, predicates, attributes JSON), in that order."""

    def __init__(self, token_lists: Sequence[Sequence[str]]):
        lib = load()
        flat = [t for lst in token_lists for t in lst]
        self._h = c_void_p()
        arr = _c_strings(flat)
        _check(lib.isg_sg_vocab_build(arr, len(flat), ctypes.byref(self._h)), "isg_sg_vocab_build")
        self._tokens = list(dict.fromkeys(flat + ["<self>", "pokemon"]))

    def __len__(self) -> int:
        return int(load().isg_sg_vocab_size(self._h))

    def lookup(self, token: str) -> int:
        return int(load().isg_sg_vocab_lookup(self._h, token.encode("utf-8")))

    def get_stoi(self) -> Dict[str, int]:
        out = {t: self.lookup(t) for t in ["<unk>", "<pad>", "<sos>", "<eos>", "<self>"] + self._tokens}
        return {t: i for t, i in out.items() if i >= 0}

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.isg_sg_vocab_free(self._h)
            self._h = None


@dataclass
class SceneGraphBatch:
    """What torch_geometric's Batch.from_data_list hands to ISubGVQA.forward (gqa.py:258), plus the
    per-graph bounds that let ops.GraphPlan.build skip its device sync."""
    x: Tensor               # [N, 4] int64 name + 3 attribute tokens
    edge_index: Tensor      # [2, E] int64
    edge_attr: Tensor       # [E] int64
    x_bbox: Tensor          # [N, 4] int64
    added_sym_edge: Tensor  # [S] int64, per-graph edge positions (not offset, quirk Q6)
    batch: Tensor           # [N] int64
    ptr: Tensor             # [B+1] int64
    num_graphs: int
    max_nodes: int
    max_edges: int
    graph_sizes: Optional[Tensor] = None      # HOST int64 [2, B] nodes / in-edges per graph, when some graph lies beyond a graph tile
                                              # (ops.GraphPlan.build's hint: the list of such graphs is then made without a sync)
    graph_index: Optional[Tensor] = None      # HOST int64 [Q]: collate(distinct=True) -- the graph of this batch every question asks

    def to(self, device, non_blocking: bool = True) -> "SceneGraphBatch":
        mv = lambda t: t.to(device, non_blocking=non_blocking)
        return SceneGraphBatch(mv(self.x), mv(self.edge_index), mv(self.edge_attr), mv(self.x_bbox),
                               mv(self.added_sym_edge), mv(self.batch), mv(self.ptr), self.num_graphs,
                               self.max_nodes, self.max_edges, self.graph_sizes, self.graph_index)


class BatchBuffers:
    """Reusable (pinned) host buffers for one in-flight batch: grown to the high-water mark, so a steady-state collate
    neither allocates nor page-faults.  Keep one per batch in flight (the async H2D copy reads from it)."""

    def __init__(self, pin_memory: bool = False):
        self.pin = pin_memory
        self._buf = {}

    def _get(self, name: str, numel: int) -> Tensor:
        t = self._buf.get(name)
        if t is None or t.numel() < numel:
            t = torch.empty(max(numel, 1) * 5 // 4 + 16, dtype=torch.int64, pin_memory=self.pin)
            self._buf[name] = t
        return t[:numel]

    def views(self, N: int, E: int, S: int, B: int):
        return (self._get("x", N * 4).view(N, 4), self._get("edge_index", 2 * E).view(2, E), self._get("edge_attr", E),
                self._get("x_bbox", N * 4).view(N, 4), self._get("added_sym_edge", S), self._get("batch", N),
                self._get("ptr", B + 1))


class SceneGraphStore:
    """All scene graphs of one or more GQA JSON files, converted once (GQASceneGraphs, scene_graph.py:49-72)."""

    def __init__(self, vocab: SceneGraphVocab):
        lib = load()
        self.vocab = vocab
        self._h = c_void_p()
        _check(lib.isg_sg_store_create(vocab._h, ctypes.byref(self._h)), "isg_sg_store_create")

    def add_json_file(self, path: str) -> "SceneGraphStore":
        _check(load().isg_sg_store_add_json_file(self._h, os.fsencode(path)), f"isg_sg_store_add_json_file({path})")
        return self

    def add_json(self, text) -> "SceneGraphStore":
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        _check(load().isg_sg_store_add_json(self._h, data, len(data)), "isg_sg_store_add_json")
        return self

    def __len__(self) -> int:
        return int(load().isg_sg_store_num_graphs(self._h))

    def __contains__(self, image_id: str) -> bool:
        return load().isg_sg_store_find(self._h, image_id.encode("utf-8")) >= 0

    def slots(self, image_ids: Sequence[str]) -> Tensor:
        """Store slot of every id (-1 = unknown -> dummy graph); resolve once per dataset, collate by slot per batch."""
        out = torch.empty(len(image_ids), dtype=torch.int64)
        _check(load().isg_sg_store_find_many(self._h, _c_strings(image_ids), len(image_ids), out.data_ptr()),
               "isg_sg_store_find_many")
        return out

    def collate(self, image_ids, pin_memory: Optional[bool] = None, out: Optional["BatchBuffers"] = None,
                threads: int = 4, distinct: bool = False) -> SceneGraphBatch:
        """query_and_translate per graph + Batch.from_data_list, written into (pinned) host tensors.
        ``image_ids``: id strings, or an int64 tensor of slots from ``slots()``.  ``out``: reusable buffers.
        ``distinct``: the batch holds every distinct slot ONCE, in the order of first occurrence (all unknown ids share the one
        dummy graph); ``graph_index[q]`` is then the graph of the batch that image_ids[q] names, and ``graph_sizes`` is always
        filled -- what ISubGVQA.encode_scene / ask take for several questions per image."""
        lib = load()
        slots = image_ids if torch.is_tensor(image_ids) else self.slots(image_ids)
        slots = slots.contiguous()
        graph_index = None
        if distinct:
            first = {}
            graph_index = torch.tensor([first.setdefault(s, len(first)) for s in slots.clamp(min=-1).tolist()], dtype=torch.int64)
            slots = torch.tensor(list(first), dtype=torch.int64)
        B = slots.numel()
        tot = (c_int64 * 3)()
        _check(lib.isg_sg_collate_sizes(self._h, slots.data_ptr(), B, tot), "isg_sg_collate_sizes")
        N, E, S = int(tot[0]), int(tot[1]), int(tot[2])
        if out is None:
            pin = torch.cuda.is_available() if pin_memory is None else pin_memory
            out = BatchBuffers(pin)
        x, ei, ea, bb, sym, batch, ptr = out.views(N, E, S, B)
        bounds = (c_int64 * 2)()
        _check(lib.isg_sg_collate(self._h, slots.data_ptr(), B, x.data_ptr(), ei.data_ptr(), ea.data_ptr(),
                                  bb.data_ptr(), sym.data_ptr(), batch.data_ptr(), ptr.data_ptr(), bounds,
                                  int(threads)), "isg_sg_collate")
        sizes = None
        if distinct or int(bounds[0]) > 64 or int(bounds[1]) > 256:      # a graph beyond the 64-node / 256-in-edge tiles of the kernels
            sizes = torch.stack([ptr[1:] - ptr[:-1], torch.bincount(batch[ei[1]], minlength=B)]) if E > 0 else \
                torch.stack([ptr[1:] - ptr[:-1], torch.zeros(B, dtype=torch.int64)])
        return SceneGraphBatch(x, ei, ea, bb, sym, batch, ptr, B, int(bounds[0]), int(bounds[1]), sizes, graph_index)

    def object_nodes(self, image_ids, object_ids: Sequence[Sequence[str]]):
        """(nodes int32 [total], ptr int64 [B + 1]): for question b, nodes[ptr[b]:ptr[b + 1]] are the LOCAL node indices of the GQA
        object ids object_ids[b] in the graph of image_ids[b] as collate() numbers it (objects by ascending id STRING), NO_NODE
        (-2) where the image is unknown, its graph is a dummy, it has no such object, or the id is None.  ``image_ids``: id
        strings, or an int64 tensor of slots from ``slots()``."""
        slots = image_ids if torch.is_tensor(image_ids) else self.slots(image_ids)
        slots = slots.to(torch.int64).contiguous()
        B = slots.numel()
        if len(object_ids) != B:
            raise ValueError(f"object_nodes: {B} images, {len(object_ids)} id lists")
        flat = [None if i is None else str(i) for ids in object_ids for i in ids]
        ptr = torch.zeros(B + 1, dtype=torch.int64)
        if B:
            ptr[1:] = torch.tensor([len(ids) for ids in object_ids], dtype=torch.int64).cumsum(0)
        nodes = torch.empty(len(flat), dtype=torch.int32)
        _check(load().isg_sg_store_object_nodes(self._h, slots.data_ptr(), B, ptr.data_ptr(), _c_strings(flat), nodes.data_ptr()),
               "isg_sg_store_object_nodes")
        return nodes, ptr

    def object_bytes(self) -> int:
        """Bytes the store keeps to resolve object ids: the id pool and its offsets."""
        return int(load().isg_sg_store_object_bytes(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.isg_sg_store_free(self._h)
            self._h = None


def read_token_lists(meta_info_dir: str) -> List[List[str]]:
    """The six vocabulary sources in the reference's order (scene_graph.py:152-163)."""
    import json

    def lines(name):
        with open(os.path.join(meta_info_dir, name)) as f:
            return f.read().splitlines()

    def js(name):
        with open(os.path.join(meta_info_dir, name)) as f:
            return json.load(f)
    return [lines("name_gqa.txt"), lines("attr_gqa.txt"), lines("rel_gqa.txt"), js("objects.json"),
            js("predicates.json"), js("attributes.json")]


def declared_symbols(header_path: str) -> List[str]:
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(isg_[a-z0-9_]+)\s*\(", text)))
