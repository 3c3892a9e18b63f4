"""Batch assembly in front of ISubGVQA.forward.

Reference behaviour: gqa_collate, ISubGVQA/datasets/gqa.py:237-272: zip the dataset items, tokenise the question strings
with the CLIP tokenizer (padding=True), Batch.from_data_list the scene graphs, LongTensor the labels.  Here the dataset
item carries the IMAGE ID instead of a converted graph (the conversion happened once, inside the C++ store) and the
scene-graph part of the batch is one isg_sg_collate call into pinned memory.  The tokenizer is injected: the reference's
is a download (isubgvqa.py:116-119, CLIPTokenizer.from_pretrained) and stays outside this path.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch


def gqa_collate(data: Sequence[tuple], scene_graphs, tokenizer: Optional[Callable] = None, pin_memory: Optional[bool] = None,
                distinct: bool = False, annotations: Optional["ObjectAnnotations"] = None):
    """data: (questionID, image_id, question_text, qst_types, short_answer_label, image_id) tuples (gqa.py:186-193 with the
    scene graph replaced by its image id).  Returns the reference's 7-tuple (gqa.py:262-270).  distinct=True: the scene-graph
    batch holds every image once and carries the questions' graph_index (SceneGraphStore.collate); the tuple is the same.
    annotations (an ObjectAnnotations): every item carries the question record's `annotations` dict as a SEVENTH field, and the
    tuple gets an eighth entry, the gold table int32 [B, F, M] of annotations.encode -- indices local to a graph, so the same
    table serves distinct=True."""
    if annotations is not None:
        question_id, graph_ids, question_text, qst_types, labels, img, annos = zip(*data)
    else:
        question_id, graph_ids, question_text, qst_types, labels, img = zip(*data)
    qsts_padded = qsts_attention_mask = None
    if tokenizer is not None:
        q = tokenizer(list(question_text), return_tensors="pt", padding=True)            # :252-256
        qsts_padded, qsts_attention_mask = q["input_ids"], q["attention_mask"]
    scene_graph = scene_graphs.collate(list(graph_ids), pin_memory, distinct=distinct)   # :258
    out = (question_id, scene_graph, qsts_padded, qsts_attention_mask, torch.LongTensor(labels), img, qst_types)
    if annotations is None:
        return out
    return out + (annotations.encode(annos, list(graph_ids), getattr(scene_graphs, "store", scene_graphs)),)


class GroupedBatchSampler:
    """A batch sampler (torch.utils.data.DataLoader(batch_sampler=...)) whose batches REPEAT scene graphs: every batch holds
    `images_per_batch` images and up to `questions_per_image` questions of each -- what SceneGraphStore.collate(distinct=True)
    and ISubGVQA.forward_shared are for; a shuffled sampler over GQA's questions almost never draws an image twice in one batch.

    image_ids: the image of every dataset item, in item order (any hashable).  Per epoch the questions of an image are shuffled
    and cut into groups of at most questions_per_image (the last group of an image is what is left over); the groups of all
    images are shuffled and dealt into batches, and a group whose image already sits in the batch waits for the next one -- so a
    batch never holds more than questions_per_image questions of an image.  Every question appears exactly once per epoch
    (drop_last=True drops the batches with fewer than images_per_batch groups).  Deterministic per (seed, epoch): set_epoch()
    as with torch's DistributedSampler.  Host only."""

    def __init__(self, image_ids: Sequence, images_per_batch: int, questions_per_image: int, seed: int, drop_last: bool = False):
        if int(images_per_batch) < 1 or int(questions_per_image) < 1:
            raise ValueError(f"GroupedBatchSampler: images_per_batch = {images_per_batch}, questions_per_image = {questions_per_image}")
        self.images_per_batch, self.questions_per_image = int(images_per_batch), int(questions_per_image)
        self.seed, self.drop_last, self.epoch = int(seed), bool(drop_last), 0
        by_image = {}
        for i, image in enumerate(image_ids):
            by_image.setdefault(image, []).append(i)
        self._items = list(by_image.values())             # images in the order of their first question
        self._made = None                                 # (epoch, batches)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _batches(self) -> list:
        if self._made is not None and self._made[0] == self.epoch:
            return self._made[1]
        gen = torch.Generator().manual_seed(self.seed * 1000003 + self.epoch)
        groups = []                                       # (image number, item indices)
        for image, items in enumerate(self._items):
            order = torch.randperm(len(items), generator=gen).tolist()
            for lo in range(0, len(items), self.questions_per_image):
                groups.append((image, [items[j] for j in order[lo:lo + self.questions_per_image]]))
        stream = [groups[j] for j in torch.randperm(len(groups), generator=gen).tolist()]
        batches, waiting, pos = [], [], 0
        while pos < len(stream) or waiting:
            images, batch, still = set(), [], []
            for group in waiting:                         # the groups that waited go first, in their order
                if len(images) < self.images_per_batch and group[0] not in images:
                    images.add(group[0])
                    batch += group[1]
                else:
                    still.append(group)
            while pos < len(stream) and len(images) < self.images_per_batch:
                group = stream[pos]
                pos += 1
                if group[0] in images:
                    still.append(group)
                else:
                    images.add(group[0])
                    batch += group[1]
            waiting = still
            if len(images) == self.images_per_batch or not self.drop_last:
                batches.append(batch)
        self._made = (self.epoch, batches)
        return batches

    def __iter__(self):
        return iter([list(b) for b in self._batches()])

    def __len__(self) -> int:
        return len(self._batches())


class QuestionTypes:
    """The id space of the questions' types for an evaluation by type (include/isg_eval.h): every name of every facet gets ONE id
    in [0, num_groups), facet after facet, so two facets never share an id and one device table holds them all.

    The reference's dataset hands every question's `types` dict ({"structural": ..., "semantic": ..., "detailed": ...},
    gqa.py:186-193) through its collate as the last entry of the 7-tuple; encode() takes that entry as it is.
    names: {facet: [name, ...]} fixes the ids; with names=None the id space is empty until fit() has seen the dicts."""

    def __init__(self, facets: Sequence[str] = ("structural", "semantic"), names: Optional[dict] = None):
        self.facets = tuple(facets)
        if not 1 <= len(self.facets) <= 4:
            raise ValueError(f"QuestionTypes: 1 to 4 facets (the device table's F), got {len(self.facets)}")
        self._names = {f: [] for f in self.facets}
        self._ids: dict = {}
        if names is not None:
            for f in self.facets:
                for n in names[f]:
                    self._add(f, n)
            self._renumber()

    def _add(self, facet: str, name) -> None:
        if name not in self._names[facet]:
            self._names[facet].append(name)

    def _renumber(self) -> None:
        self._ids, nxt = {}, 0
        for f in self.facets:
            for n in self._names[f]:
                self._ids[(f, n)] = nxt
                nxt += 1
        if nxt > 256:
            raise ValueError(f"QuestionTypes: {nxt} groups; the device table holds 256 (drop a facet such as `detailed`)")

    def fit(self, qst_types: Sequence[dict]) -> "QuestionTypes":
        """Add the names of these dicts, each facet in order of first occurrence, behind the names already known."""
        for t in qst_types:
            for f in self.facets:
                if isinstance(t, dict) and t.get(f) is not None:
                    self._add(f, t[f])
        self._renumber()
        return self

    @property
    def num_groups(self) -> int:
        return len(self._ids)

    @property
    def group_names(self) -> list:
        """[(facet, name)] by id."""
        return list(self._ids)

    def encode(self, qst_types: Sequence[dict]) -> torch.Tensor:
        """Host int32 [B, F] of group ids, -1 for an unknown name or a missing key; pinned when CUDA is there."""
        rows = [[self._ids.get((f, t.get(f) if isinstance(t, dict) else None), -1) for f in self.facets] for t in qst_types]
        out = torch.tensor(rows, dtype=torch.int32).view(len(rows), len(self.facets))
        return out.pin_memory() if torch.cuda.is_available() else out


class ObjectAnnotations:
    """GQA's object annotations as node indices, for the grounding score (include/isg_grounding.h; the sibling of QuestionTypes).

    Every GQA question record carries `annotations`: {"question": {...}, "answer": {...}, "fullAnswer": {...}}, each facet mapping
    word positions ("4", "2:4") to the id of the scene-graph object the words refer to.  Only the values are used, in the dict's
    order.  A value may be an id string, several ids separated by commas, or a list of id strings."""

    def __init__(self, facets: Sequence[str] = ("question", "answer", "fullAnswer"), max_gold: int = 64):
        self.facets = tuple(facets)
        if not 1 <= len(self.facets) <= 3:
            raise ValueError(f"ObjectAnnotations: 1 to 3 facets (the device table's F), got {len(self.facets)}")
        if not 1 <= int(max_gold) <= 64:
            raise ValueError(f"ObjectAnnotations: max_gold = {max_gold}; a facet of the device table holds 1 to 64 entries")
        self.max_gold = int(max_gold)

    @staticmethod
    def _ids(value) -> list:
        if isinstance(value, (list, tuple)):
            return [i for v in value for i in ObjectAnnotations._ids(v)]
        return [p.strip() for p in str(value).split(",") if p.strip()]

    def object_ids(self, annotations: Sequence[dict]) -> list:
        """[[ids of facet 0, ids of facet 1, ...] per question]: the annotated object ids as strings, values in dict order."""
        out = []
        for q, a in enumerate(annotations):
            row = []
            for f in self.facets:
                words = a.get(f) if isinstance(a, dict) else None
                ids = [i for v in words.values() for i in self._ids(v)] if isinstance(words, dict) else []
                if len(ids) > self.max_gold:
                    raise ValueError(f"ObjectAnnotations: question {q} annotates {len(ids)} objects in `{f}`, more than "
                                     f"max_gold = {self.max_gold}")
                row.append(ids)
            out.append(row)
        return out

    def encode(self, annotations: Sequence[dict], image_ids, store) -> torch.Tensor:
        """Host int32 [B, F, M] of LOCAL node indices (store.object_nodes: loader.SceneGraphStore, or anything with that method),
        M = the longest facet list of the batch (at least 1); -1 pads, -2 = annotated but not a node of the graph.  Pinned when
        CUDA is there."""
        ids = self.object_ids(annotations)
        B, F = len(ids), len(self.facets)
        if len(image_ids) != B:
            raise ValueError(f"ObjectAnnotations.encode: {B} annotations, {len(image_ids)} image ids")
        M = max([len(f) for row in ids for f in row] + [1])
        out = torch.full((B, F, M), -1, dtype=torch.int32)
        if B:
            nodes, ptr = store.object_nodes(image_ids, [[i for f in row for i in f] for row in ids])
            at = ptr.tolist()
            for q, row in enumerate(ids):
                lo = at[q]
                for f, lst in enumerate(row):
                    out[q, f, :len(lst)] = nodes[lo:lo + len(lst)]
                    lo += len(lst)
        return out.pin_memory() if torch.cuda.is_available() else out
