"""include/isg_grounding.h restated as Python loops over sets (not a test module): the table of a batch and the running totals.
Everything is an integer; the GPU tests compare with these exactly.  The layout constants are read from the header by the tests and
passed in (`C` = isubgvqa_amd._lib_grounding.CONSTANTS), so a number of the header is restated nowhere."""
import math


def kept(mask, threshold, n):
    v = float(mask[n])
    return v == v and v > threshold


def restate_table(mask, ptr, gold, threshold=0.0):
    """[[12 ints] per question] of mask [N], ptr [B + 1] and gold [B][F][M] (lists or tensors)."""
    mask = [float(v) for v in (mask.reshape(-1).tolist() if hasattr(mask, "tolist") else mask)]
    ptr = ptr.tolist() if hasattr(ptr, "tolist") else list(ptr)
    gold = gold.tolist() if hasattr(gold, "tolist") else gold
    rows = []
    for g, facets in enumerate(gold):
        lo, hi = ptr[g], ptr[g + 1]
        n = hi - lo
        picked = {i for i in range(n) if kept(mask, threshold, lo + i)}
        unresolved = sum(1 for f in facets for e in f if e == -2)
        bad = sum(1 for f in facets for e in f if e < -2 or e >= n)
        row = [len(picked), n, unresolved, bad] + [0] * 8
        union = set()
        for s, f in enumerate(facets):
            objects = {e for e in f if 0 <= e < n}
            row[4 + 2 * s], row[5 + 2 * s] = len(objects), len(objects & picked)
            union |= objects
        row[10], row[11] = len(union), len(union & picked)
        rows.append(row)
    return rows


def bad_group_ids(groups, G):
    """(count, first row or None) of the ids below -1 or at or above G."""
    rows = groups.tolist() if hasattr(groups, "tolist") else groups
    bad = [(r, i) for r, ids in enumerate(rows) for i in ids if i < -1 or i >= G]
    return len(bad), (bad[0][0] if bad else None)


def add_totals(totals, table, C, pred=None, label=None, groups=None, G=0):
    """totals ([1 + G][ISG_GROUND_TOTALS] lists of ints, or None for zeros) with the table's questions added: row 0 every question,
    row 1 + g those of group g, once per facet of `groups` that names g."""
    T, HEAD, BLOCK, HIST = C["ISG_GROUND_TOTALS"], C["ISG_GROUND_HEAD"], C["ISG_GROUND_BLOCK"], C["ISG_GROUND_HIST"]
    out = [[0] * T for _ in range(1 + G)] if totals is None else [list(r) for r in totals]
    pred = None if pred is None else [int(v) for v in pred]
    label = None if label is None else [int(v) for v in label]
    groups = None if groups is None else (groups.tolist() if hasattr(groups, "tolist") else groups)
    for q, row in enumerate(table):
        correct = pred is not None and pred[q] == label[q]
        member = [0] + ([] if groups is None else [1 + i for i in groups[q] if 0 <= i < G])
        for r in member:
            t = out[r]
            t[0] += 1
            t[1] += int(correct)
            t[2] += row[2]
            t[3] += row[3]
            for s in range(4):
                size, hits = row[4 + 2 * s], row[5 + 2 * s]
                if size == 0:
                    continue
                for c in ((0, 1) if correct else (0,)):
                    at = HEAD + (2 * s + c) * BLOCK
                    t[at] += 1
                    t[at + 1] += row[0]
                    t[at + 2] += row[1]
                    t[at + 3] += size
                    t[at + 4] += hits
                    t[at + 5] += int(hits > 0)
                    t[at + 6] += int(hits == size)
                    t[at + 8 + size] += 1
                    t[at + 8 + HIST + size] += hits
    return out


def macro_recall(table, s, rows=None):
    """The mean over the questions with |G_s| > 0 of hits / |G_s|, straight from the table (NaN without such a question)."""
    parts = [r[5 + 2 * s] / r[4 + 2 * s] for q, r in enumerate(table) if r[4 + 2 * s] > 0 and (rows is None or q in rows)]
    return math.fsum(parts) / len(parts) if parts else float("nan")
